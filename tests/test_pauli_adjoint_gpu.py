"""Two-state Pauli circuits with transition elements and adjoint gradients on the device (artensor_amd/adjoint.py;
artn_pauli_adjoint) against pauli_evolve_ (bit for bit), exact integer arithmetic and the numpy oracle of tests/adjoint_oracle.py.

Tolerance of a transition element (derived, not measured).  With `unit` = 2^-24 (complex64) or 2^-52 (complex128) and G the
growth of tests/test_pauli_evolve_gpu.py, each state before step k carries a rounding error of at most K unit ||state|| G in the
2-norm, and the element is linear in both, so the two errors enter as 2 K unit ||lam|| ||phi|| G^2; the float64 sum of n terms
adds at most n 2^-52 ||lam|| ||phi|| G^2:
    |t_k - ref_k| <= 2 K unit ||lam|| ||phi|| G^2 + n 2^-52 ||lam|| ||phi|| G^2
E and grad of adjoint_gradient are sums of such elements over the terms of H (lam = H phi, ||lam|| <= sum |c| ||phi||): the same
bound with lam = phi = amps0, times sum |c|, is asserted for E and for every entry of grad as it stands.  G counts
|cos| + |sin| <= sqrt(2) per rotation, so the layered ansatz of the gradient test uses small angles (G^2 = 5.7 over its 47
rotations) and a start state near a basis state, whose gradients (0.04 to 0.4) lie 60 to 600 bounds above the complex64 bound
(6.2e-4); with angles of order 1 the bound would exceed the gradients and the test could not fail.
The parameter shift of a parameter with m rotations is a signed sum of 2 m energies, each within the bound of ITS circuit (one
angle moved by pi / 4, which raises G), so |grad - shift| <= bound + 2 m bound_shifted."""
import ctypes
import os

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd.fixtures import load_case
from adjoint_oracle import oracle_gradient, oracle_pair
from test_pauli_apply_gpu import DEV, GOLDEN, addressing_strings, crand, gpu, ising
from test_pauli_evolve_gpu import bits_of, growth, random_steps

pytestmark = pytest.mark.gpu

KINDS = ["c64", "c128"]
TOP = {"c64": 3, "c128": 2}


def bound(kind, steps, lam, phi):
    unit = 2.0 ** -24 if kind == "c64" else 2.0 ** -52
    nl, nph = (np.linalg.norm(np.asarray(x).astype(np.complex128).reshape(-1)) for x in (lam, phi))
    g2 = growth(steps) ** 2
    return 2 * len(steps) * unit * nl * nph * g2 + np.asarray(phi).size * 2.0 ** -52 * nl * nph * g2


def patterns(n):
    return {"all": None, "none": [False] * n, "alternating": [k % 2 == 0 for k in range(n)]}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nq", [9, 10, 11, 12, 13])
def test_states_bit_for_bit_and_elements_against_the_oracle(nq, kind):
    rng = np.random.default_rng(100 + nq)
    lam0, phi0 = crand(rng, (2,) * nq, kind), crand(rng, (2,) * nq, kind)
    steps = random_steps(rng, nq, 24)
    want_lam, want_phi = A.pauli_evolve_(gpu(lam0), steps), A.pauli_evolve_(gpu(phi0), steps)
    ref_t, _, _ = oracle_pair(lam0, phi0, steps)
    tol = bound(kind, steps, lam0, phi0)
    for max_rank in range(TOP[kind] + 1):
        for name, measure in patterns(24).items():
            lam, phi = gpu(lam0), gpu(phi0)
            t = A.pauli_evolve_pair_(lam, phi, steps, measure, max_rank)
            assert torch.equal(bits_of(phi), bits_of(want_phi)) and torch.equal(bits_of(lam), bits_of(want_lam)), (max_rank, name)
            assert t.dtype == np.complex128 and t.shape == (24,)
            flags = np.ones(24, bool) if measure is None else np.array(measure)
            assert np.all(t[~flags] == 0)
            err = np.abs(t - ref_t)[flags].max() if flags.any() else 0.0
            print(f"nq {nq} {kind} R {max_rank} {name}: err {err:.3e} bound {tol:.3e} ratio {err / tol:.3f}")
            assert err <= tol
            circ = A.PauliPairCircuit(phi.shape, phi.stride(), phi.dtype, steps, DEV, measure, max_rank)
            lam2, phi2 = gpu(lam0), gpu(phi0)
            t2 = circ(lam2, phi2, device=True)
            assert t2.is_cuda and t2.dtype == torch.float64 and t2.shape == (24, 2)
            assert np.array_equal(t2.cpu().numpy().view(np.complex128).reshape(-1).view(np.int64), t.view(np.int64))
            assert torch.equal(bits_of(phi2), bits_of(phi)) and torch.equal(bits_of(lam2), bits_of(lam))


@pytest.mark.parametrize("kind", KINDS)
def test_exact_transition_elements(kind):
    """Gaussian integers in [-8, 7], eight steps whose coefficients are Gaussian integers with |alpha| + |beta| <= 2: an
    amplitude is at most 8 sqrt(2) 2^k < 2^(k + 4) in modulus after k steps, so below 2^12 throughout (exact in float32), a term
    conj(lam) b is below 2^24 and any sum of the 2^13 terms below 2^37 < 2^53: every partial sum is an exact integer in float64
    whatever the order, so t_k must EQUAL the integer numpy computes."""
    nq = 13
    rng = np.random.default_rng(8)
    strings = addressing_strings(nq)
    picks = [0, 2, 6, 13, 16, 19, 20, 21]                 # diagonal, register, lanes, bit 10, high + low with Z, Y counts 1, 2, 3
    coeffs = [(0, 1), (1, 1j), (1, -1), (1j, 1), (0, -1j), (1, 1), (-1, 1j), (1j, -1j)]
    steps = [(complex(a), complex(b), strings[i]) for (a, b), i in zip(coeffs, picks)]
    mk = lambda: (rng.integers(-8, 8, (2,) * nq) + 1j * rng.integers(-8, 8, (2,) * nq)).astype(np.complex64 if kind == "c64" else np.complex128)
    lam0, phi0 = mk(), mk()
    want, want_lam, want_phi = oracle_pair(lam0, phi0, steps)
    assert np.all(want.real == np.round(want.real)) and np.abs(want).max() < 2.0 ** 53
    for max_rank in range(TOP[kind] + 1):
        lam, phi = gpu(lam0), gpu(phi0)
        t = A.pauli_evolve_pair_(lam, phi, steps, max_rank=max_rank)
        assert np.array_equal(t, want), max_rank
        assert np.array_equal(phi.cpu().numpy().astype(np.complex128), want_phi) and np.array_equal(lam.cpu().numpy().astype(np.complex128), want_lam)


@pytest.mark.parametrize("kind", KINDS)
def test_permuted_layouts(kind):
    rng = np.random.default_rng(17)
    lam0, phi0 = crand(rng, (2,) * 12, kind), crand(rng, (2,) * 12, kind)
    perm = [int(p) for p in rng.permutation(12)]
    lam, phi = gpu(lam0).permute(perm), gpu(phi0).permute(perm)
    assert not phi.is_contiguous()
    steps = random_steps(rng, 12, 9) + [(0.3, "X" * 12), (0.5, 0.5, {0: "Y", -1: "Z"})]
    t = A.pauli_evolve_pair_(lam, phi, steps)
    want, want_lam, want_phi = oracle_pair(lam0.transpose(perm), phi0.transpose(perm), steps)
    tol = bound(kind, steps, lam0, phi0)
    print(f"perm {perm} {kind}: err {np.abs(t - want).max():.3e} bound {tol:.3e}")
    assert np.abs(t - want).max() <= tol
    for x, x0 in ((lam, lam0), (phi, phi0)):
        assert torch.equal(bits_of(x), bits_of(A.pauli_evolve_(gpu(x0).permute(perm), steps)))


def test_n12_contraction_output():
    case = load_case(os.path.join(GOLDEN, "n12_dense.npz"))
    phi = A.tensor_contraction(case.fresh_tensors(device=DEV), case.scheme)
    two = [d for d, e in enumerate(phi.shape) if e == 2]
    assert len(two) == 12
    phi0 = phi.cpu().numpy()
    lam = A.pauli_sum_apply(phi, ising(two))
    lam0 = lam.cpu().numpy()
    steps = A.trotter_steps(ising(two), 0.05)
    t = A.pauli_evolve_pair_(lam, phi, steps)
    want, _, _ = oracle_pair(lam0, phi0, steps)
    tol = bound("c64", steps, lam0, phi0)
    print(f"n12: err {np.abs(t - want).max():.3e} bound {tol:.3e}")
    assert np.abs(t - want).max() <= tol
    again = torch.empty_strided(phi.shape, phi.stride(), dtype=phi.dtype, device=DEV)
    again.copy_(torch.from_numpy(phi0).to(DEV))
    assert torch.equal(bits_of(phi), bits_of(A.pauli_evolve_(again, steps)))


@pytest.mark.parametrize("max_rank", [0, 2])
def test_grid_stride_and_determinism(max_rank):
    nq = 24                                               # 2^14 tiles: 2^14 >> R blocks, more than the 2048 workgroups
    gen = torch.Generator(device=DEV).manual_seed(5)
    lam0 = torch.view_as_complex(torch.randn((2,) * nq + (2,), generator=gen, device=DEV))
    phi0 = torch.view_as_complex(torch.randn((2,) * nq + (2,), generator=gen, device=DEV))
    s = lambda ops: "".join(ops.get(nq - 1 - d, "I") for d in range(nq))
    steps = [(0.3, s({0: "Z", 23: "Z"})), (-0.7, s({1: "X"})), (0.4, s({12: "Y", 3: "Z"})), (0.9, s({23: "X", 5: "X"})),
             (0.2, 0.5j, s({17: "Y", 12: "X", 0: "Z"})), (-0.1, s({2: "Y"}))]
    lam, phi = lam0.clone(), phi0.clone()
    t = A.pauli_evolve_pair_(lam, phi, steps, max_rank=max_rank)
    lam1, phi1 = lam0.clone(), phi0.clone()
    assert np.array_equal(A.pauli_evolve_pair_(lam1, phi1, steps, max_rank=max_rank).view(np.int64), t.view(np.int64))
    assert torch.equal(bits_of(phi1), bits_of(phi)) and torch.equal(bits_of(lam1), bits_of(lam))
    lam2, phi2 = lam0.clone(), phi0.clone()
    one = np.array([A.pauli_evolve_pair_(lam2, phi2, [st], max_rank=max_rank)[0] for st in steps])
    assert torch.equal(bits_of(phi2), bits_of(phi)) and torch.equal(bits_of(lam2), bits_of(lam))
    scale = float(torch.linalg.vector_norm(lam0) * torch.linalg.vector_norm(phi0)) * growth(steps) ** 2
    print(f"R {max_rank}: fused against one step per call {np.abs(one - t).max():.3e}, allowed {2.0 ** nq * 2.0 ** -52 * scale:.3e}")
    assert np.abs(one - t).max() <= 2.0 ** nq * 2.0 ** -52 * scale   # (the same states bit for bit: only the summation order differs)


def gradient_cases():
    nq = 12
    zz = lambda g: [(g, {a: "Z", a + 1: "Z"}) for a in range(nq - 1)]
    xs = lambda b: [(b, {a: "X"}) for a in range(nq)]
    layered = zz(0.02) + xs(-0.03) + [(0.025, {4: "Y", 11: "Z"})] + zz(-0.015) + xs(0.01)   # small angles: see the module docstring
    params = [0] * (nq - 1) + [1] * nq + [-1] + [2] * (nq - 1) + [3] * nq
    rng = np.random.default_rng(21)
    rand = [(float(rng.uniform(-2, 2)), "".join(rng.choice(list("IXYZ"), nq))) for _ in range(10)]
    return {"layers": (layered, params), "layers, every rotation": (layered, None), "random strings": (rand, None)}


def energy_bound(kind, rotations, terms, a0):
    n2 = np.vdot(a0.astype(np.complex128), a0.astype(np.complex128)).real
    return bound(kind, [(-t, p) for t, p in reversed(rotations)], a0, a0) * sum(abs(c) for c, _ in terms) / n2


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", list(gradient_cases()))
def test_adjoint_gradient(case, kind):
    nq = 12
    rotations, params = gradient_cases()[case]
    terms = ising(list(range(nq)))
    rng = np.random.default_rng(31)
    a0 = crand(rng, (2,) * nq, kind)
    if case != "random strings":                         # near |0..0>: gradients of order 0.1
        a0 = a0 * a0.real.dtype.type(0.02)
        a0[(0,) * nq] += 1
    amps0 = gpu(a0)
    keep = bits_of(amps0).clone()
    e, grad = A.adjoint_gradient(amps0, rotations, terms, params)
    assert torch.equal(bits_of(amps0), keep)
    want_e, want_grad = oracle_gradient(a0, rotations, terms, params)
    assert isinstance(e, float) and grad.dtype == np.float64 and grad.shape == want_grad.shape
    n2 = np.vdot(a0.astype(np.complex128), a0.astype(np.complex128)).real
    tol = energy_bound(kind, rotations, terms, a0)
    print(f"{case} {kind}: E {want_e:.4f} err {abs(e - want_e):.3e}; |grad| {np.abs(want_grad).min():.3e} .. {np.abs(want_grad).max():.3e} "
          f"err {np.abs(grad - want_grad).max():.3e}; bound {tol:.3e}")
    assert np.abs(want_grad).max() > 20 * tol            # (the check below can fail)
    assert abs(e - want_e) <= tol
    assert np.all(np.abs(grad - want_grad) <= tol)
    # parameter shift on the device, from calls that exist without the adjoint kernels
    idx = list(range(len(rotations))) if params is None else params
    for q in sorted({p for p in idx if p >= 0})[:3]:
        shift, allowed = 0.0, tol
        for k, (theta, p) in enumerate(rotations):
            if idx[k] != q:
                continue
            for sign in (1.0, -1.0):
                moved = rotations[:k] + [(theta + sign * np.pi / 4, p)] + rotations[k + 1:]
                psi = gpu(a0)
                A.pauli_evolve_(psi, moved)
                shift += sign * A.pauli_sum_expectation(psi, terms, normalize=False) / n2
                allowed += energy_bound(kind, moved, terms, a0)
        print(f"  parameter {q}: grad {grad[q]:.6f} shift {shift:.6f} allowed {allowed:.3e}")
        assert abs(grad[q] - shift) <= allowed, (q, grad[q], shift)


def test_zero_hamiltonian_and_normalize():
    rng = np.random.default_rng(2)
    a0 = crand(rng, (2,) * 12, "c64")
    rotations = [(0.3, "X" * 12), (-0.4, {3: "Y", 11: "Z"})]
    e, grad = A.adjoint_gradient(gpu(a0), rotations, [(0.0, "Z" * 12), (0.0, {1: "X"})])
    assert e == 0.0 and np.all(grad == 0.0) and grad.shape == (2,)
    terms = ising(list(range(12)))
    e1, g1 = A.adjoint_gradient(gpu(a0), rotations, terms, normalize=False)
    e2, g2 = A.adjoint_gradient(gpu(a0), rotations, terms)
    n2 = A.norm2(gpu(a0))
    assert e2 == e1 / n2 and np.array_equal(g2, g1 / n2)
    assert A.adjoint_gradient(gpu(a0), rotations, terms, params=[-1, -1])[1].shape == (0,)
    with pytest.raises(ValueError, match="real coefficients"):
        A.adjoint_gradient(gpu(a0), rotations, [(1j, "Z" * 12)])
    with pytest.raises(ValueError, match="params"):
        A.adjoint_gradient(gpu(a0), rotations, terms, params=[0])
    with pytest.raises(RuntimeError, match="above the two-state maximum"):       # (valid for the forward circuit alone)
        A.adjoint_gradient(gpu(a0), rotations, terms, max_rank=4)


def test_argument_checks():
    rng = np.random.default_rng(4)
    store = gpu(crand(rng, (2,) * 13, "c64"))
    steps = [(0.3, "X" * 12), (0.2, "Z" * 12)]
    lam, phi = store[0], store[1]
    with pytest.raises(ValueError, match="overlaps"):
        A.pauli_evolve_pair_(phi, phi, steps)
    with pytest.raises(ValueError, match="built for shape"):
        A.pauli_evolve_pair_(lam.permute(1, 0, *range(2, 12)), phi, steps)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.pauli_evolve_pair_(lam.cpu(), phi, steps)
    with pytest.raises(ValueError, match="one flag per step"):
        A.pauli_evolve_pair_(lam, phi, steps, measure=[True])
    with pytest.raises(RuntimeError, match="above the two-state maximum"):
        A.pauli_evolve_pair_(lam, phi, steps, max_rank=4)
    # the raw entry point: refusals that the Python layer never lets through
    circ = A.PauliPairCircuit(phi.shape, phi.stride(), phi.dtype, steps, DEV)
    out = torch.empty((2, 2), dtype=torch.float64, device=DEV)

    space = torch.empty(circ.workspace_bytes // 8, dtype=torch.float64, device=DEV)

    def call(lam_p, phi_p, table=circ._table.data_ptr(), tb=circ.table_bytes, ws=space.data_ptr(), wb=circ.workspace_bytes,
             out_p=out.data_ptr()):
        return N.lib().artn_pauli_adjoint(ctypes.byref(circ._d), lam_p, phi_p, circ._ops.ctypes.data_as(ctypes.c_void_p), 2, -1, table, tb,
                                          ws, wb, out_p, N.current_stream_ptr(store.device))
    lp, pp = lam.data_ptr(), phi.data_ptr()
    assert call(lp, lp + 8 * 2048) == -1 and b"overlaps" in N.lib().artn_last_error()
    assert call(None, pp) == -1 and call(lp, pp, table=None) == -1 and call(lp, pp, ws=None) == -1 and call(lp, pp, out_p=None) == -1
    assert call(lp, pp, wb=circ.workspace_bytes - 1) == -1 and call(lp, pp, tb=circ.table_bytes - 1) == -1
    assert call(lp + 8, pp) == -2 and call(lp, pp, ws=space.data_ptr() + 8) == -2
    torch.cuda.synchronize()
    assert call(lp, pp) == 0
    torch.cuda.synchronize()
