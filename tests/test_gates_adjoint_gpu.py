"""Two-state gate circuits with transition elements and adjoint gradients on the device (artensor_amd/gate_adjoint.py;
artn_gates_adjoint) against apply_gates_ (bit for bit), exact integer arithmetic and the numpy oracle of
tests/gates_adjoint_oracle.py.

Tolerance of a transition element (derived from the bound of tests/test_gates_gpu.py, not measured).  With c = 2 * 2^-24
(complex64) or 32 * 2^-53 (complex128) and G the `growth` of the circuit, each state before gate k is within c K ||state|| G of
the oracle in the 2-norm; the element is linear in both states and in M, so the two errors enter as 2 c K G^2 ||M|| ||lam|| ||phi||,
and the float64 sum of n terms adds at most n 2^-52 G^2 ||M|| ||lam|| ||phi||:
    |t_k - ref_k| <= ||M_k||_2 (2 c K G^2 + n 2^-52 G^2) ||lam|| ||phi||
E and grad of gate_adjoint_gradient: all gates unitary (G = 1), ||M|| = 1/2 for the rotations of the fixture, lam = H phi with
||lam|| <= sum|c| ||phi||, c' = 2^-24 or 16 * 2^-53 per gate of the forward AND of the backward circuit (hence 4 c' K), and
2 Re t per gate of a parameter:
    |grad_p - ref_p| <= m_p sum|c| 2 (1/2) (4 c' K + 2^nq 2^-52)
with m_p the number of gates sharing parameter p; the same with m = 1 for E."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from gates_adjoint_oracle import oracle_gate_gradient, oracle_gate_pair
from test_gates_adjoint_cpu import gradient_bound, gradient_fixture
from test_gates_gpu import ASYM1, ASYM2, growth, random_circuit
from test_pauli_adjoint_gpu import energy_bound
from test_pauli_apply_gpu import DEV, crand, gpu, ising
from test_pauli_evolve_gpu import bits_of

pytestmark = pytest.mark.gpu

KINDS = ["c64", "c128"]
TOP = {"c64": 3, "c128": 2}


def same_bits(x, y):
    return np.array_equal(np.asarray(x).view(np.int64), np.asarray(y).view(np.int64))


def element_bounds(kind, gates, measure, lam, phi):
    c = 2 * 2.0 ** -24 if kind == "c64" else 32 * 2.0 ** -53
    nl, nph = (np.linalg.norm(np.asarray(x).astype(np.complex128).reshape(-1)) for x in (lam, phi))
    g2 = growth(gates) ** 2
    per = (2 * c * len(gates) * g2 + np.asarray(phi).size * 2.0 ** -52 * g2) * nl * nph
    return np.array([0.0 if m is None else np.linalg.norm(np.asarray(m), 2) * per for m in measure])


def random_measures(rng, gates):
    return [rng.standard_normal((2 ** len(d),) * 2) + 1j * rng.standard_normal((2 ** len(d),) * 2) for _, d in gates]


def patterns(ms):
    return {"all": list(ms), "none": None, "alternating": [m if k % 2 == 0 else None for k, m in enumerate(ms)]}


# ---- 1. states bit for bit, elements against the oracle -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(nq):
    rng = np.random.default_rng(1800 + nq)
    gates = random_circuit(rng, nq, 24)
    ms = random_measures(rng, gates)
    lam128, phi128 = crand(rng, (2,) * nq, "c128"), crand(rng, (2,) * nq, "c128")
    inputs = {"c64": (lam128.astype(np.complex64), phi128.astype(np.complex64)), "c128": (lam128, phi128)}
    return gates, ms, inputs, {kind: oracle_gate_pair(*inputs[kind], gates, ms)[0] for kind in inputs}


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nq", [9, 10, 11, 12, 13, 14])
def test_states_bit_for_bit_and_elements_against_the_oracle(nq, kind):
    gates, ms, inputs, refs = random_case(nq)
    lam0, phi0 = inputs[kind]
    ref_t = refs[kind]
    want_lam, want_phi = A.apply_gates_(gpu(lam0), gates), A.apply_gates_(gpu(phi0), gates)
    tol = element_bounds(kind, gates, ms, lam0, phi0)
    for max_rank in range(TOP[kind] + 1):
        for name, measure in patterns(ms).items():
            lam, phi = gpu(lam0), gpu(phi0)
            t = A.apply_gates_pair_(lam, phi, gates, measure, max_rank)
            assert torch.equal(bits_of(phi), bits_of(want_phi)) and torch.equal(bits_of(lam), bits_of(want_lam)), (max_rank, name)
            assert t.dtype == np.complex128 and t.shape == (24,)
            flags = np.array([measure is not None and m is not None for m in (measure or ms)])
            assert np.all(t[~flags] == 0)
            ratio = (np.abs(t - ref_t)[flags] / tol[flags]).max() if flags.any() else 0.0
            err = np.abs(t - ref_t)[flags].max() if flags.any() else 0.0
            print(f"nq {nq} {kind} R {max_rank} {name}: err {err:.3e} bound {tol.min():.3e} .. {tol.max():.3e} ratio {ratio:.3f}")
            assert np.all(np.abs(t - ref_t)[flags] <= tol[flags])
            circ = A.GatePairCircuit(phi.shape, phi.stride(), phi.dtype, gates, DEV, measure, max_rank)
            lam2, phi2 = gpu(lam0), gpu(phi0)
            t2 = circ(lam2, phi2, device=True)
            assert t2.is_cuda and t2.dtype == torch.float64 and t2.shape == (24, 2)
            assert same_bits(t2.cpu().numpy().view(np.complex128).reshape(-1), t)
            assert torch.equal(bits_of(phi2), bits_of(phi)) and torch.equal(bits_of(lam2), bits_of(lam))


# ---- 2. exact transition elements -----------------------------------------------------------------------------------------------
I = 1j
U1 = [np.array([[1, I], [0, -I]]), np.array([[0, 1], [I, -1]]), np.array([[-I, 0], [1, 1]])]
M1 = [np.array([[0, 1], [-I, I]]), np.array([[I, -1], [0, 1]]), np.array([[1, 0], [-1, I]])]
U2 = [np.array([[1, 0, I, 0], [0, 0, 0, -1], [I, 1, 0, 0], [0, -I, 0, 1]]), np.array([[0, 1, 0, 0], [I, 0, 0, 1], [0, 0, -1, I], [1, 0, 0, 0]]),
      np.array([[0, 0, 1, -I], [1, 0, 0, 0], [0, I, 0, 1], [0, -1, I, 0]])]
M2 = [np.array([[0, I, 0, 1], [1, 0, 0, 0], [0, 0, -I, -1], [0, 1, I, 0]]), np.array([[1, 0, 0, -I], [0, 0, I, 0], [1, -1, 0, 0], [0, 0, 0, I]]),
      np.array([[0, 0, -1, 0], [I, 1, 0, 0], [0, 0, 1, I], [-I, 0, 0, 1]])]
DIAG2, MDIAG2 = np.diag([1, I, -1, -I]), np.diag([I, 0, 1, -1])


@pytest.mark.parametrize("kind", KINDS)
def test_exact_transition_elements(kind):
    """Gaussian integers in [-8, 7], eight gates whose U and M have entries in {0, 1, -1, i, -i} with at most two per row: an
    amplitude is at most 8 sqrt(2) 2^k < 2^(k + 4) in modulus after k gates, so below 2^12 throughout (exact in float32),
    (M phi)_i is below 2^12 before the last gate, a term conj(lam) (M phi) below 2^24 and any sum of the 2^13 terms below
    2^38 < 2^53: every partial sum is an exact integer in float64 whatever the order, so t_k must EQUAL the integer numpy computes.
    Contiguous [2]*13: dim d is memory bit 12 - d."""
    nq = 13
    rng = np.random.default_rng(8)
    dim = lambda b: nq - 1 - b
    gates = [(U1[0], (dim(0),)),                    # register
             (U1[1], (dim(5),)),                    # piece
             (U1[2], (dim(10),)),                   # bit 10
             (U2[0], (dim(11), dim(12))),           # two high bits
             (U2[1], (dim(12), dim(1))),            # high + register
             (U2[2], (dim(4), dim(11))),            # piece + high, d0 > d1
             (DIAG2, (dim(3), dim(10))),            # diagonal gate, dense M: staged for the measure alone
             (U2[0], (dim(1), dim(0)))]             # register + register
    measure = [M1[0], M1[1], M1[2], M2[0], M2[1], M2[2], M2[0], MDIAG2]
    assert gates[5][1][0] > gates[5][1][1]
    for m, _ in gates:
        assert np.abs(m).sum(axis=1).max() <= 2
    for m in measure:
        assert np.abs(m).sum(axis=1).max() <= 2 and (np.array_equal(m, MDIAG2) or not np.array_equal(m, m.T))
    mk = lambda: (rng.integers(-8, 8, (2,) * nq) + 1j * rng.integers(-8, 8, (2,) * nq)).astype(np.complex64 if kind == "c64" else np.complex128)
    lam0, phi0 = mk(), mk()
    want, want_lam, want_phi = oracle_gate_pair(lam0, phi0, gates, measure)
    assert np.all(want.real == np.round(want.real)) and np.all(want.imag == np.round(want.imag)) and np.abs(want).max() < 2.0 ** 53
    assert np.all(want != 0) and max(np.abs(want_phi).max(), np.abs(want_lam).max()) < 2.0 ** 12
    for max_rank in range(TOP[kind] + 1):
        lam, phi = gpu(lam0), gpu(phi0)
        t = A.apply_gates_pair_(lam, phi, gates, measure, max_rank)
        assert np.array_equal(t, want), (max_rank, t, want)
        assert np.array_equal(phi.cpu().numpy().astype(np.complex128), want_phi) and np.array_equal(lam.cpu().numpy().astype(np.complex128), want_lam)


# ---- 3. permuted layouts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_permuted_layouts(kind):
    rng = np.random.default_rng(17)
    lam0, phi0 = crand(rng, (2,) * 12, kind), crand(rng, (2,) * 12, kind)
    perm = [int(p) for p in rng.permutation(12)]
    lam, phi = gpu(lam0).permute(perm), gpu(phi0).permute(perm)
    assert not phi.is_contiguous()
    gates = random_circuit(rng, 12, 9) + [(ASYM2, (7, 2)), (ASYM2, (-1, 3)), (ASYM1, (-12,)), (ASYM2, (-2, -11))]
    assert any(len(d) == 2 and d[0] > d[1] for _, d in gates) and any(x < 0 for _, d in gates for x in d)
    ms = random_measures(rng, gates)
    t = A.apply_gates_pair_(lam, phi, gates, ms)
    want, _, _ = oracle_gate_pair(lam0.transpose(perm), phi0.transpose(perm), gates, ms)
    tol = element_bounds(kind, gates, ms, lam0, phi0)
    print(f"perm {perm} {kind}: err {np.abs(t - want).max():.3e} bound {tol.min():.3e} ratio {(np.abs(t - want) / tol).max():.3f}")
    assert np.all(np.abs(t - want) <= tol)
    for x, x0 in ((lam, lam0), (phi, phi0)):
        assert torch.equal(bits_of(x), bits_of(A.apply_gates_(gpu(x0).permute(perm), gates)))


# ---- 4. more blocks than workgroups, run to run ---------------------------------------------------------------------------------
@pytest.mark.parametrize("max_rank", [0, 2])
def test_grid_stride_and_determinism(max_rank):
    nq = 24                                               # 2^14 tiles: 2^14 >> R blocks, more than the 2048 workgroups
    gen = torch.Generator(device=DEV).manual_seed(5)
    lam0 = torch.view_as_complex(torch.randn((2,) * nq + (2,), generator=gen, device=DEV))
    phi0 = torch.view_as_complex(torch.randn((2,) * nq + (2,), generator=gen, device=DEV))
    dim = lambda b: nq - 1 - b
    gates = [(ASYM2, (dim(0), dim(23))), (ASYM1, (dim(1),)), (ASYM2, (dim(12), dim(3))), (ASYM2, (dim(23), dim(17))), (ASYM1, (dim(5),)),
             (np.diag([1, 1j, -1, 0.5]), (dim(12), dim(2))), (ASYM2, (dim(2), dim(1)))]
    measure = [ASYM2.T, None, ASYM2, ASYM2.conj(), ASYM1.T, ASYM2, None]
    lam, phi = lam0.clone(), phi0.clone()
    t = A.apply_gates_pair_(lam, phi, gates, measure, max_rank)
    lam1, phi1 = lam0.clone(), phi0.clone()
    assert same_bits(A.apply_gates_pair_(lam1, phi1, gates, measure, max_rank), t)
    assert torch.equal(bits_of(phi1), bits_of(phi)) and torch.equal(bits_of(lam1), bits_of(lam))
    assert t[1] == 0 and t[6] == 0 and np.all(t[[0, 2, 3, 4, 5]] != 0)
    assert torch.equal(bits_of(phi), bits_of(A.apply_gates_(phi0.clone(), gates))) and torch.equal(bits_of(lam), bits_of(A.apply_gates_(lam0.clone(), gates)))
    # one gate per call: the same states bit for bit, so only the summation order differs
    lam2, phi2 = lam0.clone(), phi0.clone()
    one = np.array([A.apply_gates_pair_(lam2, phi2, [g], [m], max_rank)[0] for g, m in zip(gates, measure)])
    assert torch.equal(bits_of(phi2), bits_of(phi)) and torch.equal(bits_of(lam2), bits_of(lam))
    scale = float(torch.linalg.vector_norm(lam0) * torch.linalg.vector_norm(phi0)) * growth(gates) ** 2 * max(
        np.linalg.norm(m, 2) for m in measure if m is not None)
    print(f"R {max_rank}: fused against one gate per call {np.abs(one - t).max():.3e}, allowed {2.0 ** nq * 2.0 ** -52 * scale:.3e}")
    assert np.abs(one - t).max() <= 2.0 ** nq * 2.0 ** -52 * scale


# ---- 5. the gradient ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rank", ["default", "maximum"])
def test_gate_adjoint_gradient(rank, kind):
    gates, terms, psi0, want_e, want_grad = gradient_fixture()
    nq = 12
    a0 = psi0.astype(np.complex64 if kind == "c64" else np.complex128)
    amps0 = gpu(a0)
    keep = bits_of(amps0).clone()
    max_rank = None if rank == "default" else TOP[kind]
    e, grad = A.gate_adjoint_gradient(amps0, gates, terms, max_rank=max_rank)
    assert torch.equal(bits_of(amps0), keep)
    assert isinstance(e, float) and grad.dtype == np.float64 and grad.shape == want_grad.shape == (60,)
    tol = gradient_bound(kind, len(gates), nq, terms)
    print(f"{kind} {rank}: E {want_e:.4f} err {abs(e - want_e):.3e}; |grad| {np.abs(want_grad).min():.3e} .. {np.abs(want_grad).max():.3e} "
          f"err {np.abs(grad - want_grad).max():.3e}; bound {tol:.3e} ratio {np.abs(grad - want_grad).max() / tol:.3f}")
    assert np.mean(np.abs(want_grad) > 20 * gradient_bound("c64", len(gates), nq, terms)) >= 0.8       # (the check below can fail)
    assert abs(e - want_e) <= tol
    assert np.all(np.abs(grad - want_grad) <= tol)


@pytest.mark.parametrize("kind", KINDS)
def test_gate_adjoint_gradient_with_shared_and_constant_parameters(kind):
    gates, terms, psi0, _, _ = gradient_fixture()
    nq = 12
    params = [j % 30 for j in range(60)]                   # the two layers share their angles ...
    for j in (3, 17, 41):                                  # ... and three gates are constants
        params[j] = -1
    want_e, want_grad = oracle_gate_gradient(psi0, gates, terms, params)
    amps0 = gpu(psi0.astype(np.complex64 if kind == "c64" else np.complex128))
    keep = bits_of(amps0).clone()
    e, grad = A.gate_adjoint_gradient(amps0, gates, terms, params)
    assert torch.equal(bits_of(amps0), keep) and grad.shape == want_grad.shape == (30,)
    m = np.array([sum(p == q for p in params) for q in range(30)])
    assert sorted(set(m)) == [1, 2]
    tol = m * gradient_bound(kind, len(gates), nq, terms)
    print(f"{kind} shared: err {np.abs(grad - want_grad).max():.3e} bound {tol.min():.3e} ratio {(np.abs(grad - want_grad) / tol).max():.3f}")
    assert abs(e - want_e) <= tol.min() and np.all(np.abs(grad - want_grad) <= tol)
    assert A.gate_adjoint_gradient(amps0, gates, terms, [-1] * 60)[1].shape == (0,)
    with pytest.raises(ValueError, match="params"):
        A.gate_adjoint_gradient(amps0, gates, terms, [0] * 59)
    with pytest.raises(ValueError, match="real coefficients"):
        A.gate_adjoint_gradient(amps0, gates, [(1j, "Z" * 12)])


# ---- 6. consistency with the Pauli-rotation adjoint -----------------------------------------------------------------------------
def rotation_case():
    """Two layers of rz, rx on every qubit and rzz on alternating bonds with SMALL angles -- the bound of adjoint_gradient grows
    with prod (|cos| + |sin|) over the rotations (tests/test_pauli_adjoint_gpu.py) -- on a product state of generic one-qubit
    states, whose gradients are of order 0.1 to 1."""
    nq = 12
    rng = np.random.default_rng(6)
    spec = []
    for layer in range(2):
        spec += [("rz", float(rng.uniform(-0.04, 0.04)), (q,)) for q in range(nq)]
        spec += [("rx", float(rng.uniform(-0.04, 0.04)), (q,)) for q in range(nq)]
        spec += [("rzz", float(rng.uniform(-0.04, 0.04)), (q, q + 1)) for q in range(layer, nq - 1, 2)]
    a = np.ones(1, dtype=np.complex128)
    for q in range(nq):
        polar, phase = rng.uniform(0.4, 1.2), rng.uniform(-np.pi, np.pi)
        a = np.kron(a, np.array([np.cos(polar), np.sin(polar) * np.exp(1j * phase)]))
    return spec, ising(list(range(nq))), a.reshape((2,) * nq)


@pytest.mark.parametrize("kind", KINDS)
def test_rotations_as_gates_give_the_gradient_of_adjoint_gradient(kind):
    nq = 12
    spec, terms, a128 = rotation_case()
    gates = [A.parametric_gate(*s) for s in spec]
    rotations = [(th / 2, {d: name[-1].upper() for d in dims}) for name, th, dims in spec]
    a0 = a128.astype(np.complex64 if kind == "c64" else np.complex128)
    e, grad = A.gate_adjoint_gradient(gpu(a0), gates, terms)
    e17, grad17 = A.adjoint_gradient(gpu(a0), rotations, terms)
    # d/dtheta of exp(-i (theta / 2) P) is half the derivative in the rotation's own angle
    allowed = gradient_bound(kind, len(gates), nq, terms) + energy_bound(kind, rotations, terms, a0)
    print(f"{kind}: E {e:.6f} / {e17:.6f}; |grad| up to {np.abs(grad).max():.3e}, difference {np.abs(grad - grad17 / 2).max():.3e}, "
          f"allowed {allowed:.3e}")
    assert np.abs(oracle_gate_gradient(a128, gates, terms)[1]).max() > 20 * allowed                 # (the check below can fail)
    assert abs(e - e17) <= allowed and np.all(np.abs(grad - grad17 / 2) <= allowed)


# ---- 7. refusals, each before any launch ----------------------------------------------------------------------------------------
def test_argument_checks():
    rng = np.random.default_rng(4)
    store = gpu(crand(rng, (2,) * 13, "c64"))
    gates = [(ASYM1, (0,)), (ASYM2, (11, 3))]
    measure = [ASYM1, None]
    lam, phi = store[0], store[1]
    with pytest.raises(ValueError, match="overlaps"):
        A.apply_gates_pair_(phi, phi, gates, measure)
    with pytest.raises(ValueError, match="built for shape"):
        A.apply_gates_pair_(lam.permute(1, 0, *range(2, 12)), phi, gates, measure)
    with pytest.raises(ValueError, match="built for shape"):
        A.apply_gates_pair_(lam.to(torch.complex128), phi, gates, measure)
    with pytest.raises(TypeError, match="complex"):
        A.apply_gates_pair_(lam.real.contiguous(), phi.real.contiguous(), gates, measure)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_gates_pair_(lam.cpu(), phi, gates, measure)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_gates_pair_(lam, phi.cpu(), gates, measure)
    with pytest.raises(ValueError, match="one entry per gate"):
        A.apply_gates_pair_(lam, phi, gates, [ASYM1])
    with pytest.raises(RuntimeError, match="artn error -2.*one or two"):
        A.apply_gates_pair_(lam, phi, [(np.eye(8), (0, 1, 2))])
    with pytest.raises(RuntimeError, match="artn error -2.*above the two-state maximum"):
        A.apply_gates_pair_(lam, phi, gates, measure, max_rank=4)
    with pytest.raises(RuntimeError, match="artn error -1.*measure"):
        A.apply_gates_pair_(lam, phi, gates, [ASYM1 * np.nan, None])
    keep = bits_of(store).clone()
    with pytest.raises(ValueError, match="not unitary"):
        A.gate_adjoint_gradient(phi, [A.parametric_gate("rx", 0.3, 0), (ASYM1, (1,))], [(1.0, "Z" * 12)])
    with pytest.raises(RuntimeError, match="above the two-state maximum"):     # (valid for the forward circuit alone)
        A.gate_adjoint_gradient(phi, [A.parametric_gate("rx", 0.3, 0)], [(1.0, "Z" * 12)], max_rank=4)
    with pytest.raises(ValueError, match="one or two dims"):
        A.gate_adjoint_gradient(phi, [(np.eye(8), (0, 1, 2))], [(1.0, "Z" * 12)])
    torch.cuda.synchronize()
    assert torch.equal(bits_of(store), keep)
    # the raw entry point: refusals that the Python layer never lets through
    circ = A.GatePairCircuit(phi.shape, phi.stride(), phi.dtype, gates, DEV, measure)
    out = torch.empty((2, 2), dtype=torch.float64, device=DEV)
    space = torch.empty(circ.workspace_bytes // 8, dtype=torch.float64, device=DEV)

    def call(lam_p, phi_p, table=circ._table.data_ptr(), tb=circ.table_bytes, ws=space.data_ptr(), wb=circ.workspace_bytes,
             out_p=out.data_ptr()):
        return N.lib().artn_gates_adjoint(ctypes.byref(circ._d), lam_p, phi_p, circ._k.ctypes.data_as(ctypes.c_void_p),
                                          circ._dims.ctypes.data_as(ctypes.c_void_p), 2, -1, table, tb, ws, wb, out_p,
                                          N.current_stream_ptr(store.device))
    lp, pp = lam.data_ptr(), phi.data_ptr()
    assert call(lp, lp + 8 * 2048) == -1 and b"overlaps" in N.lib().artn_last_error()
    assert call(None, pp) == -1 and call(lp, pp, table=None) == -1 and call(lp, pp, ws=None) == -1 and call(lp, pp, out_p=None) == -1
    assert call(lp, pp, wb=circ.workspace_bytes - 1) == -1 and call(lp, pp, tb=circ.table_bytes - 1) == -1
    assert call(lp + 8, pp) == -2 and call(lp, pp, ws=space.data_ptr() + 8) == -2
    torch.cuda.synchronize()
    assert torch.equal(bits_of(store), keep)
    assert call(lp, pp) == 0
    torch.cuda.synchronize()
    assert not torch.equal(bits_of(store), keep)


# ---- 8. side streams ------------------------------------------------------------------------------------------------------------
def test_one_circuit_on_two_streams():
    nq = 14
    gates, ms, inputs, _ = random_case(nq)
    lam0, phi0 = inputs["c64"]
    circ = A.GatePairCircuit((2,) * nq, gpu(phi0).stride(), torch.complex64, gates, DEV, ms)
    lam_d, phi_d = gpu(lam0), gpu(phi0)
    t_d = circ(lam_d, phi_d, device=True)
    states = [(gpu(lam0), gpu(phi0)) for _ in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    outs = []
    for st, (lam, phi) in zip(streams, states):
        with torch.cuda.stream(st):
            outs.append(circ(lam, phi, device=True))
    torch.cuda.synchronize()
    for t, (lam, phi) in zip(outs, states):
        assert torch.equal(t.view(torch.int64), t_d.view(torch.int64))
        assert torch.equal(bits_of(phi), bits_of(phi_d)) and torch.equal(bits_of(lam), bits_of(lam_d))
