"""The Krylov vector algebra and drivers on the device (artensor_amd/krylov.py): krylov_dots and krylov_combine_ against numpy
complex128 with derived bounds and against the package's own overlap / norm2 bit for bit, the refusals through Python, and the
Lanczos and exp(-i t H) drivers against dense np.kron matrices and the numpy restatement of tests/krylov_oracle.py.

Sizes: n in {1, 3, 4} (below one segment, a ragged tail alone, one segment), 1023 / 1024 / 1025 (around one tile), 4100 (several
workgroups and a tail), 2^21 + 1031 (more than one sweep of the 2048-workgroup grid, and a tail)."""
import math

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N

import krylov_oracle as KO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = N.KRYLOV_BATCH
SIZES = [1, 3, 4, 1023, 1024, 1025, 4100, 2 ** 21 + 1031]
DTYPES = [torch.complex64, torch.complex128]
P = {torch.complex64: 24, torch.complex128: 53}
NP = {torch.complex64: np.complex64, torch.complex128: np.complex128}
PERM12 = (7, 0, 11, 3, 5, 1, 9, 2, 10, 4, 8, 6)


def bits(t):
    """The stored bytes of a tensor in logical order, as unsigned integers (== on them is == on the bits)."""
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return a.view(np.uint32 if a.dtype == np.complex64 else np.uint64)


def vectors(count, shape, dtype, seed, perm=None):
    """`count` random vectors on the device (one generator call), each its own allocation, and their complex128 host copies."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    real = torch.float32 if dtype == torch.complex64 else torch.float64
    out = []
    for _ in range(count):
        t = torch.view_as_complex(torch.randn(tuple(shape) + (2,), dtype=real, device=DEV, generator=g))
        out.append(t.permute(perm) if perm is not None else t)
    return out, [v.cpu().numpy().astype(np.complex128) for v in out]


def layout_cases():
    cases = [((n,), None) for n in SIZES]
    cases.append(((2,) * 12, PERM12))
    return cases


def case_id(c):
    return "perm12" if c[1] is not None else f"n{c[0][0]}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["c64", "c128"])
@pytest.mark.parametrize("case", layout_cases(), ids=case_id)
def test_dots_against_numpy_and_bit_for_bit_against_overlap(case, dtype):
    shape, perm = case
    vs, hs = vectors(65, shape, dtype, 11, perm)                # a full basis: m = 64 is 64 / B launches into one workspace
    w, hw = vs[-1], hs[-1]
    vs, hs = vs[:-1], hs[:-1]
    n = hw.size
    ref = [A.overlap(v, w) for v in vs]                        # (<v|w>, |v|^2, |w|^2): the exact reference, computed once
    want = [np.vdot(h, hw) for h in hs]
    bound = [4 * (n + 4) * 2.0 ** -53 * float(np.sum(np.abs(h) * np.abs(hw))) for h in hs]
    for m in (1, 2, B, B + 1, 2 * B + 1, 63, 64):
        dots, nw = A.krylov_dots(vs[:m], w)
        assert dots.shape == (m,) and dots.dtype == np.complex128
        for j in range(m):
            err = abs(dots[j] - want[j])
            assert err <= bound[j], (m, j, err, bound[j])
            assert dots[j].real == ref[j][0].real and dots[j].imag == ref[j][0].imag, (m, j)      # whichever batch j falls in
        assert nw == ref[0][2]
        again, nw2 = A.krylov_dots(vs[:m], w)
        assert np.array_equal(again.view(np.uint64), dots.view(np.uint64)) and nw2 == nw
    d, dn = A.krylov_dots(vs[:B + 1], w, device=True)
    assert d.shape == (B + 1, 2) and d.dtype == torch.float64 and d.is_cuda and dn.dim() == 0
    assert d[:, 0].tolist() == [r[0].real for r in ref[:B + 1]] and d[:, 1].tolist() == [r[0].imag for r in ref[:B + 1]]
    assert float(dn) == ref[0][2]
    dots, nw = A.krylov_dots([w, vs[0], w], w)                 # w among the vectors: <w|w> = |w|^2 up to the order of the terms
    assert abs(dots[0] - nw) <= 4 * (n + 4) * 2.0 ** -53 * nw and dots[0].real == dots[2].real


def combine_reference(coeffs, hs):
    want = np.zeros(hs[0].shape, dtype=np.complex128)
    mag = np.zeros(hs[0].shape, dtype=np.float64)
    for c, h in zip(coeffs, hs):
        want += c * h
        mag += abs(c) * np.abs(h)
    return want, mag


@pytest.mark.parametrize("dtype", DTYPES, ids=["c64", "c128"])
@pytest.mark.parametrize("case", layout_cases(), ids=case_id)
def test_combine_against_numpy_and_its_exact_properties(case, dtype):
    shape, perm = case
    pool, hpool = vectors(17, shape, dtype, 23, perm)          # m = 64 cycles through 17 tensors: inputs may repeat
    rng = np.random.default_rng(3)
    y = torch.empty_like(pool[0])
    assert y.stride() == pool[0].stride()
    for m in (1, 2, 3, 17, 64):
        xs, hx = [pool[j % 17] for j in range(m)], [hpool[j % 17] for j in range(m)]
        coeffs = rng.standard_normal(m) + 1j * rng.standard_normal(m)
        if m >= 3:
            coeffs[1] = coeffs[1].real                          # a real and an imaginary coefficient among them
            coeffs[2] = 1j * coeffs[2].imag
        n2 = A.krylov_combine_(y, coeffs, xs)
        got = y.cpu().numpy()
        want, mag = combine_reference(coeffs, hx)
        bound = 8 * m * 2.0 ** -53 * mag
        for part in (np.real, np.imag):
            slack = bound + (2.0 ** -24 * np.abs(part(want)) if dtype == torch.complex64 else 0.0)
            err = np.abs(part(got).astype(np.float64) - part(want))
            assert np.all(err <= slack), (m, float((err - slack).max()))
        assert n2 == A.norm2(y), m                              # the reported norm: bit for bit norm2 of what was stored
        first = bits(y).copy()
        assert A.krylov_combine_(y, coeffs, xs) == n2 and np.array_equal(bits(y), first)          # two runs are identical
        # y = X_0, in place, equals the out-of-place result
        x0 = xs[0].clone()
        assert x0.stride() == xs[0].stride()
        n2_alias = A.krylov_combine_(x0, coeffs, [x0] + xs[1:])
        assert n2_alias == n2 and np.array_equal(bits(x0), first), m
        # terms with a zero coefficient change nothing, a vector full of NaN among them
        nan = torch.full_like(pool[0], complex(float("nan"), float("nan")))
        z = torch.empty_like(pool[0])
        if m < 62:
            n2_zero = A.krylov_combine_(z, [0.0] + list(coeffs[:1]) + [0.0] + list(coeffs[1:]) + [0j], [nan, xs[0], pool[5]] + xs[1:] + [nan])
            assert n2_zero == n2 and np.array_equal(bits(z), first), m
    # a lone vector with coefficient 1 is copied exactly; the dtype of the device result
    n2 = A.krylov_combine_(y, [1.0], [pool[3]], device=True)
    assert n2.dim() == 0 and n2.dtype == torch.float64 and n2.is_cuda
    assert np.array_equal(bits(y), bits(pool[3])) and float(n2) == A.norm2(pool[3])
    # the scale pass in place, and an all-zero combination
    x = pool[4].clone()
    n2 = A.krylov_combine_(x, [0.5], [x])
    assert np.array_equal(bits(x), bits(pool[4] * 0.5)) and n2 == A.norm2(x)        # (a power of two: exact)
    assert A.krylov_combine_(x, [0.0, 0.0], [pool[0], x]) == 0.0 and not bits(x).any()


def test_refusals_through_python():
    c128 = torch.zeros(64, dtype=torch.complex128, device=DEV)
    c64 = torch.zeros(64, dtype=torch.complex64, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps"):                              # partial overlap of y and an input
        A.krylov_combine_(c128[0:8], [1.0, 1.0], [c128[16:24], c128[4:12]])
    with pytest.raises(RuntimeError, match="overlaps"):
        A.krylov_combine_(c128[4:12], [1.0], [c128[0:8]])
    a = torch.zeros(2, 2, 2, dtype=torch.complex64, device=DEV)
    for call in (lambda: A.krylov_dots([a.permute(1, 0, 2)], a), lambda: A.krylov_combine_(a, [1.0], [a.permute(2, 1, 0)])):
        with pytest.raises(ValueError, match="equal strides"):                       # mismatched strides
            call()
    for call in (lambda: A.krylov_dots([c64[::2]], c64[::2]), lambda: A.krylov_combine_(c64[::2], [1.0], [c64[::2]])):
        with pytest.raises(ValueError, match="not dense"):                           # a view that is not dense
            call()
    for call in (lambda: A.krylov_dots([c64[1:5]], c64[1:5]), lambda: A.krylov_combine_(c64[1:5], [1.0], [c64[1:5]]),
                 lambda: A.krylov_dots([c64[1:5]], c64[8:12]), lambda: A.krylov_combine_(c64[8:12], [1.0], [c64[1:5]])):
        with pytest.raises(ValueError, match="16-byte"):                             # a view that starts at an odd element
            call()
    cpu = torch.zeros(8, dtype=torch.complex64)
    for call in (lambda: A.krylov_dots([cpu], c64[:8]), lambda: A.krylov_dots([c64[:8]], cpu),
                 lambda: A.krylov_combine_(cpu, [1.0], [c64[:8]]), lambda: A.krylov_combine_(c64[:8], [1.0], [cpu])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(ValueError, match="share dtype"):
        A.krylov_dots([c128[:8]], c64[:8])
    with pytest.raises(RuntimeError, match="at most 64"):                            # m = 65
        A.krylov_combine_(c64[:8], [1.0] * 65, [c64[8:16]] * 65)
    assert A.krylov_combine_(c64[:8], [1.0] * 64, [c64[8:16]] * 64) == 0.0
    with pytest.raises(ValueError, match="coefficients for"):
        A.krylov_combine_(c64[:8], [1.0, 2.0], [c64[8:16]])
    with pytest.raises(RuntimeError, match="finite"):
        A.krylov_combine_(c64[:8], [float("inf")], [c64[8:16]])
    with pytest.raises(ValueError, match="at least one"):
        A.krylov_dots([], c64[:8])
    # the drivers
    terms = KO.ising_terms(3, 1.0, 0.7)
    psi = torch.ones(2, 2, 2, dtype=torch.complex64, device=DEV)
    op = A.PauliSumOperator(psi.shape, psi.stride(), psi.dtype, terms, psi.device)
    with pytest.raises(ValueError, match=r"m \+ 1 = 66"):                            # more basis vectors than one launch combines
        A.lanczos(op, psi, 65)
    with pytest.raises(ValueError, match=r"m \+ 1 = 66"):
        A.krylov_evolve(psi, terms, 0.1, m=65)
    with pytest.raises(ValueError, match="keep_basis=False"):
        A.lanczos(op, psi, 5, reorthogonalize="full", keep_basis=False)
    with pytest.raises(ValueError, match="'full' or 'none'"):
        A.lanczos(op, psi, 5, reorthogonalize="partial")
    complex_terms = terms + [(0.5j, "XII")]
    with pytest.raises(ValueError, match="real coefficients"):
        A.lanczos_ground_state(psi, complex_terms)
    with pytest.raises(ValueError, match="real coefficients"):
        A.krylov_evolve(psi, complex_terms, 0.1)
    with pytest.raises(ValueError, match="norm"):
        A.lanczos(op, torch.zeros_like(psi), 3)
    for call in (lambda: A.lanczos(op, psi.cpu(), 3), lambda: A.lanczos_ground_state(psi.cpu(), terms),
                 lambda: A.krylov_evolve(psi.cpu(), terms, 0.1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def start_vector(nq, dtype, seed):
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(2 ** nq) + 1j * rng.standard_normal(2 ** nq)).astype(NP[dtype])
    return torch.from_numpy(v).reshape((2,) * nq).to(DEV), v


@pytest.mark.parametrize("dtype", DTYPES, ids=["c64", "c128"])
def test_lanczos_is_complete_on_sixty_four_states(dtype):
    """6 qubits, an Ising chain whose longitudinal field makes the spectrum distinct (smallest gap 0.0178), m = 64, full
    re-orthogonalisation.  tau and tau_orth are 8 times what the numpy restatement (stored vectors rounded to the dtype) shows on
    the same input, the factor covering the different summation order.  The restatement measured, on the CPU: complex64
    max |theta - lambda| 9.4e-8 and max |V^H V - I| 1.8e-7; complex128 1.9e-14 and 1.5e-15."""
    terms = KO.ising_terms(6, 1.0, 0.9, 0.35)
    h = KO.dense_hamiltonian(terms, 6)
    lam = np.linalg.eigvalsh(h)
    psi, host = start_vector(6, dtype, 64)
    store = None if dtype == torch.complex128 else np.complex64
    r = KO.lanczos_numpy(h, host, 64, "full", store=store)
    th = np.linalg.eigvalsh(KO.tridiagonal(r["alphas"], r["betas"]))
    tau = 8 * np.abs(th[:, None] - lam[None, :]).min(axis=1).max()
    tau_orth = 8 * np.abs(r["basis"].conj().T @ r["basis"] - np.eye(64)).max()
    op = A.PauliSumOperator(psi.shape, psi.stride(), psi.dtype, terms, psi.device)
    before = bits(psi).copy()
    res = A.lanczos(op, psi, 64, reorthogonalize="full")
    assert np.array_equal(bits(psi), before)
    assert res.iterations == 64 and len(res.alphas) == 64 and len(res.betas) == 63 and len(res.basis) == 64
    dist = np.abs(res.ritz_values[:, None] - lam[None, :]).min(axis=1).max()
    v = np.stack([b.cpu().numpy().reshape(-1).astype(np.complex128) for b in res.basis], axis=1)
    orth = np.abs(v.conj().T @ v - np.eye(64)).max()
    print(f"{dtype}: max distance of a Ritz value to the spectrum {dist:.3e} (tau {tau:.3e}), orthogonality {orth:.3e} (tau_orth {tau_orth:.3e}); "
          f"passes {res.passes}, peak {res.peak_bytes} bytes")
    assert dist <= tau
    assert abs(res.ritz_values[0] - lam[0]) <= tau and abs(res.ritz_values[-1] - lam[-1]) <= tau
    assert orth <= tau_orth
    assert res.passes > 0 and res.peak_bytes == 65 * 64 * psi.element_size()      # the basis and the last residual vector


GROUND_CASES = {
    # the numpy restatement converges in 44 (complex128, tol 1e-9 C) / 26 (complex64, tol 1e-4 C) steps at h = 1.5
    "ising": lambda: KO.ising_terms(10, 1.0, 1.5),
    # ... and in 34 / 20 steps on the Heisenberg chain
    "heisenberg": lambda: KO.heisenberg_terms(10, 1.0),
}
_DENSE = {}


def dense_case(name):
    """(terms, H, eigenvalues, C) of a 10-qubit case: built once and shared."""
    if name not in _DENSE:
        terms = GROUND_CASES[name]()
        h = KO.dense_hamiltonian(terms, 10)
        _DENSE[name] = (terms, h, np.linalg.eigvalsh(h), sum(abs(c) for c, _ in terms))
    return _DENSE[name]


@pytest.mark.parametrize("dtype", DTYPES, ids=["c64", "c128"])
@pytest.mark.parametrize("name", list(GROUND_CASES))
def test_ground_state(name, dtype):
    terms, h, lam, c = dense_case(name)
    p = P[dtype]
    tol = (1e-9 if dtype == torch.complex128 else 1e-4) * c
    psi, host = start_vector(10, dtype, 10)
    r = KO.lanczos_numpy(h, host, 200, "full", tol=tol, store=None if dtype == torch.complex128 else np.complex64)
    assert r["converged"] and r["iterations"] <= 100            # within half of max_iter
    e0, state, info = A.lanczos_ground_state(psi, terms, max_iter=200, tol=tol, reorthogonalize="full")
    m = info.iterations
    x = state.cpu().numpy().reshape(-1).astype(np.complex128)
    x /= np.linalg.norm(x)
    res = np.linalg.norm(h @ x - e0 * x)
    rounding = 64 * m * 2.0 ** -p * c
    expect = A.pauli_sum_expectation(state, terms)
    print(f"{name} {dtype}: {m} steps (restatement {r['iterations']}), E0 {e0:.12f} (lambda_0 {lam[0]:.12f}), |r| {res:.3e} "
          f"(bound {tol + rounding:.3e}), |E - <H>| {abs(e0 - expect):.3e}, passes {info.passes}")
    assert info.converged and info.restarts == 0 and m <= 100
    assert res <= tol + rounding
    assert abs(e0 - lam[0]) <= res
    assert abs(e0 - lam[0]) < abs(e0 - lam[1])
    assert abs(e0 - expect) <= tol + rounding
    assert state.shape == psi.shape and state.stride() == psi.stride() and state.dtype == dtype


@pytest.mark.parametrize("dtype", DTYPES, ids=["c64", "c128"])
def test_evolution_from_the_complete_space(dtype):
    """6 qubits, m = 64, C t = 2: the Krylov space is the whole space, so the result is exp(-i t H) psi to rounding."""
    p = P[dtype]
    terms = KO.ising_terms(6, 1.0, 0.9, 0.35)
    h = KO.dense_hamiltonian(terms, 6)
    c = sum(abs(x) for x, _ in terms)
    psi, host = start_vector(6, dtype, 6)
    norm = np.linalg.norm(host.astype(np.complex128))
    t = 2.0 / c
    out, err = A.krylov_evolve(psi, terms, t, m=64)
    got = out.cpu().numpy().reshape(-1).astype(np.complex128)
    exact = KO.expm_exact(h, host, t)
    miss = np.linalg.norm(got - exact)
    print(f"{dtype}: error {miss:.3e} (bound {64 * 64 * 2.0 ** -p * 3 * norm:.3e}), estimate {err:.3e}")
    assert miss <= 64 * 64 * 2.0 ** -p * (1 + c * t) * norm
    assert abs(np.linalg.norm(got) - norm) <= 64 * 64 * 2.0 ** -p * norm


@pytest.mark.parametrize("dtype", DTYPES, ids=["c64", "c128"])
def test_evolution_with_thirty_vectors(dtype):
    """10 qubits, m = 30, C t = 24: long enough that the truncation of the Krylov space shows (the restatement misses the exact
    result by 1.0e-5 in complex128 and 1.4e-5 with complex64 storage, the estimate says 2.9e-4)."""
    p, m = P[dtype], 30
    terms, h, _, c = dense_case("ising")
    psi, host = start_vector(10, dtype, 30)
    norm = np.linalg.norm(host.astype(np.complex128))
    t = 24.0 / c
    exact = KO.expm_exact(h, host, t)
    ref, _ = KO.evolve_numpy(h, host, t, m, store=None if dtype == torch.complex128 else np.complex64)
    ref_miss = np.linalg.norm(ref - exact)
    before = bits(psi).copy()
    target = torch.empty_like(psi)
    out, err = A.krylov_evolve(psi, terms, t, m=m, out=target)
    assert out is target and np.array_equal(bits(psi), before)          # out= is honoured, the input untouched
    got = out.cpu().numpy().reshape(-1).astype(np.complex128)
    miss = np.linalg.norm(got - exact)
    rounding = 64 * m * 2.0 ** -p * (1 + c * t) * norm
    print(f"{dtype}: error {miss:.3e}, estimate {err:.3e}, restatement {ref_miss:.3e}, rounding term {rounding:.3e}")
    assert miss <= 8 * err + rounding
    assert miss <= 8 * ref_miss
    assert abs(np.linalg.norm(got) - norm) <= 64 * m * 2.0 ** -p * norm
    # t = 0 returns the input to two roundings (the scale pass and the combination); the coefficients exp(0) S S^T e_1 are e_1 to
    # float64 rounding only, which spreads 64 m 2^-53 |psi| over the elements
    out0, err0 = A.krylov_evolve(psi, terms, 0.0, m=m)
    a = host.astype(np.complex128)
    d = np.abs(out0.cpu().numpy().reshape(-1).astype(np.complex128) - a)
    assert np.all(d <= 2 * 2.0 ** -p * np.abs(a) * math.sqrt(2.0) + 64 * m * 2.0 ** -53 * norm)
    with pytest.raises(ValueError, match="out must have"):
        A.krylov_evolve(psi, terms, t, m=m, out=torch.empty(1024, dtype=dtype, device=DEV))


def test_lanczos_takes_any_callable_and_runs_without_a_basis():
    """A diagonal operator written with torch: 32 distinct entries, so 32 steps find all of them; then the three-vector form
    (no re-orthogonalisation, no basis) against the restatement's first steps."""
    rng = np.random.default_rng(32)
    diag = np.sort(rng.standard_normal(32)) + np.arange(32) * 0.05
    d = torch.from_numpy(diag.astype(np.complex128)).reshape((2,) * 5).to(DEV)
    calls = []

    def op(x, out):
        calls.append(1)
        return torch.mul(x, d, out=out)

    psi, host = start_vector(5, torch.complex128, 5)
    res = A.lanczos(op, psi, 32, reorthogonalize="full")
    scale = np.abs(diag).max()
    assert res.iterations == 32 == len(calls)
    assert np.abs(res.ritz_values - diag).max() <= 64 * 32 * 2.0 ** -53 * scale * 32
    ref = KO.lanczos_numpy(np.diag(diag).astype(np.complex128), host, 12, "none")
    res = A.lanczos(op, psi, 12, reorthogonalize="none", keep_basis=False)
    assert res.basis is None and res.iterations == 12 and res.peak_bytes == 3 * 32 * 16
    assert np.abs(res.alphas - ref["alphas"]).max() <= 2.0 ** -30 * scale and np.abs(res.betas - ref["betas"]).max() <= 2.0 ** -30 * scale
    kept = A.lanczos(op, psi, 12, reorthogonalize="none")
    assert np.array_equal(kept.alphas, res.alphas) and np.array_equal(kept.betas, res.betas) and len(kept.basis) == 12
    with pytest.raises(ValueError, match="must write into"):
        A.lanczos(lambda x, out: x * 2, psi, 3)
