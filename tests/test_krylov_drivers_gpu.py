"""The branches of the Krylov drivers (artensor_amd/krylov.py) that decide whether a user gets a right answer: a breakdown at the
first step and at a later one, the second re-orthogonalisation sweep, the `tol` stop, restarts of lanczos_ground_state, states
viewed through a permutation of their dims, and every call on a side stream.  References are dense np.kron matrices in complex128
and the numpy restatement of tests/krylov_oracle.py with `store=` set to the storage dtype; a bound is tol + 64 m 2^-p C or 8 times
what the restatement shows on the same input, as in test_krylov_gpu.py.

`passes` is checked against the sum the docstrings define, written out in want_passes below."""
import cmath
import math

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import krylov

import krylov_oracle as KO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B = N.KRYLOV_BATCH
DTYPES = [torch.complex64, torch.complex128]
IDS = ["c64", "c128"]
P = {torch.complex64: 24, torch.complex128: 53}
NP = {torch.complex64: np.complex64, torch.complex128: np.complex128}
STORE = {torch.complex64: np.complex64, torch.complex128: None}
PERM10 = (7, 0, 3, 5, 1, 9, 2, 4, 8, 6)


def bits(t):
    """The stored bytes of a tensor in logical order, as unsigned integers (== on them is == on the bits)."""
    a = np.ascontiguousarray(t.detach().cpu().numpy())
    return a.view(np.uint32 if a.dtype == np.complex64 else np.uint64)


def host(t):
    return t.cpu().numpy().reshape(-1).astype(np.complex128)


def start_vector(nq, dtype, seed):
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal(2 ** nq) + 1j * rng.standard_normal(2 ** nq)).astype(NP[dtype])
    return torch.from_numpy(v).reshape((2,) * nq).to(DEV), v


def on_device(v, dtype, nq):
    return torch.from_numpy(np.asarray(v).astype(NP[dtype])).reshape((2,) * nq).to(DEV)


_DENSE = {}


def permuted(terms):
    """The strings for a state viewed through PERM10: dim d of the view is dim PERM10[d] of the contiguous tensor."""
    return [(c, "".join(s[PERM10[d]] for d in range(10))) for c, s in terms]


def dense_case(name, perm=False):
    """(terms, H, eigenvalues, C) of a 10-qubit chain, as it is or with its strings permuted (the spectrum is the same one): built
    once and shared, never written."""
    if (name, perm) not in _DENSE:
        terms = KO.ising_terms(10, 1.0, 1.5) if name == "ising" else KO.heisenberg_terms(10, 1.0)
        if perm:
            _, _, lam, c = dense_case(name)
            _DENSE[name, perm] = (permuted(terms), KO.dense_hamiltonian(permuted(terms), 10), lam, c)
        else:
            h = KO.dense_hamiltonian(terms, 10)
            _DENSE[name, perm] = (terms, h, np.linalg.eigvalsh(h), sum(abs(c) for c, _ in terms))
    return _DENSE[name, perm]


def want_passes(steps, second=(), scaled=None, ritz_vector=False):
    """What the docstrings of KrylovResult, lanczos and lanczos_ground_state add up to for one run of `steps` steps with full
    re-orthogonalisation: a pass is one read or one write of a state-sized vector.  norm2 of the start reads it (1) and the
    normalisation reads it and writes v_0 (2).  Step j applies the operator (one read, one write), then sweeps: krylov_dots reads
    each of the j + 1 basis vectors once and w once per batch of B of them, and the removal reads w and the vectors and writes w
    in launches of at most 63 vectors; a step in `second` sweeps twice.  Every step but the last scales w into the next basis
    vector (one read, one write); `scaled` overrides that count.  The Ritz vector of lanczos_ground_state reads the basis and
    writes the state."""
    total = 1 + 2
    for j in range(steps):
        k = j + 1
        sweep = k + -(-k // B) + sum(min(63, k - at) + 2 for at in range(0, k, 63))
        total += 2 + sweep * (2 if j in second else 1)
    total += 2 * (steps - 1 if scaled is None else scaled)
    return total + (steps + 1 if ritz_vector else 0)


DIAGONAL_TERMS = [(-1.0, "ZZII"), (-1.0, "IZZI"), (-1.0, "IIZZ"), (0.25, "ZIII"), (0.5, "IIZI")]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_an_eigenstate_start_breaks_down_at_the_first_step(dtype):
    """H is diagonal, so basis state 5 = |0101> is an exact eigenstate in both dtypes with the eigenvalue 3 + 0.25 + 0.5 = 3.75;
    the start is 3 e_5.  Every number of the run is exact: the normalised start is e_5, H e_5 = 3.75 e_5, the removal leaves 0."""
    p = P[dtype]
    v0 = np.zeros(16, dtype=np.complex128)
    v0[5] = 3.0
    psi = on_device(v0, dtype, 4)
    e5 = on_device(v0 / 3.0, dtype, 4)
    h = KO.dense_hamiltonian(DIAGONAL_TERMS, 4)
    assert h[5, 5] == 3.75 and np.count_nonzero(h - np.diag(np.diag(h))) == 0
    r = KO.lanczos_numpy(h, v0, 8, "full", store=STORE[dtype])
    assert r["iterations"] == 1 and r["breakdown"] and r["alphas"].tolist() == [3.75]
    op = A.PauliSumOperator(psi.shape, psi.stride(), psi.dtype, DIAGONAL_TERMS, psi.device)
    before = bits(psi).copy()
    nbytes = 16 * psi.element_size()
    res = A.lanczos(op, psi, 8, reorthogonalize="full")
    assert res.iterations == 1 and res.breakdown and res.converged
    assert res.alphas.tolist() == [3.75] and res.betas.shape == (0,) and res.ritz_values.tolist() == [3.75]
    assert res.beta_last == 0.0 and res.residual == 0.0 and res.norm0 == 3.0
    assert len(res.basis) == 1 and np.array_equal(bits(res.basis[0]), bits(e5))
    assert res.passes == want_passes(1, second={0}) == 15      # (the sweep that leaves nothing is repeated)
    assert res.peak_bytes == 2 * nbytes                        # v_0 and the residual vector
    for mode, keep in (("none", True), ("none", False)):
        res = A.lanczos(op, psi, 8, reorthogonalize=mode, keep_basis=keep)
        assert res.iterations == 1 and res.breakdown and res.converged and res.alphas.tolist() == [3.75] and res.betas.shape == (0,)
        assert res.beta_last == 0.0 and res.residual == 0.0 and (len(res.basis) == 1 if keep else res.basis is None)
    e0, state, info = A.lanczos_ground_state(psi, DIAGONAL_TERMS)
    assert e0 == 3.75 and np.array_equal(bits(state), bits(e5))
    assert info.restarts == 0 and info.iterations == 1 and info.breakdown and info.converged and info.residual == 0.0
    assert info.alphas.tolist() == [3.75] and [len(b) for b in info.betas] == [0]
    assert info.passes == want_passes(1, second={0}, ritz_vector=True) == 17 and info.peak_bytes == 3 * nbytes
    for out in (None, torch.empty_like(psi)):
        got, err = A.krylov_evolve(psi, DIAGONAL_TERMS, 0.7, m=8, out=out)
        assert out is None or got is out
        g = host(got)
        want = 3.0 * cmath.exp(-0.7j * 3.75)
        # two roundings of the dtype, and the coefficient exp(-i t T) e_1 to float64 rounding (the form of the t = 0 check of
        # test_evolution_with_thirty_vectors, with m = 1)
        print(f"{dtype}: |out_5 - 3 exp(-0.7i 3.75)| {abs(g[5] - want):.3e}")
        assert abs(g[5] - want) <= 2 * 2.0 ** -p * abs(want) * math.sqrt(2.0) + 64 * 2.0 ** -53 * 3.0
        assert not np.delete(g, 5).any() and err == 0.0
    assert np.array_equal(bits(psi), before)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_start_vector_the_operator_annihilates(dtype):
    """(Z I - I Z)|00> = 0: the scale of the breakdown test is 0 and so is beta."""
    terms = [(1.0, "ZI"), (-1.0, "IZ")]
    v0 = np.array([1.0, 0.0, 0.0, 0.0])
    psi = on_device(v0, dtype, 2)
    assert not (KO.dense_hamiltonian(terms, 2) @ v0).any()
    op = A.PauliSumOperator(psi.shape, psi.stride(), psi.dtype, terms, psi.device)
    for mode in ("full", "none"):
        res = A.lanczos(op, psi, 4, reorthogonalize=mode)
        assert res.iterations == 1 and res.breakdown and res.converged
        assert res.alphas.tolist() == [0.0] and res.betas.shape == (0,) and res.ritz_values.tolist() == [0.0]
        assert res.beta_last == 0.0 and res.residual == 0.0 and len(res.basis) == 1 and np.array_equal(bits(res.basis[0]), bits(psi))
    e0, state, info = A.lanczos_ground_state(psi, terms)
    assert e0 == 0.0 and np.array_equal(bits(state), bits(psi)) and info.restarts == 0 and info.breakdown
    assert math.isfinite(info.residual) and math.isfinite(info.tol) and np.isfinite(host(state)).all()
    out, err = A.krylov_evolve(psi, terms, 0.7, m=4)
    assert np.array_equal(host(out), v0) and err == 0.0


def diagonal32():
    """The 32 distinct entries of test_lanczos_takes_any_callable_and_runs_without_a_basis."""
    rng = np.random.default_rng(32)
    return np.sort(rng.standard_normal(32)) + np.arange(32) * 0.05


def diagonal_operator(entries, dtype):
    """op(x, out) = entries * x written with torch, and the entries as the device stores them (rounded to the real dtype)."""
    stored = entries.astype(NP[dtype]).astype(np.complex128)
    d = torch.from_numpy(entries.astype(NP[dtype])).reshape((2,) * 5).to(DEV)
    return (lambda x, out: torch.mul(x, d, out=out)), np.diag(stored)


SUPPORT = [3, 9, 14, 20, 27]


@pytest.mark.parametrize("mode", ["full", "none"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_a_small_invariant_subspace_breaks_down_after_five_steps(dtype, mode):
    """A start vector on five entries of a diagonal operator spans an invariant subspace of dimension 5: the sixth vector is
    rounding alone.  With full re-orthogonalisation (both dtypes) and with none in complex128 the restatement breaks down after
    exactly 5 steps with the five entries as Ritz values.  With "none" and complex64 storage it does not: the beta of step 5 is
    rounding of complex64, 1e-6, far above 2^-40, and the run goes on to 12 steps with Ritz values off the spectrum -- the limit
    of the fixed threshold that the docstring of lanczos states; there the device must agree with the restatement."""
    diag = diagonal32()
    op, h = diagonal_operator(diag, dtype)
    rng = np.random.default_rng(5)
    v0 = np.zeros(32, dtype=np.complex128)
    v0[SUPPORT] = rng.standard_normal(5) + 1j * rng.standard_normal(5)
    v0 = v0.astype(NP[dtype])
    psi = on_device(v0, dtype, 5)
    r = KO.lanczos_numpy(h, v0, 12, mode, store=STORE[dtype])
    res = A.lanczos(op, psi, 12, reorthogonalize=mode)
    print(f"{dtype} {mode}: {res.iterations} steps (restatement {r['iterations']}), breakdown {res.breakdown}, restatement's last "
          f"beta / (2^-40 scale) {r['breakdown_ratio']:.3e}")
    if dtype == torch.complex64 and mode == "none":
        assert r["iterations"] == 12 and not r["breakdown"] and r["breakdown_ratio"] > 2.0 ** 20
        assert res.iterations == 12 and not res.breakdown and not res.converged and len(res.basis) == 12
        return
    want = diag.astype(NP[dtype]).real.astype(np.float64)[SUPPORT]
    ref_err = np.abs(np.linalg.eigvalsh(KO.tridiagonal(r["alphas"], r["betas"])) - want).max()
    assert r["iterations"] == 5 and r["breakdown"] and 0.0 < ref_err
    err = np.abs(res.ritz_values - want).max()
    print(f"    Ritz values against the five entries {err:.3e} (restatement {ref_err:.3e})")
    assert res.iterations == 5 and res.breakdown and res.converged and res.beta_last == 0.0 and res.residual == 0.0
    assert len(res.alphas) == 5 and len(res.betas) == 4 and len(res.basis) == 5
    assert err <= 8 * ref_err
    off = np.setdiff1d(np.arange(32), SUPPORT)
    for b in res.basis:
        assert not host(b)[off].any()
    if mode == "full":
        assert res.peak_bytes == 6 * 32 * psi.element_size()


RESTARTS = [(torch.complex64, 70, [64, 6]), (torch.complex64, 130, [64, 64, 2]), (torch.complex128, 70, [64, 1])]


@pytest.mark.parametrize("dtype,max_iter,runs", RESTARTS, ids=["c64-70", "c64-130", "c128-70"])
def test_restarts_of_the_ground_state_run(dtype, max_iter, runs):
    """The 10-qubit Ising chain with tol = 0, so that only a breakdown ends a run early.  The restatement gives the runs above.
    In complex128 the restart vector is an eigenvector to rounding and the restatement's second run breaks down at its first step,
    a factor 400 under the threshold (test_krylov_cpu.py prints it); where the device lands is not known, so both outcomes pass:
    65 steps ending in a breakdown, or all 70 without one."""
    terms, h, lam, c = dense_case("ising")
    p = P[dtype]
    psi, v0 = start_vector(10, dtype, 10)
    nbytes = 1024 * psi.element_size()
    e_ref, _, done_ref, restarts_ref, runs_ref, last = KO.ground_state_numpy(h, v0, max_iter, 0.0, "full", store=STORE[dtype])
    assert runs_ref == runs and restarts_ref == len(runs) - 1
    # the restatement's first sweeps, run by run: where a second one follows, and that none of them is near the threshold
    second, x = [], v0
    for k in runs:
        r = KO.lanczos_numpy(h, x, k, "full", tol=0.0, store=STORE[dtype])
        assert not np.any((r["first_sweep"] > 0.25 / 1.5) & (r["first_sweep"] < 0.25 * 1.5))
        second.append(set(np.nonzero(r["first_sweep"] < 0.25)[0].tolist()))
        _, s = np.linalg.eigh(KO.tridiagonal(r["alphas"], r["betas"]))
        x = r["basis"][:, :k] @ s[:, 0]
        x = x if STORE[dtype] is None else x.astype(np.complex64)
    assert second[0] == set() and all(s == {0} for s in second[1:])        # a restart vector is nearly an eigenvector
    before = bits(psi).copy()
    e0, state, info = A.lanczos_ground_state(psi, terms, max_iter=max_iter, tol=0.0, reorthogonalize="full")
    assert np.array_equal(bits(psi), before)
    x = host(state)
    x /= np.linalg.norm(x)
    res = np.linalg.norm(h @ x - e0 * x)
    rounding = 64 * max_iter * 2.0 ** -p * c
    got_runs = [len(b) + 1 for b in info.betas]
    print(f"{dtype} max_iter {max_iter}: runs {got_runs} (restatement {runs_ref}), E0 - lambda_0 {e0 - lam[0]:.3e} (restatement "
          f"{e_ref - lam[0]:.3e}), |r| {res:.3e} (bound {rounding:.3e}), breakdown {info.breakdown}, passes {info.passes}")
    assert state.shape == psi.shape and state.stride() == psi.stride() and state.dtype == dtype
    assert info.restarts == len(runs) - 1 and info.tol == 0.0 and info.basis is None
    assert isinstance(info.betas, list) and all(isinstance(b, np.ndarray) for b in info.betas)
    assert len(info.alphas) == info.iterations == sum(got_runs)
    if dtype == torch.complex64:
        assert info.iterations == max_iter and not info.converged and not info.breakdown
        assert got_runs == runs
        assert abs(e0 - lam[0]) <= res <= rounding
        assert info.passes == sum(want_passes(k, second=s, ritz_vector=True) for k, s in zip(runs, second))
    else:
        assert (info.breakdown and info.converged and info.iterations == 65 and got_runs == [64, 1] and info.residual == 0.0) \
            or (not info.converged and not info.breakdown and info.iterations == 70 and got_runs == [64, 6])
        assert abs(e0 - lam[0]) <= rounding and res <= rounding
        first = want_passes(64, ritz_vector=True)
        if info.breakdown:
            assert info.passes == first + want_passes(1, second={0}, ritz_vector=True)
        else:                                                  # which later steps sweep twice is not known
            assert first + want_passes(6, second={0}, ritz_vector=True) <= info.passes \
                <= first + want_passes(6, second=set(range(6)), ritz_vector=True)
    assert abs(e0 - lam[0]) < abs(e0 - lam[1])
    # the basis, the residual vector and one state; the start of a restarted run is a second state
    assert info.peak_bytes == (64 + 1 + (2 if len(runs) > 2 else 1)) * nbytes
    # a restart does not lose ground: the Rayleigh quotient of the first run's Ritz vector, recomputed here
    op = A.PauliSumOperator(psi.shape, psi.stride(), psi.dtype, terms, psi.device)
    one = A.lanczos(op, psi, 64, reorthogonalize="full", tol=0.0)
    assert one.iterations == 64 and not one.converged and np.array_equal(one.alphas, info.alphas[:64])
    assert np.array_equal(one.betas, info.betas[0]) and one.passes == want_passes(64) and one.peak_bytes == 65 * nbytes
    theta, s = krylov.ritz(one.alphas, one.betas)
    ritz_vector = torch.empty_like(psi)
    A.krylov_combine_(ritz_vector, s[:, 0], one.basis)
    quotient = A.pauli_sum_expectation(ritz_vector, terms)
    print(f"    Rayleigh quotient of the first Ritz vector - lambda_0 {quotient - lam[0]:.3e}, theta_0 - lambda_0 {theta[0] - lam[0]:.3e}")
    assert abs(quotient - theta[0]) <= rounding and e0 <= quotient + rounding


def quotients(v, h, store):
    """<v_j|w_j> / <v_j|v_j> of the columns of v, with w_j = h v_j as the run stores it."""
    w = h @ v if store is None else (h @ v).astype(store).astype(np.complex128)
    return (np.einsum("ij,ij->j", v.conj(), w) / np.einsum("ij,ij->j", v.conj(), v)).real


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_second_sweep_where_w_is_almost_parallel_to_v(dtype):
    """op = D + 1000 with D the 32-entry diagonal: |op(v_j)|^2 is 1e6 and what is left after the first sweep is of order 1, so the
    second sweep runs at every step (asserted through the restatement) and its correction to alpha is what the cancellation lost."""
    diag = diagonal32()
    op, h = diagonal_operator(diag + 1000.0, dtype)
    psi, v0 = start_vector(5, dtype, 5)
    r = KO.lanczos_numpy(h, v0, 32, "full", store=STORE[dtype])
    assert r["iterations"] == 32 and r["first_sweep"].shape == (32,) and r["first_sweep"].max() < 0.25 / 1.5
    ref_err = np.abs(np.linalg.eigvalsh(KO.tridiagonal(r["alphas"], r["betas"])) - 1000.0 - diag).max()
    ref_orth = np.abs(r["basis"].conj().T @ r["basis"] - np.eye(32)).max()
    ref_alpha = np.abs(r["alphas"] - quotients(r["basis"], h, STORE[dtype])).max()
    res = A.lanczos(op, psi, 32, reorthogonalize="full")
    v = np.stack([host(b) for b in res.basis], axis=1)
    err = np.abs(res.ritz_values - 1000.0 - diag).max()
    orth = np.abs(v.conj().T @ v - np.eye(32)).max()
    alpha = np.abs(res.alphas - quotients(v, h, STORE[dtype])).max()
    print(f"{dtype}: Ritz values - 1000 against the diagonal {err:.3e} (restatement {ref_err:.3e}), orthogonality {orth:.3e} "
          f"(restatement {ref_orth:.3e}), alphas against the Rayleigh quotients of the basis {alpha:.3e} (restatement {ref_alpha:.3e})")
    assert res.iterations == 32 and len(res.alphas) == 32 and len(res.betas) == 31 and len(res.basis) == 32
    assert err <= 8 * ref_err and orth <= 8 * ref_orth
    # what the second sweep adds to alpha_j is 1000 (1 - |v_j|^2) to first order: with it alpha_j is the Rayleigh quotient of the
    # stored v_j, without it alpha_j is off by 1000 times the rounding of the dtype
    assert 0.0 < ref_alpha and alpha <= 8 * ref_alpha
    assert res.passes == want_passes(32, second=set(range(32)))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_the_drivers_on_a_permuted_view(dtype):
    """A 10-qubit state viewed through a permutation of its dims, with the strings permuted to match: the Heisenberg ground state
    and the Ising evolution with 30 vectors, to the bounds of test_ground_state and test_evolution_with_thirty_vectors, against
    the dense matrix of the permuted strings."""
    p = P[dtype]
    base, _ = start_vector(10, dtype, 10)
    psi = base.permute(PERM10)
    assert not psi.is_contiguous() and psi.stride() != base.stride()
    v0 = host(psi)
    before = bits(psi).copy()
    # the ground state
    terms, h, lam, c = dense_case("heisenberg", perm=True)
    assert [s for _, s in terms] != [s for _, s in dense_case("heisenberg")[0]]
    tol = (1e-9 if dtype == torch.complex128 else 1e-4) * c
    e0, state, info = A.lanczos_ground_state(psi, terms, max_iter=200, tol=tol, reorthogonalize="full")
    m = info.iterations
    x = host(state)
    x /= np.linalg.norm(x)
    res = np.linalg.norm(h @ x - e0 * x)
    rounding = 64 * m * 2.0 ** -p * c
    expect = A.pauli_sum_expectation(state, terms)
    print(f"{dtype}: {m} steps, E0 - lambda_0 {e0 - lam[0]:.3e}, |r| {res:.3e} (bound {tol + rounding:.3e}), |E - <H>| {abs(e0 - expect):.3e}")
    assert info.converged and info.restarts == 0 and m <= 100
    assert res <= tol + rounding and abs(e0 - lam[0]) <= res and abs(e0 - lam[0]) < abs(e0 - lam[1])
    assert abs(e0 - expect) <= tol + rounding
    assert state.shape == psi.shape and state.stride() == psi.stride() and state.dtype == dtype
    # the evolution
    terms, h, _, c = dense_case("ising", perm=True)
    norm = np.linalg.norm(v0)
    t, m = 24.0 / c, 30
    exact = KO.expm_exact(h, v0, t)
    ref, _ = KO.evolve_numpy(h, v0, t, m, store=STORE[dtype])
    ref_miss = np.linalg.norm(ref - exact)
    rounding = 64 * m * 2.0 ** -p * (1 + c * t) * norm
    target = torch.empty_like(psi)
    assert target.stride() == psi.stride()
    results = []
    for out in (None, target):
        got, err = A.krylov_evolve(psi, terms, t, m=m, out=out)
        assert (got is target) if out is not None else (got.stride() == psi.stride() and got.shape == psi.shape)
        miss = np.linalg.norm(host(got) - exact)
        print(f"{dtype}: error {miss:.3e}, estimate {err:.3e}, restatement {ref_miss:.3e}, rounding term {rounding:.3e}")
        assert miss <= 8 * err + rounding and miss <= 8 * ref_miss
        assert abs(np.linalg.norm(host(got)) - norm) <= 64 * m * 2.0 ** -p * norm
        results.append(bits(got).copy())
    assert np.array_equal(results[0], results[1])
    with pytest.raises(ValueError, match="out must have"):       # the strides of the contiguous layout
        A.krylov_evolve(psi, terms, t, m=m, out=torch.empty_like(base))
    assert np.array_equal(bits(psi), before)


def test_lanczos_stops_on_tol_and_runs_without_a_basis_in_complex64():
    """lanczos with `tol` called directly (lanczos_ground_state hides it behind restarts), and the three-vector form in complex64
    against the restatement with complex64 storage, to 8 times that restatement's own deviation from its complex128 run."""
    terms, h, lam, c = dense_case("ising")
    for dtype in DTYPES:
        tol = (1e-9 if dtype == torch.complex128 else 1e-4) * c
        psi, v0 = start_vector(10, dtype, 10)
        r = KO.lanczos_numpy(h, v0, 64, "full", tol=tol, store=STORE[dtype])
        assert r["converged"] and not r["breakdown"] and r["iterations"] < 62
        op = A.PauliSumOperator(psi.shape, psi.stride(), psi.dtype, terms, psi.device)
        res = A.lanczos(op, psi, 64, reorthogonalize="full", tol=tol)
        print(f"{dtype}: stopped after {res.iterations} steps (restatement {r['iterations']}), residual {res.residual:.3e} (tol {tol:.3e})")
        assert abs(res.iterations - r["iterations"]) <= 2 and res.converged and not res.breakdown and 0.0 < res.residual < tol
        k = res.iterations
        assert len(res.alphas) == k == len(res.basis) and len(res.betas) == k - 1 and res.beta_last > 0.0
        assert res.passes == want_passes(k) and res.peak_bytes == (k + 1) * 1024 * psi.element_size()
        assert abs(res.ritz_values[0] - lam[0]) <= tol + 64 * k * 2.0 ** -P[dtype] * c
    diag = diagonal32()
    op, h32 = diagonal_operator(diag, torch.complex64)
    psi, v0 = start_vector(5, torch.complex64, 5)
    ref = KO.lanczos_numpy(h32, v0, 12, "none", store=np.complex64)
    ref128 = KO.lanczos_numpy(h32, v0, 12, "none")
    dev_a, dev_b = np.abs(ref["alphas"] - ref128["alphas"]).max(), np.abs(ref["betas"] - ref128["betas"]).max()
    res = A.lanczos(op, psi, 12, reorthogonalize="none", keep_basis=False)
    got_a, got_b = np.abs(res.alphas - ref["alphas"]).max(), np.abs(res.betas - ref["betas"]).max()
    print(f"complex64 without a basis: alphas {got_a:.3e} (restatement against complex128 {dev_a:.3e}), betas {got_b:.3e} ({dev_b:.3e})")
    assert res.basis is None and res.iterations == 12 and res.peak_bytes == 3 * 32 * 8 and not res.converged
    assert 0.0 < dev_a and 0.0 < dev_b and got_a <= 8 * dev_a and got_b <= 8 * dev_b
    kept = A.lanczos(op, psi, 12, reorthogonalize="none")
    assert np.array_equal(kept.alphas, res.alphas) and np.array_equal(kept.betas, res.betas) and len(kept.basis) == 12


def stream_calls(vs, w, psi, device):
    """Every wrapper and both drivers on the current stream, results as host values (device=True: read by the caller later)."""
    terms = dense_case("ising")[0]
    out = {}
    out["dots"] = A.krylov_dots(vs[:2 * B + 1], w, device=device)
    y = torch.empty_like(w)
    out["combine"] = A.krylov_combine_(y, np.linspace(-1.0, 1.0, 17) + 0.25j, vs[:17], device=device)
    out["y"] = y
    out["norm2"] = A.norm2(w, device=device)
    if not device:
        tol = 1e-4 * dense_case("ising")[3]
        e0, state, info = A.lanczos_ground_state(psi, terms, max_iter=100, tol=tol)
        out["ground"] = (e0, state, info.iterations, info.alphas, info.betas[0])
        out["evolve"] = A.krylov_evolve(psi, terms, 0.5, m=20)
    return out


def as_bits(out):
    """The results of stream_calls as lists of integer arrays."""
    f = lambda x: np.atleast_1d(np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x, dtype=np.float64)).view(np.uint64)
    got = [f(out["dots"][0]) if isinstance(out["dots"][0], torch.Tensor) else out["dots"][0].view(np.uint64), f(out["dots"][1]),
           f(out["combine"]), bits(out["y"]), f(out["norm2"])]
    if "ground" in out:
        e0, state, k, alphas, betas = out["ground"]
        got += [f(e0), bits(state), f(k), f(alphas), f(betas), bits(out["evolve"][0]), f(out["evolve"][1])]
    return got


@pytest.mark.parametrize("device", [False, True], ids=["host results", "device results"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_every_call_on_a_side_stream(dtype, device):
    """A stream only orders work, so each call made on a side stream right behind the torch ops that produce its inputs, with no
    synchronisation in between, must give bit for bit what the same call gives afterwards on the default stream.  A launch or a
    workspace on another stream than the current one would read vectors that are still being written."""
    n = 2 ** 21 + 1031
    real = torch.float32 if dtype == torch.complex64 else torch.float64
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        g = torch.Generator(device=DEV).manual_seed(7)
        vs = [torch.view_as_complex(torch.randn(n, 2, dtype=real, device=DEV, generator=g)) for _ in range(2 * B + 1)]
        w = torch.view_as_complex(torch.randn(n, 2, dtype=real, device=DEV, generator=g))
        for v in vs:                                           # w is the last thing the stream finishes
            w = w + 0.125 * v
        psi = torch.view_as_complex(torch.randn((2,) * 10 + (2,), dtype=real, device=DEV, generator=g)) + 0.5 * w[:1024].reshape((2,) * 10)
        assert N.current_stream_ptr(w.device).value == side.cuda_stream
        first = stream_calls(vs, w, psi, device)
        side.synchronize()
        first = as_bits(first)
    torch.cuda.synchronize()
    assert N.current_stream_ptr(w.device).value in (None, 0, torch.cuda.default_stream().cuda_stream)
    again = stream_calls(vs, w, psi, device)
    torch.cuda.synchronize()
    again = as_bits(again)
    assert len(first) == len(again)
    for k, (a, b) in enumerate(zip(first, again)):
        assert np.array_equal(a, b), k
    assert np.isfinite(first[0].view(np.float64)).all() and first[4].view(np.float64)[0] > 0.0
