"""Host-side checks of the Krylov vector algebra and drivers (artensor_amd/krylov.py; artn_krylov_query / _dots / _combine): the
symbols and constants, the query's arithmetic, every refusal with its code, the host-only tridiagonal mathematics against dense
numpy, and the numpy restatement of the recurrence (tests/krylov_oracle.py, the oracle of test_krylov_gpu.py) against eigvalsh.
No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import krylov

import krylov_oracle as KO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = N.KRYLOV_BATCH


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_krylov_query", "artn_krylov_dots", "artn_krylov_combine"]
    assert N.ABI_VERSION == 9 and N.lib().artn_abi_version() == 9
    raw = open(os.path.join(ROOT, "include", "artn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    consts = dict(re.findall(r"#define (ARTN_KRYLOV_[A-Z_]+) (\d+)", text))
    assert int(consts["ARTN_KRYLOV_BATCH"]) == B and 2 <= B <= 16
    assert int(consts["ARTN_KRYLOV_MAX_VECS"]) == N.KRYLOV_MAX_VECS == 64
    assert re.search(r"#define ARTN_ABI_VERSION 9\b", text)
    assert ctypes.sizeof(N.ArtnKrylovInfo) == 4 * 4 + 5 * 8
    for name in ("krylov_dots", "krylov_combine_", "krylov_info", "lanczos", "lanczos_ground_state", "krylov_evolve"):
        assert getattr(A, name) is getattr(krylov, name)


def query(n, dtype, m):
    info = N.ArtnKrylovInfo()
    return N.lib().artn_krylov_query(n, dtype, m, ctypes.byref(info)), info


def test_query_properties_over_random_sizes():
    rng = np.random.default_rng(16)
    cases = [(1, 1), (4, B), (1023, B + 1), (2 ** 21 + 1031, 2 * B + 1), (2 ** 40, 64), (2 ** 30, 32)]
    cases += [(int(2 ** rng.uniform(0, 40)), int(rng.integers(1, 200))) for _ in range(200)]
    for n, m in cases:
        for dtype, elem in ((N.ARTN_C64, 8), (N.ARTN_C128, 16)):
            rc, i = query(n, dtype, m)
            assert rc == 0, (n, m)
            plan = A.born.born_plan(n, torch.complex64 if dtype == N.ARTN_C64 else torch.complex128)
            assert i.grid == plan["overlap_grid"] == min(-(-n // 1024), 2048)       # the grid of artn_born_overlap
            assert i.batch == B
            assert i.dots_launches == -(-m // B) and i.combine_launches == 1
            assert i.dots_workspace_bytes == 32 * i.grid * (-(-m // 2) + 1)
            assert i.combine_workspace_bytes == 8 * i.grid
            assert i.dots_bytes_read == (m + -(-m // B)) * n * elem
            assert i.combine_bytes_read == m * n * elem and i.combine_bytes_written == n * elem
    info = A.krylov_info((2,) * 12, [2 ** p for p in (3, 0, 11, 7, 1, 9, 2, 10, 4, 8, 6, 5)], 2 * B + 1, torch.complex128)
    assert info["n"] == 4096 and info["grid"] == 4 and info["dots_launches"] == 3 and info["batch"] == B


def test_query_refusals():
    err = N.lib().artn_last_error
    assert query(0, N.ARTN_C64, 1)[0] == -1 and b"element count" in err()
    assert query(2 ** 40 + 1, N.ARTN_C64, 1)[0] == -1 and b"element count" in err()
    assert query(16, N.ARTN_C64, 0)[0] == -1 and b"at least one" in err()
    assert query(16, N.ARTN_C64, -3)[0] == -1
    assert query(16, N.ARTN_C64_BF16, 1)[0] == -2 and b"complex" in err()
    assert query(16, 7, 1)[0] == -2
    assert N.lib().artn_krylov_query(16, N.ARTN_C64, 1, None) == -1 and b"null" in err()
    with pytest.raises(ValueError, match="dense"):
        A.krylov_info((2, 2), (4, 1), 3)
    with pytest.raises(RuntimeError, match="at least one"):
        A.krylov_info((2, 2), (2, 1), 0)
    with pytest.raises(TypeError, match="complex"):
        A.krylov_info((2, 2), (2, 1), 3, dtype=torch.float32)


def _bufs():
    buf = np.zeros(4096, dtype=np.complex128)
    base = (buf.ctypes.data + 15) & ~15
    return buf, base


def dots_rc(vecs, w, n=4, dtype=N.ARTN_C64, ws=None, ws_bytes=1 << 20, out=None, m=None, table=True):
    tab = (ctypes.c_void_p * max(len(vecs), 1))(*vecs) if table else None
    return N.lib().artn_krylov_dots(tab, len(vecs) if m is None else m, ctypes.c_void_p(w), n, dtype, ctypes.c_void_p(ws),
                                    ws_bytes, ctypes.c_void_p(out), None)


def combine_rc(y, coeff, xs, n=4, dtype=N.ARTN_C64, ws=None, ws_bytes=1 << 20, out=None, m=None, table=True, have_coeff=True):
    tab = (ctypes.c_void_p * max(len(xs), 1))(*xs) if table else None
    c = np.ascontiguousarray(np.asarray(coeff, dtype=np.complex128))
    return N.lib().artn_krylov_combine(ctypes.c_void_p(y), c.ctypes.data_as(ctypes.c_void_p) if have_coeff else None, tab,
                                       len(xs) if m is None else m, n, dtype, ctypes.c_void_p(ws), ws_bytes, ctypes.c_void_p(out),
                                       None)


def test_dots_and_combine_refuse_bad_arguments_and_run_nowhere_without_a_gpu():
    """Every call here is refused before anything is launched, so host addresses are safe to pass.  n = 4 complex64 elements are
    32 bytes; one workgroup: 64 bytes of workspace for a dots of one vector, 8 for a combine."""
    err = N.lib().artn_last_error
    buf, base = _bufs()
    w, ws, out = base, base + 4096, base + 8192
    v = [base + 256 * (j + 1) for j in range(8)]
    many = [base + 16384 + 32 * j for j in range(65)]
    one = [1.0]
    cases = {
        "dots: null w": (lambda: dots_rc(v[:2], 0, ws=ws, out=out), -1, b"null"),
        "dots: null table": (lambda: dots_rc([], w, ws=ws, out=out, m=2, table=False), -1, b"null"),
        "dots: null vector": (lambda: dots_rc([v[0], 0], w, ws=ws, out=out), -1, b"null"),
        "dots: null workspace": (lambda: dots_rc(v[:2], w, ws=0, out=out), -1, b"null"),
        "dots: null out": (lambda: dots_rc(v[:2], w, ws=ws, out=0), -1, b"null"),
        "dots: m = 0": (lambda: dots_rc([], w, ws=ws, out=out), -1, b"at least one"),
        "dots: small workspace": (lambda: dots_rc(v[:2], w, ws=ws, ws_bytes=63, out=out), -1, b"workspace"),
        "dots: dtype": (lambda: dots_rc(v[:2], w, dtype=N.ARTN_C64_BF16, ws=ws, out=out), -2, b"complex"),
        "dots: misaligned w": (lambda: dots_rc(v[:2], w + 8, ws=ws, out=out), -2, b"16-byte"),
        "dots: misaligned vector": (lambda: dots_rc([v[0], v[1] + 8], w, ws=ws, out=out), -2, b"16-byte"),
        "combine: null y": (lambda: combine_rc(0, one, v[:1], ws=ws, out=out), -1, b"null"),
        "combine: null coefficients": (lambda: combine_rc(w, one, v[:1], ws=ws, out=out, have_coeff=False), -1, b"null"),
        "combine: null table": (lambda: combine_rc(w, one, [], ws=ws, out=out, m=1, table=False), -1, b"null"),
        "combine: null vector": (lambda: combine_rc(w, [1.0, 1.0], [v[0], 0], ws=ws, out=out), -1, b"null"),
        "combine: null workspace": (lambda: combine_rc(w, one, v[:1], ws=0, out=out), -1, b"null"),
        "combine: null out": (lambda: combine_rc(w, one, v[:1], ws=ws, out=0), -1, b"null"),
        "combine: m = 0": (lambda: combine_rc(w, [], [], ws=ws, out=out), -1, b"at least one"),
        "combine: m = 65": (lambda: combine_rc(w, [1.0] * 65, many, ws=ws, out=out), -1, b"at most 64"),
        "combine: small workspace": (lambda: combine_rc(w, one, v[:1], ws=ws, ws_bytes=7, out=out), -1, b"workspace"),
        "combine: dtype": (lambda: combine_rc(w, one, v[:1], dtype=5, ws=ws, out=out), -2, b"complex"),
        "combine: misaligned y": (lambda: combine_rc(w + 8, one, v[:1], ws=ws, out=out), -2, b"16-byte"),
        "combine: misaligned vector": (lambda: combine_rc(w, one, [v[0] + 8], ws=ws, out=out), -2, b"16-byte"),
        "combine: y overlaps the end of a vector": (lambda: combine_rc(v[0] + 16, [1.0, 2.0], [v[1], v[0]], ws=ws, out=out), -1, b"overlaps"),
        "combine: a vector overlaps the end of y": (lambda: combine_rc(v[0], [1.0, 2.0], [v[0], v[0] + 16], ws=ws, out=out), -1, b"overlaps"),
        "combine: overlap under a zero coefficient": (lambda: combine_rc(v[0], [1.0, 0.0], [v[1], v[0] + 16], ws=ws, out=out), -1, b"overlaps"),
        "combine: nan coefficient": (lambda: combine_rc(w, [1.0, float("nan")], v[:2], ws=ws, out=out), -1, b"finite"),
        "combine: infinite coefficient": (lambda: combine_rc(w, [1.0, complex(0.0, float("inf"))], v[:2], ws=ws, out=out), -1, b"finite"),
    }
    for name, (call, want, text) in cases.items():
        rc = call()
        if torch.cuda.is_available():
            assert rc == want and text in err(), (name, rc, err())
        else:
            assert rc == -4 and b"no gfx950 device" in err(), name
    del buf


def test_there_is_no_cpu_fallback():
    a = torch.zeros(2, 2, dtype=torch.complex64)
    terms = [(1.0, "ZZ"), (0.5, "XI")]
    for call in (lambda: A.krylov_dots([a], a), lambda: A.krylov_combine_(a, [1.0], [a]),
                 lambda: A.lanczos(lambda x, out: out, a, 2), lambda: A.lanczos_ground_state(a, terms),
                 lambda: A.krylov_evolve(a, terms, 0.1)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_ritz_pairs_and_the_exponential_against_dense_numpy():
    rng = np.random.default_rng(5)
    for k in (1, 2, 7, 40):
        alphas, betas = rng.standard_normal(k), np.abs(rng.standard_normal(k - 1)) + 0.1
        t_mat = KO.tridiagonal(alphas, betas)
        theta, s = krylov.ritz(alphas, betas)
        scale = np.abs(t_mat).sum(axis=1).max()
        assert np.all(np.diff(theta) >= 0)
        assert np.abs(theta - np.linalg.eigvalsh(t_mat)).max() <= 64 * k * 2.0 ** -53 * scale
        assert np.abs(t_mat @ s - s * theta).max() <= 64 * k * 2.0 ** -53 * scale        # Ritz vectors: T s = theta s
        assert np.abs(s.T @ s - np.eye(k)).max() <= 64 * k * 2.0 ** -53
        for t in (0.0, 0.3, -2.5):
            got = krylov.expm_e1(alphas, betas, t)
            # a reference that shares nothing with eigh: the Taylor series of exp(-i t T / 2^s) e_1, squared s times as a matrix
            sq = max(0, int(np.ceil(np.log2(max(abs(t) * scale, 1e-300)))) + 1)
            small = -1j * t * t_mat / 2.0 ** sq
            term, acc = np.eye(k, dtype=np.complex128), np.eye(k, dtype=np.complex128)
            for p in range(1, 30):
                term = term @ small / p
                acc = acc + term
            for _ in range(sq):
                acc = acc @ acc
            err = np.abs(got - acc[:, 0]).max()
            print(f"k {k}, t {t}: err {err:.2e}")
            assert err <= 256 * k * 2.0 ** -53 * (1 + abs(t) * scale)
            assert abs(np.linalg.norm(got) - 1.0) <= 64 * k * 2.0 ** -53
    with pytest.raises(ValueError, match="off-diagonal"):
        krylov.ritz([1.0, 2.0], [0.1, 0.2])


@pytest.mark.parametrize("store", [None, np.complex64], ids=["complex128", "rounded to complex64"])
def test_the_numpy_restatement_of_the_recurrence_against_eigvalsh(store):
    """The oracle of the GPU tests, checked on its own: a complete run (64 steps on 64 states, full re-orthogonalisation) gives
    the spectrum, a short run with tol gives the ground state to the Hermitian residual bound, and without re-orthogonalisation
    the extreme Ritz values still converge."""
    p = 53 if store is None else 24
    terms = KO.ising_terms(6, 1.0, 0.9, 0.35)
    h = KO.dense_hamiltonian(terms, 6)
    assert np.abs(h - h.conj().T).max() == 0.0
    lam = np.linalg.eigvalsh(h)
    c = sum(abs(x) for x, _ in terms)
    rng = np.random.default_rng(64)
    v0 = rng.standard_normal(64) + 1j * rng.standard_normal(64)
    if store is not None:
        v0 = v0.astype(store)
    r = KO.lanczos_numpy(h, v0, 64, "full", store=store)
    assert r["iterations"] == 64 and r["basis"].shape == (64, 64)
    theta = np.linalg.eigvalsh(KO.tridiagonal(r["alphas"], r["betas"]))
    assert np.abs(theta - lam).max() <= 64 * 64 * 2.0 ** -p * c
    v = r["basis"]
    assert np.abs(v.conj().T @ v - np.eye(64)).max() <= 64 * 64 * 2.0 ** -p
    # the ground state with a tolerance, on 10 qubits
    terms = KO.ising_terms(10, 1.0, 1.5)
    h = KO.dense_hamiltonian(terms, 10)
    lam = np.linalg.eigvalsh(h)
    c = sum(abs(x) for x, _ in terms)
    v0 = rng.standard_normal(1024) + 1j * rng.standard_normal(1024)
    tol = (1e-9 if store is None else 1e-4) * c
    r = KO.lanczos_numpy(h, v0, 100, "full", tol=tol, store=store)
    assert r["converged"] and r["iterations"] <= 100 and r["residual"] < tol
    theta, s = np.linalg.eigh(KO.tridiagonal(r["alphas"], r["betas"]))
    x = r["basis"] @ s[:, 0]
    x /= np.linalg.norm(x)
    res = np.linalg.norm(h @ x - theta[0] * x)
    assert res <= tol + 64 * r["iterations"] * 2.0 ** -p * c
    assert abs(theta[0] - lam[0]) <= res and abs(theta[0] - lam[0]) < abs(theta[0] - lam[1])
    # the plain three-term recurrence: the extremes converge without re-orthogonalisation
    r = KO.lanczos_numpy(h, v0, 100, "none", store=store)
    theta = np.linalg.eigvalsh(KO.tridiagonal(r["alphas"], r["betas"]))
    assert abs(theta[0] - lam[0]) <= 1e-4 * c and abs(theta[-1] - lam[-1]) <= 1e-4 * c
    # exp(-i t H) v from the complete space is exact to rounding
    h6 = KO.dense_hamiltonian(KO.ising_terms(6, 1.0, 0.9, 0.35), 6)
    c6 = sum(abs(x) for x, _ in KO.ising_terms(6, 1.0, 0.9, 0.35))
    v6 = (rng.standard_normal(64) + 1j * rng.standard_normal(64))
    if store is not None:
        v6 = v6.astype(store).astype(np.complex128)
    out, est = KO.evolve_numpy(h6, v6, 2.0 / c6, 64, store=store)
    assert np.linalg.norm(out - KO.expm_exact(h6, v6, 2.0 / c6)) <= 64 * 64 * 2.0 ** -p * 3.0 * np.linalg.norm(v6)


RESTART_CASES = [(np.complex64, 70, [64, 6], False), (np.complex64, 130, [64, 64, 2], False), (None, 70, [64, 1], True)]


@pytest.mark.parametrize("store,max_iter,runs,converged", RESTART_CASES, ids=["c64-70", "c64-130", "c128-70"])
def test_the_restatement_of_the_restarted_ground_state_against_eigvalsh(store, max_iter, runs, converged):
    """ground_state_numpy, the oracle of the restart tests of test_krylov_drivers_gpu.py, on their input: the 10-qubit Ising
    chain at h = 1.5 with tol = 0, so that only a breakdown ends a run early.  With complex64 storage 70 steps are runs of 64 and
    6 and 130 steps runs of 64, 64 and 2; in complex128 the restart vector is an eigenvector to rounding and the second run breaks
    down at its first step.  The margin of that breakdown is printed: beta / (2^-40 scale) of the last step, measured 2.5e-3."""
    p = 53 if store is None else 24
    terms = KO.ising_terms(10, 1.0, 1.5)
    h = KO.dense_hamiltonian(terms, 10)
    lam = np.linalg.eigvalsh(h)
    c = sum(abs(x) for x, _ in terms)
    rng = np.random.default_rng(10)                               # start_vector(10, dtype, 10) of the GPU tests
    v0 = (rng.standard_normal(1024) + 1j * rng.standard_normal(1024)).astype(np.complex128 if store is None else store)
    e0, state, done, restarts, got_runs, last = KO.ground_state_numpy(h, v0, max_iter, 0.0, "full", store=store)
    x = state / np.linalg.norm(state)
    res = np.linalg.norm(h @ x - e0 * x)
    print(f"{'complex128' if store is None else 'complex64'} max_iter {max_iter}: runs {got_runs}, E0 - lambda_0 {e0 - lam[0]:.3e}, |r| {res:.3e}, "
          f"last beta / (2^-40 scale) {last['breakdown_ratio']:.3e}")
    assert got_runs == runs and done == sum(runs) and restarts == len(runs) - 1
    assert last["converged"] == converged == last["breakdown"] and last["iterations"] == runs[-1]
    assert res <= 64 * max_iter * 2.0 ** -p * c and abs(e0 - lam[0]) <= 64 * max_iter * 2.0 ** -p * c
    assert abs(e0 - lam[0]) < abs(e0 - lam[1])
    if store is not None:                                         # (in complex128 both sides are rounding of eigvalsh and of h @ x)
        assert abs(e0 - lam[0]) <= res
    if converged:
        assert last["breakdown_ratio"] <= 1.0 and last["residual"] == 0.0 == last["beta_last"]
    # one run is lanczos_numpy itself, and max_vecs cuts the runs
    one = KO.lanczos_numpy(h, v0, 40, "full", tol=0.0, store=store)
    e1, _, done1, restarts1, runs1, last1 = KO.ground_state_numpy(h, v0, 40, 0.0, "full", store=store)
    assert runs1 == [40] and restarts1 == 0 and done1 == 40 and np.array_equal(one["alphas"], last1["alphas"])
    assert e1 == np.linalg.eigh(KO.tridiagonal(one["alphas"], one["betas"]))[0][0]
    assert KO.ground_state_numpy(h, v0, 40, 0.0, "full", store=store, max_vecs=16)[4] == [16, 16, 8]
