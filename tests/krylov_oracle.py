"""Numpy restatements for the Krylov tests (imported by test_krylov_cpu.py and test_krylov_gpu.py; nothing here comes from the
package): chain Hamiltonians as term lists and as dense np.kron matrices, and the Lanczos recurrence of artensor_amd/krylov.py
written again on dense arrays, with a switch that rounds every STORED vector to the dtype the device run stores it in."""
import math

import numpy as np

PAULI = {"I": np.eye(2, dtype=np.complex128), "X": np.array([[0, 1], [1, 0]], dtype=np.complex128),
         "Y": np.array([[0, -1j], [1j, 0]], dtype=np.complex128), "Z": np.array([[1, 0], [0, -1]], dtype=np.complex128)}
BREAKDOWN = 2.0 ** -40


def _string(nq, ops):
    s = ["I"] * nq
    for q, c in ops.items():
        s[q] = c
    return "".join(s)


def ising_terms(nq, j=1.0, h=1.0, g=0.0):
    """Open transverse-field Ising chain -j sum Z Z - h sum X (- g sum Z: a longitudinal field that makes the spectrum distinct)."""
    terms = [(-j, _string(nq, {q: "Z", q + 1: "Z"})) for q in range(nq - 1)]
    terms += [(-h, _string(nq, {q: "X"})) for q in range(nq)]
    if g:
        terms += [(-g * (1.0 + 0.1 * q), _string(nq, {q: "Z"})) for q in range(nq)]
    return terms


def heisenberg_terms(nq, j=1.0, hs=0.0):
    """Open antiferromagnetic Heisenberg chain j sum (XX + YY + ZZ) + hs sum (-1)^q Z (a staggered field)."""
    terms = [(j, _string(nq, {q: c, q + 1: c})) for q in range(nq - 1) for c in "XYZ"]
    if hs:
        terms += [(hs * (-1) ** q, _string(nq, {q: "Z"})) for q in range(nq)]
    return terms


def dense_hamiltonian(terms, nq):
    """sum c_k P_k as a 2^nq x 2^nq matrix; character d of a string acts on dim d of a [2] * nq tensor (np.kron order)."""
    h = np.zeros((2 ** nq, 2 ** nq), dtype=np.complex128)
    for c, s in terms:
        m = np.ones((1, 1), dtype=np.complex128)
        for ch in s:
            m = np.kron(m, PAULI[ch])
        h += c * m
    return h


def tridiagonal(alphas, betas):
    return np.diag(np.asarray(alphas, dtype=float)) + np.diag(np.asarray(betas, dtype=float), 1) + np.diag(np.asarray(betas, dtype=float), -1)


def lanczos_numpy(h, v0, m, reorthogonalize="full", tol=None, store=None):
    """The recurrence on a dense matrix `h` in complex128.  store=np.complex64 rounds every vector the device run stores in
    that dtype (the normalised start, each op(v), each orthogonalised w, each scaled v).  `h` may be a callable v -> h v.  Returns a
    dict: alphas [k], betas [k - 1], beta_last, basis [n, k], converged, breakdown, residual, iterations, norm0, and per step
    first_sweep [k] = |w after the first sweep|^2 / |op(v)|^2 (a second sweep ran where it is below 0.25; "full" only), and
    breakdown_ratio = beta / (2^-40 scale) of the last step taken (inf where scale is 0 and beta is not)."""
    rnd = (lambda x: x.astype(store).astype(np.complex128)) if store is not None else (lambda x: x)
    v0 = np.asarray(v0, dtype=np.complex128).reshape(-1)
    norm0 = math.sqrt(np.vdot(v0, v0).real)
    v = rnd(v0 * (1.0 / norm0))
    basis, alphas, betas = [v], [], []
    beta_last, scale, residual, converged, breakdown, first_sweep, ratio = 0.0, 0.0, None, False, False, [], None
    apply = h if callable(h) else (lambda x: h @ x)
    for j in range(m):
        w = rnd(apply(v))
        nw = np.vdot(w, w).real
        if reorthogonalize == "full":
            vm = np.stack(basis, axis=1)
            hh = vm.conj().T @ w
            alpha = hh[j].real
            w = rnd(w - vm @ hh)
            first_sweep.append(np.vdot(w, w).real / nw if nw else 0.0)
            if np.vdot(w, w).real < 0.25 * nw:
                hh = vm.conj().T @ w
                alpha += hh[j].real
                w = rnd(w - vm @ hh)
        else:
            alpha = np.vdot(v, w).real
            w = w - alpha * v
            if j:
                w = w - betas[-1] * basis[-2]
            w = rnd(w)
        alphas.append(alpha)
        beta = math.sqrt(np.vdot(w, w).real)
        if j == 0:
            scale = math.sqrt(nw)
        ratio = beta / (BREAKDOWN * scale) if scale else (math.inf if beta else 0.0)
        if beta <= BREAKDOWN * scale:
            converged, breakdown, beta_last, residual = True, True, 0.0, 0.0
            break
        scale = max(scale, beta)
        beta_last = beta
        if tol is not None:
            _, s = np.linalg.eigh(tridiagonal(alphas, betas))
            residual = abs(beta * s[-1, 0])
            if residual < tol:
                converged = True
                break
        if j == m - 1:
            break
        betas.append(beta)
        v = rnd(w * (1.0 / beta))
        basis.append(v)
    return {"alphas": np.array(alphas), "betas": np.array(betas), "beta_last": beta_last, "basis": np.stack(basis, axis=1),
            "converged": converged, "breakdown": breakdown, "residual": residual, "iterations": len(alphas), "norm0": norm0,
            "first_sweep": np.array(first_sweep), "breakdown_ratio": ratio}


def ground_state_numpy(h, v0, max_iter, tol, reorthogonalize="full", store=None, max_vecs=64):
    """lanczos_ground_state of artensor_amd/krylov.py on dense arrays: runs of at most max_vecs steps, each followed by the Ritz
    vector basis[:, :k] @ s[:, 0] of its lowest Ritz pair, rounded to `store`; the next run starts from that vector unless the run
    converged or max_iter steps are done.  Returns (E0, state, iterations, restarts, runs, last): runs the step count of every
    run, last the dict of the last one."""
    rnd = (lambda x: x.astype(store).astype(np.complex128)) if store is not None else (lambda x: x)
    x, done, restarts, runs = np.asarray(v0, dtype=np.complex128).reshape(-1), 0, 0, []
    while True:
        r = lanczos_numpy(h, x, min(max_vecs, max_iter - done), reorthogonalize, tol=tol, store=store)
        k = r["iterations"]
        theta, s = np.linalg.eigh(tridiagonal(r["alphas"], r["betas"]))
        state = rnd(r["basis"][:, :k] @ s[:, 0])
        done += k
        runs.append(k)
        if r["converged"] or done >= max_iter:
            return float(theta[0]), state, done, restarts, runs, r
        x, restarts = state, restarts + 1


def evolve_numpy(h, v0, t, m, store=None):
    """exp(-i t h) v0 from the m-step Krylov space of the restatement, and the a-posteriori estimate."""
    r = lanczos_numpy(h, v0, m, "full", store=store)
    theta, s = np.linalg.eigh(tridiagonal(r["alphas"], r["betas"]))
    c = s @ (np.exp(-1j * t * theta) * s[0, :])
    return r["basis"] @ (r["norm0"] * c), r["norm0"] * r["beta_last"] * abs(c[-1])


def expm_exact(h, v0, t):
    lam, u = np.linalg.eigh(h)
    return u @ (np.exp(-1j * t * lam) * (u.conj().T @ np.asarray(v0, dtype=np.complex128).reshape(-1)))
