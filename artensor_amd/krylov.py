"""Krylov drivers on the device: the two fused streaming passes such a driver is made of (C ABI: artn_krylov_query,
artn_krylov_dots, artn_krylov_combine) and two small drivers on top of them -- Lanczos for extremal eigenpairs of a Hermitian
operator and exp(-i t H)|psi> from the same recurrence.

    krylov_dots(vectors, w)             <V_j|w> for every j and |w|^2: w is read once per ARTN_KRYLOV_BATCH vectors, each V_j once
    krylov_combine_(y, coeffs, vectors) y <- sum_j c_j X_j in one launch (at most 64 vectors), returns |y|^2 of the stored values

Every vector of a call is a dense GPU tensor of complex64 or complex128 (what born.py takes) and all of them share dtype, shape,
strides and device; nothing is ever copied.  Arithmetic is float64 in a fixed order: each dot is bit for bit what
`overlap(V_j, w)` returns, the reported norm is bit for bit `norm2(y)` of the result, and both are bit-identical from run to run.

The operator of the drivers is a `PauliSumOperator` or any callable `op(amps, out) -> out` on tensors of one layout, so the
drivers do not depend on the Pauli code; `lanczos_ground_state` and `krylov_evolve` take `terms = [(c_k, string_k), ...]` with
REAL coefficients and build the operator once.  The small tridiagonal problem is solved on the host (numpy.linalg.eigh).  There is
no CPU fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import _native
from ._state import _DTYPES, _checked, _dense_layout, _dtype_code
from .born import norm2

__all__ = ["krylov_info", "krylov_dots", "krylov_combine_", "ritz", "expm_e1", "KrylovResult", "lanczos", "lanczos_ground_state",
           "krylov_evolve"]

BATCH = _native.KRYLOV_BATCH
MAX_VECS = _native.KRYLOV_MAX_VECS
_BREAKDOWN = 2.0 ** -40


def _info(n, dtype, m):
    info = _native.ArtnKrylovInfo()
    _native.check(_native.lib().artn_krylov_query(int(n), _DTYPES[dtype], int(m), ctypes.byref(info)))
    return info


def krylov_info(shape, strides, m, dtype=torch.complex64):
    """Host-only: what krylov_dots and krylov_combine_ do for m vectors of this layout -- the grid, the batch B, the streaming
    launches of each (a finish launch follows), the workspaces and the nominal bytes moved (ValueError for a layout that is not
    dense, RuntimeError where the library refuses, TypeError for a dtype that is not complex)."""
    _dtype_code(dtype, "krylov_info")
    n = _dense_layout(shape, strides)
    i = _info(n, dtype, m)
    return {"n": n, "grid": i.grid, "batch": i.batch, "dots_launches": i.dots_launches, "combine_launches": i.combine_launches,
            "dots_workspace_bytes": i.dots_workspace_bytes, "combine_workspace_bytes": i.combine_workspace_bytes,
            "dots_bytes_read": i.dots_bytes_read, "combine_bytes_read": i.combine_bytes_read,
            "combine_bytes_written": i.combine_bytes_written}


def _same_layout(vectors, ref, what):
    """The vectors as a list and the element count, after checking that each is what born.py takes and lies like `ref`."""
    n = _checked(ref, what)
    vectors = list(vectors)
    if not vectors:
        raise ValueError(f"{what}: at least one vector is needed")
    for v in vectors:
        if v is ref:
            continue
        _checked(v, what)
        if v.dtype != ref.dtype or v.device != ref.device:
            raise ValueError(f"{what}: every vector must share dtype and device")
        if tuple(v.shape) != tuple(ref.shape) or tuple(v.stride()) != tuple(ref.stride()):
            raise ValueError(f"{what}: every vector must have equal shapes and equal strides (got {tuple(v.shape)}/{tuple(v.stride())} "
                             f"and {tuple(ref.shape)}/{tuple(ref.stride())})")
    return vectors, n


def _table(vectors):
    return (ctypes.c_void_p * len(vectors))(*[v.data_ptr() for v in vectors])


def krylov_dots(vectors, w, device=False):
    """(dots, |w|^2): dots[j] = <V_j|w> (conjugate-linear in V_j) as a complex128 numpy array [m] and a float.  device=True: a
    float64 GPU tensor [m, 2] (real and imaginary parts) and a 0-dim one, without a host synchronisation."""
    what = "krylov.krylov_dots"
    vectors, n = _same_layout(vectors, w, what)
    m = len(vectors)
    info = _info(n, w.dtype, m)
    ws = torch.empty(info.dots_workspace_bytes // 8, dtype=torch.float64, device=w.device)
    out = torch.empty(2 * m + 1, dtype=torch.float64, device=w.device)
    with torch.cuda.device(w.device):
        _native.check(_native.lib().artn_krylov_dots(_table(vectors), m, w.data_ptr(), n, _DTYPES[w.dtype], ws.data_ptr(),
                                                     info.dots_workspace_bytes, out.data_ptr(),
                                                     _native.current_stream_ptr(w.device)))
    if device:
        return out[:2 * m].view(m, 2), out[2 * m]
    host = out.cpu().numpy()
    return host[:2 * m].view(np.complex128).copy(), float(host[2 * m])


def krylov_combine_(y, coeffs, vectors, device=False):
    """y <- sum_j coeffs[j] * vectors[j] in one launch and |y|^2 of what was stored (a float; device=True: a 0-dim float64 GPU
    tensor, no host synchronisation).  y may be one of the vectors; a y that overlaps one without being it is refused.  At most
    64 vectors; a coefficient that is exactly 0 skips its vector altogether."""
    what = "krylov.krylov_combine_"
    vectors, n = _same_layout(vectors, y, what)
    m = len(vectors)
    c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.complex128).reshape(-1))
    if c.size != m:
        raise ValueError(f"{what}: {c.size} coefficients for {m} vectors")
    info = _info(n, y.dtype, m)
    ws = torch.empty(max(info.combine_workspace_bytes // 8, 1), dtype=torch.float64, device=y.device)
    out = torch.empty(4, dtype=torch.float64, device=y.device)
    with torch.cuda.device(y.device):
        _native.check(_native.lib().artn_krylov_combine(y.data_ptr(), c.ctypes.data_as(ctypes.c_void_p), _table(vectors), m, n,
                                                        _DTYPES[y.dtype], ws.data_ptr(), info.combine_workspace_bytes,
                                                        out.data_ptr(), _native.current_stream_ptr(y.device)))
    return out[0] if device else float(out[0])


# ---- the host half: the tridiagonal problem --------------------------------------------------------------------------------
def _tridiagonal(alphas, betas):
    a, b = np.asarray(alphas, dtype=np.float64), np.asarray(betas, dtype=np.float64)
    if a.ndim != 1 or a.size < 1 or b.shape != (a.size - 1,):
        raise ValueError(f"a tridiagonal of {a.size} diagonal entries takes {max(a.size - 1, 0)} off-diagonal ones, got {b.size}")
    return np.diag(a) + np.diag(b, 1) + np.diag(b, -1)


def ritz(alphas, betas):
    """(theta, S): eigenvalues (ascending) and orthonormal eigenvectors (columns) of the real symmetric tridiagonal matrix with
    diagonal `alphas` [k] and off-diagonal `betas` [k - 1].  Host-only."""
    return np.linalg.eigh(_tridiagonal(alphas, betas))


def expm_e1(alphas, betas, t):
    """exp(-i t T) e_1 for that matrix T, from its eigendecomposition: a complex128 array [k].  Host-only."""
    theta, s = ritz(alphas, betas)
    return s @ (np.exp(-1j * float(t) * theta) * s[0, :])


class KrylovResult:
    """What a run did.  alphas [k] and betas [k - 1] are the tridiagonal matrix after k = iterations steps, beta_last the norm of
    the residual vector of the last step (0.0 after a breakdown), ritz_values its eigenvalues, residual the estimate
    |beta_last s_k| for the lowest Ritz pair, basis the k orthonormal vectors (None with keep_basis=False), norm0 the norm of the
    start vector.  passes counts the reads and writes of a state-sized vector that were issued (an operator application as one
    read and one write), peak_bytes the device memory the run held beyond its arguments."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __repr__(self):
        return (f"KrylovResult(iterations={self.iterations}, converged={self.converged}, breakdown={self.breakdown}, "
                f"residual={self.residual}, passes={self.passes}, peak_bytes={self.peak_bytes})")


def _check_basis_size(m, what):
    if m > MAX_VECS:
        raise ValueError(f"{what}: the Ritz vector and the evolved state are ONE combination over the m basis vectors and one launch "
                         f"takes at most {MAX_VECS}, so m + 1 = {m + 1} is too many: m <= {MAX_VECS} (keep_basis=False with "
                         f"reorthogonalize='none' has no limit)")


def lanczos(op, v0, m, reorthogonalize="full", tol=None, keep_basis=True):
    """At most m steps of the Lanczos recurrence of the Hermitian `op` from v0 (never written), with a normalised basis.

    A step is w = op(v_j); one krylov_dots of w against the vectors to remove; one krylov_combine_ with y = w that removes them
    and yields beta_j^2; one krylov_combine_ that scales w into v_{j+1}.  reorthogonalize="full" removes v_0 .. v_j, and again
    when the first sweep left less than half of |w|; "none" removes v_j, and beta_{j-1} v_{j-1} from the recurrence.  alpha_j is
    the real part of <v_j|w>.  The run ends early, converged, at a breakdown (beta_j <= 2^-40 times the largest of the earlier
    betas and |op(v_0)|) and, with `tol`, once |beta_j s_j| of the lowest Ritz pair is below tol.  keep_basis=False (only with
    "none") holds three vectors and returns Ritz values alone.  The threshold 2^-40 is fixed: with "none" and complex64 storage the
    beta of an invariant subspace is rounding of complex64 (about 1e-6), so no breakdown is detected and the run goes on with Ritz
    values off the spectrum; "full" detects it in both dtypes.  Returns a KrylovResult."""
    what = "krylov.lanczos"
    n = _checked(v0, what)
    m = int(m)
    if reorthogonalize not in ("full", "none"):
        raise ValueError(f"{what}: reorthogonalize is 'full' or 'none', got {reorthogonalize!r}")
    if m < 1:
        raise ValueError(f"{what}: at least one step is needed")
    full = reorthogonalize == "full"
    if not keep_basis and full:
        raise ValueError(f"{what}: keep_basis=False goes with reorthogonalize='none' only (full re-orthogonalisation reads the basis)")
    if keep_basis:
        _check_basis_size(m, what)
    nbytes = n * v0.element_size()
    count = {"passes": 0, "vectors": 0}

    def new():
        count["vectors"] += 1
        return torch.empty_strided(tuple(v0.shape), tuple(v0.stride()), dtype=v0.dtype, device=v0.device)

    def dots(vs, w):
        count["passes"] += len(vs) + -(-len(vs) // BATCH)
        return krylov_dots(vs, w)

    def combine(y, c, vs):
        count["passes"] += len(vs) + 1
        return krylov_combine_(y, c, vs)

    def remove(w, h, vs):
        """w <- w - sum_i h_i vs[i] and |w|^2: one launch up to 63 vectors (only the 64th step of a full basis takes two)."""
        for at in range(0, len(vs), MAX_VECS - 1):
            part = slice(at, at + MAX_VECS - 1)
            n2 = combine(w, [1.0] + list(-h[part]), [w] + vs[part])
        return n2

    n0 = norm2(v0)
    count["passes"] += 1
    if not (n0 > 0.0 and math.isfinite(n0)):
        raise ValueError(f"{what}: the start vector has norm^2 {n0}")
    norm0 = math.sqrt(n0)
    v = new()
    combine(v, [1.0 / norm0], [v0])
    basis, v_prev, spare = [v], None, None
    alphas, betas = [], []
    beta_last, scale, residual = 0.0, 0.0, None
    converged = breakdown = False
    for j in range(m):
        w = spare if spare is not None else new()
        spare = None
        got = op(v, w)
        if got is not w:
            raise ValueError(f"{what}: op(amps, out) must write into `out` and return it")
        count["passes"] += 2
        if full:
            h, nw = dots(basis, w)
            alpha = h[j].real
            n2 = remove(w, h, basis)
            if n2 < 0.25 * nw:                              # more than half of |w| went: once more (twice is enough)
                h, _ = dots(basis, w)
                alpha += h[j].real
                n2 = remove(w, h, basis)
        else:
            h, nw = dots([v], w)
            alpha = h[0].real
            if v_prev is None:
                n2 = combine(w, [1.0, -alpha], [w, v])
            else:
                n2 = combine(w, [1.0, -alpha, -betas[-1]], [w, v, v_prev])
        if not (math.isfinite(n2) and math.isfinite(alpha)):
            raise FloatingPointError(f"{what}: step {j} produced alpha {alpha}, beta^2 {n2}")
        alphas.append(alpha)
        beta = math.sqrt(n2)
        if j == 0:
            scale = math.sqrt(nw)
        if beta <= _BREAKDOWN * scale:                      # an invariant subspace: the Ritz pairs are exact
            converged = breakdown = True
            beta_last, residual = 0.0, 0.0
            break
        scale = max(scale, beta)
        beta_last = beta
        if tol is not None:
            _, s = ritz(alphas, betas)
            residual = abs(beta * s[-1, 0])
            if residual < tol:
                converged = True
                break
        if j == m - 1:
            break
        betas.append(beta)
        combine(w, [1.0 / beta], [w])
        if keep_basis:
            basis.append(w)
            v_prev, v = v, w
        else:
            spare, v_prev, v = v_prev, v, w
    theta, s = ritz(alphas, betas)
    if residual is None:
        residual = abs(beta_last * s[-1, 0])
    return KrylovResult(alphas=np.array(alphas), betas=np.array(betas), beta_last=beta_last, iterations=len(alphas),
                        converged=converged, breakdown=breakdown, residual=residual, ritz_values=theta,
                        basis=basis[:len(alphas)] if keep_basis else None, norm0=norm0, passes=count["passes"],
                        peak_bytes=count["vectors"] * nbytes)


def _real_terms(terms, what):
    terms = list(terms)
    if not terms:
        raise ValueError(f"{what}: at least one term is needed")
    if any(complex(c).imag != 0.0 for c, _ in terms):
        raise ValueError(f"{what} takes real coefficients (a Hermitian sum)")
    return terms


def lanczos_ground_state(amps0, terms, max_iter=200, tol=None, reorthogonalize="full"):
    """(E0, state, info): the lowest Ritz value of H = sum_k c_k P_k (real c_k) from the start vector amps0, its normalised Ritz
    vector in the layout of amps0 (ONE krylov_combine_ over the basis) and a KrylovResult.  The run stops once the residual estimate
    is below tol (default: sqrt(eps of the dtype) * sum |c_k|) or after max_iter steps.  A basis holds at most 64 vectors: a run
    that needs more restarts the recurrence from the current Ritz vector (a plain restart; info.restarts counts them).  info.alphas
    is one array over all runs; info.betas is a LIST with one array per run (a restart has no beta that joins two runs)."""
    what = "krylov.lanczos_ground_state"
    _native.require_gpu(amps0, what)
    terms = _real_terms(terms, what)
    n = _checked(amps0, what)
    from .pauli import PauliSumOperator
    op = PauliSumOperator(amps0.shape, amps0.stride(), amps0.dtype, terms, amps0.device)
    if tol is None:
        tol = math.sqrt(torch.finfo(amps0.dtype).eps) * sum(abs(complex(c)) for c, _ in terms)
    max_iter = int(max_iter)
    if max_iter < 1:
        raise ValueError(f"{what}: max_iter must be at least 1")
    nbytes = n * amps0.element_size()
    x, done, passes, peak, restarts = amps0, 0, 0, 0, 0
    alphas, betas = [], []
    while True:
        res = lanczos(op, x, min(MAX_VECS, max_iter - done), reorthogonalize, tol, keep_basis=True)
        theta, s = ritz(res.alphas, res.betas)
        state = torch.empty_strided(tuple(amps0.shape), tuple(amps0.stride()), dtype=amps0.dtype, device=amps0.device)
        krylov_combine_(state, s[:, 0], res.basis)
        done += res.iterations
        passes += res.passes + res.iterations + 1
        peak = max(peak, res.peak_bytes + (1 if x is amps0 else 2) * nbytes)
        alphas.append(res.alphas)
        betas.append(res.betas)
        if res.converged or done >= max_iter:
            break
        x, restarts = state, restarts + 1
        del res
    info = KrylovResult(alphas=np.concatenate(alphas), betas=betas, beta_last=res.beta_last, iterations=done,
                        converged=res.converged, breakdown=res.breakdown, residual=res.residual, ritz_values=theta, basis=None,
                        norm0=res.norm0, passes=passes, peak_bytes=peak, restarts=restarts, tol=tol)
    return float(theta[0]), state, info


def krylov_evolve(amps, terms, t, m=30, out=None):
    """(out, err): exp(-i t H)|amps> for H = sum_k c_k P_k (real c_k) from an m-step Krylov space of amps with full
    re-orthogonalisation -- out = |amps| V exp(-i t T) e_1, ONE krylov_combine_ over the basis -- and the a-posteriori estimate
    err = |amps| beta_m |[exp(-i t T)]_{m,1}| of the error in the 2-norm.  `amps` is not written; out=None allocates the result
    in its layout."""
    what = "krylov.krylov_evolve"
    _native.require_gpu(amps, what)
    terms = _real_terms(terms, what)
    _checked(amps, what)
    m = int(m)
    if m < 1:
        raise ValueError(f"{what}: at least one step is needed")
    _check_basis_size(m, what)
    t = float(t)
    if out is None:
        out = torch.empty_strided(tuple(amps.shape), tuple(amps.stride()), dtype=amps.dtype, device=amps.device)
    elif not isinstance(out, torch.Tensor) or out.dtype != amps.dtype or out.device != amps.device \
            or tuple(out.shape) != tuple(amps.shape) or tuple(out.stride()) != tuple(amps.stride()):
        raise ValueError(f"{what}: out must have the shape, strides, dtype and device of amps")
    from .pauli import PauliSumOperator
    op = PauliSumOperator(amps.shape, amps.stride(), amps.dtype, terms, amps.device)
    res = lanczos(op, amps, m, "full")
    c = expm_e1(res.alphas, res.betas, t)
    krylov_combine_(out, res.norm0 * c, res.basis)
    return out, res.norm0 * res.beta_last * abs(c[-1])
