"""numpy restatement of artensor_amd/measure.py, float64: the oracle of test_measure_cpu.py and test_measure_gpu.py.

Every function takes the state as its LOGICAL array (shape [2] * n or any shape with the measured dims of extent 2); layouts are
the tests' business (their own `permute`).  An outcome is the integer whose most significant digit is the first listed dim."""
import math

import numpy as np


def probabilities(state, dims):
    """q[o] = sum of |state|^2 over every dim not in `dims`, float64, by reshape / sum."""
    dims = [int(d) % state.ndim for d in dims]
    rest = [d for d in range(state.ndim) if d not in dims]
    a = np.transpose(state, dims + rest).reshape(2 ** len(dims), -1).astype(np.complex128)
    return (a.real * a.real + a.imag * a.imag).sum(axis=1)


def choose(q, uniform):
    """The choice rule: the smallest o whose inclusive cumulative sum of q exceeds uniform * total, or the last o with q[o] > 0
    where rounding leaves none; an o with q[o] == 0 is never returned.  -1 where total is not finite or not > 0."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    cum = np.cumsum(q)
    total = float(cum[-1])
    if not (math.isfinite(total) and total > 0.0):
        return -1
    t = float(uniform) * total
    for o in range(q.size):
        if q[o] > 0.0 and cum[o] > t:
            return o
    return int(np.nonzero(q > 0.0)[0][-1])


def mid_uniform(q, o):
    """The uniform number in the middle of outcome o's interval: (cum[o - 1] + q[o] / 2) / total."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    cum = np.cumsum(q)
    return float(((cum[o - 1] if o else 0.0) + q[o] / 2) / cum[-1])


def digits(o, k):
    return [(int(o) >> (k - 1 - j)) & 1 for j in range(k)]


def _index(ndim, dims, values):
    idx = [slice(None)] * ndim
    for d, v in zip(dims, values):
        idx[int(d) % ndim] = v
    return tuple(idx)


def kept_mask(shape, dims, o):
    """Boolean array: True where the measured digits spell o."""
    m = np.zeros(shape, dtype=bool)
    m[_index(len(shape), dims, digits(o, len(dims)))] = True
    return m


def scale_of(q, o, renormalize=True):
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    return float(np.sqrt(np.cumsum(q)[-1] / q[o])) if renormalize else 1.0


def scaled(values, scale):
    """float64(c) * scale per component, rounded once to the dtype of `values`."""
    real = np.float32 if values.dtype == np.complex64 else np.float64
    v = np.ascontiguousarray(values)
    comp = v.view(real).astype(np.float64) * np.float64(scale)
    return comp.astype(real).view(values.dtype).reshape(values.shape)


def collapsed(state, dims, o, scale):
    """Every element whose measured digits differ from o is +0.0, the others float64(c) * scale rounded once (scale == 1: unchanged)."""
    out = np.zeros_like(state)
    at = _index(state.ndim, dims, digits(o, len(dims)))
    out[at] = state[at] if scale == 1.0 else scaled(state[at], scale)
    return out


def reset(state, dims, o, scale):
    """new[r, 0..0] = a[r, o] * scale, +0.0 everywhere else."""
    out = np.zeros_like(state)
    src = _index(state.ndim, dims, digits(o, len(dims)))
    out[_index(state.ndim, dims, [0] * len(dims))] = state[src] if scale == 1.0 else scaled(state[src], scale)
    return out


def rdm(state, dims):
    """rho[i, j] = sum_r a[i, r] conj(a[j, r]) over the listed dims, complex128."""
    dims = [int(d) % state.ndim for d in dims]
    rest = [d for d in range(state.ndim) if d not in dims]
    a = np.transpose(state, dims + rest).reshape(2 ** len(dims), -1).astype(np.complex128)
    return a @ a.conj().T


def channel_weights(state, kraus, dims):
    """p_j = Re tr(K_j^+ K_j rho) / Re tr(rho)."""
    rho = rdm(state, dims)
    tr = np.trace(rho).real
    return np.array([np.trace(np.asarray(k).conj().T @ np.asarray(k) @ rho).real / tr for k in kraus], dtype=np.float64)


def amplitude_damping(gamma):
    return [np.array([[1, 0], [0, math.sqrt(1 - gamma)]], dtype=np.complex128),
            np.array([[0, math.sqrt(gamma)], [0, 0]], dtype=np.complex128)]


def depolarizing2(p):
    """Two-qubit depolarising channel: sqrt(1 - p) II and sqrt(p / 15) times the 15 other Pauli products."""
    paulis = [np.eye(2), np.array([[0, 1], [1, 0]]), np.array([[0, -1j], [1j, 0]]), np.array([[1, 0], [0, -1]])]
    out = []
    for i, a in enumerate(paulis):
        for j, b in enumerate(paulis):
            w = math.sqrt(1 - p) if i == j == 0 else math.sqrt(p / 15)
            out.append((w * np.kron(a, b)).astype(np.complex128))
    return out
