"""Diagonal operators: a classical cost function f(i) = sum_k c_k (-1)^popcount(i & zmask_k) applied to a state as ONE object
(C ABI: artn_diag_query, artn_diag_pack, artn_diag_values, artn_diag_expect, artn_diag_apply, artn_diag_pair).

terms = [(c_k, string_k), ...] as for pauli_sum_expectation, with REAL c_k and strings of I and Z only (a str over "IZ" of
the tensor's dims, or a dict {dim: "Z"}; {} is the identity, a constant).  Repeated strings are allowed and are not merged.
This is the cost layer of QAOA, a MaxCut, QUBO or Ising energy, a phase oracle, the ZZ part of a Trotter step.  Every
operation is one streaming pass over the amplitudes whatever the number of terms:

    op = DiagonalOperator(amps.shape, amps.stride(), amps.dtype, terms, amps.device)    # plan, pack, upload once
    op.evolve_(amps, gamma)          a <- a * exp(-i gamma f), in place
    op.multiply_(amps)               a <- a * f, in place: C|psi> without a second buffer
    op.expectation(amps)             (<f>, <f^2> - <f>^2), normalised by sum |a|^2 of the same pass
    op.moments(amps)                 [sum p, sum p f, sum p f^2], p = |a|^2
    op.pair_(lam, phi, gamma)        <lam| f |phi> taken before the phase; both states take the phase in the same pass

f is evaluated in float64 in the fixed order of include/artn.h (VALUE CONTRACT): it is a function of the memory index and
the term list alone, the same for both dtypes; sums are float64 in a fixed order without atomics, so every result is
bit-identical from run to run.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _native
from ._state import _Prebuilt, _checked, _desc, _dtype_code, _lib, _overlaps, _packed, _ptr
from .adjoint import PauliPairCircuit
from .born import norm2, overlap
from .pauli import PauliCircuit, pauli_ops

__all__ = ["DiagonalOperator", "diagonal_evolve_", "diagonal_expectation", "diagonal_values", "diagonal_info", "ising_terms",
           "maxcut_terms", "qaoa_gradient"]

_KERNELS = ("artn_diag_apply", "diagonal-operator kernels")    # what _lib looks for, and what it calls them


def _split(terms, n_dims, what):
    """(float64 [K] coefficients, uint8 ops [K, n_dims]) of terms = [(c_k, string_k), ...] with real c_k."""
    terms = list(terms)
    if not terms:
        raise ValueError(f"{what}: at least one term is needed")
    if any(not isinstance(t, (tuple, list)) or len(t) != 2 for t in terms):
        raise ValueError(f"{what}: terms are (coefficient, string) pairs")
    if any(complex(c).imag != 0.0 for c, _ in terms):
        raise ValueError(f"{what}: a diagonal operator takes real coefficients")
    coeff = np.ascontiguousarray([complex(c).real for c, _ in terms], dtype=np.float64)
    ops, _ = pauli_ops([p for _, p in terms], n_dims)
    return coeff, ops


def _query(d, ops, arrays=False):
    n = ops.shape[0]
    info = _native.ArtnDiagInfo()
    if arrays:
        zm, lo, hi = (np.zeros(n, dtype=np.uint64) for _ in range(3))
        group, group_lo = np.zeros(n, dtype=np.int32), np.zeros(_native.DIAG_MAX_GROUPS, dtype=np.uint64)
        out = (zm, lo, hi, group, group_lo)
        ptrs = [_ptr(x) for x in out]
    else:
        out, ptrs = (), [None] * 5
    _native.check(_lib(*_KERNELS, "diagonal").artn_diag_query(ctypes.byref(d), _ptr(ops), n, ctypes.byref(info), *ptrs))
    return (info,) + out


def diagonal_info(shape, strides, terms, dtype=torch.complex64):
    """Host-only: the plan of a diagonal operator.  K, n_static, n_dynamic, G (n_groups), tile_bits, n_tiles, table_bytes,
    workspace_bytes, bytes_read / bytes_written per operation (VALUES, EXPECT, PHASE, MULTIPLY, PAIR) and, per term, zmask, lo
    (the mask inside a tile), hi (the mask of the tile index) and group (-1: static); group_lo per group."""
    _dtype_code(dtype, "diagonal_info")
    _, ops = _split(terms, len(shape), "diagonal_info")
    info, zm, lo, hi, group, group_lo = _query(_desc(shape, strides, dtype), ops, arrays=True)
    return {"K": info.n_terms, "n_static": info.n_static, "n_dynamic": info.n_dynamic, "G": info.n_groups,
            "tile_bits": info.tile_bits, "n_tiles": info.n_tiles, "table_bytes": info.table_bytes,
            "workspace_bytes": info.workspace_bytes,
            "bytes_read": {o: int(info.bytes_read[i]) for i, o in enumerate(_native.DIAG_OPS)},
            "bytes_written": {o: int(info.bytes_written[i]) for i, o in enumerate(_native.DIAG_OPS)},
            "zmask": [int(v) for v in zm], "lo": [int(v) for v in lo], "hi": [int(v) for v in hi],
            "group": [int(v) for v in group], "group_lo": [int(v) for v in group_lo[:info.n_groups]]}


def _pack(d, ops, coeff):
    """The operator's table (include/artn.h) as a uint64 numpy array, and the query's info."""
    table, info = _packed(_query(d, ops)[0], lambda *table: _lib(*_KERNELS, "diagonal").artn_diag_pack(
        ctypes.byref(d), _ptr(ops), _ptr(coeff), ops.shape[0], *table))
    return table.view(np.uint64), info


class DiagonalOperator(_Prebuilt):
    """f = sum_k c_k Z-string_k for tensors of one layout: validates, plans, packs the table and copies it to `device` once.
    The workspace of the sums is allocated per call, so an instance holds no state that two calls share."""

    def __init__(self, shape, strides, dtype, terms, device):
        self._bind(shape, strides, dtype, device)
        coeff, self._ops = _split(terms, len(self.shape), "DiagonalOperator")
        self._d = _desc(self.shape, self.strides, dtype)
        table, info = _pack(self._d, self._ops, coeff)
        self.n_terms, self.n_static, self.n_dynamic, self.n_groups = info.n_terms, info.n_static, info.n_dynamic, info.n_groups
        self.tile_bits, self.n_tiles = info.tile_bits, info.n_tiles
        self.table_bytes, self.workspace_bytes = info.table_bytes, info.workspace_bytes
        self._upload(table.view(np.uint8))

    def _apply(self, amps, mode, gamma, what):
        self._check(amps, what)
        with torch.cuda.device(amps.device):
            _native.check(_lib(*_KERNELS, what).artn_diag_apply(ctypes.byref(self._d), amps.data_ptr(), _ptr(self._ops), self.n_terms,
                                                                self._table.data_ptr(), self.table_bytes, mode, float(gamma),
                                                                _native.current_stream_ptr(amps.device)))
        return amps

    def evolve_(self, amps, gamma):
        """amps <- amps * exp(-i gamma f) in place (one launch; gamma == 0: none).  Returns amps."""
        return self._apply(amps, _native.DIAG_PHASE, gamma, "diagonal.DiagonalOperator.evolve_")

    def multiply_(self, amps):
        """amps <- amps * f in place: each component one float64 product, rounded once.  Returns amps."""
        return self._apply(amps, _native.DIAG_MULTIPLY, 0.0, "diagonal.DiagonalOperator.multiply_")

    def values(self):
        """f as a float64 GPU tensor with the state's shape and strides (for tests and small states: 8 bytes per element)."""
        what = "diagonal.DiagonalOperator.values"
        out = torch.empty_strided(self.shape, self.strides, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _native.check(_lib(*_KERNELS, what).artn_diag_values(ctypes.byref(self._d), _ptr(self._ops), self.n_terms,
                                                                 self._table.data_ptr(), self.table_bytes, out.data_ptr(),
                                                                 _native.current_stream_ptr(self.device)))
        return out

    def moments(self, amps, device=False):
        """[sum p, sum p f, sum p f^2], p = |a|^2 formed in float64, from one read pass: float64 numpy [3], or with device=True
        a float64 GPU tensor [3] without a host synchronisation."""
        what = "diagonal.DiagonalOperator.moments"
        self._check(amps, what)
        out = torch.empty(3, dtype=torch.float64, device=amps.device)
        ws = torch.empty(self.workspace_bytes // 8, dtype=torch.float64, device=amps.device)   # (per call: calls may overlap on streams)
        with torch.cuda.device(amps.device):
            _native.check(_lib(*_KERNELS, what).artn_diag_expect(ctypes.byref(self._d), amps.data_ptr(), _ptr(self._ops), self.n_terms,
                                                                 self._table.data_ptr(), self.table_bytes, ws.data_ptr(),
                                                                 self.workspace_bytes, out.data_ptr(),
                                                                 _native.current_stream_ptr(amps.device)))
        return out if device else out.cpu().numpy()

    def expectation(self, amps, device=False):
        """(E, var) = (<f>, <f^2> - <f>^2), normalised by sum |a|^2 of the same pass: floats, or 0-dim float64 GPU tensors with
        device=True (no host synchronisation)."""
        m = self.moments(amps, device=True)
        if not device:
            m = m.cpu().numpy()
        e, e2 = m[1] / m[0], m[2] / m[0]
        var = e2 - e * e
        return (e, var) if device else (float(e), float(var))

    def pair_(self, lam, phi, gamma, device=False, evolve=True):
        """t = sum_i conj(lam_i) f(i) phi_i from the values BEFORE the phase; in the same pass lam and phi both take
        exp(-i gamma f) in place and are afterwards bit for bit what evolve_ leaves on each alone.  evolve=False: the
        transition element only, nothing is written.  Returns a complex, or with device=True the float64 GPU tensor [Re, Im]
        without a host synchronisation."""
        what = "diagonal.DiagonalOperator.pair_"
        for x in (lam, phi):
            self._check(x, what)
        if _overlaps(lam, phi):
            raise ValueError(f"{what}: lam overlaps phi")
        out = torch.empty(2, dtype=torch.float64, device=phi.device)
        ws = torch.empty(self.workspace_bytes // 8, dtype=torch.float64, device=phi.device)
        mode = _native.DIAG_PAIR_EVOLVE if evolve else _native.DIAG_PAIR_TRANSITION
        with torch.cuda.device(phi.device):
            _native.check(_lib(*_KERNELS, what).artn_diag_pair(ctypes.byref(self._d), lam.data_ptr(), phi.data_ptr(), _ptr(self._ops),
                                                               self.n_terms, self._table.data_ptr(), self.table_bytes, mode, float(gamma),
                                                               ws.data_ptr(), self.workspace_bytes, out.data_ptr(),
                                                               _native.current_stream_ptr(phi.device)))
        if device:
            return out
        re, im = out.tolist()
        return complex(re, im)


def _operator(amps, terms, what):
    _native.require_gpu(amps, what)
    _checked(amps, what)
    return DiagonalOperator(amps.shape, amps.stride(), amps.dtype, terms, amps.device)


def diagonal_evolve_(amps, terms, gamma):
    """amps <- amps * exp(-i gamma f) in place, f = sum_k c_k Z-string_k.  (Plans and uploads per call: build a DiagonalOperator
    once to apply the same operator repeatedly.)"""
    return _operator(amps, terms, "diagonal.diagonal_evolve_").evolve_(amps, gamma)


def diagonal_expectation(amps, terms):
    """(<f>, <f^2> - <f>^2) of one read pass over amps, normalised by sum |amps|^2 of the same pass."""
    return _operator(amps, terms, "diagonal.diagonal_expectation").expectation(amps)


def diagonal_values(op):
    """f of a DiagonalOperator as a float64 GPU tensor with the state's shape and strides."""
    if not isinstance(op, DiagonalOperator):
        raise TypeError(f"diagonal_values: a DiagonalOperator expected, got {type(op).__name__}")
    return op.values()


def ising_terms(J, h=None, offset=0.0):
    """The terms of f(z) = sum_{q<r} J_qr z_q z_r + sum_q h_q z_q + offset with z_q = (-1)^(bit of dim q).  J: a dict
    {(q, r): J_qr} (q != r; a pair may be listed once) or a square array whose UPPER triangle is read (a non-zero lower triangle
    must mirror it); h: a dict {q: h_q} or a sequence; zero entries of arrays give no term.  Strings are dicts {dim: "Z"}, so the
    list fits a tensor of any number of dims that has them."""
    terms = []
    if isinstance(J, dict):
        seen = set()
        for (q, r), c in J.items():
            q, r = int(q), int(r)
            if q == r or (min(q, r), max(q, r)) in seen:
                raise ValueError(f"ising_terms: the bond ({q}, {r}) joins a qubit to itself or is listed twice")
            seen.add((min(q, r), max(q, r)))
            terms.append((float(c), {q: "Z", r: "Z"}))
    else:
        Jm = np.asarray(J, dtype=np.float64)
        if Jm.ndim != 2 or Jm.shape[0] != Jm.shape[1]:
            raise ValueError(f"ising_terms: J is a dict or a square array, got shape {Jm.shape}")
        low = np.tril(Jm, -1)
        if low.any() and not np.array_equal(low, np.triu(Jm, 1).T):
            raise ValueError("ising_terms: the lower triangle of J is neither zero nor the mirror of the upper one")
        for q in range(Jm.shape[0]):
            for r in range(q + 1, Jm.shape[0]):
                if Jm[q, r] != 0.0:
                    terms.append((float(Jm[q, r]), {q: "Z", r: "Z"}))
    if h is not None:
        items = h.items() if isinstance(h, dict) else enumerate(np.asarray(h, dtype=np.float64).reshape(-1))
        for q, c in items:
            if isinstance(h, dict) or c != 0.0:
                terms.append((float(c), {int(q): "Z"}))
    if float(offset) != 0.0:
        terms.append((float(offset), {}))
    if not terms:
        raise ValueError("ising_terms: no term at all")
    return terms


def maxcut_terms(edges, weights=None):
    """The terms of the cut value f(z) = sum_(q,r) w_qr (1 - z_q z_r) / 2 of the graph `edges` = [(q, r), ...] (weights: one per
    edge, default 1): -w/2 on every ZZ bond and the constant sum w / 2.  f(i) is the weight of the edges the bitstring i cuts."""
    edges = [(int(q), int(r)) for q, r in edges]
    w = [1.0] * len(edges) if weights is None else [float(x) for x in weights]
    if len(w) != len(edges) or not edges:
        raise ValueError(f"maxcut_terms: {len(edges)} edges and {len(w)} weights")
    if any(q == r for q, r in edges):
        raise ValueError("maxcut_terms: an edge joins a vertex to itself")
    terms = [(-0.5 * x, {q: "Z", r: "Z"}) for (q, r), x in zip(edges, w)]
    terms.append((0.5 * float(np.sum(w)), {}))
    return terms


def qaoa_gradient(amps0, cost_terms, gammas, betas, normalize=True, max_rank=None):
    """(E, grad) of E = <psi| C |psi>, psi = prod_{l = p-1 .. 0} [M(beta_l) exp(-i gamma_l C)] amps0, C = the diagonal operator of
    cost_terms and M(beta) = prod_q exp(-i beta X_q) over every dim q of extent 2, by the adjoint method.  grad is float64 numpy
    [2p]: dE/dgamma_0 .. dE/dgamma_{p-1}, then dE/dbeta_0 .. dE/dbeta_{p-1}.

    Forward, per layer: DiagonalOperator.evolve_ and one PauliCircuit for the mixer.  Then lam = copy(phi), multiply_(lam) and
    E = Re <phi|lam>.  Backward, per layer: the mixer through a PauliPairCircuit of the reversed rotations with negated angle,
    every step measured (dE/dbeta_l = sum_q 2 Im t_q), and the cost layer as ONE pair_(lam, phi, -gamma_l)
    (dE/dgamma_l = 2 Im t).  The mixer circuits are built once per DISTINCT beta and reused by the layers that share it.
    normalize=True divides E and grad by sum |amps0|^2.  max_rank is passed to both mixer circuits (the two-state limits apply to
    the backward one).  amps0 is never written; two state-sized tensors are allocated."""
    what = "diagonal.qaoa_gradient"
    _native.require_gpu(amps0, what)
    _checked(amps0, what)
    gammas, betas = [float(g) for g in gammas], [float(b) for b in betas]
    if len(gammas) != len(betas) or not gammas:
        raise ValueError(f"{what}: one gamma and one beta per layer, at least one layer (got {len(gammas)} and {len(betas)})")
    shape, strides, dtype, dev = amps0.shape, amps0.stride(), amps0.dtype, amps0.device
    qubits = [q for q, e in enumerate(shape) if int(e) == 2]
    if not qubits:
        raise ValueError(f"{what}: the tensor has no dim of extent 2 for the mixer")
    p = len(gammas)
    op = DiagonalOperator(shape, strides, dtype, cost_terms, dev)
    # built first: a refusal (max_rank, the layout) comes before any work on the device
    forward, backward = {}, {}
    for b in betas:
        if b not in forward:
            forward[b] = PauliCircuit(shape, strides, dtype, [(b, {q: "X"}) for q in qubits], dev, max_rank)
            backward[b] = PauliPairCircuit(shape, strides, dtype, [(-b, {q: "X"}) for q in reversed(qubits)], dev, None, max_rank)
    phi = torch.empty_strided(shape, strides, dtype=dtype, device=dev)
    phi.copy_(amps0)
    for g, b in zip(gammas, betas):
        op.evolve_(phi, g)
        forward[b](phi)
    lam = torch.empty_strided(shape, strides, dtype=dtype, device=dev)
    lam.copy_(phi)
    op.multiply_(lam)
    energy = overlap(phi, lam)[0].real
    grad = np.zeros(2 * p, dtype=np.float64)
    # the sweep runs with negated angles: U^+ = exp(+i theta G), and every t is taken before U^+ is applied
    for layer in range(p - 1, -1, -1):
        t = backward[betas[layer]](lam, phi)
        grad[p + layer] = float(np.sum(2.0 * t.imag))
        grad[layer] = 2.0 * op.pair_(lam, phi, -gammas[layer]).imag
    if normalize:
        n2 = norm2(amps0)
        energy, grad = energy / n2, grad / n2
    return energy, grad
