"""Expectation values of Pauli strings and of sums of them (Hamiltonians) on an amplitude tensor on the device (C ABI:
artn_pauli_query, artn_pauli_expect), and the same operators APPLIED to the tensor: y = H a in one launch (artn_pauli_apply_query,
artn_pauli_apply_pack, artn_pauli_apply), and IN-PLACE circuits of steps a <- alpha a + beta P a -- rotations exp(-i theta P) among
them -- fused into runs that read and write the state once (artn_pauli_evolve_query, artn_pauli_evolve_pack, artn_pauli_evolve).

A Pauli string gives every dim of `amps` one of I, X, Y, Z -- X, Y and Z only on dims of extent 2, every other dim (a row
dimension, an extent-1 dim) carries I.  It is written either as a `str` of length amps.dim() over "IXYZ" (any case; character d
acts on dim d) or as a dict {dim: 'X', ...} with every other dim I (negative dims count from the end).  A string is a signed
permutation of the basis, so <psi|P|psi> is one streaming pass over the amplitudes with one multiply per amplitude, whatever the
weight of the string; strings that move the same dims (equal X/Y positions) share a pass, sixteen at a time.

The functions take what born.py takes -- a dense GPU tensor of complex64 or complex128 in any permuted layout, never copied --
and keep its contract: terms and sums in float64, a fixed summation order, bit-identical results from run to run.  There is no
CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _native
from ._state import (_Prebuilt, _RunCircuit, _checked, _desc, _dtype_code, _max_rank, _overlaps, _packed, _ptr, _run_keys, _run_pack,
                     _run_query)
from .born import norm2, overlap

__all__ = ["pauli_ops", "pauli_info", "pauli_expectation", "pauli_sum_expectation", "pauli_apply_info", "PauliSumOperator",
           "pauli_sum_apply", "pauli_apply", "pauli_rotate", "pauli_sum_variance", "pauli_evolve_info", "PauliCircuit",
           "pauli_evolve_", "pauli_rotate_", "pauli_apply_", "trotter_steps"]

_CODES = {"I": 0, "X": 1, "Y": 2, "Z": 3}


def _one(p, nd):
    row = np.zeros(nd, dtype=np.uint8)
    if isinstance(p, str):
        if len(p) != nd:
            raise ValueError(f"a Pauli string of length {len(p)} for a tensor of {nd} dims: {p!r}")
        items = enumerate(p)
    elif isinstance(p, dict):
        items = p.items()
    else:
        raise TypeError(f"a Pauli string is a str over IXYZ or a dict {{dim: letter}}, got {type(p).__name__}")
    seen = set()
    for dim, letter in items:
        d = int(dim) + nd if int(dim) < 0 else int(dim)
        if d < 0 or d >= nd or d in seen:
            raise ValueError(f"Pauli string {p!r}: dims must be distinct dims of a {nd}-dim tensor")
        seen.add(d)
        code = _CODES.get(letter.upper()) if isinstance(letter, str) and len(letter) == 1 else None
        if code is None:
            raise ValueError(f"Pauli string {p!r}: {letter!r} is not one of I, X, Y, Z")
        row[d] = code
    return row


def pauli_ops(paulis, n_dims):
    """uint8 [n_terms, n_dims] operator codes (0..3 = I, X, Y, Z) of one string or a list of strings, and whether it was one."""
    single = isinstance(paulis, (str, dict))
    terms = [paulis] if single else list(paulis)
    if not terms:
        raise ValueError("at least one Pauli string is needed")
    return np.ascontiguousarray(np.stack([_one(p, int(n_dims)) for p in terms])), single


def _query(d, ops, masks=False):
    n_terms = ops.shape[0]
    info = _native.ArtnPauliInfo()
    if masks:
        xm, zm = np.zeros(n_terms, dtype=np.uint64), np.zeros(n_terms, dtype=np.uint64)
        ny, group = np.zeros(n_terms, dtype=np.int32), np.zeros(n_terms, dtype=np.int32)
        ptrs = [x.ctypes.data_as(ctypes.c_void_p) for x in (xm, zm, ny, group)]
    else:
        xm = zm = ny = group = None
        ptrs = [None] * 4
    _native.check(_native.lib().artn_pauli_query(ctypes.byref(d), ops.ctypes.data_as(ctypes.c_void_p), n_terms,
                                                 ctypes.byref(info), *ptrs))
    return info, xm, zm, ny, group


def pauli_info(shape, strides, paulis, dtype=torch.complex64):
    """Host-only: the memory-bit masks of every string (xmask: bits under X or Y, zmask: bits under Z or Y, n_y), the group
    (strings of equal xmask) of each, the number of groups and of passes over the amplitudes, the workspace and the bytes read
    (RuntimeError where the library refuses; TypeError for a dtype that is not complex)."""
    _dtype_code(dtype, "pauli_info")
    ops, _ = pauli_ops(paulis, len(shape))
    info, xm, zm, ny, group = _query(_desc(shape, strides, dtype), ops, masks=True)
    return {"xmask": [int(v) for v in xm], "zmask": [int(v) for v in zm], "n_y": [int(v) for v in ny],
            "group": [int(v) for v in group], "n_groups": info.n_groups, "n_launches": info.n_launches,
            "terms_per_launch": info.terms_per_launch, "workspace_bytes": info.workspace_bytes, "bytes_read": info.bytes_read}


def _raw(amps, ops, what):
    """float64 GPU tensor [n_terms + 1]: the raw sums in term order, then sum |a|^2."""
    _checked(amps, what)
    d = _desc(amps.shape, amps.stride(), amps.dtype)
    info, *_ = _query(d, ops)
    n_terms = ops.shape[0]
    out = torch.empty(n_terms + 1, dtype=torch.float64, device=amps.device)
    ws = torch.empty(max(info.workspace_bytes // 8, 1), dtype=torch.float64, device=amps.device)
    with torch.cuda.device(amps.device):
        _native.check(_native.lib().artn_pauli_expect(ctypes.byref(d), amps.data_ptr(), ops.ctypes.data_as(ctypes.c_void_p),
                                                      n_terms, out.data_ptr(), ws.data_ptr(), info.workspace_bytes,
                                                      _native.current_stream_ptr(amps.device)))
    return out


def pauli_expectation(amps, paulis, normalize=True, device=False):
    """<amps|P|amps> for one Pauli string (a float) or a list of them (a float64 numpy array), divided by sum |amps|^2 of the
    same call unless normalize=False.  device=True: a float64 GPU tensor (0-dim for one string), no host synchronisation.
    A string's raw value does not depend on what else the call holds, bit for bit; the norm comes from the call's first pass,
    whose summation order follows the first string's X/Y positions, so normalised values may differ in the last bit."""
    _native.require_gpu(amps, "pauli.pauli_expectation")
    ops, single = pauli_ops(paulis, amps.dim())
    out = _raw(amps, ops, "pauli.pauli_expectation")
    vals = out[:-1] / out[-1] if normalize else out[:-1]
    if single:
        return vals[0] if device else float(vals[0])
    return vals if device else vals.cpu().numpy()


def pauli_sum_expectation(amps, terms, normalize=True):
    """sum_k c_k <P_k> for terms = [(c_k, string_k), ...] from ONE call of the library: a float when every coefficient is real,
    a complex otherwise."""
    _native.require_gpu(amps, "pauli.pauli_sum_expectation")
    terms = list(terms)
    if not terms:
        raise ValueError("at least one term is needed")
    coeffs = [complex(c) for c, _ in terms]
    ops, _ = pauli_ops([p for _, p in terms], amps.dim())
    out = _raw(amps, ops, "pauli.pauli_sum_expectation").cpu().numpy()
    vals = out[:-1] / out[-1] if normalize else out[:-1]
    if all(c.imag == 0.0 for c in coeffs):
        return float(np.dot(np.array([c.real for c in coeffs]), vals))
    return complex(np.dot(np.array(coeffs), vals))


# ---- y = H a ----------------------------------------------------------------------------------------------------------------
def _split_terms(terms, n_dims):
    """([n_terms, 2] float64 coefficients, uint8 ops) of terms = [(c_k, string_k), ...]."""
    terms = list(terms)
    if not terms:
        raise ValueError("at least one term is needed")
    coeff = np.array([[complex(c).real, complex(c).imag] for c, _ in terms], dtype=np.float64)
    ops, _ = pauli_ops([p for _, p in terms], n_dims)
    return np.ascontiguousarray(coeff), ops


def _apply_query(d, ops, coeff, arrays=False):
    n_terms = ops.shape[0]
    info = _native.ArtnPauliApplyInfo()
    if arrays:
        xm, zm, gx = (np.zeros(n_terms, dtype=np.uint64) for _ in range(3))
        ny, group, pos = (np.zeros(n_terms, dtype=np.int32) for _ in range(3))
        folded = np.zeros((n_terms, 2), dtype=np.float64)
        out = (xm, zm, ny, group, folded, gx, pos)
        ptrs = [_ptr(x) for x in out]
    else:
        out, ptrs = (), [None] * 7
    _native.check(_native.lib().artn_pauli_apply_query(ctypes.byref(d), _ptr(ops), _ptr(coeff), n_terms, ctypes.byref(info), *ptrs))
    return (info,) + out


def pauli_apply_info(shape, strides, terms, dtype=torch.complex64):
    """Host-only: what one call of y = H a does for terms = [(c_k, string_k), ...].  Per term: xmask, zmask, n_y, group and the
    folded coefficient c_k (-i)^n_y (complex).  Per group (numbered as they first appear): group_xmask and group_pos, its position
    in the summation order of every output element; group_order lists the groups in that order.  n_xmask_hi: the partner tiles
    fetched per output tile; table_bytes; the nominal bytes_read and bytes_written; n_launches (1)."""
    _dtype_code(dtype, "pauli_apply_info")
    coeff, ops = _split_terms(terms, len(shape))
    info, xm, zm, ny, group, folded, gx, pos = _apply_query(_desc(shape, strides, dtype), ops, coeff, arrays=True)
    ng = info.n_groups
    pos = [int(v) for v in pos[:ng]]
    return {"xmask": [int(v) for v in xm], "zmask": [int(v) for v in zm], "n_y": [int(v) for v in ny], "group": [int(v) for v in group],
            "folded": [complex(r, i) for r, i in folded], "n_groups": ng, "group_xmask": [int(v) for v in gx[:ng]], "group_pos": pos,
            "group_order": [int(g) for g in np.argsort(pos)], "n_xmask_hi": info.n_xmask_hi, "table_bytes": info.table_bytes,
            "bytes_read": info.bytes_read, "bytes_written": info.bytes_written, "n_launches": info.n_launches}


def _pack(d, ops, coeff):
    """The term table (include/artn.h) as a uint8 numpy array."""
    return _packed(_apply_query(d, ops, coeff)[0],
                   lambda *table: _native.lib().artn_pauli_apply_pack(ctypes.byref(d), _ptr(ops), _ptr(coeff), ops.shape[0], *table))


class PauliSumOperator(_Prebuilt):
    """H = sum_k c_k P_k (terms = [(c_k, string_k), ...], complex coefficients allowed) for tensors of one layout: validates,
    packs the term table and copies it to `device` once; op(amps, out=None) is then one launch that writes H|amps> in the layout of
    amps.  `amps` is read in place and never written."""

    def __init__(self, shape, strides, dtype, terms, device):
        self._bind(shape, strides, dtype, device)
        coeff, self._ops = _split_terms(terms, len(self.shape))
        self._d = _desc(self.shape, self.strides, dtype)
        table, info = _pack(self._d, self._ops, coeff)
        self.n_terms, self.n_groups, self.table_bytes = self._ops.shape[0], info.n_groups, info.table_bytes
        self._upload(table)

    def __call__(self, amps, out=None):
        what = "pauli.PauliSumOperator"
        self._check(amps, what)
        if out is None:
            out = torch.empty_strided(self.shape, self.strides, dtype=self.dtype, device=amps.device)
        else:
            if not isinstance(out, torch.Tensor) or out.dtype != amps.dtype or out.device != amps.device \
                    or tuple(out.shape) != self.shape or tuple(out.stride()) != self.strides:
                raise ValueError(f"{what}: out must have the shape, strides, dtype and device of amps")
            if _overlaps(out, amps):
                raise ValueError(f"{what}: out overlaps amps (there is no in-place form)")
            if out.data_ptr() % 16:
                raise ValueError(f"{what}: out must start on a 16-byte boundary")
        with torch.cuda.device(amps.device):
            _native.check(_native.lib().artn_pauli_apply(ctypes.byref(self._d), amps.data_ptr(), out.data_ptr(), _ptr(self._ops),
                                                         self.n_terms, self._table.data_ptr(), self.table_bytes,
                                                         _native.current_stream_ptr(amps.device)))
        return out


def pauli_sum_apply(amps, terms, out=None):
    """H|amps> for H = sum_k c_k P_k, terms = [(c_k, string_k), ...]: one launch; the result has the shape, strides and dtype of
    amps (out=None allocates it)."""
    _checked(amps, "pauli.pauli_sum_apply")
    return PauliSumOperator(amps.shape, amps.stride(), amps.dtype, terms, amps.device)(amps, out)


def pauli_apply(amps, string, out=None):
    """P|amps> for one Pauli string."""
    _checked(amps, "pauli.pauli_apply")
    return PauliSumOperator(amps.shape, amps.stride(), amps.dtype, [(1.0, string)], amps.device)(amps, out)


def pauli_rotate(amps, string, theta, out=None):
    """exp(-i theta P)|amps> = cos(theta) amps - i sin(theta) P amps: a two-term sum (I, P), one launch, out of place."""
    _checked(amps, "pauli.pauli_rotate")
    theta = float(theta)
    terms = [(np.cos(theta), {}), (-1j * np.sin(theta), string)]
    return PauliSumOperator(amps.shape, amps.stride(), amps.dtype, terms, amps.device)(amps, out)


def pauli_sum_variance(amps, terms):
    """(E, var) of H = sum_k c_k P_k with REAL coefficients: E = Re<a|Ha> / |a|^2 and var = |Ha|^2 / |a|^2 - E^2, from one apply,
    one overlap and one norm."""
    _native.require_gpu(amps, "pauli.pauli_sum_variance")
    terms = list(terms)
    if any(complex(c).imag != 0.0 for c, _ in terms):
        raise ValueError("pauli_sum_variance takes real coefficients (a Hermitian sum)")
    y = pauli_sum_apply(amps, terms)
    aha, na, _ = overlap(amps, y)
    e = aha.real / na
    return e, norm2(y) / na - e * e


# ---- in-place circuits -------------------------------------------------------------------------------------------------------
def _split_steps(steps, n_dims):
    """([n_steps, 4] float64 alpha, beta; uint8 ops) of steps = [(theta, string) | (alpha, beta, string), ...]."""
    steps = list(steps)
    if not steps:
        raise ValueError("at least one step is needed")
    coeff, strings = np.zeros((len(steps), 4), dtype=np.float64), []
    for k, step in enumerate(steps):
        if not isinstance(step, (tuple, list)) or len(step) not in (2, 3):
            raise ValueError(f"step {k}: (theta, string) or (alpha, beta, string) expected, got {step!r}")
        if len(step) == 2:
            theta = float(step[0])
            coeff[k] = (np.cos(theta), 0.0, 0.0, -np.sin(theta))
        else:
            alpha, beta = complex(step[0]), complex(step[1])
            coeff[k] = (alpha.real, alpha.imag, beta.real, beta.imag)
        strings.append(step[-1])
    ops, _ = pauli_ops(strings, n_dims)
    return np.ascontiguousarray(coeff), ops


# what a circuit query writes: xmask, zmask, n_y, run, slot_mask, run_rank, run_basis, run_pivot
_STEP_ARRAYS = ((np.uint64, 0),) * 2 + ((np.int32, 0),) * 4 + tuple((t, _native.PAULI_EVOLVE_MAX_RANK) for t in (np.uint64, np.int32))


def _evolve_query(d, ops, coeff, max_rank, arrays=False):
    return _run_query("artn_pauli_evolve_query", _native.ArtnPauliEvolveInfo(), d, (ops, coeff), max_rank, _STEP_ARRAYS, arrays)


def _step_keys(coeff, xm, zm, ny, run, slot):
    """The per-step lists of pauli_evolve_info."""
    return {"xmask": [int(v) for v in xm], "zmask": [int(v) for v in zm], "n_y": [int(v) for v in ny],
            "alpha": [complex(c[0], c[1]) for c in coeff], "beta": [complex(c[2], c[3]) for c in coeff],
            "run": [int(v) for v in run], "slot_mask": [int(v) for v in slot]}


def pauli_evolve_info(shape, strides, steps, dtype=torch.complex64, max_rank=None):
    """Host-only: how a circuit of steps = [(theta, string) | (alpha, beta, string), ...] is cut into runs.  Per step: xmask, zmask,
    n_y, alpha, beta (complex), run and slot_mask.  Per run: run_rank, run_basis (memory-bit masks, ascending pivots) and
    run_pivot.  n_runs = n_launches, the effective max_rank, table_bytes, bytes_read = bytes_written = n_runs * bytes of the
    state."""
    _dtype_code(dtype, "pauli_evolve_info")
    coeff, ops = _split_steps(steps, len(shape))
    info, *steps, rank, basis, pivot = _evolve_query(_desc(shape, strides, dtype), ops, coeff, _max_rank(max_rank), arrays=True)
    return {**_step_keys(coeff, *steps), **_run_keys(info, rank, run_basis=basis, run_pivot=pivot)}


def _evolve_pack(d, ops, coeff, max_rank):
    """The circuit table (include/artn.h) as a uint8 numpy array."""
    return _run_pack(_evolve_query, "artn_pauli_evolve_pack", d, (ops, coeff), max_rank)


class PauliCircuit(_RunCircuit):
    """An ordered list of steps a <- alpha a + beta P a for tensors of one layout: steps = [(theta, string), ...] for the rotation
    exp(-i theta P) or (alpha, beta, string) for the general step.  Validates, cuts the runs, packs the table and copies it to
    `device` once; circ(amps) then updates amps IN PLACE with one launch per run and returns it.  max_rank: a run holds blocks of
    up to 2^max_rank tiles of 2^10 elements in LDS (None: 64 KiB per workgroup; 0: one launch per step with a flip above the tile)."""

    def __init__(self, shape, strides, dtype, steps, device, max_rank=None):
        (self._ops, _), _ = self._build(shape, strides, dtype, device, max_rank, lambda nd: _split_steps(steps, nd)[::-1], _evolve_query,
                                        "artn_pauli_evolve_pack")
        self.n_steps = self._n

    def __call__(self, amps):
        return self._run("pauli.PauliCircuit", "artn_pauli_evolve", amps, _ptr(self._ops))


def pauli_evolve_(amps, steps, max_rank=None):
    """The circuit `steps` (see PauliCircuit) applied to amps in place; returns amps."""
    _checked(amps, "pauli.pauli_evolve_")
    return PauliCircuit(amps.shape, amps.stride(), amps.dtype, steps, amps.device, max_rank)(amps)


def pauli_rotate_(amps, string, theta):
    """amps <- exp(-i theta P) amps in place: one launch, no second buffer."""
    _checked(amps, "pauli.pauli_rotate_")
    return PauliCircuit(amps.shape, amps.stride(), amps.dtype, [(float(theta), string)], amps.device)(amps)


def pauli_apply_(amps, string):
    """amps <- P amps in place: an exact signed permutation."""
    _checked(amps, "pauli.pauli_apply_")
    return PauliCircuit(amps.shape, amps.stride(), amps.dtype, [(0.0, 1.0, string)], amps.device)(amps)


def trotter_steps(terms, dt, order=1):
    """Rotation list of one Trotter step of exp(-i dt H), H = sum_k c_k P_k with REAL c_k, terms = [(c_k, string_k), ...]: order 1
    is exp(-i dt c_K P_K) ... exp(-i dt c_1 P_1) as [(dt c_1, P_1), ..., (dt c_K, P_K)]; order 2 the symmetric product, half
    angles up to the last term, its full angle once (the two middle factors merged), then the half angles back: 2 K - 1 steps."""
    terms = list(terms)
    if not terms:
        raise ValueError("at least one term is needed")
    if order not in (1, 2):
        raise ValueError(f"trotter_steps: order 1 or 2, got {order!r}")
    coeffs = []
    for c, _ in terms:
        c = complex(c)
        if c.imag != 0.0:
            raise ValueError("trotter_steps takes real coefficients (a Hermitian sum)")
        coeffs.append(c.real)
    dt = float(dt)
    if order == 1:
        return [(dt * c, p) for c, (_, p) in zip(coeffs, terms)]
    half = [(0.5 * dt * c, p) for c, (_, p) in zip(coeffs[:-1], terms[:-1])]
    return half + [(dt * coeffs[-1], terms[-1][1])] + half[::-1]
