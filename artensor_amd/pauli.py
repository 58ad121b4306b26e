"""Expectation values of Pauli strings and of sums of them (Hamiltonians) on an amplitude tensor on the device (C ABI:
artn_pauli_query, artn_pauli_expect).

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
from .born import _DTYPES, _checked

__all__ = ["pauli_ops", "pauli_info", "pauli_expectation", "pauli_sum_expectation"]

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


def _desc(shape, strides, dtype):
    nd = len(shape)
    if nd > _native.ARTN_MAX_LABELS:
        raise ValueError(f"at most {_native.ARTN_MAX_LABELS} dims")
    d = _native.ArtnMarginalDesc()
    d.dtype, d.n_dims = _DTYPES[dtype], nd
    for pos in range(nd):                                     # the caller's dim order; keep[] is not read
        d.extent[pos], d.stride[pos] = int(shape[pos]), int(strides[pos])
    return d


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
    if dtype not in _DTYPES:
        raise TypeError(f"pauli_info: complex64 or complex128 expected, got {dtype}")
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
