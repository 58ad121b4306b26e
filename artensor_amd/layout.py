"""IN-PLACE permutations of the index bits of a dense state: relayout without a second buffer, qubit remapping, SWAP networks and
qubit reversal as pure data movement (C ABI: artn_bitperm_query, artn_bitperm_pack, artn_bitperm_apply).

A dim of extent 2^e and stride 2^s is the FIELD of memory bits s .. s+e-1; a dim of extent 1 carries no bit.  Every function here
turns its argument into `dst_bit` -- memory bit b of an element's index becomes bit dst_bit[b] -- and the library moves the
elements: new[pi(i)] == old[i] bit for bit (the sign of a zero, NaN payloads, denormals: an element is only ever copied), in
at most max(1, ceil((h - 1) / 7)) passes over the state, h the number of moved bits at or above a 128-byte line, each pass one
read and one write of the state through a 32 KiB tile in LDS (include/artn.h has the contract and the plan).  The identity issues
no launch.  GPU tensors only; there is no CPU fallback.
"""
import ctypes
from collections import Counter

import numpy as np
import torch

from . import _native
from ._state import _Prebuilt, _checked, _desc, _dtype_code, _lib, _packed, _ptr

__all__ = ["permute_dims_", "swap_dims_", "reverse_qubits_", "relayout_", "BitPermutation", "bit_permutation_info",
           "busiest_dims_order"]

_KERNELS = ("artn_bitperm_apply", "bit-permutation kernel")    # what _lib looks for, and what it calls it


def _fields(shape, strides, what):
    """Per dim (first bit, number of bits) of a dense power-of-two layout, and the number of index bits."""
    fields, n_bits = [], 0
    for k, (e, s) in enumerate(zip(shape, strides)):
        e, s = int(e), int(s)
        if e < 1 or e & (e - 1):
            raise ValueError(f"{what}: power-of-two extents expected, dim {k} has extent {e}")
        if e == 1:
            fields.append((0, 0))
            continue
        if s < 1 or s & (s - 1):
            raise ValueError(f"{what}: the tensor is not dense (shape {tuple(shape)}, strides {tuple(strides)})")
        fields.append((s.bit_length() - 1, e.bit_length() - 1))
        n_bits += e.bit_length() - 1
    return fields, n_bits


def _is_permutation(p, n):
    return sorted(p) == list(range(n))


def dst_bit_of_perm(shape, strides, perm):
    """dst_bit of permute_dims_: the field of dim perm[k] moves to the field of dim k."""
    what = "layout.permute_dims_"
    perm = [int(p) for p in perm]
    if not _is_permutation(perm, len(shape)):
        raise ValueError(f"{what}: perm must be a permutation of range({len(shape)}), got {perm}")
    fields, n_bits = _fields(shape, strides, what)
    dst = list(range(n_bits))
    for k, src in enumerate(perm):
        if int(shape[src]) != int(shape[k]):
            raise ValueError(f"{what}: dim {src} (extent {shape[src]}) cannot take the place of dim {k} (extent {shape[k]}) in place; "
                             "relayout_ moves dims of different extents")
        for t in range(fields[k][1]):
            dst[fields[src][0] + t] = fields[k][0] + t
    return dst


def dst_bit_of_order(shape, strides, order=None):
    """(dst_bit, new strides) of relayout_: the dims lie in memory in `order`, slowest first (None: range(dim), contiguous)."""
    what = "layout.relayout_"
    order = list(range(len(shape))) if order is None else [int(k) for k in order]
    if not _is_permutation(order, len(shape)):
        raise ValueError(f"{what}: order must be a permutation of range({len(shape)}), got {order}")
    fields, n_bits = _fields(shape, strides, what)
    new_strides, at = [0] * len(shape), 0
    dst = list(range(n_bits))
    for k in reversed(order):
        new_strides[k] = 1 << at
        for t in range(fields[k][1]):
            dst[fields[k][0] + t] = at + t
        at += fields[k][1]
    return dst, tuple(new_strides)


def _dst_array(dst_bit):
    dst = np.array([int(b) for b in dst_bit] or [0], dtype=np.int32)
    return dst, len(dst_bit)


def _resolve(shape, strides, dst_bit, perm, order, what):
    """(dst_bit list, strides of the view afterwards) from exactly one of dst_bit / perm / order (none: order=None of relayout_)."""
    if sum(x is not None for x in (dst_bit, perm, order)) > 1:
        raise ValueError(f"{what}: give one of dst_bit, perm and order")
    if dst_bit is not None:
        return [int(b) for b in dst_bit], tuple(int(s) for s in strides)
    if perm is not None:
        return dst_bit_of_perm(shape, strides, perm), tuple(int(s) for s in strides)
    return dst_bit_of_order(shape, strides, order)


def _query(d, dst, n_bits, arrays=False):
    info = _native.ArtnBitpermInfo()
    P = _native.BITPERM_MAX_PASSES
    pass_map = np.full((P, _native.BITPERM_MAX_BITS), -1, dtype=np.int32)
    tiles = np.full((P, 16), -1, dtype=np.int32)
    load, store = np.zeros((P, 16), dtype=np.uint64), np.zeros((P, 16), dtype=np.uint64)
    _native.check(_lib(*_KERNELS, "layout").artn_bitperm_query(
        ctypes.byref(d), _ptr(dst), n_bits, ctypes.byref(info),
        *((_ptr(x) for x in (pass_map, tiles, load, store)) if arrays else (None,) * 4)))
    return info, pass_map, tiles, load, store


def bit_permutation_info(shape, strides, dtype=torch.complex64, perm=None, order=None, dst_bit=None):
    """Host-only: the plan of one bit permutation, given as `perm` (permute_dims_), `order` (relayout_; also when nothing is
    given) or `dst_bit`.  n_bits, dst_bit, passes, line_bits, moved, moved_high (h), table_bytes, lds_bytes, bytes_moved (nominal:
    2 x state x passes), load_degree / store_degree (the worst pass), strides (of the view afterwards) and, per pass, pass_info:
    moved_mask, map (per memory bit, where the pass sends it), tile (the memory bits of the tile, ascending), tb, n_tiles, grid,
    load_degree, store_degree and the LDS columns load_col / store_col (per tile-local bit)."""
    _dtype_code(dtype, "bit_permutation_info")
    dst_list, new_strides = _resolve(shape, strides, dst_bit, perm, order, "bit_permutation_info")
    dst, n_bits = _dst_array(dst_list)
    info, pass_map, tiles, load, store = _query(_desc(shape, strides, dtype), dst, n_bits, arrays=True)
    passes = []
    for p in range(info.passes):
        tb = info.tile_bits[p]
        passes.append({"moved_mask": int(info.moved_mask[p]), "map": tuple(int(b) for b in pass_map[p, :info.n_bits]),
                       "tile": [int(b) for b in tiles[p, :tb]], "tb": tb, "n_tiles": info.n_tiles[p], "grid": info.grid[p],
                       "load_degree": info.load_degree[p], "store_degree": info.store_degree[p],
                       "load_col": [int(c) for c in load[p, :tb]], "store_col": [int(c) for c in store[p, :tb]]})
    return {"n_bits": info.n_bits, "dst_bit": tuple(dst_list), "passes": info.passes, "line_bits": info.line_bits,
            "moved": info.moved, "moved_high": info.moved_high, "table_bytes": info.table_bytes, "lds_bytes": info.lds_bytes,
            "bytes_moved": info.bytes_moved, "load_degree": max([p["load_degree"] for p in passes] or [1]),
            "store_degree": max([p["store_degree"] for p in passes] or [1]), "strides": new_strides, "pass_info": passes}


def _pack(d, dst, n_bits):
    """The permutation's table (include/artn.h) as a uint8 numpy array."""
    return _packed(_query(d, dst, n_bits)[0],
                   lambda *table: _lib(*_KERNELS, "layout").artn_bitperm_pack(ctypes.byref(d), _ptr(dst), n_bits, *table))


class BitPermutation(_Prebuilt):
    """One bit permutation for tensors of one layout, given as `dst_bit`, `perm` (permute_dims_) or `order` (relayout_).
    Validates, plans, packs the table and copies it to `device` once; p(amps) then moves the elements of amps IN PLACE, one launch
    per pass on the current stream, and returns the view that holds the result: amps itself for dst_bit and perm, a new view on
    the same storage with the strides of `order` for order."""

    def __init__(self, shape, strides, dtype, dst_bit=None, device=None, perm=None, order=None):
        self._bind(shape, strides, dtype, "cuda" if device is None else device)
        if dst_bit is None and perm is None and order is None:
            raise ValueError("BitPermutation: give one of dst_bit, perm and order")
        dst_list, self.new_strides = _resolve(self.shape, self.strides, dst_bit, perm, order, "BitPermutation")
        self.dst_bit = tuple(dst_list)
        self._dst, self.n_bits = _dst_array(dst_list)
        self._d = _desc(self.shape, self.strides, dtype)
        table, info = _pack(self._d, self._dst, self.n_bits)
        self.passes, self.table_bytes, self.bytes_moved = info.passes, info.table_bytes, info.bytes_moved
        self._table = None                                     # (the identity holds no table and issues no launch)
        if self.passes:
            self._upload(table)

    def __call__(self, amps):
        what = "layout.BitPermutation"
        self._check(amps, what)
        if self.passes:
            with torch.cuda.device(amps.device):
                _native.check(_lib(*_KERNELS, what).artn_bitperm_apply(ctypes.byref(self._d), amps.data_ptr(), _ptr(self._dst),
                                                                       self.n_bits, self._table.data_ptr(), self.table_bytes,
                                                                       _native.current_stream_ptr(amps.device)))
        if self.new_strides == self.strides:
            return amps
        return torch.as_strided(amps, self.shape, self.new_strides, amps.storage_offset())


def _apply(amps, what, **how):
    _checked(amps, what)
    return BitPermutation(amps.shape, amps.stride(), amps.dtype, device=amps.device, **how)(amps)


def permute_dims_(amps, perm):
    """In place, same shape and strides: afterwards amps == (old amps).permute(perm), element for element.  shape[perm[k]] must
    equal shape[k]; a dim of extent 2^e moves as one field of e bits.  Returns amps.  (Plans and uploads per call: build a
    BitPermutation once to apply the same permutation repeatedly.)"""
    _native.require_gpu(amps, "layout.permute_dims_")
    dst_bit_of_perm(amps.shape, amps.stride(), perm)           # the argument errors come before any device work
    return _apply(amps, "layout.permute_dims_", perm=perm)


def swap_dims_(amps, d0, d1):
    """The transposition of dims d0 and d1, in place: what apply_gate_(SWAP, (d0, d1)) computes, as data movement."""
    _native.require_gpu(amps, "layout.swap_dims_")
    n = amps.dim()
    d0, d1 = int(d0), int(d1)
    if not (-n <= d0 < n and -n <= d1 < n):
        raise ValueError(f"layout.swap_dims_: dims {d0}, {d1} out of range for {n} dims")
    perm = list(range(n))
    perm[d0 % n], perm[d1 % n] = perm[d1 % n], perm[d0 % n]
    return permute_dims_(amps, perm)


def reverse_qubits_(amps, dims=None):
    """The reversal of the listed dims (default: all), in place: the first listed dim trades places with the last one, and so on
    -- the tail of a QFT as one call."""
    _native.require_gpu(amps, "layout.reverse_qubits_")
    n = amps.dim()
    dims = list(range(n)) if dims is None else [int(k) for k in dims]
    if len(set(dims)) != len(dims) or any(not 0 <= k < n for k in dims):
        raise ValueError(f"layout.reverse_qubits_: distinct dims in 0 .. {n - 1} expected, got {dims}")
    perm = list(range(n))
    for k, other in zip(dims, reversed(dims)):
        perm[k] = other
    return permute_dims_(amps, perm)


def relayout_(amps, order=None):
    """Moves the DATA of amps in place and returns a new view t on the same storage with t.shape == amps.shape and t == (old amps)
    element for element, whose dims lie in memory in `order` (slowest first; None: range(dim), so t.is_contiguous()).  Any
    power-of-two extents.  The old view `amps` is STALE afterwards -- it still has its strides and now shows permuted data; this is
    documented, not detected."""
    _native.require_gpu(amps, "layout.relayout_")
    dst_bit_of_order(amps.shape, amps.stride(), order)
    _checked(amps, "layout.relayout_")
    return BitPermutation(amps.shape, amps.stride(), amps.dtype, device=amps.device,
                          order=list(range(amps.dim())) if order is None else order)(amps)


def busiest_dims_order(gates, n_dims):
    """Pure Python: an `order` for relayout_ that puts the dims the circuit gates = [(matrix, dims), ...] targets most often
    fastest in memory (last in the order); ties go by dim, the higher dim faster, as in a contiguous layout."""
    n_dims = int(n_dims)
    count = Counter()
    for _, dims in gates:
        for k in ([int(dims)] if isinstance(dims, (int, np.integer)) else dims):
            k = int(k)
            if not 0 <= k < n_dims:
                raise ValueError(f"layout.busiest_dims_order: dim {k} out of range for {n_dims} dims")
            count[k] += 1
    return sorted(range(n_dims), key=lambda k: (count[k], k))
