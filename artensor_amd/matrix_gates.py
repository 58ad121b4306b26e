"""IN-PLACE dense gates on three to seven qubits of an amplitude tensor on the float64 MATRIX CORES (C ABI: artn_mgate_query,
artn_mgate_pack, artn_mgate_apply), circuits that route every gate to the kernel family that takes it, and gate fusion to a
width of up to seven.

A gate is `(matrix, dims)` as in wide_gates.py: `dims` a tuple of k distinct dims of `amps`, each of extent 2, `matrix` a complex
[2^k, 2^k] array, any matrix; the first listed dim is the most significant digit of the row and column index.  A matrix gate is
ONE launch that reads and writes the state once: the plan, the tiles and the LDS image are the wide gates', the arithmetic is a
complex GEMM per tile on v_mfma_f64_16x16x4_f64.

ARITHMETIC CONTRACT (include/artn.h; a family beside the wide gates, not a change to them).  Every output component is a float64
sum of its 2 * 2^k real products in an order fixed by the plan, rounded once to the dtype.  No atomics: results are bit-identical
from run to run and between an eager call and a graph replay.  Where every product and every partial sum is exactly representable
(integers below 2^53; below 2^24 after the final rounding for complex64) the result is exact whatever the order, so on finite data
identity and signed-permutation matrices reproduce their input values under `==`.  Unlike the wide gates, zero coefficients ARE
multiplied: the sign of a zero is not preserved, and a non-finite element may make its whole group non-finite.  The result is not
bit for bit apply_wide_gate_'s; every component agrees with the exact one within

    2^-24 |exact| (complex64 only) + 4 * 2^k * 2^-53 * sum_c (|Re u| + |Im u|)(|Re x| + |Im x|).

apply_wide_gate_, WideGate, FusedCircuit and fuse_gates are untouched and keep refusing six qubits.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _native
from ._state import _Prebuilt, _checked, _desc, _dims, _dtype_code, _interleaved, _lib, _packed, _ptr
from .gates import GateCircuit, _matrix
from .wide_gates import WideGate, _fuse, _width

__all__ = ["apply_matrix_gate_", "MatrixGate", "matrix_gate_info", "BlockCircuit", "apply_blocks_", "fuse_gates_wide"]


def _split_gate(matrix, dims, n_dims, what):
    """(k, int32 dims [k], float64 mat [2 * 4^k]); a k the library does not take keeps a zero matrix, so that the library refuses it."""
    dims = _dims(dims, n_dims)
    k = int(dims.shape[0])
    if not _native.MGATE_MIN_K <= k <= _native.MGATE_MAX_K:
        return k, (dims if k else np.zeros(1, dtype=np.int32)), np.zeros(2, dtype=np.float64)
    return k, dims, _interleaved(_matrix(matrix, k, what))


def _mgate_query(d, k, dims, mat, arrays=False, what="matrix_gates"):
    info = _native.ArtnMgateInfo()
    target, tile = np.full(_native.MGATE_MAX_K, -1, dtype=np.int32), np.full(12, -1, dtype=np.int32)
    _native.check(_lib("artn_mgate_apply", "matrix gates", what).artn_mgate_query(
        ctypes.byref(d), k, _ptr(dims), _ptr(mat), ctypes.byref(info), _ptr(target) if arrays else None, _ptr(tile) if arrays else None))
    return info, target, tile


def matrix_gate_info(shape, strides, matrix, dims, dtype=torch.complex64):
    """Host-only: the plan of one gate, the keys of wide_gate_info (table_bytes = 544 + 16 * 4^k)."""
    _dtype_code(dtype, "matrix_gate_info")
    k, dims, mat = _split_gate(matrix, dims, len(shape), "matrix_gate_info")
    info, target, tile = _mgate_query(_desc(shape, strides, dtype), k, dims, mat, arrays=True, what="matrix_gate_info")
    return {"k": info.k, "target_bits": tuple(int(b) for b in target[:k]), "tile_bits": [int(b) for b in tile[:info.tile_bits]],
            "tb": info.tile_bits, "n_tiles": info.n_tiles, "segment": info.segment, "lds_bytes": info.lds_bytes,
            "table_bytes": info.table_bytes, "bytes_read": info.bytes_read, "bytes_written": info.bytes_written,
            "diagonal": bool(info.diagonal)}


def _mgate_pack(d, k, dims, mat):
    """The gate's table (include/artn.h) as a uint8 numpy array."""
    return _packed(_mgate_query(d, k, dims, mat)[0],
                   lambda *table: _native.lib().artn_mgate_pack(ctypes.byref(d), k, _ptr(dims), _ptr(mat), *table))


class MatrixGate(_Prebuilt):
    """One gate (matrix, dims), k = len(dims) in 3..7, for tensors of one layout.  Validates, plans, packs the table and copies it
    to `device` once; g(amps) then updates amps IN PLACE with one launch and returns it."""

    def __init__(self, shape, strides, dtype, matrix, dims, device):
        self._bind(shape, strides, dtype, device)
        self.k, self._dims, mat = _split_gate(matrix, dims, len(self.shape), "MatrixGate")
        self._d = _desc(self.shape, self.strides, dtype)
        table, info = _mgate_pack(self._d, self.k, self._dims, mat)
        self.table_bytes, self.tile_bits, self.n_tiles = info.table_bytes, info.tile_bits, info.n_tiles
        self._upload(table)

    def __call__(self, amps):
        self._check(amps, "matrix_gates.MatrixGate")
        with torch.cuda.device(amps.device):
            _native.check(_native.lib().artn_mgate_apply(ctypes.byref(self._d), amps.data_ptr(), self.k, _ptr(self._dims),
                                                         self._table.data_ptr(), self.table_bytes,
                                                         _native.current_stream_ptr(amps.device)))
        return amps


def apply_matrix_gate_(amps, matrix, dims):
    """amps <- U amps for one gate on len(dims) = 3..7 dims, in place, on the matrix cores: one launch, no second buffer; returns
    amps.  (Plans and uploads per call: build a MatrixGate once to apply the same gate repeatedly.)"""
    _checked(amps, "matrix_gates.apply_matrix_gate_")
    return MatrixGate(amps.shape, amps.stride(), amps.dtype, matrix, dims, amps.device)(amps)


class BlockCircuit(_Prebuilt):
    """An ordered list of gates [(matrix, dims), ...] of ANY width 1..7 for tensors of one layout.  The list is cut, in order and
    never reordered, into maximal stretches of gates on one or two dims -- each ONE GateCircuit with the given max_rank -- and
    single wider gates: a MatrixGate when its width is at least `mfma_from` (3..8; 8 = never), a WideGate otherwise.  The default
    6 sends to the matrix cores only what has no other route, so a list with no gate wider than five is FusedCircuit bit for
    bit.  A gate of width 6 or 7 below mfma_from has no route: ValueError.  n_launches is the sum of the stretches' runs plus
    the number of wider gates."""

    def __init__(self, shape, strides, dtype, gates, device, max_rank=None, mfma_from=6):
        self._bind(shape, strides, dtype, device)
        if isinstance(mfma_from, bool) or not isinstance(mfma_from, (int, np.integer)) or not 3 <= int(mfma_from) <= 8:
            raise ValueError(f"BlockCircuit: mfma_from must be an integer in 3..8 (8: never), got {mfma_from!r}")
        self.mfma_from = int(mfma_from)
        gates = list(gates)
        if not gates:
            raise ValueError("at least one gate is needed")
        widths = [_width(gate, g) for g, gate in enumerate(gates)]
        for g, w in enumerate(widths):
            if w > _native.MGATE_MAX_K:
                raise ValueError(f"gate {g}: one to {_native.MGATE_MAX_K} dims expected, got {w}")
            if _native.WGATE_MAX_K < w < self.mfma_from:
                raise ValueError(f"gate {g}: a gate on {w} dims runs on the matrix cores only, and mfma_from is {self.mfma_from}")
        self.parts, stretch = [], []
        for gate, w in zip(gates, widths):
            if w <= 2:
                stretch.append(gate)
                continue
            if stretch:
                self.parts.append(GateCircuit(self.shape, self.strides, dtype, stretch, self.device, max_rank))
                stretch = []
            kind = MatrixGate if w >= self.mfma_from else WideGate
            self.parts.append(kind(self.shape, self.strides, dtype, gate[0], gate[1], self.device))
        if stretch:
            self.parts.append(GateCircuit(self.shape, self.strides, dtype, stretch, self.device, max_rank))
        self.n_gates = len(gates)
        self.n_matrix = sum(isinstance(p, MatrixGate) for p in self.parts)
        self.n_wide = sum(isinstance(p, WideGate) for p in self.parts)
        self.n_launches = sum(p.n_runs if isinstance(p, GateCircuit) else 1 for p in self.parts)
        self.table_bytes = sum(p.table_bytes for p in self.parts)

    def __call__(self, amps):
        self.parts[0]._check(amps, "matrix_gates.BlockCircuit")  # (no table of its own: a part has its layout, and a table)
        for part in self.parts:
            part(amps)
        return amps


def apply_blocks_(amps, gates, max_rank=None, mfma_from=6):
    """The circuit `gates` (see BlockCircuit; widths 1..7) applied to amps in place; returns amps.  Every call plans, packs and
    uploads again: build a BlockCircuit once to apply the same circuit repeatedly."""
    _checked(amps, "matrix_gates.apply_blocks_")
    return BlockCircuit(amps.shape, amps.stride(), amps.dtype, gates, amps.device, max_rank, mfma_from)(amps)


def fuse_gates_wide(gates, max_width):
    """fuse_gates (wide_gates.py: the same walk, the same order of the products, the same ascending dims) with the limit lifted:
    max_width in 2..7, gates of up to seven qubits.  For max_width <= 5 and gates of at most five qubits the result is
    fuse_gates' own.  Blocks wider than five run through BlockCircuit."""
    return _fuse(gates, max_width, _native.MGATE_MAX_K, "fuse_gates_wide")
