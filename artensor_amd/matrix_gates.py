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
import numpy as np
import torch

from . import _native
from ._state import _checked, _desc
from .gates import GateCircuit
from .wide_gates import WideGate, _DenseGate, _fuse, _PartsCircuit, _width

__all__ = ["apply_matrix_gate_", "MatrixGate", "matrix_gate_info", "BlockCircuit", "apply_blocks_", "fuse_gates_wide"]


class MatrixGate(_DenseGate):
    """One gate (matrix, dims), k = len(dims) in 3..7, for tensors of one layout.  Validates, plans, packs the table and copies it
    to `device` once; g(amps) then updates amps IN PLACE with one launch and returns it."""

    _prefix, _name, _family = "artn_mgate", "matrix_gates.MatrixGate", "matrix gates"
    _k_min, _k_max = _native.MGATE_MIN_K, _native.MGATE_MAX_K


_split_gate, _mgate_query, _mgate_pack = MatrixGate._split, MatrixGate._query, MatrixGate._pack


def matrix_gate_info(shape, strides, matrix, dims, dtype=torch.complex64):
    """Host-only: the plan of one gate, the keys of wide_gate_info (table_bytes = 544 + 16 * 4^k)."""
    return MatrixGate._info(shape, strides, matrix, dims, dtype, "matrix_gate_info")


def apply_matrix_gate_(amps, matrix, dims):
    """amps <- U amps for one gate on len(dims) = 3..7 dims, in place, on the matrix cores: one launch, no second buffer; returns
    amps.  (Plans and uploads per call: build a MatrixGate once to apply the same gate repeatedly.)"""
    _checked(amps, "matrix_gates.apply_matrix_gate_")
    return MatrixGate(amps.shape, amps.stride(), amps.dtype, matrix, dims, amps.device)(amps)


class BlockCircuit(_PartsCircuit):
    """An ordered list of gates [(matrix, dims), ...] of ANY width 1..7 for tensors of one layout.  The list is cut, in order and
    never reordered, into maximal stretches of gates on one or two dims -- each ONE GateCircuit with the given max_rank -- and
    single wider gates: a MatrixGate when its width is at least `mfma_from` (3..8; 8 = never), a WideGate otherwise.  The default
    6 sends to the matrix cores only what has no other route, so a list with no gate wider than five is FusedCircuit bit for
    bit.  A gate of width 6 or 7 below mfma_from has no route: ValueError.  n_launches is the sum of the stretches' runs plus
    the number of wider gates."""

    _name = "matrix_gates.BlockCircuit"

    def __init__(self, shape, strides, dtype, gates, device, max_rank=None, mfma_from=6):
        self._bind(shape, strides, dtype, device)
        if isinstance(mfma_from, bool) or not isinstance(mfma_from, (int, np.integer)) or not 3 <= int(mfma_from) <= 8:
            raise ValueError(f"BlockCircuit: mfma_from must be an integer in 3..8 (8: never), got {mfma_from!r}")
        self.mfma_from = int(mfma_from)
        gates = list(gates)
        for g, gate in enumerate(gates):                           # every refusal comes before anything is built
            w = _width(gate, g)
            if w > _native.MGATE_MAX_K:
                raise ValueError(f"gate {g}: one to {_native.MGATE_MAX_K} dims expected, got {w}")
            if _native.WGATE_MAX_K < w < self.mfma_from:
                raise ValueError(f"gate {g}: a gate on {w} dims runs on the matrix cores only, and mfma_from is {self.mfma_from}")
        self._cut(dtype, gates, max_rank, GateCircuit, lambda width: MatrixGate if width >= self.mfma_from else WideGate)
        self.n_matrix = sum(isinstance(p, MatrixGate) for p in self.parts)
        self.n_wide = sum(isinstance(p, WideGate) for p in self.parts)


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
