"""IN-PLACE dense gates on one to five qubits of an amplitude tensor on the device (C ABI: artn_wgate_query, artn_wgate_pack,
artn_wgate_apply), circuits that mix them with the one- and two-qubit runs of gates.py, and gate fusion to a width.

A gate is `(matrix, dims)` as in gates.py: `dims` a tuple of k distinct dims of `amps`, each of extent 2 (negative dims count from
the end), `matrix` anything np.asarray turns into a complex [2^k, 2^k] array (or [2] * 2k, reshaped) -- any matrix, unitary or
not; the first listed dim is the most significant digit of the row and column index:

    new[.., i0, .., i_{k-1}, ..] = sum_j U[(i0 .. i_{k-1})_2, (j0 .. j_{k-1})_2] a[.., j0, .., j_{k-1}, ..]

A wide gate is ONE launch that reads and writes the state once, whatever its width and wherever its targets lie.  It keeps the
arithmetic contract of gates.py stated for any k (include/artn.h), so a one- or two-qubit gate through apply_wide_gate_ is
apply_gate_ bit for bit.  apply_gate_, apply_gates_ and GateCircuit are untouched and keep refusing k = 3.  There is no CPU
fallback.
"""
import ctypes

import numpy as np
import torch

from . import _native
from ._state import _Prebuilt, _checked, _desc, _dims, _dtype_code, _interleaved, _lib, _packed, _ptr
from .gates import GateCircuit, _matrix

__all__ = ["apply_wide_gate_", "WideGate", "wide_gate_info", "FusedCircuit", "apply_circuit_", "fuse_gates"]


class _DenseGate(_Prebuilt):
    """One gate (matrix, dims) of a dense-gate family, for tensors of one layout: validates, plans, packs the table and copies it
    to `device` once; g(amps) then updates amps IN PLACE with one launch and returns it.  A family (WideGate here, MatrixGate in
    matrix_gates.py) declares `_prefix` (its entries are <prefix>_query, _pack, _apply), `_k_min` and `_k_max`, `_name` (the
    module-qualified name in messages) and `_family`: None, or what the refusal of a library built before the family calls it."""

    _prefix = _name = _family = None
    _k_min = _k_max = 0

    def __init__(self, shape, strides, dtype, matrix, dims, device):
        self._bind(shape, strides, dtype, device)
        self.k, self._dims, mat = self._split(matrix, dims, len(self.shape), type(self).__name__)
        self._d = _desc(self.shape, self.strides, dtype)
        table, info = self._pack(self._d, self.k, self._dims, mat)
        self.table_bytes, self.tile_bits, self.n_tiles = info.table_bytes, info.tile_bits, info.n_tiles
        self._upload(table)

    def __call__(self, amps):
        self._check(amps, self._name)
        with torch.cuda.device(amps.device):
            _native.check(getattr(_native.lib(), self._prefix + "_apply")(
                ctypes.byref(self._d), amps.data_ptr(), self.k, _ptr(self._dims), self._table.data_ptr(), self.table_bytes,
                _native.current_stream_ptr(amps.device)))
        return amps

    @classmethod
    def _split(cls, matrix, dims, n_dims, what):
        """(k, int32 dims [k], float64 mat [2 * 4^k]); a k the library does not take keeps a zero matrix, so that the library refuses it."""
        dims = _dims(dims, n_dims)
        k = int(dims.shape[0])
        if not cls._k_min <= k <= cls._k_max:
            return k, (dims if k else np.zeros(1, dtype=np.int32)), np.zeros(2, dtype=np.float64)
        return k, dims, _interleaved(_matrix(matrix, k, what))

    @classmethod
    def _query(cls, d, k, dims, mat, arrays=False, what=None):
        lib = _lib(cls._prefix + "_apply", cls._family, what or cls._name.split(".")[0]) if cls._family else _native.lib()
        info = _native.ArtnWgateInfo()
        target, tile = np.full(cls._k_max, -1, dtype=np.int32), np.full(12, -1, dtype=np.int32)
        _native.check(getattr(lib, cls._prefix + "_query")(ctypes.byref(d), k, _ptr(dims), _ptr(mat), ctypes.byref(info),
                                                           _ptr(target) if arrays else None, _ptr(tile) if arrays else None))
        return info, target, tile

    @classmethod
    def _info(cls, shape, strides, matrix, dims, dtype, what):
        _dtype_code(dtype, what)
        k, dims, mat = cls._split(matrix, dims, len(shape), what)
        info, target, tile = cls._query(_desc(shape, strides, dtype), k, dims, mat, arrays=True, what=what)
        return {"k": info.k, "target_bits": tuple(int(b) for b in target[:k]), "tile_bits": [int(b) for b in tile[:info.tile_bits]],
                "tb": info.tile_bits, "n_tiles": info.n_tiles, "segment": info.segment, "lds_bytes": info.lds_bytes,
                "table_bytes": info.table_bytes, "bytes_read": info.bytes_read, "bytes_written": info.bytes_written,
                "diagonal": bool(info.diagonal)}

    @classmethod
    def _pack(cls, d, k, dims, mat):
        """The gate's table (include/artn.h) as a uint8 numpy array."""
        return _packed(cls._query(d, k, dims, mat)[0],
                       lambda *table: getattr(_native.lib(), cls._prefix + "_pack")(ctypes.byref(d), k, _ptr(dims), _ptr(mat), *table))


class WideGate(_DenseGate):
    """One gate (matrix, dims), k = len(dims) in 1..5, for tensors of one layout.  Validates, plans, packs the table and copies it
    to `device` once; g(amps) then updates amps IN PLACE with one launch and returns it."""

    _prefix, _name = "artn_wgate", "wide_gates.WideGate"
    _k_min, _k_max = 1, _native.WGATE_MAX_K


_split_gate, _wgate_query, _wgate_pack = WideGate._split, WideGate._query, WideGate._pack


def wide_gate_info(shape, strides, matrix, dims, dtype=torch.complex64):
    """Host-only: the plan of one gate.  target_bits (the memory bits of dims, in the order listed), tile_bits (ascending: the
    targets and the lowest other memory bits), tb (their number: 12 for complex64, 11 for complex128, or log2 of a smaller
    state), n_tiles, segment (elements of a contiguous piece of a tile), lds_bytes, table_bytes, bytes_read = bytes_written =
    bytes of the state, diagonal."""
    return WideGate._info(shape, strides, matrix, dims, dtype, "wide_gate_info")


def apply_wide_gate_(amps, matrix, dims):
    """amps <- U amps for one gate on len(dims) = 1..5 dims, in place: one launch, no second buffer; returns amps.  (Plans and
    uploads per call: build a WideGate once to apply the same gate repeatedly.)"""
    _checked(amps, "wide_gates.apply_wide_gate_")
    return WideGate(amps.shape, amps.stride(), amps.dtype, matrix, dims, amps.device)(amps)


def _width(gate, g):
    if not isinstance(gate, (tuple, list)) or len(gate) != 2:
        raise ValueError(f"gate {g}: (matrix, dims) expected, got {gate!r}")
    return 1 if isinstance(gate[1], (int, np.integer)) else len(gate[1])


class _PartsCircuit(_Prebuilt):
    """A gate list cut into `parts` that are applied in order; a class declares `_name`, the module-qualified name in messages."""

    _name = None

    def _cut(self, dtype, gates, max_rank, narrow, wider):
        """The list cut, in order and never reordered, into maximal stretches of gates on one or two dims -- each ONE
        narrow(..., stretch, device, max_rank) -- and single wider gates, each one wider(width)(..., matrix, dims, device);
        `wider` may raise.  Sets parts, n_gates, n_launches and table_bytes."""
        gates = list(gates)
        if not gates:
            raise ValueError("at least one gate is needed")
        self.parts, stretch = [], []
        for g, gate in enumerate(gates):
            width = _width(gate, g)
            if width <= 2:
                stretch.append(gate)
                continue
            if stretch:
                self.parts.append(narrow(self.shape, self.strides, dtype, stretch, self.device, max_rank))
                stretch = []
            self.parts.append(wider(width)(self.shape, self.strides, dtype, gate[0], gate[1], self.device))
        if stretch:
            self.parts.append(narrow(self.shape, self.strides, dtype, stretch, self.device, max_rank))
        self.n_gates = len(gates)
        self.n_launches = sum(p.n_runs if isinstance(p, narrow) else 1 for p in self.parts)
        self.table_bytes = sum(p.table_bytes for p in self.parts)

    def __call__(self, amps):
        self.parts[0]._check(amps, self._name)                 # (no table of its own: a part has its layout, and a table)
        for part in self.parts:
            part(amps)
        return amps


class FusedCircuit(_PartsCircuit):
    """An ordered list of gates [(matrix, dims), ...] of ANY width 1..5 for tensors of one layout.  The list is cut, in order,
    into maximal stretches of gates on one or two dims -- each ONE GateCircuit with the given max_rank -- and single gates on
    three to five dims -- each one WideGate; gates are never reordered, and wide gates are not fused into LDS runs.  A circuit
    of narrow gates only is therefore apply_gates_ bit for bit.  circ(amps) updates amps IN PLACE and returns it; n_launches is
    the sum of the stretches' runs plus the number of wide gates."""

    _name = "wide_gates.FusedCircuit"

    def __init__(self, shape, strides, dtype, gates, device, max_rank=None):
        self._bind(shape, strides, dtype, device)
        self._cut(dtype, gates, max_rank, GateCircuit, lambda width: WideGate)      # (the library refuses a width above five)
        self.n_wide = sum(isinstance(p, WideGate) for p in self.parts)


def apply_circuit_(amps, gates, max_rank=None):
    """The circuit `gates` (see FusedCircuit; widths 1..5) applied to amps in place; returns amps.  Every call plans, packs and
    uploads again: build a FusedCircuit once to apply the same circuit repeatedly."""
    _checked(amps, "wide_gates.apply_circuit_")
    return FusedCircuit(amps.shape, amps.stride(), amps.dtype, gates, amps.device, max_rank)(amps)


def _embed(m, dims, into):
    """The matrix m on `dims` as a matrix on the qubits `into` (a superset), the first of `into` the most significant digit."""
    w, k = len(into), len(dims)
    axes = [into.index(q) for q in dims]
    u = np.eye(2 ** w, dtype=np.complex128).reshape((2,) * w + (2 ** w,))
    u = np.moveaxis(np.tensordot(m.reshape((2,) * (2 * k)), u, axes=(list(range(k, 2 * k)), axes)), list(range(k)), axes)
    return u.reshape(2 ** w, 2 ** w)


def fuse_gates(gates, max_width):
    """Opt-in, pure Python: a shorter list of gates on up to max_width (2..5, required) qubits with the same product.  The gates
    are walked in order; a BLOCK (matrix, qubits) is OPEN while it is the last block on every one of its qubits.  A gate whose
    qubits' last blocks are all open, and cover together with the gate at most max_width qubits, replaces them by one block at
    its own position: open blocks commute past everything between them and the gate.  Its matrix is the gate times the
    kron-embedded blocks in their original order, formed in complex128; its dims are in ascending order.  Any other gate starts
    a block of its own (a gate wider than max_width, up to 5, stays as it is).  This changes rounding (fewer, different
    matrices), so nothing calls it implicitly; the result is deterministic."""
    return _fuse(gates, max_width, _native.WGATE_MAX_K, "fuse_gates")


def _fuse(gates, max_width, top, who):
    """fuse_gates for gates and blocks of up to `top` qubits (matrix_gates.fuse_gates_wide lifts the limit to 7)."""
    if isinstance(max_width, bool) or not isinstance(max_width, (int, np.integer)) or not 2 <= int(max_width) <= top:
        raise ValueError(f"{who}: max_width must be an integer in 2..{top}, got {max_width!r}")
    max_width = int(max_width)
    out, last = [], {}                                         # out: [matrix, qubits] or None (joined); last[q]: index into out
    for g, gate in enumerate(gates):
        k = _width(gate, g)
        dims = (int(gate[1]),) if isinstance(gate[1], (int, np.integer)) else tuple(int(x) for x in gate[1])
        if not 1 <= k <= top or len(set(dims)) != k:
            raise ValueError(f"gate {g}: one to {top} distinct dims expected, got {dims}")
        m = _matrix(gate[0], k, f"gate {g}")
        before = sorted({last[q] for q in dims if q in last})
        is_open = all(all(last[q] == b for q in out[b][1]) for b in before)
        union = tuple(sorted(set(dims).union(*(out[b][1] for b in before))))
        if is_open and len(union) <= max_width:
            m = _embed(m, dims, union)
            for b in before[::-1]:                             # the gate, then the blocks from the last to the first
                m = m @ _embed(out[b][0], out[b][1], union)
                out[b] = None
            dims = union
        out.append([m, dims])
        for q in dims:
            last[q] = len(out) - 1
    return [(m, d) for m, d in (x for x in out if x is not None)]
