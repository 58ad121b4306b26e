"""IN-PLACE dense gates under any number of control qubits and under classical conditions held in device memory (C ABI:
artn_cgate_query, artn_cgate_pack, artn_cgate_apply).

A controlled gate is `(matrix, targets, controls, control_values)`: `matrix` any complex [2^t, 2^t] array on the t = 1..5 dims
`targets` (the first listed dim the most significant digit, as in gates.py and wide_gates.py), `controls` any number of further
dims of extent 2, `control_values` the digit each control must have (default: all 1; an int is read with its most significant
digit on the first listed control).  The elements whose control digits match get exactly the arithmetic of apply_wide_gate_
for `matrix` on `targets`; every other element keeps its bits, and the elements that differ in a control at or above a 128-byte
line are neither read nor written (include/artn.h has the contract and the plan).  ONE launch per call.

A classical condition `when(outcome, equals, mask=None)` names an int64 in device memory -- what measure_ / reset_ return with
device=True, the record of measure.collapse_, or any int64 GPU tensor -- and the gate is applied iff o >= 0 and (o & mask) ==
equals.  The kernel reads the value; the host never does, so a measure-then-correct sequence is enqueued without a
synchronisation.  There is no CPU fallback.
"""
import cmath
import ctypes

import numpy as np
import torch

from . import _native
from ._state import _Prebuilt, _checked, _desc, _dims, _dtype_code, _interleaved, _lib, _packed, _ptr
from .gates import _matrix

__all__ = ["apply_controlled_gate_", "ControlledGate", "controlled_gate_info", "mcx_", "mcz_", "mcphase_", "when", "Condition"]

_KERNELS = ("artn_cgate_apply", "controlled-gate kernels")     # what _lib looks for, and what it calls them


class Condition:
    """What when() returns: the tensor that holds the int64, the mask and the value.  (o & mask) == equals and o >= 0 applies."""

    def __init__(self, tensor, mask, equals):
        self.tensor, self.mask, self.equals = tensor, mask, equals

    def __repr__(self):
        return f"Condition(mask={self.mask:#x}, equals={self.equals:#x}, device={self.tensor.device})"


def when(outcome, equals, mask=None):
    """A classical condition for `condition=`: apply iff o >= 0 and (o & mask) == equals, o the int64 in the first 8 bytes of the
    GPU tensor `outcome` (a 0-dim or larger int64 tensor, or the 4-element float64 record of measure.collapse_).  mask=None: all
    bits.  Validates on the host only; the tensor is never read here."""
    what = "controlled.when"
    if not isinstance(outcome, torch.Tensor):
        raise TypeError(f"{what}: a GPU tensor expected, got {type(outcome).__name__}")
    if not outcome.is_cuda:
        raise RuntimeError(f"{what}: the outcome must live on the GPU (got a {outcome.device} tensor); there is no CPU fallback")
    if outcome.dtype == torch.float64:
        if outcome.numel() != _native.MEASURE_RECORD_BYTES // 8 or not outcome.is_contiguous():
            raise TypeError(f"{what}: a float64 outcome is the 4-element record of measure.collapse_, got {tuple(outcome.shape)}")
    elif outcome.dtype != torch.int64:
        raise TypeError(f"{what}: an int64 tensor (or the float64 record of measure.collapse_) expected, got {outcome.dtype}")
    if outcome.numel() < 1:
        raise ValueError(f"{what}: the outcome tensor has no element")
    if outcome.data_ptr() % 8:
        raise ValueError(f"{what}: the outcome must start on an 8-byte boundary")
    for name, v in (("equals", equals), ("mask", mask)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise TypeError(f"{what}: {name} must be an integer, got {v!r}")
    equals = int(equals)
    if not 0 <= equals < 2 ** 63:
        raise ValueError(f"{what}: equals must lie in 0 .. 2^63 - 1, got {equals}")
    if mask is None:
        mask = -1
    else:
        mask = int(mask)
        if not 0 <= mask < 2 ** 63:
            raise ValueError(f"{what}: mask must lie in 0 .. 2^63 - 1, got {mask}")
        if equals & ~mask:
            raise ValueError(f"{what}: equals {equals:#x} has bits outside mask {mask:#x}: the condition could never hold")
    return Condition(outcome, mask, equals)


def _control_values(control_values, c, what):
    if control_values is None:
        return np.ones(max(c, 1), dtype=np.int32)
    if isinstance(control_values, (int, np.integer)) and not isinstance(control_values, bool):
        v = int(control_values)
        if not 0 <= v < 2 ** c:
            raise ValueError(f"{what}: control_values {v} does not fit {c} controls (0 .. {2 ** c - 1} expected)")
        values = [(v >> (c - 1 - j)) & 1 for j in range(c)]          # the most significant digit on the first listed control
    else:
        values = [int(x) for x in control_values]
        if len(values) != c:
            raise ValueError(f"{what}: {len(values)} control_values for {c} controls")
        if any(x not in (0, 1) for x in values):
            raise ValueError(f"{what}: control_values are 0 or 1, got {values}")
    return np.array(values + [0] * (c == 0), dtype=np.int32)


def _split_dims(targets, controls, control_values, n_dims, what):
    """(t, int32 targets, c, int32 controls, int32 values): the arrays have one entry where there is no target or no control."""
    targets = _dims(targets, n_dims)
    controls = _dims(() if controls is None else controls, n_dims)
    t, c = int(targets.shape[0]), int(controls.shape[0])
    both = sorted(set(int(x) for x in targets) & set(int(x) for x in controls))
    if both:
        raise ValueError(f"{what}: dims {both} are listed as targets and as controls")
    values = _control_values(control_values, c, what)
    return t, (targets if t else np.zeros(1, dtype=np.int32)), c, (controls if c else np.zeros(1, dtype=np.int32)), values


def _split(matrix, targets, controls, control_values, n_dims, what):
    """(t, int32 targets, c, int32 controls, int32 values, float64 mat [2 * 4^t]); a t the library does not take keeps a zero
    matrix, so that the library refuses it."""
    t, targets, c, controls, values = _split_dims(targets, controls, control_values, n_dims, what)
    if not 1 <= t <= _native.WGATE_MAX_K:
        return t, targets, c, controls, values, np.zeros(2, dtype=np.float64)
    return t, targets, c, controls, values, _interleaved(_matrix(matrix, t, what))


def _cgate_query(d, t, targets, c, controls, values, mat, arrays=False):
    info = _native.ArtnCgateInfo()
    target, control, tile = (np.full(n, -1, dtype=np.int32) for n in (_native.WGATE_MAX_K, max(c, 1), 12))
    _native.check(_lib(*_KERNELS, "controlled").artn_cgate_query(
        ctypes.byref(d), t, _ptr(targets), c, _ptr(controls), _ptr(values), _ptr(mat), ctypes.byref(info),
        _ptr(target) if arrays else None, _ptr(control) if arrays else None, _ptr(tile) if arrays else None))
    return info, target, control, tile


def controlled_gate_info(shape, strides, matrix, targets, controls, control_values=None, dtype=torch.complex64):
    """Host-only: the plan of one controlled gate.  t, c, c_high / c_low (controls at or above / below a 128-byte line),
    target_bits and control_bits (memory bits in the order listed), control_values, tile_bits (ascending), tb, n_selected
    (elements the gate acts on), n_tiles, segment, lds_bytes, table_bytes, bytes_read = bytes_written = the bytes of the
    elements whose high controls match, diagonal."""
    _dtype_code(dtype, "controlled_gate_info")
    t, targets, c, controls, values, mat = _split(matrix, targets, controls, control_values, len(shape), "controlled_gate_info")
    info, target, control, tile = _cgate_query(_desc(shape, strides, dtype), t, targets, c, controls, values, mat, arrays=True)
    return {"t": info.t, "c": info.c, "c_high": info.c_high, "c_low": info.c_low,
            "target_bits": tuple(int(b) for b in target[:t]), "control_bits": tuple(int(b) for b in control[:c]),
            "control_values": tuple(int(v) for v in values[:c]), "tile_bits": [int(b) for b in tile[:info.tile_bits]],
            "tb": info.tile_bits, "n_selected": info.n_selected, "n_tiles": info.n_tiles, "segment": info.segment,
            "lds_bytes": info.lds_bytes, "table_bytes": info.table_bytes, "bytes_read": info.bytes_read,
            "bytes_written": info.bytes_written, "diagonal": bool(info.diagonal)}


def _cgate_pack(d, t, targets, c, controls, values, mat):
    """The gate's table (include/artn.h) as a uint8 numpy array."""
    return _packed(_cgate_query(d, t, targets, c, controls, values, mat)[0],
                   lambda *table: _lib(*_KERNELS, "controlled").artn_cgate_pack(ctypes.byref(d), t, _ptr(targets), c, _ptr(controls),
                                                                                _ptr(values), _ptr(mat), *table))


class ControlledGate(_Prebuilt):
    """One controlled gate for tensors of one layout.  Validates, plans, packs the table and copies it to `device` once;
    g(amps, condition=None) then updates amps IN PLACE with one launch and returns it.  The condition belongs to the call, not
    to the table: one ControlledGate serves any condition."""

    def __init__(self, shape, strides, dtype, matrix, targets, controls, device, control_values=None):
        self._bind(shape, strides, dtype, device)
        self.t, self._targets, self.c, self._controls, self._values, mat = _split(matrix, targets, controls, control_values,
                                                                                  len(self.shape), "ControlledGate")
        self._d = _desc(self.shape, self.strides, dtype)
        table, info = _cgate_pack(self._d, self.t, self._targets, self.c, self._controls, self._values, mat)
        self.table_bytes, self.tile_bits, self.n_tiles = info.table_bytes, info.tile_bits, info.n_tiles
        self.c_high, self.c_low = info.c_high, info.c_low
        self._upload(table)

    def __call__(self, amps, condition=None):
        what = "controlled.ControlledGate"
        self._check(amps, what)
        cond, mask, equals = None, 0, 0
        if condition is not None:
            if not isinstance(condition, Condition):
                raise TypeError(f"{what}: condition is what when(outcome, equals, mask) returns, got {type(condition).__name__}")
            if condition.tensor.device != amps.device:
                raise ValueError(f"{what}: the condition lives on {condition.tensor.device}, the amplitudes on {amps.device}")
            cond, mask, equals = condition.tensor.data_ptr(), condition.mask, condition.equals
        with torch.cuda.device(amps.device):
            _native.check(_lib(*_KERNELS, what).artn_cgate_apply(
                ctypes.byref(self._d), amps.data_ptr(), self.t, _ptr(self._targets), self.c, _ptr(self._controls), _ptr(self._values),
                self._table.data_ptr(), self.table_bytes, cond, mask, equals, _native.current_stream_ptr(amps.device)))
        return amps


def apply_controlled_gate_(amps, matrix, targets, controls, control_values=None, condition=None):
    """amps <- the gate `matrix` on `targets` where the `controls` have `control_values`, under `condition`, in place: one
    launch, no second buffer; returns amps.  (Plans and uploads per call: build a ControlledGate once to apply the same gate
    repeatedly.)"""
    if isinstance(amps, torch.Tensor):                        # the argument errors come before any device work
        _split(matrix, targets, controls, control_values, amps.dim(), "controlled.apply_controlled_gate_")
    _checked(amps, "controlled.apply_controlled_gate_")
    if condition is not None and not isinstance(condition, Condition):
        raise TypeError(f"controlled.apply_controlled_gate_: condition is what when(outcome, equals, mask) returns, got {type(condition).__name__}")
    return ControlledGate(amps.shape, amps.stride(), amps.dtype, matrix, targets, controls, amps.device, control_values)(amps, condition)


_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)


def mcx_(amps, controls, target, condition=None):
    """X on `target` where every control is 1 (no controls: X), in place."""
    return apply_controlled_gate_(amps, _X, (target,), controls, None, condition)


def _last_is_target(dims, what):
    dims = [int(dims)] if isinstance(dims, (int, np.integer)) else [int(x) for x in dims]
    if not dims:
        raise ValueError(f"{what}: at least one dim expected")
    return dims[-1:], dims[:-1]


def mcz_(amps, dims, condition=None):
    """-1 on the elements whose listed digits are all 1 (the last listed dim is the target, the others are controls), in place."""
    target, controls = _last_is_target(dims, "controlled.mcz_")
    return apply_controlled_gate_(amps, np.diag([1.0, -1.0]), target, controls, None, condition)


def mcphase_(amps, dims, phi, condition=None):
    """e^{i phi} on the elements whose listed digits are all 1, in place."""
    target, controls = _last_is_target(dims, "controlled.mcphase_")
    return apply_controlled_gate_(amps, np.diag([1.0, cmath.exp(1j * float(phi))]), target, controls, None, condition)
