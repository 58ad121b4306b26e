"""Batched quantum trajectories: B states in ONE tensor, measured, reset and sent through noise channels with a draw PER STATE,
in place (C ABI: artn_measure_batch_query / _choose / _collapse, artn_channel_batch_query / _pack / _choose / _apply).

`batch_dims` are distinct dims of `amps` of any power-of-two extent, disjoint from the measured or target dims.  Trajectory b is
the mixed-radix integer of their digits, the first listed dim the most significant; B is the product of their extents.
Uniforms, outcomes, probabilities and records are row b of a device tensor.  The batch dims are spectators of every unitary
operation (GateCircuit, WideGate, MatrixGate, PauliCircuit, DiagonalOperator ...): those apply to all trajectories at once as
they are.  Here every trajectory gets its own outcome or Kraus operator:

    measure_batch_     draws o[b] from q[b, :] = marginal_probabilities(amps, batch_dims + dims)[b] and uniforms[b] by the rule of
                       measure_, collapses slice b onto it
    postselect_batch_  the same with the outcomes given (one int for all, or an int64 GPU tensor [B])
    reset_batch_       draws as measure_batch_ does and moves the observed branch of every slice to |0..0>
    collapse_batch_    the work of the three; returns the [B, 4] records
    BatchChannelOp     one trajectory step of a Channel (FIXED or DIAGONAL form) on every slice: operator j[b] drawn with
                       probability w_j / sum_j w_j from uniforms[b], K_j * scale applied to slice b; channel_batch_ builds one per call
    trajectory_norms   sum |amps|^2 of every slice, [B]
    BatchConditionalGate  a controlled gate chosen per trajectory from a table of at most 16 cases by an int64 per trajectory in
                       device memory -- the outcomes above, where they lie (C ABI: artn_cgate_batch_query / _pack / _apply);
                       apply_conditional_gate_batch_ builds one per call, correct_batch_ is the X / Z correction by two bits
    pauli_expectation_batch  <psi_b|P|psi_b> of every trajectory for up to sixteen strings of equal X/Y positions per pass over the
                       tensor (C ABI: artn_pauli_batch_query / _expect); pauli_sum_expectation_batch is sum_k c_k <P_k> per
                       trajectory, trajectory_mean the (weighted) mean over trajectories and its standard error
    sample_batch       S bitstrings from every trajectory, drawn from |amps_b|^2 / norm_b with uniforms[b, :] (C ABI:
                       artn_sample_batch_query / artn_sample_batch); sample_batch_flat returns flat memory indices and the norms

Slice b afterwards is bit for bit what the unbatched call leaves on that slice with record[b]: measure.collapse_ for the
measurements, apply_wide_gate_(slice, K_j * scale) for the channels.  A trajectory where nothing can be observed or drawn
(outcome -1: its q sums to 0 or is not finite, or the post-selected outcome has probability 0) and one that draws an exact
identity under scale == 1 keep every bit, whatever their neighbours do.  batch_dims=() is B = 1 and gives what the unbatched
calls give, bit for bit.

One layout rule: every memory bit of a batch dim lies at or above a 128-byte line (bit 4 for complex64, bit 3 for complex128);
layout.relayout_ moves a dim there.  At most 24 batch bits; B * D <= 2^24 (D = 2^len(dims)).

Every call only enqueues on the current stream: no host synchronisation, nothing comes back to the host.  uniforms=None draws
torch.rand(B, dtype=float64, generator=generator) on the device.  float64 sums in a fixed order, no atomics: results are
bit-identical from run to run.  There is no CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _native
from ._state import _Prebuilt, _checked, _dense_layout, _desc, _dims, _dtype_code, _interleaved, _lib, _packed, _ptr
from .born import marginal_probabilities, memory_to_multi_index
from .channel import Channel, _split
from .controlled import _split_dims
from .gates import _matrix
from .measure import _dims as _measured_dims
from .pauli import pauli_ops

__all__ = ["measure_batch_", "postselect_batch_", "reset_batch_", "collapse_batch_", "BatchChannelOp", "channel_batch_",
           "trajectory_info", "trajectory_norms", "BatchConditionalGate", "apply_conditional_gate_batch_", "conditional_gate_info",
           "correct_batch_", "pauli_expectation_batch", "pauli_sum_expectation_batch", "trajectory_mean", "pauli_batch_info",
           "sample_batch", "sample_batch_flat", "sample_batch_info"]

_KERNELS = ("artn_channel_batch_apply", "batched-trajectory kernels")   # what _lib looks for, and what it calls them
_LINE_BIT = {torch.complex64: 4, torch.complex128: 3}                   # index bits of a 128-byte line


def _batch(shape, strides, dims, batch_dims, dtype, role, what):
    """The batch dims as an int32 array, and B; ValueError for what the family refuses by name (include/artn.h)."""
    nd = len(shape)
    _dtype_code(dtype, what)
    batch = _dims(() if batch_dims is None else batch_dims, nd)
    used = [int(x) for x in dims]
    if any(x < 0 or x >= nd for x in batch) or len(set(batch.tolist())) != batch.shape[0]:
        raise ValueError(f"{what}: batch_dims must name distinct dims of a {nd}-dim tensor, got {batch.tolist()}")
    for x in batch.tolist():
        if x in used:
            raise ValueError(f"{what}: dim {x} is both a batch dim and a {role} one")
    for x, e in enumerate(shape):
        if int(e) < 1 or int(e) & (int(e) - 1):
            raise ValueError(f"{what}: power-of-two extents expected; dim {x} has extent {int(e)}")
    n = _dense_layout(shape, strides)
    bits = 0
    for x in batch.tolist():
        e, s = int(shape[x]), int(strides[x])
        if e == 1:
            continue
        if s.bit_length() - 1 < _LINE_BIT[dtype]:
            raise ValueError(f"{what}: batch dim {x} holds memory bit {s.bit_length() - 1}, below a 128-byte line (bit "
                             f"{_LINE_BIT[dtype]} of {dtype}): a line would span two trajectories -- move the dim up with "
                             "layout.relayout_")
        bits += e.bit_length() - 1
    if bits > _native.BATCH_MAX_BITS:
        raise ValueError(f"{what}: at most {_native.BATCH_MAX_BITS} batch bits, these dims have {bits}")
    if bits + len(used) > 24:
        raise ValueError(f"{what}: B * D = 2^{bits + len(used)} is above 2^24, what the streaming marginal keeps")
    if role == "target" and (n >> bits) < 2 ** len(used):
        raise ValueError(f"{what}: a channel on {len(used)} dims needs a trajectory of at least 2^{len(used)} elements; these have "
                         f"{n >> bits}")
    return batch, 1 << bits


def _form(ch, what):
    if not isinstance(ch, Channel):
        raise TypeError(f"{what}: a Channel expected, got {type(ch).__name__}")
    if ch.form == "DENSE":
        raise ValueError(f"{what}: batched channels take the FIXED and DIAGONAL forms; the DENSE form needs a reduced density "
                         "matrix per trajectory, which does not exist")


def _measure_plan(shape, strides, dims, batch_dims, dtype, what):
    _dtype_code(dtype, what)
    dims = np.array(_measured_dims(shape, dims, what), dtype=np.int32)
    batch, _ = _batch(shape, strides, dims, batch_dims, dtype, "measured", what)
    d, info = _desc(shape, strides, dtype), _native.ArtnBatchInfo()
    _native.check(_lib(*_KERNELS, what).artn_measure_batch_query(ctypes.byref(d), dims.shape[0], _ptr(dims), batch.shape[0], _ptr(batch),
                                                                 ctypes.byref(info)))
    return d, dims, batch, info


def _channel_plan(shape, strides, ch, dims, batch_dims, dtype, what, arrays=False):
    _dtype_code(dtype, what)
    _form(ch, what)
    dims, mats, weights = _split(ch, dims, len(shape), what)
    batch, _ = _batch(shape, strides, dims, batch_dims, dtype, "target", what)
    d, info = _desc(shape, strides, dtype), _native.ArtnBatchInfo()
    target, tile = np.full(_native.WGATE_MAX_K, -1, dtype=np.int32), np.full(12, -1, dtype=np.int32)
    _native.check(_lib(*_KERNELS, what).artn_channel_batch_query(ctypes.byref(d), ch.t, _ptr(dims), batch.shape[0], _ptr(batch), ch.m,
                                                                 ch.form_code, _ptr(mats), ctypes.byref(info),
                                                                 _ptr(target) if arrays else None, _ptr(tile) if arrays else None))
    return d, dims, batch, mats, weights, info, target, tile


def _pack(d, ch, dims, batch, mats, weights, info):
    """The channel's table (include/artn.h) as a uint8 numpy array."""
    return _packed(info, lambda *table: _lib(*_KERNELS, "trajectories").artn_channel_batch_pack(
        ctypes.byref(d), ch.t, _ptr(dims), batch.shape[0], _ptr(batch), ch.m, ch.form_code, _ptr(mats), _ptr(weights), *table))[0]


def trajectory_info(shape, strides, dims, batch_dims, dtype=torch.complex64, channel=None):
    """Host-only: the plan of a batched measurement of `dims` (channel=None) or of one batched step of `channel` on `dims`.  B, D,
    n, fields (the batch dims merged where they are adjacent in memory and in order, as (shift, width, pos): b = OR of
    ((index >> shift) & (2^width - 1)) << pos), grid, launches (choose + the pass; the marginal's come on top), record_bytes
    and the nominal bytes; for a measurement also reset_launches, for a channel tb, tile_bits (ascending), target_bits, n_tiles
    (n_tiles << tb == n), segment, lds_bytes and table_bytes."""
    what = "trajectory_info"
    if channel is None:
        _, _, _, info = _measure_plan(shape, strides, dims, batch_dims, dtype, what)
    else:
        _, _, _, _, _, info, target, tile = _channel_plan(shape, strides, channel, dims, batch_dims, dtype, what, arrays=True)
    out = {"B": info.B, "D": info.D, "n": info.n, "batch_bits": info.batch_bits,
           "fields": [(int(info.field_shift[f]), int(info.field_width[f]), int(info.field_pos[f])) for f in range(info.n_fields)],
           "grid": info.grid, "launches": info.launches, "record_bytes": info.record_bytes, "bytes_read": info.bytes_read,
           "bytes_written": info.bytes_written}
    if channel is None:
        out["reset_launches"] = info.reset_launches
    else:
        out.update(tb=info.tile_bits, tile_bits=[int(b) for b in tile[:info.tile_bits]],
                   target_bits=tuple(int(b) for b in target[:channel.t]), n_tiles=info.n_tiles, segment=info.segment,
                   lds_bytes=info.lds_bytes, table_bytes=info.table_bytes, form=channel.form)
    return out


def _uniforms(uniforms, generator, B, device, what):
    if uniforms is None:
        return torch.rand(B, dtype=torch.float64, device=device, generator=generator)
    if not isinstance(uniforms, torch.Tensor) or uniforms.dtype != torch.float64 or uniforms.numel() != B or not uniforms.is_cuda:
        raise ValueError(f"{what}: uniforms is a float64 GPU tensor of {B} elements, one per trajectory")
    return uniforms.to(device).reshape(B).contiguous()


def _outcomes(outcomes, B, D, device, what):
    if isinstance(outcomes, torch.Tensor):
        if outcomes.dtype != torch.int64 or outcomes.numel() != B or not outcomes.is_cuda:
            raise ValueError(f"{what}: outcomes is an int or an int64 GPU tensor of {B} elements, one per trajectory")
        return outcomes.to(device).reshape(B).contiguous()
    o = int(outcomes)
    if not 0 <= o < D:
        raise ValueError(f"{what}: outcome {o} of {D} outcomes (0 .. {D - 1} expected)")
    return torch.full((B,), o, dtype=torch.int64, device=device)   # (a fill: no host-to-device copy)


def _q(amps, batch, dims, B, D):
    return marginal_probabilities(amps, batch.tolist() + dims.tolist()).reshape(B, D)


def collapse_batch_(amps, dims, batch_dims, outcomes=None, uniforms=None, generator=None, renormalize=True, reset=False):
    """The work of measure_batch_ / postselect_batch_ / reset_batch_.  Returns the records, a float64 GPU tensor [B, 4]: row b is
    [outcome (the bits of an int64: records.view(torch.int64)[:, 0]), probability, total, scale] of trajectory b.
    outcomes=None draws with `uniforms` / `generator`."""
    what = "trajectories.collapse_batch_"
    _checked(amps, what)
    d, dims, batch, info = _measure_plan(amps.shape, amps.stride(), dims, batch_dims, amps.dtype, what)
    dev, lib, B, D = amps.device, _lib(*_KERNELS, what), info.B, info.D
    forced = None if outcomes is None else _outcomes(outcomes, B, D, dev, what)
    u = _uniforms(uniforms, generator, B, dev, what) if forced is None else None
    q = _q(amps, batch, dims, B, D)
    rec = torch.empty((B, _native.MEASURE_RECORD_BYTES // 8), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = _native.current_stream_ptr(dev)
        _native.check(lib.artn_measure_batch_choose(q.data_ptr(), B, D, None if u is None else u.data_ptr(),
                                                    None if forced is None else forced.data_ptr(), int(bool(renormalize)),
                                                    rec.data_ptr(), stream))
        _native.check(lib.artn_measure_batch_collapse(ctypes.byref(d), amps.data_ptr(), dims.shape[0], _ptr(dims), batch.shape[0],
                                                      _ptr(batch), rec.data_ptr(), int(bool(reset)), stream))
    return rec


def _result(rec):
    return rec.view(torch.int64)[:, 0], rec[:, 1]


def measure_batch_(amps, dims, batch_dims, uniforms=None, generator=None, renormalize=True):
    """Measure `dims` of every trajectory in place.  Returns (outcomes int64 [B], probabilities float64 [B]) on the device;
    outcome -1 and probability 0 where nothing can be observed (that slice is untouched)."""
    return _result(collapse_batch_(amps, dims, batch_dims, None, uniforms, generator, renormalize, False))


def postselect_batch_(amps, dims, batch_dims, outcomes, renormalize=True):
    """Project `dims` of trajectory b onto outcomes[b] (an int: the same for all) in place.  Returns (outcomes, probabilities) as
    measure_batch_ does: -1 and 0 where the outcome cannot be observed."""
    if outcomes is None:
        raise ValueError("trajectories.postselect_batch_: outcomes are needed")
    return _result(collapse_batch_(amps, dims, batch_dims, outcomes, None, None, renormalize, False))


def reset_batch_(amps, dims, batch_dims, uniforms=None, generator=None, renormalize=True):
    """Measure `dims` of every trajectory and put them back to 0 in place: new[b][r, 0..0] = a[b][r, o[b]] * scale[b].  Returns the
    (outcomes, probabilities) that were observed."""
    return _result(collapse_batch_(amps, dims, batch_dims, None, uniforms, generator, renormalize, True))


class BatchChannelOp(_Prebuilt):
    """One channel on `dims` of every trajectory, for tensors of one layout.  Validates, plans, packs the table and copies it to
    `device` once; op(amps, uniforms=None, generator=None, renormalize=True) then performs one step on every slice of amps IN
    PLACE and returns (j int64 [B], p float64 [B]) on the device; op.step(amps, ...) returns the [B, 4] records instead."""

    def __init__(self, shape, strides, dtype, channel, dims, batch_dims, device):
        what = "BatchChannelOp"
        self._bind(shape, strides, dtype, device)
        self._d, self._dims, self._batch, mats, weights, info, _, _ = _channel_plan(self.shape, self.strides, channel, dims, batch_dims,
                                                                                     dtype, what)
        self.channel, self.t, self.m, self.form = channel, channel.t, channel.m, channel.form
        self.dims, self.batch_dims = tuple(int(x) for x in self._dims), tuple(int(x) for x in self._batch)
        self.B, self.D, self.tile_bits, self.n_tiles = info.B, info.D, info.tile_bits, info.n_tiles
        self.table_bytes, self.record_bytes = info.table_bytes, info.record_bytes
        self._upload(_pack(self._d, channel, self._dims, self._batch, mats, weights, info))

    def _upload(self, table):
        # (pinned and non-blocking, as ChannelOp's: channel_batch_ builds an object per call)
        self._table = torch.from_numpy(table).pin_memory().to(self.device, non_blocking=True)

    def step(self, amps, uniforms=None, generator=None, renormalize=True):
        """One step of every trajectory, enqueued on the current stream.  Returns the records, float64 [B, 4]: row b is
        [j (the bits of an int64), probability w_j / total, total, scale] of trajectory b."""
        what = "trajectories.BatchChannelOp"
        self._check(amps, what)
        dev, lib, B = amps.device, _lib(*_KERNELS, what), self.B
        u = _uniforms(uniforms, generator, B, dev, what)
        src = _q(amps, self._batch, self._dims, B, self.D) if self.form == "DIAGONAL" else None
        rec = torch.empty((B, _native.MEASURE_RECORD_BYTES // 8), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            stream = _native.current_stream_ptr(dev)
            _native.check(lib.artn_channel_batch_choose(self._table.data_ptr(), self.table_bytes, self.t, self.m, self.channel.form_code,
                                                        None if src is None else src.data_ptr(), u.data_ptr(), B,
                                                        int(bool(renormalize)), rec.data_ptr(), stream))
            _native.check(lib.artn_channel_batch_apply(ctypes.byref(self._d), amps.data_ptr(), self.t, _ptr(self._dims),
                                                       self._batch.shape[0], _ptr(self._batch), self.m, self._table.data_ptr(),
                                                       self.table_bytes, rec.data_ptr(), stream))
        return rec

    def __call__(self, amps, uniforms=None, generator=None, renormalize=True):
        return _result(self.step(amps, uniforms, generator, renormalize))


def channel_batch_(amps, channel, dims, batch_dims, uniforms=None, generator=None, renormalize=True):
    """One trajectory step of `channel` on `dims` of every slice of amps, in place.  Returns (j, p) as BatchChannelOp does.  (Plans
    and uploads per call: build a BatchChannelOp once to apply the same channel repeatedly.)"""
    _checked(amps, "trajectories.channel_batch_")
    return BatchChannelOp(amps.shape, amps.stride(), amps.dtype, channel, dims, batch_dims, amps.device)(amps, uniforms, generator,
                                                                                                         renormalize)


# ---- conditional gates: a controlled gate chosen per trajectory by a device-side selector -------------------------------------------
_CGATE_KERNELS = ("artn_cgate_batch_apply", "conditional-gate kernels")


def _integer(v, name, what):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
        raise TypeError(f"{what}: {name} must be an integer, got {v!r}")
    v = int(v)
    if not 0 <= v < 2 ** 63:
        raise ValueError(f"{what}: {name} must lie in 0 .. 2^63 - 1, got {v}")
    return v


def _cases(cases, t, mask, what):
    """(int64 keys [m], float64 mats [m * 2 * 4^t], mask as the library takes it).  The number of cases, repeated keys and keys
    outside the mask are the library's to refuse; a t it does not take keeps zero matrices, so that it refuses t."""
    pairs = list(cases.items()) if isinstance(cases, dict) else [tuple(p) for p in cases]
    if any(len(p) != 2 for p in pairs):
        raise ValueError(f"{what}: cases is a dict {{key: matrix}} or a list of (key, matrix) pairs")
    keys = np.array([_integer(k, "a key", what) for k, _ in pairs] + [0] * (not pairs), dtype=np.int64)
    if 1 <= t <= _native.WGATE_MAX_K and pairs:
        mats = np.concatenate([_interleaved(_matrix(u, t, what)) for _, u in pairs])
    else:
        mats = np.zeros(max(len(pairs), 1) * 2, dtype=np.float64)
    return len(pairs), keys, mats, -1 if mask is None else _integer(mask, "mask", what)


def _cgate_plan(shape, strides, dtype, cases, targets, batch_dims, controls, control_values, mask, what, arrays=False):
    _dtype_code(dtype, what)
    nd = len(shape)
    t, targets, c, controls, values = _split_dims(targets, controls, control_values, nd, what)
    batch = _dims(() if batch_dims is None else batch_dims, nd)
    m, keys, mats, mask = _cases(cases, t, mask, what)
    d, info = _desc(shape, strides, dtype), _native.ArtnCgateBatchInfo()
    target, control, tile = (np.full(n, -1, dtype=np.int32) for n in (_native.WGATE_MAX_K, max(c, 1), 12))
    _native.check(_lib(*_CGATE_KERNELS, what).artn_cgate_batch_query(
        ctypes.byref(d), t, _ptr(targets), c, _ptr(controls), _ptr(values), batch.shape[0], _ptr(batch) if batch.shape[0] else None, m,
        _ptr(keys), mask, _ptr(mats), None, 1, ctypes.byref(info), _ptr(target) if arrays else None, _ptr(control) if arrays else None,
        _ptr(tile) if arrays else None))
    return d, (t, targets, c, controls, values, batch), (m, keys, mats, mask), info, (target, control, tile)


def conditional_gate_info(shape, strides, cases, targets, batch_dims, controls=(), control_values=None, dtype=torch.complex64, mask=None):
    """Host-only: the plan of one conditional gate.  The keys of controlled_gate_info (t, c, c_high / c_low, target_bits,
    control_bits, control_values, tile_bits ascending, tb, n_selected, n_tiles with n_tiles << tb == n >> c_high, segment, lds_bytes,
    table_bytes, nominal bytes, diagonal: every case is) and m, keys, B, batch_bits, fields (as trajectory_info's), grid."""
    what = "conditional_gate_info"
    _, (t, _, c, _, values, _), (m, keys, _, _), info, (target, control, tile) = _cgate_plan(
        shape, strides, dtype, cases, targets, batch_dims, controls, control_values, mask, what, arrays=True)
    return {"t": info.t, "c": info.c, "c_high": info.c_high, "c_low": info.c_low,
            "target_bits": tuple(int(b) for b in target[:t]), "control_bits": tuple(int(b) for b in control[:c]),
            "control_values": tuple(int(v) for v in values[:c]), "tile_bits": [int(b) for b in tile[:info.tile_bits]],
            "tb": info.tile_bits, "n_selected": info.n_selected, "n_tiles": info.n_tiles, "segment": info.segment,
            "lds_bytes": info.lds_bytes, "table_bytes": info.table_bytes, "bytes_read": info.bytes_read,
            "bytes_written": info.bytes_written, "diagonal": bool(info.diagonal), "m": info.m, "keys": tuple(int(k) for k in keys[:m]),
            "B": info.B, "batch_bits": info.batch_bits,
            "fields": [(int(info.field_shift[f]), int(info.field_width[f]), int(info.field_pos[f])) for f in range(info.n_fields)],
            "grid": info.grid}


def _selector(selector, B, device, what):
    """(address, stride in 8-byte words) of the B selector words; host-only checks, the tensor is never read."""
    if not isinstance(selector, torch.Tensor):
        raise TypeError(f"{what}: the selector is a GPU tensor, got {type(selector).__name__}")
    if not selector.is_cuda:
        raise RuntimeError(f"{what}: the selector must live on the GPU (got a {selector.device} tensor); there is no CPU fallback")
    if selector.device != device:
        raise ValueError(f"{what}: the selector lives on {selector.device}, the amplitudes on {device}")
    words = _native.MEASURE_RECORD_BYTES // 8
    if selector.dtype == torch.float64:
        if selector.dim() != 2 or tuple(selector.shape) != (B, words) or selector.stride(1) != 1:
            raise ValueError(f"{what}: a float64 selector is the [{B}, {words}] records of collapse_batch_ / BatchChannelOp.step, got "
                             f"shape {tuple(selector.shape)}, strides {tuple(selector.stride())}")
        stride = selector.stride(0) if B > 1 else words
    elif selector.dtype == torch.int64:
        if selector.dim() > 1 or selector.numel() != B:
            raise ValueError(f"{what}: the selector is an int64 GPU tensor of {B} elements, one per trajectory, got shape "
                             f"{tuple(selector.shape)}")
        stride = selector.stride(0) if B > 1 else 1
    else:
        raise TypeError(f"{what}: an int64 selector (or the float64 records of collapse_batch_) expected, got {selector.dtype}")
    if stride < 1:
        raise ValueError(f"{what}: a selector stride of at least one 8-byte word is needed, not {stride}")
    if selector.data_ptr() % 8:
        raise ValueError(f"{what}: the selector must start on an 8-byte boundary")
    return selector.data_ptr(), int(stride)


class BatchConditionalGate(_Prebuilt):
    """A gate chosen per trajectory, for tensors of one layout.  `cases` is a dict {key: matrix} or a list of (key, matrix) pairs,
    1 to 16 of them: distinct integer keys in 0 .. 2^63 - 1 inside `mask` (None: all bits), each matrix complex [2^t, 2^t] on
    `targets` (t = 1..5, the first listed dim the most significant digit, as apply_wide_gate_); controls / control_values as
    ControlledGate's; batch_dims as the rest of this module's, disjoint from targets and controls.  Validates, plans, packs the
    table and copies it to `device` once.

    g(amps, selector) then updates amps IN PLACE with ONE launch and returns it.  `selector` holds one int64 per trajectory on
    the GPU: an int64 tensor of B elements with any stride (the view records.view(torch.int64)[:, 0] that measure_batch_ returns
    is read where it lies), or the float64 [B, 4] records of collapse_batch_ / BatchChannelOp.step.  With o = selector[b]:
    o < 0, no case with key == (o & mask), or a case that is exactly the identity leave trajectory b untouched -- no tile of it
    is read or written; otherwise slice b becomes bit for bit what apply_controlled_gate_ leaves on a dense clone of it for that
    case's matrix.  The host never reads the selector."""

    def __init__(self, shape, strides, dtype, cases, targets, batch_dims, device, controls=(), control_values=None, mask=None):
        what = "BatchConditionalGate"
        self._bind(shape, strides, dtype, device)
        self._d, split, (self.m, keys, mats, self._mask), info, _ = _cgate_plan(self.shape, self.strides, dtype, cases, targets, batch_dims,
                                                                                controls, control_values, mask, what)
        self.t, self._targets, self.c, self._controls, self._values, self._batch = split
        self.keys, self.mask = tuple(int(k) for k in keys[:self.m]), mask
        self.B, self.tile_bits, self.n_tiles, self.grid, self.table_bytes = info.B, info.tile_bits, info.n_tiles, info.grid, info.table_bytes
        self.c_high, self.c_low = info.c_high, info.c_low
        self.batch_dims = tuple(int(x) for x in self._batch)
        self._upload(_packed(info, lambda *table: _lib(*_CGATE_KERNELS, what).artn_cgate_batch_pack(
            ctypes.byref(self._d), self.t, _ptr(self._targets), self.c, _ptr(self._controls), _ptr(self._values), self._batch.shape[0],
            _ptr(self._batch) if self._batch.shape[0] else None, self.m, _ptr(keys), self._mask, _ptr(mats), *table))[0])

    def _upload(self, table):
        # (pinned and non-blocking, as BatchChannelOp's: apply_conditional_gate_batch_ builds an object per call)
        self._table = torch.from_numpy(table).pin_memory().to(self.device, non_blocking=True)

    def __call__(self, amps, selector):
        what = "trajectories.BatchConditionalGate"
        self._check(amps, what)
        sel, stride = _selector(selector, self.B, amps.device, what)
        with torch.cuda.device(amps.device):
            _native.check(_lib(*_CGATE_KERNELS, what).artn_cgate_batch_apply(
                ctypes.byref(self._d), amps.data_ptr(), self.t, _ptr(self._targets), self.c, _ptr(self._controls), _ptr(self._values),
                self._batch.shape[0], _ptr(self._batch) if self._batch.shape[0] else None, self.m, self._table.data_ptr(),
                self.table_bytes, sel, stride, self._mask, _native.current_stream_ptr(amps.device)))
        return amps


def apply_conditional_gate_batch_(amps, cases, targets, batch_dims, selector, controls=(), control_values=None, mask=None):
    """amps <- for every trajectory b the case of `cases` that selector[b] names, on `targets` under `controls`, in place: one
    launch; returns amps.  (Plans and uploads per call: build a BatchConditionalGate once to apply the same cases repeatedly.)"""
    _checked(amps, "trajectories.apply_conditional_gate_batch_")
    return BatchConditionalGate(amps.shape, amps.stride(), amps.dtype, cases, targets, batch_dims, amps.device, controls, control_values,
                                mask)(amps, selector)


_PAULI_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_PAULI_Z = np.diag([1.0, -1.0]).astype(np.complex128)


def correct_batch_(amps, target, batch_dims, selector, x_bit=None, z_bit=None):
    """The Pauli correction of teleportation and of active reset, per trajectory and in one launch: with o = selector[b], X on
    `target` where bit x_bit of o is set, THEN Z where bit z_bit is set (the matrix Z^z X^x; the mask is the two bits, the cases
    the four products, the identity among them, which leaves its trajectories untouched).  x_bit or z_bit None: no such
    correction.  A trajectory with o < 0 is untouched.  Applied twice with one selector it gives back the input bit for bit where
    at most one of the two bits is set, and its negative where both are: (ZX)^2 = -1."""
    what = "trajectories.correct_batch_"
    bits = [None if b is None else _integer(b, name, what) for b, name in ((x_bit, "x_bit"), (z_bit, "z_bit"))]
    if bits[0] is None and bits[1] is None:
        raise ValueError(f"{what}: x_bit or z_bit is needed")
    if bits[0] == bits[1] or any(b is not None and b > 62 for b in bits):
        raise ValueError(f"{what}: x_bit and z_bit are different bits 0 .. 62 of the selector, got {x_bit} and {z_bit}")
    cases = {}
    for x in range(1 if bits[0] is None else 2):
        for z in range(1 if bits[1] is None else 2):
            key = (x << bits[0] if x else 0) | (z << bits[1] if z else 0)
            cases[key] = np.linalg.matrix_power(_PAULI_Z, z) @ np.linalg.matrix_power(_PAULI_X, x)
    mask = sum(1 << b for b in bits if b is not None)
    return apply_conditional_gate_batch_(amps, cases, (target,), batch_dims, selector, mask=mask)


def trajectory_norms(amps, batch_dims):
    """sum |amps|^2 of every trajectory: marginal_probabilities over the batch dims, as a float64 GPU tensor [B]."""
    batch = _dims(() if batch_dims is None else batch_dims, amps.dim())
    return marginal_probabilities(amps, batch.tolist()).reshape(-1)


# ---- observables per trajectory ---------------------------------------------------------------------------------------------------
_PAULI_KERNELS = ("artn_pauli_batch_expect", "batched Pauli-expectation kernels")


def _pauli_query(d, ops, batch, what, masks=False):
    n_terms = ops.shape[0]
    info = _native.ArtnPauliBatchInfo()
    out = tuple(np.zeros(n_terms, dtype=t) for t in (np.uint64, np.uint64, np.int32, np.int32, np.uint64, np.uint64)) if masks else ()
    _native.check(_lib(*_PAULI_KERNELS, what).artn_pauli_batch_query(
        ctypes.byref(d), _ptr(ops), n_terms, batch.shape[0], _ptr(batch) if batch.shape[0] else None, ctypes.byref(info),
        *([_ptr(x) for x in out] if masks else [None] * 6)))
    return (info,) + out


def pauli_batch_info(shape, strides, paulis, batch_dims, dtype=torch.complex64):
    """Host-only: the plan of pauli_expectation_batch.  Per string: xmask, zmask (memory bits), local_xmask, local_zmask (the same
    compressed onto the bits that are no batch bits), n_y and group.  B, n, batch_bits, local_bits (M), tile_bits = min(10, M),
    fields (as trajectory_info's); n_groups, n_launches (passes over the tensor, each followed by one finish launch),
    terms_per_launch; chunks and chunks_halved (the C of a pass whose partner lies inside / outside the tile), grid,
    workspace_bytes, out_bytes and bytes_read."""
    what = "pauli_batch_info"
    _dtype_code(dtype, what)
    ops, _ = pauli_ops(paulis, len(shape))
    batch = _dims(() if batch_dims is None else batch_dims, len(shape))
    info, xm, zm, ny, group, xl, zl = _pauli_query(_desc(shape, strides, dtype), ops, batch, what, masks=True)
    return {"xmask": [int(v) for v in xm], "zmask": [int(v) for v in zm], "n_y": [int(v) for v in ny], "group": [int(v) for v in group],
            "local_xmask": [int(v) for v in xl], "local_zmask": [int(v) for v in zl], "n_groups": info.n_groups,
            "n_launches": info.n_launches, "terms_per_launch": info.terms_per_launch, "B": info.B, "n": info.n,
            "batch_bits": info.batch_bits, "local_bits": info.local_bits, "tile_bits": info.tile_bits,
            "fields": [(int(info.field_shift[f]), int(info.field_width[f]), int(info.field_pos[f])) for f in range(info.n_fields)],
            "chunks": info.chunks, "chunks_halved": info.chunks_halved, "grid": info.grid, "workspace_bytes": info.workspace_bytes,
            "out_bytes": info.out_bytes, "bytes_read": info.bytes_read}


def _pauli_raw(amps, ops, batch_dims, what):
    """float64 GPU tensor [B, n_terms + 1]: row b holds the raw sums of trajectory b in term order, then its sum |a|^2."""
    _checked(amps, what)
    batch = _dims(() if batch_dims is None else batch_dims, amps.dim())
    d = _desc(amps.shape, amps.stride(), amps.dtype)
    info = _pauli_query(d, ops, batch, what)[0]
    n_terms = ops.shape[0]
    out = torch.empty((info.B, n_terms + 1), dtype=torch.float64, device=amps.device)
    ws = torch.empty(max(info.workspace_bytes // 8, 1), dtype=torch.float64, device=amps.device)   # (per call: calls may overlap on streams)
    with torch.cuda.device(amps.device):
        _native.check(_lib(*_PAULI_KERNELS, what).artn_pauli_batch_expect(
            ctypes.byref(d), amps.data_ptr(), _ptr(ops), n_terms, batch.shape[0], _ptr(batch) if batch.shape[0] else None,
            out.data_ptr(), ws.data_ptr(), info.workspace_bytes, _native.current_stream_ptr(amps.device)))
    return out


def pauli_expectation_batch(amps, paulis, batch_dims, normalize=True):
    """<psi_b|P|psi_b> of every trajectory b for one Pauli string or a list of them (written as for pauli_expectation; I on every
    batch dim).  Returns (values, norms) on the device: values float64 [B, n_terms] ([B] for one string), divided by norms[b]
    unless normalize=False; norms float64 [B], sum |amps|^2 of every trajectory from the same call.  A trajectory of norm 0 gives
    NaN under normalize=True (0 / 0: nothing is checked on the host).  Strings of equal X/Y positions share a pass over the
    tensor, sixteen at a time.  batch_dims=() is B = 1: row 0 holds pauli_expectation(..., normalize=False)'s raw values bit for
    bit; so does row b of a batched call against a dense clone of slice b whenever a trajectory has at least 2^10 elements and
    B * (elements of a trajectory / 2^10) <= 2048 (pauli_batch_info: chunks == local tiles)."""
    what = "trajectories.pauli_expectation_batch"
    _native.require_gpu(amps, what)
    ops, single = pauli_ops(paulis, amps.dim())
    out = _pauli_raw(amps, ops, batch_dims, what)
    vals, norms = out[:, :-1], out[:, -1]
    if normalize:
        vals = vals / norms[:, None]
    return (vals[:, 0] if single else vals), norms


def pauli_sum_expectation_batch(amps, terms, batch_dims, normalize=True):
    """sum_k c_k <P_k> of every trajectory for terms = [(c_k, string_k), ...] with REAL coefficients: one call of the library and
    one float64 matmul on the device.  Returns (E float64 [B], norms float64 [B])."""
    what = "trajectories.pauli_sum_expectation_batch"
    _native.require_gpu(amps, what)
    terms = list(terms)
    if not terms:
        raise ValueError(f"{what}: at least one term is needed")
    coeffs = [complex(c) for c, _ in terms]
    if any(c.imag != 0.0 for c in coeffs):
        raise ValueError(f"{what}: real coefficients expected (a Hermitian sum); take real and imaginary parts in two calls")
    vals, norms = pauli_expectation_batch(amps, [p for _, p in terms], batch_dims, normalize)
    c = torch.from_numpy(np.array([c.real for c in coeffs], dtype=np.float64)).pin_memory().to(amps.device, non_blocking=True)
    return vals @ c, norms


def trajectory_mean(values, weights=None):
    """(mean, standard error) over dim 0 of `values` ([B] or [B, n_terms]), on the device of `values`, torch only.  weights=None:
    the mean and std(ddof=1) / sqrt(B).  weights w (a floating tensor [B]: the norms of trajectories kept unnormalised with
    renormalize=False): sum w v / sum w and sqrt(sum w^2 (v - mean)^2) / sum w; a row with w == 0 is left out even where its value
    is NaN."""
    what = "trajectories.trajectory_mean"
    if not isinstance(values, torch.Tensor) or not values.is_floating_point() or values.dim() < 1:
        raise TypeError(f"{what}: values is a floating tensor [B] or [B, n_terms]")
    B = values.shape[0]
    if weights is None:
        return values.mean(dim=0), values.std(dim=0, unbiased=True) / float(B) ** 0.5
    if not isinstance(weights, torch.Tensor) or not weights.is_floating_point():
        raise TypeError(f"{what}: weights is a floating tensor of {B} non-negative weights (the norms), not outcomes, records' integer "
                        f"view or a selector; got {weights.dtype if isinstance(weights, torch.Tensor) else type(weights).__name__}")
    if weights.dim() != 1 or weights.shape[0] != B or weights.device != values.device:
        raise ValueError(f"{what}: weights has one entry per trajectory, shape [{B}] on {values.device}; got shape "
                         f"{tuple(weights.shape)} on {weights.device}")
    w = weights.to(values.dtype).reshape((B,) + (1,) * (values.dim() - 1))
    live, zero = w != 0, torch.zeros((), dtype=values.dtype, device=values.device)
    total = w.sum(dim=0)
    mean = torch.where(live, w * values, zero).sum(dim=0) / total
    err = torch.where(live, (w * (values - mean)) ** 2, zero).sum(dim=0).sqrt() / total
    return mean, err


# ---- bitstrings per trajectory ------------------------------------------------------------------------------------------------------
_SAMPLE_KERNELS = ("artn_sample_batch", "batched sampling kernels")
_SAMPLE_FORMS = {_native.SAMPLE_BATCH_SMALL: "SMALL", _native.SAMPLE_BATCH_TILED: "TILED"}


def _sample_plan(shape, strides, batch_dims, n_samples, dtype, what):
    """(descriptor, batch dims, info).  The family's refusals by name (_batch), then the library's (n > 2^40, B * S > 2^28)."""
    batch, B = _batch(shape, strides, (), batch_dims, dtype, "sampled", what)
    n, S = _dense_layout(shape, strides), int(n_samples)
    if S < 0:
        raise ValueError(f"{what}: n_samples must not be negative, got {S}")
    if n > 2 ** 40:
        raise ValueError(f"{what}: at most 2^40 elements, this tensor has {n}")
    if B * S > 2 ** 28:
        raise ValueError(f"{what}: B * n_samples = {B} * {S} is above 2^28 samples (2 GiB of indices)")
    d, info = _desc(shape, strides, dtype), _native.ArtnSampleBatchInfo()
    _native.check(_lib(*_SAMPLE_KERNELS, what).artn_sample_batch_query(ctypes.byref(d), batch.shape[0],
                                                                       _ptr(batch) if batch.shape[0] else None, S, ctypes.byref(info)))
    return d, batch, info


def sample_batch_info(shape, strides, batch_dims, n_samples, dtype=torch.complex64):
    """Host-only: the plan of sample_batch.  B, n, batch_bits, local_bits (M), block_bits and blocks_per_trajectory (those of
    born_plan(2^M)), form ("SMALL": M < 10 and B > 1, one launch; "TILED": three), fields (as trajectory_info's), launches, grid
    (the workgroups of each launch), workspace_bytes (B * blocks_per_trajectory * 16; 0 for SMALL) and bytes_read_min (one
    reading of the tensor)."""
    _, _, info = _sample_plan(shape, strides, batch_dims, n_samples, dtype, "sample_batch_info")
    return {"B": info.B, "n": info.n, "batch_bits": info.batch_bits, "local_bits": info.local_bits, "block_bits": info.block_bits,
            "blocks_per_trajectory": info.blocks_per_trajectory, "form": _SAMPLE_FORMS[info.form],
            "fields": [(int(info.field_shift[f]), int(info.field_width[f]), int(info.field_pos[f])) for f in range(info.n_fields)],
            "launches": info.launches, "grid": [int(g) for g in info.grid[:info.launches]], "workspace_bytes": info.workspace_bytes,
            "bytes_read_min": info.bytes_read_min}


def _sample_uniforms(uniforms, n_samples, generator, B, device, what):
    """float64 [B, S] on `device`.  Host-only checks: dtype and shape; the values are never read here."""
    if uniforms is None:
        if n_samples is None or int(n_samples) < 0:
            raise ValueError(f"{what}: give n_samples or uniforms")
        return None, int(n_samples)
    if not isinstance(uniforms, torch.Tensor) or uniforms.dtype != torch.float64:
        raise ValueError(f"{what}: uniforms is a float64 GPU tensor [B, S] = [{B}, n_samples], one row per trajectory")
    if uniforms.dim() != 2 or uniforms.shape[0] != B:
        raise ValueError(f"{what}: uniforms has shape [B, S] = [{B}, n_samples], one row per trajectory; got {tuple(uniforms.shape)}")
    if n_samples is not None and int(n_samples) != uniforms.shape[1]:
        raise ValueError(f"{what}: n_samples = {int(n_samples)} disagrees with uniforms of shape {tuple(uniforms.shape)}")
    if not uniforms.is_cuda or uniforms.device != device:
        raise ValueError(f"{what}: uniforms must live on {device}, where the amplitudes are; got {uniforms.device}")
    return uniforms, int(uniforms.shape[1])


def sample_batch_flat(amps, batch_dims, n_samples=None, *, uniforms=None, generator=None):
    """S draws from every trajectory.  Returns (flat, prob, norms) on the device: flat int64 [B, S], the flat MEMORY index of
    sample (b, s) in the whole tensor (what born.memory_to_multi_index takes); prob float64 [B, S] = |amps[flat]|^2 / norms[b];
    norms float64 [B] = sum |amps_b|^2.  See sample_batch for the arguments and the rule.  With S = 0 nothing is launched and
    norms is NaN: it was not computed."""
    what = "trajectories.sample_batch_flat"
    _checked(amps, what)
    dev = amps.device
    B = _batch(amps.shape, amps.stride(), (), batch_dims, amps.dtype, "sampled", what)[1]
    uniforms, S = _sample_uniforms(uniforms, n_samples, generator, B, dev, what)
    d, batch, info = _sample_plan(amps.shape, amps.stride(), batch_dims, S, amps.dtype, what)
    if S == 0:
        return (torch.empty((B, 0), dtype=torch.int64, device=dev), torch.empty((B, 0), dtype=torch.float64, device=dev),
                torch.full((B,), float("nan"), dtype=torch.float64, device=dev))
    if uniforms is None:
        uniforms = torch.rand((B, S), dtype=torch.float64, device=dev, generator=generator)
    us, order = torch.sort(uniforms.contiguous(), dim=1)  # ascending per row: a block is read once for all its samples
    us = us.contiguous()                                  # (the library reads rows of S consecutive doubles)
    flat_sorted = torch.empty((B, S), dtype=torch.int64, device=dev)
    prob_sorted = torch.empty((B, S), dtype=torch.float64, device=dev)
    norms = torch.empty(B, dtype=torch.float64, device=dev)
    ws = torch.empty(max(info.workspace_bytes // 8, 1), dtype=torch.float64, device=dev)   # (per call: calls may overlap on streams)
    with torch.cuda.device(dev):
        _native.check(_lib(*_SAMPLE_KERNELS, what).artn_sample_batch(
            ctypes.byref(d), amps.data_ptr(), batch.shape[0], _ptr(batch) if batch.shape[0] else None, us.data_ptr(), S,
            flat_sorted.data_ptr(), prob_sorted.data_ptr(), norms.data_ptr(), ws.data_ptr(), info.workspace_bytes,
            _native.current_stream_ptr(dev)))
    live = (torch.isfinite(norms) & (norms > 0))[:, None]
    flat = torch.empty_like(flat_sorted).scatter_(1, order, flat_sorted)
    prob = torch.empty_like(prob_sorted).scatter_(1, order, prob_sorted / norms[:, None])
    flat = torch.where(live, flat, torch.full_like(flat, -1))
    prob = torch.where(live, prob, torch.full_like(prob, float("nan")))
    return flat, prob, norms


def sample_batch(amps, batch_dims, n_samples=None, *, uniforms=None, generator=None):
    """Draw S multi-indices from EVERY trajectory of amps with probability |amps_b[idx]|^2 / norm_b.

    Returns (idx, prob) on the device: idx int64 [B, S, amps.dim()], multi-indices in the tensor's logical dim order, the batch
    dims' columns holding the digits of b; prob float64 [B, S].  `uniforms` is a float64 GPU tensor [B, S], any order within a
    row; sample (b, s) belongs to uniforms[b, s]: it is the element of trajectory b whose cumulative-probability interval, in
    LOCAL-index order (local bit j: the j-th lowest memory bit that is no batch bit), contains uniforms[b, s].  Without
    `uniforms`, torch.rand((B, n_samples), dtype=float64, generator=generator) on the device supplies them.  Only dtype and shape
    of `uniforms` are checked (on the host: the values are never read there); a value at or above 1 takes the trajectory's last
    non-zero element, a negative one gives index -1 and probability 0.

    Row b is bit for bit what born.sample gives on a dense clone of slice b with its dims in local-bit order and uniforms[b];
    batch_dims=() is born.sample itself, without its host synchronisation.  A DEAD trajectory (its norm 0 or not finite) is no
    error: its rows are -1 in every column of idx and NaN in prob, and it changes no other row.  The call only enqueues on the
    current stream and can be captured into a HIP graph.  Limits: power-of-two extents, n <= 2^40, B * S <= 2^28."""
    flat, prob, _ = sample_batch_flat(amps, batch_dims, n_samples, uniforms=uniforms, generator=generator)
    idx = memory_to_multi_index(flat, amps.shape, amps.stride())
    return torch.where((flat < 0)[..., None], torch.full_like(idx, -1), idx), prob
