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
from ._state import _Prebuilt, _checked, _dense_layout, _desc, _dims, _dtype_code, _lib, _packed, _ptr
from .born import marginal_probabilities
from .channel import Channel, _split
from .measure import _dims as _measured_dims

__all__ = ["measure_batch_", "postselect_batch_", "reset_batch_", "collapse_batch_", "BatchChannelOp", "channel_batch_",
           "trajectory_info", "trajectory_norms"]

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


def trajectory_norms(amps, batch_dims):
    """sum |amps|^2 of every trajectory: marginal_probabilities over the batch dims, as a float64 GPU tensor [B]."""
    batch = _dims(() if batch_dims is None else batch_dims, amps.dim())
    return marginal_probabilities(amps, batch.tolist()).reshape(-1)
