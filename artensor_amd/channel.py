"""Noise channels for quantum trajectories, DRAWN AND APPLIED ON THE DEVICE, in place (C ABI: artn_channel_query,
artn_channel_pack, artn_channel_choose, artn_channel_apply).

A Channel is a set of m = 1..256 operators on t = 1..5 qubits.  One trajectory step draws an operator j with probability
w_j / sum_j w_j and applies K_j * scale to `dims` of the state with the tile kernel of wide_gates.py -- everything enqueued on the
current stream; the host never sees the draw unless it asks for it.  Where the weights w_j come from is the channel's FORM,
decided when it is built:

    FIXED     Channel.mixture(probs, unitaries) and the named mixtures (depolarizing, pauli_channel, bit_flip, phase_flip):
              K_j = sqrt(p_j) U_j.  w_j = p_j whatever the state is, so NO pass over the state is made for the draw; the matrices
              applied are the U_j as given (exact Pauli matrices for the named ones) and scale is exactly 1.  A draw that lands on
              an exact identity matrix returns before touching the state: in weak noise a step costs two small launches.
    DIAGONAL  Channel.from_kraus where every K_j has at most one non-zero entry per column (amplitude and phase damping, projective
              and reset-like sets): K_j^+ K_j is diagonal, w_j = sum_d e_j[d] q[d] with e_j[d] = sum_r |K_j[r, d]|^2 and
              q = marginal_probabilities(amps, dims).
    DENSE     any other set from Channel.from_kraus: w_j = Re tr(K_j^+ K_j rho), rho = reduced_density_matrix(amps, dims).

With trace = sum_d q[d] (Re tr rho), scale = sqrt(trace / w_j): the squared norm of the state stays `trace`; renormalize=False
applies K_j itself.  `dims`, `uniform`, `generator` and `device` mean what they mean for measure_: the first listed dim is the
most significant digit, `uniform` is a float in [0, 1) or a float64 GPU tensor of one element, and with device=True a call
synchronises nowhere and returns 0-dim GPU tensors -- the returned j is the int64 at the head of the step's record, so
controlled.when(j, ...) takes it as it takes a measurement outcome.  (A prebuilt ChannelOp only enqueues launches.  channel_
and channel_step_ build a ChannelOp per call: they plan and pack on the host and upload the table from pinned memory with a
non-blocking copy on the current stream, so they do not wait for the device either, but they pay that host work every time.)
The state afterwards is bit for bit apply_wide_gate_(amps, M, dims) for M = K_j * scale (one float64 multiply per component),
and untouched bit for bit where nothing is drawn (j = -1) or an exact identity is drawn with scale == 1.  float64 sums in a
fixed order, no atomics: results are bit-identical from run to run.  There is no CPU fallback.
"""
import ctypes
import itertools
import math

import numpy as np
import torch

from . import _native
from ._state import (_Prebuilt, _checked, _checked_uniform, _desc, _device_uniform, _dims, _dtype_code, _interleaved, _lib, _packed,
                     _ptr)
from .born import marginal_probabilities
from .rdm import reduced_density_matrix

__all__ = ["Channel", "ChannelOp", "channel_", "channel_step_", "channel_info", "depolarizing", "pauli_channel", "bit_flip",
           "phase_flip", "amplitude_damping", "phase_damping"]

_CHECK_BOUND = 1e-10                                           # the bound of measure.apply_channel_


def _matrices(mats, what):
    ms = [np.asarray(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m).astype(np.complex128) for m in mats]
    if not 1 <= len(ms) <= _native.CHANNEL_MAX_OPS:
        raise ValueError(f"{what}: 1 to {_native.CHANNEL_MAX_OPS} operators expected, got {len(ms)}")
    size = ms[0].size
    t = max(size.bit_length() - 1, 0) // 2
    if size != 4 ** t or not 1 <= t <= _native.WGATE_MAX_K:
        raise ValueError(f"{what}: operators are 2^t x 2^t matrices, t = 1..{_native.WGATE_MAX_K}; operator 0 has {size} entries")
    for j, m in enumerate(ms):
        if m.size != size:
            raise ValueError(f"{what}: operator {j} has {m.size} entries, operator 0 has {size}")
        if not np.isfinite(m.view(np.float64)).all():
            raise ValueError(f"{what}: operator {j} has an entry that is not finite")
    return np.stack([m.reshape(2 ** t, 2 ** t) for m in ms]), t


class Channel:
    """m operators on t qubits and the form of their weights.  Build one with Channel.from_kraus, Channel.mixture or a named
    constructor.  `matrices` [m, D, D] complex128 is what the device applies (K_j; the U_j of a mixture), `weights` float64 is
    what the draw reads ([m] p_j, [m, D] e_j or [m, D, D] complex E_j), `kraus` the Kraus operators of the channel
    (K_j = sqrt(p_j) U_j for a mixture), `form` one of "FIXED", "DIAGONAL", "DENSE"."""

    def __init__(self, matrices, weights, form, t):
        self.matrices, self.weights, self.form, self.t, self.m = matrices, weights, form, t, int(matrices.shape[0])

    def __repr__(self):
        return f"Channel(t={self.t}, m={self.m}, form={self.form})"

    @property
    def form_code(self):
        return _native.CHANNEL_FORMS.index(self.form)

    @property
    def kraus(self):
        if self.form == "FIXED":
            return np.sqrt(self.weights)[:, None, None] * self.matrices
        return self.matrices

    @staticmethod
    def from_kraus(kraus, check=True):
        """The channel rho -> sum_j K_j rho K_j^+.  DIAGONAL where every K_j has at most one non-zero entry per column, DENSE
        otherwise.  check=True refuses max |sum_j K_j^+ K_j - I| > 1e-10."""
        what = "Channel.from_kraus"
        ks, t = _matrices(kraus, what)
        D = 2 ** t
        if check:
            gap = float(np.abs(sum(k.conj().T @ k for k in ks) - np.eye(D)).max())
            if not gap <= _CHECK_BOUND:
                raise ValueError(f"{what}: sum_j K_j^+ K_j differs from the identity by {gap:.3e} (above 1e-10): the p_j would be no "
                                 "probabilities -- pass check=False to apply the set as it is")
        if int(((ks != 0).sum(axis=1)).max()) <= 1:            # non-zeros per column, over every operator
            return Channel(ks, (np.abs(ks) ** 2).sum(axis=1), "DIAGONAL", t)
        return Channel(ks, np.stack([k.conj().T @ k for k in ks]), "DENSE", t)

    @staticmethod
    def mixture(probs, unitaries, check=True):
        """The channel rho -> sum_j p_j U_j rho U_j^+, that is K_j = sqrt(p_j) U_j.  check=True refuses a U_j with
        max |U_j^+ U_j - I| > 1e-10 and probabilities with |sum_j p_j - 1| > 1e-10; a negative p_j is always refused."""
        what = "Channel.mixture"
        us, t = _matrices(unitaries, what)
        p = np.asarray(probs, dtype=np.float64).reshape(-1)
        if p.shape[0] != us.shape[0]:
            raise ValueError(f"{what}: {p.shape[0]} probabilities for {us.shape[0]} unitaries")
        if not np.isfinite(p).all() or (p < 0).any():
            raise ValueError(f"{what}: probabilities are finite and not negative, got {p.tolist()}")
        if check:
            gap = abs(float(p.sum()) - 1.0)
            if not gap <= _CHECK_BOUND:
                raise ValueError(f"{what}: the probabilities sum to 1 {'+' if p.sum() > 1 else '-'} {gap:.3e} (above 1e-10)")
            for j, u in enumerate(us):
                gap = float(np.abs(u.conj().T @ u - np.eye(2 ** t)).max())
                if not gap <= _CHECK_BOUND:
                    raise ValueError(f"{what}: U_{j}^+ U_{j} differs from the identity by {gap:.3e} (above 1e-10)")
        return Channel(us, p.copy(), "FIXED", t)


_I = np.eye(2, dtype=np.complex128)
_X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
_Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
_Z = np.array([[1, 0], [0, -1]], dtype=np.complex128)


def _probability(p, name, what):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"{what}: {name} must lie in [0, 1], got {p}")
    return p


def depolarizing(p, n_qubits=1):
    """rho -> (1 - p) rho + p / (4^n - 1) * sum over the 4^n - 1 non-identity Pauli strings P of P rho P^+; n = 1..4.  FIXED;
    operator 0 is the identity, the others the strings in the order I < X < Y < Z, the first qubit the most significant."""
    p, n = _probability(p, "p", "depolarizing"), int(n_qubits)
    if not 1 <= n <= 4:
        raise ValueError(f"depolarizing: n_qubits must lie in 1..4 (4^n operators, at most {_native.CHANNEL_MAX_OPS}), got {n}")
    us = []
    for s in itertools.product((_I, _X, _Y, _Z), repeat=n):
        u = s[0]
        for f in s[1:]:
            u = np.kron(u, f)
        us.append(u)
    rest = p / (4 ** n - 1)
    probs = np.full(4 ** n, rest)
    probs[0] = 1.0 - rest * (4 ** n - 1)
    return Channel.mixture(probs, us, check=False)


def pauli_channel(px, py, pz):
    """rho -> (1 - px - py - pz) rho + px X rho X + py Y rho Y + pz Z rho Z.  FIXED; operators I, X, Y, Z."""
    px, py, pz = (_probability(v, n, "pauli_channel") for v, n in ((px, "px"), (py, "py"), (pz, "pz")))
    p0 = 1.0 - px - py - pz
    if p0 < -_CHECK_BOUND:
        raise ValueError(f"pauli_channel: px + py + pz = {px + py + pz} is above 1")
    return Channel.mixture([max(p0, 0.0), px, py, pz], [_I, _X, _Y, _Z], check=False)


def bit_flip(p):
    """rho -> (1 - p) rho + p X rho X.  FIXED; operators I, X."""
    p = _probability(p, "p", "bit_flip")
    return Channel.mixture([1.0 - p, p], [_I, _X], check=False)


def phase_flip(p):
    """rho -> (1 - p) rho + p Z rho Z.  FIXED; operators I, Z."""
    p = _probability(p, "p", "phase_flip")
    return Channel.mixture([1.0 - p, p], [_I, _Z], check=False)


def amplitude_damping(gamma):
    """K_0 = diag(1, sqrt(1 - gamma)), K_1 = sqrt(gamma) |0><1|.  DIAGONAL."""
    g = _probability(gamma, "gamma", "amplitude_damping")
    return Channel.from_kraus([[[1, 0], [0, math.sqrt(1.0 - g)]], [[0, math.sqrt(g)], [0, 0]]], check=False)


def phase_damping(lam):
    """K_0 = diag(1, sqrt(1 - lam)), K_1 = sqrt(lam) |1><1|.  DIAGONAL."""
    g = _probability(lam, "lam", "phase_damping")
    return Channel.from_kraus([[[1, 0], [0, math.sqrt(1.0 - g)]], [[0, 0], [0, math.sqrt(g)]]], check=False)


_KERNELS = ("artn_channel_apply", "channel kernels")            # what _lib looks for, and what it calls them


def _split(ch, dims, n_dims, what):
    if not isinstance(ch, Channel):
        raise TypeError(f"{what}: a Channel expected, got {type(ch).__name__}")
    dims = _dims(dims, n_dims)
    if int(dims.shape[0]) != ch.t:
        raise ValueError(f"{what}: the channel acts on {ch.t} dims, {int(dims.shape[0])} given")
    weights = _interleaved(ch.weights) if ch.form == "DENSE" else np.ascontiguousarray(ch.weights, dtype=np.float64).reshape(-1)
    return dims, _interleaved(ch.matrices), weights


def _query(d, ch, dims, mats, arrays=False):
    info = _native.ArtnChannelInfo()
    target, tile = np.full(_native.WGATE_MAX_K, -1, dtype=np.int32), np.full(12, -1, dtype=np.int32)
    _native.check(_lib(*_KERNELS, "channel").artn_channel_query(ctypes.byref(d), ch.t, _ptr(dims), ch.m, ch.form_code, _ptr(mats),
                                                                ctypes.byref(info), _ptr(target) if arrays else None,
                                                                _ptr(tile) if arrays else None))
    return info, target, tile


def channel_info(shape, strides, ch, dims, dtype=torch.complex64):
    """Host-only: the plan of one channel step.  t, m, form, target_bits (memory bits of dims in the order listed), tile_bits
    (ascending), tb, n_tiles, segment, lds_bytes, table_bytes, record_bytes, reduction (what the draw reads: None, "marginal" or
    "rdm"), launches (choose + pass; the reduction's launches come on top), launches_by_form, and the nominal bytes of the pass
    (nothing is read or written where an exact identity or nothing is drawn)."""
    _dtype_code(dtype, "channel_info")
    dims, mats, _ = _split(ch, dims, len(shape), "channel_info")
    info, target, tile = _query(_desc(shape, strides, dtype), ch, dims, mats, arrays=True)
    reductions = (None, "marginal", "rdm")
    return {"t": info.t, "m": info.m, "form": _native.CHANNEL_FORMS[info.form],
            "target_bits": tuple(int(b) for b in target[:info.t]), "tile_bits": [int(b) for b in tile[:info.tile_bits]],
            "tb": info.tile_bits, "n_tiles": info.n_tiles, "segment": info.segment, "lds_bytes": info.lds_bytes,
            "table_bytes": info.table_bytes, "record_bytes": info.record_bytes, "reduction": reductions[info.reduction[info.form]],
            "launches": int(info.launches[info.form]),
            "launches_by_form": {_native.CHANNEL_FORMS[f]: int(info.launches[f]) for f in range(3)},
            "bytes_read": info.bytes_read, "bytes_written": info.bytes_written}


def _pack(d, ch, dims, mats, weights):
    """The channel's table (include/artn.h) as a uint8 numpy array."""
    return _packed(_query(d, ch, dims, mats)[0],
                   lambda *table: _lib(*_KERNELS, "channel").artn_channel_pack(ctypes.byref(d), ch.t, _ptr(dims), ch.m, ch.form_code,
                                                                               _ptr(mats), _ptr(weights), *table))


class ChannelOp(_Prebuilt):
    """One channel on `dims` for tensors of one layout.  Validates, plans, packs the table and copies it to `device` once;
    op(amps, uniform=None, generator=None, renormalize=True, device=False) then performs one trajectory step on amps IN PLACE and
    returns (j, p) as channel_ does; op.step(amps, ...) returns the step's record instead."""

    def __init__(self, shape, strides, dtype, ch, dims, device):
        self._bind(shape, strides, dtype, device)
        self._dims, mats, weights = _split(ch, dims, len(self.shape), "ChannelOp")
        self.channel, self.t, self.m, self.form = ch, ch.t, ch.m, ch.form
        self.dims = tuple(int(x) for x in self._dims)
        self._d = _desc(self.shape, self.strides, dtype)
        table, info = _pack(self._d, ch, self._dims, mats, weights)
        self.table_bytes, self.record_bytes, self.tile_bits, self.n_tiles = info.table_bytes, info.record_bytes, info.tile_bits, info.n_tiles
        self._upload(table)

    def _upload(self, table):
        # (pinned and non-blocking: a pageable copy would make the host wait for the stream, and channel_ builds a ChannelOp per call)
        self._table = torch.from_numpy(table).pin_memory().to(self.device, non_blocking=True)

    def step(self, amps, uniform=None, generator=None, renormalize=True):
        """One step, enqueued on the current stream without a host synchronisation.  Returns the record as a float64 GPU tensor of
        4 + 2 * 4^t: [j (the bits of an int64: record.view(torch.int64)[0]), probability w_j / total, total, scale], then the
        current matrix K_j * scale as (Re, Im) pairs, row-major."""
        what = "channel.ChannelOp"
        _checked_uniform(uniform, what)
        self._check(amps, what)
        dev, lib = amps.device, _lib(*_KERNELS, what)
        src = None
        if self.form == "DIAGONAL":
            src = marginal_probabilities(amps, self.dims)
        elif self.form == "DENSE":
            src = reduced_density_matrix(amps, self.dims)
        u = _device_uniform(uniform, generator, dev)
        rec = torch.empty(self.record_bytes // 8, dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            stream = _native.current_stream_ptr(dev)
            _native.check(lib.artn_channel_choose(self._table.data_ptr(), self.table_bytes, self.t, self.m, self.channel.form_code,
                                                  None if src is None else src.data_ptr(), u.data_ptr(), int(bool(renormalize)),
                                                  rec.data_ptr(), self.record_bytes, stream))
            _native.check(lib.artn_channel_apply(ctypes.byref(self._d), amps.data_ptr(), self.t, _ptr(self._dims), self.m,
                                                 self._table.data_ptr(), self.table_bytes, rec.data_ptr(), self.record_bytes,
                                                 stream))
        return rec

    def __call__(self, amps, uniform=None, generator=None, renormalize=True, device=False):
        return _result(self.step(amps, uniform, generator, renormalize), device, "channel.ChannelOp")


def _result(rec, device, what):
    if device:
        return rec.view(torch.int64)[0], rec[1]
    host = rec[:4].cpu()                                       # the one synchronisation: 32 bytes
    j, p = int(host.view(torch.int64)[0]), float(host[1])
    if j < 0:
        raise ValueError(f"{what}: nothing can be drawn (sum_j w_j = {float(host[2])!r}, or the state has no norm); the state is "
                         "unchanged")
    return j, p


def channel_step_(amps, ch, dims, uniform=None, generator=None, renormalize=True):
    """ChannelOp(...).step(amps, ...): one step without a host synchronisation; returns the record (a float64 GPU tensor)."""
    if isinstance(amps, torch.Tensor):                        # the argument errors come before any device work
        _split(ch, dims, amps.dim(), "channel.channel_step_")
    _checked_uniform(uniform, "channel.channel_step_")
    _checked(amps, "channel.channel_step_")
    return ChannelOp(amps.shape, amps.stride(), amps.dtype, ch, dims, amps.device).step(amps, uniform, generator, renormalize)


def channel_(amps, ch, dims, uniform=None, generator=None, renormalize=True, device=False):
    """One trajectory step of `ch` on `dims` of amps, in place.  Returns (j, p), p = w_j / sum_j w_j: Python int and float, or
    with device=True 0-dim GPU tensors (int64, float64) without a host synchronisation.  device=False raises ValueError where
    nothing could be drawn (the state is unchanged then); device=True returns j = -1 and p = 0.  (Plans and uploads per call:
    build a ChannelOp once to apply the same channel repeatedly.)"""
    return _result(channel_step_(amps, ch, dims, uniform, generator, renormalize), device, "channel.channel_")
