"""Projective measurement of a few qubits of an amplitude tensor on the device, IN PLACE: measure, post-select, reset (C ABI:
artn_measure_query, artn_measure_choose, artn_measure_collapse), and one quantum-trajectory step of a Kraus channel.

`dims` are 1 to 10 distinct dims of `amps`, each of extent 2 (negative dims count from the end).  An outcome is the integer whose
most significant digit is the first listed dim -- the convention of reduced_density_matrix and apply_gate_.  With
q = marginal_probabilities(amps, dims).reshape(-1) and total = q[0] + q[1] + ..., outcome o has probability q[o] / total.

    measure_     draws o (the smallest o whose inclusive running sum of q exceeds uniform * total; never one with q[o] == 0),
                 zero-fills every element whose measured digits differ from o and scales the rest
    postselect_  the same with o given
    reset_       draws as measure_ does, then leaves new[r, 0..0] = a[r, o] * scale and +0.0 everywhere else: bit for bit
                 postselect_ followed by pauli_apply_ of X on the set digits of o

renormalize=True scales by sqrt(total / q[o]), so the squared norm of the state stays `total`; renormalize=False leaves the kept
elements unchanged bit for bit.  Projected elements are WRITTEN as +0.0 and never read: -0.0, denormals and non-finite values
there vanish.  Every kept component c becomes float64(c) * scale, rounded once.

The outcome is chosen ON THE DEVICE and the collapse reads it from device memory: with device=True a call enqueues the marginal,
the choice and the collapse on the current stream, returns 0-dim GPU tensors (int64 outcome, float64 probability) and
synchronises nowhere; with device=False it ends with one device-to-host copy of the 32-byte record and returns (int, float).
Where nothing can be observed -- total is not finite or not > 0, or a post-selected q[o] is 0 -- the state is left untouched bit
for bit; device=False raises ValueError, device=True returns outcome -1 and probability 0.

The functions take what pauli.py takes -- a dense GPU tensor of complex64 or complex128 with power-of-two extents in any permuted
layout, 16-byte aligned, never copied.  The sums are float64 in a fixed order: bit-identical from run to run.  There is no CPU
fallback.
"""
import ctypes
import math

import numpy as np
import torch

from . import _native
from ._state import _checked, _checked_uniform, _dense_layout, _device_uniform, _dtype_code, _lib
from .born import _marginal_desc, marginal_probabilities
from .gates import apply_gate_
from .rdm import reduced_density_matrix

__all__ = ["measure_info", "measure_", "postselect_", "reset_", "collapse_", "apply_channel_", "choose_outcome"]


def _dims(shape, dims, what):
    """The measured dims as a list of non-negative ints; ValueError unless they are 1..10 distinct dims of extent 2."""
    nd = len(shape)
    dims = [dims] if isinstance(dims, (int, np.integer)) else list(dims)
    dims = [int(x) + nd if -nd <= int(x) < 0 else int(x) for x in dims]
    if not 1 <= len(dims) <= _native.MEASURE_MAX_DIMS:
        raise ValueError(f"{what}: 1 to {_native.MEASURE_MAX_DIMS} dims are measured in one call, got {len(dims)} "
                         "(measuring in groups gives the same distribution)")
    if any(x < 0 or x >= nd for x in dims) or len(set(dims)) != len(dims):
        raise ValueError(f"{what}: dims must name distinct dims of a {nd}-dim tensor, got {dims}")
    for x in dims:
        if int(shape[x]) != 2:
            raise ValueError(f"{what}: a measured dim has extent 2; dim {x} has extent {int(shape[x])}")
    return dims


def _plan(shape, strides, dims, dtype, what):
    _dtype_code(dtype, what)
    dims = _dims(shape, dims, what)
    _dense_layout(shape, strides)
    d, _ = _marginal_desc(shape, strides, dims, dtype)
    info = _native.ArtnMeasureInfo()
    _native.check(_native.lib().artn_measure_query(ctypes.byref(d), ctypes.byref(info)))
    return d, dims, info


def measure_info(shape, strides, dims, dtype=torch.complex64):
    """Host-only: the memory bit of every measured dim (in listed order), k, D = 2^k, the grid, the launches of a collapse (1) and
    of a reset (2), the record size, and the nominal bytes of either: all n elements written, the n / D kept ones read.
    (ValueError for dims that cannot be measured or a layout that is not dense; RuntimeError where the library refuses.)"""
    _, _, info = _plan(shape, strides, dims, dtype, "measure_info")
    return {"k": info.k, "dim": info.dim, "n": info.n, "memory_bits": [int(info.mem_bit[j]) for j in range(info.k)],
            "grid": info.grid, "collapse_launches": info.collapse_launches, "reset_launches": info.reset_launches,
            "record_bytes": info.record_bytes, "bytes_read": info.bytes_read, "bytes_written": info.bytes_written}


def collapse_(amps, dims, outcome=None, uniform=None, generator=None, renormalize=True, reset=False):
    """The work of measure_ / postselect_ / reset_, enqueued on the current stream without a host synchronisation.  Returns the
    record as a float64 GPU tensor of 4: [outcome (the bits of an int64: record.view(torch.int64)[0]), probability, total,
    scale].  outcome=None draws with `uniform` / `generator`; an int post-selects."""
    what = "measure.collapse_"
    if not isinstance(amps, torch.Tensor):
        _native.require_gpu(amps, what)
    dims = _dims(amps.shape, dims, what)
    if outcome is None:
        _checked_uniform(uniform, what)
        forced = -1
    else:
        forced = int(outcome)
        if not 0 <= forced < 2 ** len(dims):
            raise ValueError(f"{what}: outcome {forced} of {len(dims)} measured dims (0 .. {2 ** len(dims) - 1} expected)")
    _checked(amps, what)
    lib = _lib("artn_measure_collapse", "measurement kernels", what)
    d, dims, info = _plan(amps.shape, amps.stride(), dims, amps.dtype, what)
    dev = amps.device
    q = marginal_probabilities(amps, dims)
    u = _device_uniform(uniform, generator, dev) if forced < 0 else None
    rec = torch.empty(_native.MEASURE_RECORD_BYTES // 8, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = _native.current_stream_ptr(dev)
        _native.check(lib.artn_measure_choose(q.data_ptr(), info.dim, None if u is None else u.data_ptr(), forced,
                                              int(bool(renormalize)), rec.data_ptr(), stream))
        _native.check(lib.artn_measure_collapse(ctypes.byref(d), amps.data_ptr(), rec.data_ptr(), int(bool(reset)), stream))
    return rec


def _result(rec, device, what):
    if device:
        return rec.view(torch.int64)[0], rec[1]
    host = rec.cpu()                                           # the one synchronisation: 32 bytes
    o, p = int(host.view(torch.int64)[0]), float(host[1])
    if o < 0:
        raise ValueError(f"{what}: nothing can be observed (sum |amps|^2 = {float(host[2])!r} over the measured outcomes, or the "
                         "post-selected outcome has probability 0); the state is unchanged")
    return o, p


def measure_(amps, dims, uniform=None, generator=None, renormalize=True, device=False):
    """Measure `dims` in place.  Returns (outcome, probability): Python int and float, or with device=True 0-dim GPU tensors
    (int64, float64) without a host synchronisation.  `uniform` is a float in [0, 1) or a float64 GPU tensor of one element;
    None draws torch.rand(1, dtype=float64, generator=generator) on the device."""
    return _result(collapse_(amps, dims, None, uniform, generator, renormalize, False), device, "measure.measure_")


def postselect_(amps, dims, outcome, renormalize=True, device=False):
    """Project `dims` onto `outcome` in place.  Returns its probability (device=True: a 0-dim float64 GPU tensor, 0 where the
    outcome cannot be observed)."""
    if outcome is None:
        raise ValueError("measure.postselect_: an outcome is needed")
    return _result(collapse_(amps, dims, outcome, None, None, renormalize, False), device, "measure.postselect_")[1]


def reset_(amps, dims, uniform=None, generator=None, renormalize=True, device=False):
    """Measure `dims` and put them back to 0 in place: new[r, 0..0] = a[r, o] * scale.  Returns the (outcome, probability) that
    was observed, as measure_ does."""
    return _result(collapse_(amps, dims, None, uniform, generator, renormalize, True), device, "measure.reset_")


def choose_outcome(q, uniform):
    """The choice rule on the host (numpy float64): the smallest o whose inclusive running sum of q exceeds uniform * total, or
    the last o with q[o] > 0 where rounding leaves none; -1 where total is not finite or not > 0.  Returns (o, total)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    cum = np.cumsum(q)                                         # sequential, ascending: the device's order
    total = float(cum[-1])
    if not (math.isfinite(total) and total > 0.0):
        return -1, total
    hit = np.nonzero((cum > float(uniform) * total) & (q > 0.0))[0]
    live = np.nonzero(q > 0.0)[0]
    return int(hit[0] if hit.size else live[-1]), total


def _kraus(kraus, k, check, what):
    ks = [np.asarray(m.detach().cpu().numpy() if isinstance(m, torch.Tensor) else m).astype(np.complex128) for m in kraus]
    if not ks:
        raise ValueError(f"{what}: at least one Kraus operator is needed")
    D = 2 ** k
    for j, m in enumerate(ks):
        if m.size != D * D:
            raise ValueError(f"{what}: Kraus operator {j} has {m.size} entries for {k} dims ({D} x {D} expected)")
    ks = [m.reshape(D, D) for m in ks]
    if check:
        gap = float(np.abs(sum(m.conj().T @ m for m in ks) - np.eye(D)).max())
        if not gap <= 1e-10:
            raise ValueError(f"{what}: sum_j K_j^+ K_j differs from the identity by {gap:.3e} (above 1e-10): the p_j would be no "
                             "probabilities -- pass check=False to apply the set as it is")
    return ks


def apply_channel_(amps, kraus, dims, uniform=None, generator=None, check=True):
    """One quantum-trajectory step of the channel {K_j} on one or two dims, in place: draws j with probability
    p_j = Re tr(K_j^+ K_j rho) / Re tr(rho), rho = reduced_density_matrix(amps, dims), by the rule of measure_, then applies
    apply_gate_(amps, K_j / sqrt(p_j), dims).  Returns (j, p_j) as Python int and float.  Pure Python over existing calls: rho goes
    to the host, so this call synchronises.  check=True refuses a set with max |sum_j K_j^+ K_j - I| > 1e-10."""
    what = "measure.apply_channel_"
    if not isinstance(amps, torch.Tensor):
        _native.require_gpu(amps, what)
    dims = _dims(amps.shape, dims, what)
    if len(dims) > 2:
        raise ValueError(f"{what}: channels act on one or two dims, got {len(dims)}")
    ks = _kraus(kraus, len(dims), check, what)
    _checked_uniform(uniform, what)
    _checked(amps, what)
    rho = reduced_density_matrix(amps, dims).cpu().numpy()
    tr = float(np.trace(rho).real)
    w = np.array([float(np.trace(m.conj().T @ m @ rho).real) for m in ks], dtype=np.float64)
    u = float(_device_uniform(uniform, generator, amps.device).item())
    j, total = choose_outcome(np.maximum(w, 0.0), u)
    if j < 0 or not (math.isfinite(tr) and tr > 0.0):
        raise ValueError(f"{what}: nothing can be drawn (tr rho = {tr!r}, sum_j w_j = {total!r}); the state is unchanged")
    p = float(w[j] / tr)
    apply_gate_(amps, ks[j] / math.sqrt(p), dims)
    return j, p
