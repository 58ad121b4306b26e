"""Born statistics of an amplitude tensor on the device: overlap / norm / fidelity, marginal
probabilities and bitstring sampling (C ABI: the artn_born_* and artn_marginal* entry points).

Every function takes a GPU tensor of complex64 or complex128 and works on its MEMORY layout: the
tensor must be dense (its strides a permutation of a contiguous layout -- exactly what
`collect.permute(permute_dims)` at the end of `TensorNetworkSimulation.contraction` returns), it
is never copied, and indices are translated between memory order and the logical dims.  All sums
are float64 in a fixed order: results are bit-identical from run to run.  There is no CPU
fallback.
"""
import ctypes

import torch

from . import _native
from ._state import _DTYPES, _checked, _dense_layout

__all__ = ["born_plan", "overlap", "norm2", "fidelity", "block_sums", "marginal_info", "marginal_probabilities", "sample",
           "linear_xeb", "memory_to_multi_index"]


def memory_to_multi_index(mem_index, shape, strides):
    """Logical multi-index [..., len(shape)] of flat MEMORY indices of a dense layout (torch or numpy int64 arrays)."""
    _dense_layout(shape, strides)
    cols = [(mem_index // int(s)) % int(e) if int(e) != 1 else mem_index * 0 for e, s in zip(shape, strides)]
    if isinstance(mem_index, torch.Tensor):
        return torch.stack(cols, dim=-1) if cols else mem_index.new_zeros(mem_index.shape + (0,))
    import numpy as np
    return np.stack(cols, axis=-1) if cols else np.zeros(np.shape(mem_index) + (0,), dtype=np.int64)


def born_plan(n, dtype=torch.complex64):
    """Host-only: block size, block count and workspace of the Born kernels for n elements."""
    p = _native.ArtnBornPlan()
    _native.check(_native.lib().artn_born_plan(int(n), _DTYPES[dtype], ctypes.byref(p)))
    return {"block_bits": p.block_bits, "n_blocks": p.n_blocks, "overlap_grid": p.overlap_grid,
            "workspace_bytes": p.workspace_bytes}


def _overlap4(a, b, what):
    n = _checked(a, what)
    if b is not None and b is not a:
        _checked(b, what)
        if b.dtype != a.dtype or b.device != a.device:
            raise ValueError(f"{what}: a and b must share dtype and device")
        if tuple(a.shape) != tuple(b.shape) or tuple(a.stride()) != tuple(b.stride()):
            raise ValueError(f"{what}: a and b must have equal shapes and equal strides (got {tuple(a.shape)}/{tuple(a.stride())} "
                             f"and {tuple(b.shape)}/{tuple(b.stride())})")
    plan = born_plan(n, a.dtype)
    ws = torch.empty(plan["workspace_bytes"] // 8, dtype=torch.float64, device=a.device)
    out = torch.empty(4, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _native.check(_native.lib().artn_born_overlap(
            a.data_ptr(), None if b is None or b is a else b.data_ptr(), n, _DTYPES[a.dtype], ws.data_ptr(),
            plan["workspace_bytes"], out.data_ptr(), _native.current_stream_ptr(a.device)))
    return out


def overlap(a, b, device=False):
    """(<a|b>, |a|^2, |b|^2) in one pass over both tensors, float64 accumulation.  device=True: the float64 tensor
    [Re<a|b>, Im<a|b>, |a|^2, |b|^2] on the GPU, without a host synchronisation."""
    out = _overlap4(a, b, "born.overlap")
    if device:
        return out
    re, im, na, nb = out.tolist()
    return complex(re, im), na, nb


def norm2(a, device=False):
    """sum |a|^2 (one read of the tensor).  device=True: a 0-dim float64 GPU tensor, no host synchronisation."""
    out = _overlap4(a, None, "born.norm2")
    return out[2] if device else float(out[2])


def fidelity(a, b, device=False):
    """|<a|b>|^2 / (|a|^2 |b|^2).  (The reference's notebook, examples/sycamore.ipynb cell 7, prints the square root of
    this number.)"""
    out = _overlap4(a, b, "born.fidelity")
    f = (out[0] * out[0] + out[1] * out[1]) / (out[2] * out[3])
    return f if device else float(f)


def block_sums(amps):
    """(block_sum, prefix): float64 sums of |a|^2 over blocks of 2^block_bits consecutive MEMORY elements and their
    inclusive prefix sums (born_plan says how many)."""
    n = _checked(amps, "born.block_sums")
    plan = born_plan(n, amps.dtype)
    bs = torch.empty(plan["n_blocks"], dtype=torch.float64, device=amps.device)
    prefix = torch.empty_like(bs)
    with torch.cuda.device(amps.device):
        _native.check(_native.lib().artn_born_block_sums(amps.data_ptr(), n, _DTYPES[amps.dtype], bs.data_ptr(),
                                                         prefix.data_ptr(), _native.current_stream_ptr(amps.device)))
    return bs, prefix


def _marginal_desc(shape, strides, keep, dtype):
    nd = len(shape)
    keep = [int(k) + nd if int(k) < 0 else int(k) for k in keep]
    if any(k < 0 or k >= nd for k in keep) or len(set(keep)) != len(keep):
        raise ValueError(f"keep must name distinct dims of a {nd}-dim tensor, got {keep}")
    if nd > _native.ARTN_MAX_LABELS:
        raise ValueError(f"at most {_native.ARTN_MAX_LABELS} dims")
    d = _native.ArtnMarginalDesc()
    d.dtype, d.n_dims = _DTYPES[dtype], nd
    for pos, dim in enumerate(keep + [x for x in range(nd) if x not in keep]):   # kept dims first, in the order asked for
        d.extent[pos], d.stride[pos], d.keep[pos] = int(shape[dim]), int(strides[dim]), int(pos < len(keep))
    return d, keep


def marginal_info(shape, strides, keep, dtype=torch.complex64):
    """Host-only: which kernel a marginal takes, its workspace and output size (RuntimeError where the library refuses)."""
    d, _ = _marginal_desc(shape, strides, keep, dtype)
    info = _native.ArtnMarginalInfo()
    _native.check(_native.lib().artn_marginal_query(ctypes.byref(d), ctypes.byref(info)))
    return {"kernel": info.kernel, "chunk_bits": info.chunk_bits, "bin_bits": info.bin_bits, "grid": info.grid,
            "workspace_bytes": info.workspace_bytes, "out_elems": info.out_elems}


def marginal_probabilities(amps, keep, normalize=False):
    """float64 tensor of shape [amps.shape[d] for d in keep]: |amps|^2 summed over every other dim.  keep=() gives the
    0-dim norm; a leading row dimension of a sparse result is a dim like any other."""
    _checked(amps, "born.marginal_probabilities")
    d, keep = _marginal_desc(amps.shape, amps.stride(), keep, amps.dtype)
    info = _native.ArtnMarginalInfo()
    _native.check(_native.lib().artn_marginal_query(ctypes.byref(d), ctypes.byref(info)))
    out = torch.empty([amps.shape[k] for k in keep], dtype=torch.float64, device=amps.device)
    ws = torch.empty(max(info.workspace_bytes // 8, 1), dtype=torch.float64, device=amps.device)
    with torch.cuda.device(amps.device):
        _native.check(_native.lib().artn_marginal(ctypes.byref(d), amps.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                  info.workspace_bytes, _native.current_stream_ptr(amps.device)))
    return out / out.sum() if normalize else out


def _checked_uniforms(uniforms):
    if not isinstance(uniforms, torch.Tensor) or uniforms.dtype != torch.float64 or uniforms.dim() != 1:
        raise ValueError("uniforms must be a 1-dim float64 tensor")
    if uniforms.numel() and not bool(((uniforms >= 0) & (uniforms < 1)).all()):
        raise ValueError("uniforms must lie in [0, 1)")
    return uniforms


def sample(amps, n_samples=None, *, uniforms=None, generator=None):
    """Draw multi-indices with probability |amps[idx]|^2 / total.

    Returns (indices, probabilities): int64 [m, amps.dim()] multi-indices in the tensor's logical dim order (for a
    [2]*n result the bitstrings, first qubit first; for a closed sparse result [rows] the row numbers into
    bitstrings_sorted) and float64 [m] probabilities.  `uniforms` (float64 in [0, 1), any order; output s belongs to
    uniforms[s]) is the explicit form: sample s is the element whose cumulative-probability interval, in memory order,
    contains uniforms[s].  Otherwise torch.rand(n_samples, dtype=float64, generator=generator) on the device supplies
    them."""
    if uniforms is not None:
        uniforms = _checked_uniforms(uniforms)
        if n_samples is not None and int(n_samples) != uniforms.numel():
            raise ValueError("n_samples disagrees with len(uniforms)")
    elif n_samples is None or int(n_samples) < 0:
        raise ValueError("give n_samples or uniforms")
    n = _checked(amps, "born.sample")
    dev = amps.device
    if uniforms is None:
        uniforms = torch.rand(int(n_samples), dtype=torch.float64, device=dev, generator=generator)
    uniforms = uniforms.to(dev)
    m = uniforms.numel()
    _, prefix = block_sums(amps)
    total = prefix[-1]
    targets, order = torch.sort(uniforms * total)          # ascending: a block is read once for all its samples
    flat_sorted = torch.empty(m, dtype=torch.int64, device=dev)
    prob_sorted = torch.empty(m, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().artn_born_pick(amps.data_ptr(), n, _DTYPES[amps.dtype], prefix.data_ptr(), targets.data_ptr(),
                                                   m, flat_sorted.data_ptr(), prob_sorted.data_ptr(),
                                                   _native.current_stream_ptr(dev)))
    if not float(total) > 0.0:
        raise ValueError("cannot sample: every amplitude is zero (or the norm is not finite)")
    flat = torch.empty_like(flat_sorted)
    flat[order] = flat_sorted
    prob = torch.empty_like(prob_sorted)
    prob[order] = prob_sorted / total
    return memory_to_multi_index(flat, amps.shape, amps.stride()), prob


def linear_xeb(probabilities, n_qubits):
    """Linear cross-entropy benchmark 2^n * mean(p) - 1 of the ideal probabilities of the drawn bitstrings."""
    return float(2.0 ** int(n_qubits) * probabilities.to(torch.float64).mean() - 1.0)
