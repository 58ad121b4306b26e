"""What the state modules (adjoint born channel controlled diagonal gate_adjoint gates krylov layout measure pauli rdm trajectories wide_gates)
share on the host: the checks of a tensor and of a dtype, the layout descriptor, the marshalling of dims, matrices and packed
tables, and the base class of the objects that are built once for tensors of one layout.  A family's wrapper writes its argument
split, its query and pack calls and its apply call; everything else it takes from here.  This module imports no state module.
"""
import ctypes

import numpy as np
import torch

from . import _native

_DTYPES = {torch.complex64: _native.ARTN_C64, torch.complex128: _native.ARTN_C128}


def _dtype_code(dtype, what):
    """The ARTN_* code of a complex dtype; TypeError for any other."""
    if dtype not in _DTYPES:
        raise TypeError(f"{what}: complex64 or complex128 expected, got {dtype}")
    return _DTYPES[dtype]


def _dense_layout(shape, strides):
    """Number of elements of a dense layout; ValueError when the strides are not a permutation of a contiguous layout."""
    n = 1
    for e, s in sorted(((int(e), int(s)) for e, s in zip(shape, strides) if e != 1), key=lambda p: p[1]):
        if e < 1:
            raise ValueError("Born statistics of an empty tensor are undefined")
        if s != n:
            raise ValueError(f"the tensor is not dense (shape {tuple(shape)}, strides {tuple(strides)}): its strides are not a "
                             "permutation of a contiguous layout -- pass amps.contiguous()")
        n *= e
    return n


def _checked(t, what):
    _native.require_gpu(t, what)
    if t.dtype not in _DTYPES:
        raise TypeError(f"{what}: complex64 or complex128 amplitudes expected, got {t.dtype}")
    n = _dense_layout(t.shape, t.stride())
    if t.data_ptr() % 16:
        raise ValueError(f"{what}: the tensor's memory must start on a 16-byte boundary (this view starts at an odd element "
                         "of its storage) -- pass amps.contiguous().clone()")
    return n


def _overlaps(a, b):
    """Whether the memory of two tensors of one dense layout intersects."""
    nbytes = b.numel() * b.element_size()
    return a.data_ptr() < b.data_ptr() + nbytes and b.data_ptr() < a.data_ptr() + nbytes


def _desc(shape, strides, dtype):
    nd = len(shape)
    if nd > _native.ARTN_MAX_LABELS:
        raise ValueError(f"at most {_native.ARTN_MAX_LABELS} dims")
    d = _native.ArtnMarginalDesc()
    d.dtype, d.n_dims = _DTYPES[dtype], nd
    for pos in range(nd):                                     # the caller's dim order; keep[] is not read
        d.extent[pos], d.stride[pos] = int(shape[pos]), int(strides[pos])
    return d


def _ptr(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def _max_rank(max_rank):
    return -1 if max_rank is None else int(max_rank)


def _dims(dims, n_dims):
    dims = [int(dims)] if isinstance(dims, (int, np.integer)) else [int(x) for x in dims]
    return np.array([x + n_dims if -n_dims <= x < 0 else x for x in dims], dtype=np.int32)


def _interleaved(z):
    """float64 (Re, Im) pairs of a complex array, row-major."""
    z = np.ascontiguousarray(z, dtype=np.complex128)
    return z.view(np.float64).reshape(-1).copy()


def _lib(symbol, family, what):
    """The library, once it is known to hold the kernels of a family (`symbol` is one of their entry points)."""
    if not _native.has(symbol):
        raise RuntimeError(f"{what}: the loaded library has no {family} -- rebuild it with `make`")
    return _native.lib()


def _packed(info, pack):
    """(table, info): the table of info.table_bytes (include/artn.h) as a uint8 numpy array on an 8-byte boundary, filled by
    pack(pointer, bytes) -- the family's artn_*_pack with its own arguments in front."""
    table = np.zeros(info.table_bytes // 8, dtype=np.uint64)
    _native.check(pack(_ptr(table), info.table_bytes))
    return table.view(np.uint8), info


def _checked_uniform(uniform, what):
    """Host-only validation of `uniform`: None, a float in [0, 1), or a float64 GPU tensor of one element (its value is not read)."""
    if uniform is None:
        return
    if isinstance(uniform, torch.Tensor):
        if uniform.dtype != torch.float64 or uniform.numel() != 1 or not uniform.is_cuda:
            raise ValueError(f"{what}: a uniform tensor is float64, on the GPU, with one element")
        return
    u = float(uniform)
    if not 0.0 <= u < 1.0:
        raise ValueError(f"{what}: uniform must lie in [0, 1), got {u}")


def _device_uniform(uniform, generator, device):
    if uniform is None:
        return torch.rand(1, dtype=torch.float64, device=device, generator=generator)
    if isinstance(uniform, torch.Tensor):
        return uniform.to(device).reshape(1).contiguous()
    return torch.full((1,), float(uniform), dtype=torch.float64, device=device)   # (a fill: no host-to-device copy)


class _Prebuilt:
    """An object built once for tensors of one layout: it keeps shape, strides, dtype and device, and its packed table on the
    device in `_table` (None where there is nothing to launch)."""

    def _bind(self, shape, strides, dtype, device):
        """The head of a constructor.  The messages carry the bare class name."""
        name = type(self).__name__
        _dtype_code(dtype, name)
        self.shape, self.strides, self.dtype = tuple(int(e) for e in shape), tuple(int(s) for s in strides), dtype
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{name}: artensor_amd executes on MI355X only (got device {self.device}); there is no CPU fallback")

    def _upload(self, table):
        self._table = torch.from_numpy(table).to(self.device)

    def _check(self, x, what):
        """The head of a call, `what` the module-qualified name: x is what born.py takes, lies as the object was built for, and
        lives where the table lives (read now, not when the object was built)."""
        _checked(x, what)
        if tuple(x.shape) != self.shape or tuple(x.stride()) != self.strides or x.dtype != self.dtype:
            raise ValueError(f"{what}: built for shape {self.shape}, strides {self.strides}, {self.dtype}; got "
                             f"{tuple(x.shape)}, {tuple(x.stride())}, {x.dtype}")
        if self._table is not None and x.device != self._table.device:
            raise ValueError(f"{what}: built for {self._table.device}, got a tensor on {x.device}")


# ---- the run circuits: PauliCircuit, GateCircuit and their two-state forms PauliPairCircuit, GatePairCircuit ---------------------
def _run_query(entry, info, d, operands, max_rank, outputs, arrays):
    """One artn_*_query of a run circuit, entry(d, *operands, n, max_rank, info, *outputs): (info,) with nulls for the outputs, or
    with arrays=True (info, *outputs), a zeroed numpy array per (dtype, width) of `outputs` -- one row per step or gate (the run
    arrays too: a circuit has no more runs than that), width 0 for a flat one."""
    n = operands[0].shape[0]
    out = tuple(np.zeros((n, w) if w else n, dtype=t) for t, w in outputs) if arrays else ()
    ptrs = [_ptr(x) for x in out] if arrays else [None] * len(outputs)
    _native.check(getattr(_native.lib(), entry)(ctypes.byref(d), *[_ptr(x) for x in operands], n, max_rank, ctypes.byref(info), *ptrs))
    return (info,) + out


def _run_pack(query, entry, d, operands, max_rank):
    """(table, info) of a run circuit: query(d, *operands, max_rank) sizes the table that entry(d, *operands, n, max_rank, ...) fills."""
    return _packed(query(d, *operands, max_rank)[0],
                   lambda *table: getattr(_native.lib(), entry)(ctypes.byref(d), *[_ptr(x) for x in operands], operands[0].shape[0],
                                                                max_rank, *table))


def _run_keys(info, rank, **run_lists):
    """What the info dict of every run circuit says of the runs and of the whole circuit; run_lists: key -> its [n, MAX_RANK] array."""
    nr = info.n_runs
    ranks = [int(v) for v in rank[:nr]]
    keys = {"n_measured": info.n_measured} if hasattr(info, "n_measured") else {}
    keys.update(n_runs=nr, n_launches=info.n_launches, max_rank=info.max_rank, run_rank=ranks)
    keys.update((key, [[int(v) for v in a[r, :ranks[r]]] for r in range(nr)]) for key, a in run_lists.items())
    keys.update((key, getattr(info, key)) for key in ("table_bytes", "workspace_bytes", "bytes_read", "bytes_written") if hasattr(info, key))
    return keys


class _RunCircuit(_Prebuilt):
    """A circuit that the library applies in place as LDS-resident runs, built once for tensors of one layout."""

    def _build(self, shape, strides, dtype, device, max_rank, split, query, pack):
        """The constructor.  split(n_dims): the operands in the order of the library's entries; query(d, *operands, max_rank) and
        the name of the pack entry.  Returns (operands, info): the subclass keeps what its calls pass again, under its own names."""
        self._bind(shape, strides, dtype, device)
        operands = split(len(self.shape))
        self._d, self._max_rank = _desc(self.shape, self.strides, dtype), _max_rank(max_rank)
        table, info = _run_pack(query, pack, self._d, operands, self._max_rank)
        self._n, self.n_runs, self.max_rank, self.table_bytes = operands[0].shape[0], info.n_runs, info.max_rank, info.table_bytes
        self._upload(table)
        return operands, info

    def _run(self, what, entry, amps, *operands):
        """amps updated in place by entry(d, amps, *operands, n, max_rank, table, ...); returns amps."""
        self._check(amps, what)
        with torch.cuda.device(amps.device):
            _native.check(getattr(_native.lib(), entry)(ctypes.byref(self._d), amps.data_ptr(), *operands, self._n, self._max_rank,
                                                        self._table.data_ptr(), self.table_bytes,
                                                        _native.current_stream_ptr(amps.device)))
        return amps


class _PairCircuit(_RunCircuit):
    """... on two tensors, with the transition element of every measured step or gate; the workspace is allocated per call."""

    def _build(self, *args):
        operands, info = super()._build(*args)
        self.workspace_bytes = info.workspace_bytes
        return operands, info

    def _run(self, what, entry, lam, phi, device, *operands):
        """Both updated in place by entry(d, lam, phi, *operands, n, max_rank, table, workspace, out, ...); returns t."""
        for x in (lam, phi):
            self._check(x, what)
        if _overlaps(lam, phi):
            raise ValueError(f"{what}: lam overlaps phi")
        out = torch.empty((self._n, 2), dtype=torch.float64, device=phi.device)
        ws = torch.empty(self.workspace_bytes // 8, dtype=torch.float64, device=phi.device)   # (per call: calls may overlap on streams)
        with torch.cuda.device(phi.device):
            _native.check(getattr(_native.lib(), entry)(ctypes.byref(self._d), lam.data_ptr(), phi.data_ptr(), *operands, self._n,
                                                        self._max_rank, self._table.data_ptr(), self.table_bytes, ws.data_ptr(),
                                                        self.workspace_bytes, out.data_ptr(), _native.current_stream_ptr(phi.device)))
        return out if device else out.cpu().numpy().view(np.complex128).reshape(self._n)
