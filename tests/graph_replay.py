"""The harness of tests/test_graph_replay_gpu.py: capture one operation into a HIP graph, replay it on changing contents, and
compare every replay bit for bit with an eager run of the same call on the default stream.

An operation is `op(*tensors) -> tensor | tuple of tensors | None` on STATIC device tensors (amplitudes, uniforms): the graph
bakes their addresses in, so a replay sees whatever was copied into them last.  Everything the operation needs besides them
(compiled objects, tables) is built by the caller before capture.  The capture runs on torch's own capture stream -- one stream,
no event fork or join -- so every case is a side-stream run as well.
"""
import numpy as np
import torch

DEV = "cuda:0"
NQ = 16                                                        # 2^16 elements: 64 tiles of 2^10, 0.5 MiB in complex64
KINDS = {"c64": (np.complex64, torch.complex64), "c128": (np.complex128, torch.complex128)}
LAYOUTS = ["contiguous", "permuted"]


def store_perm(nd, layout):
    """perm[i]: the logical dim stored at position i of the contiguous storage.  "permuted": the top three dims rotated."""
    if layout == "contiguous" or nd < 3:
        return list(range(nd))
    return [2, 0, 1] + list(range(3, nd))


def strided_empty(shape, kind, layout, device=DEV):
    """An uninitialised tensor of logical shape `shape` in `layout` (also on the CPU: the host-only plan checks need its strides)."""
    perm = store_perm(len(shape), layout)
    store = torch.empty([shape[p] for p in perm], dtype=KINDS[kind][1], device=device)
    return store.permute([perm.index(d) for d in range(len(shape))])


def crand(seed, shape, kind):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(KINDS[kind][0])


def fill(t, host):
    """Copy a LOGICAL host array (or a Python float for a one-element tensor) into a static tensor, whatever its strides."""
    if isinstance(host, float):
        t.fill_(host)
    else:
        t.copy_(torch.from_numpy(np.ascontiguousarray(host)).to(t.device).reshape(t.shape))


def twin(t):
    """A second tensor with the strides and the contents of t."""
    out = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)
    out.copy_(t)
    return out


def bits(t):
    """The bytes of a tensor in logical order (bitwise comparison: -0.0 differs from 0.0, a NaN equals itself)."""
    t = t.reshape(-1)                                          # (first: view_as_real of 16 dims would have 17)
    t = torch.view_as_real(t) if t.is_complex() else t
    return t.contiguous().reshape(-1).view(torch.uint8)


def memory(t):
    """The elements of a dense tensor in MEMORY order, as numpy."""
    return torch.as_strided(t, (t.numel(),), (1,), t.storage_offset()).cpu().numpy()


def memory_of(host, strides):
    """The MEMORY-order array of a logical host array laid out with `strides` (in elements)."""
    mem = np.empty(host.size, dtype=host.dtype)
    np.lib.stride_tricks.as_strided(mem, shape=host.shape, strides=tuple(int(s) * mem.itemsize for s in strides))[...] = host
    return mem


def logical_of(mem, shape, strides):
    """The logical array of a MEMORY-order array."""
    return np.lib.stride_tricks.as_strided(mem, shape=tuple(shape), strides=tuple(int(s) * mem.itemsize for s in strides)).copy()


def _tuple(x):
    if x is None:
        return ()
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def capture_and_replay(op, statics, contents, verify, replays=3, between=None):
    """Warm `op` up eagerly on scratch copies, capture it once on `statics`, then for r in range(replays): copy contents(r) into
    the statics, replay, run the eager twin on clones on the default stream, require equal bits of every output and every
    static, and hand the host copies to verify(r, hosts, statics_after, outputs) for the comparison with the host reference.
    contents(-1) fills the statics for the warm-up and the capture.  between(r) runs after replay r (unrelated eager work)."""
    first = contents(-1)
    for s, h in zip(statics, first):
        fill(s, h)
    op(*[twin(s) for s in statics])                            # warm-up: lazy kernel attributes, the allocator
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _tuple(op(*statics))
    torch.cuda.synchronize()
    for r in range(replays):
        hosts = contents(r)
        for s, h in zip(statics, hosts):
            fill(s, h)
        twins = [twin(s) for s in statics]
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        eager = _tuple(op(*twins))
        torch.cuda.synchronize()
        assert len(eager) == len(outs)
        for k, (x, y) in enumerate(zip(outs, eager)):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)), f"replay {r}: output {k} differs from the eager run"
        for k, (x, y) in enumerate(zip(statics, twins)):
            assert torch.equal(bits(x), bits(y)), f"replay {r}: static tensor {k} differs from the eager run"
        verify(r, hosts, [np.ascontiguousarray(s.cpu().numpy()) for s in statics], [np.ascontiguousarray(o.cpu().numpy()) for o in outs])
        if between is not None:
            between(r)
            torch.cuda.synchronize()
    return graph, outs
