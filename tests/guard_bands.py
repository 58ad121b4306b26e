"""The harness of tests/test_guard_bands_gpu.py: operands of a state operation inside sentinel bands of ONE allocation, at a
storage offset, so that an access outside an operand is seen instead of landing in the allocator's slack.

banded() lays out   [band][offset gap][state 0][band][state 1] ... [state m-1][band]   in one flat buffer.  Every band and gap
element holds a quiet NaN with a recognisable payload in both components (SENTINEL: one fixed 32- or 64-bit pattern), and is
compared as integers afterwards, as graph_replay.bits does:
  * a STORE into a band or the gap changes the pattern: assert_bands_intact names the element by its distance from the nearest
    state edge (neighbouring states are one band apart, so cross-talk between operands is seen as well);
  * a LOAD from a band that enters arithmetic makes the result NaN, and the family's own reference rejects it.
Three blind spots, none of them claimed.  A load whose value is discarded (a prefetch past the end that is masked out, a lane
that reads and then does not store).  A store that writes the sentinel's own bits back: with one fixed pattern in every band
element, a kernel that moves band elements among themselves (an X or a permutation on a whole tile past the end), or whose
arithmetic on sentinels hands the payload through, leaves the band equal to itself; such a kernel is seen only where the same
stray tile also reaches an operand, or misses one it should have written.  And an access further than one band from every
operand.

Works on numpy arrays ("numpy"), CPU tensors ("cpu") and the GPU; tests/test_guard_bands_cpu.py runs numpy stand-ins through it,
clean and with planted errors."""
import numpy as np
import torch

MIN_BAND = 4096                                                # elements per side: the margin of the matrix-gate test
SENTINEL = {4: np.uint32(0x7FC5A5A5), 8: np.uint64(0x7FF8A5A5A5A5A5A5)}    # per real component: quiet NaN + payload
OFFSET_BYTES = (0, 16, 80)                                     # 80: 16-byte aligned, not 32-, 64- or 128-byte aligned
_TORCH = {np.dtype(np.complex64): torch.complex64, np.dtype(np.complex128): torch.complex128, np.dtype(np.float64): torch.float64,
          np.dtype(np.float32): torch.float32, np.dtype(np.int64): torch.int64}


def offsets_of(dtype):
    """The three storage offsets in ELEMENTS of a numpy dtype: 0, 16 bytes, 80 bytes."""
    size = np.dtype(dtype).itemsize
    assert all(b % size == 0 for b in OFFSET_BYTES)
    return [b // size for b in OFFSET_BYTES]


def band_for(*units):
    """The band width for cases whose plans move at most `units` elements at once: never below MIN_BAND, a multiple of it."""
    return -(-max((MIN_BAND,) + tuple(int(u) for u in units)) // MIN_BAND) * MIN_BAND


def _words(dtype):
    """(unsigned integer dtype of one real component, components per element)."""
    dtype = np.dtype(dtype)
    comp = dtype.itemsize // 2 if dtype.kind == "c" else dtype.itemsize
    return {4: np.uint32, 8: np.uint64}[comp], dtype.itemsize // comp


def _extent(shape, strides):
    """Elements a dense view spans in memory (its element count; refused unless the strides are a dense layout)."""
    n = int(np.prod(shape, dtype=np.int64)) if len(shape) else 1
    span = 1 + sum((int(e) - 1) * int(s) for e, s in zip(shape, strides))
    assert span == n and all(int(s) > 0 for s in strides), f"not a dense layout: shape {tuple(shape)} strides {tuple(strides)}"
    return n


def banded(mems, shape, strides, dtype, offset=0, band=MIN_BAND, device="cpu"):
    """(store, views, layout).  mems: MEMORY-order host arrays, one per state; shape / strides: one layout for all of them, or a
    list with one (shape, strides) pair per state when `shape` is a list of tuples.  dtype: a numpy dtype.  device: "numpy",
    "cpu" or a GPU.  layout = {"band", "offset", "starts", "sizes", "total", "dtype"} is what assert_bands_intact and
    states_of take."""
    dtype = np.dtype(dtype)
    per_state = len(shape) > 0 and isinstance(shape[0], (tuple, list, torch.Size))
    shapes = [tuple(s) for s in shape] if per_state else [tuple(shape)] * len(mems)
    strides_ = [tuple(s) for s in strides] if per_state else [tuple(strides)] * len(mems)
    assert len(mems) == len(shapes) == len(strides_) >= 1 and band >= 1 and offset >= 0
    sizes = [_extent(sh, st) for sh, st in zip(shapes, strides_)]
    starts, at = [], band + offset
    line = 128 // dtype.itemsize                               # every state starts at the same phase of a 128-byte line
    assert band % line == 0, f"a band of {band} elements is no multiple of a 128-byte line"
    for n in sizes:
        starts.append(at)
        at += n + band + (-n) % line                           # (one band between neighbours, widened to the next line)
    total = at
    word, per = _words(dtype)
    raw = np.full(total * per, SENTINEL[np.dtype(word).itemsize], dtype=word)
    for mem, start, n in zip(mems, starts, sizes):
        mem = np.ascontiguousarray(mem).reshape(-1)
        assert mem.size == n and mem.dtype == dtype, (mem.size, n, mem.dtype, dtype)
        raw[start * per:(start + n) * per] = mem.view(word)     # (as integers: raw bit patterns survive)
    layout = {"band": band, "offset": offset, "starts": starts, "sizes": sizes, "total": total, "dtype": dtype}
    host = raw.view(dtype)
    if device == "numpy":
        views = [np.lib.stride_tricks.as_strided(host[s:], shape=sh, strides=tuple(int(x) * dtype.itemsize for x in st))
                 for s, sh, st in zip(starts, shapes, strides_)]
        return host, views, layout
    store = torch.from_numpy(host).to(device)
    assert store.dtype == _TORCH[dtype]
    return store, [torch.as_strided(store, sh, st, s) for s, sh, st in zip(starts, shapes, strides_)], layout


def _raw(store, layout):
    host = store if isinstance(store, np.ndarray) else store.detach().cpu().numpy()
    word, per = _words(layout["dtype"])
    assert host.size == layout["total"] and host.dtype == layout["dtype"]
    return np.ascontiguousarray(host).view(word), per


def assert_bands_intact(store, layout, label=""):
    """Every band and the offset gap hold the sentinel bit for bit; else the first differing element, by its distance from the
    nearest state edge."""
    raw, per = _raw(store, layout)
    inside = np.zeros(layout["total"], dtype=bool)
    for s, n in zip(layout["starts"], layout["sizes"]):
        inside[s:s + n] = True
    bad = (raw != SENTINEL[raw.dtype.itemsize]).reshape(-1, per).any(axis=1) & ~inside
    if not bad.any():
        return
    e = int(np.flatnonzero(bad)[0])
    edges = [(abs(e - s) if e < s else e - (s + n) + 1, f"{'in front of' if e < s else 'behind'} state {j}")
             for j, (s, n) in enumerate(zip(layout["starts"], layout["sizes"]))]
    dist, where = min(edges)
    raise AssertionError(f"{label}: {int(bad.sum())} guard elements changed; the first is store element {e}, {dist} element(s) {where} "
                         f"(band {layout['band']}, offset {layout['offset']}, states at {layout['starts']} of sizes {layout['sizes']})")


def states_of(store, layout):
    """The states' memory as host arrays, in MEMORY order (copies)."""
    host = store if isinstance(store, np.ndarray) else store.detach().cpu().numpy()
    return [host[s:s + n].copy() for s, n in zip(layout["starts"], layout["sizes"])]


def same_bits(x, y):
    """Two host arrays of one dtype hold the same bytes (a NaN equals itself, -0.0 differs from 0.0)."""
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8))
