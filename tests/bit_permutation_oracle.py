"""The numpy restatement of artensor_amd.layout: a bit permutation is a transpose of the (2,) * nb memory cube.

dst_bit[b] is where memory bit b of an element's index goes: new[pi(i)] == old[i] with bit dst_bit[b] of pi(i) == bit b of i.
Nothing here shares code with the package: dst_bit of a `perm` or an `order` is derived from index arithmetic on strided views.
"""
import numpy as np


def permute_bits(mem, dst_bit):
    """new memory of old memory `mem` ([2^nb] or [2^nb, ...]: trailing axes ride along) under dst_bit."""
    nb = len(dst_bit)
    assert mem.shape[0] == 1 << nb and sorted(dst_bit) == list(range(nb))
    tail = mem.shape[1:]
    inv = [0] * nb
    for b, c in enumerate(dst_bit):
        inv[c] = b
    # cube axis j is memory bit nb - 1 - j; the new cube's axis for bit c is the old cube's axis for bit inv[c]
    axes = [nb - 1 - inv[nb - 1 - j] for j in range(nb)] + [nb + t for t in range(len(tail))]
    return np.ascontiguousarray(mem.reshape((2,) * nb + tail).transpose(axes)).reshape(mem.shape)


def pi(i, dst_bit):
    return sum(((i >> b) & 1) << c for b, c in enumerate(dst_bit))


def compose(maps, nb):
    """The dst_bit of the passes `maps` (each a per-bit map) applied in order."""
    dst = list(range(nb))
    for m in maps:
        dst = [m[c] for c in dst]
    return dst


def inverse(dst_bit):
    inv = [0] * len(dst_bit)
    for b, c in enumerate(dst_bit):
        inv[c] = b
    return inv


def view(mem, shape, strides):
    """The logical tensor of flat memory `mem` under (shape, strides in elements)."""
    return np.lib.stride_tricks.as_strided(mem, shape=tuple(shape), strides=tuple(int(s) * mem.itemsize for s in strides))


def contiguous_strides(shape, order=None):
    """Element strides with the dims in memory in `order`, slowest first."""
    order = list(range(len(shape))) if order is None else list(order)
    strides, s = [0] * len(shape), 1
    for k in reversed(order):
        strides[k] = s
        s *= int(shape[k])
    return tuple(strides)


def dst_bit_by_index(n, old_of_new_mem):
    """dst_bit from the memory-level map: old_of_new_mem[j] is the old memory index whose element ends at new memory index j."""
    nb = n.bit_length() - 1
    new_of_old = np.empty(n, dtype=np.int64)
    new_of_old[old_of_new_mem] = np.arange(n, dtype=np.int64)
    dst = [int(new_of_old[1 << b]).bit_length() - 1 for b in range(nb)]
    assert all(int(new_of_old[1 << b]) == 1 << dst[b] for b in range(nb))
    assert all(int(new_of_old[i]) == pi(i, dst) for i in range(0, n, max(1, n // 257)))
    return dst


def dst_bit_of_perm(shape, strides, perm):
    """dst_bit such that the same (shape, strides) view afterwards equals (old view).permute(perm)."""
    n = int(np.prod([int(e) for e in shape], dtype=np.int64))
    new = np.empty(n, dtype=np.int64)
    view(new, shape, strides)[...] = view(np.arange(n, dtype=np.int64), shape, strides).transpose(perm)
    return dst_bit_by_index(n, new)


def dst_bit_of_order(shape, strides, order=None):
    """(dst_bit, new strides) such that the view with the new strides afterwards equals the old view."""
    n = int(np.prod([int(e) for e in shape], dtype=np.int64))
    new_strides = contiguous_strides(shape, order)
    new = np.empty(n, dtype=np.int64)
    view(new, shape, new_strides)[...] = view(np.arange(n, dtype=np.int64), shape, strides)
    return dst_bit_by_index(n, new), new_strides


def transposition(nb, x, y):
    dst = list(range(nb))
    dst[x], dst[y] = y, x
    return dst


def cycle(nb, bits):
    dst = list(range(nb))
    for i, b in enumerate(bits):
        dst[b] = bits[(i + 1) % len(bits)]
    return dst


def named_permutations(nb, lb):
    """name -> dst_bit of the named cases that exist at nb bits (lb: the index bits of a 128-byte line)."""
    out = {"identity": list(range(nb)), "reversal": [nb - 1 - b for b in range(nb)], "rotation": [(b + 1) % nb for b in range(nb)]}
    if lb >= 2 and nb >= 2:
        out["swap_low_low"] = transposition(nb, 0, min(lb, nb) - 1)
    if nb > lb:
        out["swap_low_high"] = transposition(nb, 1, nb - 1)
    if nb > lb + 1:
        out["swap_high_high"] = transposition(nb, lb, nb - 1)
        out["swap_high_adjacent"] = transposition(nb, nb - 2, nb - 1)
    if nb >= lb + 8:
        out["cycle_8_high"] = cycle(nb, list(range(nb - 8, nb)))
    if nb >= lb + 9:
        out["cycle_9_high"] = cycle(nb, list(range(nb - 9, nb)))
    return out
