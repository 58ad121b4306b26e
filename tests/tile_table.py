"""The packed column tables of the tile kernels (wide gates, controlled gates, channels), followed in numpy as the kernel follows
them.  Shared by test_wide_gates_cpu.py, test_controlled_gates_cpu.py and test_tile_tables_cpu.py; no GPU."""
import numpy as np


def xor_cols(index, cols):
    out = np.zeros_like(index)
    for b, col in enumerate(cols):
        out ^= ((index >> b) & 1) * int(col)
    return out


def insert_holes(q, holes):
    """q with a 0 inserted at every bit of `holes`, ascending: the first element of a tile, before high_want."""
    for p in holes:
        p = int(p)
        q = ((q >> p) << (p + 1)) | (q & ((1 << p) - 1))
    return q


def follow_columns(tb, k, seg_bits, want, target_bit, target_pos, swizzle, mem_col, lds_col):
    """Every index the kernel forms from the columns: phases 1 and 4 (tile-local index -> memory offset and LDS index) and phases 2
    and 3 ((row, group) -> LDS index).  `want`: the targets' memory bits in the order listed.  Returns (mem, off, rest): the memory
    offset of every tile-local index, of every [row, group], and the latter without the target bits."""
    gb = tb - k
    assert tuple(target_bit[:k]) == tuple(want) and all(mem_col[target_pos[j]] == 1 << want[j] for j in range(k))
    assert not mem_col[tb:].any() and not lds_col[tb:].any() and not swizzle[k:].any() and all(int(s) < 2 ** gb for s in swizzle)
    u = np.arange(2 ** tb, dtype=np.int64)
    mem, lds = xor_cols(u, mem_col), xor_cols(u, lds_col)
    assert np.array_equal(mem[:2 ** seg_bits], u[:2 ** seg_bits])       # a segment is contiguous, and the first one starts the tile
    assert np.array_equal(np.sort(lds), u)                              # the image is a bijection: nothing outside 2^tb
    # the low window: 64 consecutive tile-local indices take 64 different values of the low six LDS index bits (the banks)
    w = min(6, gb)
    for start in range(0, 2 ** tb, max(2 ** w, 2 ** tb // 8)):
        assert np.array_equal(np.sort(lds[start:start + 2 ** w] & (2 ** w - 1)), u[:2 ** w])
    # (row c, group g) -> LDS index, as phases 2 and 3 form it; row bit i is the i-th target from the LAST listed one
    c, g = np.meshgrid(np.arange(2 ** k), np.arange(2 ** gb), indexing="ij")
    idx = ((c << gb) | g) ^ xor_cols(c, swizzle[:k])
    assert np.array_equal(np.sort(idx.reshape(-1)), u)
    where = np.empty(2 ** tb, dtype=np.int64)
    where[lds] = mem                                                   # LDS index -> memory offset inside the tile
    off = where[idx]                                                   # [row, group]
    row_of = sum(((off >> want[k - 1 - i]) & 1) << i for i in range(k))
    assert np.array_equal(row_of, c)
    rest = off & ~sum(1 << b for b in want)
    assert (rest == rest[0:1]).all() and len(set(rest[0])) == 2 ** gb   # a group differs in the target bits only
    assert np.array_equal(np.argsort(rest[0]), np.arange(2 ** gb))     # consecutive groups: ascending memory order
    return mem, off, rest


def wgate_fields(table):
    """The arrays of an ArtnWgateTable (the first 480 bytes of a wide gate's or a channel's table)."""
    w = table.view(np.uint64)
    names = ["k", "tile_bits", "n_tiles", "segment", "flags", "group_bits", "n_high", "block_mask"]
    head = {k: int(v) for k, v in zip(names, w[:8])}
    arrays = {"target_bit": w[8:13], "target_pos": w[13:18], "high_bit": w[18:23], "swizzle": w[23:28], "mem_col": w[28:44],
              "lds_col": w[44:60]}
    return head, {k: v.astype(np.int64) for k, v in arrays.items()}


def cgate_fields(table):
    """The arrays of an ArtnCgateTable (1000 bytes)."""
    w = table.view(np.uint64)
    names = ["t", "tile_bits", "n_tiles", "segment", "flags", "group_bits", "segment_bits", "block_mask", "n_holes", "high_want",
             "high_mask", "group_mask", "group_want"]
    head = {k: int(v) for k, v in zip(names, w[:13])}
    arrays = {"target_bit": w[13:18], "target_pos": w[18:23], "swizzle": w[23:28], "mem_col": w[28:44], "lds_col": w[44:60],
              "hole_bit": w[60:124]}
    assert int(w[124]) == 0
    return head, {k: v.astype(np.int64) for k, v in arrays.items()}
