"""The references of the matrix-core gates (artensor_amd/matrix_gates.py; artn_mgate_*), shared by test_matrix_gates_cpu.py,
test_matrix_gates_gpu.py and test_matrix_gates_large_gpu.py.  No GPU.

oracle      numpy complex128: tensordot on the (permuted) logical view.
bound       the a-priori error bound of include/artn.h per real component, from the oracle and the cover
            sum_c (|Re u| + |Im u|)(|Re x| + |Im x|).
emulate     the packed table followed index by index as the kernel follows it -- tile bases, memory offsets and LDS indices from
            the column tables, the coefficients from the FRAGMENT ORDER through the lane formula of one instruction, the steps in
            the contract's order, one rounding -- so the result comes from the table bytes and the memory alone.
"""
import numpy as np

HEADER_WORDS = 68                                              # ArtnMgateTable: 544 bytes
MAX_K = 7


def oracle(x, m, dims):
    """U on the dims `dims` of the logical array x (the first listed dim the most significant digit), in complex128."""
    k = len(dims)
    u = np.asarray(m, dtype=np.complex128).reshape((2,) * (2 * k))
    y = np.tensordot(u, np.asarray(x, dtype=np.complex128), axes=(list(range(k, 2 * k)), list(dims)))
    return np.moveaxis(y, list(range(k)), list(dims))


def cover(x, m, dims):
    """sum_c (|Re u| + |Im u|)(|Re x| + |Im x|) per output element: it bounds the sum of the magnitudes of the products of either
    component."""
    m = np.asarray(m, dtype=np.complex128)
    x = np.asarray(x, dtype=np.complex128)
    return oracle(np.abs(x.real) + np.abs(x.imag), np.abs(m.real) + np.abs(m.imag), dims).real


def bound(exact, cov, k, single):
    """Per real component (the last axis: Re, Im): 2^-24 |exact| for complex64 (the one rounding) + 4 * 2^k * 2^-53 * cover (a
    float64 sum of 2^(k+1) products in any order, factor 2 of slack)."""
    parts = np.stack([np.abs(exact.real), np.abs(exact.imag)], axis=-1)
    return (2.0 ** -24 * parts if single else 0.0) + (4 * 2 ** k * 2.0 ** -53 * cov)[..., None]


def components(z):
    return np.stack([z.real, z.imag], axis=-1)


def fields(table):
    """(head, arrays, U) of a packed table (uint8): the header of ArtnMgateTable and U rebuilt from the fragment order."""
    w = table[:8 * HEADER_WORDS].view(np.uint64)
    names = ["k", "tile_bits", "n_tiles", "segment", "flags", "group_bits", "n_high", "reserved"]
    head = {n: int(v) for n, v in zip(names, w[:8])}
    arrays = {"target_bit": w[8:15], "target_pos": w[15:22], "high_bit": w[22:29], "swizzle": w[29:36], "mem_col": w[36:52],
              "lds_col": w[52:68]}
    arrays = {n: v.astype(np.int64) for n, v in arrays.items()}
    k = head["k"]
    frag = table[8 * HEADER_WORDS:].view(np.float64)
    assert frag.size == 2 * 4 ** k
    f = frag.reshape(2 ** k // 8, 2 ** k // 2, 8, 2, 2)      # [rb][s][n][h][c] = U[8 rb + n][2 s + h], c = Re, Im
    u = (f[..., 0] + 1j * f[..., 1]).transpose(0, 2, 1, 3).reshape(2 ** k, 2 ** k)
    return head, arrays, u


def xor_cols(index, cols):
    out = np.zeros_like(index)
    for b, col in enumerate(cols):
        out ^= ((index >> b) & 1) * int(col)
    return out


def insert_holes(q, holes):
    for p in holes:
        p = int(p)
        q = ((q >> p) << (p + 1)) | (q & ((1 << p) - 1))
    return q


def lane_operand(frag, rb, s, steps):
    """The A operand [16 rows i][4 contracted kk] of the instruction (rb, s), read through the lane formula of include/artn.h:
    lane (j, q) takes entry (j >> 1) * 4 + (q >> 1) * 2 + ((j ^ q) & 1) of the 32 doubles of (rb, s), negated for j even, q odd."""
    j, q = np.meshgrid(np.arange(16), np.arange(4), indexing="ij")
    v = frag[(rb * steps + s) * 32 + (j >> 1) * 4 + (q >> 1) * 2 + ((j ^ q) & 1)]
    return np.where((j & 1 == 0) & (q & 1 == 1), -v, v)


def emulate(table, mem, dtype):
    """(out, trace): the memory-order array after the gate, from the packed table (uint8) and the memory-order input alone.
    trace: 'address' [n_tiles, 2^tb] every memory index loaded (and stored), 'lds' [2^tb] the LDS index of every tile-local
    index, 'row_group' [2^k, G] the LDS index of (row, group)."""
    head, arr, _ = fields(table)
    k, tb, n_tiles, gb, n_high = head["k"], head["tile_bits"], head["n_tiles"], head["group_bits"], head["n_high"]
    assert gb == tb - k and head["segment"] == 1 << (tb - n_high)
    frag = table[8 * HEADER_WORDS:].view(np.float64)
    rows, steps, groups = 2 ** k, 2 ** k // 2, 2 ** gb
    seg_bits = tb - n_high
    # phases 1 and 4
    base = insert_holes(np.arange(n_tiles, dtype=np.int64) << seg_bits, arr["high_bit"][:n_high])
    u = np.arange(2 ** tb, dtype=np.int64)
    memoff, lds = xor_cols(u, arr["mem_col"]), xor_cols(u, arr["lds_col"])
    address = base[:, None] | memoff[None, :]
    image = np.empty((n_tiles, 2 ** tb), dtype=np.complex128)
    image[:, lds] = mem[address]
    # phases 2 and 3: (row c, group g) at ((c << gb) | g) ^ sw(c)
    c, g = np.meshgrid(np.arange(rows), np.arange(groups), indexing="ij")
    where = ((c << gb) | g) ^ xor_cols(c, arr["swizzle"][:k])
    x = image[:, where]                                        # [tile, row, group]
    acc = np.zeros((n_tiles, rows, 2, groups))                 # [tile, output row, Re / Im, group]: the D operands
    for rb in range(rows // 8):
        for s in range(steps):
            a_op = lane_operand(frag, rb, s, steps)            # [16, 4]
            for kk in range(4):                                # the four products of a step, in order
                xin = x[:, 2 * s + (kk >> 1), :]
                b_row = xin.imag if kk & 1 else xin.real       # [tile, group]
                acc[:, 8 * rb:8 * rb + 8] += a_op[:, kk].reshape(1, 8, 2, 1) * b_row[:, None, None, :]
    part = np.float32 if dtype == np.complex64 else np.float64
    y = acc[:, :, 0].astype(part).astype(np.float64) + 1j * acc[:, :, 1].astype(part).astype(np.float64)
    out_image = np.empty_like(image)
    out_image[:, where] = y
    out = np.array(mem, dtype=np.complex128)
    out[address] = out_image[:, lds]
    return out.astype(dtype), {"address": address, "lds": lds, "row_group": where}
