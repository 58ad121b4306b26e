"""Without controls, a controlled gate's packed table carries the wide gate's columns, swizzle, block mask and tile walk, field for
field: one packer fills both (artn_state_host.h).  test_channel_cpu.py asserts the same of the channel's table.  No GPU."""
import numpy as np
import pytest
import torch

from test_controlled_gates_cpu import pack as controlled_pack
from test_gates_cpu import random_unitary
from test_pauli_apply_cpu import contiguous_strides
from test_wide_gates_cpu import pack as wide_pack
from tile_table import cgate_fields, wgate_fields

TB = {torch.complex64: 12, torch.complex128: 11}


def target_sets(n_bits, k, tb):
    """Memory bits: the lowest, a set that straddles the contiguous segment of the tile, the highest -- listed out of order."""
    low = list(range(k))
    edge = min(tb, n_bits) - 1                                              # the last bit a tile of low targets would hold
    straddle = [edge] if k == 1 else sorted({0, n_bits - 1} | set(range(max(0, edge + 1 - k), n_bits)))[:k]
    top = list(range(n_bits - k, n_bits))
    return [s[1:] + s[:1] for s in (low, straddle, top) if len(set(s)) == k]


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_a_controlled_gate_without_controls_packs_the_wide_gates_table(dtype):
    rng = np.random.default_rng(29)
    cases = 0
    for n_bits in (3, TB[dtype], 14):
        shape = (2,) * n_bits
        strides = contiguous_strides(shape)                                 # dim d is memory bit n_bits - 1 - d
        for k in (1, 3, 5):
            if k > n_bits:
                continue
            m = random_unitary(rng, 2 ** k)
            if k == 5:
                m = np.kron(np.diag([1, 1j]), m[:16, :16])                   # a block mask that is not full
            for bits in target_sets(n_bits, k, TB[dtype]):
                dims = [n_bits - 1 - b for b in bits]
                wt, winfo = wide_pack(shape, strides, m, dims, dtype)
                ct, cinfo = controlled_pack(shape, strides, m, dims, (), None, dtype)
                whead, warr = wgate_fields(wt)
                chead, carr = cgate_fields(ct)
                for name in ("mem_col", "lds_col", "swizzle", "target_bit", "target_pos"):
                    assert np.array_equal(warr[name], carr[name]), (n_bits, k, bits, name)
                assert tuple(carr["target_bit"][:k]) == tuple(bits)
                for name in ("block_mask", "tile_bits", "n_tiles", "segment"):
                    assert whead[name] == chead[name], (n_bits, k, bits, name)
                assert (winfo.tile_bits, winfo.n_tiles, winfo.segment) == (cinfo.tile_bits, cinfo.n_tiles, cinfo.segment)
                assert chead["n_holes"] == whead["n_high"] and 1 << chead["segment_bits"] == chead["segment"]
                assert np.array_equal(carr["hole_bit"][:chead["n_holes"]], warr["high_bit"][:whead["n_high"]])
                assert chead["group_mask"] == chead["group_want"] == chead["high_mask"] == chead["high_want"] == 0
                assert chead["n_tiles"] == (1 if n_bits <= TB[dtype] else 2 ** (n_bits - TB[dtype]))
                cases += 1
    assert cases == 24                                                     # 2 widths fit 2^3, 3 the others; 3 target sets each
