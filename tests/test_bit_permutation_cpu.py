"""Host-side checks of the in-place bit permutations (artensor_amd.layout), through the query and the packed table only: the
passes compose to the permutation, respect the tile's capacity and the bound on their number; dst_bit of a perm or an order is
what index arithmetic on strided views gives; the LDS maps are invertible and conflict-free under the bank model; a numpy walk of
the packed table -- the kernel's tile walk, column XORs and two LDS maps, element for element -- reproduces the oracle; every
refusal has its code and text."""
import ctypes

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd.pauli import _desc, _ptr

import bit_permutation_oracle as O

DTYPES = {torch.complex64: (4, 12), torch.complex128: (3, 11)}             # line bits LB, tile bits TB


def info_of(nb, dst, dtype=torch.complex64):
    return A.bit_permutation_info((2,) * nb, O.contiguous_strides((2,) * nb), dtype, dst_bit=dst)


def bound(h, moved):
    """The issue's bound on the passes: h moved bits at or above a line, `moved` moved bits in all."""
    return max(1, -(-(h - 1) // 7)) if moved else 0


def rank_gf2(vectors):
    vs, rank = list(vectors), 0
    for bit in range(16):
        at = next((i for i in range(rank, len(vs)) if (vs[i] >> bit) & 1), None)
        if at is None:
            continue
        vs[rank], vs[at] = vs[at], vs[rank]
        vs = [v ^ vs[rank] if i != rank and (v >> bit) & 1 else v for i, v in enumerate(vs)]
        rank += 1
    return rank


def xor_cols(cols, u):
    x = 0
    for j, c in enumerate(cols):
        if (u >> j) & 1:
            x ^= c
    return x


def degrees(p, dtype):
    """(load, store) conflict degree of a pass, recomputed from its columns under the bank model of include/artn.h."""
    tb = p["tb"]
    if dtype == torch.complex64:
        load, wl, store, ws = [2, 4, 8, 16], 4, [2, 4, 8, 16, 32], 5
    else:
        load, wl, store, ws = [1, 2, 4], 3, [1, 2, 4 | 8, 4 | 16], 4
    out = []
    for gens, w, cols in ((load, wl, p["load_col"]), (store, ws, p["store_col"])):
        gens = [g for g in gens if not g >> tb]
        out.append(1 << (len(gens) - rank_gf2([xor_cols(cols, g) & ((1 << w) - 1) for g in gens])))
    return tuple(out)


def check_plan(nb, dst, dtype):
    """The structural properties of one plan; returns the info."""
    lb, tb_max = DTYPES[dtype]
    info = info_of(nb, dst, dtype)
    h = sum(1 for b in range(nb) if dst[b] != b and b >= lb)
    assert info["n_bits"] == nb and info["moved_high"] == h and info["line_bits"] == lb
    assert info["moved"] == sum(1 for b in range(nb) if dst[b] != b)
    assert info["passes"] == len(info["pass_info"]) <= bound(h, info["moved"])
    if list(dst) == list(range(nb)):
        assert info["passes"] == 0
    elif h <= 8:
        assert info["passes"] == 1
    assert O.compose([p["map"] for p in info["pass_info"]], nb) == list(dst)
    elem = 8 if dtype == torch.complex64 else 16
    assert info["bytes_moved"] == 2 * elem * (1 << nb) * info["passes"]
    assert info["table_bytes"] == N.BITPERM_TABLE_HEADER_BYTES + N.BITPERM_PASS_BYTES * info["passes"]
    for p in info["pass_info"]:
        tb = min(tb_max, nb)
        moved = [b for b in range(nb) if p["map"][b] != b]
        assert p["moved_mask"] == sum(1 << b for b in moved) and moved
        assert sorted(p["map"][b] for b in moved) == moved                  # a permutation of its moved bits among themselves
        assert p["tb"] == tb == len(p["tile"]) and p["tile"] == sorted(p["tile"])
        assert set(moved) <= set(p["tile"]) and set(range(min(lb, nb))) <= set(p["tile"])
        if nb > tb_max:
            assert sum(1 for b in moved if b >= lb) <= tb_max - lb          # the capacity of a pass
        rest = [b for b in range(nb) if b not in moved and b >= lb]
        assert [b for b in p["tile"] if b not in moved and b >= lb] == rest[:tb - len(set(moved) | set(range(min(lb, nb))))]
        assert p["n_tiles"] == (1 << nb) >> tb and p["grid"] == min(p["n_tiles"], p["grid"]) >= 1
        # both LDS maps are invertible; the store columns are the load columns under the pass's tile-local map
        assert rank_gf2(p["load_col"]) == tb and rank_gf2(p["store_col"]) == tb
        assert all(c < 1 << tb for c in p["load_col"] + p["store_col"])
        pos = {b: j for j, b in enumerate(p["tile"])}
        for j, b in enumerate(p["tile"]):
            assert p["store_col"][pos[p["map"][b]]] == p["load_col"][j]
        assert (p["load_degree"], p["store_degree"]) == degrees(p, dtype)
        assert p["load_degree"] == 1
    return info


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_named_permutations_plan_and_lds_degrees(dtype):
    lb, _ = DTYPES[dtype]
    report = []
    for nb in (2, 5, 8, 12, 13, 16, 20, 21, 30, 34):
        for name, dst in O.named_permutations(nb, lb).items():
            info = check_plan(nb, dst, dtype)
            report.append((nb, name, info["passes"], info["store_degree"]))
            if name == "identity":
                assert info["passes"] == 0 and info["bytes_moved"] == 0
            if name == "cycle_8_high" or name.startswith("swap"):
                assert info["passes"] == 1
            if name == "cycle_9_high":
                assert info["passes"] == 2
            if dtype == torch.complex64:
                assert info["store_degree"] == 1, (nb, name)
    print("complex128 store degrees (nb, case, passes, degree):" if dtype == torch.complex128 else "complex64:", report)
    if dtype == torch.complex128:                                           # reported; the search reaches 1 here as well
        assert max(r[3] for r in report) <= 2


def test_the_20_bit_reversal_and_rotation_take_several_passes_within_the_bound():
    for name in ("reversal", "rotation"):
        info = check_plan(20, O.named_permutations(20, 4)[name], torch.complex64)
        assert info["moved_high"] == 16 and 2 <= info["passes"] <= 3


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_random_permutations_compose_and_respect_capacity_and_bound(dtype):
    rng = np.random.default_rng(24)
    worst = 1
    for k in range(160):
        nb = int(rng.integers(8, 35))
        dst = list(range(nb))
        if k % 3 == 0:                                                      # a few moved bits: short cycles that share a pass
            some = rng.choice(nb, size=min(nb, int(rng.integers(2, 12))), replace=False)
            for b, c in zip(sorted(some), some):
                dst[int(b)] = int(c)
        else:
            dst = [int(b) for b in rng.permutation(nb)]
        worst = max(worst, check_plan(nb, dst, dtype)["store_degree"])
    print(f"{dtype}: worst store degree over the random set {worst}")
    if dtype == torch.complex64:
        assert worst == 1


LAYOUTS = [                                                                 # (shape, the dims in memory, slowest first)
    ((2, 2, 2, 2, 2, 2), None),
    ((2, 4, 1, 8, 2, 4), (3, 0, 5, 1, 2, 4)),                                # extents 1, 4 and 8, permuted strides
    ((4, 2, 4, 2, 1, 2), (5, 3, 0, 1, 4, 2)),
    ((8, 8, 2, 1, 2), (1, 4, 2, 0, 3)),
]


def random_perm_within_extents(rng, shape):
    """A permutation of the dims that only trades dims of equal extent."""
    perm = list(range(len(shape)))
    for e in set(shape):
        same = [k for k in range(len(shape)) if shape[k] == e]
        for k, src in zip(same, rng.permutation(same)):
            perm[k] = int(src)
    return perm


@pytest.mark.parametrize("shape, memory_order", LAYOUTS)
def test_dst_bit_of_perm_and_order_agree_with_index_arithmetic(shape, memory_order):
    from artensor_amd import layout
    strides = O.contiguous_strides(shape, memory_order)
    rng = np.random.default_rng(len(shape) + shape[0])
    dims = len(shape)
    for _ in range(12):
        order = [int(k) for k in rng.permutation(dims)]
        dst, new_strides = layout.dst_bit_of_order(shape, strides, order)
        want, want_strides = O.dst_bit_of_order(shape, strides, order)
        assert dst == want
        assert all(s == w for s, w, e in zip(new_strides, want_strides, shape) if e != 1)
        info = A.bit_permutation_info(shape, strides, order=order)
        assert list(info["dst_bit"]) == want and info["strides"] == new_strides
    assert layout.dst_bit_of_order(shape, strides)[0] == O.dst_bit_of_order(shape, strides)[0]
    assert A.bit_permutation_info(shape, strides)["dst_bit"] == tuple(O.dst_bit_of_order(shape, strides)[0])   # default: contiguous
    for _ in range(12):
        perm = random_perm_within_extents(rng, shape)
        assert layout.dst_bit_of_perm(shape, strides, perm) == O.dst_bit_of_perm(shape, strides, perm)
        assert list(A.bit_permutation_info(shape, strides, perm=perm)["dst_bit"]) == O.dst_bit_of_perm(shape, strides, perm)
    if len(set(shape)) > 1:
        k = next(k for k in range(1, dims) if shape[k] != shape[0])
        bad = list(range(dims))
        bad[0], bad[k] = k, 0
        with pytest.raises(ValueError, match="cannot take the place"):
            layout.dst_bit_of_perm(shape, strides, bad)


# ---- the kernel's walk of the packed table, in numpy ----------------------------------------------------------------------------
def packed_table(nb, dst, dtype):
    d = _desc((2,) * nb, O.contiguous_strides((2,) * nb), dtype)
    dst_a = np.array(list(dst) or [0], dtype=np.int32)
    info = N.ArtnBitpermInfo()
    N.check(N.lib().artn_bitperm_query(ctypes.byref(d), _ptr(dst_a), nb, ctypes.byref(info), None, None, None, None))
    table = np.zeros(info.table_bytes // 8, dtype=np.uint64)
    N.check(N.lib().artn_bitperm_pack(ctypes.byref(d), _ptr(dst_a), nb, _ptr(table), info.table_bytes))
    return table, info


def walk_table(mem, table, chunk_elems):
    """What artn_k_bitperm does with the table, tile by tile: hole insertion, the XOR columns of memory offset and of the two LDS
    maps.  Also checks that the tiles of a pass are disjoint and cover the state and that every chunk is contiguous and aligned."""
    n = mem.shape[0]
    n_passes = int(table[0])
    for p in range(n_passes):
        rec = table[8 + 72 * p: 8 + 72 * (p + 1)]
        tb, n_tiles, seg_bits, n_holes = (int(x) for x in rec[:4])
        mem_col, load_col, store_col, holes = rec[8:24], rec[24:40], rec[40:56], rec[56:72]
        u = np.arange(1 << tb, dtype=np.uint64)
        off, lidx, sidx = (np.zeros(1 << tb, dtype=np.uint64) for _ in range(3))
        for j in range(tb):
            bit = ((u >> np.uint64(j)) & np.uint64(1)).astype(bool)
            off[bit] ^= mem_col[j]
            lidx[bit] ^= load_col[j]
            sidx[bit] ^= store_col[j]
        base = np.arange(n_tiles, dtype=np.uint64) << np.uint64(seg_bits)
        for j in range(n_holes):
            h = np.uint64(int(holes[j]))
            base = ((base >> h) << (h + np.uint64(1))) | (base & ((np.uint64(1) << h) - np.uint64(1)))
        addr = (base[:, None] | off[None, :]).astype(np.int64)
        assert np.array_equal(np.sort(addr.reshape(-1)), np.arange(n))      # disjoint tiles that cover the state, in bounds
        if (1 << tb) >= chunk_elems:
            first = addr[:, ::chunk_elems]
            assert not (first % chunk_elems).any()
            assert all(np.array_equal(addr[:, k::chunk_elems], first + k) for k in range(chunk_elems))
        lds = np.empty((n_tiles, 1 << tb) + mem.shape[1:], dtype=mem.dtype)
        lds[:, lidx.astype(np.int64)] = mem[addr]
        out = np.empty_like(mem)
        out[addr] = lds[:, sidx.astype(np.int64)]
        mem = out
    return mem


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_a_numpy_walk_of_the_packed_table_reproduces_the_oracle(dtype):
    lb, tb = DTYPES[dtype]
    rng = np.random.default_rng(7)
    for nb in (1, 2, 3, lb, lb + 1, tb - 1, tb, tb + 1, 16, 18):
        mem = rng.integers(0, 1 << 62, size=1 << nb, dtype=np.int64)
        cases = dict(O.named_permutations(nb, lb))
        for k in range(4):
            cases[f"random{k}"] = [int(b) for b in rng.permutation(nb)]
        for name, dst in cases.items():
            table, info = packed_table(nb, dst, dtype)
            assert int(table[0]) == info.passes and int(table[1]) == nb
            got = walk_table(mem, table, 2 if dtype == torch.complex64 else 1)
            assert np.array_equal(got, O.permute_bits(mem, dst)), (nb, name)
            i = int(rng.integers(0, 1 << nb))
            assert got[O.pi(i, dst)] == mem[i]


def test_busiest_dims_order_on_a_hand_made_list():
    m = np.eye(2)
    gates = [(m, (3,)), (np.eye(4), (3, 1)), (m, 1), (np.eye(4), (0, 3)), (m, (4,))]
    # counts: dim 0: 1, 1: 2, 2: 0, 3: 3, 4: 1, 5: 0 -> slowest first, ties by dim
    assert A.busiest_dims_order(gates, 6) == [2, 5, 0, 4, 1, 3]
    assert A.busiest_dims_order([], 3) == [0, 1, 2]
    with pytest.raises(ValueError, match="out of range"):
        A.busiest_dims_order([(m, (6,))], 6)


def query_rc(d, dst, n_bits):
    info = N.ArtnBitpermInfo()
    rc = N.lib().artn_bitperm_query(ctypes.byref(d), None if dst is None else _ptr(dst), n_bits, ctypes.byref(info), None, None, None, None)
    return rc, (N.lib().artn_last_error() or b"").decode()


def test_every_refusal_returns_its_code_and_text():
    lib = N.lib()
    d = _desc((2,) * 6, O.contiguous_strides((2,) * 6), torch.complex64)
    ok = np.array([1, 0, 2, 3, 4, 5], dtype=np.int32)
    assert query_rc(d, ok, 6)[0] == 0
    for dst, text in ((np.array([1, 1, 2, 3, 4, 5], dtype=np.int32), "dst_bit is not a permutation of 0 .. 5: entry 1 is 1"),
                      (np.array([0, 1, 2, 3, 4, 6], dtype=np.int32), "entry 5 is 6"),
                      (np.array([0, -1, 2, 3, 4, 5], dtype=np.int32), "entry 1 is -1")):
        rc, msg = query_rc(d, dst, 6)
        assert rc == -1 and text in msg, msg
    rc, msg = query_rc(d, ok, 5)
    assert rc == -1 and "6 index bits, not 5" in msg
    rc, msg = query_rc(d, None, 6)
    assert rc == -1 and msg == "null pointer"
    assert lib.artn_bitperm_query(ctypes.byref(d), _ptr(ok), 6, None, None, None, None, None) == -1
    assert lib.artn_last_error().decode() == "null info"
    rc, msg = query_rc(_desc((2, 3, 2), (6, 2, 1), torch.complex64), ok, 3)
    assert rc == -2 and msg == "bit permutations take power-of-two extents"
    big = _desc((1 << 20, 1 << 20, 2), (1 << 21, 2, 1), torch.complex64)
    rc, msg = query_rc(big, ok, 41)
    assert rc == -2 and msg == "bit permutations take at most 2^40 elements"
    rc, msg = query_rc(_desc((2, 2), (4, 1), torch.complex64), ok, 2)
    assert rc == -1 and "not dense" in msg
    bad_dtype = _desc((2,) * 6, O.contiguous_strides((2,) * 6), torch.complex64)
    bad_dtype.dtype = 7
    rc, msg = query_rc(bad_dtype, ok, 6)
    assert rc == -2 and msg == "bit permutations take complex64 or complex128"
    # pack: a table that is too small, a misaligned table
    table = np.zeros(N.BITPERM_TABLE_HEADER_BYTES // 8 + N.BITPERM_PASS_BYTES // 8 + 1, dtype=np.uint64)
    need = N.BITPERM_TABLE_HEADER_BYTES + N.BITPERM_PASS_BYTES
    assert lib.artn_bitperm_pack(ctypes.byref(d), _ptr(ok), 6, _ptr(table), need) == 0
    assert lib.artn_bitperm_pack(ctypes.byref(d), _ptr(ok), 6, _ptr(table), need - 8) == -1
    assert lib.artn_last_error().decode() == "table smaller than artn_bitperm_query reports"
    assert lib.artn_bitperm_pack(ctypes.byref(d), _ptr(ok), 6, ctypes.c_void_p(table.ctypes.data + 4), need) == -2
    assert lib.artn_last_error().decode() == "artn_bitperm_pack needs an 8-byte aligned table"
    assert lib.artn_bitperm_pack(ctypes.byref(d), _ptr(ok), 6, None, need) == -1
    # the Python layer's own refusals
    with pytest.raises(ValueError, match="one of dst_bit, perm and order"):
        A.bit_permutation_info((2, 2), (2, 1), perm=(1, 0), order=(1, 0))
    with pytest.raises(ValueError, match="permutation of range"):
        A.bit_permutation_info((2, 2), (2, 1), perm=(1, 1))
    with pytest.raises(ValueError, match="power-of-two extents"):
        A.bit_permutation_info((3, 2), (2, 1), order=(1, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.permute_dims_(torch.zeros(2, 2, dtype=torch.complex64), (1, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.relayout_(torch.zeros(2, 2, dtype=torch.complex64))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the CPU-only refusal")
def test_apply_refuses_without_a_device():
    d = _desc((2,) * 6, O.contiguous_strides((2,) * 6), torch.complex64)
    ok = np.array([1, 0, 2, 3, 4, 5], dtype=np.int32)
    table = np.zeros(80, dtype=np.uint64)
    rc = N.lib().artn_bitperm_apply(ctypes.byref(d), _ptr(table), _ptr(ok), 6, _ptr(table), 640, None)
    assert rc == -4 and "no gfx950 device" in N.lib().artn_last_error().decode()
