"""Host-side checks of the wide gates (artensor_amd/wide_gates.py: wide_gate_info, WideGate, FusedCircuit, fuse_gates;
artn_wgate_query / _pack / _apply): the symbols, the refusals with their error codes, the properties of the tile plan on random
permuted layouts, the packed table followed index by index the way the kernel follows it (every address inside the state, every
element visited once, the LDS image a bijection, groups and rows where the convention puts them), and fuse_gates against dense
unitaries and the n12 fixture.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import wide_gates as WG
from artensor_amd.fixtures import load_case
from test_gates_cpu import dense_unitary, n12_gates, numpy_gate, random_unitary
from test_gpu_parity import amp_rel
from test_pauli_apply_cpu import contiguous_strides, desc, ptr
from tile_table import follow_columns, insert_holes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INVALID, UNSUPPORTED, NODEVICE = -1, -2, -4
TB = {torch.complex64: 12, torch.complex128: 11}


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_wgate_query", "artn_wgate_pack", "artn_wgate_apply"]
    assert N.ABI_VERSION == 9 and N.lib().artn_abi_version() == 9
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    assert "#define ARTN_ABI_VERSION 9" in text and "#define ARTN_WGATE_MAX_K 5" in text
    assert "#define ARTN_WGATE_TILE_BITS_C64 12" in text and "#define ARTN_WGATE_TILE_BITS_C128 11" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert ctypes.sizeof(N.ArtnWgateInfo) == 4 * 4 + 6 * 8
    assert N.WGATE_MAX_K == 5 and N.WGATE_TABLE_HEADER_BYTES == 480
    for name in ("apply_wide_gate_", "WideGate", "wide_gate_info", "FusedCircuit", "apply_circuit_", "fuse_gates"):
        assert getattr(A, name) is getattr(WG, name)


def query_rc(shape, strides, dims, mat=None, dtype=N.ARTN_C64, k=None, info=True, null_mat=False):
    k = len(dims) if k is None else k
    dims = np.asarray(list(dims) + [0] * 8, dtype=np.int32)
    if mat is None:
        mat = np.zeros(2 * 4 ** max(min(k, 5), 1))
        mat[0] = 1
    out = N.ArtnWgateInfo()
    return N.lib().artn_wgate_query(ctypes.byref(desc(shape, strides, dtype)), k, ptr(dims), None if null_mat else ptr(mat),
                                    ctypes.byref(out) if info else None, None, None)


def last_error():
    return N.lib().artn_last_error()


def test_the_refusals_and_their_error_codes():
    shape, strides = (2, 2, 4, 2, 2, 2), (1, 2, 4, 16, 32, 64)
    assert query_rc(shape, strides, [0, 1, 3]) == 0
    assert query_rc(shape, strides, [5, 0, 4, 1, 3]) == 0
    assert query_rc(shape, strides, [0]) == 0 and query_rc(shape, strides, [4, 1]) == 0
    assert query_rc(shape, strides, [0, 1, 3, 4, 5, 0], k=6) == UNSUPPORTED and b"one to five" in last_error()
    assert query_rc(shape, strides, [], k=0) == UNSUPPORTED and b"one to five" in last_error()
    assert query_rc((2, 2), (1, 2), [0, 1, 0], k=3) == INVALID and b"at least 2^3" in last_error()
    assert query_rc(shape, strides, [0, 1, 1]) == INVALID and b"differ" in last_error()
    assert query_rc(shape, strides, [0, 6, 1]) == INVALID and b"out of range" in last_error()
    assert query_rc(shape, strides, [0, -1, 1]) == INVALID and b"out of range" in last_error()
    assert query_rc(shape, strides, [0, 2, 1]) == INVALID and b"extent 4" in last_error()
    for bad in (np.nan, np.inf, -np.inf):
        mat = np.zeros(2 * 64)
        mat[77] = bad
        assert query_rc(shape, strides, [0, 1, 3], mat) == INVALID and b"finite" in last_error()
    assert query_rc(shape, strides, [0, 1, 3], info=False) == INVALID and b"null" in last_error()
    assert query_rc(shape, strides, [0, 1, 3], null_mat=True) == INVALID and b"null" in last_error()
    # the layout and dtype refusals of artn_gates_query
    assert query_rc(shape, strides, [0, 1, 3], dtype=N.ARTN_C64_BF16) == UNSUPPORTED and b"complex64 or complex128" in last_error()
    assert query_rc(shape, (1, 2, 4, 16, 32, 128), [0, 1, 3]) == INVALID and b"not dense" in last_error()
    assert query_rc((2, 3, 2, 2), (1, 2, 6, 12), [0, 2, 3]) == UNSUPPORTED and b"power-of-two" in last_error()
    # pack: a table that is too small, misaligned or null
    d, dims, mat = desc(shape, strides), np.array([0, 1, 3], dtype=np.int32), np.zeros(2 * 64)
    info = N.ArtnWgateInfo()
    assert N.lib().artn_wgate_query(ctypes.byref(d), 3, ptr(dims), ptr(mat), ctypes.byref(info), None, None) == 0
    assert info.table_bytes == 480 + 16 * 64 and info.k == 3 and info.diagonal == 1
    buf = np.zeros(info.table_bytes // 8 + 2, dtype=np.uint64)
    assert N.lib().artn_wgate_pack(ctypes.byref(d), 3, ptr(dims), ptr(mat), ptr(buf), info.table_bytes - 1) == INVALID
    assert b"smaller" in last_error()
    assert N.lib().artn_wgate_pack(ctypes.byref(d), 3, ptr(dims), ptr(mat), ctypes.c_void_p(buf.ctypes.data + 4), info.table_bytes) == UNSUPPORTED
    assert b"8-byte" in last_error()
    assert N.lib().artn_wgate_pack(ctypes.byref(d), 3, ptr(dims), ptr(mat), None, info.table_bytes) == INVALID
    assert N.lib().artn_wgate_pack(ctypes.byref(d), 3, ptr(dims), None, ptr(buf), info.table_bytes) == INVALID
    assert N.lib().artn_wgate_pack(ctypes.byref(d), 3, ptr(dims), ptr(mat), ptr(buf), info.table_bytes) == 0


def test_apply_refuses_bad_pointers_and_runs_nowhere_without_a_gpu():
    """Every call here is refused before anything is launched, so host addresses are safe to pass."""
    shape, strides = (2, 2, 2), (4, 2, 1)
    d, dims = desc(shape, strides), np.array([0, 2, 1], dtype=np.int32)
    buf = np.zeros(256, dtype=np.complex128)
    base = (buf.ctypes.data + 15) & ~15
    a, table, nbytes = base, base + 256, 480 + 16 * 64
    cases = {"small table": (a, table, nbytes - 1, INVALID), "null array": (0, table, nbytes, INVALID), "null table": (a, 0, nbytes, INVALID),
             "misaligned array": (a + 8, table, nbytes, UNSUPPORTED), "misaligned table": (a, table + 4, nbytes, UNSUPPORTED)}
    gpu = N.lib().artn_device_count() > 0
    for name, (pa, pt, nb, want) in cases.items():
        rc = N.lib().artn_wgate_apply(ctypes.byref(d), ctypes.c_void_p(pa), 3, ptr(dims), ctypes.c_void_p(pt), nb, None)
        assert rc == (want if gpu else NODEVICE), name
    if not gpu:
        assert b"gfx950" in last_error()
    t = torch.zeros((2,) * 4, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_wide_gate_(t, np.eye(8), (0, 1, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_circuit_(t, [(np.eye(8), (0, 1, 2)), (np.eye(2), (0,))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.WideGate(t.shape, t.stride(), t.dtype, np.eye(8), (0, 1, 2), "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.FusedCircuit(t.shape, t.stride(), t.dtype, [(np.eye(8), (0, 1, 2))], "cpu")
    with pytest.raises(TypeError):
        A.wide_gate_info((2, 2, 2), (4, 2, 1), np.eye(8), (0, 1, 2), torch.float32)
    with pytest.raises(ValueError, match="entries"):
        A.wide_gate_info((2, 2, 2), (4, 2, 1), np.eye(4), (0, 1, 2))
    with pytest.raises(RuntimeError, match="artn error -2.*one to five"):
        A.wide_gate_info((2,) * 6, contiguous_strides((2,) * 6), np.eye(64), range(6))
    assert A.wide_gate_info((2, 2, 2), (4, 2, 1), np.eye(8).reshape((2,) * 6), (-1, 0, 1))["target_bits"] == (0, 2, 1)


def random_layout(rng, n_bits):
    """Dims of extent 2, and a few of extent 4 and 8, adding up to n_bits memory bits, with a random permutation of the strides."""
    shape, left = [], n_bits
    while left:
        e = int(rng.choice([1, 1, 1, 1, 2, 3])) if len(shape) >= 5 else 1   # (at least five dims of extent 2 where they fit)
        e = min(e, left)
        shape.append(2 ** e)
        left -= e
    shape = [shape[i] for i in rng.permutation(len(shape))]
    perm = rng.permutation(len(shape))
    order = np.argsort(perm)
    strides = contiguous_strides([shape[p] for p in perm])
    return tuple(shape), tuple(strides[order[d]] for d in range(len(shape)))


def random_gate(rng, shape, k):
    twos = [d for d, e in enumerate(shape) if e == 2]
    dims = tuple(int(x) for x in rng.choice(twos, size=k, replace=False))
    return random_unitary(rng, 2 ** k), dims


def layouts_and_gates():
    rng = np.random.default_rng(15)
    for n_bits in range(3, 17):
        for k in range(1, 6):
            shape, strides = random_layout(rng, n_bits)
            if sum(e == 2 for e in shape) < k:
                continue
            yield n_bits, k, shape, strides, random_gate(rng, shape, k)


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_plan_properties(dtype):
    seen = set()
    for n_bits, k, shape, strides, (m, dims) in layouts_and_gates():
        info = A.wide_gate_info(shape, strides, m, dims, dtype)
        target = tuple(int(strides[d]).bit_length() - 1 for d in dims)
        assert info["target_bits"] == target and info["k"] == k              # what the strides say, in the order listed
        tb = min(TB[dtype], n_bits)
        others = [b for b in range(n_bits) if b not in target][:tb - k]
        assert info["tb"] == tb and info["tile_bits"] == sorted(list(target) + others)   # the targets and the LOWEST other bits
        assert info["n_tiles"] << tb == 2 ** n_bits and (n_bits > TB[dtype] or info["n_tiles"] == 1)
        seg = info["segment"]
        assert seg >= 2 ** (tb - k) and seg & (seg - 1) == 0 and info["tile_bits"][:seg.bit_length() - 1] == list(range(seg.bit_length() - 1))
        elem = 8 if dtype == torch.complex64 else 16
        assert info["lds_bytes"] == elem << tb <= 32 * 1024
        assert info["table_bytes"] == 480 + 16 * 4 ** k
        assert info["bytes_read"] == info["bytes_written"] == elem * 2 ** n_bits
        assert not info["diagonal"] and A.wide_gate_info(shape, strides, np.diag(np.diag(m)), dims, dtype)["diagonal"]
        seen.add((k, n_bits > TB[dtype], any(e > 2 for e in shape)))
    assert {(k, big, True) for k in range(1, 6) for big in (False, True)} <= seen


def pack(shape, strides, m, dims, dtype):
    k, dims, mat = WG._split_gate(m, dims, len(shape), "test")
    return WG._wgate_pack(WG._desc(shape, strides, dtype), k, dims, mat)


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_the_packed_table_followed_as_the_kernel_follows_it(dtype):
    """Every index the kernel forms from the table, in numpy: phases 1 and 4 (tile-local index -> memory offset and LDS index)
    and phases 2 and 3 ((row, group) -> LDS index)."""
    for n_bits, k, shape, strides, (m, dims) in layouts_and_gates():
        table, info = pack(shape, strides, m, dims, dtype)
        words = table.view(np.uint64)
        head = [int(w) for w in words[:8]]
        target_bit, target_pos, high_bit, swizzle = (words[8 + 5 * j:13 + 5 * j].astype(np.int64) for j in range(4))
        mem_col, lds_col = words[28:44].astype(np.int64), words[44:60].astype(np.int64)
        tb, n = info.tile_bits, 2 ** n_bits
        gb, n_high = tb - k, head[6]
        assert head[:4] == [k, tb, info.n_tiles, info.segment] and head[4] == 0 and head[5] == gb
        assert table.nbytes == info.table_bytes == 480 + 16 * 4 ** k
        want = tuple(int(strides[d]).bit_length() - 1 for d in dims)
        seg_bits = tb - n_high
        assert 2 ** seg_bits == info.segment and sorted(high_bit[:n_high]) == list(high_bit[:n_high]) and set(high_bit[:n_high]) <= set(want)
        mem, _, _ = follow_columns(tb, k, seg_bits, want, target_bit, target_pos, swizzle, mem_col, lds_col)
        # tiles: every element of the state exactly once
        q = insert_holes(np.arange(info.n_tiles, dtype=np.int64) << seg_bits, high_bit[:n_high])
        every = (q[:, None] | mem[None, :]).reshape(-1)
        assert every.min() == 0 and every.max() == n - 1 and np.array_equal(np.sort(every), np.arange(n))
        # the matrix, row-major (Re, Im), and the mask of its non-zero 8 x 8 blocks
        mat = table[480:].view(np.float64).reshape(2 ** k, 2 ** k, 2)
        assert np.array_equal(mat[..., 0] + 1j * mat[..., 1], m)
        assert head[7] == (1 << max(1, 2 ** k // 8) ** 2) - 1
    table, _ = pack((2,) * 5, contiguous_strides((2,) * 5), np.kron(np.diag([1, 2]), np.ones((16, 16))), range(5), dtype)
    assert int(table.view(np.uint64)[7]) == 0b1100_1100_0011_0011 and int(table.view(np.uint64)[4]) == 0
    table, _ = pack((2,) * 5, contiguous_strides((2,) * 5), np.eye(32), range(5), dtype)
    assert int(table.view(np.uint64)[7]) == 0b1000_0100_0010_0001 and int(table.view(np.uint64)[4]) == N.GATE_DIAGONAL


def random_mixed_circuit(rng, nq, count, widths=(1, 2, 3)):
    gates = []
    for _ in range(count):
        k = int(rng.choice(widths))
        dims = tuple(int(x) for x in rng.choice(nq, size=k, replace=False))
        gates.append((random_unitary(rng, 2 ** k), dims))
    return gates


@pytest.mark.parametrize("seed", range(6))
def test_fuse_gates_keeps_the_unitary(seed):
    rng = np.random.default_rng(seed)
    nq, count = 7, 40
    gates = random_mixed_circuit(rng, nq, count)
    assert {len(d) for _, d in gates} == {1, 2, 3}
    want = dense_unitary(gates, nq)
    counts = []
    for width in (2, 3, 4, 5):
        fused = A.fuse_gates(gates, width)
        assert all(m.dtype == np.complex128 and m.shape == (2 ** len(d),) * 2 for m, d in fused)
        assert all(len(d) <= width or any(set(d) == set(d0) for _, d0 in gates if len(d0) > width) for _, d in fused)
        again = A.fuse_gates(gates, width)
        assert len(again) == len(fused) and all(d == e and np.array_equal(m, o) for (m, d), (o, e) in zip(fused, again))
        err = np.linalg.norm(dense_unitary(fused, nq) - want, 2)
        bound = 16 * count * 2.0 ** -53
        print(f"fuse_gates seed {seed} width {width}: {len(gates)} -> {len(fused)} gates, 2-norm error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
        counts.append(len(fused))
    assert counts[-1] < len(gates)


def test_fuse_gates_on_the_n12_circuit():
    bonds, nq = n12_gates()
    gates = A.gates_from_bonds(bonds, nq)
    want = load_case(os.path.join(GOLDEN, "n12_dense.npz")).arrays["state_vec"]
    counts = {}
    for width in (2, 3, 4, 5):
        fused = A.fuse_gates(gates, width)
        counts[width] = len(fused)
        assert max(len(d) for _, d in fused) <= width and all(tuple(sorted(d)) == d for _, d in fused)
        psi = np.zeros((2,) * nq, dtype=np.complex128)
        psi[(0,) * nq] = 1
        for m, dims in fused:
            psi = numpy_gate(psi, m, dims)
        err = amp_rel(psi.reshape(-1), want)
        print(f"n12 after fuse_gates at width {width}: {len(gates)} -> {len(fused)} gates, amp_rel {err:.3e}")
        assert err < 1e-5
    merged = len(A.merge_gates(gates))
    print(f"n12: merge_gates {merged} gates, fuse_gates {counts}")
    assert counts[2] >= counts[3] >= counts[4] >= counts[5] and counts[4] < merged


def test_fuse_gates_arguments():
    gates = [(np.eye(2), (0,)), (np.eye(4), (0, 1))]
    with pytest.raises(TypeError):
        A.fuse_gates(gates)
    for bad in (1, 6, 0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="max_width"):
            A.fuse_gates(gates, bad)
    with pytest.raises(ValueError, match="distinct"):
        A.fuse_gates([(np.eye(4), (1, 1))], 3)
    with pytest.raises(ValueError, match="distinct"):
        A.fuse_gates([(np.eye(64), range(6))], 5)
    wide = [(np.eye(2), (0,)), (np.eye(32), (4, 3, 2, 1, 0)), (np.eye(2), (4,))]   # wider than max_width: a block of its own
    assert [d for _, d in A.fuse_gates(wide, 3)] == [(0,), (4, 3, 2, 1, 0), (4,)]
    assert [d for _, d in A.fuse_gates(wide, 5)] == [(0, 1, 2, 3, 4)]
    # an open block moves to the gate that joins it, a closed one does not
    x, h = np.array([[0, 1], [1, 0]]), np.array([[1, 1], [1, -1]]) / np.sqrt(2)
    cx = np.eye(4)[[0, 1, 3, 2]]
    out = A.fuse_gates([(h, (0,)), (cx, (1, 2)), (x, (3,)), (cx, (0, 3))], 2)
    assert [d for _, d in out] == [(1, 2), (0, 3)] and np.allclose(out[1][0], cx @ np.kron(h, x))
    out = A.fuse_gates([(cx, (0, 1)), (cx, (1, 2)), (h, (0,))], 2)            # (0, 1) is closed by (1, 2): h cannot join it
    assert [d for _, d in out] == [(0, 1), (1, 2), (0,)]
    out = A.fuse_gates([(cx, (0, 1)), (cx, (1, 2)), (h, (0,))], 3)
    assert [d for _, d in out] == [(0, 1, 2)]
    assert np.allclose(dense_unitary(out, 3), dense_unitary([(cx, (0, 1)), (cx, (1, 2)), (h, (0,))], 3))
