"""Host-side checks of the matrix-core gates (artensor_amd/matrix_gates.py: matrix_gate_info, MatrixGate, BlockCircuit,
fuse_gates_wide; artn_mgate_query / _pack / _apply), through the built library: the symbols, the refusals with their codes and
texts, the invariants of the plan and of the packed table followed as the kernel follows it (tests/matrix_gate_oracle.py), the
fusion to widths up to seven and the routing of BlockCircuit.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import matrix_gates as MG
from graph_replay import logical_of
from matrix_gate_oracle import emulate, fields, oracle
from test_gates_cpu import dense_unitary, random_unitary
from test_pauli_apply_cpu import contiguous_strides, desc, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, NODEVICE = -1, -2, -4
TB = {torch.complex64: 12, torch.complex128: 11}
NP = {torch.complex64: np.complex64, torch.complex128: np.complex128}


def last_error():
    return N.lib().artn_last_error()


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_mgate_query", "artn_mgate_pack", "artn_mgate_apply"]
    assert N.ABI_VERSION == 9 and N.lib().artn_abi_version() == 9
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    assert "#define ARTN_MGATE_MAX_K 7" in text and "#define ARTN_WGATE_MAX_K 5" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert N.MGATE_MAX_K == 7 and N.MGATE_TABLE_HEADER_BYTES == 544 and N.WGATE_TABLE_HEADER_BYTES == 480
    for name in ("apply_matrix_gate_", "MatrixGate", "matrix_gate_info", "BlockCircuit", "apply_blocks_", "fuse_gates_wide"):
        assert getattr(A, name) is getattr(MG, name)


def query_rc(shape, strides, dims, mat=None, dtype=N.ARTN_C64, k=None, info=True, null_mat=False):
    k = len(dims) if k is None else k
    dims = np.asarray(list(dims) + [0] * 10, dtype=np.int32)
    if mat is None:
        mat = np.zeros(2 * 4 ** max(min(k, 7), 1))
        mat[0] = 1
    out = N.ArtnMgateInfo()
    return N.lib().artn_mgate_query(ctypes.byref(desc(shape, strides, dtype)), k, ptr(dims), None if null_mat else ptr(mat),
                                    ctypes.byref(out) if info else None, None, None)


def test_the_refusals_and_their_error_codes():
    shape, strides = (2, 2, 4, 2, 2, 2, 2, 2, 2), (1, 2, 4, 16, 32, 64, 128, 256, 512)
    assert query_rc(shape, strides, [0, 1, 3]) == 0
    assert query_rc(shape, strides, [8, 0, 4, 1, 3, 7, 5]) == 0
    assert query_rc(shape, strides, [0, 1], k=2) == UNSUPPORTED and b"three to seven" in last_error()
    assert query_rc(shape, strides, [0, 1, 3, 4, 5, 6, 7, 8], k=8) == UNSUPPORTED and b"three to seven" in last_error()
    assert query_rc((2, 2), (1, 2), [0, 1, 0], k=3) == INVALID and b"at least 2^3" in last_error()
    assert query_rc(shape, strides, [0, 1, 1]) == INVALID and b"differ" in last_error()
    assert query_rc(shape, strides, [0, 9, 1]) == INVALID and b"out of range" in last_error()
    assert query_rc(shape, strides, [0, -1, 1]) == INVALID and b"out of range" in last_error()
    assert query_rc(shape, strides, [0, 2, 1]) == INVALID and b"extent 4" in last_error()
    assert query_rc((2, 3, 2, 2), (1, 2, 6, 12), [0, 2, 3]) == UNSUPPORTED and b"power-of-two" in last_error()
    for bad in (np.nan, np.inf, -np.inf):
        mat = np.zeros(2 * 64)
        mat[77] = bad
        assert query_rc(shape, strides, [0, 1, 3], mat) == INVALID and b"finite" in last_error()
    assert query_rc(shape, strides, [0, 1, 3], info=False) == INVALID and b"null" in last_error()
    assert query_rc(shape, strides, [0, 1, 3], null_mat=True) == INVALID and b"null" in last_error()
    assert query_rc(shape, strides, [0, 1, 3], dtype=N.ARTN_C64_BF16) == UNSUPPORTED and b"complex64 or complex128" in last_error()
    assert query_rc(shape, (1, 2, 4, 16, 32, 64, 128, 256, 1024), [0, 1, 3]) == INVALID and b"not dense" in last_error()
    # pack: a table that is too small, misaligned or null
    d, dims, mat = desc(shape, strides), np.array([0, 1, 3], dtype=np.int32), np.zeros(2 * 64)
    info = N.ArtnMgateInfo()
    assert N.lib().artn_mgate_query(ctypes.byref(d), 3, ptr(dims), ptr(mat), ctypes.byref(info), None, None) == 0
    assert info.table_bytes == 544 + 16 * 64 and info.k == 3 and info.diagonal == 1
    buf = np.zeros(info.table_bytes // 8 + 2, dtype=np.uint64)
    assert N.lib().artn_mgate_pack(ctypes.byref(d), 3, ptr(dims), ptr(mat), ptr(buf), info.table_bytes - 1) == INVALID
    assert b"smaller" in last_error()
    assert N.lib().artn_mgate_pack(ctypes.byref(d), 3, ptr(dims), ptr(mat), ctypes.c_void_p(buf.ctypes.data + 4), info.table_bytes) == UNSUPPORTED
    assert b"8-byte" in last_error()
    assert N.lib().artn_mgate_pack(ctypes.byref(d), 3, ptr(dims), ptr(mat), None, info.table_bytes) == INVALID
    assert N.lib().artn_mgate_pack(ctypes.byref(d), 3, ptr(dims), None, ptr(buf), info.table_bytes) == INVALID
    assert N.lib().artn_mgate_pack(ctypes.byref(d), 3, ptr(dims), ptr(mat), ptr(buf), info.table_bytes) == 0
    # nothing leaked into the wide gates
    with pytest.raises(RuntimeError, match="artn error -2.*one to five"):
        A.wide_gate_info((2,) * 6, contiguous_strides((2,) * 6), np.eye(64), range(6))
    with pytest.raises(RuntimeError, match="artn error -2.*three to seven"):
        A.matrix_gate_info((2,) * 8, contiguous_strides((2,) * 8), np.eye(256), range(8))
    with pytest.raises(RuntimeError, match="artn error -2.*three to seven"):
        A.matrix_gate_info((2,) * 8, contiguous_strides((2,) * 8), np.eye(4), (0, 1))
    assert A.matrix_gate_info((2,) * 7, contiguous_strides((2,) * 7), np.eye(128), range(7))["table_bytes"] == 544 + 256 * 1024


def test_apply_refuses_bad_pointers_and_runs_nowhere_without_a_gpu():
    """Every call here is refused before anything is launched, so host addresses are safe to pass."""
    shape, strides = (2, 2, 2), (4, 2, 1)
    d, dims = desc(shape, strides), np.array([0, 2, 1], dtype=np.int32)
    buf = np.zeros(256, dtype=np.complex128)
    base = (buf.ctypes.data + 15) & ~15
    a, table, nbytes = base, base + 256, 544 + 16 * 64
    cases = {"small table": (a, table, nbytes - 1, INVALID), "null array": (0, table, nbytes, INVALID), "null table": (a, 0, nbytes, INVALID),
             "misaligned array": (a + 8, table, nbytes, UNSUPPORTED), "misaligned table": (a, table + 4, nbytes, UNSUPPORTED)}
    gpu = N.lib().artn_device_count() > 0
    for name, (pa, pt, nb, want) in cases.items():
        rc = N.lib().artn_mgate_apply(ctypes.byref(d), ctypes.c_void_p(pa), 3, ptr(dims), ctypes.c_void_p(pt), nb, None)
        assert rc == (want if gpu else NODEVICE), name
    if not gpu:
        assert b"gfx950" in last_error()
    t = torch.zeros((2,) * 7, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_matrix_gate_(t, np.eye(8), (0, 1, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_blocks_(t, [(np.eye(64), range(6)), (np.eye(2), (0,))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.MatrixGate(t.shape, t.stride(), t.dtype, np.eye(128), range(7), "cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.BlockCircuit(t.shape, t.stride(), t.dtype, [(np.eye(64), range(6))], "cpu")
    with pytest.raises(TypeError):
        A.matrix_gate_info((2, 2, 2), (4, 2, 1), np.eye(8), (0, 1, 2), torch.float32)
    with pytest.raises(ValueError, match="entries"):
        A.matrix_gate_info((2, 2, 2), (4, 2, 1), np.eye(4), (0, 1, 2))
    assert A.matrix_gate_info((2, 2, 2), (4, 2, 1), np.eye(8).reshape((2,) * 6), (-1, 0, 1))["target_bits"] == (0, 2, 1)


# ---- the layouts and target sets shared with the GPU tests ---------------------------------------------------------------------

def layout(n_bits, permuted, seed=0):
    """(shape, strides, dim_of): [2] * n_bits, contiguous (dim d is memory bit n - 1 - d) or with a random assignment of the
    memory bits to the dims; dim_of[b] = the dim on memory bit b."""
    shape = (2,) * n_bits
    bit_of = list(range(n_bits - 1, -1, -1))
    if permuted:
        bit_of = [int(b) for b in np.random.default_rng(100 + seed + n_bits).permutation(n_bits)]
    strides = tuple(1 << b for b in bit_of)
    return shape, strides, {b: d for d, b in enumerate(bit_of)}


def target_sets(n_bits, k, tb):
    """name -> memory bits in the order listed: the lowest, the highest, a set straddling the tile (bits below and at or above
    tb where the state has them), and one listed in descending order."""
    spread = sorted({int(round(x)) for x in np.linspace(0, n_bits - 1, k)})
    spare = [b for b in range(n_bits) if b not in spread]
    while len(spread) < k:
        spread.append(spare.pop())
    spread = sorted(spread)
    mixed = list(range(k - k // 2)) + list(range(n_bits - k // 2, n_bits))
    return {"lowest": tuple(range(k)), "highest": tuple(range(n_bits - k, n_bits)), "straddle": tuple(spread),
            "descending": tuple(sorted(mixed, reverse=True))}


def cases(k, dtype):
    for n_bits in sorted({k, 10, 14}):
        if n_bits < k:
            continue
        for permuted in (False, True):
            shape, strides, dim_of = layout(n_bits, permuted, k)
            for name, bits in target_sets(n_bits, k, TB[dtype]).items():
                yield n_bits, permuted, name, shape, strides, bits, tuple(dim_of[b] for b in bits)


def pack(shape, strides, m, dims, dtype):
    k, dims, mat = MG._split_gate(m, dims, len(shape), "test")
    return MG._mgate_pack(MG._desc(shape, strides, dtype), k, dims, mat)


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128], ids=["c64", "c128"])
@pytest.mark.parametrize("k", [3, 4, 5, 6, 7])
def test_the_plan_and_the_packed_table_followed_as_the_kernel_follows_them(k, dtype):
    rng = np.random.default_rng(1000 * k + TB[dtype])
    elem = 8 if dtype == torch.complex64 else 16
    seen = set()
    for n_bits, permuted, name, shape, strides, bits, dims in cases(k, dtype):
        n = 2 ** n_bits
        m = random_unitary(rng, 2 ** k) if name != "straddle" else rng.standard_normal((2 ** k, 2 ** k)) + 1j * rng.standard_normal((2 ** k, 2 ** k))
        info = A.matrix_gate_info(shape, strides, m, dims, dtype)
        tb = min(TB[dtype], n_bits)
        others = [b for b in range(n_bits) if b not in bits][:tb - k]
        assert info["target_bits"] == bits and info["k"] == k and info["tb"] == tb
        assert info["tile_bits"] == sorted(list(bits) + others) and info["n_tiles"] << tb == n
        assert info["lds_bytes"] == elem << tb <= 32 * 1024 and info["table_bytes"] == 544 + 16 * 4 ** k
        assert info["segment"] * elem >= min(128, n * elem) and info["segment"] >= 2 ** (tb - k)
        table, packed = pack(shape, strides, m, dims, dtype)
        head, arr, u = fields(table)
        assert table.nbytes == info["table_bytes"] and head["k"] == k and head["tile_bits"] == tb and head["reserved"] == 0
        assert np.array_equal(u, m)                            # the fragment order, inverted
        assert tuple(arr["target_bit"][:k]) == bits and not arr["mem_col"][tb:].any() and not arr["lds_col"][tb:].any()
        mem = rng.standard_normal(n) + 1j * rng.standard_normal(n)
        got, trace = emulate(table, mem, np.complex128)
        address = trace["address"].reshape(-1)
        assert address.min() == 0 and address.max() == n - 1                       # every address inside the state
        assert np.array_equal(np.sort(address), np.arange(n))                      # every element loaded and stored once
        assert np.array_equal(np.sort(trace["lds"]), np.arange(2 ** tb))           # the LDS image a bijection
        assert np.array_equal(np.sort(trace["row_group"].reshape(-1)), np.arange(2 ** tb))
        want = oracle(logical_of(mem, shape, strides), m, dims)
        err = np.abs(logical_of(got, shape, strides) - want).max()
        assert err <= 1e-13 * max(1.0, np.abs(want).max()), (n_bits, permuted, name, err)
        seen.add((n_bits, permuted, name))
    assert len(seen) == 8 * len({k, 10, 14})


def random_mixed_circuit(rng, nq, count, widths):
    gates = []
    for _ in range(count):
        w = int(rng.choice(widths))
        dims = tuple(int(x) for x in rng.choice(nq, size=w, replace=False))
        gates.append((random_unitary(rng, 2 ** w), dims))
    return gates


@pytest.mark.parametrize("seed", range(3))
def test_fuse_gates_wide_keeps_the_product(seed):
    rng = np.random.default_rng(seed)
    nq, count = 8, 40
    gates = random_mixed_circuit(rng, nq, count, (1, 2))            # nothing wider than the smallest max_width
    want = dense_unitary(gates, nq)
    counts = []
    for width in range(2, 8):
        fused = A.fuse_gates_wide(gates, width)
        assert all(m.dtype == np.complex128 and m.shape == (2 ** len(d),) * 2 and len(d) <= width for m, d in fused)
        err = np.abs(dense_unitary(fused, nq) - want).max()
        assert err <= 1e-12, (width, err)
        if width <= 5:
            narrow = A.fuse_gates(gates, width)
            assert len(narrow) == len(fused) and all(d == e and np.array_equal(m, o) for (m, d), (o, e) in zip(fused, narrow))
        counts.append(len(fused))
    print(f"fuse_gates_wide seed {seed}: {len(gates)} gates -> {dict(zip(range(2, 8), counts))}")
    assert max(counts[3:]) < counts[0] < len(gates)            # (the walk is greedy: the counts need not fall monotonically)


def test_fuse_gates_wide_arguments():
    gates = [(np.eye(2), (0,)), (np.eye(4), (0, 1))]
    for bad in (1, 8, 0, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="max_width"):
            A.fuse_gates_wide(gates, bad)
    with pytest.raises(ValueError, match="max_width"):
        A.fuse_gates(gates, 6)                                 # fuse_gates keeps its own limit
    with pytest.raises(ValueError, match="distinct"):
        A.fuse_gates([(np.eye(64), range(6))], 5)
    with pytest.raises(ValueError, match="distinct"):
        A.fuse_gates_wide([(np.eye(256), range(8))], 7)
    wide = [(np.eye(2), (0,)), (np.eye(64), (5, 4, 3, 2, 1, 0)), (np.eye(4), (6, 0))]
    assert [d for _, d in A.fuse_gates_wide(wide, 3)] == [(0,), (5, 4, 3, 2, 1, 0), (6, 0)]
    assert [d for _, d in A.fuse_gates_wide(wide, 7)] == [(0, 1, 2, 3, 4, 5, 6)]


class Recorder:
    """Stands in for the three part classes: BlockCircuit's routing is host logic, checked without a device."""
    made = []

    def __init__(self, kind, gates):
        self.kind, self.gates, self.table_bytes, self.n_runs = kind, gates, 8, 2


def test_block_circuit_routing(monkeypatch):
    class FakeGateCircuit(Recorder):
        def __init__(self, shape, strides, dtype, gates, device, max_rank):
            super().__init__("narrow", [tuple(d) if not isinstance(d, int) else (d,) for _, d in gates])

    class FakeWide(Recorder):
        def __init__(self, shape, strides, dtype, matrix, dims, device):
            super().__init__("wide", [tuple(dims)])

    class FakeMatrix(Recorder):
        def __init__(self, shape, strides, dtype, matrix, dims, device):
            super().__init__("matrix", [tuple(dims)])

    monkeypatch.setattr(MG, "GateCircuit", FakeGateCircuit)
    monkeypatch.setattr(MG, "WideGate", FakeWide)
    monkeypatch.setattr(MG, "MatrixGate", FakeMatrix)
    monkeypatch.setattr(MG.BlockCircuit, "_bind", lambda self, shape, strides, dtype, device: setattr(self, "shape", tuple(shape)) or
                        setattr(self, "strides", tuple(strides)) or setattr(self, "device", device))
    shape = (2,) * 8
    strides = contiguous_strides(shape)
    gates = [(np.eye(2), 0), (np.eye(4), (1, 2)), (np.eye(16), (0, 1, 2, 3)), (np.eye(64), range(6)), (np.eye(2), (7,)),
             (np.eye(128), range(7)), (np.eye(8), (5, 6, 7))]

    def kinds(**kw):
        c = MG.BlockCircuit(shape, strides, torch.complex64, gates, "cuda:0", **kw)
        return [p.kind for p in c.parts], c

    got, c = kinds()
    assert got == ["narrow", "wide", "matrix", "narrow", "matrix", "wide"] and c.mfma_from == 6
    assert c.n_launches == 2 + 1 + 1 + 2 + 1 + 1 and c.n_gates == 7 and c.table_bytes == 48
    assert c.parts[0].gates == [(0,), (1, 2)]
    assert kinds(mfma_from=3)[0] == ["narrow", "matrix", "matrix", "narrow", "matrix", "matrix"]
    assert kinds(mfma_from=4)[0] == ["narrow", "matrix", "matrix", "narrow", "matrix", "wide"]
    assert kinds(mfma_from=5)[0] == ["narrow", "wide", "matrix", "narrow", "matrix", "wide"]
    for bad in (7, 8):                                         # the gate on six dims has no route
        with pytest.raises(ValueError, match="matrix cores only"):
            kinds(mfma_from=bad)
    for bad in (2, 9, None, True, 6.0):
        with pytest.raises(ValueError, match="mfma_from"):
            kinds(mfma_from=bad)
    narrow = gates[:3] + gates[4:5] + gates[6:]
    c = MG.BlockCircuit(shape, strides, torch.complex64, narrow, "cuda:0", mfma_from=8)
    assert [p.kind for p in c.parts] == ["narrow", "wide", "narrow", "wide"]
    with pytest.raises(ValueError, match="at least one gate"):
        MG.BlockCircuit(shape, strides, torch.complex64, [], "cuda:0")
    with pytest.raises(ValueError, match="one to 7"):
        MG.BlockCircuit(shape, strides, torch.complex64, [(np.eye(256), range(8))], "cuda:0")
