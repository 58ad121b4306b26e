"""Host-side checks of the in-place gate circuits (artensor_amd/gates.py: gate_circuit_info, GateCircuit, gates_from_bonds,
merge_gates; artn_gates_query / _pack / artn_gates_apply): the symbols, the properties of the run plan on random circuits over
random permuted layouts (order, rank cap and its one exception, gates without high bits, slot masks, blocks), the packed table by
the layout documented in include/artn.h, the refusals with their error codes, gates_from_bonds on the n12 circuit against the
reference's state vector with plain numpy, merge_gates against dense unitaries.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import gates as G
from artensor_amd.fixtures import load_case
from test_gpu_parity import amp_rel
from test_pauli_apply_cpu import contiguous_strides, desc, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
TILE_BITS = 10
INVALID, UNSUPPORTED, NODEVICE = -1, -2, -4


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_gates_query", "artn_gates_pack", "artn_gates_apply"]
    assert N.ABI_VERSION == 9 and N.lib().artn_abi_version() == 9
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    assert "#define ARTN_ABI_VERSION 9" in text and "#define ARTN_GATES_MAX_RANK 4" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert ctypes.sizeof(N.ArtnGatesInfo) == 4 * 4 + 3 * 8
    assert N.GATES_MAX_RANK == 4
    for name in ("apply_gates_", "apply_gate_", "GateCircuit", "gate_circuit_info", "gates_from_bonds", "run_circuit", "merge_gates"):
        assert getattr(A, name) is getattr(G, name)


def random_unitary(rng, dim):
    q, r = np.linalg.qr(rng.standard_normal((dim, dim)) + 1j * rng.standard_normal((dim, dim)))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def random_layout(rng, nq):
    """[2]*nq with a random permutation of the contiguous strides; every third layout carries an extent-1 and an extent-4 dim."""
    shape = [2] * nq
    if nq % 3 == 0:
        shape[int(rng.integers(nq))] = 1
        shape[int(rng.integers(nq))] = 4
    base = contiguous_strides(shape)
    perm = rng.permutation(len(shape))
    order = np.argsort(perm)
    permuted = [shape[p] for p in perm]
    strides = contiguous_strides(permuted)
    return tuple(shape), tuple(strides[order[d]] for d in range(len(shape))), base


def random_gates(rng, shape, count):
    twos = [d for d, e in enumerate(shape) if e == 2]
    gates = []
    for g in range(count):
        k = 1 + int(rng.integers(2))
        dims = tuple(int(x) for x in rng.choice(twos, size=k, replace=False))
        m = random_unitary(rng, 2 ** k)
        if g % 5 == 0:
            m = np.diag(np.diag(m))                                        # (diagonal: thread-local wherever it acts)
        gates.append((m, dims))
    return gates


def insert_zeros(q, positions):
    for p in sorted(positions):
        q = ((q >> p) << (p + 1)) | (q & ((1 << p) - 1))
    return q


@pytest.mark.parametrize("max_rank", [None, 0, 1, 2, 3, 4])
@pytest.mark.parametrize("nq", [8, 11, 12, 13, 15, 16])
@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_plan_properties(nq, dtype, max_rank):
    lib_max = 4 if dtype == torch.complex64 else 3
    if max_rank is not None and max_rank > lib_max:
        with pytest.raises(RuntimeError, match="artn error -2.*max_rank"):
            A.gate_circuit_info((2,) * 14, contiguous_strides((2,) * 14), [(np.eye(2), (0,))], dtype, max_rank)
        return
    rng = np.random.default_rng(100 * nq + (7 if max_rank is None else max_rank))
    shape, strides, _ = random_layout(rng, nq)
    gates = random_gates(rng, shape, 60)
    info = A.gate_circuit_info(shape, strides, gates, dtype, max_rank)
    n = int(np.prod(shape))
    tile_bits = max(n.bit_length() - 1 - TILE_BITS, 0)                     # log2 of the number of tiles
    cap = min(lib_max - 1 if max_rank is None else max_rank, tile_bits)
    assert info["max_rank"] == cap
    # gates keep their order: gate g's bits are those of ITS dims, in the order listed
    assert info["bits"] == [tuple(int(strides[d]).bit_length() - 1 for d in dims) for _, dims in gates]
    high = [sorted(b for b in bits if b >= TILE_BITS) for bits in info["bits"]]
    nr = info["n_runs"]
    assert info["n_launches"] == nr and len(info["run_rank"]) == nr == len(info["run_pivot"])
    assert info["run"][0] == 0 and info["run"][-1] == nr - 1
    assert all(b - a in (0, 1) for a, b in zip(info["run"][:-1], info["run"][1:]))
    elem = 8 if dtype == torch.complex64 else 16
    assert info["bytes_read"] == info["bytes_written"] == nr * n * elem
    assert info["table_bytes"] == 32 + 64 * nr + 320 * len(gates)
    for g, (m, dims) in enumerate(gates):
        diagonal = not np.any(m - np.diag(np.diag(m)))
        assert info["local"][g] == (diagonal or all(b < 2 for b in info["bits"][g]))
    for r in range(nr):
        members = [g for g in range(len(gates)) if info["run"][g] == r]
        pivot, rank = info["run_pivot"][r], info["run_rank"][r]
        with_high = [g for g in members if high[g]]
        assert pivot == sorted({b for g in members for b in high[g]}) and rank == len(pivot)
        # at most the cap -- except that a run always takes its first gate with a high bit; its rank is then that gate's, and
        # only gates on those bits join
        if rank > cap:
            assert rank == len(high[with_high[0]]) and all(set(high[g]) <= set(high[with_high[0]]) for g in with_high)
        # a gate without high bits never opens a run (but the first); the gate that opens the next run did not fit
        if r > 0:
            assert high[members[0]]
        if r + 1 < nr:
            nxt = members[-1] + 1
            assert with_high and len(set(pivot) | set(high[nxt])) > max(cap, rank)
        # the slot masks decode back to the gate's high bits through the pivots
        for g in members:
            assert 0 <= info["slot_mask"][g] < 2 ** rank
            assert sorted(p for j, p in enumerate(pivot) if (info["slot_mask"][g] >> j) & 1) == high[g]
        # the blocks enumerated from the pivots partition the tiles
        if n >= 2 ** TILE_BITS:
            tiles, seen = n >> TILE_BITS, []
            for q in range(tiles >> rank):
                rep = insert_zeros(q, [p - TILE_BITS for p in pivot])
                seen += [rep | sum(1 << (p - TILE_BITS) for j, p in enumerate(pivot) if (s >> j) & 1) for s in range(2 ** rank)]
            assert sorted(seen) == list(range(tiles))
        else:
            assert nr == 1 and rank == 0


def test_a_gate_on_two_high_bits_gets_a_run_of_its_own_below_rank_two():
    shape = (2,) * 14                                                      # dim d is memory bit 13 - d
    strides = contiguous_strides(shape)
    x = np.array([[0, 1], [1, 0]])
    cz = np.diag([1, 1, 1, -1])
    gates = [(x, (13,)), (cz, (0, 1)), (x, (5,)), (x, (0,)), (cz, (1, 0)), (x, (2,)), (cz, (2, 3)), (x, (12,))]
    for max_rank in (0, 1):                                                # (gates on the bits of the rank-2 gate stay in its run)
        info = A.gate_circuit_info(shape, strides, gates, max_rank=max_rank)
        assert info["max_rank"] == max_rank
        assert info["run"] == [0, 0, 0, 0, 0, 1, 2, 2] and info["run_rank"] == [2, 1, 2]
        assert info["run_pivot"] == [[12, 13], [11], [10, 11]]
    info = A.gate_circuit_info(shape, strides, gates, max_rank=2)
    assert info["run"] == [0, 0, 0, 0, 0, 1, 1, 1] and info["run_pivot"] == [[12, 13], [10, 11]]
    assert A.gate_circuit_info(shape, strides, gates, max_rank=4)["n_runs"] == 1


def pack(shape, strides, gates, dtype=torch.complex64, max_rank=None):
    k, dims, mat = G._split_gates(gates, len(shape))
    table, info = G._gates_pack(G._desc(shape, strides, dtype), k, dims, mat, G._max_rank(max_rank))
    return table, info


@pytest.mark.parametrize("max_rank", [0, 2, None])
def test_the_packed_table_decodes_to_the_query(max_rank):
    rng = np.random.default_rng(5)
    shape, strides, _ = random_layout(rng, 14)
    gates = random_gates(rng, shape, 30)
    info = A.gate_circuit_info(shape, strides, gates, max_rank=max_rank)
    table, pinfo = pack(shape, strides, gates, max_rank=max_rank)
    nr, ng = info["n_runs"], len(gates)
    assert table.nbytes == pinfo.table_bytes == info["table_bytes"] == 32 + 64 * nr + 320 * ng
    words = table.view(np.uint64)
    assert list(words[:4]) == [nr, ng, info["max_rank"], 0]
    runs = words[4:4 + 8 * nr].reshape(nr, 8)
    first = 0
    for r in range(nr):
        count = info["run"].count(r)
        assert list(runs[r, :4]) == [first, count, info["run_rank"][r], 0]
        assert list(runs[r, 4:]) == info["run_pivot"][r] + [0] * (4 - info["run_rank"][r])
        first += count
    recs = table[32 + 64 * nr:].reshape(ng, 320)
    for g, (m, dims) in enumerate(gates):
        head = recs[g, :64].view(np.uint64)
        k = len(dims)
        diagonal = not np.any(m - np.diag(np.diag(m)))
        assert head[0] == k and head[1] == (1 if diagonal else 0) | (2 if info["local"][g] else 0)
        bits = list(info["bits"][g])[::-1]                                 # T_0 is the LAST listed dim
        pivot = info["run_pivot"][info["run"][g]]
        for j in range(2):
            b = bits[j] if j < k else None
            assert head[2 + j] == (b if j < k else 0)
            assert head[4 + j] == (1 << pivot.index(b) if j < k and b >= TILE_BITS else 0)
            assert head[6 + j] == (1 << b if j < k and b < TILE_BITS else 0)
        assert (head[4] | head[5]) == info["slot_mask"][g]
        mat = recs[g, 64:].view(np.float64).reshape(4, 4, 2)
        want = np.zeros((4, 4), dtype=np.complex128)
        want[:2 ** k, :2 ** k] = m
        assert np.array_equal(mat[..., 0] + 1j * mat[..., 1], want)


def query_rc(shape, strides, k, dims, mat=None, dtype=N.ARTN_C64, max_rank=-1, n_gates=None):
    k = np.asarray(k, dtype=np.int32)
    dims = np.ascontiguousarray(np.asarray(dims, dtype=np.int32).reshape(len(k), 2))
    if mat is None:
        mat = np.zeros((len(k), 32))
        mat[:, 0] = 1
    info = N.ArtnGatesInfo()
    return N.lib().artn_gates_query(ctypes.byref(desc(shape, strides, dtype)), ptr(k), ptr(dims), ptr(mat), len(k) if n_gates is None else n_gates,
                                    max_rank, ctypes.byref(info), *([None] * 6))


def test_the_refusals_and_their_error_codes():
    shape, strides = (2, 2, 4, 2), (1, 2, 4, 16)
    assert query_rc(shape, strides, [1, 2], [[0, -1], [3, 1]]) == 0
    assert query_rc(shape, strides, [3], [[0, 1]]) == UNSUPPORTED and b"one or two" in N.lib().artn_last_error()
    assert query_rc(shape, strides, [0], [[0, 1]]) == UNSUPPORTED
    assert query_rc(shape, strides, [2], [[1, 1]]) == INVALID and b"differ" in N.lib().artn_last_error()
    assert query_rc(shape, strides, [1], [[4, 0]]) == INVALID and b"out of range" in N.lib().artn_last_error()
    assert query_rc(shape, strides, [1], [[-1, 0]]) == INVALID
    assert query_rc(shape, strides, [2], [[0, 2]]) == INVALID and b"extent 4" in N.lib().artn_last_error()
    for bad in (np.nan, np.inf, -np.inf):
        mat = np.zeros((1, 32))
        mat[0, 5] = bad
        assert query_rc(shape, strides, [2], [[0, 1]], mat) == INVALID and b"finite" in N.lib().artn_last_error()
    mat = np.zeros((1, 32))
    mat[0, 9] = np.nan                                                     # (beyond the 2 x 2 matrix of a one-qubit gate: not read)
    assert query_rc(shape, strides, [1], [[0, 0]], mat) == 0
    # section 13's refusals
    assert query_rc(shape, strides, [1], [[0, 0]], n_gates=0) == INVALID
    assert query_rc(shape, strides, [1], [[0, 0]], max_rank=-2) == INVALID
    assert query_rc(shape, strides, [1], [[0, 0]], max_rank=5) == UNSUPPORTED
    assert query_rc(shape, strides, [1], [[0, 0]], dtype=N.ARTN_C128, max_rank=4) == UNSUPPORTED
    assert query_rc(shape, strides, [1], [[0, 0]], dtype=N.ARTN_C128, max_rank=3) == 0
    assert query_rc(shape, strides, [1], [[0, 0]], dtype=N.ARTN_C64_BF16) == UNSUPPORTED
    assert query_rc(shape, (1, 2, 4, 32), [1], [[0, 0]]) == INVALID and b"not dense" in N.lib().artn_last_error()
    assert query_rc((2, 3), (1, 2), [1], [[0, 0]]) == UNSUPPORTED
    d, k, dims = desc(shape, strides), np.array([1], dtype=np.int32), np.zeros((1, 2), dtype=np.int32)
    mat = np.zeros((1, 32))
    assert N.lib().artn_gates_query(ctypes.byref(d), ptr(k), ptr(dims), ptr(mat), 1, -1, None, *([None] * 6)) == INVALID
    info = N.ArtnGatesInfo()
    assert N.lib().artn_gates_query(ctypes.byref(d), ptr(k), ptr(dims), None, 1, -1, ctypes.byref(info), *([None] * 6)) == INVALID
    # pack: a table that is too small or misaligned
    assert N.lib().artn_gates_query(ctypes.byref(d), ptr(k), ptr(dims), ptr(mat), 1, -1, ctypes.byref(info), *([None] * 6)) == 0
    assert info.table_bytes == 32 + 64 + 320
    buf = np.zeros(info.table_bytes // 8 + 2, dtype=np.uint64)
    assert N.lib().artn_gates_pack(ctypes.byref(d), ptr(k), ptr(dims), ptr(mat), 1, -1, ptr(buf), info.table_bytes - 1) == INVALID
    assert N.lib().artn_gates_pack(ctypes.byref(d), ptr(k), ptr(dims), ptr(mat), 1, -1, ctypes.c_void_p(buf.ctypes.data + 4), info.table_bytes) == UNSUPPORTED
    assert N.lib().artn_gates_pack(ctypes.byref(d), ptr(k), ptr(dims), ptr(mat), 1, -1, None, info.table_bytes) == INVALID
    assert N.lib().artn_gates_pack(ctypes.byref(d), ptr(k), ptr(dims), ptr(mat), 1, -1, ptr(buf), info.table_bytes) == 0


def test_apply_refuses_bad_pointers_and_runs_nowhere_without_a_gpu():
    """Every call here is refused before anything is launched, so host addresses are safe to pass."""
    shape, strides = (2, 2), (2, 1)
    d, k, dims = desc(shape, strides), np.array([1], dtype=np.int32), np.zeros((1, 2), dtype=np.int32)
    buf = np.zeros(128, dtype=np.complex128)
    base = (buf.ctypes.data + 15) & ~15
    a, table, nbytes = base, base + 256, 32 + 64 + 320
    cases = {"small table": (a, table, nbytes - 1, INVALID), "null array": (0, table, nbytes, INVALID), "null table": (a, 0, nbytes, INVALID),
             "misaligned array": (a + 8, table, nbytes, UNSUPPORTED), "misaligned table": (a, table + 4, nbytes, UNSUPPORTED)}
    gpu = N.lib().artn_device_count() > 0
    for name, (pa, pt, nb, want) in cases.items():
        rc = N.lib().artn_gates_apply(ctypes.byref(d), ctypes.c_void_p(pa), ptr(k), ptr(dims), None, 1, -1, ctypes.c_void_p(pt), nb, None)
        assert rc == (want if gpu else NODEVICE), name
    if not gpu:
        assert b"gfx950" in N.lib().artn_last_error()
    t = torch.zeros((2,) * 4, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_gates_(t, [(np.eye(2), (0,))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_gate_(t, np.eye(2), (0,))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.GateCircuit(t.shape, t.stride(), t.dtype, [(np.eye(2), (0,))], "cpu")
    with pytest.raises(TypeError):
        A.gate_circuit_info((2, 2), (2, 1), [(np.eye(2), (0,))], torch.float32)
    with pytest.raises(ValueError, match="at least one gate"):
        A.gate_circuit_info((2, 2), (2, 1), [])
    with pytest.raises(ValueError, match="entries"):
        A.gate_circuit_info((2, 2), (2, 1), [(np.eye(4), (0,))])
    assert A.gate_circuit_info((2, 2), (2, 1), [(np.eye(4).reshape(2, 2, 2, 2), (-1, 0))])["bits"] == [(0, 1)]


def numpy_gate(psi, m, dims):
    """U on the LOGICAL array: np.tensordot over the gate's column digits, np.moveaxis back."""
    k = len(dims)
    u = np.asarray(m, dtype=np.complex128).reshape((2,) * (2 * k))
    return np.moveaxis(np.tensordot(u, psi, axes=(list(range(k, 2 * k)), list(dims))), list(range(k)), list(dims))


def n12_gates():
    case = load_case(os.path.join(GOLDEN, "n12_gates.npz"))
    return [(case.tensors[k], case.meta["inds"][k]) for k in range(len(case.meta["inds"]))], case.meta["n_qubits"]


def test_gates_from_bonds_reproduces_the_reference_state_vector():
    bonds, nq = n12_gates()
    gates = A.gates_from_bonds(bonds, nq)
    assert len(gates) == len(bonds) == 480 and sorted({len(d) for _, d in gates}) == [1, 2]
    psi = np.zeros((2,) * nq, dtype=np.complex128)
    psi[(0,) * nq] = 1
    for m, dims in gates:
        psi = numpy_gate(psi, m, dims)
    want = load_case(os.path.join(GOLDEN, "n12_dense.npz")).arrays["state_vec"]
    err = amp_rel(psi.reshape(-1), want)
    print(f"n12 through gates_from_bonds and numpy: amp_rel {err:.3e}")
    assert err < 1e-5
    with pytest.raises(ValueError, match="do not pair"):
        A.gates_from_bonds([(np.eye(2), ["2-0", "1-0"])], 1)


def dense_unitary(gates, nq):
    u = np.eye(2 ** nq, dtype=np.complex128).reshape((2,) * nq + (2 ** nq,))
    for m, dims in gates:
        u = numpy_gate(u, m, dims)
    return u.reshape(2 ** nq, 2 ** nq)


@pytest.mark.parametrize("seed", range(6))
def test_merge_gates_keeps_the_unitary(seed):
    rng = np.random.default_rng(seed)
    nq, count = 6, 40
    gates = []
    for g in range(count):
        k = 1 if rng.random() < 0.6 else 2
        dims = tuple(int(x) for x in rng.choice(nq, size=k, replace=False))
        if g % 9 == 8 and len(gates[-1][1]) == 2:
            dims = gates[-1][1]                                            # (consecutive gates on identical dims)
            k = 2
        gates.append((random_unitary(rng, 2 ** k), dims))
    merged = A.merge_gates(gates)
    assert len(merged) <= len(gates) and all(m.dtype == np.complex128 for m, _ in merged)
    err = np.linalg.norm(dense_unitary(merged, nq) - dense_unitary(gates, nq), 2)
    bound = 16 * count * 2.0 ** -53
    print(f"merge_gates seed {seed}: {len(gates)} -> {len(merged)} gates, 2-norm error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_merge_gates_shortens_the_n12_circuit():
    bonds, nq = n12_gates()
    gates = A.gates_from_bonds(bonds, nq)
    merged = A.merge_gates(gates)
    assert len(merged) < len(gates)
    psi = np.zeros((2,) * nq, dtype=np.complex128)
    psi[(0,) * nq] = 1
    for m, dims in merged:
        psi = numpy_gate(psi, m, dims)
    want = load_case(os.path.join(GOLDEN, "n12_dense.npz")).arrays["state_vec"]
    assert amp_rel(psi.reshape(-1), want) < 1e-5
    print(f"n12: {len(gates)} gates -> {len(merged)} after merge_gates")
