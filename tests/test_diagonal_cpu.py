"""Host-side checks of the diagonal operators (artensor_amd/diagonal.py; artn_diag_query / _pack / _values / _expect / _apply /
_pair): the symbols, every refusal with its code and a word of its text, the plan and the packed S table against the numpy
oracle (tests/diagonal_oracle.py) on random term lists over permuted layouts, ising_terms and maxcut_terms against brute-force
cost vectors, and the oracle's f (in the contract's order) against an exact sum.  No GPU needed.

(The refusal of a misaligned ARRAY comes after the device check in every entry that takes one, as in the other families, so
it is checked in test_diagonal_gpu.py; here the alignment refusal is the table's, in artn_diag_pack.)"""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import diagonal
from artensor_amd.pauli import _desc, _ptr, pauli_ops

import diagonal_oracle as DO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["artn_diag_query", "artn_diag_pack", "artn_diag_values", "artn_diag_expect", "artn_diag_apply", "artn_diag_pair"]


def contiguous(shape):
    out, s = [], 1
    for e in reversed(shape):
        out.append(s)
        s *= e
    return tuple(reversed(out))


def refused(rc, code, word):
    assert rc == code, (rc, N.lib().artn_last_error())
    assert word in N.lib().artn_last_error().decode(), N.lib().artn_last_error()


def query(shape, strides, strings, dtype=torch.complex64, n_terms=None, ops=None):
    if ops is None:
        ops, _ = pauli_ops(strings, len(shape))
    d = _desc(shape, strides, dtype)
    info = N.ArtnDiagInfo()
    return N.lib().artn_diag_query(ctypes.byref(d), _ptr(ops), ops.shape[0] if n_terms is None else n_terms, ctypes.byref(info),
                                   None, None, None, None, None), info


def test_the_symbols_are_declared_exported_and_bound():
    raw = open(os.path.join(ROOT, "include", "artn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in NAMES:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    consts = dict(re.findall(r"#define (ARTN_DIAG_[A-Z_]+) (\d+)", text))
    assert int(consts["ARTN_DIAG_MAX_GROUPS"]) == N.DIAG_MAX_GROUPS == DO.MAX_GROUPS == 64
    assert int(consts["ARTN_DIAG_MAX_TERMS"]) == N.DIAG_MAX_TERMS == 65536
    assert int(consts["ARTN_DIAG_TILE_BITS"]) == N.DIAG_TILE_BITS == DO.TILE_BITS == 10
    assert (int(consts["ARTN_DIAG_PHASE"]), int(consts["ARTN_DIAG_MULTIPLY"])) == (N.DIAG_PHASE, N.DIAG_MULTIPLY) == (0, 1)
    assert (int(consts["ARTN_DIAG_PAIR_EVOLVE"]), int(consts["ARTN_DIAG_PAIR_TRANSITION"])) == (0, 1)
    assert [int(consts["ARTN_DIAG_OP_" + o]) for o in N.DIAG_OPS] == [0, 1, 2, 3, 4]
    assert re.search(r"#define ARTN_ABI_VERSION 9\b", text) and N.lib().artn_abi_version() == 9
    assert ctypes.sizeof(N.ArtnDiagInfo) == 6 * 4 + 13 * 8
    for name in ("DiagonalOperator", "diagonal_evolve_", "diagonal_expectation", "diagonal_values", "diagonal_info", "ising_terms",
                 "maxcut_terms", "qaoa_gradient"):
        assert getattr(A, name) is getattr(diagonal, name)


def test_every_refusal_of_the_plan():
    shape = (2,) * 12
    st = contiguous(shape)
    refused(query(shape, st, ["IIIIIIIIIIXZ"])[0], -1, "I and Z only")
    refused(query(shape, st, [{0: "Z"}, {3: "Y"}])[0], -1, "term 1")
    refused(query((4, 2), (2, 1), [{0: "Z"}])[0], -1, "extent 2")
    refused(query(shape, st, [{0: "Z"}], n_terms=0)[0], -1, "at least one term")
    refused(query((3, 2), (2, 1), [{1: "Z"}])[0], -2, "power-of-two")
    refused(query(shape, st, [{0: "Z"}], dtype=torch.complex64, ops=np.full((1, 12), 7, dtype=np.uint8))[0], -1, "operator code 7")
    refused(query((2, 2), (4, 1), [{0: "Z"}])[0], -1, "not dense")
    # G: dims 0 and 1 are memory bits 11 and 10 (above the tile); a distinct pattern of the low bits per term is a group each
    def high_terms(count):
        return [{0: "Z", **{11 - b: "Z" for b in range(7) if (j >> b) & 1}} for j in range(count)]
    rc, info = query(shape, st, high_terms(64))
    assert rc == 0 and info.n_groups == 64 and info.n_dynamic == 64 and info.n_static == 0
    refused(query(shape, st, high_terms(65))[0], -2, "65 groups")
    # K: the cap itself passes, one more is refused (before the strings are read)
    ops = np.zeros((N.DIAG_MAX_TERMS + 1, 12), dtype=np.uint8)
    rc, info = query(shape, st, None, ops=ops[:-1])
    assert rc == 0 and info.n_terms == 65536 and info.n_static == 65536 and info.n_groups == 0
    refused(query(shape, st, None, ops=ops)[0], -2, "at most 65536 terms")
    info = N.ArtnDiagInfo()
    refused(N.lib().artn_diag_query(None, _ptr(ops), 1, ctypes.byref(info), None, None, None, None, None), -1, "null descriptor")
    d = _desc(shape, st, torch.complex64)
    refused(N.lib().artn_diag_query(ctypes.byref(d), _ptr(ops), 1, None, None, None, None, None, None), -1, "null info")
    refused(N.lib().artn_diag_query(ctypes.byref(d), None, 1, ctypes.byref(info), None, None, None, None, None), -1, "null pointer")


def test_every_refusal_of_the_pack():
    shape = (2,) * 11
    st = contiguous(shape)
    ops, _ = pauli_ops([{0: "Z", 10: "Z"}, {5: "Z"}], 11)
    d = _desc(shape, st, torch.complex128)
    need = 64 + 8 * 1024 + 32 + 16
    rc, info = query(shape, st, None, dtype=torch.complex128, ops=ops)
    assert rc == 0 and info.table_bytes == need and info.workspace_bytes == 2 * 32
    table = np.zeros(need // 8 + 2, dtype=np.uint64)
    c = np.array([0.5, -1.25])
    p = lambda coeff, tab, nbytes: N.lib().artn_diag_pack(ctypes.byref(d), _ptr(ops), coeff, 2, tab, nbytes)   # noqa: E731
    refused(p(None, _ptr(table), need), -1, "null pointer")
    refused(p(_ptr(c), None, need), -1, "null pointer")
    refused(p(_ptr(np.array([0.5, np.inf])), _ptr(table), need), -1, "coefficient of term 1 is not finite")
    refused(p(_ptr(c), _ptr(table), need - 8), -1, "table smaller than artn_diag_query reports")
    refused(p(_ptr(c), ctypes.c_void_p(table.ctypes.data + 4), need), -2, "artn_diag_pack needs an 8-byte aligned table")
    assert p(_ptr(c), _ptr(table), need) == 0
    assert table[:6].tolist() == [2, 1, 1, 1, 10, 2]


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the CPU-only refusal")
def test_the_device_entries_refuse_without_a_device():
    lib = N.lib()
    shape = (2,) * 4
    d = _desc(shape, contiguous(shape), torch.complex64)
    ops, _ = pauli_ops([{0: "Z"}], 4)
    buf = np.zeros(1024, dtype=np.uint64)
    p = _ptr(buf)
    word = "no gfx950 device visible"
    refused(lib.artn_diag_values(ctypes.byref(d), _ptr(ops), 1, p, 8192, p, None), -4, word)
    refused(lib.artn_diag_expect(ctypes.byref(d), p, _ptr(ops), 1, p, 8192, p, 8192, p, None), -4, word)
    refused(lib.artn_diag_apply(ctypes.byref(d), p, _ptr(ops), 1, p, 8192, 0, 0.5, None), -4, word)
    refused(lib.artn_diag_pair(ctypes.byref(d), p, p, _ptr(ops), 1, p, 8192, 0, 0.5, p, 8192, p, None), -4, word)


def test_python_side_checks():
    shape = (2,) * 4
    with pytest.raises(ValueError, match="real coefficients"):
        A.diagonal_info(shape, contiguous(shape), [(1j, {0: "Z"})])
    with pytest.raises(ValueError, match="at least one term"):
        A.diagonal_info(shape, contiguous(shape), [])
    with pytest.raises(RuntimeError, match="I and Z only"):
        A.diagonal_info(shape, contiguous(shape), [(1.0, "XIII")])
    with pytest.raises(TypeError, match="complex64 or complex128"):
        A.diagonal_info(shape, contiguous(shape), [(1.0, "ZIII")], dtype=torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.DiagonalOperator(shape, contiguous(shape), torch.complex64, [(1.0, "ZIII")], "cpu")
    cpu = torch.zeros(shape, dtype=torch.complex64)
    for call in (lambda: A.qaoa_gradient(cpu, [(1.0, "ZZII")], [0.1], [0.2]), lambda: A.diagonal_evolve_(cpu, [(1.0, "ZZII")], 0.1),
                 lambda: A.diagonal_expectation(cpu, [(1.0, "ZZII")])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError, match="DiagonalOperator expected"):
        A.diagonal_values(cpu)


def random_terms(rng, nd, count, qubits):
    terms = []
    for _ in range(count):
        k = int(rng.integers(0, 4))
        dims = rng.choice(qubits, size=min(k, len(qubits)), replace=False) if k else []
        terms.append((float(rng.choice([-2.0, -0.75, 0.5, 1.0, 3.25, 1e-3])), {int(q): "Z" for q in dims}))
    terms.append(terms[0])                                                 # a repeated string is a term of its own
    return terms


LAYOUTS = [((2,) * 5, None), ((2,) * 10, 3), ((2,) * 13, None), ((2,) * 13, 5), ((2, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 4), 7),
           ((2,) * 16, 11)]


@pytest.mark.parametrize("shape, seed", LAYOUTS)
def test_the_query_and_the_packed_table_equal_the_oracle(shape, seed):
    rng = np.random.default_rng(100 + (seed or 0))
    nd = len(shape)
    st = list(contiguous(shape))
    if seed is not None:                                                   # a permuted dense layout: shuffle which dim owns which stride
        moving = [i for i, e in enumerate(shape) if e == 2]
        perm = rng.permutation(len(moving))
        st2 = list(st)
        for a, b in zip(moving, perm):
            st2[a] = st[moving[b]]
        st = st2
    qubits = [i for i, e in enumerate(shape) if e == 2]
    terms = random_terms(rng, nd, 40, qubits)
    plan = DO.Plan(shape, st, terms)
    info = A.diagonal_info(shape, st, terms, dtype=torch.complex128)
    assert info["zmask"] == plan.zm and info["lo"] == plan.lo and info["hi"] == plan.hi
    assert info["group"] == plan.group and info["group_lo"] == plan.group_lo and info["G"] == plan.G
    assert (info["K"], info["n_static"], info["n_dynamic"]) == (len(terms), len(plan.static), plan.n_dynamic)
    assert info["tile_bits"] == plan.tb and info["n_tiles"] == plan.n >> plan.tb and info["table_bytes"] == plan.table_bytes
    assert info["bytes_read"]["PHASE"] == info["bytes_written"]["MULTIPLY"] == plan.n * 16
    assert info["bytes_written"]["VALUES"] == plan.n * 8 and info["bytes_written"]["EXPECT"] == 0
    coeff, ops = diagonal._split(terms, nd, "test")
    table, _ = diagonal._pack(_desc(shape, st, torch.complex128), ops, coeff)
    S = table[8:8 + (1 << plan.tb)]
    assert np.array_equal(S, plan.static_table().view(np.uint64))          # bit for bit
    recs = table[8 + (1 << plan.tb):]
    at = 0
    for g in range(plan.G):
        assert recs[4 * g:4 * g + 4].tolist() == [plan.group_lo[g], at, len(plan.members[g]), 0]
        at += len(plan.members[g])
    trm = recs[4 * plan.G:].reshape(-1, 2)
    order = [k for g in range(plan.G) for k in plan.members[g]]
    assert trm[:, 0].tolist() == [plan.hi[k] for k in order]
    assert np.array_equal(trm[:, 1], np.array([plan.coeff[k] for k in order]).view(np.uint64))


def brute_force(n, fn):
    """fn(z) for every bitstring of a contiguous [2]*n state in memory order: dim q is memory bit n - 1 - q, z_q = +-1."""
    out = np.zeros(1 << n)
    for i in range(1 << n):
        z = [1 - 2 * ((i >> (n - 1 - q)) & 1) for q in range(n)]
        out[i] = fn(z)
    return out


def test_ising_and_maxcut_terms_against_brute_force():
    n = 6
    shape, st = (2,) * n, contiguous((2,) * n)
    rng = np.random.default_rng(5)
    J = {(q, r): float(rng.integers(-4, 5)) / 4 for q, r in itertools.combinations(range(n), 2) if rng.random() < 0.6}
    h = {q: float(rng.integers(-4, 5)) / 8 for q in range(n)}
    want = brute_force(n, lambda z: sum(c * z[q] * z[r] for (q, r), c in J.items()) + sum(c * z[q] for q, c in h.items()) + 0.5)
    assert np.array_equal(DO.Plan(shape, st, A.ising_terms(J, h, 0.5)).values(), want)      # quarters and eighths: exact
    Jm = np.zeros((n, n))
    for (q, r), c in J.items():
        Jm[q, r] = c
    hv = [h[q] for q in range(n)]
    assert np.array_equal(DO.Plan(shape, st, A.ising_terms(Jm, hv, 0.5)).values(), want)
    assert np.array_equal(DO.Plan(shape, st, A.ising_terms(Jm + Jm.T, hv, 0.5)).values(), want)   # a symmetric matrix: each bond once
    with pytest.raises(ValueError, match="lower triangle"):
        A.ising_terms(Jm + 2 * Jm.T)
    with pytest.raises(ValueError, match="listed twice"):
        A.ising_terms({(0, 1): 1.0, (1, 0): 1.0})
    edges = [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (5, 0), (0, 3)]
    w = [1.0, 2.0, 0.5, 1.0, 3.0, 1.0, 0.25]
    cut = brute_force(n, lambda z: sum(x for (q, r), x in zip(edges, w) if z[q] != z[r]))
    assert np.array_equal(DO.Plan(shape, st, A.maxcut_terms(edges, w)).values(), cut)
    assert np.array_equal(DO.Plan(shape, st, A.maxcut_terms(edges)).values(), brute_force(n, lambda z: sum(z[q] != z[r] for q, r in edges)))


def test_the_contract_order_agrees_with_an_exact_sum():
    shape = (2,) * 13
    rng = np.random.default_rng(9)
    st = [int(s) for s in np.array(contiguous(shape))[rng.permutation(13)]]
    terms = [(float(rng.standard_normal()), {int(q): "Z" for q in rng.choice(13, size=int(rng.integers(1, 5)), replace=False)})
             for _ in range(60)]
    f = DO.Plan(shape, st, terms).values()
    scale = sum(abs(c) for c, _ in terms)
    for i in rng.integers(0, 1 << 13, size=300):
        assert abs(f[i] - math.fsum(DO.values_plain(shape, st, terms, int(i)))) <= 1e-13 * scale
