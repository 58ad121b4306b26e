"""Adjoint gradients of gate circuits without a GPU: the host-only half of the C ABI (artn_gates_adjoint_query,
artn_gates_adjoint_pack: cuts, rank limits, sizes, table and refusals), the numpy oracle of tests/gates_adjoint_oracle.py against
central finite differences, parametric_gate, and the fixture of the GPU gradient test with the condition that lets it fail."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import gate_adjoint as GA
from artensor_amd import gates as G
from gates_adjoint_oracle import oracle_gate, oracle_gate_energy, oracle_gate_gradient, oracle_gate_pair
from test_gates_cpu import contiguous_strides, desc, ptr, random_gates, random_layout, random_unitary
from test_pauli_apply_gpu import crand, ising, oracle_string

OK, INVALID, UNSUPPORTED, NODEVICE = 0, -1, -2, -4
TOP = {torch.complex64: 3, torch.complex128: 2}
NAMES = ["rx", "ry", "rz", "phase", "rxx", "ryy", "rzz", "crx", "cry", "crz", "cphase"]


def test_the_symbols_are_declared_exported_and_bound():
    for name in ("artn_gates_adjoint_query", "artn_gates_adjoint_pack", "artn_gates_adjoint"):
        assert name in N.exported_symbols() and N.has(name)
    assert N.ABI_VERSION == 9 and N.lib().artn_abi_version() == 9
    assert N.GATES_ADJOINT_MAX_RANK == 3 and ctypes.sizeof(N.ArtnGatesAdjointInfo) == 4 * 4 + 4 * 8
    for name in ("gate_adjoint_info", "GatePairCircuit", "apply_gates_pair_", "gate_adjoint_gradient", "parametric_gate"):
        assert hasattr(A, name)


def random_measure(rng, gates, every=2):
    """A dense random M for every `every`-th gate (diagonal for every sixth), None for the others."""
    out = []
    for g, (m, dims) in enumerate(gates):
        rows = 2 ** len(dims)
        mm = rng.standard_normal((rows, rows)) + 1j * rng.standard_normal((rows, rows))
        out.append(None if g % every else (np.diag(np.diag(mm)) if g % 6 == 0 else mm))
    return out


@pytest.mark.parametrize("max_rank", [None, 0, 1, 2, 3])
@pytest.mark.parametrize("nq", [8, 11, 12, 13, 15, 16])
@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_plan_properties(nq, dtype, max_rank):
    top = TOP[dtype]
    if max_rank is not None and max_rank > top:
        with pytest.raises(RuntimeError, match="artn error -2.*two-state maximum"):
            A.gate_adjoint_info((2,) * 14, contiguous_strides((2,) * 14), [(np.eye(2), (0,))], dtype, max_rank=max_rank)
        return
    rng = np.random.default_rng(100 * nq + (7 if max_rank is None else max_rank))
    shape, strides, _ = random_layout(rng, nq)
    gates = random_gates(rng, shape, 60)
    measure = random_measure(rng, gates)
    info = A.gate_adjoint_info(shape, strides, gates, dtype, measure, max_rank)
    eff = top - 1 if max_rank is None else max_rank
    ref = A.gate_circuit_info(shape, strides, gates, dtype, eff)
    assert info["max_rank"] == ref["max_rank"] <= eff
    for key in ("bits", "run", "slot_mask", "local", "n_runs", "run_rank", "run_pivot"):
        assert info[key] == ref[key], key
    n = int(np.prod(shape))
    elem = 8 if dtype == torch.complex64 else 16
    nr = info["n_runs"]
    assert info["n_launches"] == nr + 1
    assert info["bytes_read"] == info["bytes_written"] == 2 * nr * n * elem == 2 * ref["bytes_read"]
    assert info["table_bytes"] == 32 + 64 * nr + N.GATES_ADJOINT_GATE_BYTES * 60 == ref["table_bytes"] + (592 - 320) * 60
    assert info["workspace_bytes"] == 60 * min(max(n >> 10, 1), 2048) * 4 * 2 * 8
    assert info["n_measured"] == 30 and info["measure"] == [m is not None for m in measure]
    assert A.gate_adjoint_info(shape, strides, gates, dtype, None, max_rank)["n_measured"] == 0


def test_default_and_maximum_ranks_and_the_grid_limit():
    shape = (2,) * 24
    strides = contiguous_strides(shape)
    gates = [(np.eye(2), (d,)) for d in range(8)]                           # memory bits 23 .. 16
    for dtype, default, top in ((torch.complex64, 2, 3), (torch.complex128, 1, 2)):
        assert A.gate_adjoint_info(shape, strides, gates, dtype)["max_rank"] == default
        assert A.gate_adjoint_info(shape, strides, gates, dtype, max_rank=top)["max_rank"] == top
        assert A.gate_adjoint_info(shape, strides, gates, dtype, max_rank=top)["n_runs"] == -(-8 // top)
    assert A.gate_adjoint_info(shape, strides, gates)["workspace_bytes"] == 8 * 2048 * 64
    small = (2,) * 9
    info = A.gate_adjoint_info(small, contiguous_strides(small), gates, max_rank=3)
    assert info["n_runs"] == 1 and info["max_rank"] == 0 and info["workspace_bytes"] == 8 * 64
    # a two-qubit gate on two high bits opens a run of rank 2 whatever max_rank is
    cz = np.diag([1, 1, 1, -1])
    for dtype in (torch.complex64, torch.complex128):
        info = A.gate_adjoint_info(shape, strides, [(np.eye(2), (23,)), (cz, (0, 1)), (np.eye(2), (2,))], dtype, max_rank=0)
        assert info["run"] == [0, 0, 1] and info["run_rank"] == [2, 1] and info["max_rank"] == 0


def pair_pack(shape, strides, gates, measure, dtype=torch.complex64, max_rank=None):
    k, dims, mat = G._split_gates(gates, len(shape))
    flags, mmat = GA._split_measure(measure, k)
    d = G._desc(shape, strides, dtype)
    info = GA._pair_query(d, k, dims, mat, mmat, flags, G._max_rank(max_rank))[0]
    table = np.zeros(info.table_bytes // 8, dtype=np.uint64)
    assert N.lib().artn_gates_adjoint_pack(ctypes.byref(d), ptr(k), ptr(dims), ptr(mat), ptr(mmat), ptr(flags), len(k), G._max_rank(max_rank),
                                           ptr(table), info.table_bytes) == OK
    return table, info


@pytest.mark.parametrize("max_rank", [0, 1, None])
def test_the_table_is_the_gate_table_with_the_measure_behind_every_record(max_rank):
    rng = np.random.default_rng(5)
    shape, strides, _ = random_layout(rng, 14)
    gates = random_gates(rng, shape, 30)
    measure = random_measure(rng, gates, every=3)
    table, info = pair_pack(shape, strides, gates, measure, max_rank=max_rank)
    eff = info.max_rank
    k, dims, mat = G._split_gates(gates, len(shape))
    ref, rinfo = G._gates_pack(G._desc(shape, strides, torch.complex64), k, dims, mat, eff)
    nr = info.n_runs
    assert rinfo.n_runs == nr and table.nbytes == info.table_bytes == 32 + 64 * nr + 592 * 30
    ref = ref.view(np.uint64)
    head = 4 + 8 * nr                                                       # 8-byte words before the gate records
    assert np.array_equal(table[:head], ref[:head])
    pinfo = A.gate_adjoint_info(shape, strides, gates, measure=measure, max_rank=max_rank)
    for g in range(30):
        rec = table[head + 74 * g: head + 74 * (g + 1)]
        assert np.array_equal(rec[:40], ref[head + 40 * g: head + 40 * (g + 1)]), g
        rows = 2 ** len(gates[g][1])
        mm = rec[40:72].view(np.float64).reshape(4, 4, 2)
        word = int(rec[72])
        assert int(rec[73]) == 0 and word >> 16 == 0
        assert (word >> 8) & 0xff == pinfo["run_rank"][pinfo["run"][g]]
        if measure[g] is None:
            assert word & 3 == 0 and not mm.any()
            continue
        want = np.zeros((4, 4), dtype=np.complex128)
        want[:rows, :rows] = measure[g]
        assert word & 1 and np.array_equal(mm[..., 0] + 1j * mm[..., 1], want)
        assert bool(word & 2) == (not (want - np.diag(np.diag(want))).any())


def raw_query(shape, strides, k, dims, mat=None, mmat=None, flags=None, dtype=N.ARTN_C64, max_rank=-1, d=True, info=True, null_mat=False):
    k = np.asarray(k, dtype=np.int32)
    dims = np.ascontiguousarray(np.asarray(dims, dtype=np.int32).reshape(len(k), 2))
    if mat is None:
        mat = np.zeros((len(k), 32))
        mat[:, 0] = 1
    out = N.ArtnGatesAdjointInfo()
    return N.lib().artn_gates_adjoint_query(ctypes.byref(desc(shape, strides, dtype)) if d else None, ptr(k), ptr(dims),
                                            None if null_mat else ptr(mat), None if mmat is None else ptr(mmat),
                                            None if flags is None else ptr(np.asarray(flags, dtype=np.uint8)), len(k), max_rank,
                                            ctypes.byref(out) if info else None, *([None] * 6))


def test_the_refusals_and_their_error_codes():
    lib = N.lib()
    shape, strides = (2, 2, 4, 2), (1, 2, 4, 16)
    assert raw_query(shape, strides, [1, 2], [[0, -1], [3, 1]]) == OK
    # ARTN_E_UNSUPPORTED: k outside {1, 2}, another dtype, a rank above the maximum
    assert raw_query(shape, strides, [3], [[0, 1]]) == UNSUPPORTED and b"one or two" in lib.artn_last_error()
    assert raw_query(shape, strides, [0], [[0, 1]]) == UNSUPPORTED
    assert raw_query(shape, strides, [1], [[0, 0]], dtype=7) == UNSUPPORTED
    assert raw_query(shape, strides, [1], [[0, 0]], max_rank=3) == OK
    assert raw_query(shape, strides, [1], [[0, 0]], max_rank=4) == UNSUPPORTED and b"maximum 3" in lib.artn_last_error()
    assert raw_query(shape, strides, [1], [[0, 0]], dtype=N.ARTN_C128, max_rank=2) == OK
    assert raw_query(shape, strides, [1], [[0, 0]], dtype=N.ARTN_C128, max_rank=3) == UNSUPPORTED and b"maximum 2" in lib.artn_last_error()
    # ARTN_E_INVALID: max_rank below -1, null pointers, a bad dim, entries that are not finite
    assert raw_query(shape, strides, [1], [[0, 0]], max_rank=-2) == INVALID
    assert raw_query(shape, strides, [1], [[0, 0]], d=False) == INVALID
    assert raw_query(shape, strides, [1], [[0, 0]], info=False) == INVALID
    assert raw_query(shape, strides, [1], [[0, 0]], null_mat=True) == INVALID
    assert raw_query(shape, strides, [2], [[1, 1]]) == INVALID and b"differ" in lib.artn_last_error()
    assert raw_query(shape, strides, [1], [[4, 0]]) == INVALID and b"out of range" in lib.artn_last_error()
    assert raw_query(shape, strides, [1], [[2, 0]]) == INVALID and b"extent 4" in lib.artn_last_error()
    bad = np.zeros((2, 32))
    bad[1, 3] = np.inf
    assert raw_query(shape, strides, [1, 1], [[0, 0], [1, 0]], mat=bad) == INVALID and b"finite" in lib.artn_last_error()
    good = np.zeros((2, 32))
    bad[1, 3] = np.nan
    assert raw_query(shape, strides, [1, 1], [[0, 0], [1, 0]], mmat=good, flags=[1, 1]) == OK
    assert raw_query(shape, strides, [1, 1], [[0, 0], [1, 0]], mmat=bad, flags=[1, 0]) == OK      # (read for flagged gates only)
    assert raw_query(shape, strides, [1, 1], [[0, 0], [1, 0]], mmat=bad, flags=[0, 1]) == INVALID and b"measure" in lib.artn_last_error()
    assert raw_query(shape, strides, [1, 1], [[0, 0], [1, 0]], mmat=None, flags=[0, 1]) == INVALID
    assert raw_query(shape, strides, [1, 1], [[0, 0], [1, 0]], mmat=None, flags=[0, 0]) == OK
    # pack: a null or small table is invalid, a misaligned one unsupported
    d = desc(shape, strides, N.ARTN_C64)
    k, dims = np.array([1], dtype=np.int32), np.zeros((1, 2), dtype=np.int32)
    mat = np.zeros((1, 32))
    nbytes = 32 + 64 + 592
    table = np.zeros(nbytes // 8 + 1, dtype=np.uint64)
    pack = lambda t, nb, m=mat, mr=-1: lib.artn_gates_adjoint_pack(ctypes.byref(d), ptr(k), ptr(dims), None if m is None else ptr(m), None, None,
                                                                   1, mr, t, nb)
    assert pack(ptr(table), nbytes) == OK
    assert pack(None, nbytes) == INVALID and pack(ptr(table), nbytes - 1) == INVALID and pack(ptr(table), nbytes, m=None) == INVALID
    assert pack(ptr(table), nbytes, mr=-2) == INVALID and pack(ptr(table), nbytes, mr=4) == UNSUPPORTED
    assert pack(ctypes.c_void_p(table.ctypes.data + 4), nbytes) == UNSUPPORTED


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the CPU-only refusal")
def test_no_device_no_computation():
    shape, strides = (2,) * 12, contiguous_strides((2,) * 12)
    d = desc(shape, strides, N.ARTN_C64)
    k, dims = np.array([1], dtype=np.int32), np.zeros((1, 2), dtype=np.int32)
    buf = np.zeros(2 ** 12, dtype=np.complex64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert N.lib().artn_gates_adjoint(ctypes.byref(d), p, p, ptr(k), ptr(dims), 1, -1, p, 32 + 64 + 592, p, 4 * 64, p, None) == NODEVICE
    assert b"gfx950" in N.lib().artn_last_error()
    a = torch.zeros(shape, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.gate_adjoint_gradient(a, [A.parametric_gate("rx", 0.3, 0)], [(1.0, "Z" * 12)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_gates_pair_(a, a.clone(), [(np.eye(2), (0,))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.GatePairCircuit(a.shape, a.stride(), a.dtype, [(np.eye(2), (0,))], "cpu")


# ---- parametric_gate ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_parametric_gate(name):
    two = name in ("rxx", "ryy", "rzz") or name[0] == "c"
    dims = (3, 1) if two else (2,)
    theta, h = 0.73, 1e-5
    u, du, got_dims = A.parametric_gate(name, theta, dims)
    rows = 4 if two else 2
    assert got_dims == dims and u.dtype == du.dtype == np.complex128 and u.shape == du.shape == (rows, rows)
    assert np.abs(u @ u.conj().T - np.eye(rows)).max() <= 1e-14
    central = (A.parametric_gate(name, theta + h, dims)[0] - A.parametric_gate(name, theta - h, dims)[0]) / (2 * h)
    assert np.abs(du - central).max() <= 1e-9
    assert np.abs(A.parametric_gate(name, 0.0, dims)[0] - np.eye(rows)).max() == 0
    x, y, z = (GA._P1[c] for c in "xyz")
    if name in ("rx", "ry", "rz"):
        p = {"rx": x, "ry": y, "rz": z}[name]
        assert np.abs(u - (np.cos(theta / 2) * np.eye(2) - 1j * np.sin(theta / 2) * p)).max() <= 1e-15
    if name == "phase":
        assert np.abs(u - np.diag([1, np.exp(1j * theta)])).max() == 0
    if name == "rzz":
        assert np.abs(u - np.diag(np.exp(-0.5j * theta * np.array([1, -1, -1, 1])))).max() <= 1e-15
    if name[0] == "c":
        # the first listed dim is the control: on the logical array, the slice control = 0 is untouched
        inner = A.parametric_gate(name[1:], theta, 0)[0]
        rng = np.random.default_rng(1)
        psi = crand(rng, (2,) * 4, "c128")
        out = oracle_gate(psi, u, dims)
        assert np.array_equal(out[:, :, :, 0], psi[:, :, :, 0])
        assert np.abs(out[:, :, :, 1] - oracle_gate(psi[:, :, :, 1], inner, (1,))).max() <= 1e-15
    with pytest.raises(ValueError, match="acts on"):
        A.parametric_gate(name, theta, (0,) if two else (0, 1))


def test_parametric_gate_refuses_an_unknown_name():
    with pytest.raises(ValueError, match="unknown gate"):
        A.parametric_gate("u3", 0.1, 0)


# ---- the oracle against finite differences --------------------------------------------------------------------------------------
def test_oracle_gradient_against_central_differences():
    nq, h = 8, 1e-5
    rng = np.random.default_rng(8)
    psi0 = crand(rng, (2,) * nq, "c128")
    names = NAMES + ["ry", "crx", "rzz"]
    spec = []
    for g, name in enumerate(names):
        two = name in ("rxx", "ryy", "rzz") or name[0] == "c"
        dims = tuple(int(x) for x in rng.choice(nq, size=2 if two else 1, replace=False))
        spec.append((name, float(rng.uniform(-np.pi, np.pi)), dims))
    fixed = [(random_unitary(rng, 4), (5, 2)), (random_unitary(rng, 2), (7,))]

    def build(thetas):
        gates = [A.parametric_gate(name, th, dims) for (name, _, dims), th in zip(spec, thetas)]
        return gates[:4] + fixed[:1] + gates[4:] + fixed[1:]

    thetas = [s[1] for s in spec]
    terms = ising(list(range(nq))) + [(0.4, {1: "Y", 6: "Z"})]
    scale = sum(abs(c) for c, _ in terms)
    e, grad = oracle_gate_gradient(psi0, build(thetas), terms)
    assert abs(e - oracle_gate_energy(psi0, build(thetas), terms)) <= 1e-12 * scale
    assert grad.shape == (len(spec),) and np.abs(grad).max() > 1e-3 * scale
    for p in range(len(spec)):
        up, down = list(thetas), list(thetas)
        up[p] += h
        down[p] -= h
        central = (oracle_gate_energy(psi0, build(up), terms) - oracle_gate_energy(psi0, build(down), terms)) / (2 * h)
        assert abs(grad[p] - central) <= 1e-8 * scale, (p, spec[p][0], grad[p], central)
    # shared and constant parameters: the sums of the per-gate derivatives
    params = [0, 1, 0, -1] + [2] * (len(spec) - 5) + [-1]
    _, shared = oracle_gate_gradient(psi0, build(thetas), terms, params)
    assert shared.shape == (3,)
    for q in range(3):
        assert abs(shared[q] - sum(grad[k] for k, p in enumerate(params) if p == q)) <= 1e-12 * scale
    # the pair oracle is what the gradient oracle sweeps
    gates = build(thetas)
    back = [(np.asarray(g[0]).conj().T, g[-1]) for g in gates[::-1]]
    measure = [g[1] @ np.asarray(g[0]).conj().T if len(g) == 3 else None for g in gates[::-1]]
    phi = psi0.astype(np.complex128)
    for g in gates:
        phi = oracle_gate(phi, g[0], g[-1])
    lam = sum(c * oracle_string(phi, p) for c, p in terms)
    t, lam0, phi0 = oracle_gate_pair(lam, phi, back, measure)
    assert np.abs(phi0 - psi0).max() <= 1e-12
    par = [k for k, g in enumerate(gates) if len(g) == 3]
    n2 = np.vdot(psi0, psi0).real
    assert np.abs(2 * t[::-1][par].real / n2 - grad).max() <= 1e-12 * scale


# ---- the fixture of the GPU gradient test ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gradient_fixture():
    """12 qubits, two layers of RY on every qubit, RZ on every qubit, a CNOT ring and RZZ on the even bonds, angles uniform in
    (-pi, pi); Ising terms with -1 ZZ and -0.7 X; start state |0..0>.  (gates, terms, psi0, oracle E, oracle grad)."""
    nq = 12
    rng = np.random.default_rng(2026)
    cnot = np.eye(4)[[0, 1, 3, 2]].astype(np.complex128)
    gates = []
    for layer in range(2):
        gates += [A.parametric_gate("ry", float(rng.uniform(-np.pi, np.pi)), q) for q in range(nq)]
        gates += [A.parametric_gate("rz", float(rng.uniform(-np.pi, np.pi)), q) for q in range(nq)]
        gates += [(cnot, (q, (q + 1) % nq)) for q in range(nq)]
        gates += [A.parametric_gate("rzz", float(rng.uniform(-np.pi, np.pi)), (q, q + 1)) for q in range(0, nq, 2)]
    terms = ising(list(range(nq)))
    psi0 = np.zeros((2,) * nq, dtype=np.complex128)
    psi0[(0,) * nq] = 1
    e, grad = oracle_gate_gradient(psi0, gates, terms)
    return gates, terms, psi0, e, grad


def gradient_bound(kind, n_gates, nq, terms, shared=1):
    """m_p * sum|c| * 2 * ||M|| * (4 c' K + 2^nq 2^-52) with ||M|| = 1/2 and G = 1 (tests/test_gates_adjoint_gpu.py)."""
    c = 2.0 ** -24 if kind == "c64" else 16 * 2.0 ** -53
    return shared * sum(abs(x) for x, _ in terms) * 2 * 0.5 * (4 * c * n_gates + 2.0 ** nq * 2.0 ** -52)


def test_the_gradient_fixture_lets_the_gpu_test_fail():
    gates, terms, psi0, e, grad = gradient_fixture()
    assert len(gates) == 84 and sum(len(g) == 3 for g in gates) == 60 and grad.shape == (60,)
    bound = gradient_bound("c64", 84, 12, terms)
    share = float(np.mean(np.abs(grad) > 20 * bound))
    print(f"fixture: E {e:.4f}, bound {bound:.3e}, |grad| up to {np.abs(grad).max():.3f}, {100 * share:.0f} % above 20 bounds")
    assert 3.8e-4 < bound < 4.0e-4
    assert share >= 0.8
    for u, du, _ in (g for g in gates if len(g) == 3):
        assert abs(np.linalg.norm(du @ u.conj().T, 2) - 0.5) <= 1e-15
