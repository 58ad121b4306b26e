"""Adjoint gradients without a GPU: the numpy oracle of tests/adjoint_oracle.py against two routes that share nothing with the
adjoint formula (dense np.kron matrices: the exact parameter-shift identity and a central difference), and the host-only half of
the C ABI (artn_pauli_adjoint_query, artn_pauli_adjoint_pack): cuts, rank limits, sizes, table flags and refusals."""
import ctypes

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd.pauli import _desc, _evolve_query, _ptr, _split_steps
from adjoint_oracle import oracle_energy, oracle_gradient, oracle_pair
from test_pauli_apply_gpu import P2, crand, ising
from test_pauli_evolve_gpu import random_steps

OK, INVALID, UNSUPPORTED, NODEVICE = 0, -1, -2, -4


def dense(p, nq):
    m = np.eye(1, dtype=np.complex128)
    for c in p:
        m = np.kron(m, P2[c])
    return m


def dense_energy(psi0, rotations, h):
    v = psi0.reshape(-1).astype(np.complex128)
    for theta, p in rotations:
        v = np.cos(theta) * v - 1j * np.sin(theta) * (dense(p, len(p)) @ v)
    return np.vdot(v, h @ v).real / np.vdot(psi0, psi0).real


@pytest.mark.parametrize("nq", [4, 5, 6])
def test_oracle_gradient_against_parameter_shift_and_central_difference(nq):
    rng = np.random.default_rng(nq)
    psi0 = crand(rng, (2,) * nq, "c128")
    rotations = [(float(rng.uniform(-2, 2)), "".join(rng.choice(list("IXYZ"), nq))) for _ in range(7)]
    terms = [(float(rng.standard_normal()), "".join(rng.choice(list("IXYZ"), nq))) for _ in range(5)]
    h = sum(c * dense(p, nq) for c, p in terms)
    e, grad = oracle_gradient(psi0, rotations, terms)
    assert abs(e - dense_energy(psi0, rotations, h)) <= 1e-9
    assert abs(e - oracle_energy(psi0, rotations, terms)) <= 1e-12
    for k, (theta, p) in enumerate(rotations):
        def at(x):
            return dense_energy(psi0, rotations[:k] + [(x, p)] + rotations[k + 1:], h)
        shift = at(theta + np.pi / 4) - at(theta - np.pi / 4)          # exact for exp(-i theta P)
        central = (at(theta + 1e-5) - at(theta - 1e-5)) / 2e-5
        assert abs(grad[k] - shift) <= 1e-9, (k, grad[k], shift)
        assert abs(grad[k] - central) <= 1e-9 * max(1.0, np.abs(h).sum()) + 1e-8, (k, grad[k], central)


def test_oracle_params_sharing_and_constants():
    nq = 5
    rng = np.random.default_rng(11)
    psi0 = crand(rng, (2,) * nq, "c128")
    terms = ising(list(range(nq)))
    layer = lambda g, b: [(g, {a: "Z", a + 1: "Z"}) for a in range(nq - 1)] + [(b, {a: "X"}) for a in range(nq)]
    as_str = lambda p: "".join(p.get(d, "I") for d in range(nq))
    rotations = [(t, as_str(p)) for t, p in layer(0.3, -0.8) + [(0.45, {2: "Y"})] + layer(-0.6, 0.2)]
    params = [0] * (nq - 1) + [1] * nq + [-1] + [2] * (nq - 1) + [3] * nq
    terms = [(c, as_str(p)) for c, p in terms]
    e, grad = oracle_gradient(psi0, rotations, terms, params)
    _, full = oracle_gradient(psi0, rotations, terms)
    assert grad.shape == (4,)
    for q in range(4):
        assert abs(grad[q] - sum(full[k] for k, p in enumerate(params) if p == q)) <= 1e-12
    # against the dense route: all rotations of a parameter shifted together by a small step
    h = sum(c * dense(p, nq) for c, p in terms)
    for q in range(4):
        def at(dx):
            return dense_energy(psi0, [(t + (dx if params[k] == q else 0.0), p) for k, (t, p) in enumerate(rotations)], h)
        assert abs(grad[q] - (at(1e-5) - at(-1e-5)) / 2e-5) <= 1e-7
    t, _, _ = oracle_pair(psi0, psi0, rotations, [p >= 0 for p in params])
    assert t[2 * nq - 1] == 0 and np.all(t[:nq - 1] != 0)


def query(shape, steps, dtype=torch.complex64, measure=None, max_rank=-1):
    coeff, ops = _split_steps(steps, len(shape))
    d = _desc(shape, torch.empty(shape, device="meta").stride(), dtype)
    flags = None if measure is None else np.ascontiguousarray(measure, dtype=np.uint8)
    info = N.ArtnPauliAdjointInfo()
    rc = N.lib().artn_pauli_adjoint_query(ctypes.byref(d), _ptr(ops), _ptr(coeff), None if flags is None else _ptr(flags), len(steps),
                                          max_rank, ctypes.byref(info), *[None] * 8)
    return rc, info, d, ops, coeff, flags


def test_entry_points_exist():
    assert N.has("artn_pauli_adjoint") and N.has("artn_pauli_adjoint_query") and N.has("artn_pauli_adjoint_pack")
    assert N.PAULI_ADJOINT_MAX_RANK == 3
    assert ctypes.sizeof(N.ArtnPauliAdjointInfo) == 4 * 4 + 4 * 8


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_run_cuts_equal_the_single_state_cuts_at_the_same_rank(dtype):
    rng = np.random.default_rng(3)
    shape = (2,) * 16
    steps = random_steps(rng, 16, 40)
    top = 3 if dtype == torch.complex64 else 2
    for max_rank in [None] + list(range(top + 1)):
        info = A.pauli_adjoint_info(shape, torch.empty(shape, device="meta").stride(), steps, dtype, max_rank=max_rank)
        eff = top - 1 if max_rank is None else max_rank
        assert info["max_rank"] == eff
        ref = A.pauli_evolve_info(shape, torch.empty(shape, device="meta").stride(), steps, dtype, max_rank=eff)
        for key in ("xmask", "zmask", "n_y", "run", "slot_mask", "n_runs", "run_rank", "run_basis", "run_pivot", "table_bytes"):
            assert info[key] == ref[key], key
        elem = 8 if dtype == torch.complex64 else 16
        assert info["n_launches"] == info["n_runs"] + 1
        assert info["bytes_read"] == info["bytes_written"] == 2 * info["n_runs"] * 2 ** 16 * elem == 2 * ref["bytes_read"]
        assert info["workspace_bytes"] == 40 * 64 * 64                      # 2^16 elements: 64 tiles
        assert info["table_bytes"] == 32 + 96 * info["n_runs"] + 64 * 40
        assert info["n_measured"] == 40
    assert A.pauli_adjoint_info(shape, torch.empty(shape, device="meta").stride(), steps, dtype, measure=[k % 3 == 0 for k in range(40)]
                                )["n_measured"] == 14
    # the grid limit and the small form
    big = (2,) * 24
    assert A.pauli_adjoint_info(big, torch.empty(big, device="meta").stride(), [(0.1, "X" * 24)], dtype
                                )["workspace_bytes"] == 2048 * 64
    small = (2,) * 9
    info = A.pauli_adjoint_info(small, torch.empty(small, device="meta").stride(), [(0.1, "X" * 9), (0.2, "Z" * 9)], dtype, max_rank=0)
    assert info["n_runs"] == 1 and info["workspace_bytes"] == 2 * 64


def test_rank_caps_and_refusals():
    shape = (2,) * 14
    steps = [(0.3, "X" * 14), (0.2, "ZZ" + "I" * 12)]
    assert query(shape, steps, torch.complex64, max_rank=3)[0] == OK
    assert query(shape, steps, torch.complex64, max_rank=4)[0] == UNSUPPORTED
    assert b"maximum 3" in N.lib().artn_last_error()
    assert query(shape, steps, torch.complex128, max_rank=2)[0] == OK
    assert query(shape, steps, torch.complex128, max_rank=3)[0] == UNSUPPORTED
    assert b"maximum 2" in N.lib().artn_last_error()
    assert query(shape, steps, max_rank=-2)[0] == INVALID
    rc, info, d, ops, coeff, _ = query(shape, steps)
    assert rc == OK and info.max_rank == 2
    lib = N.lib()
    # another dtype
    bad = _desc(shape, torch.empty(shape, device="meta").stride(), torch.complex64)
    bad.dtype = 7
    assert lib.artn_pauli_adjoint_query(ctypes.byref(bad), _ptr(ops), _ptr(coeff), None, 2, -1, ctypes.byref(info), *[None] * 8) == UNSUPPORTED
    # null pointers
    assert lib.artn_pauli_adjoint_query(None, _ptr(ops), _ptr(coeff), None, 2, -1, ctypes.byref(info), *[None] * 8) == INVALID
    assert lib.artn_pauli_adjoint_query(ctypes.byref(d), None, _ptr(coeff), None, 2, -1, ctypes.byref(info), *[None] * 8) == INVALID
    assert lib.artn_pauli_adjoint_query(ctypes.byref(d), _ptr(ops), None, None, 2, -1, ctypes.byref(info), *[None] * 8) == INVALID
    assert lib.artn_pauli_adjoint_query(ctypes.byref(d), _ptr(ops), _ptr(coeff), None, 2, -1, None, *[None] * 8) == INVALID
    table = np.zeros(info.table_bytes // 8 + 1, dtype=np.uint64)
    assert lib.artn_pauli_adjoint_pack(ctypes.byref(d), _ptr(ops), _ptr(coeff), None, 2, -1, None, info.table_bytes) == INVALID
    assert lib.artn_pauli_adjoint_pack(ctypes.byref(d), _ptr(ops), None, None, 2, -1, _ptr(table), info.table_bytes) == INVALID
    assert lib.artn_pauli_adjoint_pack(ctypes.byref(d), _ptr(ops), _ptr(coeff), None, 2, -1, _ptr(table), info.table_bytes - 1) == INVALID
    assert lib.artn_pauli_adjoint_pack(ctypes.byref(d), _ptr(ops), _ptr(coeff), None, 2, -2, _ptr(table), info.table_bytes) == INVALID
    assert lib.artn_pauli_adjoint_pack(ctypes.byref(d), _ptr(ops), _ptr(coeff), None, 2, 4, _ptr(table), info.table_bytes) == UNSUPPORTED
    assert lib.artn_pauli_adjoint_pack(ctypes.byref(d), _ptr(ops), _ptr(coeff), None, 2, -1, ctypes.c_void_p(table.ctypes.data + 4),
                                       info.table_bytes) == UNSUPPORTED
    assert lib.artn_pauli_adjoint_pack(ctypes.byref(d), _ptr(ops), _ptr(coeff), None, 2, -1, _ptr(table), info.table_bytes) == OK


def test_the_table_is_the_evolve_table_with_the_flags_in_the_n_y_word():
    rng = np.random.default_rng(5)
    shape = (2,) * 13
    steps = random_steps(rng, 13, 12)
    measure = [k % 2 == 0 for k in range(12)]
    rc, info, d, ops, coeff, flags = query(shape, steps, measure=measure, max_rank=1)
    assert rc == OK
    table = np.zeros(info.table_bytes // 8, dtype=np.uint64)
    assert N.lib().artn_pauli_adjoint_pack(ctypes.byref(d), _ptr(ops), _ptr(coeff), _ptr(flags), 12, 1, _ptr(table), info.table_bytes) == OK
    ref = np.zeros(info.table_bytes // 8, dtype=np.uint64)
    einfo, _, _, ny, run, _, rank, _, _ = _evolve_query(d, ops, coeff, 1, arrays=True)
    assert einfo.table_bytes == info.table_bytes
    assert N.lib().artn_pauli_evolve_pack(ctypes.byref(d), _ptr(ops), _ptr(coeff), 12, 1, _ptr(ref), info.table_bytes) == OK
    first = 4 + 12 * info.n_runs                                         # 8-byte words before the step records
    word = np.arange(12) * 8 + first + 3
    assert np.array_equal(np.delete(table, word), np.delete(ref, word))
    for k in range(12):
        w = int(table[word[k]])
        assert (w & 0xff, (w >> 8) & 1, (w >> 16) & 0xff, w >> 24) == (int(ny[k]), int(measure[k]), int(rank[run[k]]), 0)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the CPU-only refusal")
def test_no_device_no_computation():
    rc, info, d, ops, coeff, _ = query((2,) * 12, [(0.3, "X" * 12)])
    buf = np.zeros(2 ** 12, dtype=np.complex64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert N.lib().artn_pauli_adjoint(ctypes.byref(d), p, p, _ptr(ops), 1, -1, p, info.table_bytes, p, info.workspace_bytes, p, None) == NODEVICE
    assert b"gfx950" in N.lib().artn_last_error()
    a = torch.zeros((2,) * 12, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.adjoint_gradient(a, [(0.3, "X" * 12)], [(1.0, "Z" * 12)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.pauli_evolve_pair_(a, a.clone(), [(0.3, "X" * 12)])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.PauliPairCircuit(a.shape, a.stride(), a.dtype, [(0.3, "X" * 12)], "cpu")
