"""Host-side checks of the in-place Pauli circuits (artensor_amd/pauli.py: pauli_evolve_info, PauliCircuit, trotter_steps;
artn_pauli_evolve_query / _pack / artn_pauli_evolve): the symbols, the properties of the run plan (partition, rank cap, greedy
maximality, slot masks, pivots, blocks), the phase convention (the state recomputed in numpy from the info ALONE against an oracle
that applies the 2 x 2 matrices axis by axis), the packed table by the layout documented in include/artn.h, trotter_steps against
a dense matrix exponential, the refusals.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import pauli
from test_pauli_apply_cpu import contiguous_strides, desc, oracle_apply, ptr, random_strings
from test_pauli_cpu import LAYOUTS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHASE = [1, -1j, -1, 1j]                                       # (-i)^ny
TILE_BITS = 10
PLAN_LAYOUTS = dict(LAYOUTS)
PLAN_LAYOUTS["[2]*14"] = ((2,) * 14, contiguous_strides((2,) * 14))


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_pauli_evolve_query", "artn_pauli_evolve_pack", "artn_pauli_evolve"]
    assert N.ABI_VERSION == 9 and N.lib().artn_abi_version() == 9
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    assert "#define ARTN_ABI_VERSION 9" in text and "#define ARTN_PAULI_EVOLVE_MAX_RANK 4" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert ctypes.sizeof(N.ArtnPauliEvolveInfo) == 4 * 4 + 3 * 8
    assert N.PAULI_EVOLVE_MAX_RANK == 4
    for name in ("pauli_evolve_", "pauli_rotate_", "pauli_apply_", "PauliCircuit", "pauli_evolve_info", "trotter_steps"):
        assert getattr(A, name) is getattr(pauli, name)


def random_steps(rng, shape, count):
    """Rotations, applications and general (alpha, beta) steps on random strings, with some diagonal and identity strings."""
    strings = random_strings(rng, shape, count)
    for k in range(0, count, 7):
        strings[k] = "".join("Z" if c in "XY" else c for c in strings[k])           # (xm = 0: never ends a run)
    steps = []
    for k, s in enumerate(strings):
        kind = k % 3
        if kind == 0:
            steps.append((float(rng.uniform(-2, 2)), s))
        elif kind == 1:
            steps.append((0.0, 1.0, s))
        else:
            steps.append((complex(*rng.standard_normal(2)), complex(*rng.standard_normal(2)), s))
    return steps


def gf2_rank(vectors):
    basis = []
    for v in vectors:
        for b in basis:
            v = min(v, v ^ b)
        if v:
            basis.append(v)
    return len(basis)


def xor_of(basis, mask):
    out = 0
    for j, b in enumerate(basis):
        if (mask >> j) & 1:
            out ^= b
    return out


def insert_zeros(q, positions):
    for p in sorted(positions):
        q = ((q >> p) << (p + 1)) | (q & ((1 << p) - 1))
    return q


@pytest.mark.parametrize("max_rank", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("name", list(PLAN_LAYOUTS))
@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_plan_properties(name, dtype, max_rank):
    if dtype == torch.complex128 and max_rank == 4:
        with pytest.raises(RuntimeError, match="max_rank"):
            A.pauli_evolve_info((2,) * 14, contiguous_strides((2,) * 14), [(0.1, "X" * 14)], dtype, max_rank)
        return
    shape, strides = PLAN_LAYOUTS[name]
    rng = np.random.default_rng(len(name) + 10 * max_rank)
    steps = random_steps(rng, shape, 50)
    info = A.pauli_evolve_info(shape, strides, steps, dtype, max_rank)
    ref = A.pauli_info(shape, strides, [s[-1] for s in steps], dtype)
    for key in ("xmask", "zmask", "n_y"):
        assert info[key] == ref[key], key
    n = int(np.prod(shape))
    tile_bits = max(n.bit_length() - 1 - TILE_BITS, 0)                     # log2 of the number of tiles
    cap = min(max_rank, tile_bits)
    assert info["max_rank"] == cap
    hi = [x >> TILE_BITS << TILE_BITS for x in info["xmask"]]
    nr = info["n_runs"]
    assert info["n_launches"] == nr and len(info["run_rank"]) == nr
    # the runs partition the steps in order
    assert info["run"][0] == 0 and info["run"][-1] == nr - 1
    assert all(b - a in (0, 1) for a, b in zip(info["run"][:-1], info["run"][1:]))
    elem = 8 if dtype == torch.complex64 else 16
    assert info["bytes_read"] == info["bytes_written"] == nr * n * elem
    assert info["table_bytes"] == 32 + 96 * nr + 64 * len(steps)
    for r in range(nr):
        members = [k for k in range(len(steps)) if info["run"][k] == r]
        basis, pivot, rank = info["run_basis"][r], info["run_pivot"][r], info["run_rank"][r]
        vectors = [hi[k] for k in members if hi[k]]
        assert rank == len(basis) == len(pivot) == gf2_rank(vectors)
        # at most the cap -- except that a run always takes its first step with a high flip (max_rank = 0: exactly one such step)
        assert rank <= max(cap, 1 if vectors else 0)
        if cap == 0:
            assert len(vectors) <= 1
        # greedy maximality: the step that opens the next run did not fit
        if r + 1 < nr:
            nxt = members[-1] + 1
            assert hi[nxt] != 0 and gf2_rank(vectors + [hi[nxt]]) > cap and vectors
        # reduced echelon form: distinct ascending pivots, each set in exactly one basis vector; every step's xm_hi is the XOR
        # of the basis its slot mask selects
        assert pivot == sorted(set(pivot)) and all(p >= TILE_BITS for p in pivot)
        for j, p in enumerate(pivot):
            assert [(b >> p) & 1 for b in basis] == [int(i == j) for i in range(rank)]
        for k in members:
            assert 0 <= info["slot_mask"][k] < 2 ** rank
            assert xor_of(basis, info["slot_mask"][k]) == hi[k]
        # the blocks enumerated from the pivots partition the tiles
        tiles = max(n >> TILE_BITS, 1)
        if n >= 2 ** TILE_BITS:
            seen = []
            for q in range(tiles >> rank):
                rep = insert_zeros(q, [p - TILE_BITS for p in pivot])
                seen += [rep ^ (xor_of(basis, s) >> TILE_BITS) for s in range(2 ** rank)]
            assert sorted(seen) == list(range(tiles))
    if n >= 2 ** (TILE_BITS + 2) and max_rank >= 1:
        assert max(info["run_rank"]) == cap                               # (the cap is reached)


def test_a_heavy_string_has_rank_one_and_diagonal_steps_never_end_a_run():
    shape = (2,) * 14
    strides = contiguous_strides(shape)
    steps = [(0.3, "X" * 14), (0.1, "ZZ" + "I" * 12), (0.2, "Y" * 14), (0.4, "I" * 13 + "X"), (0.5, "X" + "I" * 13)]
    info = A.pauli_evolve_info(shape, strides, steps, max_rank=1)
    assert info["n_runs"] == 2 and info["run"] == [0, 0, 0, 0, 1] and info["run_rank"] == [1, 1]
    assert info["run_basis"][0] == [0b1111 << 10] and info["run_pivot"][0] == [13] and info["slot_mask"] == [1, 0, 1, 0, 1]
    info = A.pauli_evolve_info(shape, strides, steps, max_rank=0)
    assert info["run"] == [0, 0, 1, 1, 2] and info["max_rank"] == 0
    assert A.pauli_evolve_info(shape, strides, steps)["max_rank"] == 3              # 64 KiB: 8 tiles of complex64
    assert A.pauli_evolve_info(shape, strides, steps, torch.complex128)["max_rank"] == 2
    assert A.pauli_evolve_info((2,) * 11, contiguous_strides((2,) * 11), [(0.3, "X" * 11)])["max_rank"] == 1   # two tiles


def state_from_info(a_mem, info):
    """The state in MEMORY order after the circuit, from the info alone, in complex128."""
    i = np.arange(a_mem.size, dtype=np.uint64)
    a = a_mem.astype(np.complex128)
    for xm, zm, ny, alpha, beta in zip(info["xmask"], info["zmask"], info["n_y"], info["alpha"], info["beta"]):
        par = np.array([bin(int(v) & zm).count("1") & 1 for v in i])
        a = alpha * a + beta * PHASE[ny % 4] * (1.0 - 2.0 * par) * a[(i ^ np.uint64(xm)).astype(np.int64)]
    return a


def step_pair(step):
    if len(step) == 2:
        return np.cos(step[0]), -1j * np.sin(step[0])
    return complex(step[0]), complex(step[1])


def test_the_phase_convention_against_the_axis_by_axis_oracle():
    shape = (2,) * 6
    rng = np.random.default_rng(6)
    a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    steps = random_steps(rng, shape, 12) + [(0.7, "YIIIII"), (0.3 - 0.2j, 1.1j, "YYYIZX"), (0.0, 1.0, "IYIIYI")]
    for perm in (list(range(6)), [3, 0, 5, 1, 4, 2]):
        mem = np.ascontiguousarray(a.transpose(np.argsort(perm)))
        t = mem.transpose(perm)
        assert (t == a).all()
        strides = [s // 16 for s in t.strides]
        info = A.pauli_evolve_info(shape, strides, steps, torch.complex128)
        got_mem = state_from_info(mem.reshape(-1), info)
        got = np.lib.stride_tricks.as_strided(got_mem, shape, [16 * s for s in strides])
        want, growth = a.astype(np.complex128), 1.0
        for step in steps:
            alpha, beta = step_pair(step)
            want = alpha * want + beta * oracle_apply(want, step[-1])
            growth *= max(1.0, abs(alpha) + abs(beta))
        err = np.abs(got - want).max()
        bound = 8 * len(steps) * 2.0 ** -53 * growth * np.abs(a).max()
        print(f"perm {perm}: err {err:.3e} (bound {bound:.3e})")
        assert err <= bound


def test_the_packed_table_decodes_by_the_documented_layout():
    shape, strides = PLAN_LAYOUTS["[2]*14"]
    rng = np.random.default_rng(3)
    steps = random_steps(rng, shape, 30)
    for max_rank in (None, 0, 2):
        info = A.pauli_evolve_info(shape, strides, steps, max_rank=max_rank)
        coeff, ops = pauli._split_steps(steps, 14)
        table, inf = pauli._evolve_pack(pauli._desc(shape, strides, torch.complex64), ops, coeff, pauli._max_rank(max_rank))
        assert table.dtype == np.uint8 and table.size == info["table_bytes"] == inf.table_bytes
        u, f = table.view(np.uint64), table.view(np.float64)
        nr, ns = info["n_runs"], len(steps)
        assert u[:4].tolist() == [nr, ns, info["max_rank"], 0]
        first = 0
        for r in range(nr):
            rec = u[4 + 12 * r: 4 + 12 * (r + 1)].tolist()
            count, rank = info["run"].count(r), info["run_rank"][r]
            assert rec[:4] == [first, count, rank, 0]
            assert rec[4:8] == info["run_basis"][r] + [0] * (4 - rank) and rec[8:12] == info["run_pivot"][r] + [0] * (4 - rank)
            first += count
        assert first == ns
        at = 4 + 12 * nr
        for k in range(ns):
            rec = u[at + 8 * k: at + 8 * k + 4].tolist()
            assert rec == [info["xmask"][k] & 1023, info["slot_mask"][k], info["zmask"][k], info["n_y"][k]]
            alpha, beta = step_pair(steps[k])
            co = f[at + 8 * k + 4: at + 8 * k + 8]
            if len(steps[k]) == 3:
                assert complex(co[0], co[1]) == alpha and complex(co[2], co[3]) == beta
            else:
                assert co[0] == np.cos(steps[k][0]) and co[1] == 0.0 and co[2] == 0.0 and co[3] == -np.sin(steps[k][0])
        assert u.size == at + 8 * ns


# ---- trotter_steps -----------------------------------------------------------------------------------------------------------
P2 = {"I": np.eye(2, dtype=np.complex128), "X": np.array([[0, 1], [1, 0]], dtype=np.complex128),
      "Y": np.array([[0, -1j], [1j, 0]], dtype=np.complex128), "Z": np.diag([1.0, -1.0]).astype(np.complex128)}


def string_matrix(p, nq):
    letters = ["I"] * nq
    for d, c in p.items():
        letters[d] = c
    m = np.ones((1, 1), dtype=np.complex128)
    for c in letters:
        m = np.kron(m, P2[c])
    return m


def test_trotter_steps_against_the_dense_exponential():
    nq = 6
    terms = [(-1.0, {q: "Z", q + 1: "Z"}) for q in range(nq - 1)] + [(-0.7, {q: "X"}) for q in range(nq)]
    mats = [string_matrix(p, nq) for _, p in terms]
    h = sum(c * m for (c, _), m in zip(terms, mats))
    w, v = np.linalg.eigh(h)

    def exact(dt):
        return (v * np.exp(-1j * dt * w)) @ v.conj().T

    def product(steps):
        u = np.eye(2 ** nq, dtype=np.complex128)
        for theta, p in steps:                                             # the first step acts first
            u = (np.cos(theta) * np.eye(2 ** nq) - 1j * np.sin(theta) * string_matrix(p, nq)) @ u
        return u

    first = A.trotter_steps(terms, 0.1)
    assert first == [(0.1 * c, p) for c, p in terms] and A.trotter_steps(terms, 0.1, order=1) == first
    second = A.trotter_steps(terms, 0.1, order=2)
    assert len(second) == 2 * len(terms) - 1 and second == second[::-1]             # symmetric, the middle merged
    assert second[len(terms) - 1] == (0.1 * terms[-1][0], terms[-1][1])
    assert second[:len(terms) - 1] == [(0.05 * c, p) for c, p in terms[:-1]]
    for order, least in ((1, 3.0), (2, 6.0)):
        errs = [np.linalg.norm(product(A.trotter_steps(terms, dt, order)) - exact(dt), 2) for dt in (0.1, 0.05, 0.025)]
        print(f"order {order}: one-step errors {errs}, ratios {errs[0] / errs[1]:.2f} {errs[1] / errs[2]:.2f}")
        assert errs[0] / errs[1] > least and errs[1] / errs[2] > least
        u = product(A.trotter_steps(terms, 0.1, order))
        assert np.abs(u.conj().T @ u - np.eye(2 ** nq)).max() < 1e-13
    with pytest.raises(ValueError, match="real"):
        A.trotter_steps([(1.0, {0: "Z"}), (0.5j, {1: "X"})], 0.1)
    with pytest.raises(ValueError, match="order"):
        A.trotter_steps(terms, 0.1, order=3)
    with pytest.raises(ValueError, match="at least one"):
        A.trotter_steps([], 0.1)


# ---- refusals ----------------------------------------------------------------------------------------------------------------
COEFF2 = np.array([[1.0, 0.0, 0.0, 0.0], [0.5, 0.0, 0.0, -0.5]])


def query(shape, strides, ops, dtype=N.ARTN_C64, n_steps=None, max_rank=-1, coeff=COEFF2):
    ops = np.ascontiguousarray(np.asarray(ops, dtype=np.uint8))
    info = N.ArtnPauliEvolveInfo()
    rc = N.lib().artn_pauli_evolve_query(ctypes.byref(desc(shape, strides, dtype)), ptr(ops), None if coeff is None else ptr(coeff),
                                         ops.shape[0] if n_steps is None else n_steps, max_rank, ctypes.byref(info), *([None] * 8))
    return rc, info


def test_refusals():
    err = N.lib().artn_last_error
    ok = [[3, 0], [1, 2]]
    nbytes = 32 + 96 + 2 * 64
    rc, info = query((2, 2), (2, 1), ok)
    assert rc == 0 and (info.n_runs, info.n_launches, info.max_rank, info.table_bytes) == (1, 1, 0, nbytes)
    for strides in ((1, 1), (4, 1), (2, 2), (0, 1)):                          # a layout that is not dense
        assert query((2, 2), strides, ok)[0] == -1 and b"dense" in err()
    assert query((2, 3), (3, 1), [[1, 0]])[0] == -2 and b"power-of-two" in err()     # an extent that is no power of two
    for code in (1, 2, 3):                                                    # X, Y, Z on a dim of extent 4
        assert query((2, 4), (4, 1), [[0, code]])[0] == -1 and b"extent" in err()
    assert query((2, 2), (2, 1), ok, n_steps=0)[0] == -1 and b"at least one" in err()       # zero steps
    assert query((2, 2), (2, 1), ok, max_rank=5)[0] == -2 and b"max_rank" in err()          # above the maximum
    assert query((2, 2), (2, 1), ok, max_rank=4)[0] == 0
    assert query((2, 2), (2, 1), ok, dtype=N.ARTN_C128, max_rank=4)[0] == -2 and b"max_rank" in err()
    assert query((2, 2), (2, 1), ok, dtype=N.ARTN_C128, max_rank=3)[0] == 0
    assert query((2, 2), (2, 1), ok, max_rank=-2)[0] == -1 and b"max_rank" in err()
    assert query((2, 2), (2, 1), ok, coeff=None)[0] == -1 and b"null" in err()
    d, ops = desc((2, 2), (2, 1)), np.array(ok, dtype=np.uint8)
    table = np.zeros(nbytes // 8 + 1, dtype=np.uint64)
    pack = N.lib().artn_pauli_evolve_pack
    assert pack(ctypes.byref(d), ptr(ops), ptr(COEFF2), 2, -1, ptr(table), nbytes) == 0
    assert pack(ctypes.byref(d), ptr(ops), ptr(COEFF2), 2, -1, ptr(table), nbytes - 1) == -1 and b"table" in err()      # a short table
    assert pack(ctypes.byref(d), ptr(ops), ptr(COEFF2), 2, -1, ctypes.c_void_p(table.ctypes.data + 4), nbytes) == -2 \
        and b"8-byte" in err()                                                                                          # a misaligned one
    assert pack(ctypes.byref(d), ptr(ops), ptr(COEFF2), 2, -1, None, nbytes) == -1
    assert pack(ctypes.byref(d), ptr(ops), ptr(COEFF2), 2, 5, ptr(table), nbytes) == -2 and b"max_rank" in err()
    # through the Python layer
    with pytest.raises(RuntimeError, match="dense"):
        A.pauli_evolve_info((2, 2), (4, 1), [(0.1, "ZZ")])
    with pytest.raises(RuntimeError, match="extent"):
        A.pauli_evolve_info((2, 4), (4, 1), [(0.1, "ZX")])
    with pytest.raises(RuntimeError, match="power-of-two"):
        A.pauli_evolve_info((2, 3), (3, 1), [(0.1, "ZI")])
    with pytest.raises(RuntimeError, match="max_rank"):
        A.pauli_evolve_info((2, 2), (2, 1), [(0.1, "ZZ")], max_rank=5)
    with pytest.raises(ValueError, match="at least one"):
        A.pauli_evolve_info((2, 2), (2, 1), [])
    with pytest.raises(ValueError, match="step 0"):
        A.pauli_evolve_info((2, 2), (2, 1), [("ZZ",)])
    with pytest.raises(TypeError, match="complex"):
        A.pauli_evolve_info((2, 2), (2, 1), [(0.1, "ZZ")], dtype=torch.float32)


def evolve_rc(a_ptr, table_ptr, table_bytes, max_rank=-1):
    """Status code of artn_pauli_evolve on hand-made pointers: [2, 2] complex64, two steps."""
    ops = np.array([[3, 0], [1, 2]], dtype=np.uint8)
    return N.lib().artn_pauli_evolve(ctypes.byref(desc((2, 2), (2, 1))), ctypes.c_void_p(a_ptr), ptr(ops), 2, max_rank,
                                     ctypes.c_void_p(table_ptr), table_bytes, None)


def test_evolve_refuses_bad_pointers_and_runs_nowhere_without_a_gpu():
    """Every call here is refused before anything is launched, so host addresses are safe to pass."""
    err = N.lib().artn_last_error
    buf = np.zeros(64, dtype=np.complex128)
    base = (buf.ctypes.data + 15) & ~15
    a, table, nbytes = base, base + 256, 32 + 96 + 2 * 64
    cases = {
        "short table": (a, table, nbytes - 1, -1, -1, b"table"),
        "misaligned table": (a, table + 4, nbytes, -1, -2, b"8-byte"),
        "misaligned a": (a + 8, table, nbytes, -1, -2, b"16-byte"),
        "null a": (0, table, nbytes, -1, -1, b"null"),
        "max_rank above the maximum": (a, table, nbytes, 5, -2, b"max_rank"),
    }
    for name, (pa, pt, nb, mr, want, text) in cases.items():
        rc = evolve_rc(pa, pt, nb, mr)
        if torch.cuda.is_available():
            assert rc == want and text in err(), name
        else:
            assert rc == -4 and b"no gfx950 device" in err(), name


def test_in_place_functions_have_no_cpu_fallback():
    a = torch.zeros(2, 2, dtype=torch.complex64)
    for call in (lambda: A.pauli_apply_(a, "ZZ"), lambda: A.pauli_rotate_(a, "XI", 0.3),
                 lambda: A.pauli_evolve_(a, [(0.5, "ZZ"), (1.0, 1j, {0: "X"})]),
                 lambda: A.PauliCircuit(a.shape, a.stride(), a.dtype, [(0.3, "ZZ")], "cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
