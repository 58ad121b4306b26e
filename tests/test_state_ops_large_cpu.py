"""The machinery of tests/test_state_ops_large_gpu.py (tests/exact_state.py: the index hash, the expected values by recursion
over partner indices, the comparator) at 2^10 to 2^14 elements with torch on the CPU, against oracles that share nothing with
it: numpy_gate (np.tensordot on the logical array, test_gates_cpu.py), oracle_apply (axis by axis, test_pauli_apply_cpu.py) and
string_matrix (np.kron, test_pauli_evolve_cpu.py).  Then numpy stand-ins for a kernel plant five plausible errors, and the
comparator has to reject each: this is what a green run of the GPU module is worth.  No GPU needed."""
import numpy as np
import pytest
import torch

import artensor_amd as A
import exact_state as E
from test_gates_cpu import numpy_gate
from test_pauli_apply_cpu import oracle_apply
from test_pauli_evolve_cpu import string_matrix

SMALL = 1 << 9                                                            # chunk of the small runs: several chunks per array


def hash_state(n_elems):
    f, g = E.hash_index(torch.arange(n_elems))
    return f.numpy().astype(np.float64) + 1j * g.numpy().astype(np.float64)


def as_store(a, dtype=torch.complex64):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).to(dtype)


# ---- 1. the hash --------------------------------------------------------------------------------------------------------------
def test_hash_values_range_and_int64_arithmetic():
    rng = np.random.default_rng(0)
    idx = np.concatenate([np.arange(64), rng.integers(0, 1 << 34, 400), [(1 << 34) - 1, (1 << 32) - 1, 1 << 32, 1 << 31, 1 << 33]])
    f, g = E.hash_index(torch.from_numpy(idx.astype(np.int64)))
    assert f.dtype == g.dtype == torch.int64
    assert [(int(a), int(b)) for a, b in zip(f, g)] == [E.hash_python(int(i)) for i in idx]     # no overflow: unbounded integers agree
    f, g = E.hash_index(torch.arange(1 << 16))
    for v in (f, g):
        assert int(v.min()) == -8 and int(v.max()) == 7
        counts = np.bincount(v.numpy() + 8, minlength=16)
        assert counts.min() > 0.8 * 4096 and counts.max() < 1.2 * 4096
    assert E.M32 * E.MIX < 1 << 59 and 3 * E.HIGH < 1 << 32


def test_hash_depends_on_every_index_bit_up_to_33():
    rng = np.random.default_rng(1)
    idx = torch.from_numpy(rng.integers(0, 1 << 34, 4096).astype(np.int64))
    f0, g0 = E.hash_index(idx)
    for bit in range(34):
        f1, g1 = E.hash_index(idx ^ (1 << bit))
        changed = float(((f0 != f1) | (g0 != g1)).double().mean())
        assert changed > 0.9, (bit, changed)                              # (two independent 4-bit values differ with 255/256)
        assert float((f0 != f1).double().mean()) > 0.8 and float((g0 != g1).double().mean()) > 0.8, bit


def test_fill_is_the_hash_whatever_the_chunk():
    for dtype in (torch.complex64, torch.complex128):
        store = E.fill(torch.zeros(5000, dtype=dtype), chunk=SMALL)
        assert np.array_equal(store.numpy().astype(np.complex128), hash_state(5000))
        assert E.compare_all(store, [], chunk=SMALL) == {"compared": 5000, "bad": 0, "first_bad": None, "peak": 8}
    assert E.hash_norm2(5000, "cpu", chunk=SMALL) == int(round((np.abs(hash_state(5000)) ** 2).sum()))


# ---- 2. gates -----------------------------------------------------------------------------------------------------------------
POOL1 = [E.G1, E.U5, E.U2, E.V2, E.X, E.Y, E.Z, E.S]
POOL2 = [E.G2, E.D10A, E.D10B, E.D4, E.CNOT, E.SWAP, E.CZ, E.ISWAP]


def random_gates(rng, nq, count, dense_two=3):
    """Gates on memory bits: dense and permutation matrices of both pools, both orders of the bits; at most `dense_two` dense
    4 x 4 matrices (4 partners each)."""
    gates, dense = [], 0
    for g in range(count):
        k = 1 + (g % 3 != 0)
        bits = tuple(int(b) for b in rng.choice(nq, size=k, replace=False))
        pool = POOL1 if k == 1 else POOL2
        m = pool[int(rng.integers(len(pool)))]
        if k == 2 and np.count_nonzero(m) > 4:
            dense += 1
            if dense > dense_two:
                m = POOL2[4 + g % 4]
        gates.append((m, bits))
    return gates


def oracle_gates(a_flat, nq, gates, perm=None):
    """numpy_gate on the logical array: the contiguous [2]*nq array (dim d = memory bit nq - 1 - d), permuted by `perm`."""
    perm = list(range(nq)) if perm is None else list(perm)
    psi = a_flat.reshape((2,) * nq).transpose(perm)
    for m, bits in gates:
        psi = numpy_gate(psi, m, [perm.index(nq - 1 - b) for b in bits])
    return np.ascontiguousarray(psi.transpose(np.argsort(perm))).reshape(-1)


@pytest.mark.parametrize("nq", [10, 13, 14])
def test_expected_gate_values_against_numpy_gate(nq):
    rng = np.random.default_rng(nq)
    a = hash_state(1 << nq)
    gates = random_gates(rng, nq, 12)
    assert any(b[0] < b[-1] for _, b in gates) and any(b[0] > b[-1] for _, b in gates)
    ops = E.gate_ops(gates)
    want = oracle_gates(a, nq, gates)
    re, im = E.evaluate(ops, torch.arange(1 << nq))
    assert np.array_equal(re.numpy() + 1j * im.numpy(), want)
    assert max(np.abs(want.real).max(), np.abs(want.imag).max()) <= E.bound(ops)
    for dtype in (torch.complex64, torch.complex128):
        rep = E.compare_all(as_store(want, dtype), ops, chunk=1 << 15)
        E.assert_exact(rep, ops, dtype, f"{nq} qubits")
        assert rep["compared"] == 1 << nq and rep["peak"] == int(max(np.abs(want.real).max(), np.abs(want.imag).max()))
    sample = torch.from_numpy(rng.permutation(1 << nq)[:300].astype(np.int64))
    assert E.compare_sample(as_store(want), ops, sample, chunk=1 << 12)["bad"] == 0


def test_the_cases_of_the_large_tests_on_a_small_array():
    """whole_gate_cases and the matrices of fused_gates, the top bits of 2^14 elements standing in for those of 2^30; the
    permuted view as the GPU module builds it: bits from strides."""
    nq = 14
    a = hash_state(1 << nq)
    for name, (gates, _) in E.whole_gate_cases(nq).items():
        assert E.compare_all(as_store(oracle_gates(a, nq, gates)), E.gate_ops(gates), chunk=1 << 13)["bad"] == 0, name
    view = torch.zeros(1 << nq, dtype=torch.complex64).view((2,) * nq).permute([2, 0, 1] + list(range(3, nq)))
    api = [(E.G2, (0, 2)), (E.G1, (1,))]
    gates = [(m, tuple(int(view.stride(d)).bit_length() - 1 for d in dims)) for m, dims in api]
    assert [b for _, b in gates] == [(nq - 3, nq - 2), (nq - 1,)]
    assert A.gate_circuit_info(view.shape, view.stride(), api)["bits"] == [b for _, b in gates]
    psi = a.reshape((2,) * nq).transpose([2, 0, 1] + list(range(3, nq)))
    for m, dims in api:
        psi = numpy_gate(psi, m, list(dims))
    want = np.ascontiguousarray(psi.transpose([1, 2, 0] + list(range(3, nq)))).reshape(-1)
    assert E.compare_all(as_store(want), E.gate_ops(gates), chunk=1 << 13)["bad"] == 0
    psi = a.reshape((2,) * nq)
    for alpha, beta, letters in E.whole_steps(nq):
        psi = alpha * psi + beta * oracle_apply(psi, E.api_string(nq, letters))
    assert E.compare_all(as_store(psi), E.step_ops(E.whole_steps(nq)), chunk=1 << 12)["bad"] == 0
    terms = E.sum_terms(nq)
    y = sum(c * oracle_apply(a.reshape((2,) * nq), E.api_string(nq, l)) for c, l in terms)
    assert E.compare_all(as_store(y), [E.PauliSum(terms)], chunk=1 << 12)["bad"] == 0


def test_scale2_is_the_growth_of_the_norm():
    nq = 12
    gates = [(E.D10A, (11, 10)), (E.CNOT, (3, 11)), (E.D10B, (2, 9)), (E.S, (10,)), (E.D4, (9, 11)), (E.U5, (0,)), (E.ISWAP, (5, 11))]
    ops = E.gate_ops(gates)
    assert E.scale2(ops) == 10 * 10 * 4 * 5 and E.scale2(E.gate_ops([(E.G2, (1, 0))])) is None
    store = as_store(oracle_gates(hash_state(1 << nq), nq, gates))
    direct = E.expected_norm2(store, ops, chunk=1 << 14)
    assert direct == E.scale2(ops) * E.hash_norm2(1 << nq, "cpu") == int(round(float((store.abs().double() ** 2).sum())))
    steps = [(1, 2j, {11: "X", 3: "Z"}), (0, 1j, {10: "Y", 11: "Z"}), (1 + 1j, 1 - 1j, {0: "Y", 9: "X"})]
    assert E.scale2(E.step_ops(steps)) == 5 * 1 * 4 and E.scale2(E.step_ops([(1, 1, {0: "X"})])) is None
    assert E.expected_norm2(store, E.step_ops(steps), chunk=1 << 12) == 20 * E.hash_norm2(1 << nq, "cpu")


# ---- 3. the circuits of the GPU module: plans, bounds, sample sets (host only) ------------------------------------------------
@pytest.mark.parametrize("n, dtype", [(30, torch.complex64), (29, torch.complex128), (32, torch.complex64)])
def test_the_large_circuits_meet_their_conditions(n, dtype):
    shape, strides = (2,) * n, tuple(1 << (n - 1 - d) for d in range(n))
    mean_norm2 = 43                                                        # E f^2 + E g^2 = 2 * 21.5 of uniform values in [-8, 7]
    gates = E.fused_gates(n)
    ops = E.gate_ops(gates)
    assert len(gates) == 30 and sum(op.T == 4 for op in ops) == 5 and all(op.T == 1 for op in ops if op.T != 4)
    info = A.gate_circuit_info(shape, strides, E.api_gates(n, gates), dtype)
    assert info["n_runs"] >= 3 and max(info["run_rank"]) == info["max_rank"] >= 2 and sum(r >= 2 for r in info["run_rank"]) >= 3
    assert len({b for _, bits in gates for b in bits if b >= 22}) >= 4
    assert E.bound(ops) < 1 << 24 and E.scale2(ops) * mean_norm2 * 2 ** n < 1 << 53
    steps = E.fused_steps(n)
    ops = E.step_ops(steps)
    assert len(steps) == 30 and sum(op.T == 2 for op in ops) == 7
    info = A.pauli_evolve_info(shape, strides, E.api_steps(n, steps), dtype)
    assert info["n_runs"] >= 3 and max(info["run_rank"]) == info["max_rank"] >= 2 and sum(r >= 2 for r in info["run_rank"]) >= 3
    zs = [[b for b, l in s[2].items() if l == "Z"] for s in steps]         # the sign: index bits inside the tile AND far above it
    assert all(max(b for b, l in s[2].items() if l in "XY") >= 22 for s in steps) and all(min(z) < n // 3 and max(z) >= n - n // 3 for z in zs)
    assert {b for z in zs for b in z} == set(range(n))
    assert E.bound(ops) < 1 << 24 and E.scale2(ops) * mean_norm2 * 2 ** n < 1 << 53
    for name, (g, _) in E.whole_gate_cases(n).items():
        assert E.bound(E.gate_ops(g)) < 1 << 24 and E.leaves(E.gate_ops(g)) <= 8, name
    assert E.bound(E.step_ops(E.whole_steps(n))) < 1 << 24
    terms = E.sum_terms(n)
    pinfo = A.pauli_apply_info(shape, strides, [(c, E.api_string(n, l)) for c, l in terms], dtype)
    assert len(terms) >= 6 and pinfo["n_groups"] >= 3 and len({x >> 22 for x in pinfo["group_xmask"]}) >= 3
    assert E.bound([E.PauliSum(terms)]) < 1 << 24
    batch = A.pauli_info(shape, strides, [E.api_string(n, l) for l in E.expectation_batch(n)], dtype)
    assert batch["n_groups"] == 1 and batch["n_launches"] == 2


@pytest.mark.parametrize("n, esz", [(30, 8), (29, 16), (32, 8)])
def test_sample_sets_hold_the_edges(n, esz):
    s = E.sample_indices(1 << n, esz, 1 << 18).numpy()
    assert s.size == 1 << 18 == np.unique(s).size and s.min() == 0 and s.max() == (1 << n) - 1
    have = set(s.tolist())
    edges = [(1 << 31) // esz, (1 << 32) // esz] + ([1 << 31] if n == 32 else [])
    assert all(e < 1 << n for e in edges)
    for lo, hi in [(0, 1024), ((1 << n) - 1024, 1 << n)] + [(e - 2048, e + 2048) for e in edges]:
        assert have.issuperset(range(lo, hi))
    assert len(have - set(range(1024))) > (1 << 18) - 16384                # the rest is spread over the array
    assert np.unique(s >> (n - 8)).size == 256


# ---- 4. Pauli steps, sums and expectation values ------------------------------------------------------------------------------
def random_steps(rng, nq, count):
    coeffs = [(1, 2j), (2 - 1j, 1 + 2j), (0, 1), (0, -1j), (1 + 1j, 1 - 1j), (-2, 0), (0, 1j)]
    return [coeffs[k % len(coeffs)] + (E.random_letters(rng, nq, rng.choice(nq, size=1 + k % 3, replace=False)),) for k in range(count)]


@pytest.mark.parametrize("nq", [10, 12])
def test_expected_step_values_against_the_axis_by_axis_oracle_and_the_dense_matrices(nq):
    rng = np.random.default_rng(50 + nq)
    a = hash_state(1 << nq)
    steps = random_steps(rng, nq, 9) + [(1, -1j, {b: "Y" for b in range(nq)}), (0, 1, {b: "Z" for b in range(nq)})]
    psi, vec = a.reshape((2,) * nq), a.copy()
    for alpha, beta, letters in steps:
        psi = alpha * psi + beta * oracle_apply(psi, E.api_string(nq, letters))
        if nq == 10:
            vec = alpha * vec + beta * (string_matrix(E.api_string(nq, letters), nq) @ vec)
    assert nq != 10 or np.array_equal(vec, psi.reshape(-1))
    ops = E.step_ops(steps)
    rep = E.compare_all(as_store(psi, torch.complex128), ops, chunk=1 << 16)
    E.assert_exact(rep, ops, torch.complex128, f"{nq} qubits, {len(steps)} steps")
    assert np.abs(psi.real).max() <= E.bound(ops)


def test_expected_sums_and_expectation_values_against_the_dense_matrices():
    nq = 10
    rng = np.random.default_rng(7)
    a = hash_state(1 << nq)
    terms = E.sum_terms(nq)
    h = sum(c * string_matrix(E.api_string(nq, l), nq) for c, l in terms)
    op = E.PauliSum(terms)
    E.assert_exact(E.compare_all(as_store(h @ a), [op], chunk=1 << 12), [op], torch.complex64, "sum of 7 strings")
    strings = [E.random_letters(rng, nq, rng.choice(nq, size=k % 4, replace=False)) for k in range(8)] + [{b: "Y" for b in range(nq)}, {}]
    sums, den = E.expectation_sums(1 << nq, strings, "cpu", chunk=SMALL)
    assert den == int(round(np.vdot(a, a).real))
    for (num, imag), letters in zip(sums, strings):
        want = np.vdot(a, string_matrix(E.api_string(nq, letters), nq) @ a)
        assert imag == 0 and num == int(round(want.real)) and abs(want.imag) < 1e-9, letters
    assert sums[-1][0] == den


# ---- 5. the comparator rejects plausible wrong answers ------------------------------------------------------------------------
def standin_gate(a, m, bits, error=None):
    """A kernel's view of one gate, in numpy on the flat array: row and column digits from the memory index.  error: what a
    subtly wrong kernel would do instead."""
    n, k = a.size, len(bits)
    nbits = n.bit_length() - 1
    m = np.asarray(m, dtype=np.complex128).reshape(2 ** k, 2 ** k)
    if error == "transposed matrix":
        m = m.T
    if error == "swapped targets":
        bits = bits[::-1]
    i = np.arange(n)
    r = sum(((i >> b) & 1) << (k - 1 - j) for j, b in enumerate(bits))
    base = i & ~sum(1 << b for b in bits)
    out = np.zeros(n, dtype=np.complex128)
    for c in range(2 ** k):
        partner = base | sum(((c >> (k - 1 - j)) & 1) << b for j, b in enumerate(bits))
        if error == "partner index narrowed":
            partner = partner & ((1 << (nbits - 1)) - 1)                   # bit 31 of a 2^32 array, at small scale: the top bit
        out += m[r, c] * a[partner]
    if error == "one tile left unwritten":
        tile = slice(n // 2 + 1024, n // 2 + 2048)
        out[tile] = a[tile]
    return out


def standin_string(a, letters, error=None):
    n = a.size
    nbits = n.bit_length() - 1
    i = np.arange(n)
    xm = sum(1 << b for b, l in letters.items() if l in "XY")
    sm = sum(1 << b for b, l in letters.items() if l in "YZ")
    ny = sum(l == "Y" for l in letters.values())
    signed = i & sm
    if error == "sign from the low index bits":
        signed = signed & ((1 << (nbits // 2)) - 1)                        # the low 32 bits of a 64-bit index, at small scale
    parity = np.array([bin(int(v)).count("1") & 1 for v in signed])
    return (-1j) ** ny * (1 - 2 * parity) * a[i ^ xm]


GATE_ERRORS = ["transposed matrix", "swapped targets", "partner index narrowed", "one tile left unwritten"]


@pytest.mark.parametrize("error", [None] + GATE_ERRORS)
def test_the_comparator_rejects_a_wrong_gate(error):
    nq = 13
    a = hash_state(1 << nq)
    sample = E.sample_indices(1 << nq, 8, 1 << 10)
    for gates in ([(E.G2, (nq - 1, nq - 2))], [(E.G2, (3, nq - 1)), (E.G1, (nq - 1,))], [(E.G1, (nq - 1,))], [(E.D10A, (nq - 1, 0))]):
        if error == "swapped targets" and len(gates[0][1]) == 1:
            continue
        got = a
        for g, (m, bits) in enumerate(gates):
            got = standin_gate(got, m, bits, error if g == 0 else None)
        assert np.array_equal(got, oracle_gates(a, nq, gates)) == (error is None)
        ops = E.gate_ops(gates)
        rep = E.compare_all(as_store(got), ops, chunk=1 << 12)
        part = E.compare_sample(as_store(got), ops, sample.clone(), chunk=1 << 11)
        print(f"{error}: {[b for _, b in gates]}: {rep['bad']} of {rep['compared']} elements differ, {part['bad']} of the {part['compared']} sampled")
        if error is None:
            assert rep["bad"] == 0 and part["bad"] == 0 and rep["first_bad"] is None
            continue
        assert rep["bad"] > 0 and 0 <= rep["first_bad"] < 1 << nq
        assert rep["bad"] == int(np.count_nonzero(got != oracle_gates(a, nq, gates)))
        with pytest.raises(AssertionError):
            E.assert_exact(rep, ops, torch.complex64, str(error))
        if error != "one tile left unwritten":
            assert part["bad"] > 0
        elif E.scale2(ops) is not None:                                    # a tile the sample misses: the norm invariant sees it
            assert rep["bad"] <= 1024 and int(round((np.abs(got) ** 2).sum())) != E.scale2(ops) * E.hash_norm2(1 << nq, "cpu")


@pytest.mark.parametrize("error", [None, "sign from the low index bits"])
def test_the_comparator_rejects_a_wrong_sign(error):
    nq = 12
    a = hash_state(1 << nq)
    for letters in ({b: "Z" for b in range(nq)}, {nq - 1: "X", 2: "Y", 9: "Z", 0: "Z"}, E.random_letters(np.random.default_rng(3), nq, (nq - 1, 4))):
        got = standin_string(a, letters, error)
        assert np.array_equal(got, oracle_apply(a.reshape((2,) * nq), E.api_string(nq, letters)).reshape(-1)) == (error is None)
        rep = E.compare_all(as_store(got), [E.PauliStep(0, 1, letters)], chunk=SMALL)
        assert (rep["bad"] == 0) == (error is None), letters
        if error:
            assert rep["bad"] >= 1 << (nq - 2)
        # the same error in an expectation value: the exact numerator moves
        (num, _), = E.expectation_sums(1 << nq, [letters], "cpu", chunk=SMALL)[0]
        assert (int(round(np.vdot(a, got).real)) == num) == (error is None)


def test_values_at_and_past_the_limit_are_refused():
    """assert_exact refuses a comparison whose integers float32 cannot hold; -0.0 equals 0; NaN is a mismatch."""
    ops = E.gate_ops([(E.G2, (3, 1))] * 7)
    assert E.bound(ops) >= 1 << 24
    with pytest.raises(AssertionError):
        E.assert_exact({"compared": 1, "bad": 0, "first_bad": None, "peak": 1}, ops, torch.complex64)
    E.assert_exact({"compared": 1, "bad": 0, "first_bad": None, "peak": 1}, ops, torch.complex128)
    store = E.fill(torch.zeros(2048, dtype=torch.complex64))
    zero = int((store.real == 0).nonzero()[0])
    store.real[zero] = -0.0
    assert E.compare_all(store, [])["bad"] == 0
    store.imag[7] = float("nan")
    assert E.compare_all(store, []) == {"compared": 2048, "bad": 1, "first_bad": 7, "peak": 8}


# ---- 6. the machinery of tests/test_wide_ops_large_gpu.py: gates on 3 to 5 bits, the salted state, exact sums, Projector -------
WIDE_POOL = {3: [E.W3, E.TOFFOLI, E.FREDKIN, E.CCZ, E.PAIR3, E.XZY], 4: [E.W4, np.kron(E.PAIR3, E.S), np.kron(E.CNOT, E.ISWAP)],
             5: [E.W5, np.kron(E.TOFFOLI, E.D4), np.kron(E.G1, np.kron(E.SWAP, E.CZ))[:, ::-1]]}


@pytest.mark.parametrize("nq", [10, 12])
def test_expected_wide_gate_values_against_numpy_gate(nq):
    """k = 3, 4, 5: dense matrices (8, 16, 32 partners) and sparse ones, the targets in arbitrary order."""
    rng = np.random.default_rng(300 + nq)
    a = hash_state(1 << nq)
    for k, pool in WIDE_POOL.items():
        for m in pool:
            bits = tuple(int(b) for b in rng.permutation(nq)[:k])
            gates = [(m, bits), (E.G1, (bits[1],)), (E.PAIR3, (bits[2], nq - 1 if nq - 1 not in bits[:3] else bits[0], bits[1]))][:2 + (k == 3)]
            gates = [g for g in gates if len(set(g[1])) == len(g[1])]
            ops = E.gate_ops(gates)
            assert ops[0].T == max(np.count_nonzero(m, axis=1)) <= 2 ** k
            want = oracle_gates(a, nq, gates)
            rep = E.compare_all(as_store(want, torch.complex128), ops, chunk=1 << 14)
            E.assert_exact(rep, ops, torch.complex128, f"{nq} qubits, k = {k}, bits {bits}")
            assert rep["peak"] == int(max(np.abs(want.real).max(), np.abs(want.imag).max())) <= E.bound(ops)
    assert any(np.count_nonzero(p[0]) == 4 ** k for k, p in WIDE_POOL.items()) and [E.Gate(E.WIDE[k], range(k)).T for k in (3, 4, 5)] == [8, 16, 32]
    for k, s2, growth in ((3, 20, 12), (4, 40, 24), (5, 80, 48)):
        g = E.Gate(E.WIDE[k], range(k))
        assert (g.scale2, g.growth) == (s2, growth) and np.abs(E.WIDE[k]).max() == 2
    pair = E.Gate(E.PAIR3, (2, 1, 0))
    assert pair.T == 2 and pair.growth == 5 and (np.count_nonzero(E.PAIR3, axis=1) == 2).all() and not np.array_equal(E.PAIR3, E.PAIR3.T)


def salted_state(n_elems):
    f, g = E.hash_index(torch.arange(n_elems), salt=1)
    return f.numpy().astype(np.float64) + 1j * g.numpy().astype(np.float64)


def test_the_salted_state_is_a_second_hash_state():
    rng = np.random.default_rng(2)
    idx = np.concatenate([np.arange(64), rng.integers(0, 1 << 34, 400), [(1 << 34) - 1, 1 << 32, 1 << 31, 1 << 33]]).astype(np.int64)
    f, g = E.hash_index(torch.from_numpy(idx), salt=1)
    assert [(int(x), int(y)) for x, y in zip(f, g)] == [E.hash_python(int(i), salt=1) for i in idx] == [E.hash_python(int(i) ^ E.SALT) for i in idx]
    f0, g0 = E.hash_index(torch.from_numpy(idx))
    assert [(int(x), int(y)) for x, y in zip(f0, g0)] == [E.hash_python(int(i)) for i in idx]
    assert float(((f != f0) | (g != g0)).double().mean()) > 0.9
    third = [range(0, 11), range(11, 23), range(23, 34)]
    assert E.SALT >> 33 == 1 and all(any(E.SALT >> b & 1 for b in r) for r in third)
    store = E.fill(torch.zeros(5000, dtype=torch.complex64), chunk=SMALL, salt=1)
    assert np.array_equal(store.numpy().astype(np.complex128), salted_state(5000))
    assert E.compare_all(store, [], chunk=SMALL, salt=1)["bad"] == 0 and E.compare_all(store, [], chunk=SMALL)["bad"] > 4000
    assert E.hash_norm2(5000, "cpu", chunk=SMALL, salt=1) == int(round((np.abs(salted_state(5000)) ** 2).sum()))
    nq = 10
    gates = [(E.G2, (9, 2)), (E.TOFFOLI, (0, 9, 4))]
    want = oracle_gates(salted_state(1 << nq), nq, gates)
    assert E.compare_all(as_store(want), E.gate_ops(gates), chunk=SMALL, salt=1)["bad"] == 0


def test_inner_sums_against_numpy():
    nq = 13                                                                  # (whole_steps flips bit 12)
    a, b = salted_state(1 << nq), hash_state(1 << nq)
    gates, measure = E.pair_gates(nq)
    for k in range(len(gates) + 1):
        ops = E.gate_ops(gates[:k])
        A_k, B_k = oracle_gates(a, nq, gates[:k]), oracle_gates(b, nq, gates[:k])
        want = np.vdot(A_k, B_k)
        assert E.inner_sums(1 << nq, ops, 1, ops, 0, chunk=SMALL) == (int(round(want.real)), int(round(want.imag)))
        if k < len(gates) and measure[k] is not None:
            want = np.vdot(A_k, oracle_gates(B_k, nq, [(measure[k], gates[k][1])]))
            got = E.inner_sums(1 << nq, ops, 1, ops, 0, M=E.Gate(measure[k], gates[k][1]), chunk=SMALL)
            assert got == (int(round(want.real)), int(round(want.imag))) and got[1] != 0
    steps = E.whole_steps(nq)
    psi_a, psi_b = a.reshape((2,) * nq), b.reshape((2,) * nq)
    for k, (alpha, beta, letters) in enumerate(steps):
        want = np.vdot(psi_a, oracle_apply(psi_b, E.api_string(nq, letters)))
        ops = E.step_ops(steps[:k])
        assert E.inner_sums(1 << nq, ops, 1, ops, 0, M=E.PauliStep(0, 1, letters), chunk=SMALL) == (int(round(want.real)), int(round(want.imag)))
        psi_a, psi_b = (alpha * p + beta * oracle_apply(p, E.api_string(nq, letters)) for p in (psi_a, psi_b))
    assert E.inner_sums(1 << nq, [], 0, [], 0) == (E.hash_norm2(1 << nq, "cpu"), 0)
    with pytest.raises(AssertionError):                                      # partial sums float64 cannot hold are refused
        E.inner_sums(1 << 10, [E.PauliSum([(1 << 20, {0: "X"})])], 0, [E.PauliSum([(1 << 20, {3: "Z"})])], 1)


def test_marginal_and_rdm_sums_against_numpy():
    nq = 12
    a = hash_state(1 << nq)
    for bits in ((11, 5, 0), (0, 11), (11, 10, 7, 4, 1, 0), (3,), (11, 10, 6, 5, 4, 3, 2, 0, 1, 8)):
        k = len(bits)
        rest = [d for d in range(nq) if d not in E.dims_of(nq, bits)]
        m = a.reshape((2,) * nq).transpose(list(E.dims_of(nq, bits)) + rest).reshape(2 ** k, -1)   # rows: the first bit the most significant
        want = (np.abs(m) ** 2).sum(axis=1)
        assert E.marginal_sums(1 << nq, bits, chunk=SMALL) == [int(round(v)) for v in want]
        if k <= 6:
            rho = m @ m.conj().T
            re, im = E.rdm_sums(1 << nq, bits, chunk=SMALL)
            assert np.array_equal(np.array(re) + 1j * np.array(im), rho)
            assert [re[c][c] for c in range(2 ** k)] == E.marginal_sums(1 << nq, bits) and all(im[c][c] == 0 for c in range(2 ** k))
    assert sum(E.marginal_sums(1 << nq, (4, 9))) == E.hash_norm2(1 << nq, "cpu")


def test_projector_against_numpy():
    nq = 10
    a = hash_state(1 << nq)
    i = np.arange(1 << nq)
    for bits, outcome in (((9, 2), 1), ((2, 9), 1), ((0,), 0), ((9, 8, 0), 5)):
        k = len(bits)
        digit = sum(((i >> b) & 1) << (k - 1 - j) for j, b in enumerate(bits))
        ops = E.gate_ops([(E.G1, (bits[0],))]) + [E.Projector(bits, outcome)]
        want = np.where(digit == outcome, oracle_gates(a, nq, [(E.G1, (bits[0],))]), 0)
        assert E.compare_all(as_store(want), ops, chunk=SMALL)["bad"] == 0
        assert E.compare_all(as_store(oracle_gates(a, nq, [(E.G1, (bits[0],))])), ops, chunk=SMALL)["bad"] > 100
    assert E.scale2([E.Projector((1,), 0)]) is None and E.bound([E.Projector((1,), 0)]) == 8


@pytest.mark.parametrize("n, dtype", [(30, torch.complex64), (29, torch.complex128), (32, torch.complex64)])
def test_the_wide_circuits_meet_their_conditions(n, dtype):
    shape, strides = (2,) * n, tuple(1 << (n - 1 - d) for d in range(n))
    mean_norm2, limit = 43, E.LIMIT[dtype]
    tb = 12 if dtype == torch.complex64 else 11
    for name, gates in E.wide_whole_cases(n).items():
        ops = E.gate_ops(gates)
        assert E.bound(ops) < 1 << 24 and E.leaves(ops) == (4 if name == "pair3" else 1), name
        for m, bits in gates:
            info = A.wide_gate_info(shape, strides, m, E.dims_of(n, bits), dtype)
            assert info["target_bits"] == bits and info["tb"] == tb and info["n_tiles"] == 1 << (n - tb) and n - 1 in bits
    for (k, where), bits in E.wide_sampled_cases(n).items():
        ops = E.gate_ops([(E.WIDE[k], bits)])
        assert E.leaves(ops) == 2 ** k and E.bound(ops) == 8 * 3 * 2 ** (k - 1) < 1 << 24 and E.scale2(ops) == 5 * 2 ** (k - 1)
        assert E.scale2(ops) * mean_norm2 * 2 ** n < 1 << 53
        info = A.wide_gate_info(shape, strides, E.WIDE[k], E.dims_of(n, bits), dtype)
        assert info["target_bits"] == bits and not info["diagonal"]
        assert {"above": all(b >= 12 for b in bits), "inside": all(b < 11 for b in bits),
                "mixed": {n - 1, n - 2} < set(bits) and min(bits) < 11}[where]
    parts = E.wide_fused_parts(n)
    ops = E.gate_ops(E.wide_fused_gates(n))
    assert len(parts) == 8 and [isinstance(p, list) for p in parts] == [True, False] * 4 and all(len(p) in (2, 3) for p in parts[::2])
    assert [len(p[1]) for p in parts[1::2]] == [3, 4, 5, 3]
    assert E.leaves(ops) == 2 ** 12 and sum(op.T > 1 for op in ops) == 3                      # W3, W4, W5: 8 * 16 * 32
    assert E.bound(ops) == 8 * 12 * 24 * 48 < 1 << 24 and E.scale2(ops) == 64000 and (n == 32 or 64000 * mean_norm2 * 2 ** n < 1 << 53)   # (run at the 8 GiB sizes)
    assert all(A.gate_circuit_info(shape, strides, E.api_gates(n, p), dtype)["n_runs"] >= 1 for p in parts[::2])
    for m in E.CHANNEL_UNITARIES:
        g = E.Gate(m, (n - 1, 6, n - 2))
        assert g.T == 1 and g.scale2 == 1
    ch = A.Channel.mixture(E.CHANNEL_PROBS, E.CHANNEL_UNITARIES)
    assert ch.form == "FIXED" and A.channel_info(shape, strides, ch, E.dims_of(n, (n - 1, 6, n - 2)), dtype)["target_bits"] == (n - 1, 6, n - 2)
    proj = A.Channel.from_kraus([np.diag(np.eye(4)[d]) for d in range(4)])
    info = A.channel_info(shape, strides, proj, E.dims_of(n, (n - 1, 2)), dtype)
    assert proj.form == "DIAGONAL" and info["reduction"] == "marginal" and info["target_bits"] == (n - 1, 2)
    if n == 32:
        return                                                                                # the two-state and Krylov cases: 8 GiB sizes only
    gates, measure = E.pair_gates(n)
    ops = E.gate_ops(gates)
    growth_m = max(E.Gate(m, g[1]).growth for m, g in zip(measure, gates) if m is not None)
    assert E.bound(ops) < 1 << 24 and E.leaves(ops) == 8 and 2 * E.bound(ops) ** 2 * growth_m * 2 ** n < 1 << 53
    # (complex128: the two-state default max_rank is 1 and max_rank=0 cuts the same runs, so the fused plan is max_rank=2)
    fused = [r for r in E.pair_max_ranks(dtype) if r != 0][-1]
    assert E.pair_max_ranks(dtype)[:2] == [None, 0] and fused == (None if dtype == torch.complex64 else 2)
    infos = [A.gate_adjoint_info(shape, strides, E.api_gates(n, gates), dtype, measure, r) for r in (fused, 0)]
    assert infos[0]["n_runs"] != infos[1]["n_runs"] and infos[0]["run_rank"] != infos[1]["run_rank"] and infos[0]["n_measured"] == 2
    steps = E.whole_steps(n)
    infos = [A.pauli_adjoint_info(shape, strides, E.api_steps(n, steps), dtype, None, r) for r in (fused, 0)]
    assert infos[0]["n_runs"] != infos[1]["n_runs"] and infos[0]["run_rank"] != infos[1]["run_rank"] and infos[0]["n_measured"] == 2
    assert 2 * E.bound(E.step_ops(steps)) ** 2 * 2 ** n < 1 << 53
    assert A.krylov_info(shape, strides, A.krylov.BATCH + 1, dtype)["dots_launches"] >= 2
    assert (2 + 1 + 1 + 1) * 8 < limit                                                        # krylov_combine_: |2 - i| + |i| + |-1| times 8
    for bits in ((n - 1, 0), (n - 1, n - 2, 20, 11, 1, 0)):
        info = A.rdm_info(shape, strides, E.dims_of(n, bits), dtype)
        assert info["kernel"] == A._native.RDM_STREAM and info["dim"] == 2 ** len(bits)


def standin_wide(a, m, bits, error=None):
    """A tile kernel's view of one wide gate in numpy: the tile holds the targets and the lowest other bits; every tile is read,
    multiplied and written back.  error: what a subtly wrong kernel or host packer would do instead."""
    n, k = a.size, len(bits)
    nbits = n.bit_length() - 1
    m = np.asarray(m, dtype=np.complex128).reshape(2 ** k, 2 ** k)
    if error == "transposed matrix":
        m = m.T
    if error == "reversed target order":
        bits = bits[::-1]
    if error == "one target bit off by one":
        bits = bits[:-1] + (bits[-1] + 1 if bits[-1] + 1 not in bits and bits[-1] + 1 < nbits else bits[-1] - 1,)
    i = np.arange(n)
    r = sum(((i >> b) & 1) << (k - 1 - j) for j, b in enumerate(bits))
    base = i & ~sum(1 << b for b in bits)
    out = np.zeros(n, dtype=np.complex128)
    for c in range(2 ** k):
        src = base | sum(((c >> (k - 1 - j)) & 1) << b for j, b in enumerate(bits))
        if error == "byte offset narrowed to 32 bits":
            src = src & ((1 << (nbits - 1)) - 1)                            # 2^32 bytes of a 2^33-byte array, at small scale
        out += m[r, c] * a[src]
    if error == "one tile skipped":
        tile_bits = sorted(set(bits) | set([b for b in range(nbits) if b not in bits][:8 - k]))
        skipped = sum(1 << b for b in range(nbits) if b not in tile_bits and b != 9)   # the tile whose other bits are all 1 but one
        sel = (i & ~sum(1 << b for b in tile_bits)) == skipped
        out[sel] = a[sel]
    return out


WIDE_ERRORS = ["transposed matrix", "reversed target order", "one target bit off by one", "byte offset narrowed to 32 bits",
               "one tile skipped"]


@pytest.mark.parametrize("error", [None] + WIDE_ERRORS)
def test_the_comparator_rejects_a_wrong_wide_gate(error):
    nq = 13
    a = hash_state(1 << nq)
    sample = E.sample_indices(1 << nq, 8, 1 << 12)                        # the two edge tiles and as many random indices
    t, u = nq - 1, nq - 2
    cases = [[(E.TOFFOLI, (t, 3, u))], [(E.FREDKIN, (5, t, 11))], [(E.PAIR3, (t, 10, 1)), (E.PAIR3, (1, 10, t))], [(E.W3, (t, 6, u))],
             [(E.W4, (u, 2, t, 10))], [(E.W5, (8, t, 10, 0, u))]]
    for gates in cases:
        if error == "transposed matrix" and np.array_equal(gates[0][0], gates[0][0].T):
            continue                                                       # (Toffoli and Fredkin are symmetric)
        got = a
        for g, (m, bits) in enumerate(gates):
            got = standin_wide(got, m, bits, error if g == 0 else None)
        assert np.array_equal(got, oracle_gates(a, nq, gates)) == (error is None)
        ops = E.gate_ops(gates)
        rep = E.compare_all(as_store(got), ops, chunk=1 << 12)
        part = E.compare_sample(as_store(got), ops, sample.clone(), chunk=1 << 11)
        print(f"{error}: {[b for _, b in gates]}: {rep['bad']} of {rep['compared']} elements differ, {part['bad']} of the {part['compared']} sampled")
        if error is None:
            assert rep["bad"] == 0 and part["bad"] == 0 and rep["first_bad"] is None
            continue
        assert rep["bad"] > 0 and rep["bad"] == int(np.count_nonzero(got != oracle_gates(a, nq, gates)))
        with pytest.raises(AssertionError):
            E.assert_exact(rep, ops, torch.complex64, str(error))
        if error != "one tile skipped":
            assert part["bad"] > 0
        elif E.scale2(ops) not in (None, 1):                               # the sampled cases (dense gates): a tile the sample may miss changes the norm
            assert rep["bad"] <= 256 and int(round((np.abs(got) ** 2).sum())) != E.scale2(ops) * E.hash_norm2(1 << nq, "cpu")
