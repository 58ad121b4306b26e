"""The state-streaming kernels (gates: apply_gates_; Pauli circuits: pauli_evolve_, pauli_apply_; y = H a: pauli_sum_apply;
pauli_expectation) on states past 4 GiB, checked EXACTLY: 2^30 complex64 and 2^29 complex128 (8 GiB: byte offsets cross 2^32,
and a complex128 launch has more blocks than the 2048-workgroup grid cap) and, for the in-place families, 2^32 complex64
(32 GiB: element indices cross 2^31).  2^33 elements, where an unsigned 32-bit element index would wrap, are deliberately
left out: 64 GiB on a shared card.

tests/exact_state.py holds the method: the state is an integer hash of the memory index, every expected value is an integer
computed on the device from the index alone, chunk by chunk, and while every component stays below 2^24 (complex64) or 2^53
(complex128) the kernels' arithmetic -- float64 products and sums, one rounding per component -- reproduces it exactly, so
results are compared with ==.  tests/test_state_ops_large_cpu.py checks that method against the numpy oracles of the small
suites and shows that it rejects a narrowed index, a transposed matrix, swapped targets, a skipped tile and a sign taken from
the low index bits.

Short circuits are compared on every element.  The fused 30-step circuits cost 4^5 (gates) or 2^7 (Pauli steps) hash
evaluations per element, so they are compared on 2^18 sampled indices -- the first and the last tile, 2048 elements on either
side of byte offsets 2^31 and 2^32 and of element index 2^31, the rest pseudo-random -- plus one whole-array invariant: every
step of those circuits is a Gaussian-integer multiple of a unitary, so sum |expected|^2 over the whole array IS the integer
scale2 * sum |hash|^2 (test_scale2_is_the_growth_of_the_norm evaluates both sides), it stays below 2^53, and A.norm2 of the
result has to equal it; a block skipped or written twice anywhere changes it.

Every test skips, with the figures, when the device has less free memory than the state plus 4 GiB, and asserts that its
peak stays within that."""
import numpy as np
import pytest
import torch

import artensor_amd as A
import exact_state as E
from exact_state import Budget, norm_invariant

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GIB = 1 << 30
SIZES = {"c64-n30": (torch.complex64, 30), "c128-n29": (torch.complex128, 29), "c64-n32": (torch.complex64, 32)}
IN_PLACE = list(SIZES)
OUT_OF_PLACE = ["c64-n30", "c128-n29"]                                   # y = H a needs a second array: the 8 GiB sizes
SAMPLE = 1 << 18


# ---- gates --------------------------------------------------------------------------------------------------------------------
CASES = list(E.whole_gate_cases(30))
# the 32 GiB state takes four of the cases (bits 31 and 30 are the pair around element index 2^31), the 8 GiB sizes all seven
SUBSET_32 = ["top2", "top2-rev-r0", "top-piece", "reg-top-r0"]
WHOLE = [(size, case) for size in IN_PLACE for case in (SUBSET_32 if size == "c64-n32" else CASES)]


@pytest.mark.parametrize("size, case", WHOLE)
def test_gates_whole_array(size, case):
    b = Budget(size)
    gates, max_rank = E.whole_gate_cases(b.n)[case]
    ops = E.gate_ops(gates)
    assert E.bound(ops) < E.LIMIT[b.dtype]
    t = b.view()
    info = A.gate_circuit_info(t.shape, t.stride(), E.api_gates(b.n, gates), b.dtype, max_rank)
    assert info["bits"] == [bits for _, bits in gates]
    assert A.apply_gates_(t, E.api_gates(b.n, gates), max_rank=max_rank) is t
    label = f"gates {size} {case} (bits {info['bits']}, max_rank {max_rank}: runs of rank {info['run_rank']})"
    E.assert_exact(E.compare_all(b.store, ops), ops, b.dtype, label)
    b.close(label)


@pytest.mark.parametrize("size", IN_PLACE)
def test_gates_on_a_view_with_the_top_three_dims_permuted(size):
    b = Budget(size)
    t = b.view().permute([2, 0, 1] + list(range(3, b.n)))
    assert not t.is_contiguous() and t.data_ptr() == b.store.data_ptr()
    api = [(E.G2, (0, 2)), (E.G1, (1,))]
    gates = [(m, tuple(int(t.stride(d)).bit_length() - 1 for d in dims)) for m, dims in api]
    assert [bits for _, bits in gates] == [(b.n - 3, b.n - 2), (b.n - 1,)]
    ops = E.gate_ops(gates)
    assert A.gate_circuit_info(t.shape, t.stride(), api, b.dtype)["bits"] == [bits for _, bits in gates]
    assert A.apply_gates_(t, api) is t
    label = f"gates {size} on a permuted view"
    E.assert_exact(E.compare_all(b.store, ops), ops, b.dtype, label)
    b.close(label)


@pytest.mark.parametrize("size", IN_PLACE)
def test_gates_fused_circuit(size):
    b = Budget(size)
    gates = E.fused_gates(b.n)
    ops = E.gate_ops(gates)
    t = b.view()
    info = A.gate_circuit_info(t.shape, t.stride(), E.api_gates(b.n, gates), b.dtype)
    assert info["n_runs"] >= 3 and max(info["run_rank"]) >= 2 and E.leaves(ops) == 4 ** 5 and E.bound(ops) < E.LIMIT[b.dtype]
    A.apply_gates_(t, E.api_gates(b.n, gates))
    label = f"gates {size} fused: 30 gates, n_runs {info['n_runs']}, run_rank {info['run_rank']}"
    sample = E.sample_indices(1 << b.n, b.store.element_size(), SAMPLE).to(DEV)
    E.assert_exact(E.compare_sample(b.store, ops, sample), ops, b.dtype, label)
    norm_invariant(b, ops, label)
    b.close(label)


# ---- in-place Pauli circuits --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_rank", [None, 0])
@pytest.mark.parametrize("size", IN_PLACE)
def test_pauli_evolve_whole_array(size, max_rank):
    b = Budget(size)
    steps = E.whole_steps(b.n)
    ops = E.step_ops(steps)
    assert E.bound(ops) < E.LIMIT[b.dtype]
    t = b.view()
    info = A.pauli_evolve_info(t.shape, t.stride(), E.api_steps(b.n, steps), b.dtype, max_rank)
    assert all(x >> (b.n - 1) for x in info["xmask"])                       # both steps flip the topmost bit
    assert A.pauli_evolve_(t, E.api_steps(b.n, steps), max_rank=max_rank) is t
    label = f"pauli_evolve_ {size} two steps, max_rank {max_rank}: runs of rank {info['run_rank']}"
    E.assert_exact(E.compare_all(b.store, ops), ops, b.dtype, label)
    b.close(label)


@pytest.mark.parametrize("size", IN_PLACE)
def test_pauli_evolve_fused_circuit(size):
    b = Budget(size)
    steps = E.fused_steps(b.n)
    ops = E.step_ops(steps)
    t = b.view()
    info = A.pauli_evolve_info(t.shape, t.stride(), E.api_steps(b.n, steps), b.dtype)
    assert info["n_runs"] >= 3 and max(info["run_rank"]) >= 2 and E.leaves(ops) == 2 ** 7 and E.bound(ops) < E.LIMIT[b.dtype]
    A.pauli_evolve_(t, E.api_steps(b.n, steps))
    label = f"pauli_evolve_ {size} fused: 30 steps, n_runs {info['n_runs']}, run_rank {info['run_rank']}"
    sample = E.sample_indices(1 << b.n, b.store.element_size(), SAMPLE).to(DEV)
    E.assert_exact(E.compare_sample(b.store, ops, sample), ops, b.dtype, label)
    norm_invariant(b, ops, label)
    b.close(label)


@pytest.mark.parametrize("size", IN_PLACE)
def test_pauli_apply_twice_gives_back_the_state(size):
    b = Budget(size)
    letters = E.random_letters(np.random.default_rng(6000 + b.n), b.n, (b.n - 1, b.n - 2, 23, 6, 1))
    string = E.api_string(b.n, letters)
    t = b.view()
    assert A.pauli_apply_(t, string) is t
    ops = [E.PauliStep(0, 1, letters)]
    label = f"pauli_apply_ {size}"
    E.assert_exact(E.compare_all(b.store, ops), ops, b.dtype, label + ", once")
    A.pauli_apply_(t, string)
    E.assert_exact(E.compare_all(b.store, []), [], b.dtype, label + ", twice")
    b.close(label)


# ---- y = H a ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", OUT_OF_PLACE)
def test_pauli_sum_apply(size):
    b = Budget(size, arrays=2)
    terms = E.sum_terms(b.n)
    op = E.PauliSum(terms)
    t = b.view()
    api = [(c, E.api_string(b.n, letters)) for c, letters in terms]
    info = A.pauli_apply_info(t.shape, t.stride(), api, b.dtype)
    assert len(terms) >= 6 and info["n_groups"] >= 3 and len({x >> 22 for x in info["group_xmask"]}) >= 3 and info["n_launches"] == 1
    y = A.pauli_sum_apply(t, api)
    assert y.shape == t.shape and y.stride() == t.stride() and y.data_ptr() != t.data_ptr()
    label = f"pauli_sum_apply {size}: {len(terms)} terms in {info['n_groups']} groups"
    E.assert_exact(E.compare_all(y.reshape(-1), [op]), [op], b.dtype, label)
    E.assert_exact(E.compare_all(b.store, []), [], b.dtype, label + ", amps unchanged")
    del y
    b.close(label)


# ---- expectation values -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["classes", "batch17"])
@pytest.mark.parametrize("size", OUT_OF_PLACE)
def test_pauli_expectation(size, which):
    b = Budget(size)
    strings = E.expectation_strings(b.n) if which == "classes" else E.expectation_batch(b.n)
    api = [E.api_string(b.n, s) for s in strings]
    t = b.view()
    info = A.pauli_info(t.shape, t.stride(), api, b.dtype)
    if which == "classes":
        assert info["xmask"][:3] == [0, 1 << (b.n - 1), (1 << 3) | (1 << 7)] and info["xmask"][3] >> (b.n - 1) == 1
        assert info["zmask"][0] == (1 << b.n) - (1 << 22) and info["zmask"][2] >> (b.n - 1) == 1 and len(strings[3]) == b.n
    else:
        assert len(strings) == 17 and info["n_groups"] == 1 and info["n_launches"] == 2
    sums, den = E.expectation_sums(1 << b.n, strings, DEV)
    assert den < 1 << 53 and all(abs(num) < 1 << 53 and imag == 0 for num, imag in sums)
    got = A.pauli_expectation(t, api)
    raw = A.pauli_expectation(t, api, normalize=False)
    norm = A.norm2(b.store)
    for k, (num, _) in enumerate(sums):
        want = float(num) / float(den)
        print(f"pauli_expectation {size} {which} string {k}: numerator {num} (raw {raw[k]!r}), sum |a|^2 {den}, value {got[k]!r}, want {want!r}")
        assert raw[k] == float(num), k                                      # exact integers, whatever the summation order
        assert abs(got[k] - want) <= 2.0 ** -52 * abs(want), k              # one rounding of the division
    assert norm == float(den)
    b.close(f"pauli_expectation {size} {which}")
