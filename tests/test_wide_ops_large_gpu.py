"""The families that test_state_ops_large_gpu.py leaves out, on states past 4 GiB, checked EXACTLY with the method of
tests/exact_state.py (an integer hash of the memory index as the state, integer predictions from the index alone, ==):

    wide gates      apply_wide_gate_, WideGate, FusedCircuit (artn_k_wgate, k = 3..5)
    channels        channel_ in the FIXED and the DIAGONAL form (artn_channel_choose, artn_k_channel, the marginal pass)
    two-state runs  apply_gates_pair_, pauli_evolve_pair_ (artn_k_gates_adjoint, artn_k_pauli_adjoint) and their t_k
    Krylov passes   krylov_dots with a second pass over w, krylov_combine_ with y among the vectors
    Born and RDM    overlap of two arrays, marginal_probabilities, reduced_density_matrix, sample

Sizes: 2^30 complex64 and 2^29 complex128 (8 GiB per array: byte offsets cross 2^32) everywhere; 2^32 complex64 (32 GiB: element
indices cross 2^31) for a few one-array in-place cases of the wide gates and the FIXED channel.  At most three arrays per test.

Whole array (compare_all): the permutation-like wide gates (Toffoli, Fredkin, CCZ), the two-non-zeros-per-row gate in both target
orders, the wide gate on a permuted view, every channel draw, both states of the two-state runs, all three vectors of
krylov_combine_.  Sampled (compare_sample on exactly sample_indices(n, esz, 2^18), always with the whole-array norm invariant):
one dense gate (8, 16, 32 partners per element) of k = 3, 4, 5 with targets above, inside and across the tile, and the mixed
FusedCircuit (2^12 hash evaluations per element).  The sums (t_k, dots, norms, marginals, density matrices, the cumulative sums
behind sample) are integers below 2^53 accumulated in float64, so they equal the chunked int64 sums of exact_state.py whatever
the summation order.

tests/test_state_ops_large_cpu.py checks this machinery at 10 to 14 qubits against numpy and shows that it rejects five planted
wide-gate errors.  Every test skips, with the figures, when the device has less free memory than its arrays plus 4 GiB, and
asserts that its peak stays within that."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import artensor_amd as A
import exact_state as E
import measure_oracle as MO
from exact_state import DEV, Budget, norm_invariant

pytestmark = pytest.mark.gpu

EIGHT = ["c64-n30", "c128-n29"]                                            # 8 GiB per array
BIG = "c64-n32"                                                            # 32 GiB: one-array in-place cases only
SAMPLE = 1 << 18
LAYOUTS = ["contiguous", "rotated"]


def layout_view(flat, n, layout):
    """The [2]*n view of a flat array; "rotated": the top three dims permuted, as in test_gates_on_a_view_with_the_top_three_dims_permuted."""
    t = flat.view((2,) * n)
    if layout == "rotated":
        t = t.permute([2, 0, 1] + list(range(3, n)))
        assert not t.is_contiguous() and t.data_ptr() == flat.data_ptr()
    return t


def second_array(b, salt=1):
    return E.fill(torch.empty_like(b.store), salt=salt)


# ---- wide gates ---------------------------------------------------------------------------------------------------------------
WHOLE = [(size, case) for size in EIGHT for case in E.wide_whole_cases(30)] + [(BIG, "toffoli"), (BIG, "pair3")]


@pytest.mark.parametrize("size, case", WHOLE)
def test_wide_gates_whole_array(size, case):
    b = Budget(size)
    gates = E.wide_whole_cases(b.n)[case]
    ops = E.gate_ops(gates)
    assert E.bound(ops) < E.LIMIT[b.dtype] and E.leaves(ops) <= 4
    t = b.view()
    for m, bits in gates:                                                   # one call per gate
        info = A.wide_gate_info(t.shape, t.stride(), m, E.dims_of(b.n, bits), b.dtype)
        assert info["target_bits"] == bits and info["n_tiles"] == (1 << b.n) >> info["tb"]
        assert A.apply_wide_gate_(t, m, E.dims_of(b.n, bits)) is t
    label = f"wide gate {size} {case} (bits {[bits for _, bits in gates]}, tile of 2^{info['tb']}, {info['n_tiles']} tiles)"
    E.assert_exact(E.compare_all(b.store, ops), ops, b.dtype, label)
    b.close(label)


SAMPLED = [(size, k, where) for size in EIGHT for k in (3, 4, 5) for where in ("above", "inside", "mixed")] + [(BIG, 4, "mixed")]


@pytest.mark.parametrize("size, k, where", SAMPLED)
def test_wide_gates_dense_sampled(size, k, where):
    """One dense gate, 2^k partners per element: 2^18 sampled indices and the norm, scale2 = 5 * 2^(k-1) times that of the hash."""
    b = Budget(size)
    bits = E.wide_sampled_cases(b.n)[(k, where)]
    ops = E.gate_ops([(E.WIDE[k], bits)])
    assert E.bound(ops) < E.LIMIT[b.dtype] and E.leaves(ops) == 2 ** k and E.scale2(ops) == 5 * 2 ** (k - 1)
    t = b.view()
    info = A.wide_gate_info(t.shape, t.stride(), E.WIDE[k], E.dims_of(b.n, bits), b.dtype)
    assert info["target_bits"] == bits
    if where == "inside":                                                   # the prebuilt object once, the one-call form otherwise
        assert A.WideGate(t.shape, t.stride(), b.dtype, E.WIDE[k], E.dims_of(b.n, bits), DEV)(t) is t
    else:
        assert A.apply_wide_gate_(t, E.WIDE[k], E.dims_of(b.n, bits)) is t
    label = f"dense wide gate {size} k={k} {where} (bits {bits}, tile bits {info['tile_bits']})"
    sample = E.sample_indices(1 << b.n, b.store.element_size(), SAMPLE).to(DEV)
    E.assert_exact(E.compare_sample(b.store, ops, sample), ops, b.dtype, label)
    norm_invariant(b, ops, label)
    b.close(label)


@pytest.mark.parametrize("size", EIGHT)
def test_fused_circuit_of_narrow_stretches_and_wide_gates(size):
    """Eight parts, four narrow stretches and four wide gates; W3, W4 and W5 are dense, every other gate a signed permutation:
    leaves = 8 * 16 * 32 = 2^12."""
    b = Budget(size)
    parts, gates = E.wide_fused_parts(b.n), E.wide_fused_gates(b.n)
    ops = E.gate_ops(gates)
    t = b.view()
    narrow = [A.gate_circuit_info(t.shape, t.stride(), E.api_gates(b.n, p), b.dtype)["n_runs"] for p in parts[::2]]
    wide = [A.wide_gate_info(t.shape, t.stride(), m, E.dims_of(b.n, bits), b.dtype) for m, bits in parts[1::2]]
    circ = A.FusedCircuit(t.shape, t.stride(), b.dtype, E.api_gates(b.n, gates), DEV)
    assert [w["target_bits"] for w in wide] == [bits for _, bits in parts[1::2]] and [w["k"] for w in wide] == [3, 4, 5, 3]
    assert circ.n_wide == len(wide) >= 2 and len(narrow) >= 2 and all(r >= 1 for r in narrow) and circ.n_launches == sum(narrow) + circ.n_wide
    assert E.leaves(ops) == 2 ** 12 and E.bound(ops) < E.LIMIT[b.dtype]
    assert circ(t) is t
    label = f"FusedCircuit {size}: {len(gates)} gates, {circ.n_wide} wide launches, narrow runs {narrow}"
    sample = E.sample_indices(1 << b.n, b.store.element_size(), SAMPLE).to(DEV)
    E.assert_exact(E.compare_sample(b.store, ops, sample), ops, b.dtype, label)
    norm_invariant(b, ops, label)
    b.close(label)


@pytest.mark.parametrize("size", EIGHT)
def test_wide_gate_on_a_view_with_the_top_three_dims_permuted(size):
    b = Budget(size)
    t = layout_view(b.store, b.n, "rotated")
    api = (0, 2, 5)
    bits = E.bits_of(t, api)
    assert bits == (b.n - 3, b.n - 2, b.n - 6)
    ops = E.gate_ops([(E.PAIR3, bits)])
    assert A.wide_gate_info(t.shape, t.stride(), E.PAIR3, api, b.dtype)["target_bits"] == bits
    assert A.apply_wide_gate_(t, E.PAIR3, api) is t
    label = f"wide gate {size} on a permuted view (API dims {api} = bits {bits})"
    E.assert_exact(E.compare_all(b.store, ops), ops, b.dtype, label)
    b.close(label)


# ---- channels -----------------------------------------------------------------------------------------------------------------
FIXED = [(size, j) for size in EIGHT for j in (0, 1, 2, 3)] + [(BIG, 2)]


@pytest.mark.parametrize("size, j", FIXED)
def test_channel_fixed_form(size, j):
    """A mixture of the identity, Toffoli, X (x) Z (x) Y and Fredkin on bits (n-1, 6, n-2); the uniform number lies in the middle
    of operator j's interval, so rounding cannot move the draw.  Operator 0, an exact identity, leaves the state untouched."""
    b = Budget(size)
    bits = (b.n - 1, 6, b.n - 2)
    ch = A.Channel.mixture(E.CHANNEL_PROBS, E.CHANNEL_UNITARIES)
    assert ch.form == "FIXED"
    t = b.view()
    got, p = A.channel_(t, ch, E.dims_of(b.n, bits), uniform=MO.mid_uniform(E.CHANNEL_PROBS, j))
    ops = E.gate_ops([(E.CHANNEL_UNITARIES[j], bits)]) if j else []
    label = f"channel FIXED {size} draw {j} (returned {got}, p {p!r})"
    assert got == j and abs(p - E.CHANNEL_PROBS[j]) <= 2.0 ** -50, label
    E.assert_exact(E.compare_all(b.store, ops), ops, b.dtype, label)
    b.close(label)


DIAGONAL = [("c64-n30", 2, False), ("c64-n30", 1, True), ("c128-n29", 3, False), ("c128-n29", 0, True)]


@pytest.mark.parametrize("size, j, device", DIAGONAL)
def test_channel_diagonal_form_projective(size, j, device):
    """{|d><d|} on bits (n-1, 2), renormalize=False: the weights are the four marginal integers, the draw follows the documented
    rule (the smallest j whose inclusive running sum exceeds uniform * total), the state is the projected hash state."""
    b = Budget(size)
    bits = (b.n - 1, 2)
    q = E.marginal_sums(1 << b.n, bits, DEV)
    total = sum(q)
    uniform = float(Fraction(2 * sum(q[:j]) + q[j], 2 * total))             # the middle of operator j's interval
    rule = next(c for c in range(4) if sum(q[:c + 1]) > Fraction(uniform) * total)
    assert rule == j and all(v > 0 for v in q)
    ch = A.Channel.from_kraus([np.diag(np.eye(4)[d]) for d in range(4)])
    assert ch.form == "DIAGONAL"
    t = b.view()
    got, p = A.channel_(t, ch, E.dims_of(b.n, bits), uniform=uniform, renormalize=False, device=device)
    if device:
        assert got.dim() == 0 and p.dim() == 0 and got.dtype == torch.int64 and p.dtype == torch.float64 and got.is_cuda and p.is_cuda
        got, p = int(got), float(p)
    want = float(q[j]) / float(total)
    label = f"channel DIAGONAL {size} draw {j} device={device} (weights {q}, returned {got}, p {p!r}, want {want!r})"
    assert got == j and abs(p - want) <= 2.0 ** -52 * want, label
    ops = [E.Projector(bits, j)]
    E.assert_exact(E.compare_all(b.store, ops), ops, b.dtype, label)
    b.close(label)


# ---- two-state kernels --------------------------------------------------------------------------------------------------------
PAIRS = [(size, r) for size in EIGHT for r in E.pair_max_ranks(E.SIZES[size][0])]


def check_pair(b, lam, ops, measured, tk, label):
    """Both states over the whole array, every measured t_k against the integers, every other entry 0."""
    E.assert_exact(E.compare_all(b.store, ops), ops, b.dtype, label + ", phi")
    E.assert_exact(E.compare_all(lam, ops, salt=1), ops, b.dtype, label + ", lam")
    for k, m in enumerate(measured):
        if m is None:
            assert tk[k] == 0, (label, k)
            continue
        want = E.inner_sums(1 << b.n, ops[:k], 1, ops[:k], 0, M=m, device=DEV)
        print(f"{label}: t_{k} = {tk[k]!r}, integers {want}")
        assert tk[k] == complex(*want), (label, k)


@pytest.mark.parametrize("size, max_rank", PAIRS)
def test_apply_gates_pair(size, max_rank):
    b = Budget(size, arrays=2)
    lam = second_array(b)
    gates, measure = E.pair_gates(b.n)
    ops, api = E.gate_ops(gates), E.api_gates(b.n, gates)
    t = b.view()
    fused = [r for r in E.pair_max_ranks(b.dtype) if r != 0][-1]
    cut, whole = (A.gate_adjoint_info(t.shape, t.stride(), api, b.dtype, measure, r) for r in (0, fused))
    assert cut["n_runs"] != whole["n_runs"] and cut["run_rank"] != whole["run_rank"]
    info = A.gate_adjoint_info(t.shape, t.stride(), api, b.dtype, measure, max_rank)
    tk = A.apply_gates_pair_(lam.view(t.shape), t, api, measure=measure, max_rank=max_rank)
    label = f"apply_gates_pair_ {size} max_rank {max_rank}: runs of rank {info['run_rank']}"
    check_pair(b, lam, ops, [None if m is None else E.Gate(m, g[1]) for m, g in zip(measure, gates)], tk, label)
    del lam
    b.close(label)


@pytest.mark.parametrize("size, max_rank", PAIRS)
def test_pauli_evolve_pair(size, max_rank):
    b = Budget(size, arrays=2)
    lam = second_array(b)
    steps = E.whole_steps(b.n)
    ops, api = E.step_ops(steps), E.api_steps(b.n, steps)
    t = b.view()
    fused = [r for r in E.pair_max_ranks(b.dtype) if r != 0][-1]
    cut, whole = (A.pauli_adjoint_info(t.shape, t.stride(), api, b.dtype, None, r) for r in (0, fused))
    assert cut["n_runs"] != whole["n_runs"] and cut["run_rank"] != whole["run_rank"]
    info = A.pauli_adjoint_info(t.shape, t.stride(), api, b.dtype, None, max_rank)
    tk = A.pauli_evolve_pair_(lam.view(t.shape), t, api, max_rank=max_rank)  # measure=None: both steps measured
    label = f"pauli_evolve_pair_ {size} max_rank {max_rank}: runs of rank {info['run_rank']}"
    check_pair(b, lam, ops, [E.PauliStep(0, 1, letters) for _, _, letters in steps], tk, label)
    del lam
    b.close(label)


# ---- Krylov passes ------------------------------------------------------------------------------------------------------------
def krylov_vectors(b):
    """V0 = the hash state (b.store), V1 = the salted one, w = the hash state after one signed-permutation pauli_apply_."""
    letters = E.random_letters(np.random.default_rng(7000 + b.n), b.n, (b.n - 1, b.n - 2, 21, 9, 0))
    v1, w = second_array(b), second_array(b, salt=0)
    A.pauli_apply_(w.view((2,) * b.n), E.api_string(b.n, letters))
    return v1, w, [E.PauliStep(0, 1, letters)]


@pytest.mark.parametrize("size", EIGHT)
def test_krylov_dots_with_a_second_pass(size):
    b = Budget(size, arrays=3)
    v1, w, ops_w = krylov_vectors(b)
    shape = (2,) * b.n
    m = A.krylov.BATCH + 1
    vectors = ([b.view(), v1.view(shape)] * m)[:m]                          # repeats: the vectors are only read
    assert A.krylov_info(shape, b.view().stride(), m, b.dtype)["dots_launches"] >= 2
    dots, nw = A.krylov_dots(vectors, w.view(shape))
    want = [E.inner_sums(1 << b.n, [], salt, ops_w, 0, device=DEV) for salt in (0, 1)]
    norm = E.hash_norm2(1 << b.n, DEV)
    label = f"krylov_dots {size}: {m} vectors"
    print(f"{label}: dots {dots[:2]!r}, integers {want}; |w|^2 {nw!r}, integer {norm}")
    assert all(dots[j] == complex(*want[j % 2]) for j in range(m)) and nw == float(norm), label
    for j in (0, 1):
        ov = A.overlap(vectors[j], w.view(shape))
        assert ov[0] == dots[j] and ov[2] == nw, (label, j)                 # bit for bit
    E.assert_exact(E.compare_all(w, ops_w), ops_w, b.dtype, label + ", w")
    del v1, w, vectors
    b.close(label)


def compare_combination(store, coeffs, sources, chunk=E.CHUNK):
    """Every element of `store` against sum_j coeffs[j] * (the state `ops_j` on the hash of `salt_j`), coeffs Gaussian integers;
    returns the report and the integer sum |expected|^2."""
    tally, norm = E.Tally(store.device), 0
    for lo in range(0, store.numel(), chunk):
        i = torch.arange(lo, min(lo + chunk, store.numel()), device=store.device)
        re, im = torch.zeros_like(i), torch.zeros_like(i)
        for c, (ops, salt) in zip(coeffs, sources):
            r, m = E.evaluate(ops, i, salt)
            cr, ci = int(c.real), int(c.imag)
            re += cr * r - ci * m
            im += cr * m + ci * r
        tally.add(store[lo:lo + i.numel()], re, im, i)
        norm += int((re * re).sum() + (im * im).sum())
    return tally.report(), norm


@pytest.mark.parametrize("size", EIGHT)
def test_krylov_combine_into_one_of_its_vectors(size):
    b = Budget(size, arrays=3)
    v1, w, ops_w = krylov_vectors(b)
    shape = (2,) * b.n
    coeffs = [2 - 1j, 1j, -1]
    got = A.krylov_combine_(b.view(), coeffs, [b.view(), v1.view(shape), w.view(shape)])
    report, norm = compare_combination(b.store, coeffs, [([], 0), ([], 1), (ops_w, 0)])
    label = f"krylov_combine_ {size}: y = V0 among three vectors"
    print(f"{label}: compared {report['compared']} elements, 3 hash evaluations each, largest |expected component| {report['peak']} "
          f"(a-priori bound {5 * 8}, limit {E.LIMIT[b.dtype]}), mismatches {report['bad']}, first {report['first_bad']}; "
          f"norm {got!r}, integer {norm}")
    assert report["bad"] == 0 and report["peak"] <= 5 * 8 < E.LIMIT[b.dtype], label
    assert norm < 1 << 53 and got == float(norm) and A.norm2(b.store) == got, label
    E.assert_exact(E.compare_all(v1, [], salt=1), [], b.dtype, label + ", V1 unchanged")
    E.assert_exact(E.compare_all(w, ops_w), ops_w, b.dtype, label + ", w unchanged")
    del v1, w
    b.close(label)


# ---- Born statistics and reduced density matrices, exactly --------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", EIGHT)
def test_overlap_of_two_arrays(size, layout):
    b = Budget(size, arrays=2)
    v1 = second_array(b)
    ov, n1, n0 = A.overlap(layout_view(v1, b.n, layout), layout_view(b.store, b.n, layout))
    want = E.inner_sums(1 << b.n, [], 1, [], 0, device=DEV)
    norms = [E.hash_norm2(1 << b.n, DEV, salt=s) for s in (1, 0)]
    label = f"overlap {size} {layout}"
    print(f"{label}: <V1|V0> {ov!r}, integers {want}; norms {n1!r} {n0!r}, integers {norms}")
    assert ov == complex(*want) and [n1, n0] == [float(v) for v in norms] and max(norms) < 1 << 53, label
    del v1
    b.close(label)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", EIGHT)
def test_marginals_and_density_matrices(size, layout):
    b = Budget(size)
    n, t = b.n, layout_view(b.store, b.n, layout)
    label = f"marginals and RDM {size} {layout}"
    for bits in ((n - 1, 15, 0), (n - 1, 2, 13, n - 2, 0, 15, 3, 12, 1, 14)):
        want = E.marginal_sums(1 << n, bits, DEV)
        got = A.marginal_probabilities(t, E.dims_on(t, bits))
        assert tuple(got.shape) == (2,) * len(bits) and got.dtype == torch.float64
        bad = int((got.reshape(-1).cpu() != torch.tensor([float(v) for v in want], dtype=torch.float64)).sum())
        print(f"{label}: marginal of bits {bits}: {len(want)} entries, largest {max(want)} (limit 2^53), mismatches {bad}")
        assert bad == 0, (label, bits)
    for bits in ((n - 1, 0), (n - 1, n - 2, 20, 11, 1, 0)):
        D = 2 ** len(bits)
        keep = E.dims_on(t, bits)
        assert A.rdm_info(t.shape, t.stride(), keep, b.dtype)["kernel"] == A._native.RDM_STREAM
        re, im = E.rdm_sums(1 << n, bits, DEV)
        rho = A.reduced_density_matrix(t, keep)
        assert tuple(rho.shape) == (D, D) and rho.dtype == torch.complex128
        host = rho.cpu()
        bad = int(((host.real != torch.tensor(re, dtype=torch.float64)) | (host.imag != torch.tensor(im, dtype=torch.float64))).sum())
        print(f"{label}: RDM of bits {bits}: {D} x {D}, trace {sum(re[c][c] for c in range(D))} (limit 2^53), mismatches {bad}")
        assert bad == 0, (label, bits)
        assert bool((host == host.mH).all()) and bool((host.diagonal().imag == 0).all()), (label, bits)
    b.close(label)


def cumulative_before(n, points, chunk=E.CHUNK):
    """(sum of |hash|^2 over the elements below p for every p of the ascending `points`, the total): Python ints."""
    out, run, todo = [], 0, list(points)
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        f, g = E.hash_index(torch.arange(lo, hi, device=DEV))
        c = torch.cumsum(f * f + g * g, 0)
        while todo and todo[0] < hi:
            p = todo.pop(0)
            out.append(run + (int(c[p - lo - 1]) if p > lo else 0))
        run += int(c[-1])
    return out, run


def expected_draws(n, targets, chunk=E.CHUNK):
    """For every integer T of `targets` (int64, on the device): the first memory index whose inclusive cumulative sum of
    |hash|^2 exceeds T, and |hash|^2 there -- the element whose interval holds T + 0.5."""
    index = torch.full_like(targets, -1)
    run = 0
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        f, g = E.hash_index(torch.arange(lo, hi, device=DEV))
        c = torch.cumsum(f * f + g * g, 0) + run
        pos = torch.searchsorted(c, targets, right=True)
        index = torch.where((index < 0) & (pos < hi - lo), pos + lo, index)
        run = int(c[-1])
    f, g = E.hash_index(index)
    return index, f * f + g * g


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", EIGHT)
def test_sample_with_forced_uniforms(size, layout):
    """2^12 uniforms (T_k + 0.5) / total for integers T_k: 0, total - 1, the integers just below and above the cumulative sum at
    the element of byte offset 2^32 and at the last element, the rest spread over [0, total)."""
    b = Budget(size)
    n, t = b.n, layout_view(b.store, b.n, layout)
    edge = (1 << 32) // b.store.element_size()
    (c_edge, c_last), total = cumulative_before(1 << n, [edge, (1 << n) - 1])
    special = [0, total - 1, c_edge - 1, c_edge, c_last - 1, min(c_last, total - 1)]
    spread = [(k * total) // 4091 for k in range(1, 4091)]
    targets = torch.tensor(special + spread, dtype=torch.int64)
    assert targets.numel() == 1 << 12 and int(targets.min()) == 0 and int(targets.max()) == total - 1 and total < 1 << 53
    u = (targets.double() + 0.5) / float(total)
    assert float((u * float(total) - (targets.double() + 0.5)).abs().max()) < 0.25 and float(u.max()) < 1.0
    index, weight = expected_draws(1 << n, targets.to(DEV))
    assert int(index[3]) >= edge > int(index[2]) and int(index.max()) <= (1 << n) - 1 and int(index.min()) >= 0
    got, prob = A.sample(t, uniforms=u.to(DEV))
    strings = torch.stack([(index >> (int(t.stride(d)).bit_length() - 1)) & 1 for d in range(n)], dim=-1)
    want = weight.double() / float(total)
    bad = int((got != strings).any(dim=1).sum())
    off = int(((prob - want).abs() > 2.0 ** -52 * want).sum())
    label = f"sample {size} {layout}"
    print(f"{label}: {targets.numel()} draws, total {total} (limit 2^53), indices {int(index.min())}..{int(index.max())}, "
          f"around element {edge}: {int(index[2])} and {int(index[3])}; wrong bitstrings {bad}, wrong probabilities {off}")
    assert bad == 0 and off == 0, label
    b.close(label)
