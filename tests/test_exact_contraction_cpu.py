"""Host-side checks of the exact-integer contraction tests (tests/exact_contraction.py, tests/exact_cases.py): the integer
reference against numpy's complex128 einsum, the exactness condition for every case the GPU file runs, planted errors that
`==` rejects -- one of which the max-norm tolerance of the parity tests accepts -- the coverage of the required planner paths,
and the emulators of the bit kernel, the two-operand GEMM and the extent GEMM on the same operands with `==`.

The planner plans for 256 CUs when no device is visible, the CU count of an MI355X, so the path assertions are made here;
test_exact_contraction_gpu.py repeats them per case on the device before it compares values."""
import numpy as np
import pytest

import exact_cases as E
import exact_contraction as X
from helpers import emulate, emulate_gemm, emulate_xgemm

STEP_TOL = 1e-5   # tests/test_gpu_parity.py


def rel(got, want):   # tests/test_gpu_parity.py
    want = np.asarray(want)
    return np.abs(np.asarray(got) - want).max() / max(np.abs(want).max(), 1e-30)


def _einsum128(eq, a, b):
    la, lb, lo = X.labels(eq)
    sym = {}
    for x in la + lb + lo:
        sym.setdefault(x, chr(65 + len(sym)) if len(sym) < 26 else chr(97 + len(sym) - 26))
    s = "".join(sym[x] for x in la) + "," + "".join(sym[x] for x in lb) + "->" + "".join(sym[x] for x in lo)
    big = np.size(a) * np.size(b) > 2 ** 36   # (the packed GEMM's shapes: through BLAS, the same integers below 2^53)
    return np.einsum(s, np.asarray(a, dtype=np.complex128), np.asarray(b, dtype=np.complex128), optimize=big)


@pytest.mark.parametrize("seed", range(44))
def test_reference_against_numpy_einsum(seed):
    """exact_einsum and its chained forms (pair, triple, gathered, accumulate) against a complex128 np.einsum on random small
    equations with shuffled label orders (as test_random_bit_steps draws them), batch labels and extents 2..5"""
    rng = np.random.default_rng(seed)
    ra = int(rng.integers(6, 11))
    k1, n1, k2, n2 = (int(x) for x in rng.integers(0, 4, size=4))
    batch = int(rng.choice([0, 0, 3, 5]))
    eqs, sa, sbs = E.bit_pair(seed, k1, n1, min(k2, ra - k1 + n1), n2, ra, batch=batch, mode=seed % 3)
    if seed % 4 == 3:   # extents that are no powers of two, label tuples
        eq, sa1, sb1 = E.extent_step(seed, dict(m0=3, m1=2, m2=5), dict(n0=3, n1=2), dict(k0=5, k1=3), dict(h0=2) if seed % 8 == 3 else None)
        a, (b,) = X.draw_chain(seed, "dense", "complex64", [(eq, sb1)], sa1)
        assert np.array_equal(X.exact_einsum(eq, a, b), _einsum128(eq, a, b))
    cls = ("wide", "dense")[seed % 2]
    a, (b1, b2) = X.draw_chain(seed, cls, "complex64", list(zip(eqs, sbs)), sa)
    mid = _einsum128(eqs[0], a, b1)
    assert np.array_equal(X.exact_einsum(eqs[0], a, b1), mid)
    want = _einsum128(eqs[1], mid, b2)
    assert np.array_equal(X.exact_pair(eqs[0], a, b1, eqs[1], b2), want)
    acc = X.draw_acc(rng, want.shape)
    assert np.array_equal(X.exact_accumulate(acc, want), acc.astype(np.complex128) + want)
    # a third step on the pair's result: contract its two slowest labels with a fresh small operand
    lo2 = X.labels(eqs[1])[2]
    if len(lo2) >= 3 and "z" not in lo2[-2:]:
        eq3 = "".join(lo2) + "," + "".join(lo2[-2:]) + "w->" + "".join(lo2[:-2]) + "w"
        b3 = X.draw_small(rng, X.labels(eq3)[1], (2, 2, 2), tuple(lo2[-2:]), cls)
        assert np.array_equal(X.exact_triple(eqs[0], a, b1, eqs[1], b2, eq3, b3), _einsum128(eq3, want, b3))
    if batch:   # rows gathered out of both operands (repeats)
        rows_a, rows_b = rng.integers(0, batch, size=7), rng.integers(0, batch, size=7)
        if X.labels(eqs[0])[1][0] == "z":
            assert np.array_equal(X.exact_gathered(eqs[0], a, rows_a, b1, rows_b), _einsum128(eqs[0], a[rows_a], b1[rows_b]))


def test_the_heavy_path_of_the_reference_is_the_integer_one(monkeypatch):
    """products above X.HEAVY multiply-adds go through float64 matmul: the same integers"""
    eq, sa, sb = E.bit_step(5, 4, 4, 12)
    a, (b,) = X.draw_chain(5, "wide", "complex64", [(eq, sb)], sa)
    want = X.exact_einsum(eq, a, b)
    monkeypatch.setattr(X, "HEAVY", 1)
    assert np.array_equal(X.exact_einsum(eq, a, b), want)


def test_generators_follow_their_class_rules():
    rng = np.random.default_rng(0)
    a = X.draw_a(rng, (2,) * 12, "wide")
    re, im = X.int_parts(a)
    for part in (re, im):
        assert np.all(np.abs(part) < 2 ** 20) and np.all(np.abs(part) >= 2 ** 19) and np.all(part & 1)   # 20 significant bits each
    b = X.draw_small(rng, "abcdxy", (2,) * 6, ("a", "c", "d"), "wide")   # 8 contracted values, 8 columns
    cols = b.transpose(1, 4, 5, 0, 2, 3).reshape(8, 8)
    assert np.all((cols != 0).sum(axis=1) == 4) and len({tuple(np.flatnonzero(c)) for c in cols}) > 1
    assert set(np.unique(cols[cols != 0])) <= set(X._UNITS)
    d = X.draw_small(rng, "abcdxy", (2,) * 6, ("a", "c", "d"), "dense")
    assert set(np.unique(np.abs(d.real))) == {1, 2} == set(np.unique(np.abs(d.imag)))
    h = X.draw_small(rng, "abcdxy", (2,) * 6, ("a", "c", "d"), "bf16", cap=X.bf16_cap(8))
    assert np.abs(h.real).max() <= 128 and np.abs(h.real).min() >= 1 and X._is_bf16(h)
    assert X.bf16_cap(512) == 90 and 512 * (2 * 90) ** 2 < 2 ** 24 <= 512 * (2 * 91) ** 2
    assert not X._is_bf16(np.array([257 + 0j])) and X._is_bf16(np.array([256 + 3j, 384 - 1j]))
    w = X.draw_a(rng, (64,), "wide128", "complex128")
    assert w.dtype == np.complex128 and np.abs(w.real).max() < 2 ** 44 and np.abs(w.real).min() >= 2 ** 43
    with pytest.raises(AssertionError, match="range quantity"):   # a case that violates the condition is an error, never a skip
        X.assert_exact_range("complex64", [("ab,bc->ac", np.full((2, 16), 2.0 ** 20 + 0j), np.ones((16, 2), dtype=np.complex64))])


@pytest.mark.parametrize("name", list(E.cases()))
def test_exactness_condition_of_every_gpu_case(name):
    """assert_exact_range for every case of the shared table, on the reference alone: a range failure shows up without a GPU"""
    case = E.cases()[name]
    _, _, q = E.exact_result(case)
    assert 0 < q < X.LIMIT[case.arith_kind]
    print(f"{name}: range quantity {X.headroom(q, case.arith_kind)}")


@pytest.mark.parametrize("case", E.wide_pairs(), ids=lambda c: c.name)
def test_exactness_condition_of_the_worker_s_wide_kernel_pairs(case):
    _, _, q = E.exact_result(case)
    assert 0 < q < X.LIMIT["complex64"]
    print(f"{case.name}: range quantity {X.headroom(q, 'complex64')}")


def test_planned_paths():
    """Every case gets the planner's answer committed in PLANNED, and the table covers every required path"""
    cases, live = E.cases(), {}
    assert set(cases) == set(E.PLANNED)
    for name, case in cases.items():
        got, info = E.planned(case)   # (asserts the case's path_properties on the whole answer)
        assert got == E.PLANNED[name], (name, got, E.PLANNED[name])
        live[name] = info
    P = live
    sel = lambda pred: [n for n, c in cases.items() if pred(c, P[n])]
    c64 = lambda c: c.dtype == "complex64" and c.precision is None
    single_bits = sel(lambda c, p: c.kind == "step" and c64(c) and p["kernel"] == E.KERNEL_BITS and "ARTN_FORCE_BITS" in c.env)
    for cls in ("wide", "dense"):
        mine = [n for n in single_bits if cases[n].cls == cls]
        assert {P[n]["k_bits"] for n in mine} == set(range(1, 9)), cls                                   # k = 1..8, k > 6 chained
        new_bits = {len(cases[n].b_shapes[0]) - P[n]["k_bits"] for n in mine}
        assert new_bits >= {0, 1, 2, 3, 4, 5, 6, 7}, (cls, new_bits)                                      # growing, size-preserving, shrinking
        assert {P[n]["arith"] for n in mine} == {0, 1}
        narrow = [n for n in mine if P[n]["k_bits"] in (5, 6) and P[n]["arith"] == 1 and P[n]["n_tile_bits"] <= 4]
        assert {P[n]["k_bits"] for n in narrow} == {5, 6}, cls                                           # narrow three-product form
        assert max(int(np.prod(cases[n].a_shape)) for n in mine) <= 2 ** 16
    assert sel(lambda c, p: c.precision == "bf16" and p["kernel"] == E.KERNEL_BITS and p["arith"] == 2)
    full = sel(lambda c, p: c64(c) and not c.env and p["kernel"] == E.KERNEL_BITS and c.get("full") and int(np.prod(c.a_shape)) == 2 ** 22
               and c.kind in ("step", "pair"))
    for kind in ("step", "pair"):
        assert {P[n]["k_bits"] for n in full if cases[n].kind == kind} == {3, 4, 5, 6}, kind             # FULL / artn_k_alt
        assert {P[n]["arith"] for n in full if cases[n].kind == kind} == {0, 1} or kind == "pair"
    pairs = {(P[n]["k_bits"], P[n]["k2_bits"]) for n in sel(lambda c, p: c.kind == "pair" and c64(c))}
    assert pairs >= {(6, 4), (3, 4), (5, 3), (4, 5), (4, 4), (5, 5), (5, 4), (3, 3), (2, 5), (3, 6)}, pairs   # the n30 chain's and the listed ones
    assert sel(lambda c, p: c.kind == "pair" and c.a_shape[0] not in (2,) and c64(c))                    # batch labels
    for kind in ("acc_pair", "acc_step"):
        assert {c.dtype for c in cases.values() if c.kind == kind} == {"complex64", "complex128"}, kind
    assert (6, 6) in {(P[n]["k_bits"], P[n]["k2_bits"]) for n in sel(lambda c, p: c.get("wide"))}                  # artn_k_wide, planned by default
    assert {tuple(len(X.contracted_labels(eq)) for eq in c.eqs) for c in E.wide_pairs()} == {(6, 6), (5, 6), (6, 5)}
    assert {c.cls for c in E.wide_pairs()} == {"wide", "dense"}
    gathers = sel(lambda c, p: c.kind == "gather")
    assert {cases[n].rows for n in gathers} >= {1, 7, 1000} and max(P[n]["k_bits"] for n in gathers) > 6
    assert {P[n]["kernel"] for n in gathers} == {E.KERNEL_BITS, E.KERNEL_GEMM}
    assert sel(lambda c, p: c.kind == "row_pairs")
    gemm = sel(lambda c, p: c64(c) and p["kernel"] == E.KERNEL_GEMM)
    assert {P[n]["arith"] for n in gemm} == {0, 1} and any(cases[n].get("split_k") for n in gemm) and any(cases[n].kind == "view" for n in gemm)
    assert len(sel(lambda c, p: c.kind == "step" and not c.env and c64(c) and p["kernel"] == E.KERNEL_GEMM and c.name.startswith("gemm_m"))) >= len(E.GEMM_STEPS)
    assert {(c.precision, P[c.name]["arith"]) for c in cases.values() if P[c.name]["kernel"] == E.KERNEL_PGEMM} == {("bf16", 2), (None, 1)}
    xg = sel(lambda c, p: p["kernel"] == E.KERNEL_XGEMM)
    assert {P[n]["m_tile_bits"] for n in xg} == {4, 6, 7}                              # xrow, xrow64, xgemm
    assert any(cases[n].get("rereads") == 3 for n in xg) and any(cases[n].dtype == "complex128" for n in xg)
    c128 = sel(lambda c, p: c.dtype == "complex128")
    assert {(P[n]["kernel"], cases[n].kind) for n in c128} >= {(E.KERNEL_GEMM, "step"), (E.KERNEL_BITS, "pair"), (E.KERNEL_BITS, "step"),
                                                               (E.KERNEL_GENERIC, "step"), (E.KERNEL_XGEMM, "step")}
    for k in (E.KERNEL_GEMM, E.KERNEL_BITS, E.KERNEL_GENERIC):
        assert {cases[n].cls for n in c128 if P[n]["kernel"] == k} == {"wide128", "dense"}
    assert len(sel(lambda c, p: c64(c) and p["kernel"] == E.KERNEL_GENERIC and "ARTN_FORCE_GENERIC" in c.env)) == 3


VIEW_CASES = [n for n, c in E.cases().items() if E.has_views(c)]


def test_view_cases_reach_every_kernel_family():
    """At least two cases with an operand view, a storage offset or an 8-byte B are planned on each of artn_k_bits,
    artn_k_bits128, the two-operand GEMM, the f64 GEMM, the extent GEMM and the packed GEMM themselves (cases the planner sends
    to the strided kernel -- an 8-byte A or C, by design -- do not count), every view kind is in use, and the three older view
    cases are still there."""
    cases = E.cases()
    assert {"gemm_views_wide", "gemm_views_dense", "xgemm_views_dense"} <= set(VIEW_CASES)
    count = {}
    for n in VIEW_CASES:
        c, (kernel, arith) = cases[n], E.PLANNED[n][:2]
        if c.kind not in ("step", "view"):
            continue
        family = {(E.KERNEL_BITS, False): "bits", (E.KERNEL_BITS, True): "bits128", (E.KERNEL_GEMM, False): "gemm", (E.KERNEL_GEMM, True): "gemm128",
                  (E.KERNEL_XGEMM, False): "xgemm", (E.KERNEL_XGEMM, True): "xgemm", (E.KERNEL_PGEMM, False): "pgemm"}.get((kernel, arith == 3))
        if family:
            count[family] = count.get(family, 0) + 1
    assert set(count) == {"bits", "bits128", "gemm", "gemm128", "xgemm", "pgemm"} and min(count.values()) >= 2, count
    used = {kind for n in VIEW_CASES for kind in cases[n].get("views", {}).values()}
    assert used == set(E.VIEW_KINDS), used
    for which in ("a", "b", "out"):   # an 8-byte base under A alone, B alone and the result alone
        assert any(cases[n].get("views") == {which: "offset8"} for n in VIEW_CASES), which
    assert {cases[n].m_tile_bits for n in VIEW_CASES if "m_tile_bits" in cases[n]} == {4, 6}   # the row-streaming forms
    assert {cases[n].precision for n in VIEW_CASES if E.PLANNED[n][0] == E.KERNEL_PGEMM} == {"bf16", None}
    kinds = {cases[n].kind for n in VIEW_CASES}
    assert kinds == {"view", "step", "pair", "gather", "row_pairs", "acc_step", "acc_pair"}, kinds
    # a gap skips an address bit and keeps every stride a power of two; a permuted A is dense
    for n in VIEW_CASES:
        c = cases[n]
        r = E.view_of(c)["a"]
        strides, _, contiguous = E.view_layout(r, 8)
        if c.get("views", {}).get("a") == "gap":
            assert all(s & (s - 1) == 0 for s in strides) and not contiguous and r.numel == 4 * int(np.prod(c.a_shape)), n
        if c.get("views", {}).get("a") == "permuted":
            assert sorted(strides) == sorted(E.view_layout(E._recipe(r.base_shape), 8)[0]) and not contiguous, n


@pytest.mark.parametrize("name", VIEW_CASES)
def test_view_slicing_is_torch_s_own(name):
    """The strides, the 16-byte phase of the first element and the contiguity that view_layout reads off numpy are what torch
    gives for the same recipe on a CPU tensor: the GPU test asserts them on what it passes to the library."""
    import torch
    case = E.cases()[name]
    dt = torch.complex128 if case.dtype == "complex128" else torch.complex64
    for which, r in E.view_of(case).items():
        flat = torch.empty(r.numel, dtype=dt)
        t = E.apply_view(r, flat)
        strides, phase, contiguous = E.view_layout(r, flat.element_size())
        assert tuple(t.stride()) == strides and t.is_contiguous() == contiguous, (which, tuple(t.stride()), strides)
        assert (t.data_ptr() - flat.data_ptr()) % 16 == phase, which
        rows = (case.rows,) if case.kind in ("gather", "row_pairs") else E.result_shape(case)[:1]
        want_shape = {"a": case.a_shape, "b": case.b_shapes[0], "out": rows + E.result_shape(case)[1:]}[which]
        assert tuple(t.shape) == tuple(want_shape), which
    a_kind, out_kind = case.get("views", {}).get("a"), case.get("views", {}).get("out")
    if a_kind in ("offset16", "offset8"):
        assert E.view_layout(E.view_of(case)["a"], 8 if dt == torch.complex64 else 16)[1:] == (0 if a_kind == "offset16" else 8, True)
    if out_kind == "offset8":
        assert E.view_layout(E.view_of(case)["out"], 8)[1:] == (8, True)


@pytest.mark.parametrize("name", VIEW_CASES)
def test_view_references_against_numpy_einsum(name):
    """exact_result of every case with views against complex128 np.einsum on the materialised (copied) views, and the base
    around the views holds no zero: a read one stride off the view changes the result"""
    case = E.cases()[name]
    a, smalls, acc, rows = ops = E.operands(case)
    want, start, _ = E.exact_result(case, ops)
    v = E.view_of(case)
    va, vb = np.ascontiguousarray(E.apply_view(v["a"], a)), np.ascontiguousarray(E.apply_view(v["b"], smalls[0]))
    assert va.shape == case.a_shape and vb.shape == case.b_shapes[0]
    if case.kind != "view":
        outside = np.ones(a.shape, dtype=bool)
        E.apply_view(v["a"], outside)[...] = False
        assert np.all(a[outside] != 0)
    if rows is not None:
        va, vb = va[rows[0]], vb[rows[1]]
    got = _einsum128(case.eqs[0], va, vb)
    if len(case.eqs) == 2:
        got = _einsum128(case.eqs[1], got, smalls[1])
    if start is not None:
        got = got + start.astype(np.complex128)
    assert np.array_equal(got, want)


def test_pairs_of_11_or_more_contracted_bits_fuse_on_the_wide_kernel_only():
    """6 + 6, 5 + 6 and 6 + 5 pairs fuse on artn_k_wide and nowhere else: by default from 2 048 tiles on (the 2^23-element case
    of the table), below that the planner declines them ("contracted bits spill") unless ARTN_WIDE_MIN_TILES lowers the
    threshold when the library loads -- which is how tests/exact_worker.py reaches them at 2^18 elements."""
    from artensor_amd import contraction as C
    for ra, fused in ((18, False), (22, False), (23, True)):
        eqs, sa, sbs = E.bit_pair(6666, 6, 6, 6, 6, ra)
        info = C.pair_info(eqs[0], sa, sbs[0], eqs[1], sbs[1])
        assert (info is not None) == fused, ra
        assert not fused or (E.is_wide(info) and (info["k_bits"], info["k2_bits"], info["arith"]) == (6, 6, 1))


# ---- planted errors ------------------------------------------------------------------------------------------------------
def _round_to_bits(x, bits):
    """round every real and imaginary part to `bits` significant bits (nearest)"""
    def part(v):
        m, e = np.frexp(v.astype(np.float64))
        return np.ldexp(np.rint(np.ldexp(m, bits)), e - bits)
    return part(x.real) + 1j * part(x.imag)


def test_planted_errors():
    """Four corruptions of a correct result are each rejected by `==`; the first -- the streamed operand carried with 16
    significant bits, what two bfloat16 pieces instead of three hold -- passes rel() < STEP_TOL on class wide: the gap in the
    max-norm tolerance that the exact tests close."""
    eq, sa, sb = E.bit_step(606, 6, 6, 16)
    for cls in ("wide", "dense"):
        a, (b,) = X.draw_chain(606, cls, "complex64", [(eq, sb)], sa)
        X.assert_exact_range("complex64", [(eq, a, b)])
        want = X.exact_einsum(eq, a, b)
        la, lb, lo = X.labels(eq)
        # 1. A rounded to 16 significant bits (class wide: the values of class dense have 11 and come through unchanged)
        a16 = _round_to_bits(a, 16)
        assert np.array_equal(a16, a) == (cls == "dense")
        if cls == "wide":
            lost = X.exact_einsum(eq, a16, b)
            assert not np.array_equal(lost, want)
            assert rel(lost, want) < STEP_TOL, rel(lost, want)
            print(f"A with 16 significant bits: rel {rel(lost, want):.2e} passes {STEP_TOL}, {np.count_nonzero(lost != want)} of {want.size} values differ")
        # 2. two output lanes of one 32 x 32 block swapped
        flat = want.reshape(-1, 32, 32).copy()
        i = next(i for i in range(32) if flat[3, 5, i] != flat[3, 5, (i + 1) % 32])
        flat[3, 5, [i, (i + 1) % 32]] = flat[3, 5, [(i + 1) % 32, i]]
        assert not np.array_equal(flat.reshape(want.shape), want)
        # 3. the imaginary part of one small-operand entry negated
        b_bad = b.copy()
        pos = tuple(np.argwhere(b.imag != 0)[7])
        b_bad[pos] = np.conj(b_bad[pos])
        assert not np.array_equal(X.exact_einsum(eq, a, b_bad), want)
        # 4. the last of the K terms dropped
        kax = [lb.index(x) for x in X.contracted_labels(eq)]
        b_cut = b.copy()
        b_cut[tuple(slice(-1, None) if n in kax else slice(None) for n in range(b.ndim))] = 0
        a_last = a[tuple(slice(-1, None) if x in X.contracted_labels(eq) else slice(None) for x in la)]
        assert np.any(a_last != 0)
        assert np.any(b != b_cut)   # (class wide: some column drew the last position -- 4 of 64 per column, 64 columns)
        assert not np.array_equal(X.exact_einsum(eq, a, b_cut), want)


# ---- the emulators on exact operands -------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", ["wide", "dense"])
@pytest.mark.parametrize("k,n,ra", [(3, 3, 14), (5, 5, 15), (6, 2, 16), (8, 4, 15), (4, 7, 13)])
def test_bit_kernel_emulation_is_exact(k, n, ra, cls, monkeypatch):
    monkeypatch.setenv("ARTN_FORCE_BITS", "1")
    eq, sa, sb = E.bit_step(100 * k + n, k, n, ra)
    a, (b,) = X.draw_chain(100 * k + n, cls, "complex64", [(eq, sb)], sa)
    X.assert_exact_range("complex64", [(eq, a, b)])
    got, used = emulate(eq, a, b)
    assert used == E.KERNEL_BITS
    assert np.array_equal(got, X.exact_einsum(eq, a, b).astype(np.complex64))


@pytest.mark.parametrize("cls", ["wide", "dense"])
@pytest.mark.parametrize("m,n,k,batch", [(8, 8, 7, 3), (7, 6, 9, 0), (5, 5, 11, 0)])
def test_gemm_emulation_is_exact(m, n, k, batch, cls):
    eq, sa, sb = E.gemm_step(10 * m + k, m, n, k, batch)
    a, (b,) = X.draw_chain(10 * m + k, cls, "complex64", [(eq, sb)], sa)
    X.assert_exact_range("complex64", [(eq, a, b)])
    got, info = emulate_gemm(eq, a, b)
    assert got is not None and info["kernel"] == E.KERNEL_GEMM
    assert np.array_equal(got, X.exact_einsum(eq, a, b).astype(np.complex64))


@pytest.mark.parametrize("cls", ["wide", "dense"])
@pytest.mark.parametrize("seed", range(3))
def test_extent_gemm_emulation_is_exact(seed, cls):
    """the replay of artn_k_xgemm (tests/test_xgemm_emulation.py) on extents 3, 5, 6, 9 mixed with 2, once planned for one CU
    (many rounds, the second launch for the last columns)"""
    eq, sa, sb = E.extent_step(40 + seed, dict(m0=9, m1=5, m2=6, m3=2, m4=3), dict(n0=3, n1=6, n2=[2, 5, 7][seed]), dict(k0=3, k1=5, k2=2),
                               dict(h0=2) if seed == 1 else None)
    a, (b,) = X.draw_chain(40 + seed, cls, "complex64", [(eq, sb)], sa)
    X.assert_exact_range("complex64", [(eq, a, b)])
    want = X.exact_einsum(eq, a, b).astype(np.complex64)
    for n_cu in (None, 1):
        got, info, modes = emulate_xgemm(eq, a, b, n_cu=n_cu)
        assert got is not None and info["kernel"] == E.KERNEL_XGEMM
        assert np.array_equal(got, want), (n_cu, modes)
