"""The contraction engine on exact-integer operands: every planner-selectable arithmetic path, compared with `==`.

Operands are Gaussian integers chosen (tests/exact_contraction.py) so that every product and every partial sum of a launch,
in any order, is an integer its accumulator holds exactly -- the range quantity max sum_k (|a_re| + |a_im|)(|b_re| + |b_im|)
stays below 2^24 (complex64, precision("bf16")) or 2^53 (complex128) at every stage, which covers the three products of the
3M form too.  The result must then equal the integer reference bit for bit, whatever the summation order, tile shape,
split-K, 3M or 4M form, MFMA shape or fusion; an operand that lost its low bits on the way to the matrix cores, or one wrong
lane of one small output, fails here although it passes the 1e-5 max-norm tolerance of test_gpu_parity.py
(test_exact_contraction_cpu.py::test_planted_errors shows both).

Every case of tests/exact_cases.py first asserts its path from the planner's own answer (PLANNED), then the exactness
condition on the reference alone, then np.array_equal.  A case that is planned onto another kernel fails; none is skipped
(fused triples excepted, on builds without them: that test runs on development builds only).  Each test prints the largest range quantity as a power of two.

Cases with operand views, storage offsets and 8-byte bases (exact_cases.view_cases) run through run_view_case: operands sliced
out of device copies of the reference's bases, layout asserted, everything inside guard margins that must come back unchanged."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import contraction as C
from artensor_amd.fixtures import load_case
import exact_cases as E
import exact_contraction as X
from helpers import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = E.cases()
SCHEME_SEED = 8   # (integer_leaves: every amplitude of the n12 state is non-zero with these leaves)


def gpu(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=8)   # (a case's operands and reference are up to a few hundred MB: the last few only)
def reference(name):
    """(operands, exact result, accumulator start, range quantity) of a case: computed once, never modified"""
    case = CASES[name]
    ops = E.operands(case)
    res, start, q = E.exact_result(case, ops)
    return ops, res, start, q


def assert_planned(case):
    got, info = E.planned(case)   # (asserts the case's path_properties on the whole answer)
    assert got == E.PLANNED[case.name], (case.name, dict(zip(E.INFO_FIELDS, got or ())), "planned", dict(zip(E.INFO_FIELDS, E.PLANNED[case.name])))
    return info


def run_case(case, a, smalls, start, rows):
    """the case's launch on the GPU; returns the result as a numpy array"""
    dt = torch.complex128 if case.dtype == "complex128" else torch.complex64
    with E.environment(case.env), A.precision(case.precision):
        if case.kind == "step":
            ta, tb = gpu(a), gpu(smalls[0])
            if case.get("split_k"):
                la, lb, lo = X.labels(case.eqs[0])
                assert C._big_k_outer(la, lb, lo, tuple(ta.shape), tuple(ta.stride()), tuple(tb.shape), tuple(tb.stride()), dt), "no split-K"
            got = A.contract(case.eqs[0], ta, tb)
        elif case.kind == "pair":
            got = C.contract2(case.eqs[0], gpu(a), gpu(smalls[0]), case.eqs[1], gpu(smalls[1]))
            assert got is not None, "the planner declined the pair"
        elif case.kind == "acc_pair":
            ta, tb1, tb2 = gpu(a), gpu(smalls[0]), gpu(smalls[1])
            got = gpu(start)
            d1, d2, out_shape = C._pair_descriptors(case.eqs[0], ta, tb1, case.eqs[1], tb2)
            assert tuple(out_shape) == tuple(got.shape)
            rc = N.lib().artn_contract2_acc(ctypes.byref(d1), ctypes.byref(d2), ta.data_ptr(), tb1.data_ptr(), tb2.data_ptr(), got.data_ptr(),
                                            N.current_stream_ptr(torch.device(DEV)))
            assert rc == 0, (rc, N.lib().artn_last_error())
        elif case.kind == "acc_step":
            ta, tb = gpu(a), gpu(smalls[0])
            got = gpu(start)
            la, lb, lo = X.labels(case.eqs[0])
            d, out_shape = C._descriptor(la, lb, lo, tuple(ta.shape), tuple(ta.stride()), tuple(tb.shape), tuple(tb.stride()), dt)
            assert tuple(out_shape) == tuple(got.shape)
            rc = N.lib().artn_contract_acc(ctypes.byref(d), ta.data_ptr(), tb.data_ptr(), got.data_ptr(), N.current_stream_ptr(torch.device(DEV)))
            assert rc == 0, (rc, N.lib().artn_last_error())
        elif case.kind == "gather":
            ra, rb = (torch.from_numpy(r) for r in rows)
            got = C.contract_gathered(case.eqs[0], gpu(a), ra, gpu(smalls[0]), rb)
            assert got is not None, "the gathered step does not fit the tiled kernels"
            one = C.contract_gathered(case.eqs[0], gpu(a), ra, gpu(smalls[0][rows[1]]), None)   # one operand gathered only
            assert one is not None and torch.equal(one, got)
        elif case.kind == "row_pairs":
            ra, rb = (torch.from_numpy(r) for r in rows)
            got = C.contract_row_pairs(case.eqs[0], gpu(a), ra, gpu(smalls[0]), rb)
            assert got is not None, "the pairs do not re-use rows enough"
        else:
            raise AssertionError(case.kind)
    assert got.dtype == dt
    return got.cpu().numpy()


MARGIN = 64               # guard elements on either side of every base and result buffer (a multiple of 16 bytes)
SENTINEL = complex(-77.0, 13.0)


def _bits(t):
    """the elements of a complex tensor as integer pairs: comparisons bit for bit"""
    return torch.view_as_real(t).view(torch.int32 if t.dtype == torch.complex64 else torch.int64)


class Guarded:
    """The device operand of a view recipe (exact_cases.view_of): its flat base between two margins of SENTINEL, sliced as
    numpy slices the reference's base, with the strides, the 16-byte phase of the pointer and the contiguity that numpy gives
    asserted on what is passed -- a `.contiguous()` on the way would change all three.  flat None: a result buffer, SENTINEL
    throughout.  assert_untouched compares the whole storage with its image from before the call, bit for bit; written=True
    leaves out the view's own elements, the only ones a launch may change."""

    def __init__(self, recipe, dtype, flat=None):
        self.recipe = recipe
        self.store = torch.full((2 * MARGIN + recipe.numel,), SENTINEL, dtype=dtype, device=DEV)
        if flat is not None:
            assert flat.shape == (recipe.numel,)
            self.store[MARGIN:MARGIN + recipe.numel] = torch.from_numpy(flat).to(DEV)
        self.view = E.apply_view(recipe, self.store, shift=MARGIN)
        strides, phase, contiguous = E.view_layout(recipe, self.store.element_size())
        assert tuple(self.view.stride()) == strides, (tuple(self.view.stride()), strides)
        assert self.view.data_ptr() % 16 == phase and self.view.is_contiguous() == contiguous, (self.view.data_ptr() % 16, phase, contiguous)
        self.snapshot()

    def snapshot(self):
        self.image = self.store.clone()

    def fill(self, values):
        self.view.copy_(gpu(values))
        self.snapshot()

    def assert_untouched(self, written=False):
        same = (_bits(self.store) == _bits(self.image)).all(dim=1)
        if written:
            own = torch.zeros_like(same)
            E.apply_view(self.recipe, own, shift=MARGIN)[...] = True
            same |= own
        assert bool(same.all()), (int((~same).sum()), "elements outside the view changed")


class _Launches:
    def __init__(self):
        self.infos = []

    def record(self, info, e0, e1):
        self.infos.append(info)


def run_view_case(case, a, smalls, start, rows):
    """the launch of a case with operand views: every operand and the result inside guard margins"""
    dt = torch.complex128 if case.dtype == "complex128" else torch.complex64
    v = E.view_of(case)
    ga, gb, go = Guarded(v["a"], dt, a), Guarded(v["b"], dt, smalls[0]), Guarded(v["out"], dt)
    ta, tb, out = ga.view, gb.view, go.view
    eq = case.eqs[0]
    stream = N.current_stream_ptr(torch.device(DEV))
    with E.environment(case.env), A.precision(case.precision):
        if case.kind in ("step", "view"):
            assert case.kind != "view" or not ta.is_contiguous()
            assert A.contract(eq, ta, tb, out=out) is out
        elif case.kind == "pair":
            b2 = gpu(smalls[1])
            C.profiler = seen = _Launches()
            try:
                got = C.contract2(eq, ta, tb, case.eqs[1], b2)
                if ta.is_contiguous():   # (at a 16-byte offset: still one launch)
                    assert got is not None and len(seen.infos) == 1 and seen.infos[0]["k2_bits"] == E.PLANNED[case.name][3] > 0, seen.infos
                else:                    # declined: the caller runs the two steps one after the other
                    assert got is None and seen.infos == []
                    got = A.contract(case.eqs[1], A.contract(eq, ta, tb), b2)
                    assert len(seen.infos) == 2 and all(i["k2_bits"] == 0 for i in seen.infos), seen.infos
                    assert tuple(seen.infos[0][f] for f in E.INFO_FIELDS) == E.PLANNED[case.name]
            finally:
                C.profiler = None
            out.copy_(got)
        elif case.kind == "gather":
            ra, rb = (torch.from_numpy(r) for r in rows)
            if tb.data_ptr() % 16 == ta.data_ptr() % 16 == 0:
                assert C.contract_gathered(eq, ta, ra, tb, rb, out=out) is out, "the gathered step does not fit the tiled kernels"
            else:   # refused (nothing written); the sparse executor's chunk loop then gathers both operands explicitly
                assert C.contract_gathered(eq, ta, ra, tb, rb, out=out) is None
                go.assert_untouched()
                tensors = {0: ta, 1: tb}
                C._sparse_step(tensors, ((0, 1), eq, ([ra[:3], ra[3:]], [rb[:3], rb[3:]]), None))
                out.copy_(tensors[0])
        elif case.kind == "row_pairs":
            ra, rb = (torch.from_numpy(r) for r in rows)
            assert C.contract_row_pairs(eq, ta, ra, tb, rb, out=out) is out, "the pairs do not re-use rows enough"
        elif case.kind == "acc_step" and case.get("wrapper"):
            go.fill(start)
            assert A.tensor_contraction({0: ta, 1: tb}, [((0, 1), eq)], accumulate_into=out) is out
        elif case.kind == "acc_step":
            go.fill(start)
            la, lb, lo = X.labels(eq)
            d, out_shape = C._descriptor(la, lb, lo, tuple(ta.shape), tuple(ta.stride()), tuple(tb.shape), tuple(tb.stride()), dt)
            assert tuple(out_shape) == tuple(out.shape)
            rc = N.lib().artn_contract_acc(ctypes.byref(d), ta.data_ptr(), tb.data_ptr(), out.data_ptr(), stream)
            assert rc == 0, (rc, N.lib().artn_last_error())
        elif case.kind == "acc_pair":
            go.fill(start)
            b2 = gpu(smalls[1])
            d1, d2, out_shape = C._pair_descriptors(eq, ta, tb, case.eqs[1], b2)
            assert tuple(out_shape) == tuple(out.shape)
            rc = N.lib().artn_contract2_acc(ctypes.byref(d1), ctypes.byref(d2), ta.data_ptr(), tb.data_ptr(), b2.data_ptr(), out.data_ptr(), stream)
            assert rc == 0, (rc, N.lib().artn_last_error())
        else:
            raise AssertionError(case.kind)
    ga.assert_untouched()
    gb.assert_untouched()
    go.assert_untouched(written=True)
    return out.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_exact_case(name):
    case = CASES[name]
    assert_planned(case)
    (a, smalls, _, rows), want, start, q = reference(name)   # (the exactness condition is asserted inside, on the reference alone)
    print(f"{name}: range quantity {X.headroom(q, case.arith_kind)}")
    got = (run_view_case if E.has_views(case) else run_case)(case, a, smalls, start, rows)
    assert got.shape == want.shape
    assert np.array_equal(got, want.astype(got.dtype)), (name, int(np.count_nonzero(got != want)), "of", got.size, "values differ")


def _scheme_leaves(case, dtype):
    leaves = E.integer_leaves({i: tuple(t.shape) for i, t in case.tensors.items()}, seed=SCHEME_SEED)
    return leaves, {i: gpu(t.astype(np.complex64 if dtype == torch.complex64 else np.complex128)) for i, t in leaves.items()}


def test_whole_dense_scheme_on_integer_leaves(monkeypatch):
    """The n12 dense scheme with its leaves replaced by integer tensors of the same shapes (complex-signed permutations, X, Z,
    S, unnormalised H): the one-launch program artn_k_program<float>, the same scheme step by step with the program and the
    fusing switched off, and artn_k_program<double> -- all three equal to the integer run of the scheme."""
    case = load_case(os.path.join(GOLDEN, "n12_dense.npz"))
    shapes = {k: tuple(t.shape) for k, t in case.tensors.items()}
    for dtype in (torch.complex64, torch.complex128):
        prog, main = C._plan_small_program(case.scheme, shapes, dtype)
        assert prog is not None and prog.n_steps == 68 and main == []
    leaves, _ = _scheme_leaves(case, torch.complex64)
    want, q = E.exact_dense_scheme(leaves, case.scheme, "complex64")
    print(f"n12 dense scheme: range quantity {X.headroom(q, 'complex64')}, {np.count_nonzero(want)} non-zero amplitudes")
    assert np.count_nonzero(want) == want.size
    got = A.tensor_contraction(_scheme_leaves(case, torch.complex64)[1], case.scheme).cpu().numpy()
    assert got.dtype == np.complex64 and np.array_equal(got, want.astype(np.complex64))
    got128 = A.tensor_contraction(_scheme_leaves(case, torch.complex128)[1], case.scheme).cpu().numpy()
    assert got128.dtype == np.complex128 and np.array_equal(got128, want)
    monkeypatch.setenv("ARTN_NO_PROGRAM", "1")
    monkeypatch.setenv("ARTN_NO_FUSE", "1")
    C._plan_cache.clear()
    C._pair_cache.clear()
    try:
        cut = A.tensor_contraction(_scheme_leaves(case, torch.complex64)[1], case.scheme).cpu().numpy()
    finally:
        monkeypatch.delenv("ARTN_NO_PROGRAM")
        monkeypatch.delenv("ARTN_NO_FUSE")
        C._plan_cache.clear()
        C._pair_cache.clear()
    assert np.array_equal(cut, want.astype(np.complex64))


def test_whole_sparse_scheme_on_integer_leaves(monkeypatch):
    """The n12 sparse-state fixture (5 bitstrings) through tensor_contraction_sparse on the same integer leaves: the default
    chain plan, pairs from the left (ARTN_CHAIN_PLAN=0) and complex128, against the integer run of the scheme's four kinds
    of step."""
    case = load_case(os.path.join(GOLDEN, "n12_sparse5.npz"))
    leaves, _ = _scheme_leaves(case, torch.complex64)
    want, q = E.exact_sparse_scheme(leaves, case.scheme, "complex64")
    print(f"n12 sparse scheme: range quantity {X.headroom(q, 'complex64')}, {np.count_nonzero(want)} of {want.size} amplitudes non-zero")
    assert np.count_nonzero(want) == want.size
    got = A.tensor_contraction_sparse(_scheme_leaves(case, torch.complex64)[1], case.scheme).cpu().numpy()
    assert np.array_equal(got, want.astype(np.complex64).reshape(got.shape))
    got128 = A.tensor_contraction_sparse(_scheme_leaves(case, torch.complex128)[1], case.scheme).cpu().numpy()
    assert got128.dtype == np.complex128 and np.array_equal(got128, want.reshape(got128.shape))
    monkeypatch.setenv("ARTN_CHAIN_PLAN", "0")
    left = A.tensor_contraction_sparse(_scheme_leaves(case, torch.complex64)[1], case.scheme).cpu().numpy()
    assert np.array_equal(left, want.astype(np.complex64).reshape(left.shape))


def test_switches_read_when_the_library_loads():
    """ARTN_XROW64=0 (the row-streaming cases on the 16-row instantiations of artn_k_xrow) and ARTN_WIDE=1 ARTN_WIDE_MIN_TILES=1
    (artn_k_wide, the only kernel that fuses 6 + 6, 5 + 6 and 6 + 5 pairs, at 2^18 elements) are read once per process:
    tests/exact_worker.py runs those cases in a process of its own, path asserted, compared with `==`."""
    env = dict(os.environ, ARTN_XROW64="0", ARTN_WIDE="1", ARTN_WIDE_MIN_TILES="1")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "exact_worker.py")], env=env,
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "exact worker ok" in r.stdout, r.stdout[-2000:]


def _tool(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("tool,seed", [("stress_random", 21), ("stress_extents", 22)])
def test_randomised_steps_on_exact_operands(tool, seed):
    """tools/stress_random.py and tools/stress_extents.py with exact=True: 40 random cases each, operands from the generators
    of tests/exact_contraction.py, compared with `==`."""
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")   # (small random steps on the strided kernel warn by design)
        assert _tool(tool).main(40, seed=seed, exact=True) == 0


@pytest.mark.skipif(not N.has("artn_contract3"), reason="three-step fusion is compiled into development builds only (make dev)")
def test_fused_triples_exactly():
    """artn_contract3 on the two triples of the n30 scheme (2^26-element surrogates: the planner takes triples from 2^14 tiles
    on), class dense, against the integer run of the three steps."""
    from helpers import shrink_triple
    steps = E._n30_steps()
    for (n1, n2, n3) in [(125, 128, 131), (149, 155, 159)]:
        (eq1, sa, sb1), (eq2, _, sb2), (eq3, _, sb3) = steps[n1], steps[n2], steps[n3]
        e1, sa_, sb1_, e2, sb2_, e3, sb3_ = shrink_triple(eq1, sa, sb1, eq2, sb2, eq3, sb3, max_log2=26)
        info = C.triple_info(e1, sa_, sb1_, e2, sb2_, e3, sb3_)
        assert info is not None and info["n_tiles"] >= 2 ** 14 and info["k3_bits"] > 0, (n1, info)
        a, (b1, b2, b3) = X.draw_chain(n1, "dense", "complex64", [(e1, sb1_), (e2, sb2_), (e3, sb3_)], sa_)
        want, q = X.exact_chain("complex64", [(e1, a, b1), (e2, None, b2), (e3, None, b3)])
        print(f"triple {n1}-{n2}-{n3}: range quantity {X.headroom(q, 'complex64')}")
        got = C.contract3(e1, gpu(a), gpu(b1), e2, gpu(b2), e3, gpu(b3))
        assert got is not None, (n1, n2, n3)
        assert np.array_equal(got.cpu().numpy(), want.astype(np.complex64))
        del got
        torch.cuda.empty_cache()
