"""CPU-side checks of the drop-in boundary: the C-ABI library loads, exports every symbol
include/artn.h declares, refuses to compute without a GPU (no CPU fallback), and its
host-only planner answers queries."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef ARTN_DEV_\w+.*?#endif", "", text, flags=re.S)   # (development-only entry points: not the product ABI)
    return sorted(set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = N.lib()
    names = declared_symbols()
    assert len(names) >= 10
    assert names == N.exported_symbols()
    for name in names:
        assert hasattr(lib, name), name
    assert lib.artn_abi_version() == N.ABI_VERSION
    assert lib.artn_device_count() >= 0


def test_product_library_carries_no_development_entry_points_or_switches():
    """ABI 7 (round 5): the experiments that lost their A/B measurements -- three-step fusion, the split-bf16 arithmetic,
    some thirty planner switches -- are compiled into development builds only (make dev); the product library exports the
    header's entry points and reads a handful of switches from the environment."""
    lib = N.lib()
    dev = os.path.basename(N.LIB_PATH) != "libartn_hip.so" or os.environ.get("ARTN_LIB")
    if not dev and not hasattr(lib, "artn_contract3"):
        assert not N.has("artn_contract3_query")
        assert A.contraction.triple_info("ABCDEFGHIJKLMNOPQRSTUVWX,ABCab->DEFGHIJKLMNOPQRSTUVWXab", (2,) * 24, (2,) * 5,
                             "DEFGHIJKLMNOPQRSTUVWXab,DEFcd->GHIJKLMNOPQRSTUVWXabcd", (2,) * 5,
                             "GHIJKLMNOPQRSTUVWXabcd,GHIef->JKLMNOPQRSTUVWXabcdef", (2,) * 5) is None
    blob = open(N.LIB_PATH, "rb").read()
    switches = set(re.findall(rb"ARTN_[A-Z][A-Z0-9_]{2,}", blob))
    env_like = {s.decode() for s in switches}
    # names that are not environment switches (error text, macros that ended up in strings) are few; the bound is on all of them
    if not hasattr(lib, "artn_contract3"):
        assert len(env_like) < 15, sorted(env_like)


def test_struct_layouts_match_header():
    # sizes the C side was compiled with (ArtnStepDesc: 2 int32 + 4 arrays of 96 int64)
    assert ctypes.sizeof(N.ArtnStepDesc) == 8 + 4 * 96 * 8
    assert ctypes.sizeof(N.ArtnStepInfo) == 10 * 4 + 2 * 8 + 2 * 8 + 4 * 4 + 8 + 8 + 2 * 4   # (+ k3_bits, stage1_reruns: ABI versions 5, 7)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the CPU-only refusal")
def test_no_cpu_fallback_anywhere():
    a = torch.zeros(2, 2, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.contract("ab,bc->ac", a, a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.tensor_contraction({0: a, 1: a}, [((0, 1), "ab,bc->ac")])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.tensor_contraction_sparse({0: a, 1: a}, [((0, 1), "ab,bc->ac", [[torch.tensor([0])], [torch.tensor([0])]])])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.accumulate(a, a)
    # the raw ABI refuses too: no device -> ARTN_E_NODEVICE, never a host computation
    d, _ = A.contraction._descriptor(("a", "b"), ("b", "c"), ("a", "c"), (2, 2), (2, 1), (2, 2), (2, 1), torch.complex64)
    buf = np.zeros(8, dtype=np.complex64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert N.lib().artn_contract(ctypes.byref(d), p, p, p, None) == -4
    assert b"gfx950" in N.lib().artn_last_error()
    assert N.lib().artn_axpy_c64(p, p, 4, None) == -4
    assert N.lib().artn_sum_axis_c64(p, p, 1, 2, 2, None) == -4
    assert N.lib().artn_contract_gather(ctypes.byref(d), p, p, p, 0, None, 0, None, 0, None, None) == -4
    assert N.lib().artn_contract2(ctypes.byref(d), ctypes.byref(d), p, p, p, p, None) == -4
    assert N.lib().artn_contract2_acc(ctypes.byref(d), ctypes.byref(d), p, p, p, p, None) == -4
    assert N.lib().artn_contract_acc(ctypes.byref(d), p, p, p, None) == -4
    if N.has("artn_contract3"):   # (development builds)
        assert N.lib().artn_contract3(ctypes.byref(d), ctypes.byref(d), ctypes.byref(d), p, p, p, p, p, None) == -4
    assert N.lib().artn_absmax_normalize_c128(p, 4, p, None) == -4
    assert N.lib().artn_gather_rows(p, p, p, 1, 8, 1, None, None) == -4
    assert N.lib().artn_absmax_normalize_c64(p, 4, p, None) == -4


def test_planner_query_and_errors():
    info = A.step_info("ab,bc->ac", (2, 2), (2, 2))
    assert info["kernel"] == N.KERNEL_GENERIC and info["flops"] == 64.0 and info["out_shape"] == (2, 2)
    la = "ABCDEFGHIJKLMNOPQRSTUV"
    info = A.step_info(la + ",DKRUvwxyX->" + "".join(c for c in la if c not in "DKRU") + "vwxyX", (2,) * 22, (2,) * 9)
    assert info["kernel"] == N.KERNEL_BITS_MFMA and info["k_bits"] == 4
    assert info["lds_bytes"] <= 160 * 1024 and info["run_in_bits"] >= 1
    with pytest.raises(RuntimeError):
        A.step_info("ab,bc", (2, 2), (2, 2))
    with pytest.raises(RuntimeError):
        A.step_info("aab,bc->ac", (2, 2, 2), (2, 2))
    with pytest.raises(RuntimeError):
        A.step_info("ab,bc->ad", (2, 2), (2, 2))
    with pytest.raises(RuntimeError):
        A.step_info("ab,bc->ac", (2, 3), (2, 2))


def test_label_tuples_lift_the_alphabet_limit():
    # 60 distinct labels: more than the reference's 50-letter einsum alphabet (contraction.py:9-10)
    la = tuple(range(40))
    lb = tuple(range(36, 60))
    lo = tuple(x for x in la if x < 36) + tuple(x for x in lb if x >= 40)
    info = A.step_info((la, lb, lo), (2,) * 40, (2,) * 24)
    assert info["flops"] == 8.0 * 2.0 ** 60
    with pytest.raises(RuntimeError, match="alphabet"):
        A.einsum_eq_convert(([list(la)], [list(lb)])[0] + [list(lb)], list(lo))


def test_row_indices_are_validated_on_the_host_with_the_reference_semantics():
    """tensors[i][idx] in the reference (contraction.py:149-150, :177-178, :187) raises IndexError for
    an index outside [-rows, rows) and wraps negative ones; _device_index does both once per index
    tensor, before anything is launched."""
    from artensor_amd import contraction as C
    ok = torch.tensor([0, 3, -1, -4, 2])
    dev = C._device_index(ok, "cpu", 4)
    assert dev.tolist() == [0, 3, 3, 0, 2]
    assert C._device_index(ok, "cpu", 4) is dev                 # cached per (index tensor, rows)
    with pytest.raises(RuntimeError, match="row index out of range"):
        C._device_index(torch.tensor([0, 4]), "cpu", 4)
    with pytest.raises(RuntimeError, match="row index out of range"):
        C._device_index(torch.tensor([-5]), "cpu", 4)
    assert C._device_index(torch.tensor([7, 9]), "cpu", None).tolist() == [7, 9]   # unvalidated (kernel flag tests)


def test_precision_is_thread_local_and_caches_are_bounded():
    import threading
    from artensor_amd import contraction as C
    seen = {}

    def other():
        seen["before"] = C.precision.current()
        with C.precision("bf16"):
            seen["inside"] = C.precision.current()
        seen["after"] = C.precision.current()

    with C.precision("bf16"):
        th = threading.Thread(target=other)
        th.start()
        th.join()
        assert C.precision.current() == "bf16"
    assert C.precision.current() is None
    assert seen == {"before": None, "inside": "bf16", "after": None}
    b = C._Bounded(3)
    for k in range(10):
        b[k] = k
        assert len(b) <= 3
    assert b[9] == 9
    assert isinstance(C._desc_cache, C._Bounded) and isinstance(C._plan_cache, C._Bounded)


def test_single_row_index_lists_follow_the_reference_indexing():
    """`t[idx]` with ONE index (reference contraction.py:177-179): the sparse executor takes the row as a view -- negative indices
    count from the end, out of range raises (the reference dies with IndexError, contraction.py:192-195), several rows or rows of
    8 bytes (not 16-byte aligned views) keep the gather path."""
    from artensor_amd import contraction as C
    t = torch.zeros(3, 4, dtype=torch.complex64)
    assert C._single_row(torch.tensor([2]), t) == 2
    assert C._single_row(torch.tensor([-1]), t) == 2 and C._single_row(torch.tensor([-3]), t) == 0
    assert C._single_row(torch.tensor([0, 1]), t) is None
    assert C._single_row(torch.tensor([0]), torch.zeros(3, 1, dtype=torch.complex64)) is None
    assert C._single_row(torch.tensor([0]), torch.zeros((), dtype=torch.complex64)) is None
    with pytest.raises(RuntimeError, match="row index out of range"):
        C._single_row(torch.tensor([3]), t)
    with pytest.raises(RuntimeError, match="row index out of range"):
        C._single_row(torch.tensor([-4]), t)


def test_result_shape_is_one_function_with_and_without_the_extent_check():
    """_result_shape(la, lb, lo, shape_a, shape_b): the shape of a step's result.  The sites that check the two operands'
    extents against each other (_descriptor, _plain_form) pass check=True and get the descriptor's error; every other site
    keeps reading the second operand's extent, as its own copy of the computation did."""
    from artensor_amd import contraction as C
    la, lb, lo = ("a", "b"), ("b", "c"), ("c", "a")
    assert C._result_shape(la, lb, lo, (4, 3), (3, 5)) == (5, 4)
    assert C._result_shape(la, lb, lo, (4, 3), (3, 5), check=True) == (5, 4)
    assert C._result_shape(la, lb, lo, (4, 3), (2, 5)) == (5, 4)           # (not a checking site: no error)
    assert C._result_shape(la, lb, ("b",), (4, 3), (2, 5)) == (2,)
    with pytest.raises(RuntimeError, match="label 'b' has extent 3 in one operand and 2 in the other"):
        C._result_shape(la, lb, lo, (4, 3), (2, 5), check=True)
    with pytest.raises(RuntimeError, match="label 'b' has extent 3 in one operand and 2 in the other"):
        C._descriptor(la, lb, lo, (4, 3), (3, 1), (2, 5), (5, 1), torch.complex64)
    assert C._plain_form(((0, 1), (la, lb, lo)), (4, 3), (2, 5), 8) is None   # (the chain planner: no form, no error)
    # empty label tuples: a scalar result, a scalar operand
    assert C._result_shape(la, la, (), (4, 3), (4, 3), check=True) == ()
    assert C._result_shape(la, (), la, (4, 3), ()) == (4, 3)
    assert C._result_shape((), (), (), (), ()) == () and C._numel(()) == 1
    assert C._numel((4, 3, 0)) == 0 and C._numel((2,) * 40) == 2 ** 40


def test_a_compiled_launch_has_defaults_for_everything_but_its_first_step():
    from artensor_amd import contraction as C
    d, out_shape = C._descriptor(("a", "b"), ("b", "c"), ("a", "c"), (2, 2), (2, 1), (2, 2), (2, 1), torch.complex64)
    op = C._Op((0,), 5, 7, d, out_shape)
    assert (op.steps, op.i, op.j, op.out_shape) == ((0,), 5, 7, (2, 2)) and op.d1 is d
    assert op.j2 is None and op.j3 is None and op.d2 is None and op.d3 is None and op.info is None
    assert op.sum_rows == 0 and op.acc is None
    op = C._Op((0, 1), 5, 7, d, out_shape, j2=8, d2=d, info={"kernel": 1}, sum_rows=4, acc=False)
    assert (op.j2, op.d2, op.info, op.sum_rows, op.acc) == (8, d, {"kernel": 1}, 4, False)
    assert not hasattr(op, "__dict__")   # (slots: one of these per launch of every cached plan)
    # what _compile_dense emits is made of the same thing: the one step of a tiny scheme
    prog, ops = C._compile_dense([((0, 1), "ab,bc->ac")], {0: (2, 2), 1: (2, 2)}, torch.complex64)
    assert prog is None and len(ops) == 1
    op = ops[0]
    assert (op.steps, op.i, op.j, op.j2, op.j3, op.d2, op.d3, op.info, op.sum_rows, op.acc) == ((0,), 0, 1, None, None, None, None, None, 0, None)


@pytest.mark.parametrize("chain_plan", ["1", "0"])
def test_a_step_whose_equation_does_not_match_its_operand_ranks_is_named_as_such(monkeypatch, chain_plan):
    """_compile_dense forms the groups of steps before it emits them; a step with more labels than its operand has
    dimensions must still be refused by the descriptor builder, with its message and at its place in the execution order
    (not as a label that looks like a missing tensor id)."""
    from artensor_amd import contraction as C
    monkeypatch.setenv("ARTN_CHAIN_PLAN", chain_plan)
    with pytest.raises(RuntimeError, match="operand rank does not match the equation"):
        C._compile_dense([((0, 1), "abc,bd->acd")], {0: (2, 2), 1: (2, 2)}, torch.complex64)
    # ... behind good steps on the same tensor, and in front of a step whose operands disagree on an extent: the first
    # bad step in execution order is the one reported
    scheme = [((0, 1), "ab,bc->ac"), ((0, 2), "ac,cd->ad"), ((0, 3), "adx,de->ae"), ((0, 4), "ae,ef->af")]
    shapes = {0: (2, 2), 1: (2, 2), 2: (2, 2), 3: (2, 2), 4: (3, 2)}
    with pytest.raises(RuntimeError, match="operand rank does not match the equation"):
        C._compile_dense(scheme, shapes, torch.complex64)
    scheme[2] = ((0, 3), "ad,de->ae")
    with pytest.raises(RuntimeError, match="label 'e' has extent 2 in one operand and 3 in the other"):
        C._compile_dense(scheme, shapes, torch.complex64)
    with pytest.raises(KeyError):     # (tensor_contraction reports it: "scheme refers to tensor id 7 that was not supplied")
        C._compile_dense([((0, 7), "ab,bc->ac")], {0: (2, 2)}, torch.complex64)

