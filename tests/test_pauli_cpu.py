"""Host-side checks of the Pauli-string layer (artensor_amd/pauli.py, artn_pauli_query / artn_pauli_expect): the translation of
strings to memory-bit masks, the grouping and launch count, the refusals, the two ways of writing a string.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import pauli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LETTERS = "IXYZ"


def contiguous_strides(shape):
    out, s = [], 1
    for e in reversed(shape):
        out.append(s)
        s *= e
    return out[::-1]


def masks_in_python(shape, strides, string):
    """xmask, zmask, n_y recomputed from the strides: a dim of extent 2 and stride 2^b is memory bit b."""
    xm = zm = ny = 0
    for d, c in enumerate(string.upper()):
        if c == "I":
            continue
        assert shape[d] == 2
        b = int(strides[d])
        assert b & (b - 1) == 0
        xm |= b if c in "XY" else 0
        zm |= b if c in "ZY" else 0
        ny += c == "Y"
    return xm, zm, ny


def groups_in_python(xmasks):
    first = {}
    return [first.setdefault(x, len(first)) for x in xmasks]


def random_strings(rng, shape, count):
    return ["".join(rng.choice(list(LETTERS)) if e == 2 else "I" for e in shape) for _ in range(count)]


def query(shape, strides, ops, dtype=torch.complex64, n_dims=None, n_terms=None, info=True):
    """Status code of artn_pauli_query on a hand-made descriptor."""
    d = N.ArtnMarginalDesc()
    d.dtype, d.n_dims = {torch.complex64: N.ARTN_C64, torch.complex128: N.ARTN_C128}.get(dtype, dtype), len(shape) if n_dims is None else n_dims
    for i, (e, s) in enumerate(zip(shape, strides)):
        d.extent[i], d.stride[i] = e, s
    ops = np.ascontiguousarray(np.asarray(ops, dtype=np.uint8))
    inf = N.ArtnPauliInfo()
    return N.lib().artn_pauli_query(ctypes.byref(d), ops.ctypes.data_as(ctypes.c_void_p), ops.shape[0] if n_terms is None else n_terms,
                                    ctypes.byref(inf) if info else None, None, None, None, None)


def test_the_feature_is_additive_to_abi_9():
    assert N.ABI_VERSION == 9 and N.lib().artn_abi_version() == 9
    assert N.has("artn_pauli_expect") and N.has("artn_pauli_query")
    assert ctypes.sizeof(N.ArtnPauliInfo) == 4 * 4 + 2 * 8
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"#ifdef ARTN_DEV_\w+.*?#endif", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text)))
    assert declared == N.exported_symbols()
    assert "artn_pauli_query" in declared and "artn_pauli_expect" in declared


LAYOUTS = {
    "contiguous": ((2,) * 12, contiguous_strides((2,) * 12)),
    "permuted": ((2,) * 12, [contiguous_strides((2,) * 12)[p] for p in (7, 0, 11, 3, 5, 1, 9, 2, 10, 4, 8, 6)]),
    "extent-1 dims": ((1, 2, 2, 1, 2, 2, 2, 1), (77, 1, 16, 5, 2, 8, 4, 1)),
    "extent-4 dim carrying I": ((2, 4, 2, 2, 8, 2), (1, 2, 8, 16, 32, 256)),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_masks_and_groups_against_the_strides(name, dtype):
    shape, strides = LAYOUTS[name]
    rng = np.random.default_rng(len(name))
    strings = random_strings(rng, shape, 40) + ["I" * len(shape)]
    info = A.pauli_info(shape, strides, strings, dtype)
    want = [masks_in_python(shape, strides, s) for s in strings]
    assert info["xmask"] == [w[0] for w in want]
    assert info["zmask"] == [w[1] for w in want]
    assert info["n_y"] == [w[2] for w in want]
    assert info["group"] == groups_in_python(info["xmask"])
    assert info["n_groups"] == len(set(info["xmask"]))
    T = info["terms_per_launch"]
    counts = np.bincount(info["group"])
    assert info["n_launches"] == sum(-(-int(c) // T) for c in counts)
    n = int(np.prod(shape))
    assert info["workspace_bytes"] > 0
    assert info["bytes_read"] == info["n_launches"] * n * (8 if dtype == torch.complex64 else 16)


def test_launch_count_of_groups_of_T_T_plus_1_and_2T_plus_3_terms():
    shape = (2,) * 12
    strides = contiguous_strides(shape)
    T = A.pauli_info(shape, strides, "Z" * 12)["terms_per_launch"]
    assert T >= 1
    rng = np.random.default_rng(5)

    def group_of(letters_x, count):     # `count` distinct-or-not strings with the X positions fixed and Z/I elsewhere
        return ["".join(letters_x[d] if letters_x[d] != "I" else rng.choice(["I", "Z"]) for d in range(12)) for _ in range(count)]

    for count, launches in ((T, 1), (T + 1, 2), (2 * T + 3, 3)):
        info = A.pauli_info(shape, strides, group_of("I" * 12, count))
        assert (info["n_groups"], info["n_launches"]) == (1, launches)
        assert info["bytes_read"] == launches * 4096 * 8
    # three groups at once, interleaved in the input order
    ga, gb, gc = group_of("XIIIIIIIIIII", T), group_of("IIIIIIIIIIXX", T + 1), group_of("I" * 12, 2 * T + 3)
    mixed = []
    for i in range(2 * T + 3):
        mixed += [g[i] for g in (gc, gb, ga) if i < len(g)]
    info = A.pauli_info(shape, strides, mixed)
    assert info["n_groups"] == 3 and info["n_launches"] == 1 + 2 + 3
    assert info["group"] == groups_in_python(info["xmask"])
    assert info["workspace_bytes"] > 0 and info["bytes_read"] == 6 * 4096 * 8
    # X and Y on the same dims share a group; the Re/Im choice is per term
    info = A.pauli_info(shape, strides, ["XIIIIIIIIIIZ", "YIIIIIIIIIII", "IXIIIIIIIIII"])
    assert info["group"] == [0, 0, 1] and info["n_y"] == [0, 1, 0]


def test_refusals():
    err = N.lib().artn_last_error
    ok = [[3, 0], [1, 2]]
    assert query((2, 2), (2, 1), ok) == 0
    assert query((2, 2), (1, 2), ok) == 0
    # a layout that is not dense
    for strides in ((1, 1), (4, 1), (2, 2), (0, 1)):
        assert query((2, 2), strides, ok) == -1
        assert b"dense" in err()
    assert query((2, 1, 2), (2, 99, 1), [[1, 0, 3]]) == 0                 # the stride of an extent-1 dim means nothing
    # an operator code above 3
    assert query((2, 2), (2, 1), [[4, 0]]) == -1 and b"operator code" in err()
    assert query((2, 2), (2, 1), [[0, 0], [0, 255]]) == -1 and b"operator code" in err()
    # X, Y or Z on a dim whose extent is not 2
    for code in (1, 2, 3):
        assert query((2, 4), (4, 1), [[0, code]]) == -1 and b"extent" in err()
        assert query((1, 2), (2, 1), [[code, 0]]) == -1 and b"extent" in err()
    assert query((2, 4), (4, 1), [[3, 0]]) == 0
    # n_terms < 1
    assert query((2, 2), (2, 1), ok, n_terms=0) == -1 and b"at least one" in err()
    assert query((2, 2), (2, 1), ok, n_terms=-3) == -1
    # null pointers
    assert query((2, 2), (2, 1), ok, info=False) == -1
    assert N.lib().artn_pauli_query(None, None, 1, ctypes.byref(N.ArtnPauliInfo()), None, None, None, None) == -1
    # an extent that is no power of two
    assert query((2, 3), (3, 1), [[1, 0]]) == -2 and b"power-of-two" in err()
    assert query((6,), (1,), [[0]]) == -2
    # more than 96 dims
    assert query((2,) * 96, contiguous_strides((2,) * 40) + [1] * 56, [[0] * 97], n_dims=97) == -2 and b"96" in err()
    # n > 2^40
    shape = (2,) * 41
    assert query(shape, contiguous_strides(shape), [[0] * 41]) == -2 and b"2^40" in err()
    assert query((2,) * 40, contiguous_strides((2,) * 40), [[1] * 40]) == 0
    # a dtype that is not complex64 / complex128
    assert query((2, 2), (2, 1), ok, dtype=N.ARTN_C64_BF16) == -2
    # through the Python layer
    with pytest.raises(RuntimeError, match="dense"):
        A.pauli_info((2, 2), (4, 1), "ZZ")
    with pytest.raises(RuntimeError, match="extent"):
        A.pauli_info((2, 4), (4, 1), "ZZ")
    with pytest.raises(TypeError, match="complex"):
        A.pauli_info((2, 2), (2, 1), "ZZ", dtype=torch.float32)


def test_expect_refuses_a_small_workspace_and_runs_nowhere_without_a_gpu():
    d = N.ArtnMarginalDesc()
    d.dtype, d.n_dims = N.ARTN_C64, 2
    d.extent[0], d.extent[1], d.stride[0], d.stride[1] = 2, 2, 2, 1
    ops = np.array([[3, 0]], dtype=np.uint8)
    buf = np.zeros(64, dtype=np.complex128)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    rc = N.lib().artn_pauli_expect(ctypes.byref(d), p, ops.ctypes.data_as(ctypes.c_void_p), 1, p, p, 0, None)
    if torch.cuda.is_available():
        assert rc == -1 and b"workspace" in N.lib().artn_last_error()     # (refused before anything is launched)
    else:
        assert rc == -4 and b"no gfx950 device" in N.lib().artn_last_error()


def test_the_two_ways_of_writing_a_string():
    ops, single = pauli.pauli_ops("IxYz", 4)
    assert single and ops.dtype == np.uint8 and ops.tolist() == [[0, 1, 2, 3]]
    same, single = pauli.pauli_ops({1: "X", -2: "y", 3: "Z"}, 4)
    assert single and (same == ops).all()
    both, single = pauli.pauli_ops(["IXYZ", {1: "x", 2: "Y", -1: "z"}, {}], 4)
    assert not single and both.tolist() == [[0, 1, 2, 3], [0, 1, 2, 3], [0, 0, 0, 0]]
    shape, strides = (2,) * 4, contiguous_strides((2,) * 4)
    a, b = A.pauli_info(shape, strides, ["IXYZ"]), A.pauli_info(shape, strides, [{1: "X", 2: "Y", 3: "Z"}])
    assert a == b and a["xmask"] == [0b0110] and a["zmask"] == [0b0011] and a["n_y"] == [1]
    for bad in ("IXY", "IXYZZ", ""):
        with pytest.raises(ValueError, match="length"):
            pauli.pauli_ops(bad, 4)
    for bad in ("IXYA", "IX Z", {0: "Q"}, {0: "XY"}, {0: 1}):
        with pytest.raises(ValueError, match="not one of"):
            pauli.pauli_ops(bad, 4)
    for bad in ({4: "X"}, {-5: "X"}, {0: "X", -4: "Z"}):
        with pytest.raises(ValueError, match="dims"):
            pauli.pauli_ops(bad, 4)
    with pytest.raises(ValueError, match="at least one"):
        pauli.pauli_ops([], 4)
    with pytest.raises(TypeError):
        pauli.pauli_ops([3], 4)


def test_pauli_functions_have_no_cpu_fallback():
    """A CPU tensor is refused wherever the test runs."""
    a = torch.zeros(2, 2, dtype=torch.complex64)
    for call in (lambda: A.pauli_expectation(a, "ZZ"), lambda: A.pauli_expectation(a, ["ZZ", "XI"], device=True),
                 lambda: A.pauli_sum_expectation(a, [(0.5, "ZZ"), (1j, {0: "X"})])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
