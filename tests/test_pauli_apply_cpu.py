"""Host-side checks of y = H a (artensor_amd/pauli.py: pauli_apply_info, PauliSumOperator; artn_pauli_apply_query / _pack / artn_pauli_apply):
the symbols, the masks, folded coefficients and group order of the info call, the phase convention (y recomputed in numpy from the
info ALONE against an oracle that applies the 2 x 2 matrices axis by axis), the packed table by the layout documented in
include/artn.h, the refusals.  No GPU needed."""
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
Y2 = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
PHASE = [1, -1j, -1, 1j]                                       # (-i)^ny


def contiguous_strides(shape):
    out, s = [], 1
    for e in reversed(shape):
        out.append(s)
        s *= e
    return out[::-1]


def letters(p, nd):
    if isinstance(p, str):
        return list(p.upper())
    out = ["I"] * nd
    for d, c in p.items():
        out[d] = c.upper()
    return out


def oracle_apply(a_logical, p):
    """P a of the LOGICAL array, axis by axis in complex128 (np.flip for X, a sign multiply for Z, np.tensordot for Y)."""
    psi = np.asarray(a_logical).astype(np.complex128)
    phi = psi
    for d, c in enumerate(letters(p, psi.ndim)):
        if c == "X":
            phi = np.flip(phi, axis=d)
        elif c == "Z":
            sign = np.ones(psi.ndim, dtype=int)
            sign[d] = 2
            phi = phi * np.array([1.0, -1.0]).reshape(sign)
        elif c == "Y":
            phi = np.moveaxis(np.tensordot(Y2, phi, axes=([1], [d])), 0, d)
    return phi


def random_strings(rng, shape, count):
    return ["".join(rng.choice(list("IXYZ")) if e == 2 else "I" for e in shape) for _ in range(count)]


def desc(shape, strides, dtype=N.ARTN_C64):
    d = N.ArtnMarginalDesc()
    d.dtype, d.n_dims = dtype, len(shape)
    for i, (e, s) in enumerate(zip(shape, strides)):
        d.extent[i], d.stride[i] = e, s
    return d


def ptr(x):
    return x.ctypes.data_as(ctypes.c_void_p)


def query(shape, strides, ops, coeff=None, dtype=N.ARTN_C64, n_terms=None):
    """Status code of artn_pauli_apply_query on a hand-made descriptor."""
    ops = np.ascontiguousarray(np.asarray(ops, dtype=np.uint8))
    info = N.ArtnPauliApplyInfo()
    rc = N.lib().artn_pauli_apply_query(ctypes.byref(desc(shape, strides, dtype)), ptr(ops), None if coeff is None else ptr(coeff),
                                        ops.shape[0] if n_terms is None else n_terms, ctypes.byref(info), *([None] * 7))
    return rc, info


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_pauli_apply_query", "artn_pauli_apply_pack", "artn_pauli_apply"]
    assert N.ABI_VERSION == 9 and N.lib().artn_abi_version() == 9
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert ctypes.sizeof(N.ArtnPauliApplyInfo) == 4 * 4 + 3 * 8
    for name in ("pauli_sum_apply", "pauli_apply", "pauli_rotate", "pauli_sum_variance", "PauliSumOperator", "pauli_apply_info"):
        assert getattr(A, name) is getattr(pauli, name)


SHAPE13 = (2,) * 13
LAYOUTS = {
    "contiguous": contiguous_strides(SHAPE13),
    "permuted": [contiguous_strides(SHAPE13)[p] for p in (7, 0, 11, 3, 12, 5, 1, 9, 2, 10, 4, 8, 6)],
}


@pytest.mark.parametrize("name", list(LAYOUTS))
@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_info_masks_folded_coefficients_and_group_order(name, dtype):
    strides = LAYOUTS[name]
    rng = np.random.default_rng(len(name))
    strings = random_strings(rng, SHAPE13, 60) + ["I" * 13, "Z" * 13, "ZIIIIIIIIIIIZ"]
    coeffs = rng.standard_normal(len(strings)) + 1j * rng.standard_normal(len(strings))
    info = A.pauli_apply_info(SHAPE13, strides, list(zip(coeffs, strings)), dtype)
    ref = A.pauli_info(SHAPE13, strides, strings, dtype)
    for key in ("xmask", "zmask", "n_y", "group", "n_groups"):
        assert info[key] == ref[key], key
    for c, ny, f in zip(coeffs, info["n_y"], info["folded"]):
        assert f == c * PHASE[ny % 4]                                       # (a swap and sign changes: exact)
    ng = info["n_groups"]
    gx = info["group_xmask"]
    assert len(gx) == ng and all(gx[g] == x for g, x in zip(info["group"], info["xmask"]))
    order = info["group_order"]
    assert sorted(order) == list(range(ng)) and [info["group_pos"][g] for g in order] == list(range(ng))
    # sorted by xm_hi, ties in first-appearance order (= ascending group number): exactly Python's stable sort
    assert order == sorted(range(ng), key=lambda g: gx[g] >> 10)
    assert len({gx[g] >> 10 for g in range(ng)}) == info["n_xmask_hi"] > 1
    elem = 8 if dtype == torch.complex64 else 16
    assert info["bytes_read"] == info["bytes_written"] == 2 ** 13 * elem
    assert info["n_launches"] == 1
    assert info["table_bytes"] == 32 * (1 + ng + len(strings))


def y_from_info(a_mem, info):
    """y in MEMORY order from the info alone: a[i ^ xm], signs by popcount, the groups in the reported order."""
    n = a_mem.size
    i = np.arange(n, dtype=np.uint64)
    y = np.zeros(n, dtype=np.complex128)
    for g in info["group_order"]:
        w = np.zeros(n, dtype=np.complex128)
        for k, gk in enumerate(info["group"]):
            if gk == g:
                par = np.bitwise_count(i & np.uint64(info["zmask"][k])) & 1 if hasattr(np, "bitwise_count") else \
                    np.array([bin(int(v) & info["zmask"][k]).count("1") & 1 for v in i])
                w += info["folded"][k] * (1.0 - 2.0 * par)
        y += w * a_mem[(i ^ np.uint64(info["group_xmask"][g])).astype(np.int64)]
    return y


def test_the_phase_convention_against_the_axis_by_axis_oracle():
    shape = (2,) * 6
    rng = np.random.default_rng(6)
    a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    strings = random_strings(rng, shape, 12) + ["YIIIII", "YYYIZX"]           # (ny = 1 and 3 for certain)
    coeffs = rng.standard_normal(14) + 1j * rng.standard_normal(14)
    for perm in (list(range(6)), [3, 0, 5, 1, 4, 2]):
        # the logical tensor `t` is a permuted view of contiguous memory `mem`: t = mem.transpose(perm)
        mem = np.ascontiguousarray(a.transpose(np.argsort(perm)))
        t = mem.transpose(perm)
        assert (t == a).all()
        strides = [s // 16 for s in t.strides]
        for terms in ([(c, s) for c, s in zip(coeffs, strings)], [(1.0, strings[-1])], [(1.0, strings[-2])]):
            info = A.pauli_apply_info(shape, strides, terms, torch.complex128)
            y_mem = y_from_info(mem.reshape(-1), info)
            want = sum(c * oracle_apply(a, s) for c, s in terms)
            got = np.lib.stride_tricks.as_strided(y_mem, shape, [16 * s for s in strides])
            err = np.abs(got - want).max()
            bound = 8 * len(terms) * 2.0 ** -53 * sum(abs(c) for c, _ in terms) * np.abs(a).max()
            print(f"perm {perm}, {len(terms)} terms: err {err:.3e} (bound {bound:.3e})")
            assert err <= bound


def test_the_packed_table_decodes_by_the_documented_layout():
    strides = LAYOUTS["permuted"]
    rng = np.random.default_rng(3)
    strings = random_strings(rng, SHAPE13, 30) + ["I" * 13, "ZZIIIIIIIIIII"]
    coeffs = rng.standard_normal(len(strings)) + 1j * rng.standard_normal(len(strings))
    terms = list(zip(coeffs, strings))
    info = A.pauli_apply_info(SHAPE13, strides, terms)
    coeff, ops = pauli._split_terms(terms, 13)
    table, inf = pauli._pack(pauli._desc(SHAPE13, strides, torch.complex64), ops, coeff)
    assert table.dtype == np.uint8 and table.size == info["table_bytes"] == inf.table_bytes
    u, f = table.view(np.uint64).reshape(-1, 4), table.view(np.float64).reshape(-1, 4)
    ng, nt = info["n_groups"], len(strings)
    assert u[0].tolist() == [ng, nt, info["n_xmask_hi"], 0]
    at = 0
    for p, g in enumerate(info["group_order"]):
        members = [k for k in range(nt) if info["group"][k] == g]             # the caller's order
        assert u[1 + p].tolist() == [info["group_xmask"][g], at, len(members), 0]
        for k in members:
            rec = 1 + ng + at
            assert u[rec, 0] == info["zmask"][k] and u[rec, 1] == info["zmask"][k] & 3
            assert complex(f[rec, 2], f[rec, 3]) == info["folded"][k]
            at += 1
    assert at == nt and u.shape[0] == 1 + ng + nt


def test_refusals():
    err = N.lib().artn_last_error
    ok = [[3, 0], [1, 2]]
    assert query((2, 2), (2, 1), ok)[0] == 0
    rc, info = query((2, 2), (2, 1), ok, np.array([[1.0, 0.0], [0.0, 2.0]]))
    assert rc == 0 and (info.n_groups, info.n_launches, info.table_bytes) == (2, 1, 32 * 5)
    for strides in ((1, 1), (4, 1), (2, 2), (0, 1)):                          # a layout that is not dense
        assert query((2, 2), strides, ok)[0] == -1 and b"dense" in err()
    assert query((2, 3), (3, 1), [[1, 0]])[0] == -2 and b"power-of-two" in err()     # an extent that is no power of two
    for code in (1, 2, 3):                                                    # X, Y, Z on a dim of extent 4
        assert query((2, 4), (4, 1), [[0, code]])[0] == -1 and b"extent" in err()
    assert query((2, 2), (2, 1), ok, n_terms=0)[0] == -1 and b"at least one" in err()      # an empty term list
    assert N.lib().artn_pauli_apply_query(ctypes.byref(desc((2, 2), (2, 1))), ptr(np.zeros((1, 2), np.uint8)), None, 1, None,
                                          *([None] * 7)) == -1
    # a table that is too small, a null table
    d, ops = desc((2, 2), (2, 1)), np.array(ok, dtype=np.uint8)
    table = np.zeros(32 * 5 // 8, dtype=np.uint64)
    assert N.lib().artn_pauli_apply_pack(ctypes.byref(d), ptr(ops), None, 2, ptr(table), 32 * 5) == 0
    assert N.lib().artn_pauli_apply_pack(ctypes.byref(d), ptr(ops), None, 2, ptr(table), 32 * 5 - 1) == -1 and b"table" in err()
    assert N.lib().artn_pauli_apply_pack(ctypes.byref(d), ptr(ops), None, 2, None, 32 * 5) == -1
    # through the Python layer
    with pytest.raises(RuntimeError, match="dense"):
        A.pauli_apply_info((2, 2), (4, 1), [(1.0, "ZZ")])
    with pytest.raises(RuntimeError, match="extent"):
        A.pauli_apply_info((2, 4), (4, 1), [(1.0, "ZX")])
    with pytest.raises(RuntimeError, match="power-of-two"):
        A.pauli_apply_info((2, 3), (3, 1), [(1.0, "ZI")])
    with pytest.raises(ValueError, match="at least one"):
        A.pauli_apply_info((2, 2), (2, 1), [])
    with pytest.raises(TypeError, match="complex"):
        A.pauli_apply_info((2, 2), (2, 1), [(1.0, "ZZ")], dtype=torch.float32)


def apply_rc(a_ptr, y_ptr, table_ptr, table_bytes):
    """Status code of artn_pauli_apply on hand-made pointers: [2, 2] complex64 (32 bytes), two terms."""
    ops = np.array([[3, 0], [1, 2]], dtype=np.uint8)
    return N.lib().artn_pauli_apply(ctypes.byref(desc((2, 2), (2, 1))), ctypes.c_void_p(a_ptr), ctypes.c_void_p(y_ptr), ptr(ops), 2,
                                    ctypes.c_void_p(table_ptr), table_bytes, None)


def test_apply_refuses_bad_pointers_and_runs_nowhere_without_a_gpu():
    """Every call here is refused before anything is launched, so host addresses are safe to pass."""
    err = N.lib().artn_last_error
    buf = np.zeros(64, dtype=np.complex128)
    base = (buf.ctypes.data + 15) & ~15
    a, y, table, nbytes = base, base + 256, base + 512, 32 * 5
    cases = {
        "small table": (a, y, table, nbytes - 1, -1, b"table"),
        "misaligned y": (a, y + 8, table, nbytes, -2, b"16-byte"),
        "misaligned a": (a + 8, y, table, nbytes, -2, b"16-byte"),
        "y == a": (a, a, table, nbytes, -1, b"overlaps"),
        "y overlaps the end of a": (a, a + 16, table, nbytes, -1, b"overlaps"),
        "a overlaps the end of y": (y + 16, y, table, nbytes, -1, b"overlaps"),
        "null y": (a, 0, table, nbytes, -1, b"null"),
    }
    for name, (pa, py, pt, nb, want, text) in cases.items():
        rc = apply_rc(pa, py, pt, nb)
        if torch.cuda.is_available():
            assert rc == want and text in err(), name
        else:
            assert rc == -4 and b"no gfx950 device" in err(), name


def test_apply_functions_have_no_cpu_fallback():
    a = torch.zeros(2, 2, dtype=torch.complex64)
    for call in (lambda: A.pauli_apply(a, "ZZ"), lambda: A.pauli_sum_apply(a, [(0.5, "ZZ"), (1j, {0: "X"})]),
                 lambda: A.pauli_rotate(a, "XI", 0.3), lambda: A.pauli_sum_variance(a, [(1.0, "ZZ")]),
                 lambda: A.PauliSumOperator(a.shape, a.stride(), a.dtype, [(1.0, "ZZ")], "cpu")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
