"""Host-side checks of the Pauli expectation values per trajectory (artensor_amd/trajectories.py: pauli_batch_info,
pauli_expectation_batch, pauli_sum_expectation_batch, trajectory_mean; artn_pauli_batch_query / _expect): the symbols, the plan
on random permuted layouts against the pure-Python plan of pauli_batch_oracle.py, every refusal by its code and a word of its
text, the Python-side errors, trajectory_mean on CPU tensors against numpy, and the bound of the exact-integer states.  No GPU
needed: artn_pauli_batch_expect checks every argument before it looks for a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import pauli
from artensor_amd import trajectories as T

import pauli_batch_oracle as PO
from test_pauli_apply_cpu import contiguous_strides, desc, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NAMES = ("pauli_expectation_batch", "pauli_sum_expectation_batch", "trajectory_mean", "pauli_batch_info")
LB = {torch.complex64: 4, torch.complex128: 3}


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_pauli_batch_query", "artn_pauli_batch_expect"]
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    assert "#define ARTN_ABI_VERSION 9" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert ctypes.sizeof(N.ArtnPauliBatchInfo) == 8 * 4 + 7 * 8 + 3 * 4 * N.BATCH_MAX_FIELDS
    body = re.search(r"typedef struct ArtnPauliBatchInfo \{(.*?)\} ArtnPauliBatchInfo;", text, flags=re.S).group(1)
    fields = [f.strip().split("[")[0] for line in body.split(";") if line.strip()
              for f in re.sub(r"^\s*\w+\s+", "", line.strip()).split(",")]
    assert fields == [name for name, _ in N.ArtnPauliBatchInfo._fields_]


def test_the_names_live_in_trajectories():
    for name in NAMES:
        assert getattr(A, name) is getattr(T, name) and name in T.__all__
    assert not set(NAMES) & set(pauli.__all__)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def layouts(dtype):
    """(shape, strides, batch dims, strings): 8 to 16 dims of extent 2 in a random memory order, batch bits at or above the line."""
    rng = np.random.default_rng(41 if dtype == torch.complex64 else 42)
    lb = LB[dtype]
    for nd in range(8, 17):
        for mode in ("no batch", "one", "few", "many"):
            bit = [int(b) for b in rng.permutation(nd)]
            high = [b for b in range(nd) if b >= lb]
            nbb = {"no batch": 0, "one": 1, "few": min(3, len(high)), "many": len(high) - int(rng.integers(0, 2))}[mode]
            bbits = [int(b) for b in rng.choice(high, size=nbb, replace=False)]
            batch = [bit.index(b) for b in bbits]
            free = [d for d in range(nd) if d not in batch]
            strings = []
            for k in range(int(rng.integers(1, 60))):
                s = ["I"] * nd
                movers = free[:2] if k % 3 else free[-2:]      # few distinct X/Y positions: groups that fill up
                for d in free:
                    if d in movers:
                        s[d] = str(rng.choice(list("IIZZZZXY")))
                    elif rng.random() < 0.5:
                        s[d] = "Z"
                strings.append("".join(s))
            yield (2,) * nd, tuple(1 << b for b in bit), batch, strings


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_the_plan_agrees_with_the_oracle(dtype):
    seen = set()
    elem = 8 if dtype == torch.complex64 else 16
    for shape, strides, batch, strings in layouts(dtype):
        info = A.pauli_batch_info(shape, strides, strings, batch, dtype)
        want = PO.plan(shape, strides, strings, batch)
        for key in ("xmask", "zmask", "n_y", "group", "local_xmask", "local_zmask", "n_groups", "n_launches", "B", "n", "batch_bits",
                    "local_bits", "tile_bits", "chunks", "chunks_halved", "grid", "workspace_bytes", "out_bytes", "fields"):
            assert info[key] == want[key], (key, shape, strides, batch)
        assert info["terms_per_launch"] == PO.TERMS and info["bytes_read"] == info["n_launches"] * info["n"] * elem
        assert all(x < 2 ** info["local_bits"] for x in info["local_xmask"] + info["local_zmask"])
        seen.add((info["B"] > 1, info["local_bits"] >= 10, info["chunks"] < want["tiles"], info["n_launches"] > info["n_groups"]))
    assert {(True, True, False, True), (True, False, False, True), (False, True, False, True)} <= seen, seen
    # C < T: 2^22 elements, B = 8 on the top bits, and B = 1 beyond 2048 tiles
    nd = 22
    shape, strides = (2,) * nd, tuple(contiguous_strides((2,) * nd))
    info = A.pauli_batch_info(shape, strides, ["I" * 3 + "X" + "Z" * 18], [0, 1, 2], dtype)
    assert (info["B"], info["local_bits"], info["chunks"], info["chunks_halved"], info["grid"]) == (8, 19, 256, 256, 2048)
    assert info == {**info, **{k: v for k, v in PO.plan(shape, strides, ["I" * 3 + "X" + "Z" * 18], [0, 1, 2]).items() if k in info}}
    info = A.pauli_batch_info(shape, strides, ["Z" * nd], (), dtype)
    assert (info["B"], info["chunks"], info["chunks_halved"], info["fields"]) == (1, 2048, 2048, [])
    assert info["workspace_bytes"] == A.pauli_info(shape, strides, ["Z" * nd], dtype)["workspace_bytes"]


def test_batch_dims_empty_is_the_unbatched_plan():
    rng = np.random.default_rng(3)
    for nd in (0, 1, 4, 9, 10, 13):
        shape = (2,) * nd
        strides = tuple(1 << int(b) for b in rng.permutation(nd))
        strings = ["".join(rng.choice(list("IXYZ"), nd)) for _ in range(20)]
        one, many = A.pauli_info(shape, strides, strings), A.pauli_batch_info(shape, strides, strings, ())
        for key in ("xmask", "zmask", "n_y", "group", "n_groups", "n_launches", "terms_per_launch", "workspace_bytes", "bytes_read"):
            assert one[key] == many[key], (nd, key)
        assert many["local_xmask"] == many["xmask"] and many["local_zmask"] == many["zmask"] and many["B"] == 1


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def call(shape, strides, strings, batch, dtype=N.ARTN_C64, *, expect=False, a=256, out=256, ws=256, ws_bytes=None, ops=None, nb=None):
    """(code, message) of artn_pauli_batch_query, or of artn_pauli_batch_expect with made-up addresses (never dereferenced: every
    call here is refused before a device is looked for)."""
    if ops is None:
        ops, _ = pauli.pauli_ops(strings, len(shape))
    ops = np.ascontiguousarray(ops, dtype=np.uint8)
    b = np.array(list(batch), dtype=np.int32)
    d, info = desc(shape, strides, dtype), N.ArtnPauliBatchInfo()
    nb = b.shape[0] if nb is None else nb
    bp = ptr(b) if b.shape[0] else None
    if expect:
        if ws_bytes is None:
            assert N.lib().artn_pauli_batch_query(ctypes.byref(d), ptr(ops), ops.shape[0], nb, bp, ctypes.byref(info), *[None] * 6) == 0
            ws_bytes = info.workspace_bytes
        rc = N.lib().artn_pauli_batch_expect(ctypes.byref(d), a, ptr(ops), ops.shape[0], nb, bp, out, ws, ws_bytes, None)
    else:
        rc = N.lib().artn_pauli_batch_query(ctypes.byref(d), ptr(ops), ops.shape[0], nb, bp, ctypes.byref(info), *[None] * 6)
    return rc, (N.lib().artn_last_error() or b"").decode()


def refused(code, word, *args, **kw):
    rc, msg = call(*args, **kw)
    assert rc == code and word in msg, (rc, msg)


def test_every_refusal_has_its_code_and_its_text():
    nd = 12
    shape, strides = (2,) * nd, contiguous_strides((2,) * nd)                 # dim d holds memory bit 11 - d
    z = "I" * 2 + "Z" * 10
    # X, Y or Z on a batch dimension
    for letter in "XYZ":
        refused(INVALID, "batch dimension", shape, strides, [z, letter + "I" * 11], [0, 1])
        refused(INVALID, "batch dimension", shape, strides, [letter + "I" * 11], [0, 1], expect=True, ws_bytes=1 << 20)
    # what artn_pauli_query calls invalid
    refused(INVALID, "operator code", shape, strides, None, [0], ops=np.full((1, nd), 4))
    refused(INVALID, "extent 2", (4,) + (2,) * 10, contiguous_strides((4,) + (2,) * 10), None, [], ops=np.array([[1] + [0] * 10]))
    refused(INVALID, "not dense", shape, [2 * s for s in strides], [z], [0])
    refused(INVALID, "at least one", shape, strides, None, [0], ops=np.zeros((0, nd)))
    # what state_batch_dims calls invalid
    refused(INVALID, "out of range", shape, strides, [z], [nd])
    refused(INVALID, "out of range", shape, strides, [z], [-1])
    refused(INVALID, "repeated", shape, strides, [z], [1, 1])
    refused(INVALID, "negative", shape, strides, [z], [], nb=-1)
    # a workspace smaller than the query reports; null pointers
    refused(INVALID, "workspace smaller", shape, strides, [z], [0, 1], expect=True, ws_bytes=8)
    refused(INVALID, "null pointer", shape, strides, [z], [0, 1], expect=True, a=None)
    # a batch bit below the line (complex64: bit 4; complex128: bit 3)
    refused(UNSUPPORTED, "below a 128-byte line", shape, strides, ["Z" * 11 + "I"], [11])
    refused(UNSUPPORTED, "below a 128-byte line", shape, strides, ["I" * 8 + "I" + "ZZZ"], [8])
    rc, _ = call(shape, strides, ["I" * 8 + "I" + "ZZZ"], [8], N.ARTN_C128)
    assert rc == 0
    refused(UNSUPPORTED, "below a 128-byte line", shape, strides, ["I" * 9 + "I" + "ZZ"], [9], N.ARTN_C128)
    # more than ARTN_BATCH_MAX_BITS batch bits
    big = (2,) * 30
    refused(UNSUPPORTED, "batch bits", big, contiguous_strides(big), ["I" * 25 + "Z" * 5], list(range(25)))
    # B * (n_terms + 1) above 2^28
    refused(UNSUPPORTED, "2^28", big, contiguous_strides(big), ["I" * 24 + "Z" * 6] * 16, list(range(24)))
    rc, _ = call(big, contiguous_strides(big), ["I" * 24 + "Z" * 6] * 15, list(range(24)))
    assert rc == 0
    # alignment
    refused(UNSUPPORTED, "16-byte aligned", shape, strides, [z], [0, 1], expect=True, a=264)
    refused(UNSUPPORTED, "8-byte aligned", shape, strides, [z], [0, 1], expect=True, out=260)
    refused(UNSUPPORTED, "8-byte aligned", shape, strides, [z], [0, 1], expect=True, ws=260)
    # the refusals of the unbatched query
    refused(UNSUPPORTED, "complex64 or complex128", shape, strides, [z], [0], 99)
    refused(UNSUPPORTED, "power-of-two", (3,) + (2,) * 10, contiguous_strides((3,) + (2,) * 10), None, [], ops=np.zeros((1, 11)))
    refused(UNSUPPORTED, "2^40", (2,) * 41, contiguous_strides((2,) * 41), None, [], ops=np.zeros((1, 41)))
    d, info, ops = desc((1,) * 96, (1,) * 96), N.ArtnPauliBatchInfo(), np.zeros((1, 97), dtype=np.uint8)
    d.n_dims = 97
    assert N.lib().artn_pauli_batch_query(ctypes.byref(d), ptr(ops), 1, 0, None, ctypes.byref(info), *[None] * 6) == UNSUPPORTED
    assert "at most 96 dimensions" in N.lib().artn_last_error().decode()


def test_python_side_errors():
    shape = (2,) * 8
    with pytest.raises(RuntimeError, match="batch dimension"):
        A.pauli_batch_info(shape, contiguous_strides(shape), ["X" + "I" * 7], [0])
    with pytest.raises(TypeError, match="complex64 or complex128"):
        A.pauli_batch_info(shape, contiguous_strides(shape), ["Z" * 8], [], torch.float32)
    cpu = torch.zeros(shape, dtype=torch.complex64)
    for f in (A.pauli_expectation_batch, A.pauli_sum_expectation_batch):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(cpu, [(1.0, "Z" * 8)] if f is A.pauli_sum_expectation_batch else "Z" * 8, [0])
    v = torch.zeros(4, dtype=torch.float64)
    with pytest.raises(TypeError, match="selector"):           # outcomes or the integer view of the records are no weights
        A.trajectory_mean(v, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="one entry per trajectory"):
        A.trajectory_mean(v, torch.zeros((4, 4), dtype=torch.float64))                      # the [B, 4] records
    with pytest.raises(ValueError, match="one entry per trajectory"):
        A.trajectory_mean(v, torch.zeros(3, dtype=torch.float64))
    with pytest.raises(TypeError, match="floating"):
        A.trajectory_mean([0.0, 1.0])


def test_complex_coefficients_are_refused_before_the_device(monkeypatch):
    monkeypatch.setattr(N, "require_gpu", lambda t, what: None)
    with pytest.raises(ValueError, match="real coefficients"):
        A.pauli_sum_expectation_batch(torch.zeros((2,) * 8, dtype=torch.complex64), [(1.0, "Z" * 8), (1j, "X" * 8)], [0])
    with pytest.raises(ValueError, match="at least one term"):
        A.pauli_sum_expectation_batch(torch.zeros((2,) * 8, dtype=torch.complex64), [], [0])


# ---- trajectory_mean ----------------------------------------------------------------------------------------------------------------
def test_trajectory_mean_agrees_with_numpy():
    rng = np.random.default_rng(8)
    for shape in ((64,), (64, 5)):
        v = rng.standard_normal(shape)
        mean, err = A.trajectory_mean(torch.from_numpy(v))
        assert np.allclose(mean.numpy(), v.mean(axis=0), rtol=0, atol=1e-15)
        assert np.allclose(err.numpy(), v.std(axis=0, ddof=1) / 8.0, rtol=1e-14, atol=0)
        w = rng.random(64)
        w[::5] = 0.0
        vn = v.copy()
        vn[::5] = np.nan                                       # dead trajectories: norm 0, value 0 / 0
        live = w != 0
        wb = w[live].reshape((-1,) + (1,) * (v.ndim - 1))
        want = (wb * v[live]).sum(axis=0) / w.sum()
        want_err = np.sqrt((wb ** 2 * (v[live] - want) ** 2).sum(axis=0)) / w.sum()
        mean, err = A.trajectory_mean(torch.from_numpy(vn), torch.from_numpy(w))
        assert np.isfinite(mean.numpy()).all() and np.isfinite(err.numpy()).all()
        assert np.allclose(mean.numpy(), want, rtol=0, atol=1e-15) and np.allclose(err.numpy(), want_err, rtol=1e-13, atol=0)
        ones, e1 = A.trajectory_mean(torch.from_numpy(v), torch.ones(64, dtype=torch.float64))
        assert np.allclose(ones.numpy(), v.mean(axis=0), rtol=0, atol=1e-15)
        assert np.allclose(e1.numpy(), v.std(axis=0, ddof=0) / 8.0, rtol=1e-13, atol=0)      # (equal weights: the ddof=0 form)


# ---- the exact-integer states ---------------------------------------------------------------------------------------------------------
def test_the_exact_states_stay_below_2_to_53():
    """Every case of test_pauli_batch_gpu.py that compares with ==: (local bits, bound on |re| and |im|)."""
    for M, bound in ((3, 2 ** 10), (4, 2 ** 10), (7, 2 ** 10), (9, 2 ** 10), (19, 2 ** 4)):
        assert PO.exact_bound(M, bound) < 2 ** 53, (M, bound)
    rng = np.random.default_rng(0)
    for kind in ("c64", "c128"):
        a = PO.exact_state(rng, (2,) * 9, kind)
        assert np.abs(a.real).max() <= 2 ** 10 and np.abs(a.imag).max() <= 2 ** 10 and np.abs(a.real).max() > 2 ** 9
        for p in ("XYZIXYZIX", "ZZZZZZZZZ", "YYIIIIIII", "IIIIIIIIY"):
            got, norm = PO.exact_oracle(a, p)
            want = PO.oracle(a, p)                             # the float oracle is exact here as well
            assert (got, norm) == want
