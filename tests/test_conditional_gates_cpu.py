"""Host-side checks of the conditional gates (artensor_amd/trajectories.py: conditional_gate_info, BatchConditionalGate,
apply_conditional_gate_batch_, correct_batch_; artn_cgate_batch_query / _pack / _apply): the symbols, the plan on random permuted
layouts (no batch bit and no high control in the tile, the tile count), the packed table followed tile by tile the way the kernel
follows it (every element with the wanted high control bits exactly once, every tile inside one trajectory, the trajectory the
batch fields give for the tile's first element), every refusal by its message, batch_dims=() against controlled_gate_info, and
the numpy oracle against an explicit Kronecker construction.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import trajectories as T
from artensor_amd._state import _packed

import conditional_gate_oracle as CO
import trajectories_oracle as TO
from test_gates_cpu import random_unitary
from test_pauli_apply_cpu import contiguous_strides, desc, ptr
from tile_table import cgate_fields as decode
from tile_table import follow_columns, insert_holes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, NODEVICE = -1, -2, -4
TB = {torch.complex64: 12, torch.complex128: 11}
LB = {torch.complex64: 4, torch.complex128: 3}
HEADER, CASES = 1000, 400
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Z = np.diag([1.0, -1.0]).astype(np.complex128)


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_cgate_batch_query", "artn_cgate_batch_pack", "artn_cgate_batch_apply"]
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    assert "#define ARTN_ABI_VERSION 9" in text and "#define ARTN_CGATE_BATCH_MAX_CASES 16" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert ctypes.sizeof(N.ArtnCgateBatchInfo) == ctypes.sizeof(N.ArtnCgateInfo) + 4 * 4 + 8 + 3 * 4 * N.BATCH_MAX_FIELDS
    assert N.CGATE_BATCH_CASES_BYTES == CASES == 8 * (2 + 3 * N.CGATE_BATCH_MAX_CASES)
    for name in ("BatchConditionalGate", "apply_conditional_gate_batch_", "conditional_gate_info", "correct_batch_"):
        assert getattr(A, name) is getattr(T, name) and name in T.__all__
    from artensor_amd import controlled
    assert not {"BatchConditionalGate", "correct_batch_"} & set(controlled.__all__)


# ---- layouts: dim d of extent 2 holds memory bit bit[d] ------------------------------------------------------------------------------
def strides_of(bit):
    return tuple(1 << b for b in bit)


def dims_for_bits(bit, bits):
    return [bit.index(b) for b in bits]


def layouts_and_gates(dtype):
    """(n_bits, bit, targets, controls, values, batch, cases): batch bits at or above the line, anywhere among the others."""
    rng = np.random.default_rng(31 if dtype == torch.complex64 else 32)
    lb = LB[dtype]
    for n_bits in range(7, 18):
        for t in range(1, 6):
            for mode in ("no batch", "one", "few", "many"):
                bit = [int(b) for b in rng.permutation(n_bits)]
                high = [b for b in range(n_bits) if b >= lb]
                room = n_bits - t
                nbb = {"no batch": 0, "one": 1, "few": min(3, len(high), room), "many": min(len(high), room, n_bits // 2)}[mode]
                bbits = [int(b) for b in rng.choice(high, size=nbb, replace=False)]
                free = [b for b in range(n_bits) if b not in bbits]
                if len(free) < t:
                    continue
                picked = [int(b) for b in rng.permutation(free)]
                c = int(rng.integers(0, min(len(free) - t, 4) + 1))
                tbits, cbits = picked[:t], picked[t:t + c]
                m = int(rng.integers(1, 5))
                cases = [(int(k), random_unitary(rng, 2 ** t)) for k in rng.choice(64, size=m, replace=False)]
                yield (n_bits, bit, dims_for_bits(bit, tbits), dims_for_bits(bit, cbits), [int(v) for v in rng.integers(0, 2, size=c)],
                       dims_for_bits(bit, bbits), cases)


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_plan_properties(dtype):
    elem = 8 if dtype == torch.complex64 else 16
    seen = set()
    for n_bits, bit, targets, controls, values, batch, cases in layouts_and_gates(dtype):
        shape, strides = (2,) * n_bits, strides_of(bit)
        info = A.conditional_gate_info(shape, strides, cases, targets, batch, controls, values, dtype)
        t, c, n = len(targets), len(controls), 2 ** n_bits
        tbits, cbits, bbits = [bit[d] for d in targets], [bit[d] for d in controls], [bit[d] for d in batch]
        assert info["target_bits"] == tuple(tbits) and info["control_bits"] == tuple(cbits) and (info["t"], info["c"], info["m"]) == (t, c, len(cases))
        high = [b for b in cbits if b >= LB[dtype]]
        assert info["c_high"] == len(high) and info["c_low"] == c - len(high)
        assert info["B"] == 2 ** len(batch) and info["batch_bits"] == len(batch) and info["keys"] == tuple(k for k, _ in cases)
        assert info["fields"] == TO.fields(shape, strides, batch)
        sub = n_bits - len(high) - len(batch)
        tb = min(TB[dtype], sub)
        others = [b for b in range(n_bits) if b not in tbits and b not in high and b not in bbits][:tb - t]
        assert info["tb"] == tb and info["tile_bits"] == sorted(tbits + others)
        assert not set(info["tile_bits"]) & set(bbits) and not set(info["tile_bits"]) & set(high)   # no batch bit, no high control
        assert all(b in info["tile_bits"] for b in cbits if b < LB[dtype])
        assert info["n_tiles"] * 2 ** tb * 2 ** len(high) == n                                      # n_tiles . 2^tb . 2^c_high == n
        assert info["grid"] == min(info["n_tiles"], 2048) and info["n_selected"] == n >> c
        assert info["bytes_read"] == info["bytes_written"] == (n >> len(high)) * elem
        assert info["lds_bytes"] == elem << tb and info["table_bytes"] == HEADER + CASES + len(cases) * 16 * 4 ** t
        assert not info["diagonal"]
        seen.add((len(batch) > 0, len(high) > 0, c > len(high), sub > TB[dtype]))
    assert {(True, True, True, False), (True, True, False, False), (True, False, False, False), (False, False, False, True)} <= seen, seen


def pack(shape, strides, cases, targets, batch, controls, values, dtype, mask=None):
    d, (t, tg, c, ct, vals, bt), (m, keys, mats, mask), info, _ = T._cgate_plan(shape, strides, dtype, cases, targets, batch, controls, values,
                                                                             mask, "test")
    return _packed(info, lambda *table: N.lib().artn_cgate_batch_pack(ctypes.byref(d), t, ptr(tg), c, ptr(ct), ptr(vals), bt.shape[0],
                                                                      ptr(bt) if bt.shape[0] else None, m, ptr(keys), mask, ptr(mats), *table))


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_the_packed_table_followed_as_the_kernel_follows_it(dtype):
    for n_bits, bit, targets, controls, values, batch, cases in layouts_and_gates(dtype):
        if n_bits > 15:
            continue
        shape, strides = (2,) * n_bits, strides_of(bit)
        table, info = pack(shape, strides, cases, targets, batch, controls, values, dtype)
        head, arr = decode(table[:HEADER])
        t, n, m = len(targets), 2 ** n_bits, len(cases)
        tbits, cbits = [bit[d] for d in targets], [bit[d] for d in controls]
        tb, gb = info.tile_bits, info.tile_bits - t
        assert table.nbytes == info.table_bytes
        assert (head["t"], head["tile_bits"], head["n_tiles"], head["segment"]) == (t, tb, info.n_tiles, info.segment)
        assert head["group_bits"] == gb and 1 << head["segment_bits"] == info.segment and head["flags"] == 0
        high_mask = sum(1 << b for b in cbits if b >= LB[dtype])
        high_want = sum(v << b for b, v in zip(cbits, values) if b >= LB[dtype])
        low_mask = sum(1 << b for b in cbits if b < LB[dtype])
        low_want = sum(v << b for b, v in zip(cbits, values) if b < LB[dtype])
        assert head["high_mask"] == high_mask and head["high_want"] == high_want
        holes = arr["hole_bit"][:head["n_holes"]]
        assert list(holes) == sorted(set(int(h) for h in holes)) and not arr["hole_bit"][head["n_holes"]:].any()
        tile_bits = [int(x).bit_length() - 1 for x in arr["mem_col"][:tb]]
        s = head["segment_bits"]
        assert set(int(h) for h in holes) == set(tile_bits[s:]) | {b for b in cbits if b >= LB[dtype]}
        mem, off, rest = follow_columns(tb, t, s, tuple(tbits), arr["target_bit"], arr["target_pos"], arr["swizzle"], arr["mem_col"],
                                        arr["lds_col"])
        # the walk: every element with the wanted high control bits, exactly once, all inside the state
        base = insert_holes(np.arange(info.n_tiles, dtype=np.int64) << s, holes) | high_want
        tiles = base[:, None] | mem[None, :]
        assert not (base[:, None] & mem[None, :]).any()
        every = tiles.reshape(-1)
        assert every.min() >= 0 and every.max() < n
        index = np.arange(n, dtype=np.int64)
        assert np.array_equal(np.sort(every), index[(index & high_mask) == high_want])
        # every tile lies in one trajectory: the one the batch fields give for its first element
        of_element = TO.batch_index(tiles, shape, strides, batch)
        assert (of_element == of_element[:, :1]).all()
        by_fields = np.zeros_like(base)
        for f in range(info.n_fields):
            by_fields |= ((base >> info.field_shift[f]) & ((1 << info.field_width[f]) - 1)) << info.field_pos[f]
        assert np.array_equal(by_fields, of_element[:, 0]) and set(by_fields.tolist()) == set(range(info.B))
        # the group mask passes exactly the groups whose low control bits are right
        g = np.arange(2 ** gb, dtype=np.int64)
        passes = (g & head["group_mask"]) == head["group_want"]
        assert np.array_equal(passes, (rest[0] & low_mask) == low_want)
        computed = (base[:, None, None] | off[None, :, passes]).reshape(-1)
        cmask, cwant = high_mask | low_mask, high_want | low_want
        assert np.array_equal(np.sort(computed), index[(index & cmask) == cwant]) and computed.size == info.n_selected
        # the cases: m, keys, flags, block masks, then the matrices
        w = table[HEADER:HEADER + CASES].view(np.int64)
        assert int(w[0]) == m and int(w[1]) == 0 and list(w[2:2 + m]) == [k for k, _ in cases] and (w[2 + m:18] == -1).all()
        assert not w[18:34].any()
        full = (1 << max(1, 2 ** t // 8) ** 2) - 1
        assert list(w[34:34 + m]) == [full] * m and not w[34 + m:50].any() and head["block_mask"] == full
        mats = table[HEADER + CASES:].view(np.float64).reshape(m, 2 ** t, 2 ** t, 2)
        for j, (_, u) in enumerate(cases):
            assert np.array_equal(mats[j, ..., 0] + 1j * mats[j, ..., 1], u)
    # the flags: the identity and a diagonal case
    shape = (2,) * 8
    table, info = pack(shape, contiguous_strides(shape), [(0, np.eye(2)), (1, Z), (2, X)], [7], [0, 1], (), None, torch.complex64)
    w = table[HEADER:HEADER + CASES].view(np.int64)
    assert list(w[18:21]) == [N.CGATE_CASE_DIAGONAL | N.CGATE_CASE_IDENTITY, N.CGATE_CASE_DIAGONAL, 0] and info.diagonal == 0
    assert decode(table[:HEADER])[0]["flags"] == 0
    table, info = pack(shape, contiguous_strides(shape), [(0, np.eye(2)), (1, Z)], [7], [0, 1], (), None, torch.complex64)
    assert info.diagonal == 1 and decode(table[:HEADER])[0]["flags"] == N.GATE_DIAGONAL


def test_without_batch_dims_the_plan_is_the_controlled_gates():
    rng = np.random.default_rng(5)
    for dtype in (torch.complex64, torch.complex128):
        for n_bits in (3, 9, 14):
            bit = [int(b) for b in rng.permutation(n_bits)]
            shape, strides = (2,) * n_bits, strides_of(bit)
            u = random_unitary(rng, 4)
            targets, controls = (0, 2), (1,)
            one = A.controlled_gate_info(shape, strides, u, targets, controls, [0], dtype)
            two = A.conditional_gate_info(shape, strides, {3: u}, targets, (), controls, [0], dtype)
            for key in ("t", "c", "c_high", "c_low", "target_bits", "control_bits", "control_values", "tile_bits", "tb", "n_selected", "n_tiles",
                        "segment", "lds_bytes", "bytes_read", "bytes_written", "diagonal"):
                assert one[key] == two[key], key
            assert two["B"] == 1 and two["fields"] == [] and two["table_bytes"] == one["table_bytes"] + CASES


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_by_its_message():
    shape = (4, 2) + (2,) * 9                                  # dims 0 and 1: memory bits 9..10 and 8; dim 10: memory bit 0
    strides = contiguous_strides(shape)
    info = lambda cases, targets, batch, **k: A.conditional_gate_info(shape, strides, cases, targets, batch, **k)
    assert info({1: X}, [5], [0, 1], controls=[2, 10])["B"] == 8
    with pytest.raises(RuntimeError, match="artn error -1.*dimension 5 is both a batch dimension and a target one"):
        info({1: X}, [5], [5])
    with pytest.raises(RuntimeError, match="artn error -1.*dimension 2 is both a batch dimension and a control one"):
        info({1: X}, [5], [0, 2], controls=[2])
    with pytest.raises(RuntimeError, match="artn error -1.*the batch dimensions must differ; dimension 0 is repeated"):
        info({1: X}, [5], [0, 0])
    with pytest.raises(RuntimeError, match="artn error -1.*batch dimension 11 out of range"):
        info({1: X}, [5], [11])
    with pytest.raises(RuntimeError, match="artn error -2.*batch dimension 10 holds memory bit 0, below a 128-byte line"):
        info({1: X}, [5], [10])
    with pytest.raises(RuntimeError, match=r"artn error -2.*batch dimension 7 holds memory bit 3, below a 128-byte line \(bit 4"):
        info({1: X}, [5], [7])
    assert info({1: X}, [5], [7], dtype=torch.complex128)["B"] == 2    # (bit 3 is the line of complex128)
    big = (2,) * 30
    with pytest.raises(RuntimeError, match="artn error -2.*at most 24 batch bits; these dimensions have 25"):
        A.conditional_gate_info(big, contiguous_strides(big), {1: X}, [29], list(range(25)))
    assert A.conditional_gate_info(big, contiguous_strides(big), {1: X}, [29], list(range(24)))["B"] == 2 ** 24
    with pytest.raises(RuntimeError, match="artn error -1.*a conditional gate has 1 to 16 cases, not 0"):
        info({}, [5], [0])
    with pytest.raises(RuntimeError, match="artn error -1.*a conditional gate has 1 to 16 cases, not 17"):
        info({k: X for k in range(17)}, [5], [0])
    assert info({k: X for k in range(16)}, [5], [0])["m"] == 16
    with pytest.raises(RuntimeError, match="artn error -1.*the keys must differ; key 6 is repeated"):
        info([(6, X), (2, Z), (6, Z)], [5], [0])
    with pytest.raises(RuntimeError, match=r"artn error -1.*the key of case 1 \(4\) has bits outside the mask"):
        info([(1, X), (4, Z)], [5], [0], mask=3)
    bad = X.copy()
    bad[0, 1] = np.inf
    with pytest.raises(RuntimeError, match="artn error -1.*an entry of the matrix of case 1 is not finite"):
        info([(1, X), (2, bad)], [5], [0])
    with pytest.raises(RuntimeError, match=r"artn error -1.*needs a trajectory of at least 2\^3 elements once the controls are taken out"):
        A.conditional_gate_info((2, 2), (1, 2), {1: np.eye(8)}, [0, 1, 0], ())
    with pytest.raises(RuntimeError, match=r"artn error -1.*a gate on 1 dimensions under 1 controls needs a trajectory of at least 2\^1"):
        A.conditional_gate_info((2, 2, 2), (4, 2, 1), {1: X}, [1], [0, 2], controls=[0])
    # the refusals of the controlled gates, in this family's wording where it is a family's
    with pytest.raises(RuntimeError, match="artn error -2.*conditional gates act on one to five target"):
        info({1: np.eye(64)}, range(2, 8), [0])
    with pytest.raises(RuntimeError, match="artn error -1.*repeated"):
        info({1: X}, [5], [0], controls=[3, 3])
    with pytest.raises(RuntimeError, match="artn error -2.*conditional gates take power-of-two"):
        A.conditional_gate_info((2, 3, 2), (1, 2, 6), {1: X}, [0], ())
    # Python's own: keys and mask are integers in range, the control values fit
    with pytest.raises(TypeError, match="a key must be an integer"):
        info({1.5: X}, [5], [0])
    with pytest.raises(ValueError, match=r"a key must lie in 0 \.\. 2\^63 - 1"):
        info({-1: X}, [5], [0])
    with pytest.raises(ValueError, match="mask must lie"):
        info({1: X}, [5], [0], mask=2 ** 63)
    with pytest.raises(ValueError, match=r"dims \[5\] are listed as targets and as controls"):
        info({1: X}, [5], [0], controls=[5])
    with pytest.raises(ValueError, match="entries"):
        info({1: np.eye(4)}, [5], [0])
    # the selector: the raw query takes its address and its stride (never read: any address will do)
    d = desc(shape, strides)
    targets, batch, keys = (np.array(x, dtype=np.int32) for x in ([5], [0], [1]))
    keys = keys.astype(np.int64)
    mats = np.zeros(8)
    out = N.ArtnCgateBatchInfo()
    q = lambda sel, stride: N.lib().artn_cgate_batch_query(ctypes.byref(d), 1, ptr(targets), 0, None, None, 1, ptr(batch), 1, ptr(keys), -1,
                                                           ptr(mats), ctypes.c_void_p(sel), stride, ctypes.byref(out), None, None, None)
    assert q(4096, 1) == 0 and q(4096 + 8, 4) == 0 and q(0, 1) == 0
    assert q(4096 + 4, 1) == UNSUPPORTED and b"8-byte aligned selector" in N.lib().artn_last_error()
    assert q(4096, 0) == INVALID and b"a selector stride of at least one 8-byte word is needed, not 0" in N.lib().artn_last_error()
    assert q(4096, -4) == INVALID and b"selector stride" in N.lib().artn_last_error()


def test_apply_runs_nowhere_without_a_gpu_and_python_checks_the_selector_on_the_host():
    shape = (2,) * 8
    t = torch.zeros(shape, dtype=torch.complex64)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            A.apply_conditional_gate_batch_(t, {1: X}, [7], [0], torch.zeros(2, dtype=torch.int64))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            A.BatchConditionalGate(shape, t.stride(), t.dtype, {1: X}, [7], [0], "cpu")
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            A.correct_batch_(t, 7, [0], torch.zeros(2, dtype=torch.int64), x_bit=0)

    class FakeGpu(torch.Tensor):                               # a host tensor that claims to live on the device
        is_cuda = True

    fake = lambda x: x.as_subclass(FakeGpu)
    dev = torch.device("cpu")
    sel = lambda x, B=4: T._selector(x, B, dev, "test")
    with pytest.raises(TypeError, match="GPU tensor"):
        sel([0, 1, 2, 3])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        sel(torch.zeros(4, dtype=torch.int64))
    with pytest.raises(TypeError, match="int64 selector"):
        sel(fake(torch.zeros(4, dtype=torch.int32)))
    with pytest.raises(ValueError, match="of 4 elements, one per trajectory"):
        sel(fake(torch.zeros(5, dtype=torch.int64)))
    with pytest.raises(ValueError, match="records"):
        sel(fake(torch.zeros(4, 3, dtype=torch.float64)))
    with pytest.raises(ValueError, match="selector stride"):
        sel(fake(torch.zeros(1, dtype=torch.int64).expand(4)))
    rec = torch.zeros(4, 4, dtype=torch.float64)
    assert sel(fake(rec)) == (rec.data_ptr(), 4)
    assert sel(fake(rec.view(torch.int64)[:, 0])) == (rec.data_ptr(), 4)           # the view measure_batch_ returns: no copy
    word = torch.zeros(6, dtype=torch.int64)
    assert sel(fake(word[1:5])) == (word.data_ptr() + 8, 1)
    assert sel(fake(word[:1]), B=1) == (word.data_ptr(), 1) and sel(fake(rec[:1]), B=1) == (rec.data_ptr(), 4)
    # correct_batch_: the bits
    g = fake(torch.zeros(2, dtype=torch.int64))
    for kw, text in ((dict(), "x_bit or z_bit is needed"), (dict(x_bit=1, z_bit=1), "different bits"), (dict(x_bit=63), "different bits")):
        with pytest.raises(ValueError, match=text):
            A.correct_batch_(t, 7, [0], g, **kw)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------------
def kron_embedded(n, u, targets, controls, values):
    """The 2^n x 2^n matrix of u on `targets` under `controls` == `values` (dim 0 the most significant bit), element by element."""
    t = len(targets)
    full = np.zeros((2 ** n, 2 ** n), dtype=np.complex128)
    digit = lambda i, d: (i >> (n - 1 - d)) & 1
    for col in range(2 ** n):
        if any(digit(col, d) != v for d, v in zip(controls, values)):
            full[col, col] = 1
            continue
        c = sum(digit(col, d) << (t - 1 - k) for k, d in enumerate(targets))
        for r in range(2 ** t):
            row = col
            for k, d in enumerate(targets):
                row = (row & ~(1 << (n - 1 - d))) | (((r >> (t - 1 - k)) & 1) << (n - 1 - d))
            full[row, col] = u[r, c]
    return full


def test_the_oracle_against_an_explicit_kronecker_construction():
    rng = np.random.default_rng(9)
    n = 6
    # the embedding itself, against numpy's kron where the targets are adjacent and in order
    u2 = random_unitary(rng, 4)
    assert np.allclose(kron_embedded(4, u2, [1, 2], [], []), np.kron(np.kron(np.eye(2), u2), np.eye(2)))
    psi = rng.standard_normal((2,) * (n + 2)) + 1j * rng.standard_normal((2,) * (n + 2))
    batch = [6, 1]                                             # trajectory b = 2 * digit(dim 6) + digit(dim 1)
    rest = [d for d in range(n + 2) if d not in batch]
    for targets, controls, values in (([0], [], []), ([4, 2], [7], [0]), ([7, 0, 3], [5, 2], [1, 0])):
        t = len(targets)
        cases = [(2, random_unitary(rng, 2 ** t)), (1, np.eye(2 ** t)), (5, random_unitary(rng, 2 ** t))]
        selector = np.array([6, -1, 5, 3], dtype=np.int64)     # mask 3: case 2, dead, case 1 (the identity), no match
        got = CO.conditional_oracle(psi, selector, cases, targets, batch, controls, values, mask=3)
        sl = TO.slices(psi, batch)
        sub = lambda dims: [rest.index(d) for d in dims]
        want = sl.copy()
        want[0] = (kron_embedded(n, cases[0][1], sub(targets), sub(controls), values) @ sl[0].reshape(-1)).reshape(sl[0].shape)
        assert np.allclose(TO.slices(got, batch), want, atol=1e-13)
        assert np.array_equal(TO.slices(got, batch)[1:], sl[1:]) and not np.allclose(got, psi)
        got = CO.conditional_oracle(psi, selector, cases, targets, batch, controls, values)          # all bits: 5 matches, 6 and 3 do not
        want = sl.copy()
        want[2] = (kron_embedded(n, cases[2][1], sub(targets), sub(controls), values) @ sl[2].reshape(-1)).reshape(sl[2].shape)
        assert np.allclose(TO.slices(got, batch), want, atol=1e-13)
    assert CO.case_of(-1, cases) is None and CO.case_of(7, cases, 5) == 2 and CO.is_identity(np.eye(4)) and not CO.is_identity(X)
