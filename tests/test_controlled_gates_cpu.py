"""Host-side checks of the controlled gates (artensor_amd/controlled.py: controlled_gate_info, ControlledGate, when, mcx_ ...;
artn_cgate_query / _pack / _apply): the symbols, every refusal with its code and a word of its text, the Python-side
validation, the properties of the plan on random permuted layouts (low / high controls by the 128-byte line, tiles, bytes,
segments), and the packed table followed index by index the way the kernel follows it: the addresses visited are exactly the
elements whose high control bits are the wanted ones, each once; the LDS image is a bijection; the groups that pass the mask
are those whose low control bits are right; rows lie where the first-listed-is-most-significant convention puts them; with no
control the walk is the wide gate's.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import controlled as CG
from test_gates_cpu import random_unitary
from test_pauli_apply_cpu import contiguous_strides, desc, ptr
from test_wide_gates_cpu import pack as wide_pack
from test_wide_gates_cpu import random_layout
from tile_table import cgate_fields as decode
from tile_table import follow_columns, insert_holes, xor_cols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED, NODEVICE = -1, -2, -4
TB = {torch.complex64: 12, torch.complex128: 11}
LB = {torch.complex64: 4, torch.complex128: 3}
HEADER = 1000


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_cgate_query", "artn_cgate_pack", "artn_cgate_apply"]
    assert N.ABI_VERSION == 9 and N.lib().artn_abi_version() == 9
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    assert "#define ARTN_ABI_VERSION 9" in text and "#define ARTN_CGATE_MAX_HOLES 64" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert ctypes.sizeof(N.ArtnCgateInfo) == 6 * 4 + 7 * 8
    assert N.CGATE_TABLE_HEADER_BYTES == HEADER == 8 * (13 + 3 * 5 + 2 * 16 + N.CGATE_MAX_HOLES + 1)
    for name in ("apply_controlled_gate_", "ControlledGate", "controlled_gate_info", "mcx_", "mcz_", "mcphase_", "when"):
        assert getattr(A, name) is getattr(CG, name)
    assert A.controlled is CG


def query_rc(shape, strides, targets, controls=(), values=None, mat=None, dtype=N.ARTN_C64, t=None, c=None, info=True,
             null=()):
    t = len(targets) if t is None else t
    c = len(controls) if c is None else c
    targets = np.asarray(list(targets) + [0] * 8, dtype=np.int32)
    controls = np.asarray(list(controls) + [0] * 8, dtype=np.int32)
    values = np.asarray(([1] * max(c, 0) if values is None else list(values)) + [1] * 8, dtype=np.int32)
    if mat is None:
        mat = np.zeros(2 * 4 ** max(min(t, 5), 1))
        mat[0] = 1
    out = N.ArtnCgateInfo()
    return N.lib().artn_cgate_query(ctypes.byref(desc(shape, strides, dtype)), t, None if "targets" in null else ptr(targets), c,
                                    None if "controls" in null else ptr(controls), None if "values" in null else ptr(values),
                                    None if "mat" in null else ptr(mat), ctypes.byref(out) if info else None, None, None, None)


def last_error():
    return N.lib().artn_last_error()


def test_the_refusals_and_their_error_codes():
    shape, strides = (2, 2, 4, 2, 2, 2), (1, 2, 4, 16, 32, 64)
    assert query_rc(shape, strides, [0, 1], [3, 4, 5]) == 0
    assert query_rc(shape, strides, [5, 0, 4, 1, 3]) == 0
    assert query_rc(shape, strides, [0], [1, 3, 4, 5], [0, 1, 0, 1]) == 0
    assert query_rc(shape, strides, [0], [1], null=("values",)) == 0                       # NULL values: all 1
    assert query_rc(shape, strides, [0], [], null=("controls", "values")) == 0             # c = 0 needs no control array
    # t outside 1..5
    assert query_rc(shape, strides, [0, 1, 3, 4, 5, 0], t=6) == UNSUPPORTED and b"one to five target" in last_error()
    assert query_rc(shape, strides, [], t=0) == UNSUPPORTED and b"one to five target" in last_error()
    assert query_rc((2, 2), (1, 2), [0, 1, 0], t=3) == INVALID and b"at least 2^3" in last_error()
    # c < 0
    assert query_rc(shape, strides, [0], [], c=-1) == INVALID and b"negative" in last_error()
    # dims: out of range, repeated, shared, of another extent -- among the targets and among the controls
    assert query_rc(shape, strides, [0, 6]) == INVALID and b"out of range" in last_error()
    assert query_rc(shape, strides, [0], [1, -1]) == INVALID and b"out of range" in last_error()
    assert query_rc(shape, strides, [0], [6]) == INVALID and b"out of range" in last_error()
    assert query_rc(shape, strides, [0, 1, 1]) == INVALID and b"repeated" in last_error()
    assert query_rc(shape, strides, [0], [1, 3, 1]) == INVALID and b"repeated" in last_error()
    assert query_rc(shape, strides, [0, 1], [3, 1]) == INVALID and b"both a target and a control" in last_error()
    assert query_rc(shape, strides, [0, 2]) == INVALID and b"extent 4" in last_error()
    assert query_rc(shape, strides, [0], [2]) == INVALID and b"extent 4" in last_error()
    # a control value other than 0 / 1
    for bad in (2, -1):
        assert query_rc(shape, strides, [0], [1, 3], [1, bad]) == INVALID and b"control value" in last_error()
    # a matrix entry that is not finite
    for bad in (np.nan, np.inf, -np.inf):
        mat = np.zeros(2 * 16)
        mat[13] = bad
        assert query_rc(shape, strides, [0, 1], [3], mat=mat) == INVALID and b"finite" in last_error()
    # null pointers
    assert query_rc(shape, strides, [0, 1], [3], info=False) == INVALID and b"null" in last_error()
    for which in ("targets", "controls", "mat"):
        assert query_rc(shape, strides, [0, 1], [3], null=(which,)) == INVALID and b"null" in last_error(), which
    assert N.lib().artn_cgate_query(None, 1, None, 0, None, None, None, ctypes.byref(N.ArtnCgateInfo()), None, None, None) == INVALID
    # the layout and dtype refusals, in the wording of the family
    assert query_rc(shape, strides, [0], [1], dtype=N.ARTN_C64_BF16) == UNSUPPORTED and b"controlled gates take complex64 or complex128" in last_error()
    assert query_rc(shape, (1, 2, 4, 16, 32, 128), [0], [1]) == INVALID and b"not dense" in last_error()
    assert query_rc((2, 3, 2, 2), (1, 2, 6, 12), [0], [2]) == UNSUPPORTED and b"controlled gates take power-of-two" in last_error()
    # pack: a table that is too small, misaligned or null
    d = desc(shape, strides)
    targets, controls, values = (np.array(x, dtype=np.int32) for x in ([0, 1], [3, 5], [1, 0]))
    mat = np.zeros(2 * 16)
    info = N.ArtnCgateInfo()
    args = (ctypes.byref(d), 2, ptr(targets), 2, ptr(controls), ptr(values))
    assert N.lib().artn_cgate_query(*args, ptr(mat), ctypes.byref(info), None, None, None) == 0
    assert info.table_bytes == HEADER + 16 * 16 and (info.t, info.c, info.c_high, info.c_low, info.diagonal) == (2, 2, 2, 0, 1)
    buf = np.zeros(info.table_bytes // 8 + 2, dtype=np.uint64)
    assert N.lib().artn_cgate_pack(*args, ptr(mat), ptr(buf), info.table_bytes - 1) == INVALID and b"smaller" in last_error()
    assert N.lib().artn_cgate_pack(*args, ptr(mat), ctypes.c_void_p(buf.ctypes.data + 4), info.table_bytes) == UNSUPPORTED
    assert b"8-byte aligned table" in last_error()
    assert N.lib().artn_cgate_pack(*args, ptr(mat), None, info.table_bytes) == INVALID and b"null" in last_error()
    assert N.lib().artn_cgate_pack(*args, None, ptr(buf), info.table_bytes) == INVALID and b"null" in last_error()
    assert N.lib().artn_cgate_pack(*args, ptr(mat), ptr(buf), info.table_bytes) == 0


def test_apply_refuses_bad_pointers_and_runs_nowhere_without_a_gpu():
    """Every call here is refused before anything is launched, so host addresses are safe to pass."""
    shape, strides = (2, 2, 2), (4, 2, 1)
    d = desc(shape, strides)
    targets, controls, values = (np.array(x, dtype=np.int32) for x in ([0, 2], [1], [1]))
    buf = np.zeros(512, dtype=np.complex128)
    base = (buf.ctypes.data + 15) & ~15
    a, table, cond, nbytes = base, base + 256, base + 4096, HEADER + 16 * 16
    cases = {"small table": (a, table, nbytes - 1, cond, INVALID, b"smaller"), "null array": (0, table, nbytes, cond, INVALID, b"null"),
             "null table": (a, 0, nbytes, cond, INVALID, b"null"),
             "misaligned array": (a + 8, table, nbytes, cond, UNSUPPORTED, b"16-byte aligned array"),
             "misaligned table": (a, table + 4, nbytes, cond, UNSUPPORTED, b"8-byte aligned table"),
             "misaligned condition": (a, table, nbytes, cond + 4, UNSUPPORTED, b"8-byte aligned condition")}
    gpu = N.lib().artn_device_count() > 0
    for name, (pa, pt, nb, pc, want, word) in cases.items():
        rc = N.lib().artn_cgate_apply(ctypes.byref(d), ctypes.c_void_p(pa), 2, ptr(targets), 1, ptr(controls), ptr(values),
                                      ctypes.c_void_p(pt), nb, ctypes.c_void_p(pc), 1, 1, None)
        assert rc == (want if gpu else NODEVICE), name
        assert (word if gpu else b"gfx950") in last_error(), name
    t = torch.zeros((2,) * 4, dtype=torch.complex64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_controlled_gate_(t, np.eye(2), (0,), (1, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.mcx_(t, (1, 2), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.mcz_(t, (1, 2, 0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.mcphase_(t, (1, 2, 0), 0.3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.ControlledGate(t.shape, t.stride(), t.dtype, np.eye(2), (0,), (1, 2), "cpu")


def test_python_side_validation_without_a_device():
    shape = (2,) * 6
    strides = contiguous_strides(shape)
    t = torch.zeros(shape, dtype=torch.complex64)
    info = lambda *a, **k: A.controlled_gate_info(shape, strides, *a, **k)
    # control_values: length and range, as a list and as an int
    with pytest.raises(ValueError, match="2 control_values for 3 controls"):
        info(np.eye(2), (0,), (1, 2, 3), [1, 0])
    with pytest.raises(ValueError, match="0 or 1"):
        info(np.eye(2), (0,), (1, 2, 3), [1, 2, 0])
    with pytest.raises(ValueError, match="does not fit 3 controls"):
        info(np.eye(2), (0,), (1, 2, 3), 8)
    with pytest.raises(ValueError, match="does not fit"):
        info(np.eye(2), (0,), (1, 2, 3), -1)
    assert info(np.eye(2), (0,), (1, 2, 3), 0b110)["control_values"] == (1, 1, 0)        # the first listed control: the top digit
    assert info(np.eye(2), (0,), (1, 2, 3))["control_values"] == (1, 1, 1)
    assert info(np.eye(2), (0,), (1, 2, 3), [0, 1, 0])["control_values"] == (0, 1, 0)
    assert info(np.eye(2), (0,), ())["c"] == 0 and info(np.eye(2), (0,), None)["c"] == 0
    # targets overlapping controls; negative dims count from the end
    with pytest.raises(ValueError, match=r"dims \[2\] are listed as targets and as controls"):
        info(np.eye(4), (0, 2), (1, -4))
    assert info(np.eye(4), (-1, 0), (-2,))["target_bits"] == (0, 5) and info(np.eye(4), (-1, 0), (-2,))["control_bits"] == (1,)
    # the same errors come from the apply call before the device is asked for
    with pytest.raises(ValueError, match="control_values for"):
        A.apply_controlled_gate_(t, np.eye(2), (0,), (1, 2), [1])
    with pytest.raises(ValueError, match="targets and as controls"):
        A.apply_controlled_gate_(t, np.eye(2), (0,), (0, 1))
    with pytest.raises(ValueError, match="entries"):
        info(np.eye(4), (0,), (1,))
    with pytest.raises(TypeError):
        info(np.eye(2), (0,), (1,), dtype=torch.float32)
    with pytest.raises(RuntimeError, match="artn error -2.*one to five target"):
        info(np.eye(64), range(6), ())
    with pytest.raises(RuntimeError, match="artn error -1.*repeated"):
        info(np.eye(2), (0,), (1, 1))
    # when(): host-only validation
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.when(torch.zeros((), dtype=torch.int64), 1)
    with pytest.raises(TypeError, match="GPU tensor"):
        A.when(3, 1)

    class FakeGpu(torch.Tensor):                                            # a host tensor that claims to live on the device
        is_cuda = True

    def fake(x):
        return x.as_subclass(FakeGpu)

    with pytest.raises(TypeError, match="int64"):
        A.when(fake(torch.zeros(1, dtype=torch.int32)), 1)
    with pytest.raises(TypeError, match="record"):
        A.when(fake(torch.zeros(3, dtype=torch.float64)), 1)
    with pytest.raises(ValueError, match="no element"):
        A.when(fake(torch.zeros(0, dtype=torch.int64)), 1)
    ok = fake(torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="outside mask"):
        A.when(ok, 3, mask=1)
    with pytest.raises(ValueError, match="equals must lie"):
        A.when(ok, -1)
    with pytest.raises(ValueError, match="mask must lie"):
        A.when(ok, 0, mask=-2)
    with pytest.raises(TypeError, match="integer"):
        A.when(ok, 1.0)
    cond = A.when(ok, 2, mask=6)
    assert (cond.mask, cond.equals) == (6, 2) and cond.tensor is ok
    assert A.when(ok, 5).mask == -1
    assert A.when(fake(torch.zeros(4, dtype=torch.float64)), 0, mask=1).mask == 1


def random_controlled(rng, shape, strides, t, c):
    twos = [d for d, e in enumerate(shape) if e == 2]
    picked = [int(x) for x in rng.choice(twos, size=t + c, replace=False)]
    return random_unitary(rng, 2 ** t), tuple(picked[:t]), tuple(picked[t:]), [int(v) for v in rng.integers(0, 2, size=c)]


def layouts_and_gates():
    rng = np.random.default_rng(21)
    for n_bits in range(6, 17):
        for t in range(1, 6):
            for mode in ("none", "few", "many", "all"):
                shape, strides = random_layout(rng, n_bits)
                twos = sum(e == 2 for e in shape)
                if twos < t:
                    continue
                c = {"none": 0, "few": min(twos - t, int(rng.integers(1, 4))), "many": (twos - t + 1) // 2, "all": twos - t}[mode]
                yield n_bits, shape, strides, random_controlled(rng, shape, strides, t, c)


def bits_of_dims(strides, dims):
    return tuple(int(strides[d]).bit_length() - 1 for d in dims)


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_plan_properties(dtype):
    seen = set()
    elem = 8 if dtype == torch.complex64 else 16
    for n_bits, shape, strides, (m, targets, controls, values) in layouts_and_gates():
        info = A.controlled_gate_info(shape, strides, m, targets, controls, values, dtype)
        t, c, n = len(targets), len(controls), 2 ** n_bits
        tbits, cbits = bits_of_dims(strides, targets), bits_of_dims(strides, controls)
        assert info["target_bits"] == tbits and info["control_bits"] == cbits and (info["t"], info["c"]) == (t, c)
        high = [b for b in cbits if b >= LB[dtype]]                          # the classification follows the 128-byte line
        assert info["c_high"] == len(high) and info["c_low"] == c - len(high)
        sub = n_bits - len(high)
        tb = min(TB[dtype], sub)
        others = [b for b in range(n_bits) if b not in tbits and b not in high][:tb - t]
        assert info["tb"] == tb and info["tile_bits"] == sorted(list(tbits) + others)
        assert all(b in info["tile_bits"] for b in cbits if b < LB[dtype])  # a low control is an index bit of the tile
        assert info["n_tiles"] << tb == n >> len(high) and (sub > TB[dtype] or info["n_tiles"] == 1)
        assert info["n_selected"] == n >> c
        assert info["bytes_read"] == info["bytes_written"] == (n >> len(high)) * elem
        seg = info["segment"]
        s = seg.bit_length() - 1
        assert seg & (seg - 1) == 0 and info["tile_bits"][:s] == list(range(s)) and (s == tb or info["tile_bits"][s] != s)
        assert seg * elem >= min(128, elem << tb)                            # runs of a line, where the sub-state has one
        assert info["lds_bytes"] == elem << tb <= 32 * 1024 and info["table_bytes"] == HEADER + 16 * 4 ** t
        assert not info["diagonal"] and A.controlled_gate_info(shape, strides, np.diag(np.diag(m)), targets, controls, values, dtype)["diagonal"]
        seen.add((t, len(high) > 0, c > len(high), sub > TB[dtype]))
    for t in range(1, 6):
        assert {(t, True, True, False), (t, True, False, False), (t, False, False, True), (t, True, False, True)} <= {s for s in seen if s[0] == t}, t


def pack(shape, strides, m, targets, controls, values, dtype):
    t, targets, c, controls, values, mat = CG._split(m, targets, controls, values, len(shape), "test")
    return CG._cgate_pack(CG._desc(shape, strides, dtype), t, targets, c, controls, values, mat)


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_the_packed_table_followed_as_the_kernel_follows_it(dtype):
    for n_bits, shape, strides, (m, targets, controls, values) in layouts_and_gates():
        table, info = pack(shape, strides, m, targets, controls, values, dtype)
        head, arr = decode(table)
        t, n = len(targets), 2 ** n_bits
        tbits, cbits = bits_of_dims(strides, targets), bits_of_dims(strides, controls)
        tb, gb = info.tile_bits, info.tile_bits - t
        assert table.nbytes == info.table_bytes == HEADER + 16 * 4 ** t
        assert (head["t"], head["tile_bits"], head["n_tiles"], head["segment"]) == (t, tb, info.n_tiles, info.segment)
        assert head["group_bits"] == gb and 1 << head["segment_bits"] == info.segment and head["flags"] == 0
        high_mask = sum(1 << b for b in cbits if b >= LB[dtype])
        high_want = sum(v << b for b, v in zip(cbits, values) if b >= LB[dtype])
        low_mask = sum(1 << b for b in cbits if b < LB[dtype])
        low_want = sum(v << b for b, v in zip(cbits, values) if b < LB[dtype])
        assert head["high_mask"] == high_mask and head["high_want"] == high_want
        mem_col, lds_col, swizzle = arr["mem_col"], arr["lds_col"], arr["swizzle"]
        holes = arr["hole_bit"][:head["n_holes"]]
        assert list(holes) == sorted(set(int(h) for h in holes)) and not arr["hole_bit"][head["n_holes"]:].any()
        tile_bits = [int(c).bit_length() - 1 for c in mem_col[:tb]]
        s = head["segment_bits"]
        assert set(int(h) for h in holes) == set(tile_bits[s:]) | {b for b in cbits if b >= LB[dtype]}
        mem, off, rest = follow_columns(tb, t, s, tbits, arr["target_bit"], arr["target_pos"], swizzle, mem_col, lds_col)
        # the walk: exactly the elements whose high control bits are the wanted ones, each once, all inside the state
        base = insert_holes(np.arange(info.n_tiles, dtype=np.int64) << s, holes) | high_want
        every = (base[:, None] | mem[None, :]).reshape(-1)
        assert not (base[:, None] & mem[None, :]).any()
        assert every.min() >= 0 and every.max() < n
        index = np.arange(n, dtype=np.int64)
        assert np.array_equal(np.sort(every), index[(index & high_mask) == high_want])
        # the group mask passes exactly the groups whose low control bits are right
        g = np.arange(2 ** gb, dtype=np.int64)
        passes = (g & head["group_mask"]) == head["group_want"]
        assert np.array_equal(passes, (rest[0] & low_mask) == low_want)
        assert bin(head["group_mask"]).count("1") == info.c_low and head["group_want"] & ~head["group_mask"] == 0
        # so the elements computed are exactly the selected ones
        computed = (base[:, None, None] | off[None, :, passes]).reshape(-1)
        cmask, cwant = high_mask | low_mask, high_want | low_want
        assert np.array_equal(np.sort(computed), index[(index & cmask) == cwant]) and computed.size == info.n_selected
        mat = table[HEADER:].view(np.float64).reshape(2 ** t, 2 ** t, 2)
        assert np.array_equal(mat[..., 0] + 1j * mat[..., 1], m)
        assert head["block_mask"] == (1 << max(1, 2 ** t // 8) ** 2) - 1
        # no control: the wide gate's walk, field by field
        if not controls:
            wt, winfo = wide_pack(shape, strides, m, targets, dtype)
            ww = wt.view(np.uint64)
            assert [int(x) for x in ww[:4]] == [t, tb, info.n_tiles, info.segment] and int(ww[7]) == head["block_mask"]
            assert np.array_equal(ww[8:13].astype(np.int64), arr["target_bit"]) and np.array_equal(ww[13:18].astype(np.int64), arr["target_pos"])
            assert np.array_equal(ww[23:28].astype(np.int64), swizzle)
            assert np.array_equal(ww[28:44].astype(np.int64), mem_col) and np.array_equal(ww[44:60].astype(np.int64), lds_col)
            n_high = int(ww[6])
            assert list(ww[18:18 + n_high].astype(np.int64)) == list(holes) and tb - n_high == s
            assert head["group_mask"] == 0 and head["high_mask"] == 0 and np.array_equal(wt[480:], table[HEADER:])
    table, _ = pack((2,) * 7, contiguous_strides((2,) * 7), np.eye(32), range(5), (5, 6), None, dtype)
    assert decode(table)[0]["block_mask"] == 0b1000_0100_0010_0001 and decode(table)[0]["flags"] == N.GATE_DIAGONAL


def test_high_controls_at_the_top_of_a_large_state():
    """The plan of the 2^32 test: 19 high controls on memory bits 12..30, targets on bits 31 and 0."""
    nq = 32
    shape = (2,) * nq
    strides = contiguous_strides(shape)
    dim = lambda b: nq - 1 - b
    values = [0] + [1] * 18
    table, info = pack(shape, strides, np.eye(4)[[3, 2, 1, 0]], (dim(31), dim(0)), [dim(b) for b in range(12, 31)], values, torch.complex64)
    head, arr = decode(table)
    assert (info.c_high, info.c_low, info.tile_bits, info.n_tiles, info.n_selected) == (19, 0, 12, 2, 2 ** 13)
    assert info.bytes_read == 2 ** 13 * 8
    holes = arr["hole_bit"][:head["n_holes"]]
    assert head["segment_bits"] == 11 and list(holes) == list(range(12, 32))  # bits 0..10 and 31 are the tile, bit 11 counts tiles
    want = sum(1 << b for b in range(13, 31))
    assert head["high_want"] == want and head["high_mask"] == want | 1 << 12
    base = insert_holes(np.arange(2, dtype=np.int64) << 11, holes) | want
    assert [int(b) for b in base] == [want, want | 1 << 11]
    top = int(base[1]) | int(xor_cols(np.array([2 ** 12 - 1], dtype=np.int64), arr["mem_col"])[0])
    assert top == want | 1 << 31 | (1 << 12) - 1 and 2 ** 31 < top < 2 ** 32  # the last address: past 2^31, inside the state
