"""Host-side checks of the noise channels (artensor_amd/channel.py; artn_channel_query / _pack / _choose / _apply): the symbols,
every refusal with its code and text, the Python-side checks, the form each constructor and hand-made set takes, the packed
table against artn_wgate_pack and against the numpy oracle (tests/channel_oracle.py), and the oracle's choice rule against
measure_oracle's.  No GPU needed."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import channel
from artensor_amd.pauli import _desc, _ptr
from artensor_amd.wide_gates import _wgate_pack

import channel_oracle as CO
import measure_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / math.sqrt(2)


def strides_of(bits):
    return [1 << b for b in bits]


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_channel_query", "artn_channel_pack", "artn_channel_choose", "artn_channel_apply"]
    raw = open(os.path.join(ROOT, "include", "artn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    consts = dict(re.findall(r"#define (ARTN_CHANNEL_[A-Z_]+) (\d+)", text))
    assert int(consts["ARTN_CHANNEL_MAX_OPS"]) == N.CHANNEL_MAX_OPS == 256
    assert [int(consts["ARTN_CHANNEL_" + f]) for f in N.CHANNEL_FORMS] == [0, 1, 2]
    assert int(consts["ARTN_CHANNEL_OP_DIAGONAL"]) == N.CHANNEL_OP_DIAGONAL and int(consts["ARTN_CHANNEL_OP_IDENTITY"]) == N.CHANNEL_OP_IDENTITY
    assert re.search(r"#define ARTN_ABI_VERSION 9\b", text) and N.lib().artn_abi_version() == 9
    assert ctypes.sizeof(N.ArtnChannelInfo) == 10 * 4 + 8 * 8
    for name in ("Channel", "ChannelOp", "channel_", "channel_step_", "channel_info", "depolarizing", "pauli_channel", "bit_flip",
                 "phase_flip", "amplitude_damping", "phase_damping"):
        assert getattr(A, name) is getattr(channel, name)


def test_the_form_of_every_constructor_and_of_hand_made_sets():
    for ch, form, t, m in ((A.depolarizing(0.1), "FIXED", 1, 4), (A.depolarizing(0.1, 2), "FIXED", 2, 16),
                           (A.depolarizing(0.1, 4), "FIXED", 4, 256), (A.pauli_channel(0.1, 0.2, 0.05), "FIXED", 1, 4),
                           (A.bit_flip(0.2), "FIXED", 1, 2), (A.phase_flip(0.2), "FIXED", 1, 2),
                           (A.amplitude_damping(0.3), "DIAGONAL", 1, 2), (A.phase_damping(0.3), "DIAGONAL", 1, 2)):
        assert (ch.form, ch.t, ch.m) == (form, t, m), ch
    # the named mixtures pack EXACT Pauli matrices, operator 0 the identity, and their Kraus sets are complete
    probs, us = CO.depolarizing(0.1, 2)
    ch = A.depolarizing(0.1, 2)
    assert all((a == b).all() for a, b in zip(ch.matrices, us)) and np.allclose(ch.weights, probs, rtol=0, atol=1e-16)
    assert (A.pauli_channel(0.1, 0.2, 0.05).matrices == np.stack(CO.PAULIS)).all()
    assert (A.bit_flip(0.2).matrices == np.stack([CO.PAULIS[0], CO.PAULIS[1]])).all()
    assert (A.phase_flip(0.2).matrices == np.stack([CO.PAULIS[0], CO.PAULIS[3]])).all()
    for ch in (A.depolarizing(0.3, 3), A.amplitude_damping(0.3), A.phase_damping(0.7), A.pauli_channel(0.1, 0.2, 0.3)):
        assert np.abs(sum(k.conj().T @ k for k in ch.kraus) - np.eye(2 ** ch.t)).max() < 1e-15
    # hand-made: one non-zero per column is DIAGONAL (a reset-like set, a permutation); a Hadamard-rotated damping set is DENSE
    reset = [np.array([[1, 0], [0, 0]]), np.array([[0, 1], [0, 0]])]
    assert A.Channel.from_kraus(reset).form == "DIAGONAL" and CO.classify(reset) == "DIAGONAL"
    assert A.Channel.from_kraus([np.eye(4)[[2, 0, 3, 1]] * 1j]).form == "DIAGONAL"
    rotated = [H @ k @ H for k in CO.amplitude_damping(0.3)]
    ch = A.Channel.from_kraus(rotated)
    assert ch.form == "DENSE" and CO.classify(rotated) == "DENSE"
    assert all(np.allclose(e, f, rtol=0, atol=1e-16) for e, f in zip(ch.weights, CO.effects(rotated, "DENSE")))
    ad = A.amplitude_damping(0.3)
    assert np.allclose(ad.weights, np.stack(CO.effects(CO.amplitude_damping(0.3), "DIAGONAL")), rtol=0, atol=1e-16)
    assert np.allclose(ad.weights, [[1.0, 0.7], [0.0, 0.3]], rtol=0, atol=4e-16) and ad.weights[1, 0] == 0.0 and ad.weights[0, 0] == 1.0
    mix = A.Channel.mixture([0.25, 0.75], [np.eye(2), H])
    assert mix.form == "FIXED" and (mix.matrices[1] == H).all() and (mix.weights == [0.25, 0.75]).all()
    assert np.allclose(mix.kraus[1], math.sqrt(0.75) * H)


def test_python_side_checks():
    with pytest.raises(ValueError, match="above 1e-10"):
        A.Channel.from_kraus([np.eye(2), 1e-4 * np.eye(2)])
    assert A.Channel.from_kraus([np.eye(2), 1e-4 * np.eye(2)], check=False).m == 2
    assert A.Channel.from_kraus([np.eye(2) * (1 + 4e-11)]).m == 1            # within the bound
    with pytest.raises(ValueError, match="U_1"):
        A.Channel.mixture([0.5, 0.5], [np.eye(2), 1.001 * np.eye(2)])
    with pytest.raises(ValueError, match="sum to 1"):
        A.Channel.mixture([0.5, 0.4], [np.eye(2), np.eye(2)])
    assert A.Channel.mixture([0.5, 0.4], [np.eye(2), 1.001 * np.eye(2)], check=False).form == "FIXED"
    with pytest.raises(ValueError, match="not negative"):
        A.Channel.mixture([1.5, -0.5], [np.eye(2), np.eye(2)], check=False)
    with pytest.raises(ValueError, match="2 probabilities for 1 unitaries"):
        A.Channel.mixture([0.5, 0.5], [np.eye(2)])
    with pytest.raises(ValueError, match="1 to 256 operators"):
        A.Channel.from_kraus([])
    with pytest.raises(ValueError, match="1 to 256 operators"):
        A.Channel.mixture([1 / 257] * 257, [np.eye(2)] * 257)
    with pytest.raises(ValueError, match="2\\^t x 2\\^t"):
        A.Channel.from_kraus([np.eye(3)])
    with pytest.raises(ValueError, match="2\\^t x 2\\^t"):
        A.Channel.from_kraus([np.eye(64)], check=False)
    with pytest.raises(ValueError, match="operator 1 has 16 entries"):
        A.Channel.from_kraus([np.eye(2), np.eye(4)], check=False)
    with pytest.raises(ValueError, match="not finite"):
        A.Channel.from_kraus([np.array([[1, np.nan], [0, 1]])], check=False)
    for bad in (lambda: A.depolarizing(1.5), lambda: A.depolarizing(0.1, 5), lambda: A.bit_flip(-0.1), lambda: A.phase_flip(2),
                lambda: A.amplitude_damping(1.1), lambda: A.phase_damping(-1), lambda: A.pauli_channel(0.5, 0.4, 0.3)):
        with pytest.raises(ValueError):
            bad()
    shape, strides = (2,) * 8, strides_of(range(8))
    with pytest.raises(TypeError, match="a Channel expected"):
        A.channel_info(shape, strides, [np.eye(2)], [0])
    with pytest.raises(ValueError, match="acts on 1 dims, 2 given"):
        A.channel_info(shape, strides, A.bit_flip(0.1), [0, 1])
    with pytest.raises(TypeError, match="complex64 or complex128"):
        A.channel_info(shape, strides, A.bit_flip(0.1), [0], torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.channel_(torch.zeros(shape, dtype=torch.complex64), A.bit_flip(0.1), [0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.ChannelOp(shape, strides, torch.complex64, A.bit_flip(0.1), [0], "cpu")


def test_info_reports_the_plan():
    n = 14
    bits = [3, 0, 11, 7, 1, 9, 2, 10, 4, 8, 6, 5, 13, 12]
    for dtype, elem, tb in ((torch.complex64, 8, 12), (torch.complex128, 16, 11)):
        for ch, dims, red in ((A.depolarizing(0.1), [12], None), (A.amplitude_damping(0.2), [-1], "marginal"),
                              (A.Channel.from_kraus([H @ k @ H for k in CO.amplitude_damping(0.3)]), [2], "rdm"),
                              (A.depolarizing(0.1, 3), [12, 0, 13], None)):
            info = A.channel_info((2,) * n, strides_of(bits), ch, dims, dtype)
            t = ch.t
            wd = {"FIXED": 1, "DIAGONAL": 2 ** t, "DENSE": 2 * 4 ** t}[ch.form]
            assert (info["t"], info["m"], info["form"], info["tb"]) == (t, ch.m, ch.form, tb)
            assert info["target_bits"] == tuple(bits[d] for d in dims) and info["n_tiles"] == 2 ** (n - tb)
            assert info["table_bytes"] == 512 + ch.m * (16 + 8 * wd + 16 * 4 ** t) and info["record_bytes"] == 32 + 16 * 4 ** t
            assert info["reduction"] == red and info["launches"] == 2 and info["lds_bytes"] == elem << tb
            assert info["bytes_read"] == info["bytes_written"] == elem << n
            assert sorted(info["tile_bits"]) == info["tile_bits"] and set(info["target_bits"]) <= set(info["tile_bits"])
    small = A.channel_info((2,) * 6, strides_of(range(6)), A.bit_flip(0.1), [0])
    assert small["tb"] == 6 and small["n_tiles"] == 1


def raw_args(t=1, m=2, n=8, dtype=torch.complex64):
    d = _desc((2,) * n, strides_of(range(n)), dtype)
    dims = np.arange(t, dtype=np.int32)
    mats = np.zeros(m * 2 * 4 ** t)
    return d, dims, mats


def refused(rc, code, text):
    assert rc == code, (rc, N.lib().artn_last_error())
    assert text in N.lib().artn_last_error().decode(), N.lib().artn_last_error()


def test_every_refusal_of_query_and_pack_has_its_code_and_text():
    lib, info = N.lib(), N.ArtnChannelInfo()
    q = lambda d, t, dims, m, form, mats: lib.artn_channel_query(ctypes.byref(d), t, _ptr(dims), m, form, _ptr(mats), ctypes.byref(info), None, None)
    d, dims, mats = raw_args()
    assert q(d, 1, dims, 2, 0, mats) == 0
    refused(lib.artn_channel_query(None, 1, _ptr(dims), 2, 0, _ptr(mats), ctypes.byref(info), None, None), -1, "null descriptor")
    refused(lib.artn_channel_query(ctypes.byref(d), 1, _ptr(dims), 2, 0, _ptr(mats), None, None, None), -1, "null info")
    refused(lib.artn_channel_query(ctypes.byref(d), 1, None, 2, 0, _ptr(mats), ctypes.byref(info), None, None), -1, "null pointer")
    for t in (0, 6, -1):
        refused(q(d, t, np.arange(6, dtype=np.int32), 2, 0, mats), -2, f"channels act on one to five dimensions, not {t}")
    for m in (0, 257, -3):
        refused(q(d, 1, dims, m, 0, mats), -1, f"a channel has 1 to 256 operators, not {m}")
    refused(q(d, 1, dims, 2, 3, mats), -1, "unknown weight form 3")
    refused(q(d, 1, np.array([8], dtype=np.int32), 2, 0, mats), -1, "dimension 8 out of range")
    refused(q(d, 1, np.array([-1], dtype=np.int32), 2, 0, mats), -1, "dimension -1 out of range")
    refused(q(d, 2, np.array([3, 3], dtype=np.int32), 2, 0, np.zeros(64)), -1, "the dimensions must differ; dimension 3 is repeated")
    d4 = _desc((2, 4, 2), (1, 2, 8), torch.complex64)
    refused(q(d4, 1, np.array([1], dtype=np.int32), 2, 0, mats), -1, "channels act on dimensions of extent 2; dimension 1 has extent 4")
    d3 = _desc((2, 3, 2), (1, 2, 6), torch.complex64)
    refused(q(d3, 1, dims, 2, 0, mats), -2, "channels take power-of-two extents")
    gap = _desc((2, 2), (1, 4), torch.complex64)
    refused(q(gap, 1, dims, 2, 0, mats), -1, "not dense")
    dt = _desc((2, 2), (1, 2), torch.complex64)
    dt.dtype = 77
    refused(q(dt, 1, dims, 2, 0, mats), -2, "channels take complex64 or complex128")
    tiny = _desc((2, 2), (1, 2), torch.complex64)
    refused(q(tiny, 3, np.arange(3, dtype=np.int32), 1, 0, np.zeros(128)), -1, "a channel on 3 dimensions needs a state of at least 2^3 elements")
    bad = mats.copy()
    bad[9] = np.inf
    refused(q(d, 1, dims, 2, 0, bad), -1, "an entry of operator 1 is not finite")
    # precedence, as in the gate families: the layout before t, t before the dims, the dims before m and the matrices
    refused(q(d3, 9, np.array([77], dtype=np.int32), 0, 0, bad), -2, "power-of-two")
    refused(q(d, 9, np.array([77], dtype=np.int32), 0, 0, bad), -2, "one to five")
    refused(q(d, 1, np.array([77], dtype=np.int32), 0, 0, bad), -1, "out of range")
    refused(q(d, 1, dims, 0, 0, bad), -1, "operators")
    # pack
    table = np.zeros(1024, dtype=np.uint64)
    w = np.array([0.5, 0.5])
    p = lambda mats_, w_, tab, nbytes: lib.artn_channel_pack(ctypes.byref(d), 1, _ptr(dims), 2, 0, mats_, w_, tab, nbytes)
    assert p(_ptr(mats), _ptr(w), _ptr(table), 8192) == 0
    refused(p(None, _ptr(w), _ptr(table), 8192), -1, "null pointer")
    refused(p(_ptr(mats), None, _ptr(table), 8192), -1, "null pointer")
    refused(p(_ptr(mats), _ptr(w), None, 8192), -1, "null pointer")
    refused(p(_ptr(mats), _ptr(np.array([0.5, np.nan])), _ptr(table), 8192), -1, "a weight of operator 1 is not finite")
    need = 512 + 2 * (16 + 8 + 16 * 4)
    refused(p(_ptr(mats), _ptr(w), _ptr(table), need - 8), -1, "table smaller than artn_channel_query reports")
    assert p(_ptr(mats), _ptr(w), _ptr(table), need) == 0
    refused(p(_ptr(mats), _ptr(w), ctypes.c_void_p(table.ctypes.data + 4), 8000), -2, "artn_channel_pack needs an 8-byte aligned table")


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the CPU-only refusal")
def test_choose_and_apply_refuse_without_a_device():
    lib = N.lib()
    d, dims, _ = raw_args()
    buf = np.zeros(1024, dtype=np.uint64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    refused(lib.artn_channel_choose(p, 8192, 1, 2, 0, None, p, 1, p, 96, None), -4, "no gfx950 device visible")
    refused(lib.artn_channel_apply(ctypes.byref(d), p, 1, _ptr(dims), 2, p, 8192, p, 96, None), -4, "no gfx950 device visible")


def table_parts(table, t, m, wd):
    words = table.view(np.uint64)
    ops = words[64:64 + 2 * m].reshape(m, 2)
    weights = words[64 + 2 * m:64 + 2 * m + wd * m].view(np.float64).reshape(m, wd)
    mats = words[64 + 2 * m + wd * m:].view(np.float64).reshape(m, 4 ** t, 2)
    return words[:60], words[60:64], ops, weights, mats


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
def test_the_packed_table_matches_the_wide_gate_and_the_oracle(dtype):
    rng = np.random.default_rng(5)
    n = 14
    bits = [3, 0, 11, 7, 1, 9, 2, 10, 4, 8, 6, 5, 13, 12]
    shape, strides = (2,) * n, strides_of(bits)
    d = _desc(shape, strides, dtype)
    # m = 1: the first 480 bytes are what artn_wgate_pack writes for the same matrix and dims
    for dims in ([0], [12, 1], [2, 13, 5], [4, 12, 0, 13], [13, 3, 12, 6, 1]):
        t = len(dims)
        for kind in ("dense", "diagonal", "sparse"):
            m = rng.standard_normal((2 ** t, 2 ** t)) + 1j * rng.standard_normal((2 ** t, 2 ** t))
            if kind == "diagonal":
                m = np.diag(np.diag(m))
            if kind == "sparse":
                m = m * (rng.random(m.shape) < 0.05)
                m[0, 0] = 1
            ch = A.Channel.from_kraus([m], check=False)
            dd, mats, weights = channel._split(ch, dims, n, "test")
            table, info = channel._pack(d, ch, dd, mats, weights)
            gate, ginfo = _wgate_pack(d, t, dd, mats)
            head, extra, ops, _, packed = table_parts(table, t, 1, info.weight_doubles)
            assert (head == gate.view(np.uint64)[:60]).all(), (dims, kind)
            assert list(extra) == [1, ch.form_code, info.weight_doubles, 0]
            assert ops[0, 0] == CO.block_mask(m) == gate.view(np.uint64)[7] and ops[0, 1] == CO.op_flags(m)
            assert (packed.reshape(-1) == mats).all()
            assert (info.tile_bits, info.n_tiles, info.lds_bytes) == (ginfo.tile_bits, ginfo.n_tiles, ginfo.lds_bytes)
    # per operator: block mask, diagonal flag, identity flag; the header carries the OR and the AND
    probs, us = CO.depolarizing(0.2, 4)
    ch = A.depolarizing(0.2, 4)
    dims = [13, 3, 12, 6]
    dd, mats, weights = channel._split(ch, dims, n, "test")
    table, info = channel._pack(d, ch, dd, mats, weights)
    head, extra, ops, w, packed = table_parts(table, 4, 256, 1)
    assert list(extra) == [256, 0, 1, 0] and np.allclose(w.reshape(-1), probs, rtol=0, atol=1e-16)
    assert [int(x) for x in ops[:, 0]] == [CO.block_mask(u) for u in us]
    assert [int(x) for x in ops[:, 1]] == [CO.op_flags(u) for u in us]
    assert int(ops[0, 1]) == 3 and sum(int(x) & 2 for x in ops[:, 1]) == 2 and sum(int(x) & 1 for x in ops[:, 1]) == 16
    assert head[7] == np.bitwise_or.reduce(ops[:, 0]) and head[4] == 0
    assert (packed.reshape(256, -1).view(np.complex128).reshape(256, 16, 16) == np.stack(us)).all()
    ad = A.amplitude_damping(0.3)
    dd, mats, weights = channel._split(ad, [5], n, "test")
    table, info = channel._pack(d, ad, dd, mats, weights)
    head, extra, ops, w, packed = table_parts(table, 1, 2, 2)
    assert list(extra) == [2, 1, 2, 0] and (w == ad.weights).all() and [int(x) for x in ops[:, 1]] == [1, 0] and head[4] == 0
    rot = A.Channel.from_kraus([H @ k @ H for k in CO.amplitude_damping(0.3)])
    dd, mats, weights = channel._split(rot, [5], n, "test")
    table, info = channel._pack(d, rot, dd, mats, weights)
    _, extra, _, w, _ = table_parts(table, 1, 2, 8)
    assert list(extra) == [2, 2, 8, 0] and (w.reshape(2, 2, 2, 2).reshape(2, 4, 2).view(np.complex128).reshape(2, 2, 2) == rot.weights).all()


def test_the_oracles_choice_rule_is_measure_oracles():
    rng = np.random.default_rng(11)
    for trial in range(200):
        m = int(rng.integers(1, 20))
        w = rng.random(m) * (rng.random(m) < 0.7)
        for u in list(rng.random(8)) + [0.0, float(np.nextafter(1.0, 0.0))]:
            assert CO.choose(w, u) == MO.choose(w, u) == A.measure.choose_outcome(w, u)[0]
    assert CO.choose([0.0, 0.0], 0.3) == -1 and CO.choose([np.inf, 1.0], 0.3) == -1 and CO.choose([np.nan], 0.3) == -1
    assert CO.choose([0.0, 1.0, 0.0], 0.0) == 1 and CO.choose([0.5, 0.0, 0.5, 0.0], float(np.nextafter(1.0, 0.0))) == 2
    # the record: probability, total and scale
    j, p, total, scale = CO.record("DIAGONAL", np.array([0.3, 0.1]), 0.5, 0.9)
    assert (j, p, total) == (1, 0.1 / 0.4, 0.4) and scale == math.sqrt(0.5 / 0.1)
    assert CO.record("FIXED", np.array([0.3, 0.7]), None, 0.9) == (1, 0.7, 1.0, 1.0)
    assert CO.record("DENSE", np.array([0.3, 0.7]), 0.0, 0.9) == (-1, 0.0, 1.0, 1.0)
    assert CO.record("DENSE", np.array([0.3, 0.7]), 2.0, 0.1, renormalize=False)[3] == 1.0
