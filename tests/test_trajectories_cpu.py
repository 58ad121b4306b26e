"""Host-only checks of artensor_amd.trajectories: what the family refuses, by name; the plan against the numpy oracle; the oracle's
batch index against brute force.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import channel as C
from artensor_amd import trajectories as T
from artensor_amd._state import _desc, _ptr

import trajectories_oracle as TO


def contiguous(shape):
    s, out = 1, []
    for e in reversed(shape):
        out.append(s)
        s *= e
    return tuple(reversed(out))


def permuted(rng, n):
    """A [2] * n tensor in a random permuted layout: dim d holds memory bit bit[d]."""
    bit = [int(b) for b in rng.permutation(n)]
    return (2,) * n, tuple(1 << b for b in bit), bit


DENSE = A.Channel.from_kraus([np.array([[1, 1], [1, -1]]) / 2, np.array([[1, -1], [-1, 1]]) / 2 * 1j, np.eye(2) / np.sqrt(2)], check=False)


def library_refuses(shape, strides, dims, batch, dtype, code, text, channel=None):
    """The raw entry gives `code` and names the reason."""
    d, info = _desc(shape, strides, dtype), N.ArtnBatchInfo()
    dims, batch = np.array(dims, dtype=np.int32), np.array(batch, dtype=np.int32)
    if channel is None:
        rc = N.lib().artn_measure_batch_query(ctypes.byref(d), len(dims), _ptr(dims), len(batch), _ptr(batch), ctypes.byref(info))
    else:
        rc = N.lib().artn_channel_batch_query(ctypes.byref(d), channel.t, _ptr(dims), len(batch), _ptr(batch), channel.m, channel.form_code,
                                              None, ctypes.byref(info), None, None)
    assert rc == code and text in N.lib().artn_last_error().decode(), (rc, N.lib().artn_last_error())


@pytest.mark.parametrize("dtype, line", [(torch.complex64, 4), (torch.complex128, 3)])
def test_every_refusal_is_by_name(dtype, line):
    assert N.has("artn_channel_batch_apply")
    shape = (4, 2) + (2,) * 8
    st = contiguous(shape)
    dep, damp = C.depolarizing(0.1), C.amplitude_damping(0.1)
    # a batch dim that is also measured, or a target
    with pytest.raises(ValueError, match="both a batch dim and a measured one"):
        T.trajectory_info(shape, st, [2, 3], [0, 3], dtype)
    with pytest.raises(ValueError, match="both a batch dim and a target one"):
        T.trajectory_info(shape, st, [1], [0, 1], dtype, channel=dep)
    library_refuses(shape, st, [2, 3], [0, 3], dtype, -1, "both a batch dimension and a measured one")
    library_refuses(shape, st, [1], [0, 1], dtype, -1, "both a batch dimension and a target one", dep)
    # a batch bit below the line: the highest bit below it, and bit 0
    for bit in (line - 1, 0):
        dim = 9 - bit
        with pytest.raises(ValueError, match=f"memory bit {bit}, below a 128-byte line.*relayout_"):
            T.trajectory_info(shape, st, [2], [0, dim], dtype)
        with pytest.raises(ValueError, match="below a 128-byte line.*relayout_"):
            T.trajectory_info(shape, st, [2], [dim], dtype, channel=damp)
        library_refuses(shape, st, [2], [0, dim], dtype, -2, "below a 128-byte line", None)
        library_refuses(shape, st, [2], [dim], dtype, -2, "relayout_", damp)
    T.trajectory_info(shape, st, [2], [9 - line], dtype)       # (exactly at the line: accepted)
    # more than 24 batch bits (host-only: nothing is allocated)
    big = (1 << 25, 2) + (2,) * 5
    with pytest.raises(ValueError, match="at most 24 batch bits"):
        T.trajectory_info(big, contiguous(big), [1], [0], dtype)
    library_refuses(big, contiguous(big), [1], [0], dtype, -2, "at most 24 batch bits")
    # B * D above 2^24
    wide = (1 << 22,) + (2,) * 8
    with pytest.raises(ValueError, match=r"B \* D = 2\^25 is above 2\^24"):
        T.trajectory_info(wide, contiguous(wide), [1, 2, 3], [0], dtype)
    library_refuses(wide, contiguous(wide), [1, 2, 3], [0], dtype, -2, "above 2^24")
    T.trajectory_info(wide, contiguous(wide), [1, 2], [0], dtype)
    # a trajectory below 2^t elements (only without batch bits can a state be that small; with them the line rule comes first)
    two = A.depolarizing(0.1, 2)
    with pytest.raises(ValueError, match=r"trajectory of at least 2\^2 elements"):
        T.trajectory_info((2, 1, 1), (1, 1, 1), [0, 1], (), dtype, channel=two)
    # an extent that is no power of two
    odd = (4, 3, 2, 2, 2, 2, 2)
    with pytest.raises(ValueError, match="power-of-two extents"):
        T.trajectory_info(odd, contiguous(odd), [3], [0], dtype)
    with pytest.raises(ValueError, match="power-of-two extents"):
        T.trajectory_info(odd, contiguous(odd), [3], [0], dtype, channel=dep)
    library_refuses(odd, contiguous(odd), [3], [0], dtype, -2, "power-of-two extents")
    library_refuses(odd, contiguous(odd), [3], [0], dtype, -2, "batched channels take power-of-two extents", dep)
    # the DENSE form
    assert DENSE.form == "DENSE"
    with pytest.raises(ValueError, match="DENSE form needs a reduced density matrix per trajectory"):
        T.trajectory_info(shape, st, [2], [0], dtype, channel=DENSE)
    library_refuses(shape, st, [2], [0], dtype, -2, "DENSE form needs a reduced density matrix per trajectory", DENSE)
    with pytest.raises(ValueError, match="DENSE form"):
        T.BatchChannelOp(shape, st, dtype, DENSE, [2], [0], "cuda:0")
    # what measure_ refuses stays refused
    with pytest.raises(ValueError, match="extent 2"):
        T.trajectory_info(shape, st, [0], [1], dtype)
    with pytest.raises(ValueError, match="1 to 10 dims"):
        T.trajectory_info((2,) * 16, contiguous((2,) * 16), list(range(11)), (), dtype)


def test_a_trajectory_below_2_to_the_t_in_the_library():
    # (the Python front stops at dims of extent 2 first; the raw entry sees a state of 2 elements and t = 2)
    shape, st = (2, 1), (1, 1)
    d, info = _desc(shape, st, torch.complex64), N.ArtnBatchInfo()
    dims = np.array([0, 0], dtype=np.int32)
    rc = N.lib().artn_channel_batch_query(ctypes.byref(d), 2, _ptr(dims), 0, None, 2, 0, None, ctypes.byref(info), None, None)
    assert rc == -1                                            # (the repeated dim is named first: a 2-element state has one dim of extent 2)
    shape, st = (2, 2, 2), (1, 2, 4)
    d = _desc(shape, st, torch.complex64)
    dims = np.array([0, 1, 2], dtype=np.int32)
    ch = A.depolarizing(0.1, 3)
    assert N.lib().artn_channel_batch_query(ctypes.byref(d), 3, _ptr(dims), 0, None, ch.m, 0, None, ctypes.byref(info), None, None) == 0
    assert (info.B, info.tile_bits, info.n_tiles) == (1, 3, 1)


@pytest.mark.parametrize("dtype, line, TB", [(torch.complex64, 4, 12), (torch.complex128, 3, 11)])
def test_the_plan_follows_the_oracle_on_random_permuted_layouts(dtype, line, TB):
    rng = np.random.default_rng(5)
    dep2 = A.depolarizing(0.1, 2)
    for trial in range(60):
        n = int(rng.integers(8, 21))
        shape, st, bit = permuted(rng, n)
        high = [d for d in range(n) if bit[d] >= line]
        nb = int(rng.integers(0, min(len(high), 9) + 1))
        batch = [int(x) for x in rng.permutation(high)[:nb]]
        free = [d for d in range(n) if d not in batch]
        dims = [int(x) for x in rng.permutation(free)[:2]]
        # measurement
        info = T.trajectory_info(shape, st, dims, batch, dtype)
        assert (info["B"], info["D"], info["n"]) == (2 ** nb, 4, 2 ** n)
        assert info["fields"] == TO.fields(shape, st, batch)
        assert info["record_bytes"] == 32 * 2 ** nb and (info["launches"], info["reset_launches"]) == (2, 3)
        # ... the fields name the oracle's trajectory of every flat index they are asked about
        flat = rng.integers(0, 2 ** n, size=64)
        b = np.zeros(64, dtype=np.int64)
        for s, w, p in info["fields"]:
            b |= ((flat >> s) & ((1 << w) - 1)) << p
        assert (b == TO.batch_index(flat, shape, st, batch)).all()
        # channel
        ci = T.trajectory_info(shape, st, dims, batch, dtype, channel=dep2)
        assert (ci["B"], ci["D"], ci["fields"]) == (2 ** nb, 4, info["fields"])
        tb = min(TB, n - nb)
        assert ci["tb"] == tb and len(ci["tile_bits"]) == tb and ci["tile_bits"] == sorted(set(ci["tile_bits"]))
        assert ci["target_bits"] == tuple(bit[d] for d in dims) and set(ci["target_bits"]) <= set(ci["tile_bits"])
        assert not set(ci["tile_bits"]) & {bit[d] for d in batch}
        assert ci["n_tiles"] << tb == 2 ** n and ci["grid"] == min(ci["n_tiles"], 2048)
        others = [x for x in range(n) if x not in ci["target_bits"] and x not in {bit[d] for d in batch}]
        assert sorted(set(ci["tile_bits"]) - set(ci["target_bits"])) == others[:tb - 2]   # the lowest that are free


def test_extents_above_two_and_merging():
    shape = (4, 2, 8) + (2,) * 6                               # memory bits: dim 0 -> 10, 11; dim 1 -> 9; dim 2 -> 6, 7, 8
    st = contiguous(shape)
    assert T.trajectory_info(shape, st, [5], [0, 1, 2])["fields"] == [(6, 6, 0)] == TO.fields(shape, st, [0, 1, 2])
    assert T.trajectory_info(shape, st, [5], [0, 2])["fields"] == [(10, 2, 3), (6, 3, 0)] == TO.fields(shape, st, [0, 2])
    assert T.trajectory_info(shape, st, [5], [2, 1, 0])["fields"] == [(6, 3, 3), (9, 1, 2), (10, 2, 0)] == TO.fields(shape, st, [2, 1, 0])
    assert T.trajectory_info(shape, st, [5], [1, 0])["B"] == 8
    one = (1, 4, 1) + (2,) * 7                                 # extent 1 carries no bit
    assert T.trajectory_info(one, contiguous(one), [4], [0, 1, 2])["fields"] == [(7, 2, 0)]


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("ch", [C.depolarizing(0.2), C.amplitude_damping(0.3), C.depolarizing(0.1, 3),
                                A.Channel.from_kraus([np.eye(32)])])
def test_without_batch_dims_plan_and_table_are_the_channel_familys(ch, dtype):
    rng = np.random.default_rng(9)
    for n in (5, 14):
        shape, st, _ = permuted(rng, n)
        dims = [int(x) for x in rng.permutation(n)[:ch.t]]
        want = C.channel_info(shape, st, ch, dims, dtype)
        got = T.trajectory_info(shape, st, dims, (), dtype, channel=ch)
        for key in ("tile_bits", "target_bits", "tb", "n_tiles", "segment", "lds_bytes", "table_bytes", "bytes_read", "bytes_written"):
            assert got[key] == want[key], key
        assert (got["B"], got["fields"], got["launches"]) == (1, [], want["launches"])
        d = _desc(shape, st, dtype)
        dd, mats, weights = C._split(ch, dims, n, "test")
        table = C._pack(d, ch, dd, mats, weights)[0]
        _, dims_, batch, mats_, weights_, info, _, _ = T._channel_plan(shape, st, ch, dims, (), dtype, "test")
        assert (T._pack(d, ch, dims_, batch, mats_, weights_, info) == table).all()


def test_the_oracles_batch_index_is_brute_force_on_tiny_shapes():
    rng = np.random.default_rng(3)
    for shape in ((2, 2, 2), (4, 2, 2), (2, 8, 2, 4), (2, 2, 2, 2, 2), (1, 4, 2)):
        nd = len(shape)
        order = [int(x) for x in rng.permutation(nd)]          # a permuted dense layout
        st, s = [0] * nd, 1
        for x in order:
            st[x] = s
            s *= shape[x]
        for nb in range(nd + 1):
            batch = [int(x) for x in rng.permutation(nd)[:nb]]
            brute = TO.batch_index_brute(shape, st, batch)
            flat = np.arange(s)
            assert TO.batch_index(flat, shape, st, batch).tolist() == [brute[i] for i in range(s)]
            assert max(brute.values()) == TO.batch_size(shape, batch) - 1
            # the slices hold the elements the index names
            logical = np.empty(shape, dtype=np.int64)
            for idx in np.ndindex(*shape):
                logical[idx] = sum(i * t for i, t in zip(idx, st))
            sl = TO.slices(logical, batch)
            for b in range(sl.shape[0]):
                assert all(brute[int(i)] == b for i in sl[b].reshape(-1))
            assert (TO.unslice(sl, shape, batch) == logical).all()
