"""artensor_amd.trajectories on the device: the records of every trajectory are those of the unbatched choose kernels, every slice
is bit for bit what the unbatched library entry leaves on a dense clone of it with that record, dead and idle trajectories keep
every bit, runs repeat bit for bit, and 1024 trajectories in one tensor follow the density matrix.  At most 2^16 elements per
case."""
import ctypes
import math

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import trajectories as T
from artensor_amd.born import _marginal_desc

import channel_oracle as CO
import trajectories_oracle as TO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = {"c64": (np.complex64, torch.complex64, np.uint32, 4, 12), "c128": (np.complex128, torch.complex128, np.uint64, 3, 11)}
H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / math.sqrt(2)


def crand(rng, shape, kind):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(KINDS[kind][0])


def poison(rng, shape, kind):
    """-0.0, denormals, infinities and NaNs with payloads among ordinary values."""
    word = KINDS[kind][2]
    real = np.float32 if kind == "c64" else np.float64
    vals = rng.standard_normal(2 * int(np.prod(shape))).astype(real).view(word)
    if kind == "c64":
        special = np.array([0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00123, 0xffa00001, 0x7f800055], dtype=word)
    else:
        special = np.array([0x8000000000000000, 0x0000000000000001, 0x800fffffffffffff, 0x7ff0000000000000, 0xfff0000000000000,
                            0x7ff8000000000123, 0xfff4000000000001, 0x7ff0000000000055], dtype=word)
    where = rng.permutation(vals.size)[:vals.size // 4]
    vals[where] = special[np.arange(where.size) % special.size]
    return vals.view(KINDS[kind][0]).reshape(shape)


def finite_poison(rng, shape, kind):
    """-0.0 and denormals among ordinary values: finite, so a sum of squares stays finite."""
    word = KINDS[kind][2]
    a = crand(rng, shape, kind)
    v = a.view(word).reshape(-1)
    special = np.array([0x80000000, 0x00000001, 0x807fffff] if kind == "c64" else
                       [0x8000000000000000, 0x0000000000000001, 0x800fffffffffffff], dtype=word)
    where = rng.permutation(v.size)[:v.size // 4]
    v[where] = special[np.arange(where.size) % 3]
    return a


class Case:
    """A tensor whose dim d holds memory bit bit[d] (extent 2 each), or a contiguous tensor of `shape`; `logical` is its host
    image in dim order, `view` the GPU tensor (memory never copied)."""

    def __init__(self, kind, logical, bit=None):
        self.kind, self.word = kind, KINDS[kind][2]
        n = logical.ndim
        if bit is None:
            self.base = torch.from_numpy(np.ascontiguousarray(logical)).to(DEV)
            self.view = self.base
        else:                                                  # memory dim m holds bit n - 1 - m
            self.perm = [n - 1 - b for b in bit]               # view dim d = memory dim perm[d]
            mem = np.ascontiguousarray(np.transpose(logical, np.argsort(self.perm)))
            self.base = torch.from_numpy(mem).to(DEV)
            self.view = self.base.permute(*self.perm)
        assert tuple(self.view.shape) == logical.shape
        self.before = logical.copy()

    def host(self):
        return self.view.cpu().numpy()


def bits_of(x, word):
    return np.ascontiguousarray(x).view(word)


def dims_for_bits(bit, bits):
    return [bit.index(b) for b in bits]


def spread(B):
    """B uniforms that cover [0, 1) evenly, in a scrambled order: small and large ones among any few trajectories in a row."""
    return torch.from_numpy(((np.arange(B) * 7 + 3) % B + 0.5) / B if B % 7 else (np.arange(B) + 0.5) / B).to(DEV)


def records_of(rec):
    host = rec.cpu().numpy()
    return host.view(np.int64)[:, 0].copy(), host


# ---- references: the unbatched library entries, slice by slice -------------------------------------------------------------------
def reference_measure_records(q, uniforms, forced, renormalize):
    B, D = q.shape
    out = torch.empty((B, 4), dtype=torch.float64, device=DEV)
    stream = N.current_stream_ptr(torch.device(DEV))
    for b in range(B):
        N.check(N.lib().artn_measure_choose(q[b].data_ptr(), D, None if uniforms is None else uniforms[b:b + 1].data_ptr(),
                                            -1 if forced is None else int(forced[b]), int(renormalize), out[b].data_ptr(), stream))
    return out


def reference_collapse(case, dims, batch, rec, reset):
    """artn_measure_collapse on a dense clone of every slice with record[b]; returns the slices [B, ...] on the host."""
    sl = torch.from_numpy(TO.slices(case.before, batch)).to(DEV)
    sub = TO.rest_dims(case.before.ndim, dims, batch)
    d, _ = _marginal_desc(sl[0].shape, sl[0].stride(), sub, sl.dtype)
    stream = N.current_stream_ptr(torch.device(DEV))
    for b in range(sl.shape[0]):
        N.check(N.lib().artn_measure_collapse(ctypes.byref(d), sl[b].data_ptr(), rec[b].data_ptr(), int(reset), stream))
    return sl.cpu().numpy()


def check_measure(case, dims, batch, *, reset=False, renormalize=True, uniforms=None, outcomes=None):
    """`outcomes`: None (drawn), an int, or an int64 host tensor [B]."""
    B, D = TO.batch_size(case.before.shape, batch), 2 ** len(dims)
    q = A.marginal_probabilities(case.view, list(batch) + list(dims)).reshape(B, D)
    forced = None
    if outcomes is None:
        uniforms = spread(B) if uniforms is None else uniforms
    else:
        uniforms = None
        forced = outcomes if isinstance(outcomes, torch.Tensor) else torch.full((B,), outcomes, dtype=torch.int64)
    rec = T.collapse_batch_(case.view, dims, batch, outcomes=outcomes.to(DEV) if isinstance(outcomes, torch.Tensor) else outcomes,
                            uniforms=uniforms, renormalize=renormalize, reset=reset)
    assert rec.shape == (B, 4) and rec.dtype == torch.float64
    want = reference_measure_records(q, uniforms, forced, renormalize)
    assert (rec.cpu().numpy().view(np.int64) == want.cpu().numpy().view(np.int64)).all()
    o, host = records_of(rec)
    if outcomes is None:                                       # ... and the numpy oracle's choice
        assert o.tolist() == TO.choose(q.cpu().numpy(), uniforms.cpu().numpy())
    ref = reference_collapse(case, dims, batch, rec, reset)
    got = TO.slices(case.host(), batch)
    assert (bits_of(got, case.word) == bits_of(ref, case.word)).all()
    return o, host, got


def reference_channel_records(op, q, uniforms, renormalize):
    ch, B = op.channel, op.B
    single = A.ChannelOp((2,) * max(ch.t, 1), tuple(1 << i for i in reversed(range(ch.t))), op.dtype, ch, list(range(ch.t)), DEV)
    out = torch.empty((B, single.record_bytes // 8), dtype=torch.float64, device=DEV)
    stream = N.current_stream_ptr(torch.device(DEV))
    for b in range(B):
        N.check(N.lib().artn_channel_choose(single._table.data_ptr(), single.table_bytes, ch.t, ch.m, ch.form_code,
                                            None if q is None else q[b].data_ptr(), uniforms[b:b + 1].data_ptr(), int(renormalize),
                                            out[b].data_ptr(), single.record_bytes, stream))
    return out


def check_channel(case, ch, dims, batch, *, renormalize=True, uniforms=None):
    B = TO.batch_size(case.before.shape, batch)
    op = T.BatchChannelOp(case.view.shape, case.view.stride(), case.view.dtype, ch, dims, batch, DEV)
    assert op.B == B
    q = A.marginal_probabilities(case.view, list(batch) + list(dims)).reshape(B, 2 ** ch.t) if ch.form == "DIAGONAL" else None
    uniforms = spread(B) if uniforms is None else uniforms
    rec = op.step(case.view, uniforms=uniforms, renormalize=renormalize)
    want = reference_channel_records(op, q, uniforms, renormalize)
    assert (rec.cpu().numpy().view(np.int64) == want[:, :4].cpu().numpy().view(np.int64)).all()
    j, host = records_of(rec)
    # apply_wide_gate_ of K_j * scale on a dense clone of every slice
    sl = torch.from_numpy(TO.slices(case.before, batch)).to(DEV)
    sub = TO.rest_dims(case.before.ndim, dims, batch)
    gates = {}
    for b in range(B):
        if j[b] < 0:
            continue
        key = (int(j[b]), float(host[b, 3]))
        if key not in gates:
            gates[key] = A.WideGate(sl[0].shape, sl[0].stride(), sl.dtype, CO.current_matrix(ch.matrices[key[0]], key[1]), sub, DEV)
        gates[key](sl[b])
    got = TO.slices(case.host(), batch)
    assert (bits_of(got, case.word) == bits_of(sl.cpu().numpy(), case.word)).all()
    return j, host, got


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def layout_cases():
    """(name, kind, bit-of-dim list or None with a shape, batch dims, measured dims, target dims)."""
    out = []
    for kind in ("c64", "c128"):
        line = KINDS[kind][3]
        # batch leading, extents 4 and 2 (contiguous): 9 qubits behind them
        out.append((f"leading-{kind}", kind, ("shape", (4, 2) + (2,) * 9), [0, 1], [3, 10], [10, 2, 5]))
        # a batch bit exactly at the line, memory bit 0 measured / a target alongside, measured bits above and below the batch bits
        n = 11
        bit = list(range(n - 1, -1, -1))                       # dim d holds bit n - 1 - d
        out.append((f"line-{kind}", kind, ("bits", bit), dims_for_bits(bit, [line, line + 2]), dims_for_bits(bit, [0, n - 1, line + 1]),
                    dims_for_bits(bit, [n - 1, 0])))
        # scattered batch bits in a random permuted layout, listed against memory order
        rng = np.random.default_rng(11 if kind == "c64" else 12)
        n = 13
        bit = [int(b) for b in rng.permutation(n)]
        hi = sorted(b for b in range(n) if b >= line)
        out.append((f"scattered-{kind}", kind, ("bits", bit), dims_for_bits(bit, [hi[1], hi[6], hi[3]]),
                    dims_for_bits(bit, [1, hi[5], hi[0]]), dims_for_bits(bit, [hi[2], 0, hi[4], 2])))
    return out


LAYOUTS = layout_cases()


def make_case(rng, kind, spec, fill=crand):
    how, what = spec
    if how == "shape":
        return Case(kind, fill(rng, what, kind))
    return Case(kind, fill(rng, (2,) * len(what), kind), what)


@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("renormalize", [True, False])
@pytest.mark.parametrize("name, kind, spec, batch, dims, targets", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_measured_slices_are_the_unbatched_collapse(name, kind, spec, batch, dims, targets, renormalize, reset):
    rng = np.random.default_rng(21)
    case = make_case(rng, kind, spec)
    o, host, _ = check_measure(case, dims, batch, reset=reset, renormalize=renormalize)
    assert (o >= 0).all() and len(set(o.tolist())) > 1         # the trajectories differ in what they observe
    assert ((host[:, 3] == 1.0) == (not renormalize)).all()
    # post-selection: one outcome for all, and one per trajectory
    case = make_case(rng, kind, spec)
    check_measure(case, dims, batch, reset=reset, renormalize=renormalize, outcomes=2 ** len(dims) - 2)
    case = make_case(rng, kind, spec)
    B = TO.batch_size(case.before.shape, batch)
    check_measure(case, dims, batch, reset=reset, renormalize=renormalize,
                  outcomes=torch.from_numpy(rng.integers(0, 2 ** len(dims), size=B)).to(torch.int64))


CHANNELS = {"depol1": lambda: A.depolarizing(0.6), "depol2": lambda: A.depolarizing(0.7, 2), "damp": lambda: A.amplitude_damping(0.3),
            "bitflip": lambda: A.bit_flip(0.5)}


def diagonal_set(t):
    """A one-non-zero-per-column set on t qubits: products of amplitude damping (even positions) and phase damping (odd)."""
    factors = [CO.amplitude_damping(0.3) if q % 2 == 0 else CO.phase_damping(0.4) for q in range(t)]
    out = []
    for idx in np.ndindex(*(2,) * t):
        m = np.eye(1, dtype=np.complex128)
        for q, i in enumerate(idx):
            m = np.kron(m, factors[q][i])
        out.append(m)
    return out


def channel_on(t, form, rng=None):
    if form == "DIAGONAL":
        return A.Channel.from_kraus(diagonal_set(t))
    if t <= 3:
        return A.depolarizing(0.7, t)
    rng = np.random.default_rng(77)
    D = 2 ** t
    u, _ = np.linalg.qr(rng.standard_normal((D, D)) + 1j * rng.standard_normal((D, D)))
    us = [np.eye(D, dtype=np.complex128), CO.pauli_string([1, 0, 3, 2, 0][:t]), u, np.diag(np.exp(1j * rng.standard_normal(D)))]
    return A.Channel.mixture([0.25] * 4, us)


@pytest.mark.parametrize("form", ["FIXED", "DIAGONAL"])
@pytest.mark.parametrize("renormalize", [True, False])
@pytest.mark.parametrize("name, kind, spec, batch, dims, targets", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_channel_slices_are_the_wide_gate_of_the_scaled_operator(name, kind, spec, batch, dims, targets, renormalize, form):
    rng = np.random.default_rng(31)
    for t in sorted({1, len(targets)}):
        case = make_case(rng, kind, spec)
        ch = channel_on(t, form)
        assert ch.form == form
        j, host, _ = check_channel(case, ch, targets[:t], batch, renormalize=renormalize)
        assert (j >= 0).all() and (form == "DIAGONAL" or len(set(j.tolist())) > 1)   # (FIXED: the trajectories draw different operators)
        if form == "DIAGONAL":
            assert ((host[:, 3] == 1.0) == (not renormalize)).all()
        else:
            assert (host[:, 3] == 1.0).all()


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
SIZES = [
    # (kind, trajectory bits s, batch bits, t): the minimum 2^t; tile bits - 1, + 0, + 1 (one row block and several)
    ("c64", 4, 3, 4), ("c64", 5, 2, 5), ("c128", 3, 3, 3),
    ("c64", 11, 2, 1), ("c64", 12, 2, 3), ("c64", 13, 2, 5), ("c64", 13, 1, 2),
    ("c128", 10, 2, 2), ("c128", 11, 2, 4), ("c128", 12, 2, 5),
]


@pytest.mark.parametrize("kind, s, nbb, t", SIZES)
def test_trajectory_sizes_around_the_tile(kind, s, nbb, t):
    """The trajectory's bits are the low s memory bits but for one target moved above the batch bits (where s allows), so the
    tile has a separate high bit."""
    rng = np.random.default_rng(41)
    n = s + nbb
    bit = list(range(n - 1, -1, -1))
    batch_bits = list(range(s, n))
    if s > t and s >= 8:                                       # swap the top trajectory bit with the top memory bit
        batch_bits = list(range(s - 1, n - 1))
    free = [b for b in range(n) if b not in batch_bits]
    targets = [free[-1]] + free[:t - 1]
    batch, dims = dims_for_bits(bit, batch_bits[::-1]), dims_for_bits(bit, targets)
    for form in ("FIXED", "DIAGONAL"):
        case = Case(kind, crand(rng, (2,) * n, kind), bit)
        ch = channel_on(t, form)
        info = T.trajectory_info(case.view.shape, case.view.stride(), dims, batch, case.view.dtype, channel=ch)
        assert info["tb"] == min(KINDS[kind][4], s) and info["n_tiles"] == 2 ** (n - info["tb"]) and info["B"] == 2 ** nbb
        check_channel(case, ch, dims, batch)
    case = Case(kind, crand(rng, (2,) * n, kind), bit)
    check_measure(case, dims[:2], batch)
    case = Case(kind, crand(rng, (2,) * n, kind), bit)
    check_measure(case, dims[:1], batch, reset=True)


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_1024_trajectories_of_16_elements(kind):
    rng = np.random.default_rng(51)
    shape = (1024,) + (2,) * 4
    for ch, dims in ((A.depolarizing(0.7), [3]), (A.depolarizing(0.7, 2), [1, 4])):
        case = Case(kind, crand(rng, shape, kind))
        j, _, _ = check_channel(case, ch, dims, [0])
        assert len(set(j.tolist())) == ch.m
    case = Case(kind, crand(rng, shape, kind))
    check_measure(case, [2, 4], [0])
    case = Case(kind, crand(rng, shape, kind))
    check_measure(case, [1], [0], reset=True)


def test_more_tiles_than_the_grid():
    """4096 trajectories of 16 elements: 4096 tiles of 2^4 elements on a grid of 2048 workgroups; both numbers from the plan."""
    rng = np.random.default_rng(61)
    shape = (4096,) + (2,) * 4
    case = Case("c64", crand(rng, shape, "c64"))
    ch = A.bit_flip(0.5)
    info = T.trajectory_info(case.view.shape, case.view.stride(), [2], [0], torch.complex64, channel=ch)
    assert info["n_tiles"] == 4096 and info["grid"] == 2048 and info["n_tiles"] > info["grid"] and info["tb"] == 4
    j, _, _ = check_channel(case, ch, [2], [0])
    assert set(j[:2048].tolist()) == {0, 1} == set(j[2048:].tolist())
    case = Case("c64", crand(rng, shape, "c64"))
    check_measure(case, [3], [0])


# ---- no batch dims: the unbatched calls, on the whole tensor ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_without_batch_dims_the_calls_are_the_unbatched_ones(kind):
    rng = np.random.default_rng(71)
    for n, dims in ((1, [0]), (2, [1, 0]), (6, [4, 0]), (13, [12, 3])):
        bit = [int(b) for b in rng.permutation(n)]
        a = crand(rng, (2,) * n, kind)
        for reset in (False, True):
            for u in (0.1, 0.8):
                one, two = Case(kind, a, bit), Case(kind, a, bit)
                want = A.measure.collapse_(one.view, dims, uniform=u, reset=reset)
                got = T.collapse_batch_(two.view, dims, (), uniforms=torch.full((1,), u, dtype=torch.float64, device=DEV), reset=reset)
                assert (got.cpu().numpy().view(np.int64) == want.cpu().numpy().view(np.int64).reshape(1, 4)).all()
                assert (bits_of(two.host(), one.word) == bits_of(one.host(), one.word)).all()
        for ch in (channel_on(len(dims), "FIXED"), channel_on(len(dims), "DIAGONAL")):
            for u in (0.3, 0.95):
                one, two = Case(kind, a, bit), Case(kind, a, bit)
                want = A.ChannelOp(one.view.shape, one.view.stride(), one.view.dtype, ch, dims, DEV).step(one.view, uniform=u)
                got = T.BatchChannelOp(two.view.shape, two.view.stride(), two.view.dtype, ch, dims, (), DEV).step(
                    two.view, uniforms=torch.full((1,), u, dtype=torch.float64, device=DEV))
                assert (got.cpu().numpy().view(np.int64) == want[:4].cpu().numpy().view(np.int64).reshape(1, 4)).all()
                assert (bits_of(two.host(), one.word) == bits_of(one.host(), one.word)).all()


# ---- dead and idle trajectories --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reset", [False, True])
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_dead_trajectories_keep_every_bit_while_their_neighbours_collapse(kind, reset):
    rng = np.random.default_rng(81)
    word = KINDS[kind][2]
    shape = (8,) + (2,) * 7
    a = crand(rng, shape, kind)
    minus = 0x80000000 if kind == "c64" else 0x8000000000000000
    a[2] = 0                                                   # all zero, with the signs of a poison pattern
    a[2].view(word).reshape(-1)[::3] = minus
    a[5] = finite_poison(rng, shape[1:], kind)                 # outcome 1 of dim 3 has probability 0: -0.0 there, denormals elsewhere
    a[5][:, :, 1] = 0
    a[5][:, :, 1].view(word)[..., ::2] = minus
    a[6] = poison(rng, shape[1:], kind)                        # NaNs with payloads: the total is not finite
    case = Case(kind, a)
    o, host, got = check_measure(case, [3], [0], reset=reset, outcomes=1)
    assert o.tolist() == [1, 1, -1, 1, 1, -1, -1, 1]
    assert (host[[2, 5, 6], 1] == 0.0).all() and (host[[2, 5, 6], 3] == 1.0).all()
    for b in (2, 5, 6):
        assert (bits_of(got[b], word) == bits_of(a[b], word)).all()
    for b in (0, 1, 3, 4, 7):
        assert not (bits_of(got[b], word) == bits_of(a[b], word)).all()
    # a drawn measurement: the all-zero and the non-finite trajectories again
    case = Case(kind, a)
    o, host, got = check_measure(case, [3, 6], [0], reset=reset)
    assert o[2] == -1 and o[6] == -1 and (np.delete(o, [2, 6]) >= 0).all()
    for b in (2, 6):
        assert (bits_of(got[b], word) == bits_of(a[b], word)).all()
    # a DIAGONAL channel draws nothing there either
    case = Case(kind, a)
    j, host, got = check_channel(case, A.amplitude_damping(0.3), [4], [0])
    assert j[2] == -1 and j[6] == -1 and (np.delete(j, [2, 6]) >= 0).all()
    for b in (2, 6):
        assert (bits_of(got[b], word) == bits_of(a[b], word)).all()


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_identity_draws_leave_poisoned_slices_untouched(kind):
    rng = np.random.default_rng(91)
    word = KINDS[kind][2]
    shape = (8,) + (2,) * 12                                   # two tiles per trajectory (complex128), one (complex64)
    a = crand(rng, shape, kind)
    idle = [1, 4, 7]
    for b in idle:
        a[b] = poison(rng, shape[1:], kind)
    u = torch.tensor([0.9, 0.0, 0.7, 0.95, 0.3, 0.99, 0.8, 0.1], dtype=torch.float64, device=DEV)
    for ch, dims in ((A.depolarizing(0.5), [5]), (A.depolarizing(0.5, 2), [12, 1])):
        case = Case(kind, a)
        op = T.BatchChannelOp(case.view.shape, case.view.stride(), case.view.dtype, ch, dims, [0], DEV)
        j, p = op(case.view, uniforms=u)
        assert j.is_cuda and j.dtype == torch.int64 and p.dtype == torch.float64 and j.shape == p.shape == (8,)
        j = j.cpu().numpy()
        assert (j[idle] == 0).all() and (np.delete(j, idle) > 0).all()
        got = case.host()
        for b in range(8):
            same = (bits_of(got[b], word) == bits_of(a[b], word)).all()
            assert same == (b in idle), b


# ---- repeatability, the front ----------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_nothing_comes_to_the_host():
    rng = np.random.default_rng(101)
    n = 14
    bit = [int(b) for b in rng.permutation(n)]
    hi = [b for b in range(n) if b >= 4]
    batch, dims = dims_for_bits(bit, [hi[0], hi[4], hi[5], hi[2]]), dims_for_bits(bit, [0, hi[3]])
    a = crand(rng, (2,) * n, "c64")
    u = torch.rand(16, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    runs = []
    for _ in range(2):
        case = Case("c64", a, bit)
        out = [T.channel_batch_(case.view, A.amplitude_damping(0.2), dims[:1], batch, uniforms=u),
               T.channel_batch_(case.view, A.depolarizing(0.5, 2), dims, batch, uniforms=u),
               T.measure_batch_(case.view, dims, batch, uniforms=u),
               T.reset_batch_(case.view, dims[1:], batch, uniforms=u),
               T.postselect_batch_(case.view, dims[:1], batch, 0)]
        for o, p in out:
            assert o.is_cuda and p.is_cuda and o.dtype == torch.int64 and p.dtype == torch.float64 and o.shape == p.shape == (16,)
        runs.append(([torch.stack([o.to(torch.float64), p]).cpu().numpy() for o, p in out], case.host(),
                     T.trajectory_norms(case.view, batch).cpu().numpy()))
    for x, y in zip(runs[0][0], runs[1][0]):
        assert (x.view(np.int64) == y.view(np.int64)).all()
    assert (bits_of(runs[0][1], np.uint32) == bits_of(runs[1][1], np.uint32)).all()
    assert (runs[0][2].view(np.int64) == runs[1][2].view(np.int64)).all()
    # drawn on the device where no uniforms are given, from the generator
    case = Case("c64", a, bit)
    g = torch.Generator(device=DEV).manual_seed(5)
    o1, _ = T.measure_batch_(case.view, dims, batch, generator=g)
    case = Case("c64", a, bit)
    o2, _ = T.measure_batch_(case.view, dims, batch,
                             uniforms=torch.rand(16, dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)))
    assert (o1 == o2).all()
    with pytest.raises(ValueError, match="one per trajectory"):
        T.measure_batch_(case.view, dims, batch, uniforms=u[:3])
    with pytest.raises(ValueError, match="one per trajectory"):
        T.postselect_batch_(case.view, dims, batch, torch.zeros(3, dtype=torch.int64, device=DEV))


# ---- physics ---------------------------------------------------------------------------------------------------------------------
def test_1024_trajectories_in_one_tensor_follow_the_density_matrix():
    """The circuit of test_channel_gpu.py::test_the_trajectory_mean_follows_the_density_matrix -- 6 qubits, 7 gates; after each gate
    depolarizing(0.05) on its qubits and amplitude_damping(0.1) on qubits 1 and 4 -- on B = 1024 trajectories in one 2^16-element
    tensor.  The mean of <Z_q> over the trajectories lies within 5 / sqrt(1024) of the exact density-matrix evolution (the
    observable lies in [-1, 1]: its standard error is at most 1 / sqrt(B)).  Every trajectory keeps norm 1: 1e-12 relative per
    renormalised step (the bound of test_renormalisation_keeps_the_squared_norm for complex128) times the 14 damping steps."""
    nq, B = 6, 1024
    ry = lambda th: np.array([[math.cos(th / 2), -math.sin(th / 2)], [math.sin(th / 2), math.cos(th / 2)]], dtype=np.complex128)
    rx = lambda th: np.array([[math.cos(th / 2), -1j * math.sin(th / 2)], [-1j * math.sin(th / 2), math.cos(th / 2)]], dtype=np.complex128)
    cnot = np.eye(4, dtype=np.complex128)[[0, 1, 3, 2]]
    gates = [(H, (0,)), (cnot, (0, 1)), (ry(0.7), (2,)), (cnot, (2, 3)), (rx(1.1), (4,)), (cnot, (4, 5)), (cnot, (1, 2))]
    damped = (1, 4)
    rho = np.zeros((64, 64), dtype=np.complex128)
    rho[0, 0] = 1.0
    dep = CO.kraus_of_mixture(*CO.depolarizing(0.05))
    for m, qs in gates:
        rho = CO.apply_to_rho(rho, [m], list(qs), nq)
        for q in qs:
            rho = CO.apply_to_rho(rho, dep, [q], nq)
        for q in damped:
            rho = CO.apply_to_rho(rho, CO.amplitude_damping(0.1), [q], nq)
    diag = np.diag(rho).real.reshape((2,) * nq)
    want = [float(np.tensordot(diag, [1.0, -1.0], axes=([q], [0])).sum()) for q in range(nq)]
    # the trajectories: dim 0 is the batch, qubit q is dim q + 1
    shape = (B,) + (2,) * nq
    psi = torch.zeros(shape, dtype=torch.complex128, device=DEV)
    psi[(slice(None),) + (0,) * nq] = 1.0
    stride = psi.stride()
    ops = [A.WideGate(shape, stride, psi.dtype, m, [q + 1 for q in qs], DEV) for m, qs in gates]
    depol = {q: T.BatchChannelOp(shape, stride, psi.dtype, A.depolarizing(0.05), [q + 1], [0], DEV) for q in range(nq)}
    damp = {q: T.BatchChannelOp(shape, stride, psi.dtype, A.amplitude_damping(0.1), [q + 1], [0], DEV) for q in damped}
    g = torch.Generator(device=DEV).manual_seed(1234)
    renormalised = 0
    for gate, (m, qs) in zip(ops, gates):
        gate(psi)
        for q in qs:
            depol[q](psi, generator=g)
        for q in damped:
            damp[q](psi, generator=g)
            renormalised += 1
    assert renormalised == 14
    norms = T.trajectory_norms(psi, [0]).cpu().numpy()
    assert norms.shape == (B,)
    print(f"trajectory norms: max |norm - 1| = {np.abs(norms - 1).max():.3e}, bound {renormalised * 1e-12:.1e}")
    assert np.abs(norms - 1).max() <= renormalised * 1e-12
    mean = (psi.real ** 2 + psi.imag ** 2).mean(dim=0).cpu().numpy()
    got = [float(np.tensordot(mean, [1.0, -1.0], axes=([q], [0])).sum()) for q in range(nq)]
    for q in range(nq):
        print(f"<Z_{q}>: trajectories {got[q]:+.4f}, density matrix {want[q]:+.4f}, bound {5 / math.sqrt(B):.4f}")
    for q in range(nq):
        assert abs(got[q] - want[q]) <= 5 / math.sqrt(B), (q, got[q], want[q])
