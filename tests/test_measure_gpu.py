"""measure_, postselect_, reset_ and apply_channel_ (artensor_amd/measure.py) on the device against the numpy oracle
tests/measure_oracle.py: the choice for every mid-interval uniform, the collapse bit for bit, reset against postselect_ + X,
device-resident outcomes, the default draw, one 8 GiB state, and the trajectory step of two channels.

States of 2^1, 2^2, 2^4, 2^12 and 2^20 elements, complex64 and complex128, contiguous and one permuted layout per size.  Measured
memory bits: 0 (inside a 16-byte vector of complex64), 1, 2, 3, 9 or 10, and the top one; pairs of a bit below 4 with the top
bit; every qubit at once for n <= 10 (the result is a basis state).

Bounds: a probability is a quotient of two float64 sums of n non-negative terms, 4 n 2^-53 relative (the derived bound of
test_born_gpu.py); the norm after a renormalised collapse adds one rounding per stored component, 2^-22 relative for complex64 and
2^-51 for complex128; everything else is compared bit for bit."""
import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import measure

import exact_state as E
import measure_oracle as MO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GIB = 1 << 30
SIZES = [1, 2, 4, 12, 20]
DTYPES = {"c64": (torch.complex64, np.complex64, np.uint32, 2.0 ** -22), "c128": (torch.complex128, np.complex128, np.uint64, 2.0 ** -51)}
LAYOUTS = ["contiguous", "permuted"]
CASES = [(n, kind, layout) for n in SIZES for kind in DTYPES for layout in LAYOUTS]
IDS = [f"n{n}-{kind}-{layout}" for n, kind, layout in CASES]
LAST = float(np.nextafter(1.0, 0.0))


def tol(n_elems):
    return 4.0 * n_elems * 2.0 ** -53


class State:
    """A random logical array of [2] * n and how to put it on the device in one layout.  perm[i] is the logical dim stored at
    position i of the contiguous storage, so logical dim perm[i] is memory bit n - 1 - i."""

    def __init__(self, n, kind, layout, seed=0):
        self.n, self.kind = n, kind
        self.tdtype, self.ndtype, self.bits_dtype, self.round = DTYPES[kind]
        rng = np.random.default_rng(1000 * n + seed)
        self.perm = list(range(n)) if layout == "contiguous" else [int(x) for x in rng.permutation(n)]
        if layout == "permuted" and n > 1 and self.perm == list(range(n)):
            self.perm = self.perm[::-1]
        self.host = (rng.standard_normal((2,) * n) + 1j * rng.standard_normal((2,) * n)).astype(self.ndtype)

    def dim_of_bit(self, b):
        return self.perm[self.n - 1 - b]

    def gpu(self, host=None):
        host = self.host if host is None else host
        store = torch.from_numpy(np.ascontiguousarray(host.transpose(self.perm))).to(DEV)
        return store.permute([self.perm.index(d) for d in range(self.n)])     # logical view of the permuted storage

    def dim_sets(self):
        """Measured dims: every bit of {0, 1, 2, 3, a middle one, the top one} alone, pairs of a low bit with the top bit in
        both orders, and every qubit at once for n <= 10."""
        n = self.n
        mid = 9 if n == 12 else 10
        singles = sorted({b for b in (0, 1, 2, 3, mid, n - 1) if b < n})
        sets = [[self.dim_of_bit(b)] for b in singles]
        if n >= 2:
            lows = [b for b in (0, 1, 2, 3) if b < n - 1]
            sets += [[self.dim_of_bit(b), self.dim_of_bit(n - 1)] if i % 2 else [self.dim_of_bit(n - 1), self.dim_of_bit(b)]
                     for i, b in enumerate(lows)]
        if n <= 10:
            order = list(np.random.default_rng(n).permutation(n))
            sets.append([int(d) for d in order])
        return sets


def bits_of(t, st):
    """The logical array of a device tensor as unsigned integers (one per component)."""
    return np.ascontiguousarray(t.cpu().numpy()).view(st.bits_dtype)


def host_bits(a, st):
    return np.ascontiguousarray(a).view(st.bits_dtype)


def same_bits(x, y):
    """Two device tensors of equal layout, compared bit for bit on the device."""
    kind = torch.int32 if x.dtype == torch.complex64 else torch.int64
    return torch.equal(torch.view_as_real(x).view(kind), torch.view_as_real(y).view(kind))


# ---- 1. choice -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, kind, layout", CASES, ids=IDS)
def test_choice_returns_the_outcome_of_every_mid_interval_uniform(n, kind, layout):
    st = State(n, kind, layout)
    t0 = st.gpu()
    for dims in st.dim_sets():
        q = MO.probabilities(st.host, dims)
        total = np.cumsum(q)[-1]
        outcomes = [o for o in range(q.size) if q[o] > 0]
        if len(outcomes) > 16:
            outcomes = outcomes[:4] + outcomes[-4:]
        for o in outcomes:
            got, p = A.measure_(t0.clone(), dims, uniform=MO.mid_uniform(q, o))
            assert got == o, (dims, o, got)
            assert abs(p - q[o] / total) <= tol(2 ** n) * q[o] / total, (dims, o, p, q[o] / total)


@pytest.mark.parametrize("n, kind, layout", CASES, ids=IDS)
def test_choice_at_the_ends_of_the_interval_lands_on_a_live_outcome(n, kind, layout):
    st = State(n, kind, layout, seed=1)
    dims = [st.dim_of_bit(b) for b in sorted({0, n - 1, n // 2})][::-1]
    D = 2 ** len(dims)
    for parity in (0, 1):                                       # amplitudes exactly zero on the outcomes of this parity
        host = st.host.copy()
        for o in range(D):
            if o % 2 == parity:
                host[MO.kept_mask(host.shape, dims, o)] = 0
        live = [o for o in range(D) if o % 2 != parity]
        t0 = st.gpu(host)
        first, p = A.measure_(t0.clone(), dims, uniform=0.0)
        assert first == live[0] and p > 0
        last, p = A.measure_(t0.clone(), dims, uniform=LAST)
        assert last == live[-1] and p > 0
        last, p = A.measure_(t0.clone(), dims, uniform=torch.tensor([LAST], dtype=torch.float64, device=DEV))
        assert last == live[-1] and p > 0


# ---- 2. collapse ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, kind, layout", CASES, ids=IDS)
def test_collapse_is_exact(n, kind, layout):
    st = State(n, kind, layout, seed=2)
    real = np.float32 if kind == "c64" else np.float64
    tiny = np.finfo(real).smallest_subnormal
    for case, dims in enumerate(st.dim_sets()):
        D = 2 ** len(dims)
        o = (case * 5 + 1) % D
        host = st.host.copy()
        gone = np.flatnonzero(~MO.kept_mask(host.shape, dims, o))   # -0.0 and denormals among what is projected away
        for j, at in enumerate(gone[:: max(1, len(gone) // 64)]):
            host.reshape(-1)[at] = [complex(-0.0, -0.0), complex(tiny, -3 * tiny), complex(-0.0, 7 * tiny)][j % 3]
        q = MO.probabilities(host, dims)
        u = MO.mid_uniform(q, o)
        t0 = st.gpu(host)

        x = t0.clone()                                          # renormalize=False: kept elements bit for bit, +0.0 elsewhere
        got, p = A.measure_(x, dims, uniform=u, renormalize=False)
        assert got == o
        assert np.array_equal(bits_of(x, st), host_bits(MO.collapsed(host, dims, o, 1.0), st)), dims

        x = t0.clone()                                          # renormalize=True: the record's scale, applied in float64
        qd = A.marginal_probabilities(t0, dims).reshape(-1).cpu().numpy()
        rec = measure.collapse_(x, dims, uniform=u)
        outcome, (prob, total, scale) = int(rec.view(torch.int64)[0]), rec[1:].tolist()
        assert outcome == o
        assert total == np.cumsum(qd)[-1] and prob == qd[o] / total
        want_scale = np.sqrt(total / qd[o])
        assert abs(scale - want_scale) <= 2 * np.spacing(want_scale), (scale, want_scale)
        assert np.array_equal(bits_of(x, st), host_bits(MO.collapsed(host, dims, o, scale), st)), dims
        norm = A.norm2(x)
        assert abs(norm - total) <= (tol(2 ** n) + st.round) * total, (dims, norm, total)


# ---- 3. postselect_ ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, kind, layout", CASES, ids=IDS)
def test_postselect_is_measure_with_the_outcome_given(n, kind, layout):
    st = State(n, kind, layout, seed=3)
    t0 = st.gpu()
    for case, dims in enumerate(st.dim_sets()):
        q = MO.probabilities(st.host, dims)
        o = (case * 3 + 1) % q.size
        for renormalize in (True, False):
            x, y = t0.clone(), t0.clone()
            got, p = A.measure_(x, dims, uniform=MO.mid_uniform(q, o), renormalize=renormalize)
            p2 = A.postselect_(y, dims, o, renormalize=renormalize)
            assert got == o and p2 == p
            assert same_bits(x, y), (dims, o, renormalize)


@pytest.mark.parametrize("n, kind, layout", CASES, ids=IDS)
def test_an_impossible_outcome_leaves_the_state_alone(n, kind, layout):
    st = State(n, kind, layout, seed=4)
    dims = [st.dim_of_bit(0), st.dim_of_bit(n - 1)] if n > 1 else [0]
    o = 2 ** len(dims) - 1
    host = st.host.copy()
    host[MO.kept_mask(host.shape, dims, o)] = 0                 # outcome o has probability exactly 0
    t0 = st.gpu(host)
    x = t0.clone()
    with pytest.raises(ValueError, match="nothing can be observed"):
        A.postselect_(x, dims, o)
    assert same_bits(x, t0)
    got = A.postselect_(x, dims, o, device=True)
    assert got.is_cuda and got.dim() == 0 and float(got) == 0.0
    rec = measure.collapse_(x, dims, outcome=o, reset=True)
    assert int(rec.view(torch.int64)[0]) == -1 and float(rec[1]) == 0.0
    assert same_bits(x, t0)
    z = torch.zeros_like(t0)                                    # total == 0: no outcome at all
    with pytest.raises(ValueError, match="nothing can be observed"):
        A.measure_(z, dims, uniform=0.5)
    o_dev, p_dev = A.measure_(z, dims, uniform=0.5, device=True)
    assert int(o_dev) == -1 and float(p_dev) == 0.0
    bad = t0.clone()                                            # total not finite: untouched as well
    bad[(0,) * n] = complex(float("inf"), 0.0)
    keep = bad.clone()
    o_dev, p_dev = A.reset_(bad, dims, uniform=0.5, device=True)
    assert int(o_dev) == -1 and float(p_dev) == 0.0 and same_bits(bad, keep)


# ---- 4. reset_ -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, kind, layout", CASES, ids=IDS)
def test_reset_is_postselect_then_x_on_the_set_digits(n, kind, layout):
    st = State(n, kind, layout, seed=5)
    t0 = st.gpu()
    dims = [st.dim_of_bit(b) for b in sorted({0, n - 1} | ({min(n - 2, 9)} if n >= 3 else set()))]
    dims = dims[1:] + dims[:1]                                  # k = 3 (fewer where the state has fewer qubits), no memory order
    k = len(dims)
    q = MO.probabilities(st.host, dims)
    for o in range(2 ** k):
        for renormalize in (True, False):
            x = t0.clone()
            p = A.postselect_(x, dims, o, renormalize=renormalize)
            flips = {d: "X" for d, bit in zip(dims, MO.digits(o, k)) if bit}
            if flips:
                A.pauli_apply_(x, flips)
            y = t0.clone()
            got, p2 = A.reset_(y, dims, uniform=MO.mid_uniform(q, o), renormalize=renormalize)
            assert got == o and p2 == p
            assert same_bits(x, y), (dims, o, renormalize)
            z = t0.clone()
            A.reset_(z, dims, uniform=MO.mid_uniform(q, o), renormalize=renormalize)
            assert same_bits(y, z)
    scale = MO.scale_of(q, 1, False)
    y = t0.clone()
    A.reset_(y, dims, uniform=MO.mid_uniform(q, 1), renormalize=False)
    assert np.array_equal(bits_of(y, st), host_bits(MO.reset(st.host, dims, 1, scale), st))


# ---- 5. device=True ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, kind, layout", [c for c in CASES if c[0] in (4, 20)], ids=[i for c, i in zip(CASES, IDS) if c[0] in (4, 20)])
def test_device_outcomes_equal_the_host_ones(n, kind, layout):
    st = State(n, kind, layout, seed=6)
    t0 = st.gpu()
    dims = [st.dim_of_bit(n - 1), st.dim_of_bit(0)]
    q = MO.probabilities(st.host, dims)
    for o in range(4):
        u = MO.mid_uniform(q, o)
        for fn in (A.measure_, A.reset_):
            x, y = t0.clone(), t0.clone()
            o_host, p_host = fn(x, dims, uniform=u)
            o_dev, p_dev = fn(y, dims, uniform=u, device=True)
            assert o_dev.is_cuda and o_dev.dtype == torch.int64 and o_dev.dim() == 0
            assert p_dev.is_cuda and p_dev.dtype == torch.float64 and p_dev.dim() == 0
            assert int(o_dev) == o_host == o and float(p_dev) == p_host
            assert same_bits(x, y)
        x, y = t0.clone(), t0.clone()
        p_dev = A.postselect_(y, dims, o, device=True)
        assert float(p_dev) == A.postselect_(x, dims, o) and same_bits(x, y)


def test_device_outcome_on_a_side_stream():
    st = State(20, "c64", "permuted", seed=7)
    t0 = st.gpu()
    dims = [st.dim_of_bit(19), st.dim_of_bit(0), st.dim_of_bit(10)]
    q = MO.probabilities(st.host, dims)
    u = MO.mid_uniform(q, 5)
    x = t0.clone()
    want = A.measure_(x, dims, uniform=u)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        y = t0.clone()
        o_dev, p_dev = A.measure_(y, dims, uniform=u, device=True)
        o2, p2 = A.reset_(y, dims, uniform=0.0, device=True)    # feeds on the collapsed state, still without the host
    side.synchronize()
    assert (int(o_dev), float(p_dev)) == want == (5, want[1])
    assert int(o2) == 5 and abs(float(p2) - 1.0) <= tol(2 ** 20) + 2.0 ** -22
    A.postselect_(x, dims, 5)                                   # the same second step through the host route
    A.pauli_apply_(x, {d: "X" for d, bit in zip(dims, MO.digits(5, 3)) if bit})
    assert same_bits(x, y)


# ---- 6. default draw -----------------------------------------------------------------------------------------------------------
def test_default_draw_follows_the_born_rule():
    host = np.zeros((2,) * 4, dtype=np.complex64)
    host[0] = np.sqrt(0.7 / 8)                                   # p(first qubit = 1) = 0.3, spread over the other three
    host[1] = np.sqrt(0.3 / 8) * np.exp(1j * np.arange(8).reshape(2, 2, 2))
    t0 = torch.from_numpy(host).to(DEV)
    p1 = float(MO.probabilities(host, [0])[1] / MO.probabilities(host, [0]).sum())
    assert abs(p1 - 0.3) < 1e-6
    gen = torch.Generator(device=DEV).manual_seed(20240607)
    shots = 400
    outs = [A.measure_(t0.clone(), [0], generator=gen, device=True)[0] for _ in range(shots)]
    outs = torch.stack(outs).cpu().numpy()
    assert set(np.unique(outs)) <= {0, 1}
    freq = outs.mean()
    print(f"default draw: {int(outs.sum())} ones in {shots} shots, frequency {freq:.4f}, bound {5 * np.sqrt(0.3 * 0.7 / shots):.4f}")
    assert abs(freq - 0.3) <= 5 * np.sqrt(0.3 * 0.7 / shots)
    gen.manual_seed(20240607)                                   # the seed makes the run reproducible
    again = torch.stack([A.measure_(t0.clone(), [0], generator=gen, device=True)[0] for _ in range(shots)]).cpu().numpy()
    assert np.array_equal(outs, again)


# ---- 7. large ------------------------------------------------------------------------------------------------------------------
def test_postselect_on_an_8_gib_state():
    n = 30
    allowed = (8 << n) + (8 << (n - 1)) + 6 * GIB               # the state, a clone of the kept half, comparison temporaries
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < allowed:
        pytest.skip(f"needs {allowed / GIB:.1f} GiB of free device memory, {free / GIB:.1f} GiB free")
    store = E.fill(torch.empty(1 << n, dtype=torch.complex64, device=DEV))
    words = store.view(torch.int64)                             # one 8-byte word per element: bit-for-bit comparisons
    half = 1 << (n - 1)
    # the top memory bit (dim 0 of the contiguous view), outcome 1: the upper half stays
    q = A.marginal_probabilities(store.view((2,) * n), [0]).cpu().numpy()
    keep = words[half:].clone()
    p = A.postselect_(store.view((2,) * n), [0], 1, renormalize=False)
    assert abs(p - q[1] / q.sum()) <= tol(1 << n) * p
    assert torch.equal(words[half:], keep)
    assert int(torch.count_nonzero(words[:half])) == 0
    del keep
    # memory bit 0 (the last dim), outcome 0: the even elements stay -- the kept half of every 16-byte vector
    E.fill(store)
    q = A.marginal_probabilities(store.view((2,) * n), [n - 1]).cpu().numpy()
    keep = words[0::2].clone()
    p = A.postselect_(store.view((2,) * n), [n - 1], 0, renormalize=False)
    assert abs(p - q[0] / q.sum()) <= tol(1 << n) * p
    assert torch.equal(words[0::2], keep)
    assert int(torch.count_nonzero(words[1::2])) == 0
    del keep, store, words
    torch.cuda.empty_cache()


# ---- 8. apply_channel_ ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(DTYPES))
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("channel", ["amplitude-damping", "depolarizing-2"])
def test_channel_step(channel, layout, kind):
    st = State(6, kind, layout, seed=8)
    t0 = st.gpu()
    if channel == "amplitude-damping":
        kraus, dims = MO.amplitude_damping(0.3), [st.dim_of_bit(0)]
    else:
        kraus, dims = MO.depolarizing2(0.1), [st.dim_of_bit(5), st.dim_of_bit(1)]
    w = MO.channel_weights(st.host, kraus, dims)
    assert abs(w.sum() - 1.0) < 1e-12
    for j in range(len(kraus)):
        u = MO.mid_uniform(w, j)
        assert MO.choose(w, u) == j
        x = t0.clone()
        got, p = A.apply_channel_(x, kraus, dims, uniform=u)
        assert got == j
        assert abs(p - w[j]) <= 1e-12 * w[j], (j, p, w[j])
        y = A.apply_gate_(t0.clone(), kraus[j] / np.sqrt(p), dims)
        assert same_bits(x, y)
    gen = torch.Generator(device=DEV).manual_seed(5)
    j, p = A.apply_channel_(t0.clone(), kraus, dims, generator=gen)
    assert 0 <= j < len(kraus) and abs(p - w[j]) <= 1e-12 * w[j]
    with pytest.raises(ValueError, match="identity"):
        A.apply_channel_(t0.clone(), kraus[:-1], dims)
