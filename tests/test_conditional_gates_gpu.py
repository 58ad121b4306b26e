"""Conditional gates on the device (artensor_amd/trajectories.py: BatchConditionalGate, apply_conditional_gate_batch_,
correct_batch_; artn_cgate_batch_apply).

Every case is compared AS INTEGERS with ControlledGate on dense clones of the slices -- a trajectory whose selector is negative,
matches no case or names the exact identity has to keep the bits it had -- and with the complex128 numpy oracle of
conditional_gate_oracle.py under the bound of one rounding per component: a component is a sum of 2^(t+1) real products, each at
most max|U| max|a|, formed in float64 and rounded once to the dtype, so |y - ref| <= 2^(t+2) eps max|U| max|a| per element (eps
the spacing of the dtype at 1; the factor 2 over the 2^(t+1) terms covers both components of the modulus).  At most 2^16
elements per case."""
import math

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import trajectories as T

import conditional_gate_oracle as CO
import guard_bands as GB
import trajectories_oracle as TO
from graph_replay import capture_and_replay
from test_gates_cpu import random_unitary
from test_trajectories_gpu import DEV, KINDS, SIZES, Case, bits_of, crand, dims_for_bits, poison

pytestmark = pytest.mark.gpu

X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Z = np.diag([1.0, -1.0]).astype(np.complex128)
I2 = np.eye(2, dtype=np.complex128)
H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / math.sqrt(2)
CNOT = np.eye(4, dtype=np.complex128)[[0, 1, 3, 2]]
PAULIS = [(0, I2), (1, X), (2, Z), (3, X @ Z)]                 # a 2-bit key picks one of four corrections
EPS = {"c64": float(np.finfo(np.float32).eps), "c128": float(np.finfo(np.float64).eps)}


def bound(kind, t, cases, before):
    finite = np.abs(before[np.isfinite(before)])
    return 2 ** (t + 2) * EPS[kind] * max(float(np.abs(u).max()) for _, u in cases) * float(finite.max())


def check(view, before, kind, cases, targets, batch, sel_host, controls=(), values=None, mask=None, selector=None, gate=None):
    """Run the gate on `view` (logical host image `before`) and compare: bit for bit with ControlledGate on dense clones of the
    slices, within the bound with the oracle on the touched slices, bit for bit with the input on the untouched ones.  Returns
    the set of touched trajectories."""
    word = KINDS[kind][2]
    cases = list(cases.items()) if isinstance(cases, dict) else list(cases)
    t, B = len(targets), TO.batch_size(before.shape, batch)
    sel_host = np.asarray(sel_host, dtype=np.int64)
    assert sel_host.shape == (B,)
    if gate is None:
        gate = T.BatchConditionalGate(view.shape, view.stride(), view.dtype, cases, targets, batch, DEV, controls, values, mask)
    assert gate.B == B
    sel = torch.from_numpy(sel_host).to(DEV) if selector is None else selector
    ptr, strides = view.data_ptr(), view.stride()
    assert gate(view, sel) is view and view.data_ptr() == ptr and view.stride() == strides
    got = TO.slices(view.cpu().numpy(), batch)
    sl = torch.from_numpy(TO.slices(before, batch)).to(DEV)
    sub_t, sub_c = TO.rest_dims(before.ndim, targets, batch), TO.rest_dims(before.ndim, controls, batch)
    refs, touched = {}, set()
    for b in range(B):
        j = CO.case_of(sel_host[b], cases, mask)
        if j is None or CO.is_identity(cases[j][1]):
            continue
        if j not in refs:
            refs[j] = A.ControlledGate(sl[0].shape, sl[0].stride(), sl.dtype, cases[j][1], sub_t, sub_c, DEV, values)
        refs[j](sl[b])
        touched.add(b)
    ref = sl.cpu().numpy()
    same = (bits_of(got, word) == bits_of(ref, word)).reshape(B, -1).all(axis=1)
    assert same.all(), f"slices {np.flatnonzero(~same).tolist()} differ from ControlledGate on a clone"
    start = TO.slices(before, batch)
    for b in range(B):
        if b not in touched:
            assert (bits_of(got[b], word) == bits_of(start[b], word)).all(), f"untouched trajectory {b} changed"
    if touched:
        rows = sorted(touched)
        want = TO.slices(CO.conditional_oracle(before, sel_host, cases, targets, batch, controls, values, mask), batch)
        err = float(np.abs(got[rows].astype(np.complex128) - want[rows]).max())
        lim = bound(kind, t, cases, start[rows])
        print(f"{kind} t {t} B {B}: {len(rows)} touched, max |y - ref| = {err:.3e}, bound {lim:.3e}")
        assert err <= lim
    return touched


def cycle(pattern, B):
    return np.array([pattern[b % len(pattern)] for b in range(B)], dtype=np.int64)


# ---- layouts ---------------------------------------------------------------------------------------------------------------------
def layout_cases():
    out = []
    for kind in ("c64", "c128"):
        line = KINDS[kind][3]
        rng = np.random.default_rng(3 if kind == "c64" else 4)
        n = 14
        bit = [int(b) for b in rng.permutation(n)]            # a permuted (non-contiguous) view
        hi = [b for b in range(n) if b >= line]
        # two non-adjacent batch fields listed against memory order; targets above, between and below the batch bits; one high
        # control above the batch bits, one below them, and a low control
        out.append((f"scattered-{kind}", kind, ("bits", bit), dims_for_bits(bit, [hi[5], hi[2], hi[6]]),
                    dims_for_bits(bit, [hi[8], hi[4], 1]), dims_for_bits(bit, [hi[7], hi[0], 0]), [1, 0, 1]))
        # the batch leading with extents 4 and 2, contiguous; a target on memory bit 0
        out.append((f"leading-{kind}", kind, ("shape", (4, 2) + (2,) * 9), [0, 1], [10, 3], [5], [1]))
        # the batch bits at the line and right above it, everything else above them
        n = 11
        bit = list(range(n - 1, -1, -1))
        out.append((f"line-{kind}", kind, ("bits", bit), dims_for_bits(bit, [line, line + 1]), dims_for_bits(bit, [n - 1, 0]),
                    dims_for_bits(bit, [line + 3, 2]), [0, 0]))
    return out


LAYOUTS = layout_cases()


@pytest.mark.parametrize("name, kind, spec, batch, targets, controls, values", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_layouts(name, kind, spec, batch, targets, controls, values):
    rng = np.random.default_rng(17)
    how, what = spec
    t = len(targets)
    for tt, cc in ((t, len(controls)), (1, 0)):
        logical = crand(rng, what if how == "shape" else (2,) * len(what), kind)
        case = Case(kind, logical, None if how == "shape" else what)
        cases = [(5, random_unitary(rng, 2 ** tt)), (9, np.eye(2 ** tt)), (2, random_unitary(rng, 2 ** tt) * 1.5), (12, random_unitary(rng, 2 ** tt))]
        B = TO.batch_size(logical.shape, batch)
        sel = cycle([5, 2, -1, 12, 7, 9, 2, 5], B)             # three cases, dead, no match, the identity
        info = T.conditional_gate_info(case.view.shape, case.view.stride(), cases, targets[:tt], batch, controls[:cc], values[:cc], case.view.dtype)
        assert info["B"] == B and info["c_high"] + info["c_low"] == cc
        touched = check(case.view, case.before, kind, cases, targets[:tt], batch, sel, controls[:cc], values[:cc])
        assert touched == {b for b in range(B) if sel[b] in (5, 2, 12)}


# ---- sizes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, s, nbb, t", SIZES)
def test_trajectory_sizes_around_the_tile(kind, s, nbb, t):
    """The shapes of test_trajectories_gpu.SIZES plus one high control on the top memory bit: after it is taken out a trajectory has
    2^s elements -- the minimum 2^t; tile bits - 1, + 0, + 1 -- and one target sits above the batch bits where s allows."""
    rng = np.random.default_rng(43)
    n = s + nbb
    bit = list(range(n, -1, -1))                               # n + 1 dims; dim 0 holds memory bit n, the control
    batch_bits = list(range(s, n))
    if s > t and s >= 8:
        batch_bits = list(range(s - 1, n - 1))
    free = [b for b in range(n) if b not in batch_bits]
    tbits = [free[-1]] + free[:t - 1]
    batch, targets, controls = dims_for_bits(bit, batch_bits[::-1]), dims_for_bits(bit, tbits), dims_for_bits(bit, [n])
    case = Case(kind, crand(rng, (2,) * (n + 1), kind), bit)
    cases = [(1, random_unitary(rng, 2 ** t)), (2, random_unitary(rng, 2 ** t))]
    info = T.conditional_gate_info(case.view.shape, case.view.stride(), cases, targets, batch, controls, [1], case.view.dtype)
    assert info["tb"] == min(KINDS[kind][4], s) and info["n_tiles"] == 2 ** (n - info["tb"]) and info["B"] == 2 ** nbb and info["c_high"] == 1
    sel = cycle([1, -1, 2, 0], 2 ** nbb)
    assert len(check(case.view, case.before, kind, cases, targets, batch, sel, controls, [1])) == 2 ** nbb // 2
    # ... and without the control, every trajectory touched
    case = Case(kind, crand(rng, (2,) * (n + 1), kind), bit)
    check(case.view, case.before, kind, cases, targets, batch + controls, cycle([2, 1], 2 ** (nbb + 1)))


def test_more_tiles_than_the_grid_and_a_choice_per_trajectory():
    """4096 trajectories of 16 elements: 4096 tiles on a grid of 2048 workgroups, both numbers from the plan.  I, X, Z, XZ by a 2-bit
    key; every case, "no match" and -1 occur in the first and in the second half of the grid."""
    rng = np.random.default_rng(61)
    shape = (4096,) + (2,) * 4
    case = Case("c64", crand(rng, shape, "c64"))
    info = T.conditional_gate_info(shape, case.view.stride(), PAULIS + [(6, H)], [2], [0], dtype=torch.complex64)
    assert info["n_tiles"] == 4096 and info["grid"] == 2048 and info["n_tiles"] > info["grid"] and info["tb"] == 4
    sel = cycle([0, 1, 2, 3, 6, 7, -1], 4096)
    for half in (sel[:2048], sel[2048:]):
        assert set(half.tolist()) == {0, 1, 2, 3, 6, 7, -1}
    touched = check(case.view, case.before, "c64", PAULIS + [(6, H)], [2], [0], sel)
    assert touched == {b for b in range(4096) if sel[b] in (1, 2, 3, 6)}


# ---- selector forms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_selector_forms(kind):
    rng = np.random.default_rng(71)
    shape = (16,) + (2,) * 6
    cases = [(k, random_unitary(rng, 4)) for k in (0, 1, 2)] + [(3, np.eye(4))]
    fresh = lambda: Case(kind, crand(rng, shape, kind))
    # a contiguous int64 [B]
    case = fresh()
    check(case.view, case.before, kind, cases, [2, 5], [0], cycle([0, 3, 2, 1, -1], 16))
    # the stride-4 view that measure_batch_ returns, read where it lies; then the float64 records themselves
    case = fresh()
    o, _ = T.measure_batch_(case.view, [1, 6], [0], uniforms=torch.from_numpy((np.arange(16) * 5 % 16 + 0.5) / 16).to(DEV))
    assert o.stride() == (4,) and not o.is_contiguous()
    before = case.view.cpu().numpy()
    host = o.cpu().numpy()
    assert len(set(host.tolist())) > 2
    check(case.view, before, kind, cases, [2, 5], [0], host, selector=o)
    case = fresh()
    rec = T.collapse_batch_(case.view, [1, 6], [0], uniforms=torch.from_numpy((np.arange(16) * 3 % 16 + 0.5) / 16).to(DEV))
    before = case.view.cpu().numpy()
    check(case.view, before, kind, cases, [2, 5], [0], rec.cpu().numpy().view(np.int64)[:, 0].copy(), selector=rec)
    # a selector at an 8-byte offset that is not a 16-byte one
    case = fresh()
    sel_host = cycle([2, 2, 0, -1, 1], 16)
    buf = torch.zeros(18, dtype=torch.int64, device=DEV)
    odd = buf[1:17] if buf.data_ptr() % 16 == 0 else buf[0:16]
    assert odd.data_ptr() % 16 == 8
    odd.copy_(torch.from_numpy(sel_host))
    check(case.view, case.before, kind, cases, [2, 5], [0], sel_host, selector=odd)
    # mask: one bit of a 2-bit outcome chooses
    case = fresh()
    sel_host = cycle([0, 1, 2, 3, -1], 16)
    touched = check(case.view, case.before, kind, [(2, cases[0][1]), (0, np.eye(4))], [2, 5], [0], sel_host, mask=2)
    assert touched == {b for b in range(16) if sel_host[b] in (2, 3)}


# ---- untouched means untouched ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_untouched_trajectories_keep_every_bit_while_their_neighbours_change(kind):
    rng = np.random.default_rng(81)
    word = KINDS[kind][2]
    shape = (8,) + (2,) * 12                                   # two tiles per trajectory (complex128), one (complex64)
    a = crand(rng, shape, kind)
    sel = np.array([1, -1, 2, 7, 0, 1, -5, 0], dtype=np.int64)  # 1 and 2: gates; -1, -5: dead; 7: no match; 0: the identity
    sentinel = np.full(2 * 2 ** 12, GB.SENTINEL[np.dtype(word).itemsize], dtype=word).view(KINDS[kind][0]).reshape(shape[1:])
    a[1], a[3], a[4] = sentinel, poison(rng, shape[1:], kind), sentinel
    a[6], a[7] = poison(rng, shape[1:], kind), poison(rng, shape[1:], kind)
    cases = [(0, np.eye(4)), (1, random_unitary(rng, 4)), (2, np.kron(X, Z))]
    for controls in ((), (3,)):
        case = Case(kind, a)
        touched = check(case.view, case.before, kind, cases, [12, 1], [0], sel, controls, [1] * len(controls))
        assert touched == {0, 2, 5}
        got = case.host()
        for b in range(8):
            assert (bits_of(got[b], word) == bits_of(a[b], word)).all() == (b not in touched), b


# ---- equalities ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_bit_for_bit_equalities(kind):
    rng = np.random.default_rng(91)
    word = KINDS[kind][2]
    n = 13
    bit = [int(b) for b in rng.permutation(n)]
    a = crand(rng, (2,) * n, kind)
    u = random_unitary(rng, 4)
    # batch_dims=() with one case is ControlledGate under when(), where the condition holds and where it does not
    for o, holds in ((6, True), (5, False), (-1, False), (14, True)):
        one, two = Case(kind, a, bit), Case(kind, a, bit)
        sel = torch.full((1,), o, dtype=torch.int64, device=DEV)
        A.ControlledGate(one.view.shape, one.view.stride(), one.view.dtype, u, [3, 9], [0, 5], DEV, [1, 0])(one.view, A.when(sel, 6, mask=7))
        A.apply_conditional_gate_batch_(two.view, {6: u}, [3, 9], (), sel, [0, 5], [1, 0], mask=7)
        assert (bits_of(two.host(), word) == bits_of(one.host(), word)).all()
        assert (bits_of(two.host(), word) == bits_of(a, word)).all() == (not holds)
    # one case without controls under a selector that matches everywhere is apply_wide_gate_
    hi = [b for b in range(n) if b >= KINDS[kind][3]]
    batch = dims_for_bits(bit, [hi[1], hi[4]])
    targets = [d for d in range(n) if d not in batch][:3]
    u3 = random_unitary(rng, 8)
    one, two = Case(kind, a, bit), Case(kind, a, bit)
    A.apply_wide_gate_(one.view, u3, targets)
    A.apply_conditional_gate_batch_(two.view, [(4, u3)], targets, batch, torch.full((4,), 4, dtype=torch.int64, device=DEV))
    assert (bits_of(two.host(), word) == bits_of(one.host(), word)).all() and not (bits_of(two.host(), word) == bits_of(a, word)).all()
    # correct_batch_ twice: the input bit for bit where at most one of the two bits is set, its negative where both are ((ZX)^2 = -1)
    case = Case(kind, a, bit)
    sel_host = np.array([0b000, 0b001, 0b100, 0b101], dtype=np.int64) | 0b010     # (bit 1 is neither: the mask hides it)
    sel = torch.from_numpy(sel_host).to(DEV)
    A.correct_batch_(case.view, targets[0], batch, sel, x_bit=0, z_bit=2)
    once = TO.slices(case.host(), batch)
    start = TO.slices(a, batch)
    for b in range(1, 4):
        assert not (bits_of(once[b], word) == bits_of(start[b], word)).all()
    assert (bits_of(once[0], word) == bits_of(start[0], word)).all()
    A.correct_batch_(case.view, targets[0], batch, sel, x_bit=0, z_bit=2)
    twice = TO.slices(case.host(), batch)
    assert (bits_of(twice[:3], word) == bits_of(start[:3], word)).all()
    assert (bits_of(twice[3], word) == bits_of(-start[3], word)).all()
    # ... and it is the four-case gate
    case, other = Case(kind, a, bit), Case(kind, a, bit)
    A.correct_batch_(case.view, targets[0], batch, sel, x_bit=0, z_bit=2)
    A.apply_conditional_gate_batch_(other.view, {0: I2, 1: X, 4: Z, 5: Z @ X}, [targets[0]], batch, sel, mask=5)
    assert (bits_of(case.host(), word) == bits_of(other.host(), word)).all()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_teleportation_of_64_states_in_one_tensor(kind):
    """Dim 0 is the batch; qubit 0 (dim 1) holds the state, qubits 1 and 2 a Bell pair.  CNOT(0 -> 1), H(0), both measured per
    trajectory, X^(m1) then Z^(m0) on qubit 2 from the outcomes where they lie; nothing comes to the host before the final check.
    complex128: one 64 x 2^3 tensor.  complex64: a trajectory of 2^3 elements is half a 128-byte line, which the layout rule of the
    batch dims does not admit, so a spectator qubit in |0> on memory bit 0 makes it 64 x 2^4."""
    rng = np.random.default_rng(101)
    B = 64
    psi = rng.standard_normal((B, 2)) + 1j * rng.standard_normal((B, 2))
    psi /= np.linalg.norm(psi, axis=1, keepdims=True)
    bell = np.array([[1, 0], [0, 1]], dtype=np.complex128) / math.sqrt(2)
    start = np.einsum("bi,jk->bijk", psi, bell).astype(KINDS[kind][0])
    if kind == "c64":
        start = np.ascontiguousarray(np.stack([start, np.zeros_like(start)], axis=-1))
    tol = 1e-6 if kind == "c64" else 1e-13
    worst = {}
    for correct in (True, False):
        amps = torch.from_numpy(start).to(DEV)
        A.apply_wide_gate_(amps, CNOT, [1, 2])
        A.apply_wide_gate_(amps, H, [1])
        g = torch.Generator(device=DEV).manual_seed(7)
        o, p = T.measure_batch_(amps, [1, 2], [0], generator=g)          # o = 2 m0 + m1
        if correct:
            assert A.correct_batch_(amps, 3, [0], o, x_bit=0, z_bit=1) is amps
        out, o = amps.cpu().numpy().astype(np.complex128), o.cpu().numpy()
        assert set(o.tolist()) == {0, 1, 2, 3}
        received = out[np.arange(B), o >> 1, o & 1]                      # the receiver's qubit in the observed branch
        if kind == "c64":
            assert not received[:, :, 1].any()
            received = received[:, :, 0]
        assert np.abs(np.linalg.norm(received, axis=1) - 1).max() <= 64 * tol
        worst[correct] = np.abs(received - psi).max(axis=1)
        print(f"{kind} corrected {correct}: max |received - psi| = {worst[correct].max():.3e} (bound {tol:.0e})")
    assert worst[True].max() <= tol
    assert (worst[False] > tol).any()                                    # without the correction the test fails


# ---- determinism and capture -----------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    rng = np.random.default_rng(111)
    n = 14
    bit = [int(b) for b in rng.permutation(n)]
    hi = [b for b in range(n) if b >= 4]
    batch, targets, controls = dims_for_bits(bit, [hi[0], hi[4], hi[5], hi[2]]), dims_for_bits(bit, [0, hi[3]]), dims_for_bits(bit, [hi[7], 2])
    a = crand(rng, (2,) * n, "c64")
    cases = [(k, random_unitary(rng, 4)) for k in range(3)]
    sel = torch.from_numpy(cycle([0, 1, 2, 3, -1], 16)).to(DEV)
    runs = []
    for _ in range(2):
        case = Case("c64", a, bit)
        gate = T.BatchConditionalGate(case.view.shape, case.view.stride(), case.view.dtype, cases, targets, batch, DEV, controls)
        for _ in range(3):
            gate(case.view, sel)
        runs.append(case.host())
    assert (bits_of(runs[0], np.uint32) == bits_of(runs[1], np.uint32)).all() and not (bits_of(runs[0], np.uint32) == bits_of(a, np.uint32)).all()


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_measure_then_correct_captured_in_a_graph(kind):
    """measure_batch_ with given uniforms, then the conditional gate on its outcomes, captured once and replayed on restored states:
    capture_and_replay compares every replay bit for bit with the eager run; here the outcomes are checked to follow the contents
    (read at replay time) and the state to be the oracle's gate on the measured state."""
    shape = (8,) + (2,) * 10
    dims, target = [2, 9], 5
    amps = torch.empty(shape, dtype=KINDS[kind][1], device=DEV)
    u = torch.empty(8, dtype=torch.float64, device=DEV)
    gate = T.BatchConditionalGate(shape, amps.stride(), amps.dtype, PAULIS, [target], [0], DEV)
    seen = []

    def op(x, uniforms):
        o, p = T.measure_batch_(x, dims, [0], uniforms=uniforms)
        gate(x, o)
        return o, p

    def contents(r):
        rng = np.random.default_rng(200 + r)
        return [crand(rng, shape, kind), rng.random(8)]

    def verify(r, hosts, after, outs):
        o = outs[0]
        measured = torch.from_numpy(hosts[0]).to(DEV)
        o2, _ = T.measure_batch_(measured, dims, [0], uniforms=torch.from_numpy(hosts[1]).to(DEV))
        assert (o2.cpu().numpy() == o).all() and (o >= 0).all()
        m = measured.cpu().numpy()
        want = CO.conditional_oracle(m, o, PAULIS, [target], [0])
        assert np.abs(after[0] - want).max() <= bound(kind, 1, PAULIS, m)
        seen.append(tuple(o.tolist()))

    capture_and_replay(op, [amps, u], contents, verify, replays=3)
    assert len(set(seen)) == 3


# ---- guard bands -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_state_and_selector_inside_guard_bands(kind):
    rng = np.random.default_rng(121)
    npdt, word = KINDS[kind][0], KINDS[kind][2]
    shape = (4,) + (2,) * 12
    strides = tuple(int(s) for s in torch.empty(shape).stride())
    cases = [(1, random_unitary(rng, 4)), (2, random_unitary(rng, 4))]
    targets, batch, controls = [12, 3], [0], [1]
    sel_host = np.array([1, -1, 2, 0], dtype=np.int64)
    info = T.conditional_gate_info(shape, strides, cases, targets, batch, controls, dtype=KINDS[kind][1])
    band = GB.band_for(2 ** info["tb"])
    gate = T.BatchConditionalGate(shape, strides, KINDS[kind][1], cases, targets, batch, DEV, controls)
    a = crand(rng, shape, kind)
    results = []
    for off_a, off_s in zip(GB.offsets_of(npdt), GB.offsets_of(np.int64)):
        store, (view,), lay = GB.banded([a.reshape(-1)], shape, strides, npdt, off_a, band, DEV)
        sstore, (sel,), slay = GB.banded([sel_host], (4,), (1,), np.int64, off_s, GB.MIN_BAND, DEV)
        assert view.data_ptr() % 16 == 0 and sel.data_ptr() % 8 == 0
        touched = check(view, a, kind, cases, targets, batch, sel_host, controls, [1], selector=sel, gate=gate)
        assert touched == {0, 2}
        GB.assert_bands_intact(store, lay, f"{kind} state at offset {off_a}")
        GB.assert_bands_intact(sstore, slay, f"{kind} selector at offset {off_s}")
        assert GB.same_bits(GB.states_of(sstore, slay)[0], sel_host)
        results.append(GB.states_of(store, lay)[0])
    assert all(GB.same_bits(r, results[0]) for r in results[1:])
