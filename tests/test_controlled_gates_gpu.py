"""Controlled gates and classical conditions on the device (artensor_amd/controlled.py: apply_controlled_gate_, ControlledGate,
mcx_, mcz_, mcphase_, when; artn_cgate_apply).

The reference is numpy_gate on the slice of the complex128 LOGICAL array that the control values select; every other element
has to keep its bits.  The bound is the derived one of test_gates_gpu.check: every output component is formed in float64 and
rounded once, so ||y - ref||_2 <= 2 K 2^-24 ||a||_2 G in complex64 and 32 K 2^-53 ||a||_2 G in complex128 (K gates, G the
product of max(1, ||U||_2)).  Everything the contract makes exact is compared bit for bit: c = 0 against apply_wide_gate_, c + t
<= 5 against the embedded matrix, the identity, signed permutations, the raw bits of unselected elements (-0.0, denormals,
infinities, NaN payloads), and a state under a condition that does not hold.

Teleportation: after CNOT, H, one device-resident measurement and the two conditioned corrections the state is compared with a
complex128 numpy run of the same protocol under (K 2 2^-24 + 2^-24) ||a|| G (complex128: (32 K + 1) 2^-53): K the gates that
were applied, one more rounding for the collapse's scale.  The norm of the state is 1 before and after the collapse."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import controlled as CG
from test_gates_cpu import numpy_gate, random_unitary
from test_gates_gpu import CNOT, X, Z, check, growth
from test_pauli_apply_gpu import DEV, KINDS, crand, gpu
from test_pauli_evolve_gpu import bits_of
from test_wide_gates_gpu import PERM14, asym, bit_to_dim, layout, signed_zero_state

pytestmark = pytest.mark.gpu

LB = {"c64": 4, "c128": 3}
H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / np.sqrt(2)


def controlled_oracle(logical, m, targets, controls, values):
    """numpy_gate on the slice the control values select; the rest of the complex128 copy unchanged."""
    psi = np.asarray(logical).astype(np.complex128)
    idx = [slice(None)] * psi.ndim
    for d, v in zip(controls, values):
        idx[d] = int(v)
    sub_dims = [d - sum(c < d for c in controls) for d in targets]
    psi[tuple(idx)] = numpy_gate(psi[tuple(idx)], m, sub_dims)
    return psi


def same_bits(x, y):
    return torch.equal(bits_of(x), bits_of(y))


# ---- 1. random gates against numpy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("t", [1, 2, 3, 4, 5])
def test_random_controlled_gates(t, kind):
    rng = np.random.default_rng(2100 + t)
    seen = set()
    for c_mode in (1, 2, 3, "all"):
        for nq in sorted({t + (c_mode if c_mode != "all" else 1), 9, 12, 13, 14}):
            c = nq - t if c_mode == "all" else c_mode
            if t + c > nq:
                continue
            a = crand(rng, (2,) * nq, kind)
            for permuted in (False, True):
                for name, m in (("unitary", random_unitary(rng, 2 ** t)), ("not unitary", asym(t, nq))):
                    view, logical = layout(a, permuted, rng)
                    picked = [int(x) for x in rng.permutation(nq)[:t + c]]
                    targets, controls = tuple(picked[:t]), tuple(picked[t:])
                    values = [int(v) for v in rng.integers(0, 2, size=c)]
                    ptr, strides = view.data_ptr(), view.stride()
                    info = A.controlled_gate_info(view.shape, strides, m, targets, controls, values, view.dtype)
                    assert A.apply_controlled_gate_(view, m, targets, controls, values) is view
                    assert view.data_ptr() == ptr and view.stride() == strides
                    label = (f"t {t} c {c} ({info['c_high']} high) {kind} [2]*{nq} {'permuted' if permuted else 'contiguous'} {name} "
                             f"targets {targets} controls {controls} = {values}")
                    check(view, controlled_oracle(logical, m, targets, controls, values), a, [(m, targets)], kind, label)
                    seen.add((info["c_high"] > 0, info["c_low"] > 0, info["n_tiles"]))
    assert {n for _, _, n in seen} >= {1, 2} and {(h, l) for h, l, _ in seen} >= {(True, False), (True, True)}


# ---- 2. every addressing form on 2^14 ---------------------------------------------------------------------------------------------
TARGET_BITS = [[0], [2], [6], [12], [13], [7, 1], [0, 13], [4, 9, 11], [12, 3, 6, 0], [13, 12, 5, 1, 0], [10, 2, 9, 4, 11]]
CONTROL_BITS = [[0], [1, 3], [2], [5, 8], [12, 13], [0, 13], [0, 5, 12], [3, 8, 13], [1, 2, 3, 5, 8, 12, 13], [13, 7, 4, 0, 10]]


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_every_addressing_form(kind):
    nq = 14
    rng = np.random.default_rng(1400)
    a = crand(rng, (2,) * nq, kind)
    store = gpu(a)
    logical = a.transpose(PERM14)
    bit = bit_to_dim(store.permute(PERM14))
    count = 0
    for tbits in TARGET_BITS:
        m = asym(len(tbits), 3)
        for cset in CONTROL_BITS:
            cbits = [b for b in cset if b not in tbits]
            if not cbits:
                continue
            for values in ([1] * len(cbits), [0] * len(cbits), [(i + 1) % 2 for i in range(len(cbits))]):
                targets, controls = tuple(bit[b] for b in tbits), tuple(bit[b] for b in cbits)
                view = store.clone().permute(PERM14)
                info = A.controlled_gate_info(view.shape, view.stride(), m, targets, controls, values, view.dtype)
                high = sum(b >= LB[kind] for b in cbits)
                assert info["target_bits"] == tuple(tbits) and info["control_bits"] == tuple(cbits)
                assert (info["c_high"], info["c_low"]) == (high, len(cbits) - high)
                A.apply_controlled_gate_(view, m, targets, controls, values)
                label = f"{kind} target bits {tbits} control bits {cbits} = {values} tiles {info['n_tiles']} segment {info['segment']}"
                check(view, controlled_oracle(logical, m, targets, controls, values), a, [(m, targets)], kind, label)
                count += 1
    assert count > 250


# ---- 3. the bit-for-bit equivalences ----------------------------------------------------------------------------------------------
def embedded(u, k, tpos, cpos, values):
    """|v><v| (x) U + (1 - |v><v|) (x) I as a 2^k matrix: digit 0 the most significant, targets on digits tpos (ascending keeps
    their order), controls on digits cpos."""
    digit = lambda r, p: (r >> (k - 1 - p)) & 1
    e = np.eye(2 ** k, dtype=np.complex128)
    for r in range(2 ** k):
        if any(digit(r, p) != v for p, v in zip(cpos, values)):
            continue
        for c in range(2 ** k):
            if any(digit(c, p) != digit(r, p) for p in cpos):
                continue
            tr = sum(digit(r, p) << (len(tpos) - 1 - i) for i, p in enumerate(tpos))
            tc = sum(digit(c, p) << (len(tpos) - 1 - i) for i, p in enumerate(tpos))
            e[r, c] = u[tr, tc]
    return e


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [5, 9, 14])
def test_bit_for_bit_equivalences(nq, kind):
    rng = np.random.default_rng(300 + nq)
    base, _ = layout(signed_zero_state(rng, nq, kind), nq != 9, rng)
    # c = 0 is apply_wide_gate_
    for t in range(1, 6):
        m, dims = asym(t, nq), tuple(int(x) for x in rng.permutation(nq)[:t])
        got = A.apply_controlled_gate_(base.clone(), m, dims, ())
        assert same_bits(got, A.apply_wide_gate_(base.clone(), m, dims)), ("c = 0", t, dims)
        assert same_bits(got, A.apply_controlled_gate_(base.clone(), m, dims, None)), ("run to run", t)
    # c + t <= 5 is the embedded matrix, however the controls are listed and wherever they lie among the wide gate's digits
    for t, c in ((1, 1), (1, 2), (2, 1), (1, 4), (2, 3), (3, 2), (4, 1), (2, 2)):
        k = t + c
        for trial in range(3):
            dims = [int(x) for x in rng.permutation(nq)[:k]]
            tpos = sorted(int(x) for x in rng.permutation(k)[:t])
            cpos = [p for p in range(k) if p not in tpos]
            values = [int(v) for v in rng.integers(0, 2, size=c)]
            m = asym(t, trial) if trial else random_unitary(rng, 2 ** t)
            targets = tuple(dims[p] for p in tpos)
            want = A.apply_wide_gate_(base.clone(), embedded(m, k, tpos, cpos, values), dims)
            for order in itertools.islice(itertools.permutations(range(c)), 4):
                controls, vals = [dims[cpos[i]] for i in order], [values[i] for i in order]
                got = A.apply_controlled_gate_(base.clone(), m, targets, controls, vals)
                assert same_bits(got, want), ("embedded", t, c, dims, tpos, values, order)
            as_int = int("".join(str(v) for v in values), 2)
            assert same_bits(A.apply_controlled_gate_(base.clone(), m, targets, [dims[p] for p in cpos], as_int), want)
    # the identity changes nothing, signed zeros included; the controls count as a set
    for t in (1, 3, 5):
        picked = [int(x) for x in rng.permutation(nq)]
        c = min(3, nq - t)
        targets, controls = picked[:t], picked[t:t + c]
        values = [int(v) for v in rng.integers(0, 2, size=c)]
        assert same_bits(A.apply_controlled_gate_(base.clone(), np.eye(2 ** t), targets, controls, values), base)
        m = asym(t, 7)
        want = A.apply_controlled_gate_(base.clone(), m, targets, controls, values)
        assert not same_bits(want, base)
        for order in itertools.permutations(range(c)):
            got = A.apply_controlled_gate_(base.clone(), m, targets, [controls[i] for i in order], [values[i] for i in order])
            assert same_bits(got, want), ("set", t, order)
    # Toffoli, Fredkin and CCZ: the 8 x 8 matrices through the wide gate
    toffoli = np.eye(8)[[0, 1, 2, 3, 4, 5, 7, 6]].astype(np.complex128)
    fredkin = np.eye(8)[[0, 1, 2, 3, 4, 6, 5, 7]].astype(np.complex128)
    ccz = np.diag([1, 1, 1, 1, 1, 1, 1, -1]).astype(np.complex128)
    swap = np.eye(4)[[0, 2, 1, 3]].astype(np.complex128)
    for dims in ((0, nq - 1, nq // 2), tuple(int(x) for x in rng.permutation(nq)[:3]), (2, 1, 0)):
        c1, c2, tg = dims
        assert same_bits(A.apply_controlled_gate_(base.clone(), X, (tg,), (c1, c2)), A.apply_wide_gate_(base.clone(), toffoli, dims))
        assert same_bits(A.mcx_(base.clone(), (c2, c1), tg), A.apply_wide_gate_(base.clone(), toffoli, dims))
        assert same_bits(A.apply_controlled_gate_(base.clone(), swap, (c2, tg), (c1,)), A.apply_wide_gate_(base.clone(), fredkin, dims))
        assert same_bits(A.mcz_(base.clone(), dims), A.apply_wide_gate_(base.clone(), ccz, dims))
        assert same_bits(A.mcphase_(base.clone(), dims, np.pi / 2), A.apply_wide_gate_(base.clone(), np.diag([1] * 7 + [np.exp(0.5j * np.pi)]), dims))
    # mcx_ twice gives back the input, with any number of controls
    for c in sorted({0, 1, 4, nq - 1}):
        picked = [int(x) for x in rng.permutation(nq)[:c + 1]]
        once = A.mcx_(base.clone(), picked[1:], picked[0])
        assert not same_bits(once, base) and same_bits(A.mcx_(once, picked[1:], picked[0]), base), c


# ---- 4. unselected elements keep their raw bits ------------------------------------------------------------------------------------
def poison(rng, shape, kind):
    """An array of -0.0, denormals, infinities and NaNs with payloads, quiet and signalling, as raw bit patterns."""
    if kind == "c64":
        pats = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0x00000000],
                        dtype=np.uint32)
        return pats[rng.integers(0, len(pats), size=tuple(shape) + (2,))].view(np.float32).view(np.complex64)[..., 0]
    pats = np.array([0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000,
                     0x7FF8000000000001, 0xFFF8123456789ABC, 0x7FF0000000000001, 0], dtype=np.uint64)
    return pats[rng.integers(0, len(pats), size=tuple(shape) + (2,))].view(np.float64).view(np.complex128)[..., 0]


def raw(a):
    """The bit patterns of a complex array: unsigned integers [..., 2]."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.complex64 else np.uint64).reshape(a.shape + (2,))


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("which, cbits", [("low", [0, 2]), ("low1", [1]), ("high", [5, 12]), ("high-top", [13, 4]), ("both", [1, 8, 13]),
                                          ("both-all", [0, 1, 2, 3, 6, 11, 12])])
def test_unselected_elements_keep_their_raw_bits(which, cbits, kind):
    nq = 14
    rng = np.random.default_rng(4000 + len(cbits))
    for tbits in ([7], [9, 3], [10, 4, 5, 9, 7]):
        tbits = [b for b in tbits if b not in cbits]
        for values in ([1] * len(cbits), [int(v) for v in rng.integers(0, 2, size=len(cbits))]):
            mem = poison(rng, (2,) * nq, kind)                             # memory order: dim j of `mem` is memory bit nq - 1 - j
            idx = [slice(None)] * nq
            for b, v in zip(cbits, values):
                idx[nq - 1 - b] = v
            selected = np.zeros((2,) * nq, dtype=bool)
            selected[tuple(idx)] = True
            mem[selected] = crand(rng, (int(selected.sum()),), kind)
            store = gpu(mem)
            view = store.permute(PERM14)
            bit = bit_to_dim(view)
            targets, controls = tuple(bit[b] for b in tbits), tuple(bit[b] for b in cbits)
            m = asym(len(tbits), 5)
            info = A.controlled_gate_info(view.shape, view.stride(), m, targets, controls, values, view.dtype)
            high = sum(b >= LB[kind] for b in cbits)
            assert (info["c_high"], info["c_low"]) == (high, len(cbits) - high)
            A.apply_controlled_gate_(view, m, targets, controls, values)
            got = store.cpu().numpy()
            assert np.array_equal(raw(got)[~selected], raw(mem)[~selected]), (which, tbits, values)
            finite = np.where(selected, mem, 0)
            want = controlled_oracle(finite.transpose(PERM14), m, targets, controls, values)
            got_sel = np.where(selected, got, 0).transpose(PERM14)
            check(got_sel, want, finite, [(m, targets)], kind, f"{kind} {which} control bits {cbits} = {values} target bits {tbits}")


# ---- 5. exactness at the extreme ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_all_controls_touch_two_elements_or_one(kind):
    nq = 14
    rng = np.random.default_rng(55)
    a = signed_zero_state(rng, nq, kind)
    for permuted in (False, True):
        view, logical = layout(a, permuted, rng)
        for target in (0, 5, nq - 1):
            controls = [d for d in range(nq) if d != target]
            rng.shuffle(controls)
            info = A.controlled_gate_info(view.shape, view.stride(), X, (target,), controls, None, view.dtype)
            assert info["n_selected"] == 2 and info["c"] == nq - 1 and info["n_tiles"] == 1
            got = A.mcx_(view.clone(), controls, target).cpu().numpy()
            want = np.array(logical)
            hi, lo = tuple([1] * nq), tuple(1 if d != target else 0 for d in range(nq))
            want[hi], want[lo] = logical[lo], logical[hi]
            assert np.array_equal(raw(got), raw(want)) and not np.array_equal(raw(got), raw(np.array(logical)))
            values = [int(v) for v in rng.integers(0, 2, size=nq - 1)]         # any other pair
            got = A.apply_controlled_gate_(view.clone(), X, (target,), controls, values).cpu().numpy()
            want = np.array(logical)
            hi, lo = list(lo), list(lo)
            for d, v in zip(controls, values):
                hi[d] = lo[d] = v
            hi[target] = 1
            want[tuple(hi)], want[tuple(lo)] = logical[tuple(lo)], logical[tuple(hi)]
            assert np.array_equal(raw(got), raw(want))
        dims = [int(x) for x in rng.permutation(nq)]
        got = A.mcz_(view.clone(), dims).cpu().numpy()
        want = np.array(logical)
        want[tuple([1] * nq)] = -want[tuple([1] * nq)]
        assert np.array_equal(raw(got), raw(want)) and int((raw(got) != raw(np.array(logical))).any(-1).sum()) == 1


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_grover_search_on_ten_qubits(kind):
    nq, marked = 10, 0b1011001110
    n = 2 ** nq
    dtype = KINDS[kind][1]
    psi = torch.zeros((2,) * nq, dtype=dtype, device=DEV)
    psi[(0,) * nq] = 1
    every = list(range(nq))
    zeros = [q for q in every if not (marked >> (nq - 1 - q)) & 1]
    layer = lambda m, dims: [(m, (q,)) for q in dims]
    A.apply_gates_(psi, layer(H, every))
    theta, unit, applied, g = np.arcsin(1 / np.sqrt(n)), (2 * 2.0 ** -24 if kind == "c64" else 32 * 2.0 ** -53), nq, growth(layer(H, every))
    index = tuple((marked >> (nq - 1 - q)) & 1 for q in every)
    rounds = int(np.pi / (4 * theta))
    probs = []
    for r in range(1, rounds + 1):
        A.apply_gates_(psi, layer(X, zeros))
        A.mcz_(psi, every)                                                   # -1 on the marked item
        A.apply_gates_(psi, layer(X, zeros))
        A.apply_gates_(psi, layer(H, every) + layer(X, every))
        A.mcz_(psi, every[::-1])                                             # -1 on |1..1>: the diffusion, up to a global sign
        A.apply_gates_(psi, layer(X, every) + layer(H, every))
        applied += 2 * len(zeros) + 2 + 4 * nq
        g *= growth(layer(H, every)) ** 2
        probs.append((r, applied, g, psi[index].abs() ** 2))                # (a device scalar: read after the loop)
    for r, k, growth_r, p in probs:
        want, err = np.sin((2 * r + 1) * theta) ** 2, unit * k * growth_r   # ||state error||_2 <= err; |amp| <= 1 + err
        bound = 2 * err + err ** 2 + 4 * 2.0 ** -53
        print(f"grover {kind} round {r}: p {float(p):.9f} want {want:.9f} diff {abs(float(p) - want):.3e} bound {bound:.3e}")
        assert abs(float(p) - want) <= bound, r
    assert float(probs[-1][3]) > 0.999


def test_more_tiles_than_workgroups():
    """2^25 complex64 under one high control: 4096 tiles for at most 2048 workgroups.  X and a phase: exact."""
    nq = 25
    store = torch.arange(2 ** nq, dtype=torch.float32, device=DEV).remainder(4093.0)
    t = torch.complex(store, -store - 1).view((2,) * nq)
    before = t.clone()
    dim = lambda b: nq - 1 - b
    m = np.array([[0, 1j], [-1, 0]])
    info = A.controlled_gate_info(t.shape, t.stride(), m, (dim(24),), (dim(20),), [1])
    assert info["n_tiles"] == 4096 and info["c_high"] == 1 and info["bytes_read"] == 2 ** 24 * 8
    A.apply_controlled_gate_(t, m, (dim(24),), (dim(20),), [1])
    want = before.clone()
    sel = before.movedim((dim(24), dim(20)), (0, 1))
    out = want.movedim((dim(24), dim(20)), (0, 1))
    out[0, 1] = torch.complex(-sel[1, 1].imag, sel[1, 1].real)                # i * x
    out[1, 1] = -sel[0, 1]
    assert same_bits(t, want) and not same_bits(t, before)


# ---- 6. classical conditions ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_conditions_on_hand_made_outcomes(kind):
    nq = 13
    rng = np.random.default_rng(66)
    a = crand(rng, (2,) * nq, kind)
    base, _ = layout(a, True, rng)
    bad = gpu(poison(rng, (2,) * nq, kind)).permute([int(p) for p in rng.permutation(nq)])
    m, targets, controls, values = asym(2, 6), (3, 11), (0, 7, 12), [1, 0, 1]
    want = A.apply_controlled_gate_(base.clone(), m, targets, controls, values)
    gate = A.ControlledGate(base.shape, base.stride(), base.dtype, m, targets, controls, base.device, values)
    bad_gate = A.ControlledGate(bad.shape, bad.stride(), bad.dtype, m, targets, controls, bad.device, values)
    outcomes = torch.tensor([5, -1, 6, 0, 2 ** 40 + 5], dtype=torch.int64, device=DEV)
    record = torch.tensor([0.0, 0.25, 1.0, 2.0], dtype=torch.float64, device=DEV)
    record.view(torch.int64)[0] = 3
    holds = [A.when(outcomes, 5), A.when(outcomes[0], 5), A.when(outcomes, 1, mask=1), A.when(outcomes, 4, mask=6), A.when(outcomes, 0, mask=2),
             A.when(outcomes[2:], 6), A.when(outcomes[3], 0), A.when(outcomes[4:], 5, mask=7), A.when(record, 3), A.when(record, 1, mask=1)]
    fails = [A.when(outcomes, 4), A.when(outcomes, 0, mask=1), A.when(outcomes[1], 0, mask=0), A.when(outcomes[1:], 1, mask=1),
             A.when(outcomes[1:], 2 ** 63 - 1), A.when(outcomes[2], 1, mask=1), A.when(outcomes[4], 5), A.when(record, 2), A.when(record, 0, mask=1)]
    for cond in holds:
        assert same_bits(gate(base.clone(), cond), want), cond
        assert same_bits(A.apply_controlled_gate_(base.clone(), m, targets, controls, values, condition=cond), want), cond
    for cond in fails:
        assert same_bits(gate(base.clone(), cond), base), cond
        assert same_bits(bad_gate(bad.clone(), cond), bad), cond                # untouched: nothing was read or written
        assert same_bits(A.mcx_(bad.clone(), (1, 2), 0, condition=cond), bad) and same_bits(A.mcz_(bad.clone(), (4,), condition=cond), bad)
    assert same_bits(gate(base.clone()), want) and same_bits(gate(base.clone(), None), want)
    with pytest.raises(TypeError, match="when"):
        gate(base.clone(), outcomes)
    with pytest.raises(ValueError, match="built for shape"):
        gate(base.clone().permute(list(range(nq))[::-1]))


def test_apply_refuses_bad_pointers_on_the_device():
    """The refusals of artn_cgate_apply come before the launch: the device pointers are real, the misaligned ones are never used."""
    t = torch.zeros((2,) * 6, dtype=torch.complex64, device=DEV)
    gate = A.ControlledGate(t.shape, t.stride(), t.dtype, np.eye(2), (0,), (5, 2), DEV)
    cond = torch.zeros(2, dtype=torch.int64, device=DEV)
    call = lambda a, table, nbytes, c: N.lib().artn_cgate_apply(ctypes.byref(gate._d), ctypes.c_void_p(a), 1, CG._ptr(gate._targets), 2,
                                                                 CG._ptr(gate._controls), CG._ptr(gate._values), ctypes.c_void_p(table),
                                                                 nbytes, ctypes.c_void_p(c), 0, 0, None)
    a, table, nb, c = t.data_ptr(), gate._table.data_ptr(), gate.table_bytes, cond.data_ptr()
    for args, rc, word in (((a, table, nb - 1, c), -1, b"smaller"), ((0, table, nb, c), -1, b"null"), ((a, 0, nb, c), -1, b"null"),
                           ((a + 8, table, nb, c), -2, b"16-byte aligned array"), ((a, table + 4, nb, c), -2, b"8-byte aligned table"),
                           ((a, table, nb, c + 4), -2, b"8-byte aligned condition")):
        assert call(*args) == rc and word in N.lib().artn_last_error(), word
    assert call(a, table, nb, c) == 0 and call(a, table, nb, 0) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="16-byte"):
        A.mcx_(torch.zeros(65, dtype=torch.complex64, device=DEV)[1:].view((2,) * 6), (1,), 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.when(torch.zeros(1, dtype=torch.int64), 0)
    with pytest.raises(TypeError, match="int64"):
        A.when(torch.zeros(2, dtype=torch.int32, device=DEV), 0)


def teleport_reference(psi, m, b, r, outcome):
    """The protocol on the complex128 logical array: CNOT, H, projection on `outcome` with renormalisation, X and Z."""
    psi = numpy_gate(psi, CNOT, [m, b])
    psi = numpy_gate(psi, H, [m])
    mb, bb = outcome >> 1, outcome & 1
    keep = np.zeros_like(psi)
    idx = [slice(None)] * psi.ndim
    idx[m], idx[b] = mb, bb
    keep[tuple(idx)] = psi[tuple(idx)]
    keep /= np.linalg.norm(keep.reshape(-1))
    if bb:
        keep = numpy_gate(keep, X, [r])
    if mb:
        keep = numpy_gate(keep, Z, [r])
    return keep


def teleport_device(view, m, b, r, u):
    """Everything is enqueued on the current stream; nothing is read on the host.  Returns the device-resident outcome."""
    A.apply_gate_(view, CNOT, (m, b))
    A.apply_gate_(view, H, (m,))
    o, _ = A.measure_(view, [m, b], uniform=u, device=True)
    A.mcx_(view, (), r, condition=A.when(o, 1, mask=1))
    A.mcz_(view, (r,), condition=A.when(o, 2, mask=2))
    return o


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [12, 14])
def test_teleportation_with_device_resident_outcomes(nq, kind):
    rng = np.random.default_rng(7000 + nq)
    perm = [int(p) for p in rng.permutation(nq)]
    m, b, r = (int(x) for x in rng.permutation(nq)[:3])
    message = crand(rng, (2,) * (nq - 2), "c128")                             # the message qubit (first dim) and its spectators
    message /= np.linalg.norm(message.reshape(-1))
    bell = np.array([[1, 0], [0, 1]]) / np.sqrt(2)
    rest = [d for d in range(nq) if d not in (m, b, r)]
    logical = np.moveaxis(np.multiply.outer(message, bell), list(range(nq)), [m] + rest + [b, r]).astype(KINDS[kind][0])
    store = gpu(np.ascontiguousarray(logical.transpose(np.argsort(perm))))     # a permuted layout of the same logical array
    unit, eps = (2 * 2.0 ** -24, 2.0 ** -24) if kind == "c64" else (32 * 2.0 ** -53, 2.0 ** -53)
    side = torch.cuda.Stream(device=DEV)
    for expected, u in enumerate((0.1, 0.35, 0.6, 0.85)):
        view = store.clone().permute(perm)
        assert view.shape == logical.shape and not view.is_contiguous()
        o = teleport_device(view, m, b, r, u)
        other = store.clone().permute(perm)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            o_side = teleport_device(other, m, b, r, u)
        torch.cuda.current_stream().wait_stream(side)
        assert int(o) == expected == int(o_side)                             # the first host read
        want = teleport_reference(logical.astype(np.complex128), m, b, r, expected)
        got = view.cpu().numpy()
        gates = [(CNOT, (m, b)), (H, (m,))] + [(X, (r,))] * (expected & 1) + [(Z, (r,))] * (expected >> 1)
        norm = np.linalg.norm(logical.astype(np.complex128).reshape(-1))
        bound = (unit * len(gates) + eps) * norm * growth(gates)
        err = np.linalg.norm((got.astype(np.complex128) - want).reshape(-1))
        print(f"teleport {kind} [2]*{nq} outcome {expected}: err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
        assert np.isfinite(err) and err <= bound
        # the receiver holds the message: the slice at the observed digits, receiver in the message's place
        idx = [slice(None)] * nq
        idx[m], idx[b] = expected >> 1, expected & 1
        kept_dims = [d for d in range(nq) if d not in (m, b)]
        received = np.moveaxis(got[tuple(idx)], kept_dims.index(r), 0)
        assert np.linalg.norm((received.astype(np.complex128) - message).reshape(-1)) <= bound + eps
        assert same_bits(other, view)                                        # the side stream: the same bits
