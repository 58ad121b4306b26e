"""Every state operation on operands inside sentinel bands of one allocation, at storage offsets of 0, 16 and 80 bytes
(tests/guard_bands.py): a store outside an operand changes a band, a load from a band that enters arithmetic turns the result
into NaN.  (A load whose value is discarded is invisible to this method.)

Each case asserts (a) every band and the offset gap bit for bit, (b) the family's existing host reference at that family's
existing bound, imported from its own test module as test_graph_replay_gpu.py imports them, (c) the operands' memory and every
output bit for bit equal to the same call on plain fresh tensors of the same layout at offset 0 -- a condition, not a tolerance:
the float64 terms come in a fixed order -- and (d) untouched memory (an out-of-place operand, the unselected half of a
controlled gate, an exact identity) keeping its bits.

The case builders (*_cases) are host-only: they read the form and the largest unit a plan moves from the *_info calls (block =
2^rank tiles of 2^10, tile bits, elements per workgroup), assert that the form is the one the size is meant to reach and that the
band covers the unit; tests/test_guard_bands_cpu.py runs them without a GPU.  Where an info call reports no tile (the Pauli
expectation and apply kernels, overlap) the unit is the whole state.  Sizes: the ones at which a kernel changes form, every state
at most 2^14 elements.  The bound of gate_check (2 units of the format per gate, in the 2-norm) is the one test_graph_replay_gpu.py
applies to WideGate and ChannelOp; a matrix-core gate forms each component in float64 and rounds it once, so it holds there too."""
import ctypes
import math

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import born, krylov, measure, rdm

import bit_permutation_oracle as BO
import channel_oracle as CO
import diagonal_oracle as DO
import measure_oracle as MO
from adjoint_oracle import oracle_pair
from gates_adjoint_oracle import oracle_gate_pair
from graph_replay import DEV, KINDS, LAYOUTS, crand, logical_of, memory_of, strided_empty
from guard_bands import MIN_BAND, assert_bands_intact, band_for, banded, offsets_of, same_bits, states_of
from matrix_gate_oracle import bound as mgate_bound
from matrix_gate_oracle import components, cover
from matrix_gate_oracle import oracle as mgate_oracle
from test_born_gpu import check_samples, oracle_marginal, sq
from test_born_gpu import tol as born_tol
from test_controlled_gates_gpu import controlled_oracle
from test_diagonal_gpu import phase_bound
from test_diagonal_gpu import same_bits as diag_same_bits
from test_gates_adjoint_gpu import element_bounds, random_measures
from test_gates_gpu import ASYM1, ASYM2, random_circuit
from test_gates_gpu import check as gate_check
from test_gates_gpu import growth as gate_growth
from test_gates_gpu import oracle as gate_oracle
from test_krylov_gpu import combine_reference
from test_pauli_adjoint_gpu import bound as pauli_pair_bound
from test_pauli_apply_gpu import check as apply_check
from test_pauli_apply_gpu import oracle_sum
from test_pauli_evolve_gpu import check as evolve_check
from test_pauli_evolve_gpu import oracle_circuit, random_steps
from test_pauli_gpu import oracle as expectation_oracle
from test_rdm_gpu import oracle_rdm
from test_wide_gates_gpu import asym

pytestmark = pytest.mark.gpu
BOTH = [(kind, lay) for kind in KINDS for lay in LAYOUTS]
both = pytest.mark.parametrize("kind, lay", BOTH, ids=[f"{kind}-{lay}" for kind, lay in BOTH])
GAMMA = 0.37
H2 = np.array([[1, 1], [1, -1]], dtype=np.complex128) / math.sqrt(2)


# ---- the case record and its runner --------------------------------------------------------------------------------------------
class Case:
    """One call on `hosts` (LOGICAL arrays of one layout, all in one store) and `extras` (one-element or short float64 arrays,
    each in a banded store of its own).  make() builds the device objects and returns op(*states, *extras) -> tensors or None;
    verify(hosts, after, outs, extras) holds (b) and (d) on host arrays.  unit: the largest number of elements the plan moves at
    once, from the info call."""

    def __init__(self, label, kind, shape, strides, hosts, unit, make, verify, extras=()):
        self.label, self.kind, self.shape, self.strides = label, kind, tuple(shape), tuple(int(s) for s in strides)
        self.hosts, self.unit, self.make, self.verify, self.extras = hosts, int(unit), make, verify, list(extras)
        self.band = band_for(self.unit)
        assert self.band >= self.unit >= 1 and self.band >= MIN_BAND, (label, self.band, self.unit)
        assert all(h.size <= 1 << 14 for h in hosts), label


def layout_of(shape, kind, lay):
    t = strided_empty(shape, kind, lay, device="cpu")
    return tuple(t.shape), tuple(t.stride())


def dim_at(strides, bit):
    """The dim of a (2,) * nq layout that lies on memory bit `bit`."""
    return list(strides).index(1 << bit)


def layouts(shape):
    """The layouts that differ for this shape (the permuted one rotates the top three dims)."""
    return LAYOUTS if len(shape) >= 3 else LAYOUTS[:1]


def nothing(x):
    """For an in-place call: its result is its argument, which the runner compares anyway."""
    return None


def _tuple(x):
    if x is None:
        return ()
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def run(case):
    npdt = KINDS[case.kind][0]
    op = case.make()
    for which, offset in enumerate(offsets_of(npdt)):
        label = f"{case.label} offset {offset}"
        mems = [memory_of(h, case.strides) for h in case.hosts]
        store, views, lay = banded(mems, case.shape, case.strides, npdt, offset, case.band, DEV)
        ex = [banded([e], (e.size,), (1,), e.dtype, offsets_of(e.dtype)[which], MIN_BAND, DEV) for e in case.extras]
        for v in views + [e[1][0] for e in ex]:
            assert v.data_ptr() % 16 == 0 and (which != 2 or v.data_ptr() % 32 != 0), label
            assert which == 0 or v.data_ptr() != v.untyped_storage().data_ptr()
        plain = []
        for h in case.hosts:
            p = torch.empty_strided(case.shape, case.strides, dtype=KINDS[case.kind][1], device=DEV)
            p.copy_(torch.from_numpy(np.ascontiguousarray(h)).to(DEV).reshape(case.shape))
            plain.append(p)
        plain_ex = [torch.from_numpy(e.copy()).to(DEV) for e in case.extras]
        outs = _tuple(op(*views, *[e[1][0] for e in ex]))
        twin = _tuple(op(*plain, *plain_ex))
        torch.cuda.synchronize()
        assert_bands_intact(store, lay, label)                                               # (a)
        for s, l in [(e[0], e[2]) for e in ex]:
            assert_bands_intact(s, l, label + " (one-element store)")
        after_mem = states_of(store, lay)
        for j, (got, p) in enumerate(zip(after_mem, plain)):                                 # (c)
            want = torch.as_strided(p, (got.size,), (1,), 0).cpu().numpy()
            assert same_bits(got, want), f"{label}: state {j} differs from the run on a plain tensor"
        assert len(outs) == len(twin)
        outs_host = [o.cpu().numpy() for o in outs]
        for j, (o, t) in enumerate(zip(outs_host, twin)):
            assert same_bits(o, t.cpu().numpy()), f"{label}: output {j} differs from the run on a plain tensor"
        extras_after = [states_of(e[0], e[2])[0] for e in ex]
        for e, a in zip(case.extras, extras_after):                                          # (d): a uniform is only read
            assert same_bits(e, a), label
        after = [logical_of(m, case.shape, case.strides) for m in after_mem]
        case.verify(case.hosts, after, outs_host, extras_after)                              # (b), (d)


def run_all(cases):
    count = 0
    for case in cases:
        run(case)
        count += 1
    assert count >= 1
    print(f"{count} cases x 3 offsets")


# ---- 1. gate, Pauli and pair runs: tiles of 2^10, blocks of 2^rank tiles ---------------------------------------------------------
def string_of(nq, letters):
    return "".join(letters.get(d, "I") for d in range(nq))


def run_sizes(rank):
    """Fewer dims than a tile, one tile, and the block of 2^rank tiles that is the whole state (max_rank=0: one launch per high gate)."""
    return sorted({1, 2, 5, 9, 10, 10 + rank} | ({12} if rank == 0 else set()))


def gate_list(nq, strides, seed):
    if nq == 1:
        return [(ASYM1, (0,))]
    if nq == 2:
        return [(ASYM2, (0, 1)), (ASYM1, (1,)), (ASYM2, (1, 0))]
    top, low = dim_at(strides, nq - 1), dim_at(strides, 0)
    high = [(ASYM1, (dim_at(strides, b),)) for b in range(10, nq)]
    return random_circuit(np.random.default_rng(seed), nq, 6) + high + [(ASYM2, (top, low)), (ASYM1, (low,)), (ASYM2, (low, top))]


def step_list(nq, strides, seed):
    if nq == 1:
        return [(0.3, "X"), (0.0, 1.0, "Y"), (0.2 - 0.1j, 0.5j, "Z")]
    top, low = dim_at(strides, nq - 1), dim_at(strides, 0)
    high = [(0.4 + 0.1 * b, string_of(nq, {dim_at(strides, b): "X", low: "Z"})) for b in range(10, nq)]
    return random_steps(np.random.default_rng(seed), nq, 5) + high + [(0.3, string_of(nq, {top: "X", low: "Z"})),
                                                                      (0.0, 1.0, string_of(nq, {top: "Z", low: "Y"}))]


def assert_run_form(info, nq, max_rank, label, top_rank):
    """The run plan of this size: the requested ceiling, and at nq = 10 + rank one block that is the whole state."""
    assert info["n_runs"] >= 1 and info["max_rank"] == min(top_rank, max(nq - 10, 0)), (label, info["max_rank"], top_rank)
    ranks = info["run_rank"]
    assert max(ranks) <= max(nq - 10, 0) or nq < 10, label
    if nq == 10 + top_rank and top_rank > 0:
        assert max(ranks) == top_rank, (label, ranks)
    if max_rank == 0 and nq > 10:
        assert info["n_runs"] >= 2, label
    return 1 << (10 + max(ranks))


def default_rank(info_fn, kind, *rest):
    """The effective max_rank of a family's run plan at the default setting (from its info call on a (2,) * 14 state)."""
    shape, strides = layout_of((2,) * 14, kind, "contiguous")
    return info_fn(shape, strides, *rest, KINDS[kind][1])["max_rank"]


def gate_circuit_cases(kind, lay, max_rank):
    dt = KINDS[kind][1]
    top_rank = 0 if max_rank == 0 else default_rank(A.gate_circuit_info, kind, [(ASYM1, (0,))])
    for nq in run_sizes(top_rank):
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        gates = gate_list(nq, strides, 8100 + nq)
        label = f"GateCircuit nq {nq} max_rank {max_rank} {kind} {lay}"
        info = A.gate_circuit_info(shape, strides, gates, dt, max_rank)
        unit = assert_run_form(info, nq, max_rank, label, top_rank)
        used = {b for bits in info["bits"] for b in bits}
        assert {0, nq - 1} <= used, label

        def verify(hosts, after, outs, extras, gates=gates, label=label):
            gate_check(after[0], gate_oracle(hosts[0], gates), hosts[0], gates, kind, label)

        yield Case(label, kind, shape, strides, [crand(8200 + nq, shape, kind)], unit,
                   lambda shape=shape, strides=strides, gates=gates: A.GateCircuit(shape, strides, dt, gates, DEV, max_rank), verify)


def pauli_circuit_cases(kind, lay, max_rank):
    dt = KINDS[kind][1]
    top_rank = 0 if max_rank == 0 else default_rank(A.pauli_evolve_info, kind, [(0.3, "X" + "I" * 13)])
    for nq in run_sizes(top_rank):
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        steps = step_list(nq, strides, 8300 + nq)
        label = f"PauliCircuit nq {nq} max_rank {max_rank} {kind} {lay}"
        info = A.pauli_evolve_info(shape, strides, steps, dt, max_rank)
        unit = assert_run_form(info, nq, max_rank, label, top_rank)
        assert max(info["xmask"]) >= 1 << (nq - 1) and any(z & 1 for z in info["zmask"]), label

        def verify(hosts, after, outs, extras, steps=steps, label=label):
            evolve_check(after[0], oracle_circuit(hosts[0], steps), hosts[0], steps, kind, label)

        yield Case(label, kind, shape, strides, [crand(8400 + nq, shape, kind)], unit,
                   lambda shape=shape, strides=strides, steps=steps: A.PauliCircuit(shape, strides, dt, steps, DEV, max_rank), verify)


def pauli_pair_cases(kind, lay, max_rank):
    dt = KINDS[kind][1]
    top_rank = 0 if max_rank == 0 else default_rank(A.pauli_adjoint_info, kind, [(0.3, "X" + "I" * 13)])
    for nq in run_sizes(top_rank):
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        steps = step_list(nq, strides, 8500 + nq)
        label = f"PauliPairCircuit nq {nq} max_rank {max_rank} {kind} {lay}"
        info = A.pauli_adjoint_info(shape, strides, steps, dt, None, max_rank)
        unit = assert_run_form(info, nq, max_rank, label, top_rank)
        assert info["n_launches"] == info["n_runs"] + 1 and info["n_measured"] == len(steps), label

        def verify(hosts, after, outs, extras, steps=steps, label=label):
            t, want_lam, want_phi = oracle_pair(hosts[0], hosts[1], steps)
            got = outs[0].view(np.complex128).reshape(-1)
            assert got.shape == t.shape and np.abs(got - t).max() <= pauli_pair_bound(kind, steps, hosts[0], hosts[1]), label
            evolve_check(after[0], want_lam, hosts[0], steps, kind, label + " lam")
            evolve_check(after[1], want_phi, hosts[1], steps, kind, label + " phi")

        def make(shape=shape, strides=strides, steps=steps):
            circ = A.PauliPairCircuit(shape, strides, dt, steps, DEV, None, max_rank)
            return lambda lam, phi: circ(lam, phi, device=True)

        yield Case(label, kind, shape, strides, [crand(8600 + nq, shape, kind), crand(8650 + nq, shape, kind)], unit, make, verify)


def gate_pair_cases(kind, lay, max_rank):
    dt = KINDS[kind][1]
    top_rank = 0 if max_rank == 0 else default_rank(A.gate_adjoint_info, kind, [(ASYM1, (0,))])
    for nq in run_sizes(top_rank):
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        gates = gate_list(nq, strides, 8700 + nq)
        ms = random_measures(np.random.default_rng(8750 + nq), gates)
        label = f"GatePairCircuit nq {nq} max_rank {max_rank} {kind} {lay}"
        info = A.gate_adjoint_info(shape, strides, gates, dt, ms, max_rank)
        unit = assert_run_form(info, nq, max_rank, label, top_rank)
        assert info["n_launches"] == info["n_runs"] + 1 and info["n_measured"] == len(gates), label

        def verify(hosts, after, outs, extras, gates=gates, ms=ms, label=label):
            t, want_lam, want_phi = oracle_gate_pair(hosts[0], hosts[1], gates, ms)
            got = outs[0].view(np.complex128).reshape(-1)
            assert got.shape == t.shape and np.all(np.abs(got - t) <= element_bounds(kind, gates, ms, hosts[0], hosts[1])), label
            gate_check(after[0], want_lam, hosts[0], gates, kind, label + " lam")
            gate_check(after[1], want_phi, hosts[1], gates, kind, label + " phi")

        def make(shape=shape, strides=strides, gates=gates, ms=ms):
            circ = A.GatePairCircuit(shape, strides, dt, gates, DEV, ms, max_rank)
            return lambda lam, phi: circ(lam, phi, device=True)

        yield Case(label, kind, shape, strides, [crand(8800 + nq, shape, kind), crand(8850 + nq, shape, kind)], unit, make, verify)


RANKS = pytest.mark.parametrize("max_rank", [None, 0])


@both
@RANKS
def test_gate_circuit(max_rank, kind, lay):
    run_all(gate_circuit_cases(kind, lay, max_rank))


@both
@RANKS
def test_pauli_circuit(max_rank, kind, lay):
    run_all(pauli_circuit_cases(kind, lay, max_rank))


@both
@RANKS
def test_pauli_pair_circuit(max_rank, kind, lay):
    run_all(pauli_pair_cases(kind, lay, max_rank))


@both
@RANKS
def test_gate_pair_circuit(max_rank, kind, lay):
    run_all(gate_pair_cases(kind, lay, max_rank))


# ---- 2. the tile kernels: wide gates, matrix-core gates, controlled gates, channels ----------------------------------------------
def tile_bits_of(kind):
    return N.WGATE_TILE_BITS[N.ARTN_C64 if kind == "c64" else N.ARTN_C128]


def tile_sizes(kind, smallest):
    tb = tile_bits_of(kind)
    return sorted({smallest, tb - 1, tb, tb + 1})


def target_bits(nq, k):
    """k memory bits of a 2^nq state that include the top bit and bit 0, in an order that is neither ascending nor descending."""
    first = [b for b in (nq - 1, 0, nq // 2, 1, nq - 2, 2, nq - 3) if 0 <= b < nq]
    bits = list(dict.fromkeys(first + list(range(nq))))[:k]
    assert len(bits) == k and (k < 2 or {nq - 1, 0} <= set(bits))
    return bits


def assert_tile_form(info, nq, kind, bits, label):
    tb = min(nq, tile_bits_of(kind))
    assert info["tb"] == tb and info["n_tiles"] == 1 << (nq - tb) and tuple(info["target_bits"]) == tuple(bits), (label, info)
    return 1 << info["tb"]


def dense_gate_cases(kind, lay, family, k):
    dt = KINDS[kind][1]
    info_fn, cls = {"wide": (A.wide_gate_info, A.WideGate), "matrix": (A.matrix_gate_info, A.MatrixGate)}[family]
    for nq in tile_sizes(kind, k):
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        bits = target_bits(nq, k)
        dims = tuple(dim_at(strides, b) for b in bits)
        m = asym(k, nq)
        label = f"{cls.__name__} k {k} nq {nq} {kind} {lay}"
        unit = assert_tile_form(info_fn(shape, strides, m, dims, dt), nq, kind, bits, label)

        def verify(hosts, after, outs, extras, m=m, dims=dims, label=label):
            if family == "wide":
                gate_check(after[0], gate_oracle(hosts[0], [(m, dims)]), hosts[0], [(m, dims)], kind, label)
                return
            exact = mgate_oracle(hosts[0], m, dims)
            lim = mgate_bound(exact, cover(hosts[0], m, dims), k, kind == "c64")
            err = np.abs(components(after[0].astype(np.complex128)) - components(exact))
            assert (err <= lim).all(), f"{label}: worst error / bound = {(err / np.maximum(lim, 1e-300)).max():.3f}"

        yield Case(label, kind, shape, strides, [crand(9000 + 10 * nq + k, shape, kind)], unit,
                   lambda shape=shape, strides=strides, m=m, dims=dims: cls(shape, strides, dt, m, dims, DEV), verify)


def mixed_circuit_cases(kind, lay, family):
    """FusedCircuit / BlockCircuit: stretches of narrow gates around wide (and, for BlockCircuit, matrix-core) gates, one tile
    more than a tile kernel holds."""
    dt = KINDS[kind][1]
    nq = tile_bits_of(kind) + 1
    shape, strides = layout_of((2,) * nq, kind, lay)
    narrow = gate_list(nq, strides, 9100)
    wide = [(asym(k, 7), tuple(dim_at(strides, b) for b in target_bits(nq, k))) for k in ((3, 5) if family == "fused" else (3, 6))]
    gates = narrow[:4] + [wide[0]] + narrow[4:] + [wide[1]]
    cls = A.FusedCircuit if family == "fused" else A.BlockCircuit
    label = f"{cls.__name__} nq {nq} {kind} {lay}"
    ninfo = A.gate_circuit_info(shape, strides, narrow, dt)
    units = [1 << (10 + max(ninfo["run_rank"]))]
    for m, dims in wide:
        info = (A.matrix_gate_info if len(dims) > 5 else A.wide_gate_info)(shape, strides, m, dims, dt)
        assert info["n_tiles"] == 2, label
        units.append(1 << info["tb"])

    def verify(hosts, after, outs, extras):
        gate_check(after[0], gate_oracle(hosts[0], gates), hosts[0], gates, kind, label)

    def make():
        circ = cls(shape, strides, dt, gates, DEV)
        assert circ.n_wide == (2 if family == "fused" else 1) and (family == "fused" or circ.n_matrix == 1)
        return circ

    yield Case(label, kind, shape, strides, [crand(9150, shape, kind)], max(units), make, verify)


@both
@pytest.mark.parametrize("k", [1, 3, 5])
def test_wide_gate(k, kind, lay):
    run_all(dense_gate_cases(kind, lay, "wide", k))


@both
@pytest.mark.parametrize("k", [3, 6, 7])
def test_matrix_gate(k, kind, lay):
    run_all(dense_gate_cases(kind, lay, "matrix", k))


@both
@pytest.mark.parametrize("family", ["fused", "block"])
def test_fused_and_block_circuits(family, kind, lay):
    run_all(mixed_circuit_cases(kind, lay, family))


def controlled_cases(kind, lay):
    """Controls on the two top memory bits (above the tile once the state has more bits than a tile) and on bits 0 and 1 (below);
    control values (1, 0): three quarters of the state must keep their bits."""
    dt = KINDS[kind][1]
    tb = tile_bits_of(kind)
    for t in (1, 2):
        for nq in sorted({t + 2, tb - 1, tb, tb + 1, tb + 2}):
            if lay not in layouts((2,) * nq):
                continue
            shape, strides = layout_of((2,) * nq, kind, lay)
            for where in ("above", "below"):
                tbits, cbits = (list(range(t)), [nq - 1, nq - 2]) if where == "above" else ([nq - 1, nq - 2][:t], [0, 1])
                if where == "below" and t == 2:
                    tbits = [nq - 1, 2]
                targets, controls = tuple(dim_at(strides, b) for b in tbits), tuple(dim_at(strides, b) for b in cbits)
                values = (1, 0)
                m = asym(t, 3 + nq)
                label = f"ControlledGate t {t} nq {nq} controls {where} {kind} {lay}"
                info = A.controlled_gate_info(shape, strides, m, targets, controls, values, dt)
                assert info["control_bits"] == tuple(cbits) and info["target_bits"] == tuple(tbits), (label, info)
                assert info["n_selected"] == 1 << (nq - 2) and info["tb"] <= tb, (label, info)
                if nq >= tb + 2:
                    assert (info["c_high"], info["c_low"]) == ((2, 0) if where == "above" else (0, 2)), (label, info)
                    assert set(cbits).isdisjoint(info["tile_bits"]) == (where == "above"), (label, info)

                def verify(hosts, after, outs, extras, m=m, targets=targets, controls=controls, label=label):
                    h = hosts[0]
                    gate_check(after[0], controlled_oracle(h, m, targets, controls, values), h, [(m, targets)], kind, label)
                    idx = np.indices(h.shape)
                    selected = (idx[controls[0]] == values[0]) & (idx[controls[1]] == values[1])
                    assert selected.sum() == h.size // 4 and same_bits(after[0][~selected], h[~selected]), label + ": unselected elements changed"

                yield Case(label, kind, shape, strides, [crand(9200 + 10 * nq + t, shape, kind)], 1 << info["tb"],
                           lambda shape=shape, strides=strides, m=m, targets=targets, controls=controls:
                           A.ControlledGate(shape, strides, dt, m, targets, controls, DEV, values), verify)


def conditioned_cases(kind, lay):
    """ControlledGate(condition=when(c, equals=6)): the int64 the condition reads sits in a banded one-element store; 6 applies
    the gate, 5 leaves every bit of the state."""
    dt = KINDS[kind][1]
    nq = tile_bits_of(kind) + 1
    shape, strides = layout_of((2,) * nq, kind, lay)
    for where in ("above", "below"):
        for flag in (6, 5):
            tbits, cbits = ([0], [nq - 1, nq - 2]) if where == "above" else ([nq - 1], [0, 1])
            targets, controls = tuple(dim_at(strides, b) for b in tbits), tuple(dim_at(strides, b) for b in cbits)
            m = asym(1, 5)
            label = f"ControlledGate under a condition, flag {flag}, controls {where} {kind} {lay}"
            info = A.controlled_gate_info(shape, strides, m, targets, controls, None, dt)
            assert info["n_tiles"] >= 1 and info["n_selected"] == 1 << (nq - 2), (label, info)

            def verify(hosts, after, outs, extras, flag=flag, targets=targets, controls=controls, label=label):
                h = hosts[0]
                assert int(extras[0][0]) == flag
                if flag != 6:
                    assert same_bits(after[0], h), label + ": the condition does not hold, yet the state changed"
                    return
                gate_check(after[0], controlled_oracle(h, m, targets, controls, (1, 1)), h, [(m, targets)], kind, label)

            def make(targets=targets, controls=controls):
                g = A.ControlledGate(shape, strides, dt, m, targets, controls, DEV)
                return lambda a, c: nothing(g(a, condition=A.when(c, equals=6)))

            yield Case(label, kind, shape, strides, [crand(9250 + flag, shape, kind)], 1 << info["tb"], make, verify,
                       extras=[np.array([flag], dtype=np.int64)])


@both
def test_controlled_gate(kind, lay):
    run_all(controlled_cases(kind, lay))


@both
def test_controlled_gate_under_a_condition_tensor(kind, lay):
    run_all(conditioned_cases(kind, lay))


CHANNELS = {
    "FIXED": lambda: (A.depolarizing(0.6, 1), CO.depolarizing(0.6, 1)[0], CO.depolarizing(0.6, 1)[1]),
    "DIAGONAL": lambda: (A.amplitude_damping(0.3), CO.effects(CO.amplitude_damping(0.3), CO.DIAGONAL), CO.amplitude_damping(0.3)),
    "DENSE": lambda: (A.Channel.from_kraus([H2 @ k @ H2 for k in CO.amplitude_damping(0.3)]),
                      CO.effects([H2 @ k @ H2 for k in CO.amplitude_damping(0.3)], CO.DENSE), [H2 @ k @ H2 for k in CO.amplitude_damping(0.3)]),
}


def channel_cases(kind, lay, form, how="step"):
    """ChannelOp.step on the top and on the bottom memory bit; the uniform sits in the middle of the interval of the pick, in a
    banded one-element store.  A FIXED pick of 0 is an exact identity: the state keeps its bits."""
    dt = KINDS[kind][1]
    ch, packed, mats = CHANNELS[form]()
    count = 0
    for nq in tile_sizes(kind, 1):
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        for bit in sorted({nq - 1, 0}):
            dims = [dim_at(strides, bit)]
            pick = count % len(mats)
            count += 1
            label = f"ChannelOp {form} {how} nq {nq} bit {bit} pick {pick} {kind} {lay}"
            info = A.channel_info(shape, strides, ch, dims, dt)
            assert info["form"] == form, (label, info)
            unit = assert_tile_form(info, nq, kind, [bit], label)
            h = crand(9300 + 10 * nq + bit, shape, kind)
            w, _ = CO.weights(form, packed, h, dims)
            uu = MO.mid_uniform(w, pick)
            assert measure.choose_outcome(w, uu)[0] == pick == CO.choose(w, uu), label

            def verify(hosts, after, outs, extras, dims=dims, pick=pick, label=label):
                h, rec = hosts[0], outs[0]
                w, trace = CO.weights(form, packed, h, dims)
                j, p, total, scale = CO.record(form, w, trace, float(extras[0][0]))
                if how == "call":                              # op(amps, device=True): (j, p), views of the same record
                    assert int(outs[0].reshape(-1)[0]) == j == pick and abs(float(outs[1].reshape(-1)[0]) - p) <= 1e-12 * p, label
                    gate = (CO.current_matrix(mats[j], scale), tuple(dims))
                    unit = 2 * 2.0 ** -24 if kind == "c64" else 32 * 2.0 ** -53
                    norm = np.linalg.norm(h.astype(np.complex128).reshape(-1)) * gate_growth([gate])
                    err = np.linalg.norm((after[0].astype(np.complex128) - gate_oracle(h, [gate])).reshape(-1))
                    assert err <= (unit + 1e-12) * norm, (label, err)     # (the host's scale: 1e-12 relative from the device's)
                    return
                assert int(rec.view(np.int64)[0]) == j == pick, (label, int(rec.view(np.int64)[0]), j)
                for got, want in ((rec[1], p), (rec[2], total), (rec[3], scale)):
                    assert abs(got - want) <= 1e-12 * abs(want), (label, got, want)
                cur = rec[4:].view(np.complex128).reshape(2, 2)
                assert (cur.view(np.float64) == CO.current_matrix(mats[j], rec[3]).view(np.float64)).all(), label
                if form == "FIXED" and j == 0:
                    assert same_bits(after[0], h), label + ": an exact identity changed the state"
                gate = (cur, tuple(dims))
                gate_check(after[0], gate_oracle(h, [gate]), h, [gate], kind, label)

            def make(shape=shape, strides=strides, dims=dims):
                step = A.ChannelOp(shape, strides, dt, ch, dims, DEV)
                torch.cuda.synchronize()                       # (the table arrives by a non-blocking copy)
                if how == "call":
                    return lambda a, u: step(a, uniform=u, device=True)
                return lambda a, u: step.step(a, uniform=u)

            yield Case(label, kind, shape, strides, [h], unit, make, verify, extras=[np.array([uu])])


@both
@pytest.mark.parametrize("how", ["step", "call"])
@pytest.mark.parametrize("form", list(CHANNELS))
def test_channel_step(form, how, kind, lay):
    run_all(channel_cases(kind, lay, form, how))


# ---- 3. measurement --------------------------------------------------------------------------------------------------------------
def per_workgroup(n, grid):
    return -(-int(n) // max(int(grid), 1))


def round_unit(kind):
    return 2.0 ** -22 if kind == "c64" else 2.0 ** -51         # the rounding terms of test_measure_gpu.DTYPES


def measure_sizes(kind):
    """The state is the measured dims alone; either side of the one-workgroup grid; tile bits - 1, tile bits, tile bits + 1."""
    tb = tile_bits_of(kind)
    return sorted({2, 9, 10, tb - 1, tb, tb + 1})


def measure_cases(kind, lay, what):
    """collapse_ (measure, reset, postselect) and the device=True wrappers, measured dims on the top and bottom memory bits."""
    dt = KINDS[kind][1]
    for nq in measure_sizes(kind):
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        mdims = [dim_at(strides, 0), dim_at(strides, nq - 1)]
        n = 2 ** nq
        info = A.measure_info(shape, strides, mdims, dt)
        assert info["n"] == n and info["memory_bits"] == [0, nq - 1] and info["grid"] >= 1, info
        unit = per_workgroup(n, info["grid"])
        o = (nq + len(what)) % 4
        h = crand(9400 + nq, shape, kind)
        q = MO.probabilities(h, mdims)
        u = MO.mid_uniform(q, o)
        assert measure.choose_outcome(q, u)[0] == o
        label = f"{what} nq {nq} outcome {o} {kind} {lay}"

        def op(a, uu, mdims=mdims, o=o):
            if what in ("measure", "reset", "postselect"):
                qd = A.marginal_probabilities(a, mdims)        # (the marginal the collapse forms again: its record is checked exactly)
                if what == "postselect":
                    return measure.collapse_(a, mdims, outcome=o), qd
                return measure.collapse_(a, mdims, uniform=uu, reset=(what == "reset")), qd
            if what == "postselect_":
                return A.postselect_(a, mdims, o, device=True)
            return getattr(A, what)(a, mdims, uniform=uu, device=True)

        def verify(hosts, after, outs, extras, mdims=mdims, o=o, n=n, label=label):
            h = hosts[0]
            q = MO.probabilities(h, mdims)
            if what in ("measure", "reset", "postselect"):
                rec, qd = outs[0], outs[1].reshape(-1)
                got_o, (prob, total, scale) = int(rec.view(np.int64)[0]), rec[1:].tolist()
                assert got_o == o, (label, got_o)
                assert abs(prob - q[o] / q.sum()) <= born_tol(n) * q[o] / q.sum() and abs(total - q.sum()) <= born_tol(n) * q.sum()
                assert total == np.cumsum(qd)[-1] and prob == qd[o] / total, label
                want_scale = np.sqrt(total / qd[o])
                assert abs(scale - want_scale) <= 2 * np.spacing(want_scale), (label, scale, want_scale)
                want = (MO.reset if what == "reset" else MO.collapsed)(h, mdims, o, scale)
                assert same_bits(after[0], want.astype(h.dtype)), label + ": not the exact collapse"
                return
            if what != "postselect_":
                assert int(outs[0].reshape(-1)[0]) == o, (label, outs[0])
            assert abs(float(outs[-1].reshape(-1)[0]) - q[o] / q.sum()) <= born_tol(n) * q[o] / q.sum(), label
            want = (MO.reset if what == "reset_" else MO.collapsed)(h.astype(np.complex128), mdims, o, 1.0) * MO.scale_of(q, o)
            err = np.linalg.norm((after[0].astype(np.complex128) - want).reshape(-1))
            assert err <= (round_unit(kind) + 2 * born_tol(n)) * np.linalg.norm(want.reshape(-1)), (label, err)

        yield Case(label, kind, shape, strides, [h], unit, lambda op=op: op, verify, extras=[np.array([u])])


@both
@pytest.mark.parametrize("what", ["measure", "reset", "postselect", "measure_", "reset_", "postselect_"])
def test_collapse(what, kind, lay):
    run_all(measure_cases(kind, lay, what))


# ---- 4. diagonal operators, Pauli expectation values and sums ------------------------------------------------------------------
SMALL_SIZES = (1, 9, 10, 11)                                   # (for the Pauli kernels: either side of the one-workgroup form below 2^10)


def z_terms(nq, strides):
    if nq == 1:
        return [(0.5, {}), (2.25, {0: "Z"})]
    top, low, mid = dim_at(strides, nq - 1), dim_at(strides, 0), dim_at(strides, nq // 2)
    return [(0.375, {top: "Z", low: "Z"}), (-1.5, {low: "Z"}), (1.0, {top: "Z", mid: "Z"}), (2.25, {mid: "Z"}), (0.5, {}),
            (-0.1, {dim_at(strides, 1): "Z", top: "Z", mid: "Z"})]


def diagonal_cases(kind, lay, mode):
    dt, npdt = KINDS[kind][1], KINDS[kind][0]
    for nq in SMALL_SIZES:
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        terms = z_terms(nq, strides)
        info = A.diagonal_info(shape, strides, terms, dt)
        assert info["n_tiles"] == 1 << max(nq - info["tile_bits"], 0) and info["K"] == len(terms), info
        f = DO.Plan(shape, strides, terms).values()
        assert np.abs(GAMMA * f).max() <= 8
        label = f"DiagonalOperator.{mode} nq {nq} {kind} {lay}"
        pair = mode.startswith("pair")

        def make(shape=shape, strides=strides, terms=terms):
            diag = A.DiagonalOperator(shape, strides, dt, terms, DEV)
            if mode == "evolve_":
                return lambda a: nothing(diag.evolve_(a, GAMMA))
            if mode == "multiply_":
                return lambda a: (diag.multiply_(a), A.diagonal_values(diag))[1]
            if mode == "moments":
                return lambda a: (diag.moments(a, device=True),) + tuple(diag.expectation(a, device=True))
            return lambda x, y: diag.pair_(x, y, GAMMA, device=True, evolve=(mode == "pair_evolve"))

        def verify(hosts, after, outs, extras, strides=strides, f=f, label=label):
            mems, got = [memory_of(h, strides) for h in hosts], [memory_of(a, strides) for a in after]
            evolved = mode in ("evolve_", "pair_evolve")
            for a, g in zip(mems, got):
                if evolved:
                    assert (np.abs(g.astype(np.complex128) - DO.phase(a, f, GAMMA)) <= phase_bound(a, f, GAMMA, kind)).all(), label
                elif mode == "multiply_":
                    assert diag_same_bits(g, DO.multiply(a, f, npdt)), label
                else:
                    assert same_bits(g, a), label + ": a state that is only read changed"
            if mode == "multiply_":
                assert diag_same_bits(memory_of(outs[0], strides), f), label
            if mode == "moments":
                want, scale = DO.moments(mems[0], f)
                mom, e, var = outs
                assert (np.abs(mom - want) <= 1e-12 * scale).all(), label
                assert abs(e - want[1] / want[0]) <= 2e-12 * scale[1] / want[0], label
                assert abs(var - (want[2] / want[0] - (want[1] / want[0]) ** 2)) <= 4e-12 * scale[2] / want[0], label
            if pair:
                want, scale = DO.transition(mems[0], f, mems[1])
                assert abs(complex(*outs[0]) - want) <= 1e-12 * scale, label

        hosts = [crand(9500 + nq + 50 * j, shape, kind) for j in range(2 if pair else 1)]
        yield Case(label, kind, shape, strides, hosts, 1 << min(info["tile_bits"], nq), make, verify)


@both
@pytest.mark.parametrize("mode", ["evolve_", "multiply_", "moments", "pair_evolve", "pair_read"])
def test_diagonal(mode, kind, lay):
    run_all(diagonal_cases(kind, lay, mode))


def pauli_strings(nq, strides):
    if nq == 1:
        return [{0: "X"}, {0: "Y"}, {0: "Z"}, {}]
    top, low, mid = dim_at(strides, nq - 1), dim_at(strides, 0), dim_at(strides, nq // 2)
    return [{low: "X", top: "Z"}, {dim_at(strides, 1): "Y", mid: "X"}, {top: "Z", low: "Z"}, {low: "X", top: "Y", mid: "Z"}, {top: "X"}, {},
            {low: "X", mid: "Z"}]


def pauli_expectation_cases(kind, lay):
    dt = KINDS[kind][1]
    for nq in SMALL_SIZES:
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        strings = pauli_strings(nq, strides)
        info = A.pauli_info(shape, strides, strings, dt)
        assert info["n_groups"] >= 2 and max(info["xmask"]) >= 1 << (nq - 1), info
        n = 2 ** nq
        label = f"pauli_expectation nq {nq} {kind} {lay}"

        def verify(hosts, after, outs, extras, strings=strings, n=n, label=label):
            assert same_bits(after[0], hosts[0]), label + ": the state is only read"
            nrm, raw = outs
            for k, p in enumerate(strings):
                w, norm2 = expectation_oracle(hosts[0], p)
                assert abs(raw[k] - w) <= born_tol(n) * norm2 and abs(nrm[k] - w / norm2) <= 2 * born_tol(n), (label, p)

        yield Case(label, kind, shape, strides, [crand(9600 + nq, shape, kind)], n,
                   lambda strings=strings: lambda a: (A.pauli_expectation(a, strings, device=True),
                                                      A.pauli_expectation(a, strings, normalize=False, device=True)), verify)


def pauli_sum_cases(kind, lay):
    """PauliSumOperator with out=: the operand and the result share one store, one band apart; out starts as other data."""
    dt = KINDS[kind][1]
    for nq in SMALL_SIZES:
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        coeffs = [0.7, -1.1, 0.4, 1.3, 0.9 - 0.2j, 0.25, -0.6j]
        terms = list(zip(coeffs, pauli_strings(nq, strides)))
        info = A.pauli_apply_info(shape, strides, terms, dt)
        assert info["n_groups"] >= 2 and info["n_launches"] == 1 and (nq <= 10 or info["n_xmask_hi"] >= 1), info
        label = f"PauliSumOperator out= nq {nq} {kind} {lay}"

        def verify(hosts, after, outs, extras, terms=terms, label=label):
            assert same_bits(after[0], hosts[0]), label + ": amps is only read"
            want = oracle_sum(hosts[0], terms)
            apply_check(after[1], want, hosts[0], terms, kind, label)
            apply_check(outs[0], want, hosts[0], terms, kind, label + " out=None")
            assert same_bits(outs[0], after[1]), label

        def make(shape=shape, strides=strides, terms=terms):
            ham = A.PauliSumOperator(shape, strides, dt, terms, DEV)

            def op(x, y):
                assert ham(x, out=y) is y
                return ham(x)
            return op

        yield Case(label, kind, shape, strides, [crand(9700 + nq, shape, kind), crand(9750 + nq, shape, kind)], 2 ** nq, make, verify)


@both
def test_pauli_expectation(kind, lay):
    run_all(pauli_expectation_cases(kind, lay))


@both
def test_pauli_sum_operator_with_out(kind, lay):
    run_all(pauli_sum_cases(kind, lay))


# ---- 5. bit permutations on raw bit patterns -------------------------------------------------------------------------------------
def raw_patterns(seed, shape, kind):
    """Every bit pattern is data (NaNs and denormals included): the permutation moves bytes."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    words = rng.integers(0, 1 << 63, size=n * (1 if kind == "c64" else 2), dtype=np.uint64)
    return words.view(KINDS[kind][0]).reshape(shape)


def bit_permutation_cases(kind, lay):
    dt = KINDS[kind][1]
    u = np.uint64 if kind == "c64" else np.dtype([("re", np.uint64), ("im", np.uint64)])
    for nq in (3, 10, 13):
        shape, strides = layout_of((2,) * nq, kind, lay)
        for name, dst in (("reversal", [nq - 1 - b for b in range(nq)]), ("shift", [(b + 1) % nq for b in range(nq)])):
            info = A.bit_permutation_info(shape, strides, dt, dst_bit=dst)
            assert info["passes"] >= 1 and info["moved"] >= 2, info
            unit = max(1 << p["tb"] for p in info["pass_info"])
            label = f"BitPermutation {name} nq {nq} {kind} {lay}"

            def verify(hosts, after, outs, extras, strides=strides, dst=dst, label=label):
                want = BO.permute_bits(memory_of(hosts[0], strides).view(u), dst)
                assert np.array_equal(memory_of(after[0], strides).view(u), want), label

            def make(shape=shape, strides=strides, dst=dst):
                perm = A.BitPermutation(shape, strides, dt, dst_bit=dst, device=DEV)
                return lambda a: nothing(perm(a))

            yield Case(label, kind, shape, strides, [raw_patterns(9800 + nq, shape, kind)], unit, make, verify)


@both
def test_bit_permutation(kind, lay):
    run_all(bit_permutation_cases(kind, lay))


# ---- 6. Born statistics, reduced density matrices --------------------------------------------------------------------------------
FLAT = (1, 3, 1000, 1024, 4100)
BLOCKS = {1: 1, 3: 1, 1000: 1, 1023: 1, 1024: 1, 1025: 2, 4100: 5}    # blocks of 2^10 elements = workgroups of the reductions


def born_flat_cases(kind):
    """overlap, norm2, fidelity, block_sums and sample (explicit uniforms in a banded store of their own)."""
    dt = KINDS[kind][1]
    for n in FLAT:
        shape, strides = (n,), (1,)
        plan = born.born_plan(n, dt)
        assert plan["block_bits"] == 10 and plan["n_blocks"] == plan["overlap_grid"] == BLOCKS[n], (n, plan)    # one block, or five with a tail of 4
        label = f"born n {n} {kind}"
        uniforms = np.concatenate([[0.0, 1.0 - 2.0 ** -53], np.random.default_rng(9900 + n).random(62)])

        def op(x, y, uu):
            bs, prefix = born.block_sums(x)
            idx, prob = A.sample(x, uniforms=uu)
            return A.overlap(x, y, device=True), A.norm2(x, device=True), A.fidelity(x, y, device=True), bs, prefix, idx, prob

        def verify(hosts, after, outs, extras, n=n, plan=plan, label=label, uniforms=uniforms):
            ha, hb = hosts
            assert same_bits(after[0], ha) and same_bits(after[1], hb), label + ": the states are only read"
            na, nb = sq(ha).sum(), sq(hb).sum()
            inner = np.vdot(ha.astype(np.complex128), hb.astype(np.complex128))
            ov, n2, fid, bs, prefix, idx, prob = outs
            assert abs(complex(ov[0], ov[1]) - inner) <= born_tol(n) * np.sqrt(na * nb) and abs(ov[2] - na) <= born_tol(n) * na, label
            assert abs(ov[3] - nb) <= born_tol(n) * nb and abs(n2 - na) <= born_tol(n) * na, label
            want_f = abs(inner) ** 2 / (na * nb)
            assert abs(fid - want_f) <= 4 * born_tol(n) * max(np.sqrt(want_f), born_tol(n)) + 4 * born_tol(n) * want_f, label
            block = 1 << plan["block_bits"]
            padded = np.zeros(plan["n_blocks"] * block)
            padded[:n] = sq(ha)
            want = padded.reshape(plan["n_blocks"], block).sum(axis=1)
            assert np.abs(bs - want).max() <= born_tol(block) * want.max() and np.abs(prefix - np.cumsum(want)).max() <= born_tol(n) * want.sum()
            check_samples(torch.empty(n), ha, uniforms, torch.from_numpy(idx), torch.from_numpy(prob))

        yield Case(label, kind, shape, strides, [crand(9950 + n, shape, kind), crand(9960 + n, shape, kind)],
                   max(1 << plan["block_bits"], per_workgroup(n, plan["overlap_grid"])), lambda op=op: op, verify, extras=[uniforms])


SHAPES = {"stream": ((2,) * 12, N.MARGINAL_STREAM, N.RDM_STREAM), "generic": ((3,) * 7, N.MARGINAL_GENERIC, N.RDM_GENERIC)}


def marginal_cases(kind, lay, form):
    dt = KINDS[kind][1]
    base, want_kernel, _ = SHAPES[form]
    shape, strides = layout_of(base, kind, lay)
    order = np.argsort(strides)
    keep = [int(order[-1]), int(order[len(order) // 2]), int(order[0])]      # the slowest, a middle and the fastest dim
    info = born.marginal_info(shape, strides, keep, dt)
    assert info["kernel"] == want_kernel, info
    n = int(np.prod(shape))
    label = f"marginal_probabilities {form} {kind} {lay}"

    def verify(hosts, after, outs, extras):
        assert same_bits(after[0], hosts[0]), label
        assert np.abs(outs[0] - oracle_marginal(hosts[0], keep)).max() <= born_tol(n) * sq(hosts[0]).sum(), label

    yield Case(label, kind, shape, strides, [crand(10000, shape, kind)], max(1 << info["chunk_bits"], per_workgroup(n, info["grid"])),
               lambda: lambda a: A.marginal_probabilities(a, keep), verify)


RDM_SHAPES = {"generic": ((2,) * 11, N.RDM_GENERIC), "stream": ((2,) * 12, N.RDM_STREAM), "mixed": ((3, 4, 5, 2, 6), N.RDM_GENERIC)}


def rdm_cases(kind, lay, form):
    dt = KINDS[kind][1]
    base, want_kernel = RDM_SHAPES[form]
    shape, strides = layout_of(base, kind, lay)
    order = np.argsort(strides)
    keep = [int(order[0]), int(order[-1])] + ([int(order[len(order) // 2])] if form != "mixed" else [])
    info = rdm.rdm_info(shape, strides, keep, dt)
    assert info["kernel"] == want_kernel and info["dim"] == int(np.prod([shape[k] for k in keep])), info
    n = int(np.prod(shape))
    label = f"reduced_density_matrix {form} {kind} {lay}"

    def verify(hosts, after, outs, extras):
        assert same_bits(after[0], hosts[0]), label
        want = oracle_rdm(hosts[0], keep)
        diag = want.diagonal().real
        scale = np.sqrt(np.outer(diag, diag))
        assert (np.abs(outs[0].real - want.real) <= born_tol(n) * scale).all() and (np.abs(outs[0].imag - want.imag) <= born_tol(n) * scale).all()

    yield Case(label, kind, shape, strides, [crand(10100, shape, kind)],
               max(1 << info["panel_bits"], per_workgroup(n, max(info["tiles"], 1))), lambda: lambda a: A.reduced_density_matrix(a, keep), verify)


@pytest.mark.parametrize("kind", list(KINDS))
def test_born_on_flat_states(kind):
    run_all(born_flat_cases(kind))


@both
@pytest.mark.parametrize("form", list(SHAPES))
def test_marginals(form, kind, lay):
    run_all(marginal_cases(kind, lay, form))


@both
@pytest.mark.parametrize("form", list(RDM_SHAPES))
def test_reduced_density_matrix(form, kind, lay):
    run_all(rdm_cases(kind, lay, form))


# ---- 7. the Krylov passes ------------------------------------------------------------------------------------------------------
KRYLOV_N = (1, 3, 1023, 1024, 1025, 4100)
COEFFS = np.array([0.7 - 0.2j, 0.0, 1.1j, -0.4])               # the vector of NaNs (x[5]) sits behind the coefficient that is exactly 0


def krylov_cases(kind):
    """Four vectors, w and a vector of NaNs in one store: dots of the four against w, then vs[0] <- a combination that skips the
    NaNs behind its zero coefficient."""
    dt = KINDS[kind][1]
    for n in KRYLOV_N:
        shape, strides = (n,), (1,)
        info = A.krylov_info(shape, strides, 4, dt)
        assert info["n"] == n and info["grid"] == BLOCKS[n] and info["batch"] >= 4, (n, info)      # 1025: a second workgroup for one element
        assert info["dots_launches"] == 1 and info["combine_launches"] == 1, (n, info)             # (four vectors: one batch)
        assert info["dots_workspace_bytes"] == 96 * info["grid"] and info["combine_workspace_bytes"] == 8 * info["grid"], (n, info)
        label = f"krylov n {n} {kind}"
        hosts = [crand(10200 + n + 10 * j, shape, kind) for j in range(5)]
        hosts.append(np.full(shape, complex(float("nan"), float("nan")), dtype=KINDS[kind][0]))

        def op(*x):
            dots, nw = A.krylov_dots(list(x[:4]), x[4], device=True)
            n2 = A.krylov_combine_(x[0], COEFFS, [x[0], x[5], x[2], x[3]], device=True)
            return dots, nw, n2

        def verify(hosts, after, outs, extras, n=n, label=label):
            dots, nw, n2 = outs
            hs = [h.astype(np.complex128) for h in hosts]
            for j in range(4):
                bound = 4 * (n + 4) * 2.0 ** -53 * float(np.sum(np.abs(hs[j]) * np.abs(hs[4])))
                assert abs(complex(*dots[j]) - np.vdot(hs[j], hs[4])) <= bound, (label, j)
            assert abs(nw - sq(hosts[4]).sum()) <= born_tol(n) * sq(hosts[4]).sum(), label
            want, mag = combine_reference(COEFFS[[0, 2, 3]], [hs[0], hs[2], hs[3]])
            for part in (np.real, np.imag):
                slack = 8 * 4 * 2.0 ** -53 * mag + (2.0 ** -24 * np.abs(part(want)) if kind == "c64" else 0.0)
                assert np.all(np.abs(part(after[0]).astype(np.float64) - part(want)) <= slack), label
            assert abs(n2 - sq(after[0]).sum()) <= born_tol(n) * sq(after[0]).sum(), label
            for j in range(1, 6):
                assert same_bits(after[j], hosts[j]), f"{label}: vector {j} is only read"

        yield Case(label, kind, shape, strides, hosts, per_workgroup(n, info["grid"]), lambda op=op: op, verify)


@pytest.mark.parametrize("kind", list(KINDS))
def test_krylov_dots_and_combine(kind):
    run_all(krylov_cases(kind))


@pytest.mark.parametrize("kind", list(KINDS))
def test_krylov_entries_with_a_banded_workspace(kind):
    """krylov_dots and krylov_combine_ allocate `ws` and `out` themselves; here the two library entries they call get both from
    one banded float64 store (one band apart), next to a banded store of the vectors.  The results equal the public calls' bit
    for bit, and no band changes."""
    dt, npdt = KINDS[kind][1], KINDS[kind][0]
    code = N.ARTN_C64 if kind == "c64" else N.ARTN_C128
    m = 4
    for n in KRYLOV_N:
        info = krylov._info(n, dt, m)
        hosts = [crand(10300 + n + 10 * j, (n,), kind) for j in range(m + 1)]
        for which, offset in enumerate(offsets_of(npdt)):
            store, vs, lay = banded(hosts, (n,), (1,), npdt, offset, band_for(per_workgroup(n, info.grid)), DEV)
            for entry in ("dots", "combine"):
                ws_bytes = info.dots_workspace_bytes if entry == "dots" else info.combine_workspace_bytes
                n_out = 2 * m + 1 if entry == "dots" else 4
                mems = [np.zeros(max(ws_bytes // 8, 1)), np.zeros(n_out)]
                fstore, (ws, out), flay = banded(mems, [(mems[0].size,), (n_out,)], [(1,), (1,)], np.float64, offsets_of(np.float64)[which],
                                                 band_for(mems[0].size), DEV)
                table = (ctypes.c_void_p * m)(*[v.data_ptr() for v in vs[:m]])
                stream = N.current_stream_ptr(torch.device(DEV))
                with torch.cuda.device(torch.device(DEV)):
                    if entry == "dots":
                        N.check(N.lib().artn_krylov_dots(table, m, vs[m].data_ptr(), n, code, ws.data_ptr(), ws_bytes, out.data_ptr(), stream))
                        want_dots, want_nw = A.krylov_dots([v.clone() for v in vs[:m]], vs[m].clone(), device=True)
                        want = torch.cat([want_dots.reshape(-1), want_nw.reshape(1)])
                    else:
                        c = np.ascontiguousarray(COEFFS.astype(np.complex128))
                        y = vs[m].clone()
                        want = A.krylov_combine_(y, COEFFS, [v.clone() for v in vs[:m]], device=True).reshape(1)
                        N.check(N.lib().artn_krylov_combine(vs[m].data_ptr(), c.ctypes.data_as(ctypes.c_void_p), table, m, n, code, ws.data_ptr(),
                                                            ws_bytes, out.data_ptr(), stream))
                torch.cuda.synchronize()
                label = f"artn_krylov_{entry} n {n} {kind} offset {offset}"
                assert_bands_intact(fstore, flay, label)
                assert_bands_intact(store, lay, label)
                got = states_of(fstore, flay)[1][:want.numel()]
                assert same_bits(got, want.cpu().numpy()), label
                if entry == "combine":
                    assert same_bits(states_of(store, lay)[m], y.cpu().numpy()), label
                for j in range(m):
                    assert same_bits(states_of(store, lay)[j], hosts[j].reshape(-1)), label


# ---- 8. what the public calls allocate themselves: the marginal, the uniform and the record of a draw ----------------------------
def float_store(mems, which):
    """Short float64 arrays in ONE banded store, one band apart: (store, views, layout)."""
    return banded(mems, [(m.size,) for m in mems], [(1,)] * len(mems), np.float64, offsets_of(np.float64)[which], MIN_BAND, DEV)


def plain_copy(view):
    p = torch.empty_strided(tuple(view.shape), tuple(view.stride()), dtype=view.dtype, device=view.device)
    p.copy_(view)
    return p


@both
@pytest.mark.parametrize("reset", [False, True])
def test_measure_entries_with_banded_marginal_uniform_and_record(reset, kind, lay):
    """collapse_ allocates the marginal q and the 4-double record itself.  Here artn_measure_choose and artn_measure_collapse,
    the two entries it calls, get q, the uniform and the record from one banded float64 store (one band apart) beside the
    banded state: record and state equal the public call's bit for bit, q and the uniform are only read, no band changes."""
    dt, npdt = KINDS[kind][1], KINDS[kind][0]
    lib, dev = N.lib(), torch.device(DEV)
    n_rec = N.MEASURE_RECORD_BYTES // 8
    for nq in measure_sizes(kind):
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        mdims = [dim_at(strides, 0), dim_at(strides, nq - 1)]
        d, _, info = measure._plan(shape, strides, mdims, dt, "measure entries")
        assert info.dim == 4 and info.n == 2 ** nq and info.record_bytes == N.MEASURE_RECORD_BYTES
        h = crand(10400 + nq, shape, kind)
        o = (nq + int(reset)) % 4
        u_host = np.array([MO.mid_uniform(MO.probabilities(h, mdims), o)])
        for which, offset in enumerate(offsets_of(npdt)):
            label = f"artn_measure_choose / _collapse nq {nq} reset {reset} {kind} {lay} offset {offset}"
            store, (a,), lay_a = banded([memory_of(h, strides)], shape, strides, npdt, offset, band_for(per_workgroup(info.n, info.grid)), DEV)
            plain = plain_copy(a)
            want = measure.collapse_(plain, mdims, uniform=torch.from_numpy(u_host).to(DEV), reset=reset)
            q_host = A.marginal_probabilities(a, mdims).reshape(-1).cpu().numpy()
            fstore, (q, u, rec), flay = float_store([q_host, u_host, np.zeros(n_rec)], which)
            assert all(t.data_ptr() % 16 == 0 for t in (q, u, rec)) and (which != 2 or rec.data_ptr() % 32 != 0)
            with torch.cuda.device(dev):
                stream = N.current_stream_ptr(dev)
                N.check(lib.artn_measure_choose(q.data_ptr(), info.dim, u.data_ptr(), -1, 1, rec.data_ptr(), stream))
                N.check(lib.artn_measure_collapse(ctypes.byref(d), a.data_ptr(), rec.data_ptr(), int(reset), stream))
            torch.cuda.synchronize()
            assert_bands_intact(fstore, flay, label)
            assert_bands_intact(store, lay_a, label)
            got_q, got_u, got_rec = states_of(fstore, flay)
            assert same_bits(got_q, q_host) and same_bits(got_u, u_host), label + ": q and the uniform are only read"
            assert same_bits(got_rec, want.cpu().numpy()) and int(got_rec.view(np.int64)[0]) == o, (label, got_rec)
            assert same_bits(states_of(store, lay_a)[0], torch.as_strided(plain, (info.n,), (1,), 0).cpu().numpy()), label
            after = logical_of(states_of(store, lay_a)[0], shape, strides)
            assert same_bits(after, (MO.reset if reset else MO.collapsed)(h, mdims, o, got_rec[3]).astype(npdt)), label + ": not the exact collapse"


@both
@pytest.mark.parametrize("form", list(CHANNELS))
def test_channel_entries_with_banded_source_uniform_and_record(form, kind, lay):
    """ChannelOp.step allocates what the draw reads (a marginal or a reduced density matrix) and the record itself.  Here
    artn_channel_choose and artn_channel_apply get source, uniform and record from one banded float64 store."""
    from artensor_amd._state import _ptr
    dt, npdt = KINDS[kind][1], KINDS[kind][0]
    lib, dev = N.lib(), torch.device(DEV)
    ch, packed, mats = CHANNELS[form]()
    for nq in tile_sizes(kind, 1):
        if lay not in layouts((2,) * nq):
            continue
        shape, strides = layout_of((2,) * nq, kind, lay)
        dims = [dim_at(strides, nq - 1)]
        step = A.ChannelOp(shape, strides, dt, ch, dims, DEV)
        torch.cuda.synchronize()
        h = crand(10500 + nq, shape, kind)
        pick = nq % len(mats)
        u_host = np.array([MO.mid_uniform(CO.weights(form, packed, h, dims)[0], pick)])
        for which, offset in enumerate(offsets_of(npdt)):
            label = f"artn_channel_choose / _apply {form} nq {nq} {kind} {lay} offset {offset}"
            store, (a,), lay_a = banded([memory_of(h, strides)], shape, strides, npdt, offset, band_for(1 << step.tile_bits), DEV)
            plain = plain_copy(a)
            want = step.step(plain, uniform=torch.from_numpy(u_host).to(DEV))
            if form == "DIAGONAL":
                src_host = A.marginal_probabilities(a, dims).reshape(-1).cpu().numpy()
            elif form == "DENSE":
                src_host = np.ascontiguousarray(A.reduced_density_matrix(a, dims).cpu().numpy()).reshape(-1).view(np.float64)
            else:
                src_host = np.zeros(1)                         # (FIXED reads nothing: a null pointer is passed)
            fstore, (src, u, rec), flay = float_store([src_host, u_host, np.zeros(step.record_bytes // 8)], which)
            with torch.cuda.device(dev):
                stream = N.current_stream_ptr(dev)
                N.check(lib.artn_channel_choose(step._table.data_ptr(), step.table_bytes, step.t, step.m, ch.form_code,
                                                None if form == "FIXED" else src.data_ptr(), u.data_ptr(), 1, rec.data_ptr(),
                                                step.record_bytes, stream))
                N.check(lib.artn_channel_apply(ctypes.byref(step._d), a.data_ptr(), step.t, _ptr(step._dims), step.m, step._table.data_ptr(),
                                               step.table_bytes, rec.data_ptr(), step.record_bytes, stream))
            torch.cuda.synchronize()
            assert_bands_intact(fstore, flay, label)
            assert_bands_intact(store, lay_a, label)
            got_src, got_u, got_rec = states_of(fstore, flay)
            assert same_bits(got_src, src_host) and same_bits(got_u, u_host), label + ": source and uniform are only read"
            assert same_bits(got_rec, want.cpu().numpy()) and int(got_rec.view(np.int64)[0]) == pick, (label, got_rec[:4])
            assert same_bits(states_of(store, lay_a)[0], torch.as_strided(plain, (2 ** nq,), (1,), 0).cpu().numpy()), label


def test_linear_xeb_on_banded_probabilities():
    """linear_xeb is torch's mean of the probabilities it is given, no kernel of this library: run on a banded device tensor,
    against numpy at the rounding of a float64 sum of m terms.  (No twin condition: the order of torch's sum is torch's.)"""
    m, nq = 1000, 12
    p = np.random.default_rng(10600).random(m) / 2 ** nq
    for which in range(3):
        store, (v,), lay = float_store([p], which)
        got = A.linear_xeb(v, nq)
        torch.cuda.synchronize()
        assert_bands_intact(store, lay, f"linear_xeb offset {which}")
        assert same_bits(states_of(store, lay)[0], p)
        assert abs(got - (2.0 ** nq * p.mean() - 1.0)) <= m * 2.0 ** -53 * 2.0 ** nq * p.mean()


# what is run by a test of its own instead of a case table: BANDED name -> test
OTHER_TESTS = {"born.linear_xeb": "test_linear_xeb_on_banded_probabilities"}


# ---- the builders, for the host-only run of tests/test_guard_bands_cpu.py --------------------------------------------------------
def all_cases():
    """Every case of this module, built on the host: {BANDED name or names: iterator of cases}."""
    for kind in KINDS:
        yield "born.overlap born.norm2 born.fidelity born.block_sums born.sample", born_flat_cases(kind)
        yield "krylov.krylov_dots krylov.krylov_combine_", krylov_cases(kind)
    for kind, lay in BOTH:
        for max_rank in (None, 0):
            yield "gates.GateCircuit", gate_circuit_cases(kind, lay, max_rank)
            yield "pauli.PauliCircuit", pauli_circuit_cases(kind, lay, max_rank)
            yield "adjoint.PauliPairCircuit", pauli_pair_cases(kind, lay, max_rank)
            yield "gate_adjoint.GatePairCircuit", gate_pair_cases(kind, lay, max_rank)
        for k in (1, 3, 5):
            yield "wide_gates.WideGate", dense_gate_cases(kind, lay, "wide", k)
        for k in (3, 6, 7):
            yield "matrix_gates.MatrixGate", dense_gate_cases(kind, lay, "matrix", k)
        yield "wide_gates.FusedCircuit", mixed_circuit_cases(kind, lay, "fused")
        yield "matrix_gates.BlockCircuit", mixed_circuit_cases(kind, lay, "block")
        yield "controlled.ControlledGate", controlled_cases(kind, lay)
        yield "controlled.ControlledGate", conditioned_cases(kind, lay)
        for form in CHANNELS:
            for how in ("step", "call"):
                yield "channel.ChannelOp", channel_cases(kind, lay, form, how)
        for what in ("measure", "reset", "postselect"):
            yield "measure.collapse_", measure_cases(kind, lay, what)
        for what in ("measure_", "reset_", "postselect_"):
            yield "measure." + what, measure_cases(kind, lay, what)
        for mode in ("evolve_", "multiply_", "moments", "pair_evolve", "pair_read"):
            yield "diagonal.DiagonalOperator diagonal.diagonal_values", diagonal_cases(kind, lay, mode)
        yield "pauli.pauli_expectation", pauli_expectation_cases(kind, lay)
        yield "pauli.PauliSumOperator", pauli_sum_cases(kind, lay)
        yield "layout.BitPermutation", bit_permutation_cases(kind, lay)
        for form in SHAPES:
            yield "born.marginal_probabilities", marginal_cases(kind, lay, form)
        for form in RDM_SHAPES:
            yield "rdm.reduced_density_matrix", rdm_cases(kind, lay, form)
