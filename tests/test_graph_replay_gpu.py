"""Every state operation that promises "enqueues on the current stream and synchronises nowhere", captured ONCE into a HIP graph
(torch.cuda.graph: its own capture stream, one stream, no fork or join) and replayed on contents that change between replays.

Each replay is compared (a) bit for bit with an eager run of the same call on clones on the default stream -- a condition, not a
tolerance: the sums are float64 in a fixed order -- and (b) with the family's existing host reference at that family's existing
bound, imported from its own test module, so that eager and replay cannot be wrong in the same way.  What a replay catches that
an eager run cannot: a launch on the wrong stream or a hidden synchronisation (capture raises), a value read on the host at
enqueue time (every replay repeats the first answer), scratch memory that is only valid on first use, lazy setup that capture
forbids.  The host-only *_info functions assert, before capture, that the multi-tile / multi-launch form is the one taken; the
same assertions run without a GPU in test_the_captured_forms_are_the_multi_tile_ones.

States have 2^16 elements ((2,) * 16, 64 tiles of 2^10) unless a form needs another shape, complex64 and complex128, contiguous
and with the top three dims rotated.

The dynamic circuit (case 5) is compared with a complex128 host run of the same branch.  Its bound, derived: every operation
forms each output component in float64 and rounds it once, ||error|| <= unit ||state|| with unit = 2 2^-24 (complex64) or
32 2^-53 (complex128, the constant of test_gates_gpu; the phase needs (8 + |gamma f|) 2^-52 <= 16 2^-52 for |gamma f| <= 8, also
below it); later operations amplify by at most their 2-norms, G their product; the two renormalisations use a scale from a float64
sum of n terms, 4 n 2^-53 relative each (the bound of test_born_gpu).  Hence
    ||y - ref||_2 <= (unit K + 2 * 4 n 2^-53) ||a||_2 G,       K = gates + collapse + conditioned gate + channel + phase.
With eps that bound relative to the state, a probability of the record differs from the host's by at most 5 eps + 4 n 2^-53
(|dq_o| and |dtotal| <= (2 eps + eps^2) total).  Uniforms sit in the middle of the predicted outcome's interval."""
import math

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import (adjoint, born, channel, controlled, diagonal, gate_adjoint, gates, krylov, layout, measure, pauli, rdm,
                          wide_gates)

import bit_permutation_oracle as BO
import channel_oracle as CO
import diagonal_oracle as DO
import measure_oracle as MO
from adjoint_oracle import oracle_pair
from gates_adjoint_oracle import oracle_gate_pair
from graph_replay import (DEV, KINDS, LAYOUTS, NQ, bits, capture_and_replay, crand, fill, logical_of, memory_of, strided_empty,
                          twin)
from test_born_gpu import oracle_marginal, sq
from test_born_gpu import tol as born_tol
from test_controlled_gates_gpu import controlled_oracle
from test_diagonal_gpu import phase_bound
from test_diagonal_gpu import same_bits as diag_same_bits
from test_gates_adjoint_gpu import element_bounds, random_measures
from test_gates_gpu import ASYM1, ASYM2, growth, random_circuit
from test_gates_gpu import check as gate_check
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

SHAPE = (2,) * NQ
BOTH = [(kind, lay) for kind in KINDS for lay in LAYOUTS]
IDS = [f"{kind}-{lay}" for kind, lay in BOTH]
both = pytest.mark.parametrize("kind, lay", BOTH, ids=IDS)
gpu = pytest.mark.gpu


# ---- the completeness tables (checked without a GPU) ---------------------------------------------------------------------------
MODULES = {"gates": gates, "wide_gates": wide_gates, "controlled": controlled, "pauli": pauli, "adjoint": adjoint,
           "gate_adjoint": gate_adjoint, "diagonal": diagonal, "layout": layout, "channel": channel, "measure": measure, "born": born,
           "rdm": rdm, "krylov": krylov}

# captured and replayed by a test of this module (a class: its call and its device=True methods)
CAPTURED = {
    "gates.GateCircuit", "wide_gates.WideGate", "wide_gates.FusedCircuit", "controlled.ControlledGate", "pauli.PauliCircuit",
    "pauli.PauliSumOperator", "pauli.pauli_expectation", "adjoint.PauliPairCircuit", "gate_adjoint.GatePairCircuit",
    "diagonal.DiagonalOperator", "diagonal.diagonal_values", "layout.BitPermutation", "channel.ChannelOp", "measure.collapse_",
    "measure.measure_", "measure.postselect_", "measure.reset_", "born.overlap", "born.norm2", "born.fidelity", "born.block_sums",
    "born.marginal_probabilities", "rdm.reduced_density_matrix", "krylov.krylov_dots", "krylov.krylov_combine_",
}

_PER_CALL = "per-call convenience: plans, packs and uploads its table from pageable host memory (torch.from_numpy(table).to(device))"
_HOST = "returns host values: ends in a device-to-host copy"
NOT_CAPTURABLE = {
    "gates.apply_gates_": _PER_CALL, "gates.apply_gate_": _PER_CALL, "gates.run_circuit": _PER_CALL,
    "wide_gates.apply_wide_gate_": _PER_CALL, "wide_gates.apply_circuit_": _PER_CALL,
    "controlled.apply_controlled_gate_": _PER_CALL, "controlled.mcx_": _PER_CALL, "controlled.mcz_": _PER_CALL,
    "controlled.mcphase_": _PER_CALL,
    "pauli.pauli_sum_apply": _PER_CALL, "pauli.pauli_apply": _PER_CALL, "pauli.pauli_rotate": _PER_CALL, "pauli.pauli_evolve_": _PER_CALL,
    "pauli.pauli_rotate_": _PER_CALL, "pauli.pauli_apply_": _PER_CALL,
    "pauli.pauli_sum_expectation": _HOST + " (out.cpu().numpy())", "pauli.pauli_sum_variance": _HOST + " (overlap and norm2 with device=False)",
    "adjoint.pauli_evolve_pair_": _PER_CALL, "adjoint.adjoint_gradient": _HOST + " and builds its circuits per call",
    "gate_adjoint.apply_gates_pair_": _PER_CALL, "gate_adjoint.gate_adjoint_gradient": _HOST + " and builds its circuits per call",
    "diagonal.diagonal_evolve_": _PER_CALL, "diagonal.diagonal_expectation": _PER_CALL,
    "diagonal.qaoa_gradient": _HOST + " and builds its circuits per call",
    "layout.permute_dims_": _PER_CALL, "layout.swap_dims_": _PER_CALL, "layout.reverse_qubits_": _PER_CALL, "layout.relayout_": _PER_CALL,
    "channel.channel_": "per-call convenience: builds a ChannelOp (pin_memory() and an upload) in the call",
    "channel.channel_step_": "per-call convenience: builds a ChannelOp (pin_memory() and an upload) in the call",
    "measure.apply_channel_": "synchronises by contract: reduced_density_matrix(amps, dims).cpu()",
    "born.sample": "synchronises by contract: float(total) on the host",
    "born.linear_xeb": _HOST + " (float(...mean()))",
    "rdm.purity": _HOST, "rdm.renyi_entropy": _HOST, "rdm.entanglement_entropy": _HOST, "rdm.expectation": _HOST,
    "krylov.lanczos": "synchronises by contract: the recurrence reads its dots on the host",
    "krylov.lanczos_ground_state": "synchronises by contract: the tridiagonal problem is solved on the host",
    "krylov.krylov_evolve": "synchronises by contract: the tridiagonal problem is solved on the host",
}

# never touch the device: plans, builders of terms, gates and channels, host arithmetic
HOST_ONLY = {
    "gates.gate_circuit_info", "gates.gates_from_bonds", "gates.merge_gates", "wide_gates.wide_gate_info", "wide_gates.fuse_gates",
    "controlled.controlled_gate_info", "controlled.when", "controlled.Condition", "pauli.pauli_ops", "pauli.pauli_info",
    "pauli.pauli_apply_info", "pauli.pauli_evolve_info", "pauli.trotter_steps", "adjoint.pauli_adjoint_info",
    "gate_adjoint.gate_adjoint_info", "gate_adjoint.parametric_gate", "diagonal.diagonal_info", "diagonal.ising_terms",
    "diagonal.maxcut_terms", "layout.bit_permutation_info", "layout.busiest_dims_order", "channel.Channel", "channel.channel_info",
    "channel.depolarizing", "channel.pauli_channel", "channel.bit_flip", "channel.phase_flip", "channel.amplitude_damping",
    "channel.phase_damping", "measure.measure_info", "measure.choose_outcome", "born.born_plan", "born.marginal_info",
    "born.memory_to_multi_index", "rdm.rdm_info", "rdm.entropy_of", "krylov.krylov_info", "krylov.ritz", "krylov.expm_e1",
    "krylov.KrylovResult",
}


def test_every_public_callable_is_in_exactly_one_table():
    public = {f"{name}.{entry}" for name, mod in MODULES.items() for entry in mod.__all__}
    tables = [CAPTURED, set(NOT_CAPTURABLE), HOST_ONLY]
    for i, x in enumerate(tables):
        for y in tables[i + 1:]:
            assert not x & y, sorted(x & y)
    listed = CAPTURED | set(NOT_CAPTURABLE) | HOST_ONLY
    assert listed - public == set(), f"listed, but not public: {sorted(listed - public)}"
    assert public - listed == set(), f"decide whether these are captured in a graph or cannot be: {sorted(public - listed)}"
    assert all(isinstance(r, str) and r and "\n" not in r for r in NOT_CAPTURABLE.values())
    for full in listed:
        mod, entry = full.split(".")
        assert callable(getattr(MODULES[mod], entry)), full


# ---- the operands of the cases, and the host-only assertions that the captured form is the multi-tile one ---------------------
GATES = random_circuit(np.random.default_rng(1601), NQ, 24) + [(ASYM2, (0, 3)), (ASYM1, (1,)), (ASYM2, (2, 0)), (ASYM1, (3,))]
WIDE = {3: (asym(3, 1), (0, 9, 15)), 5: (asym(5, 1), (1, 14, 6, 0, 11))}
FUSED = GATES[:12] + [WIDE[3]] + GATES[12:] + [(asym(4, 2), (2, 13, 5, 1))]
STEPS = random_steps(np.random.default_rng(1602), NQ, 12)
REVERSAL = [NQ - 1 - b for b in range(NQ)]
ORDER = list(range(NQ))[::-1]
ZTERMS = [(0.375, {15: "Z", 14: "Z"}), (-1.5, {0: "Z", 15: "Z"}), (1.0, {0: "Z", 1: "Z"}), (2.25, {2: "Z"}),
          (-0.1, {3: "Z", 7: "Z", 12: "Z"}), (0.5, {}), (0.75, {1: "Z", 13: "Z"})]
GAMMA = 0.37
HTERMS = [(0.7, {0: "X", 15: "Z"}), (-1.1, {1: "Y", 9: "X"}), (0.4, {}), (1.3, {14: "Z", 2: "Z"}), (0.9 - 0.2j, {2: "X", 15: "Y", 7: "Z"}),
          (0.25, {15: "X"})]
STRINGS = [{0: "X", 15: "Z"}, {1: "Y", 9: "X"}, {14: "Z", 2: "Z"}, {2: "X", 15: "Y", 7: "Z"}, {15: "X"}, {}, {0: "X", 3: "Z"}]
MEASURES = random_measures(np.random.default_rng(1603), GATES[:12])
CG = (asym(1, 4), (5,), (1, 14), (1, 0))                       # matrix, targets, controls (none of them measured), control values
MDIMS = [0, 15]
assert not set(CG[2]) & set(MDIMS) and not set(CG[1]) & set(MDIMS)    # (a control on a measured dim would select zeros after the collapse)
H2 = np.array([[1, 1], [1, -1]], dtype=np.complex128) / math.sqrt(2)
CHANNELS = {
    "FIXED": lambda: (A.depolarizing(0.6, 1), CO.depolarizing(0.6, 1)[0], CO.depolarizing(0.6, 1)[1]),
    "DIAGONAL": lambda: (A.amplitude_damping(0.3), CO.effects(CO.amplitude_damping(0.3), CO.DIAGONAL), CO.amplitude_damping(0.3)),
    "DENSE": lambda: (A.Channel.from_kraus([H2 @ k @ H2 for k in CO.amplitude_damping(0.3)]),
                      CO.effects([H2 @ k @ H2 for k in CO.amplitude_damping(0.3)], CO.DENSE), [H2 @ k @ H2 for k in CO.amplitude_damping(0.3)]),
}
GENERIC_SHAPE = (3,) * 8


def high_bit(kind):
    return N.WGATE_TILE_BITS[N.ARTN_C64 if kind == "c64" else N.ARTN_C128]


def assert_forms(shape, strides, kind):
    """Host-only: every case below takes its multi-tile or multi-launch form on a (2,) * 16 state of these strides."""
    dt = KINDS[kind][1]
    for max_rank in (None, 0):
        info = A.gate_circuit_info(shape, strides, GATES, dt, max_rank)
        assert info["n_runs"] >= 2 and max(b for bs in info["bits"] for b in bs) >= 10
    for k, (m, dims) in WIDE.items():
        info = A.wide_gate_info(shape, strides, m, dims, dt)
        assert info["k"] == k and info["n_tiles"] >= 2 and max(info["target_bits"]) >= high_bit(kind)
    narrow = [g for g in FUSED if len(g[1]) <= 2]
    assert A.gate_circuit_info(shape, strides, narrow[:12], dt)["n_runs"] >= 2 and len(FUSED) - len(narrow) == 2
    info = A.pauli_evolve_info(shape, strides, STEPS, dt)
    assert info["n_runs"] >= 2 and max(info["xmask"]) >= 1 << 10
    info = A.bit_permutation_info(shape, strides, dt, dst_bit=REVERSAL)
    assert info["passes"] >= 2
    info = A.bit_permutation_info(shape, strides, dt, order=ORDER)
    assert info["passes"] >= 1 and tuple(info["strides"]) != tuple(strides)
    info = A.diagonal_info(shape, strides, ZTERMS, dt)
    assert info["n_tiles"] == 64 and info["G"] >= 1 and info["n_static"] >= 1 and info["n_dynamic"] >= 1
    info = A.pauli_apply_info(shape, strides, HTERMS, dt)
    assert info["n_groups"] >= 2 and info["n_xmask_hi"] >= 1
    info = A.pauli_adjoint_info(shape, strides, STEPS, dt)
    assert info["n_runs"] >= 2 and info["n_launches"] == info["n_runs"] + 1
    info = A.gate_adjoint_info(shape, strides, GATES[:12], dt, MEASURES)
    assert info["n_runs"] >= 2 and info["n_measured"] == 12
    assert born.born_plan(2 ** NQ, dt)["n_blocks"] >= 2
    assert born.marginal_info(shape, strides, [15, 3, 0], dt)["kernel"] == N.MARGINAL_STREAM
    assert rdm.rdm_info(shape, strides, [0, 9, 15], dt)["kernel"] == N.RDM_STREAM
    info = A.pauli_info(shape, strides, STRINGS, dt)
    assert info["n_groups"] >= 2 and max(info["xmask"]) >= 1 << 10
    info = A.krylov_info(shape, strides, 5, dt)
    assert info["grid"] >= 2 and info["dots_launches"] >= 1 and info["combine_launches"] >= 1
    info = A.measure_info(shape, strides, MDIMS, dt)
    assert info["grid"] >= 2 and info["n"] == 2 ** NQ and max(info["memory_bits"]) >= 10
    for form, make in CHANNELS.items():
        info = A.channel_info(shape, strides, make()[0], [0], dt)
        assert info["form"] == form and info["n_tiles"] >= 2 and max(info["target_bits"]) >= high_bit(kind)
    m, targets, controls, values = CG
    info = A.controlled_gate_info(shape, strides, m, targets, controls, values, dt)
    assert info["c_high"] >= 1 and info["c_low"] >= 1 and info["n_tiles"] >= 2


def assert_generic_forms(shape, strides, kind):
    dt = KINDS[kind][1]
    assert born.marginal_info(shape, strides, [1, 6], dt)["kernel"] == N.MARGINAL_GENERIC
    assert rdm.rdm_info(shape, strides, [1, 6], dt)["kernel"] == N.RDM_GENERIC


@both
def test_the_captured_forms_are_the_multi_tile_ones(kind, lay):
    t = strided_empty(SHAPE, kind, lay, device="cpu")
    assert (lay == "contiguous") == t.is_contiguous()
    assert_forms(t.shape, t.stride(), kind)
    g = strided_empty(GENERIC_SHAPE, kind, lay, device="cpu")
    assert_generic_forms(g.shape, g.stride(), kind)


_FORMS_SEEN = set()


def state(kind, lay, shape=SHAPE):
    t = strided_empty(shape, kind, lay)
    assert (lay == "contiguous") == t.is_contiguous()
    if shape == SHAPE and (kind, lay) not in _FORMS_SEEN:
        assert_forms(t.shape, t.stride(), kind)
        _FORMS_SEEN.add((kind, lay))
    return t


def states(seed0, kind, count=1, shape=SHAPE):
    """contents(r) for `count` state tensors: a different seed per replay (and for the warm-up)."""
    return lambda r: [crand(seed0 + 100 * (r + 1) + j, shape, kind) for j in range(count)]


def npdtype(kind):
    return KINDS[kind][0]


def same(x, y):
    """Two host arrays hold the same bytes."""
    return np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


# ---- 1. in-place circuits ------------------------------------------------------------------------------------------------------
@gpu
@both
@pytest.mark.parametrize("max_rank", [None, 0])
def test_gate_circuit(max_rank, kind, lay):
    t = state(kind, lay)
    circ = A.GateCircuit(t.shape, t.stride(), t.dtype, GATES, DEV, max_rank)
    assert circ.n_runs >= 2

    def verify(r, hosts, after, outs):
        gate_check(after[0], gate_oracle(hosts[0], GATES), hosts[0], GATES, kind, f"GateCircuit max_rank {max_rank} replay {r}")

    capture_and_replay(lambda a: circ(a), [t], states(1100, kind), verify)


@gpu
@both
@pytest.mark.parametrize("k", [3, 5])
def test_wide_gate(k, kind, lay):
    t = state(kind, lay)
    gate = WIDE[k]
    g = A.WideGate(t.shape, t.stride(), t.dtype, gate[0], gate[1], DEV)
    assert g.n_tiles >= 2

    def verify(r, hosts, after, outs):
        gate_check(after[0], gate_oracle(hosts[0], [gate]), hosts[0], [gate], kind, f"WideGate k {k} replay {r}")

    capture_and_replay(lambda a: g(a), [t], states(1200 + k, kind), verify)


@gpu
@both
def test_fused_circuit(kind, lay):
    t = state(kind, lay)
    circ = A.FusedCircuit(t.shape, t.stride(), t.dtype, FUSED, DEV)
    assert circ.n_wide == 2 and circ.n_launches >= 5 and any(getattr(p, "n_runs", 0) >= 2 for p in circ.parts)

    def verify(r, hosts, after, outs):
        gate_check(after[0], gate_oracle(hosts[0], FUSED), hosts[0], FUSED, kind, f"FusedCircuit replay {r}")

    capture_and_replay(lambda a: circ(a), [t], states(1300, kind), verify)


@gpu
@both
def test_pauli_circuit(kind, lay):
    t = state(kind, lay)
    circ = A.PauliCircuit(t.shape, t.stride(), t.dtype, STEPS, DEV)
    assert circ.n_runs >= 2

    def verify(r, hosts, after, outs):
        evolve_check(after[0], oracle_circuit(hosts[0], STEPS), hosts[0], STEPS, kind, f"PauliCircuit replay {r}")

    capture_and_replay(lambda a: circ(a), [t], states(1400, kind), verify)


@gpu
@both
@pytest.mark.parametrize("how", ["dst_bit", "order"])
def test_bit_permutation(how, kind, lay):
    t = state(kind, lay)
    strides = t.stride()
    perm = A.BitPermutation(t.shape, strides, t.dtype, device=DEV, **({"dst_bit": REVERSAL} if how == "dst_bit" else {"order": ORDER}))
    assert perm.passes >= (2 if how == "dst_bit" else 1)
    u = np.uint64 if kind == "c64" else np.dtype([("re", np.uint64), ("im", np.uint64)])

    def verify(r, hosts, after, outs):
        if how == "dst_bit":                                   # new[pi(i)] == old[i], bit for bit, in memory
            want = BO.permute_bits(memory_of(hosts[0], strides).view(u), REVERSAL)
            assert np.array_equal(memory_of(after[0], strides).view(u), want)
        else:                                                  # the returned view shows the old logical tensor
            assert np.array_equal(np.ascontiguousarray(outs[0]).view(u), np.ascontiguousarray(hosts[0]).view(u))

    def op(a):
        out = perm(a)
        if how == "dst_bit":
            assert out is a
            return None
        assert out.stride() != a.stride() and out.stride() == perm.new_strides and out.data_ptr() == a.data_ptr()
        return out

    capture_and_replay(op, [t], states(1500, kind), verify)


@gpu
@both
@pytest.mark.parametrize("mode", ["evolve_", "multiply_"])
def test_diagonal_in_place(mode, kind, lay):
    t = state(kind, lay)
    strides = t.stride()
    diag = A.DiagonalOperator(t.shape, strides, t.dtype, ZTERMS, DEV)
    f = DO.Plan(SHAPE, strides, ZTERMS).values()
    assert np.abs(GAMMA * f).max() <= 8

    def op(a):
        if mode == "evolve_":
            assert diag.evolve_(a, GAMMA) is a
            return None
        assert diag.multiply_(a) is a
        return A.diagonal_values(diag)

    def verify(r, hosts, after, outs):
        a, got = memory_of(hosts[0], strides), memory_of(after[0], strides)
        if mode == "evolve_":
            err = np.abs(got.astype(np.complex128) - DO.phase(a, f, GAMMA))
            assert (err <= phase_bound(a, f, GAMMA, kind)).all(), f"replay {r}"
        else:
            assert diag_same_bits(got, DO.multiply(a, f, npdtype(kind))), f"replay {r}"
            assert diag_same_bits(memory_of(outs[0], strides), f)

    capture_and_replay(op, [t], states(1600, kind), verify)


# ---- 2. out of place, and two states -------------------------------------------------------------------------------------------
@gpu
@both
def test_pauli_sum_operator_with_out(kind, lay):
    a, out = state(kind, lay), state(kind, lay)
    ham = A.PauliSumOperator(a.shape, a.stride(), a.dtype, HTERMS, DEV)

    def verify(r, hosts, after, outs):
        assert same(after[0], hosts[0])                     # amps is only read
        want = oracle_sum(hosts[0], HTERMS)
        apply_check(after[1], want, hosts[0], HTERMS, kind, f"PauliSumOperator out= replay {r}")
        apply_check(outs[0], want, hosts[0], HTERMS, kind, f"PauliSumOperator out=None replay {r}")
        assert same(outs[0], after[1])

    def contents(r):                                           # out starts as garbage of another replay
        return [crand(2100 + r, SHAPE, kind), crand(2150 + r, SHAPE, kind)]

    def op(x, y):
        assert ham(x, out=y) is y
        fresh = ham(x)                                         # out=None: the result is allocated in the graph's pool
        assert fresh.stride() == x.stride()
        return fresh

    capture_and_replay(op, [a, out], contents, verify)


@gpu
@both
def test_pauli_pair_circuit(kind, lay):
    lam, phi = state(kind, lay), state(kind, lay)
    circ = A.PauliPairCircuit(phi.shape, phi.stride(), phi.dtype, STEPS, DEV)
    assert circ.n_runs >= 2

    def verify(r, hosts, after, outs):
        t, want_lam, want_phi = oracle_pair(hosts[0], hosts[1], STEPS)
        got = outs[0].view(np.complex128).reshape(-1)
        assert got.shape == t.shape and np.abs(got - t).max() <= pauli_pair_bound(kind, STEPS, hosts[0], hosts[1]), f"replay {r}"
        evolve_check(after[0], want_lam, hosts[0], STEPS, kind, f"PauliPairCircuit lam replay {r}")
        evolve_check(after[1], want_phi, hosts[1], STEPS, kind, f"PauliPairCircuit phi replay {r}")

    capture_and_replay(lambda x, y: circ(x, y, device=True), [lam, phi], states(2200, kind, 2), verify)


@gpu
@both
def test_gate_pair_circuit(kind, lay):
    lam, phi = state(kind, lay), state(kind, lay)
    gs = GATES[:12]
    circ = A.GatePairCircuit(phi.shape, phi.stride(), phi.dtype, gs, DEV, MEASURES)
    assert circ.n_runs >= 2 and circ.n_measured == 12

    def verify(r, hosts, after, outs):
        t, want_lam, want_phi = oracle_gate_pair(hosts[0], hosts[1], gs, MEASURES)
        got = outs[0].view(np.complex128).reshape(-1)
        assert got.shape == t.shape and np.all(np.abs(got - t) <= element_bounds(kind, gs, MEASURES, hosts[0], hosts[1])), f"replay {r}"
        gate_check(after[0], want_lam, hosts[0], gs, kind, f"GatePairCircuit lam replay {r}")
        gate_check(after[1], want_phi, hosts[1], gs, kind, f"GatePairCircuit phi replay {r}")

    capture_and_replay(lambda x, y: circ(x, y, device=True), [lam, phi], states(2300, kind, 2), verify)


@gpu
@both
@pytest.mark.parametrize("evolve", [True, False])
def test_diagonal_pair(evolve, kind, lay):
    lam, phi = state(kind, lay), state(kind, lay)
    strides = phi.stride()
    diag = A.DiagonalOperator(phi.shape, strides, phi.dtype, ZTERMS, DEV)
    f = DO.Plan(SHAPE, strides, ZTERMS).values()

    def verify(r, hosts, after, outs):
        l0, p0 = memory_of(hosts[0], strides), memory_of(hosts[1], strides)
        want, scale = DO.transition(l0, f, p0)
        assert abs(complex(*outs[0]) - want) <= 1e-12 * scale, f"replay {r}"
        for a, got in ((l0, memory_of(after[0], strides)), (p0, memory_of(after[1], strides))):
            if evolve:
                assert (np.abs(got.astype(np.complex128) - DO.phase(a, f, GAMMA)) <= phase_bound(a, f, GAMMA, kind)).all()
            else:
                assert same(got, a)

    capture_and_replay(lambda x, y: diag.pair_(x, y, GAMMA, device=True, evolve=evolve), [lam, phi], states(2400, kind, 2), verify)


# ---- 3. reductions with device=True --------------------------------------------------------------------------------------------
@gpu
@both
def test_overlap_norm_fidelity_block_sums(kind, lay):
    a, b = state(kind, lay), state(kind, lay)
    n = 2 ** NQ
    plan = born.born_plan(n, a.dtype)

    def op(x, y):
        bs, prefix = born.block_sums(x)
        return A.overlap(x, y, device=True), A.norm2(x, device=True), A.fidelity(x, y, device=True), bs, prefix

    def verify(r, hosts, after, outs):
        ha, hb = hosts
        na, nb = sq(ha).sum(), sq(hb).sum()
        inner = np.vdot(ha.astype(np.complex128), hb.astype(np.complex128))
        ov, n2, fid, bs, prefix = outs
        assert abs(complex(ov[0], ov[1]) - inner) <= born_tol(n) * np.sqrt(na * nb) and abs(ov[2] - na) <= born_tol(n) * na
        assert abs(ov[3] - nb) <= born_tol(n) * nb and abs(n2 - na) <= born_tol(n) * na
        want_f = abs(inner) ** 2 / (na * nb)
        assert abs(fid - want_f) <= 4 * born_tol(n) * max(np.sqrt(want_f), born_tol(n)) + 4 * born_tol(n) * want_f
        want = sq(memory_of(ha, a.stride())).reshape(plan["n_blocks"], -1).sum(axis=1)
        assert np.abs(bs - want).max() <= born_tol(2 ** plan["block_bits"]) * want.max()
        assert np.abs(prefix - np.cumsum(want)).max() <= born_tol(n) * want.sum()

    capture_and_replay(op, [a, b], states(3100, kind, 2), verify)


@gpu
@both
@pytest.mark.parametrize("form", ["stream", "generic"])
def test_marginals_and_density_matrices(form, kind, lay):
    shape = SHAPE if form == "stream" else GENERIC_SHAPE
    keep_m, keep_r = ([15, 3, 0], [0, 9, 15]) if form == "stream" else ([1, 6], [1, 6])
    t = state(kind, lay, shape)
    if form == "generic":
        assert_generic_forms(t.shape, t.stride(), kind)
    n = t.numel()

    def verify(r, hosts, after, outs):
        h = hosts[0]
        assert np.abs(outs[0] - oracle_marginal(h, keep_m)).max() <= born_tol(n) * sq(h).sum(), f"replay {r}"
        want = oracle_rdm(h, keep_r)
        diag = want.diagonal().real
        scale = np.sqrt(np.outer(diag, diag))
        assert (np.abs(outs[1].real - want.real) <= born_tol(n) * scale).all() and (np.abs(outs[1].imag - want.imag) <= born_tol(n) * scale).all()

    capture_and_replay(lambda x: (A.marginal_probabilities(x, keep_m), A.reduced_density_matrix(x, keep_r)), [t],
                       states(3200, kind, 1, shape), verify)


@gpu
@both
def test_pauli_expectation_batch_and_diagonal_moments(kind, lay):
    t = state(kind, lay)
    strides = t.stride()
    diag = A.DiagonalOperator(t.shape, strides, t.dtype, ZTERMS, DEV)
    f = DO.Plan(SHAPE, strides, ZTERMS).values()
    n = 2 ** NQ

    def op(x):
        e, var = diag.expectation(x, device=True)
        return A.pauli_expectation(x, STRINGS, device=True), A.pauli_expectation(x, STRINGS, normalize=False, device=True), \
            diag.moments(x, device=True), e, var

    def verify(r, hosts, after, outs):
        h = hosts[0]
        nrm, raw, mom, e, var = outs
        for k, p in enumerate(STRINGS):
            w, norm2 = expectation_oracle(h, p)
            assert abs(raw[k] - w) <= born_tol(n) * norm2 and abs(nrm[k] - w / norm2) <= 2 * born_tol(n), (r, p)
        want, scale = DO.moments(memory_of(h, strides), f)
        assert (np.abs(mom - want) <= 1e-12 * scale).all()
        assert abs(e - want[1] / want[0]) <= 2e-12 * scale[1] / want[0]
        assert abs(var - (want[2] / want[0] - (want[1] / want[0]) ** 2)) <= 4e-12 * scale[2] / want[0]

    capture_and_replay(op, [t], states(3300, kind), verify)


@gpu
@both
def test_krylov_dots_and_combine(kind, lay):
    vs = [state(kind, lay) for _ in range(7)]                  # five vectors, w, and z; then y = vs[0] <- a combination of vs[0], z, vs[2], vs[3]
    n = 2 ** NQ
    coeffs = np.array([0.7 - 0.2j, 0.0, 1.1j, -0.4])           # z sits behind the coefficient that is exactly 0

    def op(*x):
        dots, nw = A.krylov_dots(list(x[:5]), x[5], device=True)
        n2 = A.krylov_combine_(x[0], coeffs, [x[0], x[6], x[2], x[3]], device=True)
        return dots, nw, n2

    def contents(r):
        hosts = states(3400, kind, 7)(r)
        if r >= 1:                                             # a skipped vector is never read: 0 * NaN would poison every element
            hosts[6] = np.full(SHAPE, complex(float("nan"), float("nan")), dtype=npdtype(kind))
        return hosts

    def verify(r, hosts, after, outs):
        dots, nw, n2 = outs
        hs = [h.astype(np.complex128) for h in hosts]
        for j in range(5):
            bound = 4 * (n + 4) * 2.0 ** -53 * float(np.sum(np.abs(hs[j]) * np.abs(hs[5])))
            assert abs(complex(*dots[j]) - np.vdot(hs[j], hs[5])) <= bound, (r, j)
        assert abs(nw - sq(hosts[5]).sum()) <= born_tol(n) * sq(hosts[5]).sum()
        want, mag = combine_reference(coeffs[[0, 2, 3]], [hs[0], hs[2], hs[3]])
        for part in (np.real, np.imag):
            slack = 8 * 4 * 2.0 ** -53 * mag + (2.0 ** -24 * np.abs(part(want)) if kind == "c64" else 0.0)
            assert np.all(np.abs(part(after[0]).astype(np.float64) - part(want)) <= slack), r
        assert abs(n2 - sq(after[0]).sum()) <= born_tol(n) * sq(after[0]).sum()
        for j in range(1, 7):
            assert same(after[j], hosts[j])

    capture_and_replay(op, vs, contents, verify)


# ---- 4. choices made on the device ---------------------------------------------------------------------------------------------
def uniform_tensor():
    return torch.zeros(1, dtype=torch.float64, device=DEV)


def collapse_contents(seed0, kind, outcomes, impossible=()):
    """contents(r) = [state, uniform in the middle of the interval of outcomes[r]]; in the replays listed in `impossible` the
    amplitudes of that outcome are exactly zero."""
    def contents(r):
        h = crand(seed0 + 100 * (r + 1), SHAPE, kind)
        o = outcomes[r % len(outcomes)]
        if r in impossible:
            h[MO.kept_mask(h.shape, MDIMS, o)] = 0
            return [h, np.array([0.5])]
        q = MO.probabilities(h, MDIMS)
        u = MO.mid_uniform(q, o)
        assert measure.choose_outcome(q, u)[0] == o
        return [h, np.array([u])]
    return contents


def round_unit(kind):
    return 2.0 ** -22 if kind == "c64" else 2.0 ** -51         # the rounding terms of test_measure_gpu.DTYPES


@gpu
@both
@pytest.mark.parametrize("what", ["measure", "reset", "postselect"])
def test_collapse(what, kind, lay):
    t, u = state(kind, lay), uniform_tensor()
    outcomes = [3, 3, 3, 3] if what == "postselect" else [2, 0, 3, 1]    # replay r; the capture itself sees outcomes[-1]
    impossible = (1,) if what == "postselect" else ()
    n = 2 ** NQ

    def op(a, uu):
        qd = A.marginal_probabilities(a, MDIMS)                # (the marginal the collapse forms again: its record is checked exactly)
        if what == "postselect":
            return measure.collapse_(a, MDIMS, outcome=3), qd
        return measure.collapse_(a, MDIMS, uniform=uu, reset=(what == "reset")), qd

    def verify(r, hosts, after, outs):
        h, rec, qd = hosts[0], outs[0], outs[1].reshape(-1)
        o = outcomes[r]
        got_o, (prob, total, scale) = int(rec.view(np.int64)[0]), rec[1:].tolist()
        if r in impossible:
            assert got_o == -1 and prob == 0.0
            assert same(after[0], h)
            return
        q = MO.probabilities(h, MDIMS)
        assert got_o == o, (r, got_o, o)
        assert abs(prob - q[o] / q.sum()) <= born_tol(n) * q[o] / q.sum() and abs(total - q.sum()) <= born_tol(n) * q.sum()
        assert total == np.cumsum(qd)[-1] and prob == qd[o] / total
        want_scale = np.sqrt(total / qd[o])
        assert abs(scale - want_scale) <= 2 * np.spacing(want_scale), (scale, want_scale)
        want = (MO.reset if what == "reset" else MO.collapsed)(h, MDIMS, o, scale)
        assert same(after[0], want), f"replay {r}: not the exact collapse"

    capture_and_replay(op, [t, u], collapse_contents(4100, kind, outcomes, impossible), verify, replays=4)


@gpu
@both
@pytest.mark.parametrize("fn", ["measure_", "reset_", "postselect_"])
def test_the_device_true_wrappers(fn, kind, lay):
    t, u = state(kind, lay), uniform_tensor()
    outcomes = [1, 3, 0]
    n = 2 ** NQ

    def op(a, uu):
        if fn == "postselect_":
            return A.postselect_(a, MDIMS, 2, device=True)
        return getattr(A, fn)(a, MDIMS, uniform=uu, device=True)

    def verify(r, hosts, after, outs):
        h = hosts[0]
        q = MO.probabilities(h, MDIMS)
        o = 2 if fn == "postselect_" else outcomes[r]
        if fn != "postselect_":
            assert int(outs[0].reshape(-1)[0]) == o, (r, outs[0], o)
        assert abs(float(outs[-1].reshape(-1)[0]) - q[o] / q.sum()) <= born_tol(n) * q[o] / q.sum()
        scale = MO.scale_of(q, o)
        want = (MO.reset if fn == "reset_" else MO.collapsed)(h.astype(np.complex128), MDIMS, o, 1.0) * scale
        err = np.linalg.norm((after[0].astype(np.complex128) - want).reshape(-1))
        assert err <= (round_unit(kind) + 2 * born_tol(n)) * np.linalg.norm(want.reshape(-1)), (r, err)

    capture_and_replay(op, [t, u], collapse_contents(4200, kind, outcomes), verify)


@gpu
@both
@pytest.mark.parametrize("form", list(CHANNELS))
def test_channel_step(form, kind, lay):
    t, u = state(kind, lay), uniform_tensor()
    ch, packed, mats = CHANNELS[form]()
    dims = [0]
    step = A.ChannelOp(t.shape, t.stride(), t.dtype, ch, dims, DEV)
    assert step.form == form and step.n_tiles >= 2
    picks = [1, 0, 3, 2] if form == "FIXED" else [1, 0, 1, 0]

    def contents(r):
        h = crand(4300 + 100 * (r + 1), SHAPE, kind)
        w, _ = CO.weights(form, packed, h, dims)
        uu = MO.mid_uniform(w, picks[r])
        assert measure.choose_outcome(w, uu)[0] == picks[r] == CO.choose(w, uu)
        return [h, np.array([uu])]

    def verify(r, hosts, after, outs):
        h, rec = hosts[0], outs[0]
        w, trace = CO.weights(form, packed, h, dims)
        j, p, total, scale = CO.record(form, w, trace, float(hosts[1][0]))
        assert int(rec.view(np.int64)[0]) == j == picks[r], (r, int(rec.view(np.int64)[0]), j)
        for got, want in ((rec[1], p), (rec[2], total), (rec[3], scale)):
            assert abs(got - want) <= 1e-12 * abs(want), (r, got, want)
        cur = rec[4:].view(np.complex128).reshape(2, 2)
        assert (cur.view(np.float64) == CO.current_matrix(mats[j], rec[3]).view(np.float64)).all()
        if form == "FIXED" and j == 0:                         # an exact identity: the state is not touched
            assert same(after[0], h)
        gate = (cur, tuple(dims))
        gate_check(after[0], gate_oracle(h, [gate]), h, [gate], kind, f"ChannelOp {form} replay {r} j {j}")

    capture_and_replay(lambda a, uu: step.step(a, uniform=uu), [t, u], contents, verify, replays=4)

    def verify_call(r, hosts, after, outs):                    # op(amps, device=True): (j, p), views of the same record
        h = hosts[0]
        w, trace = CO.weights(form, packed, h, dims)
        j, p, total, scale = CO.record(form, w, trace, float(hosts[1][0]))
        assert int(outs[0].reshape(-1)[0]) == j == picks[r] and abs(float(outs[1].reshape(-1)[0]) - p) <= 1e-12 * p
        gate = (CO.current_matrix(mats[j], scale), tuple(dims))
        want = gate_oracle(h, [gate])                          # the host's scale: 1e-12 relative from the device's, as above
        unit = 2 * 2.0 ** -24 if kind == "c64" else 32 * 2.0 ** -53
        norm = np.linalg.norm(h.astype(np.complex128).reshape(-1)) * growth([gate])
        err = np.linalg.norm((after[0].astype(np.complex128) - want).reshape(-1))
        assert err <= (unit + 1e-12) * norm, (r, j, err)

    capture_and_replay(lambda a, uu: step(a, uniform=uu, device=True), [t, u], contents, verify_call, replays=4)


@gpu
@both
def test_controlled_gate_alone_and_under_a_condition_tensor(kind, lay):
    t = state(kind, lay)
    cond = torch.zeros(1, dtype=torch.int64, device=DEV)
    m, targets, controls, values = CG
    m2 = asym(1, 5)
    g1 = A.ControlledGate(t.shape, t.stride(), t.dtype, m, targets, controls, DEV, values)
    g2 = A.ControlledGate(t.shape, t.stride(), t.dtype, m2, (15,), (0, 13), DEV)
    assert all(g.c_high >= 1 and g.c_low >= 1 and g.n_tiles >= 2 for g in (g1, g2))
    flags = [6, 5, 6, 7]                                       # the int64 the condition reads: g2 acts iff it is 6; the capture sees 7

    def op(a, c):
        g1(a)
        g2(a, condition=A.when(c, equals=6))

    def contents(r):
        return [crand(4400 + 100 * (r + 1), SHAPE, kind), np.array([flags[r]], dtype=np.int64)]

    def verify(r, hosts, after, outs):
        h = hosts[0]
        want = controlled_oracle(h, m, targets, controls, values)
        applied = [(m, targets)]
        if flags[r] == 6:
            want = controlled_oracle(want, m2, (15,), (0, 13), (1, 1))
            applied.append((m2, (15,)))
        gate_check(after[0], want, h, applied, kind, f"ControlledGate replay {r} flag {flags[r]}")
        assert same(after[1], hosts[1])

    capture_and_replay(op, [t, cond], contents, verify)


# ---- 5. a whole dynamic circuit in one graph -----------------------------------------------------------------------------------
def host_branch(psi0, strides, f, u_meas, u_chan, m_cg, kraus, force=None):
    """The complex128 run of the circuit from psi0 = the state after GATES (logical array): (final state, outcome, p, which
    conditioned gate acted, j, p_j, the product of the 2-norms applied after GATES, the smallest norm on the way).  force: the
    pair of flags of a WRONG run -- which conditioned gates act whatever the outcome says -- with the same uniforms."""
    psi = psi0
    q = MO.probabilities(psi, MDIMS)
    o, total = measure.choose_outcome(q, u_meas)
    scale = math.sqrt(total / q[o])
    psi = MO.collapsed(psi, MDIMS, o, 1.0) * scale
    acted = [bool(o >= 0 and (o & 1) == e) for e in (0, 1)] if force is None else list(force)
    _, targets, controls, values = CG
    for e in (0, 1):
        if acted[e]:
            psi = controlled_oracle(psi, m_cg[e], targets, controls, values)
    w, trace = CO.weights(CO.DIAGONAL, CO.effects(kraus, CO.DIAGONAL), psi, [9])
    j, wt = measure.choose_outcome(w, u_chan)
    cur = np.asarray(kraus[j]) * math.sqrt(trace / w[j])
    psi = gate_oracle(psi, [(cur, (9,))])
    fl = logical_of(f, SHAPE, strides)
    psi = psi * np.exp(-1j * GAMMA * fl)
    g = max(1.0, scale) * max(1.0, np.linalg.norm(cur, 2))
    for e in (0, 1):
        if acted[e]:
            g *= max(1.0, np.linalg.norm(m_cg[e], 2))
    floor = min(math.sqrt(total), math.sqrt(trace), float(np.linalg.norm(psi.reshape(-1))))    # the norms the probabilities are relative to
    return psi, o, q[o] / total, acted, j, w[j] / wt, g, floor


@gpu
@both
def test_a_dynamic_circuit_in_one_graph(kind, lay):
    t, u_meas, u_chan = state(kind, lay), uniform_tensor(), uniform_tensor()
    strides = t.stride()
    n = 2 ** NQ
    kraus = CO.amplitude_damping(0.3)
    m_cg = [asym(1, 4), asym(1, 5)]
    circ = A.GateCircuit(t.shape, strides, t.dtype, GATES, DEV)
    _, targets, controls, values = CG
    cgs = [A.ControlledGate(t.shape, strides, t.dtype, m, targets, controls, DEV, values) for m in m_cg]
    assert all(g.c_high >= 1 and g.c_low >= 1 for g in cgs)
    damp = A.ChannelOp(t.shape, strides, t.dtype, A.amplitude_damping(0.3), [9], DEV)
    diag = A.DiagonalOperator(t.shape, strides, t.dtype, ZTERMS, DEV)
    f = DO.Plan(SHAPE, strides, ZTERMS).values()
    torch.cuda.synchronize()                                   # (the channel's table arrives by a non-blocking copy)

    def op(a, um, uc):
        circ(a)
        rec = measure.collapse_(a, MDIMS, uniform=um)
        cgs[0](a, condition=A.when(rec, equals=0, mask=1))
        cgs[1](a, condition=A.when(rec, equals=1, mask=1))
        crec = damp.step(a, uniform=uc)
        diag.evolve_(a, GAMMA)
        return rec, crec, diag.moments(a, device=True)

    outcomes, picks = [2, 1, 0, 3], [1, 0, 0, 1]              # one replay per measurement outcome; the capture sees (3, 1)

    def contents(r):
        h = crand(5100 + 100 * (r + 1), SHAPE, kind)
        psi = gate_oracle(h, GATES)
        q = MO.probabilities(psi, MDIMS)
        assert (q > 0).all()                                   # all four outcomes are live
        um = MO.mid_uniform(q, outcomes[r])
        psi = MO.collapsed(psi, MDIMS, outcomes[r], 1.0) * MO.scale_of(q, outcomes[r])
        psi = controlled_oracle(psi, m_cg[outcomes[r] & 1], targets, controls, values)
        w, _ = CO.weights(CO.DIAGONAL, CO.effects(kraus, CO.DIAGONAL), psi, [9])
        return [h, np.array([um]), np.array([MO.mid_uniform(w, picks[r])])]

    seen = set()

    def verify(r, hosts, after, outs):
        h, um, uc = hosts[0], float(hosts[1][0]), float(hosts[2][0])
        rec, crec, mom = outs
        psi0 = gate_oracle(h, GATES)
        want, o, p, acted, j, pj, g, floor = host_branch(psi0, strides, f, um, uc, m_cg, kraus)
        assert acted.count(True) == 1 and acted.index(True) == (o & 1) and o == outcomes[r] and j == picks[r]
        K = len(GATES) + 4
        unit = 2 * 2.0 ** -24 if kind == "c64" else 32 * 2.0 ** -53
        norm_h = np.linalg.norm(h.astype(np.complex128).reshape(-1))
        bound = (unit * K + 2 * born_tol(n)) * growth(GATES) * g * norm_h
        eps = bound / floor                                    # the bound relative to the smallest norm on the way
        assert eps < 0.01
        # the test can tell the branches apart: the other gate, both gates or neither end far outside the bound
        for wrong in ([not x for x in acted], [True, True], [False, False]):
            other = host_branch(psi0, strides, f, um, uc, m_cg, kraus, force=wrong)[0]
            gap = np.linalg.norm((other - want).reshape(-1))
            assert gap >= 100 * bound, (r, wrong, gap, bound)
        assert int(rec.view(np.int64)[0]) == o and int(crec.view(np.int64)[0]) == j, (r, rec, crec)
        assert abs(rec[1] - p) <= 5 * eps + born_tol(n) and abs(crec[1] - pj) <= 5 * eps + born_tol(n), (r, rec[1], p, crec[1], pj)
        err = np.linalg.norm((after[0].astype(np.complex128) - want).reshape(-1))
        assert err <= bound, (r, o, j, err, bound)
        m_want, m_scale = DO.moments(memory_of(after[0], strides), f)          # the moments of the state the replay left
        assert (np.abs(mom - m_want) <= 1e-12 * m_scale).all()
        m_ref, _ = DO.moments(memory_of(want, strides), f)                     # and of the host's branch: |d sum p f^k| <= (2 eps + eps^2) sum p max|f|^k
        fmax = float(np.abs(f).max())
        assert (np.abs(mom - m_ref) <= 3 * eps * m_ref[0] * np.array([1.0, fmax, fmax ** 2]) + 1e-12 * m_scale).all()
        seen.add((o, tuple(acted), j))

    capture_and_replay(op, [t, u_meas, u_chan], contents, verify, replays=4)
    assert len(seen) == 4 and {s[0] for s in seen} == {0, 1, 2, 3}


# ---- 6. default random draws ---------------------------------------------------------------------------------------------------
@gpu
@both
def test_default_draws_differ_between_replays(kind, lay):
    t = state(kind, lay)
    h = crand(6100, SHAPE, kind)
    h[1] = h[0] * 1j                                           # dim 0: q = [1/2, 1/2] exactly (the same terms in the same order)
    q = MO.probabilities(h, [0])
    assert q[0] == q[1]
    fill(t, h)
    keep = twin(t)
    measure.collapse_(twin(t), [0])                            # warm-up
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rec = measure.collapse_(t, [0], uniform=None)
    seen = []
    for r in range(64):
        t.copy_(keep)
        graph.replay()
        torch.cuda.synchronize()
        host = rec.cpu().numpy()
        o, scale = int(host.view(np.int64)[0]), float(host[3])
        assert o in (0, 1) and abs(host[1] - 0.5) <= born_tol(2 ** NQ)
        assert same(t.cpu().numpy(), MO.collapsed(h, [0], o, scale)), f"replay {r}, outcome {o}"
        seen.append(o)
    assert set(seen) == {0, 1}, f"64 replays of one captured default draw gave {sum(seen)} ones: the draw was baked into the graph"


# ---- 7. replay after other work ------------------------------------------------------------------------------------------------
@gpu
@both
def test_replay_after_larger_eager_calls_of_the_same_kernels(kind, lay):
    t, a, b = state(kind, lay), state(kind, lay), state(kind, lay)
    circ = A.GateCircuit(t.shape, t.stride(), t.dtype, GATES, DEV)
    big_shape = (2,) * 20
    big = [strided_empty(big_shape, kind, lay) for _ in range(2)]
    for j, x in enumerate(big):
        fill(x, crand(7000 + j, big_shape, kind))
    big_circ = A.GateCircuit(big_shape, big[0].stride(), big[0].dtype, [(m, tuple(d + 4 for d in dims)) for m, dims in GATES] + [(ASYM2, (0, 19))], DEV)
    big_wide = A.WideGate(big_shape, big[0].stride(), big[0].dtype, asym(5, 3), (0, 19, 7, 12, 3), DEV)

    def other_work(r):
        big_circ(big[0])
        big_wide(big[0])
        A.overlap(big[0], big[1], device=True)
        A.krylov_dots(big, big[1], device=True)
        A.marginal_probabilities(big[0], [19, 0])

    def verify_circ(r, hosts, after, outs):
        gate_check(after[0], gate_oracle(hosts[0], GATES), hosts[0], GATES, kind, f"after other work, replay {r}")

    capture_and_replay(lambda x: circ(x), [t], states(7100, kind), verify_circ, between=other_work)

    def verify_red(r, hosts, after, outs):
        inner = np.vdot(hosts[0].astype(np.complex128), hosts[1].astype(np.complex128))
        na, nb = sq(hosts[0]).sum(), sq(hosts[1]).sum()
        assert abs(complex(outs[0][0], outs[0][1]) - inner) <= born_tol(2 ** NQ) * np.sqrt(na * nb)
        assert abs(complex(*outs[1][0]) - inner) <= born_tol(2 ** NQ) * np.sqrt(na * nb)

    capture_and_replay(lambda x, y: (A.overlap(x, y, device=True), A.krylov_dots([x], y, device=True)[0]), [a, b],
                       states(7200, kind, 2), verify_red, between=other_work)
