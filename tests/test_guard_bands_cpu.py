"""What tests/test_guard_bands_gpu.py rests on, without a GPU: (1) every public callable of the state modules is run inside
guard bands, reaches the device only through one that is, or never touches it; (2) the method of tests/guard_bands.py works --
numpy oracles run as stand-in kernels through banded() on CPU arrays, clean and with five planted errors, each of which has to
be rejected; (3) the host-only assertions of every GPU case hold: the form is the one the *_info call reports and the band
covers the largest unit the plan moves."""
import numpy as np
import pytest
import torch

from artensor_amd import matrix_gates

import guard_bands as GB
import test_guard_bands_gpu as G
from graph_replay import KINDS, crand, logical_of, memory_of
from test_gates_cpu import numpy_gate
from test_graph_replay_gpu import HOST_ONLY as REPLAY_HOST_ONLY
from test_graph_replay_gpu import MODULES as REPLAY_MODULES

# ---- 1. the completeness tables ------------------------------------------------------------------------------------------------
MODULES = dict(REPLAY_MODULES, matrix_gates=matrix_gates)

# run inside guard bands by a test of test_guard_bands_gpu.py.  A class: its call with every device-side argument (device=True,
# out=, condition=) and its device=True methods.  linear_xeb is torch's mean, run on a banded tensor by a test of its own.
BANDED = {
    "gates.GateCircuit", "wide_gates.WideGate", "wide_gates.FusedCircuit", "matrix_gates.MatrixGate", "matrix_gates.BlockCircuit",
    "controlled.ControlledGate", "pauli.PauliCircuit", "pauli.PauliSumOperator", "pauli.pauli_expectation",
    "adjoint.PauliPairCircuit", "gate_adjoint.GatePairCircuit", "diagonal.DiagonalOperator", "diagonal.diagonal_values",
    "layout.BitPermutation", "channel.ChannelOp", "measure.collapse_", "measure.measure_", "measure.postselect_", "measure.reset_",
    "born.overlap", "born.norm2", "born.fidelity", "born.block_sums", "born.marginal_probabilities", "born.sample", "born.linear_xeb",
    "rdm.reduced_density_matrix", "krylov.krylov_dots", "krylov.krylov_combine_",
}

# per-call wrappers: what they do on the device is a call of the BANDED objects named (read off the wrapper's body); the rest of
# them is planning, packing, an allocation of their own or host arithmetic.  pauli_sum_expectation does not call
# pauli_expectation itself: both call pauli._raw, the one library entry artn_pauli_expect, with the same arguments.
VIA = {
    "gates.apply_gates_": "gates.GateCircuit", "gates.apply_gate_": "gates.GateCircuit", "gates.run_circuit": "gates.GateCircuit",
    "wide_gates.apply_wide_gate_": "wide_gates.WideGate", "wide_gates.apply_circuit_": "wide_gates.FusedCircuit",
    "matrix_gates.apply_matrix_gate_": "matrix_gates.MatrixGate", "matrix_gates.apply_blocks_": "matrix_gates.BlockCircuit",
    "controlled.apply_controlled_gate_": "controlled.ControlledGate", "controlled.mcx_": "controlled.ControlledGate",
    "controlled.mcz_": "controlled.ControlledGate", "controlled.mcphase_": "controlled.ControlledGate",
    "pauli.pauli_sum_apply": "pauli.PauliSumOperator", "pauli.pauli_apply": "pauli.PauliSumOperator",
    "pauli.pauli_rotate": "pauli.PauliSumOperator", "pauli.pauli_evolve_": "pauli.PauliCircuit", "pauli.pauli_rotate_": "pauli.PauliCircuit",
    "pauli.pauli_apply_": "pauli.PauliCircuit", "pauli.pauli_sum_expectation": "pauli.pauli_expectation",
    "pauli.pauli_sum_variance": "pauli.PauliSumOperator born.overlap born.norm2",
    "adjoint.pauli_evolve_pair_": "adjoint.PauliPairCircuit",
    "adjoint.adjoint_gradient": "pauli.PauliCircuit pauli.PauliSumOperator born.overlap born.norm2 adjoint.PauliPairCircuit",
    "gate_adjoint.apply_gates_pair_": "gate_adjoint.GatePairCircuit",
    "gate_adjoint.gate_adjoint_gradient": "gates.GateCircuit pauli.PauliSumOperator born.overlap born.norm2 gate_adjoint.GatePairCircuit",
    "diagonal.diagonal_evolve_": "diagonal.DiagonalOperator", "diagonal.diagonal_expectation": "diagonal.DiagonalOperator",
    "diagonal.qaoa_gradient": "diagonal.DiagonalOperator pauli.PauliCircuit adjoint.PauliPairCircuit born.overlap born.norm2",
    "layout.permute_dims_": "layout.BitPermutation", "layout.swap_dims_": "layout.BitPermutation",
    "layout.reverse_qubits_": "layout.BitPermutation", "layout.relayout_": "layout.BitPermutation",
    "channel.channel_": "channel.ChannelOp", "channel.channel_step_": "channel.ChannelOp",
    "measure.apply_channel_": "rdm.reduced_density_matrix gates.GateCircuit",
    "rdm.purity": "rdm.reduced_density_matrix", "rdm.renyi_entropy": "rdm.reduced_density_matrix",
    "rdm.entanglement_entropy": "rdm.reduced_density_matrix", "rdm.expectation": "rdm.reduced_density_matrix",
    "krylov.lanczos": "born.norm2 krylov.krylov_dots krylov.krylov_combine_",
    "krylov.lanczos_ground_state": "pauli.PauliSumOperator born.norm2 krylov.krylov_dots krylov.krylov_combine_",
    "krylov.krylov_evolve": "pauli.PauliSumOperator born.norm2 krylov.krylov_dots krylov.krylov_combine_",
}

HOST_ONLY = REPLAY_HOST_ONLY | {"matrix_gates.matrix_gate_info", "matrix_gates.fuse_gates_wide"}


def test_every_public_callable_is_in_exactly_one_table():
    assert len(MODULES) == 14
    public = {f"{name}.{entry}" for name, mod in MODULES.items() for entry in mod.__all__}
    tables = [BANDED, set(VIA), HOST_ONLY]
    for i, x in enumerate(tables):
        for y in tables[i + 1:]:
            assert not x & y, sorted(x & y)
    listed = BANDED | set(VIA) | HOST_ONLY
    assert listed - public == set(), f"listed, but not public: {sorted(listed - public)}"
    assert public - listed == set(), f"decide whether these run inside guard bands, go through one that does, or stay on the host: {sorted(public - listed)}"
    for name, through in VIA.items():
        assert through and set(through.split()) <= BANDED, (name, through)
    for full in listed:
        mod, entry = full.split(".")
        assert callable(getattr(MODULES[mod], entry)), full


def test_every_banded_entry_has_cases_and_every_case_its_host_only_assertions():
    """(3) Building a case runs its assertions: the form the info call reports, band >= the plan's largest unit >= 1, band >= 4096,
    at most 2^14 elements per state."""
    seen, count = set(), 0
    for names, cases in G.all_cases():
        some = 0
        for case in cases:
            assert case.band >= max(case.unit, GB.MIN_BAND) and case.band % GB.MIN_BAND == 0, case.label
            assert all(h.shape == case.shape and h.dtype == KINDS[case.kind][0] for h in case.hosts), case.label
            some += 1
        assert some >= 1, names
        count += some
        seen |= set(names.split())
    assert all(callable(getattr(G, test)) for test in G.OTHER_TESTS.values())
    seen |= set(G.OTHER_TESTS)
    assert seen == BANDED, (sorted(BANDED - seen), sorted(seen - BANDED))
    print(f"{count} cases, each at three offsets")


# ---- 2. the method: stand-in kernels on CPU arrays, clean and with planted errors ----------------------------------------------
GATE = np.array([[0.6, 0.8j], [0.8j, 0.6]])
ERRORS = ["store one past the end", "store one in front of the start", "band element in a reduction", "write between the pair",
          "addressed from the storage base"]


def standin_gate(store, view, lay, j, dim, error=None):
    """One gate on state j, in place, the way a kernel sees it: a base address and flat indices.  error: what a wrong one does."""
    start, n = lay["starts"][j], lay["sizes"][j]
    base = 0 if error == "addressed from the storage base" else start
    flat = store[base:base + n]                                # (numpy: a view of the store)
    strides = tuple(s // store.itemsize for s in view.strides)
    new = numpy_gate(logical_of(flat.copy(), view.shape, strides), GATE, [dim]).astype(store.dtype)
    flat[...] = memory_of(new, strides)
    if error == "store one past the end":
        store[start + n] = flat[-1]
    if error == "store one in front of the start":
        store[start - 1] = flat[0]


def standin_overlap(store, lay, error=None):
    """<state 0|state 1> in float64, as a reduction over flat indices; a wrong one reads one element too many."""
    (s0, s1), n = lay["starts"], lay["sizes"][0]
    extra = 1 if error == "band element in a reduction" else 0
    return np.vdot(store[s0:s0 + n + extra].astype(np.complex128), store[s1:s1 + n + extra].astype(np.complex128))


def check_pair(kind, nq, offset, error):
    """The assertions of a GPU case, (a) to (d), on a two-state call: a gate on state 0, then the overlap of the two."""
    npdt = KINDS[kind][0]
    shape, strides = G.layout_of((2,) * nq, kind, "permuted")
    hosts = [crand(70 + j, shape, kind) for j in range(2)]
    store, views, lay = GB.banded([memory_of(h, strides) for h in hosts], shape, strides, npdt, offset, GB.MIN_BAND, "numpy")
    dim = G.dim_at(strides, nq - 1)
    standin_gate(store, views[0], lay, 0, dim, error)
    if error == "write between the pair":
        store[(lay["starts"][0] + lay["sizes"][0] + lay["starts"][1]) // 2] = 1.0
    inner = standin_overlap(store, lay, error)
    GB.assert_bands_intact(store, lay, f"{error}")                                            # (a)
    after = [logical_of(m, shape, strides) for m in GB.states_of(store, lay)]
    want = numpy_gate(hosts[0].astype(np.complex128), GATE, [dim])
    unit = 2.0 ** -23 if kind == "c64" else 2.0 ** -52
    assert np.abs(after[0] - want).max() <= 4 * unit * np.abs(want).max(), "the state differs from the reference"    # (b)
    ref = np.vdot(after[0].astype(np.complex128), hosts[1].astype(np.complex128))
    assert abs(inner - ref) <= 4 * hosts[0].size * 2.0 ** -53 * np.linalg.norm(after[0]) * np.linalg.norm(hosts[1]), \
        "the overlap differs from the reference"
    twin = numpy_gate(hosts[0], GATE, [dim]).astype(npdt)                                     # (c): the same call at offset 0
    assert GB.same_bits(after[0], twin), "the state differs from the run at offset 0"
    assert GB.same_bits(after[1], hosts[1]), "the state that is only read changed"            # (d)


# the check that has to catch each planted error, by its message.  A kernel that addresses from the storage base computes on the
# sentinels of the front band: where the arithmetic keeps the payload the band compares as intact (the blind spot named in
# guard_bands.py), and the reference sees that state 0 was never updated.
CAUGHT_BY = {
    "store one past the end": r"guard elements changed.* 1 element\(s\) behind state 0",
    "store one in front of the start": r"guard elements changed.* 1 element\(s\) in front of state 0",
    "band element in a reduction": r"the overlap differs from the reference",
    "write between the pair": r"1 guard elements changed.*behind state 0|1 guard elements changed.*in front of state 1",
    "addressed from the storage base": r"guard elements changed.*in front of state 0|the state differs from the reference",
}


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("error", [None] + ERRORS)
def test_the_method_passes_a_clean_kernel_and_rejects_planted_errors(error, kind):
    for nq in (3, 10):
        for offset in GB.offsets_of(KINDS[kind][0]):
            if error is None:
                check_pair(kind, nq, offset, None)
            else:
                with pytest.raises(AssertionError, match=CAUGHT_BY[error]):
                    check_pair(kind, nq, offset, error)


def test_a_changed_band_is_named_by_its_distance_from_the_nearest_state_edge():
    mems = [np.arange(5, dtype=np.complex64), np.arange(7, dtype=np.complex64)]
    for device in ("numpy", "cpu"):
        store, views, lay = GB.banded(mems, [(5,), (7,)], [(1,), (1,)], np.complex64, 2, 4096, device)
        GB.assert_bands_intact(store, lay)
        assert lay["starts"][0] == 4096 + 2 and (lay["starts"][1] - lay["starts"][0]) % 16 == 0 and lay["starts"][1] - lay["starts"][0] - 5 >= 4096
        assert [tuple(v.shape) for v in views] == [(5,), (7,)]
        assert all(GB.same_bits(a, m) for a, m in zip(GB.states_of(store, lay), mems))
        store[lay["starts"][1] + 7 + 2] = 0                    # the third element behind state 1
        with pytest.raises(AssertionError, match=r"3 element\(s\) behind state 1"):
            GB.assert_bands_intact(store, lay)
        store[lay["starts"][0] - 1] = 0                        # the offset gap
        with pytest.raises(AssertionError, match=r"2 guard elements changed.* 1 element\(s\) in front of state 0"):
            GB.assert_bands_intact(store, lay)


def test_the_sentinel_is_a_quiet_nan_with_a_payload_and_survives_a_copy():
    for dtype, real in ((np.complex64, np.float32), (np.complex128, np.float64), (np.float64, np.float64)):
        store, _, lay = GB.banded([np.zeros(3, dtype=dtype)], (3,), (1,), dtype, 1, 4096, "cpu")
        band = store[:4096]
        assert bool(torch.isnan(torch.view_as_real(band) if band.is_complex() else band).all())
        word = GB.SENTINEL[np.dtype(real).itemsize]
        assert np.isnan(np.array([word]).view(real)[0]) and int(word) & 0xFFFF == 0xA5A5
        GB.assert_bands_intact(store.clone(), lay)
        poisoned = store[4096:4096 + 2].sum()                  # a load from the gap that enters arithmetic
        assert bool(torch.isnan(poisoned.real if poisoned.is_complex() else poisoned))
    assert GB.offsets_of(np.complex64) == [0, 2, 10] and GB.offsets_of(np.complex128) == [0, 1, 5] and GB.offsets_of(np.float64) == [0, 2, 10]
    assert GB.band_for(1) == 4096 and GB.band_for(4097, 5) == 8192 and GB.band_for(1 << 14) == 1 << 14


def test_the_blind_spots_are_what_the_docstring_says():
    """One fixed pattern: a move between two band elements, or a store of a value loaded from a band, writes the same bits back
    and is not seen; a store of anything else is."""
    store, _, lay = GB.banded([np.arange(8, dtype=np.complex128)], (8,), (1,), np.complex128, 1, 4096, "numpy")
    end = lay["starts"][0] + 8
    store[end], store[end + 1] = store[end + 1], store[end]    # a swap past the end
    store[0] = store[lay["starts"][0] - 1]                     # a copy of the offset gap into the front band
    GB.assert_bands_intact(store, lay)
    store[end] = store[end - 1]                                # a state element past the end
    with pytest.raises(AssertionError, match=r"1 element\(s\) behind state 0"):
        GB.assert_bands_intact(store, lay)
