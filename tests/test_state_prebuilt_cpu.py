"""The host-side contract the eleven prebuilt state objects share (PauliSumOperator, PauliCircuit, PauliPairCircuit, GateCircuit,
GatePairCircuit, WideGate, FusedCircuit, ControlledGate, ChannelOp, DiagonalOperator, BitPermutation): the constructor's dtype
TypeError and device RuntimeError with their full texts and their order, the dtype TypeError of every *_info function, the
require_gpu RuntimeError of every one-shot function, the argument errors that come before it, and the helpers the state modules
share being ONE object under every name they are read by.  No GPU needed."""
import re

import numpy as np
import pytest
import torch

from artensor_amd import (adjoint, born, channel, controlled, diagonal, gate_adjoint, gates, krylov, layout, measure, pauli, rdm,
                          wide_gates)

SHAPE = (2,) * 12
STRIDES = tuple(2 ** (11 - k) for k in range(12))
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
STEPS = [(0.3, {0: "X"})]
TERMS = [(1.0, {0: "Z"})]
GATES = [(X, (0,))]
WIDE = (np.eye(8), (0, 1, 2))

# name: (class, its module's name, build(shape, strides, dtype, device))
CLASSES = {
    "PauliSumOperator": (pauli.PauliSumOperator, "pauli", lambda s, st, dt, dev: pauli.PauliSumOperator(s, st, dt, TERMS, dev)),
    "PauliCircuit": (pauli.PauliCircuit, "pauli", lambda s, st, dt, dev: pauli.PauliCircuit(s, st, dt, STEPS, dev)),
    "PauliPairCircuit": (adjoint.PauliPairCircuit, "adjoint", lambda s, st, dt, dev: adjoint.PauliPairCircuit(s, st, dt, STEPS, dev)),
    "GateCircuit": (gates.GateCircuit, "gates", lambda s, st, dt, dev: gates.GateCircuit(s, st, dt, GATES, dev)),
    "GatePairCircuit": (gate_adjoint.GatePairCircuit, "gate_adjoint",
                        lambda s, st, dt, dev: gate_adjoint.GatePairCircuit(s, st, dt, GATES, dev, [X])),
    "WideGate": (wide_gates.WideGate, "wide_gates", lambda s, st, dt, dev: wide_gates.WideGate(s, st, dt, WIDE[0], WIDE[1], dev)),
    "FusedCircuit": (wide_gates.FusedCircuit, "wide_gates", lambda s, st, dt, dev: wide_gates.FusedCircuit(s, st, dt, GATES + [WIDE], dev)),
    "ControlledGate": (controlled.ControlledGate, "controlled",
                       lambda s, st, dt, dev: controlled.ControlledGate(s, st, dt, X, (0,), (1, 11), dev)),
    "ChannelOp": (channel.ChannelOp, "channel", lambda s, st, dt, dev: channel.ChannelOp(s, st, dt, channel.bit_flip(0.25), (0,), dev)),
    "DiagonalOperator": (diagonal.DiagonalOperator, "diagonal", lambda s, st, dt, dev: diagonal.DiagonalOperator(s, st, dt, TERMS, dev)),
    "BitPermutation": (layout.BitPermutation, "layout",
                       lambda s, st, dt, dev: layout.BitPermutation(s, st, dt, device=dev, perm=[1, 0] + list(range(2, len(s))))),
}


def raises(exc, text):
    return pytest.raises(exc, match="^" + re.escape(text) + "$")


@pytest.mark.parametrize("name", sorted(CLASSES))
def test_constructor_refuses_dtype_then_device(name):
    cls, _, build = CLASSES[name]
    assert cls.__name__ == name
    dtype_text = f"{name}: complex64 or complex128 expected, got torch.float32"
    device_text = f"{name}: artensor_amd executes on MI355X only (got device cpu); there is no CPU fallback"
    with raises(TypeError, dtype_text):
        build(SHAPE, STRIDES, torch.float32, "cuda")
    with raises(RuntimeError, device_text):
        build(SHAPE, STRIDES, torch.complex64, "cpu")
    with raises(RuntimeError, device_text):
        build(SHAPE, STRIDES, torch.complex128, torch.device("cpu"))
    with raises(TypeError, dtype_text):                        # both faults: the dtype is looked at first
        build(SHAPE, STRIDES, torch.float32, "cpu")


def test_bit_permutation_asks_for_an_argument_after_the_device():
    with raises(ValueError, "BitPermutation: give one of dst_bit, perm and order"):
        layout.BitPermutation(SHAPE, STRIDES, torch.complex64, device="cuda")
    with raises(RuntimeError, "BitPermutation: artensor_amd executes on MI355X only (got device cpu); there is no CPU fallback"):
        layout.BitPermutation(SHAPE, STRIDES, torch.complex64, device="cpu")
    assert layout.BitPermutation(SHAPE, STRIDES, torch.complex64, perm=list(range(12))).device == torch.device("cuda")


INFOS = {
    "pauli_info": lambda dt: pauli.pauli_info(SHAPE, STRIDES, {0: "X"}, dt),
    "pauli_apply_info": lambda dt: pauli.pauli_apply_info(SHAPE, STRIDES, TERMS, dt),
    "pauli_evolve_info": lambda dt: pauli.pauli_evolve_info(SHAPE, STRIDES, STEPS, dt),
    "pauli_adjoint_info": lambda dt: adjoint.pauli_adjoint_info(SHAPE, STRIDES, STEPS, dt),
    "gate_circuit_info": lambda dt: gates.gate_circuit_info(SHAPE, STRIDES, GATES, dt),
    "gate_adjoint_info": lambda dt: gate_adjoint.gate_adjoint_info(SHAPE, STRIDES, GATES, dt),
    "wide_gate_info": lambda dt: wide_gates.wide_gate_info(SHAPE, STRIDES, WIDE[0], WIDE[1], dt),
    "controlled_gate_info": lambda dt: controlled.controlled_gate_info(SHAPE, STRIDES, X, (0,), (1,), None, dt),
    "channel_info": lambda dt: channel.channel_info(SHAPE, STRIDES, channel.bit_flip(0.25), (0,), dt),
    "diagonal_info": lambda dt: diagonal.diagonal_info(SHAPE, STRIDES, TERMS, dt),
    "bit_permutation_info": lambda dt: layout.bit_permutation_info(SHAPE, STRIDES, dt),
    "measure_info": lambda dt: measure.measure_info(SHAPE, STRIDES, (0,), dt),
    "krylov_info": lambda dt: krylov.krylov_info(SHAPE, STRIDES, 4, dt),
    "rdm_info": lambda dt: rdm.rdm_info(SHAPE, STRIDES, (0,), dt),
    "run_circuit": lambda dt: gates.run_circuit(GATES, 12, dt),
}


@pytest.mark.parametrize("name", sorted(INFOS))
def test_info_functions_refuse_a_dtype_that_is_not_complex(name):
    for dtype in (torch.float32, torch.float64, torch.int64):
        with raises(TypeError, f"{name}: complex64 or complex128 expected, got {dtype}"):
            INFOS[name](dtype)
    if name != "run_circuit":
        assert isinstance(INFOS[name](torch.complex128), dict)


def cpu_state():
    return torch.zeros(SHAPE, dtype=torch.complex64)


ONE_SHOTS = {
    "pauli.pauli_sum_apply": lambda a: pauli.pauli_sum_apply(a, TERMS),
    "pauli.pauli_apply": lambda a: pauli.pauli_apply(a, {0: "X"}),
    "pauli.pauli_rotate": lambda a: pauli.pauli_rotate(a, {0: "X"}, 0.3),
    "pauli.pauli_evolve_": lambda a: pauli.pauli_evolve_(a, STEPS),
    "pauli.pauli_rotate_": lambda a: pauli.pauli_rotate_(a, {0: "X"}, 0.3),
    "pauli.pauli_apply_": lambda a: pauli.pauli_apply_(a, {0: "X"}),
    "adjoint.pauli_evolve_pair_": lambda a: adjoint.pauli_evolve_pair_(cpu_state(), a, STEPS),
    "gates.apply_gates_": lambda a: gates.apply_gates_(a, GATES),
    "gates.apply_gate_": lambda a: gates.apply_gate_(a, X, (0,)),
    "gate_adjoint.apply_gates_pair_": lambda a: gate_adjoint.apply_gates_pair_(cpu_state(), a, GATES),
    "wide_gates.apply_wide_gate_": lambda a: wide_gates.apply_wide_gate_(a, WIDE[0], WIDE[1]),
    "wide_gates.apply_circuit_": lambda a: wide_gates.apply_circuit_(a, GATES + [WIDE]),
    "controlled.apply_controlled_gate_": lambda a: controlled.apply_controlled_gate_(a, X, (0,), (1,)),
    "channel.channel_step_": lambda a: channel.channel_step_(a, channel.bit_flip(0.25), (0,)),
    "channel.channel_": lambda a: channel.channel_(a, channel.bit_flip(0.25), (0,)),
    "diagonal.diagonal_evolve_": lambda a: diagonal.diagonal_evolve_(a, TERMS, 0.1),
    "diagonal.diagonal_expectation": lambda a: diagonal.diagonal_expectation(a, TERMS),
    "layout.permute_dims_": lambda a: layout.permute_dims_(a, [1, 0] + list(range(2, 12))),
    "layout.relayout_": lambda a: layout.relayout_(a),
    "measure.collapse_": lambda a: measure.collapse_(a, (0,)),
}


@pytest.mark.parametrize("name", sorted(ONE_SHOTS))
def test_one_shot_functions_refuse_a_cpu_tensor(name):
    what = "channel.channel_step_" if name == "channel.channel_" else name       # channel_ is channel_step_ and a read of its record
    with raises(RuntimeError, f"{what}: artensor_amd executes on MI355X only (got a cpu tensor); there is no CPU fallback -- move the "
                              "tensors to a 'cuda' device"):
        ONE_SHOTS[name](cpu_state())
    with raises(RuntimeError, f"{what}: artensor_amd executes on MI355X only (got list); there is no CPU fallback -- move the "
                              "tensors to a 'cuda' device"):
        ONE_SHOTS[name]([0.0])


def test_argument_errors_come_before_the_device():
    a = cpu_state()
    with raises(ValueError, "controlled.apply_controlled_gate_: dims [0] are listed as targets and as controls"):
        controlled.apply_controlled_gate_(a, X, (0,), (0,))
    with raises(TypeError, "channel.channel_step_: a Channel expected, got str"):
        channel.channel_step_(a, "bit_flip", (0,))
    with raises(ValueError, "channel.channel_step_: uniform must lie in [0, 1), got 2.0"):
        channel.channel_step_(a, channel.bit_flip(0.25), (0,), uniform=2.0)


MODULES = {"adjoint": adjoint, "born": born, "channel": channel, "controlled": controlled, "diagonal": diagonal,
           "gate_adjoint": gate_adjoint, "gates": gates, "krylov": krylov, "layout": layout, "measure": measure, "pauli": pauli,
           "rdm": rdm, "wide_gates": wide_gates}
# helper: the modules it is read from by name (the first one is where it was first written)
SHARED = {"_DTYPES": ["born"], "_dense_layout": ["born"], "_checked": ["born"], "_desc": ["pauli"], "_ptr": ["pauli", "controlled"],
          "_max_rank": ["pauli"], "_dims": ["wide_gates"], "_checked_uniform": ["measure"], "_device_uniform": ["measure"]}


@pytest.mark.parametrize("helper", sorted(SHARED))
def test_shared_helpers_are_one_object(helper):
    first = getattr(MODULES[SHARED[helper][0]], helper)
    for name in SHARED[helper]:
        assert getattr(MODULES[name], helper) is first, name
    holders = [name for name, mod in MODULES.items() if hasattr(mod, helper)]
    if helper == "_dims":
        holders.remove("measure")                              # measure._dims is another function: 1..10 distinct dims of extent 2
        assert measure._dims is not first
    assert len(holders) > 1, "nothing shares it"
    for name in holders:
        assert getattr(MODULES[name], helper) is first, name


def test_the_names_tests_and_tools_read_stay_where_they_are():
    assert callable(born._marginal_desc) and callable(born._checked_uniforms)
    for name in ("_pack", "_evolve_pack", "_split_terms", "_split_steps", "_evolve_query", "_raw"):
        assert callable(getattr(pauli, name)), name
    for mod in (channel, diagonal):
        assert callable(mod._pack) and callable(mod._split)
    assert callable(wide_gates._wgate_pack)
