"""The call-time contract the eleven prebuilt state objects share, on the device: a tensor that is not the one the object was
built for is refused ON THE HOST, before any launch, with the texts and in the order every class has had -- the checks of the
tensor itself (a GPU tensor, complex, dense, 16-byte aligned), then the layout ("built for shape ..."), then the device.  One
valid call per class; the two-state calls check lam, then phi, then their overlap; the identity BitPermutation holds no table
and launches nothing.  complex64, (2,) * 12; every object is built once."""
import functools
import re

import pytest
import torch

from test_state_prebuilt_cpu import CLASSES, SHAPE, STRIDES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_ELEMS = 2 ** 12


def good():
    a = torch.zeros(SHAPE, dtype=torch.complex64, device=DEV)
    a.view(-1)[0] = 0.6
    a.view(-1)[N_ELEMS - 1] = 0.8j
    return a


# the call under test: (class, the qualified name its messages carry, call(object, x), x is returned)
CALLS = {
    "PauliSumOperator": ("PauliSumOperator", "pauli.PauliSumOperator", lambda o, x: o(x), False),
    "PauliCircuit": ("PauliCircuit", "pauli.PauliCircuit", lambda o, x: o(x), True),
    "PauliPairCircuit": ("PauliPairCircuit", "adjoint.PauliPairCircuit", lambda o, x: o(x, good()), False),
    "GateCircuit": ("GateCircuit", "gates.GateCircuit", lambda o, x: o(x), True),
    "GatePairCircuit": ("GatePairCircuit", "gate_adjoint.GatePairCircuit", lambda o, x: o(x, good()), False),
    "WideGate": ("WideGate", "wide_gates.WideGate", lambda o, x: o(x), True),
    "FusedCircuit": ("FusedCircuit", "wide_gates.FusedCircuit", lambda o, x: o(x), True),
    "ControlledGate": ("ControlledGate", "controlled.ControlledGate", lambda o, x: o(x), True),
    "ChannelOp": ("ChannelOp", "channel.ChannelOp", lambda o, x: o(x, 0.5), False),
    "ChannelOp.step": ("ChannelOp", "channel.ChannelOp", lambda o, x: o.step(x, 0.5), False),
    "DiagonalOperator.evolve_": ("DiagonalOperator", "diagonal.DiagonalOperator.evolve_", lambda o, x: o.evolve_(x, 0.1), True),
    "DiagonalOperator.multiply_": ("DiagonalOperator", "diagonal.DiagonalOperator.multiply_", lambda o, x: o.multiply_(x), True),
    "DiagonalOperator.moments": ("DiagonalOperator", "diagonal.DiagonalOperator.moments", lambda o, x: o.moments(x), False),
    "DiagonalOperator.pair_": ("DiagonalOperator", "diagonal.DiagonalOperator.pair_", lambda o, x: o.pair_(x, good(), 0.1), False),
    "BitPermutation": ("BitPermutation", "layout.BitPermutation", lambda o, x: o(x), True),
}
# the two-state calls, as call(object, lam, phi)
PAIRS = {
    "PauliPairCircuit": ("PauliPairCircuit", "adjoint.PauliPairCircuit", lambda o, lam, phi: o(lam, phi)),
    "GatePairCircuit": ("GatePairCircuit", "gate_adjoint.GatePairCircuit", lambda o, lam, phi: o(lam, phi)),
    "DiagonalOperator.pair_": ("DiagonalOperator", "diagonal.DiagonalOperator.pair_", lambda o, lam, phi: o.pair_(lam, phi, 0.1)),
}


@functools.lru_cache(maxsize=None)
def built(cls):
    return CLASSES[cls][2](SHAPE, STRIDES, torch.complex64, DEV)


def raises(exc, text):
    return pytest.raises(exc, match="^" + re.escape(text) + "$")


def built_for(what, x):
    return (f"{what}: built for shape {SHAPE}, strides {STRIDES}, torch.complex64; got {tuple(x.shape)}, {tuple(x.stride())}, "
            f"{x.dtype}")


def aligned(what):
    return (f"{what}: the tensor's memory must start on a 16-byte boundary (this view starts at an odd element of its storage) -- "
            "pass amps.contiguous().clone()")


def not_dense(x):
    return (f"the tensor is not dense (shape {tuple(x.shape)}, strides {tuple(x.stride())}): its strides are not a permutation of a "
            "contiguous layout -- pass amps.contiguous()")


def cpu_tensor(what):
    return f"{what}: artensor_amd executes on MI355X only (got a cpu tensor); there is no CPU fallback -- move the tensors to a 'cuda' device"


def odd_view(shape):
    """A contiguous view of `shape` that starts 8 bytes into its storage."""
    n = 1
    for e in shape:
        n *= e
    x = torch.zeros(n + 1, dtype=torch.complex64, device=DEV)[1:].view(shape)
    assert x.data_ptr() % 16 == 8
    return x


@pytest.mark.parametrize("name", sorted(CALLS))
def test_a_tensor_the_object_was_not_built_for_is_refused_on_the_host(name):
    cls, what, call, _ = CALLS[name]
    obj = built(cls)
    other_shape = torch.zeros((2,) * 11, dtype=torch.complex64, device=DEV)
    permuted = good().permute([1, 0] + list(range(2, 12)))
    assert tuple(permuted.shape) == SHAPE and tuple(permuted.stride()) != STRIDES
    double = torch.zeros(SHAPE, dtype=torch.complex128, device=DEV)
    for x in (other_shape, permuted, double):
        with raises(ValueError, built_for(what, x)):
            call(obj, x)
    assert f"strides {STRIDES}" in built_for(what, permuted) and f", {tuple(permuted.stride())}, " in built_for(what, permuted)
    with raises(ValueError, aligned(what)):
        call(obj, odd_view(SHAPE))
    sliced = torch.zeros(SHAPE[:-1] + (4,), dtype=torch.complex64, device=DEV)[..., ::2]
    assert tuple(sliced.shape) == SHAPE
    with raises(ValueError, not_dense(sliced)):
        call(obj, sliced)
    with raises(RuntimeError, cpu_tensor(what)):
        call(obj, torch.zeros(SHAPE, dtype=torch.complex64))
    with raises(TypeError, f"{what}: complex64 or complex128 amplitudes expected, got torch.float32"):
        call(obj, torch.zeros(SHAPE, dtype=torch.float32, device=DEV))
    # two faults at once: the checks of the tensor itself come before the layout
    with raises(RuntimeError, cpu_tensor(what)):
        call(obj, torch.zeros((2,) * 11, dtype=torch.complex64))
    with raises(ValueError, aligned(what)):
        call(obj, odd_view((2,) * 11))


@pytest.mark.parametrize("name", sorted(CALLS))
def test_one_valid_call(name):
    cls, _, call, returns_x = CALLS[name]
    x = good()
    ptr = x.data_ptr()
    got = call(built(cls), x)
    torch.cuda.synchronize()
    if returns_x:
        assert got is x
    assert x.data_ptr() == ptr and tuple(x.stride()) == STRIDES and bool(torch.isfinite(torch.view_as_real(x)).all())
    if name == "PauliSumOperator":
        assert tuple(got.shape) == SHAPE and tuple(got.stride()) == STRIDES and got.data_ptr() != ptr
    if name == "ChannelOp":
        assert got[0] in (0, 1) and 0.0 < got[1] <= 1.0
    if name == "ChannelOp.step":
        assert got.dtype == torch.float64 and got.is_cuda and got.numel() == 4 + 2 * 4


@pytest.mark.parametrize("name", sorted(PAIRS))
def test_two_states_lam_then_phi_then_the_overlap(name):
    cls, what, call = PAIRS[name]
    obj = built(cls)
    bad = torch.zeros((2,) * 11, dtype=torch.complex64, device=DEV)
    with raises(ValueError, built_for(what, bad)):              # a good lam: the error is the one of phi
        call(obj, good(), bad)
    with raises(ValueError, aligned(what)):                     # lam is checked to the end before phi is looked at
        call(obj, odd_view(SHAPE), torch.zeros(SHAPE, dtype=torch.complex64))
    with raises(ValueError, built_for(what, bad)):
        call(obj, bad, torch.zeros(SHAPE, dtype=torch.complex64))
    x = good()
    with raises(ValueError, f"{what}: lam overlaps phi"):
        call(obj, x, x)
    with raises(ValueError, f"{what}: lam overlaps phi"):
        call(obj, x, x.view(SHAPE))
    lam, phi = good(), good()
    call(obj, lam, phi)
    torch.cuda.synchronize()


def test_out_of_a_pauli_sum_may_not_overlap_amps():
    op, x = built("PauliSumOperator"), good()
    with raises(ValueError, "pauli.PauliSumOperator: out overlaps amps (there is no in-place form)"):
        op(x, out=x)
    out = torch.empty_like(x)
    assert op(x, out=out) is out
    torch.cuda.synchronize()


def test_the_table_device_is_read_at_call_time():
    """A table replaced by a CPU copy stands in for an object built for a second device."""
    for name in ("PauliCircuit", "GateCircuit", "WideGate", "ControlledGate", "DiagonalOperator.evolve_", "BitPermutation"):
        cls, what, call, _ = CALLS[name]
        obj = CLASSES[cls][2](SHAPE, STRIDES, torch.complex64, DEV)
        obj._table = obj._table.cpu()
        with raises(ValueError, f"{what}: built for cpu, got a tensor on {DEV}"):
            call(obj, good())
    fused = CLASSES["FusedCircuit"][2](SHAPE, STRIDES, torch.complex64, DEV)   # no table of its own: its first part's
    fused.parts[0]._table = fused.parts[0]._table.cpu()
    with raises(ValueError, f"wide_gates.FusedCircuit: built for cpu, got a tensor on {DEV}"):
        fused(good())


def test_channel_step_looks_at_uniform_before_amps():
    op = built("ChannelOp")
    with raises(ValueError, "channel.ChannelOp: uniform must lie in [0, 1), got 2.0"):
        op.step(torch.zeros((2,) * 11, dtype=torch.complex64), uniform=2.0)


def test_the_identity_permutation_holds_no_table_and_launches_nothing():
    from artensor_amd import layout
    for dev in (DEV, None):
        ident = layout.BitPermutation(SHAPE, STRIDES, torch.complex64, device=dev, perm=list(range(12)))
        assert ident._table is None and ident.passes == 0
        x = good()
        before = x.clone()
        assert ident(x) is x
        torch.cuda.synchronize()
        assert torch.equal(x, before)
    with raises(ValueError, built_for("layout.BitPermutation", before.view(-1))):   # still checked against its layout
        ident(before.view(-1))
