"""In-place gate circuits on the device (artensor_amd/gates.py: apply_gates_, apply_gate_, GateCircuit, run_circuit;
artn_gates_apply) against a reference that shares nothing with the memory-bit arithmetic of the kernels: np.tensordot of the
gate's [2]*2k tensor with the complex128 copy of the LOGICAL array over the gate's dims, np.moveaxis back.

Tolerance (derived, not measured).  Every output component of a gate is formed in float64 and rounded ONCE to the dtype: a relative
error of at most u = 2^-24 (complex64) or 2^-53 (complex128) per component, so ||error of gate k||_2 <= u ||state after gate k||_2.
Later gates amplify an earlier error by at most their 2-norms, the state grows by at most g_k = max(1, ||U_k||_2) per gate, and
the error norms add linearly over the K gates.  With G = prod g_k and a factor 2 on top:
    complex64:   ||y - ref||_2 <= 2 K 2^-24 ||a||_2 G
The float64 evaluation of a four-term complex sum (16 products, 14 additions behind them) adds at most about 20 u ||U||_2 ||x||_2
in complex128, where it is not hidden behind the rounding to the dtype:
    complex128:  ||y - ref||_2 <= 32 K 2^-53 ||a||_2 G
Signed permutation matrices and the identity are exact and are compared bit for bit, as is everything that only changes where the
host cuts the circuit into runs."""
import functools
import os

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd.fixtures import load_case
from test_gates_cpu import n12_gates, numpy_gate, random_unitary
from test_gpu_parity import amp_rel
from test_pauli_apply_gpu import DEV, GOLDEN, crand, gpu
from test_pauli_evolve_gpu import bits_of

pytestmark = pytest.mark.gpu

X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
Z = np.diag([1, -1]).astype(np.complex128)
S = np.diag([1, 1j]).astype(np.complex128)
CNOT = np.eye(4)[[0, 1, 3, 2]].astype(np.complex128)                     # the first listed dim is the control
SWAP = np.eye(4)[[0, 2, 1, 3]].astype(np.complex128)
CZ = np.diag([1, 1, 1, -1]).astype(np.complex128)
ISWAP = np.array([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
ASYM1 = np.array([[0.3 + 0.1j, -1.2j], [0.7, 0.2 - 0.5j]])                # asymmetric: a transposed index is an O(1) error
ASYM2 = (np.arange(16).reshape(4, 4) * 0.11 - 0.6 + 1j * np.array([[0.3, -0.1, 0.7, 0.2], [0.5, 0.9, -0.4, 0.1],
                                                                    [-0.8, 0.6, 0.25, -0.35], [0.15, -0.45, 0.55, 0.05]]))


def growth(gates):
    return float(np.prod([max(1.0, np.linalg.norm(np.asarray(m, dtype=np.complex128).reshape(2 ** len(d), -1), 2)) for m, d in gates]))


def check(got, want, a, gates, kind, label=""):
    """The 2-norm bound of the module docstring; prints the measured error next to it."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    K = len(gates)
    unit = 2 * 2.0 ** -24 if kind == "c64" else 32 * 2.0 ** -53
    bound = unit * K * np.linalg.norm(np.asarray(a).astype(np.complex128).reshape(-1)) * growth(gates)
    err = np.linalg.norm((got.astype(np.complex128) - want).reshape(-1))
    print(f"{label}: K {K} G {growth(gates):.3e} err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert np.isfinite(err) and err <= bound, label


def oracle(a_logical, gates):
    psi = np.asarray(a_logical).astype(np.complex128)
    for m, dims in gates:
        psi = numpy_gate(psi, m, [d % psi.ndim for d in dims])
    return psi


def random_circuit(rng, nq, count):
    """One- and two-qubit gates in turn, d0 < d1 and d0 > d1, random unitaries and every fourth matrix not unitary."""
    gates = []
    for g in range(count):
        k = 1 + (g % 3 != 0)
        dims = sorted(int(x) for x in rng.choice(nq, size=k, replace=False))
        if g % 2:
            dims = dims[::-1]
        m = random_unitary(rng, 2 ** k)
        if g % 4 == 3:
            m = 0.8 * (rng.standard_normal((2 ** k, 2 ** k)) + 1j * rng.standard_normal((2 ** k, 2 ** k))) / 2 ** (k / 2)
        gates.append((m, tuple(dims)))
    return gates


# ---- 1. random circuits -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_case(nq):
    rng = np.random.default_rng(900 + nq)
    gates = random_circuit(rng, nq, 24)
    a128 = crand(rng, (2,) * nq, "c128")
    inputs = {"c64": a128.astype(np.complex64), "c128": a128}
    return gates, inputs, {kind: oracle(inputs[kind], gates) for kind in inputs}


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [9, 10, 11, 12, 14])
def test_random_circuits(nq, kind):
    gates, inputs, want = random_case(nq)
    assert {len(d) for _, d in gates} == {1, 2} and any(d[0] > d[-1] for _, d in gates) and any(d[0] < d[-1] for _, d in gates)
    t = gpu(inputs[kind])
    ptr = t.data_ptr()
    assert A.apply_gates_(t, gates) is t and t.data_ptr() == ptr
    check(t, want[kind], inputs[kind], gates, kind, f"random {nq} qubits {kind}")


# ---- 2. every addressing form -------------------------------------------------------------------------------------------------
def addressing_gates(bit):
    """bit: memory bit -> dim.  One-qubit gates on a register, a piece and a high bit; two-qubit gates on all six unordered pairs
    of classes (and both high-high forms: neighbours and the two ends), in both orders of dims."""
    reg, piece, high = (0, 1), (2, 9, 5), (10, 12, 11)
    one = [(ASYM1, (bit[b],)) for b in (reg[0], reg[1], piece[0], piece[1], high[0], high[1])]
    pairs = [(reg[0], reg[1]), (reg[1], piece[0]), (reg[0], high[1]), (piece[0], piece[1]), (piece[2], high[0]), (high[0], high[2]),
             (high[0], high[1])]
    two = []
    for b0, b1 in pairs:
        two += [(ASYM2, (bit[b0], bit[b1])), (ASYM2, (bit[b1], bit[b0]))]
    return one + two


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("layout", ["contiguous", "permuted"])
def test_every_addressing_form(layout, kind):
    nq = 13
    rng = np.random.default_rng(13)
    a = crand(rng, (2,) * nq, kind)
    perm = list(range(nq)) if layout == "contiguous" else [7, 0, 11, 3, 12, 5, 1, 9, 2, 10, 4, 8, 6]
    store = gpu(a)
    view = store.permute(perm)
    assert (layout == "contiguous") == view.is_contiguous()
    bit = {int(s).bit_length() - 1: d for d, s in enumerate(view.stride())}
    gates = addressing_gates(bit)
    info = A.gate_circuit_info(view.shape, view.stride(), gates, view.dtype)
    cls = lambda b: "r" if b < 2 else "p" if b < 10 else "h"                 # register, piece, high
    assert {tuple(sorted(cls(b) for b in bits)) for bits in info["bits"]} == \
        {("r",), ("p",), ("h",), ("r", "r"), ("p", "r"), ("h", "r"), ("p", "p"), ("h", "p"), ("h", "h")}
    logical = a.transpose(perm)
    for g, gate in enumerate(gates):                                       # each as a run of its own
        t = store.clone().permute(perm)
        A.apply_gate_(t, *gate)
        check(t, oracle(logical, [gate]), a, [gate], kind, f"{layout} {kind} gate {g} bits {info['bits'][g]}")
    t = store.clone().permute(perm)
    A.apply_gates_(t, gates)
    check(t, oracle(logical, gates), a, gates, kind, f"{layout} {kind} all {len(gates)} gates")


# ---- 3. cuts are invisible, bit for bit ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_the_result_does_not_depend_on_the_cuts(kind):
    nq = 14
    rng = np.random.default_rng(14)
    gates = random_circuit(rng, nq, 36) + [(ASYM2, (0, 3)), (ASYM1, (1,)), (ASYM2, (2, 0)), (ASYM1, (3,))]   # dims 0-3: bits 13-10
    a = crand(rng, (2,) * nq, kind)
    base = gpu(a)
    assert len(gates) == 40
    assert {b for bits in A.gate_circuit_info(base.shape, base.stride(), gates)["bits"] for b in bits} >= {10, 11, 12, 13}
    ref = base.clone()
    for gate in gates:                                                     # one call per gate
        A.apply_gate_(ref, *gate)
    check(ref, oracle(a, gates), a, gates, kind, f"one call per gate {kind}")
    runs = []
    for max_rank in range(5 if kind == "c64" else 4):
        t = base.clone()
        A.apply_gates_(t, gates, max_rank=max_rank)
        runs.append(A.gate_circuit_info(base.shape, base.stride(), gates, base.dtype, max_rank)["n_runs"])
        assert torch.equal(bits_of(t), bits_of(ref)), max_rank
    assert runs == sorted(runs, reverse=True) and runs[0] > runs[-1] and (kind == "c128" or runs[-1] == 1)
    circ = A.GateCircuit(base.shape, base.stride(), base.dtype, gates, base.device)
    t = base.clone()
    assert circ(t) is t and torch.equal(bits_of(t), bits_of(ref))
    t = base.clone()
    circ(t)                                                                # (a second call of the prebuilt circuit: run to run)
    assert torch.equal(bits_of(t), bits_of(ref))


# ---- 4. exactness -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [9, 13])
def test_exact_gates(nq, kind):
    rng = np.random.default_rng(40 + nq)
    a = crand(rng, (2,) * nq, kind)
    a.real[rng.random(a.shape) < 0.2] = -0.0
    a.imag[rng.random(a.shape) < 0.2] = 0.0
    a.imag[rng.random(a.shape) < 0.1] = -0.0
    base = gpu(a)
    dims = sorted({0, 1, nq - 1, nq - 2, nq - 4, nq // 2})                  # high, piece and register bits
    # the identity, one and two qubits, fused with each other
    t = base.clone()
    A.apply_gates_(t, [(np.eye(2), (d,)) for d in dims] + [(np.eye(4), (d, e)) for d in dims for e in dims if d != e])
    assert torch.equal(bits_of(t), bits_of(base))
    # X, Y, Z as matrices are pauli_apply_
    for d in dims:
        for letter, m in (("X", X), ("Y", Y), ("Z", Z)):
            got, want = A.apply_gate_(base.clone(), m, (d,)), A.pauli_apply_(base.clone(), {d: letter})
            assert torch.equal(bits_of(got), bits_of(want)), (d, letter)
    # CNOT, SWAP, CZ, S as torch index and sign operations
    idx = [slice(None)] * nq

    def at(**fixed):
        out = list(idx)
        for d, v in fixed.items():
            out[int(d[1:])] = v
        return tuple(out)

    for c in dims:
        got, want = A.apply_gate_(base.clone(), S, (c,)), base.clone()
        one = want[at(**{f"d{c}": 1})]
        want[at(**{f"d{c}": 1})] = torch.complex(-one.imag, one.real)       # i (x + i y) = -y + i x
        assert torch.equal(bits_of(got), bits_of(want)), ("S", c)
        for t_ in dims:
            if t_ == c:
                continue
            got, want = A.apply_gate_(base.clone(), CNOT, (c, t_)), base.clone()
            want[at(**{f"d{c}": 1})] = base[at(**{f"d{c}": 1})].flip(t_ - (t_ > c))
            assert torch.equal(bits_of(got), bits_of(want)), ("CNOT", c, t_)
            got, want = A.apply_gate_(base.clone(), SWAP, (c, t_)), base.transpose(c, t_).contiguous()
            assert torch.equal(bits_of(got), bits_of(want)), ("SWAP", c, t_)
            got, want = A.apply_gate_(base.clone(), CZ, (c, t_)), base.clone()
            want[at(**{f"d{c}": 1, f"d{t_}": 1})] = -base[at(**{f"d{c}": 1, f"d{t_}": 1})]
            assert torch.equal(bits_of(got), bits_of(want)), ("CZ", c, t_)
    # a signed permutation and its inverse, in one circuit and in two calls
    perms = [(ISWAP, (0, nq - 1)), (CNOT, (nq - 2, 1)), (Y, (nq // 2,)), (S, (0,)), (SWAP, (1, nq - 4))]
    inverse = [(np.asarray(m).conj().T, d) for m, d in perms[::-1]]
    t = A.apply_gates_(base.clone(), perms + inverse)
    assert torch.equal(bits_of(t), bits_of(base))
    t = A.apply_gates_(A.apply_gates_(base.clone(), perms, max_rank=0), inverse)
    assert torch.equal(bits_of(t), bits_of(base))
    assert not torch.equal(bits_of(A.apply_gates_(base.clone(), perms)), bits_of(base))


# ---- 5. more blocks than workgroups -------------------------------------------------------------------------------------------
def test_grid_stride_over_4096_tiles():
    nq = 22
    rng = np.random.default_rng(22)
    a = crand(rng, (2,) * nq)
    base = gpu(a)
    assert a.size // 1024 == 4096 > 2048                                   # (2048: the grid cap)
    local = [(ASYM2, (nq - 3, nq - 1))]                                     # memory bits 2 and 0: one run of rank 0, 4096 blocks
    info = A.gate_circuit_info(base.shape, base.stride(), local)
    assert info["n_runs"] == 1 and info["run_rank"] == [0] and info["bits"] == [(2, 0)]
    want = oracle(a, local)
    check(A.apply_gates_(base.clone(), local), want, a, local, "c64", "2^22, bits 2 and 0")
    slow = local + [(ASYM1, (0,)), (ASYM2, (2, 0)), (ASYM2, (1, nq - 4))]   # the slowest bit; bits 19 and 21; bits 20 and 3
    want = oracle(want, slow[1:])
    for max_rank, runs in ((0, 3), (3, 1)):
        assert A.gate_circuit_info(base.shape, base.stride(), slow, max_rank=max_rank)["n_runs"] == runs
        check(A.apply_gates_(base.clone(), slow, max_rank=max_rank), want, a, slow, "c64", f"2^22, the slowest bit, max_rank {max_rank}")


# ---- 6. the n12 circuit end to end --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def n12_case():
    bonds, nq = n12_gates()
    gates = A.gates_from_bonds(bonds, nq)
    psi = np.zeros((2,) * nq, dtype=np.complex128)
    psi[(0,) * nq] = 1
    return bonds, gates, nq, psi, oracle(psi, gates)


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_the_n12_circuit(kind):
    bonds, gates, nq, psi0, want = n12_case()
    dtype = torch.complex64 if kind == "c64" else torch.complex128
    state = A.run_circuit(gates, nq, dtype=dtype, device=DEV)
    assert state.shape == (2,) * nq and state.is_contiguous() and state.dtype == dtype
    check(state, want, psi0, gates, kind, f"n12 {kind}")
    golden = load_case(os.path.join(GOLDEN, "n12_dense.npz")).arrays["state_vec"]
    err = amp_rel(state.cpu().numpy().reshape(-1), golden)
    print(f"n12 {kind} against the golden state vector: amp_rel {err:.3e}")
    assert err < 1e-5
    sv = A.state_vec(bonds, nq, dtype=dtype, device=DEV)
    fid = A.fidelity(state, sv.contiguous())
    print(f"n12 {kind} fidelity with state_vec: {fid!r}")
    assert abs(fid - 1) < 1e-5
    merged = A.run_circuit(A.merge_gates(gates), nq, dtype=dtype, device=DEV)
    assert amp_rel(merged.cpu().numpy().reshape(-1), golden) < 1e-5


# ---- 7. layouts and interop ---------------------------------------------------------------------------------------------------
def test_gates_on_the_permuted_output_of_the_n12_contraction():
    case = load_case(os.path.join(GOLDEN, "n12_dense.npz"))
    raw = A.tensor_contraction(case.fresh_tensors(device=DEV), case.scheme)
    out = raw.permute(tuple(case.meta["permute_dims"]))                    # dim q = qubit q: what the simulation returns, a view
    assert out.shape == (2,) * 12 and out.data_ptr() == raw.data_ptr() and not out.is_contiguous()
    assert sorted(out.stride()) == [2 ** b for b in range(12)] and list(out.stride()) != sorted(out.stride(), reverse=True)
    rng = np.random.default_rng(12)
    gates = random_circuit(rng, 12, 16)
    a = out.cpu().numpy()
    strides = out.stride()
    assert A.apply_gates_(out, gates) is out and out.data_ptr() == raw.data_ptr() and out.stride() == strides
    check(out, oracle(a, gates), a, gates, "c64", "n12 contraction output")


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_a_rotation_as_a_gate_is_pauli_rotate(kind):
    nq, theta = 12, 0.37
    rng = np.random.default_rng(3)
    a = crand(rng, (2,) * nq, kind)
    rx = np.cos(theta) * np.eye(2) - 1j * np.sin(theta) * X
    for q in (0, 5, nq - 1):
        gate = (rx, (q,))
        got = A.apply_gate_(gpu(a), *gate)
        other = A.pauli_rotate_(gpu(a), {q: "X"}, theta)
        check(got, other.cpu().numpy().astype(np.complex128), a, [gate, gate], kind, f"exp(-i theta X_{q}) {kind}")
        check(got, oracle(a, [gate]), a, [gate], kind, f"exp(-i theta X_{q}) {kind} against numpy")


# ---- 8. states below one tile -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [1, 2, 5])
def test_small_states(nq, kind):
    rng = np.random.default_rng(70 + nq)
    a = crand(rng, (2,) * nq, kind)
    base = gpu(a)
    if nq == 1:
        gates = [(random_unitary(rng, 2), (0,)), (ASYM1, (0,)), (S, (-1,)), (random_unitary(rng, 2), (0,))]
    else:
        gates = random_circuit(rng, nq, 12) + [(ASYM2, (0, nq - 1)), (ASYM2, (nq - 1, 0)), (ASYM1, (nq - 1,)), (CNOT, (1, 0))]
        assert any(len(d) == 2 and d[0] < d[1] for _, d in gates) and any(len(d) == 2 and d[0] > d[1] for _, d in gates)
    info = A.gate_circuit_info(base.shape, base.stride(), gates, base.dtype)
    assert info["n_runs"] == 1 and info["run_rank"] == [0] and info["max_rank"] == 0
    for g, gate in enumerate(gates[-4:]):                                  # each alone, then the circuit
        t = base.clone()
        A.apply_gate_(t, *gate)
        check(t, oracle(a, [gate]), a, [gate], kind, f"[2]*{nq} {kind} gate {g} on dims {gate[1]}")
    t = base.clone()
    assert A.apply_gates_(t, gates) is t
    check(t, oracle(a, gates), a, gates, kind, f"[2]*{nq} {kind} {len(gates)} gates")


# ---- 9. layouts that are not [2]*n --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("layout", ["extents 4 and 8", "extent 1"])
def test_non_qubit_layouts(layout, kind):
    rng = np.random.default_rng(9)
    if layout == "extents 4 and 8":
        shape, perm = (4, 2, 2, 2, 8, 2, 2, 2, 2), (1, 0, 3, 2, 5, 4, 7, 6, 8)
    else:
        shape, perm = (1, 2, 2, 1) + (2,) * 10 + (1,), (0, 5, 2, 3, 1, 4, 6, 7, 8, 9, 10, 11, 13, 12, 14)
    a = crand(rng, shape, kind)
    t = gpu(a).permute(perm)
    logical = a.transpose(perm)
    twos = [d for d, e in enumerate(t.shape) if e == 2]
    assert len(twos) == (7 if layout == "extents 4 and 8" else 12) and not t.is_contiguous()
    gates = [(ASYM1, (d,)) for d in twos] + [(ASYM2, (d, e)) for d, e in zip(twos, twos[1:] + twos[:1])] \
        + [(ASYM2, (twos[-1], twos[0])), (random_unitary(rng, 4), (twos[len(twos) // 2], twos[1]))]
    assert {d for _, dims in gates for d in dims} == set(twos)
    info = A.gate_circuit_info(t.shape, t.stride(), gates, t.dtype)
    assert info["bits"] == [tuple(int(t.stride(d)).bit_length() - 1 for d in dims) for _, dims in gates]   # extent 2: stride = 2^bit
    assert all(t.stride(d) == 1 << b for (_, dims), bits in zip(gates, info["bits"]) for d, b in zip(dims, bits))
    strides = t.stride()
    assert A.apply_gates_(t, gates) is t and t.stride() == strides
    check(t, oracle(logical, gates), a, gates, kind, f"{layout} {kind}: {len(gates)} gates on dims {twos}")


# ---- 10. argument checks ------------------------------------------------------------------------------------------------------
def test_argument_checks():
    t = gpu(np.zeros((2,) * 4, dtype=np.complex64))
    gates = [(ASYM1, (0,)), (ASYM2, (3, 1))]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_gates_(t.cpu(), gates)
    with pytest.raises(TypeError, match="complex"):
        A.apply_gate_(t.real.contiguous(), ASYM1, (0,))
    with pytest.raises(ValueError, match="dense"):
        A.apply_gate_(t[:, :, ::2], ASYM1, (0,))
    odd = torch.zeros(17, dtype=torch.complex64, device=DEV)[1:].view((2,) * 4)
    with pytest.raises(ValueError, match="16-byte"):
        A.apply_gates_(odd, gates)
    with pytest.raises(ValueError, match="at least one"):
        A.apply_gates_(t, [])
    with pytest.raises(RuntimeError, match="artn error -2.*max_rank"):
        A.apply_gates_(t, gates, max_rank=5)
    with pytest.raises(RuntimeError, match="artn error -2"):
        A.apply_gate_(t, np.eye(8), (0, 1, 2))
    with pytest.raises(RuntimeError, match="artn error -1.*differ"):
        A.apply_gate_(t, ASYM2, (1, 1))
    with pytest.raises(RuntimeError, match="artn error -1.*out of range"):
        A.apply_gate_(t, ASYM1, (4,))
    with pytest.raises(RuntimeError, match="artn error -1.*finite"):
        A.apply_gate_(t, ASYM1 * np.nan, (0,))
    with pytest.raises(RuntimeError, match="artn error -1.*extent"):
        A.apply_gate_(gpu(np.zeros((2, 4), dtype=np.complex64)), ASYM1, (1,))
    circ = A.GateCircuit(t.shape, t.stride(), t.dtype, gates, t.device)
    assert circ(t) is t
    with pytest.raises(ValueError, match="built for"):
        circ(gpu(np.zeros((2,) * 5, dtype=np.complex64)))
    with pytest.raises(ValueError, match="built for"):
        circ(t.permute(3, 2, 1, 0))
    with pytest.raises(ValueError, match="built for"):
        circ(t.to(torch.complex128))
    with pytest.raises(ValueError, match="16-byte"):
        circ(odd)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        circ(t.cpu())
    circ._table = circ._table.cpu()                                        # (stands in for a second device)
    with pytest.raises(ValueError, match="built for cpu"):
        circ(t)
