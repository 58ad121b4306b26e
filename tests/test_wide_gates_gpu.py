"""Wide gates on the device (artensor_amd/wide_gates.py: apply_wide_gate_, WideGate, FusedCircuit, apply_circuit_;
artn_wgate_apply) against the reference of test_gates_gpu -- np.tensordot of the gate's [2]*2k tensor with the complex128 copy of
the LOGICAL array -- under its bound, which is derived and not measured: every output component is formed in float64 and rounded
ONCE, so ||y - ref||_2 <= 2 K 2^-24 ||a||_2 G in complex64 and 32 K 2^-53 ||a||_2 G in complex128 (K gates, G the product of
max(1, ||U||_2)).  A 32-term complex sum in float64 adds at most about (2 * 32 + 2) 2^-53 ||U||_F ||x||_2 <= 66 * 2^-53 * sqrt(32)
||U||_2 ||x||_2 per element group before the rounding -- invisible in complex64, and in complex128 the measured ratios are
printed next to the bound.  Everything the arithmetic contract makes exact is compared bit for bit."""
import functools
import os

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd.fixtures import load_case
from test_gates_cpu import n12_gates, numpy_gate, random_unitary
from test_gates_gpu import ASYM1, ASYM2, X, Y, Z, check, oracle
from test_gpu_parity import amp_rel
from test_pauli_apply_gpu import DEV, GOLDEN, crand, gpu
from test_pauli_evolve_gpu import bits_of

pytestmark = pytest.mark.gpu

TB = {"c64": 12, "c128": 11}
PERM14 = [7, 0, 11, 3, 12, 5, 1, 9, 13, 2, 10, 4, 8, 6]


def asym(k, seed=0):
    """An asymmetric matrix that is not unitary: a transposed or permuted index is an O(1) error."""
    rng = np.random.default_rng(1000 + 10 * k + seed)
    return 0.8 * (rng.standard_normal((2 ** k, 2 ** k)) + 1j * rng.standard_normal((2 ** k, 2 ** k))) / 2 ** (k / 2)


def embed(m, pos, k):
    """m on the digits `pos` of a k-qubit matrix (digit 0 the most significant), identities elsewhere."""
    u = np.eye(2 ** k, dtype=np.complex128).reshape((2,) * k + (2 ** k,))
    return numpy_gate(u, m, list(pos)).reshape(2 ** k, 2 ** k)


def layout(a, permuted, rng):
    """(device view, logical numpy array) of the array a: as it is, or under a random permutation of its dims."""
    perm = [int(p) for p in rng.permutation(a.ndim)] if permuted else list(range(a.ndim))
    return gpu(a).permute(perm), a.transpose(perm)


def bit_to_dim(view):
    return {int(s).bit_length() - 1: d for d, s in enumerate(view.stride())}


# ---- 1. random dense gates ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("k", [3, 4, 5])
def test_random_dense_gates(k, kind):
    rng = np.random.default_rng(300 + k)
    for nq in (k, 9, 11, 12, 13, 14):
        a = crand(rng, (2,) * nq, kind)
        for permuted in (False, True):
            for name, m in (("unitary", random_unitary(rng, 2 ** k)), ("not unitary", asym(k, nq))):
                view, logical = layout(a, permuted, rng)
                dims = tuple(int(x) for x in rng.permutation(nq)[:k])
                if k > 1 and list(dims) == sorted(dims):
                    dims = dims[::-1]
                ptr, strides = view.data_ptr(), view.stride()
                assert A.apply_wide_gate_(view, m, dims) is view and view.data_ptr() == ptr and view.stride() == strides
                gate = (m, dims)
                check(view, oracle(logical, [gate]), a, [gate], kind, f"k {k} {kind} [2]*{nq} {'permuted' if permuted else 'contiguous'} {name} dims {dims}")


# ---- 2. every addressing form -------------------------------------------------------------------------------------------------
def target_sets(k, kind):
    """Memory bits of a 2^14 state: below the tile's contiguous part, inside it, the top (at or above TB as far as 14 bits
    allow), and each mixture of two."""
    mid = [3, 5, 8, 6, 9][:k]
    sets = {"low": list(range(k)), "mid": mid, "top": list(range(14 - k, 14)),
            "low+mid": [0, 1] + mid[:k - 2], "low+high": [1, 0, 2][:k - 2] + [13, 12], "mid+high": mid[:k - 2] + [12, 13],
            "low+mid+high": [0, 7, 13, 4, 12][:k]}
    if kind == "c128" and k == 3:
        sets["at or above TB"] = [11, 12, 13]
    assert all(len(set(s)) == k for s in sets.values())
    return sets


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("k", [3, 4, 5])
def test_every_addressing_form(k, kind):
    nq = 14
    rng = np.random.default_rng(14 + k)
    a = crand(rng, (2,) * nq, kind)
    store = gpu(a)
    logical = a.transpose(PERM14)
    bit = bit_to_dim(store.permute(PERM14))
    m = asym(k)
    for name, bits in target_sets(k, kind).items():
        for order in (bits, bits[::-1][1:] + bits[::-1][:1]):
            dims = tuple(bit[b] for b in order)
            view = store.clone().permute(PERM14)
            info = A.wide_gate_info(view.shape, view.stride(), m, dims, view.dtype)
            assert info["target_bits"] == tuple(order) and info["tb"] == TB[kind] and info["n_tiles"] == 2 ** (nq - TB[kind])
            A.apply_wide_gate_(view, m, dims)
            gate = (m, dims)
            check(view, oracle(logical, [gate]), a, [gate], kind, f"k {k} {kind} {name} bits {order} segment {info['segment']}")


# ---- 3. exactness -------------------------------------------------------------------------------------------------------------
def signed_zero_state(rng, nq, kind):
    a = crand(rng, (2,) * nq, kind)
    a.real[rng.random(a.shape) < 0.2] = -0.0
    a.imag[rng.random(a.shape) < 0.2] = 0.0
    a.imag[rng.random(a.shape) < 0.1] = -0.0
    return a


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [5, 9, 13])
def test_narrow_gates_and_their_embeddings_are_apply_gate_bit_for_bit(nq, kind):
    rng = np.random.default_rng(50 + nq)
    base, _ = layout(signed_zero_state(rng, nq, kind), nq == 13, rng)
    # k = 1 and k = 2 through the wide kernel
    for d in (0, nq // 2, nq - 1):
        for m in (ASYM1, random_unitary(rng, 2)):
            got, want = A.apply_wide_gate_(base.clone(), m, (d,)), A.apply_gate_(base.clone(), m, (d,))
            assert torch.equal(bits_of(got), bits_of(want)), ("k 1", d)
    for dims in ((0, nq - 1), (nq - 1, 0), (1, nq // 2), (nq - 2, nq - 1), (nq // 2, 1)):
        for m in (ASYM2, random_unitary(rng, 4)):
            got, want = A.apply_wide_gate_(base.clone(), m, dims), A.apply_gate_(base.clone(), m, dims)
            assert torch.equal(bits_of(got), bits_of(want)), ("k 2", dims)
    # a narrow matrix kron identities: the surviving terms come in the same order
    for k in (3, 4, 5):
        dims = tuple(int(x) for x in rng.permutation(nq)[:k])
        for i in range(k):                                                # identities below, between and above
            got = A.apply_wide_gate_(base.clone(), embed(ASYM1, [i], k), dims)
            assert torch.equal(bits_of(got), bits_of(A.apply_gate_(base.clone(), ASYM1, (dims[i],)))), (k, dims, i)
        for i, j in {(0, 1), (0, k - 1), (k - 2, k - 1), (1, k - 1), (0, k // 2)}:
            if i >= j:
                continue
            got = A.apply_wide_gate_(base.clone(), embed(ASYM2, [i, j], k), dims)
            assert torch.equal(bits_of(got), bits_of(A.apply_gate_(base.clone(), ASYM2, (dims[i], dims[j])))), (k, dims, i, j)


def signed_permutation(base, m, dims):
    """new[row r] = phase * old[column c] for a matrix with one entry of {1, -1, i, -i} per row, by torch index and sign
    operations on the LOGICAL tensor."""
    k, nd = len(dims), base.dim()
    rest = [d for d in range(nd) if d not in dims]
    front = base.permute(list(dims) + rest)
    rows = front.reshape(2 ** k, -1)
    out = torch.empty_like(rows)
    for r in range(2 ** k):
        (c,) = np.nonzero(m[r])[0]
        x, phase = rows[c], complex(m[r, c])
        out[r] = {1: x, -1: torch.complex(-x.real, -x.imag), 1j: torch.complex(-x.imag, x.real), -1j: torch.complex(x.imag, -x.real)}[phase]
    back = np.argsort(list(dims) + rest)
    return out.reshape(front.shape).permute([int(p) for p in back])


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [5, 13])
def test_exact_gates(nq, kind):
    rng = np.random.default_rng(60 + nq)
    base, _ = layout(signed_zero_state(rng, nq, kind), nq == 13, rng)
    toffoli = np.eye(8)[[0, 1, 2, 3, 4, 5, 7, 6]].astype(np.complex128)      # the first two listed dims control the last
    fredkin = np.eye(8)[[0, 1, 2, 3, 4, 6, 5, 7]].astype(np.complex128)      # the first controls the swap of the others
    ccz = np.diag([1, 1, 1, 1, 1, 1, 1, -1]).astype(np.complex128)
    phases = np.zeros((32, 32), dtype=np.complex128)
    phases[np.arange(32), rng.permutation(32)] = rng.choice([1, -1, 1j, -1j], size=32)
    for name, m in (("Toffoli", toffoli), ("Fredkin", fredkin), ("CCZ", ccz), ("32 phases", phases)):
        k = int(np.log2(m.shape[0]))
        for dims in (tuple(int(x) for x in rng.permutation(nq)[:k]), tuple(range(nq - k, nq)), tuple(range(k))[::-1]):
            got = A.apply_wide_gate_(base.clone(), m, dims)
            assert torch.equal(bits_of(got), bits_of(signed_permutation(base, m, dims))), (name, dims)
            assert not torch.equal(bits_of(got), bits_of(base)), (name, dims)
            assert torch.equal(bits_of(A.apply_wide_gate_(got, m.conj().T, dims)), bits_of(base)), (name, dims, "inverse")
    c1, c2, t = 0, nq - 1, nq // 2                                         # Toffoli once more, spelled out
    want = base.clone()
    idx = [slice(None)] * nq
    idx[c1], idx[c2] = 1, 1
    want[tuple(idx)] = base[tuple(idx)].flip(t - 1)
    assert torch.equal(bits_of(A.apply_wide_gate_(base.clone(), toffoli, (c1, c2, t))), bits_of(want))
    # a Pauli string as a 32 x 32 matrix is pauli_apply_
    p2 = {"I": np.eye(2), "X": X, "Y": Y, "Z": Z}
    for letters in ("XYZIY", "ZZXIX", "YIYXZ"):
        dims = tuple(int(x) for x in rng.permutation(nq)[:5])
        m = functools.reduce(np.kron, [p2[c] for c in letters])
        got = A.apply_wide_gate_(base.clone(), m, dims)
        want = A.pauli_apply_(base.clone(), {d: c for d, c in zip(dims, letters) if c != "I"})
        assert torch.equal(bits_of(got), bits_of(want)), (letters, dims)
    # the identity, signed zeros included; run to run
    for dims in (tuple(range(5)), tuple(int(x) for x in rng.permutation(nq)[:5])):
        assert torch.equal(bits_of(A.apply_wide_gate_(base.clone(), np.eye(32), dims)), bits_of(base))
    m, dims = asym(5), tuple(int(x) for x in rng.permutation(nq)[:5])
    gate = A.WideGate(base.shape, base.stride(), base.dtype, m, dims, base.device)
    assert torch.equal(bits_of(gate(base.clone())), bits_of(A.apply_wide_gate_(base.clone(), m, dims)))


# ---- 4. neighbours untouched --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [3, 5, 10, 13])
def test_the_elements_around_the_state_are_untouched(nq, kind):
    rng = np.random.default_rng(80 + nq)
    n, pad = 2 ** nq, 4098
    a = crand(rng, (2,) * nq, kind)
    sentinel = complex(-7.25, 1234.5)
    buf = torch.full((n + 2 * pad,), sentinel, dtype=torch.complex64 if kind == "c64" else torch.complex128, device=DEV)
    buf[pad:pad + n] = gpu(a).reshape(-1)
    view = buf[pad:pad + n].view((2,) * nq)
    assert view.data_ptr() % 16 == 0 and view.data_ptr() == buf.data_ptr() + pad * buf.element_size()
    k = min(nq, 4)
    gate = (asym(k), tuple(int(x) for x in rng.permutation(nq)[:k]))
    A.apply_wide_gate_(view, *gate)
    check(view, oracle(a, [gate]), a, [gate], kind, f"[2]*{nq} {kind} inside a larger buffer")
    assert bool((buf[:pad] == sentinel).all()) and bool((buf[pad + n:] == sentinel).all())


# ---- 5. more tiles than workgroups --------------------------------------------------------------------------------------------
def test_grid_stride_over_4096_tiles():
    nq = 24
    rng = np.random.default_rng(24)
    a = crand(rng, (2,) * nq)
    t = gpu(a)
    gates = [(asym(4, 1), (nq - 1, nq - 3, nq - 2, nq - 4)), (asym(4, 2), (9, 12, 10, 11)), (asym(4, 3), (2, 0, 3, 1))]   # low, middle, top
    for m, dims in gates:
        info = A.wide_gate_info(t.shape, t.stride(), m, dims)
        assert info["n_tiles"] == 4096 > 2048                              # (2048: the grid cap)
        A.apply_wide_gate_(t, m, dims)
    assert A.wide_gate_info(t.shape, t.stride(), *gates[0])["target_bits"] == (0, 2, 1, 3)
    assert A.wide_gate_info(t.shape, t.stride(), *gates[2])["target_bits"] == (21, 23, 20, 22)
    check(t, oracle(a, gates), a, gates, "c64", "2^24: k 4 on low, middle and top bits")


# ---- 6. FusedCircuit ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def n12_case():
    bonds, nq = n12_gates()
    return bonds, A.gates_from_bonds(bonds, nq), nq


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("width", [3, 4, 5])
def test_the_n12_circuit_after_fuse_gates(width, kind):
    bonds, gates, nq = n12_case()
    dtype = torch.complex64 if kind == "c64" else torch.complex128
    fused = A.fuse_gates(gates, width)
    assert max(len(d) for _, d in fused) == width
    state = torch.zeros((2,) * nq, dtype=dtype, device=DEV)
    state[(0,) * nq] = 1
    circ = A.FusedCircuit(state.shape, state.stride(), dtype, fused, DEV)
    assert circ(state) is state
    golden = load_case(os.path.join(GOLDEN, "n12_dense.npz")).arrays["state_vec"]
    err = amp_rel(state.cpu().numpy().reshape(-1), golden)
    fid = A.fidelity(state, A.state_vec(bonds, nq, dtype=dtype, device=DEV).contiguous())
    print(f"n12 {kind} width {width}: {len(gates)} -> {len(fused)} gates, {circ.n_launches} launches, amp_rel {err:.3e}, fidelity {fid!r}")
    assert err < 1e-5 and abs(fid - 1) < 1e-5


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_fused_circuits(kind):
    nq = 13
    rng = np.random.default_rng(130)
    a = crand(rng, (2,) * nq, kind)
    base, logical = layout(a, True, rng)
    narrow = []
    for g in range(20):
        k = 1 + g % 2
        narrow.append((random_unitary(rng, 2 ** k), tuple(int(x) for x in rng.permutation(nq)[:k])))
    # narrow gates only: one GateCircuit, apply_gates_ bit for bit
    for max_rank in (None, 0):
        circ = A.FusedCircuit(base.shape, base.stride(), base.dtype, narrow, DEV, max_rank=max_rank)
        runs = A.gate_circuit_info(base.shape, base.stride(), narrow, base.dtype, max_rank)["n_runs"]
        assert len(circ.parts) == 1 and circ.n_launches == runs and circ.n_wide == 0
        assert torch.equal(bits_of(circ(base.clone())), bits_of(A.apply_gates_(base.clone(), narrow, max_rank=max_rank)))
    # widths 1..5 mixed
    mixed = []
    for g, k in enumerate([1, 2, 3, 2, 1, 5, 4, 4, 1, 2, 2, 3, 5, 1]):
        m = random_unitary(rng, 2 ** k) if g % 4 else asym(k, g)
        mixed.append((m, tuple(int(x) for x in rng.permutation(nq)[:k])))
    circ = A.FusedCircuit(base.shape, base.stride(), base.dtype, mixed, DEV, max_rank=0)
    stretches = [mixed[0:2], mixed[3:5], mixed[8:11], mixed[13:14]]
    runs = [A.gate_circuit_info(base.shape, base.stride(), s, base.dtype, 0)["n_runs"] for s in stretches]
    assert [type(p).__name__ for p in circ.parts] == ["GateCircuit", "WideGate", "GateCircuit", "WideGate", "WideGate", "WideGate",
                                                      "GateCircuit", "WideGate", "WideGate", "GateCircuit"]
    assert circ.n_wide == 6 and circ.n_launches == sum(runs) + 6 and circ.n_gates == len(mixed)
    t = base.clone()
    assert circ(t) is t
    check(t, oracle(logical, mixed), a, mixed, kind, f"mixed widths {kind}: {circ.n_launches} launches")
    assert torch.equal(bits_of(A.apply_circuit_(base.clone(), mixed, max_rank=0)), bits_of(t))


# ---- 7. layouts that are not [2]*n --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_non_qubit_layouts(kind):
    rng = np.random.default_rng(7)
    shape, perm = (4, 2, 2, 2, 8, 2, 2, 2, 2, 2), (1, 0, 3, 2, 5, 4, 7, 6, 9, 8)
    a = crand(rng, shape, kind)
    t = gpu(a).permute(perm)
    logical = a.transpose(perm)
    twos = [d for d, e in enumerate(t.shape) if e == 2]
    assert len(twos) == 8 and not t.is_contiguous()
    gates = [(asym(3), (twos[0], twos[7], twos[3])), (asym(4), (twos[6], twos[1], twos[2], twos[5])),
             (asym(5), (twos[4], twos[0], twos[7], twos[2], twos[6]))]
    strides = t.stride()
    for gate in gates:
        assert A.wide_gate_info(t.shape, strides, *gate, t.dtype)["target_bits"] == tuple(int(strides[d]).bit_length() - 1 for d in gate[1])
        assert A.apply_wide_gate_(t, *gate) is t and t.stride() == strides
    check(t, oracle(logical, gates), a, gates, kind, f"extents 4 and 8 {kind}")
    four = [d for d, e in enumerate(t.shape) if e == 4][0]
    with pytest.raises(RuntimeError, match="artn error -1.*extent 4"):
        A.apply_wide_gate_(t, asym(3), (twos[0], four, twos[1]))


# ---- 8. argument checks -------------------------------------------------------------------------------------------------------
def test_argument_checks():
    t = gpu(np.zeros((2,) * 6, dtype=np.complex64))
    m3 = asym(3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_wide_gate_(t.cpu(), m3, (0, 1, 2))
    with pytest.raises(TypeError, match="complex"):
        A.apply_wide_gate_(t.real.contiguous(), m3, (0, 1, 2))
    with pytest.raises(ValueError, match="dense"):
        A.apply_wide_gate_(t[:, :, ::2], m3, (0, 1, 3))
    odd = torch.zeros(65, dtype=torch.complex64, device=DEV)[1:].view((2,) * 6)
    with pytest.raises(ValueError, match="16-byte"):
        A.apply_wide_gate_(odd, m3, (0, 1, 2))
    with pytest.raises(RuntimeError, match="artn error -2.*one to five"):
        A.apply_wide_gate_(t, np.eye(64), (0, 1, 2, 3, 4, 5))
    with pytest.raises(RuntimeError, match="artn error -1.*differ"):
        A.apply_wide_gate_(t, m3, (1, 2, 1))
    with pytest.raises(RuntimeError, match="artn error -1.*out of range"):
        A.apply_wide_gate_(t, m3, (0, 6, 1))
    with pytest.raises(RuntimeError, match="artn error -1.*finite"):
        A.apply_wide_gate_(t, m3 * np.inf, (0, 1, 2))
    with pytest.raises(ValueError, match="entries"):
        A.apply_wide_gate_(t, np.eye(4), (0, 1, 2))
    with pytest.raises(RuntimeError, match="artn error -1.*at least 2\\^3"):
        A.apply_wide_gate_(gpu(np.zeros((2, 2), dtype=np.complex64)), m3, (0, 1, 0))
    with pytest.raises(ValueError, match="at least one"):
        A.apply_circuit_(t, [])
    with pytest.raises(RuntimeError, match="artn error -2"):                # the old entry points still refuse three dims
        A.apply_gate_(t, m3, (0, 1, 2))
    for make in (lambda: A.WideGate(t.shape, t.stride(), t.dtype, m3, (0, 4, 2), t.device),
                 lambda: A.FusedCircuit(t.shape, t.stride(), t.dtype, [(ASYM1, (0,)), (m3, (0, 4, 2))], t.device)):
        obj = make()
        assert obj(t) is t
        with pytest.raises(ValueError, match="built for"):
            obj(gpu(np.zeros((2,) * 7, dtype=np.complex64)))
        with pytest.raises(ValueError, match="built for"):
            obj(t.permute(5, 4, 3, 2, 1, 0))
        with pytest.raises(ValueError, match="built for"):
            obj(t.to(torch.complex128))
        with pytest.raises(ValueError, match="16-byte"):
            obj(odd)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            obj(t.cpu())
        first = obj if isinstance(obj, A.WideGate) else obj.parts[0]
        first._table = first._table.cpu()                                  # (stands in for a second device)
        with pytest.raises(ValueError, match="built for cpu"):
            obj(t)
