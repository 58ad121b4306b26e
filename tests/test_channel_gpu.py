"""Noise channels on the device (artensor_amd/channel.py; artn_channel_choose / artn_channel_apply) against the numpy oracle
tests/channel_oracle.py and against apply_wide_gate_.

What is compared how.  The draw: the device's j equals the oracle's for uniforms that the test first proves (on the host) to lie
at least 1e-9 * total away from every boundary of the oracle's running sums; probability, total and scale agree to 1e-12
relative -- both sides add the same float64 terms, in another order.  The state: bit for bit (as integers) what
apply_wide_gate_ gives for the current matrix, which is itself compared exactly with K_j * scale recomputed on the host from the
record's j and scale.  Every state has at most 2^24 elements."""
import ctypes
import math

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd.pauli import _ptr

import channel_oracle as CO
import measure_oracle as MO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = {"c64": (np.complex64, torch.complex64, np.uint32), "c128": (np.complex128, torch.complex128, np.uint64)}
H = np.array([[1, 1], [1, -1]], dtype=np.complex128) / math.sqrt(2)
LAST = float(np.nextafter(1.0, 0.0))


def crand(rng, n, kind):
    a = rng.standard_normal((2,) * n) + 1j * rng.standard_normal((2,) * n)
    return a.astype(KINDS[kind][0])


def on_device(a, perm=None):
    """(base, view): the contiguous GPU tensor that owns the memory, and its permuted view (the same memory, never copied)."""
    base = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return base, (base if perm is None else base.permute(*perm))


def ints(base, kind):
    return base.cpu().numpy().view(KINDS[kind][2])


def dims_of_bits(n, bits):
    """dims of a CONTIGUOUS [2] * n tensor for memory bits: dim d is memory bit n - 1 - d."""
    return [n - 1 - b for b in bits]


def read(rec):
    host = rec.cpu().numpy()
    D2 = (host.size - 4) // 2
    D = int(round(math.sqrt(D2)))
    return int(host.view(np.int64)[0]), float(host[1]), float(host[2]), float(host[3]), host[4:].view(np.complex128).reshape(D, D)


def random_kraus(rng, t, m):
    """m operators with sum K^+ K = I: the blocks of a random isometry."""
    D = 2 ** t
    q, _ = np.linalg.qr(rng.standard_normal((m * D, D)) + 1j * rng.standard_normal((m * D, D)))
    return [q[j * D:(j + 1) * D] for j in range(m)]


def kron_all(*ms):
    out = np.eye(1, dtype=np.complex128)
    for m in ms:
        out = np.kron(out, m)
    return out


def diagonal_set(t):
    """A one-non-zero-per-column set on t qubits: products of amplitude damping (even positions) and phase damping (odd)."""
    factors = [CO.amplitude_damping(0.3) if q % 2 == 0 else CO.phase_damping(0.4) for q in range(t)]
    out = []
    for idx in np.ndindex(*(2,) * t):
        out.append(kron_all(*(factors[q][i] for q, i in enumerate(idx))))
    return out


def rotated_damping(gamma=0.3):
    return [H @ k @ H for k in CO.amplitude_damping(gamma)]


def case_channel(name):
    """(Channel, form, what the oracle's weights() takes, the matrices the device applies)."""
    rng = np.random.default_rng(77)
    if name.startswith("depol"):
        n = int(name[5:])
        probs, us = CO.depolarizing(0.6, n)
        return A.depolarizing(0.6, n), CO.FIXED, probs, us
    if name == "mix5":
        u, _ = np.linalg.qr(rng.standard_normal((32, 32)) + 1j * rng.standard_normal((32, 32)))
        us = [np.eye(32, dtype=np.complex128), CO.pauli_string([1, 0, 3, 2, 0]), u, np.diag(np.exp(1j * rng.standard_normal(32)))]
        probs = [0.25, 0.25, 0.25, 0.25]
        return A.Channel.mixture(probs, us), CO.FIXED, probs, us
    if name.startswith("diag"):
        ks = diagonal_set(int(name[4:]))
        return A.Channel.from_kraus(ks), CO.DIAGONAL, CO.effects(ks, CO.DIAGONAL), ks
    if name.startswith("dense"):
        t = int(name[5:])
        ks = rotated_damping() if t == 1 else random_kraus(rng, t, 5 - t)
        return A.Channel.from_kraus(ks), CO.DENSE, CO.effects(ks, CO.DENSE), ks
    raise KeyError(name)


UNIFORMS = [0.0, LAST] + [float(u) for u in np.random.default_rng(2024).random(298)]


# ---- the draw -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("name, dims", [("depol1", [2]), ("depol2", [4, 1]), ("diag1", [0]), ("diag2", [5, 2]), ("dense1", [3]),
                                        ("dense2", [1, 4])])
def test_the_draw_follows_the_oracle(name, dims, kind):
    rng = np.random.default_rng(31)
    a = crand(rng, 6, kind)                                   # 2^6: below a tile, one workgroup
    ch, form, packed, mats = case_channel(name)
    assert ch.form == form
    w, trace = CO.weights(form, packed, a, dims)
    total = float(np.cumsum(w)[-1])
    edges = CO.boundaries(w)
    # a property of the fixed-seed inputs, checked on the host before the device is asked
    for u in UNIFORMS[2:]:
        assert np.abs(edges - u * total).min() >= 1e-9 * total, (name, u)
    base, view = on_device(a)
    orig = base.clone()
    op = A.ChannelOp(view.shape, view.stride(), view.dtype, ch, dims, DEV)
    recs = []
    for u in UNIFORMS:
        base.copy_(orig)
        recs.append(op.step(view, uniform=u)[:4])
    host = torch.stack(recs).cpu().numpy()
    seen = set()
    for u, r in zip(UNIFORMS, host):
        j, p, tot, scale = CO.record(form, w, trace, u)
        gj = int(r.view(np.int64)[0])
        assert gj == j, (name, u, gj, j)
        for got, want in ((r[1], p), (r[2], tot), (r[3], scale)):
            assert abs(got - want) <= 1e-12 * abs(want), (name, u, got, want)
        seen.add(j)
    assert len(seen) == np.count_nonzero(w), (name, seen)     # (298 uniforms: every operator with a weight is drawn)


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_an_operator_of_weight_zero_is_never_drawn(kind):
    rng = np.random.default_rng(32)
    a = crand(rng, 6, kind)
    a[:, :, 1] = 0                                            # dim 2 in |0>: q[1] is exactly 0
    base, view = on_device(a)
    orig = base.clone()
    op = A.ChannelOp(view.shape, view.stride(), view.dtype, A.amplitude_damping(0.3), [2], DEV)
    recs = []
    for u in UNIFORMS:
        base.copy_(orig)
        recs.append(op.step(view, uniform=u)[:4])
    host = torch.stack(recs).cpu().numpy()
    assert (host[:, 0].copy().view(np.int64) == 0).all()
    assert (host[:, 1] == 1.0).all()


# ---- the state -------------------------------------------------------------------------------------------------------------------
def step_and_compare(a, perm, kind, ch, mats, dims, uniforms, renormalize=True):
    """Runs the step for every uniform from the same start; the result equals apply_wide_gate_ of the current matrix as integers,
    and the current matrix equals K_j * scale recomputed from the record."""
    base, view = on_device(a, perm)
    orig = base.clone()
    op = A.ChannelOp(view.shape, view.stride(), view.dtype, ch, dims, DEV)
    drawn = set()
    for u in uniforms:
        base.copy_(orig)
        j, p, total, scale, cur = read(op.step(view, uniform=u, renormalize=renormalize))
        assert 0 <= j < ch.m
        assert (cur.view(np.float64) == CO.current_matrix(mats[j], scale).view(np.float64)).all(), (j, scale)
        got = ints(base, kind).copy()
        base.copy_(orig)
        A.apply_wide_gate_(view, cur, dims)
        assert (got == ints(base, kind)).all(), (dims, u, j)
        drawn.add(j)
    return drawn


STATE_CASES = [
    # (n, kind, channel, memory bits of the targets): 2^13 complex64 and 2^12 complex128 are two tiles
    (13, "c64", "depol1", (0,)), (13, "c64", "diag1", (6,)), (13, "c64", "dense1", (12,)),
    (13, "c64", "depol2", (1, 0)), (13, "c64", "dense2", (7, 3)), (13, "c64", "diag2", (12, 11)),
    (13, "c64", "depol3", (0, 2, 1)), (13, "c64", "diag3", (10, 4, 8)), (13, "c64", "dense3", (12, 0, 11)),
    (13, "c64", "mix5", (12, 3, 11, 0, 7)),
    (12, "c128", "dense1", (0,)), (12, "c128", "depol1", (11,)), (12, "c128", "diag2", (5, 2)), (12, "c128", "dense2", (11, 10)),
    (12, "c128", "depol3", (11, 5, 0)), (12, "c128", "dense3", (3, 9, 10)), (12, "c128", "mix5", (1, 11, 4, 10, 0)),
]


@pytest.mark.parametrize("n, kind, name, bits", STATE_CASES)
def test_the_state_is_the_wide_gate_of_the_current_matrix(n, kind, name, bits):
    rng = np.random.default_rng(41)
    ch, form, packed, mats = case_channel(name)
    drawn = step_and_compare(crand(rng, n, kind), None, kind, ch, mats, dims_of_bits(n, bits), [0.03, 0.4, 0.62, 0.97])
    assert len(drawn) >= 2, drawn


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("name, seed", [("depol1", 1), ("diag2", 2), ("dense3", 3), ("mix5", 4), ("dense1", 5), ("depol3", 6)])
def test_the_state_in_random_permuted_layouts(name, seed, kind):
    rng = np.random.default_rng(50 + seed)
    n = 14
    perm = [int(x) for x in rng.permutation(n)]
    ch, form, packed, mats = case_channel(name)
    dims = [int(x) for x in rng.choice(n, size=ch.t, replace=False)]
    step_and_compare(crand(rng, n, kind), perm, kind, ch, mats, dims, [0.1, 0.55, 0.9])


def test_the_capped_grid_strides_over_4096_tiles():
    n = 24
    g = torch.Generator(device=DEV).manual_seed(9)
    base = torch.randn((2,) * n + (2,), dtype=torch.float32, device=DEV, generator=g)
    view = torch.view_as_complex(base)
    copy = view.clone()
    info = A.channel_info(view.shape, view.stride(), A.bit_flip(0.5), [0])
    assert info["n_tiles"] == 4096 and info["target_bits"] == (23,)
    j, p = A.channel_(view, A.bit_flip(0.5), [0], uniform=0.75)
    assert (j, p) == (1, 0.5)
    A.apply_wide_gate_(copy, CO.PAULIS[1], [0])
    assert torch.equal(torch.view_as_real(view).view(torch.int32), torch.view_as_real(copy).view(torch.int32))
    assert not torch.equal(view[0], view[1])


# ---- the early return -----------------------------------------------------------------------------------------------------------
def poisoned(n, kind, rng):
    """-0.0, denormals, infinities and NaNs with payloads among ordinary values, as the integers of the components."""
    word = KINDS[kind][2]
    real = np.float32 if kind == "c64" else np.float64
    vals = rng.standard_normal(2 * 2 ** n).astype(real).view(word)
    if kind == "c64":
        special = np.array([0x80000000, 0x00000001, 0x807fffff, 0x7f800000, 0xff800000, 0x7fc00123, 0xffa00001, 0x7f800055], dtype=word)
    else:
        special = np.array([0x8000000000000000, 0x0000000000000001, 0x800fffffffffffff, 0x7ff0000000000000, 0xfff0000000000000,
                            0x7ff8000000000123, 0xfff4000000000001, 0x7ff0000000000055], dtype=word)
    where = rng.permutation(vals.size)[:vals.size // 4]
    vals[where] = special[np.arange(where.size) % special.size]
    return vals.view(KINDS[kind][0]).reshape((2,) * n)


@pytest.mark.parametrize("n, kind", [(13, "c64"), (12, "c128")])
def test_the_early_return_leaves_every_bit(n, kind):
    rng = np.random.default_rng(61)
    a = poisoned(n, kind, rng)
    base, view = on_device(a)
    before = ints(base, kind).copy()
    assert (before == a.view(KINDS[kind][2]).reshape(before.shape)).all()
    # a mixture draw that lands on the identity: FIXED, scale exactly 1
    for ch, dims, u in ((A.depolarizing(0.01), [0], 0.5), (A.depolarizing(0.01, 3), [n - 1, 4, 0], 0.98), (A.bit_flip(0.3), [5], 0.0)):
        j, p, total, scale, cur = read(A.channel_step_(view, ch, dims, uniform=u))
        assert j == 0 and scale == 1.0 and (cur == np.eye(2 ** ch.t)).all()
        assert (ints(base, kind) == before).all()
    # a draw that cannot happen: the weights of a poisoned state are not finite
    for ch, dims in ((A.amplitude_damping(0.3), [2]), (A.Channel.from_kraus(rotated_damping()), [n - 1])):
        j, p = A.channel_(view, ch, dims, uniform=0.3, device=True)
        assert (int(j), float(p)) == (-1, 0.0)
        with pytest.raises(ValueError, match="nothing can be drawn"):
            A.channel_(view, ch, dims, uniform=0.3)
        assert (ints(base, kind) == before).all()
    # ... and an all-zero state (the signs of its zeros stay)
    zero = np.zeros((2,) * n, dtype=KINDS[kind][0])
    zero.view(KINDS[kind][2]).reshape(-1)[::3] = 0x80000000 if kind == "c64" else 0x8000000000000000   # -0.0
    zbase, zview = on_device(zero)
    zbefore = ints(zbase, kind).copy()
    for ch, dims in ((A.amplitude_damping(0.3), [1]), (A.Channel.from_kraus(rotated_damping()), [0])):
        rec = A.channel_step_(zview, ch, dims, uniform=0.3)
        j, p, total, scale, cur = read(rec)
        assert (j, p, total, scale) == (-1, 0.0, 0.0, 1.0) and (cur == 0).all()
        j, p = A.channel_(zview, ch, dims, uniform=0.3, device=True)
        assert (int(j), float(p)) == (-1, 0.0)
        with pytest.raises(ValueError, match="nothing can be drawn"):
            A.channel_(zview, ch, dims, uniform=0.3)
        assert (ints(zbase, kind) == zbefore).all()


# ---- renormalisation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, n, tol", [("c64", 14, 1e-6), ("c128", 12, 1e-12)])
def test_renormalisation_keeps_the_squared_norm(kind, n, tol):
    """One rounding per component over at most 2^14 elements: 1e-6 (complex64), 1e-12 (complex128) relative."""
    rng = np.random.default_rng(71)
    a = crand(rng, n, kind)
    for name, dims in (("diag1", [3]), ("diag2", [0, n - 1]), ("dense1", [n - 1]), ("dense3", [2, n - 2, 5])):
        ch = case_channel(name)[0]
        for u in (0.1, 0.8):
            base, view = on_device(a)
            trace = A.norm2(view)
            j, p, total, scale, cur = read(A.channel_step_(view, ch, dims, uniform=u))
            after = A.norm2(view)
            assert scale != 1.0 and abs(after - trace) <= tol * trace, (name, u, after, trace)
            base, view = on_device(a)
            j2, p2, total2, scale2, cur2 = read(A.channel_step_(view, ch, dims, uniform=u, renormalize=False))
            assert j2 == j and scale2 == 1.0 and (cur2 == case_channel(name)[3][j]).all()
            assert abs(A.norm2(view) - p * trace) <= tol * trace   # (K_j itself: the norm becomes w_j)


# ---- no synchronisation, and when() ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("u, flipped", [(0.2, 0), (0.9, 1)])
def test_a_side_stream_and_a_condition_on_the_draw(u, flipped):
    rng = np.random.default_rng(81)
    n, q, r = 13, 2, 9
    a = crand(rng, n, "c64")
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        base, view = on_device(a)
        uniform = torch.full((1,), u, dtype=torch.float64, device=DEV)
        j, p = A.channel_(view, A.bit_flip(0.5), [q], uniform=uniform, device=True)
        assert isinstance(j, torch.Tensor) and j.is_cuda and j.dtype == torch.int64 and j.dim() == 0
        A.mcx_(view, (), r, condition=A.when(j, 1))
    side.synchronize()
    want = np.flip(np.flip(a, axis=q), axis=r) if flipped else a
    assert int(j) == flipped and float(p) == 0.5
    assert (base.cpu().numpy().view(np.uint32) == np.ascontiguousarray(want).view(np.uint32)).all()


# ---- physics --------------------------------------------------------------------------------------------------------------------
def test_the_trajectory_mean_follows_the_density_matrix():
    """6 qubits, 7 gates; after each gate depolarizing(0.05) on its qubits and amplitude_damping(0.1) on qubits 1 and 4.  The mean of
    <Z_q> over N = 1000 trajectories lies within 5 / sqrt(N) of the exact 64 x 64 density-matrix evolution: the observable lies in
    [-1, 1], so its standard error is at most 1 / sqrt(N).  Seeded: deterministic."""
    nq, N = 6, 1000
    ry = lambda th: np.array([[math.cos(th / 2), -math.sin(th / 2)], [math.sin(th / 2), math.cos(th / 2)]], dtype=np.complex128)
    rx = lambda th: np.array([[math.cos(th / 2), -1j * math.sin(th / 2)], [-1j * math.sin(th / 2), math.cos(th / 2)]], dtype=np.complex128)
    cnot = np.eye(4, dtype=np.complex128)[[0, 1, 3, 2]]
    gates = [(H, (0,)), (cnot, (0, 1)), (ry(0.7), (2,)), (cnot, (2, 3)), (rx(1.1), (4,)), (cnot, (4, 5)), (cnot, (1, 2))]
    damped = (1, 4)
    # the exact evolution
    rho = np.zeros((64, 64), dtype=np.complex128)
    rho[0, 0] = 1.0
    dep = CO.kraus_of_mixture(*CO.depolarizing(0.05))
    for m, qs in gates:
        rho = CO.apply_to_rho(rho, [m], list(qs), nq)
        for q in qs:
            rho = CO.apply_to_rho(rho, dep, [q], nq)
        for q in damped:
            rho = CO.apply_to_rho(rho, CO.amplitude_damping(0.1), [q], nq)
    assert abs(np.trace(rho).real - 1) < 1e-12
    diag = np.diag(rho).real.reshape((2,) * nq)
    want = [float(np.tensordot(diag, [1.0, -1.0], axes=([q], [0])).sum()) for q in range(nq)]
    # the trajectories
    shape = (2,) * nq
    psi = torch.zeros(shape, dtype=torch.complex128, device=DEV)
    stride = psi.stride()
    ops = [A.WideGate(shape, stride, psi.dtype, m, qs, DEV) for m, qs in gates]
    depol = {q: A.ChannelOp(shape, stride, psi.dtype, A.depolarizing(0.05), [q], DEV) for q in range(nq)}
    damp = {q: A.ChannelOp(shape, stride, psi.dtype, A.amplitude_damping(0.1), [q], DEV) for q in damped}
    per = sum(len(qs) for _, qs in gates) + len(damped) * len(gates)
    g = torch.Generator(device=DEV).manual_seed(1234)
    uniforms = torch.rand(N * per, dtype=torch.float64, device=DEV, generator=g)
    acc = torch.zeros(shape, dtype=torch.float64, device=DEV)
    start = torch.zeros(shape, dtype=torch.complex128, device=DEV)
    start.view(-1)[0] = 1.0
    i = 0
    for _ in range(N):
        psi.copy_(start)
        for gate, (m, qs) in zip(ops, gates):
            gate(psi)
            for q in qs:
                depol[q](psi, uniform=uniforms[i:i + 1], device=True)
                i += 1
            for q in damped:
                damp[q](psi, uniform=uniforms[i:i + 1], device=True)
                i += 1
        acc += psi.real ** 2 + psi.imag ** 2
    assert i == N * per
    mean = (acc / N).cpu().numpy()
    assert abs(mean.sum() - 1) < 1e-9                          # every trajectory keeps its norm
    got = [float(np.tensordot(mean, [1.0, -1.0], axes=([q], [0])).sum()) for q in range(nq)]
    for q in range(nq):
        print(f"<Z_{q}>: trajectories {got[q]:+.4f}, density matrix {want[q]:+.4f}, bound {5 / math.sqrt(N):.4f}")
    for q in range(nq):
        assert abs(got[q] - want[q]) <= 5 / math.sqrt(N), (q, got[q], want[q])


# ---- equivalence with the host route --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("name, dims", [("diag1", [3]), ("dense1", [11]), ("diag2", [0, 7]), ("dense2", [12, 1])])
def test_the_same_draw_and_state_as_apply_channel(name, dims, kind):
    """Both routes round every component once from a float64 result of matrices that differ in the last bits (apply_channel_
    scales on the host, by 1 / sqrt(p)): each lies within u ||y||_2 of the exact product, so they differ by at most the gate
    bound of tests/test_gates_gpu.py for one gate, 2 u ||a||_2 G (complex64) and 32 u ||a||_2 G (complex128), G = max(1, ||M||_2)."""
    rng = np.random.default_rng(91)
    a = crand(rng, 13, kind)
    ch, form, packed, mats = case_channel(name)
    unit = 2 * 2.0 ** -24 if kind == "c64" else 32 * 2.0 ** -53
    for u in (0.07, 0.5, 0.93):
        base, view = on_device(a)
        j, p, total, scale, cur = read(A.channel_step_(view, ch, dims, uniform=u))
        cbase, cview = on_device(a)
        j2, p2 = A.apply_channel_(cview, ch.kraus, dims, uniform=u)
        assert j2 == j and abs(p2 - p) <= 1e-12 * p
        bound = unit * np.linalg.norm(a.astype(np.complex128).reshape(-1)) * max(1.0, np.linalg.norm(cur, 2))
        err = np.linalg.norm((base.cpu().numpy().astype(np.complex128) - cbase.cpu().numpy().astype(np.complex128)).reshape(-1))
        print(f"{name} {kind} u {u}: j {j} err {err:.3e} bound {bound:.3e}")
        assert err <= bound


# ---- the refusals of the two launching entry points -----------------------------------------------------------------------------
def test_choose_and_apply_refuse_bad_arguments_on_the_device():
    """Every refusal of artn_channel_choose and artn_channel_apply comes before the launch, with its code and text and in the
    order of the gate families: the device pointers are real, the misaligned and short ones are never used."""
    lib = N.lib()
    t = torch.zeros((2,) * 6, dtype=torch.complex64, device=DEV)
    t.view(-1)[0] = 1.0
    op = A.ChannelOp(t.shape, t.stride(), t.dtype, A.amplitude_damping(0.3), [1], DEV)       # DIAGONAL: choose reads `input`
    q = torch.tensor([1.0, 0.0], dtype=torch.float64, device=DEV)
    u = torch.full((2,), 0.5, dtype=torch.float64, device=DEV)
    rec = torch.zeros(op.record_bytes // 8 + 1, dtype=torch.float64, device=DEV)
    tab, nb, rb = op._table.data_ptr(), op.table_bytes, op.record_bytes
    assert nb == 512 + 2 * (16 + 16 + 64) and rb == 32 + 64
    P = ctypes.c_void_p

    def choose(table=tab, nbytes=nb, tt=1, m=2, form=N.CHANNEL_DIAGONAL, inp=q.data_ptr(), uni=u.data_ptr(), record=rec.data_ptr(),
               rbytes=rb):
        return lib.artn_channel_choose(P(table), nbytes, tt, m, form, P(inp), P(uni), 1, P(record), rbytes, None)

    def refused(rc, code, text):
        assert rc == code and text in lib.artn_last_error(), (rc, lib.artn_last_error())

    for tt in (0, 6):
        refused(choose(tt=tt), -2, b"channels act on one to five dimensions, not %d" % tt)
    for m in (0, 257):
        refused(choose(m=m), -1, b"a channel has 1 to 256 operators, not %d" % m)
    refused(choose(form=3), -1, b"unknown weight form 3")
    for null in ("table", "uni", "record", "inp"):
        refused(choose(**{null: 0}), -1, b"null pointer")
    refused(choose(nbytes=nb - 1), -1, b"table smaller than artn_channel_query reports")
    refused(choose(form=N.CHANNEL_DENSE), -1, b"table smaller than artn_channel_query reports")   # (a DENSE table is larger)
    refused(choose(rbytes=rb - 1), -1, b"record smaller than artn_channel_query reports")
    refused(choose(table=tab + 4), -2, b"artn_channel_choose needs an 8-byte aligned table")
    for name, value in (("inp", q.data_ptr() + 4), ("uni", u.data_ptr() + 4), ("record", rec.data_ptr() + 4)):
        refused(choose(**{name: value}), -2, b"artn_channel_choose needs 8-byte aligned arrays")
    # precedence: the counts before the pointers, a null pointer before the sizes, the sizes before the alignment
    refused(choose(tt=9, m=0, table=0), -2, b"one to five")
    refused(choose(m=0, table=0), -1, b"operators")
    refused(choose(table=0, nbytes=0, rbytes=0), -1, b"null pointer")
    refused(choose(nbytes=0, rbytes=0, table=tab + 4), -1, b"table smaller")
    refused(choose(rbytes=0, table=tab + 4), -1, b"record smaller")
    refused(choose(table=tab + 4, record=rec.data_ptr() + 4), -2, b"aligned table")
    # the FIXED form does not read `input`: a null one is accepted (the table is large enough for a FIXED channel of m = 2)
    assert choose(form=N.CHANNEL_FIXED, inp=0) == 0            # (the kernel sees a table of another form and draws nothing)
    assert choose() == 0
    torch.cuda.synchronize()
    assert int(rec.view(torch.int64)[0]) == 0 and float(rec[3]) == 1.0

    dims = np.array([1], dtype=np.int32)

    def apply(a=t.data_ptr(), tt=1, dd=dims, m=2, table=tab, nbytes=nb, record=rec.data_ptr(), rbytes=rb, desc=op._d):
        return lib.artn_channel_apply(ctypes.byref(desc) if desc is not None else None, P(a), tt, _ptr(dd) if dd is not None else None, m,
                                      P(table), nbytes, P(record), rbytes, None)

    refused(apply(desc=None), -1, b"null descriptor")
    refused(apply(dd=None), -1, b"null pointer")
    refused(apply(tt=6, dd=np.arange(6, dtype=np.int32)), -2, b"channels act on one to five dimensions, not 6")
    refused(apply(dd=np.array([6], dtype=np.int32)), -1, b"dimension 6 out of range")
    refused(apply(tt=2, dd=np.array([1, 1], dtype=np.int32)), -1, b"dimension 1 is repeated")
    for m in (0, 257):
        refused(apply(m=m), -1, b"a channel has 1 to 256 operators, not %d" % m)
    for null in ("a", "table", "record"):
        refused(apply(**{null: 0}), -1, b"null pointer")
    need = 512 + 2 * (16 + 8 + 64)                             # the smallest table of any form for t = 1, m = 2
    refused(apply(nbytes=need - 1), -1, b"table smaller than artn_channel_query reports")
    refused(apply(rbytes=rb - 1), -1, b"record smaller than artn_channel_query reports")
    refused(apply(a=t.data_ptr() + 8), -2, b"artn_channel_apply needs a 16-byte aligned array")
    refused(apply(table=tab + 4), -2, b"artn_channel_apply needs an 8-byte aligned table")
    refused(apply(record=rec.data_ptr() + 4), -2, b"artn_channel_apply needs an 8-byte aligned record")
    # precedence: the plan before the pointers, a null pointer before the sizes, the sizes before the alignment, array / table / record
    refused(apply(m=0, a=0), -1, b"operators")
    refused(apply(a=0, nbytes=0), -1, b"null pointer")
    refused(apply(nbytes=0, rbytes=0, a=t.data_ptr() + 8), -1, b"table smaller")
    refused(apply(rbytes=0, a=t.data_ptr() + 8), -1, b"record smaller")
    refused(apply(a=t.data_ptr() + 8, table=tab + 4, record=rec.data_ptr() + 4), -2, b"aligned array")
    refused(apply(table=tab + 4, record=rec.data_ptr() + 4), -2, b"aligned table")
    before = t.clone()
    assert apply(nbytes=need) == 0 and apply() == 0
    torch.cuda.synchronize()
    # dim 1 of |0..0> is in |0>: K_0 = diag(1, sqrt(0.7)) with scale 1 leaves the state as it is
    assert torch.equal(torch.view_as_real(t).view(torch.int32), torch.view_as_real(before).view(torch.int32))
    # the Python layer refuses a misaligned state before the library sees it
    with pytest.raises(ValueError, match="16-byte"):
        A.channel_(torch.zeros(65, dtype=torch.complex64, device=DEV)[1:].view((2,) * 6), A.bit_flip(0.1), [0])
