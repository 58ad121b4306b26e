"""In-place Pauli circuits on the device (artensor_amd/pauli.py: pauli_evolve_, pauli_rotate_, pauli_apply_, PauliCircuit;
artn_pauli_evolve) against references that share nothing with the mask formula of the kernels: the dense complex128 matrices of
the steps (np.kron of the 2 x 2 matrices), the axis-by-axis oracle of tests/test_pauli_apply_gpu.py, numpy flips.

Tolerance (derived, not measured).  A step a <- alpha a + beta P a is formed in float64 and rounded ONCE per component to the
dtype: a relative error of at most u = 2^-24 (complex64) or 2^-53 (complex128) per component, so ||error of step k|| <= u ||state
after step k||; the float64 products and sums of a complex128 step add a few u more, which the factor 4 there covers.  The state
grows by at most g_k = max(1, |alpha_k| + |beta_k|) per step (P is unitary), later steps amplify an earlier error by at most the
same factors, and the error norms add linearly over the K steps.  With G = prod g_k and a factor 2 on top:
    complex64:   ||y - ref||_2 <= 2 K 2^-24 ||a||_2 G
    complex128:  ||y - ref||_2 <= 4 K 2^-53 ||a||_2 G
A step with (alpha, beta) = (1, 0) or (0, 1) is exact and is compared bit for bit, as is everything that only changes where the
host cuts the circuit into runs."""
import functools
import os

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd.fixtures import load_case
from test_pauli_apply_gpu import DEV, GOLDEN, KINDS, P2, crand, gpu, ising, letters, on_bits, oracle_string

pytestmark = pytest.mark.gpu


def step_pair(step):
    if len(step) == 2:
        return complex(np.cos(step[0])), -1j * complex(np.sin(step[0]))
    return complex(step[0]), complex(step[1])


def growth(steps):
    return float(np.prod([max(1.0, abs(step_pair(s)[0]) + abs(step_pair(s)[1])) for s in steps]))


def check(got, want, a, steps, kind, label="", K=None):
    """The 2-norm bound of the module docstring; prints the measured error next to it."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    K = len(steps) if K is None else K
    unit = 2 * 2.0 ** -24 if kind == "c64" else 4 * 2.0 ** -53
    bound = unit * K * np.linalg.norm(np.asarray(a).astype(np.complex128).reshape(-1)) * growth(steps)
    err = np.linalg.norm((got.astype(np.complex128) - want).reshape(-1))
    print(f"{label}: K {K} G {growth(steps):.3e} err {err:.3e} bound {bound:.3e} ratio {err / bound:.3f}")
    assert np.isfinite(err) and err <= bound, label


def oracle_circuit(a_logical, steps):
    """The circuit on the LOGICAL array, axis by axis in complex128."""
    psi = np.asarray(a_logical).astype(np.complex128)
    for step in steps:
        alpha, beta = step_pair(step)
        psi = alpha * psi + beta * oracle_string(psi, step[-1])
    return psi


def random_steps(rng, nq, count, letters_of="IXYZ"):
    steps = []
    for k in range(count):
        s = "".join(rng.choice(list(letters_of), nq))
        kind = k % 3
        if kind == 0:
            steps.append((float(rng.uniform(-2, 2)), s))
        elif kind == 1:
            steps.append((0.0, 1.0, s))
        else:
            steps.append((complex(*rng.standard_normal(2)) * 0.6, complex(*rng.standard_normal(2)) * 0.6, s))
    return steps


def dense_string(p, nq):
    """The dense 2^nq x 2^nq matrix of a string: np.kron of its 2 x 2 matrices, the first dim the first factor (the two halves
    are built first, so that there is one large np.kron and not nq growing ones)."""
    def chain(ls):
        m = np.ones((1, 1), dtype=np.complex128)
        for letter in ls:
            m = np.kron(m, P2[letter])
        return m
    ls = letters(p, nq)
    return np.kron(chain(ls[:nq // 2]), chain(ls[nq // 2:]))


def bits_of(t):
    """The bytes of a tensor's storage order as integers (bitwise comparisons; -0.0 differs from 0.0, NaN equals itself)."""
    return torch.view_as_real(t).contiguous().view(torch.int32 if t.dtype == torch.complex64 else torch.int64)


# ---- 1. the dense matrices of the steps ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(nq):
    """24 random steps, the input in both dtypes and the dense-matrix result for each: U_k = alpha_k 1 + beta_k P_k with P_k the
    np.kron of its 2 x 2 matrices (dim 0 of a contiguous [2]*nq tensor is the first factor), applied to both inputs at once."""
    rng = np.random.default_rng(500 + nq)
    steps = random_steps(rng, nq, 24)
    a128 = crand(rng, (2,) * nq, "c128")
    inputs = {"c64": a128.astype(np.complex64), "c128": a128}
    v = np.stack([inputs["c64"].astype(np.complex128).reshape(-1), a128.reshape(-1)], axis=1)
    for step in steps:
        alpha, beta = step_pair(step)
        v = alpha * v + beta * (dense_string(step[-1], nq) @ v)
    return steps, inputs, {"c64": v[:, 0].reshape((2,) * nq), "c128": v[:, 1].reshape((2,) * nq)}


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [9, 10, 11, 12])
def test_against_the_dense_matrices(nq, kind):
    steps, inputs, want = dense_case(nq)
    assert len(steps) == 24 and {len(s) for s in steps} == {2, 3}
    t = gpu(inputs[kind])
    ptr = t.data_ptr()
    assert A.pauli_evolve_(t, steps) is t and t.data_ptr() == ptr
    check(t, want[kind], inputs[kind], steps, kind, f"dense {nq} qubits {kind}")


# ---- 2. every addressing form -------------------------------------------------------------------------------------------------
def addressing_circuits(nq):
    top = nq - 1
    th = [0.37, -1.9, 0.5]
    one = [
        {0: "X"}, {1: "Y"}, {0: "X", 1: "X", 11: "Z"},                        # bits 0-1 only: registers
        {2: "X"}, {5: "Y", 0: "Z"}, {2: "X", 7: "X", 9: "Y"},                 # piece bits only
        {10: "X"}, {11: "Y", 3: "Z"},                                         # one high bit
        {top: "X"}, {top: "Y", 10: "Z", 0: "Z"},                              # the slowest bit
        {0: "X", 3: "X", 9: "X", 10: "X", top: "X", 6: "Z"},                  # high and low together
        {1: "Y", 11: "X", 0: "Z"},
        {b: "Z" for b in range(nq)}, {},                                      # diagonal, the identity
        {b: "Y" for b in range(nq)},
    ]
    circuits = [[(th[k % 3], on_bits(nq, p))] for k, p in enumerate(one)]
    circuits += [[(0.3 - 0.2j, 0.4 + 0.9j, on_bits(nq, p))] for p in one[::3]]
    pairs = [
        ({10: "X", 2: "X"}, {11: "Y"}),                                       # two steps of rank 2 sharing a run
        ({10: "X", 11: "X"}, {11: "X", 0: "Y"}),                              # (a basis that is reduced: {10}, {11})
        ({top: "X"}, {top: "X", 10: "Y", 5: "Z"}),
        ({0: "X"}, {top: "Y", 1: "X"}),                                       # a register step, then a staged one
        ({10: "Z", 3: "X"}, {3: "X", 10: "Z"}),                               # two staged steps inside the tile
    ]
    circuits += [[(th[0], on_bits(nq, p)), (0.8, 0.6j, on_bits(nq, q))] for p, q in pairs]
    return circuits


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [12, 13])
def test_every_addressing_form(nq, kind):
    rng = np.random.default_rng(100 + nq)
    a = crand(rng, (2,) * nq, kind)
    base = gpu(a)
    for steps in addressing_circuits(nq):
        t = base.clone()
        A.pauli_evolve_(t, steps)
        check(t, oracle_circuit(a, steps), a, steps, kind, f"[2]*{nq} {kind} {[s[-1] for s in steps]}")
    info = A.pauli_evolve_info(base.shape, base.stride(), addressing_circuits(nq)[-5], base.dtype)
    assert info["n_runs"] == 1 and info["run_rank"] == [2]
    assert info["max_rank"] == min(3 if kind == "c64" else 2, nq - 10)        # (the default, capped by the number of tiles)


def test_two_blocks_of_eight_tiles_and_the_pivot_insertion():
    nq = 14
    rng = np.random.default_rng(14)
    a = crand(rng, (2,) * nq)
    base = gpu(a)
    # high masks {10, 11}, {11, 12}, {10}: pivots 10, 11, 12, bit 13 numbers the two blocks;
    # high masks {13, 10}, {13, 11}, {12}: pivots 11, 12, 13, bit 10 -- BELOW every pivot -- numbers them
    for masks, pivots in (([(10, 11), (11, 12), (10,)], [10, 11, 12]), ([(13, 10), (13, 11), (12,)], [11, 12, 13])):
        steps = [(0.41, on_bits(nq, {masks[0][0]: "X", masks[0][1]: "Y", 4: "X"})),
                 (0.2 + 0.1j, 0.7j, on_bits(nq, {masks[1][0]: "Y", masks[1][1]: "X", 13: "Z"})),
                 (-0.77, on_bits(nq, {masks[2][0]: "X", 0: "Y", 12: "Z"})), (1.3, on_bits(nq, {b: "Z" for b in (1, 10, 13)})),
                 (0.9, on_bits(nq, {masks[0][0]: "X", masks[0][1]: "X", masks[2][0]: "Y"}))]
        info = A.pauli_evolve_info(base.shape, base.stride(), steps, max_rank=3)
        assert info["n_runs"] == 1 and info["run_rank"] == [3] and info["run_pivot"] == [pivots]
        t = base.clone()
        A.pauli_evolve_(t, steps, max_rank=3)
        check(t, oracle_circuit(a, steps), a, steps, "c64", f"[2]*14 pivots {pivots}")


# ---- 3. the result does not depend on where the runs are cut ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_cut_independence_bit_for_bit(kind):
    nq = 14
    rng = np.random.default_rng(33)
    a = crand(rng, (2,) * nq, kind)
    perm = [int(p) for p in rng.permutation(nq)]
    steps = random_steps(rng, nq, 40)
    base = gpu(a)

    def run(fn):
        store = base.clone()
        t = store.permute(perm)
        assert not t.is_contiguous() and fn(t) is t
        return bits_of(store)

    ranks = [0, 1, 2, 3] + ([4] if kind == "c64" else [])
    infos = {r: A.pauli_evolve_info(base.permute(perm).shape, base.permute(perm).stride(), steps, base.dtype, r) for r in ranks}
    assert len({infos[r]["n_runs"] for r in ranks}) >= 3 and infos[0]["n_runs"] > infos[ranks[-1]]["n_runs"]
    unfused = base.clone()
    A.pauli_evolve_(unfused.permute(perm), steps, max_rank=0)                 # the unfused form
    check(unfused.permute(perm), oracle_circuit(a.transpose(perm), steps), a, steps, kind, f"40 steps permuted {kind}")
    ref = bits_of(unfused)
    for r in ranks:
        assert torch.equal(run(lambda t: A.pauli_evolve_(t, steps, max_rank=r)), ref), r
    assert torch.equal(run(lambda t: A.pauli_evolve_(t, steps)), ref)
    t0 = base.permute(perm)
    circ = A.PauliCircuit(t0.shape, t0.stride(), t0.dtype, steps, DEV)
    assert circ.n_steps == 40 and circ.n_runs == infos[3 if kind == "c64" else 2]["n_runs"]
    assert torch.equal(run(circ), ref) and torch.equal(run(circ), ref)       # two calls in a row
    one_by_one = base.clone()
    for step in steps:                                                        # one call per step
        A.pauli_evolve_(one_by_one.permute(perm), [step])
    assert torch.equal(bits_of(one_by_one), ref)


# ---- 4. exactness -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_exact_steps(kind):
    nq = 13
    rng = np.random.default_rng(44)
    a = crand(rng, (2,) * nq, kind)
    a.reshape(-1)[:4] = [0.0, -0.0, complex(-0.0, 1.0), complex(2.0, -0.0)]   # signed zeros stay what they are
    base = gpu(a)
    strings = [on_bits(nq, {1: "Y", 2: "Y", 9: "Y", 10: "Y", 7: "X"}), on_bits(nq, {4: "Y", 12: "Z"}), on_bits(nq, {4: "Y", 11: "Y"}),
               on_bits(nq, {0: "Y", 4: "Y", 11: "Y", 2: "Z"}), on_bits(nq, {12: "X"}), on_bits(nq, {0: "Z", 12: "Z"}), "X" * nq]
    t = base.clone()
    A.pauli_evolve_(t, [(1.0, 0.0, p) for p in strings] + [(0.0, p) for p in strings])     # (1, 0) and theta = 0
    assert torch.equal(bits_of(t), bits_of(base))
    for p in strings:
        t = base.clone()
        assert A.pauli_rotate_(t, p, 0.0) is t and torch.equal(bits_of(t), bits_of(base)), p
        assert A.pauli_apply_(t, p) is t
        assert torch.equal(t, A.pauli_apply(base, p)), p                      # the out-of-place kernel, by value
        want = oracle_string(a, p)
        assert (t.cpu().numpy().astype(np.complex128) == want).all(), p
        A.pauli_apply_(t, p)
        assert torch.equal(bits_of(t), bits_of(base)), p                      # P^2 = 1, bit for bit
    t = base.clone()
    A.pauli_evolve_(t, [(0.0, 1.0, p) for p in strings] + [(0.0, 1.0, p) for p in strings[::-1]])
    assert torch.equal(bits_of(t), bits_of(base))


# ---- 5. rotations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_rotate_in_place_against_out_of_place(kind):
    nq = 13
    rng = np.random.default_rng(55)
    a = crand(rng, (2,) * nq, kind)
    base = gpu(a)
    for p, theta in ((on_bits(nq, {4: "Y", 12: "Z"}), 0.37), (on_bits(nq, {1: "Y", 2: "Y", 9: "Y", 10: "Y", 7: "X"}), -1.9),
                     ("X" * nq, 0.5), (on_bits(nq, {12: "X"}), 2.2), (on_bits(nq, {3: "Z"}), 0.9), ({}, 0.81)):
        want = A.pauli_rotate(base, p, theta)
        t = base.clone()
        assert A.pauli_rotate_(t, p, theta) is t
        check(t, want.cpu().numpy().astype(np.complex128), a, [(theta, p)], kind, f"rotate {p} {theta}", K=2)


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_the_norm_after_thirty_rotations(kind):
    nq = 13
    rng = np.random.default_rng(66)
    a = crand(rng, (2,) * nq, kind)
    t = gpu(a)
    steps = [(float(rng.uniform(-3, 3)), "".join(rng.choice(list("IXYZ"), nq))) for _ in range(30)]
    before = A.norm2(t)
    A.pauli_evolve_(t, steps)
    after = A.norm2(t)
    # | ||y|| - ||a|| | <= ||y - ref|| <= e ||a|| with e the bound of the module docstring (G = 1), so the SQUARED norm moves by
    # at most 2 e + e^2, relative; plus the error of the two float64 sums themselves, (n - 1) 2^-53 each (tests/test_born_gpu.py)
    e = (2 * 2.0 ** -24 if kind == "c64" else 4 * 2.0 ** -53) * 30
    bound = 2 * e + e * e + 2 * a.size * 2.0 ** -53
    print(f"{kind}: norm2 {before:.12e} -> {after:.12e}, relative change {abs(after - before) / before:.3e} (bound {bound:.3e})")
    assert abs(after - before) <= bound * before


# ---- 6. layouts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_layouts(kind):
    rng = np.random.default_rng(7)
    a = crand(rng, (2,) * 12, kind)
    for _ in range(2):
        perm = [int(p) for p in rng.permutation(12)]
        store = gpu(a)
        t = store.permute(perm)
        assert t.data_ptr() == store.data_ptr() and not t.is_contiguous()
        steps = random_steps(rng, 12, 6) + [(0.3, "X" * 12), (0.5, 0.5, {0: "Y", -1: "Z"}), (-0.4, {5: "x"})]
        assert A.pauli_evolve_(t, steps) is t and t.stride() == store.permute(perm).stride()
        check(t, oracle_circuit(a.transpose(perm), steps), a, steps, kind, f"perm {perm}")
    # extent-1 dims and a permutation
    b = crand(rng, (1, 2, 2, 1) + (2,) * 10 + (1,), kind)
    pb = (0, 5, 2, 3, 1, 4, 6, 7, 8, 9, 10, 11, 13, 12, 14)
    steps = [(0.7, "I" + "XZ" + "I" + "YIZXIIYZXZ" + "I"), (0.2, 0.9j, "IZZIIIIIIIIIIZI"), (-1.1, {1: "X", 13: "Y"}), (0.4, "I" * 15)]
    t = gpu(b).permute(pb)
    A.pauli_evolve_(t, steps)
    check(t, oracle_circuit(b.transpose(pb), steps), b, steps, kind, "[1, 2, 2, 1, ...]")
    # an extent-4 and an extent-8 dim carrying I
    c = crand(rng, (4, 2, 2, 2, 8, 2, 2, 2, 2), kind)
    pc = (1, 0, 3, 2, 5, 4, 7, 6, 8)
    steps = [(0.6, "XIZYXIIZY"), (1.0, 0.25, "ZIZIZIZIZ"), (-0.3, "YIIIIIIIX"), (0.0, 1.0, {0: "X"})]
    t = gpu(c).permute(pc)
    A.pauli_evolve_(t, steps)
    check(t, oracle_circuit(c.transpose(pc), steps), c, steps, kind, "[2, 4, ...]")


# ---- 7. states below one tile -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [1, 2, 5, 9])
def test_small_states(nq, kind):
    rng = np.random.default_rng(30 + nq)
    a = crand(rng, (2,) * nq, kind)
    base = gpu(a)
    for q in range(nq):
        for c in "XYZ":
            t = base.clone()
            A.pauli_apply_(t, {q: c})
            assert (t.cpu().numpy().astype(np.complex128) == oracle_string(a, {q: c})).all(), (q, c)
    steps = random_steps(rng, nq, 12) + [(0.3, {0: "X"}), (0.2, 0.5j, {nq - 1: "Y"}), (1.1, "Z" * nq), (-0.6, "Y" * nq), (0.9, "I" * nq)]
    info = A.pauli_evolve_info(base.shape, base.stride(), steps, base.dtype)
    assert info["n_runs"] == 1 and info["run_rank"] == [0] and info["max_rank"] == 0
    t = base.clone()
    A.pauli_evolve_(t, steps)
    check(t, oracle_circuit(a, steps), a, steps, kind, f"[2]*{nq} {kind} {len(steps)} steps")


# ---- 8. more blocks than workgroups -------------------------------------------------------------------------------------------
def test_grid_stride_over_4096_tiles():
    nq = 22
    rng = np.random.default_rng(22)
    a = crand(rng, (2,) * nq)
    base = gpu(a)
    assert a.size // 1024 == 4096 > 2048                                       # (2048: the grid cap of the Pauli kernels)
    flat = a.astype(np.complex128).reshape(2, 2 ** 11, 2 ** 7, 2, 4)          # memory bits 21 | 20..10 | 9..3 | 2 | 1..0
    th, ph = 0.6, -1.3
    sign2 = np.array([1.0, -1.0]).reshape(1, 1, 1, 2, 1)
    # tile-local steps alone: one run of rank 0, 4096 blocks on 2048 workgroups
    local = [(th, on_bits(nq, {2: "X"})), (ph, on_bits(nq, {2: "Z"}))]
    info = A.pauli_evolve_info(base.shape, base.stride(), local)
    assert info["n_runs"] == 1 and info["run_rank"] == [0]
    want = np.cos(th) * flat - 1j * np.sin(th) * np.flip(flat, axis=3)
    want = np.cos(ph) * want - 1j * np.sin(ph) * sign2 * want
    t = base.clone()
    A.pauli_evolve_(t, local)
    check(t, want.reshape(a.shape), a, local, "c64", "2^22, bit 2")
    # a rotation on the slowest bit, unfused (2048 blocks of two tiles) and in a run with the steps above (512 blocks of eight)
    slow = local + [(th, on_bits(nq, {21: "X"})), (ph, on_bits(nq, {21: "X", 20: "X", 2: "Z"})), (ph, on_bits(nq, {19: "X"}))]
    want = np.cos(th) * want - 1j * np.sin(th) * np.flip(want, axis=0)
    w5 = want.reshape(2, 2, 2 ** 10, 2 ** 7, 2, 4)
    w5 = np.cos(ph) * w5 - 1j * np.sin(ph) * sign2.reshape(1, 1, 1, 1, 2, 1) * np.flip(w5, axis=(0, 1))
    w6 = w5.reshape(2, 2, 2, 2 ** 9, 2 ** 10)
    w6 = np.cos(ph) * w6 - 1j * np.sin(ph) * np.flip(w6, axis=2)
    for max_rank, runs in ((0, 3), (None, 1)):
        assert A.pauli_evolve_info(base.shape, base.stride(), slow, max_rank=max_rank)["n_runs"] == runs
        t = base.clone()
        A.pauli_evolve_(t, slow, max_rank=max_rank)
        check(t, w6.reshape(a.shape), a, slow, "c64", f"2^22, the slowest bit, max_rank {max_rank}")


# ---- 9. a real state ----------------------------------------------------------------------------------------------------------
def test_n12_contraction_output_takes_a_trotter_step():
    case = load_case(os.path.join(GOLDEN, "n12_dense.npz"))
    raw = A.tensor_contraction(case.fresh_tensors(device=DEV), case.scheme)
    two = [d for d, e in enumerate(raw.shape) if e == 2]
    assert len(two) == 12 and raw.numel() == 2 ** 12
    steps = A.trotter_steps(ising(two), 0.05)
    assert len(steps) == 23
    a = raw.cpu().numpy()
    ptr, strides = raw.data_ptr(), raw.stride()
    assert A.pauli_evolve_(raw, steps) is raw and raw.data_ptr() == ptr and raw.stride() == strides
    # the dense matrices on the twelve extent-2 dims, in their logical order
    v = a.astype(np.complex128).reshape(-1)
    for theta, p in steps:
        m = dense_string("".join(p.get(d, "I") for d in two), 12)
        v = np.cos(theta) * v - 1j * np.sin(theta) * (m @ v)
    check(raw, v.reshape(a.shape), a, steps, "c64", "n12 Trotter step")


# ---- 10. argument checks ------------------------------------------------------------------------------------------------------
def test_argument_checks():
    t = gpu(np.zeros((2,) * 4, dtype=np.complex64))
    steps = [(0.3, "ZZII"), (0.5, 0.5, "XIIY")]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.pauli_evolve_(t.cpu(), steps)
    with pytest.raises(TypeError, match="complex"):
        A.pauli_rotate_(t.real.contiguous(), "ZZII", 0.1)
    with pytest.raises(ValueError, match="dense"):
        A.pauli_apply_(t[:, :, ::2], "ZZII")
    odd = torch.zeros(17, dtype=torch.complex64, device=DEV)[1:].view((2,) * 4)
    with pytest.raises(ValueError, match="16-byte"):
        A.pauli_evolve_(odd, steps)
    with pytest.raises(ValueError, match="at least one"):
        A.pauli_evolve_(t, [])
    with pytest.raises(ValueError, match="length"):
        A.pauli_rotate_(t, "ZZZ", 0.1)
    with pytest.raises(RuntimeError, match="max_rank"):
        A.pauli_evolve_(t, steps, max_rank=5)
    circ = A.PauliCircuit(t.shape, t.stride(), t.dtype, steps, t.device)
    assert circ(t) is t
    with pytest.raises(ValueError, match="built for"):
        circ(t.permute(3, 2, 1, 0))
    with pytest.raises(ValueError, match="built for"):
        circ(t.to(torch.complex128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        circ(t.cpu())
    circ._table = circ._table.cpu()                                           # (stands in for a second device)
    with pytest.raises(ValueError, match="built for cpu"):
        circ(t)
