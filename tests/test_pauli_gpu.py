"""Pauli-string and Hamiltonian expectation values on the device (artensor_amd/pauli.py, artn_pauli_expect) against a numpy oracle
that shares nothing with the mask formula of the kernels: it applies the 2 x 2 matrices axis by axis to the complex128 state
(np.flip for X, a sign multiply for Z, np.tensordot for Y) and takes np.vdot.

Tolerance (derived, the bound of tests/test_born_gpu.py): a float64 sum of n terms in any order is within (n - 1) 2^-53 sum|term|
of the exact value, and by Cauchy-Schwarz sum_i |conj(a[i ^ xm]) a[i]| <= sum |a|^2 = norm2.  The raw values therefore satisfy
|got - want| <= 4 n 2^-53 norm2 (the factor 4 covers the oracle's own sum and the one rounding of each term); normalised values
get the same bound with norm2 = 1 plus one more 4 n 2^-53 for the division."""
import os

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import pauli
from artensor_amd.fixtures import load_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Y2 = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)


def tol(n):
    return 4 * n * 2.0 ** -53


def crand(rng, shape, kind="c64"):
    a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return a.astype(np.complex64 if kind == "c64" else np.complex128)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def letters(p, nd):
    """One string in either notation as a list of nd upper-case letters."""
    if isinstance(p, str):
        return list(p.upper())
    out = ["I"] * nd
    for d, c in p.items():
        out[d] = c.upper()
    return out


def oracle(a_logical, p):
    """(<a|P|a>, <a|a>) of the LOGICAL array, axis by axis in complex128."""
    psi = np.asarray(a_logical).astype(np.complex128)
    phi = psi
    for d, c in enumerate(letters(p, psi.ndim)):
        if c == "X":
            phi = np.flip(phi, axis=d)
        elif c == "Z":
            sign = np.ones(psi.ndim, dtype=int)
            sign[d] = 2
            phi = phi * np.array([1.0, -1.0]).reshape(sign)
        elif c == "Y":
            phi = np.moveaxis(np.tensordot(Y2, phi, axes=([1], [d])), 0, d)
    val = np.vdot(psi, phi)
    norm2 = float(np.vdot(psi, psi).real)
    assert abs(val.imag) <= tol(psi.size) * norm2
    return float(val.real), norm2


def check(t, a_logical, strings, label=""):
    """Raw and normalised values of every string against the oracle, one string per call and all strings in one call."""
    n = a_logical.size
    want = [oracle(a_logical, p) for p in strings]
    norm2 = want[0][1]
    raw = A.pauli_expectation(t, strings, normalize=False)
    nrm = A.pauli_expectation(t, strings)
    assert raw.dtype == np.float64 and raw.shape == (len(strings),)
    for k, p in enumerate(strings):
        w = want[k][0]
        err_raw, err_nrm = abs(raw[k] - w), abs(nrm[k] - w / norm2)
        print(f"{label} {p!r}: want {w:.6e} raw err {err_raw:.3e} (bound {tol(n) * norm2:.3e}) normalised err {err_nrm:.3e} (bound {2 * tol(n):.3e})")
        assert err_raw <= tol(n) * norm2, (label, p)
        assert err_nrm <= 2 * tol(n), (label, p)
        one = A.pauli_expectation(t, p, normalize=False)
        assert isinstance(one, float) and one == raw[k], (label, p)      # the same launch shape: bit for bit
    return raw


def on_bits(nq, ops):
    """String of a contiguous [2]*nq tensor from {memory bit: letter}: dim d is memory bit nq - 1 - d."""
    s = ["I"] * nq
    for b, c in ops.items():
        s[nq - 1 - b] = c
    return "".join(s)


def addressing_strings(nq):
    top = nq - 1
    return [
        on_bits(nq, {0: "Z", 5: "Z", 9: "Z", 10: "Z", top: "Z"}),            # xm = 0
        on_bits(nq, {b: "Z" for b in range(nq)}),
        on_bits(nq, {0: "X"}),                                                # register swap
        on_bits(nq, {0: "X", 1: "Z", 4: "Z", 11: "Z"}),
        on_bits(nq, {1: "X"}),                                                # bit 1 alone
        on_bits(nq, {0: "X", 1: "X"}),
        on_bits(nq, {2: "X", 3: "X", 4: "X", 5: "X", 6: "X", 7: "X"}),        # lanes
        on_bits(nq, {2: "X"}), on_bits(nq, {5: "X", 0: "Z"}), on_bits(nq, {7: "X", 6: "Z"}),
        on_bits(nq, {8: "X", 9: "X"}),                                        # across waves
        on_bits(nq, {8: "X"}), on_bits(nq, {9: "X", 8: "Z"}),
        on_bits(nq, {10: "X"}),                                               # bit 10 alone
        on_bits(nq, {top: "X"}),                                              # the top bit alone
        on_bits(nq, {top: "X", 10: "Z", 3: "Z"}),
        on_bits(nq, {0: "X", 3: "X", 9: "X", 10: "X", top: "X", 6: "Z"}),     # low + high mixed
        on_bits(nq, {1: "X", 11: "X", 0: "Z"}),
        "X" * nq,                                                             # all-X
        on_bits(nq, {4: "Y"}),                                                # ny mod 4 = 1
        on_bits(nq, {4: "Y", 11: "Y"}),                                       # 2
        on_bits(nq, {0: "Y", 4: "Y", 11: "Y", 2: "Z"}),                       # 3
        on_bits(nq, {1: "Y", 2: "Y", 9: "Y", 10: "Y", 7: "X"}),               # 0
        on_bits(nq, {0: "Y", 1: "Y", 2: "Y", 8: "Y", top: "Y"}),              # 5 = 1 mod 4
        "Y" * nq,
        on_bits(nq, {top: "Y", **{b: "Z" for b in range(top)}}),              # Y on the top bit, Z below it
        on_bits(nq, {top: "Y", 10: "Z", 0: "Z"}),
        "I" * nq,                                                             # the identity
    ]


# ---- 1. every addressing form at the smallest sizes where it exists ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [12, 13])
def test_every_addressing_form(nq, kind):
    rng = np.random.default_rng(100 + nq)
    a = crand(rng, (2,) * nq, kind)
    raw = check(gpu(a), a, addressing_strings(nq), f"[2]*{nq} {kind}")
    norm2 = float((np.abs(a.astype(np.complex128)) ** 2).sum())
    assert abs(raw[-1] - norm2) <= tol(a.size) * norm2                       # <I> = the norm


# ---- 2. permuted layouts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_permuted_layouts_are_read_in_place(kind):
    rng = np.random.default_rng(7)
    a = crand(rng, (2,) * 12, kind)
    base = gpu(a)
    for _ in range(3):
        perm = [int(p) for p in rng.permutation(12)]
        t = base.permute(perm)
        assert t.data_ptr() == base.data_ptr() and not t.is_contiguous()
        strings = ["".join(rng.choice(list("IXYZ"), 12)) for _ in range(6)] + ["X" * 12, {0: "Y", -1: "Z"}, {5: "x"}]
        check(t, a.transpose(perm), strings, f"perm {perm}")
        assert t.data_ptr() == base.data_ptr()
    # extent-1 dims and a leading row dimension carrying I
    b = crand(rng, (1, 2, 2, 1) + (2,) * 10 + (1,), kind)
    tb = gpu(b).permute(0, 5, 2, 3, 1, 4, 6, 7, 8, 9, 10, 11, 13, 12, 14)
    bl = b.transpose(0, 5, 2, 3, 1, 4, 6, 7, 8, 9, 10, 11, 13, 12, 14)
    strings = ["I" + "XZ" + "I" + "YIZXIIYZXZ" + "I", "IZZIIIIIIIIIIZI", {1: "X", 13: "Y"}, "I" * 15]
    check(tb, bl, strings, "[1, 2, 2, 1, ...]")
    c = crand(rng, (4, 2, 2, 2, 8, 2, 2, 2, 2), kind)                        # 2^12 elements, two wider dims carrying I
    tc = gpu(c).permute(1, 0, 3, 2, 5, 4, 7, 6, 8)
    check(tc, c.transpose(1, 0, 3, 2, 5, 4, 7, 6, 8), ["XIZYXIIZY", "ZIZIZIZIZ", "YIIIIIIIX", {0: "X"}], "[2, 4, ...]")


# ---- 3. states below one tile -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [1, 2, 5, 9])
def test_small_states(nq, kind):
    rng = np.random.default_rng(30 + nq)
    a = crand(rng, (2,) * nq, kind)
    strings = [{q: c} for q in range(nq) for c in "XYZ"] + ["I" * nq, "Y" * nq, "X" * nq]
    check(gpu(a), a, strings, f"[2]*{nq} {kind}")


# ---- 4. / 6. grid stride and determinism on one [2]*22 state ---------------------------------------------------------------
@pytest.fixture(scope="module")
def state22():
    rng = np.random.default_rng(22)
    a = crand(rng, (2,) * 22)
    strings = ["Z" * 22, on_bits(22, {21: "X"}), on_bits(22, {3: "X"}), "XYZZYXZXZYXZXYYXZXYZXY"]    # the last one: weight 22
    return a, gpu(a), strings, [oracle(a, p) for p in strings]


def test_grid_stride_over_4096_tiles(state22):
    a, t, strings, want = state22
    assert len(strings[3]) == 22 and all(c != "I" for c in strings[3])
    info = A.pauli_info(t.shape, t.stride(), strings)
    assert info["n_groups"] == 4 and a.size // 1024 > 2048
    raw = A.pauli_expectation(t, strings, normalize=False)
    nrm = A.pauli_expectation(t, strings)
    norm2 = want[0][1]
    for k, p in enumerate(strings):
        print(f"[2]*22 {p}: want {want[k][0]:.6e} raw err {abs(raw[k] - want[k][0]):.3e} (bound {tol(a.size) * norm2:.3e})")
        assert abs(raw[k] - want[k][0]) <= tol(a.size) * norm2
        assert abs(nrm[k] - want[k][0] / norm2) <= 2 * tol(a.size)


def test_two_calls_are_bit_identical(state22):
    _, t, strings, _ = state22
    for p in strings + [strings]:
        assert torch.equal(A.pauli_expectation(t, p, device=True), A.pauli_expectation(t, p, device=True))
        assert torch.equal(A.pauli_expectation(t, p, normalize=False, device=True), A.pauli_expectation(t, p, normalize=False, device=True))


# ---- 5. batching ------------------------------------------------------------------------------------------------------------
def test_batching_within_and_across_groups():
    rng = np.random.default_rng(5)
    a = crand(rng, (2,) * 13)
    t = gpu(a)
    T = A.pauli_info(t.shape, t.stride(), "Z" * 13)["terms_per_launch"]
    zs = ["".join(rng.choice(["I", "Z"], 13)) for _ in range(2 * T + 3)]
    info = A.pauli_info(t.shape, t.stride(), zs)
    assert info["n_groups"] == 1 and info["n_launches"] == 3
    norm2 = oracle(a, "I" * 13)[1]
    raw = A.pauli_expectation(t, zs, normalize=False)
    for k, p in enumerate(zs):
        assert abs(raw[k] - oracle(a, p)[0]) <= tol(a.size) * norm2, (k, p)
    # four xm interleaved in the input order: outputs in input order, equal to the one-at-a-time results bit for bit
    xparts = [on_bits(13, {}), on_bits(13, {2: "X", 6: "X"}), on_bits(13, {12: "X", 0: "X"}), on_bits(13, {10: "X"})]
    mixed = []
    for i in range(5):
        for xp in xparts:
            s = list(xp)
            for d in range(13):
                if s[d] == "I" and rng.random() < 0.4:
                    s[d] = "Z"
                elif s[d] == "X" and rng.random() < 0.4:
                    s[d] = "Y"
            mixed.append("".join(s))
    info = A.pauli_info(t.shape, t.stride(), mixed)
    assert info["n_groups"] == 4 and info["group"] == [0, 1, 2, 3] * 5
    got = A.pauli_expectation(t, mixed, normalize=False, device=True)
    for k, p in enumerate(mixed):
        assert abs(float(got[k]) - oracle(a, p)[0]) <= tol(a.size) * norm2, (k, p)
        assert torch.equal(got[k], A.pauli_expectation(t, p, normalize=False, device=True)), (k, p)
    # a Hamiltonian with complex coefficients, one call
    coeffs = rng.standard_normal(len(mixed)) + 1j * rng.standard_normal(len(mixed))
    terms = list(zip(coeffs, mixed))
    want = sum(c * oracle(a, p)[0] for c, p in terms) / norm2
    got_sum = A.pauli_sum_expectation(t, terms)
    assert isinstance(got_sum, complex)
    assert abs(got_sum - want) <= 2 * tol(a.size) * np.abs(coeffs).sum()
    real = A.pauli_sum_expectation(t, [(c.real, p) for c, p in terms], normalize=False)
    assert isinstance(real, float)
    assert abs(real - sum(c.real * oracle(a, p)[0] for c, p in terms)) <= tol(a.size) * norm2 * np.abs(coeffs.real).sum()


# ---- 7. consistency with the layers already there ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_consistency_with_marginals_rdm_and_norm(kind):
    rng = np.random.default_rng(77)
    a = crand(rng, (2,) * 14, kind)
    t = gpu(a).permute([int(p) for p in rng.permutation(14)])
    norm2 = A.norm2(t)
    P = {"X": np.array([[0, 1], [1, 0]], dtype=np.complex128), "Y": Y2, "Z": np.diag([1.0, -1.0]).astype(np.complex128)}
    for q in range(14):
        p01 = A.marginal_probabilities(t, [q]).cpu().numpy()
        assert abs(A.pauli_expectation(t, {q: "Z"}, normalize=False) - (p01[0] - p01[1])) <= 1e-12 * norm2
    for (la, lb), (qa, qb) in ((("X", "Z"), (3, 11)), (("Y", "Y"), (0, 13)), (("X", "Z"), (12, 1)), (("Y", "Y"), (6, 5))):
        via_rdm = A.expectation(t, np.kron(P[la], P[lb]), [qa, qb])
        got = A.pauli_expectation(t, {qa: la, qb: lb})
        assert abs(got - via_rdm.real) <= 1e-12 and abs(via_rdm.imag) <= 1e-12     # (both normalised: norm2 = 1)
    ops, _ = pauli.pauli_ops(["Z" * 14, {2: "X"}], 14)
    out = pauli._raw(t, ops, "test")
    assert out.shape == (3,) and abs(float(out[2]) - norm2) <= 1e-12 * norm2


# ---- 8. a real state --------------------------------------------------------------------------------------------------------
def test_n12_contraction_feeds_ten_strings():
    case = load_case(os.path.join(GOLDEN, "n12_dense.npz"))
    raw = A.tensor_contraction(case.fresh_tensors(device=DEV), case.scheme)
    ptr = raw.data_ptr()
    gold = case.arrays["raw"].reshape(raw.shape)
    rng = np.random.default_rng(12)
    two = [d for d, e in enumerate(raw.shape) if e == 2]
    assert len(two) == 12
    strings = []
    for k in range(10):
        s = ["I"] * raw.dim()
        for d in two:
            s[d] = str(rng.choice(list("IXYZ")))
        strings.append("".join(s))
    strings[0] = "".join("Z" if d in two else "I" for d in range(raw.dim()))
    strings[1] = "".join("X" if d in two else "I" for d in range(raw.dim()))
    got = A.pauli_expectation(raw, strings, normalize=False)
    assert raw.data_ptr() == ptr
    norm2 = oracle(gold, strings[0])[1]
    for k, p in enumerate(strings):
        # (the contraction itself is complex64: the amplitudes agree with the fixture's to float32 accuracy)
        assert abs(got[k] - oracle(gold, p)[0]) <= 1e-5 * norm2, (k, p)
    check(raw, raw.cpu().numpy(), strings, "n12")


# ---- 9. device=True ---------------------------------------------------------------------------------------------------------
def test_device_results_equal_the_host_values():
    rng = np.random.default_rng(9)
    a = crand(rng, (2,) * 12)
    t = gpu(a)
    strings = ["Z" * 12, on_bits(12, {11: "Y", 0: "Z"}), on_bits(12, {3: "X"})]
    for normalize in (True, False):
        dev = A.pauli_expectation(t, strings, normalize=normalize, device=True)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float64 and dev.shape == (3,)
        host = A.pauli_expectation(t, strings, normalize=normalize)
        assert (dev.cpu().numpy() == host).all()
        one = A.pauli_expectation(t, strings[1], normalize=normalize, device=True)
        assert one.is_cuda and one.dtype == torch.float64 and one.dim() == 0
        assert float(one) == A.pauli_expectation(t, strings[1], normalize=normalize) == host[1]


def test_argument_checks_on_gpu_tensors():
    t = gpu(np.zeros((2,) * 4, dtype=np.complex64))
    with pytest.raises(ValueError, match="length"):
        A.pauli_expectation(t, "ZZZ")
    with pytest.raises(ValueError, match="dense"):
        A.pauli_expectation(t[:, :, ::2], "ZZII")
    with pytest.raises(TypeError, match="complex"):
        A.pauli_expectation(t.real.contiguous(), "ZZII")
    with pytest.raises(RuntimeError, match="extent"):
        A.pauli_expectation(gpu(np.zeros((2, 4), dtype=np.complex64)), "ZZ")
    assert N.has("artn_pauli_expect")
