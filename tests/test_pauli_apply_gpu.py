"""y = H a on the device (artensor_amd/pauli.py: pauli_apply, pauli_sum_apply, pauli_rotate, pauli_sum_variance, PauliSumOperator;
artn_pauli_apply) against two numpy oracles that share nothing with the mask formula of the kernel:

  (A) the 2 x 2 matrices applied axis by axis to the complex128 copy of the LOGICAL array (np.flip for X, a sign multiply for Z,
      np.tensordot with the Y matrix), summed over the terms;
  (B) up to 11 qubits, the dense 2^n x 2^n matrix of H from np.kron.

Tolerance (derived).  K terms, C = sum |c_k|, M = max |a|: every output is a float64 sum of at most K products of size at most
|c_k| M, each product and the weight sums carry a few roundings, and the oracle has its own:
    complex128:  |got - want| <= 8 K 2^-53 C M                     per element
    complex64:   the same + 2^-24 |want|                           (one rounding of each component to float32)
A lone string with coefficient 1 is a permutation times 1, -1, i or -i: exact, compared with ==."""
import functools
import os

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd.fixtures import load_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Y2 = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
P2 = {"I": np.eye(2, dtype=np.complex128), "X": np.array([[0, 1], [1, 0]], dtype=np.complex128), "Y": Y2,
      "Z": np.diag([1.0, -1.0]).astype(np.complex128)}
KINDS = {"c64": (np.complex64, torch.complex64), "c128": (np.complex128, torch.complex128)}


def crand(rng, shape, kind="c64"):
    a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return a.astype(KINDS[kind][0])


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def letters(p, nd):
    if isinstance(p, str):
        return list(p.upper())
    out = ["I"] * nd
    for d, c in p.items():
        out[d] = c.upper()
    return out


def oracle_string(a_logical, p):
    """(A) P a of the LOGICAL array, axis by axis in complex128."""
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
    return phi


def oracle_sum(a_logical, terms):
    out = np.zeros(np.shape(a_logical), dtype=np.complex128)
    for c, p in terms:
        out = out + complex(c) * oracle_string(a_logical, p)
    return out


def dense_matrix(nq, terms):
    """(B) H as a dense matrix; dim 0 of a contiguous [2]*nq tensor is the first kron factor."""
    h = np.zeros((2 ** nq, 2 ** nq), dtype=np.complex128)
    for c, p in terms:
        m = np.ones((1, 1), dtype=np.complex128)
        for letter in letters(p, nq):
            m = np.kron(m, P2[letter])
        h += complex(c) * m
    return h


def check(got, want, a_logical, terms, kind, label=""):
    """Per-element bound of the module docstring; prints the measured error next to it."""
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    K, C, M = len(terms), sum(abs(complex(c)) for c, _ in terms), float(np.abs(a_logical).max())
    bound = 8 * K * 2.0 ** -53 * C * M + (2.0 ** -24 * np.abs(want) if kind == "c64" else 0.0)
    err = np.abs(got.astype(np.complex128) - want)
    print(f"{label}: K {K} C {C:.3e} M {M:.3e} max err {err.max():.3e}, worst err / bound {(err / bound).max():.3f} "
          f"(bound at that element {np.broadcast_to(bound, err.shape).reshape(-1)[(err / bound).argmax()]:.3e})")
    assert (err <= bound).all(), label


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


def ising(dims, j=-1.0, h=-0.7):
    """Transverse-field Ising sum on the listed dims: len - 1 ZZ bonds and len X fields."""
    return [(j, {a: "Z", b: "Z"}) for a, b in zip(dims[:-1], dims[1:])] + [(h, {d: "X"}) for d in dims]


def xmask_of(string):
    """Memory-bit xmask of a string on a CONTIGUOUS [2]*nq tensor, from the letters alone."""
    nq = len(string)
    return sum(1 << (nq - 1 - d) for d, c in enumerate(string) if c in "XY")


# ---- 1. every addressing form at the smallest sizes where it exists ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [12, 13])
def test_every_addressing_form(nq, kind):
    rng = np.random.default_rng(100 + nq)
    a = crand(rng, (2,) * nq, kind)
    t = gpu(a)
    strings = addressing_strings(nq)
    assert len(strings) == 28
    coeffs = rng.standard_normal(28) + 1j * rng.standard_normal(28)
    for c, p in zip(coeffs, strings):
        want = oracle_string(a, p)
        got = A.pauli_apply(t, p)
        assert got.dtype == t.dtype and got.shape == t.shape and got.stride() == t.stride()
        assert (got.cpu().numpy().astype(np.complex128) == want).all(), p     # by value: -0.0 == 0.0
        check(A.pauli_sum_apply(t, [(c, p)]), c * want, a, [(c, p)], kind, f"[2]*{nq} {kind} {p}")


# ---- 2. many groups and many terms per group in one launch ------------------------------------------------------------------
def test_many_groups_and_many_terms_per_group():
    nq = 13
    rng = np.random.default_rng(2)
    strings = addressing_strings(nq)
    for flips in (on_bits(nq, {}), on_bits(nq, {2: "X", 6: "X"}), on_bits(nq, {12: "X", 0: "X"}), on_bits(nq, {10: "X", 11: "X", 5: "X"})):
        for _ in range(40):
            strings.append("".join(rng.choice(["X", "Y"]) if c == "X" else rng.choice(["I", "Z"]) for c in flips))
    order = rng.permutation(len(strings))
    strings = [strings[k] for k in order]
    coeffs = rng.standard_normal(len(strings)) + 1j * rng.standard_normal(len(strings))
    terms = list(zip(coeffs, strings))
    assert len(terms) == 28 + 160
    for kind in ("c64", "c128"):
        a = crand(rng, (2,) * nq, kind)
        t = gpu(a)
        info = A.pauli_apply_info(t.shape, t.stride(), terms, t.dtype)
        xms = {xmask_of(s) for s in strings}
        assert info["n_groups"] == len(xms) and info["n_xmask_hi"] == len({x >> 10 for x in xms}) and info["n_launches"] == 1
        assert max(np.bincount(info["group"])) >= 40
        check(A.pauli_sum_apply(t, terms), oracle_sum(a, terms), a, terms, kind, f"188 terms {kind}")


# ---- 3. the dense-matrix oracle ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dense_case(nq, which):
    rng = np.random.default_rng(300 + nq)
    if which == "random":
        strings = ["".join(rng.choice(list("IXYZ"), nq)) for _ in range(30)]
        terms = list(zip(rng.standard_normal(30) + 1j * rng.standard_normal(30), strings))
    else:
        terms = ising(list(range(nq)))
    return terms, dense_matrix(nq, terms)


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("which", ["random", "ising"])
@pytest.mark.parametrize("nq", [9, 10, 11])
def test_against_the_dense_matrix(nq, which, kind):
    terms, h = dense_case(nq, which)
    assert len(terms) == (30 if which == "random" else 2 * nq - 1)
    a = crand(np.random.default_rng(nq), (2,) * nq, kind)
    want = (h @ a.astype(np.complex128).reshape(-1)).reshape(a.shape)
    check(A.pauli_sum_apply(gpu(a), terms), want, a, terms, kind, f"dense {nq} qubits {which} {kind}")


# ---- 4. permuted layouts are read in place and written in the same layout ---------------------------------------------------
def apply_in_place_checks(t, a_logical, terms, kind, label):
    before, ptr = t.clone(), t.data_ptr()
    y = A.pauli_sum_apply(t, terms)
    assert y.stride() == t.stride() and y.shape == t.shape and y.dtype == t.dtype
    assert t.data_ptr() == ptr and torch.equal(t, before)
    assert torch.equal(torch.view_as_real(t), torch.view_as_real(before))
    check(y, oracle_sum(a_logical, terms), a_logical, terms, kind, label)
    out = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=t.device)
    assert A.pauli_sum_apply(t, terms, out=out) is out and torch.equal(out, y)


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_permuted_layouts(kind):
    rng = np.random.default_rng(7)
    a = crand(rng, (2,) * 12, kind)
    base = gpu(a)
    for _ in range(3):
        perm = [int(p) for p in rng.permutation(12)]
        t = base.permute(perm)
        assert t.data_ptr() == base.data_ptr() and not t.is_contiguous()
        strings = ["".join(rng.choice(list("IXYZ"), 12)) for _ in range(6)] + ["X" * 12, {0: "Y", -1: "Z"}, {5: "x"}]
        terms = list(zip(rng.standard_normal(9) + 1j * rng.standard_normal(9), strings))
        apply_in_place_checks(t, a.transpose(perm), terms, kind, f"perm {perm}")
    # extent-1 dims and a leading row dimension carrying I
    b = crand(rng, (1, 2, 2, 1) + (2,) * 10 + (1,), kind)
    pb = (0, 5, 2, 3, 1, 4, 6, 7, 8, 9, 10, 11, 13, 12, 14)
    strings = ["I" + "XZ" + "I" + "YIZXIIYZXZ" + "I", "IZZIIIIIIIIIIZI", {1: "X", 13: "Y"}, "I" * 15]
    apply_in_place_checks(gpu(b).permute(pb), b.transpose(pb), list(zip([0.5, -1.25j, 2.0 + 1j, -0.75], strings)), kind, "[1, 2, 2, 1, ...]")
    c = crand(rng, (4, 2, 2, 2, 8, 2, 2, 2, 2), kind)                        # 2^12 elements, two wider dims carrying I
    pc = (1, 0, 3, 2, 5, 4, 7, 6, 8)
    strings = ["XIZYXIIZY", "ZIZIZIZIZ", "YIIIIIIIX", {0: "X"}]
    apply_in_place_checks(gpu(c).permute(pc), c.transpose(pc), list(zip([1.0, 0.3 - 0.1j, -2.0j, 0.7], strings)), kind, "[2, 4, ...]")


# ---- 5. states below one tile -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [1, 2, 5, 9])
def test_small_states(nq, kind):
    rng = np.random.default_rng(30 + nq)
    a = crand(rng, (2,) * nq, kind)
    t = gpu(a)
    for q in range(nq):
        for c in "XYZ":
            got = A.pauli_apply(t, {q: c}).cpu().numpy().astype(np.complex128)
            assert (got == oracle_string(a, {q: c})).all(), (q, c)
    strings = [{0: "X"}, {nq - 1: "Y"}, "Z" * nq, "Y" * nq, "I" * nq]
    terms = list(zip(rng.standard_normal(5) + 1j * rng.standard_normal(5), strings))
    check(A.pauli_sum_apply(t, terms), oracle_sum(a, terms), a, terms, kind, f"[2]*{nq} {kind} five terms")


# ---- 6. more tiles than one wave of workgroups ------------------------------------------------------------------------------
def test_grid_stride_over_4096_tiles_and_determinism():
    rng = np.random.default_rng(22)
    a = crand(rng, (2,) * 22)
    t = gpu(a)
    terms = ising(list(range(22)))
    info = A.pauli_apply_info(t.shape, t.stride(), terms)
    assert len(terms) == 43 and info["n_groups"] == 23 and a.size // 1024 > 2048     # (2048: the grid cap of the Pauli kernels)
    y = A.pauli_sum_apply(t, terms)
    assert torch.equal(y, A.pauli_sum_apply(t, terms))
    check(y, oracle_sum(a, terms), a, terms, "c64", "[2]*22 Ising")


# ---- 7. algebra -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_algebra(kind):
    nq = 13
    rng = np.random.default_rng(70)
    a = crand(rng, (2,) * nq, kind)
    t = gpu(a)
    M = float(np.abs(a).max())
    by_ny = [on_bits(nq, {1: "Y", 2: "Y", 9: "Y", 10: "Y", 7: "X"}), on_bits(nq, {4: "Y", 12: "Z"}), on_bits(nq, {4: "Y", 11: "Y"}),
             on_bits(nq, {0: "Y", 4: "Y", 11: "Y", 2: "Z"})]
    for ny, p in enumerate(by_ny):
        assert p.count("Y") % 4 == ny
        assert torch.equal(A.pauli_apply(A.pauli_apply(t, p), p), t), p       # P^2 = 1, exactly
    # Two roundings of an element of size at most |a| (to the dtype after each rotation), with margin 2
    eps = 2.0 ** -24 if kind == "c64" else 4 * 2.0 ** -53
    norm2 = A.norm2(t)
    for p, theta in ((by_ny[1], 0.37), (by_ny[0], -1.9), ("X" * nq, 0.5)):
        r = A.pauli_rotate(t, p, theta)
        back = A.pauli_rotate(r, p, -theta)
        err = float((back - t).abs().max())
        print(f"rotate {p} {theta}: round trip err {err:.3e} (bound {4 * eps * M:.3e}); norm2 change "
              f"{abs(A.norm2(r) - norm2) / norm2:.3e} (bound {4 * eps + 2 * a.size * 2.0 ** -53:.3e})")
        assert err <= 4 * eps * M
        # y = U a + e with |e| <= eps |y|: | |y|^2 - |a|^2 | <= 2 eps |a|^2 to first order, margin 2; plus the error of the two
        # float64 sums themselves, (n - 1) 2^-53 norm2 each (the bound of tests/test_born_gpu.py)
        assert abs(A.norm2(r) - norm2) <= (4 * eps + 2 * a.size * 2.0 ** -53) * norm2
        want = np.cos(theta) * a.astype(np.complex128) - 1j * np.sin(theta) * oracle_string(a, p)
        check(r, want, a, [(np.cos(theta), "I" * nq), (-1j * np.sin(theta), p)], kind, f"rotate {p}")
    theta = 0.81
    terms = [(np.cos(theta), "I" * nq), (-1j * np.sin(theta), "I" * nq)]
    check(A.pauli_rotate(t, "I" * nq, theta), np.exp(-1j * theta) * a.astype(np.complex128), a, terms, kind, "identity rotation")
    check(A.pauli_rotate(t, {}, theta), np.exp(-1j * theta) * a.astype(np.complex128), a, terms, kind, "identity rotation {}")


# ---- 8. consistency with the layers already there ----------------------------------------------------------------------------
def dyadic_state(rng, shape, kind):
    """Amplitudes m / 8 with integer |m| <= 8 in both components: exact in float32 and float64."""
    a = (rng.integers(-8, 9, shape) + 1j * rng.integers(-8, 9, shape)) / 8.0
    return a.astype(KINDS[kind][0])


@pytest.mark.parametrize("kind,data", [("c64", "dyadic"), ("c128", "dyadic"), ("c128", "gaussian")])
def test_consistency_with_overlap_and_expectation(kind, data):
    """Re overlap(a, H a) against pauli_sum_expectation(a, terms, normalize=False) within tol(n) * norm2 * C, the bound of
    tests/test_pauli_gpu.py (tol(n) = 4 n 2^-53), for 25 real-coefficient terms on a permuted [2]*14 state, in both dtypes.

    The choice of the data.  The bound knows float64 roundings only, so the identity can hold to it only where y = H a is STORED
    without a further error.  A complex64 y of generic data carries one rounding of relative size 2^-24 per element whatever the
    kernel does, and <a|e> over 2^14 such errors e is of the order 2^-24 |a| |Ha| / sqrt(n): measured on an MI355X with Gaussian
    amplitudes and coefficients, 1.059e-05 against the bound 4.285e-06 (Re<a|Ha> = 1.001732632e+03, sum c<P> = 1.001732642e+03),
    with the same float64 kernel arithmetic that passes in complex128.  The state of both dtypes is therefore dyadic: amplitudes
    m / 8 (|m| <= 8) and coefficients k / 8 (|k| <= 16), so that every element of H a is an integer below 25 * 16 * 8 * 2 < 2^24
    over 64 -- exact in float32 -- and the complex64 case checks the same thing the complex128 case does, the agreement of the two
    layers' masks, phases, signs and group handling, to the stated bound.  The Gaussian state is kept as well, in complex128,
    where the storage rounding is of the bound's own kind; Gaussian complex64 is the one combination that no complex64 output can
    pass and is not a case."""
    rng = np.random.default_rng(88)
    strings = ["".join(rng.choice(list("IXYZ"), 14)) for _ in range(25)]
    if data == "dyadic":
        a, coeffs = dyadic_state(rng, (2,) * 14, kind), rng.integers(-16, 17, 25) / 8.0
    else:
        a, coeffs = crand(rng, (2,) * 14, kind), rng.standard_normal(25)
    t = gpu(a).permute([int(p) for p in rng.permutation(14)])
    terms = list(zip(coeffs, strings))
    y = A.pauli_sum_apply(t, terms)
    assert y.dtype == t.dtype
    aha, na, _ = A.overlap(t, y)
    want = A.pauli_sum_expectation(t, terms, normalize=False)
    bound = 4 * a.size * 2.0 ** -53 * na * np.abs(coeffs).sum()                 # tol(n) * norm2 * C of tests/test_pauli_gpu.py
    print(f"{kind} {data}: Re<a|Ha> {aha.real:.9e} sum c<P> {want:.9e} diff {abs(aha.real - want):.3e} (bound {bound:.3e}) Im {aha.imag:.3e}")
    assert abs(want) > 1e3 * bound                                              # (the value is not trivially small)
    assert abs(aha.real - want) <= bound


# ---- 9. variance ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_variance_of_an_eigenstate_is_exactly_zero(kind):
    nq = 12
    rng = np.random.default_rng(9)
    strings = ["".join(rng.choice(["I", "Z"], nq)) for _ in range(10)]
    coeffs = rng.integers(-16, 17, 10) / 8.0                                   # dyadic: every sum below is exact in float32
    terms = list(zip(coeffs, strings))
    diag = np.zeros((2,) * nq)
    for c, s in terms:
        d = np.ones((2,) * nq)
        for q, letter in enumerate(s):
            if letter == "Z":
                shape = [1] * nq
                shape[q] = 2
                d = d * np.array([1.0, -1.0]).reshape(shape)
        diag = diag + c * d
    for index in ((0,) * nq, tuple(int(b) for b in rng.integers(0, 2, nq)), (1,) * nq):
        a = np.zeros((2,) * nq, dtype=KINDS[kind][0])
        a[index] = 1.0
        e, var = A.pauli_sum_variance(gpu(a), terms)
        assert isinstance(e, float) and isinstance(var, float)
        assert e == diag[index] and var == 0.0, (index, e, var)


def test_variance_of_a_random_state_against_the_dense_matrix():
    nq = 10
    rng = np.random.default_rng(10)
    strings = ["".join(rng.choice(list("IXYZ"), nq)) for _ in range(20)]
    coeffs = rng.standard_normal(20)
    terms = list(zip(coeffs, strings))
    h = dense_matrix(nq, terms)
    a = crand(rng, (2,) * nq, "c128")
    a /= np.linalg.norm(a)
    v = a.reshape(-1)
    hv = h @ v
    e_want = np.vdot(v, hv).real / np.vdot(v, v).real
    var_want = np.vdot(hv, hv).real / np.vdot(v, v).real - e_want ** 2
    e, var = A.pauli_sum_variance(gpu(a), terms)
    C = np.abs(coeffs).sum()
    print(f"E {e:.12e} (want {e_want:.12e}) var {var:.12e} (want {var_want:.12e}); bound {1e-12 * C * C:.3e}")
    assert abs(e - e_want) <= 1e-12 * C * C and abs(var - var_want) <= 1e-12 * C * C
    with pytest.raises(ValueError, match="real"):
        A.pauli_sum_variance(gpu(a), [(1.0, strings[0]), (0.5j, strings[1])])


# ---- 10. a real state -------------------------------------------------------------------------------------------------------
def test_n12_contraction_output_takes_the_ising_sum():
    case = load_case(os.path.join(GOLDEN, "n12_dense.npz"))
    raw = A.tensor_contraction(case.fresh_tensors(device=DEV), case.scheme)
    ptr = raw.data_ptr()
    two = [d for d, e in enumerate(raw.shape) if e == 2]
    assert len(two) == 12
    terms = ising(two)
    before = raw.clone()
    y = A.pauli_sum_apply(raw, terms)
    assert raw.data_ptr() == ptr and torch.equal(raw, before) and y.stride() == raw.stride()
    a = raw.cpu().numpy()
    check(y, oracle_sum(a, terms), a, terms, "c64", "n12")


# ---- 11. argument checks ----------------------------------------------------------------------------------------------------
def test_argument_checks_on_gpu_tensors():
    t = gpu(np.zeros((2,) * 4, dtype=np.complex64))
    terms = [(1.0, "ZZII"), (0.5, "XIIY")]
    with pytest.raises(ValueError, match="overlaps"):
        A.pauli_sum_apply(t, terms, out=t)
    store = torch.zeros(24, dtype=torch.complex64, device=DEV)
    with pytest.raises(ValueError, match="overlaps"):
        A.pauli_sum_apply(store[:16].view((2,) * 4), terms, out=store[8:24].view((2,) * 4))
    with pytest.raises(ValueError, match="strides"):
        A.pauli_sum_apply(t, terms, out=torch.empty_like(t).permute(1, 0, 2, 3))
    with pytest.raises(ValueError, match="dtype"):
        A.pauli_sum_apply(t, terms, out=torch.empty_like(t, dtype=torch.complex128))
    with pytest.raises(TypeError, match="complex"):
        A.pauli_apply(t.real.contiguous(), "ZZII")
    with pytest.raises(ValueError, match="dense"):
        A.pauli_apply(t[:, :, ::2], "ZZII")
    with pytest.raises(ValueError, match="at least one"):
        A.pauli_sum_apply(t, [])
    with pytest.raises(ValueError, match="length"):
        A.pauli_apply(t, "ZZZ")
    op = A.PauliSumOperator(t.shape, t.stride(), t.dtype, terms, t.device)
    assert op(t).shape == t.shape
    with pytest.raises(ValueError, match="built for"):
        op(t.permute(3, 2, 1, 0))
    with pytest.raises(ValueError, match="built for"):
        op(t.to(torch.complex128))
    # (a y that starts 8 bytes into a 16-byte unit is refused by the library as well)
    odd = torch.zeros(17, dtype=torch.complex64, device=DEV)[1:].view((2,) * 4)
    with pytest.raises(ValueError, match="16-byte"):
        A.pauli_sum_apply(t, terms, out=odd)
