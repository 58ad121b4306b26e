"""Reduced density matrices on the GPU (artensor_amd/rdm.py) against a numpy oracle in complex128: the kept dims are moved to
the front, the state is reshaped to (D, R) and rho = M @ M.conj().T.

The tolerance is derived, not measured.  Each real component of rho_ij is a float64 sum of 2 R products whose absolute values
sum to at most sqrt(rho_ii rho_jj) (Cauchy-Schwarz), so two such sums in any order -- the kernels' and the oracle's -- differ by
at most tol(n) * sqrt(rho_ii rho_jj) with tol(n) = 4 n 2^-53, the function of tests/test_born_gpu.py; the factor covers the
oracle's own rounding and, for complex128 input, the rounding of the products (complex64 products are exact in float64)."""
import os

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import rdm
from artensor_amd.fixtures import load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CDT = {"c64": (np.complex64, np.float32), "c128": (np.complex128, np.float64)}


def tol(n):
    return 4.0 * n * 2.0 ** -53


def crand(rng, shape, kind="c64"):
    ct, ft = CDT[kind]
    return (rng.standard_normal(shape).astype(ft) + 1j * rng.standard_normal(shape).astype(ft)).astype(ct)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def oracle_rdm(a_logical, keep):
    a = np.asarray(a_logical).astype(np.complex128)
    keep = [k % a.ndim for k in keep]
    rest = [d for d in range(a.ndim) if d not in keep]
    D = int(np.prod([a.shape[k] for k in keep])) if keep else 1
    m = a.transpose(keep + rest).reshape(D, -1)
    return m @ m.conj().T


def check(t, a_logical, keep, label=""):
    """The oracle comparison and the structure checks of one case; returns rho."""
    n = a_logical.size
    want = oracle_rdm(a_logical, keep)
    rho = A.reduced_density_matrix(t, keep)
    D = want.shape[0]
    assert rho.is_cuda and rho.dtype == torch.complex128 and tuple(rho.shape) == (D, D)
    got = rho.cpu().numpy()
    diag = want.diagonal().real
    scale = np.sqrt(np.outer(diag, diag))
    err = np.abs(got - want)
    worst = float((err / np.maximum(scale, 1e-300)).max())
    print(f"{label} D={D} n={n}: worst |d rho_ij| / sqrt(rho_ii rho_jj) = {worst:.3e}, tol {tol(n):.3e}")
    assert (np.abs(got.real - want.real) <= tol(n) * scale).all() and (np.abs(got.imag - want.imag) <= tol(n) * scale).all()
    # structure
    assert torch.equal(rho, rho.mH)
    assert bool((rho.diagonal().imag == 0).all())
    trace = float(got.diagonal().real.sum())
    marg = A.marginal_probabilities(t, keep).reshape(-1).cpu().numpy()
    assert np.abs(got.diagonal().real - marg).max() <= tol(n) * trace
    assert (np.abs(got.diagonal().real - marg) <= tol(n) * np.maximum(marg, got.diagonal().real)).all()
    assert abs(trace - A.norm2(t)) <= tol(n) * trace
    lam_min = float(np.linalg.eigvalsh(got).min())
    print(f"{label} smallest eigenvalue / trace = {lam_min / trace:.3e}")
    assert lam_min >= -tol(n) * trace
    # the same call again gives the same bits
    assert torch.equal(rho, A.reduced_density_matrix(t, keep))
    return rho


def kept_dims(k, where, nd=20):
    if where == "fastest":
        return list(range(nd - k, nd))
    if where == "slowest":
        return list(range(k))
    return sorted(int(x) for x in np.random.default_rng(100 + k).choice(nd, k, replace=False))


# ---- random states --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("where", ["fastest", "slowest", "mixed"])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 5, 6, 7, 10])
def test_rdm_of_a_20_qubit_state(k, where, kind, permuted):
    rng = np.random.default_rng(31)
    a = crand(rng, (2,) * 20, kind)
    t = gpu(a)
    if permuted:
        perm = list(rng.permutation(20))
        t, a = t.permute(perm), a.transpose(perm)
        assert not t.is_contiguous()
    keep = kept_dims(k, where)
    want_kernel = N.RDM_STREAM if k >= 1 else N.RDM_GENERIC
    assert rdm.rdm_info(t.shape, t.stride(), keep, t.dtype)["kernel"] == want_kernel
    check(t, a, keep, f"k={k} {where} {kind} permuted={permuted}")


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("keep", [[18, 2, 11], [5, 19, 0, 7, 12, 3, 1], [-1, 0], [9, 8, 7, 6, 5, 4, 3, 2, 1, 0]])
def test_kept_order_that_is_not_ascending(keep, kind):
    rng = np.random.default_rng(37)
    a = crand(rng, (2,) * 20, kind)
    perm = list(rng.permutation(20))
    t, a = gpu(a).permute(perm), a.transpose(perm)
    rho = check(t, a, keep, f"keep={keep} {kind}")
    # rows are digits of the kept dims, the first one most significant: the diagonal is the marginal in that order
    marg = A.marginal_probabilities(t, keep)
    assert tuple(marg.shape) == (2,) * len(keep)
    assert np.abs(rho.diagonal().real.reshape(marg.shape).cpu().numpy() - marg.cpu().numpy()).max() <= tol(a.size) * float(marg.sum())


# ---- other shapes: the generic form, and both forms at the 2^12 boundary ------------------------------------------------------
@pytest.mark.parametrize("shape,keep,kind", [((3, 4, 5, 2, 6), [1, 3], "c64"), ((3, 4, 5, 2, 6), [4, 0], "c128"),
                                             ((3, 4, 5, 2, 6), [], "c64"), ((3, 4, 5, 2, 6), [0, 1, 2, 3, 4], "c64"),
                                             ((1, 2, 1, 2), [1], "c64"), ((1, 2, 1, 2), [0, 3, 2], "c128"),
                                             ((4096, 3), [1], "c64"), ((4096, 3), [1], "c128"), ((6, 4096), [0], "c64"),
                                             ((250, 2, 2, 2), [3, 1], "c64")])
def test_rdm_of_other_shapes_takes_the_generic_form(shape, keep, kind):
    rng = np.random.default_rng(41)
    a = crand(rng, shape, kind)
    t = gpu(a)
    assert rdm.rdm_info(t.shape, t.stride(), keep, t.dtype)["kernel"] == N.RDM_GENERIC
    check(t, a, keep, f"{shape} keep={keep} {kind}")
    if len(shape) > 2:
        perm = list(rng.permutation(len(shape)))
        check(t.permute(perm), a.transpose(perm), keep, f"{shape} permuted keep={keep} {kind}")


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq,want_kernel", [(11, N.RDM_GENERIC), (12, N.RDM_STREAM), (13, N.RDM_STREAM)])
def test_both_forms_meet_at_the_boundary(nq, want_kernel, kind):
    rng = np.random.default_rng(43 + nq)
    a = crand(rng, (2,) * nq, kind)
    perm = list(rng.permutation(nq))
    t, a = gpu(a).permute(perm), a.transpose(perm)
    for keep in ([0], [nq - 1, 3], [2, 5, 1, 7], list(range(6)), list(range(nq - 7, nq))):
        assert rdm.rdm_info(t.shape, t.stride(), keep, t.dtype)["kernel"] == want_kernel
        check(t, a, keep, f"2^{nq} keep={keep} {kind}")
    # D = 256: 2^12 elements leave exactly the 16 dropped states of one panel, 2^13 leave two panels
    info = rdm.rdm_info(t.shape, t.stride(), list(range(8)), t.dtype)
    assert info["kernel"] == want_kernel
    check(t, a, list(range(8)), f"2^{nq} D=256 {kind}")
    if nq == 13:   # D = 1024 leaves 8 dropped states: below one panel, the generic form
        assert rdm.rdm_info(t.shape, t.stride(), list(range(10)), t.dtype)["kernel"] == N.RDM_GENERIC
        check(t, a, list(range(10)), f"2^{nq} D=1024 {kind}")


def test_mixed_power_of_two_extents_stream():
    rng = np.random.default_rng(47)
    shape = (4, 8, 2, 16, 4, 2, 8)
    a = crand(rng, shape)
    perm = list(rng.permutation(len(shape)))
    t, ap = gpu(a).permute(perm), a.transpose(perm)
    for keep in ([3], [0, 6], [1, 3, 5], [6, 2, 0, 4]):
        assert rdm.rdm_info(t.shape, t.stride(), keep, t.dtype)["kernel"] == N.RDM_STREAM
        check(t, ap, keep, f"{ap.shape} keep={keep}")


def test_argument_checks_on_gpu_tensors():
    a = gpu(crand(np.random.default_rng(1), (2,) * 14))
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        A.reduced_density_matrix(a[..., 0], [0])
    with pytest.raises(TypeError, match="complex"):
        A.reduced_density_matrix(a.real.contiguous(), [0])
    with pytest.raises(ValueError, match="keep"):
        A.reduced_density_matrix(a, [1, 1])
    with pytest.raises(ValueError, match="16-byte"):
        A.reduced_density_matrix(a.reshape(-1)[1:1 + 2 ** 12], [0])
    with pytest.raises(RuntimeError, match="1024"):
        A.reduced_density_matrix(a, list(range(11)))
    with pytest.raises(ValueError, match="shape"):
        A.expectation(a, np.eye(4), [0])
    norm = A.reduced_density_matrix(a, [0, 1], normalize=True)
    assert abs(float(norm.diagonal().real.sum()) - 1.0) <= 1e-15 * 4


# ---- known states on 16 qubits ------------------------------------------------------------------------------------------------
def h_tol(D, n):
    """Entropy bound for a state whose exact reduced eigenvalues are (1, 0, ..., 0): the computed matrix is within tol(n) * trace
    of it entry by entry, so each of the D eigenvalues moves by at most delta = D * tol(n) (Weyl), and an eigenvalue x <= delta
    contributes at most -x log2 x <= -delta log2 delta bits; the one near 1 contributes at most 2 delta."""
    delta = D * tol(n)
    return D * (-delta * np.log2(delta)) + 2 * delta


def eig_tol(D):
    """Entropy bound for a reduced matrix that is EXACT (integer sums): the only error is the eigenvalue solver's, backward stable,
    so each eigenvalue of the trace-one matrix moves by at most delta = D * 2^-52, and an eigenvalue that moves by delta changes
    -x log2 x by at most -delta log2 delta + 2 delta bits; for Renyi-2 the change 2 delta 2^j / ln 2 of -log2(sum x^2) is smaller."""
    delta = D * 2.0 ** -52
    return D * (-delta * np.log2(delta) + 2 * delta)


def product_state(kind, nq=16):
    """Single-qubit amplitudes with components in {0, +-1/2, +-1, +-2}: every product is exact in float32, so the complex64
    tensor IS a product state."""
    qs = [(1, 0.5j), (0.5, -1), (1, 1), (1, -1j), (2, 0.5 + 0.5j), (1j, 1), (-1, 0.5), (0.5 - 0.5j, 1)]
    a = np.ones((), dtype=np.complex128)
    for q in range(nq):
        a = np.multiply.outer(a, np.array(qs[q % len(qs)], dtype=np.complex128))
    out = a.astype(CDT[kind][0])
    assert (out.astype(np.complex128) == a).all()
    return out


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_product_state_has_purity_1_and_entropy_0(kind):
    a = product_state(kind)
    t = gpu(a)
    n = a.size
    for keep in ([0], [15], [3, 9], [0, 1, 2, 3, 4], [10, 2, 7, 15, 0, 4], list(range(8)), list(range(15, 5, -1))):
        D = 2 ** len(keep)
        check(t, a, keep, f"product {kind} keep={keep}")
        # purity = sum |rho_ij|^2 / tr^2, every |rho_ij| within tol * sqrt(rho_ii rho_jj): first order 2 tol, plus the float64 sum
        p = A.purity(t, keep)
        assert abs(p - 1.0) <= 4 * tol(n) + D * D * 2.0 ** -52
        assert A.purity(t, keep) == p
        h = A.entanglement_entropy(t, keep)
        assert 0.0 <= h <= h_tol(D, n)
        assert 0.0 <= A.renyi_entropy(t, keep, alpha=2) <= 2 * (4 * tol(n) + D * D * 2.0 ** -52) / np.log(2) + h_tol(D, n)


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_ghz_state_gives_one_bit_for_every_proper_subset(kind):
    a = np.zeros((2,) * 16, dtype=CDT[kind][0])
    a[(0,) * 16] = 1
    a[(1,) * 16] = 1
    t = gpu(a).permute(list(np.random.default_rng(3).permutation(16)))     # GHZ is symmetric: the logical state is unchanged
    for keep in ([0], [7], [15, 0], [1, 2, 3], [14, 3, 8, 5, 0], list(range(6)), list(range(4, 14)), list(range(9, -1, -1))):
        D = 2 ** len(keep)
        want = np.zeros((D, D))
        want[0, 0] = want[-1, -1] = 1.0
        rho = A.reduced_density_matrix(t, keep)
        assert (rho.cpu().numpy() == want).all()                            # sums of ones and zeros: exact
        assert (A.reduced_density_matrix(t, keep, normalize=True).cpu().numpy() == want / 2).all()
        assert abs(A.entanglement_entropy(t, keep) - 1.0) <= eig_tol(D)
        assert abs(A.renyi_entropy(t, keep, alpha=2) - 1.0) <= eig_tol(D)
        assert abs(A.entanglement_entropy(t, keep, base=np.e) - np.log(2.0)) <= eig_tol(D)
        assert abs(A.purity(t, keep) - 0.5) <= 1e-15
    full = A.reduced_density_matrix(t, list(range(10)) )
    assert float(full.diagonal().real.sum()) == 2.0


@pytest.mark.parametrize("kind", ["c64", "c128"])
def test_bell_pairs_cut_by_keep_give_one_bit_each(kind):
    """8 pairs (2i, 2i+1), each |00> + |11> with unit amplitudes: every sum is an exact integer."""
    pair = np.array([[1, 0], [0, 1]], dtype=np.complex128)
    a = np.ones((), dtype=np.complex128)
    for _ in range(8):
        a = np.multiply.outer(a, pair)
    a = a.astype(CDT[kind][0])
    t = gpu(a)
    cases = [([0], 1), ([0, 1], 0), ([0, 2], 2), ([1, 2, 3], 1), ([0, 2, 4, 6, 8], 5), ([0, 1, 2, 3, 4, 5], 0), ([15, 13, 0, 1, 6], 3),
             ([0, 2, 4, 6, 8, 10, 12, 14], 8), ([1, 0, 3, 5, 7, 9, 11, 13, 15, 14], 6), (list(range(1, 11)), 2)]
    for keep, j in cases:
        check(t, a, keep, f"bell {kind} keep={keep}")
        assert abs(A.entanglement_entropy(t, keep) - j) <= eig_tol(2 ** len(keep))
        assert abs(A.renyi_entropy(t, keep, alpha=2) - j) <= eig_tol(2 ** len(keep))
        assert abs(A.purity(t, keep) - 2.0 ** -j) <= 1e-15
    perm = list(np.random.default_rng(5).permutation(16))
    tp, ap = t.permute(perm), a.transpose(perm)
    for keep, j in [([perm.index(0)], 1), ([perm.index(0), perm.index(1)], 0), ([perm.index(4), perm.index(9), perm.index(8)], 1)]:
        check(tp, ap, keep, f"bell permuted keep={keep}")
        assert abs(A.entanglement_entropy(tp, keep) - j) <= eig_tol(2 ** len(keep))


def numpy_expectation(a, op, dims):
    a = np.asarray(a).astype(np.complex128)
    rest = [d for d in range(a.ndim) if d not in dims]
    m = a.transpose(list(dims) + rest).reshape(op.shape[0], -1)
    return np.vdot(m, op @ m) / np.vdot(m, m)


def test_expectation_values_of_pauli_operators():
    X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
    Y = np.array([[0, -1j], [1j, 0]])
    Z = np.diag([1.0, -1.0]).astype(np.complex128)
    bell = np.array([[1, 0], [0, 1]], dtype=np.complex64)                    # |00> + |11> on qubits (2, 9)
    plus = np.array([1, 1], dtype=np.complex64)
    zero = np.array([1, 0], dtype=np.complex64)
    facs = [plus if q % 3 == 0 else zero for q in range(14)]
    a = bell
    for f in facs:
        a = np.multiply.outer(a, f)
    a = np.moveaxis(a, [0, 1], [2, 9])                                       # qubit 0 is |+>, qubit 1 is |0>
    t = gpu(a)
    for op, dims, want in ((np.kron(Z, Z), [2, 9], 1.0), (np.kron(X, X), [2, 9], 1.0), (np.kron(Y, Y), [9, 2], -1.0),
                           (np.kron(Z, X), [2, 9], 0.0), (X, [0], 1.0), (Z, [0], 0.0), (Z, [1], 1.0), (X, [2], 0.0)):
        got = A.expectation(t, op, dims)
        assert isinstance(got, complex)
        assert abs(got - want) <= 1e-14 and abs(got - numpy_expectation(a, op, dims)) <= 1e-14
        assert A.expectation(t, torch.from_numpy(op), dims) == got
    # a random state, a random Hermitian operator on three dims, digits in the order asked for
    rng = np.random.default_rng(53)
    b = crand(rng, (2,) * 16)
    h = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))
    h = h + h.conj().T
    tb = gpu(b).permute(list(rng.permutation(16)))
    bl = tb.cpu().numpy()
    for dims in ([4, 11, 0], [15, 14, 13]):
        got = A.expectation(tb, h, dims)
        want = numpy_expectation(bl, h, dims)
        # |sum_ij d rho_ij h_ji| / tr <= tol * max|h| * (sum_i sqrt(rho_ii))^2 / tr <= D * tol * max|h|; twice: the oracle's own sum
        bound = 2 * 8 * tol(b.size) * np.abs(h).max()
        assert abs(got - want) <= bound and abs(got.imag) <= bound


# ---- determinism -----------------------------------------------------------------------------------------------------------
def test_every_entry_point_is_bit_reproducible():
    rng = np.random.default_rng(59)
    a = gpu(crand(rng, (2,) * 22)).permute(list(rng.permutation(22)))
    c = gpu(crand(rng, (2,) * 18, "c128"))
    d = gpu(crand(rng, (3,) * 8))
    op = rng.standard_normal((4, 4))
    for t, keeps in ((a, ([0], [21, 3, 5], list(range(6)), [20, 1, 7, 8, 9, 10, 11], list(range(10)))), (c, ([0, 17], list(range(8)))),
                     (d, ([1, 6], [7]))):
        for keep in keeps:
            assert torch.equal(A.reduced_density_matrix(t, keep), A.reduced_density_matrix(t, keep))
            assert torch.equal(A.reduced_density_matrix(t, keep, normalize=True), A.reduced_density_matrix(t, keep, normalize=True))
            assert A.purity(t, keep) == A.purity(t, keep)
            assert A.entanglement_entropy(t, keep) == A.entanglement_entropy(t, keep)
            assert A.renyi_entropy(t, keep, alpha=3) == A.renyi_entropy(t, keep, alpha=3)
    assert A.expectation(a, op, [4, 9]) == A.expectation(a, op, [4, 9])
    rho = A.reduced_density_matrix(a, [1, 2, 3])
    assert A.entropy_of(rho) == A.entropy_of(rho.cpu()) == A.entropy_of(rho.cpu().numpy()) == A.entanglement_entropy(a, [1, 2, 3])


# ---- end to end on the committed fixtures ---------------------------------------------------------------------------------
def test_n12_contraction_feeds_the_rdm_of_four_qubits():
    case = load_case(os.path.join(GOLDEN, "n12_dense.npz"))
    raw = A.tensor_contraction(case.fresh_tensors(device=DEV), case.scheme)
    gold = case.arrays["raw"].reshape(raw.shape)
    total = float((np.abs(gold.astype(np.complex128)) ** 2).sum())
    for keep in ([0, 1, 2, 3], [11, 4, 7, 2]):
        want = oracle_rdm(gold, keep)
        rho = A.reduced_density_matrix(raw, keep)
        got = rho.cpu().numpy()
        # (the contraction itself is complex64: the amplitudes agree with the fixture's to float32 accuracy)
        assert np.abs(got - want).max() <= 1e-5 * total
        assert torch.equal(rho, rho.mH) and bool((rho.diagonal().imag == 0).all())
        check(raw, raw.cpu().numpy(), keep, f"n12 keep={keep}")


def test_n30_full_size_state_in_its_permuted_layout():
    """k = 6 on the 2^30 amplitudes of the n30 contraction, in the permuted view the slice loop returns.  The oracle does not use
    the code under test: torch.matmul in complex128 on the device over up to 32 slabs of the dropped index, added in float64."""
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 24e9:
        pytest.skip(f"needs 24 GB of free device memory for the 2^30-amplitude state and its contraction, {free / 1e9:.1f} GB free")
    case = load_case(os.path.join(GOLDEN, "n30_dense.npz"))
    raw = A.tensor_contraction(case.fresh_tensors(device=DEV), case.scheme)
    assert raw.numel() == 2 ** 30
    final = raw.permute(case.meta["permute_dims"])              # the view the reference returns
    assert not final.is_contiguous()
    n = raw.numel()
    keep = [0, 1, 2, 3, 4, 5]
    info = rdm.rdm_info(final.shape, final.stride(), keep, final.dtype)
    assert info["kernel"] == N.RDM_STREAM and info["dim"] == 64 and info["tiles"] == 1
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    rho = A.reduced_density_matrix(final, keep)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"n30: device memory rise {rise} B, workspace {info['workspace_bytes']} B")
    assert rise <= info["workspace_bytes"] + 64 * 64 * 16 + 2 * 512         # the workspace and the output, nothing of the state's size
    # (torch copies at most 16 dims: runs of adjacent dropped dims of the contiguous `raw` are merged first, and the slabs are
    # ranges of the longest run)
    kept_raw = [case.meta["permute_dims"][d] for d in keep]
    shape, pos, dropped_run = [], {}, False
    for d in range(raw.dim()):
        if d in kept_raw:
            pos[d] = len(shape)
            shape.append(2)
            dropped_run = False
        elif dropped_run:
            shape[-1] *= 2
        else:
            shape.append(2)
            dropped_run = True
    merged = raw.reshape(shape)
    order = [pos[d] for d in kept_raw] + [i for i in range(len(shape)) if i not in pos.values()]
    longest = max((i for i in range(len(shape)) if i not in pos.values()), key=lambda i: shape[i])
    pieces = min(shape[longest], 32)
    step = shape[longest] // pieces
    want = torch.zeros(64, 64, dtype=torch.complex128, device=DEV)
    for s in range(pieces):
        m = merged.narrow(longest, s * step, step).permute(order).reshape(64, -1).to(torch.complex128)
        want += m @ m.mH
        del m
    want = want.cpu().numpy()
    got = rho.cpu().numpy()
    diag = want.diagonal().real
    scale = np.sqrt(np.outer(diag, diag))
    worst = float((np.abs(got - want) / scale).max())
    print(f"n30: worst |d rho_ij| / sqrt(rho_ii rho_jj) = {worst:.3e}, tol {tol(n):.3e}")
    assert (np.abs(got.real - want.real) <= tol(n) * scale).all() and (np.abs(got.imag - want.imag) <= tol(n) * scale).all()
    assert torch.equal(rho, rho.mH) and bool((rho.diagonal().imag == 0).all())
    trace = float(got.diagonal().real.sum())
    marg = A.marginal_probabilities(final, keep).reshape(-1).cpu().numpy()
    assert np.abs(got.diagonal().real - marg).max() <= tol(n) * trace
    assert abs(trace - A.norm2(final)) <= tol(n) * trace
    assert abs(trace - case.meta["norm2"]) < 1e-5
    assert float(np.linalg.eigvalsh(got).min()) >= -tol(n) * trace
    assert torch.equal(rho, A.reduced_density_matrix(final, keep))
    h = A.entanglement_entropy(final, keep)
    print(f"n30: entanglement entropy of the first six qubits {h:.6f} bits")
    assert 0.0 <= h <= 6.0
