"""Born statistics on the GPU (artensor_amd/born.py) against a numpy oracle that forms |a|^2 in float64 and uses np.cumsum,
np.vdot on complex128 and reshape(...).sum.

Tolerances are derived, not measured: a float64 sum of n non-negative terms in ANY order is within (n - 1) * 2^-53 * sum of the
exact value, so two such sums (the kernels' and the oracle's) differ by at most tol(n) = 4 * n * 2^-53 relative, the factor
covering the oracle's own rounding and the term's own rounding."""
import os

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import born
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


def sq(a):
    a = np.asarray(a)
    return a.real.astype(np.float64) ** 2 + a.imag.astype(np.float64) ** 2


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def memory_index(idx, t):
    """flat MEMORY index of logical multi-indices [m, dim] of tensor t (numpy int64)."""
    out = np.zeros(idx.shape[0], dtype=np.int64)
    for d, s in enumerate(t.stride()):
        out += idx[:, d] * s
    return out


# ---- overlap, norm, fidelity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("n", [1, 3, 1000, 2 ** 20 + 7, 2 ** 24])
def test_overlap_norm_and_fidelity(n, kind):
    rng = np.random.default_rng(n % 1000 + len(kind))
    a, b = crand(rng, n, kind), crand(rng, n, kind)
    ta, tb = gpu(a), gpu(b)
    na, nb = sq(a).sum(), sq(b).sum()
    inner = np.vdot(a.astype(np.complex128), b.astype(np.complex128))
    got_inner, got_na, got_nb = A.overlap(ta, tb)
    print(f"n={n} {kind}: norm err {abs(got_na - na) / na:.3e} inner err {abs(got_inner - inner) / np.sqrt(na * nb):.3e} tol {tol(n):.3e}")
    assert abs(got_na - na) <= tol(n) * na and abs(got_nb - nb) <= tol(n) * nb
    assert abs(got_inner - inner) <= tol(n) * np.sqrt(na * nb)
    assert abs(A.norm2(ta) - na) <= tol(n) * na
    want_f = abs(inner) ** 2 / (na * nb)
    assert abs(A.fidelity(ta, tb) - want_f) <= 4 * tol(n) * max(np.sqrt(want_f), tol(n)) + 4 * tol(n) * want_f
    dev4 = A.overlap(ta, tb, device=True)
    assert dev4.is_cuda and dev4.dtype == torch.float64 and dev4.tolist() == [got_inner.real, got_inner.imag, got_na, got_nb]
    assert abs(A.fidelity(ta, ta) - 1.0) <= 4 * tol(n)


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("n", [3, 1000, 2 ** 20 + 7])
def test_overlap_of_an_orthogonal_pair(n, kind):
    """b = a rotated so that every product conj(a[i]) b[i] is cancelled by its neighbour's: <a|b> = 0 exactly."""
    rng = np.random.default_rng(7)
    half = crand(rng, n // 2, kind)
    a = np.concatenate([half, half])
    b = np.concatenate([half, -half])
    if n % 2:
        a, b = np.concatenate([a, [1.0]]).astype(a.dtype), np.concatenate([b, [0.0]]).astype(a.dtype)
    assert a.size == n
    inner, na, nb = A.overlap(gpu(a), gpu(b))
    assert abs(inner) <= tol(n) * np.sqrt(sq(a).sum() * sq(b).sum())
    assert abs(na - sq(a).sum()) <= tol(n) * na and abs(nb - sq(b).sum()) <= tol(n) * max(nb, 1e-300)
    assert A.fidelity(gpu(a), gpu(b)) <= tol(n) ** 2


def test_overlap_of_identically_permuted_views():
    rng = np.random.default_rng(3)
    a, b = crand(rng, (2,) * 20), crand(rng, (2,) * 20)
    perm = list(rng.permutation(20))
    ta, tb = gpu(a).permute(perm), gpu(b).permute(perm)
    assert not ta.is_contiguous()
    inner, na, nb = A.overlap(ta, tb)
    n = a.size
    assert abs(inner - np.vdot(a.astype(np.complex128), b.astype(np.complex128))) <= tol(n) * np.sqrt(na * nb)
    assert abs(na - sq(a).sum()) <= tol(n) * na
    with pytest.raises(ValueError, match="equal strides"):
        A.overlap(ta, gpu(b))
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        A.norm2(gpu(a)[..., 0])


# ---- sampling -----------------------------------------------------------------------------------------------------------
def check_samples(t, a_mem, u, idx, prob):
    """a_mem: the amplitudes in MEMORY order (numpy); every sample is checked."""
    n = a_mem.size
    p = sq(a_mem)
    cdf = np.cumsum(p)
    total = cdf[-1]
    tgt = u * total
    i = memory_index(idx.cpu().numpy(), t)
    assert i.shape == u.shape and (i >= 0).all() and (i < n).all()
    below = np.where(i > 0, cdf[np.maximum(i - 1, 0)], 0.0)
    slack = tol(n) * total
    worst = max((below - tgt).max(), (tgt - cdf[i]).max())
    print(f"n={n} m={u.size}: worst interval miss {worst / total:.3e} (tol {tol(n):.3e})")
    assert (below - slack <= tgt).all() and (tgt < cdf[i] + slack).all()
    assert (p[i] > 0).all()
    assert np.abs(prob.cpu().numpy() - p[i] / total).max() <= tol(n) * (p[i] / total).max()


@pytest.mark.parametrize("n,m", [(2 ** 10, 1), (2 ** 10, 1000), (2 ** 10, 10 ** 6), (2 ** 20 + 5, 1), (2 ** 20 + 5, 1000),
                                 (2 ** 20 + 5, 10 ** 6), (2 ** 24, 1), (2 ** 24, 1000), (2 ** 24, 10 ** 6)])
def test_sampling_with_explicit_uniforms(n, m):
    rng = np.random.default_rng(n % 97 + m % 89)
    a = crand(rng, n)
    u = rng.random(m)                                          # unsorted
    t = gpu(a)
    idx, prob = A.sample(t, uniforms=torch.from_numpy(u).to(DEV))
    assert idx.shape == (m, 1) and idx.dtype == torch.int64 and prob.shape == (m,) and prob.dtype == torch.float64
    check_samples(t, a, u, idx, prob)


def test_sampling_complex128():
    rng = np.random.default_rng(5)
    a = crand(rng, 2 ** 20 + 5, "c128")
    u = rng.random(1000)
    t = gpu(a)
    idx, prob = A.sample(t, uniforms=torch.from_numpy(u).to(DEV))
    check_samples(t, a, u, idx, prob)


def test_sampling_a_single_nonzero_element():
    for n, at in ((2 ** 10, 0), (2 ** 20 + 5, 2 ** 20 + 4), (2 ** 20 + 5, 777_777), (5, 3)):
        a = np.zeros(n, dtype=np.complex64)
        a[at] = 0.3 - 0.4j
        u = np.concatenate([np.random.default_rng(1).random(1000), [0.0, 1.0 - 2.0 ** -53]])
        idx, prob = A.sample(gpu(a), uniforms=torch.from_numpy(u).to(DEV))
        assert (idx[:, 0] == at).all() and (prob == 1.0).all()
    with pytest.raises(ValueError, match="zero"):
        A.sample(gpu(np.zeros(64, dtype=np.complex64)), 3)


def test_sampling_skips_zero_quarters_and_takes_the_extreme_uniforms():
    rng = np.random.default_rng(11)
    n = 2 ** 20
    a = crand(rng, n)
    a[: n // 4] = 0
    a[-(n // 4):] = 0
    u = np.concatenate([[0.0, 1.0 - 2.0 ** -53], rng.random(5000), [1.0 - 2.0 ** -53, 0.0]])
    t = gpu(a)
    idx, prob = A.sample(t, uniforms=torch.from_numpy(u).to(DEV))
    check_samples(t, a, u, idx, prob)
    i = idx[:, 0].cpu().numpy()
    assert i.min() == n // 4 and i.max() == n - n // 4 - 1 and i[0] == n // 4 and i[1] == n - n // 4 - 1


def test_sampling_a_permuted_view_returns_logical_multi_indices():
    rng = np.random.default_rng(13)
    a = crand(rng, (2,) * 20)
    perm = list(rng.permutation(20))
    t = gpu(a).permute(perm)
    u = rng.random(2000)
    idx, prob = A.sample(t, uniforms=torch.from_numpy(u).to(DEV))
    assert idx.shape == (2000, 20)
    check_samples(t, a.reshape(-1), u, idx, prob)
    ap = a.transpose(perm)
    total = sq(a).sum()
    got = sq(ap[tuple(idx.cpu().numpy().T)]) / total           # amps[tuple(idx)] has the returned probability
    assert np.abs(got - prob.cpu().numpy()).max() <= tol(a.size) * got.max()


def chi_square(counts, p, m):
    e = m * p
    return float(((counts - e) ** 2 / e).sum())


def test_generator_path_is_reproducible_and_follows_the_distribution():
    rng = np.random.default_rng(17)
    a = crand(rng, 2 ** 10)
    t = gpu(a)
    g = torch.Generator(device=DEV)
    g.manual_seed(1234)
    idx1, p1 = A.sample(t, 10 ** 6, generator=g)
    g.manual_seed(1234)
    idx2, p2 = A.sample(t, 10 ** 6, generator=g)
    assert torch.equal(idx1, idx2) and torch.equal(p1, p2)
    p = sq(a) / sq(a).sum()
    counts = np.bincount(idx1[:, 0].cpu().numpy(), minlength=a.size)
    dof = a.size - 1
    chi2 = chi_square(counts, p, 10 ** 6)
    print(f"chi-square {chi2:.1f}, dof {dof}, bound {dof + 6 * np.sqrt(2 * dof):.1f}")
    assert chi2 <= dof + 6 * np.sqrt(2 * dof)
    assert abs(A.linear_xeb(p1, 10) - (a.size * (p ** 2).sum() - 1)) < 0.05


# ---- marginals ----------------------------------------------------------------------------------------------------------
def oracle_marginal(a_logical, keep):
    p = sq(a_logical)
    drop = tuple(d for d in range(p.ndim) if d not in keep)
    red = p.sum(axis=drop) if drop else p
    left = [d for d in range(p.ndim) if d in keep]              # order of the surviving axes
    return red.transpose([left.index(d) for d in keep]) if keep else red


KEEPS_20 = {"fastest5": [15, 16, 17, 18, 19], "slowest5": [0, 1, 2, 3, 4], "mixed8": [1, 4, 6, 9, 12, 13, 17, 19],
            "all": list(range(20)), "none": [], "reordered": [18, 2, 11]}


@pytest.mark.parametrize("permuted", [False, True])
@pytest.mark.parametrize("name", sorted(KEEPS_20))
def test_marginals_of_a_20_qubit_state(name, permuted):
    rng = np.random.default_rng(19)
    a = crand(rng, (2,) * 20)
    t = gpu(a)
    if permuted:
        perm = list(rng.permutation(20))
        t, a = t.permute(perm), a.transpose(perm)
    keep = KEEPS_20[name]
    want = oracle_marginal(a, keep)
    got = A.marginal_probabilities(t, keep)
    assert got.dtype == torch.float64 and tuple(got.shape) == tuple(want.shape)
    total = sq(a).sum()
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"{name} permuted={permuted}: max err {err / total:.3e} tol {tol(a.size):.3e}")
    assert err <= tol(a.size) * total
    norm = A.marginal_probabilities(t, keep, normalize=True)
    assert abs(float(norm.sum()) - 1.0) <= tol(a.size)
    assert np.abs(norm.cpu().numpy() - want / total).max() <= 2 * tol(a.size)


@pytest.mark.parametrize("shape,keep,kind", [((1000, 2, 2, 2), [0], "c64"), ((3,) * 8, [1, 6], "c64"), ((3,) * 8, [6, 1], "c128"),
                                             ((1024, 2, 2, 2), [0], "c64"), ((2,) * 20, [3, 17, 0], "c128"),
                                             ((4, 8, 2, 16, 4, 2), [3, 0], "c64")])
def test_marginals_of_other_shapes(shape, keep, kind):
    rng = np.random.default_rng(23)
    a = crand(rng, shape, kind)
    want = oracle_marginal(a, keep)
    got = A.marginal_probabilities(gpu(a), keep).cpu().numpy()
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= tol(a.size) * sq(a).sum()
    want_kernel = 1 if all(e & (e - 1) == 0 for e in shape) and a.size >= 4096 else 0
    assert born.marginal_info(shape, gpu(a).stride(), keep, gpu(a).dtype)["kernel"] == want_kernel


# ---- determinism --------------------------------------------------------------------------------------------------------
def test_every_entry_point_is_bit_reproducible():
    rng = np.random.default_rng(29)
    a, b = gpu(crand(rng, 2 ** 22 + 3)), gpu(crand(rng, 2 ** 22 + 3))
    assert torch.equal(A.overlap(a, b, device=True), A.overlap(a, b, device=True))
    for x, y in zip(born.block_sums(a), born.block_sums(a)):
        assert torch.equal(x, y)
    u = torch.from_numpy(rng.random(100_000)).to(DEV)
    (i1, p1), (i2, p2) = A.sample(a, uniforms=u), A.sample(a, uniforms=u)
    assert torch.equal(i1, i2) and torch.equal(p1, p2)
    c = a[: 2 ** 22].reshape((2,) * 22).permute(list(rng.permutation(22)))
    for keep in ([0, 5, 9], [21, 20, 3, 4, 5, 6, 7, 8, 9, 10]):
        assert torch.equal(A.marginal_probabilities(c, keep), A.marginal_probabilities(c, keep))
    d = gpu(crand(rng, (3,) * 8))
    assert torch.equal(A.marginal_probabilities(d, [1, 6]), A.marginal_probabilities(d, [1, 6]))
    # block sums and their prefix against the oracle; the prefix only grows where a block is non-zero
    bs, prefix = born.block_sums(a)
    plan = born.born_plan(a.numel())
    p = np.zeros(plan["n_blocks"] << plan["block_bits"])
    p[: a.numel()] = sq(a.cpu().numpy())
    want = p.reshape(plan["n_blocks"], -1).sum(axis=1)
    assert np.abs(bs.cpu().numpy() - want).max() <= tol(2 ** plan["block_bits"]) * want.max()
    assert np.abs(prefix.cpu().numpy() - np.cumsum(want)).max() <= tol(a.numel()) * want.sum()
    assert (prefix[1:] >= prefix[:-1]).all()


# ---- end to end on the committed fixtures ---------------------------------------------------------------------------------
def test_n12_contraction_feeds_norm_marginals_and_sampling():
    case = load_case(os.path.join(GOLDEN, "n12_dense.npz"))
    raw = A.tensor_contraction(case.fresh_tensors(device=DEV), case.scheme)
    gold = case.arrays["raw"].reshape(raw.shape)
    pg = sq(gold)
    total = pg.sum()
    assert abs(A.norm2(raw) - total) <= 1e-5 * total
    for q in range(raw.dim()):
        got = A.marginal_probabilities(raw, [q]).cpu().numpy()
        assert np.abs(got - oracle_marginal(gold, [q])).max() <= 1e-5 * total
    g = torch.Generator(device=DEV)
    g.manual_seed(99)
    m = 10 ** 5
    idx, prob = A.sample(raw, m, generator=g)
    flat = memory_index(idx.cpu().numpy(), raw.contiguous())
    counts = np.bincount(flat, minlength=pg.size)
    dof = pg.size - 1
    chi2 = chi_square(counts, pg.reshape(-1) / total, m)
    print(f"n12 chi-square {chi2:.1f}, dof {dof}, bound {dof + 6 * np.sqrt(2 * dof):.1f}")
    assert dof == 4095 and chi2 <= dof + 6 * np.sqrt(2 * dof)


def test_n30_full_size_state_is_consumed_in_its_permuted_layout():
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 24e9:
        pytest.skip(f"needs 24 GB of free device memory for the 2^30-amplitude state and its contraction, {free / 1e9:.1f} GB free")
    case = load_case(os.path.join(GOLDEN, "n30_dense.npz"))
    raw = A.tensor_contraction(case.fresh_tensors(device=DEV), case.scheme)
    assert raw.numel() == 2 ** 30
    final = raw.permute(case.meta["permute_dims"])              # the view the reference returns (simulation.py:115-116)
    assert not final.is_contiguous()
    n = raw.numel()
    plan = born.born_plan(n)
    info = born.marginal_info(final.shape, final.stride(), list(range(10)))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    norm = A.norm2(final)
    marg = A.marginal_probabilities(final, list(range(10)))
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    # the workspaces the plans report plus the outputs (4 and 1024 doubles); the allocator rounds each of the four tensors to 512 B
    allowed = plan["workspace_bytes"] + info["workspace_bytes"] + 4 * 8 + 1024 * 8 + 4 * 512
    print(f"n30: norm2 {norm!r} (fixture {case.meta['norm2']!r}), device memory rise {rise} B, allowed {allowed} B")
    assert rise <= allowed                                      # far below the 8 GiB a copy of the state would take
    assert abs(norm - case.meta["norm2"]) < 1e-5
    assert tuple(marg.shape) == (2,) * 10
    assert abs(float(marg.sum()) - norm) <= tol(n) * norm
