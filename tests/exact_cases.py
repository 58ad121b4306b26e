"""The case table of the exact-integer contraction tests, shared by test_exact_contraction_cpu.py (range check, path coverage)
and test_exact_contraction_gpu.py (the runs).  A case is one launch: its equations, shapes, operand class, dtype / precision,
the environment switches it runs under, and -- in PLANNED -- the planner's answer it has to get: (kernel, arith, k_bits, k2_bits,
k3_bits) exactly, which name the kernel family and its arithmetic; tile sizes and tile counts are tuning and are pinned only
where a path is defined by them (path_properties: the FULL instantiations, artn_k_wide, the second launch of the extent GEMM,
the row-streaming shapes).  The planner plans for 256 CUs when no device is visible, the CU count of an MI355X, so the same
table is checked on the host (test_planned_paths) and before every comparison on the GPU.

Operands are drawn by exact_contraction.draw_chain from the case's seed; `operands(case)` caches nothing itself (the GPU file
caches operands and references per case with functools.lru_cache)."""
import functools
import os

import numpy as np

import exact_contraction as X

KERNEL_GENERIC, KERNEL_BITS, KERNEL_GEMM, KERNEL_PGEMM, KERNEL_XGEMM = 0, 1, 2, 4, 5
INFO_FIELDS = ("kernel", "arith", "k_bits", "k2_bits", "k3_bits")
BITS, GENERIC = {"ARTN_FORCE_BITS": "1"}, {"ARTN_FORCE_GENERIC": "1"}


class Case(dict):
    """name, kind ('step' | 'pair' | 'gather' | 'row_pairs' | 'acc_step' | 'acc_pair' | 'view'), cls, dtype ('complex64' | 'complex128'), precision (None |
    'bf16'), eqs, a_shape, b_shapes, env, seed, plus what a kind needs (rows, view); views: {'a' | 'b' | 'out' -> view kind}
    of a case whose operands are views (view_cases; kind 'view': the three older cases, `view` on a and b)"""
    __getattr__ = dict.__getitem__

    @property
    def arith_kind(self):
        return "bf16" if self.precision == "bf16" else self.dtype


def _case(name, kind, cls, eqs, a_shape, b_shapes, dtype="complex64", precision=None, env=None, seed=0, **more):
    return Case(name=name, kind=kind, cls=cls, dtype=dtype, precision=precision, eqs=tuple(eqs), a_shape=tuple(a_shape),
                b_shapes=tuple(tuple(s) for s in b_shapes), env=dict(env or {}), seed=seed, **more)


# ---- equations -----------------------------------------------------------------------------------------------------------
def bit_step(seed, k, n, ra, insert=False):
    """k contracted bits of a 2^ra-element operand, n new bits, every label order shuffled (test_random_bit_steps); insert:
    the new bits keep the old ones in order (test_shrinking_single_steps_on_narrow_three_product_blocks)"""
    rng = np.random.default_rng(seed)
    la = [chr(65 + x) for x in range(ra)]
    kl = list(rng.choice(la, size=k, replace=False))
    nl = [chr(97 + x) for x in range(n)]
    lb = kl + nl
    rng.shuffle(lb)
    if insert:
        lo = [x for x in la if x not in kl]
        for x in nl:
            lo.insert(int(rng.integers(0, len(lo) + 1)), x)
    else:
        lo = [x for x in la if x not in kl] + nl
        rng.shuffle(lo)
    return "".join(la) + "," + "".join(lb) + "->" + "".join(lo), (2,) * ra, (2,) * len(lb)


def bit_pair(seed, k1, n1, k2, n2, ra, batch=0, mode=0):
    """Two consecutive bit steps on one operand (test_random_fused_pairs); batch: extent of a leading batch label z, carried by
    both small operands (mode 0), the first only (1) or the second only (2) (test_fused_pairs_with_batch_labels)"""
    rng = np.random.default_rng(seed)
    la = [chr(65 + x) for x in range(ra)]
    kl1 = list(rng.choice(la, size=k1, replace=False))
    nl1 = [chr(97 + x) for x in range(n1)]
    lb1 = kl1 + nl1
    rng.shuffle(lb1)
    lo1 = [x for x in la if x not in kl1] + nl1
    rng.shuffle(lo1)
    kl2 = list(rng.choice(lo1, size=k2, replace=False))
    nl2 = [chr(110 + x) for x in range(n2)]
    lb2 = kl2 + nl2
    rng.shuffle(lb2)
    lo2 = [x for x in lo1 if x not in kl2] + nl2
    rng.shuffle(lo2)
    if batch:
        la, lo1, lo2 = ["z"] + la, ["z"] + lo1, ["z"] + lo2
        lb1 = (["z"] if mode in (0, 1) else []) + lb1
        lb2 = (["z"] if mode in (0, 2) else []) + lb2
    shape = lambda labs: tuple(batch if x == "z" else 2 for x in labs)
    eq1 = "".join(la) + "," + "".join(lb1) + "->" + "".join(lo1)
    eq2 = "".join(lo1) + "," + "".join(lb2) + "->" + "".join(lo2)
    return (eq1, eq2), shape(la), (shape(lb1), shape(lb2))


def gemm_step(seed, m, n, k, batch=0):
    """m + k bits against k + n bits, label tuples, every order shuffled (test_gemm_kernel_steps)"""
    rng = np.random.default_rng(seed)
    ml, kl, nl = [f"m{x}" for x in range(m)], [f"k{x}" for x in range(k)], [f"n{x}" for x in range(n)]
    la, lb, lo = ml + kl, kl + nl, ml + nl
    rng.shuffle(la), rng.shuffle(lb), rng.shuffle(lo)
    sa, sb = [2] * len(la), [2] * len(lb)
    if batch:
        la, lb, lo = ["z"] + la, ["z"] + lb, ["z"] + lo
        sa, sb = [batch] + sa, [batch] + sb
    return (tuple(la), tuple(lb), tuple(lo)), tuple(sa), tuple(sb)


def extent_step(seed, M, Nn, K, H=None, rows_last=False):
    """labels with the given extents (dicts), every order shuffled; rows_last: the result's fastest label is a row label"""
    rng = np.random.default_rng(seed)
    H = H or {}
    ext = {**M, **Nn, **K, **H}
    la, lb, lo = list(M) + list(K) + list(H), list(Nn) + list(K) + list(H), list(M) + list(Nn) + list(H)
    for lst in (la, lb, lo):
        rng.shuffle(lst)
    if rows_last:
        last_m = max(i for i, x in enumerate(lo) if x in M)
        lo[last_m], lo[-1] = lo[-1], lo[last_m]
    return (tuple(la), tuple(lb), tuple(lo)), tuple(ext[x] for x in la), tuple(ext[x] for x in lb)


def gather_step(na, nb, n, free, kb, nn):
    """the shapes of test_contract_gathered: rows z lead both operands and the result"""
    la = ["z"] + [chr(65 + x) for x in range(free + kb)]
    kl = la[1:1 + kb]
    nl = [chr(97 + x) for x in range(nn)]
    lb = ["z"] + kl[::-1] + nl
    lo = ["z"] + [x for x in la[1:] if x not in kl] + nl
    eq = "".join(la) + "," + "".join(lb) + "->" + "".join(lo)
    return eq, (na,) + (2,) * (len(la) - 1), (nb,) + (2,) * (len(lb) - 1)


BIT_STEPS = [(1, 1, 12), (2, 0, 13), (3, 3, 14), (4, 4, 15), (5, 5, 15), (6, 6, 16), (4, 7, 13), (6, 2, 16), (1, 6, 12), (5, 1, 14),
             (7, 3, 15), (8, 4, 15), (8, 0, 14)]   # test_random_bit_steps' list, A up to 2^16 elements ((7, 6, 16): a GEMM step, below)
N30_PAIRS = [(75, 78), (80, 83), (88, 90), (93, 97), (101, 104), (108, 112), (123, 125), (128, 131)]   # one per (k1, k2) of the n30 chain
GEMM_STEPS = [(11, 11, 9, 0), (12, 11, 7, 0), (11, 12, 8, 0), (13, 6, 8, 0), (9, 9, 9, 5), (10, 10, 11, 0), (5, 5, 14, 0), (8, 8, 7, 3)]


@functools.lru_cache(maxsize=None)
def _n30_steps():
    from artensor_amd.fixtures import load_case
    from helpers import GOLDEN, dense_scheme_shapes
    return dense_scheme_shapes(load_case(os.path.join(GOLDEN, "n30_dense.npz")))


def n30_pair(n, m, max_log2):
    from helpers import shrink_pair
    steps = _n30_steps()
    (eq1, sa, sb1), (eq2, _, sb2) = steps[n], steps[m]
    e1, a_s, b1_s, e2, b2_s = shrink_pair(eq1, sa, sb1, eq2, sb2, max_log2=max_log2)
    return (e1, e2), a_s, (b1_s, b2_s)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> Case, in the order the GPU file runs them"""
    out = []
    both = ("wide", "dense")
    # single bit steps on artn_k_bits (ARTN_FORCE_BITS): k = 1..8 (k > 6: the chained <6, 0, true> form), 0..7 new bits, growing,
    # size-preserving and shrinking; k = 5, 6 with at most 4 result bits in the tile: the narrow three-product form
    for k, n, ra in BIT_STEPS:
        eq, sa, sb = bit_step(100 * k + n, k, n, ra)
        for cls in both:
            out.append(_case(f"bits_k{k}_n{n}_{cls}", "step", cls, [eq], sa, [sb], env=BITS, seed=100 * k + n))
    for k, n, ra, seed in [(5, 2, 16, 9), (6, 1, 16, 3), (5, 0, 16, 4)]:
        eq, sa, sb = bit_step(950 + seed, k, n, ra, insert=True)
        for cls in both:
            out.append(_case(f"narrow3_k{k}_n{n}_{cls}", "step", cls, [eq], sa, [sb], env=BITS, seed=950 + seed))
    # arith == 2: the same kernel on bfloat16 operands
    for k, n, ra in [(4, 4, 15), (6, 6, 16), (8, 4, 15)]:
        eq, sa, sb = bit_step(100 * k + n, k, n, ra)
        out.append(_case(f"bits_k{k}_n{n}_bf16", "step", "bf16", [eq], sa, [sb], precision="bf16", env=BITS, seed=100 * k + n))
    # FULL / artn_k_alt instantiations: 2^22 elements, 2^12-element tiles, 1 024 of them; one step and one pair per k1
    for k in (3, 4, 5, 6):
        eq, sa, sb = bit_step(7 * k, k, k, 22)
        out.append(_case(f"full_step_k{k}", "step", both[k % 2], [eq], sa, [sb], seed=7 * k, full=True))
        eqs, sa, sbs = bit_pair(170 + k, k, k, 9 - k, 9 - k, 22)
        out.append(_case(f"full_pair_k{k}_{9 - k}", "pair", both[(k + 1) % 2], eqs, sa, sbs, seed=170 + k, full=True))
    # fused pairs: the (k1, k2) of the n30 m14 chain on its own label orders (2^18-element surrogates) ...
    for n, m in N30_PAIRS:
        eqs, sa, sbs = n30_pair(n, m, 14 if (n, m) == (75, 78) else 18)   # (75/78 adds 6 bits: a 2^20-element result from 2^14)
        for cls in both:
            out.append(_case(f"n30_pair_{n}_{m}_{cls}", "pair", cls, eqs, sa, sbs, env=BITS, seed=n))
    # ... and (5,5), (6,4), (4,5), (2,5), (3,6) on random orders, growing and shrinking stages, 2^15..2^18 elements ((6,6), (5,6) and
    # (6,5) fuse on artn_k_wide only: one default-planned case below, the small ones in WIDE_PAIRS for tests/exact_worker.py)
    for k1, n1, k2, n2, ra in [(5, 5, 5, 5, 17), (6, 6, 4, 4, 18), (4, 4, 5, 5, 16), (2, 2, 5, 5, 15), (3, 3, 6, 6, 17),
                               (5, 6, 5, 4, 16), (6, 5, 4, 5, 17), (2, 3, 5, 4, 16)]:
        eqs, sa, sbs = bit_pair(1000 * k1 + 100 * n1 + 10 * k2 + n2, k1, n1, k2, n2, ra)
        for cls in both:
            out.append(_case(f"pair_{k1}{n1}_{k2}{n2}_{cls}", "pair", cls, eqs, sa, sbs, env=BITS, seed=10 * k1 + k2))
    # ... with a batch label in both small operands, the first only, the second only; ragged extent 3 and 7
    for (k1, k2, ra, batch, mode) in [(5, 5, 15, 3, 0), (6, 4, 15, 3, 1), (4, 5, 14, 7, 2), (3, 6, 15, 2, 0), (2, 5, 14, 3, 1)]:
        eqs, sa, sbs = bit_pair(500 + 10 * k1 + k2, k1, k1, k2, k2, ra, batch=batch, mode=mode)
        out.append(_case(f"pair_{k1}_{k2}_batch{batch}_mode{mode}", "pair", both[mode % 2], eqs, sa, sbs, env=BITS, seed=500 + k1))
    # store-phase accumulate of a pair (artn_contract2_acc): complex64 (3M pairs on 2^12-element tiles, the FULL instantiations --
    # four-product pairs add only in launches big enough for non-temporal loads, 2^24 elements) and complex128 (every tile shape)
    for n, m in [(93, 97), (108, 112)]:
        eqs, sa, sbs = n30_pair(n, m, 22)
        out.append(_case(f"acc_pair_{n}_{m}", "acc_pair", both[n % 2], eqs, sa, sbs, seed=300 + n))
    for n, m, cls in [(80, 83, "wide128"), (108, 112, "dense")]:
        eqs, sa, sbs = n30_pair(n, m, 18)
        out.append(_case(f"acc_pair_{n}_{m}_c128_{cls}", "acc_pair", cls, eqs, sa, sbs, dtype="complex128", seed=400 + n))
    # store-phase accumulate of a single step (artn_contract_acc): the big 3M steps of the n30 scheme on 2^22-element surrogates
    # (12 / 12 tiles: the FULL instantiations), and artn_k_bits128 in complex128
    from helpers import shrink_step
    for n in (108, 139, 172):
        eq, sa, sb = shrink_step(*_n30_steps()[n], max_log2=22)
        out.append(_case(f"acc_step_{n}", "acc_step", both[n % 2], [eq], sa, [sb], seed=200 + n, full=True))
    eq, sa, sb = bit_step(606, 6, 6, 16)
    for cls in ("wide128", "dense"):
        out.append(_case(f"acc_step_c128_{cls}", "acc_step", cls, [eq], sa, [sb], dtype="complex128", seed=607))
    # artn_k_wide as the planner takes it by default: 6 + 6 contracted bits, 2^23 elements = 2 048 tiles of 2^12
    eqs, sa, sbs = bit_pair(6666, 6, 6, 6, 6, 23)
    out.append(_case("wide_pair_66_default", "pair", "dense", eqs, sa, sbs, seed=6666, wide=True))
    # row gather (artn_contract_gather): 1, 7 and 1 000 rows out of a few (repeats), k = 8 and 7 > 6 (the GEMM kernel's gather)
    for na, nb, n, free, kb, nn in [(7, 5, 1, 12, 3, 2), (16, 16, 7, 13, 4, 3), (3, 9, 1000, 10, 8, 3), (6, 3, 37, 9, 7, 5)]:
        eq, sa, sb = gather_step(na, nb, n, free, kb, nn)
        for cls in both:
            out.append(_case(f"gather_{n}rows_k{kb}_{cls}", "gather", cls, [eq], sa, [sb], seed=23 + n, rows=n))
    # row-pair GEMM (contract_row_pairs): 600 pairs out of 16 x 16 distinct rows -> one unbatched step and a row gather
    for cls in both:
        out.append(_case(f"row_pairs_{cls}", "row_pairs", cls, ["zABCDEFGHIJKL,zLKJIab->zABCDEFGHab"], (16,) + (2,) * 12, [(16,) + (2,) * 6],
                         seed=41, rows=600))
    # the two-operand GEMM: test_gemm_kernel_steps' list, the (7, 6, 16) bit step, a split-K closing step
    for i, (m, n, k, batch) in enumerate(GEMM_STEPS):
        eq, sa, sb = gemm_step(1000 * m + 10 * n + k, m, n, k, batch)
        for cls in (both if m + n + k <= 28 else both[i % 2:i % 2 + 1]):
            out.append(_case(f"gemm_m{m}_n{n}_k{k}_b{batch}_{cls}", "step", cls, [eq], sa, [sb], seed=1000 * m + 10 * n + k))
    eq, sa, sb = bit_step(706, 7, 6, 16)
    for cls in both:
        out.append(_case(f"gemm_bits_k7_n6_{cls}", "step", cls, [eq], sa, [sb], env=BITS, seed=706))
    eq, sa, sb = gemm_step(77, 6, 6, 14)   # 8 tiles of 2^14-term sums: contract() splits contracted labels off and sums the parts
    for cls in both:
        out.append(_case(f"gemm_split_k14_{cls}", "step", cls, [eq], sa, [sb], seed=77, split_k=True))
    eq, sa, sb = gemm_step(78, 10, 9, 9)
    for cls in both:   # operands that are views of bigger tensors: one index of an inner axis (GEMM), of the outermost and innermost (extent GEMM)
        out.append(_case(f"gemm_views_{cls}", "view", cls, [eq], sa, [sb], seed=78, view="inner"))
    out.append(_case("xgemm_views_dense", "view", "dense", [eq], sa, [sb], seed=79, view="ends"))
    # packed-operand GEMM: precision("bf16") from 2^9 contracted values, complex64 3M from 2^11
    eq, sa, sb = gemm_step(100, 12, 11, 9)
    out.append(_case("pgemm_bf16_m12_n11_k9", "step", "bf16", [eq], sa, [sb], precision="bf16", seed=100))
    eq, sa, sb = gemm_step(200, 12, 11, 11)
    out.append(_case("pgemm_c64_m12_n11_k11", "step", "dense", [eq], sa, [sb], seed=200))
    # extent GEMMs: general (3, 5, 6, 9 mixed with 2), the second launch for the last columns, row streaming in both shapes
    eq, sa, sb = extent_step(11, dict(m0=9, m1=5, m2=6, m3=2, m4=3, m5=5, m6=2), dict(n0=3, n1=6, n2=2), dict(k0=3, k1=5, k2=2))
    for cls in both:
        out.append(_case(f"xgemm_mixed_{cls}", "step", cls, [eq], sa, [sb], seed=11))
    out.append(_case("xgemm_mixed_c128_wide128", "step", "wide128", [eq], sa, [sb], dtype="complex128", seed=11))
    out.append(_case("xgemm_mixed_c128_dense", "step", "dense", [eq], sa, [sb], dtype="complex128", seed=11))
    eq, sa, sb = extent_step(12, dict(m0=6, m1=9, m2=5, m3=2, m4=3), dict(n0=5, n1=3), dict(k0=6, k1=3), dict(h0=5))
    out.append(_case("xgemm_batch_dense", "step", "dense", [eq], sa, [sb], seed=12))
    nl = ("n4", "n3", "n2", "n1", "n0")
    eq = (("m1", "k0", "m0"), nl[:1] + ("k0",) + nl[1:], ("n4", "n3", "n2", "n1", "n0", "m1", "m0"))
    for cls in both:   # 243 columns = 2 tiles of 96 + a launch of 64
        out.append(_case(f"xgemm_tail_{cls}", "step", cls, [eq], (600, 9, 250), [(3, 9, 3, 3, 3, 3)], seed=606, rereads=3))
    for kk, nn, form, m_tile_bits in [(5, 16, 0, 6), (32, 32, 1, 6), (40, 48, 0, 4), (7, 41, 1, 4)]:
        m1, m0 = 150, 221
        if form == 0:
            eq, sa, sb = (("k", "m1", "m0"), ("n", "k"), ("n", "m1", "m0")), (kk, m1, m0), (nn, kk)
        else:
            eq, sa, sb = (("m1", "m0", "k"), ("k", "n"), ("n", "m1", "m0")), (m1, m0, kk), (kk, nn)
        out.append(_case(f"xrow_k{kk}_n{nn}_form{form}", "step", both[form], [eq], sa, [sb], seed=2026 + kk, m_tile_bits=m_tile_bits))
    eq = (tuple("abcdKefgLhijk"), ("x", "K", "L", "y"), ("y", "x") + tuple("abcdefghijk"))
    out.append(_case("xrow64_bond3", "step", "wide", [eq], (3,) * 13, [(3,) * 4], seed=2027, m_tile_bits=6))
    # complex128: artn_k_gemm128, the bits128 pair, the strided kernel
    for k, n, ra in [(4, 4, 15), (6, 6, 16), (8, 4, 15)]:
        eq, sa, sb = bit_step(100 * k + n, k, n, ra)
        for cls in ("wide128", "dense"):
            out.append(_case(f"gemm128_k{k}_n{n}_{cls}", "step", cls, [eq], sa, [sb], dtype="complex128", env=BITS, seed=100 * k + n))
    eq, sa, sb = bit_step(606, 6, 6, 16)
    for cls in ("wide128", "dense"):   # (a single step on artn_k_bits128)
        out.append(_case(f"bits128_step_k6_n6_{cls}", "step", cls, [eq], sa, [sb], dtype="complex128", seed=606))
    for n, m in [(75, 78), (93, 97), (108, 112), (128, 131)]:
        eqs, sa, sbs = n30_pair(n, m, 14 if (n, m) == (75, 78) else 18)
        for cls in ("wide128", "dense"):
            out.append(_case(f"bits128_pair_{n}_{m}_{cls}", "pair", cls, eqs, sa, sbs, dtype="complex128", seed=n))
    for k, n, ra in [(3, 3, 14), (7, 3, 15)]:
        eq, sa, sb = bit_step(100 * k + n, k, n, ra)
        for cls in ("wide128", "dense"):
            out.append(_case(f"generic128_k{k}_n{n}_{cls}", "step", cls, [eq], sa, [sb], dtype="complex128", env=GENERIC, seed=100 * k + n))
    # the generic strided kernel in complex64 (ARTN_FORCE_GENERIC)
    for k, n, ra in [(3, 3, 14), (7, 3, 15)]:
        eq, sa, sb = bit_step(100 * k + n, k, n, ra)
        out.append(_case(f"generic_k{k}_n{n}", "step", both[k % 2], [eq], sa, [sb], env=GENERIC, seed=100 * k + n))
    out.append(_case("generic_extent4", "step", "dense", ["abcdefg,gcx->abdefx"], (4,) * 7, [(4, 4, 4)], env=GENERIC, seed=5))
    out += view_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    return {c.name: c for c in out}


VIEWS = {
    "permuted": dict(a="permuted", b="permuted"), "inner": dict(a="inner", b="inner"), "ends": dict(a="ends", b="ends"),
    "gap": dict(a="gap"), "offset16": dict(a="offset16", b="offset16", out="offset16"),
    "offset8a": dict(a="offset8"), "offset8b": dict(b="offset8"), "offset8c": dict(out="offset8"),
}


def view_cases():
    """The contraction kernels on operand views, storage offsets and 8-byte bases (view kinds: above view_of), at the smallest
    shapes of the tables above; every launch writes into a result buffer inside sentinel margins"""
    out = []
    both = ("wide", "dense")

    def add(name, kind, cls, eqs, sa, sbs, view, views=None, **more):
        out.append(_case(f"v_{name}_{view}_{cls}", kind, cls, eqs, sa, sbs, views=views or VIEWS[view], **more))
    # artn_k_bits, single steps with k = 1, 4, 6: every view kind
    for k, n, ra in [(1, 1, 12), (4, 4, 15), (6, 6, 16)]:
        eq, sa, sb = bit_step(100 * k + n, k, n, ra)
        for view in VIEWS:
            for cls in both:
                add(f"bits_k{k}", "step", cls, [eq], sa, [sb], view, env=BITS, seed=100 * k + n)
    # artn_k_bits128 (a single step) and the f64 GEMM
    eq, sa, sb = bit_step(606, 6, 6, 16)
    for view in ("permuted", "gap", "offset16"):
        for cls in ("wide128", "dense"):
            add("bits128_k6", "step", cls, [eq], sa, [sb], view, dtype="complex128", seed=606)
    eq, sa, sb = bit_step(404, 4, 4, 15)
    for view in ("permuted", "offset16"):
        for cls in ("wide128", "dense"):
            add("gemm128_k4", "step", cls, [eq], sa, [sb], view, dtype="complex128", env=BITS, seed=404)
    # the two-operand GEMM: an 8-byte B is replanned inside artn_contract (the kernel moves both operands in 16-byte lanes)
    m, n, k, batch = GEMM_STEPS[-1]
    eq, sa, sb = gemm_step(1000 * m + 10 * n + k, m, n, k, batch)
    for view in ("gap", "offset16", "offset8b"):
        for cls in both:
            add(f"gemm_m{m}_n{n}_k{k}_b{batch}", "step", cls, [eq], sa, [sb], view, seed=1000 * m + 10 * n + k)
    eq, sa, sb = bit_step(706, 7, 6, 16)
    for cls in both:
        add("gemm_bits_k7", "step", cls, [eq], sa, [sb], "offset8b", env=BITS, seed=706)
    # the extent GEMM and its row-streaming form
    eq, sa, sb = extent_step(11, dict(m0=9, m1=5, m2=6, m3=2, m4=3, m5=5, m6=2), dict(n0=3, n1=6, n2=2), dict(k0=3, k1=5, k2=2))
    for n_view, view in enumerate(("permuted", "offset16", "offset8b")):
        add("xgemm_mixed", "step", both[n_view % 2], [eq], sa, [sb], view, seed=11)
    for kk, nn, form, m_tile_bits in [(5, 16, 0, 6), (7, 41, 1, 4)]:
        m1, m0 = 150, 221
        if form == 0:
            eq, sa, sb = (("k", "m1", "m0"), ("n", "k"), ("n", "m1", "m0")), (kk, m1, m0), (nn, kk)
        else:
            eq, sa, sb = (("m1", "m0", "k"), ("k", "n"), ("n", "m1", "m0")), (m1, m0, kk), (kk, nn)
        for view in ("offset16", "offset8b"):
            add(f"xrow_k{kk}_n{nn}", "step", both[form], [eq], sa, [sb], view, seed=2026 + kk, m_tile_bits=m_tile_bits)
    # the packed-operand GEMM, bf16 and complex64
    eq, sa, sb = gemm_step(100, 12, 11, 9)
    for view in ("inner", "offset16"):
        add("pgemm_bf16", "step", "bf16", [eq], sa, [sb], view, precision="bf16", seed=100)
    eq, sa, sb = gemm_step(200, 12, 11, 11)
    for view in ("inner", "offset16"):
        add("pgemm_c64", "step", "dense", [eq], sa, [sb], view, seed=200)
    # fused pairs 5 + 3 and 6 + 4: a non-contiguous A is declined by contract2 and runs as two launches, an offset one fuses
    for k1, k2, ra in [(5, 3, 16), (6, 4, 17)]:
        eqs, sa, sbs = bit_pair(1000 * k1 + 10 * k2, k1, k1, k2, k2, ra)
        for view, cls in [("inner", "wide"), ("gap", "dense"), ("offset16", "wide"), ("offset16", "dense")]:
            # (a pair's small operands stay as they are: only A decides whether contract2 fuses)
            add(f"pair_{k1}_{k2}", "pair", cls, eqs, sa, sbs, view, views=dict(a=view), env=BITS, seed=10 * k1 + k2)
    # gathered steps and row pairs: source rows out of an inner view; an 8-byte A goes through the callers' explicit gather
    eq, sa, sb = gather_step(7, 5, 7, 12, 3, 2)
    for view, cls in [("inner", "wide"), ("inner", "dense"), ("offset8a", "dense")]:
        add("gather_7rows_k3", "gather", cls, [eq], sa, [sb], view, seed=30, rows=7)
    for view, cls in [("inner", "wide"), ("inner", "dense"), ("offset8a", "wide")]:
        add("row_pairs", "row_pairs", cls, ["zABCDEFGHIJKL,zLKJIab->zABCDEFGHab"], (16,) + (2,) * 12, [(16,) + (2,) * 6], view,
            seed=41, rows=600)
    # store-phase accumulation into a contiguous buffer at a storage offset: complex128 through the entry points themselves,
    # complex64 through tensor_contraction(accumulate_into=), whose fallback adds with artn_axpy_c64 (an 8-byte accumulator
    # always ends there: artn_contract_acc refuses it)
    eq, sa, sb = bit_step(606, 6, 6, 16)
    for cls in ("wide128", "dense"):
        add("acc_step_c128", "acc_step", cls, [eq], sa, [sb], "offset16", dtype="complex128", seed=607)
    eqs, sa, sbs = n30_pair(80, 83, 16)
    for cls in ("wide128", "dense"):
        add("acc_pair_80_83_c128", "acc_pair", cls, eqs, sa, sbs, "offset16", dtype="complex128", seed=480)
    for view in ("offset16", "offset8c"):
        for cls in both:
            add("acc_step_k6", "acc_step", cls, [eq], sa, [sb], view, env=BITS, seed=608, wrapper=True)
    return out


def wide_pairs():
    """The pairs only artn_k_wide fuses -- 11 or 12 contracted bits -- at 2^18 elements, both classes: cases for a process started
    with ARTN_WIDE=1 ARTN_WIDE_MIN_TILES=1 (tests/exact_worker.py; by default the kernel is taken from 2 048 tiles on)"""
    out = []
    for k1, k2 in [(6, 6), (5, 6), (6, 5)]:
        eqs, sa, sbs = bit_pair(6000 + 10 * k1 + k2, k1, k1, k2, k2, 18)
        for cls in ("wide", "dense"):
            out.append(_case(f"wide_pair_{k1}{k2}_{cls}", "pair", cls, eqs, sa, sbs, seed=6000 + 10 * k1 + k2, wide=True))
    return out


def is_wide(info):
    """artn_k_wide: the only plans with one workgroup per CU and four 32 KiB LDS regions (tests/wide_worker.py)"""
    return info is not None and info["lds_bytes"] >= 4 * 32768 and info["grid"] <= 256


def path_properties(case, info):
    """What a case's path needs beyond PLANNED, asserted on the planner's whole answer"""
    if case.get("full"):     # FULL / artn_k_alt instantiations
        assert info["n_tiles"] >= 64 and info["tile_in_bits"] == 12 and info["tile_out_bits"] == 12, (case.name, info)
    if "wide" in case:
        assert is_wide(info) == case.wide, (case.name, info["lds_bytes"], info["grid"])
    elif info is not None and info["kernel"] == KERNEL_BITS and case.dtype == "complex64":
        assert not is_wide(info), case.name
    if "rereads" in case:    # extent GEMM: full column tiles plus the second launch for the last columns
        assert info["a_rereads"] == case.rereads, (case.name, info["a_rereads"])
    if "m_tile_bits" in case:   # 6: artn_k_xrow64, 4: artn_k_xrow
        assert info["m_tile_bits"] == case.m_tile_bits, (case.name, info["m_tile_bits"])


class environment:
    """the case's switches in os.environ for the length of a `with` (they are read per call by the library)"""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        return False


# ---- operand views -------------------------------------------------------------------------------------------------------------
# A view is a recipe on a flat base of `offset + prod(base_shape)` elements: flat[offset:].reshape(base_shape), its dims
# permuted by `perm`, then indexed with `index` -- the same three steps in numpy (the reference) and in torch (the device
# operand), so the two share slicing syntax and nothing else.  View kinds, per operand ('a', 'b': the first small operand,
# 'out': the result buffer or accumulator):
#   permuted  a: base.permute(p) of a contiguous base, p drawn from the case's seed: dense, dims in another memory order; b: transposed
#   inner     one index of an axis of extent 2 put in after five (a) / four (b) of the operand's own axes (fewer: before the last)
#   ends      big_a[1, ..., 0] and big_b[..., 1]
#   gap       a: base[..., ::2, ...] on its first free and its first contracted axis (never the last axis): every stride a power of
#             two, one address bit skipped at each of the two; b as it is
#   offset16  a contiguous operand 16 j bytes into its storage, j = 3 (a), 5 (b), 7 (out)
#   offset8   complex64 only: a contiguous operand 8 bytes into its storage
VIEW_KINDS = ("permuted", "inner", "ends", "gap", "offset16", "offset8")
OFFSET16_J = {"a": 3, "b": 5, "out": 7}


class Recipe(dict):
    """base_shape, perm, index, offset (elements)"""
    __getattr__ = dict.__getitem__

    @property
    def numel(self):
        """elements of the flat base, offset included"""
        return self.offset + int(np.prod(self.base_shape, dtype=np.int64))


def _recipe(base_shape, perm=None, index=(), offset=0):
    base_shape = tuple(int(x) for x in base_shape)
    return Recipe(base_shape=base_shape, perm=tuple(perm) if perm is not None else tuple(range(len(base_shape))), index=tuple(index), offset=offset)


def apply_view(r, flat, shift=0):
    """the view of recipe r in a flat numpy array or torch tensor; shift: elements in front of the base (a guard margin)"""
    n = int(np.prod(r.base_shape, dtype=np.int64))
    x = flat[shift + r.offset:shift + r.offset + n].reshape(r.base_shape)
    x = x.permute(*r.perm) if hasattr(x, "permute") else x.transpose(r.perm)
    return x[r.index] if r.index else x


def _view_recipe(case, which, shape):
    views = {"a": case.view, "b": case.view} if case.kind == "view" else case.get("views", {})
    kind = views.get(which)
    nd = len(shape)
    itemsize = 16 if case.dtype == "complex128" else 8
    if kind is None:
        return _recipe(shape)
    assert kind in VIEW_KINDS, kind
    if kind == "inner" and which != "out":
        pos = min(5 if which == "a" else 4, nd - 1)
        return _recipe(shape[:pos] + (2,) + shape[pos:], index=(slice(None),) * pos + (1 if which == "a" else 0,))
    if kind == "ends" and which != "out":
        return _recipe((2,) + shape + (2,), index=(1, Ellipsis, 0)) if which == "a" else _recipe(shape + (2,), index=(Ellipsis, 1))
    if kind == "permuted" and which != "out":
        p = np.random.default_rng(case.seed + 7).permutation(nd) if which == "a" else np.arange(nd)[::-1]
        base = [0] * nd
        for i in range(nd):
            base[p[i]] = shape[i]     # base.permute(p).shape[i] == base.shape[p[i]]
        return _recipe(base, perm=[int(x) for x in p])
    if kind == "gap" and which == "a":
        la, lb, lo = X.labels(case.eqs[0])
        free = [n for n, x in enumerate(la[:-1]) if x not in lb]
        con = [n for n, x in enumerate(la[:-1]) if x in lb and x not in lo]
        axes = (free[0], con[0])
        return _recipe([2 * e if n in axes else e for n, e in enumerate(shape)],
                       index=tuple(slice(None, None, 2) if n in axes else slice(None) for n in range(max(axes) + 1)))
    if kind == "offset16":
        return _recipe(shape, offset=OFFSET16_J[which] * 16 // itemsize)
    if kind == "offset8":
        assert case.dtype == "complex64", "an 8-byte base exists for complex64 only"
        return _recipe(shape, offset=1)
    return _recipe(shape)     # (a kind that shapes one operand only leaves the others as they are)


def has_views(case):
    return case.kind == "view" or bool(case.get("views"))


def view_of(case):
    """{'a', 'b', 'out'} -> Recipe of the case's streamed operand, first small operand and result buffer (plain cases: the
    contiguous operand at offset 0)"""
    out_shape = result_shape(case)
    if case.kind in ("gather", "row_pairs"):   # (one result row per index pair)
        out_shape = (case.rows,) + out_shape[1:]
    return {"a": _view_recipe(case, "a", case.a_shape), "b": _view_recipe(case, "b", case.b_shapes[0]),
            "out": _view_recipe(case, "out", out_shape)}


def view_layout(r, itemsize):
    """(element strides, byte offset of the first element mod 16, contiguous) of a recipe's view, from numpy's own slicing of
    an array of that element size"""
    flat = np.empty(r.numel, dtype=np.complex128 if itemsize == 16 else np.complex64)
    v = apply_view(r, flat)
    first = v.__array_interface__["data"][0] - flat.__array_interface__["data"][0]
    return tuple(s // itemsize for s in v.strides), first % 16, bool(v.flags["C_CONTIGUOUS"])


def view_strides(case):
    """element strides of the views of a and b"""
    v = view_of(case)
    itemsize = 16 if case.dtype == "complex128" else 8
    return view_layout(v["a"], itemsize)[0], view_layout(v["b"], itemsize)[0]


def embed(r, value, rng, kind):
    """A flat base for recipe r that holds `value` in the view's elements and drawn non-zero integers (below 2^7: they fit every
    dtype and precision) everywhere else: a kernel that reads one stride off the view reads one of them"""
    flat = X.draw_a(rng, (r.numel,), "bf16", kind, bits=127)
    apply_view(r, flat)[...] = value
    return flat


def planned(case):
    """The planner's answer for the case's launch (host only), under its switches, dtype and precision: INFO_FIELDS as a tuple
    plus the whole answer.  Gathered steps: the answer for the step on the gathered shapes, planned for any number of tiles
    as the gather entry point does (that entry point has no query of its own and plans with the gathered axis marked, so for
    'gather' and 'row_pairs' cases the path named is this answer and only the values are pinned)."""
    import torch
    import artensor_amd as A
    from artensor_amd import contraction as C
    dtype = torch.complex128 if case.dtype == "complex128" else torch.complex64
    env = dict(case.env, ARTN_FORCE_BITS="1") if case.kind == "gather" else case.env
    views = case.get("views", {})
    if "offset8" in (views.get("a"), views.get("out")) and case.kind == "step":
        # artn_contract plans an 8-byte aligned A or C with the tiled kernels switched off, as ARTN_FORCE_GENERIC does; the query
        # sees no pointers, so the switch stands in for them here (an 8-byte B changes the plan of the two-operand GEMM only,
        # inside the call: PLANNED holds the query's answer for those cases)
        env = dict(env, ARTN_FORCE_GENERIC="1")
    strided = has_views(case) and case.kind in ("step", "view", "pair")
    sa, sb = view_strides(case) if strided else (None, None)
    with environment(env), A.precision(case.precision):
        if case.kind == "pair" and not view_layout(view_of(case)["a"], 8)[2]:
            # contract2 declines a non-contiguous A: the first of the two launches that run instead
            info = A.step_info(case.eqs[0], case.a_shape, case.b_shapes[0], dtype=dtype, a_stride=sa, b_stride=sb)
        elif case.kind == "step" and strided:
            info = A.step_info(case.eqs[0], case.a_shape, case.b_shapes[0], dtype=dtype, a_stride=sa, b_stride=sb)
        elif case.kind in ("pair", "acc_pair"):
            info = C.pair_info(case.eqs[0], case.a_shape, case.b_shapes[0], case.eqs[1], case.b_shapes[1], dtype=dtype)
        elif case.kind == "row_pairs":   # (the unbatched step on the distinct rows: two private labels in place of the batch label)
            la, lb, lo = X.labels(case.eqs[0])
            ra, rb = ("row pairs", 0), ("row pairs", 1)
            info = A.step_info(((ra,) + la[1:], (rb,) + lb[1:], (ra, rb) + lo[1:]), case.a_shape, case.b_shapes[0], dtype=dtype)
        elif case.kind == "gather":
            info = A.step_info(case.eqs[0], (case.rows,) + case.a_shape[1:], (case.rows,) + case.b_shapes[0][1:], dtype=dtype)
        elif case.kind == "view":
            info = A.step_info(case.eqs[0], case.a_shape, case.b_shapes[0], dtype=dtype, a_stride=sa, b_stride=sb)
        else:
            info = A.step_info(case.eqs[0], case.a_shape, case.b_shapes[0], dtype=dtype)
    if info is not None:
        path_properties(case, info)
    return (None if info is None else tuple(int(info[f]) for f in INFO_FIELDS)), info


def operands(case):
    """(a, [small operands], accumulator or None, rows or None) of a case, from its seed.  Cases with views (has_views): a and
    the first small operand are the flat bases of their recipes (view_of; apply_view gives the operand, and the GPU test slices
    device copies of the bases the same way); 'gather' cases: a and b hold the source rows, rows = (rows_a, rows_b)."""
    stages = list(zip(case.eqs, case.b_shapes))
    kind = case.arith_kind
    acc = case.kind in ("acc_pair", "acc_step")
    if case.kind == "view":
        la, lb, lo = X.labels(case.eqs[0])
        rng = np.random.default_rng(case.seed)
        k = int(np.prod([dict(zip(lb, case.b_shapes[0]))[x] for x in X.contracted_labels(case.eqs[0])]))
        v = view_of(case)
        bsa, bsb, ib = v["a"].base_shape, v["b"].base_shape, v["b"].index
        a = X.draw_a(rng, bsa, case.cls, kind, bits=X.a_bits(case.cls, kind, [k]))
        # (the base of b by the class rule on the view's own labels plus the extra axis: every view of it keeps the rule)
        extra = len(ib) - 1 if ib[0] is not Ellipsis else len(lb)
        b = X.draw_small(rng, lb[:extra] + ("v",) + lb[extra:], bsb, X.contracted_labels(case.eqs[0]), case.cls, kind)
        return a.reshape(-1), [b.reshape(-1)], None, None
    if has_views(case):
        # the operands of the same case without views, each put into a base of drawn values: the views keep their class rules
        plain = Case(case, views={})
        a, smalls, acc, rows = operands(plain)
        v, rng = view_of(case), np.random.default_rng(case.seed + 3)
        return embed(v["a"], a, rng, kind), [embed(v["b"], smalls[0], rng, kind)] + smalls[1:], acc, rows
    if case.kind in ("gather", "row_pairs"):
        # (the rows of the operands: every source row is a stage operand of its own, so the class rules hold per row)
        a, smalls = X.draw_chain(case.seed, case.cls, kind, stages, case.a_shape)
        rng = np.random.default_rng(case.seed + 1)
        rows = (rng.integers(0, case.a_shape[0], size=case.rows), rng.integers(0, case.b_shapes[0][0], size=case.rows))
        return a, smalls, None, rows
    a, smalls = X.draw_chain(case.seed, case.cls, kind, stages, case.a_shape, acc=acc)
    return a, smalls, acc, None   # (acc: the accumulator itself is drawn by exact_result, which knows the result's shape)


def result_shape(case):
    """shape of the last result of the case's chain, from the labels' extents"""
    shape = case.a_shape
    for eq, b_shape in zip(case.eqs, case.b_shapes):
        la, lb, lo = X.labels(eq)
        ext = {**dict(zip(la, shape)), **dict(zip(lb, b_shape))}
        shape = tuple(ext[x] for x in lo)
    return shape


def exact_result(case, ops=None):
    """(exact result as complex128, accumulator start or None, largest range quantity) of a case, in integers"""
    a, smalls, acc, rows = ops if ops is not None else operands(case)
    kind = case.arith_kind
    if has_views(case):
        v = view_of(case)
        a, smalls = apply_view(v["a"], a), [apply_view(v["b"], smalls[0])] + list(smalls[1:])
    if case.kind in ("gather", "row_pairs"):
        la, lb, lo = X.labels(case.eqs[0])
        row_eq = (la[1:], lb[1:], lo[1:])
        q, memo, parts = 0, {}, []
        for ra, rb in zip(*rows):
            key = (int(ra), int(rb))
            if key not in memo:
                q = max(q, X.assert_exact_range(kind, [(row_eq, a[key[0]], smalls[0][key[1]])]))
                memo[key] = X.exact_einsum(row_eq, a[key[0]], smalls[0][key[1]])
            parts.append(memo[key])
        return np.stack(parts), None, q
    stages = [(eq, a if n == 0 else None, b) for n, (eq, b) in enumerate(zip(case.eqs, smalls))]
    start = None
    if acc:
        start = X.draw_acc(np.random.default_rng(case.seed + 2), result_shape(case), kind)
    res, q = X.exact_chain(kind, stages, acc=start)
    return res, start, q


# ---- whole schemes on integer leaves -----------------------------------------------------------------------------------------
_ONE_QUBIT = {"X": [[0, 1], [1, 0]], "Z": [[1, 0], [0, -1]], "S": [[1, 0], [0, 1j]], "H": [[1, 1], [1, -1]]}   # H unnormalised
MAX_H = 10   # every H can double the range quantity; permutations and X, Z, S keep it: 2^10 at the most, far below 2^24


def integer_leaves(shapes, seed=0):
    """id -> integer tensor (complex128) for the leaves of a qubit network: complex-signed permutation tensors for the
    two-qubit leaves (one leg fixed at 0 where the leaf has three legs), X, Z, S or the unnormalised H for the one-qubit
    leaves, at most MAX_H of them H"""
    rng = np.random.default_rng(seed)
    units = np.array([1, -1, 1j, -1j])
    out, n_h = {}, 0
    for i in sorted(shapes):
        shape = tuple(shapes[i])
        if shape == (2, 2):
            name = str(rng.choice(["X", "Z", "S", "H"], p=[0.1, 0.1, 0.1, 0.7]))
            if name == "H":
                n_h += 1
                if n_h > MAX_H:
                    name = "S"
            out[i] = np.array(_ONE_QUBIT[name], dtype=np.complex128)
        else:
            assert shape in ((2, 2, 2, 2), (2, 2, 2)), shape
            p = np.zeros((4, 4), dtype=np.complex128)
            p[np.arange(4), rng.permutation(4)] = units[rng.integers(0, 4, size=4)]
            p = p.reshape(2, 2, 2, 2)
            out[i] = p if len(shape) == 4 else np.ascontiguousarray(p[..., 0])
    return out


def exact_dense_scheme(leaves, scheme, kind):
    """(result, largest range quantity): tensors[i] <- einsum(eq, tensors[i], tensors[j]) per step, in integers, the exactness
    condition asserted at every step"""
    tensors, q, i = dict(leaves), 0, None
    for (i, j), eq in scheme:
        q = max(q, X.assert_exact_range(kind, [(eq, tensors[i], tensors[j])]))
        tensors[i] = X.exact_einsum(eq, tensors[i], tensors[j])
    return tensors[i], q


def exact_sparse_scheme(leaves, scheme, kind):
    """The sparse-state executor's four kinds of step in integers: (A) several row lists: gather both operands per chunk,
    contract, optional reshape, concatenate; (B) five fields, one row list per operand: gather both, contract; (C) five fields
    otherwise: contract, reshape, optional row select; (D) three fields: contract.  (result, largest range quantity)"""
    tensors, q, i = dict(leaves), 0, None
    idx = lambda r: np.asarray(r, dtype=np.int64)

    def step_on(eq, a, b):
        nonlocal q
        q = max(q, X.assert_exact_range(kind, [(eq, a, b)]))
        return X.exact_einsum(eq, a, b)
    for step in scheme:
        (i, j), eq, (rows_i, rows_j) = step[0], step[1], step[2]
        if len(rows_i) > 1:
            parts = []
            for ri, rj in zip(rows_i, rows_j):
                r = step_on(eq, tensors[i][idx(ri)], tensors[j][idx(rj)])
                parts.append(r.reshape(step[3]) if step[3] else r)
            tensors[i] = np.concatenate(parts, axis=0)
        elif len(step) > 3 and len(rows_i) == len(rows_j) == 1:
            tensors[i] = step_on(eq, tensors[i][idx(rows_i[0])], tensors[j][idx(rows_j[0])])
        elif len(step) > 3:
            tensors[i] = step_on(eq, tensors[i], tensors[j]).reshape(step[3])
            if len(rows_i) == 1:
                tensors[i] = tensors[i][idx(rows_i[0])]
        else:
            tensors[i] = step_on(eq, tensors[i], tensors[j])
    return tensors[i], q


# The planner's answer for every case, INFO_FIELDS order: (kernel, arith, k_bits, k2_bits, k3_bits).
# arith: 0 four products, 1 three products (3M), 2 bfloat16 operands, 3 complex128, -1 the strided kernel.
PLANNED = {
    "bits_k1_n1_wide": (1, 0, 1, 0, 0),
    "bits_k1_n1_dense": (1, 0, 1, 0, 0),
    "bits_k2_n0_wide": (1, 0, 2, 0, 0),
    "bits_k2_n0_dense": (1, 0, 2, 0, 0),
    "bits_k3_n3_wide": (1, 0, 3, 0, 0),
    "bits_k3_n3_dense": (1, 0, 3, 0, 0),
    "bits_k4_n4_wide": (1, 0, 4, 0, 0),
    "bits_k4_n4_dense": (1, 0, 4, 0, 0),
    "bits_k5_n5_wide": (1, 1, 5, 0, 0),
    "bits_k5_n5_dense": (1, 1, 5, 0, 0),
    "bits_k6_n6_wide": (1, 1, 6, 0, 0),
    "bits_k6_n6_dense": (1, 1, 6, 0, 0),
    "bits_k4_n7_wide": (1, 0, 4, 0, 0),
    "bits_k4_n7_dense": (1, 0, 4, 0, 0),
    "bits_k6_n2_wide": (1, 1, 6, 0, 0),
    "bits_k6_n2_dense": (1, 1, 6, 0, 0),
    "bits_k1_n6_wide": (1, 0, 1, 0, 0),
    "bits_k1_n6_dense": (1, 0, 1, 0, 0),
    "bits_k5_n1_wide": (1, 1, 5, 0, 0),
    "bits_k5_n1_dense": (1, 1, 5, 0, 0),
    "bits_k7_n3_wide": (1, 0, 7, 0, 0),
    "bits_k7_n3_dense": (1, 0, 7, 0, 0),
    "bits_k8_n4_wide": (1, 0, 8, 0, 0),
    "bits_k8_n4_dense": (1, 0, 8, 0, 0),
    "bits_k8_n0_wide": (1, 0, 8, 0, 0),
    "bits_k8_n0_dense": (1, 0, 8, 0, 0),
    "narrow3_k5_n2_wide": (1, 1, 5, 0, 0),
    "narrow3_k5_n2_dense": (1, 1, 5, 0, 0),
    "narrow3_k6_n1_wide": (1, 1, 6, 0, 0),
    "narrow3_k6_n1_dense": (1, 1, 6, 0, 0),
    "narrow3_k5_n0_wide": (1, 1, 5, 0, 0),
    "narrow3_k5_n0_dense": (1, 1, 5, 0, 0),
    "bits_k4_n4_bf16": (1, 2, 4, 0, 0),
    "bits_k6_n6_bf16": (1, 2, 6, 0, 0),
    "bits_k8_n4_bf16": (1, 2, 8, 0, 0),
    "full_step_k3": (1, 0, 3, 0, 0),
    "full_pair_k3_6": (1, 1, 3, 6, 0),
    "full_step_k4": (1, 0, 4, 0, 0),
    "full_pair_k4_5": (1, 1, 4, 5, 0),
    "full_step_k5": (1, 1, 5, 0, 0),
    "full_pair_k5_4": (1, 1, 5, 4, 0),
    "full_step_k6": (1, 1, 6, 0, 0),
    "full_pair_k6_3": (1, 1, 6, 3, 0),
    "n30_pair_75_78_wide": (1, 1, 6, 4, 0),
    "n30_pair_75_78_dense": (1, 1, 6, 4, 0),
    "n30_pair_80_83_wide": (1, 0, 3, 4, 0),
    "n30_pair_80_83_dense": (1, 0, 3, 4, 0),
    "n30_pair_88_90_wide": (1, 1, 5, 3, 0),
    "n30_pair_88_90_dense": (1, 1, 5, 3, 0),
    "n30_pair_93_97_wide": (1, 1, 4, 5, 0),
    "n30_pair_93_97_dense": (1, 1, 4, 5, 0),
    "n30_pair_101_104_wide": (1, 0, 4, 4, 0),
    "n30_pair_101_104_dense": (1, 0, 4, 4, 0),
    "n30_pair_108_112_wide": (1, 1, 5, 5, 0),
    "n30_pair_108_112_dense": (1, 1, 5, 5, 0),
    "n30_pair_123_125_wide": (1, 1, 5, 4, 0),
    "n30_pair_123_125_dense": (1, 1, 5, 4, 0),
    "n30_pair_128_131_wide": (1, 0, 3, 3, 0),
    "n30_pair_128_131_dense": (1, 0, 3, 3, 0),
    "pair_55_55_wide": (1, 1, 5, 5, 0),
    "pair_55_55_dense": (1, 1, 5, 5, 0),
    "pair_66_44_wide": (1, 1, 6, 4, 0),
    "pair_66_44_dense": (1, 1, 6, 4, 0),
    "pair_44_55_wide": (1, 1, 4, 5, 0),
    "pair_44_55_dense": (1, 1, 4, 5, 0),
    "pair_22_55_wide": (1, 1, 2, 5, 0),
    "pair_22_55_dense": (1, 1, 2, 5, 0),
    "pair_33_66_wide": (1, 1, 3, 6, 0),
    "pair_33_66_dense": (1, 1, 3, 6, 0),
    "pair_56_54_wide": (1, 1, 5, 5, 0),
    "pair_56_54_dense": (1, 1, 5, 5, 0),
    "pair_65_45_wide": (1, 1, 6, 4, 0),
    "pair_65_45_dense": (1, 1, 6, 4, 0),
    "pair_23_54_wide": (1, 1, 2, 5, 0),
    "pair_23_54_dense": (1, 1, 2, 5, 0),
    "pair_5_5_batch3_mode0": (1, 1, 5, 5, 0),
    "pair_6_4_batch3_mode1": (1, 1, 6, 4, 0),
    "pair_4_5_batch7_mode2": (1, 1, 4, 5, 0),
    "pair_3_6_batch2_mode0": (1, 1, 3, 6, 0),
    "pair_2_5_batch3_mode1": (1, 1, 2, 5, 0),
    "acc_pair_93_97": (1, 1, 4, 5, 0),
    "acc_pair_108_112": (1, 1, 5, 5, 0),
    "acc_pair_80_83_c128_wide128": (1, 3, 3, 4, 0),
    "acc_pair_108_112_c128_dense": (1, 3, 5, 5, 0),
    "acc_step_108": (1, 1, 5, 0, 0),
    "acc_step_139": (1, 1, 6, 0, 0),
    "acc_step_172": (1, 1, 5, 0, 0),
    "acc_step_c128_wide128": (1, 3, 6, 0, 0),
    "acc_step_c128_dense": (1, 3, 6, 0, 0),
    "wide_pair_66_default": (1, 1, 6, 6, 0),
    "gather_1rows_k3_wide": (1, 0, 3, 0, 0),
    "gather_1rows_k3_dense": (1, 0, 3, 0, 0),
    "gather_7rows_k4_wide": (1, 0, 4, 0, 0),
    "gather_7rows_k4_dense": (1, 0, 4, 0, 0),
    "gather_1000rows_k8_wide": (1, 0, 8, 0, 0),
    "gather_1000rows_k8_dense": (1, 0, 8, 0, 0),
    "gather_37rows_k7_wide": (2, 1, 7, 0, 0),
    "gather_37rows_k7_dense": (2, 1, 7, 0, 0),
    "row_pairs_wide": (1, 0, 4, 0, 0),
    "row_pairs_dense": (1, 0, 4, 0, 0),
    "gemm_m11_n11_k9_b0_wide": (2, 1, 9, 0, 0),
    "gemm_m12_n11_k7_b0_dense": (2, 1, 7, 0, 0),
    "gemm_m11_n12_k8_b0_wide": (2, 1, 8, 0, 0),
    "gemm_m13_n6_k8_b0_wide": (2, 1, 8, 0, 0),
    "gemm_m13_n6_k8_b0_dense": (2, 1, 8, 0, 0),
    "gemm_m9_n9_k9_b5_wide": (2, 1, 9, 0, 0),
    "gemm_m9_n9_k9_b5_dense": (2, 1, 9, 0, 0),
    "gemm_m10_n10_k11_b0_dense": (2, 1, 11, 0, 0),
    "gemm_m5_n5_k14_b0_wide": (2, 0, 14, 0, 0),
    "gemm_m5_n5_k14_b0_dense": (2, 0, 14, 0, 0),
    "gemm_m8_n8_k7_b3_wide": (2, 0, 7, 0, 0),
    "gemm_m8_n8_k7_b3_dense": (2, 0, 7, 0, 0),
    "gemm_bits_k7_n6_wide": (2, 0, 7, 0, 0),
    "gemm_bits_k7_n6_dense": (2, 0, 7, 0, 0),
    "gemm_split_k14_wide": (2, 0, 14, 0, 0),
    "gemm_split_k14_dense": (2, 0, 14, 0, 0),
    "gemm_views_wide": (2, 1, 9, 0, 0),
    "gemm_views_dense": (2, 1, 9, 0, 0),
    "xgemm_views_dense": (5, 1, 4, 0, 0),
    "pgemm_bf16_m12_n11_k9": (4, 2, 9, 0, 0),
    "pgemm_c64_m12_n11_k11": (4, 1, 11, 0, 0),
    "xgemm_mixed_wide": (5, 1, 4, 0, 0),
    "xgemm_mixed_dense": (5, 1, 4, 0, 0),
    "xgemm_mixed_c128_wide128": (5, 3, 4, 0, 0),
    "xgemm_mixed_c128_dense": (5, 3, 4, 0, 0),
    "xgemm_batch_dense": (5, 1, 4, 0, 0),
    "xgemm_tail_wide": (5, 1, 4, 0, 0),
    "xgemm_tail_dense": (5, 1, 4, 0, 0),
    "xrow_k5_n16_form0": (5, 1, 4, 0, 0),
    "xrow_k32_n32_form1": (5, 1, 4, 0, 0),
    "xrow_k40_n48_form0": (5, 1, 4, 0, 0),
    "xrow_k7_n41_form1": (5, 1, 4, 0, 0),
    "xrow64_bond3": (5, 1, 4, 0, 0),
    "gemm128_k4_n4_wide128": (2, 3, 4, 0, 0),
    "gemm128_k4_n4_dense": (2, 3, 4, 0, 0),
    "gemm128_k6_n6_wide128": (2, 3, 6, 0, 0),
    "gemm128_k6_n6_dense": (2, 3, 6, 0, 0),
    "gemm128_k8_n4_wide128": (2, 3, 8, 0, 0),
    "gemm128_k8_n4_dense": (2, 3, 8, 0, 0),
    "bits128_step_k6_n6_wide128": (1, 3, 6, 0, 0),
    "bits128_step_k6_n6_dense": (1, 3, 6, 0, 0),
    "bits128_pair_75_78_wide128": (1, 3, 6, 4, 0),
    "bits128_pair_75_78_dense": (1, 3, 6, 4, 0),
    "bits128_pair_93_97_wide128": (1, 3, 4, 5, 0),
    "bits128_pair_93_97_dense": (1, 3, 4, 5, 0),
    "bits128_pair_108_112_wide128": (1, 3, 5, 5, 0),
    "bits128_pair_108_112_dense": (1, 3, 5, 5, 0),
    "bits128_pair_128_131_wide128": (1, 3, 3, 3, 0),
    "bits128_pair_128_131_dense": (1, 3, 3, 3, 0),
    "generic128_k3_n3_wide128": (0, -1, 0, 0, 0),
    "generic128_k3_n3_dense": (0, -1, 0, 0, 0),
    "generic128_k7_n3_wide128": (0, -1, 0, 0, 0),
    "generic128_k7_n3_dense": (0, -1, 0, 0, 0),
    "generic_k3_n3": (0, -1, 0, 0, 0),
    "generic_k7_n3": (0, -1, 0, 0, 0),
    "generic_extent4": (0, -1, 0, 0, 0),
    # operand views, storage offsets and 8-byte bases (view_cases)
    "v_bits_k1_permuted_wide": (1, 0, 1, 0, 0),
    "v_bits_k1_permuted_dense": (1, 0, 1, 0, 0),
    "v_bits_k1_inner_wide": (1, 0, 1, 0, 0),
    "v_bits_k1_inner_dense": (1, 0, 1, 0, 0),
    "v_bits_k1_ends_wide": (5, 1, 4, 0, 0),
    "v_bits_k1_ends_dense": (5, 1, 4, 0, 0),
    "v_bits_k1_gap_wide": (1, 0, 1, 0, 0),
    "v_bits_k1_gap_dense": (1, 0, 1, 0, 0),
    "v_bits_k1_offset16_wide": (1, 0, 1, 0, 0),
    "v_bits_k1_offset16_dense": (1, 0, 1, 0, 0),
    "v_bits_k1_offset8a_wide": (0, -1, 0, 0, 0),
    "v_bits_k1_offset8a_dense": (0, -1, 0, 0, 0),
    "v_bits_k1_offset8b_wide": (1, 0, 1, 0, 0),
    "v_bits_k1_offset8b_dense": (1, 0, 1, 0, 0),
    "v_bits_k1_offset8c_wide": (0, -1, 0, 0, 0),
    "v_bits_k1_offset8c_dense": (0, -1, 0, 0, 0),
    "v_bits_k4_permuted_wide": (1, 0, 4, 0, 0),
    "v_bits_k4_permuted_dense": (1, 0, 4, 0, 0),
    "v_bits_k4_inner_wide": (1, 0, 4, 0, 0),
    "v_bits_k4_inner_dense": (1, 0, 4, 0, 0),
    "v_bits_k4_ends_wide": (5, 1, 4, 0, 0),
    "v_bits_k4_ends_dense": (5, 1, 4, 0, 0),
    "v_bits_k4_gap_wide": (1, 0, 4, 0, 0),
    "v_bits_k4_gap_dense": (1, 0, 4, 0, 0),
    "v_bits_k4_offset16_wide": (1, 0, 4, 0, 0),
    "v_bits_k4_offset16_dense": (1, 0, 4, 0, 0),
    "v_bits_k4_offset8a_wide": (0, -1, 0, 0, 0),
    "v_bits_k4_offset8a_dense": (0, -1, 0, 0, 0),
    "v_bits_k4_offset8b_wide": (1, 0, 4, 0, 0),
    "v_bits_k4_offset8b_dense": (1, 0, 4, 0, 0),
    "v_bits_k4_offset8c_wide": (0, -1, 0, 0, 0),
    "v_bits_k4_offset8c_dense": (0, -1, 0, 0, 0),
    "v_bits_k6_permuted_wide": (1, 1, 6, 0, 0),
    "v_bits_k6_permuted_dense": (1, 1, 6, 0, 0),
    "v_bits_k6_inner_wide": (1, 1, 6, 0, 0),
    "v_bits_k6_inner_dense": (1, 1, 6, 0, 0),
    "v_bits_k6_ends_wide": (5, 1, 4, 0, 0),
    "v_bits_k6_ends_dense": (5, 1, 4, 0, 0),
    "v_bits_k6_gap_wide": (1, 1, 6, 0, 0),
    "v_bits_k6_gap_dense": (1, 1, 6, 0, 0),
    "v_bits_k6_offset16_wide": (1, 1, 6, 0, 0),
    "v_bits_k6_offset16_dense": (1, 1, 6, 0, 0),
    "v_bits_k6_offset8a_wide": (0, -1, 0, 0, 0),
    "v_bits_k6_offset8a_dense": (0, -1, 0, 0, 0),
    "v_bits_k6_offset8b_wide": (1, 1, 6, 0, 0),
    "v_bits_k6_offset8b_dense": (1, 1, 6, 0, 0),
    "v_bits_k6_offset8c_wide": (0, -1, 0, 0, 0),
    "v_bits_k6_offset8c_dense": (0, -1, 0, 0, 0),
    "v_bits128_k6_permuted_wide128": (1, 3, 6, 0, 0),
    "v_bits128_k6_permuted_dense": (1, 3, 6, 0, 0),
    "v_bits128_k6_gap_wide128": (1, 3, 6, 0, 0),
    "v_bits128_k6_gap_dense": (1, 3, 6, 0, 0),
    "v_bits128_k6_offset16_wide128": (1, 3, 6, 0, 0),
    "v_bits128_k6_offset16_dense": (1, 3, 6, 0, 0),
    "v_gemm128_k4_permuted_wide128": (2, 3, 4, 0, 0),
    "v_gemm128_k4_permuted_dense": (2, 3, 4, 0, 0),
    "v_gemm128_k4_offset16_wide128": (2, 3, 4, 0, 0),
    "v_gemm128_k4_offset16_dense": (2, 3, 4, 0, 0),
    "v_gemm_m8_n8_k7_b3_gap_wide": (2, 0, 7, 0, 0),
    "v_gemm_m8_n8_k7_b3_gap_dense": (2, 0, 7, 0, 0),
    "v_gemm_m8_n8_k7_b3_offset16_wide": (2, 0, 7, 0, 0),
    "v_gemm_m8_n8_k7_b3_offset16_dense": (2, 0, 7, 0, 0),
    "v_gemm_m8_n8_k7_b3_offset8b_wide": (2, 0, 7, 0, 0),
    "v_gemm_m8_n8_k7_b3_offset8b_dense": (2, 0, 7, 0, 0),
    "v_gemm_bits_k7_offset8b_wide": (2, 0, 7, 0, 0),
    "v_gemm_bits_k7_offset8b_dense": (2, 0, 7, 0, 0),
    "v_xgemm_mixed_permuted_wide": (5, 1, 4, 0, 0),
    "v_xgemm_mixed_offset16_dense": (5, 1, 4, 0, 0),
    "v_xgemm_mixed_offset8b_wide": (5, 1, 4, 0, 0),
    "v_xrow_k5_n16_offset16_wide": (5, 1, 4, 0, 0),
    "v_xrow_k5_n16_offset8b_wide": (5, 1, 4, 0, 0),
    "v_xrow_k7_n41_offset16_dense": (5, 1, 4, 0, 0),
    "v_xrow_k7_n41_offset8b_dense": (5, 1, 4, 0, 0),
    "v_pgemm_bf16_inner_bf16": (4, 2, 9, 0, 0),
    "v_pgemm_bf16_offset16_bf16": (4, 2, 9, 0, 0),
    "v_pgemm_c64_inner_dense": (4, 1, 11, 0, 0),
    "v_pgemm_c64_offset16_dense": (4, 1, 11, 0, 0),
    "v_pair_5_3_inner_wide": (1, 1, 5, 0, 0),
    "v_pair_5_3_gap_dense": (1, 1, 5, 0, 0),
    "v_pair_5_3_offset16_wide": (1, 1, 5, 3, 0),
    "v_pair_5_3_offset16_dense": (1, 1, 5, 3, 0),
    "v_pair_6_4_inner_wide": (1, 1, 6, 0, 0),
    "v_pair_6_4_gap_dense": (1, 1, 6, 0, 0),
    "v_pair_6_4_offset16_wide": (1, 1, 6, 4, 0),
    "v_pair_6_4_offset16_dense": (1, 1, 6, 4, 0),
    "v_gather_7rows_k3_inner_wide": (1, 0, 3, 0, 0),
    "v_gather_7rows_k3_inner_dense": (1, 0, 3, 0, 0),
    "v_gather_7rows_k3_offset8a_dense": (1, 0, 3, 0, 0),
    "v_row_pairs_inner_wide": (1, 0, 4, 0, 0),
    "v_row_pairs_inner_dense": (1, 0, 4, 0, 0),
    "v_row_pairs_offset8a_wide": (1, 0, 4, 0, 0),
    "v_acc_step_c128_offset16_wide128": (1, 3, 6, 0, 0),
    "v_acc_step_c128_offset16_dense": (1, 3, 6, 0, 0),
    "v_acc_pair_80_83_c128_offset16_wide128": (1, 3, 3, 4, 0),
    "v_acc_pair_80_83_c128_offset16_dense": (1, 3, 3, 4, 0),
    "v_acc_step_k6_offset16_wide": (1, 1, 6, 0, 0),
    "v_acc_step_k6_offset16_dense": (1, 1, 6, 0, 0),
    "v_acc_step_k6_offset8c_wide": (1, 1, 6, 0, 0),
    "v_acc_step_k6_offset8c_dense": (1, 1, 6, 0, 0),
}
