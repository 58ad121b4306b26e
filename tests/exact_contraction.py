"""Exact-integer operands for the contraction engine: generators, an integer reference and the exactness condition.

Every operand is a tensor of Gaussian integers stored in the target dtype.  When, for every stage of a launch,

    Q = max over outputs of  sum_k (|a_re| + |a_im|) * (|b_re| + |b_im|)

stays below 2^24 (complex64 and precision("bf16"): an fp32 accumulator) or 2^53 (complex128), every product and every
partial sum of the four-product form is an integer the accumulator holds exactly -- in any summation order, tile shape,
split-K or fusion -- and so are the three products of the 3M form, (a_re + a_im)(b_re + b_im), a_re b_re and a_im b_im,
and its re + im fragments (|a_re + a_im| <= |a_re| + |a_im|).  The result of a correct kernel is then the integer result
bit for bit, and the tests compare with `==`.

CPU only: numpy and Python ints.  The reference shares no index arithmetic with artensor_amd: operands are split into
integer re / im parts, moved to (batch, free, contracted) order by numpy's transpose and multiplied by np.matmul in int64.
(Products of more than 2^26 multiply-adds go through float64 matmul instead -- BLAS, seconds instead of minutes; it is exact
under the same condition, sums below 2^53, which assert_exact_range checks on the magnitudes before anything is compared.)

Operand classes (`draw_a` for the streamed operand, `draw_small` for the others; seeded, deterministic):
  wide     A: |re|, |im| in [2^(bits-1), 2^bits) with the low bit set, bits = 20 unless a chain needs fewer: every value needs
           three bfloat16 pieces.  Small operands: at most 4 non-zeros per contracted column, from {+-1, +-i, +-1+-i}, at
           positions drawn per column.
  dense    A: |re|, |im| < 2^11; small operands dense with re, im in {+-1, +-2}: no zero product in any MFMA lane.
  bf16     as dense with |re|, |im| <= cap <= 128 everywhere and no zeros: every value is a bfloat16.
  wide128  complex128: A below 2^44, small operands by the `wide` rule."""
import math

import numpy as np

LIMIT = {"complex64": 2 ** 24, "bf16": 2 ** 24, "complex128": 2 ** 53}
DEFAULT_BITS = {"wide": 20, "dense": 11, "bf16": 7, "wide128": 44}
HEAVY = 1 << 26   # multiply-adds above which the reference multiplies in float64 (exact below 2^53)
ACC_BITS = 10     # |re|, |im| of a store-phase accumulator stay below 2^ACC_BITS


def labels(eq):
    """(labels of a, of b, of the result) of an einsum string or of a triple of label tuples"""
    if isinstance(eq, str):
        lhs, lo = eq.split("->")
        la, lb = lhs.split(",")
        return tuple(la), tuple(lb), tuple(lo)
    return tuple(eq[0]), tuple(eq[1]), tuple(eq[2])


def contracted_labels(eq):
    la, lb, lo = labels(eq)
    return tuple(x for x in lb if x in la and x not in lo)


def int_parts(x):
    """(re, im) of a tensor of Gaussian integers as int64 arrays; a value that is no integer is an error"""
    x = np.asarray(x)
    re, im = np.rint(x.real).astype(np.int64), np.rint(x.imag).astype(np.int64)
    assert np.array_equal(re, x.real) and np.array_equal(im, x.imag), "operand is not a tensor of Gaussian integers"
    return re, im


def from_parts(re, im, dtype=np.complex128):
    out = np.empty(np.shape(re), dtype=dtype)
    out.real = re
    out.imag = im
    assert np.array_equal(out.real, re) and np.array_equal(out.imag, im), f"values do not fit {np.dtype(dtype).name}"
    return out


def _real_contract(la, lb, lo, x, y):
    """einsum of two int64 arrays: sum-outs, transposes to (batch, free, contracted) x (batch, contracted, free), np.matmul"""
    la, lb, lo = list(la), list(lb), list(lo)
    assert len(set(la)) == len(la) and len(set(lb)) == len(lb) and len(set(lo)) == len(lo)
    for lab in [l for l in la if l not in lb and l not in lo]:
        x = x.sum(axis=la.index(lab))
        la.remove(lab)
    for lab in [l for l in lb if l not in la and l not in lo]:
        y = y.sum(axis=lb.index(lab))
        lb.remove(lab)
    ext = dict(zip(la, x.shape))
    for lab, e in zip(lb, y.shape):
        assert ext.setdefault(lab, e) == e, (lab, e, ext[lab])
    batch = [l for l in la if l in lb and l in lo]
    con = [l for l in la if l in lb and l not in lo]
    fa = [l for l in la if l not in lb]
    fb = [l for l in lb if l not in la]
    assert sorted(map(str, lo)) == sorted(map(str, batch + fa + fb)), (la, lb, lo)
    size = lambda ls: int(np.prod([ext[l] for l in ls], dtype=np.int64)) if ls else 1
    X = x.transpose([la.index(l) for l in batch + fa + con]).reshape(size(batch), size(fa), size(con))
    Y = y.transpose([lb.index(l) for l in batch + con + fb]).reshape(size(batch), size(con), size(fb))
    if size(batch) * size(fa) * size(con) * size(fb) > HEAVY:
        Z = np.matmul(X.astype(np.float64), Y.astype(np.float64))
        assert np.abs(Z).max() < 2.0 ** 53
        Z = Z.astype(np.int64)
    else:
        Z = np.matmul(X, Y)
    res = batch + fa + fb
    return Z.reshape([ext[l] for l in res]).transpose([res.index(l) for l in lo])


def exact_parts(eq, a, b):
    """(re, im) of einsum(eq, a, b) in int64, from four real integer products"""
    la, lb, lo = labels(eq)
    (ar, ai), (br, bi) = int_parts(a), int_parts(b)
    re = _real_contract(la, lb, lo, ar, br) - _real_contract(la, lb, lo, ai, bi)
    im = _real_contract(la, lb, lo, ar, bi) + _real_contract(la, lb, lo, ai, br)
    return re, im


def exact_einsum(eq, a, b):
    """einsum(eq, a, b) of Gaussian-integer tensors, exactly, as complex128 (every value below 2^53)"""
    return from_parts(*exact_parts(eq, a, b))


def exact_pair(eq1, a, b1, eq2, b2):
    return exact_einsum(eq2, exact_einsum(eq1, a, b1), b2)


def exact_triple(eq1, a, b1, eq2, b2, eq3, b3):
    return exact_einsum(eq3, exact_pair(eq1, a, b1, eq2, b2), b3)


def exact_gathered(eq, a, rows_a, b, rows_b):
    """einsum(eq, a[rows_a], b[rows_b]); rows None: the operand as it is"""
    a = np.asarray(a)[np.asarray(rows_a)] if rows_a is not None else a
    b = np.asarray(b)[np.asarray(rows_b)] if rows_b is not None else b
    return exact_einsum(eq, a, b)


def exact_accumulate(acc, value):
    """acc += value in integers (the add in the store phase of a launch)"""
    (cr, ci), (vr, vi) = int_parts(acc), int_parts(value)
    return from_parts(cr + vr, ci + vi)


def range_quantity(eq, a, b):
    """max over outputs of sum_k (|a_re| + |a_im|) (|b_re| + |b_im|), a Python int"""
    la, lb, lo = labels(eq)
    (ar, ai), (br, bi) = int_parts(a), int_parts(b)
    q = _real_contract(la, lb, lo, np.abs(ar) + np.abs(ai), np.abs(br) + np.abs(bi))
    return int(q.max()) if q.size else 0


def exact_chain(kind, stages, acc=None):
    """A chain of stages [(eq, a, b), ...] -- a None for "the exact result of the stage before" -- with the exactness condition
    asserted at every stage, each product computed once: (exact result, accumulator included; largest range quantity)"""
    limit = LIMIT[kind]
    worst, prev = 0, None
    for n, (eq, a, b) in enumerate(stages):
        a = prev if a is None else a
        assert a is not None
        q = range_quantity(eq, a, b)
        if kind == "bf16":   # operands are rounded to bfloat16 on their way to the matrix cores: they must be bfloat16 already
            for x in (a, b):
                assert _is_bf16(x), "operand of a bf16 case is not representable in bfloat16"
        if acc is not None and n == len(stages) - 1:
            cr, ci = int_parts(acc)
            q += int((np.abs(cr) + np.abs(ci)).max())
        assert q < limit, f"stage {n} of {len(stages)}: range quantity {q} = 2^{math.log2(max(q, 1)):.2f} is not below 2^{int(math.log2(limit))}"
        worst = max(worst, q)
        prev = exact_einsum(eq, a, b)
    return (prev if acc is None else exact_accumulate(acc, prev)), worst


def assert_exact_range(kind, stages, acc=None):
    """The exactness condition, on the inputs alone.  kind: 'complex64', 'bf16' or 'complex128'; stages: [(eq, a, b), ...] where
    a is None for "the exact result of the stage before" (the intermediate of a fused pair or triple); acc: the accumulator a
    store-phase add starts from.  Asserts Q < 2^24 / 2^53 for every stage (the accumulator's magnitude added to the last)
    and returns the largest Q.  A case that fails here is a bug in its generator."""
    return exact_chain(kind, stages, acc)[1]


def _is_bf16(x):
    re, im = int_parts(x)
    v = np.abs(np.concatenate([re.reshape(-1), im.reshape(-1)]))
    v = v[v > 0]
    low = v & -v                      # lowest set bit
    return bool(np.all(v < low * 256))   # 8 significant bits


def headroom(q, kind):
    """'2^21.3 of 2^24' -- the largest range quantity of a test, for its printed line"""
    return f"2^{math.log2(max(q, 1)):.1f} of 2^{int(math.log2(LIMIT[kind]))}"


# ---- generators --------------------------------------------------------------------------------------------------------
def stage_factor(cls, k_values, cap=None):
    """Worst case of sum_k (|b_re| + |b_im|) over one column of a small operand of class cls with k_values contracted values"""
    if cls in ("wide", "wide128"):
        return 2 * min(4, k_values)
    if cls == "dense":
        return 4 * k_values
    return 2 * (cap if cap is not None else bf16_cap(k_values)) * k_values


def bf16_cap(k_values):
    """Largest magnitude c <= 128 with k (2c)(2c) < 2^24: the cap of class bf16 falls as the contraction grows"""
    return max(1, min(128, math.isqrt((2 ** 24 - 1) // (4 * k_values))))


def a_bits(cls, kind, k_values, acc=False):
    """Bits of the streamed operand for a chain of stages with k_values = (K1, K2, ...) contracted values each: the class's
    own width, lowered until the worst-case bound 2 (2^bits - 1) prod(stage factors) (+ accumulator) is below the limit"""
    limit = LIMIT[kind] - (2 ** (ACC_BITS + 1) if acc else 0)
    f = 1
    for k in k_values:
        f *= stage_factor(cls, k)
    bits = DEFAULT_BITS[cls]
    while bits > 1 and 2 * (2 ** bits - 1) * f >= limit:
        bits -= 1
    assert 2 * (2 ** bits - 1) * f < limit, (cls, kind, k_values)
    return bits


def _np_dtype(kind):
    return np.complex128 if kind == "complex128" else np.complex64


def draw_a(rng, shape, cls, kind="complex64", bits=None):
    """The streamed operand of class cls; bits: see a_bits (class bf16: the magnitude cap itself, 128 when None)"""
    cap = 128 if bits is None else bits
    bits = DEFAULT_BITS[cls] if bits is None else bits
    shape = tuple(shape)
    if cls in ("wide", "wide128"):
        part = lambda: ((rng.integers(2 ** (bits - 1), 2 ** bits, size=shape, dtype=np.int64) | 1)
                        * rng.choice(np.array([-1, 1], dtype=np.int64), size=shape))
    elif cls == "dense":
        part = lambda: rng.integers(-(2 ** bits) + 1, 2 ** bits, size=shape, dtype=np.int64)
    else:
        part = lambda: rng.integers(1, cap + 1, size=shape, dtype=np.int64) * rng.choice(np.array([-1, 1], dtype=np.int64), size=shape)
    return from_parts(part(), part(), _np_dtype(kind))


_UNITS = np.array([1, -1, 1j, -1j, 1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j])


def draw_small(rng, eq_labels_b, shape, contracted, cls, kind="complex64", cap=None):
    """A small operand of class cls with labels eq_labels_b and the given shape; contracted: its contracted labels (the
    column of the `wide` rule runs over them, one column per value of the other labels)"""
    lb, shape = list(eq_labels_b), tuple(shape)
    if cls in ("wide", "wide128"):
        kax = [lb.index(x) for x in contracted]
        rest = [n for n in range(len(lb)) if n not in kax]
        K = int(np.prod([shape[n] for n in kax], dtype=np.int64)) if kax else 1
        cols = int(np.prod([shape[n] for n in rest], dtype=np.int64)) if rest else 1
        nnz = min(4, K)
        m = np.zeros((cols, K), dtype=np.complex128)
        pos = np.argsort(rng.random((cols, K)), axis=1)[:, :nnz]           # positions differ per column
        np.put_along_axis(m, pos, _UNITS[rng.integers(0, 8, size=(cols, nnz))], axis=1)
        perm = rest + kax
        t = m.reshape([shape[n] for n in perm]).transpose(np.argsort(perm))
        return np.ascontiguousarray(t).astype(_np_dtype(kind)).reshape(shape)   # (ascontiguousarray makes a scalar 1-d)
    top = 2 if cls == "dense" else (cap if cap is not None else 128)
    part = lambda: rng.integers(1, top + 1, size=shape, dtype=np.int64) * rng.choice(np.array([-1, 1], dtype=np.int64), size=shape)
    return from_parts(part(), part(), _np_dtype(kind))


def draw_acc(rng, shape, kind="complex64"):
    part = lambda: rng.integers(-(2 ** ACC_BITS) + 1, 2 ** ACC_BITS, size=tuple(shape), dtype=np.int64)
    re, im = part(), part()
    re[re == 0] = 1   # a non-zero accumulator
    return from_parts(re, im, _np_dtype(kind))


def draw_chain(seed, cls, kind, stages, a_shape, acc=False):
    """Operands of a chain of stages [(eq, b_shape), ...] on one streamed operand of shape a_shape: (a, [b1, b2, ...]) with
    a's width lowered so that the worst-case bound of every stage holds (a_bits); class bf16 gets its magnitude cap from the
    contraction length of its (single) stage."""
    rng = np.random.default_rng(seed)
    la0 = labels(stages[0][0])[0]
    ext = dict(zip(la0, a_shape))
    ks, smalls, cap = [], [], None
    for eq, b_shape in stages:
        la, lb, lo = labels(eq)
        ext_b = dict(zip(lb, b_shape))
        con = contracted_labels(eq)
        ks.append(int(np.prod([ext_b[x] for x in con], dtype=np.int64)) if con else 1)
    if cls == "bf16":
        assert len(stages) == 1
        cap = bf16_cap(ks[0])
        a = draw_a(rng, a_shape, cls, kind, bits=cap)
    else:
        a = draw_a(rng, a_shape, cls, kind, bits=a_bits(cls, kind, ks, acc))
    for eq, b_shape in stages:
        smalls.append(draw_small(rng, labels(eq)[1], b_shape, contracted_labels(eq), cls, kind, cap=cap))
    return a, smalls
