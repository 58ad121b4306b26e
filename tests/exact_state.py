"""Integer states whose image under gates and Pauli steps is predictable EXACTLY from the memory index alone (shared by
test_state_ops_large_cpu.py, which checks this file against the numpy oracles of the other suites, and
test_state_ops_large_gpu.py and test_wide_ops_large_gpu.py, which use it on states of 8 and 32 GiB).  A non-zero `salt` gives a
second, unrelated integer state for the operations on two arrays; inner_sums, marginal_sums and rdm_sums are the exact integer
values of the sums the kernels accumulate in float64; Budget and norm_invariant open and close every large GPU test.

The state.  a[i] = f(i) + i g(i) with f, g in [-8, 7] from a 32-bit integer hash of the memory index i (index bits 32 and 33
are folded in first, so every bit up to 33 matters), evaluated in torch int64; every product is formed on masked operands and
stays below 2^59.

Expected values.  A gate or a Pauli step is a sparse linear map: out[i] = sum_t c_t(i) prev[p_t(i)] with T = 1 (a signed
permutation), 2 or 4 partners and Gaussian-integer coefficients.  evaluate(ops, i) recurses through the steps on the partner
indices -- all partners of a level in ONE concatenated index tensor -- down to the hash: prod T hash evaluations per element,
no state-sized buffer, nothing but the index as input.

Exactness.  The kernels form every output component in float64 and round it once to the dtype.  While every component and
every partial sum stays below 2^24 (complex64) or 2^53 (complex128) in magnitude, products, sums and the rounding are exact,
so the result EQUALS the integer prediction.  bound(ops) is the a-priori bound 8 prod growth_k of every partial sum, growth_k
the largest row sum of |Re c| + |Im c|; Tally also records the largest predicted component.  Values are compared with ==
(-0.0 == 0.0: the accumulators of the kernels start at -0.0)."""
import numpy as np
import torch

CHUNK = 1 << 25                 # elements per chunk: int64 temporaries of 256 MiB, a handful alive at a time
M32 = 0xFFFFFFFF
MIX = 0x45D9F3B                 # < 2^27
HIGH = 0x27D4EB2F               # 3 * HIGH < 2^32
LIMIT = {torch.complex64: 1 << 24, torch.complex128: 1 << 53}
BIG = (1 << 62)
# the salted state hashes i ^ SALT: bits 1, 6, 9 (low third of 34), 14, 19 (middle), 25, 30, 33 (top)
SALT = (1 << 33) | (1 << 30) | (1 << 25) | (1 << 19) | (1 << 14) | (1 << 9) | (1 << 6) | (1 << 1)


def hash_index(i, salt=0):
    """(f, g), int64 in [-8, 7], of an int64 index tensor (any values in [0, 2^34)).  Two temporaries of the size of i.  A
    non-zero salt hashes i ^ SALT instead: a second, unrelated integer state."""
    x = i & M32
    t = i >> 32
    if salt:
        x.bitwise_xor_(SALT & M32)
        t.bitwise_xor_(SALT >> 32)
    t.bitwise_and_(3).mul_(HIGH)                               # bits 32, 33 -> one of four 32-bit words
    x.bitwise_xor_(t)
    for _ in range(2):
        torch.bitwise_right_shift(x, 16, out=t)
        x.bitwise_xor_(t).mul_(MIX).bitwise_and_(M32)          # x < 2^32 before the product: it stays below 2^59
    torch.bitwise_right_shift(x, 16, out=t)
    x.bitwise_xor_(t)
    torch.bitwise_right_shift(x, 5, out=t)
    t.bitwise_and_(15).sub_(8)
    x.bitwise_right_shift_(21).bitwise_and_(15).sub_(8)
    return t, x


def hash_python(i, salt=0):
    """hash_index for one Python int, in unbounded integers."""
    if salt:
        i ^= SALT
    x = (i & M32) ^ (((i >> 32) & 3) * HIGH)
    for _ in range(2):
        x = ((x ^ (x >> 16)) * MIX) & M32
    x ^= x >> 16
    return ((x >> 5) & 15) - 8, ((x >> 21) & 15) - 8


def fill(store, chunk=CHUNK, salt=0):
    """store (a flat complex tensor) <- the hash state (the salted one for salt != 0), chunk by chunk."""
    n = store.numel()
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        f, g = hash_index(torch.arange(lo, hi, device=store.device), salt)
        out = torch.view_as_real(store[lo:hi])
        out[:, 0].copy_(f)
        out[:, 1].copy_(g)
    return store


def _gauss(z, what):
    z = np.asarray(z, dtype=np.complex128)
    re, im = np.rint(z.real).astype(np.int64), np.rint(z.imag).astype(np.int64)
    assert np.array_equal(re + 1j * im, z), f"{what}: Gaussian integers expected"
    return re, im


def _parity(p):
    """Parity of the set bits of an int64 tensor (overwritten)."""
    for s in (32, 16, 8, 4, 2, 1):
        p.bitwise_xor_(p >> s)
    return p.bitwise_and_(1)


class Gate:
    """(matrix, bits): bits = the MEMORY bits of the gate's dims in the order listed, the first the most significant digit of
    the row and column index.  Term t of row r is the t-th non-zero column of that row, so a signed permutation costs one
    partner, a dense 4 x 4 four and a dense gate on k = 3, 4, 5 bits 8, 16, 32."""

    def __init__(self, matrix, bits):
        self.bits = tuple(int(b) for b in bits)
        k = len(self.bits)
        assert 1 <= k <= 5 and len(set(self.bits)) == k
        m = np.asarray(matrix, dtype=np.complex128).reshape(2 ** k, 2 ** k)
        re, im = _gauss(m, "gate")
        rows = [[c for c in range(2 ** k) if re[r, c] or im[r, c]] for r in range(2 ** k)]
        self.T = max(1, max(len(x) for x in rows))
        self.col = [[rows[r][t] if t < len(rows[r]) else r for r in range(2 ** k)] for t in range(self.T)]
        self.cre = [[int(re[r, rows[r][t]]) if t < len(rows[r]) else 0 for r in range(2 ** k)] for t in range(self.T)]
        self.cim = [[int(im[r, rows[r][t]]) if t < len(rows[r]) else 0 for r in range(2 ** k)] for t in range(self.T)]
        self.growth = int((np.abs(re) + np.abs(im)).sum(axis=1).max())
        g = m @ m.conj().T
        self.scale2 = int(round(g[0, 0].real)) if np.array_equal(g, g[0, 0].real * np.eye(2 ** k)) else None

    def terms(self, i):
        k = len(self.bits)
        mask = sum(1 << b for b in self.bits)
        r = torch.zeros_like(i)
        for j, b in enumerate(self.bits):
            r.bitwise_or_(((i >> b) & 1) << (k - 1 - j))
        out = []
        for t in range(self.T):
            col = torch.tensor(self.col[t], dtype=torch.int64, device=i.device)[r]
            p = i & ~mask
            for j, b in enumerate(self.bits):
                p.bitwise_or_(((col >> (k - 1 - j)) & 1) << b)
            out.append((p, torch.tensor(self.cre[t], dtype=torch.int64, device=i.device)[r],
                        torch.tensor(self.cim[t], dtype=torch.int64, device=i.device)[r]))
        return out


def _string_term(c, letters, i):
    """(partner, Re, Im) of c P at the output indices i; letters = {memory bit: 'X' | 'Y' | 'Z'}.  Bit by bit: X reads the
    flipped bit; Z multiplies by (-1)^bit; Y reads the flipped bit and multiplies by -i (bit 0) or +i (bit 1)."""
    xm = sum(1 << b for b, l in letters.items() if l in "XY")
    sm = sum(1 << b for b, l in letters.items() if l in "YZ")
    ny = sum(1 for l in letters.values() if l == "Y")
    c0 = complex(c) * (-1j) ** ny                              # every Y at bit value 0; each set bit under Y or Z flips the sign
    re, im = _gauss(c0, "coefficient")
    sign = 1 - 2 * _parity(i & sm)
    return i ^ xm, (int(re) * sign if re else 0), (int(im) * sign if im else 0)


class PauliStep:
    """a <- alpha a + beta P a with P = {memory bit: letter}."""

    def __init__(self, alpha, beta, letters):
        self.alpha, self.beta, self.letters = complex(alpha), complex(beta), {int(b): l.upper() for b, l in letters.items()}
        assert all(l in "XYZ" for l in self.letters.values())
        (are, aim), (bre, bim) = _gauss(self.alpha, "alpha"), _gauss(self.beta, "beta")
        self.a = (int(are), int(aim))
        self.T = int(self.alpha != 0) + int(self.beta != 0)
        assert self.T
        self.growth = int(abs(are) + abs(aim) + abs(bre) + abs(bim))
        cross = (self.alpha.conjugate() * self.beta).real      # (alpha + beta P)^H (alpha + beta P) = |alpha|^2 + |beta|^2 + 2 cross P
        self.scale2 = int(round(abs(self.alpha) ** 2 + abs(self.beta) ** 2)) if cross == 0 else None

    def terms(self, i):
        out = []
        if self.alpha != 0:
            out.append((i, self.a[0], self.a[1]))
        if self.beta != 0:
            out.append(_string_term(self.beta, self.letters, i))
        return out


class PauliSum:
    """y = sum_k c_k P_k a, terms = [(c_k, {memory bit: letter}), ...]."""

    def __init__(self, terms):
        self.items = [(complex(c), {int(b): l.upper() for b, l in letters.items()}) for c, letters in terms]
        self.T = len(self.items)
        self.growth = int(sum(abs(x) for c, _ in self.items for x in _gauss(c, "coefficient")))
        self.scale2 = None

    def terms(self, i):
        return [_string_term(c, letters, i) for c, letters in self.items]


class Projector:
    """|outcome><outcome| on the memory bits `bits` (the first the most significant digit): coefficient 1 where the digits of
    the index spell `outcome`, 0 elsewhere -- what a projective channel or a post-selection without renormalisation leaves."""

    def __init__(self, bits, outcome):
        self.bits, self.outcome = tuple(int(b) for b in bits), int(outcome)
        k = len(self.bits)
        assert len(set(self.bits)) == k and 0 <= self.outcome < 2 ** k
        self.T, self.growth, self.scale2 = 1, 1, None

    def terms(self, i):
        k = len(self.bits)
        keep = torch.ones_like(i)
        for j, b in enumerate(self.bits):
            keep.bitwise_and_(((i >> b) & 1) ^ (1 ^ ((self.outcome >> (k - 1 - j)) & 1)))
        return [(i, keep, 0)]


def leaves(ops):
    """Hash evaluations per element."""
    return int(np.prod([op.T for op in ops], dtype=np.int64)) if ops else 1


def bound(ops):
    """A bound of every component and of every partial sum of every step, from the coefficients alone."""
    out = 8
    for op in ops:
        out *= op.growth
    return out


def scale2(ops):
    """s with sum |out|^2 = s sum |in|^2: every step is a Gaussian-integer multiple of a unitary (None otherwise)."""
    out = 1
    for op in ops:
        if op.scale2 is None:
            return None
        out *= op.scale2
    return out


def _mul(c, v):
    """c v as a NEW tensor (the sums below are accumulated in place), None for the integer 0."""
    return None if isinstance(c, int) and c == 0 else c * v


def _acc(acc, term, sign=1):
    if term is None:
        return acc
    if acc is None:
        return term if sign == 1 else -term
    return acc.add_(term) if sign == 1 else acc.sub_(term)


def evaluate(ops, i, salt=0):
    """(Re, Im), int64, of the state after `ops` (applied in order to the hash state, the salted one for salt != 0) at the
    memory indices i."""
    if not ops:
        return hash_index(i, salt)
    n = i.numel()
    terms = ops[-1].terms(i)
    idx = terms[0][0] if len(terms) == 1 else torch.cat([t[0] for t in terms])
    terms = [(cre, cim) for _, cre, cim in terms]
    re, im = evaluate(ops[:-1], idx, salt)
    del idx
    out_re = out_im = None
    for t, (cre, cim) in enumerate(terms):
        r, m = re[t * n:(t + 1) * n], im[t * n:(t + 1) * n]
        out_re = _acc(_acc(out_re, _mul(cre, r)), _mul(cim, m), -1)           # (c + i d)(r + i m) = (c r - d m) + i (c m + d r)
        out_im = _acc(_acc(out_im, _mul(cre, m)), _mul(cim, r))
    zero = torch.zeros(n, dtype=torch.int64, device=i.device)
    return (zero if out_re is None else out_re), (zero if out_im is None else out_im)


class Tally:
    """Device-side counters of a comparison: elements compared, mismatches, the first mismatching index, the largest predicted
    component.  report() synchronises once."""

    def __init__(self, device):
        self.n = 0
        self.bad = torch.zeros((), dtype=torch.int64, device=device)
        self.first = torch.full((), BIG, dtype=torch.int64, device=device)
        self.peak = torch.zeros((), dtype=torch.int64, device=device)

    def add(self, got, re, im, index):
        g = torch.view_as_real(got)
        wrong = (g[:, 0] != re.to(g.dtype)) | (g[:, 1] != im.to(g.dtype))
        self.n += got.numel()
        self.bad += wrong.sum()
        self.first = torch.minimum(self.first, torch.where(wrong, index, BIG).min())
        self.peak = torch.maximum(self.peak, torch.maximum(re.abs().max(), im.abs().max()))

    def report(self):
        bad = int(self.bad)
        return {"compared": self.n, "bad": bad, "first_bad": int(self.first) if bad else None, "peak": int(self.peak)}


def compare_all(store, ops, chunk=CHUNK, salt=0):
    """Every element of the flat tensor `store` against evaluate(ops, ., salt); the chunk shrinks with the number of partners."""
    n = store.numel()
    step = max(min(n, chunk // leaves(ops)), 1)
    tally = Tally(store.device)
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        i = torch.arange(lo, hi, device=store.device)
        re, im = evaluate(ops, i, salt)
        tally.add(store[lo:hi], re, im, i)
    return tally.report()


def compare_sample(store, ops, sample, chunk=CHUNK // 2, salt=0):
    """The elements of `store` at the indices `sample` (an int64 tensor on its device) against evaluate(ops, .).  (Half the chunk
    of compare_all: a deep circuit keeps the partner and coefficient tensors of every level alive at once.)"""
    step = max(min(sample.numel(), chunk // leaves(ops)), 1)
    tally = Tally(store.device)
    for lo in range(0, sample.numel(), step):
        i = sample[lo:lo + step]
        re, im = evaluate(ops, i, salt)
        tally.add(store[i], re, im, i)
    return tally.report()


def assert_exact(report, ops, dtype, label=""):
    """The conditions of the module docstring, then equality."""
    print(f"{label}: compared {report['compared']} elements, {leaves(ops)} hash evaluations each, largest |expected component| "
          f"{report['peak']} (a-priori bound {bound(ops)}, limit {LIMIT[dtype]}), mismatches {report['bad']}"
          + (f", the first at memory index {report['first_bad']}" if report["bad"] else ""))
    assert bound(ops) < LIMIT[dtype] and report["peak"] < LIMIT[dtype], label
    assert report["bad"] == 0, label


def hash_norm2(n, device, chunk=CHUNK, salt=0):
    """sum |a|^2 of the hash state of n elements, a Python int."""
    total = torch.zeros((), dtype=torch.int64, device=device)
    for lo in range(0, n, chunk):
        f, g = hash_index(torch.arange(lo, min(lo + chunk, n), device=device), salt)
        total += (f * f).sum() + (g * g).sum()
    return int(total)


def expected_norm2(store, ops, chunk=CHUNK):
    """sum |expected|^2 over the whole array, a Python int, by direct evaluation (prod T hash evaluations per element)."""
    n = store.numel()
    step = max(min(n, chunk // leaves(ops)), 1)
    total = 0
    for lo in range(0, n, step):
        re, im = evaluate(ops, torch.arange(lo, min(lo + step, n), device=store.device))
        total += int((re * re).sum() + (im * im).sum())
    return total


def expectation_sums(n, strings, device, chunk=CHUNK):
    """[(numerator, imaginary part)] of <a|P|a> = sum_i conj(a[i]) (P a)[i] for every P = {memory bit: letter} of `strings` on
    the hash state of n elements, and sum |a|^2: Python ints from chunked int64 sums (every term is at most 128, the sums stay
    below 2^40)."""
    step = max(min(n, chunk // 2), 1)
    num = torch.zeros((len(strings), 2), dtype=torch.int64, device=device)
    den = torch.zeros((), dtype=torch.int64, device=device)
    ops = [[PauliStep(0, 1, s)] for s in strings]
    for lo in range(0, n, step):
        i = torch.arange(lo, min(lo + step, n), device=device)
        f, g = hash_index(i)
        den += (f * f).sum() + (g * g).sum()
        for k, op in enumerate(ops):
            re, im = evaluate(op, i)
            num[k, 0] += (f * re).sum() + (g * im).sum()
            num[k, 1] += (f * im).sum() - (g * re).sum()
    num = num.cpu().tolist()
    return [(int(a), int(b)) for a, b in num], int(den)


def inner_sums(n, ops_a, salt_a, ops_b, salt_b, M=None, device="cpu", chunk=CHUNK):
    """(Re, Im) of sum_i conj(A[i]) (M B)[i] over n elements, Python ints: A = ops_a on the hash state of salt_a, B = ops_b on
    that of salt_b, M an optional Gate (or any op) applied to B.  Chunked int64 sums; sum_i (|Re A| + |Im A|)(|Re B| + |Im B|)
    bounds every partial sum of either part in any order and has to stay below 2^53."""
    ops_a, ops_b = list(ops_a), list(ops_b) + ([M] if M is not None else [])
    step = max(min(n, chunk // max(leaves(ops_a), leaves(ops_b))), 1)
    re = im = cover = 0
    for lo in range(0, n, step):
        i = torch.arange(lo, min(lo + step, n), device=device)
        ar, ai = evaluate(ops_a, i, salt_a)
        br, bi = evaluate(ops_b, i, salt_b)
        re += int((ar * br).sum() + (ai * bi).sum())               # conj(a) b = (ar br + ai bi) + i (ar bi - ai br)
        im += int((ar * bi).sum() - (ai * br).sum())
        cover += int(((ar.abs() + ai.abs()) * (br.abs() + bi.abs())).sum())
    assert cover < 1 << 53, f"partial sums up to {cover} are not exact in float64"
    return re, im


def _digits(i, bits):
    """The digit class of the indices i: the value of the memory bits `bits`, the first the most significant."""
    k = len(bits)
    r = torch.zeros_like(i)
    for j, b in enumerate(bits):
        r.bitwise_or_(((i >> b) & 1) << (k - 1 - j))
    return r


def marginal_sums(n, bits, device="cpu", chunk=CHUNK):
    """The 2^k Python ints sum |a|^2 of the hash state of n elements per digit class of the memory bits `bits` (the first the
    most significant digit).  Their total, which bounds every partial sum, has to stay below 2^53."""
    bits = [int(b) for b in bits]
    out = torch.zeros(2 ** len(bits), dtype=torch.int64, device=device)
    for lo in range(0, n, chunk):
        i = torch.arange(lo, min(lo + chunk, n), device=device)
        f, g = hash_index(i)
        out.index_add_(0, _digits(i, bits), f.mul_(f).add_(g.mul_(g)))
    out = [int(v) for v in out.cpu().tolist()]
    assert sum(out) < 1 << 53
    return out


def rdm_sums(n, bits, device="cpu", chunk=CHUNK):
    """(Re, Im), two 2^k x 2^k lists of Python ints, of rho[i, j] = sum_r a[i, r] conj(a[j, r]) of the hash state of n elements:
    i, j the digit classes of the memory bits `bits` (the first the most significant digit), r every other bit.  Per chunk of r
    the four products F F^T, G G^T, G F^T, F G^T are float64 matrix products of integers in [-8, 7] over at most 2^25 / 2^k
    columns -- partial sums below 2^31, exact -- and the chunks are added in int64.  |rho[i, j]| and every partial sum of it are
    bounded by the trace, which has to stay below 2^53."""
    bits = [int(b) for b in bits]
    k, D = len(bits), 2 ** len(bits)
    spread = torch.tensor([sum(((c >> (k - 1 - j)) & 1) << b for j, b in enumerate(bits)) for c in range(D)], dtype=torch.int64,
                          device=device)
    rest = n >> k
    step = max(min(rest, chunk // D), 1)
    re = torch.zeros((D, D), dtype=torch.int64, device=device)
    im = torch.zeros((D, D), dtype=torch.int64, device=device)
    for lo in range(0, rest, step):
        r = torch.arange(lo, min(lo + step, rest), device=device)
        for b in sorted(bits):                                      # a zero at every kept bit, from the lowest up
            r = ((r >> b) << (b + 1)) | (r & ((1 << b) - 1))
        f, g = hash_index((spread[:, None] | r[None, :]).reshape(-1))
        f, g = f.view(D, -1).double(), g.view(D, -1).double()
        re += (f @ f.T + g @ g.T).to(torch.int64)                   # a conj(b) = (fa fb + ga gb) + i (ga fb - fa gb)
        gf = g @ f.T
        im += (gf - gf.T).to(torch.int64)
    re, im = re.cpu().tolist(), im.cpu().tolist()
    assert sum(re[c][c] for c in range(D)) < 1 << 53
    return re, im


def sample_indices(n, elem_size, count, seed=1):
    """int64 CPU tensor of `count` distinct memory indices below n: the first and the last tile of 1024 elements, the 2048
    elements on either side of byte offsets 2^31 and 2^32 and of element index 2^31 (where the array reaches them), the rest
    pseudo-random."""
    must = [torch.arange(0, min(1024, n)), torch.arange(max(n - 1024, 0), n)]
    for edge in ((1 << 31) // elem_size, (1 << 32) // elem_size, 1 << 31):
        if edge < n:
            must.append(torch.arange(max(edge - 2048, 0), min(edge + 2048, n)))
    must = torch.unique(torch.cat(must))
    gen = torch.Generator().manual_seed(seed)
    rest = torch.randint(0, n, (2 * count,), generator=gen, dtype=torch.int64)
    both = torch.cat([must, rest])
    uniq, first = np.unique(both.numpy(), return_index=True)
    keep = np.sort(first)[:max(count, must.numel())]              # the edges first, then random indices in drawing order
    return both[torch.from_numpy(keep)]


# ---- what every large-state GPU test begins and ends with ---------------------------------------------------------------------
DEV = "cuda:0"
GIB = 1 << 30
SIZES = {"c64-n30": (torch.complex64, 30), "c128-n29": (torch.complex128, 29), "c64-n32": (torch.complex64, 32)}


class Budget:
    """The hash state of one size and the memory it may cost: the state (`arrays` of them) plus 4 GiB."""

    def __init__(self, size, arrays=1):
        import pytest
        self.dtype, self.n = SIZES[size]
        self.size = size
        elem = 8 if self.dtype == torch.complex64 else 16
        self.allowed = arrays * (elem << self.n) + 4 * GIB
        torch.cuda.empty_cache()
        free, _ = torch.cuda.mem_get_info(torch.device(DEV))
        if free < self.allowed:
            pytest.skip(f"needs {self.allowed / GIB:.1f} GiB of free device memory ({arrays} array(s) of {(elem << self.n) / GIB:.0f} GiB "
                        f"and 4 GiB of chunk temporaries), {free / GIB:.1f} GiB free")
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        self.before = torch.cuda.memory_allocated()
        self.store = fill(torch.empty(1 << self.n, dtype=self.dtype, device=DEV))

    def view(self):
        return self.store.view((2,) * self.n)

    def close(self, label):
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - self.before
        print(f"{label}: peak device memory {rise / GIB:.2f} GiB, allowed {self.allowed / GIB:.2f} GiB")
        self.store = None
        torch.cuda.empty_cache()
        assert rise <= self.allowed, label


def norm_invariant(b, ops, label):
    import artensor_amd as A
    want = scale2(ops) * hash_norm2(1 << b.n, DEV)
    got = A.norm2(b.store)
    print(f"{label}: norm2 {got!r}, scale2 {scale2(ops)} * sum |hash|^2 = {want} ({want / 2 ** 53:.3f} of 2^53)")
    assert want < 1 << 53 and got == float(want), label


# ---- the circuits of the large-state tests, written on MEMORY bits -----------------------------------------------------------
X = np.array([[0, 1], [1, 0]], dtype=np.complex128)
Y = np.array([[0, -1j], [1j, 0]], dtype=np.complex128)
Z = np.diag([1, -1]).astype(np.complex128)
S = np.diag([1, 1j]).astype(np.complex128)
CNOT = np.eye(4)[[0, 1, 3, 2]].astype(np.complex128)
SWAP = np.eye(4)[[0, 2, 1, 3]].astype(np.complex128)
CZ = np.diag([1, 1, 1, -1]).astype(np.complex128)
ISWAP = np.array([[1, 0, 0, 0], [0, 0, 1j, 0], [0, 1j, 0, 0], [0, 0, 0, 1]], dtype=np.complex128)
# dense, asymmetric (a transposed matrix or swapped targets give another result), components in {-2..2}
G1 = np.array([[1 + 2j, -2], [1j, 2 - 1j]])
G2 = np.array([[1 + 2j, -1, 2j, 2 - 1j], [-2, 1 - 1j, 1, -1j], [2 - 2j, 1j, -1 + 1j, 2], [1, -2 + 1j, -2j, 1 + 1j]])
# dense Gaussian-integer multiples of unitaries: sum |out|^2 = scale2 sum |in|^2, exactly
U5 = np.array([[2, 1], [-1, 2]], dtype=np.complex128)                      # U U^H = 5
U2 = np.array([[1, 1j], [1j, 1]], dtype=np.complex128)                     # 2
V2 = np.array([[1, -1], [1, 1]], dtype=np.complex128)                      # 2
D10A = CNOT @ np.kron(U5, U2)                                              # 10
D10B = np.kron(U2, U5.T) @ ISWAP                                           # 10
D4 = np.kron(V2, U2) @ CNOT                                                # 4


def dims_of(n, bits):
    """Dims of a contiguous [2]*n tensor: dim d is memory bit n - 1 - d."""
    return tuple(n - 1 - b for b in bits)


def api_gates(n, gates):
    return [(m, dims_of(n, bits)) for m, bits in gates]


def gate_ops(gates):
    return [Gate(m, bits) for m, bits in gates]


def whole_gate_cases(n):
    """name -> (gates on memory bits, max_rank): one call each, every element compared.  At n = 32, 'top2' and 'top2-rev-r0'
    are the pair of bits 31 and 30, on either side of element index 2^31."""
    t = n - 1
    return {
        "top": ([(G1, (t,))], None),
        "top2": ([(G2, (t, t - 1))], None),
        "top2-rev-r0": ([(G2, (t - 1, t))], 0),
        "top-piece": ([(G2, (t, 5)), (G1, (t,))], None),
        "piece-top-r0": ([(G2, (6, t))], 0),
        "top-reg": ([(G2, (t, 1))], None),
        "reg-top-r0": ([(G2, (0, t)), (G1, (t - 1,))], 0),
    }


def fused_gates(n):
    """30 gates, five of them dense (scale2 10 10 4 10 4 = 16 000, growth 6 6 4 6 4), the others signed permutations; the high
    targets are bits 22, 23, 24, 26, n - 2 and n - 1."""
    t, u = n - 1, n - 2
    return [
        (CNOT, (t, 3)), (D10A, (t, u)), (X, (26,)), (ISWAP, (26, 0)), (S, (u,)),
        (D10B, (5, 26)), (SWAP, (t, 24)), (Y, (24,)), (CZ, (22, t)), (CNOT, (1, 24)),
        (D4, (24, 22)), (Z, (23,)), (ISWAP, (23, u)), (X, (12,)), (CNOT, (23, 26)),
        (D10A, (23, 0)), (SWAP, (7, 22)), (S, (26,)), (CZ, (u, 9)), (Y, (t,)),
        (D4, (u, 24)), (CNOT, (22, 23)), (ISWAP, (2, 15)), (X, (u,)), (SWAP, (26, t)),
        (CZ, (1, 0)), (Y, (22,)), (CNOT, (24, t)), (S, (4,)), (SWAP, (23, 22)),
    ]


def api_string(n, letters):
    """{dim: letter} of a contiguous [2]*n tensor from {memory bit: letter}."""
    return {n - 1 - b: l for b, l in letters.items()}


def api_steps(n, steps):
    return [(alpha, beta, api_string(n, letters)) for alpha, beta, letters in steps]


def step_ops(steps):
    return [PauliStep(*s) for s in steps]


def random_letters(rng, n, flips, z_share=0.4):
    """X or Y on the bits `flips`, Z on about z_share of the other bits -- spread over ALL bits, at least one in the lowest and
    one in the highest third, so the sign is the parity of index bits from inside the tile to the top."""
    out = {int(b): str(rng.choice(["X", "Y"])) for b in flips}
    for b in range(n):
        if b not in out and rng.random() < z_share:
            out[b] = "Z"
    for third in (range(n // 3), range(n - 1, n - 1 - n // 3, -1)):
        if not any(out.get(b) == "Z" for b in third):
            out[next(b for b in third if b not in out)] = "Z"
    return out


def whole_steps(n):
    """Two steps with general Gaussian-integer (alpha, beta): flips on the two top bits and inside the tile, Z everywhere."""
    rng = np.random.default_rng(1000 + n)
    return [(2 - 1j, 1 + 2j, random_letters(rng, n, (n - 1, 4))), (-1j, 2, random_letters(rng, n, (n - 2, n - 1, 12, 0)))]


def fused_steps(n):
    """30 steps: seven dense ones with Re(conj(alpha) beta) = 0 (multiples of unitaries: scale2 5 5 4 2 5 5 2 = 10 000, growth
    3 3 4 2 3 3 2), the others signed permutations beta P; flips on bits 22, 23, 24, 26, n - 2, n - 1 and below."""
    rng = np.random.default_rng(2000 + n)
    high = [n - 1, n - 2, 26, 24, 23, 22]
    dense = {1: (1, 2j), 5: (2, -1j), 9: (1 + 1j, 1 - 1j), 13: (1, 1j), 17: (1, -2j), 21: (2, 1j), 25: (1, -1j)}
    steps = []
    for k in range(30):
        flips = {int(b) for b in rng.choice(high, size=1 + k % 2, replace=False)} | ({int(rng.integers(0, 22))} if k % 3 == 0 else set())
        alpha, beta = dense.get(k, (0, (1, 1j, -1, -1j)[k % 4]))
        steps.append((alpha, beta, random_letters(rng, n, sorted(flips))))
    return steps


def sum_terms(n):
    """Seven terms in four groups; the flip masks of the groups differ in bits n - 1, n - 2, n - 5 and n - 7."""
    rng = np.random.default_rng(3000 + n)
    flips = [(n - 1, 3), (n - 1, 3), (n - 2, n - 5, 0), (n - 2, n - 5, 0), (n - 7,), (), (n - 7,)]
    coeff = [1 + 2j, -2, 1j, 2 - 1j, -1 - 1j, 2j, 1]
    return [(c, random_letters(rng, n, f)) for c, f in zip(coeff, flips)]


def expectation_strings(n):
    """One string per class of the expectation kernel."""
    rng = np.random.default_rng(4000 + n)
    full = {b: str(rng.choice(["X", "Y", "Z"])) for b in range(n)}
    full[n - 1] = "Y"
    return [{b: "Z" for b in range(22, n)}, {n - 1: "X"}, {3: "X", 7: "Y", n - 1: "Z"}, full]


def expectation_batch(n):
    """17 strings of one group (equal flip positions): a second pass runs."""
    rng = np.random.default_rng(5000 + n)
    return [random_letters(rng, n, (n - 1, 24, 5, 1)) for _ in range(17)]


# ---- the wide gates, channels and two-state circuits of test_wide_ops_large_gpu.py -------------------------------------------
TOFFOLI = np.eye(8)[[0, 1, 2, 3, 4, 5, 7, 6]].astype(np.complex128)        # controls: the first two listed bits
FREDKIN = np.eye(8)[[0, 1, 2, 3, 4, 6, 5, 7]].astype(np.complex128)        # control: the first listed bit
CCZ = np.diag([1, 1, 1, 1, 1, 1, 1, -1]).astype(np.complex128)
XZY = np.kron(X, np.kron(Z, Y))
PERM8 = (0, 7, 1, 6, 2, 4, 3, 5)


def _conjugated(m, perm):
    out = np.zeros_like(m)
    out[np.ix_(perm, perm)] = m
    return out


def _rows_shuffled(m, a, c):
    """Row r of the result is row (a r + c) mod 2^k of m (a odd): a permutation times m."""
    return m[[(a * r + c) % m.shape[0] for r in range(m.shape[0])]]


def _kron(*ms):
    out = np.eye(1, dtype=np.complex128)
    for m in ms:
        out = np.kron(out, m)
    return out


# two non-zeros per row (growth 5), asymmetric, and no Kronecker product: the partner of a row differs from it in 2 or 3 digits
PAIR3 = _conjugated(np.kron(np.eye(4), G1), PERM8)
# dense Gaussian-integer multiples of unitaries on 3, 4, 5 bits: ONE factor with components up to 2, so every component lies in
# {-2..2} (x 1 or i); scale2 20 40 80, growth 12 24 48; the row shuffle makes them no Kronecker products
W3 = _rows_shuffled(_kron(U5, U2, V2), 3, 5)
W4 = _rows_shuffled(_kron(U5.T, U2, V2, U2.T), 7, 3)
W5 = _rows_shuffled(_kron(U5, U2.T, V2.T, U2, V2), 11, 13)
WIDE = {3: W3, 4: W4, 5: W5}


def wide_whole_cases(n):
    """name -> gates on memory bits, ONE CALL EACH, every element compared (at most 4 hash evaluations per element)."""
    t, u = n - 1, n - 2
    return {
        "toffoli": [(TOFFOLI, (t, 3, u))],
        "fredkin": [(FREDKIN, (5, t, 12))],
        "ccz": [(CCZ, (u, t, 0))],
        "pair3": [(PAIR3, (t, 13, 1)), (PAIR3, (1, 13, t))],                # the second call in reversed target order
    }


def wide_sampled_cases(n):
    """(k, where) -> target bits of the dense gate WIDE[k]: all above the tile of 2^12 / 2^11 elements, all inside it, mixed (at
    n = 32 the mixed sets hold bits 31 and 30, on either side of element index 2^31)."""
    t, u = n - 1, n - 2
    return {
        (3, "above"): (t, 20, u), (4, "above"): (u, 25, t, 14), (5, "above"): (22, t, 13, u, 17),
        (3, "inside"): (2, 9, 0), (4, "inside"): (7, 1, 10, 4), (5, "inside"): (3, 10, 0, 8, 5),
        (3, "mixed"): (t, 6, u), (4, "mixed"): (u, 2, t, 15), (5, "mixed"): (9, t, 19, 0, u),
    }


def wide_fused_parts(n):
    """Eight parts: four stretches of two or three signed-permutation gates of fused_gates alternating with the wide gates W3,
    W4, W5 and a Fredkin.  Three dense gates: 8 * 16 * 32 = 2^12 hash evaluations per element, scale2 20 * 40 * 80 = 64 000,
    growth 12 * 24 * 48."""
    t, u = n - 1, n - 2
    g = fused_gates(n)
    return [[g[0], g[2], g[3]], (W3, (t, 13, 1)), [g[6], g[7]], (W4, (4, u, 23, t)), [g[8], g[9], g[11]],
            (W5, (u, 7, t, 0, 26)), [g[12], g[14]], (FREDKIN, (24, t, 2))]


def wide_fused_gates(n):
    return [x for part in wide_fused_parts(n) for x in (part if isinstance(part, list) else [part])]


CHANNEL_PROBS = [0.4, 0.3, 0.2, 0.1]
CHANNEL_UNITARIES = [np.eye(8, dtype=np.complex128), TOFFOLI, XZY, FREDKIN]
MEASURE1 = np.array([[2, 1j], [-1 + 1j, 1]])                               # the measured matrices of the pair circuit
MEASURE2 = np.array([[2, 0, 1j, 0], [0, 1 - 1j, 0, -1], [0, -2j, 1, 0], [1, 0, 0, 1j]])


def pair_gates(n):
    t, u = n - 1, n - 2
    return [(G2, (t, 5)), (G1, (u,)), (CNOT, (3, t))], [None, MEASURE1, MEASURE2]


def pair_max_ranks(dtype):
    """The max_rank values of the two-state cases: the default and 0, and for complex128 (whose two-state default is 1, cut
    like 0 for these circuits) also 2, the plan that fuses the steps on the two top bits into one run."""
    return [None, 0] if dtype == torch.complex64 else [None, 0, 2]


def bits_of(view, dims):
    """Memory bits of the dims of a [2]*n view, from its strides."""
    return tuple(int(view.stride(d)).bit_length() - 1 for d in dims)


def dims_on(view, bits):
    """The dims of a [2]*n view that lie on the memory bits `bits`."""
    where = {int(view.stride(d)).bit_length() - 1: d for d in range(view.dim())}
    return tuple(where[b] for b in bits)
