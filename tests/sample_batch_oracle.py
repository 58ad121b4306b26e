"""numpy restatement of trajectories.sample_batch (include/artn.h: BITSTRING SAMPLING PER TRAJECTORY).  Nothing here shares code
with the library: the address of (trajectory, local index), the float64 terms, the 4-element segment sums, the prefix inside a
block and over the blocks of a trajectory in the contract's order of additions, the target multiply, the pick rule with its
zero-element and beyond-total cases, and the deposit of the local index and of b into the memory index.

complex64: a term is r*r + m*m in float64; both products are exact there (24-bit significands), so the one rounding of the sum is
the kernel's single rounding and random states are restated bit for bit.  complex128: the kernel forms fma(r, r, m*m), which has
no numpy form; random complex128 states can NOT be restated bit for bit here.  complex128 is therefore checked on Gaussian-integer
states (every operation exact) and, on the device, against the unbatched call only."""
import numpy as np

THREADS, PREFIX_THREADS = 256, 1024


def block_bits(M):
    """artn_born_plan(2^M).block_bits"""
    return min(14, max(10, M - 16))


def local_positions(n_bits, fields):
    """The memory bits that are no batch bit, ascending: local bit j is the j-th of them.  fields: [(shift, width, pos)]."""
    taken = {s + k for s, w, _ in fields for k in range(w)}
    return [b for b in range(n_bits) if b not in taken]


def deposit(v, positions):
    """Bit j of v (ints or an int64 array) to memory bit positions[j]."""
    v = np.asarray(v, dtype=np.int64)
    out = np.zeros_like(v)
    for j, p in enumerate(positions):
        out |= ((v >> j) & 1) << p
    return out


def trajectory_address(b, fields):
    """The bits of b (ints or an int64 array) deposited into the fields."""
    b = np.asarray(b, dtype=np.int64)
    out = np.zeros_like(b)
    for s, w, pos in fields:
        out |= ((b >> pos) & ((1 << w) - 1)) << s
    return out


def address_table(n_bits, fields):
    """int64 [B, 2^M]: the memory index of (trajectory b, local index l)."""
    local = local_positions(n_bits, fields)
    B = 1 << sum(w for _, w, _ in fields)
    return trajectory_address(np.arange(B), fields)[:, None] | deposit(np.arange(1 << len(local)), local)[None, :]


def terms(x):
    """|x|^2 in float64: r*r + m*m (see the module docstring for what that means per dtype)."""
    r, m = x.real.astype(np.float64), x.imag.astype(np.float64)
    return r * r + m * m


def hierarchical_prefix(x, threads):
    """Thread k scans its K consecutive entries (local), one thread scans the per-thread totals (base, exclusive), then
    P[i] = base[k] + local[i] for k > 0 and local[i] for k = 0.  len(x) a multiple of threads, or below it (K = 1)."""
    n = x.size
    K = -(-n // threads)
    pad = np.zeros(K * threads, dtype=np.float64)
    pad[:n] = x
    local = np.cumsum(pad.reshape(threads, K), axis=1)         # (np.cumsum adds sequentially: 0 + x0, + x1 ...)
    base = np.concatenate([[0.0], np.cumsum(local[:-1, -1])])
    out = local.copy()
    out[1:] = base[1:, None] + local[1:]
    return out.reshape(-1)[:n]


def segment_sums(t):
    q = t.reshape(-1, 4)
    return ((q[:, 0] + q[:, 1]) + q[:, 2]) + q[:, 3]


def scan(t_row):
    """(segment prefixes per block [nb_t, S4], row prefix [nb_t]) of the 2^M float64 terms of one trajectory."""
    M = int(t_row.size).bit_length() - 1
    bb = block_bits(M)
    nbt = max(1, t_row.size >> bb)
    padded = np.zeros(nbt << bb, dtype=np.float64)
    padded[:t_row.size] = t_row
    pseg = np.stack([hierarchical_prefix(segment_sums(blk), THREADS) for blk in padded.reshape(nbt, -1)])
    return pseg, hierarchical_prefix(pseg[:, -1].copy(), PREFIX_THREADS), padded


def pick(pseg, prefix, padded, target):
    """(local index, raw |a|^2) for one target; (-1, 0.0) where no block claims it."""
    total = prefix[-1]
    grew = [j for j in range(prefix.size) if prefix[j] > (prefix[j - 1] if j else 0.0)]
    j = next((j for j in grew if (prefix[j - 1] if j else 0.0) <= target and (target < prefix[j] or prefix[j] == total)), None)
    if j is None:
        return -1, 0.0
    lo_t = prefix[j - 1] if j else 0.0
    r = target - lo_t
    P, ptot = pseg[j], pseg[j][-1]
    beyond = not ptot > r
    s = int(np.flatnonzero(P >= ptot)[0]) if beyond else int(np.flatnonzero(P > r)[0])
    run, chosen, lastnz = (P[s - 1] if s else 0.0), -1, -1
    i0 = (j * P.size + s) * 4
    for e in range(4):
        t = padded[i0 + e]
        run = run + t
        if t > 0.0:
            lastnz = e
            if chosen < 0 and not beyond and run > r:
                chosen = e
    if chosen < 0:
        chosen = lastnz
    return (-1, 0.0) if chosen < 0 else (i0 + chosen, float(padded[i0 + chosen]))


def sample_rows(mem, n_bits, fields, uniforms):
    """(flat int64 [B, S], raw |a|^2 float64 [B, S], norms float64 [B]) for the MEMORY-order array `mem` of 2^n_bits elements and
    uniforms [B, S] in any order: what artn_sample_batch leaves, scattered back to the uniforms' positions."""
    table = address_table(n_bits, fields)
    B, S = uniforms.shape
    assert table.shape[0] == B
    flat, raw, norms = np.full((B, S), -1, dtype=np.int64), np.zeros((B, S)), np.zeros(B)
    for b in range(B):
        pseg, prefix, padded = scan(terms(mem[table[b]]))
        norms[b] = prefix[-1]
        for s in range(S):
            l, p = pick(pseg, prefix, padded, uniforms[b, s] * norms[b])
            flat[b, s], raw[b, s] = (-1 if l < 0 else table[b, l]), p
    return flat, raw, norms


def finish(flat, raw, norms):
    """What sample_batch_flat returns from those: prob = raw / norm, dead trajectories (norm 0 or not finite) -1 / NaN."""
    with np.errstate(all="ignore"):
        prob = raw / norms[:, None]
    live = (np.isfinite(norms) & (norms > 0))[:, None]
    return np.where(live, flat, -1), np.where(live, prob, np.nan), norms
