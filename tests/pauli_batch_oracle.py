"""numpy oracle of trajectories.pauli_expectation_batch.  Values: the logical array is cut into trajectories by
trajectories_oracle.slices and every slice goes through the axis-by-axis oracle of test_pauli_gpu.py (np.flip, a sign multiply,
np.tensordot) -- nothing of the mask formula.  Exact values: the same walk in int64 on Gaussian-integer states.  Plan: a pure-Python
restatement of what include/artn.h promises (local masks by bit compression, the local tile count T, the chunk count C, the
units), written from the header's text and sharing no code with the library."""
import numpy as np

import trajectories_oracle as TO
from test_pauli_gpu import letters, oracle

TILE_BITS, MAX_GRID, TERMS = 10, 2048, 16
LINE_BIT = {"c64": 4, "c128": 3}


# ---- values ---------------------------------------------------------------------------------------------------------------------
def slice_string(p, n_dims, batch_dims):
    """The string of a slice: the letters of the dims that are no batch dims, in their order; every batch dim must carry I."""
    full = letters(p, n_dims)
    assert all(full[x] == "I" for x in batch_dims), (p, batch_dims)
    return "".join(c for x, c in enumerate(full) if x not in batch_dims)


def expect(logical, strings, batch_dims):
    """(values float64 [B, n_terms], norms float64 [B]) of the LOGICAL array, raw (not normalised)."""
    sl = TO.slices(logical, batch_dims)
    sub = [slice_string(p, logical.ndim, batch_dims) for p in strings]
    vals = np.zeros((sl.shape[0], len(strings)))
    norms = np.zeros(sl.shape[0])
    for b in range(sl.shape[0]):
        for k, p in enumerate(sub):
            vals[b, k], norms[b] = oracle(sl[b], p)
    return vals, norms


# ---- exact integers ---------------------------------------------------------------------------------------------------------------
def exact_bound(local_bits, bound):
    """The largest absolute value a partial sum of a trajectory of 2^local_bits elements can take: every term conj(a[j]) a[i] has
    parts of at most 2 bound^2, and a pass that takes half the index space counts it twice."""
    return 2 ** local_bits * 2 * bound * bound * 2


def exact_state(rng, shape, kind, bound=2 ** 10):
    """Gaussian integers with |re|, |im| <= bound (exact in float32 up to 2^24)."""
    re, im = (rng.integers(-bound, bound + 1, size=shape) for _ in range(2))
    a = (re + 1j * im).astype(np.complex64 if kind == "c64" else np.complex128)
    assert np.abs(a.real).max() <= bound and np.abs(a.imag).max() <= bound and (a.real == re).all() and (a.imag == im).all()
    return a


def _times_i(re, im):
    return -im, re


def exact_oracle(a_logical, p):
    """(<a|P|a>, <a|a>) in int64, axis by axis: X flips, Z signs, Y|0> = i|1>, Y|1> = -i|0>.  The imaginary part must vanish."""
    re, im = np.rint(a_logical.real).astype(np.int64), np.rint(a_logical.imag).astype(np.int64)
    assert (re == a_logical.real).all() and (im == a_logical.imag).all()
    pr, pi = re, im
    for d, c in enumerate(letters(p, re.ndim)):
        sign = np.ones(re.ndim, dtype=int)
        sign[d] = 2
        s = np.array([1, -1], dtype=np.int64).reshape(sign)
        if c == "X":
            pr, pi = np.flip(pr, axis=d), np.flip(pi, axis=d)
        elif c == "Z":
            pr, pi = pr * s, pi * s
        elif c == "Y":                                         # (Y phi)[0] = -i phi[1], (Y phi)[1] = i phi[0]
            fr, fi = _times_i(np.flip(pr, axis=d), np.flip(pi, axis=d))
            pr, pi = fr * -s, fi * -s
    val_re = int((re * pr + im * pi).sum())
    val_im = int((re * pi - im * pr).sum())
    assert val_im == 0
    return val_re, int((re * re + im * im).sum())


def exact_expect(logical, strings, batch_dims):
    sl = TO.slices(logical, batch_dims)
    sub = [slice_string(p, logical.ndim, batch_dims) for p in strings]
    vals = np.zeros((sl.shape[0], len(strings)), dtype=np.int64)
    norms = np.zeros(sl.shape[0], dtype=np.int64)
    for b in range(sl.shape[0]):
        for k, p in enumerate(sub):
            vals[b, k], norms[b] = exact_oracle(sl[b], p)
    return vals, norms


# ---- the plan ---------------------------------------------------------------------------------------------------------------------
def _log2(x):
    x = int(x)
    assert x >= 1 and x & (x - 1) == 0, x
    return x.bit_length() - 1


def compress(mask, keep_bits):
    """The bits of `mask` at the positions keep_bits (ascending), packed."""
    return sum(((mask >> b) & 1) << j for j, b in enumerate(keep_bits))


def plan(shape, strides, strings, batch_dims):
    """What pauli_batch_info has to report, from the header's text."""
    nd = len(shape)
    n_bits = sum(_log2(e) for e in shape)
    batch_bits = sorted(_log2(strides[x]) + j for x in batch_dims for j in range(_log2(shape[x])))
    local = [b for b in range(n_bits) if b not in batch_bits]
    M, bb = len(local), len(batch_bits)
    xm, zm, ny = [], [], []
    for p in strings:
        x = z = y = 0
        for d, c in enumerate(letters(p, nd)):
            if c == "I":
                continue
            assert shape[d] == 2 and d not in batch_dims
            bit = 1 << _log2(strides[d])
            x |= bit if c in "XY" else 0
            z |= bit if c in "ZY" else 0
            y += c == "Y"
        xm.append(x), zm.append(z), ny.append(y)
    order = []
    for x in xm:
        if x not in order:
            order.append(x)
    group = [order.index(x) for x in xm]
    launches = sum(-(-group.count(g) // TERMS) for g in range(len(order)))
    T = 2 ** (M - TILE_BITS) if M >= TILE_BITS else 1
    cap = max(1, MAX_GRID >> bb)
    C, Ch = min(T, cap), min(max(T // 2, 1), cap)
    B = 2 ** bb
    if M >= TILE_BITS:
        units = B * C
    else:
        units = 1 if B == 1 else -(-B // 2 ** (TILE_BITS - M))
    return {"xmask": xm, "zmask": zm, "n_y": ny, "group": group, "local_xmask": [compress(x, local) for x in xm],
            "local_zmask": [compress(z, local) for z in zm], "n_groups": len(order), "n_launches": launches, "B": B, "n": 2 ** n_bits,
            "batch_bits": bb, "local_bits": M, "tile_bits": min(TILE_BITS, M), "tiles": T, "chunks": C, "chunks_halved": Ch,
            "units": units, "grid": min(units, MAX_GRID), "workspace_bytes": B * C * (TERMS + 1) * 8,
            "out_bytes": B * (len(strings) + 1) * 8, "fields": TO.fields(shape, strides, batch_dims)}
