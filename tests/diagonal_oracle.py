"""numpy restatement of the diagonal operators (artensor_amd/diagonal.py; include/artn.h: DIAGONAL OPERATORS): the plan (masks,
static or dynamic, groups in the order they first appear), the value contract -- f in float64, one plain addition per term
in the contract's order, so it can be compared with the device BIT FOR BIT -- and phase, multiply, moments and the
transition element in complex128 / float64.  Everything works on arrays in MEMORY order (index = sum of stride * digit)."""
import numpy as np

TILE_BITS = 10
MAX_GROUPS = 64


def parity(x):
    """Parity of the set bits of a uint64 array, as uint64 0 / 1."""
    x = np.array(x, dtype=np.uint64, copy=True)
    for s in (32, 16, 8, 4, 2, 1):
        x ^= x >> np.uint64(s)
    return x & np.uint64(1)


def zmask(shape, strides, string):
    """The memory-bit mask of a string over I and Z (a str of len(shape) letters, or a dict {dim: letter})."""
    nd = len(shape)
    items = enumerate(string) if isinstance(string, str) else ((int(d) % nd, l) for d, l in string.items())
    m = 0
    for dim, letter in items:
        assert letter.upper() in "IZ"
        if letter.upper() == "Z":
            assert int(shape[dim]) == 2
            m |= int(strides[dim])
    return m


class Plan:
    def __init__(self, shape, strides, terms):
        self.n = int(np.prod([int(e) for e in shape], dtype=np.int64))
        self.coeff = [float(c) for c, _ in terms]
        self.zm = [zmask(shape, strides, s) for _, s in terms]
        self.tb = min(TILE_BITS, self.n.bit_length() - 1)
        inside = (1 << self.tb) - 1
        self.lo, self.hi = [z & inside for z in self.zm], [z >> self.tb for z in self.zm]
        self.group, self.group_lo, self.members = [], [], []
        for k, (lo, hi) in enumerate(zip(self.lo, self.hi)):
            if hi == 0:
                self.group.append(-1)
                continue
            if lo not in self.group_lo:
                self.group_lo.append(lo)
                self.members.append([])
            g = self.group_lo.index(lo)
            self.group.append(g)
            self.members[g].append(k)
        self.static = [k for k, g in enumerate(self.group) if g < 0]
        self.G = len(self.group_lo)
        self.n_dynamic = len(self.zm) - len(self.static)
        self.table_bytes = 64 + (8 << self.tb) + 32 * self.G + 16 * self.n_dynamic

    def static_table(self):
        """S[l]: ((0.0 + s_1) + s_2) + ... over the static terms in the caller's order."""
        l = np.arange(1 << self.tb, dtype=np.uint64)
        S = np.zeros(1 << self.tb, dtype=np.float64)
        for k in self.static:
            S = S + self._signed(l, self.lo[k], self.coeff[k])
        return S

    @staticmethod
    def _signed(index, mask, c):
        """+c or -c (exact) by the parity of index & mask."""
        return np.where(parity(index & np.uint64(mask)) == 1, -np.float64(c), np.float64(c))

    def values(self):
        """f in memory order, float64 [n], in the contract's order of additions."""
        tiles = self.n >> self.tb
        h = np.arange(tiles, dtype=np.uint64)
        l = np.arange(1 << self.tb, dtype=np.uint64)
        f = np.broadcast_to(self.static_table(), (tiles, 1 << self.tb)).copy()
        for g in range(self.G):
            w = np.zeros(tiles, dtype=np.float64)
            for k in self.members[g]:
                w = w + self._signed(h, self.hi[k], self.coeff[k])
            sigma = parity(l & np.uint64(self.group_lo[g])) == 1
            f = f + np.where(sigma[None, :], -w[:, None], w[:, None])
        return f.reshape(self.n)


def values_plain(shape, strides, terms, index):
    """sum_k c_k (-1)^popcount(index & zmask_k) as a list of (c_k * sign) per term, for an exact sum by the caller."""
    out = []
    for c, s in terms:
        z = zmask(shape, strides, s)
        out.append(-float(c) if bin(index & z).count("1") & 1 else float(c))
    return out


def phase(a, f, gamma):
    """a * exp(-i (gamma * f)) in complex128 (the phase argument rounded once, as on the device)."""
    ph = np.float64(gamma) * f
    return a.astype(np.complex128) * (np.cos(ph) - 1j * np.sin(ph))


def multiply(a, f, dtype):
    """round(a * f): each component one float64 product, rounded once to the dtype."""
    a = a.astype(np.complex128)
    out = np.empty(a.shape, dtype=dtype)
    out.real = (a.real * f).astype(out.real.dtype)
    out.imag = (a.imag * f).astype(out.imag.dtype)
    return out


def moments(a, f):
    """([sum p, sum p f, sum p f^2], [sum p, sum p |f|, sum p f^2]) in float64: the values and the scales of their bounds."""
    a = a.astype(np.complex128)
    p = a.real * a.real + a.imag * a.imag
    return (np.array([p.sum(), (p * f).sum(), (p * f * f).sum()]),
            np.array([p.sum(), (p * np.abs(f)).sum(), (p * f * f).sum()]))


def transition(lam, f, phi):
    """(sum conj(lam) f phi, sum |lam| |f| |phi|)."""
    lam, phi = lam.astype(np.complex128), phi.astype(np.complex128)
    return complex((lam.conj() * f * phi).sum()), float((np.abs(lam) * np.abs(f) * np.abs(phi)).sum())
