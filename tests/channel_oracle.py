"""numpy restatement of artensor_amd/channel.py and of the draw of artn_channel_choose, float64: the oracle of
test_channel_cpu.py and test_channel_gpu.py.  It takes Kraus operators (or probabilities and unitaries) as plain arrays and
shares no code with the package.

States are LOGICAL arrays; the first listed dim is the most significant digit (measure_oracle's convention)."""
import math

import numpy as np

import measure_oracle as MO

FIXED, DIAGONAL, DENSE = "FIXED", "DIAGONAL", "DENSE"


def classify(kraus):
    """DIAGONAL where every operator has at most one non-zero entry per column, DENSE otherwise."""
    for k in kraus:
        k = np.asarray(k)
        if (np.count_nonzero(k, axis=0) > 1).any():
            return DENSE
    return DIAGONAL


def effects(kraus, form):
    """DIAGONAL: e_j[d] = sum_r |K_j[r, d]|^2; DENSE: E_j = K_j^+ K_j."""
    ks = [np.asarray(k, dtype=np.complex128) for k in kraus]
    if form == DIAGONAL:
        return [np.array([sum(abs(k[r, d]) ** 2 for r in range(k.shape[0])) for d in range(k.shape[1])]) for k in ks]
    return [k.conj().T @ k for k in ks]


def weights(form, packed, state, dims):
    """(w, trace): FIXED -- the given probabilities, trace None; DIAGONAL -- sum_d e_j[d] q[d]; DENSE -- sum_ab Re(E_j[a,b] rho[b,a]).
    Negative residue counts as 0."""
    if form == FIXED:
        return np.asarray(packed, dtype=np.float64).copy(), None
    if form == DIAGONAL:
        q = MO.probabilities(state, dims)
        w = np.array([float(np.dot(e, q)) for e in packed])
        return np.maximum(w, 0.0), float(np.cumsum(q)[-1])
    rho = MO.rdm(state, dims)
    w = np.array([float(np.sum((e * rho.T).real)) for e in packed])
    return np.maximum(w, 0.0), float(np.cumsum(np.diag(rho).real)[-1])


def choose(w, uniform):
    """The choice rule written out as a loop: the smallest j with w_j > 0 whose inclusive ascending running sum exceeds
    uniform * total, else the last j with w_j > 0; -1 where total is not finite or not > 0."""
    w = np.asarray(w, dtype=np.float64)
    total = 0.0
    for x in w:
        total += float(x)
    if not (math.isfinite(total) and total > 0.0):
        return -1
    thr, run, last = float(uniform) * total, 0.0, -1
    for j, x in enumerate(w):
        run += float(x)
        if x > 0.0:
            last = j
            if run > thr:
                return j
    return last


def boundaries(w):
    """The inclusive running sums: where the choice changes, as multiples of total."""
    return np.cumsum(np.asarray(w, dtype=np.float64))


def record(form, w, trace, uniform, renormalize=True):
    """(j, probability, total, scale) of the device's record."""
    total = float(np.cumsum(w)[-1])
    j = choose(w, uniform)
    if form != FIXED and not (math.isfinite(trace) and trace > 0.0):
        j = -1
    if j < 0:
        return -1, 0.0, total, 1.0
    scale = 1.0 if (form == FIXED or not renormalize) else math.sqrt(trace / w[j])
    return j, float(w[j] / total), total, scale


def current_matrix(matrix, scale):
    """Every component times scale, one float64 multiply each."""
    m = np.ascontiguousarray(matrix, dtype=np.complex128)
    return (m.view(np.float64) * np.float64(scale)).view(np.complex128).reshape(m.shape)


def block_mask(matrix):
    """Bit rb * nb + cb: block (rb, cb) of 8 x 8 entries (the whole matrix below 8 rows) has a non-zero."""
    m = np.asarray(matrix)
    rows = m.shape[0]
    r = min(rows, 8)
    nb = rows // r
    mask = 0
    for row in range(rows):
        for col in range(rows):
            if m[row, col] != 0:
                mask |= 1 << ((row // r) * nb + col // r)
    return mask


def op_flags(matrix):
    """1: nothing off the diagonal is non-zero; 2: exactly the identity."""
    m = np.asarray(matrix, dtype=np.complex128)
    diagonal = not np.count_nonzero(m - np.diag(np.diag(m)))
    identity = bool((m == np.eye(m.shape[0])).all())
    return (1 if diagonal else 0) | (2 if identity else 0)


PAULIS = [np.eye(2, dtype=np.complex128), np.array([[0, 1], [1, 0]], dtype=np.complex128),
          np.array([[0, -1j], [1j, 0]], dtype=np.complex128), np.array([[1, 0], [0, -1]], dtype=np.complex128)]


def pauli_string(digits):
    m = np.eye(1, dtype=np.complex128)
    for d in digits:
        m = np.kron(m, PAULIS[d])
    return m


def depolarizing(p, n=1):
    """(probabilities, unitaries): the identity with 1 - p, every other Pauli string with p / (4^n - 1), in the order
    I < X < Y < Z with the first qubit the most significant."""
    count = 4 ** n
    us = [pauli_string([(s >> (2 * (n - 1 - q))) & 3 for q in range(n)]) for s in range(count)]
    rest = p / (count - 1)
    return [1.0 - rest * (count - 1)] + [rest] * (count - 1), us


def amplitude_damping(gamma):
    return MO.amplitude_damping(gamma)


def phase_damping(lam):
    return [np.array([[1, 0], [0, math.sqrt(1 - lam)]], dtype=np.complex128), np.array([[0, 0], [0, math.sqrt(lam)]], dtype=np.complex128)]


def kraus_of_mixture(probs, unitaries):
    return [math.sqrt(p) * np.asarray(u, dtype=np.complex128) for p, u in zip(probs, unitaries)]


def apply_to_rho(rho, kraus, qubits, n):
    """sum_j K_j rho K_j^+ with K_j on `qubits` (first listed = most significant) of an n-qubit density matrix [2^n, 2^n]."""
    t = len(qubits)
    out = np.zeros_like(rho)
    r = rho.reshape((2,) * (2 * n))
    for k in kraus:
        kt = np.asarray(k, dtype=np.complex128).reshape((2,) * (2 * t))
        x = np.tensordot(kt, r, axes=(list(range(t, 2 * t)), list(qubits)))
        x = np.moveaxis(x, list(range(t)), list(qubits))
        x = np.tensordot(kt.conj(), x, axes=(list(range(t, 2 * t)), [n + q for q in qubits]))
        x = np.moveaxis(x, list(range(t)), [n + q for q in qubits])
        out += x.reshape(rho.shape)
    return out
