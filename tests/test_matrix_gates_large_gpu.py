"""One matrix-core case past 4 GiB, by the method of tests/exact_state.py: 2^30 complex64 amplitudes (8 GiB) filled with the
integer hash state, a six-qubit signed permutation and a six-qubit dense small-integer gate whose targets include memory bits 29
and 0, the values compared as exact integers at 2^18 sampled indices (the edges of 2^31 and 2^32 bytes among them), and the
norm of the whole array.  A tile base formed in 32 bits would wrap at element 2^29."""
import types

import numpy as np
import pytest
import torch

import artensor_amd as A
import exact_state as E

pytestmark = pytest.mark.gpu
GIB = 1 << 30


class Gate6(E.Gate):
    """exact_state.Gate without its limit of five bits (its terms() is generic in k)."""

    def __init__(self, matrix, bits):
        self.bits = tuple(int(b) for b in bits)
        k = len(self.bits)
        assert 1 <= k <= 7 and len(set(self.bits)) == k
        m = np.asarray(matrix, dtype=np.complex128).reshape(2 ** k, 2 ** k)
        re, im = E._gauss(m, "gate")
        rows = [[c for c in range(2 ** k) if re[r, c] or im[r, c]] for r in range(2 ** k)]
        self.T = max(1, max(len(x) for x in rows))
        self.col = [[rows[r][t] if t < len(rows[r]) else r for r in range(2 ** k)] for t in range(self.T)]
        self.cre = [[int(re[r, rows[r][t]]) if t < len(rows[r]) else 0 for r in range(2 ** k)] for t in range(self.T)]
        self.cim = [[int(im[r, rows[r][t]]) if t < len(rows[r]) else 0 for r in range(2 ** k)] for t in range(self.T)]
        self.growth = int((np.abs(re) + np.abs(im)).sum(axis=1).max())
        g = m @ m.conj().T
        self.scale2 = int(round(g[0, 0].real)) if np.array_equal(g, g[0, 0].real * np.eye(2 ** k)) else None


def test_six_qubit_gates_on_bits_29_and_0_of_an_8_gib_state():
    n = 30
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(torch.device(E.DEV))
    if free < 10 * GIB:
        pytest.skip(f"needs 10 GiB of free device memory, {free / GIB:.1f} GiB free")
    rng = np.random.default_rng(6)
    perm = np.zeros((64, 64), dtype=np.complex128)
    perm[np.arange(64), rng.permutation(64)] = rng.choice([1, -1, 1j, -1j], size=64)
    dense = E._rows_shuffled(E._kron(E.U5, E.U2, E.V2, E.U2.T, E.V2.T, E.U2), 11, 29)       # components in {-2..2}: 160 x a unitary
    gates = [(perm, (29, 3, 0, 17, 12, 28)), (dense, (0, 29, 13, 5, 28, 20))]
    ops = [Gate6(m, b) for m, b in gates]
    assert E.bound(ops) < E.LIMIT[torch.complex64] and E.scale2(ops) == 160
    store = E.fill(torch.empty(1 << n, dtype=torch.complex64, device=E.DEV))
    view = store.view((2,) * n)
    for m, b in gates:
        A.apply_matrix_gate_(view, m, E.dims_of(n, b))
    sample = E.sample_indices(1 << n, 8, 1 << 18).to(E.DEV)
    E.assert_exact(E.compare_sample(store, ops, sample), ops, torch.complex64, "matrix gates, k = 6, 2^30 complex64")
    E.norm_invariant(types.SimpleNamespace(n=n, store=store), ops, "matrix gates, k = 6, 2^30 complex64")
