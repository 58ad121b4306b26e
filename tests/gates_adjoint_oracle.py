"""Numpy complex128 references for the two-state gate circuits and adjoint gradients of artensor_amd/gate_adjoint.py.  They work
on the LOGICAL array through np.tensordot over a gate's dims and share nothing with the memory-bit arithmetic of the kernels; the
Hamiltonian goes axis by axis through oracle_string of tests/test_pauli_apply_gpu.py."""
import numpy as np

from test_pauli_apply_gpu import oracle_string


def _dims(dims, nd):
    dims = [int(dims)] if isinstance(dims, (int, np.integer)) else [int(x) for x in dims]
    return [x % nd for x in dims]


def oracle_gate(psi, m, dims):
    """U on the logical array: the first listed dim is the most significant digit of the row and column index."""
    dims = _dims(dims, psi.ndim)
    k = len(dims)
    u = np.asarray(m, dtype=np.complex128).reshape((2,) * (2 * k))
    return np.moveaxis(np.tensordot(u, psi, axes=(list(range(k, 2 * k)), dims)), list(range(k)), dims)


def oracle_gate_pair(lam, phi, gates, measure=None):
    """(t, lam', phi'): t[k] = <lam| M_k |phi> immediately before gate k (0 where measure[k] is None), then the gate on both."""
    lam, phi = np.asarray(lam).astype(np.complex128), np.asarray(phi).astype(np.complex128)
    t = np.zeros(len(gates), dtype=np.complex128)
    for k, (m, dims) in enumerate(gates):
        if measure is not None and measure[k] is not None:
            t[k] = np.vdot(lam.reshape(-1), oracle_gate(phi, measure[k], dims).reshape(-1))
        phi, lam = oracle_gate(phi, m, dims), oracle_gate(lam, m, dims)
    return t, lam, phi


def _hamiltonian(phi, terms):
    out = np.zeros_like(phi)
    for c, p in terms:
        out = out + c * oracle_string(phi, p)
    return out


def oracle_gate_energy(psi0, gates, terms, normalize=True):
    """E = <psi0| U^+ H U |psi0>; gates entries (U, dims) or (U, dU, dims)."""
    phi = np.asarray(psi0).astype(np.complex128)
    for gate in gates:
        phi = oracle_gate(phi, gate[0], gate[-1])
    e = np.vdot(phi.reshape(-1), _hamiltonian(phi, terms).reshape(-1)).real
    return e / np.vdot(psi0, psi0).real if normalize else e


def oracle_gate_gradient(psi0, gates, terms, params=None, normalize=True):
    """(E, grad) by the adjoint formula dE/dtheta = 2 Re <lam_k| dU_k U_k^+ |phi_k>, swept from the last gate to the first.
    params: one integer per PARAMETRISED gate (U, dU, dims), -1 = constant."""
    gates = list(gates)
    slot, n_par = [], 0
    for gate in gates:
        slot.append(n_par if len(gate) == 3 else None)
        n_par += len(gate) == 3
    params = list(range(n_par)) if params is None else list(params)
    assert len(params) == n_par
    phi = np.asarray(psi0).astype(np.complex128)
    for gate in gates:
        phi = oracle_gate(phi, gate[0], gate[-1])
    lam = _hamiltonian(phi, terms)
    e = np.vdot(phi.reshape(-1), lam.reshape(-1)).real
    grad = np.zeros(max(params) + 1 if params else 0)
    for g in range(len(gates) - 1, -1, -1):
        u = np.asarray(gates[g][0], dtype=np.complex128)
        u = u.reshape(int(round(np.sqrt(u.size))), -1)
        if slot[g] is not None and params[slot[g]] >= 0:
            m = np.asarray(gates[g][1], dtype=np.complex128).reshape(u.shape) @ u.conj().T
            grad[params[slot[g]]] += 2.0 * np.vdot(lam.reshape(-1), oracle_gate(phi, m, gates[g][-1]).reshape(-1)).real
        phi, lam = oracle_gate(phi, u.conj().T, gates[g][-1]), oracle_gate(lam, u.conj().T, gates[g][-1])
    if normalize:
        n2 = np.vdot(psi0, psi0).real
        e, grad = e / n2, grad / n2
    return e, grad
