"""Numpy complex128 references for the two-state circuits and adjoint gradients of artensor_amd/adjoint.py.  They work axis by
axis through oracle_string of tests/test_pauli_apply_gpu.py and share nothing with the mask formula of the kernels."""
import numpy as np

from test_pauli_apply_gpu import oracle_string
from test_pauli_evolve_gpu import step_pair


def oracle_pair(lam, phi, steps, measure=None):
    """(t, lam', phi'): t[k] = <lam| P_k |phi> immediately before step k (0 where measure[k] is false), then the step on both."""
    lam, phi = np.asarray(lam).astype(np.complex128), np.asarray(phi).astype(np.complex128)
    t = np.zeros(len(steps), dtype=np.complex128)
    for k, step in enumerate(steps):
        alpha, beta = step_pair(step)
        p_phi, p_lam = oracle_string(phi, step[-1]), oracle_string(lam, step[-1])
        if measure is None or measure[k]:
            t[k] = np.vdot(lam.reshape(-1), p_phi.reshape(-1))
        phi, lam = alpha * phi + beta * p_phi, alpha * lam + beta * p_lam
    return t, lam, phi


def _forward(amps0, rotations):
    phi = np.asarray(amps0).astype(np.complex128)
    for theta, p in rotations:
        phi = np.cos(theta) * phi - 1j * np.sin(theta) * oracle_string(phi, p)
    return phi


def _hamiltonian(phi, terms):
    out = np.zeros_like(phi)
    for c, p in terms:
        out = out + c * oracle_string(phi, p)
    return out


def oracle_energy(amps0, rotations, terms, normalize=True):
    phi = _forward(amps0, rotations)
    e = np.vdot(phi.reshape(-1), _hamiltonian(phi, terms).reshape(-1)).real
    return e / np.vdot(amps0, amps0).real if normalize else e


def oracle_gradient(amps0, rotations, terms, params=None, normalize=True):
    """(E, grad) by the adjoint formula: dE/dtheta_k = 2 Im <lam_k| P_k |phi_k>, swept from the last rotation to the first."""
    rotations = list(rotations)
    params = list(range(len(rotations))) if params is None else list(params)
    phi = _forward(amps0, rotations)
    lam = _hamiltonian(phi, terms)
    e = np.vdot(phi.reshape(-1), lam.reshape(-1)).real
    back = [(-theta, p) for theta, p in reversed(rotations)]
    t, _, _ = oracle_pair(lam, phi, back)
    grad = np.zeros(max(params) + 1 if params else 0)
    for k, p in enumerate(params):
        if p >= 0:
            grad[p] += 2.0 * t[len(rotations) - 1 - k].imag
    if normalize:
        n2 = np.vdot(amps0, amps0).real
        e, grad = e / n2, grad / n2
    return e, grad
