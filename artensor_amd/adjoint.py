"""Adjoint gradients of circuits of Pauli rotations (C ABI: artn_pauli_adjoint_query, artn_pauli_adjoint_pack,
artn_pauli_adjoint): the in-place circuits of pauli.py applied to TWO states at once, with the transition element
t_k = <lam| P_k |phi> of every measured step taken immediately before the step.

With U = U_K ... U_1, U_k = exp(-i theta_k P_k), phi_k = U_k ... U_1 psi0 and lam_k = (U_K ... U_{k+1})^+ H phi_K,

    dE/dtheta_k = 2 Im <lam_k| P_k |phi_k>      for E = <psi0| U^+ H U |psi0>,

so one forward circuit, one H|phi> and one backward sweep of the reversed circuit with negated angles give all K derivatives.

After a call both tensors are bit for bit what pauli_evolve_ leaves on each alone, for every max_rank and every measure pattern.
The transition elements are sums in float64 in a fixed order: bit-identical from run to run for one plan; the order follows the
blocks of the runs, so they may differ in the last bits between max_rank values.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _native
from ._state import _PairCircuit, _checked, _desc, _dtype_code, _max_rank, _ptr, _run_keys, _run_query
from .born import norm2, overlap
from .pauli import _STEP_ARRAYS, PauliCircuit, PauliSumOperator, _split_steps, _step_keys

__all__ = ["pauli_adjoint_info", "PauliPairCircuit", "pauli_evolve_pair_", "adjoint_gradient"]


def _flags(measure, n_steps):
    """uint8 [n_steps] (None: every step)."""
    if measure is None:
        return np.ones(n_steps, dtype=np.uint8)
    flags = np.ascontiguousarray([1 if bool(f) else 0 for f in measure], dtype=np.uint8)
    if flags.shape != (n_steps,):
        raise ValueError(f"measure: one flag per step expected ({n_steps}), got {len(flags)}")
    return flags


def _adjoint_query(d, ops, coeff, flags, max_rank, arrays=False):
    return _run_query("artn_pauli_adjoint_query", _native.ArtnPauliAdjointInfo(), d, (ops, coeff, flags), max_rank, _STEP_ARRAYS, arrays)


def pauli_adjoint_info(shape, strides, steps, dtype=torch.complex64, measure=None, max_rank=None):
    """Host-only: how a two-state circuit is cut into runs (the cuts of pauli_evolve_info at the same effective max_rank; the
    default and the maximum lie one below the single-state ones).  The per-step and per-run lists of pauli_evolve_info, `measure`,
    n_measured, n_runs, n_launches = n_runs + 1 (the finish), table_bytes, workspace_bytes and bytes_read = bytes_written =
    2 * n_runs * bytes of a state."""
    _dtype_code(dtype, "pauli_adjoint_info")
    coeff, ops = _split_steps(steps, len(shape))
    flags = _flags(measure, ops.shape[0])
    info, *per_step, rank, basis, pivot = _adjoint_query(_desc(shape, strides, dtype), ops, coeff, flags, _max_rank(max_rank), arrays=True)
    return {**_step_keys(coeff, *per_step), "measure": [bool(f) for f in flags], **_run_keys(info, rank, run_basis=basis, run_pivot=pivot)}


class PauliPairCircuit(_PairCircuit):
    """The steps of a PauliCircuit for TWO tensors of one layout: validates, cuts the runs, packs the table and copies it to
    `device` once; the workspace is allocated per call, so an instance holds no state that two calls share.  circ(lam, phi,
    device=False) updates both IN PLACE (one launch per run and a finish launch) and returns t[k] = <lam| P_k |phi> taken
    immediately before step k, 0 for the steps `measure` leaves out: complex128 numpy [K], or with device=True a float64 GPU
    tensor [K, 2] without a host synchronisation."""

    def __init__(self, shape, strides, dtype, steps, device, measure=None, max_rank=None):
        def split(n_dims):
            coeff, ops = _split_steps(steps, n_dims)
            return ops, coeff, _flags(measure, ops.shape[0])

        (self._ops, _, _), _ = self._build(shape, strides, dtype, device, max_rank, split, _adjoint_query, "artn_pauli_adjoint_pack")
        self.n_steps = self._n

    def __call__(self, lam, phi, device=False):
        return self._run("adjoint.PauliPairCircuit", "artn_pauli_adjoint", lam, phi, device, _ptr(self._ops))


def pauli_evolve_pair_(lam, phi, steps, measure=None, max_rank=None, device=False):
    """The circuit `steps` (see pauli.PauliCircuit) applied to lam and to phi in place, and the transition elements of the
    measured steps (see PauliPairCircuit)."""
    _checked(phi, "adjoint.pauli_evolve_pair_")
    return PauliPairCircuit(phi.shape, phi.stride(), phi.dtype, steps, phi.device, measure, max_rank)(lam, phi, device)


def _adjoint_sweep(amps0, forward, sweep, terms, index, derivative, normalize):
    """(E, grad), the second half of both adjoint gradients: a copy of amps0 through the circuit forward() builds, H|phi>, the energy,
    the sweep of the reversed circuit, and grad[index[k]] += derivative(t) of position k's transition element in float64, in
    circuit order (index -1: not a parameter)."""
    shape, strides, dtype, dev = amps0.shape, amps0.stride(), amps0.dtype, amps0.device
    phi = torch.empty_strided(shape, strides, dtype=dtype, device=dev)
    phi.copy_(amps0)
    forward()(phi)
    lam = PauliSumOperator(shape, strides, dtype, terms, dev)(phi)
    energy = overlap(phi, lam)[0].real
    t = sweep(lam, phi)
    grad = np.zeros(max(index, default=-1) + 1, dtype=np.float64)
    for k, p in enumerate(index):
        if p >= 0:
            grad[p] += derivative(t[len(index) - 1 - k])
    if normalize:
        n2 = norm2(amps0)
        energy, grad = energy / n2, grad / n2
    return energy, grad


def adjoint_gradient(amps0, rotations, terms, params=None, normalize=True, max_rank=None):
    """(E, grad) of E = <amps0| U^+ H U |amps0>, U = the rotations [(theta, string), ...] applied in list order, H = sum_k c_k P_k
    with REAL c_k (terms = [(c_k, string_k), ...]), by the adjoint method: a forward PauliCircuit, one PauliSumOperator, one overlap
    and one PauliPairCircuit of the reversed rotations with negated angles.  params: None (one parameter per rotation) or one
    integer per rotation: -1 marks a constant rotation (not measured, no entry), equal indices share a parameter and their
    derivatives are added in float64 in rotation order; grad is float64 numpy of length K or max(params) + 1.  normalize=True
    divides E and grad by sum |amps0|^2.  max_rank: the two-state limits (3 / 2) apply to both circuits.  amps0 is never written; the peak extra memory is two state-sized tensors."""
    _native.require_gpu(amps0, "adjoint.adjoint_gradient")
    _checked(amps0, "adjoint.adjoint_gradient")
    rotations, terms = list(rotations), list(terms)
    if any(complex(c).imag != 0.0 for c, _ in terms):
        raise ValueError("adjoint_gradient takes real coefficients (a Hermitian sum)")
    if any(not isinstance(r, (tuple, list)) or len(r) != 2 for r in rotations):
        raise ValueError("adjoint_gradient: rotations are (theta, string) pairs")
    n_rot = len(rotations)
    if params is None:
        params = list(range(n_rot))
    else:
        params = [int(p) for p in params]
        if len(params) != n_rot or any(p < -1 for p in params):
            raise ValueError(f"params: one integer >= -1 per rotation expected ({n_rot})")
    layout = (amps0.shape, amps0.stride(), amps0.dtype)
    back = [(-float(theta), string) for theta, string in reversed(rotations)]
    # built first: max_rank follows the two-state limits, and a refusal comes before any work on the device
    sweep = PauliPairCircuit(*layout, back, amps0.device, [p >= 0 for p in reversed(params)], max_rank)
    # the sweep runs with the negated angles: U_k^+ = exp(+i theta_k P_k), and t is taken before U_k^+ is applied
    return _adjoint_sweep(amps0, lambda: PauliCircuit(*layout, rotations, amps0.device, max_rank), sweep, terms, params,
                          lambda t: 2.0 * t.imag, normalize)
