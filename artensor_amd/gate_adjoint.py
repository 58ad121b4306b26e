"""Adjoint gradients of circuits of dense one- and two-qubit gates (C ABI: artn_gates_adjoint_query, artn_gates_adjoint_pack,
artn_gates_adjoint): the in-place circuits of gates.py applied to TWO states at once, with the transition element
t_k = <lam| M_k |phi> of every measured gate taken immediately before the gate.

With U = U_K ... U_1, phi_k = U_k ... U_1 psi0, lam_k = (U_K ... U_{k+1})^+ H phi_K and E = <phi_K| H |phi_K>, a gate U_k(theta)
with derivative dU_k has

    dE/dtheta = 2 Re <lam_k| dU_k |phi_{k-1}> = 2 Re <lam_k| M_k |phi_k>,      M_k = dU_k U_k^+,

so one forward circuit, one H|phi> and one backward sweep of the reversed circuit of the U_k^+ give every derivative.  For
U = exp(-i theta P), M = -i P and this is adjoint.adjoint_gradient's 2 Im <lam| P |phi>.

After a call both tensors are bit for bit what apply_gates_ leaves on each alone, for every max_rank and every measure pattern.
The transition elements are sums in float64 in a fixed order: bit-identical from run to run for one plan; the order follows the
blocks of the runs, so they may differ in the last bits between max_rank values.  There is no CPU fallback.
"""
import numpy as np
import torch

from . import _native
from ._state import _PairCircuit, _checked, _desc, _dtype_code, _interleaved, _max_rank, _ptr, _run_keys, _run_query
from .adjoint import _adjoint_sweep
from .gates import _GATE_ARRAYS, GateCircuit, _gate_keys, _matrix, _split_gates

__all__ = ["gate_adjoint_info", "GatePairCircuit", "apply_gates_pair_", "gate_adjoint_gradient", "parametric_gate"]


def _split_measure(measure, k):
    """(uint8 flags [n], float64 mmat [n, 32]) of measure = None or one entry per gate (None or a matrix of the gate's size)."""
    n = k.shape[0]
    flags, mmat = np.zeros(n, dtype=np.uint8), np.zeros((n, 32), dtype=np.float64)
    if measure is None:
        return flags, mmat
    measure = list(measure)
    if len(measure) != n:
        raise ValueError(f"measure: one entry per gate expected ({n}), got {len(measure)}")
    for g, m in enumerate(measure):
        if m is None or k[g] not in (1, 2):
            continue
        m = _matrix(m, int(k[g]), f"measure of gate {g}")
        flags[g] = 1
        mmat[g, :2 * m.size] = _interleaved(m)
    return flags, mmat


def _pair_query(d, k, dims, mat, mmat, flags, max_rank, arrays=False):
    return _run_query("artn_gates_adjoint_query", _native.ArtnGatesAdjointInfo(), d, (k, dims, mat, mmat, flags), max_rank, _GATE_ARRAYS,
                      arrays)


def gate_adjoint_info(shape, strides, gates, dtype=torch.complex64, measure=None, max_rank=None):
    """Host-only: how a two-state circuit is cut into runs (the cuts of gate_circuit_info at the same effective max_rank; the
    default and the maximum lie one below the single-state ones).  The per-gate and per-run lists of gate_circuit_info, `measure`,
    n_measured, n_runs, n_launches = n_runs + 1 (the finish), table_bytes, workspace_bytes and bytes_read = bytes_written =
    2 * n_runs * bytes of a state."""
    _dtype_code(dtype, "gate_adjoint_info")
    k, dims, mat = _split_gates(gates, len(shape))
    flags, mmat = _split_measure(measure, k)
    info, *per_gate, rank, pivot = _pair_query(_desc(shape, strides, dtype), k, dims, mat, mmat, flags, _max_rank(max_rank), arrays=True)
    return {**_gate_keys(k, *per_gate), "measure": [bool(f) for f in flags], **_run_keys(info, rank, run_pivot=pivot)}


class GatePairCircuit(_PairCircuit):
    """The gates of a GateCircuit for TWO tensors of one layout: validates, cuts the runs, packs the table and copies it to
    `device` once; the workspace is allocated per call, so an instance holds no state that two calls share.  measure: None (no
    gate is measured) or one entry per gate, None or a matrix M of the gate's size (any matrix).  circ(lam, phi, device=False)
    updates both IN PLACE (one launch per run and a finish launch) and returns t[k] = <lam| M_k |phi> taken immediately before
    gate k, 0 for the gates that are not measured: complex128 numpy [K], or with device=True a float64 GPU tensor [K, 2] without a
    host synchronisation."""

    def __init__(self, shape, strides, dtype, gates, device, measure=None, max_rank=None):
        def split(n_dims):
            k, dims, mat = _split_gates(gates, n_dims)
            flags, mmat = _split_measure(measure, k)
            return k, dims, mat, mmat, flags

        (self._k, self._dims, *_), info = self._build(shape, strides, dtype, device, max_rank, split, _pair_query,
                                                      "artn_gates_adjoint_pack")
        self.n_gates, self.n_measured = self._n, info.n_measured

    def __call__(self, lam, phi, device=False):
        return self._run("gate_adjoint.GatePairCircuit", "artn_gates_adjoint", lam, phi, device, _ptr(self._k), _ptr(self._dims))


def apply_gates_pair_(lam, phi, gates, measure=None, max_rank=None, device=False):
    """The circuit `gates` (see gates.GateCircuit) applied to lam and to phi in place, and the transition elements of the measured
    gates (see GatePairCircuit)."""
    _checked(phi, "gate_adjoint.apply_gates_pair_")
    return GatePairCircuit(phi.shape, phi.stride(), phi.dtype, gates, phi.device, measure, max_rank)(lam, phi, device)


_P1 = {"x": np.array([[0, 1], [1, 0]], dtype=np.complex128), "y": np.array([[0, -1j], [1j, 0]], dtype=np.complex128),
       "z": np.diag([1, -1]).astype(np.complex128)}
_NAMES = ("rx", "ry", "rz", "phase", "rxx", "ryy", "rzz", "crx", "cry", "crz", "cphase")


def _rotation(p, theta):
    """exp(-i theta P / 2) and its derivative for an involution P."""
    c, s = np.cos(theta / 2), np.sin(theta / 2)
    eye = np.eye(p.shape[0], dtype=np.complex128)
    return c * eye - 1j * s * p, -0.5 * s * eye - 0.5j * c * p


def parametric_gate(name, theta, dims):
    """(U, dU/dtheta, dims) in complex128, an entry of gate_adjoint_gradient's `gates`.  rx ry rz: exp(-i theta P / 2); rxx ryy
    rzz: the same with P (x) P; phase: diag(1, e^{i theta}); crx cry crz cphase: the one-qubit gate on the second listed dim when
    the FIRST listed dim is 1."""
    name, theta = str(name).lower(), float(theta)
    dims = (int(dims),) if isinstance(dims, (int, np.integer)) else tuple(int(x) for x in dims)
    if name not in _NAMES:
        raise ValueError(f"parametric_gate: unknown gate {name!r}; one of {', '.join(_NAMES)}")
    base = name[1:] if name[0] == "c" else name
    if base == "phase":
        u, du = np.diag([1, np.exp(1j * theta)]), np.diag([0, 1j * np.exp(1j * theta)])
    elif len(base) == 2:
        u, du = _rotation(_P1[base[1]], theta)
    else:
        u, du = _rotation(np.kron(_P1[base[1]], _P1[base[2]]), theta)
    if name[0] == "c":
        one, zero = np.diag([0, 1]).astype(np.complex128), np.diag([1, 0]).astype(np.complex128)
        u, du = np.kron(zero, np.eye(2)) + np.kron(one, u), np.kron(one, du)
    if len(dims) != (1 if u.shape[0] == 2 else 2):
        raise ValueError(f"parametric_gate: {name} acts on {1 if u.shape[0] == 2 else 2} dims, got {dims}")
    return u.astype(np.complex128), du.astype(np.complex128), dims


def gate_adjoint_gradient(amps0, gates, terms, params=None, normalize=True, max_rank=None):
    """(E, grad) of E = <amps0| U^+ H U |amps0>, U = the gates applied in list order, H = sum_k c_k P_k with REAL c_k (terms =
    [(c_k, string_k), ...]), by the adjoint method: a forward GateCircuit, one PauliSumOperator, one overlap and one
    GatePairCircuit of the reversed gates U_k^+ measuring M_k = dU_k U_k^+.  gates: fixed (U, dims) or parametrised (U, dU, dims)
    entries (parametric_gate makes the latter); every U must be unitary to 1e-10, the sweep inverts by the conjugate transpose.
    params: None (one parameter per parametrised gate, in order) or one integer per PARAMETRISED gate: -1 marks a constant (not
    measured, no entry), equal indices share a parameter and their derivatives are added in float64 in gate order; grad is
    float64 numpy.  normalize=True divides E and grad by sum |amps0|^2.  max_rank: the two-state limits (3 / 2) apply to both
    circuits.  amps0 is never written; the peak extra memory is two state-sized tensors."""
    _native.require_gpu(amps0, "gate_adjoint.gate_adjoint_gradient")
    _checked(amps0, "gate_adjoint.gate_adjoint_gradient")
    gates, terms = list(gates), list(terms)
    if any(complex(c).imag != 0.0 for c, _ in terms):
        raise ValueError("gate_adjoint_gradient takes real coefficients (a Hermitian sum)")
    forward, back, back_measure, slot = [], [], [], []          # slot[g]: position among the parametrised gates, or None
    for g, gate in enumerate(gates):
        if not isinstance(gate, (tuple, list)) or len(gate) not in (2, 3):
            raise ValueError(f"gate {g}: (U, dims) or (U, dU, dims) expected")
        dims = (int(gate[-1]),) if isinstance(gate[-1], (int, np.integer)) else tuple(int(x) for x in gate[-1])
        if len(dims) not in (1, 2):
            raise ValueError(f"gate {g}: gate_adjoint_gradient takes gates on one or two dims, got {dims}")
        u = _matrix(gate[0], len(dims), f"gate {g}")
        if not np.all(np.isfinite(u.view(np.float64))) or np.abs(u @ u.conj().T - np.eye(u.shape[0])).max() > 1e-10:
            raise ValueError(f"gate {g}: the matrix is not unitary (max |U U^+ - I| above 1e-10); gate_adjoint_gradient inverts by the "
                             "conjugate transpose")
        forward.append((u, dims))
        back.append((u.conj().T, dims))
        if len(gate) == 3:
            slot.append(sum(s is not None for s in slot))
            back_measure.append(_matrix(gate[1], len(dims), f"derivative of gate {g}") @ u.conj().T)
        else:
            slot.append(None)
            back_measure.append(None)
    n_par = sum(s is not None for s in slot)
    if params is None:
        params = list(range(n_par))
    else:
        params = [int(p) for p in params]
        if len(params) != n_par or any(p < -1 for p in params):
            raise ValueError(f"params: one integer >= -1 per parametrised gate expected ({n_par})")
    back_measure = [m if s is not None and params[s] >= 0 else None for m, s in zip(back_measure, slot)]
    layout = (amps0.shape, amps0.stride(), amps0.dtype)
    # built first: max_rank follows the two-state limits, and a refusal comes before any work on the device
    sweep = GatePairCircuit(*layout, back[::-1], amps0.device, back_measure[::-1], max_rank)
    return _adjoint_sweep(amps0, lambda: GateCircuit(*layout, forward, amps0.device, max_rank), sweep, terms,
                          [-1 if s is None else params[s] for s in slot], lambda t: 2.0 * t.real, normalize)
