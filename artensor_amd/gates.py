"""IN-PLACE circuits of dense one- and two-qubit gates on an amplitude tensor on the device (C ABI: artn_gates_query,
artn_gates_pack, artn_gates_apply), fused into runs that read and write the state once.

A circuit is an ordered list of gates `(matrix, dims)`: `dims` a tuple of one or two distinct dims of `amps`, each of extent 2
(negative dims count from the end), `matrix` anything np.asarray turns into a complex [2^k, 2^k] array (or [2] * 2k, reshaped; a
CPU torch tensor works too) -- any matrix, unitary or not.  The convention is the one reduced_density_matrix uses, the first
listed dim the most significant digit: for dims = (d0, d1)

    new[.., i0, .., i1, ..] = sum_{j0, j1} U[2 i0 + i1, 2 j0 + j1] a[.., j0, .., j1, ..]

The tensor is updated in place, in its own permuted layout, and never copied; gates are never reordered.  The functions take what
pauli.py takes -- a dense GPU tensor of complex64 or complex128 -- and keep its arithmetic contract: every output component is
formed in float64 in one fixed order and rounded once, so the result is bit for bit independent of where the runs are cut.  There
is no CPU fallback.
"""
import numpy as np
import torch

from . import _native
from ._state import _RunCircuit, _checked, _desc, _dtype_code, _interleaved, _max_rank, _ptr, _run_keys, _run_pack, _run_query

__all__ = ["apply_gates_", "apply_gate_", "GateCircuit", "gate_circuit_info", "gates_from_bonds", "run_circuit", "merge_gates"]


def _matrix(matrix, k, what):
    m = np.asarray(matrix.detach().cpu().numpy() if isinstance(matrix, torch.Tensor) else matrix).astype(np.complex128)
    if m.size != 4 ** k:
        raise ValueError(f"{what}: a matrix of {m.size} entries for {k} dims (2^k x 2^k expected)")
    return m.reshape(2 ** k, 2 ** k)


def _split_gates(gates, n_dims):
    """(int32 k [n], int32 dims [n, 2], float64 mat [n, 32]) of gates = [(matrix, dims), ...]; a gate on a number of dims the
    library does not take keeps its k and a zero matrix, so that the library refuses it."""
    gates = list(gates)
    if not gates:
        raise ValueError("at least one gate is needed")
    k = np.zeros(len(gates), dtype=np.int32)
    dims = np.full((len(gates), 2), -1, dtype=np.int32)
    mat = np.zeros((len(gates), 32), dtype=np.float64)
    for g, gate in enumerate(gates):
        if not isinstance(gate, (tuple, list)) or len(gate) != 2:
            raise ValueError(f"gate {g}: (matrix, dims) expected, got {gate!r}")
        gd = [int(gate[1])] if isinstance(gate[1], (int, np.integer)) else [int(x) for x in gate[1]]
        k[g] = len(gd)
        for j, x in enumerate(gd[:2]):
            dims[g, j] = x + n_dims if -n_dims <= x < 0 else x
        if k[g] in (1, 2):
            m = _matrix(gate[0], int(k[g]), f"gate {g}")
            mat[g, :2 * m.size] = _interleaved(m)
    return k, np.ascontiguousarray(dims), mat


# what a circuit query writes: bits, run, slot_mask, local, run_rank, run_pivot
_GATE_ARRAYS = ((np.int32, 2),) + ((np.int32, 0),) * 4 + ((np.int32, _native.GATES_MAX_RANK),)


def _gates_query(d, k, dims, mat, max_rank, arrays=False):
    return _run_query("artn_gates_query", _native.ArtnGatesInfo(), d, (k, dims, mat), max_rank, _GATE_ARRAYS, arrays)


def _gate_keys(k, bits, run, slot, local):
    """The per-gate lists of gate_circuit_info."""
    return {"bits": [tuple(int(b) for b in bits[g, :k[g]]) for g in range(len(k))], "run": [int(v) for v in run],
            "slot_mask": [int(v) for v in slot], "local": [bool(v) for v in local]}


def gate_circuit_info(shape, strides, gates, dtype=torch.complex64, max_rank=None):
    """Host-only: how a circuit of gates = [(matrix, dims), ...] is cut into runs.  Per gate: bits (the memory bits of its dims, in
    the order listed), run, slot_mask and local (True: the gate needs no other thread -- a diagonal matrix or targets in memory
    bits 0-1).  Per run: run_rank and run_pivot (its high target bits, ascending).  n_runs = n_launches, the effective max_rank,
    table_bytes, bytes_read = bytes_written = n_runs * bytes of the state."""
    _dtype_code(dtype, "gate_circuit_info")
    k, dims, mat = _split_gates(gates, len(shape))
    info, *per_gate, rank, pivot = _gates_query(_desc(shape, strides, dtype), k, dims, mat, _max_rank(max_rank), arrays=True)
    return {**_gate_keys(k, *per_gate), **_run_keys(info, rank, run_pivot=pivot)}


def _gates_pack(d, k, dims, mat, max_rank):
    """The circuit table (include/artn.h) as a uint8 numpy array."""
    return _run_pack(_gates_query, "artn_gates_pack", d, (k, dims, mat), max_rank)


class GateCircuit(_RunCircuit):
    """An ordered list of gates [(matrix, dims), ...] for tensors of one layout.  Validates, cuts the runs, packs the table and
    copies it to `device` once; circ(amps) then updates amps IN PLACE with one launch per run and returns it.  max_rank: a run
    holds blocks of up to 2^max_rank tiles of 2^10 elements in LDS (None: 64 KiB per workgroup; 0: one launch per gate with a
    target above the tile; a two-qubit gate on two such targets always gets a block of four tiles)."""

    def __init__(self, shape, strides, dtype, gates, device, max_rank=None):
        (self._k, self._dims, _), _ = self._build(shape, strides, dtype, device, max_rank, lambda nd: _split_gates(gates, nd), _gates_query,
                                                  "artn_gates_pack")
        self.n_gates = self._n

    def __call__(self, amps):
        return self._run("gates.GateCircuit", "artn_gates_apply", amps, _ptr(self._k), _ptr(self._dims), None)   # (mat: in the table)


def apply_gates_(amps, gates, max_rank=None):
    """The circuit `gates` (see GateCircuit) applied to amps in place; returns amps.  Every call plans, packs and uploads the
    table again: build a GateCircuit once to apply the same circuit repeatedly."""
    _checked(amps, "gates.apply_gates_")
    return GateCircuit(amps.shape, amps.stride(), amps.dtype, gates, amps.device, max_rank)(amps)


def apply_gate_(amps, matrix, dims):
    """amps <- U amps for one gate, in place: one launch, no second buffer.  (Plans and uploads per call, as apply_gates_; a list
    of gates in ONE call is also what lets them share a pass over the state.)"""
    _checked(amps, "gates.apply_gate_")
    return GateCircuit(amps.shape, amps.stride(), amps.dtype, [(matrix, dims)], amps.device)(amps)


def gates_from_bonds(gates, n_qubits):
    """The gate tensors state_vec takes -- each `(array, inds)` or an object with `.array` / `.inds`, `inds` bond labels
    "layer-qubit", the input bonds of the circuit "0-q" -- as [(matrix, dims)] with dim q = qubit q.  A gate's bonds that are the
    current bonds of their qubits are its inputs, the others its outputs; dims lists the qubits in the order of the output bonds."""
    wire = {q: f"0-{q}" for q in range(int(n_qubits))}
    out = []
    for g, gate in enumerate(gates):
        array, inds = (gate.array, list(gate.inds)) if hasattr(gate, "inds") else (gate[0], list(gate[1]))
        inds = [str(x) for x in inds]
        qubit = [int(x.split("-")[1]) for x in inds]
        ins = {qubit[p]: p for p in range(len(inds)) if wire.get(qubit[p]) == inds[p]}
        outs = {qubit[p]: p for p in range(len(inds)) if p not in ins.values()}
        if len(ins) * 2 != len(inds) or set(ins) != set(outs):
            raise ValueError(f"gate {g}: bonds {inds} do not pair one input and one output per qubit (current bonds "
                             f"{[wire.get(q) for q in sorted(set(qubit))]})")
        qs = sorted(outs, key=lambda q: outs[q])
        k = len(qs)
        a = np.asarray(array.detach().cpu().numpy() if isinstance(array, torch.Tensor) else array)
        m = a.reshape((2,) * (2 * k)).transpose([outs[q] for q in qs] + [ins[q] for q in qs]).reshape(2 ** k, 2 ** k)
        out.append((m, tuple(qs)))
        for q in qs:
            wire[q] = inds[outs[q]]
    return out


def run_circuit(gates, n_qubits, dtype=torch.complex64, device="cuda", max_rank=None):
    """gates = [(matrix, dims), ...] with dim q = qubit q, applied in place to |0..0>: a contiguous tensor of shape (2,) * n_qubits
    is the only state-sized allocation."""
    _dtype_code(dtype, "run_circuit")
    state = torch.zeros(2 ** int(n_qubits), dtype=dtype, device=device)
    _native.require_gpu(state, "gates.run_circuit")
    state[0] = 1
    state = state.reshape((2,) * int(n_qubits))
    return apply_gates_(state, gates, max_rank) if len(gates) else state


def _embed(m1, pos):
    """A one-qubit matrix on digit `pos` of a two-qubit gate (0: the first listed dim, the most significant digit)."""
    return np.kron(m1, np.eye(2)) if pos == 0 else np.kron(np.eye(2), m1)


def merge_gates(gates):
    """Opt-in, pure Python: a shorter list with the same product.  A one-qubit gate is absorbed into the neighbouring gate on its
    qubit (the previous one, or the next two-qubit one) when no other gate on that qubit lies between them, and consecutive
    gates on identical dims are multiplied; products are formed in complex128.  The order of the remaining gates is kept.  This
    changes rounding (fewer, different matrices), so nothing calls it implicitly."""
    out, last = [], {}                                         # out: [matrix, dims] or None (absorbed); last[q]: index into out
    for g, (matrix, dims) in enumerate(gates):
        dims = (int(dims),) if isinstance(dims, (int, np.integer)) else tuple(int(x) for x in dims)
        if len(dims) not in (1, 2) or len(set(dims)) != len(dims):
            raise ValueError(f"gate {g}: one or two distinct dims expected, got {dims}")
        m = _matrix(matrix, len(dims), f"gate {g}")
        prev = [last.get(q) for q in dims]
        if len(dims) == 1 and prev[0] is not None:             # into the last gate on this qubit
            j = prev[0]
            pm, pd = out[j]
            out[j][0] = (m if len(pd) == 1 else _embed(m, pd.index(dims[0]))) @ pm
            continue
        if len(dims) == 2 and prev[0] is not None and prev[0] == prev[1] and out[prev[0]][1] == dims:
            out[prev[0]][0] = m @ out[prev[0]][0]
            continue
        if len(dims) == 2:                                     # pending one-qubit gates on either qubit move into this one
            for pos, j in enumerate(prev):
                if j is not None and len(out[j][1]) == 1:
                    m = m @ _embed(out[j][0], pos)
                    out[j] = None
        out.append([m, dims])
        for q in dims:
            last[q] = len(out) - 1
    return [(m, d) for m, d in (x for x in out if x is not None)]
