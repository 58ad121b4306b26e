"""Reduced density matrices of an amplitude tensor on the device, and what is read off them: purity, Renyi and von Neumann
entanglement entropies, expectation values of operators on a few dims (C ABI: artn_rdm_query, artn_rdm).

    rho[i, j] = sum_r amps[i, r] * conj(amps[j, r])

i and j run over the kept dims in the order they are asked for (the first one is the most significant digit), r over every
other dim: `rho.diagonal().real.reshape(kept shape)` is `marginal_probabilities(amps, keep)`.  The functions take what born.py
takes -- a dense GPU tensor of complex64 or complex128 in any permuted layout, never copied -- and keep its contract: products and
sums in float64 on the f64 matrix cores, a fixed summation order, bit-identical results from run to run, an exactly Hermitian
matrix.  At most 1024 kept states.  Power-of-two extents with at least 2^12 elements take the streaming matrix-core form; any
other shape (a bond dimension 3, a tiny state, more than 64 kept states with fewer than 16 dropped ones) takes the generic form,
one workgroup per matrix element with index arithmetic per term: correct, but its time grows as D^2 times the dropped size, so a
large state with one odd extent can run for minutes -- `rdm_info(...)["kernel"]` says which form a call takes before it runs.
There is no CPU fallback for anything that reads amplitudes; `entropy_of` works on a matrix
the caller already holds, wherever it lives.
"""
import ctypes
import math

import numpy as np
import torch

from . import _native
from ._state import _checked, _dtype_code
from .born import _marginal_desc

__all__ = ["rdm_info", "reduced_density_matrix", "purity", "renyi_entropy", "entanglement_entropy", "entropy_of", "expectation"]


def _query(d):
    info = _native.ArtnRdmInfo()
    _native.check(_native.lib().artn_rdm_query(ctypes.byref(d), ctypes.byref(info)))
    return info


def rdm_info(shape, strides, keep, dtype=torch.complex64):
    """Host-only: which form a reduced density matrix takes, its size D, the tile and split counts, the workspace and the
    FLOP it executes on the matrix cores (RuntimeError where the library refuses; TypeError for a dtype that is not complex)."""
    _dtype_code(dtype, "rdm_info")
    d, _ = _marginal_desc(shape, strides, keep, dtype)
    info = _query(d)
    return {"kernel": info.kernel, "panel_bits": info.panel_bits, "tiles": info.tiles, "splits": info.splits, "dim": info.dim,
            "workspace_bytes": info.workspace_bytes, "flops": info.flops}


def reduced_density_matrix(amps, keep, normalize=False):
    """complex128 [D, D] GPU tensor, D the product of the kept extents: amps (x) conj(amps) summed over every dim not in
    `keep`.  Unnormalised unless normalize=True (then divided by its trace).  keep=() gives the 1 x 1 norm."""
    _checked(amps, "rdm.reduced_density_matrix")
    d, keep = _marginal_desc(amps.shape, amps.stride(), keep, amps.dtype)
    info = _query(d)
    out = torch.empty((info.dim, info.dim), dtype=torch.complex128, device=amps.device)
    ws = torch.empty(max(info.workspace_bytes // 8, 2), dtype=torch.float64, device=amps.device)
    with torch.cuda.device(amps.device):
        _native.check(_native.lib().artn_rdm(ctypes.byref(d), amps.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                             info.workspace_bytes, _native.current_stream_ptr(amps.device)))
    return out / out.diagonal().real.sum() if normalize else out


def _host_matrix(rho):
    if isinstance(rho, torch.Tensor):
        rho = rho.detach().cpu().numpy()
    rho = np.asarray(rho)
    if rho.ndim != 2 or rho.shape[0] != rho.shape[1] or rho.shape[0] < 1:
        raise ValueError(f"a square matrix expected, got shape {rho.shape}")
    return rho.astype(np.complex128)


def entropy_of(rho, alpha=1, base=2):
    """Entropy of a density matrix the caller holds (torch, on any device, or numpy; normalised by its trace here).
    alpha=1: von Neumann, -tr rho log rho; otherwise Renyi, log(tr rho^alpha) / (1 - alpha).  The eigenvalues come from
    numpy.linalg.eigvalsh in float64 on the host and are clipped at 0."""
    m = _host_matrix(rho)
    tr = float(np.trace(m).real)
    if not tr > 0.0:
        raise ValueError("the matrix has no positive trace")
    lam = np.clip(np.linalg.eigvalsh((m + m.conj().T) * (0.5 / tr)), 0.0, None)
    alpha = float(alpha)
    if alpha < 0:
        raise ValueError("alpha must not be negative")
    if alpha == 1.0:
        nz = lam[lam > 0.0]
        h = float(-(nz * np.log(nz)).sum())
    elif math.isinf(alpha):
        h = float(-np.log(lam.max()))
    else:
        h = float(np.log((lam[lam > 0.0] ** alpha).sum()) / (1.0 - alpha))
    return max(h, 0.0) / math.log(base)


def purity(amps, keep):
    """tr rho^2 / (tr rho)^2 of the reduced density matrix of `keep` (1 for a product state across the cut)."""
    rho = reduced_density_matrix(amps, keep)
    tr = rho.diagonal().real.sum()
    return float((rho.real.square().sum() + rho.imag.square().sum()) / (tr * tr))   # rho is Hermitian: tr rho^2 = sum |rho_ij|^2


def renyi_entropy(amps, keep, alpha=2, base=2):
    """Renyi entropy of order alpha of the reduced state of `keep` (alpha=1: von Neumann)."""
    return entropy_of(reduced_density_matrix(amps, keep), alpha=alpha, base=base)


def entanglement_entropy(amps, keep, base=2):
    """Von Neumann entropy of the reduced state of `keep`: for a pure state, the entanglement entropy across the cut between
    `keep` and the other dims.  The D x D matrix goes to the host for its eigenvalues."""
    return entropy_of(reduced_density_matrix(amps, keep), alpha=1, base=base)


def expectation(amps, operator, dims):
    """tr(rho_dims @ operator) / tr(rho_dims) as a Python complex: the expectation value of an operator acting on `dims`
    (a [D, D] torch or numpy array in the digit order of reduced_density_matrix) in the state `amps`."""
    rho = reduced_density_matrix(amps, dims)
    op = torch.as_tensor(np.asarray(operator.detach().cpu() if isinstance(operator, torch.Tensor) else operator),
                         dtype=torch.complex128)
    if tuple(op.shape) != tuple(rho.shape):
        raise ValueError(f"operator of shape {tuple(op.shape)} for a reduced state of shape {tuple(rho.shape)}")
    op = op.to(rho.device)
    val = (rho * op.t()).sum() / rho.diagonal().real.sum()     # tr(rho op) = sum_ij rho_ij op_ji
    return complex(val.item())
