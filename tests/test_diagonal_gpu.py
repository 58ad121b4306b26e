"""The diagonal operators on the GPU (artensor_amd/diagonal.py) against the numpy oracle (tests/diagonal_oracle.py), on both
dtypes, on contiguous and permuted layouts, at the sizes where the kernel takes another path: 2^6 (the small form), 2^10
(exactly one tile, everything static), 2^13 (eight tiles: static terms, dynamic groups, a group with lo == 0) and one case
at 2^22 (more tiles than the grid: the stride loop runs).

f is compared BIT FOR BIT (the contract fixes the order of every addition), MULTIPLY bit for bit against float64 products
rounded once, PHASE within (8 + |gamma f|) 2^-52 |a| + r_T per element (r_T = 2^-23 |a| for complex64, 0 for complex128:
sincos of the device and of numpy, two fma roundings, the rounding of the phase argument, the store), the sums to 1e-12 of
the sum of the magnitudes of their terms (the same float64 terms in another order)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd.pauli import _ptr

import diagonal_oracle as DO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {"c64": (torch.complex64, np.complex64), "c128": (torch.complex128, np.complex128)}
# dim d of the view owns memory bit bits_of(nq, layout)[d] (contiguous: bit nq - 1 - d)
LAYOUTS = ["contiguous", "reversed", "shuffled"]
SIZES = [6, 10, 13]


def bits_of(nq, layout):
    if layout == "contiguous":
        return list(range(nq - 1, -1, -1))
    if layout == "reversed":
        return list(range(nq))
    return [int(b) for b in np.random.default_rng(nq).permutation(nq)]


def view_of(flat, nq, layout):
    """The [2]*nq view of a flat tensor whose dim d has stride 2^bits_of(nq, layout)[d]."""
    bits = bits_of(nq, layout)
    contiguous = flat.view((2,) * nq)                                      # dim j owns bit nq - 1 - j
    return contiguous.permute([nq - 1 - b for b in bits])


def on_bits(nq, layout, c, bits):
    """The term c * Z on the MEMORY bits `bits`, written on the dims of the view."""
    owner = {b: d for d, b in enumerate(bits_of(nq, layout))}
    return (c, {owner[b]: "Z" for b in bits})


def term_list(nq, layout, kind):
    rng = np.random.default_rng(7 * nq + len(kind))
    t = lambda c, bits: on_bits(nq, layout, c, bits)                      # noqa: E731
    tb = min(nq, 10)
    low, high = list(range(tb)), list(range(tb, nq))
    pick = lambda pool, k: [int(b) for b in rng.choice(pool, size=min(k, len(pool)), replace=False)]   # noqa: E731
    coeff = lambda: float(rng.choice([-1.5, 0.375, 1.0, 2.25, -0.1, 3e-3]))                            # noqa: E731
    if kind == "static":
        return [t(coeff(), pick(low, int(rng.integers(0, 4)))) for _ in range(12)]
    if kind == "mixed":                                                   # static, straddling, high-only, weight n, repeats, cancelling
        out = [t(coeff(), pick(low, 2)) for _ in range(5)]
        out += [t(coeff(), list(range(nq)))]
        if high:
            out += [t(coeff(), pick(low, 1) + pick(high, 1)) for _ in range(6)]
            out += [t(coeff(), pick(high, 2)) for _ in range(3)]          # lo == 0: a per-tile constant
            out += [t(0.7, [high[0], 2]), t(-0.7, [high[0], 2])]          # a group that cancels to 0.0
            out += [t(1.25, [high[-1]]), t(1.25, [high[-1]])]             # the same string twice
        out += [t(0.3, [1]), t(-0.3, [1]), out[0]]
        return out
    if kind == "high":
        return [t(coeff(), pick(high, int(rng.integers(1, 4)))) for _ in range(9)]
    if kind == "g64":                                                     # 64 groups: every pattern of six low bits under one high bit
        return [t(coeff(), [high[j % len(high)]] + [b for b in range(6) if (j >> b) & 1]) for j in range(64)] + [t(0.5, [0, 3])]
    raise KeyError(kind)


KINDS = {6: ["static", "mixed"], 10: ["static", "mixed"], 13: ["mixed", "high", "g64"]}
CASES = [(nq, layout, kind) for nq in SIZES for layout in LAYOUTS for kind in KINDS[nq]]
MIXED = [(nq, layout) for nq in SIZES for layout in LAYOUTS]


@functools.lru_cache(maxsize=None)
def reference(nq, layout, kind):
    """(terms, f in memory order): computed once, shared, never written."""
    terms = term_list(nq, layout, kind)
    shape, strides = (2,) * nq, [1 << b for b in bits_of(nq, layout)]
    f = DO.Plan(shape, strides, terms).values()
    f.setflags(write=False)
    return terms, f


@functools.lru_cache(maxsize=None)
def state(nq, dt, seed=0):
    rng = np.random.default_rng(1000 * nq + seed)
    a = (rng.standard_normal(1 << nq) + 1j * rng.standard_normal(1 << nq)).astype(DTYPES[dt][1])
    a.setflags(write=False)
    return a


def upload(a, nq, layout):
    flat = torch.from_numpy(a.copy()).to(DEV)
    return flat, view_of(flat, nq, layout)


def operator(view, terms):
    return A.DiagonalOperator(view.shape, view.stride(), view.dtype, terms, view.device)


def same_bits(got, want):
    """Zeros are compared as values (-0.0 == 0.0), everything else as integers."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype.kind == "c":
        got, want = got.view(got.real.dtype), want.view(want.real.dtype)
    zero = want == 0
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return bool((got[zero] == 0).all()) and np.array_equal(got[~zero].view(u), want[~zero].view(u))


def phase_bound(a, f, gamma, dt):
    mag = np.abs(a.astype(np.complex128))
    return (8 + np.abs(gamma * f)) * 2.0 ** -52 * mag + (2.0 ** -23 * mag if dt == "c64" else 0.0)


def gamma_for(f):
    return 57.0 / max(float(np.abs(f).max()), 1e-300)                      # |gamma f| <= 64


def memory(view, flat):
    """The flat tensor's content as numpy (the view shares its storage)."""
    return flat.cpu().numpy()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nq, layout, kind", CASES)
def test_values_and_multiply_equal_the_oracle_bit_for_bit(nq, layout, kind, dt):
    terms, f = reference(nq, layout, kind)
    a = state(nq, dt)
    flat, view = upload(a, nq, layout)
    op = operator(view, terms)
    vals = A.diagonal_values(op)
    assert vals.shape == view.shape and vals.stride() == view.stride() and vals.dtype == torch.float64
    got = torch.as_strided(vals, (1 << nq,), (1,)).cpu().numpy()            # memory order
    assert same_bits(got, f)
    assert op.multiply_(view) is view
    assert same_bits(memory(view, flat), DO.multiply(a, f, DTYPES[dt][1]))
    info = A.diagonal_info(view.shape, view.stride(), terms, dtype=view.dtype)
    assert (op.n_groups, op.n_static, op.tile_bits) == (info["G"], info["n_static"], min(nq, 10))
    if kind == "g64":
        assert info["G"] == 64
    if nq <= 10:
        assert info["G"] == 0 and info["n_tiles"] == 1


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nq, layout", MIXED)
def test_phase(nq, layout, dt):
    terms, f = reference(nq, layout, "mixed")
    a = state(nq, dt)
    gamma = gamma_for(f)
    assert np.abs(gamma * f).max() <= 64
    bound = phase_bound(a, f, gamma, dt)
    flat, view = upload(a, nq, layout)
    op = operator(view, terms)
    assert op.evolve_(view, 0.0) is view
    assert same_bits(memory(view, flat), a)                                 # gamma = 0: bit for bit
    op.evolve_(view, gamma)
    got = memory(view, flat).astype(np.complex128)
    err = np.abs(got - DO.phase(a, f, gamma))
    print(f"phase 2^{nq} {layout} {dt}: largest error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    assert abs(float(np.sum(np.abs(got) ** 2)) - float(np.sum(np.abs(a.astype(np.complex128)) ** 2))) <= float(
        np.sum(2 * np.abs(a.astype(np.complex128)) * bound + bound ** 2)) + 1e-15 * float(np.sum(np.abs(a) ** 2))
    op.evolve_(view, -gamma)
    back = memory(view, flat).astype(np.complex128)
    assert (np.abs(back - a.astype(np.complex128)) <= 2 * bound).all()
    # the one-shot wrapper is the same launch
    flat2, view2 = upload(a, nq, layout)
    A.diagonal_evolve_(view2, terms, gamma)
    assert same_bits(memory(view2, flat2), got.astype(DTYPES[dt][1]))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_phase_agrees_with_the_rotation_circuit(layout):
    nq = 13
    terms, f = reference(nq, layout, "mixed")
    a = state(nq, "c128")
    gamma = 0.37
    flat, view = upload(a, nq, layout)
    A.diagonal_evolve_(view, terms, gamma)
    flat2, view2 = upload(a, nq, layout)
    A.pauli_evolve_(view2, [(gamma * c, s) for c, s in terms])
    assert np.abs(memory(view, flat) - memory(view2, flat2)).max() <= 1e-12 * np.abs(a).max()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nq, layout", MIXED + [(16, "shuffled")])
def test_moments_and_expectation(nq, layout, dt):
    terms = term_list(nq, layout, "mixed")
    f = DO.Plan((2,) * nq, [1 << b for b in bits_of(nq, layout)], terms).values() if nq == 16 else reference(nq, layout, "mixed")[1]
    a = state(nq, dt)
    flat, view = upload(a, nq, layout)
    op = operator(view, terms)
    raw = op.moments(view, device=True)
    assert isinstance(raw, torch.Tensor) and raw.is_cuda and raw.dtype == torch.float64 and tuple(raw.shape) == (3,)
    again = op.moments(view)
    assert same_bits(raw.cpu().numpy(), again)                              # bit-identical from run to run
    assert same_bits(memory(view, flat), a)                                 # a read pass
    want, scale = DO.moments(a, f)
    assert (np.abs(again - want) <= 1e-12 * scale).all(), (again, want)
    E, var = op.expectation(view)
    assert abs(E - want[1] / want[0]) <= 2e-12 * scale[1] / want[0]
    assert abs(var - (want[2] / want[0] - (want[1] / want[0]) ** 2)) <= 4e-12 * scale[2] / want[0]
    assert abs(E - A.pauli_sum_expectation(view, terms)) <= 1e-12 * sum(abs(c) for c, _ in terms)
    E2, var2 = A.diagonal_expectation(view, terms)
    assert (E2, var2) == (E, var)
    Ed, vd = op.expectation(view, device=True)
    assert Ed.is_cuda and float(Ed) == E and float(vd) == var


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nq, layout", MIXED)
def test_pair(nq, layout, dt):
    terms, f = reference(nq, layout, "mixed")
    lam0, phi0 = state(nq, dt, seed=1), state(nq, dt, seed=2)
    gamma = gamma_for(f) / 3
    lflat, lam = upload(lam0, nq, layout)
    pflat, phi = upload(phi0, nq, layout)
    op = operator(phi, terms)
    want, scale = DO.transition(lam0, f, phi0)
    t0 = op.pair_(lam, phi, gamma, evolve=False)
    assert same_bits(memory(lam, lflat), lam0) and same_bits(memory(phi, pflat), phi0)     # transition only: nothing is written
    assert abs(t0 - want) <= 1e-12 * scale
    td = op.pair_(lam, phi, gamma, device=True)
    assert td.is_cuda and td.dtype == torch.float64 and tuple(td.shape) == (2,)
    assert complex(*td.tolist()) == t0                                      # bit-identical, and taken before the phase
    for flat0, flat in ((lam0, lflat), (phi0, pflat)):
        alone_flat, alone = upload(flat0, nq, layout)
        op.evolve_(alone, gamma)
        assert same_bits(flat.cpu().numpy(), alone_flat.cpu().numpy())
    with pytest.raises(ValueError, match="lam overlaps phi"):
        op.pair_(phi, phi, gamma)


def test_the_device_entries_refuse_bad_arguments():
    nq = 13
    terms, _ = reference(nq, "contiguous", "mixed")
    flat, view = upload(state(nq, "c64"), nq, "contiguous")
    op = operator(view, terms)
    lib, stream = N.lib(), N.current_stream_ptr(view.device)
    args = (ctypes.byref(op._d),)
    rc = lib.artn_diag_apply(*args, view.data_ptr() + 8, _ptr(op._ops), op.n_terms, op._table.data_ptr(), op.table_bytes, 0, 0.5, stream)
    assert rc == -2 and b"artn_diag_apply needs a 16-byte aligned array" in lib.artn_last_error()
    rc = lib.artn_diag_apply(*args, view.data_ptr(), _ptr(op._ops), op.n_terms, op._table.data_ptr(), op.table_bytes - 8, 0, 0.5, stream)
    assert rc == -1 and b"table smaller than artn_diag_query reports" in lib.artn_last_error()
    rc = lib.artn_diag_apply(*args, view.data_ptr(), _ptr(op._ops), op.n_terms, op._table.data_ptr(), op.table_bytes, 2, 0.5, stream)
    assert rc == -1 and b"unknown mode" in lib.artn_last_error()
    ws = torch.empty(op.workspace_bytes // 8, dtype=torch.float64, device=DEV)
    out = torch.empty(4, dtype=torch.float64, device=DEV)
    rc = lib.artn_diag_expect(*args, view.data_ptr(), _ptr(op._ops), op.n_terms, op._table.data_ptr(), op.table_bytes, ws.data_ptr(),
                              op.workspace_bytes - 8, out.data_ptr(), stream)
    assert rc == -1 and b"workspace smaller" in lib.artn_last_error()
    rc = lib.artn_diag_pair(*args, view.data_ptr(), view.data_ptr() + 1024, _ptr(op._ops), op.n_terms, op._table.data_ptr(), op.table_bytes,
                            0, 0.5, ws.data_ptr(), op.workspace_bytes, out.data_ptr(), stream)
    assert rc == -1 and b"lam overlaps phi" in lib.artn_last_error()
    torch.cuda.synchronize()
    assert same_bits(flat.cpu().numpy(), state(nq, "c64"))                  # nothing was launched
    with pytest.raises(ValueError, match="16-byte boundary"):
        op.evolve_(torch.view_as_complex(torch.zeros(2 * (1 << nq) + 2, device=DEV)[2:].view(-1, 2)).view((2,) * nq), 0.1)
    with pytest.raises(ValueError, match="built for shape"):
        op.evolve_(view.permute(list(range(nq - 1, -1, -1))), 0.1)


def test_the_stride_loop_at_2_22():
    """4096 tiles on a grid of 2048 workgroups: every workgroup takes two tiles.  Terms on bits 21, 15 and 9 and inside the tile."""
    nq, layout = 22, "contiguous"
    t = lambda c, bits: on_bits(nq, layout, c, bits)                      # noqa: E731
    terms = [t(1.5, [21]), t(-0.25, [21, 9]), t(0.75, [15, 3]), t(2.0, [4, 7]), t(-1.0, [21, 15, 11, 0]), t(0.125, list(range(nq))),
             t(0.5, [10]), t(3.0, [9])]
    f = DO.Plan((2,) * nq, [1 << b for b in bits_of(nq, layout)], terms).values()
    a = state(nq, "c64")
    flat, view = upload(a, nq, layout)
    op = operator(view, terms)
    assert op.n_tiles == 4096 and op.n_groups >= 3
    assert same_bits(torch.as_strided(op.values(), (1 << nq,), (1,)).cpu().numpy(), f)
    want, scale = DO.moments(a, f)
    assert (np.abs(op.moments(view) - want) <= 1e-12 * scale).all()
    gamma = gamma_for(f)
    op.evolve_(view, gamma)
    assert (np.abs(flat.cpu().numpy().astype(np.complex128) - DO.phase(a, f, gamma)) <= phase_bound(a, f, gamma, "c64")).all()
    flat2, view2 = upload(a, nq, layout)
    op.multiply_(view2)
    assert same_bits(flat2.cpu().numpy(), DO.multiply(a, f, np.complex64))


def qaoa_problem(dt):
    nq = 12
    edges = [(q, (q + 1) % nq) for q in range(nq)] + [(0, 5), (3, 9)]       # a ring plus two chords
    cost = [(1.0, {q: "Z", r: "Z"}) for q, r in edges]
    rng = np.random.default_rng(12)
    a = rng.standard_normal(1 << nq) + 1j * rng.standard_normal(1 << nq)
    a = (a / np.linalg.norm(a)).astype(DTYPES[dt][1])                        # amplitudes of about 2^-6
    return nq, cost, a, [0.31, -0.47], [0.52, 0.23]


@pytest.mark.parametrize("dt, bound", [("c128", 1e-9), ("c64", 1e-4)])
def test_qaoa_gradient_against_adjoint_gradient(dt, bound):
    """(E, grad) of two layers on a 12-qubit ring with two chords against adjoint_gradient with every bond a rotation that
    shares its layer's parameter.  Both routes accumulate in float64; complex64 rounds the state in every pass.  Measured on an
    MI355X: 9.7e-16 (complex128) and 4.6e-07 (complex64) of max(|E|, max |grad|) = 0.286."""
    nq, cost, a, gammas, betas = qaoa_problem(dt)
    amps0 = torch.from_numpy(a.copy()).to(DEV).view((2,) * nq)
    E, grad = A.qaoa_gradient(amps0, cost, gammas, betas)
    assert same_bits(amps0.reshape(-1).cpu().numpy(), a)                    # amps0 is never written
    rotations, params = [], []
    for l in range(2):
        rotations += [(gammas[l] * c, s) for c, s in cost]
        params += [l] * len(cost)
        rotations += [(betas[l], {q: "X"}) for q in range(nq)]
        params += [2 + l] * nq
    E_ref, grad_ref = A.adjoint_gradient(amps0, rotations, cost, params)
    scale = max(abs(E_ref), float(np.abs(grad_ref).max()))
    dist = max(abs(E - E_ref), float(np.abs(grad - grad_ref).max())) / scale
    print(f"qaoa_gradient {dt}: distance to adjoint_gradient {dist:.3e} of max(|E|, max |grad|) = {scale:.4f}")
    assert grad.dtype == np.float64 and grad.shape == (4,)
    assert dist <= bound
    with pytest.raises(ValueError, match="real coefficients"):
        A.qaoa_gradient(amps0, [(1j, {0: "Z"})], gammas, betas)
