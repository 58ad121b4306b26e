"""Host-side checks of the reduced-density-matrix layer (artensor_amd/rdm.py, artn_rdm_query / artn_rdm): the host-only query,
its refusals, the digit order of the row index, and entropy_of on matrices written down by hand.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import born, rdm


def contiguous_strides(shape):
    out, s = [], 1
    for e in reversed(shape):
        out.append(s)
        s *= e
    return out[::-1]


def info_of(shape, keep, dtype=torch.complex64, strides=None):
    return rdm.rdm_info(shape, strides or contiguous_strides(shape), keep, dtype)


def test_abi_version_is_9_on_both_sides():
    assert N.ABI_VERSION == 9
    assert N.lib().artn_abi_version() == 9
    assert "artn_rdm" in N.exported_symbols() and "artn_rdm_query" in N.exported_symbols()
    assert ctypes.sizeof(N.ArtnRdmInfo) == 4 * 4 + 2 * 8 + 8


@pytest.mark.parametrize("k", range(1, 11))
def test_query_of_the_streaming_form(k):
    """rows = min(64, max(16, D)); one tile below D = 128, T (T + 1) / 2 lower-triangle tiles of 64 rows above; the split count
    is the smallest power of two that brings tiles * splits to 512 workgroups; workspace = tiles * splits * rows^2 * 16 bytes."""
    shape = (2,) * 20
    D = 2 ** k
    for keep in (list(range(k)), list(range(20 - k, 20)), list(range(0, 2 * k, 2))):
        for dtype in (torch.complex64, torch.complex128):
            info = info_of(shape, keep, dtype)
            rows = min(64, max(16, D))
            T = max(1, D // 64)
            assert info["kernel"] == N.RDM_STREAM and info["dim"] == D
            assert info["tiles"] == T * (T + 1) // 2
            assert info["panel_bits"] == 10 - int(np.log2(rows))
            splits = 1
            while info["tiles"] * splits < 512:
                splits *= 2
            assert info["splits"] == splits                     # (2^20 elements leave enough panels for every k here)
            assert info["workspace_bytes"] == info["tiles"] * info["splits"] * rows * rows * 16
            # one 2048-FLOP MFMA per 16 x 16 block of the lower triangle and per column
            blocks = {16: 1, 32: 3, 64: 10}[rows] * T + 16 * (info["tiles"] - T)
            assert info["flops"] == 2048.0 * blocks * (2 ** 20 // max(D, 16))


def test_query_picks_the_generic_form_where_the_streaming_one_does_not_apply():
    for shape, keep in (((3, 4, 5, 2, 6), [1, 3]), ((1, 2, 1, 2), [1]), ((4096, 3), [1]), ((2,) * 11, [0, 1]),
                        ((2,) * 20, []), ((2,) * 12, list(range(10)))):
        info = info_of(shape, keep)
        assert info["kernel"] == N.RDM_GENERIC and info["workspace_bytes"] == 0 and info["flops"] == 0.0
        assert info["tiles"] == 0 and info["splits"] == 0
        assert info["dim"] == int(np.prod([shape[d] for d in keep]))
    assert info_of((2,) * 12, [0, 1])["kernel"] == N.RDM_STREAM         # exactly 2^12 elements
    assert info_of((2,) * 14, list(range(10)))["kernel"] == N.RDM_STREAM  # D = 1024 with 16 dropped states
    # the split count never exceeds the panels there are: 2^12 elements, D = 4 -> 16 rows x 64 columns per panel, 4 panels
    info = info_of((2,) * 12, [0, 1])
    assert info["splits"] == 4 and info["tiles"] == 1 and info["workspace_bytes"] == 4 * 16 * 16 * 16
    # a permuted dense layout is as good as a contiguous one
    shape = (2,) * 20
    st = contiguous_strides(shape)
    perm = [3, 0, 2, 1] + list(range(4, 20))
    assert info_of(shape, [1, 2], strides=[st[p] for p in perm])["kernel"] == N.RDM_STREAM


def test_refusals():
    def rc(shape, strides, keep, dtype=torch.complex64):
        d, _ = born._marginal_desc(shape, strides, keep, dtype)
        info = N.ArtnRdmInfo()
        return N.lib().artn_rdm_query(ctypes.byref(d), ctypes.byref(info))

    assert rc((4, 4), (4, 1), [0]) == 0
    assert rc((4, 4), (1, 4), [0]) == 0
    for strides in ((1, 1), (2, 1), (8, 1), (4, 2), (0, 1)):              # overlapping, gaps, strided, expanded
        assert rc((4, 4), strides, [0]) == -1
        assert b"dense" in N.lib().artn_last_error()
    assert rc((4, 1, 4), (4, 77, 1), [0]) == 0                             # the stride of an extent-1 dim means nothing
    with pytest.raises(RuntimeError, match="dense"):
        info_of((4, 4), [0], strides=(8, 1))
    # D = 2048: beyond the stated limit, in either form
    with pytest.raises(RuntimeError, match="1024"):
        info_of((2,) * 20, list(range(11)))
    with pytest.raises(RuntimeError, match="1024"):
        info_of((2048, 3), [0])
    assert rc((2,) * 20, contiguous_strides((2,) * 20), list(range(11))) == -2
    assert info_of((2,) * 20, list(range(10)))["dim"] == 1024
    # a real dtype
    with pytest.raises(TypeError, match="complex"):
        info_of((2,) * 12, [0], dtype=torch.float32)
    d, _ = born._marginal_desc((2,) * 12, contiguous_strides((2,) * 12), [0], torch.complex64)
    d.dtype = N.ARTN_C64_BF16
    assert N.lib().artn_rdm_query(ctypes.byref(d), ctypes.byref(N.ArtnRdmInfo())) == -2
    # repeated dims, dims out of range
    with pytest.raises(ValueError, match="keep"):
        info_of((2,) * 12, [3, 3])
    with pytest.raises(ValueError, match="keep"):
        info_of((2,) * 12, [0, -12])
    with pytest.raises(ValueError, match="keep"):
        info_of((2,) * 12, [12])
    assert N.lib().artn_rdm_query(None, ctypes.byref(N.ArtnRdmInfo())) == -1


def test_digit_order_of_the_row_index():
    """Kept dims come first in the descriptor, in the order asked for, and the first one is the most significant digit."""
    shape, strides = (2, 3, 4, 5), (60, 20, 5, 1)
    d, keep = born._marginal_desc(shape, strides, [2, -4, 1], torch.complex64)
    assert keep == [2, 0, 1]
    assert [d.extent[i] for i in range(4)] == [4, 2, 3, 5] and [d.stride[i] for i in range(4)] == [5, 60, 20, 1]
    assert [d.keep[i] for i in range(4)] == [1, 1, 1, 0]
    assert info_of(shape, [2, -4, 1], strides=strides)["dim"] == 24
    # and of the planner itself: row i of rho starts at the memory offset of the digits of i, the first kept dim most significant
    def offsets(shape, strides, keep):
        d, keep = born._marginal_desc(shape, strides, keep, torch.complex64)
        D = int(np.prod([shape[k] for k in keep]))
        got = np.full(D, -1, dtype=np.int64)
        assert N.lib().artn_rdm_row_offsets(ctypes.byref(d), got.ctypes.data_as(ctypes.c_void_p)) == 0
        digits = np.stack(np.unravel_index(np.arange(D), [shape[k] for k in keep]), axis=-1).reshape(D, len(keep))
        want = (digits * np.array([strides[k] for k in keep], dtype=np.int64)).sum(axis=1)
        return got, want

    got, want = offsets(shape, strides, [2, -4, 1])                       # generic form
    assert (got == want).all() and got[1] == 20 and got[3] == 60 and got[6] == 5
    rng = np.random.default_rng(3)
    for nq, keeps in ((20, ([19], [0, 19], [18, 2, 11], [5, 19, 0, 7, 12, 3, 1], list(range(9, -1, -1)), [3, 17, 4, 16, 5, 15, 6, 14])),
                      (12, ([0, 1], [11, 3, 7, 5, 1]))):
        shape = (2,) * nq
        st = contiguous_strides(shape)
        strides = [st[p] for p in rng.permutation(nq)]
        for keep in keeps:
            assert info_of(shape, keep, strides=strides)["kernel"] == N.RDM_STREAM
            got, want = offsets(shape, strides, keep)
            assert (got == want).all()
            assert got[1] == strides[keep[-1]] and got[len(got) // 2] == strides[keep[0]]    # last kept dim fastest, first slowest
    got, want = offsets((4, 8, 2, 16), (1, 4, 512, 32), [3, 0])           # extents above 2: digits of several bits
    assert info_of((4, 8, 2, 16), [3, 0], strides=(1, 4, 512, 32))["kernel"] == N.RDM_GENERIC and (got == want).all()
    got, want = offsets((4, 8, 2, 16, 16), (1, 4, 512, 32, 1024), [3, 0, 4])
    assert info_of((4, 8, 2, 16, 16), [3, 0, 4], strides=(1, 4, 512, 32, 1024))["kernel"] == N.RDM_STREAM and (got == want).all()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the CPU-only refusal")
def test_rdm_functions_have_no_cpu_fallback():
    a = torch.zeros(4, 4, dtype=torch.complex64)
    for call in (lambda: A.reduced_density_matrix(a, [0]), lambda: A.purity(a, [0]), lambda: A.renyi_entropy(a, [0]),
                 lambda: A.entanglement_entropy(a, [0]), lambda: A.expectation(a, np.eye(4), [0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    buf = np.zeros(64, dtype=np.complex128)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    d, _ = born._marginal_desc((4, 4), (4, 1), [0], torch.complex64)
    assert N.lib().artn_rdm(ctypes.byref(d), p, p, p, 0, None) == -4


def test_entropy_of_matrices_written_down_by_hand():
    pure = np.zeros((4, 4))
    pure[2, 2] = 1.0
    assert A.entropy_of(pure) == 0.0 and A.entropy_of(pure, alpha=2) == 0.0
    plus = np.full((2, 2), 0.5)                                            # |+><+|: pure, not diagonal
    assert abs(A.entropy_of(plus)) < 1e-14
    assert abs(A.entropy_of(np.diag([0.5, 0.5])) - 1.0) < 1e-15
    assert abs(A.entropy_of(np.diag([0.5, 0.0, 0.0, 0.5])) - 1.0) < 1e-15
    mixed = np.eye(8) / 8
    assert abs(A.entropy_of(mixed) - 3.0) < 1e-14 and abs(A.entropy_of(mixed, alpha=2) - 3.0) < 1e-14
    assert abs(A.entropy_of(mixed, alpha=0.5) - 3.0) < 1e-14 and abs(A.entropy_of(mixed, alpha=float("inf")) - 3.0) < 1e-14
    assert abs(A.entropy_of(mixed, base=np.e) - 3.0 * np.log(2.0)) < 1e-14
    # unnormalised input is normalised by its trace
    assert abs(A.entropy_of(7.0 * np.diag([0.5, 0.5])) - 1.0) < 1e-15
    # a slightly negative eigenvalue is clipped (no NaN from its logarithm)
    h = A.entropy_of(np.diag([0.5, 0.5 + 1e-17, -1e-17]))
    assert np.isfinite(h) and abs(h - 1.0) < 1e-14
    assert np.isfinite(A.entropy_of(np.diag([1.0, -1e-18]), alpha=0.5))
    # a known mixed qubit: eigenvalues 3/4, 1/4
    rho = np.array([[0.5, 0.25j], [-0.25j, 0.5]])
    want = -(0.75 * np.log2(0.75) + 0.25 * np.log2(0.25))
    assert abs(A.entropy_of(rho) - want) < 1e-14
    assert abs(A.entropy_of(rho, alpha=2) + np.log2(0.75 ** 2 + 0.25 ** 2)) < 1e-14
    # torch matrices, on the CPU too
    assert abs(A.entropy_of(torch.tensor(rho)) - want) < 1e-14
    assert abs(A.entropy_of(torch.eye(4, dtype=torch.complex128)) - 2.0) < 1e-14
    with pytest.raises(ValueError):
        A.entropy_of(np.zeros((2, 3)))
    with pytest.raises(ValueError):
        A.entropy_of(np.zeros((2, 2)))
