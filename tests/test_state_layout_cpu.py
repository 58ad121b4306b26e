"""The dense-layout check and the max_rank rule of the state operations, through the C ABI, without a GPU.

One table of descriptors goes through all six query entry points that take an amplitude array -- artn_marginal_query,
artn_rdm_query, artn_pauli_query, artn_gates_query, artn_wgate_query, artn_measure_query -- and every (return code,
artn_last_error()) pair is compared with a literal; where the query accepts the layout, a size it reports is compared as well
(kept elements, kept states, bytes read = elements * 8, the element count).  A second table does the same for max_rank on the
four circuit queries.  The families share one layout walk and one max_rank rule (artensor_amd/csrc/artn_state_host.h) but keep
their own precedence and wording, which is what the literals pin down.

The literals were recorded from the library of the commit BEFORE the six copies of the walk were folded into one, by running
observe_layouts() and observe_max_rank() below against it; they are not derived from the code under test."""
import ctypes
import functools

import numpy as np
import pytest

from artensor_amd import _native as N

C64, C128 = N.ARTN_C64, N.ARTN_C128
B20, B21 = 1 << 20, 1 << 21

# name: (dtype, n_dims or None for len(shape), shape, strides, keep, the extent-2 dimension the one gate acts on)
LAYOUTS = {
    "n_dims -1": (C64, -1, (2, 2), (2, 1), (1, 0), 0),
    "n_dims 97": (C64, 97, (2, 2), (2, 1), (1, 0), 0),
    "dtype 7": (7, None, (2, 2), (2, 1), (1, 0), 0),
    "extent 0": (C64, None, (2, 0, 2), (2, 4, 1), (1, 0, 0), 0),
    "stride 0": (C64, None, (2, 2), (0, 1), (1, 0), 0),
    "strides (1, 1)": (C64, None, (2, 2), (1, 1), (1, 0), 0),
    "strides (2, 2)": (C64, None, (2, 2), (2, 2), (1, 0), 0),
    "strides (4, 1)": (C64, None, (2, 2), (4, 1), (1, 0), 0),
    "(3, 2) dense": (C64, None, (3, 2), (2, 1), (0, 1), 1),
    "(2^21, 2^20) dense": (C64, None, (B21, B20), (B20, 1), (0, 0), 0),
    "(2, 2^21, 2^20) dense, the 2 kept": (C64, None, (2, B21, B20), (1, 2 * B20, 2), (1, 0, 0), 0),
    "(3, 2^20, 2^21) dense": (C64, None, (3, B20, B21), (1, 3, 3 * B20), (0, 0, 0), 0),
    "(3, 2^20, 2^21) dense, the 3 kept": (C64, None, (3, B20, B21), (1, 3, 3 * B20), (1, 0, 0), 0),
    "(2, 3, 2^20, 2^21) dense, the 2 kept": (C128, None, (2, 3, B20, B21), (1, 2, 6, 6 * B20), (1, 0, 0, 0), 0),
    # (2, 2^20, 2^21, 2): the third dimension crosses 2^40; the stride of the fourth leaves a gap that no copy reports
    "too big, a gap above the crossing": (C64, None, (2, B20, B21, 2), (1, 2, 2 * B20, 2 ** 43), (1, 0, 0, 0), 0),
    "a gap below the crossing": (C64, None, (2, B20, B21), (1, 4, 4 * B20), (1, 0, 0), 0),
    "extent-1 dims, strides 0 and 7, permuted": (C64, None, (2, 1, 2, 1, 2), (2, 0, 1, 7, 4), (1, 0, 0, 0, 1), 2),
    "(2, 2, 2, 2) permuted": (C128, None, (2, 2, 2, 2), (2, 8, 1, 4), (0, 1, 1, 0), 3),
    "(4, 2, 8) permuted": (C64, None, (4, 2, 8), (8, 32, 1), (0, 1, 0), 1),
    "no dimensions": (C64, None, (), (), (), 0),
}

OK = 0

# name: [marginal, rdm, pauli, gates, wgate, measure], each (return code, message, reported size or None)
LAYOUT_EXPECTED = {'n_dims -1': [(-1, 'bad number of dimensions', None),
               (-1, 'bad number of dimensions', None),
               (-1, 'bad number of dimensions', None),
               (-1, 'bad number of dimensions', None),
               (-1, 'bad number of dimensions', None),
               (-1, 'bad number of dimensions', None)],
 'n_dims 97': [(-1, 'bad number of dimensions', None),
               (-1, 'bad number of dimensions', None),
               (-2, 'Pauli expectations take at most 96 dimensions', None),
               (-2, 'gate circuits take at most 96 dimensions', None),
               (-2, 'wide gates take at most 96 dimensions', None),
               (-2, 'measurement takes at most 96 dimensions', None)],
 'dtype 7': [(-2, 'marginals take complex64 or complex128', None),
             (-2, 'reduced density matrices take complex64 or complex128', None),
             (-2, 'Pauli expectations take complex64 or complex128', None),
             (-2, 'gate circuits take complex64 or complex128', None),
             (-2, 'wide gates take complex64 or complex128', None),
             (-2, 'measurement takes complex64 or complex128', None)],
 'extent 0': [(-1, 'extent below 1', None),
              (-1, 'extent below 1', None),
              (-1, 'extent below 1', None),
              (-1, 'extent below 1', None),
              (-1, 'extent below 1', None),
              (-1, 'extent below 1', None)],
 'stride 0': [(-1, 'the tensor is not dense: stride below 1', None),
              (-1, 'the tensor is not dense: stride below 1', None),
              (-1, 'the tensor is not dense: stride below 1', None),
              (-1, 'the tensor is not dense: stride below 1', None),
              (-1, 'the tensor is not dense: stride below 1', None),
              (-1, 'the tensor is not dense: stride below 1', None)],
 'strides (1, 1)': [(-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None)],
 'strides (2, 2)': [(-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None)],
 'strides (4, 1)': [(-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                    (-1, 'the tensor is not dense: its strides overlap or leave gaps', None)],
 '(3, 2) dense': [(0, '', 2),
                  (0, '', 2),
                  (-2, 'Pauli expectations take power-of-two extents', None),
                  (-2, 'gate circuits take power-of-two extents', None),
                  (-2, 'wide gates take power-of-two extents', None),
                  (-2, 'measurement takes power-of-two extents', None)],
 '(2^21, 2^20) dense': [(-1, 'element count out of range', None),
                        (-1, 'element count out of range', None),
                        (-2, 'Pauli expectations take at most 2^40 elements', None),
                        (-2, 'gate circuits take at most 2^40 elements', None),
                        (-2, 'wide gates take at most 2^40 elements', None),
                        (-1, 'at least one dimension is measured', None)],
 '(2, 2^21, 2^20) dense, the 2 kept': [(-1, 'element count out of range', None),
                                       (-1, 'element count out of range', None),
                                       (-2, 'Pauli expectations take at most 2^40 elements', None),
                                       (-2, 'gate circuits take at most 2^40 elements', None),
                                       (-2, 'wide gates take at most 2^40 elements', None),
                                       (-2, 'measurement takes at most 2^40 elements', None)],
 '(3, 2^20, 2^21) dense': [(-1, 'element count out of range', None),
                           (-1, 'element count out of range', None),
                           (-2, 'Pauli expectations take power-of-two extents', None),
                           (-2, 'gate circuits take power-of-two extents', None),
                           (-2, 'wide gates take power-of-two extents', None),
                           (-1, 'at least one dimension is measured', None)],
 '(3, 2^20, 2^21) dense, the 3 kept': [(-1, 'element count out of range', None),
                                       (-1, 'element count out of range', None),
                                       (-2, 'Pauli expectations take power-of-two extents', None),
                                       (-2, 'gate circuits take power-of-two extents', None),
                                       (-2, 'wide gates take power-of-two extents', None),
                                       (-1, 'a measured dimension has extent 2; dimension 0 has extent 3', None)],
 '(2, 3, 2^20, 2^21) dense, the 2 kept': [(-1, 'element count out of range', None),
                                          (-1, 'element count out of range', None),
                                          (-2, 'Pauli expectations take power-of-two extents', None),
                                          (-2, 'gate circuits take power-of-two extents', None),
                                          (-2, 'wide gates take power-of-two extents', None),
                                          (-2, 'measurement takes power-of-two extents', None)],
 'too big, a gap above the crossing': [(-1, 'element count out of range', None),
                                       (-1, 'element count out of range', None),
                                       (-2, 'Pauli expectations take at most 2^40 elements', None),
                                       (-2, 'gate circuits take at most 2^40 elements', None),
                                       (-2, 'wide gates take at most 2^40 elements', None),
                                       (-2, 'measurement takes at most 2^40 elements', None)],
 'a gap below the crossing': [(-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                              (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                              (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                              (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                              (-1, 'the tensor is not dense: its strides overlap or leave gaps', None),
                              (-1, 'the tensor is not dense: its strides overlap or leave gaps', None)],
 'extent-1 dims, strides 0 and 7, permuted': [(0, '', 4), (0, '', 4), (0, '', 64), (0, '', 64), (0, '', 64), (0, '', 8)],
 '(2, 2, 2, 2) permuted': [(0, '', 4), (0, '', 4), (0, '', 256), (0, '', 256), (0, '', 256), (0, '', 16)],
 '(4, 2, 8) permuted': [(0, '', 2), (0, '', 2), (0, '', 512), (0, '', 512), (0, '', 512), (0, '', 64)],
 'no dimensions': [(0, '', 1),
                   (0, '', 1),
                   (0, '', 8),
                   (-1, 'gate 0: dimension 0 out of range', None),
                   (-1, 'a gate on 1 dimensions needs a state of at least 2^1 elements; this one has 1', None),
                   (-1, 'at least one dimension is measured', None)]}

# (query, dtype, max_rank): (return code, message, effective max_rank or None)
MAX_RANK_EXPECTED = {('pauli_evolve', 0, -2): (-1, 'max_rank below -1', None),
 ('pauli_adjoint', 0, -2): (-1, 'max_rank below -1', None),
 ('gates', 0, -2): (-1, 'max_rank below -1', None),
 ('gates_adjoint', 0, -2): (-1, 'max_rank below -1', None),
 ('pauli_evolve', 0, -1): (0, '', 3),
 ('pauli_adjoint', 0, -1): (0, '', 2),
 ('gates', 0, -1): (0, '', 3),
 ('gates_adjoint', 0, -1): (0, '', 2),
 ('pauli_evolve', 0, 0): (0, '', 0),
 ('pauli_adjoint', 0, 0): (0, '', 0),
 ('gates', 0, 0): (0, '', 0),
 ('gates_adjoint', 0, 0): (0, '', 0),
 ('pauli_evolve', 0, 1): (0, '', 1),
 ('pauli_adjoint', 0, 1): (0, '', 1),
 ('gates', 0, 1): (0, '', 1),
 ('gates_adjoint', 0, 1): (0, '', 1),
 ('pauli_evolve', 0, 2): (0, '', 2),
 ('pauli_adjoint', 0, 2): (0, '', 2),
 ('gates', 0, 2): (0, '', 2),
 ('gates_adjoint', 0, 2): (0, '', 2),
 ('pauli_evolve', 0, 3): (0, '', 3),
 ('pauli_adjoint', 0, 3): (0, '', 3),
 ('gates', 0, 3): (0, '', 3),
 ('gates_adjoint', 0, 3): (0, '', 3),
 ('pauli_evolve', 0, 4): (0, '', 4),
 ('pauli_adjoint', 0, 4): (-2, 'max_rank 4 above the two-state maximum 3 of this dtype', None),
 ('gates', 0, 4): (0, '', 4),
 ('gates_adjoint', 0, 4): (-2, 'max_rank 4 above the two-state maximum 3 of this dtype', None),
 ('pauli_evolve', 0, 5): (-2, 'max_rank 5 above the maximum 4 of this dtype', None),
 ('pauli_adjoint', 0, 5): (-2, 'max_rank 5 above the two-state maximum 3 of this dtype', None),
 ('gates', 0, 5): (-2, 'max_rank 5 above the maximum 4 of this dtype', None),
 ('gates_adjoint', 0, 5): (-2, 'max_rank 5 above the two-state maximum 3 of this dtype', None),
 ('pauli_evolve', 1, -2): (-1, 'max_rank below -1', None),
 ('pauli_adjoint', 1, -2): (-1, 'max_rank below -1', None),
 ('gates', 1, -2): (-1, 'max_rank below -1', None),
 ('gates_adjoint', 1, -2): (-1, 'max_rank below -1', None),
 ('pauli_evolve', 1, -1): (0, '', 2),
 ('pauli_adjoint', 1, -1): (0, '', 1),
 ('gates', 1, -1): (0, '', 2),
 ('gates_adjoint', 1, -1): (0, '', 1),
 ('pauli_evolve', 1, 0): (0, '', 0),
 ('pauli_adjoint', 1, 0): (0, '', 0),
 ('gates', 1, 0): (0, '', 0),
 ('gates_adjoint', 1, 0): (0, '', 0),
 ('pauli_evolve', 1, 1): (0, '', 1),
 ('pauli_adjoint', 1, 1): (0, '', 1),
 ('gates', 1, 1): (0, '', 1),
 ('gates_adjoint', 1, 1): (0, '', 1),
 ('pauli_evolve', 1, 2): (0, '', 2),
 ('pauli_adjoint', 1, 2): (0, '', 2),
 ('gates', 1, 2): (0, '', 2),
 ('gates_adjoint', 1, 2): (0, '', 2),
 ('pauli_evolve', 1, 3): (0, '', 3),
 ('pauli_adjoint', 1, 3): (-2, 'max_rank 3 above the two-state maximum 2 of this dtype', None),
 ('gates', 1, 3): (0, '', 3),
 ('gates_adjoint', 1, 3): (-2, 'max_rank 3 above the two-state maximum 2 of this dtype', None),
 ('pauli_evolve', 1, 4): (-2, 'max_rank 4 above the maximum 3 of this dtype', None),
 ('pauli_adjoint', 1, 4): (-2, 'max_rank 4 above the two-state maximum 2 of this dtype', None),
 ('gates', 1, 4): (-2, 'max_rank 4 above the maximum 3 of this dtype', None),
 ('gates_adjoint', 1, 4): (-2, 'max_rank 4 above the two-state maximum 2 of this dtype', None),
 ('pauli_evolve', 1, 5): (-2, 'max_rank 5 above the maximum 3 of this dtype', None),
 ('pauli_adjoint', 1, 5): (-2, 'max_rank 5 above the two-state maximum 2 of this dtype', None),
 ('gates', 1, 5): (-2, 'max_rank 5 above the maximum 3 of this dtype', None),
 ('gates_adjoint', 1, 5): (-2, 'max_rank 5 above the two-state maximum 2 of this dtype', None),
 ('pauli_evolve', 7, -2): (-2, 'Pauli expectations take complex64 or complex128', None),
 ('pauli_adjoint', 7, -2): (-1, 'max_rank below -1', None),
 ('gates', 7, -2): (-2, 'gate circuits take complex64 or complex128', None),
 ('gates_adjoint', 7, -2): (-1, 'max_rank below -1', None),
 ('pauli_evolve', 7, 5): (-2, 'Pauli expectations take complex64 or complex128', None),
 ('pauli_adjoint', 7, 5): (-2, 'Pauli expectations take complex64 or complex128', None),
 ('gates', 7, 5): (-2, 'gate circuits take complex64 or complex128', None),
 ('gates_adjoint', 7, 5): (-2, 'gate circuits take complex64 or complex128', None)}


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def desc(dtype, n_dims, shape, strides, keep):
    d = N.ArtnMarginalDesc()
    d.dtype, d.n_dims = dtype, len(shape) if n_dims is None else n_dims
    for i, (e, s, k) in enumerate(zip(shape, strides, keep)):
        d.extent[i], d.stride[i], d.keep[i] = e, s, k
    return d


def outcome(rc, value):
    return (rc, "", value) if rc == OK else (rc, N.lib().artn_last_error().decode(), None)


IDENTITY = np.array([1, 0, 0, 0, 0, 0, 1, 0] + [0] * 24, dtype=np.float64)  # a 2 x 2 identity in a 32-double gate slot


@functools.lru_cache(maxsize=None)
def observe_layouts():
    lib = N.lib()
    seen = {}
    for name, (dtype, n_dims, shape, strides, keep, gate_dim) in LAYOUTS.items():
        d = ctypes.byref(desc(dtype, n_dims, shape, strides, keep))
        ops = np.zeros(N.ARTN_MAX_LABELS, dtype=np.uint8)
        k, dims = np.array([1], dtype=np.int32), np.array([[gate_dim, -1]], dtype=np.int32)
        marg, rdm, pauli, gates, wgate, meas = (N.ArtnMarginalInfo(), N.ArtnRdmInfo(), N.ArtnPauliInfo(), N.ArtnGatesInfo(),
                                                N.ArtnWgateInfo(), N.ArtnMeasureInfo())
        none = [None] * 6
        seen[name] = [
            outcome(lib.artn_marginal_query(d, ctypes.byref(marg)), marg.out_elems),
            outcome(lib.artn_rdm_query(d, ctypes.byref(rdm)), rdm.dim),
            outcome(lib.artn_pauli_query(d, ptr(ops), 1, ctypes.byref(pauli), *none[:4]), pauli.bytes_read),
            outcome(lib.artn_gates_query(d, ptr(k), ptr(dims), ptr(IDENTITY), 1, -1, ctypes.byref(gates), *none), gates.bytes_read),
            outcome(lib.artn_wgate_query(d, 1, ptr(dims), ptr(IDENTITY), ctypes.byref(wgate), None, None), wgate.bytes_read),
            outcome(lib.artn_measure_query(d, ctypes.byref(meas)), meas.n),
        ]
    return seen


@functools.lru_cache(maxsize=None)
def observe_max_rank():
    lib = N.lib()
    shape = (2,) * 16
    strides = tuple(1 << b for b in range(16))
    ops, coeff = np.zeros(16, dtype=np.uint8), np.array([1.0, 0.0, 0.0, 0.0])
    k, dims = np.array([1], dtype=np.int32), np.array([[15, -1]], dtype=np.int32)
    none = [None] * 8
    seen = {}
    for dtype in (C64, C128, 7):
        d = ctypes.byref(desc(dtype, None, shape, strides, (0,) * 16))
        for max_rank in (-2, -1, 0, 1, 2, 3, 4, 5) if dtype != 7 else (-2, 5):
            ev, ad, ga, gad = N.ArtnPauliEvolveInfo(), N.ArtnPauliAdjointInfo(), N.ArtnGatesInfo(), N.ArtnGatesAdjointInfo()
            seen["pauli_evolve", dtype, max_rank] = outcome(
                lib.artn_pauli_evolve_query(d, ptr(ops), ptr(coeff), 1, max_rank, ctypes.byref(ev), *none), ev.max_rank)
            seen["pauli_adjoint", dtype, max_rank] = outcome(
                lib.artn_pauli_adjoint_query(d, ptr(ops), ptr(coeff), None, 1, max_rank, ctypes.byref(ad), *none), ad.max_rank)
            seen["gates", dtype, max_rank] = outcome(
                lib.artn_gates_query(d, ptr(k), ptr(dims), ptr(IDENTITY), 1, max_rank, ctypes.byref(ga), *none[:6]), ga.max_rank)
            seen["gates_adjoint", dtype, max_rank] = outcome(
                lib.artn_gates_adjoint_query(d, ptr(k), ptr(dims), ptr(IDENTITY), None, None, 1, max_rank, ctypes.byref(gad), *none[:6]),
                gad.max_rank)
    return seen


def test_the_tables_hold_the_cases_they_are_there_for():
    """The recorded literals themselves: both precedences, the unreported gap, the accepted layouts with their sizes."""
    assert set(LAYOUT_EXPECTED) == set(LAYOUTS) and all(len(v) == 6 for v in LAYOUT_EXPECTED.values())
    both = LAYOUT_EXPECTED["(3, 2^20, 2^21) dense"]
    assert [rc for rc, _, _ in both] == [-1, -1, -2, -2, -2, -1]
    assert both[0][1] == both[1][1] == "element count out of range" and all("power-of-two" in both[q][1] for q in (2, 3, 4))
    assert "extent 2" in LAYOUT_EXPECTED["(3, 2^20, 2^21) dense, the 3 kept"][5][1]
    assert all("2^40" in LAYOUT_EXPECTED["(2, 2^21, 2^20) dense, the 2 kept"][q][1] for q in (2, 3, 4, 5))
    assert LAYOUT_EXPECTED["too big, a gap above the crossing"] == LAYOUT_EXPECTED["(2, 2^21, 2^20) dense, the 2 kept"]
    assert all("overlap or leave gaps" in m for _, m, _ in LAYOUT_EXPECTED["a gap below the crossing"])
    assert [v for _, _, v in LAYOUT_EXPECTED["(2, 2, 2, 2) permuted"]] == [4, 4, 16 * 16, 16 * 16, 16 * 16, 16]
    assert [v for _, _, v in LAYOUT_EXPECTED["extent-1 dims, strides 0 and 7, permuted"]] == [4, 4, 8 * 8, 8 * 8, 8 * 8, 8]
    for top, query in ((4, "pauli_evolve"), (3, "pauli_adjoint"), (4, "gates"), (3, "gates_adjoint")):
        for dtype, t in ((C64, top), (C128, top - 1)):
            assert MAX_RANK_EXPECTED[query, dtype, -2][0] == -1
            assert MAX_RANK_EXPECTED[query, dtype, -1] == (OK, "", t - 1)
            assert MAX_RANK_EXPECTED[query, dtype, t] == (OK, "", t)
            rc, msg, _ = MAX_RANK_EXPECTED[query, dtype, t + 1]
            assert rc == -2 and ("two-state maximum %d" % t in msg if "adjoint" in query else "the maximum %d" % t in msg)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_every_query_answers_a_layout_as_recorded(name):
    got = observe_layouts()[name]
    for query, g, want in zip(("marginal", "rdm", "pauli", "gates", "wgate", "measure"), got, LAYOUT_EXPECTED[name]):
        assert g == want, (name, query)


def test_every_circuit_query_answers_max_rank_as_recorded():
    got = observe_max_rank()
    assert set(got) == set(MAX_RANK_EXPECTED)
    for key, want in MAX_RANK_EXPECTED.items():
        assert got[key] == want, key
