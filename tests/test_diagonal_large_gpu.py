"""The diagonal kernel on 2^30 complex64 amplitudes (8 GiB: byte offsets cross 2^32, a million tiles on a grid of 2048), checked
EXACTLY with the method of tests/exact_state.py: the coefficients are powers of two, so f is a small integer that int64
arithmetic on the memory index predicts; the state is the integer hash of the index, so every component of a * f stays far
below 2^24 (8 * 71) and MULTIPLY has to EQUAL the prediction.  VALUES is compared in the same way.  The terms sit on memory bits 29,
21 and 9 (the top of the array, the middle of the tile index, the top of the tile) and below: a tile index or a byte offset
narrowed to 32 bits, or a sign taken from the wrong half of the index, changes elements that are compared.

Skips, with the figures, when the device has less free memory than the array plus 4 GiB."""
import pytest
import torch

import artensor_amd as A
import exact_state as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GIB = 1 << 30
NQ = 30
# (coefficient, memory bits): four groups (lo = 0, bit 9, bits 3 and 0, all ten), two static terms, a term of weight n, a repeat
TERMS = [(4.0, (29,)), (-2.0, (29, 21)), (1.0, (21, 9)), (16.0, (29, 9)), (-1.0, (9,)), (8.0, (3, 0)), (2.0, (29, 21, 3, 0)),
         (1.0, tuple(range(NQ))), (-4.0, (17,)), (32.0, (21, 9))]


def api_terms():
    return [(c, E.api_string(NQ, {b: "Z" for b in bits})) for c, bits in TERMS]


def f_of(i):
    """f(i) as int64 at the memory indices i."""
    out = torch.zeros_like(i)
    for c, bits in TERMS:
        mask = sum(1 << b for b in bits)
        out += int(c) * (1 - 2 * E._parity(i & mask))
    return out


def budget(arrays_bytes):
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    need = arrays_bytes + 4 * GIB
    if free < need:
        pytest.skip(f"needs {need / GIB:.1f} GiB of free device memory, {free / GIB:.1f} GiB free")


def test_values_and_multiply_are_exact_at_2_30():
    budget(8 << NQ)
    n = 1 << NQ
    op = A.DiagonalOperator((2,) * NQ, tuple(1 << (NQ - 1 - d) for d in range(NQ)), torch.complex64, api_terms(), DEV)
    assert op.n_tiles == 1 << 20 and op.n_groups == 4 and op.n_static == 2
    vals = torch.as_strided(op.values(), (n,), (1,))
    bad = torch.zeros((), dtype=torch.int64, device=DEV)
    for lo in range(0, n, E.CHUNK):
        i = torch.arange(lo, min(lo + E.CHUNK, n), device=DEV)
        bad += (vals[lo:lo + E.CHUNK] != f_of(i).to(torch.float64)).sum()
    assert int(bad) == 0, f"{int(bad)} values differ"
    del vals
    torch.cuda.empty_cache()
    store = E.fill(torch.empty(n, dtype=torch.complex64, device=DEV))
    assert op.multiply_(store.view((2,) * NQ)).data_ptr() == store.data_ptr()
    tally = E.Tally(DEV)
    for lo in range(0, n, E.CHUNK):
        i = torch.arange(lo, min(lo + E.CHUNK, n), device=DEV)
        f = f_of(i)
        re, im = E.hash_index(i)
        tally.add(store[lo:lo + E.CHUNK], re * f, im * f, i)
    report = tally.report()
    print(f"multiply 2^30: compared {report['compared']}, mismatches {report['bad']}, largest |component of a f| {report['peak']}")
    assert report["peak"] < 1 << 24 and report["bad"] == 0, report
