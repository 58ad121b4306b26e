"""64-bit tile bases of the bit-permutation kernel: one state of 2^30 complex64 (8 GiB) filled from the memory index with the
integer hash of tests/exact_state.py, the 30-bit reversal and then one transposition of two high bits, each checked ON THE DEVICE
by exact equality: the element at memory index j must be the hash of the index whose permuted image is j.  A base narrowed to
32 bits (byte offsets pass 2^32 here), a hole inserted in the wrong order or a tile visited twice moves elements to indices
whose hash differs."""
import pytest
import torch

import artensor_amd as A

import bit_permutation_oracle as O
import exact_state as E

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GIB = 1 << 30


def compare(store, dst):
    """Every element of `store` against the hash of its source index under dst_bit `dst`."""
    n = store.numel()
    tally = E.Tally(store.device)
    for lo in range(0, n, E.CHUNK):
        j = torch.arange(lo, min(lo + E.CHUNK, n), device=store.device)
        src = torch.zeros_like(j)
        for b, c in enumerate(dst):
            src.bitwise_or_(((j >> c) & 1) << b)
        re, im = E.hash_index(src)
        tally.add(store[lo:lo + E.CHUNK], re, im, j)
    return tally.report()


def test_reversal_and_a_high_transposition_on_8_gib():
    nq, dtype = 30, torch.complex64
    need = (8 << nq) + 4 * GIB                                             # the free-memory rule of test_state_ops_large_gpu
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < need:
        pytest.skip(f"needs {need / GIB:.1f} GiB of free device memory (one array of 8 GiB and 4 GiB of temporaries), {free / GIB:.1f} GiB free")
    store = E.fill(torch.empty(1 << nq, dtype=dtype, device=DEV))
    view = store.view((2,) * nq)
    reversal = [nq - 1 - b for b in range(nq)]
    info = A.bit_permutation_info(view.shape, view.stride(), dtype, perm=list(range(nq - 1, -1, -1)))
    assert list(info["dst_bit"]) == reversal and info["moved_high"] == 26 and 2 <= info["passes"] <= 4
    assert all(p["n_tiles"] == 1 << 18 for p in info["pass_info"])
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    A.reverse_qubits_(view)
    assert torch.cuda.max_memory_allocated() - before < 32 * 1024          # no second buffer
    report = compare(store, reversal)
    assert report["compared"] == 1 << nq and report["bad"] == 0, report
    # dims 0 and 2 are memory bits 29 and 27: two bits above the tile, the top one past byte offset 2^32
    A.swap_dims_(view, 0, 2)
    report = compare(store, O.compose([reversal, O.transposition(nq, 29, 27)], nq))
    assert report["compared"] == 1 << nq and report["bad"] == 0, report
    # the untouched hash state differs from both, so the comparison can fail
    assert compare(store, list(range(nq)))["bad"] > 1 << 29
