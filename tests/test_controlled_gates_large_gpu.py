"""64-bit indices of the controlled-gate kernel, cheaply: a zero state of 2^32 complex64 (32 GiB: element indices cross 2^31),
19 high controls on memory bits 12..30 (wanted 1, bit 12 wanted 0) and a signed-permutation gate on memory bits 31 and 0.  The
launch touches the 2^13 selected elements at the top of the address range -- 64 KiB -- so the test is an allocation, a fill and
a count: the selected elements must equal the numpy permutation exactly, decoys elsewhere must keep their values, and the
number of non-zero elements of the whole state must stay what it was.  A base address narrowed to 32 bits, a hole inserted in
the wrong order or a control bit OR-ed in at the wrong place moves the writes onto zeros or decoys and changes all three."""
import numpy as np
import pytest
import torch

import artensor_amd as A

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GIB = 1 << 30


def test_high_controls_and_a_target_past_element_2_to_the_31():
    nq, dtype = 32, torch.complex64
    need = (8 << nq) + 4 * GIB                                             # the free-memory rule of test_state_ops_large_gpu
    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < need:
        pytest.skip(f"needs {need / GIB:.1f} GiB of free device memory (one array of 32 GiB and 4 GiB of temporaries), {free / GIB:.1f} GiB free")
    store = torch.zeros(1 << nq, dtype=dtype, device=DEV)
    view = store.view((2,) * nq)
    dim = lambda b: nq - 1 - b                                             # memory bit b of the contiguous view
    cbits = list(range(12, 31))
    values = [0] + [1] * 18
    want_mask = sum(v << b for b, v in zip(cbits, values))
    # the selected elements: bits 1..11 free, bits 0 and 31 the targets
    low = np.arange(1 << 12, dtype=np.int64)
    index = np.concatenate([want_mask | low, want_mask | low | 1 << 31])   # [row digit of bit 31][bits 0..11]
    vals = (np.arange(1, index.size + 1) + 1j * (np.arange(index.size) % 97 - 48.5)).astype(np.complex64)
    store[torch.from_numpy(index).to(DEV)] = torch.from_numpy(vals).to(DEV)
    decoys = np.array([0, 1, (1 << 31) - 1, 1 << 31, want_mask | 1 << 12, (want_mask | 1 << 31 | 1 << 12) + 5, want_mask ^ 1 << 30,
                       (1 << 32) - 1, want_mask & 0xFFFFFFF, (want_mask | 1 << 31) & ((1 << 31) - 1) & ~(1 << 20)], dtype=np.int64)
    assert not set(decoys) & set(index)
    store[torch.from_numpy(decoys).to(DEV)] = torch.tensor(-7.25 + 1234.5j, dtype=dtype, device=DEV)
    count = int(torch.count_nonzero(store))
    assert count == index.size + decoys.size == 2 ** 13 + 10
    # rows (bit 31, bit 0): new[0] = i old[3], new[1] = -old[2], new[2] = old[0], new[3] = -i old[1]
    m = np.zeros((4, 4), dtype=np.complex128)
    m[0, 3], m[1, 2], m[2, 0], m[3, 1] = 1j, -1, 1, -1j
    info = A.controlled_gate_info(view.shape, view.stride(), m, (dim(31), dim(0)), [dim(b) for b in cbits], values)
    assert info["target_bits"] == (31, 0) and info["c_high"] == 19 and info["n_selected"] == 2 ** 13 and info["n_tiles"] == 2
    assert info["bytes_read"] == 64 * 1024
    A.apply_controlled_gate_(view, m, (dim(31), dim(0)), [dim(b) for b in cbits], values)
    got = store[torch.from_numpy(index).to(DEV)].cpu().numpy()
    old = vals.reshape(2, 1 << 11, 2)                                      # [bit 31][bits 1..11][bit 0]
    new = np.empty_like(old)
    new[0, :, 0], new[0, :, 1] = 1j * old[1, :, 1], -old[1, :, 0]
    new[1, :, 0], new[1, :, 1] = old[0, :, 0], -1j * old[0, :, 1]
    assert np.array_equal(got, new.reshape(-1))
    assert bool((store[torch.from_numpy(decoys).to(DEV)] == torch.tensor(-7.25 + 1234.5j, dtype=dtype, device=DEV)).all())
    assert int(torch.count_nonzero(store)) == count
