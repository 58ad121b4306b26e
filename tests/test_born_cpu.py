"""Host-side checks of the Born-statistics layer (artensor_amd/born.py, artn_born_* / artn_marginal*): the two host-only
queries, the memory-index translation and the argument checks.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import born


def contiguous_strides(shape):
    out, s = [], 1
    for e in reversed(shape):
        out.append(s)
        s *= e
    return out[::-1]


def test_born_plan_covers_every_size_and_its_workspace_grows_with_n():
    sizes = sorted({1, 2, 3, 4, 5, 1000, 1023, 1024, 1025, 2 ** 20 + 7, 2 ** 24, 2 ** 30, 2 ** 30 + 1, 2 ** 32 - 1, 2 ** 32}
                   | {2 ** k for k in range(33)} | {2 ** k + 1 for k in range(32)} | {3 ** k for k in range(1, 21)})
    last_ws = 0
    for dtype in (torch.complex64, torch.complex128):
        last_ws = 0
        for n in sizes:
            p = born.born_plan(n, dtype)
            assert 10 <= p["block_bits"] <= 14
            assert p["n_blocks"] * 2 ** p["block_bits"] >= n > (p["n_blocks"] - 1) * 2 ** p["block_bits"]
            assert p["workspace_bytes"] > 0 and p["workspace_bytes"] >= last_ws
            assert p["workspace_bytes"] == 32 * p["overlap_grid"]
            last_ws = p["workspace_bytes"]
    assert born.born_plan(2 ** 30)["n_blocks"] == 2 ** 16          # the block-sum array of the full-size state: 512 KiB
    assert born.born_plan(2 ** 32)["n_blocks"] <= 2 ** 18
    plan = N.ArtnBornPlan()
    assert N.lib().artn_born_plan(0, N.ARTN_C64, ctypes.byref(plan)) == -1
    assert N.lib().artn_born_plan(16, N.ARTN_C64_BF16, ctypes.byref(plan)) == -2


def test_marginal_query_picks_the_kernel_and_sizes_the_output():
    shape = (2,) * 20
    info = born.marginal_info(shape, contiguous_strides(shape), [0, 3, 19])
    assert info["kernel"] == N.MARGINAL_STREAM and info["out_elems"] == 8 and info["chunk_bits"] == 12
    assert info["bin_bits"] == 1 and info["workspace_bytes"] == 8 * info["grid"] * 2
    info = born.marginal_info(shape, contiguous_strides(shape), [])
    assert info["kernel"] == N.MARGINAL_STREAM and info["out_elems"] == 1 and info["workspace_bytes"] > 0
    info = born.marginal_info(shape, contiguous_strides(shape), list(range(20)))
    assert info["kernel"] == N.MARGINAL_STREAM and info["out_elems"] == 2 ** 20
    info = born.marginal_info((1024, 2, 2, 2), contiguous_strides((1024, 2, 2, 2)), [0])
    assert info["kernel"] == N.MARGINAL_STREAM and info["out_elems"] == 1024
    info = born.marginal_info((3,) * 8, contiguous_strides((3,) * 8), [1, 6])
    assert info["kernel"] == N.MARGINAL_GENERIC and info["out_elems"] == 9 and info["workspace_bytes"] == 0
    info = born.marginal_info((1000, 2, 2, 2), contiguous_strides((1000, 2, 2, 2)), [0])
    assert info["kernel"] == N.MARGINAL_GENERIC and info["out_elems"] == 1000
    info = born.marginal_info((2,) * 8, contiguous_strides((2,) * 8), [0])     # below one chunk: the plain kernel
    assert info["kernel"] == N.MARGINAL_GENERIC
    # a permuted dense layout is as good as a contiguous one
    perm = [3, 0, 2, 1] + list(range(4, 20))
    st = contiguous_strides(shape)
    info = born.marginal_info(shape, [st[p] for p in perm], [1, 2])
    assert info["kernel"] == N.MARGINAL_STREAM and info["out_elems"] == 4
    # the streaming kernel's stated limit: 2^24 kept elements
    shape = (2,) * 26
    with pytest.raises(RuntimeError, match="2\\^24"):
        born.marginal_info(shape, contiguous_strides(shape), list(range(25)))
    assert born.marginal_info(shape, contiguous_strides(shape), list(range(24)))["out_elems"] == 2 ** 24


def test_marginal_query_refuses_layouts_that_are_not_dense():
    def rc(shape, strides, keep):
        d, _ = born._marginal_desc(shape, strides, keep, torch.complex64)
        info = N.ArtnMarginalInfo()
        return N.lib().artn_marginal_query(ctypes.byref(d), ctypes.byref(info))

    assert rc((4, 4), (4, 1), [0]) == 0
    assert rc((4, 4), (1, 4), [0]) == 0
    assert rc((4, 4), (1, 1), [0]) == -1            # overlapping
    assert rc((4, 4), (2, 1), [0]) == -1            # overlapping
    assert rc((4, 4), (8, 1), [0]) == -1            # gaps (a slice of a wider tensor)
    assert rc((4, 4), (4, 2), [0]) == -1            # strided
    assert rc((4, 4), (0, 1), [0]) == -1            # expanded
    assert b"dense" in N.lib().artn_last_error()
    assert rc((4, 1, 4), (4, 77, 1), [0]) == 0      # the stride of an extent-1 dim means nothing
    assert rc((3, 5), (5, 1), [1]) == 0
    assert rc((3, 5), (1, 3), [1]) == 0
    assert rc((3, 5), (4, 1), [1]) == -1


@pytest.mark.parametrize("mem_shape", [(2,) * 12, (5, 2, 3, 4), (7, 2, 2)])
def test_memory_index_translates_to_the_logical_multi_index(mem_shape):
    rng = np.random.default_rng(len(mem_shape))
    n = int(np.prod(mem_shape))
    for _ in range(5):
        perm = rng.permutation(len(mem_shape))
        arr = np.arange(n, dtype=np.int64).reshape(mem_shape).transpose(perm)     # arr[multi-index] = memory index
        strides = [s // 8 for s in arr.strides]
        logical = np.arange(n)
        want = np.stack(np.unravel_index(logical, arr.shape), axis=-1)
        mem = arr.reshape(-1)                                                      # memory index of every logical position
        got = born.memory_to_multi_index(mem, arr.shape, strides)
        assert got.shape == want.shape and (got == want).all()
        got_t = born.memory_to_multi_index(torch.from_numpy(mem.copy()), arr.shape, strides)
        assert (got_t.numpy() == want).all()


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the CPU-only refusal")
def test_born_functions_have_no_cpu_fallback():
    a = torch.zeros(4, 4, dtype=torch.complex64)
    for call in (lambda: A.overlap(a, a), lambda: A.norm2(a), lambda: A.fidelity(a, a), lambda: A.marginal_probabilities(a, [0]),
                 lambda: A.sample(a, 4), lambda: A.sample(a, uniforms=torch.zeros(3, dtype=torch.float64)),
                 lambda: born.block_sums(a)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    buf = np.zeros(64, dtype=np.complex64)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    lib = N.lib()
    assert lib.artn_born_overlap(p, p, 4, N.ARTN_C64, p, 64, p, None) == -4
    assert lib.artn_born_block_sums(p, 4, N.ARTN_C64, p, p, None) == -4
    assert lib.artn_born_pick(p, 4, N.ARTN_C64, p, p, 1, p, p, None) == -4
    d, _ = born._marginal_desc((4, 4), (4, 1), [0], torch.complex64)
    assert lib.artn_marginal(ctypes.byref(d), p, p, p, 0, None) == -4


def test_layout_and_argument_checks_raise_value_errors():
    x = torch.zeros(8, 8, dtype=torch.complex64)
    assert born._dense_layout(x.shape, x.stride()) == 64
    assert born._dense_layout(x.t().shape, x.t().stride()) == 64
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        born._dense_layout(x[:, :1].shape, x[:, :1].stride())            # a column of a wider matrix
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        born._dense_layout(x[:, :4].shape, x[:, :4].stride())
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        born._dense_layout(x[::2].shape, x[::2].stride())
    with pytest.raises(ValueError, match=r"\.contiguous\(\)"):
        born._dense_layout(x[0].expand(8, 8).shape, x[0].expand(8, 8).stride())
    with pytest.raises(ValueError, match="keep"):
        born._marginal_desc((2, 2), (2, 1), [0, 0], torch.complex64)
    with pytest.raises(ValueError, match="keep"):
        born._marginal_desc((2, 2), (2, 1), [2], torch.complex64)


def test_uniforms_are_checked_before_anything_runs():
    a = torch.zeros(16, dtype=torch.complex64)
    for bad in (torch.tensor([0.5, 1.0], dtype=torch.float64), torch.tensor([-1e-9], dtype=torch.float64),
                torch.tensor([float("nan")], dtype=torch.float64), torch.tensor([0.5], dtype=torch.float32),
                torch.zeros(2, 2, dtype=torch.float64), [0.5]):
        with pytest.raises(ValueError, match="uniforms"):
            A.sample(a, uniforms=bad)
    with pytest.raises(ValueError):
        A.sample(a)
    assert born._checked_uniforms(torch.tensor([0.0, 1.0 - 2.0 ** -53], dtype=torch.float64)).numel() == 2


def test_linear_xeb():
    assert A.linear_xeb(torch.full((7,), 2.0 ** -10, dtype=torch.float64), 10) == 0.0
    assert abs(A.linear_xeb(torch.full((7,), 2.0 ** -9, dtype=torch.float64), 10) - 1.0) < 1e-15
