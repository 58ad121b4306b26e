"""The in-place bit permutations on the device, compared with the numpy oracle by exact equality on integer views of the bytes.

The data are random 32- and 64-bit patterns reinterpreted as floats, so NaN payloads, -0.0, denormals and infinities are among
them: an element may only ever be copied.  Every state lies inside a larger allocation between two guard bands that must keep
their bytes.  Sizes: below one tile, exactly one tile, two tiles, and 2^20 complex64 where the reversal and the rotation need
more than one pass."""
import numpy as np
import pytest
import torch

import artensor_amd as A

import bit_permutation_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GUARD = 64                                                                   # elements on either side: the state stays 16-byte aligned
LINE = {torch.complex64: 4, torch.complex128: 3}
SIZES = [(torch.complex64, nb) for nb in (8, 12, 13, 16, 20)] + [(torch.complex128, nb) for nb in (7, 11, 12, 18)]


def words(dtype):
    return 1 if dtype == torch.complex64 else 2                              # int64 words per element


def random_store(n, dtype, seed):
    """(the whole allocation as a complex tensor [GUARD + n + GUARD], its bytes as a host int64 array [.., words])."""
    rng = np.random.default_rng(seed)
    host = rng.integers(-(1 << 63), (1 << 63) - 1, size=(n + 2 * GUARD, words(dtype)), dtype=np.int64)
    host[::97] = 0x7FF0000000000001 if dtype == torch.complex128 else 0x7F8000017FC00001   # NaN payloads for certain
    host[1::89] = -(1 << 63)                                                 # -0.0 (complex128) / (+0.0, -0.0) (complex64)
    dev = torch.from_numpy(host).to(DEV)
    store = torch.view_as_complex(dev.view(torch.float32).view(-1, 2)) if dtype == torch.complex64 else \
        torch.view_as_complex(dev.view(torch.float64).view(-1, 2))
    assert store.numel() == n + 2 * GUARD and store.dtype == dtype
    return store, host


def bytes_of(store):
    """The allocation's bytes as a host int64 array [.., words]."""
    real = torch.view_as_real(store)
    ints = real.view(torch.int64) if store.dtype == torch.complex128 else real.reshape(-1).view(torch.int64).view(-1, 1)
    return ints.cpu().numpy()


def state_view(store, shape, strides):
    return torch.as_strided(store, tuple(shape), tuple(strides), GUARD)


def check(store, host, want_state):
    got = bytes_of(store)
    n = want_state.shape[0]
    assert np.array_equal(got[:GUARD], host[:GUARD]) and np.array_equal(got[GUARD + n:], host[GUARD + n:]), "a guard band changed"
    assert np.array_equal(got[GUARD:GUARD + n], want_state)


def cases_for(nb, dtype, seed):
    rng = np.random.default_rng(seed)
    cases = dict(O.named_permutations(nb, LINE[dtype]))
    for k in range(3):
        cases[f"random{k}"] = [int(b) for b in rng.permutation(nb)]
    some = rng.choice(nb, size=min(nb, 5), replace=False)                    # a few short cycles
    sparse = list(range(nb))
    for b, c in zip(sorted(some), some):
        sparse[int(b)] = int(c)
    cases["sparse"] = sparse
    return cases


@pytest.mark.parametrize("dtype, nb", SIZES)
def test_named_and_random_permutations_match_the_oracle_bit_for_bit(dtype, nb):
    n = 1 << nb
    shape, strides = (2,) * nb, O.contiguous_strides((2,) * nb)
    store, host = random_store(n, dtype, 100 + nb)
    state = host[GUARD:GUARD + n].copy()
    for name, dst in cases_for(nb, dtype, nb).items():
        p = A.BitPermutation(shape, strides, dtype, dst_bit=dst, device=DEV)
        info = A.bit_permutation_info(shape, strides, dtype, dst_bit=dst)
        assert p.passes == info["passes"]
        if nb == 20 and name in ("reversal", "rotation"):
            assert 2 <= p.passes <= 3
        out = p(state_view(store, shape, strides))
        assert out.data_ptr() == store.data_ptr() + GUARD * store.element_size()
        state = O.permute_bits(state, dst)                                   # the permutations accumulate on one state
        check(store, host, state)
    # a permutation and then its inverse give the state back
    before = state.copy()
    dst = cases_for(nb, dtype, nb)["random0"]
    view = state_view(store, shape, strides)
    A.BitPermutation(shape, strides, dtype, dst_bit=dst, device=DEV)(view)
    A.BitPermutation(shape, strides, dtype, dst_bit=O.inverse(dst), device=DEV)(view)
    check(store, host, before)


@pytest.mark.parametrize("dtype, nb", [(torch.complex64, 13), (torch.complex128, 12)])
def test_the_identity_issues_no_launch_and_leaves_the_bytes(dtype, nb):
    shape, strides = (2,) * nb, O.contiguous_strides((2,) * nb)
    store, host = random_store(1 << nb, dtype, 5)
    info = A.bit_permutation_info(shape, strides, dtype, perm=list(range(nb)))
    assert info["passes"] == 0 and info["bytes_moved"] == 0 and info["pass_info"] == []
    view = state_view(store, shape, strides)
    assert A.permute_dims_(view, list(range(nb))) is view
    assert A.BitPermutation(shape, strides, dtype, perm=list(range(nb)), device=DEV)._table is None
    check(store, host, host[GUARD:GUARD + (1 << nb)])


@pytest.mark.parametrize("dtype, nb", [(torch.complex64, 13), (torch.complex128, 12)])
def test_a_transposition_equals_the_swap_gate_on_finite_data(dtype, nb):
    gen = torch.Generator(device=DEV).manual_seed(3)
    swap = np.eye(4)[[0, 2, 1, 3]]
    for d0, d1 in ((nb - 1, nb - 3), (nb - 2, 0), (0, 1), (1, nb - 1)):      # low/low, low/high, high/high, high/low
        a = torch.randn((2,) * nb, dtype=dtype, device=DEV, generator=gen)
        b = a.clone()
        assert A.swap_dims_(a, d0, d1) is a
        A.apply_gate_(b, swap, (d0, d1))
        assert np.array_equal(bytes_of(a.reshape(-1)), bytes_of(b.reshape(-1)))
    a = torch.randn((2,) * nb, dtype=dtype, device=DEV, generator=gen)
    old = a.clone()
    A.reverse_qubits_(a)
    assert torch.equal(a, old.permute(list(range(nb - 1, -1, -1))))
    A.reverse_qubits_(a, dims=(0, 3, nb - 1))
    want = old.permute(list(range(nb - 1, -1, -1))).permute([nb - 1 if k == 0 else 0 if k == nb - 1 else k for k in range(nb)])
    assert torch.equal(a, want)


LAYOUTS = [                                                                 # (shape, the dims in memory, slowest first)
    ((2, 4, 1, 8, 2, 4, 2, 2, 8, 2), (3, 0, 5, 1, 9, 2, 4, 8, 6, 7)),        # 2^14: extents 1, 4 and 8, permuted strides
    ((4, 2, 4, 2, 1, 2, 8, 2, 2, 4), (5, 3, 0, 9, 1, 4, 2, 8, 7, 6)),        # 2^14
    ((8, 8, 2, 1, 2, 2, 2, 2, 2, 2), (1, 4, 2, 0, 3, 9, 8, 5, 7, 6)),        # 2^13
]


def bits_of(t):
    """A logical tensor's bits, in logical order, as a contiguous integer tensor."""
    real = torch.view_as_real(t).contiguous()
    return real.view(torch.int32 if t.dtype == torch.complex64 else torch.int64)


def perm_within_extents(rng, shape):
    perm = list(range(len(shape)))
    for e in sorted(set(shape)):
        same = [k for k in range(len(shape)) if shape[k] == e]
        for k, src in zip(same, rng.permutation(same)):
            perm[k] = int(src)
    return perm


@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128])
@pytest.mark.parametrize("shape, memory_order", LAYOUTS)
def test_permuted_layouts_extents_1_4_8_and_a_storage_offset(dtype, shape, memory_order):
    strides = O.contiguous_strides(shape, memory_order)
    n = int(np.prod(shape))
    rng = np.random.default_rng(n + len(shape))
    store, host = random_store(n, dtype, 17)
    amps = state_view(store, shape, strides)
    assert amps.storage_offset() == GUARD and amps.data_ptr() % 16 == 0
    state = host[GUARD:GUARD + n].copy()
    # permute_dims_: same shape and strides, the dims trade places
    for _ in range(3):
        perm = perm_within_extents(rng, shape)
        old = bits_of(amps).clone()
        assert A.permute_dims_(amps, perm) is amps
        assert torch.equal(bits_of(amps), old.permute(perm + [len(shape)]))
        state = O.permute_bits(state, O.dst_bit_of_perm(shape, strides, perm))
        check(store, host, state)
    # relayout_: the data moves, a new view shows the old tensor
    for order in (None, [int(k) for k in rng.permutation(len(shape))]):
        old = bits_of(amps).clone()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        t = A.relayout_(amps, order)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - before
        assert grown < 32 * 1024, grown                                      # a table, never a second buffer
        assert t.data_ptr() == amps.data_ptr() and tuple(t.shape) == tuple(shape)
        assert tuple(s for s, e in zip(t.stride(), shape) if e != 1) == \
            tuple(s for s, e in zip(O.contiguous_strides(shape, order), shape) if e != 1)
        if order is None:
            assert t.is_contiguous()
        assert torch.equal(bits_of(t), old)                                  # == old.contiguous(), bit for bit
        dst, _ = O.dst_bit_of_order(shape, strides, order)
        state = O.permute_bits(state, dst)
        check(store, host, state)
        amps, strides = t, tuple(t.stride())                                 # (the old view is stale)


def test_a_prebuilt_permutation_serves_two_tensors_and_a_side_stream():
    nb, dtype = 14, torch.complex64
    shape, strides = (2,) * nb, O.contiguous_strides((2,) * nb)
    dst = [int(b) for b in np.random.default_rng(9).permutation(nb)]
    p = A.BitPermutation(shape, strides, dtype, dst_bit=dst, device=DEV)
    assert p.passes >= 1 and p.bytes_moved == 2 * 8 * (1 << nb) * p.passes
    stores = [random_store(1 << nb, dtype, seed) for seed in (1, 2, 3)]
    p(state_view(stores[0][0], shape, strides))
    p(state_view(stores[1][0], shape, strides))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        p(state_view(stores[2][0], shape, strides))
    side.synchronize()
    for store, host in stores:
        check(store, host, O.permute_bits(host[GUARD:GUARD + (1 << nb)], dst))
    with pytest.raises(ValueError, match="built for shape"):
        p(torch.zeros((2,) * (nb - 1), dtype=dtype, device=DEV))
    with pytest.raises(ValueError, match="16-byte boundary"):
        A.swap_dims_(torch.as_strided(stores[0][0], shape, strides, 1), 0, 1)
