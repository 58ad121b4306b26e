"""trajectories.sample_batch on the device.  Row b is bit for bit what born.sample gives on a dense clone of slice b with its dims
in local-bit order and uniforms[b] -- flat index (deposited into the memory bits that are no batch bits, OR'd with b in the
fields), probability and norm -- for both forms (SMALL: M < 10, one launch; TILED: three), both dtypes and every placement of the
batch bits; Gaussian-integer states equal the numpy oracle of sample_batch_oracle.py exactly, boundary uniforms included; a row
depends neither on where the batch bits lie nor on poisoned or empty neighbours; uniforms come back to their own positions; runs
and a graph replay repeat bit for bit; nothing outside the operands is touched.  Every comparison is == on integers or on the
bits of float64: there is no tolerance in this file.  At most 2^16 elements per case except the one M = 21 case (32 MiB)."""
import ctypes

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import born
from artensor_amd._state import _desc

import guard_bands as GB
import sample_batch_oracle as SO
import trajectories_oracle as TO
from graph_replay import capture_and_replay
from test_pauli_batch_gpu import Lay, layout
from test_sample_batch_cpu import exact_uniforms, integer_state
from test_trajectories_gpu import KINDS, crand, poison

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def i64(t):
    return t.contiguous().view(torch.int64)


def fields_of(lay, batch):
    return A.sample_batch_info(lay.view.shape, lay.view.stride(), batch, 1, lay.view.dtype)["fields"]


def unbatched_rows(lay, batch, local, u):
    """(flat int64 [B, S], prob float64 [B, S], norms float64 [B]) on the host from born.sample / born.block_sums on a dense clone
    of every slice with its dims in local-bit order; the local index goes through the oracle's address table."""
    nd = lay.logical.ndim
    sl = TO.slices(lay.logical, batch)
    rest = [d for d in range(nd) if d not in batch]
    order = sorted(range(len(rest)), key=lambda i: -local.index(lay.dims[rest[i]][0]))
    n_bits = sum(w for _, w in lay.dims)
    table = SO.address_table(n_bits, fields_of(lay, batch))
    flat, prob, norms = [], [], []
    for b in range(sl.shape[0]):
        clone = torch.from_numpy(np.ascontiguousarray(sl[b].transpose(order)).reshape(-1)).to(DEV)
        idx, p = born.sample(clone, uniforms=u[b])
        flat.append(table[b][idx[:, 0].cpu().numpy()])
        prob.append(p)
        norms.append(born.block_sums(clone)[1][-1])
    return np.stack(flat), torch.stack(prob), torch.stack(norms)


def assert_rows_equal_unbatched(lay, batch, local, u):
    flat, prob, norms = A.sample_batch_flat(lay.view, batch, uniforms=u)
    B, S = u.shape
    assert flat.shape == prob.shape == (B, S) and norms.shape == (B,)
    assert flat.dtype == torch.int64 and prob.dtype == norms.dtype == torch.float64
    want_flat, want_prob, want_norms = unbatched_rows(lay, batch, local, u)
    assert (flat.cpu().numpy() == want_flat).all(), np.argwhere(flat.cpu().numpy() != want_flat)[:8]
    assert (i64(prob) == i64(want_prob)).all() and (i64(norms) == i64(want_norms)).all()
    idx, prob2 = A.sample_batch(lay.view, batch, uniforms=u)
    assert idx.shape == (B, S, lay.view.dim()) and (i64(prob2) == i64(prob)).all()
    assert (idx == born.memory_to_multi_index(flat, lay.view.shape, lay.view.stride())).all()
    strides = torch.tensor(lay.view.stride(), device=DEV)
    assert ((idx * strides).sum(dim=-1) == flat).all()
    digits = idx[..., batch]                                                  # the batch dims' columns hold the digits of b
    b_of = torch.zeros((B, S), dtype=torch.int64, device=DEV)
    for k, d in enumerate(batch):
        b_of = b_of * lay.view.shape[d] + digits[..., k]
    assert (b_of == torch.arange(B, device=DEV)[:, None]).all()


# ---- 1. bit for bit against the unbatched call ----------------------------------------------------------------------------------------
# (kind, M, batch fields (lo, width) in the order listed = most significant first, S, storage offset in elements)
CASES_1 = [
    # SMALL, complex64 (line bit 4)
    ("c64", 4, [(4, 1)], 1, 0),                 # B = 2: one tile with 248 guarded lanes; the field at the line bit
    ("c64", 4, [(4, 3)], 3, 0),
    ("c64", 4, [(4, 8)], 257, 0),               # B = 2^8: four virtual tiles
    ("c64", 5, [(4, 1)], 3, 0),
    ("c64", 5, [(5, 3)], 257, 0),               # the field at the top
    ("c64", 5, [(4, 4), (9, 4)], 3, 0),         # two split fields listed in the order opposite to memory
    ("c64", 9, [(6, 1)], 257, 0),               # the field in the middle
    ("c64", 9, [(5, 2), (11, 1)], 1, 0),        # one extent-4 batch dim
    ("c64", 9, [(9, 8)], 3, 2),                 # a base 16 bytes into its storage
    # SMALL, complex128 (line bit 3)
    ("c128", 3, [(3, 1)], 3, 0),
    ("c128", 3, [(3, 3)], 257, 0),
    ("c128", 4, [(3, 1), (5, 7)], 1, 0),
    ("c128", 5, [(4, 1)], 1, 0),
    ("c128", 9, [(5, 3)], 257, 1),
    # TILED
    ("c64", 10, [(4, 1)], 257, 0),
    ("c64", 10, [(7, 2), (12, 1)], 3, 0),
    ("c64", 11, [(11, 1)], 1, 0),
    ("c64", 11, [(4, 1), (10, 2)], 257, 2),
    ("c64", 13, [(9, 1)], 3, 0),
    ("c64", 13, [(13, 2), (6, 1)], 257, 0),
    ("c128", 10, [(3, 1)], 3, 0),
    ("c128", 11, [(6, 1), (3, 2)], 257, 0),
    ("c128", 13, [(13, 1)], 1, 1),
    ("c128", 13, [(4, 2), (15, 1)], 3, 0),
]


@pytest.mark.parametrize("kind,M,fields,S,offset", CASES_1, ids=lambda v: str(v).replace(" ", ""))
def test_rows_equal_the_unbatched_call_bit_for_bit(kind, M, fields, S, offset):
    n_bits = M + sum(w for _, w in fields)
    rng = np.random.default_rng(100 * n_bits + S)
    dims, batch, local = layout(n_bits, fields)
    assert len(local) == M
    lay = Lay(kind, crand(rng, 2 ** n_bits, kind), dims, offset)
    assert lay.view.data_ptr() % 16 == 0 and (offset == 0 or lay.view.data_ptr() % 32 != 0)
    before = lay.memory_bits()
    info = A.sample_batch_info(lay.view.shape, lay.view.stride(), batch, S, lay.view.dtype)
    assert info["form"] == ("SMALL" if M < 10 else "TILED") and info["B"] == 2 ** (n_bits - M) and info["local_bits"] == M
    u = torch.from_numpy(rng.random((info["B"], S))).to(DEV)
    assert_rows_equal_unbatched(lay, batch, local, u)
    assert (lay.memory_bits() == before).all()


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("n_bits", [9, 12])
def test_without_batch_dims_it_is_born_sample(kind, n_bits):
    rng = np.random.default_rng(n_bits)
    dims, batch, _ = layout(n_bits, [])
    lay = Lay(kind, crand(rng, 2 ** n_bits, kind), dims)
    u = torch.from_numpy(rng.random(300)).to(DEV)
    idx, prob = A.sample_batch(lay.view, (), uniforms=u[None])
    want_idx, want_prob = born.sample(lay.view, uniforms=u)
    assert idx.shape == (1, 300, n_bits) and (idx[0] == want_idx).all() and (i64(prob[0]) == i64(want_prob)).all()
    _, _, norms = A.sample_batch_flat(lay.view, None, uniforms=u[None])
    assert (i64(norms) == i64(born.block_sums(lay.view)[1][-1:])).all()


# ---- 2. more than 1024 blocks per trajectory: the row prefix with K = 2, one workgroup per trajectory ---------------------------------
def device_case(M, S, seed):
    """(tensor [2^(M-4), 2, 16] with its batch bit at memory bit 4, uniforms [2, S]), filled on the device."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.view_as_complex(torch.randn((2 ** (M - 4), 2, 16, 2), dtype=torch.float32, device=DEV, generator=g))
    return t, torch.rand((2, S), dtype=torch.float64, device=DEV, generator=g)


def assert_device_case_equals_unbatched(t, u):
    flat, prob, norms = A.sample_batch_flat(t, [1], uniforms=u)
    for b in range(2):
        clone = t[:, b, :].contiguous().reshape(-1)
        idx, p = born.sample(clone, uniforms=u[b])
        l = idx[:, 0]
        assert (flat[b] == (((l >> 4) << 5) | (b << 4) | (l & 15))).all()
        assert (i64(prob[b]) == i64(p)).all() and (i64(norms[b:b + 1]) == i64(born.block_sums(clone)[1][-1:])).all()


def test_2048_blocks_per_trajectory():
    t, u = device_case(21, 64, 21)
    info = A.sample_batch_info(t.shape, t.stride(), [1], 64)
    assert (info["blocks_per_trajectory"], info["block_bits"], info["grid"][1]) == (2048, 10, 2)
    assert_device_case_equals_unbatched(t, u)


# ---- 3. exact-integer states against the oracle ---------------------------------------------------------------------------------------
def boundary_uniforms(cs, bb):
    """Uniforms exactly on a block prefix and on a segment prefix of one trajectory (c / total * total == c, 0 < c < total)."""
    total = cs[-1]
    ok = lambda c: 0 < c < total and (c / total) * total == c               # noqa: E731
    block = [c / total for c in cs[(1 << bb) - 1::1 << bb] if ok(c)][:1]
    seg = [c / total for c in cs[3::4] if ok(c) and c / total not in block][:2]
    return block, seg


@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("n_bits,fields", [(10, [(5, 2, 0)]), (14, [(12, 1, 1), (6, 1, 0)]), (13, [(12, 1, 0)])],
                         ids=lambda v: str(v).replace(" ", ""))
def test_integer_states_equal_the_oracle(kind, n_bits, fields):
    M = n_bits - sum(w for _, w, _ in fields)
    for seed in range(64):                                                    # (the first state whose boundaries are exact in float64)
        mem, table = integer_state(np.random.default_rng(seed), n_bits, fields, KINDS[kind][0])
        B = table.shape[0]
        rows = []
        for b in range(B):
            cs = np.cumsum(SO.terms(mem[table[b]]))
            block, seg = boundary_uniforms(cs, 10)
            rows.append((list(exact_uniforms(cs)[0]), block, seg))
        plain = [r for b, r in enumerate(rows) if B < 4 or 0 < b < B - 1]     # (not the one-element trajectories)
        if all(len(seg) == 2 and (M < 11 or block) for _, block, seg in plain):
            break
    else:
        raise AssertionError("no state with exact boundaries among 64 seeds")
    S = max(len(a) + len(b) + len(c) for a, b, c in rows)
    uniforms = np.stack([np.array((a + b + c + a * S)[:S]) for a, b, c in rows])
    uniforms = uniforms[:, np.random.default_rng(1).permutation(S)]
    dims = [(p, 1) for p in SO.local_positions(n_bits, fields)] + [(s, w) for s, w, _ in fields]
    batch = list(range(M, len(dims)))
    lay = Lay(kind, mem, dims)
    assert fields_of(lay, batch) == fields
    flat, prob, norms = A.sample_batch_flat(lay.view, batch, uniforms=torch.from_numpy(uniforms).to(DEV))
    want_flat, want_prob, want_norms = SO.finish(*SO.sample_rows(mem, n_bits, fields, uniforms))
    assert (flat.cpu().numpy() == want_flat).all()
    assert (prob.cpu().numpy() == want_prob).all() and (norms.cpu().numpy() == want_norms).all()
    assert (flat >= 0).all() and (SO.terms(mem[flat.cpu().numpy()]) > 0).all()   # no zero-probability element is ever returned
    if B >= 4:                                                                # all weight on the first / on the last element
        assert (flat[0] == int(table[0][0])).all() and (flat[-1] == int(table[-1][-1])).all()


# ---- 4. independence ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,M", [("c64", 7), ("c128", 6), ("c64", 11), ("c128", 10)])
def test_rows_depend_neither_on_the_placement_nor_on_their_neighbours(kind, M):
    rng = np.random.default_rng(M)
    lb = KINDS[kind][3]
    n_bits, B, S = M + 2, 4, 33
    rows = crand(rng, (B, 2 ** M), kind)
    u = torch.from_numpy(rng.random((B, S))).to(DEV)
    results = []
    for fields in ([(lb, 2, 0)], [(lb + 1, 1, 1), (n_bits - 1, 1, 0)]):
        table = SO.address_table(n_bits, fields)
        dims = [(p, 1) for p in SO.local_positions(n_bits, fields)] + [(s, w) for s, w, _ in fields]
        batch = list(range(M, len(dims)))
        for fill in ("clean", "poison", "zero"):
            mine = rows.copy()
            if fill == "poison":
                mine[1] = poison(rng, 2 ** M, kind)
                mine[1][0] = np.nan
            if fill == "zero":
                mine[1] = 0
                mine[3] = 0
            mem = np.zeros(2 ** n_bits, dtype=rows.dtype)
            mem[table.reshape(-1)] = mine.reshape(-1)
            lay = Lay(kind, mem, dims)
            assert fields_of(lay, batch) == fields
            before = lay.memory_bits()
            flat, prob, norms = A.sample_batch_flat(lay.view, batch, uniforms=u)
            assert (lay.memory_bits() == before).all()                        # the state is only read
            flat = flat.cpu().numpy()
            local = np.stack([np.where(flat[b] < 0, -1, np.searchsorted(table[b], flat[b])) for b in range(B)])
            assert all((table[b][local[b]] == flat[b]).all() for b in range(B) if (flat[b] >= 0).all())
            dead = {"clean": [], "poison": [1], "zero": [1, 3]}[fill]
            for b in dead:                                                    # dead rows: -1 / NaN, and -1 in every column of idx
                assert (flat[b] == -1).all() and torch.isnan(prob[b]).all()
                assert (A.sample_batch(lay.view, batch, uniforms=u)[0][b] == -1).all()
            assert not torch.isfinite(norms[1]) if fill == "poison" else True
            results.append((dead, local, i64(prob).cpu().numpy(), i64(norms).cpu().numpy()))
    _, local0, prob0, norms0 = results[0]
    assert (local0 >= 0).all()
    for dead, local, prob, norms in results[1:]:
        live = [b for b in range(B) if b not in dead]
        assert (local[live] == local0[live]).all() and (prob[live] == prob0[live]).all() and (norms[live] == norms0[live]).all()


# ---- 5. the uniforms' positions, the generator, S = 0 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("M,fields", [(6, [(4, 3)]), (11, [(8, 2)])], ids=["small", "tiled"])
def test_uniforms_come_back_to_their_own_positions(M, fields):
    n_bits = M + sum(w for _, w in fields)
    rng = np.random.default_rng(M)
    dims, batch, _ = layout(n_bits, fields)
    lay = Lay("c64", crand(rng, 2 ** n_bits, "c64"), dims)
    B = 2 ** (n_bits - M)
    base = rng.random((B, 40))
    u = np.concatenate([base, base[:, :25], base[:, 5:6].repeat(7, axis=1)], axis=1)   # duplicates
    perm = rng.permutation(u.shape[1])
    f0, p0, n0 = A.sample_batch_flat(lay.view, batch, uniforms=torch.from_numpy(np.sort(u, axis=1)).to(DEV))
    f1, p1, n1 = A.sample_batch_flat(lay.view, batch, uniforms=torch.from_numpy(u[:, perm]).to(DEV))
    where = torch.from_numpy(np.argsort(np.argsort(u[:, perm], axis=1, kind="stable"), axis=1, kind="stable")).to(DEV)
    assert (f1 == torch.gather(f0, 1, where)).all() and (i64(p1) == i64(torch.gather(p0, 1, where))).all() and (i64(n0) == i64(n1)).all()
    f2, _, _ = A.sample_batch_flat(lay.view, batch, uniforms=torch.from_numpy(u).to(DEV))
    assert (f2[:, :25] == f2[:, 40:65]).all() and (f2[:, 65:] == f2[:, 5:6]).all()
    strided = torch.from_numpy(u).to(DEV).t().contiguous().t()               # column-major uniforms: the same values, other strides
    assert not strided.is_contiguous() and (A.sample_batch_flat(lay.view, batch, uniforms=strided)[0] == f2).all()
    # uniforms=None: the generator decides, and repeats
    draws = [A.sample_batch_flat(lay.view, batch, 9, generator=torch.Generator(device=DEV).manual_seed(3)) for _ in range(2)]
    assert draws[0][0].shape == (B, 9) and (draws[0][0] == draws[1][0]).all() and (i64(draws[0][1]) == i64(draws[1][1])).all()
    want = torch.rand((B, 9), dtype=torch.float64, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3))
    assert (A.sample_batch_flat(lay.view, batch, uniforms=want)[0] == draws[0][0]).all()
    # S = 0
    idx, prob = A.sample_batch(lay.view, batch, 0)
    assert idx.shape == (B, 0, lay.view.dim()) and prob.shape == (B, 0) and idx.dtype == torch.int64 and prob.dtype == torch.float64
    flat, prob, norms = A.sample_batch_flat(lay.view, batch, uniforms=torch.empty((B, 0), dtype=torch.float64, device=DEV))
    assert flat.shape == prob.shape == (B, 0) and norms.shape == (B,)


# ---- 6. repeatability and graph replay ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,fields", [(7, [(5, 2)]), (11, [(6, 2)])], ids=["small", "tiled"])
def test_two_runs_and_a_graph_replay_are_bit_identical(M, fields):
    n_bits = M + sum(w for _, w in fields)
    dims, batch, _ = layout(n_bits, fields)
    B, S = 2 ** (n_bits - M), 50
    lay = Lay("c64", crand(np.random.default_rng(0), 2 ** n_bits, "c64"), dims)
    u = torch.empty((B, S), dtype=torch.float64, device=DEV)

    def contents(r):
        rng = np.random.default_rng(10 + r)
        return [crand(rng, lay.logical.shape, "c64"), rng.random((B, S))]

    def op(amps, uniforms):
        return A.sample_batch_flat(amps, batch, uniforms=uniforms)

    def verify(r, hosts, after, outs):
        assert GB.same_bits(after[0], hosts[0]) and GB.same_bits(after[1], hosts[1])
        again = op(lay.view, u)
        for x, y in zip(again, outs):                                         # a second eager run on the statics themselves
            assert GB.same_bits(x.cpu().numpy(), y)
        assert (outs[0] >= 0).all() and (outs[1] > 0).all()

    capture_and_replay(op, [lay.view, u], contents, verify, replays=2)


# ---- 7. inside guard bands, at the library entry --------------------------------------------------------------------------------------
def library_call(view, batch, us, out_index, out_prob, out_norm, ws, ws_bytes):
    b = np.array(batch, dtype=np.int32)
    d = _desc(view.shape, view.stride(), view.dtype)
    N.check(N.lib().artn_sample_batch(ctypes.byref(d), view.data_ptr(), b.shape[0], b.ctypes.data_as(ctypes.c_void_p), us.data_ptr(),
                                      us.shape[1], out_index.data_ptr(), out_prob.data_ptr(), out_norm.data_ptr(), ws.data_ptr(), ws_bytes,
                                      N.current_stream_ptr(view.device)))
    torch.cuda.synchronize()


@pytest.mark.parametrize("kind,M,fields", [("c64", 6, [(4, 2), (8, 1)]), ("c128", 11, [(5, 1), (12, 1)])], ids=["small", "tiled"])
def test_inside_guard_bands_nothing_else_is_touched(kind, M, fields):
    n_bits = M + sum(w for _, w in fields)
    rng = np.random.default_rng(M)
    dims, batch, _ = layout(n_bits, fields)
    B, S = 2 ** (n_bits - M), 37
    plain = Lay(kind, crand(rng, 2 ** n_bits, kind), dims)
    shape, strides, np_dtype = tuple(plain.view.shape), tuple(plain.view.stride()), KINDS[kind][0]
    info = A.sample_batch_info(shape, strides, batch, S, plain.view.dtype)
    us_host = np.sort(rng.random((B, S)), axis=1)
    words = max(info["workspace_bytes"] // 8, 1)
    # the plain call
    us = torch.from_numpy(us_host).to(DEV)
    outs = [torch.empty((B, S), dtype=torch.int64, device=DEV), torch.empty((B, S), dtype=torch.float64, device=DEV),
            torch.empty(B, dtype=torch.float64, device=DEV)]
    library_call(plain.view, batch, us, *outs, torch.empty(words, dtype=torch.float64, device=DEV), info["workspace_bytes"])
    assert (outs[0] >= 0).all()
    # the banded call: the state at a 16-byte storage offset, the uniforms, the three outputs and the workspace, each in bands
    offset = GB.offsets_of(np_dtype)[1]
    mem = plain.base.reshape(-1).cpu().numpy()
    s_store, (s_view,), s_lay = GB.banded([mem], shape, strides, np_dtype, offset=offset, device=DEV)
    assert s_view.data_ptr() % 16 == 0 and s_view.data_ptr() % 32 != 0
    made = {}
    for name, host in (("us", us_host), ("index", np.zeros((B, S), dtype=np.int64)), ("prob", np.zeros((B, S))), ("norm", np.zeros(B)),
                       ("ws", np.zeros(words))):
        store, (view,), lay = GB.banded([host.reshape(-1)], host.shape, tuple(int(s) // host.itemsize for s in host.strides), host.dtype, device=DEV)
        made[name] = (store, view, lay)
    library_call(s_view, batch, made["us"][1], made["index"][1], made["prob"][1], made["norm"][1], made["ws"][1], info["workspace_bytes"])
    GB.assert_bands_intact(s_store, s_lay, "state")
    for name, (store, view, lay) in made.items():
        GB.assert_bands_intact(store, lay, name)
    assert GB.same_bits(GB.states_of(s_store, s_lay)[0], mem) and GB.same_bits(made["us"][1].cpu().numpy(), us_host)
    for got, want in zip((made["index"][1], made["prob"][1], made["norm"][1]), outs):
        assert GB.same_bits(got.cpu().numpy(), want.cpu().numpy())
