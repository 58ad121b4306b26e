"""trajectories.pauli_expectation_batch on the device.  Where a trajectory has at least 2^10 elements and B * T <= 2048, row b is
bit for bit what pauli_expectation gives on a dense clone of slice b with its dims in local-bit order; a row does not depend on
where the batch bits lie; trajectories below one tile (several per workgroup) equal the integer oracle exactly on Gaussian-integer
states and stay within the derived bound of tests/test_pauli_gpu.py on random ones -- |got - want| <= 4 m 2^-53 norm_b with
m = 2^M elements per trajectory, twice that (norm 1) for normalised values; a poisoned trajectory leaves every other row and the
state as they were; runs and graph replays repeat bit for bit.  At most 2^16 elements per case except the one C < T case.

Strings are written by LOCAL bit: local bit j is the j-th lowest memory bit that is no batch bit."""
import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import pauli

import pauli_batch_oracle as PO
import trajectories_oracle as TO
from test_trajectories_gpu import KINDS, crand, poison, spread

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def tol(m):
    return 4 * m * 2.0 ** -53


class Lay:
    """A tensor whose logical dim d holds the memory bits lo .. lo + width - 1 of dims[d] = (lo, width); `logical` is the host
    image in dim order, `view` the GPU tensor; offset: elements in front of it in its storage."""

    def __init__(self, kind, flat, dims, offset=0):
        self.kind, self.dims = kind, list(dims)
        nd = len(dims)
        order = sorted(range(nd), key=lambda d: -dims[d][0])                  # memory dims, the highest bits first
        assert sum(w for _, w in dims) == int(flat.size).bit_length() - 1
        perm = [order.index(d) for d in range(nd)]
        store = torch.empty(flat.size + offset, dtype=KINDS[kind][1], device=DEV)
        store[offset:] = torch.from_numpy(np.ascontiguousarray(flat)).to(DEV)
        self.base = store[offset:].view([2 ** dims[d][1] for d in order])
        self.view = self.base.permute(perm)
        self.logical = flat.reshape([2 ** dims[d][1] for d in order]).transpose(perm)
        assert self.view.data_ptr() == store.data_ptr() + offset * store.element_size()

    def memory_bits(self):
        return self.base.reshape(-1).cpu().numpy().view(KINDS[self.kind][2])


def layout(n_bits, batch_fields):
    """(dims, batch dims): one extent-2 dim per local bit in a scrambled logical order, one dim per batch field (lo, width), the
    batch dims listed most significant first = the order given."""
    taken = {b for lo, w in batch_fields for b in range(lo, lo + w)}
    local = [b for b in range(n_bits) if b not in taken]
    rng = np.random.default_rng(n_bits * 100 + len(taken))
    dims = [(int(b), 1) for b in rng.permutation(local)] + list(batch_fields)
    where = [int(p) for p in rng.permutation(len(dims))]                      # batch dims anywhere in the logical order
    placed = [dims[p] for p in where]
    batch = [placed.index(f) for f in batch_fields]
    return placed, batch, local


def by_local(dims, local, ops):
    """A string {dim: letter} from {local bit: letter}."""
    return {dims.index((local[j], 1)): c for j, c in ops.items()}


def strings_for(dims, local):
    M = len(local)
    top = M - 1
    L = lambda ops: by_local(dims, local, ops)                               # noqa: E731
    out = [
        L({0: "Z", 5: "Z", 9: "Z", top: "Z"}), L({j: "Z" for j in range(M)}), L({}),      # FORM 0
        L({0: "X"}), L({1: "X", 0: "Z"}), L({0: "X", 1: "X"}),                             # FORM 1 below bit 2: the thread's own piece
        L({2: "X"}), L({5: "X", 3: "Z"}), L({9: "X", 8: "Z"}), L({j: "X" for j in range(2, 10)}), L({0: "X", 7: "X", 9: "Z"}),
        L({top: "X"}), L({10: "X"}), L({top: "X", 3: "X", 0: "Z", 10: "Z"}), L({10: "X", 0: "X", 1: "X"}),   # FORM 2
        L({4: "Y"}), L({4: "Y", top: "Y"}), L({0: "Y", 4: "Y", top: "Y", 2: "Z"}), L({1: "Y", 2: "Y", 9: "Y", 10: "Y", 7: "X"}),   # n_y = 1, 2, 3, 4
    ]
    return out


def unbatched_rows(lay, strings, batch, local):
    """[B, n_terms + 1]: artn_pauli_expect's out for the same strings on a dense clone of every slice, its dims in local-bit order."""
    nd = lay.logical.ndim
    sl = TO.slices(lay.logical, batch)
    rest = [d for d in range(nd) if d not in batch]
    sub_dims = [(local.index(lay.dims[d][0]), lay.dims[d][1]) for d in rest]
    subs = [PO.slice_string(p, nd, batch) for p in strings]
    ops, _ = pauli.pauli_ops(subs, len(rest))
    rows = []
    for b in range(sl.shape[0]):
        order = sorted(range(len(rest)), key=lambda d: -sub_dims[d][0])
        flat = np.ascontiguousarray(sl[b].transpose(order)).reshape(-1)
        clone = Lay(lay.kind, flat, sub_dims)
        assert (clone.logical == sl[b]).all()
        rows.append(pauli._raw(clone.view, ops, "test"))
    return torch.stack(rows)


def assert_rows_equal_unbatched(lay, strings, batch, local):
    info = A.pauli_batch_info(lay.view.shape, lay.view.stride(), strings, batch, lay.view.dtype)
    T = max(1, 2 ** (info["local_bits"] - 10))
    assert info["local_bits"] >= 10 and info["B"] * T <= 2048 and info["chunks"] == T        # the guard of the exact regime
    vals, norms = A.pauli_expectation_batch(lay.view, strings, batch, normalize=False)
    assert vals.shape == (info["B"], len(strings)) and norms.shape == (info["B"],) and vals.dtype == norms.dtype == torch.float64
    want = unbatched_rows(lay, strings, batch, local)
    got = torch.cat([vals, norms[:, None]], dim=1)
    same = got.view(torch.int64) == want.view(torch.int64)
    assert same.all(), f"rows/terms that differ: {(~same).nonzero().tolist()[:8]}"
    return info


# ---- 1. bit for bit against the unbatched call ----------------------------------------------------------------------------------------
CASES_1 = [("c64", 14, [(13, 1), (12, 1)]), ("c64", 14, [(7, 1), (4, 1)]), ("c64", 14, [(5, 2), (13, 1)]), ("c128", 13, [(9, 1), (3, 1)])]


@pytest.mark.parametrize("kind,n_bits,fields", CASES_1, ids=lambda v: str(v).replace(" ", ""))
def test_rows_equal_the_unbatched_call_bit_for_bit(kind, n_bits, fields):
    rng = np.random.default_rng(n_bits)
    dims, batch, local = layout(n_bits, fields)
    lay = Lay(kind, crand(rng, 2 ** n_bits, kind), dims)
    before = lay.memory_bits()
    strings = strings_for(dims, local)
    info = assert_rows_equal_unbatched(lay, strings, batch, local)
    assert info["n_groups"] >= 12
    # 17 strings of one group: two passes
    M = len(local)
    zs = [by_local(dims, local, {j: "Z" for j in range(M) if rng.random() < 0.5}) for _ in range(17)]
    info = assert_rows_equal_unbatched(lay, zs, batch, local)
    assert (info["n_groups"], info["n_launches"]) == (1, 2)
    # three groups interleaved in the caller's order
    mixed = []
    for i in range(5):
        for x in ({}, {2: "X", 6: "X"}, {M - 1: "X", 0: "X"}):
            ops = dict(x)
            for j in range(M):
                if j in ops:
                    ops[j] = "Y" if rng.random() < 0.4 else "X"
                elif rng.random() < 0.4:
                    ops[j] = "Z"
            mixed.append(by_local(dims, local, ops))
    info = assert_rows_equal_unbatched(lay, mixed, batch, local)
    assert info["n_groups"] == 3 and info["group"] == [0, 1, 2] * 5
    # ... and the oracle, so that the unbatched call is not the only witness
    want, wn = PO.expect(lay.logical, strings, batch)
    vals, norms = A.pauli_expectation_batch(lay.view, strings, batch, normalize=False)
    assert (np.abs(vals.cpu().numpy() - want) <= tol(2 ** M) * wn[:, None]).all() and (np.abs(norms.cpu().numpy() - wn) <= tol(2 ** M) * wn).all()
    assert (lay.memory_bits() == before).all()


# ---- 2. layout independence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_bits,placements", [
    ("c64", 14, [[(13, 1), (12, 1)], [(7, 1), (4, 1)], [(9, 1), (13, 1)]]),
    ("c128", 13, [[(12, 1), (11, 1)], [(3, 1), (9, 1)]]),
    ("c64", 10, [[(6, 4)], [(4, 1), (6, 1), (8, 1), (9, 1)]]),                # M = 6: the small form
])
def test_a_row_does_not_depend_on_where_the_batch_bits_lie(kind, n_bits, placements):
    rng = np.random.default_rng(2)
    nb = sum(w for _, w in placements[0])
    M = n_bits - nb
    logical = crand(rng, (2 ** nb,) + (2,) * M, kind)                          # dim 0: the trajectory; dim 1 + j: local bit M - 1 - j
    ops = [{j: "Z" for j in range(0, M, 2)}, {0: "X", 1: "Z"}, {M - 1: "X"}, {2: "Y", M - 1: "Y", 1: "Z"}, {j: "X" for j in range(M)}]
    results = []
    for fields in placements:
        taken = sorted(b for lo, w in fields for b in range(lo, lo + w))
        local = [b for b in range(n_bits) if b not in taken]
        # the trajectory index split over the fields, the first listed the most significant
        widths = [w for _, w in fields]
        dims = list(fields) + [(local[M - 1 - j], 1) for j in range(M)]
        arr = logical.reshape([2 ** w for w in widths] + [2] * M)
        order = sorted(range(len(dims)), key=lambda d: -dims[d][0])
        lay = Lay(kind, np.ascontiguousarray(arr.transpose(order)).reshape(-1), dims)
        assert (lay.logical == arr).all()
        batch = list(range(len(fields)))
        strings = [by_local(dims, local, o) for o in ops]
        vals, norms = A.pauli_expectation_batch(lay.view, strings, batch, normalize=False)
        results.append(torch.cat([vals, norms[:, None]], dim=1).view(torch.int64).cpu())
    for r in results[1:]:
        assert torch.equal(r, results[0])


# ---- 3. one tile per trajectory ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_bits,fields,halved", [("c64", 14, [(6, 2), (12, 2)], False), ("c64", 14, [(5, 1), (9, 2)], True),
                                                       ("c128", 13, [(3, 3)], False)])
def test_one_tile_per_trajectory(kind, n_bits, fields, halved):
    rng = np.random.default_rng(3)
    dims, batch, local = layout(n_bits, fields)
    M = len(local)
    assert M == (11 if halved else 10)
    lay = Lay(kind, crand(rng, 2 ** n_bits, kind), dims)
    strings = strings_for(dims, local) if halved else [by_local(dims, local, o) for o in (
        {0: "Z", 9: "Z"}, {0: "X"}, {9: "X", 2: "Z"}, {3: "Y", 9: "Y"}, {j: "X" for j in range(10)}, {})]
    info = assert_rows_equal_unbatched(lay, strings, batch, local)
    assert info["chunks"] == (2 if halved else 1) and info["chunks_halved"] == 1 and info["B"] == (8 if halved or kind == "c128" else 16)
    if halved:
        assert max(info["local_xmask"]) >= 2 ** 10


# ---- 4. the small form --------------------------------------------------------------------------------------------------------------------
def small_strings(dims, local, rng):
    M = len(local)
    top = M - 1
    ops = [{}, {j: "Z" for j in range(M)}, {0: "Z", top: "Z"}, {0: "X"}, {1: "X", 0: "Z"}, {0: "X", 1: "X"}, {top: "X"}, {top: "Y"},
           {0: "Y", top: "Y"}, {0: "Y", 1: "Y", 2: "Y"}, {j: "Y" for j in range(M)}, {2: "X", 1: "Z"}, {j: "X" for j in range(M)}]
    ops += [{j: "Z" for j in range(M) if rng.random() < 0.5} for _ in range(18)]          # a group of more than 16: two passes
    return [by_local(dims, local, o) for o in ops]


SMALL = [("c64", 10, [(4, 6)]), ("c64", 10, [(9, 1), (6, 1), (4, 1)]), ("c64", 10, [(6, 1)]), ("c64", 6, [(4, 2)]), ("c128", 6, [(3, 3)])]


@pytest.mark.parametrize("kind,n_bits,fields", SMALL, ids=lambda v: str(v).replace(" ", ""))
def test_trajectories_below_one_tile(kind, n_bits, fields):
    rng = np.random.default_rng(40 + n_bits)
    dims, batch, local = layout(n_bits, fields)
    M = len(local)
    strings = small_strings(dims, local, rng)
    info = A.pauli_batch_info([2 ** w for _, w in dims], [2 ** lo for lo, _ in dims], strings, batch, KINDS[kind][1])
    assert info["local_bits"] == M < 10 and info["tile_bits"] == M and info["chunks"] == 1 and info["B"] == 2 ** (n_bits - M)
    assert info["n_launches"] > info["n_groups"] and PO.exact_bound(M, 2 ** 10) < 2 ** 53
    # exact integers: equal to the integer oracle, whatever the order of the sums
    lay = Lay(kind, PO.exact_state(rng, 2 ** n_bits, kind), dims)
    before = lay.memory_bits()
    vals, norms = A.pauli_expectation_batch(lay.view, strings, batch, normalize=False)
    want, wn = PO.exact_expect(lay.logical, strings, batch)
    assert (vals.cpu().numpy() == want).all() and (norms.cpu().numpy() == wn).all()
    assert (lay.memory_bits() == before).all()
    # random states: the derived bound
    lay = Lay(kind, crand(rng, 2 ** n_bits, kind), dims)
    want, wn = PO.expect(lay.logical, strings, batch)
    vals, norms = A.pauli_expectation_batch(lay.view, strings, batch, normalize=False)
    err = np.abs(vals.cpu().numpy() - want) / wn[:, None]
    print(f"{kind} M={M} B={info['B']}: raw err / norm {err.max():.3e} (bound {tol(2 ** M):.3e})")
    assert (err <= tol(2 ** M)).all() and (np.abs(norms.cpu().numpy() - wn) <= tol(2 ** M) * wn).all()
    nvals, nn = A.pauli_expectation_batch(lay.view, strings, batch)
    assert torch.equal(nn, norms) and (np.abs(nvals.cpu().numpy() - want / wn[:, None]) <= 2 * tol(2 ** M)).all()
    one, _ = A.pauli_expectation_batch(lay.view, strings[4], batch, normalize=False)
    assert one.shape == (info["B"],) and torch.equal(one, vals[:, 4])


# ---- 5. isolation ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("n_bits,fields", [(14, [(8, 1), (13, 1)]), (10, [(5, 2), (8, 2)])], ids=["M12", "M6"])
def test_a_poisoned_trajectory_stays_in_its_row(kind, n_bits, fields):
    rng = np.random.default_rng(5)
    dims, batch, local = layout(n_bits, fields)
    M = len(local)
    strings = strings_for(dims, local) if M >= 11 else small_strings(dims, local, rng)
    clean = Lay(kind, crand(rng, 2 ** n_bits, kind), dims)
    B = TO.batch_size(clean.logical.shape, batch)
    cv, cn = A.pauli_expectation_batch(clean.view, strings, batch, normalize=False)
    for bad in (0, B - 1, B // 2):
        sl = TO.slices(clean.logical, batch)
        sl[bad] = poison(rng, sl[bad].shape, kind)
        logical = TO.unslice(sl, clean.logical.shape, batch)
        order = sorted(range(len(dims)), key=lambda d: -dims[d][0])
        lay = Lay(kind, np.ascontiguousarray(logical.transpose(order)).reshape(-1), dims)
        before = lay.memory_bits()
        for normalize in (False, True):
            vals, norms = A.pauli_expectation_batch(lay.view, strings, batch, normalize=normalize)
            assert (lay.memory_bits() == before).all()
            keep = torch.arange(B, device=DEV) != bad
            want = cv / cn[:, None] if normalize else cv
            assert torch.equal(vals[keep].view(torch.int64), want[keep].view(torch.int64))
            assert torch.equal(norms[keep].view(torch.int64), cn[keep].view(torch.int64))
        assert not torch.isfinite(norms[bad])


# ---- 6. C < T -----------------------------------------------------------------------------------------------------------------------------
def test_chunks_of_several_tiles():
    """The smallest shape with C < T: 2^22 complex64 elements, B = 8, M = 19 -- 512 local tiles in 256 chunks."""
    rng = np.random.default_rng(6)
    n_bits, fields = 22, [(21, 1), (12, 1), (5, 1)]
    dims, batch, local = layout(n_bits, fields)
    M = len(local)
    strings = [by_local(dims, local, o) for o in ({j: "Z" for j in range(0, M, 3)}, {0: "X", 12: "Z"}, {M - 1: "X", 11: "Z"},
                                                  {10: "Y", M - 1: "Y", 3: "X"}, {6: "Y", 18: "Z"})]
    info = A.pauli_batch_info([2 ** w for _, w in dims], [2 ** lo for lo, _ in dims], strings, batch)
    assert (info["B"], info["local_bits"], info["chunks"], info["chunks_halved"]) == (8, 19, 256, 256) and info["chunks"] < 2 ** (M - 10) == 512
    assert PO.exact_bound(M, 2 ** 4) < 2 ** 53
    lay = Lay("c64", PO.exact_state(rng, 2 ** n_bits, "c64", bound=2 ** 4), dims)
    vals, norms = A.pauli_expectation_batch(lay.view, strings, batch, normalize=False)
    want, wn = PO.exact_expect(lay.logical, strings, batch)
    assert (vals.cpu().numpy() == want).all() and (norms.cpu().numpy() == wn).all()
    lay = Lay("c64", crand(rng, 2 ** n_bits, "c64"), dims)
    vals, norms = A.pauli_expectation_batch(lay.view, strings, batch, normalize=False)
    want, wn = PO.expect(lay.logical, strings, batch)
    err = np.abs(vals.cpu().numpy() - want) / wn[:, None]
    print(f"M=19 B=8: raw err / norm {err.max():.3e} (bound {tol(2 ** M):.3e})")
    assert (err <= tol(2 ** M)).all() and (np.abs(norms.cpu().numpy() - wn) <= tol(2 ** M) * wn).all()


# ---- 7. batch_dims=() -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["c64", "c128"])
@pytest.mark.parametrize("nq", [4, 12])
def test_no_batch_dims_is_the_unbatched_call(nq, kind):
    rng = np.random.default_rng(70 + nq)
    dims, batch, local = layout(nq, [])
    lay = Lay(kind, crand(rng, 2 ** nq, kind), dims)
    ops = [{}, {0: "Z", nq - 1: "Z"}, {0: "X"}, {1: "X", 0: "Z"}, {nq - 1: "X"}, {2: "Y"}, {0: "Y", nq - 1: "Y"}, {j: "Y" for j in range(nq)}]
    ops += [{j: "Z" for j in range(nq) if rng.random() < 0.5} for _ in range(17)]
    strings = [by_local(dims, local, o) for o in ops]
    vals, norms = A.pauli_expectation_batch(lay.view, strings, (), normalize=False)
    assert vals.shape == (1, len(strings)) and norms.shape == (1,)
    assert torch.equal(vals[0].view(torch.int64), A.pauli_expectation(lay.view, strings, normalize=False, device=True).view(torch.int64))
    raw = pauli._raw(lay.view, pauli.pauli_ops(strings, nq)[0], "test")
    assert torch.equal(norms[0].view(torch.int64), raw[-1].view(torch.int64))
    terms = [(float(c), p) for c, p in zip(rng.standard_normal(len(strings)), strings)]
    E, _ = A.pauli_sum_expectation_batch(lay.view, terms, ())
    want = A.pauli_sum_expectation(lay.view, terms)
    assert E.shape == (1,) and abs(float(E[0]) - want) <= 1e-13 * sum(abs(c) for c, _ in terms)


# ---- 8. determinism and capture -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n_bits,fields", [("c64", 14, [(11, 2)]), ("c128", 10, [(4, 1), (7, 2)])], ids=["tiled", "small"])
@pytest.mark.parametrize("offset_bytes", [16, 80])
def test_runs_and_graph_replays_repeat_bit_for_bit(kind, n_bits, fields, offset_bytes):
    rng = np.random.default_rng(8)
    dims, batch, local = layout(n_bits, fields)
    lay = Lay(kind, crand(rng, 2 ** n_bits, kind), dims, offset=offset_bytes // (8 if kind == "c64" else 16))
    assert lay.view.data_ptr() % 16 == 0 and lay.view.storage_offset() * lay.view.element_size() == offset_bytes
    strings = strings_for(dims, local) if len(local) >= 11 else small_strings(dims, local, rng)

    def run():
        vals, norms = A.pauli_expectation_batch(lay.view, strings, batch, normalize=False)
        return torch.cat([vals, norms[:, None]], dim=1)

    first, second = run(), run()
    assert torch.equal(first.view(torch.int64), second.view(torch.int64))
    want, wn = PO.expect(lay.logical, strings, batch)
    assert (np.abs(first[:, :-1].cpu().numpy() - want) <= tol(2 ** len(local)) * wn[:, None]).all()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for _ in range(2):
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured.view(torch.int64), first.view(torch.int64))


# ---- 9. end to end ------------------------------------------------------------------------------------------------------------------------------
def test_phase_flip_trajectories_follow_the_channel():
    """B = 256 copies of |+>^3 |0> (the fourth qubit is a spectator: M = 4), a phase flip with p = 1/4 on qubit 1 per trajectory:
    <X_1> is +1 where I was drawn and -1 where Z was, so the mean over trajectories is 1 - 2 count / B."""
    B, bound = 256, 2 * 4 * 2 ** 4 * 2.0 ** -53
    for renormalize in (True, False):
        host = np.zeros((B, 2, 2, 2, 2), dtype=np.complex64)
        host[..., 0] = 1 / np.sqrt(8)
        amps = torch.from_numpy(host).to(DEV)
        op = A.BatchChannelOp(amps.shape, amps.stride(), amps.dtype, A.phase_flip(0.25), (1,), (0,), DEV)
        j, _ = op(amps, uniforms=spread(B), renormalize=renormalize)
        count = int((j == 1).sum())
        assert 0 < count < B
        if renormalize:
            x, norms = A.pauli_expectation_batch(amps, {1: "X"}, (0,))
            mean, err = A.trajectory_mean(x)
        else:
            x, norms = A.pauli_expectation_batch(amps, {1: "X"}, (0,))
            mean, err = A.trajectory_mean(x, norms)
        assert x.shape == (B,) and (torch.abs(torch.abs(x) - 1.0) <= bound).all() and torch.equal(x < 0, j == 1)
        assert abs(float(mean) - (1 - 2 * count / B)) <= bound and float(err) > 0
        E, _ = A.pauli_sum_expectation_batch(amps, [(0.5, {1: "X"}), (2.0, {2: "X"})], (0,))
        assert (torch.abs(E - (0.5 * x + 2.0)) <= 3 * bound).all()
