"""Host-side checks of bitstring sampling per trajectory (artensor_amd/trajectories.py: sample_batch, sample_batch_flat,
sample_batch_info; artn_sample_batch_query / artn_sample_batch): the symbols, the numpy oracle of sample_batch_oracle.py against
np.cumsum / np.searchsorted on Gaussian-integer states (every sum exact, so the expected index does not depend on the order of
additions), its index deposit against a brute-force address table, the plan against hand-computed ones, every refusal by name.
No GPU needed: artn_sample_batch checks every argument before it looks for a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import born
from artensor_amd import trajectories as T

import sample_batch_oracle as SO
import trajectories_oracle as TO
from test_pauli_apply_cpu import contiguous_strides, desc, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2
NAMES = ("sample_batch", "sample_batch_flat", "sample_batch_info")
VALUES = np.array([0, 1, -1, 1j, -1j, 1 + 1j, 1 - 1j, -1 + 1j, -1 - 1j, 2, -2], dtype=np.complex128)


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_sample_batch_query", "artn_sample_batch"]
    text = open(os.path.join(ROOT, "include", "artn.h")).read()
    assert "#define ARTN_ABI_VERSION 9" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    assert ctypes.sizeof(N.ArtnSampleBatchInfo) == 10 * 4 + 5 * 8 + 3 * 4 * N.BATCH_MAX_FIELDS
    body = re.search(r"typedef struct ArtnSampleBatchInfo \{(.*?)\} ArtnSampleBatchInfo;", text, flags=re.S).group(1)
    fields = [f.strip().split("[")[0] for line in body.split(";") if line.strip()
              for f in re.sub(r"^\s*\w+\s+", "", line.strip()).split(",")]
    assert fields == [name for name, _ in N.ArtnSampleBatchInfo._fields_]


def test_the_names_live_in_trajectories_not_in_born():
    for name in NAMES:
        assert getattr(A, name) is getattr(T, name) and name in T.__all__
    assert not set(NAMES) & set(born.__all__)


# ---- the oracle against cumsum / searchsorted -----------------------------------------------------------------------------------------
def integer_state(rng, n_bits, fields, dtype):
    """A Gaussian-integer MEMORY-order array with many zeros: whole zero segments everywhere, whole zero blocks where a trajectory
    has several; with four or more trajectories, trajectory 0 has all weight on its first element and the last one on its last."""
    table = SO.address_table(n_bits, fields)
    B, m = table.shape
    mem = np.zeros(1 << n_bits, dtype=dtype)
    for b in range(B):
        row = VALUES[rng.integers(0, VALUES.size, size=m)]
        row[rng.random(m) < 0.5] = 0
        seg = row.reshape(-1, 4)
        seg[rng.random(seg.shape[0]) < 0.3] = 0                               # whole zero segments
        if m >= 4096:
            blk = row.reshape(-1, 1024)
            blk[1:3] = 0                                                       # two whole zero blocks after the first
            blk[3, :] = 0
            blk[3, 77] = 1 + 1j                                                # one element in an otherwise zero block
        if b == 0 and B >= 4:
            row[:] = 0
            row[0] = 2
        if b == B - 1 and B >= 4:
            row[:] = 0
            row[-1] = -1j
        mem[table[b]] = row
    return mem, table


def exact_uniforms(cs):
    """Uniforms for the cumulative integer sums cs of one trajectory, and the local index each must give: mid-element targets
    (k + 0.5) / total, targets exactly on a prefix boundary (kept where c / total * total == c in float64), 0.0 and
    nextafter(1, 0)."""
    total = cs[-1]
    ks = np.unique(np.linspace(0, total - 1, 23).astype(np.int64)).astype(np.float64)
    us = [(k + 0.5) / total for k in ks]
    want = [int(np.searchsorted(cs, k + 0.5, side="right")) for k in ks]
    assert all(k < (u * total) < k + 1 for k, u in zip(ks, us))
    edges = [c for c in np.unique(cs)[:-1] if c > 0 and (c / total) * total == c][:6]
    us += [c / total for c in edges]
    want += [int(np.searchsorted(cs, c, side="right")) for c in edges]       # the next element that has weight
    nz = np.flatnonzero(np.diff(np.concatenate([[0.0], cs])) > 0)
    us += [0.0, np.nextafter(1.0, 0.0)]
    want += [int(nz[0]), int(nz[-1])]
    return np.array(us), np.array(want), len(edges)


LAYOUTS = [(8, [(4, 1, 0)]), (8, [(7, 1, 0)]), (11, [(5, 1, 1), (9, 1, 0)]), (12, [(4, 2, 0)]), (14, [(13, 1, 0)]), (14, [(6, 1, 0), (12, 1, 1)]),
           (9, []), (12, [])]


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=["c64", "c128"])
@pytest.mark.parametrize("n_bits,fields", LAYOUTS, ids=lambda v: str(v).replace(" ", ""))
def test_the_oracle_is_cumsum_and_searchsorted_on_integer_states(n_bits, fields, dtype):
    rng = np.random.default_rng(n_bits * 7 + len(fields))
    mem, table = integer_state(rng, n_bits, fields, dtype)
    B = table.shape[0]
    per_row = [exact_uniforms(np.cumsum(SO.terms(mem[table[b]]))) for b in range(B)]
    S = max(u.size for u, _, _ in per_row)
    keep = [np.r_[0:u.size, [0] * (S - u.size)].astype(np.int64) for u, _, _ in per_row]   # (equal lengths: the first one repeated)
    uniforms = np.stack([u[k] for (u, _, _), k in zip(per_row, keep)])
    want = np.stack([w[k] for (_, w, _), k in zip(per_row, keep)])
    flat, raw, norms = SO.sample_rows(mem, n_bits, fields, uniforms)
    for b in range(B):
        assert norms[b] == SO.terms(mem[table[b]]).sum()
        assert (flat[b] == table[b][want[b]]).all(), (b, flat[b], table[b][want[b]])
        assert (raw[b] == SO.terms(mem[flat[b]])).all() and (raw[b] > 0).all()       # never an element of probability zero
    assert sum(e for _, _, e in per_row) > 0                                    # some targets sat exactly on a prefix boundary
    # scattered uniforms come back to their own positions
    perm = rng.permutation(S)
    f2, r2, _ = SO.sample_rows(mem, n_bits, fields, uniforms[:, perm])
    assert (f2 == flat[:, perm]).all() and (r2 == raw[:, perm]).all()


def test_dead_trajectories_and_uniforms_outside_the_interval_in_the_oracle():
    mem = np.zeros(256, dtype=np.complex64)
    mem[32:64] = 1                                                             # trajectory 1 of (bit 5, bit 6) -> b = bit5 + 2 bit6 ...
    fields = [(5, 2, 0)]
    flat, raw, norms = SO.sample_rows(mem, 8, fields, np.array([[0.5, 1.5, -0.25]] * 4))
    f, p, _ = SO.finish(flat, raw, norms)
    assert norms.tolist() == [0.0, 32.0, 0.0, 0.0]
    assert (f[[0, 2, 3]] == -1).all() and np.isnan(p[[0, 2, 3]]).all()
    assert f[1].tolist() == [32 + 16, 63, -1] and p[1].tolist() == [1 / 32, 1 / 32, 0.0]


# ---- the deposit ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.complex64, torch.complex128], ids=["c64", "c128"])
def test_the_address_table_against_a_walk_over_every_multi_index(dtype):
    rng = np.random.default_rng(5)
    lb = 4 if dtype == torch.complex64 else 3
    for nd in (6, 8, 9):
        bit = [int(b) for b in rng.permutation(nd)]
        shape, strides = (2,) * nd, tuple(1 << b for b in bit)
        high = [b for b in range(nd) if b >= lb]
        for nbb in range(0, min(3, len(high)) + 1):
            batch = [bit.index(int(b)) for b in rng.choice(high, size=nbb, replace=False)]
            info = A.sample_batch_info(shape, strides, batch, 1, dtype)
            assert info["fields"] == TO.fields(shape, strides, batch)
            table = SO.address_table(nd, info["fields"])
            brute = TO.batch_index_brute(shape, strides, batch)
            assert table.shape == (info["B"], 1 << info["local_bits"])
            for b in range(info["B"]):
                assert table[b].tolist() == sorted(f for f, t in brute.items() if t == b)
            # ... and against the slices of a host array: slice b in local-bit order is the table's row
            mem = np.arange(1 << nd)
            logical = np.lib.stride_tricks.as_strided(mem, shape=shape, strides=tuple(s * mem.itemsize for s in strides))
            rest = [d for d in range(nd) if d not in batch]
            order = sorted(range(len(rest)), key=lambda i: -bit[rest[i]])
            sl = TO.slices(logical, batch)
            for b in range(info["B"]):
                assert (np.ascontiguousarray(sl[b].transpose(order)).reshape(-1) == table[b]).all()


# ---- the plan -------------------------------------------------------------------------------------------------------------------------
def test_sample_batch_info_against_hand_computed_plans():
    def plan(nd, batch, S, dtype=torch.complex64):
        shape = (2,) * nd
        return A.sample_batch_info(shape, contiguous_strides(shape), batch, S, dtype)   # dim d holds memory bit nd - 1 - d

    p = plan(8, [0], 5)                                                        # B = 2, M = 7: one launch, one virtual tile
    assert (p["form"], p["B"], p["local_bits"], p["block_bits"], p["blocks_per_trajectory"]) == ("SMALL", 2, 7, 10, 1)
    assert (p["launches"], p["grid"], p["workspace_bytes"], p["bytes_read_min"], p["fields"]) == (1, [1], 0, 256 * 8, [(7, 1, 0)])
    p = plan(20, list(range(12)), 1)                                           # B = 2^12, M = 8: 4 trajectories per workgroup
    assert (p["form"], p["grid"], p["batch_bits"], p["fields"]) == ("SMALL", [1024], 12, [(8, 12, 0)])
    p = plan(12, [0, 1], 3, torch.complex128)                                  # B = 4, M = 10: one block per trajectory
    assert (p["form"], p["launches"], p["grid"], p["workspace_bytes"], p["bytes_read_min"]) == ("TILED", 3, [4, 1, 4], 4 * 2 * 8, 4096 * 16)
    p = plan(30, list(range(10)), 1)                                           # 2^10 trajectories of 20 qubits
    assert (p["form"], p["block_bits"], p["blocks_per_trajectory"], p["grid"]) == ("TILED", 10, 1024, [1 << 20, 1024, 1 << 20])
    assert p["workspace_bytes"] == (1 << 20) * 16
    p = plan(22, [0], 1)                                                       # M = 21: 2^11 blocks, a workgroup per trajectory
    assert (p["block_bits"], p["blocks_per_trajectory"], p["grid"]) == (10, 2048, [4096, 2, 4096])
    p = plan(28, [0], 64)                                                      # M = 27: blocks of 2^11
    assert (p["block_bits"], p["blocks_per_trajectory"], p["grid"]) == (11, 1 << 16, [1 << 17, 2, 1 << 17])
    p = plan(32, [0], 1)                                                       # more units than the grid cap: workgroups loop
    assert (p["block_bits"], p["blocks_per_trajectory"], p["grid"][0]) == (14, 1 << 17, 1 << 18)
    p = plan(36, [0, 1], 1)
    assert (p["blocks_per_trajectory"], p["grid"]) == (1 << 20, [1 << 20, 4, 1 << 20])
    for nd in (0, 1, 5, 9, 10, 12):                                            # B = 1: the plan of the unbatched call
        p, q = plan(nd, [], 7), born.born_plan(1 << nd)
        assert (p["form"], p["B"], p["block_bits"], p["blocks_per_trajectory"]) == ("TILED", 1, q["block_bits"], q["n_blocks"])
    p = A.sample_batch_info((4, 2, 2, 4, 2), (1, 4, 8, 16, 64), [4, 3], 2)     # extents of 4; two dims that merge into one field
    assert (p["B"], p["local_bits"], p["fields"]) == (8, 4, [(4, 3, 0)])
    p = A.sample_batch_info((4, 2, 2, 4, 2), (1, 4, 8, 16, 64), [3, 4], 2)     # listed against memory: two fields
    assert p["fields"] == [(4, 2, 1), (6, 1, 0)]


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def call(shape, strides, batch, S=1, dtype=N.ARTN_C64, *, run=False, a=256, u=256, oi=256, op=256, on=256, ws=256, ws_bytes=None, nb=None):
    """(code, message) of artn_sample_batch_query, or of artn_sample_batch with made-up addresses (never dereferenced: every call
    here is refused before a device is looked for)."""
    b = np.array(list(batch), dtype=np.int32)
    d, info = desc(shape, strides, dtype), N.ArtnSampleBatchInfo()
    nb = b.shape[0] if nb is None else nb
    bp = ptr(b) if b.shape[0] else None
    if run:
        if ws_bytes is None:
            assert N.lib().artn_sample_batch_query(ctypes.byref(d), nb, bp, S, ctypes.byref(info)) == 0
            ws_bytes = info.workspace_bytes
        rc = N.lib().artn_sample_batch(ctypes.byref(d), a, nb, bp, u, S, oi, op, on, ws, ws_bytes, None)
    else:
        rc = N.lib().artn_sample_batch_query(ctypes.byref(d), nb, bp, S, ctypes.byref(info))
    return rc, (N.lib().artn_last_error() or b"").decode()


def refused(code, word, *args, **kw):
    rc, msg = call(*args, **kw)
    assert rc == code and word in msg, (rc, msg)


def test_every_refusal_of_the_library_has_its_code_and_its_text():
    nd = 12
    shape, strides = (2,) * nd, contiguous_strides((2,) * nd)                 # dim d holds memory bit 11 - d
    refused(INVALID, "not dense", shape, [2 * s for s in strides], [0])
    refused(INVALID, "out of range", shape, strides, [nd])
    refused(INVALID, "out of range", shape, strides, [-1])
    refused(INVALID, "repeated", shape, strides, [1, 1])
    refused(INVALID, "negative", shape, strides, [], nb=-1)
    refused(INVALID, "negative sample count", shape, strides, [0], -1)
    refused(INVALID, "workspace smaller", shape, strides, [0, 1], run=True, ws_bytes=8)
    for name in ("a", "u", "oi", "op", "on", "ws"):
        refused(INVALID, "null pointer", shape, strides, [0, 1], run=True, **{name: None})
    rc, _ = call(shape, strides, list(range(4)), run=True, ws=None, a=264)     # SMALL: no workspace, so none is asked for
    assert rc == UNSUPPORTED
    # a batch bit below the line (complex64: bit 4; complex128: bit 3)
    refused(UNSUPPORTED, "below a 128-byte line", shape, strides, [11])
    refused(UNSUPPORTED, "below a 128-byte line", shape, strides, [8])
    assert call(shape, strides, [8], 1, N.ARTN_C128)[0] == 0
    refused(UNSUPPORTED, "below a 128-byte line", shape, strides, [9], 1, N.ARTN_C128)
    # more than ARTN_BATCH_MAX_BITS batch bits
    big = (2,) * 30
    refused(UNSUPPORTED, "batch bits", big, contiguous_strides(big), list(range(25)))
    # B * S above 2^28
    refused(UNSUPPORTED, "2^28", big, contiguous_strides(big), list(range(24)), 17)
    assert call(big, contiguous_strides(big), list(range(24)), 16)[0] == 0
    refused(UNSUPPORTED, "2^28", shape, strides, [], (1 << 28) + 1)
    # alignment
    refused(UNSUPPORTED, "16-byte aligned", shape, strides, [0, 1], run=True, a=264)
    for name in ("u", "oi", "op", "on", "ws"):
        refused(UNSUPPORTED, "8-byte aligned", shape, strides, [0, 1], run=True, **{name: 260})
    # the layouts the family does not index by bits
    refused(UNSUPPORTED, "complex64 or complex128", shape, strides, [0], 1, 99)
    refused(UNSUPPORTED, "power-of-two", (3,) + (2,) * 10, contiguous_strides((3,) + (2,) * 10), [])
    refused(UNSUPPORTED, "2^40", (2,) * 41, contiguous_strides((2,) * 41), [])
    # S = 0: nothing to do, whatever the pointers
    assert call(shape, strides, [0, 1], 0, run=True, a=None, u=None, oi=None, op=None, on=None, ws=None)[0] == 0


def test_python_side_errors_by_name():
    nd = 12
    shape, strides = (2,) * nd, contiguous_strides((2,) * nd)
    info = A.sample_batch_info
    with pytest.raises(ValueError, match="below a 128-byte line"):
        info(shape, strides, [11], 1)
    with pytest.raises(ValueError, match="distinct dims"):
        info(shape, strides, [1, 1], 1)
    with pytest.raises(ValueError, match="distinct dims"):
        info(shape, strides, [nd], 1)
    with pytest.raises(ValueError, match="at most 24 batch bits"):
        info((2,) * 30, contiguous_strides((2,) * 30), list(range(25)), 1)
    with pytest.raises(ValueError, match=r"above 2\^28"):
        info((2,) * 30, contiguous_strides((2,) * 30), list(range(24)), 17)
    with pytest.raises(ValueError, match="power-of-two extents"):
        info((3,) + (2,) * 10, contiguous_strides((3,) + (2,) * 10), [], 1)
    with pytest.raises(ValueError, match="not dense"):
        info(shape, [2 * s for s in strides], [0], 1)
    with pytest.raises(ValueError, match=r"2\^40"):
        info((2,) * 41, contiguous_strides((2,) * 41), [], 1)
    with pytest.raises(ValueError, match="negative"):
        info(shape, strides, [0], -1)
    with pytest.raises(TypeError, match="complex64 or complex128"):
        info(shape, strides, [0], 1, torch.float32)
    # uniforms: dtype, shape and n_samples are checked on the host, before anything touches a device
    what, dev = "sample_batch", torch.device("cpu")
    with pytest.raises(ValueError, match="float64"):
        T._sample_uniforms(torch.zeros((4, 3), dtype=torch.float32), None, None, 4, dev, what)
    with pytest.raises(ValueError, match="float64"):
        T._sample_uniforms([[0.5]], None, None, 1, dev, what)
    for bad in (torch.zeros(12, dtype=torch.float64), torch.zeros((3, 4), dtype=torch.float64), torch.zeros((4, 3, 1), dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"shape \[B, S\]"):
            T._sample_uniforms(bad, None, None, 4, dev, what)
    with pytest.raises(ValueError, match="disagrees"):
        T._sample_uniforms(torch.zeros((4, 3), dtype=torch.float64), 5, None, 4, dev, what)
    with pytest.raises(ValueError, match="must live on"):
        T._sample_uniforms(torch.zeros((4, 3), dtype=torch.float64), 3, None, 4, dev, what)
    with pytest.raises(ValueError, match="give n_samples or uniforms"):
        T._sample_uniforms(None, None, None, 4, dev, what)
    assert T._sample_uniforms(None, 6, None, 4, dev, what) == (None, 6)
    cpu = torch.zeros(shape, dtype=torch.complex64)
    for f in (A.sample_batch, A.sample_batch_flat):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f(cpu, [0], 1)
