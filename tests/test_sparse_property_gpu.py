"""The sparse-state executor on arbitrary bitstring sets (the device side of test_sparse_property_cpu): the n12 pattern
compiled for every set of helpers.bitstring_sets() at every sc_target, run by A.tensor_contraction_sparse, against the
oracle on the same scheme and against the reference's state vector.  Which branch a step takes -- identity select, single
row, row pairs, chain cut, chunk loop, small-step program -- and what the identity-keyed caches hold depends on the set.

Bounds: complex64  amp_rel(hip, oracle) <= 1e-5 and amp_rel(hip, state) <= 1e-5 + amp_rel(oracle, state), rms floor 2^-6
        complex128 max|hip - oracle128| <= 1e-11 max|oracle128|
        the oracle itself, on the very scheme object the device ran: amp_rel(oracle, state) <= 1e-5 -- without it a scheme
        that is wrong (a bad row index, rows in another order than bitstrings_sorted says) is wrong in the oracle too, the
        slack above grows by the same error, and nothing here would notice
Chunked sc_targets run the scheme compiled with chunking="cover"; the reference's own split is run too where it holds
every row and must be refused by name, before any launch, where it does not (REFERENCE_CHUNKS_LEAVE_ROWS_OUT).

Measured worst amp_rel(hip, state) on an MI355X: 3.4e-6 at every sc_target (the oracle's own: 3.4e-6 to 3.5e-6).

A scheme object goes through complex64 first and complex128 after: the small-step program memo once replayed the
complex64 program on complex128 leaves (its key lacked the dtype)."""
import collections

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import contraction as C
from helpers import (AMP_RMS, SC_CHUNKED, SC_TARGETS, bitstring_sets, compile_n12_sparse, n12_sparse_pattern,
                     oracle_sparse, other_set_of_the_same_size, rows_left_out)
from test_gpu_parity import DEV, _CountingProfiler, amp_rel

pytestmark = pytest.mark.gpu
SETS = bitstring_sets()
ARMS = ({"ARTN_CHAIN_PLAN": "0"}, {"ARTN_ROW_PAIRS": "0"}, {"ARTN_CHAIN_PLAN": "0", "ARTN_ROW_PAIRS": "0"})
kernels = {sc: collections.Counter() for sc in SC_TARGETS}
worst = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst amp_rel against state_vec per sc_target (HIP): "
          + "  ".join("%d: %.2e" % (sc, worst[sc]) for sc in SC_TARGETS if sc in worst))
    print("launches per info['kernel'], per sc_target (default switches, complex64):")
    for sc in SC_TARGETS:
        print("  sc %2d: %s" % (sc, dict(sorted(kernels[sc].items()))))


def leaves(dtype=None):
    return n12_sparse_pattern()[1].fresh_tensors(dtype=dtype, device=DEV)


def clear_plans():
    for cache in (C._schedule_cache, C._chain_cache, C._left_cache, C._pair_rows_cache, C._pair_cache):
        cache.clear()


def wanted(order):
    return n12_sparse_pattern()[2][[int(b, 2) for b in order]]


def check64(got, ora, want, sc=None):
    got = got.cpu().numpy().reshape(-1)
    assert got.shape == want.shape
    e_ora, e_state, slack = amp_rel(got, ora, rms=AMP_RMS), amp_rel(got, want, rms=AMP_RMS), amp_rel(ora, want, rms=AMP_RMS)
    if sc is not None:
        worst[sc] = max(worst.get(sc, 0.0), e_state)
    assert slack <= 1e-5, slack          # the scheme itself is right: the oracle on it gives the state vector
    assert e_ora <= 1e-5, e_ora
    assert e_state <= 1e-5 + slack, (e_state, slack)


def run_all_ways(scheme, tuples, order, bitstrings, sc, monkeypatch):
    assert sorted(order) == sorted(set(bitstrings))   # (row order: see test_sparse_property_cpu.check)
    want = wanted(order)
    ora, _ = oracle_sparse(scheme)
    # complex64, default switches; the kernels of its launches go into the module's histogram
    assert C.profiler is None
    C.profiler = prof = _CountingProfiler()
    try:
        out = A.tensor_contraction_sparse(leaves(), scheme)
    finally:
        C.profiler = None
    kernels[sc].update(info["kernel"] for info, _, _ in prof.rows)
    check64(out, ora, want, sc)
    check64(A.tensor_contraction_sparse(leaves(), tuples), ora, want, sc)
    # every arm of the executor's switches, plans made afresh
    for arm in ARMS:
        with monkeypatch.context() as m:
            for k, v in arm.items():
                m.setenv(k, v)
            clear_plans()
            check64(A.tensor_contraction_sparse(leaves(), scheme), ora, want, sc)
    clear_plans()
    # complex128 against the oracle on complex128 leaves
    ora128, _ = oracle_sparse(scheme, dtype=np.complex128)
    out128 = A.tensor_contraction_sparse(leaves(torch.complex128), scheme).cpu().numpy().reshape(-1)
    assert out128.dtype == np.complex128 and out128.shape == ora128.shape
    assert amp_rel(ora128, want, rms=AMP_RMS) <= 1e-5
    assert np.abs(out128 - ora128).max() <= 1e-11 * np.abs(ora128).max()
    # scientific notation: exponent and mantissa against the oracle's, their product against the state vector
    mant, factor = oracle_sparse(scheme, scientific_notation=True)
    f, m_hip = A.tensor_contraction_sparse(leaves(), scheme, scientific_notation=True)
    f, m_hip = f.cpu().item().real, m_hip.cpu().numpy().reshape(-1)
    assert abs(f - factor) < 1e-4
    assert amp_rel(m_hip, mant) <= 1e-5
    whole = lambda mantissa, exponent: mantissa.astype(np.complex128) * 10.0 ** exponent
    slack = amp_rel(whole(mant, factor), want, rms=AMP_RMS)
    assert slack <= 1e-5, slack
    assert amp_rel(whole(m_hip, f), want, rms=AMP_RMS) <= 1e-5 + slack


@pytest.mark.parametrize("sc", SC_TARGETS)
@pytest.mark.parametrize("name", list(SETS))
def test_executor_gives_the_state_vector_at_the_bitstrings(name, sc, monkeypatch):
    bitstrings = SETS[name]
    scheme, _, order = compile_n12_sparse(bitstrings, sc)
    if sc in SC_CHUNKED:
        if rows_left_out(scheme):
            # REFERENCE_CHUNKS_LEAVE_ROWS_OUT: refused on the host, before anything is launched
            with pytest.raises(RuntimeError, match="chunks of step"):
                A.tensor_contraction_sparse(leaves(), scheme)
            scheme, _, order = compile_n12_sparse(bitstrings, sc, chunking="cover")
    chunking = "cover" if sc in SC_CHUNKED else "reference"
    tuples = compile_n12_sparse(bitstrings, sc, labels="tuples", chunking=chunking)[0]
    run_all_ways(scheme, tuples, order, bitstrings, sc, monkeypatch)


@pytest.mark.parametrize("sc", SC_TARGETS)
@pytest.mark.parametrize("name", ["rand1", "rand7", "rand37", "rand1000", "msb6_shared", "duplicates", "fixture40"])
def test_caches_do_not_replay_another_set(name, sc):
    """What an identity-keyed memo gets wrong: the same scheme twice (bit for bit), then another set of the same size from
    the same tree (its own amplitudes, not a replay of the first set's rows), then the first scheme again."""
    chunking = "cover" if sc in SC_CHUNKED else "reference"
    first, _, order1 = compile_n12_sparse(SETS[name], sc, chunking=chunking)
    run1 = A.tensor_contraction_sparse(leaves(), first)
    assert torch.equal(A.tensor_contraction_sparse(leaves(), first), run1)
    other = other_set_of_the_same_size(name)
    assert len(other) == len(set(SETS[name])) and set(other) != set(SETS[name])
    second, _, order2 = compile_n12_sparse(other, sc, chunking=chunking)
    assert sorted(order2) == sorted(other)
    check64(A.tensor_contraction_sparse(leaves(), second), oracle_sparse(second)[0], wanted(order2))
    assert torch.equal(A.tensor_contraction_sparse(leaves(), first), run1)
    check64(run1, oracle_sparse(first)[0], wanted(order1))
