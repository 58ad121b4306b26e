"""The sparse-state compiler on arbitrary bitstring sets, executed by the oracle: for any set S of n12 bitstrings,
contraction_scheme_sparse(tree, S, sc_target) run on the pattern's leaves must give state_vec at the distinct strings of
S, in the row order the compiler returns -- the reference's own state vector of all 2^12 amplitudes
(tests/golden/n12_dense.npz).

Bound: the project's 1e-5 contract on amp_rel with the rms floor 2^-6.  Measured (worst over every set, both label
forms, scientific_notation off and on), per sc_target:
    31: 4.3e-6   30: 4.3e-6   12: 4.3e-6   10: 5.0e-6   8: 5.0e-6   6: 5.0e-6   5: 5.0e-6

sc_target 10, 8, 6 and 5 reach the chunked branch.  There the reference's chunk split leaves rows out of most schemes
(helpers.rows_left_out; contraction_scheme_sparse's docstring has the arithmetic), and the reference's executor cannot
run them: those (set, sc_target) pairs are kept as the named refusal REFERENCE_CHUNKS_LEAVE_ROWS_OUT, and the same pair
compiled with chunking="cover" must meet the bound like every other."""
import numpy as np
import pytest

from artensor_amd import contraction as C
from helpers import (AMP_RMS, SC_CHUNKED, SC_TARGETS, bitstring_sets, compile_n12_sparse, n12_sparse_pattern,
                     oracle_sparse, rows_left_out)
from test_gpu_parity import amp_rel

SETS = bitstring_sets()
worst = {}


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    print("\nworst amp_rel against state_vec per sc_target (oracle): "
          + "  ".join("%d: %.2e" % (sc, worst[sc]) for sc in SC_TARGETS if sc in worst))


def check(scheme, order, bitstrings, sc):
    state = n12_sparse_pattern()[2]
    # the distinct strings of S, each once, in the order of the output rows (the reference's order is that of its row
    # bookkeeping, not the lexicographic one: trees.json's own bitstrings_sorted is not sorted); the amplitudes below pin
    # which row is which
    assert sorted(order) == sorted(set(bitstrings))
    want = state[[int(b, 2) for b in order]]
    for scinot in (False, True):
        out, factor = oracle_sparse(scheme, scientific_notation=scinot)
        assert out.shape == (len(order),)
        if scinot:
            out = out.astype(np.complex128) * 10.0 ** factor
        err = amp_rel(out, want, rms=AMP_RMS)
        worst[sc] = max(worst.get(sc, 0.0), err)
        assert err <= 1e-5, (err, scinot)


def same_lists(a, b):
    return len(a) == len(b) and all(
        len(x[2][s]) == len(y[2][s]) and all(np.array_equal(p, q) for p, q in zip(x[2][s], y[2][s]))
        for x, y in zip(a, b) for s in (0, 1))


@pytest.mark.parametrize("sc", SC_TARGETS)
@pytest.mark.parametrize("name", list(SETS))
def test_compiled_scheme_gives_the_state_vector_at_the_bitstrings(name, sc):
    bitstrings = SETS[name]
    for labels in ("einsum", "tuples"):
        scheme, _, order = compile_n12_sparse(bitstrings, sc, labels=labels)
        refused = rows_left_out(scheme)
        if not refused:
            check(scheme, order, bitstrings, sc)
        else:
            # REFERENCE_CHUNKS_LEAVE_ROWS_OUT: no full answer from the reference's executor (IndexError at the next row
            # index past the short result, or fewer amplitudes than bitstrings), and this package's executor says why
            assert sc in SC_CHUNKED
            assert sorted(order) == sorted(set(bitstrings))
            try:
                out, _ = oracle_sparse(scheme)
            except IndexError:
                pass
            else:
                assert out.size < len(order)
            with pytest.raises(RuntimeError, match="chunks of step %d " % refused[0][0]):
                C._check_chunks(scheme)
        if sc in SC_CHUNKED:
            cover, _, order_c = compile_n12_sparse(bitstrings, sc, labels=labels, chunking="cover")
            assert not rows_left_out(cover) and list(order_c) == list(order)
            C._check_chunks(cover)
            if refused:
                check(cover, order_c, bitstrings, sc)
            else:   # wherever the reference's chunks hold every row, "cover" emits the same lists
                assert same_lists(cover, scheme)


@pytest.mark.parametrize("name", ["n12_sparse_chunked", "n12_sparse_chunked6"])
def test_the_chunked_fixture_recipes_execute(name):
    """The chunked recipes of trees.json (40 bitstrings at sc_target 8 and 6): field for field the reference's schemes
    (test_sparse_scheme_matches_reference), which leave rows out; with chunking="cover" they run and give the state vector."""
    import json
    import os
    from helpers import GOLDEN, Tree
    import artensor_amd as A
    with open(os.path.join(GOLDEN, "trees.json")) as f:
        rec = json.load(f)[name]
    scheme = A.contraction_scheme_sparse(Tree(rec["tree"]), rec["bitstrings"], sc_target=rec["sc_target"])[0]
    assert rows_left_out(scheme)
    cover, _, order = A.contraction_scheme_sparse(Tree(rec["tree"]), rec["bitstrings"], sc_target=rec["sc_target"],
                                                  chunking="cover")
    assert list(order) == rec["bitstrings_sorted"]
    check(cover, order, rec["bitstrings"], rec["sc_target"])


def test_chunking_keyword_is_checked():
    with pytest.raises(RuntimeError, match="chunking"):
        compile_n12_sparse(SETS["rand5"], 8, chunking="all")
