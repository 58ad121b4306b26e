"""Host-side checks of measurement (artensor_amd/measure.py; artn_measure_query / _choose / _collapse): the symbols and
constants, the query on contiguous and permuted layouts, every refusal, the choice rule of the numpy oracle
(tests/measure_oracle.py, the oracle of test_measure_gpu.py) and of the module's host restatement, and the argument errors of
all five public functions, which are raised before any device work.  No GPU needed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import artensor_amd as A
from artensor_amd import _native as N
from artensor_amd import measure

import measure_oracle as MO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbols_are_declared_exported_and_bound():
    names = ["artn_measure_query", "artn_measure_choose", "artn_measure_collapse"]
    raw = open(os.path.join(ROOT, "include", "artn.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(artn_[a-z0-9_]+)\s*\(", text))
    for name in names:
        assert name in declared and name in N.exported_symbols() and N.has(name)
        assert getattr(N.lib(), name).restype is ctypes.c_int
    consts = dict(re.findall(r"#define (ARTN_MEASURE_[A-Z_]+) (\d+)", text))
    assert int(consts["ARTN_MEASURE_MAX_DIMS"]) == N.MEASURE_MAX_DIMS == 10
    assert int(consts["ARTN_MEASURE_RECORD_BYTES"]) == N.MEASURE_RECORD_BYTES == 32
    assert re.search(r"#define ARTN_ABI_VERSION 9\b", text) and N.lib().artn_abi_version() == 9
    assert ctypes.sizeof(N.ArtnMeasureInfo) == 4 * 4 + 5 * 8 + 4 * 10
    for name in ("measure_", "postselect_", "reset_", "measure_info", "apply_channel_"):
        assert getattr(A, name) is getattr(measure, name)


def strides_of(perm_bits):
    """strides of a [2] * n tensor whose dim d is memory bit perm_bits[d]"""
    return [1 << b for b in perm_bits]


@pytest.mark.parametrize("dtype, elem", [(torch.complex64, 8), (torch.complex128, 16)])
def test_info_reports_memory_bits_launches_and_nominal_bytes(dtype, elem):
    n = 12
    contiguous = list(range(n - 1, -1, -1))                      # dim d is memory bit n - 1 - d
    permuted = [3, 0, 11, 7, 1, 9, 2, 10, 4, 8, 6, 5]
    for bits in (contiguous, permuted):
        for dims in ([0], [n - 1], [2, 5], [5, 2], [-1, 0, 3], list(range(10)), [11, 10, 9, 8, 7, 6, 5, 4, 3, 2]):
            info = A.measure_info((2,) * n, strides_of(bits), dims, dtype)
            k = len(dims)
            assert info["k"] == k and info["dim"] == 2 ** k and info["n"] == 2 ** n
            assert info["memory_bits"] == [bits[d] for d in dims]            # listed order, first = most significant digit
            assert info["collapse_launches"] == 1 and info["reset_launches"] == 2
            assert info["record_bytes"] == 32
            assert info["bytes_written"] == elem * 2 ** n and info["bytes_read"] == elem * 2 ** (n - k)
            assert info["grid"] == min(-(-(elem * 2 ** n // 16) // 256), 2048)
    # dims of other extents take part in the layout but not in the measurement; extent-1 dims carry no index
    info = A.measure_info((4, 2, 1, 8, 2), (1, 4, 64, 16, 8), [4, 1], dtype)
    assert info["memory_bits"] == [3, 2] and info["n"] == 128 and info["bytes_read"] == elem * 32
    big = A.measure_info((2,) * 30, strides_of(range(30)), [0, 29], dtype)
    assert big["grid"] == 2048 and big["bytes_written"] == elem << 30 and big["memory_bits"] == [0, 29]


def test_info_refuses_what_cannot_be_measured():
    shape, strides = (2, 2, 3, 2), (1, 2, 4, 12)
    with pytest.raises(ValueError, match="extent 2"):
        A.measure_info(shape, strides, [2])                      # an extent-3 dim
    with pytest.raises(ValueError, match="1 to 10"):
        A.measure_info((2,) * 12, strides_of(range(12)), list(range(11)))
    with pytest.raises(ValueError, match="1 to 10"):
        A.measure_info((2,) * 12, strides_of(range(12)), [])
    with pytest.raises(ValueError, match="distinct"):
        A.measure_info((2,) * 4, strides_of(range(4)), [1, 1])
    with pytest.raises(ValueError, match="distinct"):
        A.measure_info((2,) * 4, strides_of(range(4)), [1, -3])  # the same dim twice
    with pytest.raises(ValueError, match="distinct"):
        A.measure_info((2,) * 4, strides_of(range(4)), [4])
    with pytest.raises(ValueError, match="not dense"):
        A.measure_info((2, 2), (4, 1), [0])
    with pytest.raises(TypeError):
        A.measure_info((2, 2), (2, 1), [0], dtype=torch.float32)
    with pytest.raises(RuntimeError, match="power-of-two"):
        A.measure_info(shape, strides, [0])                      # measurable dim, but the layout holds an extent 3


def test_the_library_validates_on_its_own():
    def desc(shape, strides, keep, dtype=N.ARTN_C64):
        d = N.ArtnMarginalDesc()
        d.dtype, d.n_dims = dtype, len(shape)
        for i, (e, s) in enumerate(zip(shape, strides)):
            d.extent[i], d.stride[i], d.keep[i] = e, s, int(i in keep)
        return d

    def query(d, info=True):
        i = N.ArtnMeasureInfo()
        return N.lib().artn_measure_query(ctypes.byref(d) if d is not None else None, ctypes.byref(i) if info else None)

    err = lambda: N.lib().artn_last_error()
    assert query(desc((2, 2), (2, 1), {0})) == 0
    assert query(desc((2, 2), (2, 1), {0}), info=False) == -1 and b"null" in err()
    assert query(None) == -1 and b"null" in err()
    assert query(desc((2, 2), (2, 1), set())) == -1 and b"at least one" in err()
    assert query(desc((2, 4), (1, 2), {1})) == -1 and b"extent 2" in err()
    assert query(desc((2,) * 11, strides_of(range(11)), set(range(11)))) == -1 and b"at most 10" in err()
    assert query(desc((2, 2), (4, 1), {0})) == -1 and b"not dense" in err()
    assert query(desc((2, 3), (1, 2), {0})) == -2 and b"power-of-two" in err()
    assert query(desc((2, 2), (2, 1), {0}, dtype=N.ARTN_C64_BF16)) == -2
    assert query(desc((2,) * 41, strides_of(range(41)), {0})) == -2 and b"2^40" in err()
    # artn_measure_choose / _collapse refuse bad arguments before they would launch (no device here: that refusal may come first)
    rc = N.lib().artn_measure_choose(None, 2, None, -1, 1, None, None)
    assert rc in (-1, -4)
    rc = N.lib().artn_measure_collapse(ctypes.byref(desc((2, 2), (2, 1), {0})), None, None, 0, None)
    assert rc in (-1, -4)


def test_oracle_choice_returns_the_outcome_of_every_mid_interval_uniform():
    rng = np.random.default_rng(19)
    for D in (2, 4, 8, 64, 1024):
        q = rng.random(D) ** 3
        q[rng.random(D) < 0.3] = 0.0
        q[rng.integers(D)] = 0.7                                  # at least one live outcome
        for o in np.nonzero(q > 0)[0]:
            u = MO.mid_uniform(q, o)
            assert 0.0 <= u < 1.0
            assert MO.choose(q, u) == o
            assert measure.choose_outcome(q, u)[0] == o           # the module's host restatement agrees


def test_oracle_choice_never_returns_a_zero_probability_outcome():
    last = np.nextafter(1.0, 0.0)
    rng = np.random.default_rng(20)
    for D in (2, 4, 16, 1024):
        for trial in range(20):
            q = rng.random(D)
            q[rng.random(D) < 0.5] = 0.0
            q[rng.integers(D)] = 1e-300 if trial % 2 else 0.25    # a live outcome, possibly a tiny one
            live = np.nonzero(q > 0)[0]
            assert MO.choose(q, 0.0) == live[0]
            if q[live[-1]] > 2.0 ** -40 * q.sum():                  # (its interval is wider than the rounding of the sums)
                assert MO.choose(q, last) == live[-1]
            for u in (0.0, last, *rng.random(8)):
                o = MO.choose(q, u)
                assert q[o] > 0.0
                assert measure.choose_outcome(q, u)[0] == o
    assert MO.choose([0.0, 0.0], 0.5) == -1 and MO.choose([1.0, np.inf], 0.5) == -1 and MO.choose([np.nan, 1.0], 0.5) == -1
    assert measure.choose_outcome([0.0, 0.0], 0.5)[0] == -1 and measure.choose_outcome([1.0, np.inf], 0.5)[0] == -1


def test_oracle_states_by_indexing():
    rng = np.random.default_rng(21)
    a = (rng.standard_normal((2,) * 4) + 1j * rng.standard_normal((2,) * 4)).astype(np.complex64)
    q = MO.probabilities(a, [2, 0])
    assert np.allclose(q.sum(), (np.abs(a.astype(np.complex128)) ** 2).sum(), rtol=1e-14)
    assert np.allclose(q[2], (np.abs(a[0, :, 1, :].astype(np.complex128)) ** 2).sum(), rtol=1e-14)   # digit of dim 2 first
    c = MO.collapsed(a, [2, 0], 2, 1.0)
    assert (c[0, :, 1, :] == a[0, :, 1, :]).all() and np.count_nonzero(c) == 4
    r = MO.reset(a, [2, 0], 2, 1.0)
    assert (r[0, :, 0, :] == a[0, :, 1, :]).all() and np.count_nonzero(r) == 4
    s = MO.scale_of(q, 2)
    assert np.allclose((np.abs(MO.collapsed(a, [2, 0], 2, s).astype(np.complex128)) ** 2).sum(), q.sum(), rtol=1e-6)


def test_channel_check_refuses_an_incomplete_kraus_set():
    a = torch.zeros((2,) * 4, dtype=torch.complex64)
    damping = MO.amplitude_damping(0.3)
    with pytest.raises(ValueError, match="identity"):
        A.apply_channel_(a, damping[:1], [1])
    with pytest.raises(ValueError, match="identity"):
        A.apply_channel_(a, [damping[0], 1.001 * damping[1]], [1])
    with pytest.raises(ValueError, match="identity"):
        A.apply_channel_(a, MO.depolarizing2(0.1)[:15], [0, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # a complete set passes the check and reaches the GPU requirement
        A.apply_channel_(a, damping, [1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.apply_channel_(a, MO.depolarizing2(0.1), [0, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # check=False: the incomplete set is the caller's business
        A.apply_channel_(a, damping[:1], [1], check=False)


def test_argument_errors_come_before_any_device_work():
    a = torch.zeros((2, 2, 3, 2), dtype=torch.complex64)         # a CPU tensor: any device work would raise RuntimeError first
    b = torch.zeros((2,) * 12, dtype=torch.complex64)
    calls = {
        "measure_": lambda t, dims, **kw: A.measure_(t, dims, **kw),
        "postselect_": lambda t, dims, **kw: A.postselect_(t, dims, 0, **kw),
        "reset_": lambda t, dims, **kw: A.reset_(t, dims, **kw),
        "apply_channel_": lambda t, dims, **kw: A.apply_channel_(t, [np.eye(2 ** len(dims))], dims, **kw),
    }
    for name, call in calls.items():
        with pytest.raises(ValueError, match="extent 2"):
            call(a, [2])
        with pytest.raises(ValueError, match="distinct"):
            call(a, [0, 0])
        with pytest.raises(ValueError, match="distinct"):
            call(a, [7])
        with pytest.raises(ValueError, match="1 to 10"):
            call(b, [])
        with pytest.raises(ValueError):
            call(b, list(range(11)))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(a, [0])
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call(np.zeros((2, 2), dtype=np.complex64), [0])
    for name in ("measure_", "reset_", "apply_channel_"):
        for bad in (1.0, -0.25, float("nan"), torch.zeros(1, dtype=torch.float64), torch.zeros(2, dtype=torch.float64)):
            with pytest.raises(ValueError, match="uniform"):
                calls[name](a, [0], uniform=bad)
    for bad in (-1, 2, 4):
        with pytest.raises(ValueError, match="outcome"):
            A.postselect_(a, [0], bad)
    with pytest.raises(ValueError, match="outcome"):
        A.postselect_(a, [0, 1], None)
    with pytest.raises(ValueError, match="one or two"):
        A.apply_channel_(b, [np.eye(8)], [0, 1, 2])
    with pytest.raises(ValueError, match="entries"):
        A.apply_channel_(b, [np.eye(2)], [0, 1])
    with pytest.raises(ValueError, match="at least one"):
        A.apply_channel_(b, [], [0])
    with pytest.raises(ValueError, match="extent 2"):
        A.measure_info(a.shape, a.stride(), [2])
