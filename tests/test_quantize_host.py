"""The host twin of the median-cut quantiser (rto_quantize_median_cut_host, csrc/host/median_cut.cpp) against the numpy model
of tests/quantize_ref.py: ids and palette bit for bit -- the definition in include/rto.h leaves nothing to an implementation,
so there is no tolerance.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

import quantize_ref
import rt_octree_amd as R
from rt_octree_amd import quantize, synth

RTO_E_INVALID = -1


@pytest.mark.parametrize("name", sorted(quantize_ref.CASES))
def test_host_twin_equals_the_model(name):
    rows, bits, pal, ids = quantize_ref.case(name)
    got_pal, got_ids = quantize.quantize_median_cut(rows, bits, backend="cpu")
    assert got_pal.dtype == np.float16 and got_pal.shape == (1 << bits, 3) and got_ids.dtype == np.uint16
    quantize_ref.assert_same(got_pal, got_ids, pal, ids, name)


def test_identical_rows_split_by_row_index():
    rows, bits, pal, ids = quantize_ref.case("identical_m70000")
    m = rows.shape[0]
    assert np.all(np.diff(ids.astype(np.int64)) >= 0)  # every split is a pure tie: ids follow the row index
    cnt = np.bincount(ids, minlength=1 << bits)
    assert cnt.min() == m >> bits and cnt.max() == (m >> bits) + 1
    assert np.array_equal(pal[ids].view(np.uint16), rows.view(np.uint16))


def test_without_ties_the_ids_are_those_of_the_development_helper():
    rows, bits, pal, ids = quantize_ref.case("distinct_m4096")
    _, old = synth.median_cut_ids(rows.astype(np.float32), bits, device="cpu")
    assert np.array_equal(old.astype(np.uint16), ids)
    got_pal, got_ids = quantize.quantize_median_cut(rows, bits, backend="cpu")
    assert np.array_equal(got_ids, old.astype(np.uint16))


def test_minus_zero_sorts_before_plus_zero():
    rows = np.zeros((4, 3), np.float16)
    rows[[1, 3], 0] = np.float16(-0.0)
    pal, ids = quantize.quantize_median_cut(rows, 1, backend="cpu")
    assert ids.tolist() == [1, 0, 1, 0]
    assert pal.view(np.uint16)[:, 0].tolist() == [0, 0]  # (-0 + -0) is the integer 0: the mean is +0


def _call(rows_ptr, m, bits, pal_ptr, ids_ptr):
    rc = R.lib().rto_quantize_median_cut_host(rows_ptr, m, bits, pal_ptr, ids_ptr)
    return rc, R.lib().rto_last_error().decode()


def _buffers(m, bits=16):
    rows = np.ones((max(m, 1), 3), np.float16)
    return rows, np.zeros((1 << min(max(bits, 1), 16), 3), np.float16), np.zeros(max(m, 1), np.uint16)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_refuses_non_finite_values(bad):
    rows, pal, ids = _buffers(100)
    rows[57, 2] = bad
    rc, msg = _call(rows.ctypes.data, 100, 16, pal.ctypes.data, ids.ctypes.data)
    assert rc == RTO_E_INVALID and "NaN" in msg and "57" in msg
    with pytest.raises(R.RtoError):
        quantize.quantize_median_cut(rows, 16, backend="cpu")


@pytest.mark.parametrize("m,bits", [(0, 16), (-1, 16), (1 << 31, 16), (10, 0), (10, 17)])
def test_refuses_sizes(m, bits):
    rows, pal, ids = _buffers(10, bits)
    rc, msg = _call(rows.ctypes.data, m, bits, pal.ctypes.data, ids.ctypes.data)
    assert rc == RTO_E_INVALID and msg


@pytest.mark.parametrize("null", [0, 1, 2])
def test_refuses_null_pointers(null):
    rows, pal, ids = _buffers(10)
    ptrs = [rows.ctypes.data, pal.ctypes.data, ids.ctypes.data]
    ptrs[null] = None
    rc, msg = _call(ptrs[0], 10, 16, ptrs[1], ptrs[2])
    assert rc == RTO_E_INVALID and "null" in msg


def test_refuses_a_sum_that_could_overflow():
    # 65504 = 2047 * 2^5 = 2047 * 2^29 units of 2^-24: m * that reaches 2^63 from m = ceil(2^34 / 2047) = 8392707
    m = -(-(1 << 34) // 2047)
    rows = np.full((m, 3), 1.0, np.float16)
    pal, ids = np.zeros((2, 3), np.float16), np.zeros(m, np.uint16)
    rows[12345, 1] = np.float16(-65504.0)
    rc, msg = _call(rows.ctypes.data, m, 1, pal.ctypes.data, ids.ctypes.data)
    assert rc == RTO_E_INVALID and "overflow" in msg
    rc, msg = _call(rows.ctypes.data, m - 1, 1, pal.ctypes.data, ids.ctypes.data)  # one row fewer is taken
    assert rc == 0, msg
    assert np.bincount(ids[:m - 1]).tolist() == [m // 2, (m - 1) // 2]
