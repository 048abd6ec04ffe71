"""The host statement of the lanes-per-row summation order (tests/product_cases.py) against three yardsticks that do not share its code:
the oracle's stored-order product, the correctly rounded row sums, and -- so that a bit comparison can tell the kernels apart at all --
the requirement that the order really gives other bits than the stored order on most rows.  Runs on the CPU."""
import numpy as np
import pytest

from tests.product_cases import LANES, RAMP_COLS, assert_rows_within_bound, exact_rows, lanes_per_row_sum, ramp_for
from tests.test_mixed_host import row_sums

DTYPES = [np.float64, np.float32]


def _case(lanes, dtype):
    s = ramp_for(lanes)
    x = np.random.default_rng(100 + lanes).standard_normal(RAMP_COLS).astype(dtype)
    return s, x


def test_ramp_has_one_row_of_every_length_and_unsorted_distinct_columns():
    s = ramp_for(64)
    length = np.diff(s.RowOffsets)
    assert s.Count == 706 and sorted(length.tolist()) == list(range(706)) and not np.array_equal(length, np.arange(706))
    assert s.nnz == 705 * 706 // 2 and s.ColumnIndeces.min() >= 0 and s.ColumnIndeces.max() < RAMP_COLS
    ascending = 0
    for i in range(s.Count):
        c = s.ColumnIndeces[s.RowOffsets[i]:s.RowOffsets[i + 1]]
        assert len(np.unique(c)) == len(c)
        ascending += len(c) > 2 and bool((np.diff(c) > 0).all())
    assert ascending == 0
    mag = np.log10(np.abs(s.Elements))
    assert mag.min() < -3.0 and mag.max() > 3.0
    for lanes in LANES[:-1]:
        assert np.diff(ramp_for(lanes).RowOffsets).max() == 12 * lanes + 1


def test_one_lane_is_the_stored_order_sum(oracle):
    for lanes in LANES:                                                 # every ramp, one lane
        s, x = _case(lanes, np.float64)
        got = lanes_per_row_sum(s.Elements, s.ColumnIndeces, s.RowOffsets, x, 1)
        assert np.array_equal(got, oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, x))
        x32 = x.astype(np.float32)
        got32 = lanes_per_row_sum(s.Elements, s.ColumnIndeces, s.RowOffsets, x32, 1, dtype=np.float32)
        assert got32.dtype == np.float32
        assert np.array_equal(got32, row_sums(s.Elements.astype(np.float32), s.ColumnIndeces, s.RowOffsets, x32))


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("lanes", LANES[1:])
def test_emulation_lies_within_the_any_order_bound_of_the_exact_row_sums(lanes, dtype):
    s, x = _case(lanes, dtype)
    got = lanes_per_row_sum(s.Elements, s.ColumnIndeces, s.RowOffsets, x, lanes, dtype=dtype)
    assert got.dtype == dtype
    exact, size = exact_rows(s.Elements, s.ColumnIndeces, s.RowOffsets, x, dtype=dtype)
    assert_rows_within_bound(got, s.RowOffsets, exact, size, dtype, f"{lanes} lanes")
    short = np.diff(s.RowOffsets) <= 1                                  # no addition of two nonzero numbers: the value itself
    assert np.array_equal(got[short].astype(np.float64), exact[short])


@pytest.mark.parametrize("dtype", DTYPES, ids=["float64", "float32"])
@pytest.mark.parametrize("lanes", LANES[1:])
def test_emulation_differs_from_the_stored_order_on_most_long_rows(lanes, dtype):
    """Otherwise equal bits could not tell a lanes-per-row kernel from a stored-order one (or one lane count from another)."""
    s, x = _case(lanes, dtype)
    got = lanes_per_row_sum(s.Elements, s.ColumnIndeces, s.RowOffsets, x, lanes, dtype=dtype)
    serial = lanes_per_row_sum(s.Elements, s.ColumnIndeces, s.RowOffsets, x, 1, dtype=dtype)
    length = np.diff(s.RowOffsets)
    longer = length > lanes
    differ = int((got[longer] != serial[longer]).sum())
    print(f"{lanes} lanes, {np.dtype(dtype).name}: {differ} of {int(longer.sum())} rows longer than {lanes} differ from the stored order")
    assert 2 * differ > int(longer.sum()), (differ, int(longer.sum()))
    # rows of at most `lanes` entries with at most two of them are the same sum in both orders
    assert np.array_equal(got[length <= 2], serial[length <= 2])
    if lanes > 2:                                                       # ... and half the lane count is another order again
        other = lanes_per_row_sum(s.Elements, s.ColumnIndeces, s.RowOffsets, x, lanes // 2, dtype=dtype)
        assert 2 * int((got[longer] != other[longer]).sum()) > int(longer.sum())
