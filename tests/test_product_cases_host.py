"""The host statement of the lanes-per-row summation order (tests/product_cases.py) against three yardsticks that do not share its code:
the oracle's stored-order product, the correctly rounded row sums, and -- so that a bit comparison can tell the kernels apart at all --
the requirement that the order really gives other bits than the stored order on most rows.  The emulation of the solver epilogues
(epilogue_value) is held to the same formulas in exact rational arithmetic.  Runs on the CPU."""
from fractions import Fraction

import numpy as np
import pytest

from tests.product_cases import (EPI_CHEBYSHEV, EPI_CHEBYSHEV_DOT, EPI_JACOBI, EPI_JACOBI_DOT, EPI_NAMES, EPI_OPERATIONS, EPI_RESIDUAL, EPI_RESIDUAL_DOT,
                                 EPILOGUES, LANES, RAMP_COLS, assert_rows_within_bound, case, epilogue_value, exact_rows, lanes_per_row_sum, ramp_for)
from tests.product_cases import row_sums as case_row_sums
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


# --------------------------------------------------------------------------- the solver epilogues
OMEGA, C1, C2 = 6.0 / 7.0, 0.375, -1.25
U = 2.0 ** -53


def _exact_epilogue(epi, acc, b, xo, dinv, d):
    """The formulas of epilogue_value in exact rational arithmetic from the same float64 inputs, row by row: (y, d_new or None, size, size_d)
    with size = the sum of the absolute values of the formula's terms once every bracket is multiplied out."""
    F = Fraction
    res = F(b) - F(acc)
    if epi in (EPI_RESIDUAL, EPI_RESIDUAL_DOT):
        return res, None, abs(F(b)) + abs(F(acc)), None
    if epi in (EPI_JACOBI, EPI_JACOBI_DOT):
        f = F(OMEGA) * F(dinv)
        return F(xo) + f * res, None, abs(F(xo)) + abs(f * F(b)) + abs(f * F(acc)), None
    f = F(C2) * F(dinv)
    dn = F(C1) * F(d) + f * res
    size_d = abs(F(C1) * F(d)) + abs(f * F(b)) + abs(f * F(acc))
    return F(xo) + dn, dn, abs(F(xo)) + size_d, size_d


@pytest.mark.parametrize("which", ["ramp64", "ragged"])
@pytest.mark.parametrize("epi", EPILOGUES, ids=[EPI_NAMES[e] for e in EPILOGUES])
def test_epilogue_emulation_lies_within_the_rounding_bound_of_the_exact_formula(oracle, which, epi):
    """|value - exact| <= k 2^-53 (sum of the absolute values of the formula's terms), k the number of rounded operations: 1 for the residual,
    4 for the Jacobi sweep (b - acc, dinv *, omega *, xo +), 5 for the Chebyshev step's d (b - acc, dinv *, c1 d, c2 *, +); its y = xo + d is
    one rounded addition more: 6.  The fused sum's terms are one rounded product of the rounded y: |t - u y| <= 2^-53 |u y|."""
    c = case(which)
    acc = case_row_sums(c, 1, oracle)
    y, dn, terms = epilogue_value(epi, acc, c.b, c.xo, c.dinv, OMEGA, c.d, C1, C2)
    k = EPI_OPERATIONS[epi]
    assert k == {EPI_RESIDUAL: 1, EPI_RESIDUAL_DOT: 1, EPI_JACOBI: 4, EPI_JACOBI_DOT: 4, EPI_CHEBYSHEV: 5, EPI_CHEBYSHEV_DOT: 5}[epi]
    worst = 0.0
    for i in range(c.rows):
        ey, ed, size, size_d = _exact_epilogue(epi, acc[i], c.b[i], c.xo[i], c.dinv[i], c.d[i])
        if ed is None:
            assert abs(Fraction(y[i]) - ey) <= k * Fraction(U) * size, (which, i, y[i], float(ey))
            worst = max(worst, float(abs(Fraction(y[i]) - ey) / (Fraction(U) * size)) if size else 0.0)
        else:
            assert abs(Fraction(dn[i]) - ed) <= k * Fraction(U) * size_d, (which, i, dn[i], float(ed))
            assert abs(Fraction(y[i]) - ey) <= (k + 1) * Fraction(U) * size, (which, i, y[i], float(ey))
            worst = max(worst, float(abs(Fraction(dn[i]) - ed) / (Fraction(U) * size_d)) if size_d else 0.0)
        if terms is not None:
            u = Fraction(y[i]) if epi == EPI_RESIDUAL_DOT else Fraction(c.b[i])
            assert abs(Fraction(terms[i]) - u * Fraction(y[i])) <= Fraction(U) * abs(u * Fraction(y[i])), (which, i)
    print(f"{which}, {EPI_NAMES[epi]}: the largest error is {worst:.3f} x 2^-53 x size, allowed {k}")
    assert (dn is None) == (epi not in (EPI_CHEBYSHEV, EPI_CHEBYSHEV_DOT)) and (terms is None) == (epi in (EPI_RESIDUAL, EPI_JACOBI, EPI_CHEBYSHEV))


def test_epilogue_operands_are_distinct_and_the_emulation_tells_them_apart(oracle):
    """No operand equals x[:rows] or another operand, dinv is positive and spread over six decades -- and the four ways of getting an epilogue
    subtly wrong that a kernel could take (x[row] for xo[row], a uniform dinv, dinv from another row, omega t + xo contracted into one
    rounding) each change the bits of most rows: equal bits can tell them apart."""
    for which in ("ramp64", "ragged", "poisson"):
        c = case(which)
        named = {"x": c.x[: c.rows], "w": c.w, "b": c.b, "xo": c.xo, "dinv": c.dinv, "d": c.d}
        for p in named:
            for q in named:
                assert p == q or not np.array_equal(named[p], named[q]), (p, q)
        assert (c.dinv > 0).all() and c.dinv.max() / c.dinv.min() > 1e5
        acc = case_row_sums(c, 1, oracle)
        y = epilogue_value(EPI_JACOBI, acc, c.b, c.xo, c.dinv, OMEGA)[0]
        wrong = {
            "x[row] for xo[row]": epilogue_value(EPI_JACOBI, acc, c.b, c.x[: c.rows], c.dinv, OMEGA)[0],
            "a uniform dinv": epilogue_value(EPI_JACOBI, acc, c.b, c.xo, 1.0 / 6.0, OMEGA)[0],
            "dinv of another row": epilogue_value(EPI_JACOBI, acc, c.b, c.xo, np.roll(c.dinv, 1), OMEGA)[0],
        }
        t = c.dinv * (c.b - acc)
        wrong["omega t + xo in one rounding"] = np.array([float(Fraction(OMEGA) * Fraction(a) + Fraction(z)) for a, z in zip(t, c.xo)])
        for how, other in wrong.items():
            differ = int((other != y).sum())
            print(f"{which}: {how}: {differ} of {c.rows} rows differ")
            assert differ > (c.rows // 8 if how.startswith("omega") else c.rows // 2), (which, how, differ)
