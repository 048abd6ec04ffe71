"""Every SpMV kernel of CsrMV / CsrMVDot / CsrMVFloat on every row length, operand layout and epilogue.

Kernel ids (MgcgSetSpmvKernel): 1 stream, 2..8 = 2^(k-2) lanes per row, 9 rows, 10 row-tile.  The yardstick of the stored-order kernels
(1, 2, 9, 10) is the oracle's product; of the lanes-per-row kernels, tests/product_cases.py: lanes_per_row_sum -- their stated order in
NumPy, itself held to the any-order bound of the correctly rounded row sums (tests/test_product_cases_host.py and, again, here).
Comparisons are np.array_equal unless a docstring says otherwise.  Every input is a valid product."""
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib
from conjugategradient_amd.solver import ConjugateGradientSingleGpu
from tests.gpu_util import DeviceCsr, Handles, assert_trace_close, dvec, ivec, tuning
from tests.product_cases import (KERNELS, LANE_KERNELS, MATRICES, analysis_class, assert_rows_within_bound, assert_same_rows, case, exact_rows,
                                 lanes_of, lanes_per_row_sum, ramp, ramp_of, row_sums)

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def auto_kernel(s):
    """spmv_auto_kernel (csrc/common.hpp) by the mean row length."""
    avg = s.nnz / s.Count
    return 10 if avg <= 8 else 1 if avg <= 20 else 5 if avg <= 28 else 6 if avg <= 128 else 7


@pytest.fixture(scope="module")
def h():
    hh = Handles()
    _lib.lib().MgcgSetMatrixCompression(hh.sparse, 0)     # a usable form takes precedence over a kernel id: MGCG_COMPRESSION must not decide what these tests run
    yield hh
    hh.close()


# --------------------------------------------------------------------------- the cases and their expected row sums: tests/product_cases.py
RECTANGULAR = [name for name in MATRICES if name.startswith("rect")] + ["wide-bands", "tall-bands"]
_exact = {}


def assert_within_row_bound(c, got, what):
    if c.name not in _exact:
        _exact[c.name] = exact_rows(c.s.Elements, c.s.ColumnIndeces, c.s.RowOffsets, c.x)
    exact, size = _exact[c.name]
    assert_rows_within_bound(got, c.s.RowOffsets, exact, size, np.float64, what)


def csrmv_dot(hh, c, kernel=0, rows_per_block=64, grid=0, shift=0):
    """CsrMVDot with w distinct from x into a y full of NaN; shift = 1: every array but the row offsets starts one element into its
    vector (8 bytes for the doubles, 4 for the column ids: no 16-byte alignment).  Returns (sum, y)."""
    L = _lib.lib()
    s, A = c.s, c.device()
    pad = lambda a, fill: np.concatenate([np.full(shift, fill, dtype=a.dtype), a])
    vx, vw, vy = dvec(pad(c.x, 5.0)), dvec(pad(c.w, -3.0)), dvec(np.full(c.rows + shift, np.nan))
    if shift:
        e, ci = dvec(pad(s.Elements[: s.nnz], 9.0)), ivec(pad(s.ColumnIndeces[: s.nnz], 0))
    else:
        e, ci = A.e, A.c
    L.MgcgSetSpmvKernel(hh.sparse, kernel)
    L.MgcgSetSpmvTuning(hh.sparse, rows_per_block, 0, grid)
    got = L.CsrMVDot(hh.blas, hh.sparse, vy.ToRawPtr() + 8 * shift, e.ToRawPtr() + 8 * shift, A.r.ToRawPtr(), ci.ToRawPtr() + 4 * shift,
                     vx.ToRawPtr() + 8 * shift, vw.ToRawPtr() + 8 * shift, s.nnz, c.rows, c.cols)
    L.MgcgSetSpmvKernel(hh.sparse, 0)
    L.MgcgSetSpmvTuning(hh.sparse, 64, 0, 0)
    _lib.check("CsrMVDot")
    y = vy.to_numpy(c.rows + shift)
    assert shift == 0 or np.isnan(y[0])                                             # the element in front of y is not the product's
    return got, y[shift:]


def assert_dot(c, got, y, what):
    """The any-order bound of a sum of `rows` rounded products w_i y_i, with three more additions allowed for the joins of partial sums
    that start from +0.0:  |got - fsum| <= 1.01 (rows + 3) 2^-53 sum |w_i y_i|."""
    prod = c.w * y
    want, size = math.fsum(prod), math.fsum(np.abs(prod))
    print(f"{what}: dot {got!r}, fsum {want!r}, error {abs(got - want):.3e}, bound {1.01 * (c.rows + 3) * U * size:.3e}")
    assert abs(got - want) <= 1.01 * (c.rows + 3) * U * size, (what, got, want)


# --------------------------------------------------------------------------- a. row lengths, bit for bit
@pytest.mark.parametrize("kernel", LANE_KERNELS)
def test_lanes_per_row_kernels_equal_their_stated_order_on_every_row_length(h, oracle, kernel):
    """One row of every length 0 .. 12 L + 1, and the long ramp (0 .. 705: for 64 lanes two trips of the four-strides-in-flight loop and
    every remainder behind it), at the default grid, on three workgroups and on one: a workgroup holds 256 / L rows, so on the long
    ramp's 706 rows the grid-stride loop of one workgroup takes three trips or more for every L."""
    lanes = lanes_of(kernel)
    for name in dict.fromkeys((f"ramp{lanes}", "ramp64")):
        c = case(name)
        want = row_sums(c, lanes, oracle)
        assert_within_row_bound(c, want, f"the emulation of {lanes} lanes")         # a wrong emulator cannot vouch for a wrong kernel
        for tune in (None, (64, 0, 3), (64, 0, 1)):
            got = c.device().spmv(h, c.x, kernel=kernel, tuning=tune, cols=c.cols)
            assert_same_rows(got, want, c.s.RowOffsets, f"{name}, kernel {kernel} ({lanes} lanes), tuning {tune}")
            assert_within_row_bound(c, got, f"{name}, kernel {kernel}")


@pytest.mark.parametrize("kernel", [1, 2, 9, 10])
def test_stored_order_kernels_equal_the_oracle_on_every_row_length(h, oracle, kernel):
    c = case("ramp64")
    want = row_sums(c, 1, oracle)
    for tune in (None, (64, 0, 3)):
        got = c.device().spmv(h, c.x, kernel=kernel, tuning=tune, cols=c.cols)
        assert_same_rows(got, want, c.s.RowOffsets, f"kernel {kernel}, tuning {tune}")
        assert_within_row_bound(c, got, f"kernel {kernel}")


# --------------------------------------------------------------------------- b. the epilogues of CsrMV
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("which", ["ramp", "ragged"])
def test_csrmv_epilogues_on_every_kernel(h, oracle, which, kernel):
    """alpha A x + beta y0 as the epilogue forms it (v = alpha acc; t = beta y0; v + t) from the kernel's own row sum; beta == 0 never
    reads y (y0 = NaN)."""
    c = ramp_of(kernel) if which == "ramp" else case("ragged")
    acc = row_sums(c, lanes_of(kernel), oracle)
    A = c.device()
    v = -0.5 * acc
    t = 1.75 * c.y0
    got = A.spmv(h, c.x, alpha=-0.5, beta=1.75, y0=c.y0, kernel=kernel, cols=c.cols)
    assert_same_rows(got, v + t, c.s.RowOffsets, f"kernel {kernel}: alpha = -0.5, beta = 1.75")
    got = A.spmv(h, c.x, alpha=2.5, beta=0.0, y0=np.full(c.rows, np.nan), kernel=kernel, cols=c.cols)
    assert_same_rows(got, 2.5 * acc, c.s.RowOffsets, f"kernel {kernel}: alpha = 2.5, beta = 0, y0 = NaN")


# --------------------------------------------------------------------------- c. CsrMVDot with w distinct from x
DOT_RUNS = [(1, 32), (1, 64), (1, 128), (1, 256)] + [(k, 64) for k in KERNELS[1:]]


@pytest.mark.parametrize("which", ["poisson", "ragged", "ramp"])
def test_csrmvdot_with_w_distinct_from_x_on_every_kernel(h, oracle, which):
    """y has the bits of the product alone, the returned sum is sum_i w_i y_i within the any-order bound -- and, under dot_order = 1,
    the oracle's left-to-right sum of w_i y_i bit for bit.  (A kernel that read x[row] for w[row] fails both.)"""
    for kernel, rpb in DOT_RUNS:
        c = ramp_of(kernel) if which == "ramp" else case(which)
        assert not np.array_equal(c.w, c.x[: c.rows])
        want = row_sums(c, lanes_of(kernel), oracle)
        what = f"{c.name}, kernel {kernel}, rowsPerBlock {rpb}"
        got, y = csrmv_dot(h, c, kernel, rpb)
        assert_same_rows(y, want, c.s.RowOffsets, what)
        assert_dot(c, got, y, what)
        with tuning(dot_order=1):
            got, y = csrmv_dot(h, c, kernel, rpb)
        assert_same_rows(y, want, c.s.RowOffsets, what + ", dot_order = 1")
        assert got == oracle.dot(c.w, want), (what, got, oracle.dot(c.w, want))


@pytest.mark.parametrize("kernel", [10, 9, 1, 5])
def test_csrmvdot_on_arrays_one_element_into_their_vectors(h, oracle, kernel):
    """No 16-byte alignment: kernel 10 declines to 9, 9 to 1; the lanes-per-row kernels have no alignment needs."""
    for which in ("poisson", "ragged"):
        c = case(which)
        want = row_sums(c, lanes_of(kernel), oracle)
        what = f"{which}, kernel {kernel}, shifted"
        got, y = csrmv_dot(h, c, kernel, shift=1)
        assert_same_rows(y, want, c.s.RowOffsets, what)
        assert_dot(c, got, y, what)
        with tuning(dot_order=1):
            got, y = csrmv_dot(h, c, kernel, shift=1)
        assert_same_rows(y, want, c.s.RowOffsets, what + ", dot_order = 1")
        assert got == oracle.dot(c.w, want), (what, got)


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_csrmvdot_with_w_distinct_from_x_on_the_lossless_forms(oracle, mode):
    """MgcgSetMatrixCompression on a fresh handle; whichever class the analysis reports (printed, any accepted: a form, or none and
    then the forced stored-order stream kernel), the forms are lossless and keep the stored order: the oracle's bits."""
    hh = Handles()
    _lib.lib().MgcgSetMatrixCompression(hh.sparse, mode)
    for which in ("poisson", "ragged", "ramp64"):
        c = case(which)
        want = row_sums(c, 1, oracle)
        got, y = csrmv_dot(hh, c, kernel=1)
        print(which, "mode", mode, "class", analysis_class(hh))
        assert_same_rows(y, want, c.s.RowOffsets, f"{which}, mode {mode}")
        assert_dot(c, got, y, f"{which}, mode {mode}")
        with tuning(dot_order=1):
            got, y = csrmv_dot(hh, c, kernel=1)
        assert_same_rows(y, want, c.s.RowOffsets, f"{which}, mode {mode}, dot_order = 1")
        assert got == oracle.dot(c.w, want), (which, mode, got)
        _lib.lib().MgcgAnalysisClear(hh.sparse)
    hh.close()


# --------------------------------------------------------------------------- d. rectangular products
@pytest.mark.parametrize("which", RECTANGULAR)
def test_rectangular_products_on_every_kernel(h, oracle, which):
    """700 x 1900 and 1900 x 700 -- random at 8 and at 40 entries a row, and the two banded ones -- with unsorted columns and empty rows:
    CsrMV (plain and with both epilogues of (b)) and CsrMVDot (w of length rows) under every kernel id and the auto rule."""
    c = case(which)
    length = np.diff(c.s.RowOffsets)
    assert (length == 0).sum() >= c.rows // 11 and c.rows != c.cols
    assert auto_kernel(c.s) == (6 if which.endswith("x40") else 10), (c.s.nnz / c.rows)
    A = c.device()
    for kernel in (0,) + KERNELS:
        acc = row_sums(c, lanes_of(kernel or auto_kernel(c.s)), oracle)
        what = f"{which}, kernel {kernel}"
        assert_same_rows(A.spmv(h, c.x, kernel=kernel, cols=c.cols), acc, c.s.RowOffsets, what)
        v, t = -0.5 * acc, 1.75 * c.y0
        assert_same_rows(A.spmv(h, c.x, alpha=-0.5, beta=1.75, y0=c.y0, kernel=kernel, cols=c.cols), v + t, c.s.RowOffsets, what + ", beta = 1.75")
        assert_same_rows(A.spmv(h, c.x, alpha=2.5, beta=0.0, y0=np.full(c.rows, np.nan), kernel=kernel, cols=c.cols), 2.5 * acc, c.s.RowOffsets,
                         what + ", y0 = NaN")
        got, y = csrmv_dot(h, c, kernel)
        assert_same_rows(y, acc, c.s.RowOffsets, what + ", CsrMVDot")
        assert_dot(c, got, y, what)
        with tuning(dot_order=1):
            # (the auto rule takes the stored-order stream kernel for long rows in this mode)
            want = row_sums(c, lanes_of(kernel), oracle) if kernel else row_sums(c, 1, oracle)
            got, y = csrmv_dot(h, c, kernel)
        assert_same_rows(y, want, c.s.RowOffsets, what + ", CsrMVDot, dot_order = 1")
        assert got == oracle.dot(c.w, want), (what, got)
    assert_within_row_bound(c, row_sums(c, 16, oracle), "the emulation of 16 lanes")


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_rectangular_products_on_the_lossless_forms(oracle, mode):
    """The same matrices under MgcgSetMatrixCompression (class printed; no form: the forced stored-order stream kernel).  The random ones
    may take any class.  The banded ones must be served by a form -- the wide one by the row-pattern form (class 3) where the mode
    offers it, the tall one by another than that: its kernel gathers x[row] for the masked slots of an empty row, which lies beyond x for
    the rows from columnCount on, so the analysis declines it when columnCount < rowCount."""
    hh = Handles()
    _lib.lib().MgcgSetMatrixCompression(hh.sparse, mode)
    for which in RECTANGULAR:
        c = case(which)
        acc = row_sums(c, 1, oracle)
        A = c.device()
        assert_same_rows(A.spmv(hh, c.x, kernel=1, cols=c.cols), acc, c.s.RowOffsets, f"{which}, mode {mode}")
        cls = analysis_class(hh)
        print(which, "mode", mode, "class", cls)
        if which == "wide-bands":
            assert cls == (2 if mode == 2 else 3), cls
        if which == "tall-bands":
            assert cls in (1, 2), cls
        v, t = -0.5 * acc, 1.75 * c.y0
        assert_same_rows(A.spmv(hh, c.x, alpha=-0.5, beta=1.75, y0=c.y0, kernel=1, cols=c.cols), v + t, c.s.RowOffsets, f"{which}, mode {mode}, beta = 1.75")
        assert_same_rows(A.spmv(hh, c.x, alpha=2.5, beta=0.0, y0=np.full(c.rows, np.nan), kernel=1, cols=c.cols), 2.5 * acc, c.s.RowOffsets,
                         f"{which}, mode {mode}, y0 = NaN")
        got, y = csrmv_dot(hh, c, kernel=1)
        assert_same_rows(y, acc, c.s.RowOffsets, f"{which}, mode {mode}, CsrMVDot")
        assert_dot(c, got, y, f"{which}, mode {mode}")
        _lib.lib().MgcgAnalysisClear(hh.sparse)
    hh.close()


# --------------------------------------------------------------------------- e. the handle's kernel id is what the header says
LISTED = {0: 32, 1: 1, 2: 1, 3: 2, 4: 4, 5: 8, 6: 16, 7: 32, 8: 64, 9: 1, 10: 1}      # id -> lanes per row on the long ramp (0: auto, mean 352.5 -> 7)


def test_listed_kernel_ids_do_what_the_header_lists(h, oracle):
    """On the long ramp every lane count gives other bits (asserted), so the product tells which order ran."""
    c = case("ramp64")
    assert auto_kernel(c.s) == 7
    sums = {lanes: row_sums(c, lanes, oracle) for lanes in (1, 2, 4, 8, 16, 32, 64)}
    for a in sums:
        for b in sums:
            assert a == b or (sums[a] != sums[b]).sum() > c.rows // 2, (a, b)
    assert_same_rows(c.device().spmv(h, c.x, kernel=2, cols=c.cols), oracle.spmv(c.s.Elements, c.s.ColumnIndeces, c.s.RowOffsets, c.x),
                     c.s.RowOffsets, "kernel 2: one lane per row, the oracle's bits")
    for kernel, lanes in LISTED.items():
        assert_same_rows(c.device().spmv(h, c.x, kernel=kernel, cols=c.cols), sums[lanes], c.s.RowOffsets, f"kernel id {kernel}: {lanes} lanes per row")


@pytest.mark.parametrize("kernel", [11, -1, 64, 2 ** 31 - 1])
def test_unlisted_kernel_ids_run_what_8_runs(h, oracle, kernel):
    """include/MgcgGpu.h: every other value is not an error and runs the 64-lanes-per-row kernel."""
    c = case("ramp64")
    got = c.device().spmv(h, c.x, kernel=kernel, cols=c.cols)
    assert not _lib.last_error()
    assert_same_rows(got, row_sums(c, 64, oracle), c.s.RowOffsets, f"kernel id {kernel}")


# --------------------------------------------------------------------------- f. solves under a forced kernel
_cg_refs = {}


@pytest.mark.parametrize("kernel", [1, 2, 5, 8, 9])
@pytest.mark.parametrize("which", ["ragged", "mgcg700"])
def test_solve_under_a_forced_kernel_equals_the_oracle(oracle, which, kernel):
    """SolveEx takes the handle's kernel for its products (residual, residual + dot, p.Ap epilogues): the oracle's iteration count, its
    trace within assert_trace_close and its x within 1e-10 max|x|."""
    s = case(which).s
    tol = 1e-8 * float(np.linalg.norm(s.b))
    if which not in _cg_refs:
        _cg_refs[which] = oracle.cg(s, rule=oracle.RULE_CSHARP, allowable_residual=tol, max_iteration=2000, trace=True)
    ref = _cg_refs[which]
    assert ref["status"] == oracle.OK and ref["iteration"] >= 5, ref["iteration"]
    cg = ConjugateGradientSingleGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 2000, tol, rule=_lib.RULE_CSHARP).load(s)
    _lib.lib().MgcgSetSpmvKernel(cg.cusparse, kernel)
    cg.Initialize()
    cg.Solve(trace=True)
    cg.Read()
    print(which, "kernel", kernel, "iterations", cg.Iteration, ref["iteration"], "residual", cg.Residual, ref["residual"],
          "max |x - x_oracle| / max |x|", np.abs(cg.x - ref["x"]).max() / np.abs(ref["x"]).max())
    assert cg.Iteration == ref["iteration"]
    assert_trace_close(cg.trace, ref["trace"])
    assert np.abs(cg.x - ref["x"]).max() <= 1e-10 * np.abs(ref["x"]).max()
    cg.Dispose()


# --------------------------------------------------------------------------- g. the fp32 product
@pytest.mark.parametrize("max_len,lanes", [(30, 1), (48, 8), (200, 16), (420, 32)])
def test_float_product_forms_equal_their_stated_order(h, mgcg_env, max_len, lanes):
    """A square ramp of rows 0 .. max_len: mean length max_len / 2 = 15, 24, 100, 210 selects CsrMVFloat's lane = row form and its
    8, 16 and 32 lane forms.  Each equals its order in np.float32 bit for bit; under MGCG_DOT_ORDER = 1 all equal the serial product."""
    from tests.test_gpu_mixed import DeviceSystem
    from tests.test_mixed_host import row_sums as serial_float

    s = ramp(max_len, cols=max_len + 1, seed=max_len)
    mean = s.nnz / s.Count
    assert mean == max_len / 2 and (mean <= 20) == (lanes == 1) and (lanes != 8 or 20 < mean <= 28) and (lanes != 16 or 28 < mean <= 128) and (lanes != 32 or mean > 128)
    d = DeviceSystem(h, s)
    assert d.setup() == 0
    x = np.random.default_rng(max_len).standard_normal(s.Count).astype(np.float32)
    e32 = s.Elements.astype(np.float32)
    serial = serial_float(e32, s.ColumnIndeces, s.RowOffsets, x)
    want = lanes_per_row_sum(e32, s.ColumnIndeces, s.RowOffsets, x, lanes, dtype=np.float32)
    exact, size = exact_rows(e32, s.ColumnIndeces, s.RowOffsets, x, dtype=np.float32)
    assert_rows_within_bound(want, s.RowOffsets, exact, size, np.float32, f"the float32 emulation of {lanes} lanes")
    assert (lanes == 1) == np.array_equal(want, serial)
    got = d.product(x)
    assert_same_rows(got, want, s.RowOffsets, f"CsrMVFloat, rows up to {max_len}: {lanes} lanes")
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    got = d.product(x)
    mgcg_env.delenv("MGCG_DOT_ORDER")
    assert_same_rows(got, serial, s.RowOffsets, f"CsrMVFloat, rows up to {max_len}, MGCG_DOT_ORDER = 1")


# --------------------------------------------------------------------------- h. CsrMVDot names its write
def test_csrmvdot_marks_an_analysis_of_the_arrays_it_writes_stale(oracle):
    """Compression 1: the 7-point matrix is analysed into one byte per row (class 3).  CsrMVDot then writes its y -- another matrix's
    product -- over the first entries of that matrix's `elements` vector; the next CsrMV on those arrays multiplies the new values."""
    L = _lib.lib()
    a, b = case("poisson"), case("ragged")
    assert b.rows < a.s.nnz
    hh = Handles()
    L.MgcgSetMatrixCompression(hh.sparse, 1)
    A = DeviceCsr(a.s)                                                              # its own arrays: they are overwritten below
    first = A.spmv(hh, a.x)
    assert analysis_class(hh) == 3
    assert_same_rows(first, row_sums(a, 1, oracle), a.s.RowOffsets, "before the write")
    B, vx, vw = b.device(), dvec(b.x), dvec(b.w)
    L.MgcgSetSpmvKernel(hh.sparse, 1)
    L.CsrMVDot(hh.blas, hh.sparse, A.e.ToRawPtr(), B.e.ToRawPtr(), B.r.ToRawPtr(), B.c.ToRawPtr(), vx.ToRawPtr(), vw.ToRawPtr(), b.s.nnz, b.rows, b.cols)
    L.MgcgSetSpmvKernel(hh.sparse, 0)
    _lib.check("CsrMVDot")
    elements = A.e.to_numpy(a.s.nnz)
    assert np.array_equal(elements[: b.rows], row_sums(b, 1, oracle)) and np.array_equal(elements[b.rows:], a.s.Elements[b.rows: a.s.nnz])
    want = oracle.spmv(elements, a.s.ColumnIndeces, a.s.RowOffsets, a.x)
    assert not np.array_equal(want, first)
    assert_same_rows(A.spmv(hh, a.x), want, a.s.RowOffsets, "after CsrMVDot wrote into the analysed matrix")
    L.MgcgAnalysisClear(hh.sparse)
    hh.close()
