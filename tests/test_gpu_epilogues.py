"""The six solver-only SpMV epilogues (residual, Jacobi sweep, Chebyshev step, each with and without its fused sum) on every kernel id
and every matrix form, through MgcgCsrMVEpilogue: one fused pass by the solvers' own routes (launch_spmv_auto, launch_spmv_range,
launch_spmv_two_ranges, launch_spmv for the Chebyshev step).

The expected y (and d of the Chebyshev step) is tests/product_cases.py: epilogue_value of the kernel's own row sum -- the oracle's product for
the stored-order kernels (1, 2, 9, 10) and for every lossless form, lanes_per_row_sum for kernels 3 .. 8 -- compared with assert_same_rows:
equal bits, NaN where the statement has NaN.  The emulation itself is held to exact rational arithmetic in
tests/test_product_cases_host.py.  Fused sums: the any-order bound over the rounded terms, and under dot_order = 1 the oracle's serial sum.
y is NaN before every call; every operand comes from a seed of its own (product_cases.Case).  The handles of the kernel tests switch the
matrix forms off themselves, so MGCG_COMPRESSION does not change what a forced kernel id runs."""
import ctypes as C
import math

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from tests.block_cases import assert_poisoned_product, poison
from tests.gpu_util import Handles, dvec, ivec, tuning
from tests.product_cases import (EPI_CHEBYSHEV, EPI_CHEBYSHEV_DOT, EPI_JACOBI, EPI_JACOBI_DOT, EPI_NAMES, EPI_RESIDUAL, EPI_RESIDUAL_DOT, EPILOGUES, KERNELS,
                                 Case, analysis_class, assert_same_rows, case, epilogue_value, lanes_of, lanes_per_row_sum, ramp_of, row_sums)

pytestmark = pytest.mark.gpu

OMEGA, C1, C2 = 6.0 / 7.0, 0.375, -1.25
U = 2.0 ** -53
WITHOUT_CHEBYSHEV = (EPI_RESIDUAL, EPI_RESIDUAL_DOT, EPI_JACOBI, EPI_JACOBI_DOT)
CHEBYSHEV = (EPI_CHEBYSHEV, EPI_CHEBYSHEV_DOT)
ARRAY = "array"                                            # dinv: the case's array (default), or a number = dinv NULL with that dinvScalar


@pytest.fixture(scope="module")
def h():
    hh = Handles()
    _lib.lib().MgcgSetMatrixCompression(hh.sparse, 0)
    yield hh
    hh.close()


# --------------------------------------------------------------------------- one call
_operands = {}


def _device_operands(c, shift):
    """The case's read-only arrays on the device, uploaded once; shift = 1: every one but the row offsets one element into its vector."""
    key = (c.name, shift)
    if key not in _operands:
        pad = lambda a, fill: np.concatenate([np.full(shift, fill, dtype=a.dtype), a])
        s = c.s
        _operands[key] = dict(e=dvec(pad(s.Elements[: s.nnz], 9.0)), ci=ivec(pad(s.ColumnIndeces[: s.nnz], 0)), r=ivec(s.RowOffsets), x=dvec(pad(c.x, 5.0)),
                              b=dvec(pad(c.b, -3.0)), xo=dvec(pad(c.xo, 7.0)), dinv=dvec(pad(c.dinv, 2.0)))
    return _operands[key]


def run(hh, c, epi, kernel=0, tune=None, shift=0, rows=None, gap=None, dinv=ARRAY, x=None, scaled=None, done=None, d0=None, null=(), alias=None,
        refused=False):
    """MgcgCsrMVEpilogue into a y full of NaN.  rows / gap: (begin, end); dinv: ARRAY, an array, or a number (dinv NULL, dinvScalar);
    x: another multiplied vector than the case's; scaled: (xInner, xOuter); done: the value of a device int, None = a null pointer;
    d0: what d starts from (default the case's d); null: operands handed in as NULL; alias: the operand that is handed y's address.
    Returns (sum, y, d), all rows; refused: the call must fail -- returns (sum, y, d, message)."""
    L = _lib.lib()
    s, ops = c.s, _device_operands(c, shift)
    n = c.rows
    vy = dvec(np.full(n + shift, np.nan))
    d_start = np.concatenate([np.full(shift, 11.0), c.d if d0 is None else d0])
    vd = dvec(d_start)
    keep = [vy, vd]
    ptr = {name: v.ToRawPtr() + (4 if name == "ci" else 8) * shift for name, v in ops.items() if name != "r"}
    if x is not None:
        keep.append(dvec(np.concatenate([np.full(shift, 5.0), x])))
        ptr["x"] = keep[-1].ToRawPtr() + 8 * shift
    a = _lib.EpilogueArgs()
    a.epilogue, a.elementsCount, a.rowCount, a.columnCount = int(epi), int(s.nnz), int(n), int(c.cols)
    a.y, a.elements, a.rowOffsets, a.columnIndeces = vy.ToRawPtr() + 8 * shift, ptr["e"], ops["r"].ToRawPtr(), ptr["ci"]
    a.x, a.b, a.xo, a.d = ptr["x"], ptr["b"], ptr["xo"], vd.ToRawPtr() + 8 * shift
    if isinstance(dinv, str):
        a.dinv = ptr["dinv"]
    elif np.ndim(dinv) == 1:
        keep.append(dvec(np.concatenate([np.full(shift, 2.0), dinv])))
        a.dinv = keep[-1].ToRawPtr() + 8 * shift
    else:
        a.dinv, a.dinvScalar = None, float(dinv)
    a.omega, a.c1, a.c2 = OMEGA, C1, C2
    if scaled is not None:
        a.xInner, a.xOuter = scaled
    if rows is not None:
        a.rowBegin, a.rowEnd = int(rows[0]), int(rows[1])
    if gap is not None:
        a.gapBegin, a.gapEnd = int(gap[0]), int(gap[1])
    if done is not None:
        keep.append(ivec(np.array([done], dtype=np.int32)))
        a.done = keep[-1].ToRawPtr()
    for name in null:
        setattr(a, name, None)
    if alias is not None:
        setattr(a, alias, a.y)
    L.MgcgSetSpmvKernel(hh.sparse, kernel)
    L.MgcgSetSpmvTuning(hh.sparse, *(tune or (64, 0, 0)))
    got = L.MgcgCsrMVEpilogue(hh.blas, hh.sparse, C.byref(a))
    L.MgcgSetSpmvKernel(hh.sparse, 0)
    L.MgcgSetSpmvTuning(hh.sparse, 64, 0, 0)
    message = _lib.last_error()
    if refused:
        L.MgcgClearLastError()
    else:
        _lib.check("MgcgCsrMVEpilogue")
    y, d = vy.to_numpy(n + shift), vd.to_numpy(n + shift)
    assert shift == 0 or (np.isnan(y[0]) and d[0] == 11.0)                          # the elements in front of y and d are not the pass's
    for v in keep:
        v.Dispose()
    return (got, y[shift:], d[shift:], message) if refused else (got, y[shift:], d[shift:])


def selected(n, rows=None, gap=None):
    sel = np.ones(n, dtype=bool)
    if rows is not None:
        sel[:] = False
        sel[rows[0]: rows[1]] = True
    if gap is not None:
        sel[gap[0]: gap[1]] = False
    return sel


def serial_sum(oracle, epi, c, y, sel, gap=None):
    """What the entry returns under dot_order = 1: the oracle's left-to-right sum over the selected rows; with a gap, the sum of the rows in
    front of it plus the sum of those behind it."""
    u = y if epi == EPI_RESIDUAL_DOT else c.b
    if gap is None:
        return oracle.dot(np.ascontiguousarray(u[sel]), np.ascontiguousarray(y[sel]))
    parts = [oracle.dot(np.ascontiguousarray(u[lo:hi]), np.ascontiguousarray(y[lo:hi])) for lo, hi in ((0, gap[0]), (gap[1], c.rows)) if hi > lo]
    return math.fsum(parts) if len(parts) < 2 else parts[0] + parts[1]


def check(c, epi, acc, got, what, rows=None, gap=None, dinv=ARRAY, oracle=None):
    """y: the statement's bits on the selected rows, NaN on every other; d: the Chebyshev step's new d, else untouched; the sum: 0.0 for an epilogue
    without one, else within 1.01 (n + 3) 2^-53 sum |t_i| of fsum(t_i) over the n selected rows' rounded terms t_i of the expected y (any order of
    adding n numbers makes at most n - 1 rounding errors, each of at most 2^-53 times a partial sum of at most sum |t_i| (1 + 2^-53)^n; joins of
    partial sums that start from +0.0 add nothing; three spare) -- or, with `oracle` (the call ran under dot_order = 1), the serial sum."""
    total, y, d = got
    sel = selected(c.rows, rows, gap)
    wy, wd, terms = epilogue_value(epi, acc, c.b, c.xo, c.dinv if isinstance(dinv, str) else dinv, OMEGA, c.d, C1, C2)
    assert_same_rows(y, np.where(sel, wy, np.nan), c.s.RowOffsets, what + ": y")
    assert_same_rows(d, c.d if wd is None else wd, c.s.RowOffsets, what + ": d")
    if terms is None:
        assert total == 0.0, (what, total)
        return
    t = terms[sel]
    want, size = math.fsum(t), math.fsum(np.abs(t))
    print(f"{what}: sum {total!r}, fsum {want!r}, error {abs(total - want):.3e}, bound {1.01 * (t.size + 3) * U * size:.3e}")
    assert abs(total - want) <= 1.01 * (t.size + 3) * U * size, (what, total, want)
    if oracle is not None:
        assert total == serial_sum(oracle, epi, c, wy, sel, gap), (what, total)


def run_and_check(hh, oracle, c, epi, acc, what, **kw):
    """The call at the default order of the sum and, for an epilogue with a sum, once more under dot_order = 1."""
    checked = {k: kw[k] for k in ("rows", "gap", "dinv") if k in kw}
    what = f"{c.name}, {EPI_NAMES[epi]}, {what}"
    check(c, epi, acc, run(hh, c, epi, **kw), what, **checked)
    if epi in (EPI_RESIDUAL_DOT, EPI_JACOBI_DOT, EPI_CHEBYSHEV_DOT):
        with tuning(dot_order=1):
            check(c, epi, acc, run(hh, c, epi, **kw), what + ", dot_order = 1", oracle=oracle, **checked)


# --------------------------------------------------------------------------- a. every kernel id x six epilogues
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("which", ["ramp", "ragged"])
def test_every_epilogue_on_every_kernel(h, oracle, which, kernel):
    """The kernel's ramp (every row length 0 .. 12 lanes + 1) and the long ramp (0 .. 705), or ragged_spd(1350): at the default grid and
    on ONE workgroup, which then takes many trips of its grid-stride loop (and, for a fused sum, is the only partial); the stream kernel also
    at 32, 128 and 256 rows per block."""
    names = dict.fromkeys((ramp_of(kernel).name, "ramp64")) if which == "ramp" else ["ragged"]
    tunes = [None, (64, 0, 1)] + ([(32, 0, 0), (128, 0, 0), (256, 0, 0)] if kernel == 1 else [])
    for name in names:
        c = case(name)
        acc = row_sums(c, lanes_of(kernel), oracle)
        for epi in EPILOGUES:
            for tune in tunes:
                run_and_check(h, oracle, c, epi, acc, f"kernel {kernel}, tuning {tune}", kernel=kernel, tune=tune)


# --------------------------------------------------------------------------- b. a uniform diagonal
@pytest.mark.parametrize("kernel", KERNELS)
def test_uniform_dinv_equals_an_array_of_that_number(h, oracle, kernel):
    """dinv == NULL and dinvScalar = 1/6 on the 20 x 17 x 13 Poisson matrix: the statement's bits with dinv_i = 1/6, which are those of a
    run on an array full of 1/6 -- while the case's own dinv array (read by a kernel that ignored dinvUniform) gives other bits."""
    c = case("poisson")
    acc = row_sums(c, lanes_of(kernel), oracle)
    sixth = 1.0 / 6.0
    for epi in (EPI_JACOBI, EPI_JACOBI_DOT) + CHEBYSHEV:
        for tune in (None, (64, 0, 1)):
            what = f"kernel {kernel}, tuning {tune}, uniform dinv"
            run_and_check(h, oracle, c, epi, acc, what, kernel=kernel, tune=tune, dinv=sixth)
            uniform = run(h, c, epi, kernel=kernel, tune=tune, dinv=sixth)
            array = run(h, c, epi, kernel=kernel, tune=tune, dinv=np.full(c.rows, sixth))
            assert_same_rows(uniform[1], array[1], c.s.RowOffsets, what + ": y against the run on an array")
            assert_same_rows(uniform[2], array[2], c.s.RowOffsets, what + ": d against the run on an array")
            assert uniform[0] == array[0], (what, uniform[0], array[0])
    other = epilogue_value(EPI_JACOBI, acc, c.b, c.xo, c.dinv, OMEGA)[0]
    assert (other != epilogue_value(EPI_JACOBI, acc, c.b, c.xo, sixth, OMEGA)[0]).sum() > c.rows // 2


# --------------------------------------------------------------------------- c. operand layout
@pytest.mark.parametrize("kernel", [10, 9, 1, 5])
def test_epilogues_on_arrays_one_element_into_their_vectors(h, oracle, kernel):
    """No 16-byte alignment (8 bytes into every vector of doubles, 4 into the column ids): kernel 10 declines to 9, 9 to 1; the results do
    not change, and the elements in front of y and d stay what they were (asserted in run)."""
    for which in ("poisson", "ragged"):
        c = case(which)
        acc = row_sums(c, lanes_of(kernel), oracle)
        for epi in EPILOGUES:
            run_and_check(h, oracle, c, epi, acc, f"kernel {kernel}, shifted", kernel=kernel, shift=1)


# --------------------------------------------------------------------------- d. row ranges
def ranges_of(n):
    return [(0, 1), (1, n), (257, 1031), (n - 1, n)]


@pytest.mark.parametrize("kernel", [10, 9, 1, 5])
@pytest.mark.parametrize("which", ["poisson", "ragged"])
def test_row_ranges_on_the_csr_kernels(h, oracle, which, kernel):
    """launch_spmv_range shifts y, xo, b, dinv and the row offsets by the range's first row: rows inside the range carry the statement's bits,
    every row outside it stays NaN, the sum covers the range's rows only."""
    c = case(which)
    acc = row_sums(c, lanes_of(kernel), oracle)
    for epi in WITHOUT_CHEBYSHEV:
        for rows in ranges_of(c.rows):
            run_and_check(h, oracle, c, epi, acc, f"kernel {kernel}, rows {rows}", kernel=kernel, rows=rows)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("which", ["poisson", "ragged"])
def test_row_ranges_on_the_row_pattern_and_code_forms(oracle, which, mode):
    """MgcgSetMatrixCompression 1 and 2 on a fresh handle: the Poisson matrix takes the row-pattern form (class 3) and the code form (class 2,
    or 1), where launch_spmv_range also shifts the pattern ids and the form's row base; a matrix that takes no form (class printed) runs
    the forced stored-order stream kernel.  Every form keeps the stored order: the oracle's bits."""
    hh = Handles()
    _lib.lib().MgcgSetMatrixCompression(hh.sparse, mode)
    c = case(which)
    acc = row_sums(c, 1, oracle)
    for epi in WITHOUT_CHEBYSHEV:
        for rows in ranges_of(c.rows):
            run_and_check(hh, oracle, c, epi, acc, f"mode {mode}, rows {rows}", kernel=1, rows=rows)
    cls = analysis_class(hh)
    print(which, "mode", mode, "class", cls)
    if which == "poisson":
        assert cls == (3 if mode == 1 else 2), cls
    _lib.lib().MgcgAnalysisClear(hh.sparse)
    hh.close()


@pytest.mark.parametrize("which,gap", [("poisson", (256, 512)), ("poisson", (512, 4352)), ("poisson", (300, 900)), ("ragged", (256, 512)), ("ragged", (300, 900))])
def test_two_ranges_around_a_gap(h, oracle, which, gap):
    """Kernel 10: gaps on the row-tile kernel's tile boundaries (multiples of 256) take ONE launch that skips the gap's tiles, the off-tile cut
    two launches; the gap's rows stay NaN either way and the sum runs over the rows outside it.  Kernel 1: always two launches."""
    c = case(which)
    acc = row_sums(c, 1, oracle)
    for kernel in (10, 1):
        for epi in WITHOUT_CHEBYSHEV:
            run_and_check(h, oracle, c, epi, acc, f"kernel {kernel}, gap {gap}", kernel=kernel, gap=gap)


# --------------------------------------------------------------------------- e. lossless forms, whole matrix
_big = {}


def big_case(name):
    """The matrices of the column-tiled and propagation-blocking forms, built once.  The propagation-blocking form keeps the 200 000 rows
    (13 tiles of x) of tests/test_gpu_pb.py: random_spd(n, seed=12345) was tried under mode 3 at n = 40 000, 60 000, 70 000, 80 000, 100 000
    and 140 000 (3 .. 9 tiles of 16384 columns) and the analysis took no form for any of them (class 0)."""
    if name not in _big:
        s = problems.random_spd(40000, mean_upper=14.0, seed=3) if name == "tiled" else problems.random_spd(200_000, seed=12345)
        _big[name] = Case(name, s)
    return _big[name]


FORMS = ["mode1-poisson", "mode1-ragged", "mode1-ramp64", "mode2-poisson", "mode2-ragged", "mode2-ramp64", "tiled-pack1", "tiled-pack0", "pb"]


def open_form(form, mgcg_env):
    """(handle, case, the class the analysis must report or None for any) of one entry of FORMS."""
    L = _lib.lib()
    required = None
    if form.startswith("tiled"):
        mgcg_env.setenv("MGCG_TILE_SHIFT", "12")
        mgcg_env.setenv("MGCG_TILE_PACK", form[-1])
        mode, c, required = 1, big_case("tiled"), 4
    elif form == "pb":
        mode, c, required = _lib.COMPRESSION_PB, big_case("pb"), 5
    else:
        mode, c = int(form[4]), case(form[6:])
        required = 3 if form == "mode1-poisson" else None
    hh = Handles()
    L.MgcgSetMatrixCompression(hh.sparse, mode)
    return hh, c, required


def close_form(hh):
    _lib.lib().MgcgAnalysisClear(hh.sparse)
    hh.close()


@pytest.mark.parametrize("form", FORMS)
def test_epilogues_on_the_lossless_forms(oracle, mgcg_env, form):
    """Row patterns and codes (modes 1 and 2), the column tiles (MGCG_TILE_SHIFT = 12: ten tiles of a 40 000-column matrix, with packed and
    with 16-byte entries: tiled_epilogue_kernel) and the propagation-blocking form (pb_pass2_kernel, its late operand fetch for the Jacobi
    epilogues included): all keep the stored order, so the bits are the oracle's; the class is the same after the calls."""
    hh, c, required = open_form(form, mgcg_env)
    acc = row_sums(c, 1, oracle)
    first = None
    for epi in WITHOUT_CHEBYSHEV:
        run_and_check(hh, oracle, c, epi, acc, form, kernel=1)
        cls = analysis_class(hh)
        first = cls if first is None else first
        assert cls == first and (required is None or cls == required), (form, cls, first, required)
    print(form, "class", first)
    if required is None:                                        # the Chebyshev step multiplies through plain CSR whatever the form
        for epi in CHEBYSHEV:
            run_and_check(hh, oracle, c, epi, acc, form, kernel=1)
        assert analysis_class(hh) == first
    close_form(hh)


# --------------------------------------------------------------------------- f. a multiplied vector scaled per gather
SCALED = (1.0 / 6.0, 6.0 / 7.0)


def scaled_row_sums(c, oracle):
    """A (xOuter * (xInner * x)) with the vector formed in NumPy first: inner product rounded, then the outer one."""
    t = SCALED[0] * c.x
    xs = SCALED[1] * t
    assert not np.array_equal(xs, (SCALED[0] * SCALED[1]) * c.x)                    # (one rounded factor would give other bits)
    return oracle.spmv(c.s.Elements, c.s.ColumnIndeces, c.s.RowOffsets, xs)


def test_scaled_x_on_the_row_tile_kernel_and_the_row_pattern_form(h, oracle):
    c = case("poisson")
    acc = scaled_row_sums(c, oracle)
    assert (acc != row_sums(c, 1, oracle)).sum() > c.rows // 2
    hp = Handles()
    _lib.lib().MgcgSetMatrixCompression(hp.sparse, 1)
    for hh, kernel, what in ((h, 10, "kernel 10"), (hp, 0, "row patterns")):
        for rows in [None] + ranges_of(c.rows):
            check(c, EPI_RESIDUAL, acc, run(hh, c, EPI_RESIDUAL, kernel=kernel, scaled=SCALED, rows=rows), f"poisson, scaled x, {what}, rows {rows}", rows=rows)
    assert analysis_class(hp) == 3
    close_form(hp)


# --------------------------------------------------------------------------- g. the early exit
def all_nan(c, got, what):
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all(), (what, np.nonzero(~np.isnan(got[1]))[0][:8], np.nonzero(~np.isnan(got[2]))[0][:8])


@pytest.mark.parametrize("kernel", KERNELS)
def test_done_flag_on_every_kernel(h, oracle, kernel):
    """*done = 1: the pass writes nothing -- y and d (both NaN before the call) stay NaN; *done = 0: the results of a null pointer."""
    nan = np.full(case("ragged").rows, np.nan)
    c = case("ragged")
    acc = row_sums(c, lanes_of(kernel), oracle)
    for epi in EPILOGUES:
        all_nan(c, run(h, c, epi, kernel=kernel, done=1, d0=nan), f"kernel {kernel}, {EPI_NAMES[epi]}, done = 1")
        check(c, epi, acc, run(h, c, epi, kernel=kernel, done=0), f"ragged, {EPI_NAMES[epi]}, kernel {kernel}, done = 0")
    for rows, gap in (((257, 1031), None), (None, (256, 512)), (None, (300, 900))):
        all_nan(c, run(h, c, EPI_JACOBI_DOT, kernel=kernel, done=1, d0=nan, rows=rows, gap=gap), f"kernel {kernel}, rows {rows}, gap {gap}, done = 1")


@pytest.mark.parametrize("form", FORMS)
def test_done_flag_on_the_lossless_forms(oracle, mgcg_env, form):
    hh, c, required = open_form(form, mgcg_env)
    acc = row_sums(c, 1, oracle)
    nan = np.full(c.rows, np.nan)
    for epi in WITHOUT_CHEBYSHEV:
        check(c, epi, acc, run(hh, c, epi, kernel=1, done=0), f"{form}, {EPI_NAMES[epi]}, done = 0")
        all_nan(c, run(hh, c, epi, kernel=1, done=1, d0=nan), f"{form}, {EPI_NAMES[epi]}, done = 1")
    assert required is None or analysis_class(hh) == required
    close_form(hh)


# --------------------------------------------------------------------------- h. non-finite numbers in x
@pytest.mark.parametrize("kernel", [1, 9, 10, 5])
def test_jacobi_sweep_with_poisoned_slots_of_x(h, oracle, kernel):
    """inf, -inf, NaN, the largest finite number and -0.0 in x (block_cases.poison): rows that store none of the poisoned columns stay
    finite -- a masked slot's product is dropped, not multiplied by zero -- the others have NaN exactly where the statement has it."""
    for which in ("poisson", "ragged"):
        c = case(which)
        x = c.x.copy()
        clean = poison(c.s, x, seed=kernel)
        with np.errstate(all="ignore"):
            s = c.s
            acc = (oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, x) if lanes_of(kernel) == 1
                   else lanes_per_row_sum(s.Elements, s.ColumnIndeces, s.RowOffsets, x, lanes_of(kernel)))
            want = epilogue_value(EPI_JACOBI, acc, c.b, c.xo, c.dinv, OMEGA)[0]
        for tune in (None, (64, 0, 1)):
            total, y, d = run(h, c, EPI_JACOBI, kernel=kernel, tune=tune, x=x)
            assert_poisoned_product(y, want, clean)
            assert_same_rows(y, want, c.s.RowOffsets, f"{which}, kernel {kernel}, tuning {tune}, poisoned x")


# --------------------------------------------------------------------------- i. what the entry refuses
REFUSALS = [
    ("epilogue 0", dict(epi=0), "none of the six"),
    ("epilogue 1", dict(epi=1), "none of the six"),
    ("epilogue 5", dict(epi=5), "none of the six"),
    ("epilogue 9", dict(epi=9), "none of the six"),
    ("epilogue -1", dict(epi=-1), "none of the six"),
    ("residual without b", dict(epi=EPI_RESIDUAL, null=("b",)), "null operand"),
    ("residual without x", dict(epi=EPI_RESIDUAL_DOT, null=("x",)), "null operand"),
    ("jacobi without xo", dict(epi=EPI_JACOBI, null=("xo",)), "null operand"),
    ("jacobi without b", dict(epi=EPI_JACOBI_DOT, null=("b",)), "null operand"),
    ("chebyshev without d", dict(epi=EPI_CHEBYSHEV, null=("d",)), "null operand"),
    ("chebyshev without xo", dict(epi=EPI_CHEBYSHEV_DOT, null=("xo",)), "null operand"),
    ("no row offsets", dict(epi=EPI_RESIDUAL, null=("rowOffsets",)), "null operand"),
    ("chebyshev on a range", dict(epi=EPI_CHEBYSHEV, rows=(257, 1031)), "whole matrices only"),
    ("chebyshev with a gap", dict(epi=EPI_CHEBYSHEV_DOT, gap=(256, 512)), "whole matrices only"),
    ("a range and a gap", dict(epi=EPI_JACOBI, rows=(0, 1024), gap=(256, 512)), "bad row selection"),
    ("a range beyond the matrix", dict(epi=EPI_JACOBI, rows=(1, 4421)), "bad row selection"),
    ("an empty range", dict(epi=EPI_JACOBI, rows=(5, 5)), "bad row selection"),
    ("scaled x with the Jacobi sweep", dict(epi=EPI_JACOBI, scaled=SCALED, kernel=10), "MGCG_EPI_RESIDUAL only"),
    ("scaled x with the residual's sum", dict(epi=EPI_RESIDUAL_DOT, scaled=SCALED, kernel=10), "MGCG_EPI_RESIDUAL only"),
    ("scaled x on the stream kernel", dict(epi=EPI_RESIDUAL, scaled=SCALED, kernel=1), "cannot be scaled per gather"),
    ("scaled x on 8 lanes per row", dict(epi=EPI_RESIDUAL, scaled=SCALED, kernel=5), "cannot be scaled per gather"),
    ("scaled x on a misaligned matrix", dict(epi=EPI_RESIDUAL, scaled=SCALED, kernel=10, shift=1), "cannot be scaled per gather"),
    ("y is b", dict(epi=EPI_RESIDUAL, alias="b"), "overlaps an operand"),
    ("y is xo", dict(epi=EPI_JACOBI, alias="xo"), "overlaps an operand"),
    ("y is x", dict(epi=EPI_RESIDUAL_DOT, alias="x"), "overlaps an operand"),
    ("y is d", dict(epi=EPI_CHEBYSHEV, alias="d"), "overlaps an operand"),
]


@pytest.mark.parametrize("name,kw,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_leave_y_untouched(h, name, kw, text):
    c = case("poisson")
    kw = dict(kw)
    total, y, d, message = run(h, c, kw.pop("epi"), refused=True, **kw)
    assert text in message and message.startswith("MgcgCsrMVEpilogue: "), (name, message)
    assert math.isnan(total) and np.isnan(y).all() and np.array_equal(d, c.d), name


def test_scaled_x_is_refused_on_the_code_form():
    """Mode 2 gives the Poisson matrix the per-nonzero code form, whose kernel does not scale x."""
    hh = Handles()
    _lib.lib().MgcgSetMatrixCompression(hh.sparse, 2)
    c = case("poisson")
    total, y, d, message = run(hh, c, EPI_RESIDUAL, scaled=SCALED, refused=True)
    assert "cannot be scaled per gather" in message and math.isnan(total) and np.isnan(y).all(), message
    assert analysis_class(hh) == 2
    close_form(hh)
