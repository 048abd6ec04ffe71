"""Helpers shared by the -m gpu tests: everything goes through the C ABI."""
import contextlib
import ctypes as C

import numpy as np

from conjugategradient_amd import _lib
from conjugategradient_amd.solver import VectorDouble, VectorInt


class Handles:
    def __init__(self):
        L = _lib.lib()
        _lib.require_gpu()
        L.SetDevice(0)
        self.blas = L.CreateBlas()
        self.sparse = L.CreateSparse()
        self.descr = L.CreateMatDescr()
        _lib.check("handles")
        assert self.blas and self.sparse and self.descr

    def close(self):
        L = _lib.lib()
        L.DestroyBlas(self.blas)
        L.DestroySparse(self.sparse)
        L.DestroyMatDescr(self.descr)


def dvec(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    v = VectorDouble(max(a.shape[0], 1))
    if a.shape[0]:
        v.CopyFrom(a, a.shape[0])
    return v


def ivec(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    v = VectorInt(max(a.shape[0], 1))
    if a.shape[0]:
        v.CopyFrom(a, a.shape[0])
    return v


@contextlib.contextmanager
def tuning(**knobs):
    """Library knobs (MgcgSetTuning names) set for the block's duration and put back in a finally."""
    L = _lib.lib()
    old = {}
    try:
        for name, value in knobs.items():
            was = C.c_int(0)
            assert L.MgcgGetTuning(name.encode(), C.byref(was)) == 0, name
            old[name] = was.value
            assert L.MgcgSetTuning(name.encode(), value) == 0, name
        yield
    finally:
        for name, value in old.items():
            L.MgcgSetTuning(name.encode(), value)


@contextlib.contextmanager
def library_messages():
    """The messages the library left on this thread during the block, whole and in order.  The Python classes consume a message before
    they raise -- they clear it when an iteration cap was hit, and put it behind "Export: " in their MgcgError otherwise -- so each one is
    recorded on its way out, when it is cleared."""
    L = _lib.lib()
    seen, clear = [], L.MgcgClearLastError

    def recording_clear():
        if _lib.last_error():
            seen.append(_lib.last_error())
        clear()

    L.MgcgClearLastError = recording_clear
    try:
        yield seen
    finally:
        L.MgcgClearLastError = clear


def maxit_message(who, run, max_it, residual="residual", norm=""):
    """The library's message of a run that met its iteration cap, rebuilt from what the run returned (%g, as the library prints it)."""
    return "%s: did not converge: iteration %d exceeded maxIteration %d (%s %g%s)" % (who, run["iteration"], max_it, residual, run["residual"], norm)


def nonfinite_message(who, run, what):
    """The library's message of a run that ended with NONFINITE; what: the loop's own text of what that means."""
    return "%s: stopped at iteration %d: %s" % (who, run["iteration"], what)


def same_bits(a, b):
    """Equal bit for bit (NaN payloads and the sign of zero included); lists and tuples entry by entry."""
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_bits(p, q) for p, q in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


CHECK_EVERY = (1, 4, 7)


def same_under_every_chunking(run, dot_order):
    """run() -> dict of results.  How many iterations the host enqueues ahead of the stop flag (knob check_every) must not change one bit
    of them; returns the results."""
    runs = []
    for every in CHECK_EVERY:
        with tuning(check_every=every, dot_order=dot_order):
            runs.append(run())
    for every, other in zip(CHECK_EVERY[1:], runs[1:]):
        assert other.keys() == runs[0].keys()
        for key in runs[0]:
            assert same_bits(other[key], runs[0][key]), (key, every, other[key], runs[0][key])
    return runs[0]


def cap_inside_a_chunk(lowest, highest):
    """An iteration cap in [0, highest) near the middle of [lowest, highest] whose stopping iteration (index cap + 1, the cap + 2nd enqueued) is
    the last of a chunk under neither check_every = 4 nor 7."""
    cap = next(c for c in range((lowest + highest) // 2, -1, -1) if (c + 2) % 4 and (c + 2) % 7)
    assert cap < highest, (lowest, highest)
    return cap


class DeviceCsr:
    def __init__(self, system):
        self.s = system
        self.e, self.c, self.r = dvec(system.Elements[: system.nnz]), ivec(system.ColumnIndeces[: system.nnz]), ivec(system.RowOffsets)

    def spmv(self, h, x, alpha=1.0, beta=0.0, y0=None, kernel=None, tuning=None, cols=None, period=0, tile=(0, 0)):
        L = _lib.lib()
        n = self.s.Count
        vx = dvec(x)
        vy = dvec(np.zeros(n) if y0 is None else y0)
        if kernel is not None:
            L.MgcgSetSpmvKernel(h.sparse, kernel)
        if tuning is not None:
            L.MgcgSetSpmvTuning(h.sparse, *tuning)
        L.MgcgSetSpmvPeriod(h.sparse, period)
        L.MgcgSetSpmvTile(h.sparse, *tile)
        L.CsrMV(h.sparse, h.descr, vy.ToRawPtr(), self.e.ToRawPtr(), self.r.ToRawPtr(), self.c.ToRawPtr(), vx.ToRawPtr(),
                self.s.nnz, n, n if cols is None else cols, alpha, beta)
        _lib.check("CsrMV")
        out = vy.to_numpy(n)
        L.MgcgSetSpmvKernel(h.sparse, 0)
        L.MgcgSetSpmvTuning(h.sparse, 64, 0, 0)
        L.MgcgSetSpmvPeriod(h.sparse, 0)
        L.MgcgSetSpmvTile(h.sparse, 0, 0)
        return out


def assert_trace_close(actual, desired, strict=1e-10, loose=1e-3, floor=1e-6):
    """Per-iteration residuals of the GPU loop vs the oracle.  The loops differ only in the summation
    order of the dot products (1e-16 relative per dot); CG amplifies that as the residual falls, so the
    north-star tolerance (1e-10 relative) is demanded while the residual is above `floor` * its first
    value and a loose bound below it (round-off dominated region)."""
    actual, desired = np.asarray(actual), np.asarray(desired)
    assert len(actual) == len(desired) and len(actual) > 0, (len(actual), len(desired))
    hi = desired >= floor * desired[0]
    np.testing.assert_allclose(actual[hi], desired[hi], rtol=strict)
    # round-off region: relative to the size of the problem, not to a residual that is itself noise
    np.testing.assert_allclose(actual[~hi], desired[~hi], rtol=loose, atol=1e-12 * desired[0])


def assert_iterate_close(x, ref_x, spread_refs=(), rtol=1e-10):
    """The north star's iterate tolerance: max |x - x_oracle| <= 1e-10 * max |x_oracle|.  Where a test runs deep into the round-off-dominated
    tail of CG (forced iterations, a chaotic random system), the ORACLE itself moves by more than that when only the summation order of
    its dot products changes; such a test passes `spread_refs` -- the same oracle loop's x with other device counts (resultsDot.Sum() over
    1 .. n devices, ConjugateGradientParallelGpu.cs:463,499,525) -- and the HIP loop must then lie within 1.5 x the largest distance between
    those oracles and `ref_x`.  The spread is computed and asserted here, never assumed.  Returns (distance, spread)."""
    x, ref_x = np.asarray(x), np.asarray(ref_x)
    scale = np.abs(ref_x).max()
    distance = np.abs(x - ref_x).max() / scale
    spread = max((np.abs(np.asarray(r) - ref_x).max() / scale for r in spread_refs), default=0.0)
    assert distance <= max(rtol, 1.5 * spread), (distance, spread)
    return distance, spread
