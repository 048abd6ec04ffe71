"""Multi-shift CG on the host side (no GPU needed): the library exports SolveShifted and refuses bad arguments with a message before it
asks for a device, the Python class checks its arguments before it touches the library, and the yardstick of tests/test_gpu_shifted.py --
its oracle loop -- is itself checked against numpy's dense solve of every shifted system and against the CPU oracle's plain CG."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems


def test_the_symbol_is_exported_declared_and_bound(hiplib):
    assert hasattr(hiplib, "SolveShifted") and "SolveShifted" in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "MgcgGpu.h")).read()
    assert "int SolveShifted(" in header
    assert hiplib.MgcgAbiVersion() == 3


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    one = (C.c_double * 9)(*([1.0] * 9))
    handle = C.c_void_p(8)                    # never dereferenced: every call below fails on an argument check that comes first

    def call(blas, k, shifts):
        L.MgcgClearLastError()
        st = L.SolveShifted(blas, handle, None, None, None, None, None, None, None, None, None, handle, 10, 5, k, shifts,
                            1e-8, 0, 10, _lib.RULE_NATIVE, None, None, None, None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return st, msg

    assert call(None, 1, one) == (_lib.ERROR, "SolveShifted: null handle")
    for k in (0, 9, -1):
        st, msg = call(handle, k, one)
        assert st == _lib.ERROR and f"k = {k}" in msg
    st, msg = call(handle, 2, None)
    assert st == _lib.ERROR and "NULL" in msg
    for bad in (-1.0, float("nan"), float("inf")):
        st, msg = call(handle, 3, (C.c_double * 3)(0.0, 1.0, bad))
        assert st == _lib.ERROR and "shift 2" in msg, msg


def test_python_class_checks_come_before_the_device(monkeypatch):
    import conjugategradient_amd
    from conjugategradient_amd import shifted

    assert "shifted" in conjugategradient_amd.__all__
    assert issubclass(shifted.ConjugateGradientShiftedGpu, conjugategradient_amd.solver.ConjugateGradientSingleGpu)

    def forbidden(*a, **kw):
        raise AssertionError("the device (library) was touched before the arguments were checked")
    monkeypatch.setattr(shifted, "lib", forbidden)
    monkeypatch.setattr(_lib, "require_gpu", forbidden)
    for bad in ([], [1.0] * 9, [1.0, -2.0], [float("nan")], [float("inf")], [[1.0, 2.0]], "abc", None):
        with pytest.raises(ValueError):
            shifted.ConjugateGradientShiftedGpu(10, 3, bad, 0, 10, 1e-8)
    for count in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            shifted.ConjugateGradientShiftedGpu(count, 3, [1.0], 0, 10, 1e-8)
    assert np.array_equal(shifted.check_shifts([3.0, 0.0, 3.0]), [3.0, 0.0, 3.0])      # repeats and any order are fine


def _dense(s):
    A = np.zeros((s.Count, s.Count))
    for i in range(s.Count):
        for k in range(s.RowOffsets[i], s.RowOffsets[i + 1]):
            A[i, s.ColumnIndeces[k]] += s.Elements[k]
    return A


DENSE_SOLVE_FACTOR = 1.01


@pytest.mark.parametrize("which", ["mgcg_main", "random_spd"])
def test_the_yardstick_solves_every_shifted_system(oracle, which):
    """Every column of the yardstick against np.linalg.solve(A + sigma I, b) on dense SPD systems of <= 300 rows.  The tolerance is derived,
    not guessed: plain oracle CG on the explicitly shifted matrix, stopped by the same rule at the same tolerance, leaves its own distance
    to the dense solution; the yardstick's distance over that one was measured on these two systems and eight shifts each at between 0.99999
    and 1.00006, so the factor is 1.01, asserted with a margin of 2 for the recurrence's drift."""
    from tests.test_gpu_shifted import MAX_IT, from_zero, random_spd, rule_tolerance, shifted_cg_oracle, shifted_system, shifts_for

    s = from_zero(problems.mgcg_main(300)) if which == "mgcg_main" else random_spd(257)
    A = _dense(s)
    assert np.array_equal(A, A.T)
    shifts = shifts_for(s, 8)
    tol = rule_tolerance(s, _lib.RULE_CSHARP)
    ref = shifted_cg_oracle(s, shifts, _lib.RULE_CSHARP, tol)
    assert len({c["iteration"] for c in ref}) >= 2
    for j, sigma in enumerate(shifts):
        exact = np.linalg.solve(A + sigma * np.eye(s.Count), s.b)
        plain = oracle.cg(shifted_system(s, sigma), rule=oracle.RULE_CSHARP, allowable_residual=tol, max_iteration=MAX_IT)
        assert ref[j]["status"] == plain["status"] == _lib.OK and ref[j]["iteration"] == plain["iteration"]
        mine, theirs = np.abs(ref[j]["x"] - exact).max(), np.abs(plain["x"] - exact).max()
        print(which, j, sigma, "yardstick", mine, "plain CG", theirs, "ratio", mine / theirs)
        assert mine <= 2.0 * DENSE_SOLVE_FACTOR * theirs
        assert len(ref[j]["trace"]) == ref[j]["iteration"] + 1 and ref[j]["trace"][-1] == ref[j]["residual"] < tol


@pytest.mark.parametrize("rule", [0, 1, 2, 3, 4])
def test_the_zero_shift_column_is_the_oracle_s_cg_bit_for_bit(oracle, rule):
    from tests.test_gpu_shifted import MAX_IT, from_zero, rule_tolerance, shifted_cg_oracle, shifts_for

    s = from_zero(problems.mgcg_main(300))
    shifts = shifts_for(s, 8)
    tol = rule_tolerance(s, rule)
    ref = shifted_cg_oracle(s, shifts, rule, tol)[shifts.index(0.0)]
    plain = oracle.cg(s, rule=rule, allowable_residual=tol, max_iteration=MAX_IT, trace=True)
    assert plain["iteration"] >= 5 and plain["status"] == _lib.OK
    assert ref["iteration"] == plain["iteration"] and ref["residual"] == plain["residual"] and ref["status"] == plain["status"]
    assert np.array_equal(ref["trace"], plain["trace"]) and np.array_equal(ref["x"], plain["x"])


def test_the_yardstick_on_numpy_primitives_agrees(oracle):
    """The same loop with numpy's dot, product and update (another summation order): the same stopping iterations, the iterates within round-off."""
    from tests.test_gpu_shifted import from_zero, rule_tolerance, shifted_cg_oracle, shifts_for

    s = from_zero(problems.mgcg_main(300))
    A = _dense(s)
    shifts = shifts_for(s, 3)
    tol = rule_tolerance(s, _lib.RULE_CSHARP)
    ref = shifted_cg_oracle(s, shifts, _lib.RULE_CSHARP, tol)
    other = shifted_cg_oracle(s, shifts, _lib.RULE_CSHARP, tol, dot=lambda a, b: float(a @ b), spmv=lambda v: A @ v, set_added=lambda left, right, a: left + a * right)
    for c, o in zip(ref, other):
        assert c["iteration"] == o["iteration"] and math.isclose(c["residual"], o["residual"], rel_tol=1e-6)
        assert np.abs(c["x"] - o["x"]).max() <= 1e-10 * np.abs(c["x"]).max()
