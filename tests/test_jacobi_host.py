"""Jacobi-preconditioned CG on the host side (no GPU needed): the library exports the three entry points and refuses null handles
with a message before it asks for a device, the Python classes import, and the yardstick of tests/test_gpu_jacobi.py -- its oracle
loop -- is itself checked against a plain numpy PCG."""
import ctypes as C

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems


def test_the_three_symbols_are_exported_and_bound(hiplib):
    for name in ("MgcgJacobiSetup", "SolveJacobi", "SolveJacobiParallel"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    assert hiplib.MgcgAbiVersion() == 3


def test_python_surface_imports_without_a_gpu():
    import conjugategradient_amd
    from conjugategradient_amd import frontends, jacobi, parallel

    assert "jacobi" in conjugategradient_amd.__all__
    assert issubclass(jacobi.ConjugateGradientJacobiGpu, conjugategradient_amd.solver.ConjugateGradientSingleGpu)
    assert callable(frontends.ComputerGpu.SolvePreconditioned)
    assert callable(parallel.ConjugateGradientRankGpu.SetupJacobi) and callable(parallel.ConjugateGradientRankGpu.SolveJacobi)


def test_null_handles_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    L.MgcgClearLastError()
    assert L.MgcgJacobiSetup(None, None, None, None, 10, 5, 0, None) == -1
    assert "MgcgJacobiSetup: null handle" in _lib.last_error()
    L.MgcgClearLastError()
    it, res = C.c_int(0), C.c_double(0.0)
    st = L.SolveJacobi(None, None, None, None, None, None, None, None, None, None, None, None, 10, 5, 1e-8, 0, 10, _lib.RULE_NATIVE,
                       C.byref(it), C.byref(res), None, 0)
    assert st == _lib.ERROR and "SolveJacobi: null handle" in _lib.last_error()
    L.MgcgClearLastError()
    st = L.SolveJacobiParallel(None, None, None, None, None, None, None, None, None, None, None, None, None, 10, 5, 0, 10, 0, 9,
                               1e-8, 0, 10, _lib.RULE_NATIVE, C.byref(it), C.byref(res), None, 0)
    assert st == _lib.ERROR and "SolveJacobi: null handle" in _lib.last_error()
    L.MgcgClearLastError()


def test_python_class_checks_come_before_the_device(monkeypatch):
    """Solve() before a successful Initialize() raises without a library call."""
    from conjugategradient_amd import jacobi

    cg = jacobi.ConjugateGradientJacobiGpu.__new__(jacobi.ConjugateGradientJacobiGpu)
    cg._ready = False

    def forbidden(*a, **kw):
        raise AssertionError("the device (library) was touched before the arguments were checked")
    monkeypatch.setattr(jacobi, "lib", forbidden)
    with pytest.raises(_lib.MgcgError, match="Initialize"):
        cg.Solve()


def _numpy_pcg(A, b, x, dinv, tol, max_it):
    """Textbook PCG in plain numpy (dense A): returns (x, loop bodies run)."""
    r = b - A @ x
    z = dinv * r
    p = z.copy()
    rz = r @ z
    for it in range(max_it):
        Ap = A @ p
        alpha = rz / (p @ Ap)
        x = x + alpha * p
        r = r - alpha * Ap
        if np.sqrt(r @ r) < tol:
            return x, it + 1
        z = dinv * r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, max_it


@pytest.mark.parametrize("parts", [None, [0, 40, 40, 97, 150]])
def test_the_oracle_loop_is_a_jacobi_pcg(oracle, parts):
    from tests.test_gpu_jacobi import diagonal_of, jacobi_pcg_oracle

    s = problems.mgcg_main(150)
    n = s.Count
    A = np.zeros((n, n))
    for i in range(n):
        for k in range(s.RowOffsets[i], s.RowOffsets[i + 1]):
            A[i, s.ColumnIndeces[k]] += s.Elements[k]
    d = diagonal_of(s)
    assert np.array_equal(d, np.diag(A)) and d.max() / d.min() > 1.5
    ref = jacobi_pcg_oracle(s, _lib.RULE_NATIVE, 1e-8, parts=parts)
    x, bodies = _numpy_pcg(A, s.b, s.x.copy(), 1.0 / d, 1e-8, 400)
    assert ref["status"] == _lib.OK and ref["iteration"] + 1 == bodies
    assert len(ref["trace"]) == bodies and ref["trace"][-1] == ref["residual"] < 1e-8
    assert np.abs(ref["x"] - x).max() <= 1e-10 * np.abs(x).max()
    assert np.abs(A @ ref["x"] - s.b).max() <= 1e-7
    # the same loop on numpy's primitives (another summation order): the same count, the iterate within round-off
    other = jacobi_pcg_oracle(s, _lib.RULE_NATIVE, 1e-8, parts=parts, dot=lambda a, b: float(a @ b), spmv=lambda v: A @ v,
                              set_added=lambda left, right, a: left + a * right)
    assert other["iteration"] == ref["iteration"]
    assert np.abs(other["x"] - ref["x"]).max() <= 1e-10 * np.abs(x).max()
    # the relative rule divides by the true r0.r0, not by r0.z0
    rel = jacobi_pcg_oracle(s, _lib.RULE_VIENNACL, 1e-6, parts=parts)
    r0 = s.b - A @ s.x
    rk = s.b - A @ rel["x"]
    assert np.sqrt((rk @ rk) / (r0 @ r0)) < 1e-6 and abs(rel["trace"][-1] - np.sqrt((rk @ rk) / (r0 @ r0))) <= 1e-3 * rel["trace"][-1]


@pytest.fixture
def no_device(monkeypatch):
    """Any library call from here on is a test failure: the checks must come first."""
    from conjugategradient_amd import jacobi

    def forbidden(*a, **kw):
        raise AssertionError("the device (library) was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", forbidden)
    monkeypatch.setattr(jacobi, "lib", forbidden)
    monkeypatch.setattr(_lib, "require_gpu", forbidden)


class _FakeVector:
    def __init__(self, size):
        self.size, self.Ptr = size, None


@pytest.mark.parametrize("sizes", [dict(dinv=9), dict(offsets=10), dict(elements=27), dict(columns=27), dict(count=-1)])
def test_setup_wrapper_rejects_vectors_that_are_too_small(no_device, sizes):
    from conjugategradient_amd import jacobi

    count = sizes.get("count", 10)
    with pytest.raises(ValueError):
        jacobi.jacobi_setup(None, _FakeVector(sizes.get("elements", 28)), _FakeVector(sizes.get("offsets", 11)), _FakeVector(sizes.get("columns", 28)),
                            28, count, 0, _FakeVector(sizes.get("dinv", 10)))


def test_setup_wrapper_passes_matching_sizes_on(monkeypatch):
    from conjugategradient_amd import jacobi

    seen = []

    class Lib:
        def MgcgJacobiSetup(self, *a):
            seen.append(a)
            return 0
    monkeypatch.setattr(jacobi, "lib", lambda: Lib())
    jacobi.jacobi_setup("h", _FakeVector(28), _FakeVector(11), _FakeVector(28), 28, 10, 0, _FakeVector(10))
    assert seen == [("h", None, None, None, 28, 10, 0, None)]


@pytest.mark.parametrize("what", ["offsets", "x", "b", "elements", "decreasing", "no_matrix"])
def test_class_rejects_mismatched_shapes_before_the_device(no_device, what):
    from conjugategradient_amd import jacobi
    from conjugategradient_amd.solver import SparseMatrix

    s = problems.tridiagonal(10)
    cg = jacobi.ConjugateGradientJacobiGpu.__new__(jacobi.ConjugateGradientJacobiGpu)
    cg.A, cg.x, cg.b, cg._ready = SparseMatrix.from_system(s), s.x.copy(), s.b.copy(), True
    jacobi.check_system_shapes(cg.A, cg.x, cg.b, 10)                     # the system as it is passes
    if what == "offsets":
        cg.A.RowOffsets = cg.A.RowOffsets[:-1]
    elif what == "x":
        cg.x = np.zeros(11)
    elif what == "b":
        cg.b = np.zeros((10, 1))
    elif what == "elements":
        cg.A.Elements = cg.A.Elements[:-1]
    elif what == "decreasing":
        cg.A.RowOffsets = cg.A.RowOffsets.copy()
        cg.A.RowOffsets[3] = cg.A.RowOffsets[5]
        cg.A.RowOffsets[4] = cg.A.RowOffsets[2]
    else:
        cg.A = None
    with pytest.raises(ValueError):
        cg.Initialize()
    assert cg._ready is False
