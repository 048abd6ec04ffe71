"""Shared-subspace block CG on the host side (no GPU needed): the library exports SolveBlockKrylov and refuses bad arguments with a message
before it asks for a device, the header declares it, the binding has it, and the yardstick of tests/test_gpu_blockkrylov.py solves its
systems in fewer iterations than k separate CGs need."""
import ctypes as C
import os

import numpy as np
import pytest

from conjugategradient_amd import _lib


def test_the_symbol_is_exported_declared_and_bound(hiplib):
    assert hasattr(hiplib, "SolveBlockKrylov") and "SolveBlockKrylov" in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "MgcgGpu.h")).read()
    assert "int SolveBlockKrylov(" in header
    assert hiplib.MgcgAbiVersion() == 3


def test_bad_arguments_are_refused_with_a_message_before_any_device_call(hiplib):
    L = hiplib
    handle = C.c_void_p(8)                    # never dereferenced: every call below fails on an argument check that comes first

    def call(blas, k, rule=_lib.RULE_VIENNACL):
        L.MgcgClearLastError()
        st = L.SolveBlockKrylov(blas, handle, None, None, None, None, None, None, None, None, None, 10, 5, k,
                                1e-8, 0, 10, rule, None, None, None, None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        return st, msg

    assert call(None, 1) == (_lib.ERROR, "SolveBlockKrylov: null handle")
    for k in (0, 9, -1):
        st, msg = call(handle, k)
        assert st == _lib.ERROR and f"k = {k} right-hand sides, must be 1 .. 8" in msg, msg
    st, msg = call(handle, 2, _lib.RULE_HANDMADECL)
    assert st == _lib.ERROR and "max-norm rule" in msg and "not supported" in msg, msg
    st, msg = call(handle, 2, 17)
    assert st == _lib.ERROR and "unknown stop rule 17" in msg, msg


def test_python_class_checks_come_before_the_device(monkeypatch):
    import conjugategradient_amd
    from conjugategradient_amd import block, blockkrylov

    assert "blockkrylov" in conjugategradient_amd.__all__
    assert issubclass(blockkrylov.ConjugateGradientBlockKrylovGpu, block.ConjugateGradientBlockGpu)

    def forbidden(*a, **kw):
        raise AssertionError("the device (library) was touched before the arguments were checked")
    monkeypatch.setattr(blockkrylov, "lib", forbidden)
    monkeypatch.setattr(_lib, "require_gpu", forbidden)
    for k in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError):
            blockkrylov.ConjugateGradientBlockKrylovGpu(10, 3, k, 0, 10, 1e-8)
    with pytest.raises(ValueError, match="max-norm"):
        blockkrylov.ConjugateGradientBlockKrylovGpu(10, 3, 2, 0, 10, 1e-8, rule=_lib.RULE_HANDMADECL)


def test_the_yardstick_shares_the_search_space(oracle):
    """The numpy yardstick on 12^3 Poisson with 8 right-hand sides: every column's true residual meets the tolerance, in fewer iterations than
    the fastest of the oracle's 8 separate CGs, and k = 1 takes exactly the oracle's CG iterations."""
    import dataclasses
    import math

    from conjugategradient_amd import problems
    from tests.test_gpu_blockkrylov import bcgrq_yardstick, columns, true_residuals

    csr = oracle.poisson_csr(12, 12, 12)
    n = len(csr[2]) - 1
    s = problems.poisson(12, 12, 12)
    B, X = columns(n, 8, 5)
    ref = bcgrq_yardstick(csr, B, X)
    assert ref["failed"] is None and (ref["status"] == _lib.OK).all()
    r0 = np.array([math.sqrt(oracle.dot(b, b)) for b in B])
    true = true_residuals(csr, B, ref["x"])
    print("iterations", ref["iteration"], "true / reported", true / ref["residual"])
    assert (true <= 2.0 * ref["residual"]).all() and (ref["residual"] < 1e-8 * r0 * (1.0 + 1e-9)).all()
    single = [oracle.cg(dataclasses.replace(s, b=B[j].copy(), x=X[j].copy()), rule=oracle.RULE_VIENNACL, allowable_residual=1e-8, max_iteration=2000)["iteration"]
              for j in range(8)]
    assert ref["iteration"] < min(single), (ref["iteration"], single)
    one = bcgrq_yardstick(csr, B[:1], X[:1])
    assert one["iteration"] == single[0]
    # a rank-deficient start shows at the first factorisation
    B[3] = 0.0
    bad = bcgrq_yardstick(csr, B, X)
    assert bad["failed"] == (1, 3) and np.array_equal(bad["x"], X)
