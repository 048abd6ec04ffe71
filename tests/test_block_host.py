"""Block CG on the host side (no GPU needed): the Python wrapper refuses bad k and shapes before it touches the device, and the
library's SolveBlockEx fails loudly on a host without a device."""
import os

import numpy as np
import pytest

from conjugategradient_amd import _lib, block, problems


@pytest.fixture
def no_device(monkeypatch):
    """Any library call from here on is a test failure: the checks must come first."""
    def forbidden(*a, **kw):
        raise AssertionError("the device (library) was touched before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", forbidden)
    monkeypatch.setattr(block, "lib", forbidden)
    monkeypatch.setattr(_lib, "require_gpu", forbidden)


@pytest.mark.parametrize("k", [0, 9, -1, 2.0, True])
def test_wrapper_rejects_k_outside_1_to_8(no_device, k):
    with pytest.raises(ValueError):
        block.ConjugateGradientBlockGpu(10, 3, k, 0, 10, 1e-8)
    with pytest.raises(ValueError):
        block.CsrMVBlock(None, 0, 0, 0, 0, 0, 0, 10, k)


@pytest.mark.parametrize("shape", [(3, 10), (2, 11), (20,), (2, 10, 1)])
def test_wrapper_rejects_mismatched_shapes(no_device, shape):
    s = problems.tridiagonal(10)
    with pytest.raises(ValueError):
        block.check_block(np.zeros(shape), 2, s.Count, "B")
    assert block.check_block(np.zeros((2, 10)), 2, s.Count, "B").shape == (2, 10)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="this check is for hosts without a GPU")
def test_solve_block_without_a_device_is_an_error(hiplib):
    L = hiplib
    L.MgcgClearLastError()
    it, res, st = np.zeros(2, np.int32), np.zeros(2), np.zeros(2, np.int32)
    ptr = lambda a: a.ctypes.data_as(_lib.C.c_void_p)
    ret = L.SolveBlockEx(None, None, None, None, None, None, None, None, None, None, None, 10, 5, 2, 1e-8, 0, 10, _lib.RULE_NATIVE,
                         ptr(it), ptr(res), ptr(st), None, 0)
    assert ret == _lib.ERROR
    assert "no HIP device" in _lib.last_error()
    L.MgcgClearLastError()
    x = np.ones(10)
    L.CsrMVBlock(None, None, ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), 1, 5, 2)
    assert _lib.last_error()
    L.MgcgClearLastError()
