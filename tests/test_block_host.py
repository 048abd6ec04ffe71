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


# --------------------------------------------------------------------------- the matrices of the k-column product's tests
from tests import block_cases as BC      # noqa: E402


def _per_tile(values, n_tiles, fill):
    out = np.full(4 * n_tiles, fill)
    out[: len(values)] = values
    return out.reshape(n_tiles, 4)


@pytest.mark.parametrize("n", [1350, 600_006, 600_134])
def test_ragged_spd_takes_every_path_of_the_block_product(n):
    """Every 64-row span classified by the kernel's own rule.  1350 and 600 134 are 70 mod 256: their last tile has one full wavefront,
    one of 6 rows and two that own no row; 600 006 is 198 mod 256: three full wavefronts and one of 6 rows."""
    s = BC.ragged_spd(n)
    ro = s.RowOffsets.astype(np.int64)
    length = np.diff(ro)
    cls = BC.span_classes(ro)
    n_tiles = (n + 255) // 256
    assert set(cls.tolist()) == {BC.FAST, BC.STAGED_SLOW, BC.UNSTAGED}
    tiles = _per_tile(cls, n_tiles, -1)
    full = tiles[: n // 256]
    assert (full[:, 0] == BC.FAST).all() and (full[:, 1] == BC.STAGED_SLOW).all() and (full[:, 2] == BC.UNSTAGED).all() and (full[:, 3] == BC.FAST).all()
    assert ((tiles == BC.FAST).any(axis=1) & (tiles > BC.FAST).any(axis=1)).any()        # a tile with a fast and a non-fast wavefront (every full one)
    last = tiles[-1]
    assert n % 64 != 0                                                                     # a partly filled wavefront
    assert ((last == -1).sum() >= 1) == (n % 256 == 70), last                              # wavefronts that own no row
    # what every full tile holds
    t = np.arange(n // 256)
    assert (length[np.arange(n) % 256 % BC.LONE_EVERY == BC.LONE_AT] == 1).all()          # the diagonal only
    assert (length[256 * t + BC.HUB_AT] == 9 + t % 32).all()                               # 9 .. 40: the only long row of its span
    second = length[: 256 * len(t)].reshape(-1, 256)[:, 64:128].copy()
    second[:, BC.HUB_AT - 64] = 0
    assert second.max() <= 8
    assert (length[256 * t + BC.LONG_AT] >= 250).all() and length.max() <= 501
    first_and_last = length[: 256 * len(t)].reshape(-1, 256)[:, np.r_[0:64, 192:256]]
    assert first_and_last.max() == 8 and first_and_last.min() == 1 and (first_and_last >= 2).any(axis=1).all()
    c = s.ColumnIndeces
    descending = np.zeros(n, dtype=bool)
    steps = np.diff(c.astype(np.int64))
    inside = np.ones(len(c) - 1, dtype=bool)
    inside[ro[1:-1][ro[1:-1] > 0] - 1] = False                                             # steps from one row to the next
    owner = np.repeat(np.arange(n), length)[:-1]
    descending[np.unique(owner[inside & (steps < 0)])] = True
    i = np.arange(n)
    assert descending[(i % 3 == 1) & (i % 5 != 0) & (length > 1)].all() and not descending[(i % 3 != 1) & (i % 5 != 0)].any()
    assert descending[i % 5 == 0].any() and not descending[(i % 5 == 0) & (length > 2)].all()      # random order
    # symmetric, strictly dominant, a positive diagonal
    A = s.to_scipy()
    assert abs(A - A.T).nnz == 0
    assert BC.strictly_dominant(s)
    assert int(np.abs(c.astype(np.int64) - np.repeat(np.arange(n), length)).max()) > n // 2   # far gathers


def test_streaming_system_has_slow_and_unstaged_spans_and_stays_dominant():
    """The structure at a size the host builds in no time; the positions scale with n, the 8 000 001-row matrix is checked where it is built."""
    s = BC.streaming_system(70_001)
    cls = BC.span_classes(s.RowOffsets)
    assert (cls == BC.UNSTAGED).sum() == 1 and 5 <= (cls == BC.STAGED_SLOW).sum() <= 10 and (cls == BC.FAST).sum() > 1000
    A = s.to_scipy()
    assert abs(A - A.T).nnz == 0 and BC.strictly_dominant(s)


def test_fuzz_seeds_hit_every_k():
    assert {BC.fuzz_k(seed) for seed in range(12)} == set(range(1, 9))
    assert BC.FUZZ_SEEDS >= 8 or "MGCG_FUZZ_SEEDS" in os.environ


def test_oracle_cg_converges_on_ragged_spd_within_the_cap(oracle):
    """The GPU tests run these columns under a cap of 400 iterations: the reference itself is inside it, to a relative 1e-8 (RULE_VIENNACL)
    and to the absolute 1e-8 those tests ask for (RULE_CSHARP), and the columns stop in different iterations."""
    import dataclasses

    s = BC.ragged_spd(1350)
    B, X = BC.columns(s, 8)
    its = []
    for j in range(8):
        sj = dataclasses.replace(s, b=B[j].copy(), x=X[j].copy())
        rel = oracle.cg(sj, rule=oracle.RULE_VIENNACL, allowable_residual=1e-8, max_iteration=400)
        ab = oracle.cg(sj, rule=oracle.RULE_CSHARP, allowable_residual=1e-8, max_iteration=400)
        assert rel["status"] == ab["status"] == oracle.OK and 3 <= rel["iteration"] < 400 and ab["iteration"] < 400, (j, rel["iteration"], ab["iteration"])
        r = sj.b - oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, rel["x"])
        r0 = sj.b - oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, sj.x)
        assert np.linalg.norm(r) <= 2e-8 * np.linalg.norm(r0)
        its.append(ab["iteration"])
    print("iterations", its)
    assert len(set(its)) >= 3 and max(its) >= 2 * min(its)


def test_poison_leaves_at_least_half_of_the_rows_clean(oracle):
    for s in (BC.ragged_spd(1350), problems.poisson(20, 17, 13)):
        x = np.random.default_rng(1).standard_normal(s.Count)
        clean = BC.poison(s, x)
        ref = oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, x)
        assert np.isinf(x[0]) and np.isnan(x).any() and (x == BC.DBL_MAX).sum() == 3 and (np.signbit(x) & (x == 0)).sum() == 3
        BC.assert_poisoned_product(ref, ref, clean)
        with pytest.raises(AssertionError):
            BC.assert_poisoned_product(np.full(s.Count, np.nan), ref, clean)          # y all NaN cannot pass
        leaked = ref.copy()
        leaked[np.nonzero(clean)[0][5]] = np.nan                                       # 0 * inf in one masked slot
        with pytest.raises(AssertionError):
            BC.assert_poisoned_product(leaked, ref, clean)
