"""Block CG (SolveBlockEx, CsrMVBlock, block.ConjugateGradientBlockGpu): k right-hand sides per matrix pass.

Every column of a block solve is the classical CG on that column alone, so under dot_order = 1 (every dot a serial left-to-right sum,
the oracle's arithmetic) each column's trace, iteration, residual, status and iterate must EQUAL the oracle's -- which also catches a
frozen column written after it stopped.  In the default mode only the dot products' summation order differs."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.block import ConjugateGradientBlockGpu
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.solver import ApplicationException, ConjugateGradientSingleGpu, VectorDouble
from tests import block_cases as BC
from tests.gpu_util import Handles, assert_iterate_close, assert_trace_close, cap_inside_a_chunk, dvec, ivec, same_bits, same_under_every_chunking

pytestmark = pytest.mark.gpu

RULES = [("RULE_NATIVE", _lib.RULE_NATIVE), ("RULE_CSHARP", _lib.RULE_CSHARP), ("RULE_SIMPLE", _lib.RULE_SIMPLE),
         ("RULE_HANDMADECL", _lib.RULE_HANDMADECL), ("RULE_VIENNACL", _lib.RULE_VIENNACL)]
TOL = 1e-8
MAX_IT = 400


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def _ragged(n=1337, seed=7):
    """Diagonally dominant, with empty rows and a row count that is no multiple of the 256-row tile."""
    rng = np.random.default_rng(seed)
    rows = [[] for _ in range(n)]
    for i in range(n):
        if i % 11 == 5:
            continue                                    # empty row
        for j in rng.choice(n, size=rng.integers(0, 12), replace=False):
            if j % 11 != 5 and j != i:
                rows[i].append((int(j), -rng.random()))
        rows[i].append((i, 30.0))
    e, c, r = [], [], [0]
    for i in range(n):
        for j, v in rows[i]:
            c.append(j)
            e.append(v)
        r.append(len(c))
    return np.array(e), np.array(c, dtype=np.int32), np.array(r, dtype=np.int32)


@pytest.mark.parametrize("which", ["poisson16", "mgcgmain", "ragged"])
def test_csrmv_block_equals_the_oracle_per_column(oracle, which):
    if which == "poisson16":
        e, c, r = oracle.poisson_csr(16, 16, 16)
    elif which == "mgcgmain":
        e, c, r = oracle.mgcgmain_csr(3000, 160)
        assert np.diff(r).max() > 100
    else:
        e, c, r = _ragged()
        assert (np.diff(r) == 0).any() and (len(r) - 1) % 256 != 0
    n = len(r) - 1
    h = Handles()
    de, dc, dr = dvec(e), ivec(c), ivec(r)
    rng = np.random.default_rng(3)
    L = _lib.lib()
    for k in range(1, 9):
        X = rng.standard_normal((k, n))
        X[0, ::7] = -0.0
        dx, dy = dvec(X.reshape(-1)), dvec(np.full(k * n, np.nan))
        L.CsrMVBlock(h.sparse, h.descr, dy.ToRawPtr(), de.ToRawPtr(), dr.ToRawPtr(), dc.ToRawPtr(), dx.ToRawPtr(), len(e), n, k)
        _lib.check("CsrMVBlock")
        Y = dy.to_numpy(k * n).reshape(k, n)
        for j in range(k):
            assert np.array_equal(Y[j], oracle.spmv(e, c, r, X[j])), (which, k, j)
    h.close()


_columns = BC.columns


def _block(s, k, B, X, rule, max_it=MAX_IT, min_it=0, tol=TOL):
    max_nz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientBlockGpu(s.Count, max_nz, k, min_it, max_it, tol, rule=rule).load(s, B, X)
    cg.Initialize()
    err = None
    try:
        cg.Solve(trace=True)
    except Exception as ex:      # ApplicationException / MgcgError after the per-column results were stored
        err = ex
    cg.Read()
    return cg, err


def _oracle_column(oracle, s, b, x, orule, max_it=MAX_IT, min_it=0, tol=TOL):
    sj = dataclasses.replace(s, b=b.copy(), x=x.copy())
    return oracle.cg(sj, rule=getattr(oracle, orule), allowable_residual=tol, min_iteration=min_it, max_iteration=max_it, trace=True)


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("orule,grule", RULES)
def test_block_equals_the_oracle_bit_for_bit(oracle, dot_order, orule, grule, k):
    s = problems.poisson(12, 12, 12)
    B, X = _columns(s, k)
    cg, err = _block(s, k, B, X, grule)
    assert err is None, err
    for j in range(k):
        ref = _oracle_column(oracle, s, B[j], X[j], orule)
        assert cg.Status[j] == ref["status"] == _lib.OK
        assert cg.Iteration[j] == ref["iteration"], (j, cg.Iteration, ref["iteration"])
        assert cg.Residual[j] == ref["residual"]
        assert np.array_equal(cg.trace[j], ref["trace"]), j
        assert np.array_equal(cg.X[j], ref["x"]), j
    if k > 1:
        assert len(set(cg.Iteration.tolist())) > 1, cg.Iteration     # the columns stop at different iterations


@pytest.mark.parametrize("k", [3, 8])
@pytest.mark.parametrize("orule,grule", RULES)
def test_block_default_mode_within_the_north_star(oracle, orule, grule, k):
    # tolerance 1e-6, as test_gpu_solve's rule variants: at 1e-8 this system runs into the round-off-dominated tail, where the
    # max-norm trace of ANY other summation order of the dots (SolveEx's included) leaves the 1e-10 band
    tol = 1e-6
    s = problems.poisson(12, 12, 12)
    B, X = _columns(s, k, seed=5)
    cg, err = _block(s, k, B, X, grule, tol=tol)
    assert err is None, err
    for j in range(k):
        ref = _oracle_column(oracle, s, B[j], X[j], orule, tol=tol)
        assert cg.Iteration[j] == ref["iteration"], (j, cg.Iteration, ref["iteration"])
        assert cg.Status[j] == _lib.OK
        # (the max-norm residual is one entry of r, not a sum over all of them: its round-off floor lies ~1e-15 below the first value,
        # so its strict band ends earlier)
        assert_trace_close(cg.trace[j], ref["trace"], floor=1e-4 if grule == _lib.RULE_HANDMADECL else 1e-6)
        assert_iterate_close(cg.X[j], ref["x"])


def test_iteration_cap_per_column_and_worst_status(oracle, dot_order):
    s = problems.poisson(12, 12, 12)
    k = 4
    B, X = _columns(s, k)
    free = [_oracle_column(oracle, s, B[j], X[j], "RULE_CSHARP")["iteration"] for j in range(k)]
    cap = sorted(free)[1]                                 # some columns converge within it, others do not
    assert min(free) <= cap < max(free)
    cg, err = _block(s, k, B, X, _lib.RULE_CSHARP, max_it=cap)
    assert isinstance(err, ApplicationException), err
    for j in range(k):
        ref = _oracle_column(oracle, s, B[j], X[j], "RULE_CSHARP", max_it=cap)
        assert cg.Status[j] == ref["status"], j
        assert cg.Iteration[j] == ref["iteration"] and cg.Residual[j] == ref["residual"], j
        assert np.array_equal(cg.X[j], ref["x"]), j
    assert (cg.Status == _lib.MAXIT_EXCEEDED).any() and (cg.Status == _lib.OK).any()
    # the return value is the worst column status (the same solve again from the same start)
    cg.X = X
    cg.Initialize()
    L = _lib.lib()
    st = L.SolveBlockEx(cg.cublas, cg.cusparse, cg.matDescr, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                        cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr,
                        s.nnz, s.Count, k, TOL, 0, cap, _lib.RULE_CSHARP, None, None, None, None, 0)
    L.MgcgClearLastError()
    assert st == _lib.MAXIT_EXCEEDED


def test_breakdown_column_is_isolated(oracle, dot_order):
    s = problems.poisson(12, 12, 12)
    B3, X3 = _columns(s, 3, seed=9)
    B3[1] = 0.0
    X3[1] = 0.0
    cg, err = _block(s, 3, B3, X3, _lib.RULE_NATIVE)
    assert err is not None                                # the b = 0 column breaks down (0 / 0)
    single = ConjugateGradientSingleGpu(s.Count, 7, 0, MAX_IT, TOL, rule=_lib.RULE_NATIVE).load(dataclasses.replace(s, b=B3[1].copy(), x=X3[1].copy()))
    single.Initialize()
    with pytest.raises(_lib.MgcgError):
        single.Solve()
    assert cg.Status[1] == single.status == _lib.NONFINITE
    assert cg.Iteration[1] == single.Iteration
    keep = [0, 2]
    other, err2 = _block(s, 2, B3[keep], X3[keep], _lib.RULE_NATIVE)
    assert err2 is None, err2
    for i, j in enumerate(keep):
        assert cg.Status[j] == other.Status[i] == _lib.OK
        assert cg.Iteration[j] == other.Iteration[i] and cg.Residual[j] == other.Residual[i]
        assert np.array_equal(cg.trace[j], other.trace[i])
        assert np.array_equal(cg.X[j], other.X[i])


def test_full_size_block_equals_single_solves(dot_order):
    """512^3, k = 4, three forced iterations (tolerance 0, min = max = 1: iterations 0, 1, 2): every column equals SolveEx alone."""
    n = 512
    N = n**3
    k = 4
    L = _lib.lib()
    cg = ConjugateGradientRankGpu(N, 7, 0, 10, 1e-8, rank=0, world=1, rule=_lib.RULE_NATIVE)
    cg.InitializePoisson(n, n, n)
    nnz = cg.part.elementCount
    Xb, Bb, Apb, Pb, Rb = (VectorDouble(k * N) for _ in range(5))
    rng = np.random.default_rng(1)
    cols = [1.0, 0.5, None, 1e-6]
    rand = rng.standard_normal(N)
    for j, v in enumerate(cols):
        Bb.CopyFrom(rand if v is None else np.full(N, v), N, 0, j * N)
    it, res, st = np.zeros(k, np.int32), np.zeros(k), np.zeros(k, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    ret = L.SolveBlockEx(cg.cublas, cg.cusparse, cg.matDescr, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                         Xb.Ptr, Bb.Ptr, Apb.Ptr, Pb.Ptr, Rb.Ptr, nnz, N, k, 0.0, 1, 1, _lib.RULE_NATIVE, ptr(it), ptr(res), ptr(st), None, 0)
    L.MgcgClearLastError()
    assert ret == _lib.MAXIT_EXCEEDED and (it == 2).all() and (st == _lib.MAXIT_EXCEEDED).all(), (ret, it, st)
    for v in (Apb, Pb, Rb):
        v.Dispose()
    for j, v in enumerate(cols):
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        if v is None:
            cg.vectorB.CopyFrom(rand, N)
        else:
            L.MgcgFill(cg.vectorB.Ptr, v)
        i1, r1 = C.c_int(0), C.c_double(0)
        s1 = L.SolveEx(cg.cublas, cg.cusparse, cg.matDescr, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                       cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr, nnz, N, 0.0, 1, 1, _lib.RULE_NATIVE,
                       C.byref(i1), C.byref(r1), None, 0)
        L.MgcgClearLastError()
        assert s1 == st[j] and i1.value == it[j] and r1.value == res[j], (j, s1, i1.value, r1.value, res[j])
        got = np.empty(N)
        Xb.CopyTo(got, N, 0, j * N)
        assert np.array_equal(got, cg.vectorX.to_numpy(N)), j
    for v in (Xb, Bb):
        v.Dispose()
    cg.Dispose()


@pytest.mark.parametrize("name,builder,grule", [
    ("ka1_tridiagonal10", lambda: problems.tridiagonal(10), _lib.RULE_SIMPLE),
    ("ka2_rcg21", lambda: problems.mgcg_main(21, 6, 10.0), _lib.RULE_NATIVE),
    ("ka3_mgcgmain2000", lambda: problems.mgcg_main(2000, 160), _lib.RULE_CSHARP),
    ("poisson7_12x12x12", lambda: problems.poisson(12, 12, 12), _lib.RULE_NATIVE),
])
def test_python_class_equals_single_solves_on_golden_systems(dot_order, name, builder, grule):
    from tests.conftest import golden

    g = golden(name)
    s = builder()
    n = s.Count
    max_it = max(2 * n, 50)
    rng = np.random.default_rng(2)
    B = np.stack([s.b, 2.0 * s.b, rng.standard_normal(n)])
    X = np.stack([s.x, s.x, np.zeros(n)])
    max_nz = int(np.diff(s.RowOffsets).max())
    cg = ConjugateGradientBlockGpu(n, max_nz, 3, 0, max_it, TOL, rule=grule).load(s, B, X)
    cg.Initialize()
    cg.Solve(trace=True)
    cg.Read()
    assert cg.Iteration[0] == int(g["iteration"])
    for j in range(3):
        one = ConjugateGradientSingleGpu(n, max_nz, 0, max_it, TOL, rule=grule).load(dataclasses.replace(s, b=B[j].copy(), x=X[j].copy()))
        one.Initialize()
        one.Solve(trace=True)
        one.Read()
        assert cg.Iteration[j] == one.Iteration and cg.Residual[j] == one.Residual and cg.Status[j] == one.status == _lib.OK, j
        assert np.array_equal(cg.trace[j], one.trace), j
        assert np.array_equal(cg.X[j], one.x), j


# --------------------------------------------------------------------------- refusals, and the host's chunking (8^3 Poisson: 512 rows)
def _raw_vectors(s, k, B, X):
    n = s.Count
    return dict(e=dvec(s.Elements[: s.nnz]), ro=ivec(s.RowOffsets), c=ivec(s.ColumnIndeces[: s.nnz]), x=dvec(X.reshape(-1)), b=dvec(B.reshape(-1)),
                Ap=dvec(np.full(k * n, 7.0)), p=dvec(np.full(k * n, 7.0)), r=dvec(np.full(k * n, 7.0)))


def _raw_block(h, v, s, k, rule=_lib.RULE_VIENNACL, **replace):
    """One SolveBlockEx call through the C ABI.  replace: a vector by its key in v (None: a null handle), or count / elementsCount / traceCapacity."""
    cap = MAX_IT + 8
    a = dict(v, count=s.Count, elementsCount=s.nnz, traceCapacity=cap)
    a.update(replace)
    vec = lambda name: None if a[name] is None else a[name].Ptr
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)
    it, res, st, tr = np.full(8, -7, np.int32), np.full(8, -7.0), np.full(8, -7, np.int32), np.zeros(8 * cap)
    L = _lib.lib()
    L.MgcgClearLastError()
    ret = L.SolveBlockEx(h.blas, h.sparse, h.descr, vec("e"), vec("ro"), vec("c"), vec("x"), vec("b"), vec("Ap"), vec("p"), vec("r"),
                         a["elementsCount"], a["count"], k, TOL, 0, MAX_IT, rule, ptr(it), ptr(res), ptr(st), ptr(tr), a["traceCapacity"])
    msg = _lib.last_error()
    L.MgcgClearLastError()
    kk = min(max(k, 0), 8)
    return dict(ret=ret, message=msg, iteration=it[:kk], residual=res[:kk], status=st[:kk],
                trace=[tr[j * cap: j * cap + max(int(it[j]), 0) + 1].copy() for j in range(kk)])


def test_refused_calls_enqueue_nothing_and_leave_the_handles_as_new():
    s = problems.poisson(8, 8, 8)
    k, n = 3, s.Count
    B, X = _columns(s, k)
    h, v = Handles(), _raw_vectors(s, k, B, X)
    smaller = "a device vector is smaller than the problem"
    cases = [(dict(k=0), "k = 0 right-hand sides, must be 1 .. 8"), (dict(k=9), "k = 9 right-hand sides, must be 1 .. 8"),
             (dict(rule=17), "unknown stop rule 17"), (dict(p=None), "null vector handle"), (dict(count=0), "bad sizes"),
             (dict(elementsCount=-1), "bad sizes"), (dict(x=dvec(np.zeros(k * n - 1))), smaller), (dict(ro=ivec(s.RowOffsets[:n])), smaller),
             (dict(traceCapacity=2**30), "trace capacity too large")]          # 3 * 2^30 > 2^31 - 1
    start = {name: v[name].to_numpy(k * n) for name in ("x", "Ap", "p", "r")}
    for kw, word in cases:
        got = _raw_block(h, v, s, kw.pop("k", k), **kw)
        assert got["ret"] == _lib.ERROR and "SolveBlockEx" in got["message"] and word in got["message"], (kw, got["message"])
        for name, was in start.items():
            assert np.array_equal(v[name].to_numpy(k * n), was), (kw, name)       # nothing was enqueued
    after = _raw_block(h, v, s, k)
    h2, v2 = Handles(), _raw_vectors(s, k, B, X)
    fresh = _raw_block(h2, v2, s, k)
    assert after["ret"] == fresh["ret"] == _lib.OK, (after["message"], fresh["message"])
    for key in ("iteration", "residual", "status", "trace"):
        assert same_bits(after[key], fresh[key]), key
    assert same_bits(v["x"].to_numpy(k * n), v2["x"].to_numpy(k * n))
    h.close()
    h2.close()


def _block_results(s, k, B, X, max_it):
    cg, _ = _block(s, k, B, X, _lib.RULE_VIENNACL, max_it=max_it)
    out = dict(x=cg.X, iteration=cg.Iteration, residual=cg.Residual, status=cg.Status, trace=cg.trace)
    cg.Dispose()
    return out


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("k", [1, 3, 8])
def test_chunking_cannot_change_a_result(k, order):
    """check_every = 1, 4, 7: the same bits, also when the iteration cap ends columns in the middle of a chunk."""
    s = problems.poisson(8, 8, 8)
    B, X = _columns(s, k)
    free = same_under_every_chunking(lambda: _block_results(s, k, B, X, MAX_IT), order)
    its = free["iteration"].tolist()
    print("iterations", its)
    assert (free["status"] == _lib.OK).all()
    assert k == 1 or len(set(its)) > 1, its                  # the columns stop in different iterations
    cap = cap_inside_a_chunk(min(its) if k > 1 else 0, max(its))
    capped = same_under_every_chunking(lambda: _block_results(s, k, B, X, cap), order)
    print("cap", cap, "status", capped["status"].tolist())
    assert (capped["status"] == _lib.MAXIT_EXCEEDED).any() and capped["iteration"].max() == cap + 1


# =========================================================================== every path, every k: the k-column product and the passes
# (tests/block_cases.py: ragged_spd mixes the product's fast, staged-slow and unstaged wavefronts in every 256-row tile)
@pytest.fixture(scope="module")
def handles():
    h = Handles()
    yield h
    h.close()


_cases = {}


def ragged(n):
    """ragged_spd(n) and its device copy, built once per module."""
    if n not in _cases:
        s = BC.ragged_spd(n)
        cls = BC.span_classes(s.RowOffsets)
        assert set(cls.tolist()) == {BC.FAST, BC.STAGED_SLOW, BC.UNSTAGED}
        _cases[n] = (s, BC.DeviceBlock(s))
    return _cases[n]


def _assert_product(oracle, s, X, Y, what):
    for j in range(X.shape[0]):
        ref = oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, X[j])
        assert same_bits(Y[j], ref), (what, X.shape[0], j, np.nonzero(Y[j] != ref)[0][:8])


# --------------------------------------------------------------------------- CsrMVBlock (the plain epilogue)
@pytest.mark.parametrize("seed", range(BC.FUZZ_SEEDS))
def test_csrmv_block_random_shapes(handles, oracle, seed):
    """The row-tile kernel's fuzz shapes (test_csrmv_rowtile_random_shapes: the same generator, sizes, densities, empty rows, reversed rows
    and nnz residues) with k = seed mod 8 + 1 columns: every column the oracle's stored-order product, bit for bit."""
    assert BC.FUZZ_SEEDS < 8 or {BC.fuzz_k(i) for i in range(BC.FUZZ_SEEDS)} == set(range(1, 9))      # the seeds of a run hit every k
    s, n, per_row, rng = BC.random_shape(seed)
    k = BC.fuzz_k(seed)
    X = rng.standard_normal((k, n))
    A = BC.DeviceBlock(s)
    _assert_product(oracle, s, X, A.product(handles, X), (seed, n, per_row))
    A.dispose()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257])
def test_csrmv_block_tiny_and_edge_sizes(handles, oracle, n):
    """Below, at and above a wavefront and a tile, for every k, into a y full of NaN; plus a matrix of fewer than 8 entries and one of
    empty rows only, whose product is +0.0 in every bit."""
    import scipy.sparse as sp

    M = (sp.random(n, n, density=min(1.0, 5.0 / n), random_state=n, format="csr") + sp.eye(n, format="csr") * (n % 3 == 0)).tocsr()
    M.sort_indices()
    few = sp.csr_matrix((np.array([2.0, -3.0, 0.5]), (np.array([0, 0, n - 1]), np.array([n - 1, 0, n // 2]))), shape=(n, n))
    few.sum_duplicates()
    none = sp.csr_matrix((n, n))
    rng = np.random.default_rng(n)
    for name, M in (("random", M), ("few", few), ("none", none)):
        s = problems.LinearSystem(M.data.astype(np.float64), M.indices.astype(np.int32), M.indptr.astype(np.int32), np.zeros(n), np.zeros(n), name)
        assert name != "few" or 0 < s.nnz < 8
        assert name != "none" or s.nnz == 0
        A = BC.DeviceBlock(s)
        for k in range(1, 9):
            X = rng.standard_normal((k, n))
            Y = A.product(handles, X)
            _assert_product(oracle, s, X, Y, (name, n))
            if name == "none":
                assert same_bits(Y, np.zeros((k, n)))
        A.dispose()


@pytest.mark.parametrize("n", [1350, 600_006, 600_134])
def test_csrmv_block_on_every_path(handles, oracle, n):
    """ragged_spd, k = 1 .. 8.  1350 rows: six tiles, the last one with two wavefronts that own no row.

    600 006 rows: the tile loop is launched with min(2 * 256 CUs, tiles) = 512 workgroups, so it takes a second trip above
    512 * 256 = 131 072 rows; the passes of the block loop run at most kMaxGrid = 2048 workgroups of 256 threads and stride above
    524 288 rows.  600 006 is past both, even, and 198 mod 256: its last tile (number 2343, the fifth trip of workgroup 295) has three full
    wavefronts and one of 6 rows.  600 134 is the next row count that is 70 mod 256: there the last tile, again on a fifth trip, has two
    wavefronts that own no row."""
    s, A = ragged(n)
    rng = np.random.default_rng(n)
    for k in range(1, 9):
        X = rng.standard_normal((k, n))
        X[0, ::7] = -0.0
        _assert_product(oracle, s, X, A.product(handles, X), n)


@pytest.mark.parametrize("which", ["ragged1351", "grid13x11x5"])
def test_csrmv_block_unaligned_subarrays(handles, oracle, which):
    """The matrix arrays one element, x and y one and two elements into larger vectors (test_csrmv_unaligned_subarrays), with an odd
    count: one element in, columns 0, 2, ... of x and y are 8-byte aligned only; two elements in, columns 1, 3, ... are.  The elements
    around y stay as they were."""
    s = BC.ragged_spd(1351) if which == "ragged1351" else problems.poisson(13, 11, 5)
    n, nnz = s.Count, s.nnz
    assert n % 2 == 1
    L = _lib.lib()
    e = dvec(np.concatenate([[9.0], s.Elements[:nnz]]))
    c = ivec(np.concatenate([[0], s.ColumnIndeces[:nnz]]))
    r = ivec(s.RowOffsets)
    rng = np.random.default_rng(4)
    for k in range(1, 9):
        X = rng.standard_normal((k, n))
        for lead in (1, 2):
            vx, vy = dvec(np.concatenate([np.full(lead, 5.0), X.reshape(-1), [5.0]])), dvec(np.full(k * n + lead + 1, -3.0))
            L.CsrMVBlock(handles.sparse, handles.descr, vy.ToRawPtr() + 8 * lead, e.ToRawPtr() + 8, r.ToRawPtr(), c.ToRawPtr() + 4, vx.ToRawPtr() + 8 * lead,
                         nnz, n, k)
            _lib.check("CsrMVBlock")
            out = vy.to_numpy(k * n + lead + 1)
            assert (out[:lead] == -3.0).all() and out[-1] == -3.0
            _assert_product(oracle, s, X, out[lead:-1].reshape(k, n), (which, lead))
            vx.Dispose()
            vy.Dispose()


@pytest.mark.parametrize("k", range(1, 9))
def test_csrmv_block_drops_the_products_of_masked_slots(handles, oracle, k):
    """inf, -inf and nan in x[0] and in the first stored column of six spans, in every second column of the block (and in the last):
    rows that do not store a poisoned column stay finite -- a masked slot gathers column 0 and must drop the product, 0 * inf is NaN --
    and every column equals the oracle's, NaN where it has NaN.  The other columns of the block stay finite everywhere."""
    s, A = ragged(1350)
    n = s.Count
    X = np.random.default_rng(20 + k).standard_normal((k, n))
    poisoned = sorted(set(range(0, k, 2)) | {k - 1})
    clean = {j: BC.poison(s, X[j], seed=j) for j in poisoned}
    Y = A.product(handles, X)
    for j in range(k):
        ref = oracle.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, X[j])
        if j in clean:
            BC.assert_poisoned_product(Y[j], ref, clean[j])
        else:
            assert np.isfinite(ref).all() and same_bits(Y[j], ref), j


# --------------------------------------------------------------------------- SolveBlockEx: both epilogues and the three passes, every k
_refs = {}
ORDER = [0, 2, 3, 1, 4, 6, 7, 5]


def mixed_columns(s, k, seed=11):
    """The first k of BC.columns' eight in the order b = 1, 1e-6 b, A x* with a start, random b, ...: on the well-conditioned ragged_spd
    b = 1 and a random b stop in the same iteration (the oracle's 21), the scaled column in iteration 8 and the one with a start in 22,
    so that already k = 2 freezes a column long before the other ends."""
    B, X = BC.columns(s, 8, seed=seed)
    return B[ORDER[:k]].copy(), X[ORDER[:k]].copy()


def oracle_columns(oracle, s, B, X, orule, tol=TOL, max_it=MAX_IT, key=None):
    """The oracle's CG on every column, computed once per case (the columns of BC.columns do not depend on k) and never changed."""
    out = []
    for j in range(B.shape[0]):
        kk = (key, s.name, j, orule, tol, max_it)
        if key is None or kk not in _refs:
            ref = _oracle_column(oracle, s, B[j], X[j], orule, max_it=max_it, tol=tol)
            ref["x"].setflags(write=False)
            ref["trace"].setflags(write=False)
            if key is None:
                out.append(ref)
                continue
            _refs[kk] = ref
        out.append(_refs[kk])
    return out


def assert_columns_equal(got_x, iteration, residual, status, traces, refs):
    for j, ref in enumerate(refs):
        assert status[j] == ref["status"], (j, status, ref["status"])
        assert iteration[j] == ref["iteration"], (j, iteration, ref["iteration"])
        assert residual[j] == ref["residual"], j
        assert np.array_equal(traces[j], ref["trace"]), j
        assert np.array_equal(got_x[j], ref["x"]), (j, np.nonzero(got_x[j] != ref["x"])[0][:8])


@pytest.mark.parametrize("k,orule,grule", [(k, "RULE_CSHARP", _lib.RULE_CSHARP) for k in range(1, 9)] +
                         [(2, "RULE_HANDMADECL", _lib.RULE_HANDMADECL), (5, "RULE_HANDMADECL", _lib.RULE_HANDMADECL)])
def test_block_on_every_path_equals_the_oracle_bit_for_bit(oracle, dot_order, k, orule, grule):
    """ragged_spd(1350): the residual and the p.Ap epilogue on fast, staged-slow and unstaged wavefronts and the three passes for every k,
    with columns that stop in different iterations (the frozen-column branches of every K); the max-norm rule is the pass's INF form."""
    s, _ = ragged(1350)
    B, X = mixed_columns(s, k)
    cg, err = _block(s, k, B, X, grule)
    assert err is None, err
    refs = oracle_columns(oracle, s, B, X, orule, key="free")
    assert all(ref["status"] == _lib.OK for ref in refs)
    assert_columns_equal(cg.X, cg.Iteration, cg.Residual, cg.Status, cg.trace, refs)
    print("iterations", cg.Iteration.tolist())
    if k > 1:
        assert len(set(cg.Iteration.tolist())) > 1, cg.Iteration
    cg.Dispose()


@pytest.mark.parametrize("k", [3, 6])
def test_frozen_columns_keep_their_p_and_r(handles, dot_order, k):
    """A column that stopped is written by no kernel again: when the last column ends, the direction p and the residual r of every
    column are the bits that a solve of that column alone leaves behind (the oracle does not show its p and r; the one-column solve is
    held to the oracle above)."""
    s, A = ragged(1350)
    B, X = mixed_columns(s, k)
    got = A.solve(handles, B, X, _lib.RULE_CSHARP, TOL, 0, MAX_IT)
    assert got["ret"] == _lib.OK and len(set(got["iteration"].tolist())) > 1, (got["message"], got["iteration"])
    for j in range(k):
        one = A.solve(handles, B[j: j + 1], X[j: j + 1], _lib.RULE_CSHARP, TOL, 0, MAX_IT)
        assert one["ret"] == _lib.OK and one["iteration"][0] == got["iteration"][j], j
        assert same_bits(one["x"][0], got["x"][j]) and same_bits(one["r"][0], got["r"][j]), j
        assert same_bits(one["p"][0], got["p"][j]), (j, np.nonzero(one["p"][0] != got["p"][j])[0][:8])


@pytest.mark.parametrize("k", [3, 6])
def test_block_second_trips_equal_the_oracle(handles, oracle, dot_order, k):
    """600 006 rows (test_csrmv_block_on_every_path says why), tolerance 0 and a cap of 5: both sides end at the cap.  The tile loop of both
    epilogues and the grid-stride loops of the three passes take further trips, the last one partly filled."""
    s, A = ragged(600_006)
    B, X = mixed_columns(s, k)
    got = A.solve(handles, B, X, _lib.RULE_CSHARP, 0.0, 0, 5)
    assert got["ret"] == _lib.MAXIT_EXCEEDED, got["message"]
    refs = oracle_columns(oracle, s, B, X, "RULE_CSHARP", tol=0.0, max_it=5, key="capped")
    assert all(ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 6 for ref in refs)
    cap = got["cap"]
    traces = [got["trace"][j * cap: j * cap + got["iteration"][j] + 1] for j in range(k)]
    assert_columns_equal(got["x"], got["iteration"], got["residual"], got["status"], traces, refs)


@pytest.mark.parametrize("k", [2, 7])
@pytest.mark.parametrize("n", [1, 2, 63, 65, 257])
def test_block_small_and_odd_sizes_equal_the_oracle(oracle, dot_order, n, k):
    """A dominant tridiagonal of less than a wavefront, one row more than a wavefront, one row more than a tile; odd n: columns 1, 3, ...
    of x, b and r are 8-byte aligned only."""
    from tests.test_gpu_jacobi import tridiagonal

    s, _ = tridiagonal(n)
    B, X = BC.columns(s, k)
    cg, err = _block(s, k, B, X, _lib.RULE_CSHARP)
    assert err is None, err
    refs = oracle_columns(oracle, s, B, X, "RULE_CSHARP")
    assert all(ref["status"] == _lib.OK for ref in refs)
    assert_columns_equal(cg.X, cg.Iteration, cg.Residual, cg.Status, cg.trace, refs)
    cg.Dispose()


def test_a_trace_shorter_than_the_run(handles, oracle, dot_order):
    """Capacity 4 per column: column j's first four entries at trace[4 j ...], nothing beyond 4 k, and a column that stops earlier
    leaves the rest of its own four entries alone."""
    s, A = ragged(1350)
    k, cap = 5, 4
    B, X = mixed_columns(s, k)
    B[4] = np.where(np.arange(s.Count) == 0, 1e-9, 0.0)                     # below the tolerance after its first iteration: stops within the capacity
    refs = oracle_columns(oracle, s, B, X, "RULE_CSHARP")
    used = [min(ref["iteration"] + 1, cap) for ref in refs]
    assert max(ref["iteration"] for ref in refs) + 1 > cap and min(used) < cap, [ref["iteration"] for ref in refs]
    got = A.solve(handles, B, X, _lib.RULE_CSHARP, TOL, 0, MAX_IT, trace_capacity=cap)
    assert got["ret"] == _lib.OK, got["message"]
    tr = got["trace"]
    assert (tr[k * cap:] == -1.0).all()
    for j, ref in enumerate(refs):
        assert np.array_equal(tr[j * cap: j * cap + used[j]], ref["trace"][:cap]), j
        assert (tr[j * cap + used[j]: (j + 1) * cap] == -1.0).all(), j
    assert_columns_equal(got["x"], got["iteration"], got["residual"], got["status"], [ref["trace"] for ref in refs], refs)


@pytest.mark.parametrize("k,orule,grule", [(6, "RULE_CSHARP", _lib.RULE_CSHARP), (5, "RULE_HANDMADECL", _lib.RULE_HANDMADECL)])
def test_garbage_in_the_work_space_does_not_reach_the_result(oracle, mgcg_env, k, orule, grule):
    """NaN in the caller's Ap, p and r.  The partial sums live on the handle's workspace (3 regions of 8 columns of 8192 doubles),
    allocated by the first solve of a new handle: a vector of that size full of NaN is freed just before, which is where the allocator
    usually takes it from (nothing here can check that it did).  dot_order = 1: the oracle's bits; default mode (where the partial sums
    of every workgroup are read): the bits of a solve that started from clean work vectors."""
    s, A = ragged(1350)
    B, X = mixed_columns(s, k)
    nan_space = np.full(3 * 8 * 8192, np.nan)

    def run(garbage):
        h = Handles()
        if garbage is not None:
            dvec(nan_space).Dispose()
        out = A.solve(h, B, X, grule, TOL, 0, MAX_IT, garbage=garbage)
        h.close()
        return out

    clean, dirty = run(None), run(np.nan)
    assert clean["ret"] == dirty["ret"] == _lib.OK, (clean["message"], dirty["message"])
    for key in ("iteration", "residual", "status", "trace", "x"):
        assert same_bits(clean[key], dirty[key]), key
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    got = run(np.nan)
    mgcg_env.delenv("MGCG_DOT_ORDER")
    cap = got["cap"]
    refs = oracle_columns(oracle, s, B, X, orule, key="free")
    assert_columns_equal(got["x"], got["iteration"], got["residual"], got["status"], [got["trace"][j * cap: j * cap + got["iteration"][j] + 1] for j in range(k)], refs)


@pytest.mark.parametrize("k", [2, 5])
def test_block_default_mode_on_every_path(oracle, k):
    """dot_order = 0 at tolerance 1e-6 (test_block_default_mode_within_the_north_star says why), the project's standing tolerances; the
    oracle's own spread over the summation order of its dots (1 .. 4 devices' partial sums) widens the iterate's bound only where it
    exceeds 1e-10, as assert_iterate_close documents."""
    tol = 1e-6
    s, _ = ragged(1350)
    B, X = BC.columns(s, k, seed=5)
    cg, err = _block(s, k, B, X, _lib.RULE_CSHARP, tol=tol)
    assert err is None, err
    for j in range(k):
        print("column", j, "iterations", cg.Iteration[j], "trace", cg.trace[j][:3], cg.trace[j][-2:])
        sj = dataclasses.replace(s, b=B[j].copy(), x=X[j].copy())
        ref = _oracle_column(oracle, s, B[j], X[j], "RULE_CSHARP", tol=tol)
        spread = [oracle.cg_parallel(sj, d, allowable_residual=tol, max_iteration=MAX_IT)["x"] for d in (2, 3, 4)]
        assert cg.Iteration[j] == ref["iteration"], (j, cg.Iteration, ref["iteration"])
        assert cg.Status[j] == _lib.OK
        assert_trace_close(cg.trace[j], ref["trace"])
        print("column", j, "distance, oracle spread", assert_iterate_close(cg.X[j], ref["x"], spread_refs=spread))
    cg.Dispose()


# --------------------------------------------------------------------------- the streaming forms, at the smallest size that takes them
STREAMING_ROWS = 8_000_001       # the product and the block loop's passes take their non-temporal forms from 8 000 000 rows


@pytest.fixture(scope="module")
def streaming():
    """The dominant tridiagonal plus hub rows and one span of more than 512 entries (the unstaged branch has non-temporal loads of its
    own), built and sent to the device once."""
    s = BC.streaming_system(STREAMING_ROWS)
    cls = BC.span_classes(s.RowOffsets)
    assert (cls == BC.UNSTAGED).sum() == 1 and (cls == BC.STAGED_SLOW).sum() >= 5 and BC.strictly_dominant(s)
    A = BC.DeviceBlock(s)
    yield s, A
    A.dispose()


def _streaming_columns(n, k, seed):
    rng = np.random.default_rng(seed)
    B = rng.standard_normal((k, n))
    B[k - 1] *= 1e-3
    return B, np.zeros((k, n))


def test_streaming_product_equals_the_oracle(handles, oracle, streaming):
    s, A = streaming
    X = np.random.default_rng(8).standard_normal((3, s.Count))
    _assert_product(oracle, s, X, A.product(handles, X), "streaming")


@pytest.mark.parametrize("k,orule,grule", [(2, "RULE_HANDMADECL", _lib.RULE_HANDMADECL), (3, "RULE_CSHARP", _lib.RULE_CSHARP)])
def test_streaming_block_solve_equals_the_oracle(handles, oracle, dot_order, streaming, k, orule, grule):
    """Tolerance 0, cap 3: both sides end at the cap."""
    s, A = streaming
    B, X = _streaming_columns(s.Count, k, 80 + k)
    got = A.solve(handles, B, X, grule, 0.0, 0, 3)
    assert got["ret"] == _lib.MAXIT_EXCEEDED, got["message"]
    refs = oracle_columns(oracle, s, B, X, orule, tol=0.0, max_it=3)
    assert all(ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 4 for ref in refs)
    cap = got["cap"]
    assert_columns_equal(got["x"], got["iteration"], got["residual"], got["status"], [got["trace"][j * cap: j * cap + got["iteration"][j] + 1] for j in range(k)], refs)


def test_streaming_gram_product_equals_the_yardstick(handles, oracle, dot_order, streaming):
    """SolveBlockKrylov, k = 2, cap 2 (tolerance 0): the Gram epilogue's non-temporal form."""
    from tests.test_gpu_blockkrylov import bcgrq_yardstick

    s, A = streaming
    k = 2
    B, X = _streaming_columns(s.Count, k, 90)
    ref = bcgrq_yardstick((s.Elements, s.ColumnIndeces, s.RowOffsets), B, X, rule=_lib.RULE_VIENNACL, tol=0.0, max_it=2)
    assert ref["failed"] is None and ref["iteration"] == 3 and (ref["status"] == _lib.MAXIT_EXCEEDED).all()
    got = A.solve(handles, B, X, _lib.RULE_VIENNACL, 0.0, 0, 2, krylov=True)
    assert got["ret"] == _lib.MAXIT_EXCEEDED, got["message"]
    assert got["iteration"] == ref["iteration"]
    assert np.array_equal(got["status"], ref["status"]) and np.array_equal(got["residual"], ref["residual"])
    cap = got["cap"]
    for j in range(k):
        assert np.array_equal(got["trace"][j * cap: j * cap + ref["iteration"] + 1], ref["trace"][j]), j
    assert np.array_equal(got["x"], ref["x"])
