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
from oracle import oracle as O
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


def _columns(s, k, seed=11):
    """k columns cycling through b = 1, seeded random b, b scaled by 1e-6, b = A x* with a nonzero start x."""
    rng = np.random.default_rng(seed)
    n = s.Count
    B, X = np.zeros((k, n)), np.zeros((k, n))
    for j in range(k):
        kind = j % 4
        if kind == 0:
            B[j] = 1.0 + 0.25 * (j // 4)
        elif kind == 1:
            B[j] = rng.standard_normal(n)
        elif kind == 2:
            B[j] = 1e-6 * (1.0 + 0.5 * rng.random(n))
        else:
            xs = rng.standard_normal(n)
            B[j] = O.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, xs)
            X[j] = rng.standard_normal(n)
    return B, X


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
