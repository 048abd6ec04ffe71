"""Jacobi-preconditioned CG (MgcgJacobiSetup, SolveJacobi, SolveJacobiParallel, jacobi.ConjugateGradientJacobiGpu,
ComputerGpu.SolvePreconditioned, ConjugateGradientRankGpu.SolveJacobi).

The reference for every comparison is ``jacobi_pcg_oracle`` below: the loop order of oracle_pcg_parts (oracle/mg_oracle.c) written with the
CPU oracle's own primitives -- oracle.spmv, oracle.dot, oracle.set_added carry the reference's serial arithmetic -- with oracle_mg_apply
replaced by z = dinv * r (numpy's element-wise product, dinv = 1.0 / diag) and the library's five stop rules on the TRUE residual
(MGCG_RULE_VIENNACL against the true r0.r0).  ``parts`` cuts every dot at rank boundaries and adds the pieces in rank order.  Under
dot_order = 1 the HIP loop must EQUAL it; in the default mode only the summation order of the dots (and of long rows) differs."""
import math
import threading

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.frontends import ComputerGpu
from conjugategradient_amd.jacobi import ConjugateGradientJacobiGpu
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.solver import ApplicationException, ConjugateGradientSingleGpu
from oracle import oracle as O
from tests.gpu_util import Handles, assert_iterate_close, assert_trace_close, dvec, ivec

pytestmark = pytest.mark.gpu

RULES = [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_HANDMADECL, _lib.RULE_VIENNACL]
MAX_IT = 400


# --------------------------------------------------------------------------- the yardstick
def diagonal_of(s):
    """a_ii = the first stored entry of row i whose column is i."""
    ro, c, e = s.RowOffsets, s.ColumnIndeces, s.Elements
    d = np.zeros(s.Count)
    for i in range(s.Count):
        k = np.nonzero(c[ro[i]: ro[i + 1]] == i)[0]
        d[i] = e[ro[i] + k[0]]
    return d


def stop_decision(rule, tol, min_it, max_it, it, rr_new, inf, rr0):
    """The library's five rules (include/MgcgGpu.h) on the true residual: (residual, shown in the trace, stop, status)."""
    res = inf if rule == _lib.RULE_HANDMADECL else math.sqrt(rr_new)
    shown = res
    if rule == _lib.RULE_NATIVE:
        converged = min_it <= it and res < tol
    elif rule == _lib.RULE_SIMPLE:
        converged = min_it < it and res < tol
    elif rule == _lib.RULE_VIENNACL:
        shown = math.sqrt(rr_new / rr0)
        converged = min_it < it and rr_new / rr0 < tol * tol
    else:
        converged = min_it <= it <= max_it and res < tol
    status, stop = _lib.OK, converged
    if not stop and it >= min_it and it > max_it:
        stop, status = True, _lib.MAXIT_EXCEEDED
    if not stop and not math.isfinite(res):
        stop, status = True, _lib.NONFINITE
    return res, shown, stop, status


def jacobi_pcg_oracle(s, rule=_lib.RULE_CSHARP, tol=1e-8, min_it=0, max_it=MAX_IT, parts=None, dot=None, spmv=None, set_added=None, diag=None):
    """dot / spmv / set_added: the primitives (default: the CPU oracle's; tests/test_jacobi_host.py plugs numpy's in to test this loop).
    diag: the matrix diagonal if the caller knows it (default: diagonal_of(s), a Python loop over the rows)."""
    dot = dot or O.dot
    spmv = spmv or (lambda v: O.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, v))
    set_added = set_added or O.set_added
    parts = [0, s.Count] if parts is None else [int(v) for v in parts]

    def dots(a, b):
        total = 0.0
        for lo, hi in zip(parts[:-1], parts[1:]):
            total += dot(a[lo:hi], b[lo:hi]) if hi > lo else 0.0
        return total

    dinv = 1.0 / (diagonal_of(s) if diag is None else diag)
    x = np.zeros(s.Count) if rule == _lib.RULE_SIMPLE else np.array(s.x, dtype=np.float64)
    r = set_added(np.asarray(s.b, dtype=np.float64), spmv(x), -1.0)
    z = dinv * r
    p = z.copy()
    rz, rr0 = dots(r, z), dots(r, r)
    trace, it = [], 0
    while True:
        Ap = spmv(p)
        alpha = rz / dots(p, Ap)
        x = set_added(x, p, alpha)
        r = set_added(r, Ap, -alpha)
        rr_new = dots(r, r)
        inf = float(np.abs(r).max()) if rule == _lib.RULE_HANDMADECL else 0.0
        res, shown, stop, status = stop_decision(rule, tol, min_it, max_it, it, rr_new, inf, rr0)
        trace.append(shown)
        if stop:
            break
        z = dinv * r
        rz_new = dots(r, z)
        beta = rz_new / rz
        p = set_added(z, p, beta)
        rz = rz_new
        it += 1
    return dict(x=x, iteration=it, residual=res, status=status, trace=np.array(trace))


# --------------------------------------------------------------------------- systems
def scaled_poisson(n=16):
    """S A S for the 7-point Poisson matrix on n^3 cells, S = diag(10^(3 ((i 2654435761) mod 1000) / 999)), b = (S A S) 1."""
    s = problems.poisson(n, n, n)
    i = np.arange(s.Count, dtype=np.uint64)
    S = 10.0 ** (3.0 * ((i * np.uint64(2654435761)) % np.uint64(1000)).astype(np.float64) / 999.0)
    rows = np.repeat(np.arange(s.Count), np.diff(s.RowOffsets))
    e = s.Elements[: s.nnz] * (S[rows] * S[s.ColumnIndeces[: s.nnz]])
    b = O.spmv(e, s.ColumnIndeces[: s.nnz], s.RowOffsets, np.ones(s.Count))
    return problems.LinearSystem(e, s.ColumnIndeces[: s.nnz].copy(), s.RowOffsets.copy(), np.zeros(s.Count), b, f"scaled-poisson{n}", s.grid)


def ragged(n=1337, seed=7):
    """Symmetric, ragged rows (2 .. ~24 entries, unsorted, the diagonal anywhere in the row), a varying positive diagonal that dominates
    its row, no empty rows, a row count that is no multiple of the 256-row tile."""
    rng = np.random.default_rng(seed)
    rows = [dict() for _ in range(n)]
    for i in range(n):
        for j in rng.choice(n, size=rng.integers(1, 12), replace=False):
            j = int(j)
            if j != i:
                v = -rng.random()
                rows[i][j] = v
                rows[j][i] = v
    e, c, r = [], [], [0]
    for i in range(n):
        entries = list(rows[i].items())
        diag = (i, sum(-v for _, v in entries) + 0.5 + 10.0 * rng.random())
        entries.insert(int(rng.integers(0, len(entries) + 1)), diag)
        for j, v in entries:
            c.append(j)
            e.append(v)
        r.append(len(c))
    e, c, r = np.array(e), np.array(c, dtype=np.int32), np.array(r, dtype=np.int32)
    assert n % 256 != 0 and (np.diff(r) > 0).all()
    b = np.cos(np.arange(n) * 0.3) * (1.0 + np.arange(n) % 5)
    return problems.LinearSystem(e, c, r, np.zeros(n), b, "ragged")


def tridiagonal(n):
    """Symmetric tridiagonal, -1 off the diagonal, the diagonal 2.5 + (i mod 7) (strictly dominant), b = cos(0.3 i).  Returns (system, diagonal)."""
    i = np.arange(n)
    cols = np.stack([i - 1, i, i + 1], axis=1)
    diag = 2.5 + (i % 7)
    vals = np.stack([-np.ones(n), diag, -np.ones(n)], axis=1)
    keep = (cols >= 0) & (cols < n)
    ro = np.concatenate([[0], np.cumsum(keep.sum(axis=1))]).astype(np.int32)
    return problems.LinearSystem(vals[keep], cols[keep].astype(np.int32), ro, np.zeros(n), np.cos(0.3 * i), "tridiagonal"), diag


SYSTEMS = {
    "viennacl4000": lambda: problems.viennacl_main(4000),      # diagonal first, columns unsorted
    "mgcgmain3000": lambda: problems.mgcg_main(3000),
    "scaled_poisson16": scaled_poisson,
    "ragged": ragged,
}


def rule_tolerance(s, rule):
    """Absolute rules: 1e-10 of the first residual's size (every system reaches it well inside MAX_IT); the relative rule: 1e-8."""
    if rule == _lib.RULE_VIENNACL:
        return 1e-8
    r0 = s.b - O.spmv(s.Elements, s.ColumnIndeces, s.RowOffsets, np.zeros(s.Count) if rule == _lib.RULE_SIMPLE else s.x)
    return 1e-10 * (np.abs(r0).max() if rule == _lib.RULE_HANDMADECL else math.sqrt(O.dot(r0, r0)))


@pytest.fixture
def dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    yield
    mgcg_env.delenv("MGCG_DOT_ORDER")


def solve(cls, s, rule, tol, min_it=0, max_it=MAX_IT, compression=None):
    """One solve through the Python class; an iteration cap that was hit is a result here, not an exception."""
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = cls(s.Count, maxnz, min_it, max_it, tol, rule=rule).load(s)
    if compression is not None:
        _lib.lib().MgcgSetMatrixCompression(cg.cusparse, compression)
    cg.Initialize()
    try:
        cg.Solve(trace=True)
    except ApplicationException:
        assert cg.status == _lib.MAXIT_EXCEEDED
    cg.Read()
    out = dict(x=cg.x.copy(), iteration=cg.Iteration, residual=cg.Residual, status=cg.status, trace=cg.trace)
    cg.Dispose()
    return out


def assert_equal_runs(got, ref):
    assert got["status"] == ref["status"]
    assert got["iteration"] == ref["iteration"], (got["iteration"], ref["iteration"])
    assert got["residual"] == ref["residual"]
    assert np.array_equal(got["trace"], ref["trace"])
    assert np.array_equal(got["x"], ref["x"])


# --------------------------------------------------------------------------- 1. bit equality with the oracle
@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_solve_jacobi_equals_the_oracle_bit_for_bit(oracle, dot_order, which, rule):
    s = SYSTEMS[which]()
    tol = rule_tolerance(s, rule)
    ref = jacobi_pcg_oracle(s, rule, tol)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 1, ref["iteration"]
    got = solve(ConjugateGradientJacobiGpu, s, rule, tol)
    print(which, rule, "iterations", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"])
    assert_equal_runs(got, ref)


STREAMING_ROWS = 3_000_001      # the smallest row count at which the vector passes take their streaming-hint forms (n > 3 000 000); odd: the tail element runs


@pytest.fixture(scope="module")
def streaming_system():
    return tridiagonal(STREAMING_ROWS)


@pytest.mark.parametrize("rule", [_lib.RULE_CSHARP, _lib.RULE_HANDMADECL])
def test_streaming_hint_forms_equal_the_oracle_bit_for_bit(oracle, dot_order, streaming_system, rule):
    """The r update and the x/p update above 3 M rows (non-temporal loads and stores; under RULE_HANDMADECL also the max-norm form of the r
    update): six forced iterations, tolerance 0, so that both sides stop at the iteration cap."""
    s, diag = streaming_system
    ref = jacobi_pcg_oracle(s, rule, 0.0, min_it=0, max_it=6, diag=diag)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 7, (ref["status"], ref["iteration"])
    got = solve(ConjugateGradientJacobiGpu, s, rule, 0.0, min_it=0, max_it=6)
    print(rule, "iterations", got["iteration"], ref["iteration"], "residual", got["residual"], ref["residual"])
    assert_equal_runs(got, ref)


def test_iteration_cap_equals_the_oracle(oracle, dot_order):
    s = scaled_poisson()
    ref = jacobi_pcg_oracle(s, _lib.RULE_CSHARP, 0.0, max_it=9)
    assert ref["status"] == _lib.MAXIT_EXCEEDED and ref["iteration"] == 10
    assert_equal_runs(solve(ConjugateGradientJacobiGpu, s, _lib.RULE_CSHARP, 0.0, max_it=9), ref)


# --------------------------------------------------------------------------- 2. default mode
@pytest.mark.parametrize("which", list(SYSTEMS))
def test_default_mode_within_the_north_star(oracle, which):
    # the relative rule at 1e-6: the loop stops where assert_trace_close's strict band (residual >= 1e-6 of the first) ends
    s = SYSTEMS[which]()
    ref = jacobi_pcg_oracle(s, _lib.RULE_VIENNACL, 1e-6)
    got = solve(ConjugateGradientJacobiGpu, s, _lib.RULE_VIENNACL, 1e-6)
    print(which, "iterations", got["iteration"], ref["iteration"])
    assert got["status"] == ref["status"] == _lib.OK
    assert abs(got["iteration"] - ref["iteration"]) <= 1
    m = min(len(got["trace"]), len(ref["trace"]))
    assert_trace_close(got["trace"][:m], ref["trace"][:m])
    print(which, "distance", assert_iterate_close(got["x"], ref["x"]))


# --------------------------------------------------------------------------- 3. the feature does its job
def test_jacobi_needs_a_quarter_of_the_plain_iterations_on_the_driver_matrix(oracle):
    s = problems.viennacl_main(4000)
    plain = solve(ConjugateGradientSingleGpu, s, _lib.RULE_CSHARP, 1e-8, max_it=s.Count)
    jac = solve(ConjugateGradientJacobiGpu, s, _lib.RULE_CSHARP, 1e-8, max_it=s.Count)
    print("loop bodies: plain", plain["iteration"] + 1, "jacobi", jac["iteration"] + 1)
    assert plain["status"] == jac["status"] == _lib.OK
    assert 4 * (jac["iteration"] + 1) <= plain["iteration"] + 1


def test_jacobi_converges_on_the_scaled_poisson_where_plain_cg_does_not(oracle):
    s = scaled_poisson()
    ref = jacobi_pcg_oracle(s, _lib.RULE_VIENNACL, 1e-8)
    print("oracle loop bodies", ref["iteration"] + 1)
    assert ref["status"] == _lib.OK and ref["iteration"] + 1 < 200
    jac = solve(ConjugateGradientJacobiGpu, s, _lib.RULE_VIENNACL, 1e-8)
    print("jacobi loop bodies", jac["iteration"] + 1)
    assert jac["status"] == _lib.OK and jac["iteration"] + 1 < 200
    plain = solve(ConjugateGradientSingleGpu, s, _lib.RULE_VIENNACL, 1e-8)
    assert plain["status"] == _lib.MAXIT_EXCEEDED


# --------------------------------------------------------------------------- 4. exact identity
def test_uniform_power_of_two_diagonal_equals_plain_cg_bit_for_bit(dot_order):
    """tridiagonal(512) has the diagonal 2.0: dinv = 0.5 is exact and scaling by a power of two commutes with every rounding of the loop
    (p is half the plain loop's p, alpha twice its alpha, x, r and beta the same)."""
    s = problems.tridiagonal(512)
    assert (diagonal_of(s) == 2.0).all()
    for rule in (_lib.RULE_CSHARP, _lib.RULE_VIENNACL):
        plain = solve(ConjugateGradientSingleGpu, s, rule, 1e-8, max_it=200)
        jac = solve(ConjugateGradientJacobiGpu, s, rule, 1e-8, max_it=200)
        assert plain["iteration"] >= 5
        assert_equal_runs(jac, plain)


# --------------------------------------------------------------------------- 5. set-up rejects what it must
def _with_bad_row(kind, row, n=300):
    s = problems.mgcg_main(n)
    e, c, ro = s.Elements[: s.nnz].copy(), s.ColumnIndeces[: s.nnz].copy(), s.RowOffsets.copy()
    k = int(ro[row] + np.nonzero(c[ro[row]: ro[row + 1]] == row)[0][0])
    if kind == "no_diagonal":
        e, c = np.delete(e, k), np.delete(c, k)
        ro[row + 1:] -= 1
        assert ro[row + 1] > ro[row]
    elif kind == "empty":
        cut = np.arange(ro[row], ro[row + 1])
        e, c = np.delete(e, cut), np.delete(c, cut)
        ro[row + 1:] -= len(cut)
    else:
        e[k] = {"zero": 0.0, "negative": -3.0, "nan": np.nan, "inf": np.inf, "subnormal": 1e-310}[kind]      # (1 / 1e-310 overflows)
    return problems.LinearSystem(e, c, ro, s.x.copy(), s.b.copy(), kind)


@pytest.mark.parametrize("kind", ["no_diagonal", "empty", "zero", "negative", "nan", "inf", "subnormal"])
def test_setup_rejects_rows_without_a_positive_finite_diagonal(kind):
    row = 137
    s = _with_bad_row(kind, row)
    k211 = int(s.RowOffsets[211] + np.nonzero(s.ColumnIndeces[s.RowOffsets[211]: s.RowOffsets[212]] == 211)[0][0])
    s.Elements[k211] = 0.0                               # a second bad row further down: the message names the FIRST
    L = _lib.lib()
    h = Handles()
    de, dc, dr, dd = dvec(s.Elements), ivec(s.ColumnIndeces), ivec(s.RowOffsets), dvec(np.zeros(s.Count))
    L.MgcgClearLastError()
    assert L.MgcgJacobiSetup(h.sparse, de.Ptr, dr.Ptr, dc.Ptr, s.nnz, s.Count, 0, dd.Ptr) == -1
    msg = _lib.last_error()
    print(kind, msg)
    assert f"row {row} " in msg and "211" not in msg
    L.MgcgClearLastError()
    # a dinv vector that is too small is refused before anything runs
    small = dvec(np.zeros(s.Count - 1))
    assert L.MgcgJacobiSetup(h.sparse, de.Ptr, dr.Ptr, dc.Ptr, s.nnz, s.Count, 0, small.Ptr) == -1 and "dinv" in _lib.last_error()
    L.MgcgClearLastError()
    h.close()
    # the Python class raises in Initialize, before any solve ...
    cg = ConjugateGradientJacobiGpu(s.Count, 160, 0, MAX_IT, 1e-8, rule=_lib.RULE_CSHARP).load(s)
    with pytest.raises(_lib.MgcgError, match=f"row {row} "):
        cg.Initialize()
    with pytest.raises(_lib.MgcgError, match="Initialize"):
        cg.Solve()
    cg.Dispose()
    # ... and the library stays usable
    good = problems.mgcg_main(300)
    ref = jacobi_pcg_oracle(good, _lib.RULE_CSHARP, 1e-8)
    got = solve(ConjugateGradientJacobiGpu, good, _lib.RULE_CSHARP, 1e-8)
    assert got["status"] == _lib.OK and abs(got["iteration"] - ref["iteration"]) <= 1


# --------------------------------------------------------------------------- 6. matrix forms
@pytest.mark.parametrize("which", ["poisson12", "mgcgmain3000"])
def test_lossless_matrix_forms_give_the_same_iterate(dot_order, which):
    if which == "poisson12":
        s = problems.poisson(12, 12, 12)
        s.b[:] = np.random.default_rng(3).standard_normal(s.Count)
    else:
        s = SYSTEMS[which]()
    runs = [solve(ConjugateGradientJacobiGpu, s, _lib.RULE_CSHARP, 1e-8, compression=mode)
            for mode in (_lib.COMPRESSION_OFF, _lib.COMPRESSION_BEST, _lib.COMPRESSION_CODES, _lib.COMPRESSION_PB)]
    assert runs[0]["status"] == _lib.OK and runs[0]["iteration"] >= 3
    for other in runs[1:]:
        assert_equal_runs(other, runs[0])


# --------------------------------------------------------------------------- 7. ranks
def run_ranks(world, make_rank, timeout=300):
    """world ranks as host threads on MGCG_VIRTUAL_DEVICES of the one GPU over the loopback transport, under a timeout of their own."""
    L = _lib.lib()
    group = L.MgcgLoopbackCreate(world)
    results, errors = [None] * world, [None] * world

    def body(rank):
        try:
            L.SetDevice(rank)
            comm = L.MgcgCommInitLoopback(group, rank)
            assert comm, _lib.last_error()
            results[rank] = make_rank(rank, comm)
            L.MgcgCommDestroy(comm)
        except BaseException as e:      # noqa: BLE001 -- reported after the join
            errors[rank] = e

    threads = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=timeout)
    assert not any(t.is_alive() for t in threads), "a rank is still blocked in a collective"
    L.MgcgLoopbackDestroy(group)
    for e in errors:
        if e is not None:
            raise e
    return results


def _rank_solve(s, world, rule, tol, max_it=MAX_IT):
    maxnz = int(np.diff(s.RowOffsets).max())

    def make_rank(rank, comm):
        cg = ConjugateGradientRankGpu(s.Count, maxnz, 0, max_it, tol, rank=rank, world=world, comm=comm, rule=rule, device=rank).load(s)
        cg.Initialize()
        cg.SetupJacobi()
        cg.SolveJacobi(trace=True)
        cg.Read()
        p = cg.part
        out = dict(offset=p.offset, count=p.count, x=cg.x[p.offset: p.offset + p.count].copy(), iteration=cg.Iteration, residual=cg.Residual,
                   status=cg.status, trace=cg.trace)
        cg.Dispose()
        return out

    return run_ranks(world, make_rank)


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("which", ["viennacl4000", "scaled_poisson16"])
def test_ranks_equal_the_oracle_with_its_dots_cut_at_their_rows(oracle, mgcg_env, dot_order, world, which):
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s = SYSTEMS[which]()
    rule, tol = (_lib.RULE_CSHARP, rule_tolerance(s, _lib.RULE_CSHARP)) if which == "viennacl4000" else (_lib.RULE_VIENNACL, 1e-8)
    parts = problems.partition_offsets(s.Count, world)
    ref = jacobi_pcg_oracle(s, rule, tol, parts=parts)
    assert ref["status"] == _lib.OK and ref["iteration"] >= 1
    res = _rank_solve(s, world, rule, tol)
    x = np.zeros(s.Count)
    for r in res:
        x[r["offset"]: r["offset"] + r["count"]] = r["x"]
        assert r["status"] == _lib.OK and r["iteration"] == ref["iteration"] and r["residual"] == ref["residual"]
        assert np.array_equal(r["trace"], ref["trace"])
    assert [r["offset"] for r in res] == parts[:-1]
    assert np.array_equal(x, ref["x"])


def test_a_rank_without_rows_takes_part(oracle, mgcg_env, dot_order):
    world = 4
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    s = problems.mgcg_main(3, 160)                      # 3 rows over 4 ranks: offsets [0, 0, 0, 0, 3]
    parts = problems.partition_offsets(s.Count, world)
    assert parts == [0, 0, 0, 0, 3]
    ref = jacobi_pcg_oracle(s, _lib.RULE_CSHARP, 1e-8, max_it=50, parts=parts)
    res = _rank_solve(s, world, _lib.RULE_CSHARP, 1e-8, max_it=50)
    assert [r["count"] for r in res] == [0, 0, 0, 3]
    for r in res:
        assert r["status"] == ref["status"] == _lib.OK and r["iteration"] == ref["iteration"] and r["residual"] == ref["residual"]
    assert np.array_equal(res[3]["x"], ref["x"])


def test_a_set_up_failure_on_one_rank_ends_every_rank_with_an_error(mgcg_env):
    world = 2
    mgcg_env.setenv("MGCG_VIRTUAL_DEVICES", str(world))
    row = 211                                           # of 300 rows: rank 1's
    s = _with_bad_row("zero", row)
    good = problems.mgcg_main(300)

    def make_rank(rank, comm):
        L = _lib.lib()
        cg = ConjugateGradientRankGpu(s.Count, 160, 0, MAX_IT, 1e-8, rank=rank, world=world, comm=comm, device=rank).load(s)
        cg.Initialize()
        msgs = []
        try:
            cg.SetupJacobi()
            msgs.append("set up")
        except _lib.MgcgError as e:
            msgs.append(str(e))
        try:
            cg.SolveJacobi()
            msgs.append("no error")
        except _lib.MgcgError as e:
            msgs.append(str(e))
        msgs.append(cg.status)
        L.MgcgClearLastError()
        cg.Dispose()
        # the same communicator afterwards: a normal solve
        cg = ConjugateGradientRankGpu(good.Count, 160, 0, MAX_IT, 1e-8, rank=rank, world=world, comm=comm, device=rank).load(good)
        cg.Initialize()
        cg.SetupJacobi()
        cg.SolveJacobi()
        msgs.append(cg.Iteration)
        cg.Dispose()
        return msgs

    out = run_ranks(world, make_rank, timeout=120)
    ref = jacobi_pcg_oracle(good, _lib.RULE_CSHARP, 1e-8, parts=problems.partition_offsets(good.Count, world))
    assert out[0][0] == "set up" and f"row {row} " in out[1][0], out
    assert "another rank failed" in out[0][1] and "null handle" in out[1][1], out
    for rank in range(world):
        assert out[rank][2] == _lib.ERROR
        assert abs(out[rank][3] - ref["iteration"]) <= 1


# --------------------------------------------------------------------------- 8. the ViennaCL front-end
def test_computer_gpu_solve_preconditioned(oracle):
    s = problems.viennacl_main(4000)
    ref = jacobi_pcg_oracle(s, _lib.RULE_VIENNACL, 1e-4, max_it=s.Count)
    plain = ComputerGpu(s.Count)
    plain.Write(s.Elements, s.RowOffsets, s.ColumnIndeces, s.x, s.b)
    plain.Solve(1e-4, 0, s.Count)
    cg = ComputerGpu(s.Count)
    cg.Write(s.Elements, s.RowOffsets, s.ColumnIndeces, s.x, s.b)
    cg.SolvePreconditioned(1e-4, 0, s.Count)
    print("loop bodies: plain", plain.Iteration(), "preconditioned", cg.Iteration(), "oracle", ref["iteration"] + 1)
    assert cg.Iteration() == ref["iteration"] + 1
    x = np.empty(s.Count)
    cg.Read(x)
    assert_iterate_close(x, ref["x"])
    plain.Dispose()
    cg.Dispose()


# --------------------------------------------------------------------------- 9. full size
def test_full_size_driver_matrix(oracle):
    s = problems.viennacl_main()
    assert s.Count == 172835
    ref = jacobi_pcg_oracle(s, _lib.RULE_VIENNACL, 1e-6, max_it=s.Count)
    got = solve(ConjugateGradientJacobiGpu, s, _lib.RULE_VIENNACL, 1e-6, max_it=s.Count)
    print("iterations", got["iteration"], ref["iteration"])
    assert got["status"] == ref["status"] == _lib.OK
    assert abs(got["iteration"] - ref["iteration"]) <= 1
    print("distance", assert_iterate_close(got["x"], ref["x"]))
