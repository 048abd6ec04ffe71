"""The deferred x update (knob x_defer, MGCG_X_DEFER): the one-rank unpreconditioned loop applies x += alpha p once per group of B
iterations from a ring of B directions, oldest first -- the same rounded products and sums as one term per iteration.  Every call must
leave the caller exactly the bits of B = 1: x, r, p, Ap, the residual trace, Iteration and Residual, whatever the call's length, where its
groups end, which stop rule ends a solve inside a group and in which order the dots are summed.  Several ranks and MGCG keep B = 1."""
import ctypes as C

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.parallel import ConjugateGradientMgRankGpu, ConjugateGradientRankGpu
from conjugategradient_amd.solver import ApplicationException

pytestmark = pytest.mark.gpu

GROUPS = (2, 3, 4, 8)


def _state(cg):
    n = cg.part.count
    return {"x": cg.vectorX.to_numpy(n), "r": cg.vectorR.to_numpy(n), "p": cg.vectorP.to_numpy(n), "Ap": cg.vectorAp.to_numpy(n)}


def _assert_same(got, want, what):
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k, int((got[k] != want[k]).sum()))


def _steps_run(mgcg_env, defer, n, calls, read_every=True):
    """CgSteps calls on the 7-point n^3 system: (steps, restart) per call; the residual returned and the caller's vectors after each."""
    mgcg_env.setenv("MGCG_X_DEFER", str(defer))
    cg = ConjugateGradientRankGpu(n**3, 7, 0, 10**6, 1e-8, rank=0, world=1)
    cg.InitializePoisson(n, n, n)
    out = []
    for i, (k, restart) in enumerate(calls):
        res = cg.Steps(k, restart=restart)
        out.append((res, _state(cg) if read_every or i == len(calls) - 1 else None))
    cg.Dispose()
    return out


def _compare_runs(base, got, what):
    for i, ((r0, s0), (r1, s1)) in enumerate(zip(base, got)):
        assert r1 == r0, (what, i, r1, r0)
        if s0 is not None:
            _assert_same(s1, s0, (what, i))


# K below B, equal to B, not a multiple of B; restart = False continuations of several lengths (bench.py's form: a short
# restart, then one long continuation)
CALLS = [(3, True), (1, False), (2, False), (8, False), (11, False), (4, False), (5, False), (16, False), (7, True), (9, False)]


@pytest.mark.parametrize("n", [64, 256])
def test_steps_leave_the_bits_of_one_term_per_iteration(mgcg_env, n):
    base = _steps_run(mgcg_env, 1, n, CALLS, read_every=(n == 64))
    for b in GROUPS:
        _compare_runs(base, _steps_run(mgcg_env, b, n, CALLS, read_every=(n == 64)), ("B", b, "n", n))


def test_steps_in_the_reference_dot_order(mgcg_env):
    mgcg_env.setenv("MGCG_DOT_ORDER", "1")
    calls = [(3, True), (5, False), (8, False), (2, False)]
    base = _steps_run(mgcg_env, 1, 32, calls)
    for b in GROUPS:
        _compare_runs(base, _steps_run(mgcg_env, b, 32, calls), ("dot_order 1, B", b))


def test_steps_at_full_size(mgcg_env):
    """The bench's sequence at 512^3 (warm-up restart, one timed continuation), the default group length against B = 1."""
    calls = [(5, True), (20, False)]
    base = _steps_run(mgcg_env, 1, 512, calls, read_every=False)
    v = C.c_int(0)
    mgcg_env.delenv("MGCG_X_DEFER")
    assert _lib.lib().MgcgGetTuning(b"x_defer", C.byref(v)) == 0
    _compare_runs(base, _steps_run(mgcg_env, v.value, 512, calls, read_every=False), ("512^3, B", v.value))


def _solve_run(mgcg_env, defer, n, rule, tol, max_it, min_it=0, dot_order=0):
    mgcg_env.setenv("MGCG_X_DEFER", str(defer))
    mgcg_env.setenv("MGCG_DOT_ORDER", str(dot_order))
    cg = ConjugateGradientRankGpu(n**3, 7, min_it, max_it, tol, rank=0, world=1, rule=rule)
    cg.InitializePoisson(n, n, n)
    status = "ok"
    try:
        cg.Solve(trace=True)
    except ApplicationException:
        status = "maxit"
    out = dict(_state(cg), trace=cg.trace.copy(), it=cg.Iteration, res=cg.Residual, status=status)
    # the caller's p after a stop inside a group is where a continuation reads it from
    res2 = cg.Steps(3, restart=False)
    out["after"] = dict(_state(cg), res=res2)
    cg.Dispose()
    return out


def _compare_solves(base, got, what):
    assert got["status"] == base["status"] and got["it"] == base["it"] and got["res"] == base["res"], (what, got["it"], base["it"])
    assert np.array_equal(got["trace"], base["trace"]), what
    _assert_same(got, {k: base[k] for k in ("x", "r", "p", "Ap")}, what)
    assert got["after"]["res"] == base["after"]["res"], what
    _assert_same(got["after"], {k: base["after"][k] for k in ("x", "r", "p", "Ap")}, (what, "continuation"))


@pytest.mark.parametrize("rule", [_lib.RULE_NATIVE, _lib.RULE_CSHARP, _lib.RULE_SIMPLE, _lib.RULE_HANDMADECL, _lib.RULE_VIENNACL])
def test_solve_stopping_inside_a_group(mgcg_env, rule):
    n = 64
    tol = 1e-6 if rule != _lib.RULE_VIENNACL else 1e-8
    base = _solve_run(mgcg_env, 1, n, rule, tol, 5000)
    inside = 0
    for b in GROUPS:
        got = _solve_run(mgcg_env, b, n, rule, tol, 5000)
        _compare_solves(got, base, ("rule", rule, "B", b))
        inside += (base["it"] + 1) % b != 0
    assert inside > 0                                               # (at least one group length ends the solve inside a group)


def test_solve_stopped_by_the_iteration_cap_and_with_a_minimum(mgcg_env):
    n = 64
    base = _solve_run(mgcg_env, 1, n, _lib.RULE_CSHARP, 1e-30, 13)
    assert base["status"] == "maxit"
    for b in GROUPS:
        _compare_solves(_solve_run(mgcg_env, b, n, _lib.RULE_CSHARP, 1e-30, 13), base, ("maxit, B", b))
    base = _solve_run(mgcg_env, 1, n, _lib.RULE_NATIVE, 1e300, 5000, min_it=6)          # stops exactly at the minimum
    for b in GROUPS:
        _compare_solves(_solve_run(mgcg_env, b, n, _lib.RULE_NATIVE, 1e300, 5000, min_it=6), base, ("minimum, B", b))


def test_solve_in_the_reference_dot_order(mgcg_env):
    base = _solve_run(mgcg_env, 1, 24, _lib.RULE_NATIVE, 1e-8, 5000, dot_order=1)
    for b in GROUPS:
        _compare_solves(_solve_run(mgcg_env, b, 24, _lib.RULE_NATIVE, 1e-8, 5000, dot_order=1), base, ("dot_order 1, B", b))


def test_several_ranks_and_multigrid_keep_one_term_per_iteration(mgcg_env, capfd):
    """The set-up report (MGCG_VERBOSE=2) names the group length where the ring is used: the one-rank loop, not the several-ranks path of
    a one-rank communicator (MGCG_FORCE_MULTIRANK) nor the preconditioned loop -- and those give the same bits under every x_defer."""
    L = _lib.lib()
    L.SetDevice(0)
    n = 32
    mgcg_env.setenv("MGCG_VERBOSE", "2")
    mgcg_env.setenv("MGCG_X_DEFER", "4")
    capfd.readouterr()
    cg = ConjugateGradientRankGpu(n**3, 7, 0, 2000, 1e-8, rank=0, world=1)
    cg.InitializePoisson(n, n, n)
    cg.Solve()
    cg.Dispose()
    assert "deferred x update in groups of 4" in capfd.readouterr().err

    buf = (C.c_char * 128)()
    assert L.MgcgCommGetUniqueId(buf) == 0, _lib.last_error()
    comm = L.MgcgCommInitRank(buf, 1, 0)
    assert comm, _lib.last_error()
    mgcg_env.setenv("MGCG_FORCE_MULTIRANK", str(n * n))
    mgcg_env.setenv("MGCG_OVERLAP", "0")
    got = []
    for b in (1, 4):
        mgcg_env.setenv("MGCG_X_DEFER", str(b))
        capfd.readouterr()
        cg = ConjugateGradientRankGpu(n**3, 7, 0, 2000, 1e-8, rank=0, world=1, comm=comm)
        cg.InitializePoisson(n, n, n)
        cg.Solve(trace=True)
        res = cg.Steps(5, restart=False)
        got.append((dict(_state(cg), trace=cg.trace.copy(), it=cg.Iteration, res=cg.Residual, res2=res)))
        cg.Dispose()
        mg = ConjugateGradientMgRankGpu(n**3, 7, 0, 400, 1e-8, (n, n, n), rank=0, world=1, comm=comm, levels=3)
        mg.InitializePoisson(n, n, n)
        mg.Setup()
        mg.Solve()
        mg.Read()
        got[-1]["mg_x"], got[-1]["mg_it"] = mg.x.copy(), mg.Iteration
        mg.Dispose()
        assert "deferred x update" not in capfd.readouterr().err, b
    L.MgcgCommDestroy(comm)
    a, b = got
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    mgcg_env.setenv("MGCG_FORCE_MULTIRANK", "0")
    capfd.readouterr()
    mg = ConjugateGradientMgRankGpu(n**3, 7, 0, 400, 1e-8, (n, n, n), rank=0, world=1, levels=3)
    mg.InitializePoisson(n, n, n)
    mg.Setup()
    mg.Solve()
    mg.Dispose()
    assert "deferred x update" not in capfd.readouterr().err
