"""Measurement only: what the Jacobi-preconditioned loop (SolveJacobi) buys and what it costs, in one session on one GPU.

1. ``problems.viennacl_main()`` at full size (172 835 rows, diagonal 51 .. 1.7e5): SolveEx against SolveJacobi -- loop bodies and wall
   time to the driver's own tolerance (relative 1e-4, MGCG_RULE_VIENNACL) and to an absolute 1e-8 (MGCG_RULE_CSHARP).
2. 512^3 7-point Poisson from the device generator: ms per iteration of both loops.  The diagonal is uniform there, so Jacobi cannot
   help convergence: this run measures only what the loop costs.  Both loops run with tolerance 0 under an iteration cap; the time of
   K1 bodies is subtracted from that of K2 so that the set-up of a call drops out.  The plain loop runs at its default (deferred x
   update in groups of 8) and with ``MgcgSetTuning("x_defer", 1)``; the caps stay below the placement draw's threshold, so neither
   loop draws.  The three forms alternate inside every repeat.

    python -m conjugategradient_amd.tools.jacobi_cg_run --out profiles/jacobi/jacobi_cg_run.json
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python -m conjugategradient_amd.tools.jacobi_cg_run --only jacobi
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import time

import numpy as np

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.jacobi import ConjugateGradientJacobiGpu
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.solver import ApplicationException, ConjugateGradientSingleGpu, VectorDouble


def timed_solve(cls, s, rule, tol, repeats=3):
    maxnz = int(np.diff(s.RowOffsets).max())
    cg = cls(s.Count, maxnz, 0, s.Count, tol, rule=rule).load(s)
    times = []
    for _ in range(repeats + 1):                      # the first solve pays the code-object loads and the matrix analysis
        cg.Initialize()
        _lib.lib().MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        cg.Solve()
        times.append((time.perf_counter() - t0) * 1e3)
    out = dict(loop_bodies=cg.Iteration + 1, residual=cg.Residual, wall_ms_first=times[0], wall_ms=sorted(times[1:])[len(times[1:]) // 2],
               wall_ms_all=times[1:])
    cg.Dispose()
    return out


def driver_matrix():
    s = problems.viennacl_main()
    d = s.Elements[s.RowOffsets[:-1]]                  # the drivers store the diagonal first
    out = dict(rows=s.Count, nnz=int(s.nnz), diagonal_min=float(d.min()), diagonal_max=float(d.max()))
    for name, rule, tol in (("relative_1e-4", _lib.RULE_VIENNACL, 1e-4), ("absolute_1e-8", _lib.RULE_CSHARP, 1e-8)):
        out[name] = dict(plain=timed_solve(ConjugateGradientSingleGpu, s, rule, tol), jacobi=timed_solve(ConjugateGradientJacobiGpu, s, rule, tol))
    return out


def poisson_cost(n, k1, k2, repeats, only=None):
    L = _lib.lib()
    N = n ** 3
    cg = ConjugateGradientRankGpu(N, 7, 0, 10, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE)
    cg.InitializePoisson(n, n, n)
    nnz = cg.part.elementCount
    dinv = VectorDouble(N)
    if L.MgcgJacobiSetup(cg.cusparse, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, nnz, N, 0, dinv.Ptr) != 0:
        _lib.check("MgcgJacobiSetup")
    it, res = C.c_int(0), C.c_double(0.0)

    def run(jacobi, cap):
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        common = (cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr,
                  cg.vectorP.Ptr, cg.vectorR.Ptr)
        tail = (nnz, N, 0.0, 0, cap, _lib.RULE_NATIVE, C.byref(it), C.byref(res), None, 0)
        if jacobi:
            st = L.SolveJacobi(cg.cublas, cg.cusparse, cg.matDescr, *common, dinv.Ptr, *tail)
        else:
            st = L.SolveEx(cg.cublas, cg.cusparse, cg.matDescr, *common, *tail)
        ms = (time.perf_counter() - t0) * 1e3
        L.MgcgClearLastError()
        assert st == _lib.MAXIT_EXCEEDED and it.value == cap + 1, (st, it.value)
        return ms

    forms = (("plain_default", False, None), ("plain_x_defer_1", False, 1), ("jacobi", True, None))

    def select(defer):
        L.MgcgReloadEnvironment()                      # back to the defaults
        if defer is not None:
            assert L.MgcgSetTuning(b"x_defer", defer) == 0

    if only:                                           # one call for a kernel trace
        _, jacobi, defer = next(f for f in forms if f[0] == only)
        select(defer)
        run(jacobi, k1)
        L.MgcgReloadEnvironment()
        dinv.Dispose()
        cg.Dispose()
        return dict(n=n, rows=N, only=only, loop_bodies=k1 + 1)
    samples = {name: [] for name, _, _ in forms}
    for rep in range(repeats + 1):                     # round 0 warms up: code objects, matrix shape, the ring of the deferred x update
        for name, jacobi, defer in forms:              # the forms alternate, so a drift of the machine meets all three alike
            select(defer)
            a, b = run(jacobi, k1), run(jacobi, k2)
            if rep:
                samples[name].append((b - a) / (k2 - k1))
    L.MgcgReloadEnvironment()
    out = dict(n=n, rows=N, nnz=int(nnz), caps=[k1, k2])
    for name, _, _ in forms:
        out[name] = dict(ms_per_iteration=sorted(samples[name])[len(samples[name]) // 2], samples=samples[name])
    out["ratio_to_plain_default"] = out["jacobi"]["ms_per_iteration"] / out["plain_default"]["ms_per_iteration"]
    out["ratio_to_plain_x_defer_1"] = out["jacobi"]["ms_per_iteration"] / out["plain_x_defer_1"]["ms_per_iteration"]
    # from bytes: the product ~104 B/row; vector passes 80 B/row (Jacobi), 64 (plain, x every iteration), 32 + 8 + 8/8 = 56 + 8/8 (deferred x)
    out["byte_ratio_to_plain_x_defer_1"] = (104 + 80) / (104 + 64)
    dinv.Dispose()
    cg.Dispose()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--caps", type=int, nargs=2, default=[20, 120])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-driver", action="store_true")
    ap.add_argument("--only", choices=["plain_default", "plain_x_defer_1", "jacobi"], default=None,
                    help="run only this loop at n^3, once, for caps[0] iterations (for a kernel trace)")
    a = ap.parse_args()
    _lib.require_gpu()
    result = {}
    if not a.skip_driver and not a.only:
        result["viennacl_main"] = driver_matrix()
    result["poisson"] = poisson_cost(a.n, a.caps[0], a.caps[1], a.repeats, a.only)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    try:
        main()
    except ApplicationException as e:
        raise SystemExit(f"a solve ran into its iteration cap: {e}")
