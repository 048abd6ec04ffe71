"""Measurement only: what the K-cycle (MgSetCycle(mg, 1, inner)) buys or costs the aggregation multigrid next to the V-cycle OF THE SAME
HIERARCHY in the same process, on one GPU.  Every solve starts from x = 0 with an N(0,1) right-hand side and stops at
|| r || < 1e-8 || b || (the absolute 2-norm rule with that bound) or at the cap.  No figure here is an acceptance threshold.

  poisson256     256^3 7-point Poisson from the device generator                         SolveMg and SolveGmresMg(10)
  permuted128    the 128^3 matrix with rows and columns permuted                         the same
  graph64        the Laplacian of the 64^3 grid graph, weights 10^U(0,3), + 1e-3 I       the same
  upwind256      256^3 convection-diffusion, first-order upwinding, strength="symmetric" SolveGmresMg(10) alone (A != A^T)

Per leg and per passes = 2, 3: one set-up, then the modes V, K with conjugate steps, K with minimal-residual steps switched on that
hierarchy by MgSetCycle.  Reported: rows and entries per level; ms per MgApply (the time of --applies calls, the device drained either
side) beside the bytes the cycle's passes move by the model below and the launches per apply counted from solver.hip's launch sequence;
iterations and seconds to solution under SolveMg and under SolveGmresMg(10, orth 1) -- the second beside the first on a K handle is the
evidence for or against SolveMg's standard beta -- beside SolveEx (SolveGmres(10) on the upwind leg) and the geometric MgSetup of the
same grid where there is one.

The byte model (Jacobi smoother, V(1,1), 4 sweeps on the last level; n rows, z entries of a level; 12 z + 4 n bytes per matrix pass):
  a level with a map:  first sweep 24 n, residual pass (12 z + 4 n) + 24 n, restriction 12 n + 8 n_c, prolongation 20 n + 8 n_c gathered,
                       last sweep (12 z + 4 n) + 40 n                                     = 24 z + 128 n + 16 n_c
  the last level:      24 n + 3 ((12 z + 4 n) + 40 n)
  a K step on C:       two products (12 z + 4 n + 16 n each) and 13 (inner 0) or 11 (inner 1) vectors of 8 n
Under the K-cycle of L + 1 levels the cycle of level l runs 2^l times for 1 <= l < L (two per K step, nested) and 2^(L-1) times on the
last level, and the K step on level l once per cycle of level l - 1.  Launches: a level with a map 5, the last level 4, a K step 6 (two products,
two sums passes, the residual and the combine pass) on top of its two cycles.

Without --leg every leg runs as a child process of its own under a time limit of its own, and the script ends at the first one that fails.

    python -m conjugategradient_amd.tools.kcycle_run --out profiles/kcycle/kcycle_run.json
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

CAP = 2000
M, ORTH = 10, 1
OMEGA_STENCIL = 6.0 / 7.0
LEGS = {"poisson256": 420, "permuted128": 300, "graph64": 300, "upwind256": 420}      # the leg's time limit in seconds
MODES = (("V", 0, 0), ("K_conjugate", 1, 0), ("K_minimal", 1, 1))


def median(v):
    return sorted(v)[len(v) // 2]


def cycle_model(rows, nnz, k, inner):
    """(bytes, launches) of one application by the model of the module's docstring."""
    last = len(rows) - 1
    matrix = [12 * z + 4 * n for n, z in zip(rows, nnz)]
    own_bytes = [2 * matrix[l] + 128 * rows[l] + 16 * rows[l + 1] for l in range(last)] + [24 * rows[last] + 3 * (matrix[last] + 40 * rows[last])]
    times = [1 if (l == 0 or not k) else 2 ** min(l, last - 1) for l in range(len(rows))]      # cycles of level l per application
    total_bytes, launches = 0, 0
    for l in range(len(rows)):
        total_bytes += times[l] * own_bytes[l]
        launches += times[l] * (4 if l == last else 5)
        if k and 1 <= l < last:                       # level l is the C of a K step, which runs once per cycle of level l - 1
            total_bytes += times[l - 1] * (2 * (matrix[l] + 16 * rows[l]) + (11 if inner else 13) * 8 * rows[l])
            launches += times[l - 1] * 6
    return total_bytes, launches


def run_leg(leg, repeats, applies):
    from conjugategradient_amd import _lib, problems
    from conjugategradient_amd.amg import ConjugateGradientAmgGpu
    from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
    from conjugategradient_amd.solver import ApplicationException, VectorDouble
    from conjugategradient_amd.tools.amg_cg_run import permuted_poisson, randn_rhs

    _lib.require_gpu()
    L = _lib.lib()
    symmetric = leg != "upwind256"
    grid = None
    kw = dict(omega=OMEGA_STENCIL)
    if leg == "poisson256":
        n = 256
        grid = (n, n, n)
        cg = ConjugateGradientAmgGpu(n ** 3, 7, 0, CAP, 0.0, passes=2, **kw)
        cg.InitializePoisson(grid)
        bnorm = randn_rhs(cg)
        s = None
    else:
        if leg == "permuted128":
            s = permuted_poisson(128)
        elif leg == "graph64":
            from conjugategradient_amd.tools.gs_smoother_run import graph_laplacian
            s = graph_laplacian(64)
            kw = dict(omega=0.8)
        else:
            s = problems.convection_diffusion(256, 256, 256, (2.0, 1.0, 0.5), upwind=True)
            grid = s.grid
            kw = dict(omega=0.8, strength="symmetric")
        s.b = np.random.default_rng(20261019).standard_normal(s.Count)
        bnorm = float(np.linalg.norm(s.b))
        cg = ConjugateGradientAmgGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, CAP, 0.0, passes=2, **kw).load(s)
        cg.Initialize()
    cg.AllowableResidual = 1e-8 * bnorm
    out = dict(rows=cg.Count, stop_level=cg.AllowableResidual, cap=CAP, m=M, orth=ORTH, omega=kw["omega"])

    def note(key):
        print(json.dumps({leg: {key: out[key]}}), file=sys.stderr, flush=True)

    def solves(obj, solve):
        """`repeats` solves from x = 0 behind one that warms up; the cap and a breakdown are results."""
        samples = []
        for rep in range(repeats + 1):
            L.MgcgFill(obj.vectorX.Ptr, 0.0)
            L.MgcgDeviceSynchronize()
            t0 = time.perf_counter()
            try:
                solve()
            except (ApplicationException, _lib.MgcgError):
                pass
            if rep:
                samples.append(time.perf_counter() - t0)
            L.MgcgClearLastError()
        med = median(samples)
        return dict(status=obj.status, iterations=obj.Iteration, seconds=med, ms_per_iteration=1e3 * med / max(obj.Iteration, 1),
                    residual_over_b=obj.Residual / bnorm, samples_s=samples)

    def both(obj):
        r = dict()
        if symmetric:
            r["SolveMg"] = solves(obj, obj.Solve)
        r["SolveGmresMg"] = solves(obj, lambda: obj.SolveGmres(m=M, orth=ORTH))
        return r

    vr, vz = VectorDouble(cg.Count), VectorDouble(cg.Count)
    vr.CopyFrom(np.random.default_rng(5).standard_normal(cg.Count), cg.Count)

    def apply_ms(mg):
        for rep in range(2):                               # the first round warms up
            L.MgcgDeviceSynchronize()
            t0 = time.perf_counter()
            for _ in range(applies):
                L.MgApply(mg, vr.ToRawPtr(), vz.ToRawPtr())
            L.MgcgDeviceSynchronize()
            ms = 1e3 * (time.perf_counter() - t0) / applies
        _lib.check("MgApply")
        return ms

    for passes in (2, 3):
        cg.passes = passes
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        cg.Setup()
        L.MgcgDeviceSynchronize()
        setup_s = time.perf_counter() - t0
        rows = [int(L.MgLevelRows(cg.mg, l)) for l in range(cg.levels)]
        nnz = [int(L.MgLevelNnz(cg.mg, l)) for l in range(cg.levels)]
        key = f"passes{passes}"
        out[key] = dict(setup_s=setup_s, level_rows=rows, level_nonzeros=nnz, operator_complexity=sum(nnz) / nnz[0])
        for name, cycle, inner in MODES:
            L.MgcgDeviceSynchronize()
            t0 = time.perf_counter()
            if L.MgSetCycle(cg.mg, cycle, inner) != 0:
                _lib.check("MgSetCycle")
            switch_s = time.perf_counter() - t0
            model_bytes, launches = cycle_model(rows, nnz, cycle, inner)
            ms = apply_ms(cg.mg)
            out[key][name] = dict(MgSetCycle_s=switch_s, apply_ms=ms, model_bytes=model_bytes, launches_per_apply=launches,
                                  model_GBps_at_this_time=model_bytes / ms / 1e6, **both(cg))
        v = out[key]["V"]
        for name, _, _ in MODES[1:]:
            k = out[key][name]
            k["to_V"] = dict(apply_ms=k["apply_ms"] / v["apply_ms"], model_bytes=k["model_bytes"] / v["model_bytes"])
            for loop in k:
                if loop.startswith("Solve"):
                    k["to_V"][loop] = dict(iterations=k[loop]["iterations"] / max(v[loop]["iterations"], 1), seconds=k[loop]["seconds"] / v[loop]["seconds"])
        note(key)
    L.MgSetCycle(cg.mg, 0, 0)

    # the comparators of the same process: no preconditioner, and the geometric hierarchy where the matrix has a grid
    def plain():
        it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
        matrix = (cg.cublas, cg.cusparse, cg.matDescr, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                  cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr)
        nz = int(cg.A.RowOffsets[cg.Count]) if cg.A is not None else cg._nnz
        if symmetric:
            cg.status = L.SolveEx(*matrix, nz, cg.Count, cg.AllowableResidual, 0, 20000, _lib.RULE_CSHARP, C.byref(it), C.byref(res), None, 0)
        else:
            cg.status = L.SolveGmres(*matrix, cg.vectorWork.Ptr, M, ORTH, nz, cg.Count, cg.AllowableResidual, 0, 3000, _lib.RULE_CSHARP,
                                     C.byref(it), C.byref(res), C.byref(true), None, 0)
        cg.Iteration, cg.Residual = it.value, res.value

    out["plain"] = {"SolveEx" if symmetric else "SolveGmres": solves(cg, plain)}
    note("plain")
    vr.Dispose()
    vz.Dispose()
    if grid is not None:
        geo = ConjugateGradientMgGpu(cg.Count, 7, 0, CAP, cg.AllowableResidual, grid)
        if s is None:
            geo.InitializePoisson()
            randn_rhs(geo)                                 # the same seed: the same right-hand side
        else:
            geo.load(s)
            geo.Initialize()
        out["geometric"] = dict(level_rows=[int(L.MgLevelRows(geo.mg, l)) for l in range(geo.levels)], **both(geo))
        note("geometric")
        geo.Dispose()
    cg.Dispose()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--leg", choices=list(LEGS), default=None, help="run this leg in this process")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), help="the legs to run, each as a child process under its own time limit")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--applies", type=int, default=20, help="MgApply calls per timing")
    a = ap.parse_args()
    if a.leg:
        result = {a.leg: run_leg(a.leg, a.repeats, a.applies)}
    else:
        result = {}
        for leg in a.legs:
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.kcycle_run", "--leg", leg, "--repeats", str(a.repeats), "--applies", str(a.applies)],
                                   stdout=subprocess.PIPE, timeout=LEGS[leg], check=True)      # a leg that fails or hangs ends the script
            result.update(json.loads(child.stdout))
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
