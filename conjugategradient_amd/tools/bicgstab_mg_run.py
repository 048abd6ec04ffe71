"""Measurement only: what the V-cycle buys BiCGStab (SolveBicgstabMg against SolveBicgstab), on one GPU.  Every run starts from x = 0 with
an N(0,1) right-hand side and stops at || r || < 1e-8 || b || (MGCG_RULE_NATIVE) or at the cap of 20 000 bodies.  No figure here is an
acceptance threshold.

  central_mild     256^3 convection_diffusion, c = (.5, .25, 0)
  central_strong   256^3 convection_diffusion, c = (.9, .9, .9)
  upwind           256^3 convection_diffusion, c = (2, 1, .5), first-order upwinding

Per leg, on one copy of the matrix: SolveBicgstab, and SolveBicgstabMg with the geometric hierarchy of the matrix itself (MgSetup), the
geometric hierarchy of problems.symmetric_part (a second object, handed over through hierarchy=) and the aggregation hierarchy of the
matrix itself (MgSetupAggregation, the class's defaults) -- bodies, ms per body (time of the call / bodies run), seconds to solution, the
set-up's seconds (the hierarchy alone: the matrix is on the device already) and seconds to solution including set-up, TrueResidual beside
Residual.  One solve warms up, the median of --repeats follows.

Without --leg every leg runs as a child process of its own under a time limit of its own, and the script ends at the first one that fails.

Byte model per row at 7 entries per row, stated, not measured: the product ~104; the plain passes 24 + 8 + 56 + 32 = 120, two products: 328
per body; the V-cycle form's passes 24 + 8 + 64 + 32 = 128, two products and two cycles: 336 + two cycles per body.

    python -m conjugategradient_amd.tools.bicgstab_mg_run --out profiles/bicgstab_mg/bicgstab_mg_run.json
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

BYTES = {"product": 104, "bicgstab_s_kernel": 24, "bicgstab_tau_kernel": 8, "bicgstab_x_kernel": 64, "bicgstab_p_kernel": 32,
         "passes": 128, "plain_passes": 120, "jacobi_passes": 160, "body_without_the_cycles": 336, "plain_body": 328}
MAX_IT = 20000
STENCILS = {"central_mild": ((0.5, 0.25, 0.0), False), "central_strong": ((0.9, 0.9, 0.9), False), "upwind": ((2.0, 1.0, 0.5), True)}
LEGS = {"central_mild": 900, "central_strong": 900, "upwind": 900}      # the leg's time limit in seconds


def median(v):
    return sorted(v)[len(v) // 2]


def timed_solves(cg, solve, repeats):
    """`repeats` solves from x = 0 behind one that warms up; the cap and a breakdown are results."""
    from conjugategradient_amd import _lib
    from conjugategradient_amd.solver import ApplicationException

    L = _lib.lib()
    samples = []
    for rep in range(repeats + 1):
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
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
    return dict(status=cg.status, bodies=cg.Iteration, s_to_solution=med, ms_per_body=1e3 * med / max(cg.Iteration, 1), residual=cg.Residual,
                true_residual=cg.TrueResidual, true_to_residual=cg.TrueResidual / cg.Residual if cg.Residual else None, samples_s=samples)


def plain_on(cg, nnz, level):
    """SolveBicgstab on the vectors of a multigrid object (the work vectors are those of its SolveBicgstab method)."""
    from conjugategradient_amd import _lib

    L = _lib.lib()
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)

    def solve():
        cg.status = L.SolveBicgstab(cg.cublas, cg.cusparse, cg.matDescr, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                                    cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr,
                                    cg.vectorV.Ptr, cg.vectorS.Ptr, cg.vectorT.Ptr, cg.vectorRhat.Ptr, nnz, cg.Count,
                                    level, 0, MAX_IT, _lib.RULE_NATIVE, C.byref(it), C.byref(res), C.byref(true), None, 0)
        cg.Iteration, cg.Residual, cg.TrueResidual = it.value, res.value, true.value

    return solve


def run_leg(leg, n, repeats):
    from conjugategradient_amd import _lib, problems
    from conjugategradient_amd.amg import ConjugateGradientAmgGpu
    from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
    from conjugategradient_amd.solver import VectorDouble

    _lib.require_gpu()
    L = _lib.lib()
    c, upwind = STENCILS[leg]
    s = problems.convection_diffusion(n, n, n, c, upwind=upwind)
    s.b = np.random.default_rng(7).standard_normal(s.Count)
    level = 1e-8 * float(np.linalg.norm(s.b))
    out = dict(rows=s.Count, nonzeros=s.nnz, c=list(c), upwind=upwind, stop_level=level, cap=MAX_IT)

    def setup(cg):
        """Initialize() uploads the matrix and builds the hierarchy; Setup() alone, once more, is the hierarchy's cost."""
        cg.Initialize()
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        cg.Setup()
        L.MgcgDeviceSynchronize()
        return time.perf_counter() - t0

    def with_setup(r, setup_s, cg):
        r.update(setup_s=setup_s, s_to_solution_with_setup=r["s_to_solution"] + setup_s, levels=cg.levels,
                 level_rows=[int(L.MgLevelRows(cg.mg, l)) for l in range(cg.levels)])
        return r

    geo = ConjugateGradientMgGpu(s.Count, 7, 0, MAX_IT, level, s.grid, rule=_lib.RULE_NATIVE).load(s)
    geo_s = setup(geo)
    for name in ("vectorV", "vectorS", "vectorT", "vectorRhat"):
        setattr(geo, name, VectorDouble(s.Count))
    out["plain"] = timed_solves(geo, plain_on(geo, s.nnz, level), repeats)
    print(json.dumps({leg: {"plain": out["plain"]}}), file=sys.stderr, flush=True)
    out["geometric_own"] = with_setup(timed_solves(geo, geo.SolveBicgstab, repeats), geo_s, geo)
    print(json.dumps({leg: {"geometric_own": out["geometric_own"]}}), file=sys.stderr, flush=True)

    half = ConjugateGradientMgGpu(s.Count, 7, 0, MAX_IT, level, s.grid, rule=_lib.RULE_NATIVE).load(problems.symmetric_part(s))
    half_s = setup(half)
    out["geometric_symmetric_part"] = with_setup(timed_solves(geo, lambda: geo.SolveBicgstab(hierarchy=half), repeats), half_s, half)
    print(json.dumps({leg: {"geometric_symmetric_part": out["geometric_symmetric_part"]}}), file=sys.stderr, flush=True)
    half.Dispose()
    geo.Dispose()

    agg = ConjugateGradientAmgGpu(s.Count, 7, 0, MAX_IT, level, rule=_lib.RULE_NATIVE).load(s)
    agg_s = setup(agg)
    out["aggregation_own"] = with_setup(timed_solves(agg, agg.SolveBicgstab, repeats), agg_s, agg)
    agg.Dispose()
    for name in ("geometric_own", "geometric_symmetric_part", "aggregation_own"):
        r, p = out[name], out["plain"]
        out[f"{name}_to_plain"] = dict(bodies=r["bodies"] / max(p["bodies"], 1), ms_per_body=r["ms_per_body"] / p["ms_per_body"],
                                       s_to_solution=r["s_to_solution"] / p["s_to_solution"],
                                       s_to_solution_with_setup=r["s_to_solution_with_setup"] / p["s_to_solution"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--leg", choices=list(LEGS), default=None, help="run this leg in this process")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), help="the legs to run, each as a child process under its own time limit")
    ap.add_argument("--n", type=int, default=256, help="the grid is n^3")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        result = {a.leg: run_leg(a.leg, a.n, a.repeats)}
    else:
        result = {"byte_model_per_row": BYTES, "n": a.n}
        for leg in a.legs:
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.bicgstab_mg_run", "--leg", leg, "--n", str(a.n), "--repeats", str(a.repeats)],
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
