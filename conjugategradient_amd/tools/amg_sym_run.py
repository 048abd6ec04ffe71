"""Measurement only: what matching on the symmetric part (MgSetupAggregationEx, strength = 1) buys the aggregation V-cycle on nonsymmetric
stencils, on one GPU.  Every run starts from x = 0 with an N(0,1) right-hand side and stops at || r || < 1e-8 || b || (MGCG_RULE_NATIVE) or
at the cap of 20 000 bodies (plain SolveGmres: 3000 steps).  No figure here is an acceptance threshold: the comparators are the
strength = 0 hierarchy and the plain loop of the same process.

  central_mild     256^3 convection_diffusion, c = (.5, .25, 0)
  central_strong   256^3 convection_diffusion, c = (.9, .9, .9)
  upwind           256^3 convection_diffusion, c = (2, 1, .5), first-order upwinding

Per leg, on one copy of the matrix, SolveBicgstabMg and SolveGmresMg (m = 10, orth = 1) behind five forms: the aggregation hierarchy of
strength 0 (the class's defaults), of strength 1 with the Jacobi smoother, of strength 1 with the Gauss-Seidel smoother (MgSetSmoother on
the same hierarchy; its seconds are the colouring's), the geometric hierarchy of the matrix (MgSetup), and no preconditioner (SolveBicgstab,
SolveGmres(10), orth = 1).  Reported: rows per level, the set-up's seconds (the hierarchy alone: the matrix is on the device already), what
strength = 1 adds to the strength = 0 set-up, the seconds of one MgcgSymmetricPart of the fine matrix (count only), bodies (BiCGStab: two
cycles and two products each) or steps (GMRES: one of each), ms per body (time of the call / bodies run), seconds to solution without and
with set-up, TrueResidual beside Residual.  One solve warms up, the median of --repeats follows.

Without --leg every leg runs as a child process of its own under a time limit of its own, and the script ends at the first one that fails.

    python -m conjugategradient_amd.tools.amg_sym_run --out profiles/amg_sym/amg_sym_run.json
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

MAX_IT = 20000
PLAIN_GMRES_CAP = 3000
M, ORTH = 10, 1
STENCILS = {"central_mild": ((0.5, 0.25, 0.0), False), "central_strong": ((0.9, 0.9, 0.9), False), "upwind": ((2.0, 1.0, 0.5), True)}
LEGS = {"central_mild": 900, "central_strong": 900, "upwind": 900}      # the leg's time limit in seconds
FORMS = ("aggregation_strength0", "aggregation_strength1_jacobi", "aggregation_strength1_gs", "geometric_own")


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


def plain_on(cg, nnz, level, which):
    """SolveBicgstab or SolveGmres(M), orth = ORTH, on the vectors of a multigrid object (the work vectors are those of its methods)."""
    from conjugategradient_amd import _lib

    L = _lib.lib()
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
    matrix = (cg.cublas, cg.cusparse, cg.matDescr, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
              cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr)

    def solve():
        if which == "bicgstab":
            cg.status = L.SolveBicgstab(*matrix, cg.vectorV.Ptr, cg.vectorS.Ptr, cg.vectorT.Ptr, cg.vectorRhat.Ptr, nnz, cg.Count,
                                        level, 0, MAX_IT, _lib.RULE_NATIVE, C.byref(it), C.byref(res), C.byref(true), None, 0)
        else:
            cg.status = L.SolveGmres(*matrix, cg.vectorWork.Ptr, M, ORTH, nnz, cg.Count, level, 0, PLAIN_GMRES_CAP, _lib.RULE_NATIVE,
                                     C.byref(it), C.byref(res), C.byref(true), None, 0)
        cg.Iteration, cg.Residual, cg.TrueResidual = it.value, res.value, true.value

    return solve


def run_leg(leg, n, repeats):
    from conjugategradient_amd import _lib, problems
    from conjugategradient_amd.amg import ConjugateGradientAmgGpu
    from conjugategradient_amd.multigrid import ConjugateGradientMgGpu

    _lib.require_gpu()
    L = _lib.lib()
    c, upwind = STENCILS[leg]
    s = problems.convection_diffusion(n, n, n, c, upwind=upwind)
    s.b = np.random.default_rng(7).standard_normal(s.Count)
    level = 1e-8 * float(np.linalg.norm(s.b))
    out = dict(rows=s.Count, nonzeros=s.nnz, c=list(c), upwind=upwind, stop_level=level, cap=MAX_IT, plain_gmres_cap=PLAIN_GMRES_CAP, m=M, orth=ORTH)

    def note(key):
        print(json.dumps({leg: {key: out[key]}}), file=sys.stderr, flush=True)

    def timed(call):
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        got = call()
        L.MgcgDeviceSynchronize()
        return time.perf_counter() - t0, got

    def both(cg, key, setup_s, **more):
        """The two solvers behind cg's hierarchy as it stands."""
        shape = dict(setup_s=setup_s, levels=cg.levels, level_rows=[int(L.MgLevelRows(cg.mg, l)) for l in range(cg.levels)],
                     level_nonzeros=[int(L.MgLevelNnz(cg.mg, l)) for l in range(cg.levels)], **more)
        out[key] = dict(shape)
        for name, solve in (("bicgstab", cg.SolveBicgstab), ("gmres", lambda: cg.SolveGmres(m=M, orth=ORTH))):
            r = timed_solves(cg, solve, repeats)
            r["s_to_solution_with_setup"] = r["s_to_solution"] + setup_s
            out[key][name] = r
        note(key)

    # Initialize() uploads the matrix and builds the hierarchy; Setup() alone, once more, is the hierarchy's cost
    agg = ConjugateGradientAmgGpu(s.Count, 7, 0, MAX_IT, level, rule=_lib.RULE_NATIVE).load(s)
    agg.Initialize()
    own_s, _ = timed(agg.Setup)
    both(agg, "aggregation_strength0", own_s)                 # (allocates the work vectors of the plain loops below)
    out["plain"] = dict(bicgstab=timed_solves(agg, plain_on(agg, s.nnz, level, "bicgstab"), repeats),
                        gmres=timed_solves(agg, plain_on(agg, s.nnz, level, "gmres"), repeats))
    note("plain")
    part_s, count = timed(lambda: L.MgcgSymmetricPart(agg.cublas, agg.cusparse, agg.vectorA.Ptr, agg.vectorRowOffsets.Ptr, agg.vectorColumnIndeces.Ptr,
                                                      s.nnz, s.Count, None, None, None, 0))
    out["symmetric_part_of_the_fine_matrix"] = dict(seconds=part_s, nonzeros=int(count))
    agg.strength = "symmetric"
    sym_s, _ = timed(agg.Setup)
    both(agg, "aggregation_strength1_jacobi", sym_s, setup_added_by_strength1_s=sym_s - own_s)
    gs_s, refused = timed(lambda: L.MgSetSmoother(agg.mg, 1))
    if refused == 0:
        both(agg, "aggregation_strength1_gs", sym_s + gs_s, colouring_s=gs_s, colours=[int(L.MgLevelColours(agg.mg, l)) for l in range(agg.levels)])
    else:
        out["aggregation_strength1_gs"] = dict(refused=_lib.last_error())
        L.MgcgClearLastError()
    agg.Dispose()

    geo = ConjugateGradientMgGpu(s.Count, 7, 0, MAX_IT, level, s.grid, rule=_lib.RULE_NATIVE).load(s)
    geo.Initialize()
    geo_s, _ = timed(geo.Setup)
    both(geo, "geometric_own", geo_s)
    geo.Dispose()

    for form in FORMS:
        if "refused" in out[form]:
            continue
        for name in ("bicgstab", "gmres"):
            r = out[form][name]
            for other, key in ((out["plain"][name], "to_plain"), (out["aggregation_strength0"][name], "to_strength0")):
                r[key] = dict(bodies=r["bodies"] / max(other["bodies"], 1), ms_per_body=r["ms_per_body"] / other["ms_per_body"],
                              s_to_solution=r["s_to_solution"] / other["s_to_solution"])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--leg", choices=list(LEGS), default=None, help="run this leg in this process")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), help="the legs to run, each as a child process under its own time limit")
    ap.add_argument("--n", type=int, default=256, help="the grid is n^3")
    ap.add_argument("--repeats", type=int, default=2)
    a = ap.parse_args()
    if a.leg:
        result = {a.leg: run_leg(a.leg, a.n, a.repeats)}
    else:
        result = {"n": a.n}
        for leg in a.legs:
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.amg_sym_run", "--leg", leg, "--n", str(a.n), "--repeats", str(a.repeats)],
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
