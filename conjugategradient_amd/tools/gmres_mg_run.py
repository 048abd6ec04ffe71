"""Measurement only: what V-cycle-preconditioned flexible GMRES(m) (SolveGmresMg) costs beside SolveBicgstabMg and plain SolveGmres(20), on
one GPU.  Every run starts from x = 0 with an N(0,1) right-hand side and stops at || r || < 1e-8 || b || (MGCG_RULE_NATIVE) or at the cap
of 20 000 steps (plain SolveGmres: 3000).  No figure here is an acceptance threshold.

  central_mild     256^3 convection_diffusion, c = (.5, .25, 0)
  central_strong   256^3 convection_diffusion, c = (.9, .9, .9)
  upwind           256^3 convection_diffusion, c = (2, 1, .5), first-order upwinding

Per leg, on one copy of the matrix and in one process: with the geometric hierarchy of the matrix itself (MgSetup) and with its aggregation
hierarchy (MgSetupAggregation, the class's defaults), SolveBicgstabMg and SolveGmresMg with m in {10, 20, 30} and orth in {1, 2}; and
plain SolveGmres(20), orth = 2, on the same vectors -- steps (bodies for BiCGStab: two cycles and two products each), ms per step (time of
the call / steps run), seconds to solution, the set-up's seconds (the hierarchy alone: the matrix is on the device already) and seconds to
solution including set-up, TrueResidual / Residual.  One solve warms up, the median of --repeats follows.

Without --leg every leg runs as a child process of its own under a time limit of its own, and the script ends at the first one that fails.

Byte model per row at 7 entries per row, stated, not measured: a step is one cycle, one product (~104) and section
27's passes at the step's place j in its cycle, 8 x (orth x (2 (j + 1) + 3 ceil((j + 1) / 8)) + 2) bytes; a BiCGStab body is two cycles,
two products and 128 bytes of passes.

    python -m conjugategradient_amd.tools.gmres_mg_run --out profiles/gmres_mg/gmres_mg_run.json
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
PLAIN_CAP = 3000
PLAIN_M = 20
RATE_TBS = 5.75                      # 559 bytes per row x 256^3 rows / 1.63 ms (section 27, GMRES(20) orth 2)
PRODUCT_BYTES = 104
BICGSTAB_PASS_BYTES = 128            # section 24's four passes
STENCILS = {"central_mild": ((0.5, 0.25, 0.0), False), "central_strong": ((0.9, 0.9, 0.9), False), "upwind": ((2.0, 1.0, 0.5), True)}
LEGS = {"central_mild": 420, "central_strong": 420, "upwind": 420}      # the leg's time limit in seconds
FORMS = [(m, orth) for m in (10, 20, 30) for orth in (1, 2)]


def pass_bytes(j, orth):
    """Section 27's passes of a step at place j of its cycle, bytes per row: per Gram-Schmidt pass c + q vectors read by the dots and
    c + 2 q read and written by the update (c = j + 1 columns in q launches), and pass N's 2."""
    c = j + 1
    q = (c + 7) // 8
    return 8 * (orth * (2 * c + 3 * q) + 2)


def mean_pass_bytes(steps, m, orth):
    """... averaged over a run of `steps` steps restarted every m."""
    return sum(pass_bytes(k % m, orth) for k in range(steps)) / max(steps, 1)


def cycle_share_bytes(steps, m):
    """The close and the restart, bytes per row per step of a run of `steps` steps: per cycle of cols columns the x pass (cols + 2 ceil(cols
    / 8) vectors) and, in front of every cycle but the first, a product (104) and the restart's pass (3 vectors)."""
    total, k = 0, 0
    while k < steps:
        cols = min(m, steps - k)
        total += 8 * (cols + 2 * ((cols + 7) // 8)) + (104 + 24 if k else 0)
        k += cols
    return total / max(steps, 1)


def predicted_ms_per_step(steps, m, orth, rows, body_ms):
    """The byte model, written down before the first run: a step is one cycle, one product and section 27's passes at
    the observed places j.  Bytes move at RATE_TBS, the rate at which section 27's measured steps meet their byte table (1.63 ms for 559
    bytes per row at 256^3); the cycle's cost is taken from this leg's own BiCGStab body: (body - 2 products - 128 bytes) / 2."""
    ms = lambda bytes_per_row: 1e3 * bytes_per_row * rows / (RATE_TBS * 1e12)
    cycle_ms = (body_ms - ms(2 * PRODUCT_BYTES + BICGSTAB_PASS_BYTES)) / 2
    return dict(cycle_ms=cycle_ms, product_ms=ms(PRODUCT_BYTES), passes_ms=ms(mean_pass_bytes(steps, m, orth) + cycle_share_bytes(steps, m)),
                ms_per_step=cycle_ms + ms(PRODUCT_BYTES + mean_pass_bytes(steps, m, orth) + cycle_share_bytes(steps, m)))


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
    return dict(status=cg.status, steps=cg.Iteration, s_to_solution=med, ms_per_step=1e3 * med / max(cg.Iteration, 1), residual=cg.Residual,
                true_residual=cg.TrueResidual, true_to_residual=cg.TrueResidual / cg.Residual if cg.Residual else None, samples_s=samples)


def plain_on(cg, nnz, level):
    """SolveGmres(20) on the vectors of a multigrid object (the work vector is that of its SolveGmres method: long enough)."""
    from conjugategradient_amd import _lib

    L = _lib.lib()
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)

    def solve():
        cg.status = L.SolveGmres(cg.cublas, cg.cusparse, cg.matDescr, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                                 cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr, cg.vectorWork.Ptr,
                                 PLAIN_M, 2, nnz, cg.Count, level, 0, PLAIN_CAP, _lib.RULE_NATIVE, C.byref(it), C.byref(res), C.byref(true), None, 0)
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
    out = dict(rows=s.Count, nonzeros=s.nnz, c=list(c), upwind=upwind, stop_level=level, cap=MAX_IT, plain_cap=PLAIN_CAP)

    def note(key):
        print(json.dumps({leg: {key: out[key]}}), file=sys.stderr, flush=True)

    def hierarchy_runs(cg, key):
        """Initialize() uploads the matrix and builds the hierarchy; Setup() alone, once more, is the hierarchy's cost."""
        cg.Initialize()
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        cg.Setup()
        L.MgcgDeviceSynchronize()
        setup_s = time.perf_counter() - t0
        shape = dict(setup_s=setup_s, levels=cg.levels, level_rows=[int(L.MgLevelRows(cg.mg, l)) for l in range(cg.levels)])
        old = timed_solves(cg, cg.SolveBicgstab, repeats)
        old.update(shape, s_to_solution_with_setup=old["s_to_solution"] + setup_s, cycles=2 * old["steps"])
        out[f"{key}_bicgstab"] = old
        note(f"{key}_bicgstab")
        for m, orth in FORMS:
            r = timed_solves(cg, lambda: cg.SolveGmres(m=m, orth=orth), repeats)
            r.update(shape, m=m, orth=orth, s_to_solution_with_setup=r["s_to_solution"] + setup_s, cycles=r["steps"],
                     mean_pass_bytes_per_row=mean_pass_bytes(r["steps"], m, orth), cycle_share_bytes_per_row=cycle_share_bytes(r["steps"], m),
                     predicted=predicted_ms_per_step(r["steps"], m, orth, s.Count, old["ms_per_step"]),
                     to_bicgstab=dict(cycles=r["steps"] / max(2 * old["steps"], 1), s_to_solution=r["s_to_solution"] / old["s_to_solution"]))
            out[f"{key}_gmres_m{m}_orth{orth}"] = r
            note(f"{key}_gmres_m{m}_orth{orth}")

    geo = ConjugateGradientMgGpu(s.Count, 7, 0, MAX_IT, level, s.grid, rule=_lib.RULE_NATIVE).load(s)
    hierarchy_runs(geo, "geometric")
    plain = timed_solves(geo, plain_on(geo, s.nnz, level), min(repeats, 1))
    plain.update(m=PLAIN_M, orth=2, mean_pass_bytes_per_row=mean_pass_bytes(plain["steps"], PLAIN_M, 2))
    out["plain_gmres"] = plain
    note("plain_gmres")
    geo.Dispose()

    agg = ConjugateGradientAmgGpu(s.Count, 7, 0, MAX_IT, level, rule=_lib.RULE_NATIVE).load(s)
    hierarchy_runs(agg, "aggregation")
    agg.Dispose()
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
        result = {"n": a.n, "forms": FORMS}
        for leg in a.legs:
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.gmres_mg_run", "--leg", leg, "--n", str(a.n), "--repeats", str(a.repeats)],
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
