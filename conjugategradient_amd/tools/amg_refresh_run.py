"""Measurement only: what MgUpdateValues -- the numeric refresh of an aggregation hierarchy whose maps are kept -- costs next to the two
set-ups it stands in for, on one GPU, in one process per leg.  No figure here is an acceptance threshold.

  poisson256_p2 / _p3   256^3 7-point Poisson from the device generator, 2 and 3 matching passes a level
  permuted128           the 128^3 matrix with rows and columns permuted, 2 passes
  upwind256             256^3 convection-diffusion, first-order upwinding, strength="symmetric", 2 passes; solved by SolveGmresMg(10)

Per leg: the set-up by the library's matching (timed), a solve; the FIRST MgUpdateValues (source lists, shadow buffers and one numeric
pass; the list build is that time less a later call's), then the median of --calls later ones; a solve again, which must take the
iterations and the time of the first since the refresh is given the values the hierarchy was built from (the cost of a refresh does not
depend on the values); then the parent's two routes to a hierarchy for new values of the same pattern, each --repeats times:
MgDestroy + MgSetupAggregates with the kept maps (host arrays prepared outside the timing) -- the cheapest route to the same bits, the
yardstick -- and MgDestroy + MgSetupAggregation(Ex).  MgUpdateBytes stands beside the bytes of the hierarchy's own levels and maps.

The byte model of a refresh (n rows, z entries of a level, z' entries of the next):
  a level with a map:  a once 8 z (gathered through the list), sources 4 z, offsets 4 (z' + 1), C 8 z'
  every level:         the diagonal check and D^-1 read the matrix once each (12 z + 4 n), D^-1 is written and read again: 16 n

Without --leg every leg runs as a child process of its own under a time limit of its own, and the script ends at the first one that fails.

    python -m conjugategradient_amd.tools.amg_refresh_run --out profiles/refresh/amg_refresh_run.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

CAP = 2000
M, ORTH = 10, 1
LEGS = {"poisson256_p2": 420, "poisson256_p3": 420, "permuted128": 300, "upwind256": 420}      # the leg's time limit in seconds


def median(v):
    return sorted(v)[len(v) // 2]


def refresh_model(rows, nnz):
    """Bytes of one refresh by the model of the module's docstring: (the numeric passes, the D^-1 passes)."""
    numeric = sum(12 * z + 4 * (zc + 1) + 8 * zc for z, zc in zip(nnz[:-1], nnz[1:]))
    dinv = sum(2 * (12 * z + 4 * n) + 16 * n for n, z in zip(rows, nnz))
    return numeric, dinv


def run_leg(leg, repeats, calls):
    from conjugategradient_amd import _lib, problems
    from conjugategradient_amd.amg import ConjugateGradientAmgGpu
    from conjugategradient_amd.solver import ApplicationException, _ptr
    from conjugategradient_amd.tools.amg_cg_run import permuted_poisson, randn_rhs

    _lib.require_gpu()
    L = _lib.lib()
    symmetric = leg != "upwind256"
    kw = dict(omega=6.0 / 7.0, passes=3 if leg.endswith("_p3") else 2)
    if leg.startswith("poisson256"):
        cg = ConjugateGradientAmgGpu(256 ** 3, 7, 0, CAP, 0.0, **kw)
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        cg.InitializePoisson((256, 256, 256))               # (the generator's pass is part of this first time, not of the later ones)
        L.MgcgDeviceSynchronize()
        first_setup_s = time.perf_counter() - t0
        bnorm = randn_rhs(cg)
    else:
        if leg == "permuted128":
            s = permuted_poisson(128)
        else:
            s = problems.convection_diffusion(256, 256, 256, (2.0, 1.0, 0.5), upwind=True)
            kw.update(omega=0.8, strength="symmetric")
        s.b = np.random.default_rng(20261019).standard_normal(s.Count)
        bnorm = float(np.linalg.norm(s.b))
        cg = ConjugateGradientAmgGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, CAP, 0.0, **kw).load(s)
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        cg.Initialize()                                     # (with the upload of the matrix)
        L.MgcgDeviceSynchronize()
        first_setup_s = time.perf_counter() - t0
    cg.AllowableResidual = 1e-8 * bnorm
    nz = int(cg.A.RowOffsets[cg.Count]) if cg.A is not None else cg._nnz

    def timed(call):
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        call()
        L.MgcgDeviceSynchronize()
        return time.perf_counter() - t0

    def solve():
        """`repeats` solves from x = 0 behind one that warms up; the cap and a breakdown are results."""
        samples = []
        for rep in range(repeats + 1):
            L.MgcgFill(cg.vectorX.Ptr, 0.0)
            L.MgcgDeviceSynchronize()
            t0 = time.perf_counter()
            try:
                cg.Solve() if symmetric else cg.SolveGmres(m=M, orth=ORTH)
            except (ApplicationException, _lib.MgcgError):
                pass
            if rep:
                samples.append(time.perf_counter() - t0)
            L.MgcgClearLastError()
        return dict(loop="SolveMg" if symmetric else "SolveGmresMg", status=cg.status, iterations=cg.Iteration, seconds=median(samples),
                    residual_over_b=cg.Residual / bnorm, samples_s=samples)

    rows = [int(L.MgLevelRows(cg.mg, l)) for l in range(cg.levels)]
    nnz = [int(L.MgLevelNnz(cg.mg, l)) for l in range(cg.levels)]
    own_bytes = sum(12 * z + 4 * (n + 1) for n, z in zip(rows[1:], nnz[1:])) + sum(8 * n for n in rows) + sum(12 * n + 4 * (nc + 1) for n, nc in zip(rows[:-1], rows[1:]))
    out = dict(rows=cg.Count, passes=kw["passes"], level_rows=rows, level_nonzeros=nnz, first_setup_with_upload_s=first_setup_s,
               hierarchy_bytes_levels_dinv_maps=own_bytes)
    out["solve_after_setup"] = solve()

    maps = [cg.level_aggregates(l) for l in range(cg.levels - 1)]
    first_s = timed(lambda: cg.UpdateValues(None))
    later = [timed(lambda: cg.UpdateValues(None)) for _ in range(calls)]
    numeric, dinv = refresh_model(rows, nnz)
    lengths = [float(z) / zc for z, zc in zip(nnz[:-1], nnz[1:])]
    out["refresh"] = dict(first_call_s=first_s, later_call_s=median(later), later_samples_s=later, list_build_s=first_s - median(later),
                          update_bytes=cg.update_bytes(), model_bytes_numeric=numeric, model_bytes_dinv=dinv,
                          model_GBps_at_this_time=(numeric + dinv) / median(later) / 1e9, mean_segment_per_level=lengths)
    out["solve_after_refresh"] = solve()

    # the parent's routes: a whole set-up for the new values
    level_rows = np.asarray(rows, dtype=np.int32)
    flat = np.ascontiguousarray(np.concatenate(maps), dtype=np.int32) if maps else np.zeros(1, dtype=np.int32)
    matrix = (cg.cublas, cg.cusparse, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, nz, cg.Count)

    def from_kept_maps():
        L.MgDestroy(cg.mg)
        cg.mg = L.MgSetupAggregates(*matrix, len(rows), _ptr(level_rows), _ptr(flat), cg.omega, cg.nu, cg.nuCoarse, cg.sigma)
        _lib.check("MgSetupAggregates")

    kept = [timed(from_kept_maps) for _ in range(repeats)]
    assert [int(L.MgLevelNnz(cg.mg, l)) for l in range(cg.levels)] == nnz
    out["MgDestroy_MgSetupAggregates_kept_maps"] = dict(seconds=median(kept), samples_s=kept)
    matching = [timed(cg.Setup) for _ in range(repeats)]
    out["MgDestroy_MgSetupAggregation"] = dict(seconds=median(matching), samples_s=matching)
    r = out["refresh"]
    r["to_kept_maps_setup"] = r["later_call_s"] / median(kept)
    r["to_matching_setup"] = r["later_call_s"] / median(matching)
    cg.Dispose()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--leg", choices=list(LEGS), default=None, help="run this leg in this process")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), help="the legs to run, each as a child process under its own time limit")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5, help="MgUpdateValues calls behind the first")
    a = ap.parse_args()
    if a.leg:
        result = {a.leg: run_leg(a.leg, a.repeats, a.calls)}
    else:
        result = {}
        for leg in a.legs:
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.amg_refresh_run", "--leg", leg, "--repeats", str(a.repeats), "--calls", str(a.calls)],
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
