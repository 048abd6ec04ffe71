"""Measurement only: what LOBPCG (MgcgSolveLobpcg, MgcgSolveLobpcgMg) costs per body and to solution, on one GPU.  No figure here is an
acceptance threshold.

  plain, jacobi, vcycle, aggregation   the k = 4 lowest eigenpairs of the 256^3 Poisson matrix (generated on the device) to a relative 1e-6,
                from the default start block: bodies, products (one k-column product per body and two outside the loop), ms per body
                beside the byte model's prediction, seconds to solution, the restarts, the true residuals.  vcycle: the geometric
                hierarchy (MgSetup); aggregation: MgSetupAggregation's.
  extremes      lambda_min and lambda_max alone (k = 1, plain, relative 1e-6) beside MgcgEstimateSpectrum with as many products (Lanczos
                steps) in the same process.

Byte model per body, stated, not measured (kernels_lobpcg.hip), with n rows, nnz stored entries and k columns: the residual pass reads X
and AX and writes R and W (4k columns, one more with the diagonal); X^T W reads 2k; W - X T reads 2k and writes k; W^T W reads 2k; W T reads
and writes k; the product reads the matrix once (12 bytes per stored entry, 4 per row), gathers k columns and writes k (a perfect cache);
G_B and G_A are six K x K tiles each that read 2k columns; the combine pass reads 6k and writes 4k: 47k columns of 8 bytes per row next to
the product.  A cycle of a hierarchy is not in the model.  ``predicted_ms_per_body`` is that sum at ``--rate`` TB/s.

Without --leg every leg runs as a child process of its own under a time limit of its own, and the script ends at the first one that
fails, aborts or runs into its limit.

    python -m conjugategradient_amd.tools.lobpcg_run --out profiles/lobpcg
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

LEGS = {"plain": 500, "jacobi": 500, "vcycle": 400, "aggregation": 400, "extremes": 500}          # the leg's time limit in seconds
GRID = (256, 256, 256)
K = 4
REL = 1e-6


def byte_model(n, nnz, k, dinv=False):
    """Bytes per body: (the vector passes, the product)."""
    return dict(vector_passes=8.0 * n * (47 * k + (1 if dinv else 0)), product=12.0 * nnz + 4.0 * (n + 1) + 16.0 * k * n)


def build(leg, grid, cap):
    """The object that holds the matrix on the device (and, for the hierarchy legs, the hierarchy)."""
    from conjugategradient_amd.amg import ConjugateGradientAmgGpu
    from conjugategradient_amd.multigrid import ConjugateGradientMgGpu

    n = grid[0] * grid[1] * grid[2]
    if leg == "aggregation":
        cg = ConjugateGradientAmgGpu(n, 7, 0, cap, REL)
        cg.InitializePoisson(grid)
    else:
        cg = ConjugateGradientMgGpu(n, 7, 0, cap, REL, grid)
        cg.InitializePoisson()
    return cg


def solve(cg, leg, k, largest=False):
    from conjugategradient_amd import _lib
    from conjugategradient_amd.eigen import lobpcg_call
    from conjugategradient_amd.jacobi import jacobi_setup
    from conjugategradient_amd.solver import ApplicationException, VectorDouble

    L = _lib.lib()
    dinv = None
    if leg == "jacobi":
        dinv = VectorDouble(cg.Count)
        jacobi_setup(cg.cusparse, cg.vectorA, cg.vectorRowOffsets, cg.vectorColumnIndeces, cg._nnz, cg.Count, 0, dinv)
    L.MgcgDeviceSynchronize()
    t0 = time.perf_counter()
    try:
        if leg in ("vcycle", "aggregation"):
            cg.SolveLobpcg(k)
        else:
            lobpcg_call(cg, "MgcgSolveLobpcg", k, (), (dinv.Ptr if dinv else None,), largest, True, False, None, 1)
    except (ApplicationException, _lib.MgcgError):
        pass
    seconds = time.perf_counter() - t0
    bodies = cg.Iteration + 1
    out = dict(status=int(cg.status), bodies=bodies, products=bodies + 1, restarts=cg.Restarts, seconds_to_solution=seconds, ms_per_body=seconds * 1e3 / max(bodies, 1),
               theta=[float(v) for v in cg.Theta], residual=[float(v) for v in cg.Residual], true_residual=[float(v) for v in cg.TrueResidual])
    if dinv:
        dinv.Dispose()
    return out


def run_leg(leg, grid, cap, rate):
    from conjugategradient_amd import _lib

    _lib.require_gpu()
    cg = build(leg, grid, cap)
    n, nnz = cg.Count, cg._nnz
    out = dict(grid=list(grid), rows=n, stored_entries=nnz, rate_TBps=rate)
    if leg == "extremes":
        L = _lib.lib()
        model = byte_model(n, nnz, 1)
        out["byte_model_per_body"] = model
        out["predicted_ms_per_body"] = sum(model.values()) / (rate * 1e12) * 1e3
        for which, largest in (("lambda_min", False), ("lambda_max", True)):
            solve(cg, "plain", 1, largest)                  # warms up
            r = solve(cg, "plain", 1, largest)
            lo, hi, done = C.c_double(0), C.c_double(0), C.c_int(0)
            L.MgcgDeviceSynchronize()
            t0 = time.perf_counter()
            st = L.MgcgEstimateSpectrum(cg.cublas, cg.cusparse, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, nnz, n, 0, int(r["products"]), 1,
                                        C.byref(lo), C.byref(hi), None, C.byref(done))
            L.MgcgDeviceSynchronize()
            r["estimate_spectrum"] = dict(status=int(st), steps=done.value, seconds=time.perf_counter() - t0, value=hi.value if largest else lo.value)
            out[which] = r
    else:
        model = byte_model(n, nnz, K, leg == "jacobi")
        out["byte_model_per_body"] = model
        out["predicted_ms_per_body"] = sum(model.values()) / (rate * 1e12) * 1e3
        warm_cap, cg.MaxIteration = cg.MaxIteration, 3
        solve(cg, leg, K)                                   # warms up: code objects, the workspace
        cg.MaxIteration = warm_cap
        out["to_relative_1e-6"] = solve(cg, leg, K)
    cg.Dispose()
    return out


def readme(result):
    lines = ["# LOBPCG (MgcgSolveLobpcg, MgcgSolveLobpcgMg), one MI355X", "",
             "Written by `python -m conjugategradient_amd.tools.lobpcg_run --out profiles/lobpcg`; the numbers are in `lobpcg_run.json`.",
             f"The {K} lowest eigenpairs of the Poisson matrix to a relative {REL:g}, default start block.  `predicted`: the byte model of a body",
             "(vector passes and the k-column product, no cycle) at the stated rate; status 0 converged, 1 the cap was hit.  A preconditioned leg that",
             "takes longer to solution than the plain one is marked.", "",
             "| preconditioner | status | bodies | products | restarts | ms per body | predicted | measured / predicted | seconds to solution | largest true residual |", "|---|---|---|---|---|---|---|---|---|---|"]
    base = result.get("plain", {}).get("to_relative_1e-6")          # the baseline of "slower today": the plain loop's seconds to solution
    for leg in LEGS:
        r = result.get(leg)
        if not r or "to_relative_1e-6" not in r:
            continue
        t = r["to_relative_1e-6"]
        note = " **slower today than plain**" if base and leg != "plain" and t["seconds_to_solution"] > base["seconds_to_solution"] else ""
        lines.append(f"| {leg} ({r['grid'][0]}^3) | {t['status']} | {t['bodies']} | {t['products']} | {t['restarts']} | {t['ms_per_body']:.3f} | {r['predicted_ms_per_body']:.3f} at {r['rate_TBps']} TB/s | "
                     f"{t['ms_per_body'] / r['predicted_ms_per_body']:.2f} | {t['seconds_to_solution']:.3f}{note} | {max(t['true_residual']):.3e} |")
    e = result.get("extremes")
    if e:
        lines += ["", f"## lambda_min and lambda_max alone (k = 1, plain, {e['grid'][0]}^3) beside MgcgEstimateSpectrum with as many products", "",
                  "| | LOBPCG status | bodies | value | true residual | seconds | Lanczos steps | Lanczos value | Lanczos seconds | |", "|---|---|---|---|---|---|---|---|---|---|"]
        for which in ("lambda_min", "lambda_max"):
            r, s = e[which], e[which]["estimate_spectrum"]
            note = "**LOBPCG is slower today**" if r["seconds_to_solution"] > s["seconds"] else ""
            lines.append(f"| {which} | {r['status']} | {r['bodies']} | {r['theta'][0]:.12g} | {r['true_residual'][0]:.3e} | {r['seconds_to_solution']:.3f} | {s['steps']} | {s['value']:.12g} | {s['seconds']:.3f} | {note} |")
    return "\n".join(lines)


def write(out, result):
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "lobpcg_run.json"), "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    with open(os.path.join(out, "README.md"), "w") as f:
        f.write(readme(result) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="a directory: lobpcg_run.json and README.md are written there")
    ap.add_argument("--leg", choices=list(LEGS), default=None, help="run this leg in this process")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), help="the legs to run, each as a child process under its own time limit")
    ap.add_argument("--grid", type=int, nargs=3, default=list(GRID), help="the Poisson grid")
    ap.add_argument("--cap", type=int, default=4000, help="at most this many bodies per solve")
    ap.add_argument("--rate", type=float, default=5.4, help="TB/s of the byte model's prediction")
    a = ap.parse_args()
    if a.leg:
        result = {a.leg: run_leg(a.leg, tuple(a.grid), a.cap, a.rate)}
    else:
        result = {}
        for leg in a.legs:
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.lobpcg_run", "--leg", leg, "--grid", *map(str, a.grid), "--cap", str(a.cap),
                                    "--rate", str(a.rate)], stdout=subprocess.PIPE, timeout=LEGS[leg], check=True)      # a leg that fails or hangs ends the script
            result.update(json.loads(child.stdout))
            if a.out:                                      # what is measured so far survives a later leg's failure
                write(a.out, result)
    print(json.dumps(result, indent=1))
    if a.out:
        write(a.out, result)


if __name__ == "__main__":
    main()
