"""Measurement only: what LSQR (MgcgSolveLsqr) costs per body and to solution, on one GPU.  No figure here is an acceptance threshold.

  convdiff256   (a) 256^3 upwind convection_diffusion with c = (2, 1, .5), N(0,1) right-hand side, to a relative 1e-8 in g (MGCG_RULE_VIENNACL):
                bodies, ms per body, seconds to solution; SolveBicgstab and SolveGmres (m = 20) to a relative 1e-8 in || r || on the same
                matrix in the same process.  LSQR works on the spectrum of A^T A and is expected to be far slower to solution.
  tall4m        (b) problems.sparse_rectangular(4 194 304, 1 048 576, 8), its own N(0,1) right-hand side: the same per-body figures from a fixed
                number of bodies, and the set-up (Initialize(): the upload and the transposition on the device) timed by itself.
  trace_a, trace_b   a fixed number of bodies of (a) / (b), once, for a kernel trace

Byte model per body, stated, not measured (kernels_lsqr.hip): pass U 24 bytes per row, pass V 56 per column; a product reads its matrix
once (12 bytes per stored entry and 4 per row of offsets), gathers one vector and writes the other (8 bytes per row and per column, with a
perfect cache).  ``predicted_ms_per_body`` is that sum at ``--rate`` TB/s (default 5.4: what the MINRES passes reach).

Without --leg every leg runs as a child process of its own under a time limit of its own, and the script ends at the first one that
fails, aborts or runs into its limit.

    python -m conjugategradient_amd.tools.lsqr_run --out profiles/lsqr
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m conjugategradient_amd.tools.lsqr_run --leg trace_a
    python conjugategradient_amd/tools/trace_kernel_medians.py OUT      (the two products' and the two passes' medians: bytes / median = rate)
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

LEGS = {"convdiff256": 900, "tall4m": 600}          # the leg's time limit in seconds
TRACES = {"trace_a": "convdiff256", "trace_b": "tall4m"}
CONVECTION = (2.0, 1.0, 0.5)
TALL = (4 * 1024 * 1024, 1024 * 1024, 8)
MAX_BODIES = 20000


def byte_model(rows, columns, nnz):
    """Bytes per body: (the two products, pass U, pass V)."""
    product = 12.0 * nnz + 4.0 * (rows + 1) + 8.0 * (rows + columns)
    product_t = 12.0 * nnz + 4.0 * (columns + 1) + 8.0 * (rows + columns)
    return dict(product_A=product, product_AT=product_t, pass_U=24.0 * rows, pass_V=56.0 * columns)


def build(which):
    from conjugategradient_amd import problems

    if which == "convdiff256":
        s = problems.convection_diffusion(256, 256, 256, CONVECTION, upwind=True)
        b = np.random.default_rng(7).standard_normal(s.Count)
        return s, problems.least_squares(s, s.Count, b, "convdiff256")
    return None, problems.sparse_rectangular(*TALL)


def lsqr_solve(ls, tol, cap, rule, damp=0.0):
    """(object, seconds of Initialize(), run(bodies=None) -> dict)."""
    from conjugategradient_amd import _lib
    from conjugategradient_amd.lsqr import LeastSquaresGpu
    from conjugategradient_amd.solver import ApplicationException

    L = _lib.lib()
    cg = LeastSquaresGpu(ls.Rows, ls.Columns, int(np.diff(ls.RowOffsets).max()), 0, cap, tol, rule=rule, damp=damp).load(ls)
    t0 = time.perf_counter()
    cg.Initialize()
    L.MgcgDeviceSynchronize()
    setup = time.perf_counter() - t0

    def run(bodies=None):
        cg.MaxIteration, cg.AllowableResidual = (cap, tol) if bodies is None else (bodies - 1, 0.0)
        L.MgcgDeviceSynchronize()
        t1 = time.perf_counter()
        try:
            cg.Solve()
        except ApplicationException:
            pass
        ms = (time.perf_counter() - t1) * 1e3
        return dict(status=cg.status, bodies=cg.Iteration, ms=ms, ms_per_body=ms / max(cg.Iteration, 1), g=cg.Residual, residual_norm=cg.ResidualNorm,
                    true_residual=cg.TrueResidual, true_normal_residual=cg.TrueNormalResidual)
    return cg, setup, run


def others(s, b, cap):
    """SolveBicgstab and SolveGmres (m = 20) to a relative 1e-8 in || r || on the square system, x = 0."""
    from conjugategradient_amd import _lib, problems
    from conjugategradient_amd.bicgstab import BiConjugateGradientStabGpu
    from conjugategradient_amd.gmres import GeneralizedMinimalResidualGpu
    from conjugategradient_amd.solver import ApplicationException

    sys_b = problems.LinearSystem(s.Elements, s.ColumnIndeces, s.RowOffsets, np.zeros(s.Count), b, s.name, s.grid)
    tol = 1e-8 * float(np.linalg.norm(b))
    out = {}
    for name, make in (("bicgstab", lambda: BiConjugateGradientStabGpu(s.Count, 7, 0, cap, tol, rule=_lib.RULE_NATIVE)),
                       ("gmres_20", lambda: GeneralizedMinimalResidualGpu(s.Count, 7, 0, cap, tol, rule=_lib.RULE_NATIVE, m=20))):
        cg = make().load(sys_b)
        cg.Initialize()
        ms = []
        for _ in range(2):                              # the first run warms up
            cg.vectorX.CopyFrom(sys_b.x, s.Count)
            _lib.lib().MgcgDeviceSynchronize()
            t0 = time.perf_counter()
            try:
                cg.Solve()
            except (ApplicationException, _lib.MgcgError):
                pass
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = dict(status=cg.status, iterations=cg.Iteration, seconds_to_solution=ms[-1] / 1e3, residual=cg.Residual, true_residual=cg.TrueResidual)
        cg.Dispose()
    return out


def run_leg(leg, cap, bodies, rate):
    from conjugategradient_amd import _lib

    _lib.require_gpu()
    which = TRACES.get(leg, leg)
    s, ls = build(which)
    model = byte_model(ls.Rows, ls.Columns, ls.nnz)
    out = dict(rows=ls.Rows, columns=ls.Columns, stored_entries=ls.nnz, byte_model_per_body=model,
               predicted_ms_per_body=sum(model.values()) / (rate * 1e12) * 1e3, rate_TBps=rate)
    cg, setup, run = lsqr_solve(ls, 1e-8, cap, _lib.RULE_VIENNACL)
    out["setup_seconds_upload_and_transposition"] = setup
    if leg in TRACES:
        out["traced"] = run(bodies)
        cg.Dispose()
        return out
    run(8)                                              # warms up: code objects, matrix shapes, the workspace
    out["fixed_bodies"] = run(bodies)
    if which == "convdiff256":
        out["to_relative_1e-8_in_g"] = run()
        out["to_relative_1e-8_in_g"]["seconds_to_solution"] = out["to_relative_1e-8_in_g"]["ms"] / 1e3
    cg.Dispose()
    if which == "convdiff256":
        out["others_to_relative_1e-8_in_r"] = others(s, ls.b, cap)
    return out


def readme(result):
    lines = ["# LSQR (MgcgSolveLsqr), one MI355X", "",
             "Written by `python -m conjugategradient_amd.tools.lsqr_run --out profiles/lsqr`; the numbers are in `lsqr_run.json`.",
             "x = 0, N(0,1) right-hand side.  `predicted`: the byte model of a body (two products, pass U, pass V) at the stated rate.", ""]
    for leg in LEGS:
        if leg not in result:
            continue
        r = result[leg]
        f = r["fixed_bodies"]
        lines += [f"## {leg} ({r['rows']} x {r['columns']}, {r['stored_entries']} stored entries)", "",
                  f"- set-up (upload and device transposition): {r['setup_seconds_upload_and_transposition']:.3f} s",
                  f"- {f['bodies']} bodies: {f['ms_per_body']:.3f} ms per body, predicted {r['predicted_ms_per_body']:.3f} at {r['rate_TBps']} TB/s"]
        if "to_relative_1e-8_in_g" in r:
            t = r["to_relative_1e-8_in_g"]
            lines.append(f"- to a relative 1e-8 in g: status {t['status']}, {t['bodies']} bodies, {t['seconds_to_solution']:.3f} s, "
                         f"|| b - A x || {t['true_residual']:.3e}, || A^T (b - A x) || {t['true_normal_residual']:.3e}")
            for name, o in r.get("others_to_relative_1e-8_in_r", {}).items():
                slower = "LSQR is slower today" if t["seconds_to_solution"] > o["seconds_to_solution"] else ""
                lines.append(f"- {name}: status {o['status']}, {o['iterations']} iterations, {o['seconds_to_solution']:.3f} s to solution, "
                             f"|| b - A x || {o['true_residual']:.3e}  {slower}")
        lines.append("")
    return "\n".join(lines)


def write(out, result):
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "lsqr_run.json"), "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    with open(os.path.join(out, "README.md"), "w") as f:
        f.write(readme(result) + "\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="a directory: lsqr_run.json and README.md are written there")
    ap.add_argument("--leg", choices=list(LEGS) + list(TRACES), default=None, help="run this leg in this process")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), help="the legs to run, each as a child process under its own time limit")
    ap.add_argument("--cap", type=int, default=MAX_BODIES, help="at most this many bodies (iterations of the other loops) per solve")
    ap.add_argument("--bodies", type=int, default=64, help="bodies of the fixed-length and traced runs")
    ap.add_argument("--rate", type=float, default=5.4, help="TB/s of the byte model's prediction")
    a = ap.parse_args()
    if a.leg:
        result = {a.leg: run_leg(a.leg, a.cap, a.bodies, a.rate)}
    else:
        result = {}
        for leg in a.legs:
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.lsqr_run", "--leg", leg, "--cap", str(a.cap), "--bodies", str(a.bodies),
                                    "--rate", str(a.rate)], stdout=subprocess.PIPE, timeout=LEGS[leg], check=True)      # a leg that fails or hangs ends the script
            result.update(json.loads(child.stdout))
            if a.out:                                      # what is measured so far survives a later leg's failure
                write(a.out, result)
    print(json.dumps(result, indent=1))
    if a.out:
        write(a.out, result)


if __name__ == "__main__":
    main()
