"""Measurement only: multicolour ILU(0) (MgSetupIlu0) against the plain loop, the diagonal and one-level SSOR ON THE SAME SYSTEM in the
same process.

Every system is a leg of its own: a child process under its own time limit, so that one leg's failure or timeout costs the others nothing.
A leg puts the matrix on the device once, then measures the forms "plain", "jacobi", "ssor" (MgSetupAggregates with levels = 1, nuCoarse = 2,
omega = 1 and MgSetSmoother(mg, 1)) and "ilu" (MgSetupIlu0, shift 0) under the leg's loops.  Reported:

  setup             ilu: MgIluSetupMs's split (checks and colouring, building B, factorisation) and the wall time of the call with the
                    device drained either side; ssor: the wall time of the two calls
  ms_per_application  MgApply enqueued K times between two device synchronisations, median of the repeats (gs_smoother_run's measure), the
                    byte model beside it and the rate model / time
  to_1e-8           one solve from x = 0 to || r || < 1e-8 || b ||, N(0,1) right-hand side: status, iterations and seconds, per loop
  bytes_model       ilu: 12 B per entry (values and columns once) + 72 B per row (offsets and diagonal positions in both passes 16, pinv 8,
                    rowOf twice 8, r 8, y written and read 16, t 8, z 8); the gathers of y and t are not counted, as x is not in a product's.
                    ssor: two sweeps of 12 B per entry + 40 B per row (gs_smoother_run's model)

  poisson256    256^3 7-point Poisson (device generator): CG
  permuted128   the 128^3 matrix with rows and columns permuted: CG
  convdiff256   256^3 central convection-diffusion, c = (.5, .25, 0): BiCGStab and GMRES(10)
  upwind256     256^3 upwind convection-diffusion, c = (2, 1, .5): BiCGStab and GMRES(10)
  random1m      problems.random_spd(1 000 000): CG
  viennacl      problems.viennacl_main(): CG
Where a set-up refuses (colours, pivots) the refusal is the record.  --n scales the three 256^3 legs down.

    python -m conjugategradient_amd.tools.ilu_run --out profiles/ilu/ilu_run.json
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

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.solver import ApplicationException, _ptr
from conjugategradient_amd.tools.amg_cg_run import Bench, permuted_poisson, randn_rhs
from conjugategradient_amd.tools.gs_smoother_run import cycle_ms

LEGS = ("poisson256", "permuted128", "convdiff256", "upwind256", "random1m", "viennacl")
NONSYMMETRIC = ("convdiff256", "upwind256")
SEED = 20261019
GMRES_M = 10


def make_bench(leg, n):
    """Bench of a leg: the matrix on the device behind a one-level ConjugateGradientAmgGpu (whose own hierarchy is not measured)."""
    if leg == "poisson256":
        cg = ConjugateGradientAmgGpu(n ** 3, 7, 0, 10, 0.0, levels=1, aggregates=[])
        cg.InitializePoisson((n, n, n))
        return Bench(cg, randn_rhs(cg))
    s = {"permuted128": lambda: permuted_poisson(n // 2),
         "convdiff256": lambda: problems.convection_diffusion(n, n, n, c=(0.5, 0.25, 0.0)),
         "upwind256": lambda: problems.convection_diffusion(n, n, n, c=(2.0, 1.0, 0.5), upwind=True),
         "random1m": lambda: problems.random_spd(1_000_000),
         "viennacl": problems.viennacl_main}[leg]()
    s.b = np.random.default_rng(SEED).standard_normal(s.Count)
    cg = ConjugateGradientAmgGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 10, 0.0, levels=1, aggregates=[]).load(s)
    cg.Initialize()
    return Bench(cg, float(np.linalg.norm(s.b)))


def krylov(b, loop, form, tol, cap):
    """One BiCGStab or GMRES(10) solve from x = 0 through the object's native-call path: (status, iterations, seconds)."""
    cg, L = b.cg, b.L
    cg._ensure_vectors(b.N, "vectorV", "vectorS", "vectorT", "vectorRhat")
    cg._ensure_work(2 * GMRES_M + 1)
    L.MgcgFill(cg.vectorX.Ptr, 0.0)
    L.MgcgDeviceSynchronize()
    cg.AllowableResidual, cg.MinIteration, cg.MaxIteration = tol, 0, cap
    mg = () if form in ("plain", "jacobi") else (b.mg[form][0],)
    more = (b.dinv.Ptr,) if form == "jacobi" else ()
    suffix = {"plain": "", "jacobi": "Jacobi"}.get(form, "Mg")
    if loop == "bicgstab":
        work = (cg.vectorV.Ptr, cg.vectorS.Ptr, cg.vectorT.Ptr, cg.vectorRhat.Ptr, *more)
    else:
        work = (cg.vectorWork.Ptr, *more, GMRES_M, 2)
    t0 = time.perf_counter()
    try:
        cg._native_solve(("SolveBicgstab" if loop == "bicgstab" else "SolveGmres") + suffix, loop, False, head=mg, work=work, third=("TrueResidual", float("nan")))
    except (ApplicationException, _lib.MgcgError):
        pass
    seconds = time.perf_counter() - t0
    L.MgcgClearLastError()
    return cg.status, cg.Iteration, seconds, cg.TrueResidual


def run_leg(leg, n, repeats):
    b = make_bench(leg, n)
    L = b.L
    N, nnz = b.N, b.nnz
    out = dict(rows=N, nnz=nnz)
    forms = ["plain", "jacobi"]
    # one level, forward + backward sweep, omega = 1: SSOR
    rows, none = np.asarray([N], dtype=np.int32), np.zeros(1, dtype=np.int32)
    try:
        b.setup("ssor", lambda L_, *m: L_.MgSetupAggregates(*m, N, 1, _ptr(rows), _ptr(none), 1.0, 1, 2, 0.5))
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        status = L.MgSetSmoother(b.mg["ssor"][0], 1)
        L.MgcgDeviceSynchronize()
        if status != 0:
            raise _lib.MgcgError(_lib.last_error())
        out["ssor"] = dict(setup_seconds=b.mg["ssor"][1] + time.perf_counter() - t0, colours=int(L.MgLevelColours(b.mg["ssor"][0], 0)),
                           bytes_model=2 * (12 * nnz + 40 * N))
        forms.append("ssor")
    except _lib.MgcgError as err:
        out["ssor"] = dict(refused=str(err))
        if "ssor" in b.mg:
            L.MgDestroy(b.mg.pop("ssor")[0])
    L.MgcgClearLastError()
    try:
        b.setup("ilu", lambda L_, *m: L_.MgSetupIlu0(*m, N, 0.0))
        mg = b.mg["ilu"][0]
        ms, lo, hi = np.zeros(3), C.c_double(0.0), C.c_double(0.0)
        L.MgIluSetupMs(mg, _ptr(ms))
        L.MgIluPivotRange(mg, C.byref(lo), C.byref(hi))
        out["ilu"] = dict(setup_seconds=b.mg["ilu"][1], setup_ms=dict(colouring=ms[0], building_b=ms[1], factorisation=ms[2]), colours=int(L.MgIluColours(mg)),
                          pivots=[lo.value, hi.value], bytes_model=12 * nnz + 72 * N)
        forms.append("ilu")
    except _lib.MgcgError as err:
        out["ilu"] = dict(refused=str(err))
        b.mg.pop("ilu", None)
    L.MgcgClearLastError()
    for form in forms[2:]:
        median, samples = cycle_ms(b, b.mg[form][0], 20, repeats)
        out[form].update(ms_per_application=median, application_samples=samples, model_gb_per_s=out[form]["bytes_model"] / median / 1e6)
    tol = 1e-8 * b.bnorm
    if leg in NONSYMMETRIC:
        for loop in ("bicgstab", "gmres10"):
            for form in forms:
                krylov(b, loop, form, 0.0, 3)                      # warm-up: the first call of a loop pays for its workspace
                st, it, seconds, true = krylov(b, loop, form, tol, 20000)
                out.setdefault(form, {})[loop + "_to_1e-8"] = dict(status=st, iterations=it, seconds=seconds, true_residual_over_b=true / b.bnorm)
    else:
        for form in forms:
            b.call(form, 0.0, 3)                                   # warm-up: the first call of a loop pays for its workspace
            st, it, ms = b.call(form, tol, 20000)
            out.setdefault(form, {})["cg_to_1e-8"] = dict(status=st, iterations=it, seconds=ms / 1e3, residual_over_b=b.res.value / b.bnorm)
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=LEGS)
    ap.add_argument("--leg", default=None, choices=LEGS, help="run this one leg in this process and print its JSON (what the parent starts)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--n", type=int, default=256, help="the grid of the stencil legs is n^3 (permuted: (n / 2)^3)")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        _lib.require_gpu()
        print("RESULT " + json.dumps(run_leg(a.leg, a.n, a.repeats)), flush=True)
        return
    result = {}
    for leg in a.legs:
        cmd = [sys.executable, "-m", "conjugategradient_amd.tools.ilu_run", "--leg", leg, "--n", str(a.n), "--repeats", str(a.repeats)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            result[leg] = dict(error=f"timed out after {a.timeout} s")
            print(leg, json.dumps(result[leg]), flush=True)
            break                                                 # a leg that hangs: start nothing more on the device
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")]
        if done.returncode != 0 or not lines:
            result[leg] = dict(error=f"exit status {done.returncode}", stderr=done.stderr[-2000:])
            print(leg, json.dumps(result[leg]), flush=True)
            if done.returncode < 0 or done.returncode in (134, 139):
                break                                             # a fault: start nothing more on the device
            continue
        result[leg] = json.loads(lines[-1][len("RESULT "):])
        print(leg, json.dumps(result[leg]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
