"""Measurement only: what BiCGStab (SolveBicgstab, SolveBicgstabJacobi) costs, on one GPU.  Every run starts from x = 0 with an N(0,1)
right-hand side and stops at || r || < 1e-8 || b || (MGCG_RULE_NATIVE).  No figure here is an acceptance threshold.

  poisson512, poisson256   n^3 7-point Poisson from the device generator: SolveBicgstab against SolveEx's loop (SolveParallel without a
                           communicator, default and x_defer = 1), the forms alternated inside every repeat of ONE process, median of the
                           repeats -- bodies, ms per body (time of the call / bodies run), time to solution, and the cost of a body over
                           that of a plain iteration beside the ratio the counted bytes predict
  convdiff256              256^3 convection_diffusion with c = (.5, .25, 0), which no other solver here handles: bodies, time, TrueResidual / Residual
  random                   random_nonsymmetric at 1 M rows x 31 per row: plain against Jacobi
  trace                    40 bodies of SolveBicgstab and of the plain loop (x_defer = 1) at 512^3, once, for a kernel trace

Without --leg every leg runs as a child process of its own under a time limit of its own, and the script ends at the first one that fails.

Byte model per row at 7 entries per row, stated, not measured: the product ~104; BiCGStab's passes 24 + 8 + 56 + 32 = 120, two products:
328 per body; the plain loop's passes 24 + 40, one product: 168 per iteration: 1.95 x per body.

    python -m conjugategradient_amd.tools.bicgstab_run --out profiles/bicgstab/bicgstab_run.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m conjugategradient_amd.tools.bicgstab_run --leg trace
    python conjugategradient_amd/tools/trace_kernel_medians.py OUT          (the rate at which each pass streams: bytes per row x rows / median)
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

BYTES = {"product": 104, "bicgstab_s_kernel": 24, "bicgstab_tau_kernel": 8, "bicgstab_x_kernel": 56, "bicgstab_p_kernel": 32,
         "jacobi_form": {"bicgstab_s_kernel": 40, "bicgstab_tau_kernel": 8, "bicgstab_x_kernel": 64, "bicgstab_p_kernel": 48},
         "update_r_kernel": 24, "update_xp_final_kernel": 40, "bicgstab": 328, "plain_x_defer_1": 168, "ratio": 328 / 168}
MAX_IT = 20000
LEGS = {"poisson512": 900, "poisson256": 300, "convdiff256": 600, "random": 300}      # the leg's time limit in seconds


def median(v):
    return sorted(v)[len(v) // 2]


class PoissonBench:
    """The n^3 Poisson matrix on the device with an N(0,1) right-hand side, and the two loops' calls on it."""

    def __init__(self, n):
        from conjugategradient_amd import _lib
        from conjugategradient_amd.parallel import ConjugateGradientRankGpu
        from conjugategradient_amd.solver import VectorDouble

        self._lib = _lib
        self.L = _lib.lib()
        self.n, self.N = n, n * n * n
        cg = ConjugateGradientRankGpu(self.N, 7, 0, MAX_IT, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE)
        cg.InitializePoisson(n, n, n)
        b = np.random.default_rng(7).standard_normal(self.N)
        cg.vectorB.CopyFrom(b, self.N)
        self.normb = float(np.linalg.norm(b))
        del b
        self.cg = cg
        self.work = [VectorDouble(self.N) for _ in range(4)]                  # v, s, t, rhat
        self.it, self.res, self.true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)

    def close(self):
        for v in self.work:
            v.Dispose()
        self.cg.Dispose()

    def run(self, loop, tol=None, cap=MAX_IT):
        """One solve from x = 0; returns (status, bodies run, ms of the call, Residual, TrueResidual or None)."""
        L, cg, p, _lib = self.L, self.cg, self.cg.part, self._lib
        tol = 1e-8 * self.normb if tol is None else tol
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        L.MgcgDeviceSynchronize()
        head = (None, cg.cublas, cg.cusparse, cg.matDescr, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr)
        part = (self.N, p.count, p.offset, p.elementCount, p.minJ, p.maxJ)
        stop = (tol, 0, cap, _lib.RULE_NATIVE, C.byref(self.it), C.byref(self.res))
        t0 = time.perf_counter()
        if loop == "plain":
            st = L.SolveParallel(*head, *part, *stop, None, 0)
        else:
            st = L.SolveBicgstabParallel(*head, *(v.Ptr for v in self.work), *part, *stop, C.byref(self.true), None, 0)
        ms = (time.perf_counter() - t0) * 1e3
        L.MgcgClearLastError()
        # the plain loop reports the index of its last body, BiCGStab the number of bodies run
        bodies = self.it.value + 1 if loop == "plain" else self.it.value
        return st, bodies, ms, self.res.value, (self.true.value if loop != "plain" else None)

    def compare(self, repeats):
        forms = (("plain_default", "plain", None), ("plain_x_defer_1", "plain", 1), ("bicgstab", "bicgstab", None))
        samples = {name: [] for name, _, _ in forms}
        out = dict(rows=self.N, relative_tolerance=1e-8, stop_level=1e-8 * self.normb)
        for rep in range(repeats + 1):                 # round 0 warms up: code objects, matrix shape, the workspace's vectors
            for name, loop, defer in forms:            # the forms alternate, so a drift of the machine meets all alike
                self.L.MgcgReloadEnvironment()
                if defer is not None:
                    assert self.L.MgcgSetTuning(b"x_defer", defer) == 0
                st, bodies, ms, res, true = self.run(loop)
                if rep:
                    samples[name].append(ms)
                out[name] = dict(status=st, bodies=bodies, residual=res, true_residual=true)
        self.L.MgcgReloadEnvironment()
        for name, _, _ in forms:
            med = median(samples[name])
            out[name].update(ms_to_solution=med, ms_per_body=med / max(out[name]["bodies"], 1), samples=samples[name])
        for base in ("plain_default", "plain_x_defer_1"):
            out[f"bicgstab_to_{base}"] = dict(bodies=out["bicgstab"]["bodies"] / out[base]["bodies"],
                                              ms_per_body=out["bicgstab"]["ms_per_body"] / out[base]["ms_per_body"],
                                              ms_to_solution=out["bicgstab"]["ms_to_solution"] / out[base]["ms_to_solution"],
                                              bytes_per_body=BYTES["ratio"])
        return out


def host_system(s, jacobi, repeats):
    """A system built on the host through the Python class; median of `repeats` solves behind one that warms up."""
    from conjugategradient_amd import _lib
    from conjugategradient_amd.bicgstab import BiConjugateGradientStabGpu, BiConjugateGradientStabJacobiGpu
    from conjugategradient_amd.solver import ApplicationException

    rng = np.random.default_rng(7)
    s.b = rng.standard_normal(s.Count)
    level = 1e-8 * float(np.linalg.norm(s.b))
    cls = BiConjugateGradientStabJacobiGpu if jacobi else BiConjugateGradientStabGpu
    cg = cls(s.Count, int(np.diff(s.RowOffsets).max()), 0, MAX_IT, level, rule=_lib.RULE_NATIVE).load(s)
    cg.Initialize()
    samples = []
    zero = np.zeros(s.Count)
    for rep in range(repeats + 1):
        cg.vectorX.CopyFrom(zero, s.Count)
        _lib.lib().MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        try:
            cg.Solve()
        except (ApplicationException, _lib.MgcgError):
            pass
        if rep:
            samples.append((time.perf_counter() - t0) * 1e3)
    med = median(samples)
    out = dict(rows=s.Count, nonzeros=s.nnz, jacobi=jacobi, status=cg.status, bodies=cg.Iteration, ms_to_solution=med, ms_per_body=med / max(cg.Iteration, 1),
               residual=cg.Residual, true_residual=cg.TrueResidual, true_to_residual=cg.TrueResidual / cg.Residual if cg.Residual else None,
               stop_level=level, samples=samples)
    cg.Dispose()
    return out


def run_leg(leg, repeats):
    from conjugategradient_amd import _lib, problems

    _lib.require_gpu()
    if leg in ("poisson512", "poisson256"):
        b = PoissonBench(int(leg[len("poisson"):]))
        out = b.compare(repeats)
        b.close()
        return out
    if leg == "convdiff256":
        return host_system(problems.convection_diffusion(256, 256, 256, (0.5, 0.25, 0.0)), False, repeats)
    if leg == "random":
        return [host_system(problems.random_nonsymmetric(1_000_000, 31, 12345), jacobi, repeats) for jacobi in (False, True)]
    if leg == "trace":
        b = PoissonBench(512)
        assert b.L.MgcgSetTuning(b"x_defer", 1) == 0             # update_r_kernel + update_xp_final_kernel every iteration
        b.run("plain", tol=0.0, cap=39)
        b.L.MgcgReloadEnvironment()
        b.run("bicgstab", tol=0.0, cap=39)
        b.close()
        return dict(n=512, bodies=40)
    raise SystemExit(f"unknown leg {leg}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--leg", choices=list(LEGS) + ["trace"], default=None, help="run this leg in this process")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), help="the legs to run, each as a child process under its own time limit")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        result = {a.leg: run_leg(a.leg, a.repeats)}
    else:
        result = {"byte_model_per_row": BYTES}
        for leg in a.legs:
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.bicgstab_run", "--leg", leg, "--repeats", str(a.repeats)],
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
