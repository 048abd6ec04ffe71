"""Measurement only: what MINRES (SolveMinres) costs next to SolveEx on the 7-point Poisson matrix, in one process on one GPU, the forms
alternated inside every repeat, median of the repeats.  No figure here is an acceptance threshold.

  definite    n^3 Poisson (--n 256 512) from the device generator with an N(0,1) right-hand side, to a relative 1e-8: SolveMinres with
              shift 0 against SolveEx's loop -- iterations, ms per iteration (time of the call / bodies run), time to solution
  indefinite  256^3 with shift 0.01 and 0.05: iterations, ms per iteration, TrueResidual against Residual

Byte model per row and iteration at 7 entries per row, stated, not measured: the product ~104, MINRES' passes 32 + 64 = 200 in all;
the plain loop's passes 64 = 168 in all: 1.19 x per iteration.

    python -m conjugategradient_amd.tools.minres_run --out profiles/minres/minres_run.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m conjugategradient_amd.tools.minres_run --only both --n 512
    python conjugategradient_amd/tools/trace_kernel_medians.py OUT          (the rate at which each pass streams: bytes per row x rows / median)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import time

import numpy as np

from conjugategradient_amd import _lib
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.solver import VectorDouble

BYTES = {"product": 104, "minres_lanczos_kernel": 32, "minres_update_kernel": 64, "update_r_kernel": 24, "update_xp_final_kernel": 40,
         "minres": 200, "plain_x_defer_1": 168, "ratio": 200 / 168}
MAX_IT = 20000


class Bench:
    """The n^3 Poisson matrix on the device with an N(0,1) right-hand side, and the two loops' calls on it."""

    def __init__(self, n):
        self.L = _lib.lib()
        self.n, self.N = n, n * n * n
        cg = ConjugateGradientRankGpu(self.N, 7, 0, MAX_IT, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE)
        cg.InitializePoisson(n, n, n)
        b = np.random.default_rng(7).standard_normal(self.N)
        cg.vectorB.CopyFrom(b, self.N)
        self.normb = float(np.linalg.norm(b))
        del b
        cg.vectorR.Dispose()
        cg.vectorR = VectorDouble(self.N)
        self.cg, self.w1, self.w2 = cg, VectorDouble(self.N), VectorDouble(self.N)
        self.it, self.res, self.true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)

    def close(self):
        self.w1.Dispose()
        self.w2.Dispose()
        self.cg.Dispose()

    def run(self, loop, shift=0.0, tol=None, cap=MAX_IT):
        """One solve from x = 0; returns (status, bodies run, ms of the call, Residual, TrueResidual or None)."""
        L, cg, p = self.L, self.cg, self.cg.part
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
            st = L.SolveMinresParallel(*head, self.w1.Ptr, self.w2.Ptr, *part, float(shift), *stop, C.byref(self.true), None, 0)
        ms = (time.perf_counter() - t0) * 1e3
        L.MgcgClearLastError()
        # the plain loop reports the index of its last body, MINRES the number of bodies run
        bodies = self.it.value + 1 if loop == "plain" else self.it.value
        return st, bodies, ms, self.res.value, (self.true.value if loop != "plain" else None)

    def definite(self, repeats):
        forms = (("plain_default", "plain", None), ("plain_x_defer_1", "plain", 1), ("minres", "minres", None))
        samples = {name: [] for name, _, _ in forms}
        out = dict(rows=self.N, relative_tolerance=1e-8)
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
            med = sorted(samples[name])[len(samples[name]) // 2]
            out[name].update(ms_to_solution=med, ms_per_iteration=med / max(out[name]["bodies"], 1), samples=samples[name])
        for base in ("plain_default", "plain_x_defer_1"):
            out[f"minres_to_{base}"] = dict(iterations=out["minres"]["bodies"] / out[base]["bodies"],
                                            ms_per_iteration=out["minres"]["ms_per_iteration"] / out[base]["ms_per_iteration"],
                                            ms_to_solution=out["minres"]["ms_to_solution"] / out[base]["ms_to_solution"])
        return out

    def indefinite(self, shift, repeats):
        samples, last = [], None
        for rep in range(repeats + 1):
            last = self.run("minres", shift)
            if rep:
                samples.append(last[2])
        st, bodies, _, res, true = last
        med = sorted(samples)[len(samples) // 2]
        return dict(shift=shift, status=st, bodies=bodies, ms_to_solution=med, ms_per_iteration=med / max(bodies, 1), residual=res,
                    true_residual=true, true_to_residual=true / res if res else None, stop_level=1e-8 * self.normb, samples=samples)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--n", type=int, nargs="*", default=[256, 512], help="n of the n^3 definite runs")
    ap.add_argument("--shifts", type=float, nargs="*", default=[0.01, 0.05], help="shifts of the indefinite runs at 256^3")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["minres", "plain", "both"], default=None,
                    help="run only these loops at the first n, once, for 40 bodies (for a kernel trace)")
    a = ap.parse_args()
    _lib.require_gpu()
    result = {"byte_model_per_row": BYTES}
    if a.only:
        b = Bench(a.n[0])
        if a.only in ("plain", "both"):
            assert b.L.MgcgSetTuning(b"x_defer", 1) == 0         # update_r_kernel + update_xp_final_kernel every iteration
            b.run("plain", tol=0.0, cap=40)
            b.L.MgcgReloadEnvironment()
        if a.only in ("minres", "both"):
            b.run("minres", tol=0.0, cap=40)
        b.close()
        result["only"] = dict(form=a.only, n=a.n[0], bodies=41)
    else:
        for n in a.n:
            b = Bench(n)
            result[f"poisson{n}"] = b.definite(a.repeats)
            if n == 256:
                result["poisson256_indefinite"] = [b.indefinite(s, a.repeats) for s in a.shifts]
            b.close()
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
