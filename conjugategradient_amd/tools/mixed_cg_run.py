"""Measurement only: the mixed-precision loop (SolveMixed) against SolveEx at its defaults, in one process on one GPU.

1. Per-iteration time at n^3 7-point Poisson: both loops forced (tolerance 0 under an iteration cap) for two lengths; the time of the
   shorter run is subtracted from the longer one's so that the set-up of a call drops out.  SolveMixed stops at the first update slot
   behind its cap, so its lengths are read off the returned iteration.  The forms alternate inside every round; median of the rounds.
2. Full solves at n^3 to a relative 1e-8 (MGCG_RULE_VIENNACL): one seeded N(0,1) right-hand side, and b = A 1.  Iterations, reliable
   updates, seconds to solution and the final TRUE residual || b - A x || / || b ||, recomputed with CsrMV for both loops.
3. The same on the driver matrix ``problems.viennacl_main()``.

    python -m conjugategradient_amd.tools.mixed_cg_run --out profiles/mixed/mixed_cg_run.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m conjugategradient_amd.tools.mixed_cg_run --only mixed
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import time

import numpy as np

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.solver import ConjugateGradientSingleGpu, VectorDouble


def median(v):
    return sorted(v)[len(v) // 2]


class Bench:
    """One matrix on the device with the vectors of both loops."""

    def __init__(self, cg, nnz, n, vecE, vecRo, vecC):
        L = _lib.lib()
        self.cg, self.nnz, self.n, self.E, self.Ro, self.Ci = cg, int(nnz), int(n), vecE, vecRo, vecC
        self.e32 = VectorDouble((self.nnz + 1) // 2)
        self.work = VectorDouble(self.n)
        exact = C.c_int(0)
        if L.MgcgMixedSetup(cg.cusparse, vecE.Ptr, vecRo.Ptr, vecC.Ptr, self.nnz, self.n, self.e32.Ptr, C.byref(exact)) != 0:
            _lib.check("MgcgMixedSetup")
        self.exact = bool(exact.value)

    def run(self, mixed, tol, cap, rule):
        L, cg = _lib.lib(), self.cg
        it, res, up = C.c_int(0), C.c_double(0.0), C.c_int(0)
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        L.MgcgDeviceSynchronize()
        common = (cg.cublas, cg.cusparse, cg.matDescr, self.E.Ptr, self.Ro.Ptr, self.Ci.Ptr, cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr)
        t0 = time.perf_counter()
        if mixed:
            st = L.SolveMixed(*common, self.e32.Ptr, self.nnz, self.n, tol, 0, cap, rule, C.byref(it), C.byref(res), C.byref(up), None, 0)
        else:
            st = L.SolveEx(*common, self.nnz, self.n, tol, 0, cap, rule, C.byref(it), C.byref(res), None, 0)
        seconds = time.perf_counter() - t0
        L.MgcgClearLastError()
        return dict(status=st, loop_bodies=it.value + 1, residual=res.value, reliable_updates=up.value if mixed else None, seconds=seconds)

    def true_relative_residual(self):
        """|| b - A x || / || b || with the library's own fp64 product and dots."""
        L, cg = _lib.lib(), self.cg
        raw = L.ToRawPtr_Double
        w, x, b = raw(self.work.Ptr), raw(cg.vectorX.Ptr), raw(cg.vectorB.Ptr)
        L.CsrMV(cg.cusparse, cg.matDescr, w, raw(self.E.Ptr), L.ToRawPtr_Int(self.Ro.Ptr), L.ToRawPtr_Int(self.Ci.Ptr), x, self.nnz, self.n, self.n, -1.0, 0.0)
        L.Axpy(cg.cublas, w, b, self.n, 1.0)
        rr = L.Dot(cg.cublas, w, w, self.n)
        bb = L.Dot(cg.cublas, b, b, self.n)
        _lib.check("true residual")
        return math.sqrt(rr / bb)

    def per_iteration(self, k1, k2, rounds):
        samples = {"plain": [], "mixed": []}
        for rep in range(rounds + 1):                     # round 0 warms up: code objects, the ring of the deferred x update, the fp32 work vectors
            for name in ("plain", "mixed"):               # the forms alternate, so a drift of the machine meets both alike
                a, b = self.run(name == "mixed", 0.0, k1, _lib.RULE_NATIVE), self.run(name == "mixed", 0.0, k2, _lib.RULE_NATIVE)
                assert a["status"] == b["status"] == _lib.MAXIT_EXCEEDED, (a, b)
                if rep:
                    samples[name].append((b["seconds"] - a["seconds"]) * 1e3 / (b["loop_bodies"] - a["loop_bodies"]))
        out = {name: dict(ms_per_iteration=median(v), samples=v) for name, v in samples.items()}
        out["ratio_plain_over_mixed"] = out["plain"]["ms_per_iteration"] / out["mixed"]["ms_per_iteration"]
        out["byte_model_ratio"] = 168.0 / 100.0
        return out

    def full_solve(self, rel, cap, rounds):
        out = {}
        for name in ("plain", "mixed"):
            out[name] = []
        for rep in range(rounds + 1):
            for name in ("plain", "mixed"):
                r = self.run(name == "mixed", rel, cap, _lib.RULE_VIENNACL)
                r["true_relative_residual"] = self.true_relative_residual()
                if rep:
                    out[name].append(r)
        res = {}
        for name, runs in out.items():
            res[name] = dict(runs[0], seconds=median([r["seconds"] for r in runs]), seconds_all=[r["seconds"] for r in runs])
        res["speedup_to_solution"] = res["plain"]["seconds"] / res["mixed"]["seconds"]
        res["iteration_ratio"] = res["mixed"]["loop_bodies"] / res["plain"]["loop_bodies"]
        return res

    def dispose(self):
        self.e32.Dispose()
        self.work.Dispose()


def poisson(n, caps, rounds, rel, only, skip_full):
    L = _lib.lib()
    N = n ** 3
    cg = ConjugateGradientRankGpu(N, 7, 0, 10, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE)
    cg.InitializePoisson(n, n, n)
    B = Bench(cg, cg.part.elementCount, N, cg.vectorElements, cg.vectorRowOffsets, cg.vectorColumnIndeces)
    out = dict(n=n, rows=N, nnz=B.nnz, exact=B.exact)
    if only:                                              # one forced call for a kernel trace
        out["only"] = dict(form=only, **B.run(only == "mixed", 0.0, caps[0], _lib.RULE_NATIVE))
    else:
        out["per_iteration"] = B.per_iteration(caps[0], caps[1], rounds)
        if not skip_full:
            cap = 20 * n
            b = np.random.default_rng(20261018).standard_normal(N)
            cg.vectorB.CopyFrom(b, N)
            del b
            out["random_rhs"] = B.full_solve(rel, cap, rounds)
            L.MgcgFill(cg.vectorX.Ptr, 1.0)               # b = A 1
            L.CsrMV(cg.cusparse, cg.matDescr, L.ToRawPtr_Double(cg.vectorB.Ptr), L.ToRawPtr_Double(B.E.Ptr), L.ToRawPtr_Int(B.Ro.Ptr), L.ToRawPtr_Int(B.Ci.Ptr),
                    L.ToRawPtr_Double(cg.vectorX.Ptr), B.nnz, N, N, 1.0, 0.0)
            _lib.check("b = A 1")
            out["a_times_ones_rhs"] = B.full_solve(rel, cap, rounds)
    B.dispose()
    cg.Dispose()
    return out


def driver_matrix(rel, rounds):
    s = problems.viennacl_main()
    cg = ConjugateGradientSingleGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, s.Count, rel, rule=_lib.RULE_VIENNACL).load(s)
    cg.Initialize()
    B = Bench(cg, s.nnz, s.Count, cg.vectorA, cg.vectorRowOffsets, cg.vectorColumnIndeces)
    out = dict(rows=s.Count, nnz=int(s.nnz), exact=B.exact, relative_tolerance=rel, **B.full_solve(rel, s.Count, rounds))
    B.dispose()
    cg.Dispose()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--caps", type=int, nargs=2, default=[22, 122])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--rel", type=float, default=1e-8)
    ap.add_argument("--skip-driver", action="store_true")
    ap.add_argument("--skip-full", action="store_true", help="per-iteration times only")
    ap.add_argument("--only", choices=["plain", "mixed"], default=None, help="run only this loop at n^3, once, forced for caps[0] iterations (for a kernel trace)")
    a = ap.parse_args()
    _lib.require_gpu()
    result = {"poisson": poisson(a.n, a.caps, a.rounds, a.rel, a.only, a.skip_full)}
    if not a.skip_driver and not a.only:
        result["viennacl_main"] = driver_matrix(a.rel, a.rounds)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
