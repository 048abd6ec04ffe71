"""Measurement only: what preconditioned MINRES (SolveMinresJacobi, SolveMinresMg) costs and gains next to SolveMinres in the same build, in
one process on one GPU, the forms alternated inside every repeat, median of the repeats.  No figure here is an acceptance threshold.

Every run starts from x = 0 with an N(0,1) right-hand side and stops at a relative 1e-8 IN THE NORM ITS RECURRENCE SEES
(MGCG_RULE_VIENNACL: phibar^2 / beta1^2 < 1e-16) -- the 2-norm for SolveMinres, the M^-1 norm for the preconditioned loops -- or at the cap
of 20 000 bodies; the 2-norm of the true residual relative to || b ||_2 is recorded next to it for every form.

  vcycle   256^3 Poisson (device generator) with shift 0.01 and 0.05: SolveMinres against SolveMinresMg with the geometric hierarchy (MgSetup)
           and with the aggregation hierarchy (MgSetupAggregation), both built from the matrix itself: bodies, ms per body, seconds to the
           end, TrueResidual and Residual, and whether the run converged within the cap
  jacobi   viennacl_main() at full size with shift 0 and 60: SolveMinres against SolveMinresJacobi
  body     512^3 Poisson, 200 bodies (tolerance 0): ms per body of SolveMinres and of SolveMinresJacobi with shift 0 and shift 0.01, next to
           the byte ratios 216 / 200 and 224 / 200

Byte model per row and body at 7 entries per row, stated, not measured: the product ~104; MINRES' passes 32 + 64, 200 in all; the
Jacobi form's passes 48 + 72 (40 + 72 with shift 0), 224 (216) in all.

    python -m conjugategradient_amd.tools.pminres_run --out profiles/pminres/pminres_run.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m conjugategradient_amd.tools.pminres_run --only trace
    python conjugategradient_amd/tools/trace_kernel_medians.py OUT          (the rate at which each pass streams: bytes per row x rows / median)
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import time

import numpy as np

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.minres import MinimalResidualGpu, MinimalResidualJacobiGpu
from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.solver import ApplicationException, VectorDouble

BYTES = {"product": 104, "minres_lanczos_kernel": 32, "minres_update_kernel": 64, "pminres_lanczos_kernel": 48, "pminres_lanczos_kernel_shift_0": 40,
         "pminres_update_kernel": 72, "minres": 200, "jacobi": 224, "jacobi_shift_0": 216, "ratio": 224 / 200, "ratio_shift_0": 216 / 200}
MAX_IT = 20000
REL = 1e-8
STATUS = {_lib.OK: "MGCG_OK", _lib.MAXIT_EXCEEDED: "MGCG_MAXIT_EXCEEDED", _lib.NONFINITE: "MGCG_NONFINITE", _lib.ERROR: "MGCG_ERROR"}


def timed(cg, solve):
    """One solve from x = 0; the cap and a breakdown are results.  Returns a dict of what the call left."""
    L = _lib.lib()
    L.MgcgFill(cg.vectorX.Ptr, 0.0)
    L.MgcgDeviceSynchronize()
    t0 = time.perf_counter()
    try:
        solve()
    except (ApplicationException, _lib.MgcgError):
        pass
    ms = (time.perf_counter() - t0) * 1e3
    L.MgcgClearLastError()
    return dict(status=STATUS.get(cg.status, cg.status), bodies=cg.Iteration, ms=ms, residual=cg.Residual, true_residual=cg.TrueResidual)


WARM_BODIES = 50


def alternate(forms, repeats):
    """forms: name -> callable(cap) returning timed()'s dict.  Round 0 warms up (code objects, matrix shape, the work space) with a cap of
    WARM_BODIES bodies; the forms alternate inside every repeat."""
    samples, last = {name: [] for name in forms}, {}
    for rep in range(repeats + 1):
        for name, run in forms.items():
            last[name] = run(MAX_IT if rep else WARM_BODIES)
            if rep:
                samples[name].append(last[name]["ms"])
    out = {}
    for name in forms:
        med = sorted(samples[name])[len(samples[name]) // 2]
        r = dict(last[name])
        del r["ms"]
        r.update(s_to_the_end=med / 1e3, ms_per_body=med / max(r["bodies"], 1), samples_ms=samples[name])
        out[name] = r
    return out


def plain_on(cg, shift, nnz, cap):
    """SolveMinres on the vectors of a multigrid class (its r vector has `Count` entries); w1 and w2 are those of its SolveMinres method."""
    L = _lib.lib()
    it, res, true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)
    for name in ("vectorW1", "vectorW2"):
        if getattr(cg, name, None) is None:
            setattr(cg, name, VectorDouble(cg.Count))

    def solve():
        cg.status = L.SolveMinres(cg.cublas, cg.cusparse, cg.matDescr, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                                  cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr, cg.vectorW1.Ptr, cg.vectorW2.Ptr,
                                  nnz, cg.Count, float(shift), REL, 0, cap, _lib.RULE_VIENNACL, C.byref(it), C.byref(res), C.byref(true), None, 0)
        cg.Iteration, cg.Residual, cg.TrueResidual = it.value, res.value, true.value

    return solve


def vcycle(n, shifts, repeats, kinds=("geometric", "aggregation")):
    """n^3 Poisson: SolveMinres against SolveMinresMg, per hierarchy (each class holds its own copy of the matrix)."""
    N = n * n * n
    b = np.random.default_rng(7).standard_normal(N)
    normb = float(np.linalg.norm(b))
    out = dict(rows=N, relative_tolerance=REL, cap=MAX_IT, norm_b=normb, hierarchies={})
    for kind in kinds:
        t0 = time.perf_counter()
        if kind == "geometric":
            cg = ConjugateGradientMgGpu(N, 7, 0, MAX_IT, REL, (n, n, n), rule=_lib.RULE_VIENNACL)
            cg.InitializePoisson()
        else:
            cg = ConjugateGradientAmgGpu(N, 7, 0, MAX_IT, REL, rule=_lib.RULE_VIENNACL)
            cg.InitializePoisson((n, n, n))
        _lib.lib().MgcgDeviceSynchronize()
        setup_s = time.perf_counter() - t0
        cg.vectorB.CopyFrom(b, N)
        L = _lib.lib()
        rows = [int(L.MgLevelRows(cg.mg, l)) for l in range(cg.levels)]
        runs = []
        for shift in shifts:
            def with_cycle(cap, s=shift):
                cg.MaxIteration = cap
                return timed(cg, lambda: cg.SolveMinres(shift=s))

            forms = {"minres": lambda cap, s=shift: timed(cg, plain_on(cg, s, cg._nnz, cap)), "vcycle": with_cycle}
            r = alternate(forms, repeats)
            for f in r.values():
                f["relative_true_residual"] = f["true_residual"] / normb
                f["converged_within_the_cap"] = f["status"] == "MGCG_OK"
            r["shift"] = shift
            r["vcycle_to_minres"] = dict(bodies=r["vcycle"]["bodies"] / r["minres"]["bodies"], ms_per_body=r["vcycle"]["ms_per_body"] / r["minres"]["ms_per_body"],
                                         s_to_the_end=r["vcycle"]["s_to_the_end"] / r["minres"]["s_to_the_end"])
            runs.append(r)
            print(json.dumps({kind: r}), flush=True)
        out["hierarchies"][kind] = dict(levels=cg.levels, level_rows=rows, setup_s_with_the_matrix=setup_s, runs=runs)
        cg.Dispose()
    return out


def jacobi(shifts, repeats, n=None):
    """viennacl_main(): SolveMinres against SolveMinresJacobi, each to a relative 1e-8 in its own norm."""
    s = problems.viennacl_main() if n is None else problems.viennacl_main(n)
    s.b = np.random.default_rng(7).standard_normal(s.Count)
    normb = float(np.linalg.norm(s.b))
    maxnz = int(np.diff(s.RowOffsets).max())
    out = dict(rows=s.Count, nnz=int(s.RowOffsets[s.Count]), relative_tolerance=REL, cap=MAX_IT, norm_b=normb, runs=[])
    for shift in shifts:
        a = MinimalResidualGpu(s.Count, maxnz, 0, MAX_IT, REL, rule=_lib.RULE_VIENNACL, shift=shift).load(s)
        p = MinimalResidualJacobiGpu(s.Count, maxnz, 0, MAX_IT, REL, rule=_lib.RULE_VIENNACL, shift=shift).load(s)
        a.Initialize()
        p.Initialize()
        def of(cg):
            def run(cap):
                cg.MaxIteration = cap
                return timed(cg, cg.Solve)
            return run

        r = alternate({"minres": of(a), "jacobi": of(p)}, repeats)
        for f in r.values():
            f["relative_true_residual"] = f["true_residual"] / normb
        r["shift"] = shift
        r["jacobi_to_minres"] = dict(bodies=r["jacobi"]["bodies"] / r["minres"]["bodies"], ms_per_body=r["jacobi"]["ms_per_body"] / r["minres"]["ms_per_body"],
                                     s_to_the_end=r["jacobi"]["s_to_the_end"] / r["minres"]["s_to_the_end"])
        out["runs"].append(r)
        print(json.dumps({"jacobi": r}), flush=True)
        a.Dispose()
        p.Dispose()
    return out


class Body:
    """The n^3 Poisson matrix on the device with an N(0,1) right-hand side: a fixed number of bodies of SolveMinres and of SolveMinresJacobi."""

    def __init__(self, n):
        self.L = _lib.lib()
        self.N = n * n * n
        cg = ConjugateGradientRankGpu(self.N, 7, 0, MAX_IT, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE)
        cg.InitializePoisson(n, n, n)
        cg.vectorB.CopyFrom(np.random.default_rng(7).standard_normal(self.N), self.N)
        cg.vectorR.Dispose()
        cg.vectorR = VectorDouble(self.N)
        cg.SetupJacobi()
        self.cg, self.w1, self.w2, self.r1 = cg, VectorDouble(self.N), VectorDouble(self.N), VectorDouble(self.N)
        self.it, self.res, self.true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)

    def close(self):
        for v in (self.w1, self.w2, self.r1):
            v.Dispose()
        self.cg.Dispose()

    def run(self, loop, shift, cap):
        L, cg, p = self.L, self.cg, self.cg.part
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        L.MgcgDeviceSynchronize()
        head = (None, cg.cublas, cg.cusparse, cg.matDescr, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr)
        tail = (self.N, p.count, p.offset, p.elementCount, p.minJ, p.maxJ, float(shift), 0.0, 0, cap, _lib.RULE_NATIVE,
                C.byref(self.it), C.byref(self.res), C.byref(self.true), None, 0)
        t0 = time.perf_counter()
        if loop == "minres":
            st = L.SolveMinresParallel(*head, self.w1.Ptr, self.w2.Ptr, *tail)
        else:
            st = L.SolveMinresJacobiParallel(*head, self.r1.Ptr, self.w1.Ptr, self.w2.Ptr, cg.vectorDinv.Ptr, *tail)
        ms = (time.perf_counter() - t0) * 1e3
        L.MgcgClearLastError()
        return dict(status=STATUS.get(st, st), bodies=self.it.value, ms=ms, residual=self.res.value, true_residual=self.true.value)

    def cost(self, bodies, repeats):
        def of(loop, shift):
            return lambda cap: self.run(loop, shift, min(cap, bodies) - 1)

        forms = {"minres_shift_0": of("minres", 0.0), "jacobi_shift_0": of("jacobi", 0.0), "minres_shift_0.01": of("minres", 0.01), "jacobi_shift_0.01": of("jacobi", 0.01)}
        out = alternate(forms, repeats)
        out["rows"] = self.N
        for sh, bytes_ in (("0", 216 / 200), ("0.01", 224 / 200)):
            out[f"jacobi_to_minres_shift_{sh}"] = dict(ms_per_body=out[f"jacobi_shift_{sh}"]["ms_per_body"] / out[f"minres_shift_{sh}"]["ms_per_body"], bytes=bytes_)
        return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--parts", nargs="*", default=["vcycle", "jacobi", "body"], choices=["vcycle", "jacobi", "body"])
    ap.add_argument("--n", type=int, default=256, help="n of the n^3 Poisson runs with the V-cycle")
    ap.add_argument("--body-n", type=int, default=512, help="n of the n^3 body-cost runs")
    ap.add_argument("--bodies", type=int, default=200)
    ap.add_argument("--shifts", type=float, nargs="*", default=[0.01, 0.05], help="shifts of the V-cycle runs")
    ap.add_argument("--jacobi-shifts", type=float, nargs="*", default=[0.0, 60.0])
    ap.add_argument("--jacobi-n", type=int, default=None, help="rows of viennacl_main (default: its full size)")
    ap.add_argument("--hierarchies", nargs="*", default=["geometric", "aggregation"], choices=["geometric", "aggregation"])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", choices=["trace"], default=None, help="41 bodies of SolveMinres and of SolveMinresJacobi (shift 0.01) at --body-n, once, for a kernel trace")
    a = ap.parse_args()
    _lib.require_gpu()
    result = {"byte_model_per_row": BYTES}
    if a.only:
        b = Body(a.body_n)
        b.run("minres", 0.01, 40)
        b.run("jacobi", 0.01, 40)
        b.close()
        result["only"] = dict(form=a.only, n=a.body_n, bodies=41)
    else:
        if "vcycle" in a.parts:
            result[f"poisson{a.n}_vcycle"] = vcycle(a.n, a.shifts, a.repeats, a.hierarchies)
        if "jacobi" in a.parts:
            result["viennacl_main_jacobi"] = jacobi(a.jacobi_shifts, a.repeats, a.jacobi_n)
        if "body" in a.parts:
            b = Body(a.body_n)
            result[f"poisson{a.body_n}_body"] = b.cost(a.bodies, a.repeats)
            b.close()
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
