#!/usr/bin/env python3
"""Shared-subspace block CG (SolveBlockKrylov) against SolveBlockEx on the 7-point Poisson matrix (default 512^3, generated on the
device), k seeded N(0,1) right-hand sides, x0 = 0, RULE_VIENNACL at --tol, in ONE process, the two forms alternated:
  * per-iteration time of both for k in --ks: (a forced 50-iteration solve - a forced 10-iteration solve) / 40, HIP-event timed;
    forced = tolerance 0 with min = max (rule NATIVE), median of --rounds rounds;
  * iterations to the stop and seconds to solution of both (--solve-rounds full solves each, alternated; median);
  * the model bytes of an iteration (SolveBlockEx 12 nnz + 4 N + 80 k N, SolveBlockKrylov 12 nnz + 4 N + 96 k N) and their fraction of 8 TB/s.
The comparator is always SolveBlockEx in the same process.  Prints one JSON object (--out: also writes it)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from conjugategradient_amd import _lib  # noqa: E402
from conjugategradient_amd.parallel import ConjugateGradientRankGpu  # noqa: E402
from conjugategradient_amd.solver import VectorDouble  # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--ks", default="4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--solve-rounds", type=int, default=1)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--max-it", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only-krylov", type=int, default=0, help="run only SolveBlockKrylov with this k, 10 forced iterations, once (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    _lib.require_gpu()
    n = a.n
    N = n**3
    ks = [int(v) for v in a.ks.split(",")] if not a.only_krylov else [a.only_krylov]
    kmax = max(ks)
    cg = ConjugateGradientRankGpu(N, 7, 0, 10, 1e-8, rank=0, world=1, rule=_lib.RULE_NATIVE)
    cg.InitializePoisson(n, n, n)
    nnz = cg.part.elementCount
    A = (cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr)
    X, B, AP, P, R = (VectorDouble(kmax * N) for _ in range(5))
    rng = np.random.default_rng(a.seed)
    for j in range(kmax):
        B.CopyFrom(rng.standard_normal(N), N, 0, j * N)
    ev0, ev1 = L.MgcgEventCreate(), L.MgcgEventCreate()
    it8 = (C.c_int * 8)()
    res = (C.c_double * 8)()
    st = (C.c_int * 8)()

    def timed(fn):
        L.MgcgEventRecord(ev0)
        out = fn()
        L.MgcgEventRecord(ev1)
        return float(L.MgcgEventElapsedMs(ev0, ev1)), out

    def block_ex(k, tol, min_it, max_it, rule):
        L.MgcgFill(X.Ptr, 0.0)
        s = L.SolveBlockEx(cg.cublas, cg.cusparse, cg.matDescr, *A, X.Ptr, B.Ptr, AP.Ptr, P.Ptr, R.Ptr, nnz, N, k,
                           tol, min_it, max_it, rule, it8, res, st, None, 0)
        L.MgcgClearLastError()
        return s, [it8[j] for j in range(k)], [res[j] for j in range(k)]

    def krylov(k, tol, min_it, max_it, rule):
        L.MgcgFill(X.Ptr, 0.0)
        it = C.c_int(0)
        s = L.SolveBlockKrylov(cg.cublas, cg.cusparse, cg.matDescr, *A, X.Ptr, B.Ptr, AP.Ptr, P.Ptr, R.Ptr, nnz, N, k,
                               tol, min_it, max_it, rule, C.byref(it), res, st, None, 0)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        assert s != _lib.NONFINITE and s != _lib.ERROR, msg
        return s, [it.value] * k, [res[j] for j in range(k)]

    def forced(fn, k, iters):
        s, its, _ = fn(k, 0.0, iters - 2, iters - 2, _lib.RULE_NATIVE)
        assert s == _lib.MAXIT_EXCEEDED and all(v == iters - 1 for v in its), (s, its)

    if a.only_krylov:
        forced(krylov, a.only_krylov, 10)
        print(json.dumps({"only_krylov": a.only_krylov, "iterations": 10}))
        return

    forms = {"block_ex": block_ex, "krylov": krylov}
    for k in ks:                                                   # warm-up
        for fn in forms.values():
            forced(fn, k, 10)
    per_it = {(f, k): [] for f in forms for k in ks}
    for _ in range(a.rounds):
        for k in ks:
            for f, fn in forms.items():
                t10, _ = timed(lambda: forced(fn, k, 10))
                t50, _ = timed(lambda: forced(fn, k, 50))
                per_it[(f, k)].append((t50 - t10) / 40.0)
    solves = {(f, k): [] for f in forms for k in ks}
    for _ in range(a.solve_rounds):
        for k in ks:
            for f, fn in forms.items():
                ms, (s, its, rs) = timed(lambda: fn(k, a.tol, 0, a.max_it, _lib.RULE_VIENNACL))
                assert s == _lib.OK, (f, k, s)
                solves[(f, k)].append({"seconds": ms * 1e-3, "iterations": its, "residual": rs})

    out = {"n": n, "rows": N, "nnz": nnz, "rounds": a.rounds, "solve_rounds": a.solve_rounds, "tol": a.tol, "seed": a.seed, "peak_Bps": PEAK, "k": {}}
    for k in ks:
        entry = {}
        for f in forms:
            ms = statistics.median(per_it[(f, k)])
            byt = 12 * nnz + 4 * N + (80 if f == "block_ex" else 96) * k * N
            runs = solves[(f, k)]
            entry[f] = {"ms_per_iteration": ms, "samples": per_it[(f, k)], "model_bytes": byt, "frac_of_peak": byt / (ms * 1e-3) / PEAK,
                        "iterations_to_stop": max(runs[0]["iterations"]), "iterations_per_column": runs[0]["iterations"],
                        "seconds_to_solution": statistics.median(r["seconds"] for r in runs), "residual": runs[0]["residual"]}
        entry["ratio_ms_per_iteration"] = entry["krylov"]["ms_per_iteration"] / entry["block_ex"]["ms_per_iteration"]
        entry["model_ratio"] = entry["krylov"]["model_bytes"] / entry["block_ex"]["model_bytes"]
        entry["ratio_iterations"] = entry["krylov"]["iterations_to_stop"] / entry["block_ex"]["iterations_to_stop"]
        entry["speedup_to_solution"] = entry["block_ex"]["seconds_to_solution"] / entry["krylov"]["seconds_to_solution"]
        out["k"][str(k)] = entry
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    L.MgcgEventDestroy(ev0)
    L.MgcgEventDestroy(ev1)


if __name__ == "__main__":
    main()
