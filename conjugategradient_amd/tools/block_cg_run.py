#!/usr/bin/env python3
"""Block CG against single right-hand-side solves on the 7-point Poisson matrix (default 512^3, generated on the device), in ONE
process, the forms alternated round by round:
  * per-iteration time of SolveEx (one right-hand side) and of SolveBlockEx for k in --ks: (a forced 50-iteration solve - a forced
    10-iteration solve) / 40, HIP-event timed; forced = tolerance 0 with min = max (rule NATIVE), median of --rounds rounds;
  * CsrMVBlock for every k against k x CsrMV (median of --reps products each);
  * the algorithmic bytes of each (block iteration 12 nnz + 4 N + 80 k N, block product 12 nnz + 4 (N + 1) + 16 k N), their fraction
    of 8 TB/s, the milliseconds per right-hand side per iteration and their ratio to the single solve.
Prints one JSON object (--out: also writes it)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from conjugategradient_amd import _lib  # noqa: E402
from conjugategradient_amd.parallel import ConjugateGradientRankGpu  # noqa: E402
from conjugategradient_amd.solver import VectorDouble  # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--ks", default="1,2,4,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only-block", type=int, default=0, help="run only SolveBlockEx with this k, once (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    _lib.require_gpu()
    n = a.n
    N = n**3
    ks = [int(v) for v in a.ks.split(",")] if not a.only_block else [a.only_block]
    kmax = max(ks)
    cg = ConjugateGradientRankGpu(N, 7, 0, 10, 1e-8, rank=0, world=1, rule=_lib.RULE_NATIVE)
    cg.InitializePoisson(n, n, n)
    nnz = cg.part.elementCount
    A = (cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr)
    X, B, AP, P, R = (VectorDouble(kmax * N) for _ in range(5))
    L.MgcgFill(B.Ptr, 1.0)
    ev0, ev1 = L.MgcgEventCreate(), L.MgcgEventCreate()
    it = (C.c_int * 8)()
    res = (C.c_double * 8)()
    st = (C.c_int * 8)()

    def timed(fn):
        L.MgcgEventRecord(ev0)
        fn()
        L.MgcgEventRecord(ev1)
        return float(L.MgcgEventElapsedMs(ev0, ev1))

    def single(iters):
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        i1, r1 = C.c_int(0), C.c_double(0)
        s = L.SolveEx(cg.cublas, cg.cusparse, cg.matDescr, *A, cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr,
                      cg.vectorR.Ptr, nnz, N, 0.0, iters - 2, iters - 2, _lib.RULE_NATIVE, C.byref(i1), C.byref(r1), None, 0)
        L.MgcgClearLastError()
        assert s == _lib.MAXIT_EXCEEDED and i1.value == iters - 1, (s, i1.value)

    def blockk(k, iters):
        L.MgcgFill(X.Ptr, 0.0)
        s = L.SolveBlockEx(cg.cublas, cg.cusparse, cg.matDescr, *A, X.Ptr, B.Ptr, AP.Ptr, P.Ptr, R.Ptr, nnz, N, k,
                           0.0, iters - 2, iters - 2, _lib.RULE_NATIVE, it, res, st, None, 0)
        L.MgcgClearLastError()
        assert s == _lib.MAXIT_EXCEEDED and all(it[j] == iters - 1 for j in range(k)), (s, list(it)[:k])

    if a.only_block:
        blockk(a.only_block, 10)
        print(json.dumps({"only_block": a.only_block, "iterations": 10}))
        return

    L.MgcgFill(cg.vectorB.Ptr, 1.0)
    single(10)                                                   # warm-up (the first solve runs the placement draw)
    for k in ks:
        blockk(k, 10)
    forms = ["single"] + [f"block{k}" for k in ks]
    per_it = {f: [] for f in forms}
    for _ in range(a.rounds):
        for f in forms:
            run = single if f == "single" else (lambda iters, k=int(f[5:]): blockk(k, iters))
            t10 = timed(lambda: run(10))
            t50 = timed(lambda: run(50))
            per_it[f].append((t50 - t10) / 40.0)

    # products: CsrMVBlock(k) against k x CsrMV (raw device pointers, not Vector handles)
    Araw = (cg.vectorElements.ToRawPtr(), cg.vectorRowOffsets.ToRawPtr(), cg.vectorColumnIndeces.ToRawPtr())
    y, x = AP.ToRawPtr(), P.ToRawPtr()

    def csrmv():
        L.CsrMV(cg.cusparse, cg.matDescr, y, *Araw, x, nnz, N, N, 1.0, 0.0)

    def csrmv_block(k):
        L.CsrMVBlock(cg.cusparse, cg.matDescr, y, *Araw, x, nnz, N, k)

    L.MgcgFill(P.Ptr, 1.0)
    spmv = {"csrmv": []}
    spmv.update({f"block{k}": [] for k in ks})
    csrmv()
    for k in ks:
        csrmv_block(k)
    _lib.check("products (warm-up)")
    for _ in range(a.reps):
        spmv["csrmv"].append(timed(csrmv))
        for k in ks:
            spmv[f"block{k}"].append(timed(lambda k=k: csrmv_block(k)))
    _lib.check("products")

    single_ms = statistics.median(per_it["single"])
    out = {"n": n, "rows": N, "nnz": nnz, "rounds": a.rounds, "reps": a.reps, "peak_Bps": PEAK,
           "single": {"ms_per_iteration": single_ms, "bytes": 12 * nnz + 4 * N + 80 * N,
                      "frac_of_peak": (12 * nnz + 4 * N + 80 * N) / (single_ms * 1e-3) / PEAK, "samples": per_it["single"]},
           "block": {}, "spmv": {}}
    csr_ms = statistics.median(spmv["csrmv"])
    out["spmv"]["csrmv"] = {"ms": csr_ms, "bytes": 12 * nnz + 4 * (N + 1) + 16 * N,
                            "frac_of_peak": (12 * nnz + 4 * (N + 1) + 16 * N) / (csr_ms * 1e-3) / PEAK}
    for k in ks:
        ms = statistics.median(per_it[f"block{k}"])
        byt = 12 * nnz + 4 * N + 80 * k * N
        out["block"][str(k)] = {"ms_per_iteration": ms, "ms_per_rhs_iteration": ms / k, "ratio_to_single": ms / k / single_ms,
                                "bytes": byt, "frac_of_peak": byt / (ms * 1e-3) / PEAK, "samples": per_it[f"block{k}"]}
        pm = statistics.median(spmv[f"block{k}"])
        pb = 12 * nnz + 4 * (N + 1) + 16 * k * N
        out["spmv"][f"block{k}"] = {"ms": pm, "k_x_csrmv_ms": k * csr_ms, "ratio_to_k_csrmv": pm / (k * csr_ms), "bytes": pb,
                                    "frac_of_peak": pb / (pm * 1e-3) / PEAK}
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
