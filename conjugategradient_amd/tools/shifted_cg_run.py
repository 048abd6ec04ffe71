#!/usr/bin/env python3
"""Measurement only: multi-shift CG (SolveShifted) against k separate SolveEx runs on explicitly shifted matrices, on the 7-point Poisson
matrix (default 512^3, generated on the device), in ONE process, the forms alternated round by round.

  * Shifts: k values spread evenly in the exponent over 6e-1 .. 6e-4 (the diagonal is 6), largest first.
  * Both forms run forced solves of equal length: tolerance 0 with the iteration cap, so no column drops out and every solve runs
    cap + 2 loop bodies.  Per iteration = (time at caps[1] - time at caps[0]) / (caps[1] - caps[0]), HIP-event timed, so that a call's
    set-up drops out; median of --rounds rounds after a warm-up round.  The caps stay below the placement draw's threshold.
  * The comparator: for every shift, sigma_j is added to the STORED diagonal of the device matrix -- with the library's own BLAS-1 exports:
    mask = (e + 1) * (1 / 7) is exactly 1.0 on the diagonal (6) and 0.0 off it (-1), and e = e0 + sigma_j * mask -- and SolveEx runs on
    it at its defaults (deferred x update in groups of 8).  Only the solves are timed; the k times are added.
  * Bytes per iteration from the model of DESIGN.md section 15: multi-shift 12 nnz + 44 N + (3 + 4 k) 8 N, a separate solve
    12 nnz + 92 N (bench.py's algorithmic bytes).
  * --odd also times SolveShifted at (n - 1)^3 rows for the largest k: an odd row count, where columns of x are not 16-byte aligned and
    the pass takes one element at a time.

    python -m conjugategradient_amd.tools.shifted_cg_run --out profiles/shifted/shifted_cg_run.json
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m conjugategradient_amd.tools.shifted_cg_run --only shifted8
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m conjugategradient_amd.tools.shifted_cg_run --only plain
(--only: one forced solve of caps[0] iterations, for a kernel trace; tools/trace_kernel_medians.py OUT gives the medians.)"""
from __future__ import annotations

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


def shifts_for(k):
    return [6.0 * 10.0 ** (-1.0 - (3.0 * j / (k - 1) if k > 1 else 0.0)) for j in range(k)]


class Bench:
    def __init__(self, n, kmax):
        L = self.L = _lib.lib()
        self.n, self.N, self.kmax = n, n ** 3, kmax
        N = self.N
        cg = self.cg = ConjugateGradientRankGpu(N, 7, 0, 10, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE)
        cg.InitializePoisson(n, n, n)
        self.nnz = cg.part.elementCount
        self.A = (cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr)
        self.X, self.PS = VectorDouble(kmax * N), VectorDouble(kmax * N)
        L.MgcgFill(cg.vectorB.Ptr, 1.0)
        self.ev0, self.ev1 = L.MgcgEventCreate(), L.MgcgEventCreate()
        self.e0 = self.mask = None

    def timed(self, fn):
        L = self.L
        L.MgcgDeviceSynchronize()
        L.MgcgEventRecord(self.ev0)
        fn()
        L.MgcgEventRecord(self.ev1)
        return float(L.MgcgEventElapsedMs(self.ev0, self.ev1))

    def shifted(self, k, cap):
        cg, L = self.cg, self.L
        sh = (C.c_double * k)(*shifts_for(k))
        it, st = (C.c_int * 8)(), (C.c_int * 8)()
        s = L.SolveShifted(cg.cublas, cg.cusparse, cg.matDescr, *self.A, self.X.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr,
                           self.PS.Ptr, self.nnz, self.N, k, C.cast(sh, C.c_void_p), 0.0, 0, cap, _lib.RULE_NATIVE,
                           C.cast(it, C.c_void_p), None, C.cast(st, C.c_void_p), None, 0)
        L.MgcgClearLastError()
        assert s == _lib.MAXIT_EXCEEDED and all(it[j] == cap + 1 for j in range(k)), (s, list(it)[:k], list(st)[:k])

    def plain(self, cap):
        cg, L = self.cg, self.L
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        it, res = C.c_int(0), C.c_double(0.0)
        s = L.SolveEx(cg.cublas, cg.cusparse, cg.matDescr, *self.A, cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr,
                      self.nnz, self.N, 0.0, 0, cap, _lib.RULE_NATIVE, C.byref(it), C.byref(res), None, 0)
        L.MgcgClearLastError()
        assert s == _lib.MAXIT_EXCEEDED and it.value == cap + 1, (s, it.value)

    def set_shift(self, sigma):
        """The stored diagonal becomes 6 + sigma (exactly: one rounded add), the off-diagonals stay -1."""
        cg, L, nnz = self.cg, self.L, self.nnz
        e = cg.vectorElements.ToRawPtr()
        if self.e0 is None:
            self.e0, self.mask = VectorDouble(nnz), VectorDouble(nnz)
            L.CopyFromDevice_Double(e, self.e0.ToRawPtr(), nnz, 0, 0)
            L.MgcgFill(self.mask.Ptr, 1.0)
            L.Axpy(cg.cublas, self.mask.ToRawPtr(), e, nnz, 1.0)             # 1 + e: 7 on the diagonal, 0 off it
            L.Scal(cg.cublas, self.mask.ToRawPtr(), 1.0 / 7.0, nnz)          # fl(7 * fl(1 / 7)) = 1.0
        L.CopyFromDevice_Double(self.e0.ToRawPtr(), e, nnz, 0, 0)
        if sigma != 0.0:
            L.Axpy(cg.cublas, e, self.mask.ToRawPtr(), nnz, sigma)
        L.MgcgAnalysisClear(cg.cusparse)                                     # (the matrix was rewritten in place)
        L.MgcgDeviceSynchronize()
        _lib.check("set_shift")

    def separate(self, k, cap):
        """k SolveEx runs, one per shifted matrix; returns the sum of the solves' times (ms)."""
        total = 0.0
        for sigma in shifts_for(k):
            self.set_shift(sigma)
            total += self.timed(lambda: self.plain(cap))
        self.set_shift(0.0)
        return total


def model_bytes(nnz, N, k):
    return 12 * nnz + 44 * N + (3 + 4 * k) * 8 * N, k * (12 * nnz + 92 * N)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--ks", default="1,4,8")
    ap.add_argument("--caps", type=int, nargs=2, default=[20, 70])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--odd", action="store_true", help="also SolveShifted at (n - 1)^3 rows with the largest k")
    ap.add_argument("--only", default=None, help="'plain' or 'shiftedK': that solve alone, once, caps[0] iterations (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    ks = [int(v) for v in a.ks.split(",")]
    c0, c1 = a.caps
    if a.only:
        k = 1 if a.only == "plain" else int(a.only[len("shifted"):])
        B = Bench(a.n, k)
        if a.only == "plain":
            B.plain(c0)
        else:
            B.shifted(k, c0)
        print(json.dumps({"only": a.only, "n": a.n, "loop_bodies": c0 + 2}))
        return
    B = Bench(a.n, max(ks))
    samples = {("shifted", k): [] for k in ks}
    samples.update({("separate", k): [] for k in ks})
    for rnd in range(a.rounds + 1):                       # round 0 warms up: code objects, the matrix shape, the ring of the deferred x update
        for k in ks:                                      # the forms alternate, so a drift of the machine meets both alike
            t0, t1 = B.timed(lambda: B.shifted(k, c0)), B.timed(lambda: B.shifted(k, c1))
            u0, u1 = B.separate(k, c0), B.separate(k, c1)
            if rnd:
                samples[("shifted", k)].append((t1 - t0) / (c1 - c0))
                samples[("separate", k)].append((u1 - u0) / (c1 - c0))
    out = dict(n=a.n, rows=B.N, nnz=int(B.nnz), caps=[c0, c1], rounds=a.rounds, per_k={})
    for k in ks:
        ms, sep = statistics.median(samples[("shifted", k)]), statistics.median(samples[("separate", k)])
        bm, bs = model_bytes(B.nnz, B.N, k)
        out["per_k"][str(k)] = dict(shifts=shifts_for(k), shifted_ms_per_iteration=ms, separate_ms_per_iteration=sep, ratio=sep / ms,
                                    byte_ratio=bs / bm, shifted_model_bytes=bm, separate_model_bytes=bs,
                                    shifted_fraction_of_peak=bm / (ms * 1e-3) / PEAK, separate_fraction_of_peak=bs / (sep * 1e-3) / PEAK,
                                    shifted_samples=samples[("shifted", k)], separate_samples=samples[("separate", k)])
    if a.odd:
        k = max(ks)
        del B
        O = Bench(a.n - 1, k)
        s = []
        for rnd in range(a.rounds + 1):
            t0, t1 = O.timed(lambda: O.shifted(k, c0)), O.timed(lambda: O.shifted(k, c1))
            if rnd:
                s.append((t1 - t0) / (c1 - c0))
        out["odd_rows"] = dict(n=a.n - 1, rows=O.N, k=k, shifted_ms_per_iteration=statistics.median(s), samples=s,
                               ns_per_row=statistics.median(s) * 1e6 / O.N, even_ns_per_row=out["per_k"][str(k)]["shifted_ms_per_iteration"] * 1e6 / out["rows"])
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
