#!/usr/bin/env python3
"""BASELINE config 5 (random SPD, 10 M rows, ~31 nonzeros per row, columns without locality) in the three forms the library has for it, in
one process on the same arrays: plain CSR (compression off, no automatic tiles), the column tiles (class 4, mode 1) and the
propagation-blocking form (class 5, mode 3).  Per form: set-up ms (the first product minus a plain one), the product (median of --reps
HIP-event-timed CsrMV, the forms alternated), CG ms per iteration over --steps CgSteps, the algorithmic bytes of a product and their
fraction of 8 TB/s, and whether the products equal the CSR product bit for bit.  Prints one JSON object (--out: also writes it)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from conjugategradient_amd import _lib, problems  # noqa: E402
from conjugategradient_amd.parallel import ConjugateGradientRankGpu  # noqa: E402
from conjugategradient_amd.solver import VectorDouble, VectorInt  # noqa: E402

PEAK = 8.0e12
FORMS = (("csr", _lib.COMPRESSION_OFF), ("class4", _lib.COMPRESSION_BEST), ("class5", _lib.COMPRESSION_PB))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.lib()
    _lib.require_gpu()
    assert L.MgcgSetTuning(b"auto_tiles", 0) == 0                  # plain CSR means plain CSR
    s = problems.random_spd(a.rows, mean_upper=14.0, seed=12345)
    n, nnz = s.Count, s.nnz
    e, c, r = VectorDouble(nnz), VectorInt(nnz), VectorInt(n + 1)
    e.CopyFrom(s.Elements, nnz); c.CopyFrom(s.ColumnIndeces, nnz); r.CopyFrom(s.RowOffsets, n + 1)
    x, y = VectorDouble(n), VectorDouble(n)
    x.CopyFrom(np.cos(np.arange(n) * 0.01), n)
    blas, descr = L.CreateBlas(), L.CreateMatDescr()
    ev0, ev1 = L.MgcgEventCreate(), L.MgcgEventCreate()
    handles = {}
    for name, mode in FORMS:
        handles[name] = L.CreateSparse()
        L.MgcgSetMatrixCompression(handles[name], mode)

    def product(name):
        L.MgcgEventRecord(ev0)
        L.CsrMV(handles[name], descr, y.ToRawPtr(), e.ToRawPtr(), r.ToRawPtr(), c.ToRawPtr(), x.ToRawPtr(), nnz, n, n, 1.0, 0.0)
        L.MgcgEventRecord(ev1)
        ms = L.MgcgEventElapsedMs(ev0, ev1)
        _lib.check("CsrMV")
        return ms

    out = {"rows": n, "nnz": nnz, "algorithmic_bytes": nnz * 12.0 + n * 20.0, "forms": {}}
    ys = {}
    for name, mode in FORMS:
        first = product(name)
        again = product(name)
        info = L.MgcgAnalysisInfo(handles[name], 0, None, None, None, None)
        ys[name] = y.to_numpy(n).copy()
        out["forms"][name] = {"mode": mode, "class": info if info >= 0 else 0, "setup_ms": max(first - again, 0.0)}
    times = {name: [] for name, _ in FORMS}
    for _ in range(a.reps):
        for name, _ in FORMS:
            times[name].append(product(name))
    for name, _ in FORMS:
        f = out["forms"][name]
        f["product_ms"] = float(np.median(times[name]))
        f["product_fraction_of_8TBs"] = out["algorithmic_bytes"] / (f["product_ms"] * 1e-3) / PEAK
        f["equal_to_csr"] = bool(np.array_equal(ys[name], ys["csr"]))
    # CG per iteration: one rank, the solver's own loop (CgSteps), each form on its own solver
    b = s.b.copy()
    for name, mode in FORMS:
        cg = ConjugateGradientRankGpu(n, int(np.diff(s.RowOffsets).max()), 0, 10 * a.steps, 1e-30).load(s)
        _lib.check("load")
        L.MgcgSetMatrixCompression(cg.cusparse, mode)
        cg.b[:] = b
        cg.Initialize()
        cg.Steps(3, restart=True)                                    # analysis, code objects, placement
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        L.MgcgEventRecord(ev0)
        cg.Steps(a.steps, restart=False)
        L.MgcgEventRecord(ev1)
        ms = L.MgcgEventElapsedMs(ev0, ev1)
        L.MgcgDeviceSynchronize()
        wall = (time.perf_counter() - t0) * 1e3
        out["forms"][name]["cg_ms_per_iteration"] = ms / a.steps
        out["forms"][name]["cg_wall_ms_per_iteration"] = wall / a.steps
        out["forms"][name]["cg_class"] = L.MgcgAnalysisInfo(cg.cusparse, 0, None, None, None, None)
        cg.Dispose()
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    for h in handles.values():
        L.DestroySparse(h)
    L.DestroyBlas(blas)
    L.DestroyMatDescr(descr)
    L.MgcgEventDestroy(ev0)
    L.MgcgEventDestroy(ev1)


if __name__ == "__main__":
    main()
