"""Measurement only: what an iteration of the single-reduction loop (SolveSingleReduce) costs next to SolveEx / SolveJacobi, in one
process on one GPU, the forms alternated inside every repeat, median of the repeats.

Every figure is ms per iteration: all loops run with tolerance 0 under an iteration cap, and the time of K1 bodies is subtracted from
that of K2 so that the set-up of a call drops out.  The plain loop runs at its default (deferred x update) and with x_defer = 1.

  poisson   n^3 7-point Poisson from the device generator (--n 512 and --n 256): plain, Jacobi, single-reduction with and without dinv
  drivers   problems.mgcg_main() and problems.viennacl_main() at full size, the same five forms
  slab      the 512 x 512 x 64 slab of one rank of an 8-GPU run on the forced several-ranks path (a one-rank RCCL communicator under
            MGCG_FORCE_MULTIRANK): SolveParallel / SolveJacobiParallel against SolveSingleReduceParallel, with MgcgCommProbe's price of an
            all-reduce (what = 0) and of a kernel boundary (what = 3) beside them

    python -m conjugategradient_amd.tools.sreduce_cg_run --out profiles/sreduce/sreduce_cg_run.json
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python -m conjugategradient_amd.tools.sreduce_cg_run --only sreduce --n 512
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import time

import numpy as np

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.parallel import ConjugateGradientRankGpu
from conjugategradient_amd.solver import VectorDouble

FORMS = (("plain_default", "plain", None), ("plain_x_defer_1", "plain", 1), ("jacobi", "jacobi", None),
         ("sreduce", "sreduce", None), ("sreduce_jacobi", "sreduce_jacobi", None))
# bytes per row and iteration at 7 entries per row: the product ~104, the passes 64 (plain, x every iteration), 80 (Jacobi), 72 and 88
BYTES = {"plain_x_defer_1": 168, "jacobi": 184, "sreduce": 176, "sreduce_jacobi": 192}


class Bench:
    """One matrix on the device and the loops' calls on it.  comm: None, or a communicator for the several-ranks exports."""

    def __init__(self, cg, comm=None):
        self.L, self.cg, self.comm = _lib.lib(), cg, comm
        p = cg.part
        self.N, self.nnz = cg.Count, p.elementCount
        self.dinv, self.s = VectorDouble(max(p.count, 1)), VectorDouble(max(p.count, 1))
        if self.L.MgcgJacobiSetup(cg.cusparse, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, self.nnz, p.count, p.offset, self.dinv.Ptr) != 0:
            _lib.check("MgcgJacobiSetup")
        self.it, self.res = C.c_int(0), C.c_double(0.0)

    def close(self):
        self.dinv.Dispose()
        self.s.Dispose()
        self.cg.Dispose()

    def run(self, loop, cap):
        L, cg, p = self.L, self.cg, self.cg.part
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        L.MgcgDeviceSynchronize()
        head = (self.comm, cg.cublas, cg.cusparse, cg.matDescr, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr)
        tail = (self.N, p.count, p.offset, self.nnz, p.minJ, p.maxJ, 0.0, 0, cap, _lib.RULE_NATIVE, C.byref(self.it), C.byref(self.res), None, 0)
        t0 = time.perf_counter()
        if loop == "plain":
            st = L.SolveParallel(*head, *tail)
        elif loop == "jacobi":
            st = L.SolveJacobiParallel(*head, self.dinv.Ptr, *tail)
        else:
            st = L.SolveSingleReduceParallel(*head, self.s.Ptr, self.dinv.Ptr if loop == "sreduce_jacobi" else None, *tail)
        ms = (time.perf_counter() - t0) * 1e3
        L.MgcgClearLastError()
        assert st == _lib.MAXIT_EXCEEDED and self.it.value == cap + 1, (loop, st, self.it.value)
        return ms

    def select(self, defer):
        self.L.MgcgReloadEnvironment()                 # back to the defaults (and to the caller's environment: MGCG_FORCE_MULTIRANK)
        if defer is not None:
            assert self.L.MgcgSetTuning(b"x_defer", defer) == 0

    def cost(self, k1, k2, repeats, forms=FORMS):
        samples = {name: [] for name, _, _ in forms}
        for rep in range(repeats + 1):                 # round 0 warms up: code objects, matrix shape, the workspace's vectors
            for name, loop, defer in forms:            # the forms alternate, so a drift of the machine meets all alike
                self.select(defer)
                a, b = self.run(loop, k1), self.run(loop, k2)
                if rep:
                    samples[name].append((b - a) / (k2 - k1))
        self.L.MgcgReloadEnvironment()
        out = dict(rows=self.N, nnz=int(self.nnz), caps=[k1, k2])
        for name, _, _ in forms:
            out[name] = dict(ms_per_iteration=sorted(samples[name])[len(samples[name]) // 2], samples=samples[name])
        ms = {name: out[name]["ms_per_iteration"] for name, _, _ in forms}
        if "plain_x_defer_1" in ms:
            out["sreduce_to_plain_x_defer_1"] = ms["sreduce"] / ms["plain_x_defer_1"]
            out["sreduce_to_plain_default"] = ms["sreduce"] / ms["plain_default"]
        else:
            out["sreduce_to_plain"] = ms["sreduce"] / ms["plain"]
        out["sreduce_jacobi_to_jacobi"] = ms["sreduce_jacobi"] / ms["jacobi"]
        return out


def poisson_bench(nx, ny, nz, comm=None):
    cg = ConjugateGradientRankGpu(nx * ny * nz, 7, 0, 10, 0.0, rank=0, world=1, comm=comm, rule=_lib.RULE_NATIVE)
    cg.InitializePoisson(nx, ny, nz)
    return Bench(cg, comm)


def system_bench(s):
    cg = ConjugateGradientRankGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 10, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE).load(s)
    cg.Initialize()
    return Bench(cg)


def slab(nx, planes, k1, k2, repeats):
    """The several-ranks path on one GPU: every launch and collective call of the path on the device's own stream, without the wire time."""
    L = _lib.lib()
    L.SetDevice(0)
    buf = (C.c_char * 128)()
    if L.MgcgCommGetUniqueId(buf) != 0:
        return dict(skipped="no RCCL: " + _lib.last_error())
    comm = L.MgcgCommInitRank(buf, 1, 0)
    _lib.check("MgcgCommInitRank")
    os.environ["MGCG_FORCE_MULTIRANK"] = "1"
    os.environ["MGCG_OVERLAP"] = "0"                   # the exchange in line for both loops: the single-reduction loop has no other schedule
    L.MgcgReloadEnvironment()
    b = poisson_bench(nx, nx, planes, comm)
    out = b.cost(k1, k2, repeats, forms=(("plain", "plain", None), ("jacobi", "jacobi", None), ("sreduce", "sreduce", None), ("sreduce_jacobi", "sreduce_jacobi", None)))
    out["slab"] = f"{nx} x {nx} x {planes}"
    out["probe_us"] = {name: L.MgcgCommProbe(comm, what, count, 200) for name, what, count in
                       (("allreduce_8B", 0, 1), ("allreduce_16B", 0, 2), ("allreduce_24B", 0, 3), ("kernel_boundary", 3, 0))}
    ms = {k: out[k]["ms_per_iteration"] for k in ("plain", "sreduce")}
    out["saved_us_per_iteration"] = 1e3 * (ms["plain"] - ms["sreduce"])
    b.close()
    del os.environ["MGCG_FORCE_MULTIRANK"], os.environ["MGCG_OVERLAP"]
    L.MgcgReloadEnvironment()
    L.MgcgCommDestroy(comm)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--n", type=int, nargs="*", default=[512, 256], help="n of the n^3 Poisson runs")
    ap.add_argument("--caps", type=int, nargs=2, default=[20, 120])
    ap.add_argument("--driver-caps", type=int, nargs=2, default=[10, 60], help="few bodies: the Jacobi forms converge to the underflow range within a few hundred")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip", nargs="*", default=[], choices=["poisson", "drivers", "slab"])
    ap.add_argument("--only", choices=[f[0] for f in FORMS], default=None,
                    help="run only this loop at the first n, once, for caps[0] iterations (for a kernel trace)")
    a = ap.parse_args()
    _lib.require_gpu()
    result = {"byte_model_per_row": BYTES}
    if a.only:
        _, loop, defer = next(f for f in FORMS if f[0] == a.only)
        b = poisson_bench(a.n[0], a.n[0], a.n[0])
        b.select(defer)
        b.run(loop, a.caps[0])
        b.L.MgcgReloadEnvironment()
        b.close()
        result["only"] = dict(form=a.only, n=a.n[0], loop_bodies=a.caps[0] + 1)
    else:
        if "poisson" not in a.skip:
            for n in a.n:
                b = poisson_bench(n, n, n)
                result[f"poisson{n}"] = b.cost(a.caps[0], a.caps[1], a.repeats)
                b.close()
        if "drivers" not in a.skip:
            for name, make in (("mgcg_main", problems.mgcg_main), ("viennacl_main", problems.viennacl_main)):
                b = system_bench(make())
                result[name] = b.cost(a.driver_caps[0], a.driver_caps[1], a.repeats)
                b.close()
        if "slab" not in a.skip:
            result["slab"] = slab(512, 64, a.caps[0], a.caps[1], a.repeats)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
