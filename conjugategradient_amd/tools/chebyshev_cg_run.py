"""Measurement only: what the Chebyshev-preconditioned loop (SolveChebyshev) costs next to SolveEx / SolveJacobi, in one process on one
GPU, the forms alternated inside every repeat, median of the repeats.

Per iteration: all loops run with tolerance 0 under an iteration cap, and the time of K1 bodies is subtracted from that of K2 so that
the set-up of a call drops out; a Chebyshev iteration of degree m holds m products, so ms per product stands beside ms per iteration.
The plain loop runs at its default (deferred x update) and with x_defer = 1.  To solution: every form once to a relative 1e-8
(MGCG_RULE_VIENNACL) from x = 0, iterations and seconds; the Poisson systems get an N(0,1) right-hand side.  Bounds: lambdaMax from
MgcgGershgorinBound, lambdaMin = lambdaMax / 30.

  poisson   n^3 7-point Poisson from the device generator (--n 512 and --n 256): plain, Jacobi, Chebyshev m = 2, 4, 8 without the diagonal
  drivers   problems.mgcg_main() and problems.viennacl_main() at full size: the same, per iteration without the diagonal (with it the forced
            loop reaches the underflow range within a few bodies), to solution with it
  slab      the 512 x 512 x 64 slab of one rank of an 8-GPU run on the forced several-ranks path (a one-rank RCCL communicator under
            MGCG_FORCE_MULTIRANK), per iteration only

    python -m conjugategradient_amd.tools.chebyshev_cg_run --out profiles/chebyshev/chebyshev_cg_run.json
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python -m conjugategradient_amd.tools.chebyshev_cg_run --only cheb4 --n 512
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

DEGREES = (2, 4, 8)
BASE_FORMS = (("plain_default", "plain", None), ("plain_x_defer_1", "plain", 1), ("jacobi", "jacobi", None))
CHEB_FORMS = tuple((f"cheb{m}", f"cheb{m}", None) for m in DEGREES)
FORMS = BASE_FORMS + CHEB_FORMS
EIG_RATIO = 30.0


def bytes_per_row(m):
    """7 entries per row: the loop's product 104, the first pass 40, the x / p update 40, a step 104 + 32."""
    return 184 + 136 * (m - 1)


BYTES = {"plain_x_defer_1": 168, "jacobi": 184, **{f"cheb{m}": bytes_per_row(m) for m in DEGREES}}


class Bench:
    """One matrix on the device and the loops' calls on it.  comm: None, or a communicator for the several-ranks exports."""

    def __init__(self, cg, comm=None):
        self.L, self.cg, self.comm = _lib.lib(), cg, comm
        p = cg.part
        self.N, self.nnz = cg.Count, p.elementCount
        self.dinv, self.d = VectorDouble(max(p.count, 1)), VectorDouble(max(p.count, 1))
        self.z, self.z2 = VectorDouble(self.N), VectorDouble(self.N)
        if self.L.MgcgJacobiSetup(cg.cusparse, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, self.nnz, p.count, p.offset, self.dinv.Ptr) != 0:
            _lib.check("MgcgJacobiSetup")
        self.lmax = {}
        for jacobi in (False, True):
            bound = C.c_double(0.0)
            if self.L.MgcgGershgorinBound(cg.cusparse, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, self.nnz, p.count, p.offset,
                                          self.dinv.Ptr if jacobi else None, C.byref(bound)) != 0:
                _lib.check("MgcgGershgorinBound")
            self.lmax[jacobi] = bound.value
        self.it, self.res = C.c_int(0), C.c_double(0.0)

    def close(self):
        for v in (self.dinv, self.d, self.z, self.z2):
            v.Dispose()
        self.cg.Dispose()

    def call(self, loop, tol, cap, rule, jacobi=False):
        """One solve from x = 0: (status, iterations, ms)."""
        L, cg, p = self.L, self.cg, self.cg.part
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        L.MgcgDeviceSynchronize()
        head = (self.comm, cg.cublas, cg.cusparse, cg.matDescr, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr)
        part = (self.N, p.count, p.offset, self.nnz, p.minJ, p.maxJ)
        tail = (tol, 0, cap, rule, C.byref(self.it), C.byref(self.res), None, 0)
        t0 = time.perf_counter()
        if loop == "plain":
            st = L.SolveParallel(*head, *part, *tail)
        elif loop == "jacobi":
            st = L.SolveJacobiParallel(*head, self.dinv.Ptr, *part, *tail)
        else:
            m = int(loop[4:])
            lmax = self.lmax[jacobi]
            st = L.SolveChebyshevParallel(*head, self.dinv.Ptr if jacobi else None, self.z.Ptr, self.z2.Ptr, self.d.Ptr, *part,
                                          m, lmax / EIG_RATIO, lmax, *tail)
        ms = (time.perf_counter() - t0) * 1e3
        L.MgcgClearLastError()
        return st, self.it.value, ms

    def run(self, loop, cap):
        """cap + 1 forced bodies: ms, or None when the loop broke down before the cap (r.z in the underflow range)."""
        st, it, ms = self.call(loop, 0.0, cap, _lib.RULE_NATIVE)
        return ms if st == _lib.MAXIT_EXCEEDED and it == cap + 1 else None

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
                if rep and a is not None and b is not None:
                    samples[name].append((b - a) / (k2 - k1))
        self.L.MgcgReloadEnvironment()
        out = dict(rows=self.N, nnz=int(self.nnz), caps=[k1, k2], lambda_max=self.lmax[False])
        for name, loop, _ in forms:
            if not samples[name]:
                out[name] = dict(ms_per_iteration=None, note="the forced loop broke down before its cap")
                continue
            ms = sorted(samples[name])[len(samples[name]) // 2]
            out[name] = dict(ms_per_iteration=ms, samples=samples[name])
            if loop.startswith("cheb"):
                out[name]["ms_per_product"] = ms / int(loop[4:])
        base = {k: out[k]["ms_per_iteration"] for k in ("plain_x_defer_1", "plain_default", "plain", "jacobi") if k in out}
        for name, loop, _ in forms:
            if loop.startswith("cheb") and out[name]["ms_per_iteration"] is not None:
                for k, v in base.items():
                    out[name][f"per_product_to_{k}"] = out[name]["ms_per_product"] / v
        return out

    def to_solution(self, forms, jacobi, rel=1e-8, cap=20000):
        """Every form once to || r || / || r0 || < rel from x = 0."""
        out = {}
        for name, loop, defer in forms:
            self.select(defer)
            st, it, ms = self.call(loop, rel, cap, _lib.RULE_VIENNACL, jacobi=jacobi)
            out[name] = dict(status=st, iterations=it, loop_bodies=it + 1, seconds=ms / 1e3, residual=self.res.value)
            if loop.startswith("cheb"):
                out[name]["products"] = (it + 1) * int(loop[4:])
        self.L.MgcgReloadEnvironment()
        return out


def poisson_bench(nx, ny, nz, comm=None):
    cg = ConjugateGradientRankGpu(nx * ny * nz, 7, 0, 10, 0.0, rank=0, world=1, comm=comm, rule=_lib.RULE_NATIVE)
    cg.InitializePoisson(nx, ny, nz)
    return Bench(cg, comm)


def system_bench(s):
    cg = ConjugateGradientRankGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 10, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE).load(s)
    cg.Initialize()
    return Bench(cg)


def randn_rhs(b):
    """An N(0,1) right-hand side, uploaded in pieces."""
    rng = np.random.default_rng(20261018)
    piece = 1 << 24
    for lo in range(0, b.N, piece):
        n = min(piece, b.N - lo)
        b.cg.vectorB.CopyFrom(rng.standard_normal(n), n, 0, lo)


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
    os.environ["MGCG_OVERLAP"] = "0"                   # the exchange in line for every loop: the Chebyshev loop has no other schedule
    L.MgcgReloadEnvironment()
    b = poisson_bench(nx, nx, planes, comm)
    out = b.cost(k1, k2, repeats, forms=(("plain", "plain", None), ("jacobi", "jacobi", None)) + CHEB_FORMS)
    out["slab"] = f"{nx} x {nx} x {planes}"
    out["probe_us"] = {name: L.MgcgCommProbe(comm, what, count, 200) for name, what, count in
                       (("allreduce_8B", 0, 1), ("allreduce_16B", 0, 2), ("kernel_boundary", 3, 0))}
    b.close()
    del os.environ["MGCG_FORCE_MULTIRANK"], os.environ["MGCG_OVERLAP"]
    L.MgcgReloadEnvironment()
    L.MgcgCommDestroy(comm)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--n", type=int, nargs="*", default=[512, 256], help="n of the n^3 Poisson runs")
    ap.add_argument("--caps", type=int, nargs=2, default=[10, 60])
    ap.add_argument("--driver-caps", type=int, nargs=2, default=[10, 60])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip", nargs="*", default=[], choices=["poisson", "drivers", "slab", "solution"])
    ap.add_argument("--only", choices=[f[0] for f in FORMS], default=None,
                    help="run only this loop at the first n, once, for caps[0] iterations (for a kernel trace)")
    a = ap.parse_args()
    _lib.require_gpu()
    result = {"byte_model_per_row": BYTES, "eig_ratio": EIG_RATIO}
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
                if "solution" not in a.skip:
                    randn_rhs(b)
                    result[f"poisson{n}"]["to_1e-8"] = b.to_solution(FORMS, jacobi=False)
                b.close()
        if "drivers" not in a.skip:
            for name, make in (("mgcg_main", problems.mgcg_main), ("viennacl_main", problems.viennacl_main)):
                b = system_bench(make())
                result[name] = b.cost(a.driver_caps[0], a.driver_caps[1], a.repeats)
                if "solution" not in a.skip:
                    result[name]["to_1e-8"] = b.to_solution(FORMS, jacobi=True)
                    result[name]["to_1e-8"]["lambda_max_of_dinv_a"] = b.lmax[True]
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
