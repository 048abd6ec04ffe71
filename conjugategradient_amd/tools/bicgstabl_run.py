"""Measurement only: what BiCGStab(l) (SolveBicgstabL) costs beside SolveBicgstab, on one GPU, plain form, l = 1, 2 and 4.  Every run starts
from x = 0 with an N(0,1) right-hand side and stops at || r || < 1e-8 || b || (MGCG_RULE_NATIVE).  No figure here is an acceptance threshold.

  convdiff256_mild     256^3 convection_diffusion with c = (.5, .25, 0)
  convdiff256_5        the same with c = (5, 5, 5)
  convdiff256_20       the same with c = (20, 20, 20)
  poisson512           512^3 7-point Poisson from the device generator
  trace                20 bodies of SolveBicgstab and of SolveBicgstabL with each l at 256^3, c = (.5, .25, 0), once, for a kernel trace

Per leg SolveBicgstab and SolveBicgstabL with each l run in ONE process, alternated inside every repeat, median of the repeats: bodies,
products (2 per body of BiCGStab, 2 l per body of BiCGStab(l); a last body that the stop test ended in front of a step counts in full), ms
per body, ms per product, seconds to solution, TrueResidual / Residual.  Without --leg every leg runs as a child process of its own under
a time limit of its own, and the script ends at the first one that fails.

Byte model per row at 7 entries per row, stated, not measured: the product ~104; the passes of a BiCGStab body 120, of a BiCGStab(l) body
160 / 304 / 736 for l = 1 / 2 / 4 (kernels_bicgstabl.hip): per product 164 for BiCGStab against 184 / 180 / 196 -- 1.12 x, 1.10 x, 1.20 x.

    python -m conjugategradient_amd.tools.bicgstabl_run --out profiles/bicgstabl
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m conjugategradient_amd.tools.bicgstabl_run --leg trace
    python conjugategradient_amd/tools/trace_kernel_medians.py OUT          (the rate at which each pass streams: vectors x 8 bytes x rows / median)
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

ELLS = (1, 2, 4)
PRODUCT = 104
PASSES = {"bicgstab": 120, 1: 160, 2: 304, 4: 736}
BYTES_PER_PRODUCT = {"bicgstab": PRODUCT + PASSES["bicgstab"] / 2, **{ell: PRODUCT + PASSES[ell] / (2 * ell) for ell in ELLS}}
MAX_PRODUCTS = 6000
LEGS = {"convdiff256_mild": 600, "convdiff256_5": 600, "convdiff256_20": 900, "poisson512": 900}      # the leg's time limit in seconds
CONVECTION = {"convdiff256_mild": (0.5, 0.25, 0.0), "convdiff256_5": (5.0, 5.0, 5.0), "convdiff256_20": (20.0, 20.0, 20.0)}


def median(v):
    return sorted(v)[len(v) // 2]


class Bench:
    """One matrix on the device with an N(0,1) right-hand side, and the loops' C calls on it."""

    def __init__(self, leg):
        from conjugategradient_amd import _lib, problems
        from conjugategradient_amd.parallel import ConjugateGradientRankGpu
        from conjugategradient_amd.solver import VectorDouble

        self._lib = _lib
        self.L = _lib.lib()
        if leg == "poisson512":
            self.N = 512 ** 3
            cg = ConjugateGradientRankGpu(self.N, 7, 0, MAX_PRODUCTS, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE)
            cg.InitializePoisson(512, 512, 512)
        else:
            s = problems.convection_diffusion(256, 256, 256, CONVECTION[leg])
            self.N = s.Count
            cg = ConjugateGradientRankGpu(self.N, 7, 0, MAX_PRODUCTS, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE).load(s)
            cg.Initialize()
            del s
        b = np.random.default_rng(7).standard_normal(self.N)
        cg.vectorB.CopyFrom(b, self.N)
        self.normb = float(np.linalg.norm(b))
        del b
        self.cg = cg
        self.four = [VectorDouble(self.N) for _ in range(4)]                  # v, s, t, rhat
        self.work = VectorDouble(2 * max(ELLS) * (self.N + (self.N & 1)))
        self.it, self.res, self.true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)

    def close(self):
        for v in self.four + [self.work]:
            v.Dispose()
        self.cg.Dispose()

    def run(self, ell, tol=None, cap=None):
        """One solve from x = 0; ell None: SolveBicgstab.  Returns (status, bodies, ms of the call, Residual, TrueResidual)."""
        L, cg, p, _lib = self.L, self.cg, self.cg.part, self._lib
        per_body = 2 if ell is None else 2 * ell
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        L.MgcgDeviceSynchronize()
        head = (cg.cublas, cg.cusparse, cg.matDescr, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr)
        stop = (1e-8 * self.normb if tol is None else tol, 0, MAX_PRODUCTS // per_body if cap is None else cap, _lib.RULE_NATIVE, C.byref(self.it), C.byref(self.res), C.byref(self.true), None, 0)
        t0 = time.perf_counter()
        if ell is None:
            st = L.SolveBicgstab(*head, *(v.Ptr for v in self.four), p.elementCount, self.N, *stop)
        else:
            st = L.SolveBicgstabL(*head, self.work.Ptr, ell, p.elementCount, self.N, *stop)
        ms = (time.perf_counter() - t0) * 1e3
        L.MgcgClearLastError()
        return st, self.it.value, ms, self.res.value, self.true.value

    def compare(self, repeats):
        forms = [("bicgstab", None)] + [(f"bicgstabl_{ell}", ell) for ell in ELLS]
        samples = {name: [] for name, _ in forms}
        out = dict(rows=self.N, relative_tolerance=1e-8, stop_level=1e-8 * self.normb, product_cap=MAX_PRODUCTS)
        for rep in range(repeats + 1):                 # round 0 warms up: code objects, matrix shape, the workspace's vectors
            for name, ell in forms:                    # the forms alternate, so a drift of the machine meets all alike
                st, bodies, ms, res, true = self.run(ell)
                if rep:
                    samples[name].append(ms)
                per_body = 2 if ell is None else 2 * ell
                out[name] = dict(status=st, bodies=bodies, products=bodies * per_body, residual=res, true_residual=true,
                                 true_to_residual=true / res if res else None, bytes_per_product=BYTES_PER_PRODUCT["bicgstab" if ell is None else ell])
        for name, _ in forms:
            med = median(samples[name])
            o = out[name]
            o.update(seconds_to_solution=med / 1e3, ms_per_body=med / max(o["bodies"], 1), ms_per_product=med / max(o["products"], 1), samples_ms=samples[name])
        base = out["bicgstab"]
        for name, _ in forms[1:]:
            o = out[name]
            o["to_bicgstab"] = dict(products=o["products"] / max(base["products"], 1), ms_per_product=o["ms_per_product"] / base["ms_per_product"],
                                    seconds_to_solution=o["seconds_to_solution"] / base["seconds_to_solution"],
                                    bytes_per_product=o["bytes_per_product"] / base["bytes_per_product"])
        return out


def run_leg(leg, repeats):
    from conjugategradient_amd import _lib

    _lib.require_gpu()
    if leg == "trace":
        b = Bench("convdiff256_mild")
        for ell in (None,) + ELLS:
            b.run(ell, tol=0.0, cap=19)
        b.close()
        return dict(rows=b.N, bodies=20)
    b = Bench(leg)
    out = b.compare(repeats)
    b.close()
    return out


STATUS = {0: "OK", 1: "cap", 3: "NONFINITE"}


def readme(result):
    """The measured table as markdown; a figure where the new loop is slower than SolveBicgstab in the same process is set in bold."""
    lines = ["# BiCGStab(l) beside BiCGStab, one MI355X, plain form", "",
             "Written by `python -m conjugategradient_amd.tools.bicgstabl_run --out profiles/bicgstabl`; the numbers are in `bicgstabl_run.json`.",
             "N(0,1) right-hand side, x = 0, stop at a relative 1e-8 (MGCG_RULE_NATIVE), at most %d products; median of the repeats, the loops" % MAX_PRODUCTS,
             "alternated inside one process.  Status: what the call returned (cap: the product cap; NONFINITE: a breakdown).  **Bold**: slower than",
             "`SolveBicgstab` in the same run -- per product, or to solution (only where both ended OK).  'model': the byte table's ratio per product.",
             "What the tables say, and the kernel trace: `READING.md`, written by hand -- this tool never touches it.", ""]
    for leg in LEGS:
        if leg not in result:
            continue
        r = result[leg]
        base = r["bicgstab"]
        lines += [f"## {leg} ({r['rows']} rows)", "",
                  "| loop | status | bodies | products | ms / body | ms / product | x BiCGStab per product (model) | s to solution | TrueResidual / Residual |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for name in ["bicgstab"] + [f"bicgstabl_{ell}" for ell in ELLS]:
            o = r[name]
            ratio, secs = "", f"{o['seconds_to_solution']:.3f}"
            if name != "bicgstab":
                t = o["to_bicgstab"]
                ratio = f"{t['ms_per_product']:.2f} ({t['bytes_per_product']:.2f})"
                if t["ms_per_product"] > 1.0:
                    ratio = f"**{ratio}**"
                if o["status"] == 0 and base["status"] == 0 and t["seconds_to_solution"] > 1.0:
                    secs = f"**{secs}**"
            lines.append(f"| {name} | {STATUS.get(o['status'], o['status'])} | {o['bodies']} | {o['products']} | {o['ms_per_body']:.3f} | {o['ms_per_product']:.3f} | "
                         f"{ratio} | {secs} | {o['true_to_residual']:.3g} |")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="a directory: bicgstabl_run.json and README.md are written there")
    ap.add_argument("--leg", choices=list(LEGS) + ["trace"], default=None, help="run this leg in this process")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), help="the legs to run, each as a child process under its own time limit")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        result = {a.leg: run_leg(a.leg, a.repeats)}
    else:
        result = {"byte_model_per_row": {"product": PRODUCT, "passes_per_body": {str(k): v for k, v in PASSES.items()},
                                         "per_product": {str(k): v for k, v in BYTES_PER_PRODUCT.items()}}}
        for leg in a.legs:
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.bicgstabl_run", "--leg", leg, "--repeats", str(a.repeats)],
                                   stdout=subprocess.PIPE, timeout=LEGS[leg], check=True)      # a leg that fails or hangs ends the script
            result.update(json.loads(child.stdout))
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "bicgstabl_run.json"), "w") as f:
            f.write(text + "\n")
        with open(os.path.join(a.out, "README.md"), "w") as f:
            f.write(readme(result) + "\n")


if __name__ == "__main__":
    main()
