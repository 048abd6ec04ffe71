"""Measurement only: what restarted GMRES(m) (SolveGmres) costs beside SolveBicgstab and SolveBicgstabL (l = 2), on one GPU, plain form,
m = 10, 20, 30 and orth = 1, 2.  Every run starts from x = 0 with an N(0,1) right-hand side and stops at || r || < 1e-8 || b ||
(MGCG_RULE_NATIVE).  No figure here is an acceptance threshold: GMRES moves more bytes per product than both and is expected to be slower.

  convdiff256_mild     256^3 convection_diffusion with c = (.5, .25, 0)
  convdiff256_5        the same with c = (5, 5, 5)
  convdiff256_20       the same with c = (20, 20, 20)
  poisson512           512^3 7-point Poisson from the device generator
  trace                2 cycles of SolveGmres with m = 20, orth = 2 (and 20 bodies of SolveBicgstab for its pass X) at 256^3, c = (.5, .25, 0),
                       once, for a kernel trace

Per leg all loops run in ONE process, alternated inside every repeat, median of the repeats: status, steps (GMRES: Arnoldi steps = products;
the others: products), ms per step, seconds to solution, TrueResidual / Residual.  Round 0 warms up with two cycles per loop.  Without --leg
every leg runs as a child process of its own under a time limit of its own, and the script ends at the first one that fails, aborts or runs
into its limit.

Byte model per row at 7 entries per row, stated, not measured (kernels_gmres.hip): the product ~104; an orthogonalisation pass at step j
moves 2 c + 3 q vectors (c = j + 1 columns in q = ceil(c / 8) launches), pass N 2, the close cols + 2 ceil(cols / 8) per cycle and the restart
a product and 3 vectors per cycle; averaged over a cycle.  BiCGStab: 164 per product, BiCGStab(2): 180.

    python -m conjugategradient_amd.tools.gmres_run --out profiles/gmres
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python -m conjugategradient_amd.tools.gmres_run --leg trace
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

MS = (10, 20, 30)
ORTHS = (1, 2)
PRODUCT = 104
OTHERS = {"bicgstab": 164.0, "bicgstabl_2": 180.0}
MAX_PRODUCTS = 6000
LEGS = {"convdiff256_mild": 600, "convdiff256_5": 600, "convdiff256_20": 900, "poisson512": 900}      # the leg's time limit in seconds
CONVECTION = {"convdiff256_mild": (0.5, 0.25, 0.0), "convdiff256_5": (5.0, 5.0, 5.0), "convdiff256_20": (20.0, 20.0, 20.0)}


def bytes_per_step(m, orth):
    """The byte table of kernels_gmres.hip averaged over a cycle of m steps, without the product."""
    vectors = 0
    for j in range(m):
        c = j + 1
        q = (c + 7) // 8
        vectors += orth * (2 * c + 3 * q) + 2
    vectors += m + 2 * ((m + 7) // 8)                      # the close
    vectors += 3                                           # the restart's r.r and v_0 behind its product
    return 8.0 * vectors / m + PRODUCT / m


def median(v):
    return sorted(v)[len(v) // 2]


class Bench:
    """One matrix on the device with an N(0,1) right-hand side, and the loops' C calls on it."""

    def __init__(self, leg, cap):
        from conjugategradient_amd import _lib, problems
        from conjugategradient_amd.parallel import ConjugateGradientRankGpu
        from conjugategradient_amd.solver import VectorDouble

        self._lib = _lib
        self.L = _lib.lib()
        self.cap = cap
        if leg == "poisson512":
            self.N = 512 ** 3
            cg = ConjugateGradientRankGpu(self.N, 7, 0, cap, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE)
            cg.InitializePoisson(512, 512, 512)
        else:
            s = problems.convection_diffusion(256, 256, 256, CONVECTION[leg])
            self.N = s.Count
            cg = ConjugateGradientRankGpu(self.N, 7, 0, cap, 0.0, rank=0, world=1, rule=_lib.RULE_NATIVE).load(s)
            cg.Initialize()
            del s
        b = np.random.default_rng(7).standard_normal(self.N)
        cg.vectorB.CopyFrom(b, self.N)
        self.normb = float(np.linalg.norm(b))
        del b
        self.cg = cg
        self.four = [VectorDouble(self.N) for _ in range(4)]                  # v, s, t, rhat
        self.work = VectorDouble((max(MS) + 1) * (self.N + (self.N & 1)))     # GMRES: m + 1 slices; BiCGStab(2): 4
        self.it, self.res, self.true = C.c_int(0), C.c_double(0.0), C.c_double(0.0)

    def close(self):
        for v in self.four + [self.work]:
            v.Dispose()
        self.cg.Dispose()

    def run(self, form, tol=None, products=None):
        """One solve from x = 0.  form: "bicgstab", "bicgstabl_2" or ("gmres", m, orth).  Returns (status, products, ms of the call, Residual,
        TrueResidual)."""
        L, cg, p, _lib = self.L, self.cg, self.cg.part, self._lib
        per_it = 2 if form == "bicgstab" else 4 if form == "bicgstabl_2" else 1
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        L.MgcgDeviceSynchronize()
        head = (cg.cublas, cg.cusparse, cg.matDescr, cg.vectorElements.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr,
                cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr)
        cap = (self.cap if products is None else products) // per_it
        stop = (1e-8 * self.normb if tol is None else tol, 0, cap, _lib.RULE_NATIVE, C.byref(self.it), C.byref(self.res), C.byref(self.true), None, 0)
        t0 = time.perf_counter()
        if form == "bicgstab":
            st = L.SolveBicgstab(*head, *(v.Ptr for v in self.four), p.elementCount, self.N, *stop)
        elif form == "bicgstabl_2":
            st = L.SolveBicgstabL(*head, self.work.Ptr, 2, p.elementCount, self.N, *stop)
        else:
            st = L.SolveGmres(*head, self.work.Ptr, form[1], form[2], p.elementCount, self.N, *stop)
        ms = (time.perf_counter() - t0) * 1e3
        L.MgcgClearLastError()
        return st, self.it.value * per_it, ms, self.res.value, self.true.value

    def compare(self, repeats):
        forms = [("bicgstab", "bicgstab"), ("bicgstabl_2", "bicgstabl_2")] + [(f"gmres_{m}_orth{o}", ("gmres", m, o)) for m in MS for o in ORTHS]
        samples = {name: [] for name, _ in forms}
        out = dict(rows=self.N, relative_tolerance=1e-8, stop_level=1e-8 * self.normb, product_cap=self.cap)
        for name, form in forms:                       # round 0 warms up: code objects, matrix shape, the workspace's vectors
            self.run(form, tol=0.0, products=64)
        for _ in range(repeats):
            for name, form in forms:                   # the loops alternate, so a drift of the machine meets all alike
                st, products, ms, res, true = self.run(form)
                samples[name].append(ms)
                model = OTHERS[name] if name in OTHERS else PRODUCT + bytes_per_step(form[1], form[2])
                out[name] = dict(status=st, steps=products, residual=res, true_residual=true, true_to_residual=true / res if res else None,
                                 bytes_per_step=model)
        for name, _ in forms:
            med = median(samples[name])
            o = out[name]
            o.update(seconds_to_solution=med / 1e3, ms_per_step=med / max(o["steps"], 1), samples_ms=samples[name])
        base = out["bicgstabl_2"]
        for name, _ in forms:
            o = out[name]
            o["to_bicgstabl_2"] = dict(ms_per_step=o["ms_per_step"] / base["ms_per_step"], bytes_per_step=o["bytes_per_step"] / base["bytes_per_step"])
            o["predicted_ms_per_step"] = base["ms_per_step"] * o["bytes_per_step"] / base["bytes_per_step"]
        return out


def run_leg(leg, repeats, cap):
    from conjugategradient_amd import _lib

    _lib.require_gpu()
    if leg == "trace":
        b = Bench("convdiff256_mild", cap)
        b.run(("gmres", 20, 2), tol=0.0, products=39)      # 40 steps: two cycles
        b.run("bicgstab", tol=0.0, products=38)            # 20 bodies
        b.close()
        return dict(rows=b.N, steps=40)
    b = Bench(leg, cap)
    out = b.compare(repeats)
    b.close()
    return out


STATUS = {0: "OK", 1: "cap", 3: "NONFINITE"}


def readme(result):
    """The measured table as markdown; where GMRES is slower per step than BiCGStab(2) in the same process the row says so."""
    lines = ["# GMRES(m) beside BiCGStab and BiCGStab(2), one MI355X, plain form", "",
             "Written by `python -m conjugategradient_amd.tools.gmres_run --out profiles/gmres`; the numbers are in `gmres_run.json`.",
             "N(0,1) right-hand side, x = 0, stop at a relative 1e-8 (MGCG_RULE_NATIVE), at most `product_cap` products (see the json); median of",
             "the repeats, the loops alternated inside one process.  A step is one product.  Status: what the call returned (cap: the product",
             "cap; NONFINITE: a breakdown).  'predicted': BiCGStab(2)'s measured ms per product in the same process times the byte model's ratio.",
             "What the tables say, and the kernel trace: `READING.md`, written by hand -- this tool never touches it.", ""]
    for leg in LEGS:
        if leg not in result:
            continue
        r = result[leg]
        lines += [f"## {leg} ({r['rows']} rows, at most {r['product_cap']} products)", "",
                  "| loop | status | steps | ms / step | predicted | bytes / row / step (model) | x BiCGStab(2) per step (model) | s to solution | TrueResidual / Residual | |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for name, o in r.items():
            if not isinstance(o, dict):
                continue
            t = o["to_bicgstabl_2"]
            note = "slower today" if name.startswith("gmres") and t["ms_per_step"] > 1.0 else ""
            lines.append(f"| {name} | {STATUS.get(o['status'], o['status'])} | {o['steps']} | {o['ms_per_step']:.3f} | {o['predicted_ms_per_step']:.3f} | {o['bytes_per_step']:.0f} | "
                         f"{t['ms_per_step']:.2f} ({t['bytes_per_step']:.2f}) | {o['seconds_to_solution']:.3f} | {o['true_to_residual']:.3g} | {note} |")
        lines.append("")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="a directory: gmres_run.json and README.md are written there")
    ap.add_argument("--leg", choices=list(LEGS) + ["trace"], default=None, help="run this leg in this process")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), help="the legs to run, each as a child process under its own time limit")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cap", type=int, default=MAX_PRODUCTS, help="at most this many products per solve")
    a = ap.parse_args()
    if a.leg:
        result = {a.leg: run_leg(a.leg, a.repeats, a.cap)}
    else:
        result = {"byte_model_per_row_per_step": {"product": PRODUCT, **{k: v for k, v in OTHERS.items()},
                                                  **{f"gmres_{m}_orth{o}": PRODUCT + bytes_per_step(m, o) for m in MS for o in ORTHS}}}
        for leg in a.legs:
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.gmres_run", "--leg", leg, "--repeats", str(a.repeats), "--cap", str(a.cap)],
                                   stdout=subprocess.PIPE, timeout=LEGS[leg], check=True)      # a leg that fails or hangs ends the script
            result.update(json.loads(child.stdout))
            if a.out:                                      # what is measured so far survives a later leg's failure
                write(a.out, result)
    print(json.dumps(result, indent=1))
    if a.out:
        write(a.out, result)


def write(out, result):
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "gmres_run.json"), "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    with open(os.path.join(out, "README.md"), "w") as f:
        f.write(readme(result) + "\n")


if __name__ == "__main__":
    main()
