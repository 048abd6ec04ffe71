"""Measurement only: what the aggregation V-cycle (MgSetupAggregation / MgSetupAggregates + SolveMg) costs next to SolveEx, SolveJacobi
and, on grids, the geometric SolveMg -- in one process on one GPU, the forms alternated inside every repeat, median of the repeats.

Set-up: wall time of the set-up call, the device drained before and after.  Per iteration: every loop runs with tolerance 0 under an
iteration cap, and the time of K1 bodies is subtracted from that of K2 so that the start of a call drops out.  To solution: every form
once from x = 0 to || r || < 1e-8 || b || (the absolute 2-norm rule with that bound: SolveMg has no relative rule), iterations and
seconds; the generated systems get an N(0,1) right-hand side.  omega = 6/7 on the stencils, the class default 0.8 elsewhere.

  poisson   n^3 7-point Poisson from the device generator (--n 512 256): plain, Jacobi, the geometric hierarchy (3 levels), the SAME
            hierarchy from 2x2x2 box maps through MgSetupAggregates (the indexed transfer priced against the geometric kernels),
            and the library's own aggregates (3 levels, and the default 8)
  permuted  the m^3 matrix with rows and columns permuted (--permuted 256): plain, Jacobi, the library's aggregates
  random    problems.random_spd at BASELINE config 5's size (--random 10000000): the same
  drivers   problems.mgcg_main() and problems.viennacl_main() at full size: the same

    python -m conjugategradient_amd.tools.amg_cg_run --out profiles/amg/amg_cg_run.json
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
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.solver import VectorDouble, _ptr

OMEGA_STENCIL = 6.0 / 7.0


def box_maps(n, levels):
    """The 2x2x2 maps of an n^3 grid, int32 throughout (the finest one of 512^3 is 0.5 GB)."""
    maps = []
    for _ in range(levels - 1):
        if n % 2:
            break
        h = n // 2
        i = np.arange(n, dtype=np.int32) // 2
        maps.append(((i[:, None, None] * h + i[None, :, None]) * h + i[None, None, :]).ravel())
        n = h
    return maps


class Bench:
    """One matrix on the device (in a ConjugateGradientAmgGpu's vectors), the hierarchies built on it and the loops' calls."""

    def __init__(self, cg, bnorm):
        self.L, self.cg, self.bnorm = _lib.lib(), cg, bnorm
        self.N = cg.Count
        self.nnz = int(cg.A.RowOffsets[cg.Count]) if cg.A is not None else cg._nnz
        self.dinv = VectorDouble(self.N)
        if self.L.MgcgJacobiSetup(cg.cusparse, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, self.nnz, self.N, 0, self.dinv.Ptr) != 0:
            _lib.check("MgcgJacobiSetup")
        self.mg = {}                                   # form -> (handle, set-up seconds, rows per level)
        self.it, self.res = C.c_int(0), C.c_double(0.0)

    def _matrix(self):
        cg = self.cg
        return (cg.cublas, cg.cusparse, cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr, self.nnz)

    def setup(self, form, call):
        """call(L, *matrix) -> hierarchy; timed with the device drained either side."""
        L = self.L
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        mg = call(L, *self._matrix())
        L.MgcgDeviceSynchronize()
        seconds = time.perf_counter() - t0
        _lib.check(form)
        if not mg:
            raise _lib.MgcgError(f"{form}: the set-up returned NULL")
        self.mg[form] = (mg, seconds, [int(L.MgLevelRows(mg, l)) for l in range(L.MgLevels(mg))])

    def close(self):
        for mg, _, _ in self.mg.values():
            self.L.MgDestroy(mg)
        self.dinv.Dispose()
        self.cg.Dispose()

    def call(self, form, tol, cap):
        """One solve from x = 0 under the absolute 2-norm rule: (status, iterations, ms)."""
        L, cg = self.L, self.cg
        L.MgcgFill(cg.vectorX.Ptr, 0.0)
        L.MgcgDeviceSynchronize()
        head = (cg.cublas, cg.cusparse, cg.matDescr)
        mat = (cg.vectorA.Ptr, cg.vectorRowOffsets.Ptr, cg.vectorColumnIndeces.Ptr)
        vec = (cg.vectorX.Ptr, cg.vectorB.Ptr, cg.vectorAp.Ptr, cg.vectorP.Ptr, cg.vectorR.Ptr)
        tail = (self.nnz, self.N, tol, 0, cap, _lib.RULE_CSHARP, C.byref(self.it), C.byref(self.res), None, 0)
        t0 = time.perf_counter()
        if form == "plain":
            st = L.SolveEx(*head, *mat, *vec, *tail)
        elif form == "jacobi":
            st = L.SolveJacobi(*head, *mat, *vec, self.dinv.Ptr, *tail)
        else:
            st = L.SolveMg(*head, self.mg[form][0], *mat, *vec, cg.vectorZ.Ptr, *tail)
        ms = (time.perf_counter() - t0) * 1e3
        L.MgcgClearLastError()
        return st, self.it.value, ms

    def forms(self):
        return ["plain", "jacobi"] + list(self.mg)

    def cost(self, k1, k2, repeats):
        samples = {f: [] for f in self.forms()}
        for rep in range(repeats + 1):                 # round 0 warms up
            for f in self.forms():                     # the forms alternate, so a drift of the machine meets all alike
                (sa, _, a), (sb, _, b) = self.call(f, 0.0, k1), self.call(f, 0.0, k2)
                if rep and sa == _lib.MAXIT_EXCEEDED and sb == _lib.MAXIT_EXCEEDED:
                    samples[f].append((b - a) / (k2 - k1))
        out = {}
        for f, v in samples.items():
            out[f] = dict(ms_per_iteration=sorted(v)[len(v) // 2] if v else None, samples=v)
        return out

    def to_solution(self, rel=1e-8, cap=20000):
        out = {}
        for f in self.forms():
            st, it, ms = self.call(f, rel * self.bnorm, cap)
            out[f] = dict(status=st, iterations=it, seconds=ms / 1e3, residual_over_b=self.res.value / self.bnorm)
        return out

    def report(self, caps, repeats, solution=True):
        out = dict(rows=self.N, nnz=self.nnz)
        out["setup"] = {f: dict(seconds=s, rows_per_level=rows) for f, (_, s, rows) in self.mg.items()}
        out["per_iteration"] = self.cost(caps[0], caps[1], repeats)
        if solution:
            out["to_1e-8"] = self.to_solution()
        return out


def randn_rhs(cg):
    """An N(0,1) right-hand side, uploaded in pieces; returns its 2-norm."""
    rng = np.random.default_rng(20261019)
    piece, ss = 1 << 24, 0.0
    for lo in range(0, cg.Count, piece):
        n = min(piece, cg.Count - lo)
        v = rng.standard_normal(n)
        ss += float(v @ v)
        cg.vectorB.CopyFrom(v, n, 0, lo)
    return math.sqrt(ss)


def own(levels, omega):
    return lambda L, *m: L.MgSetupAggregation(*m[:6], m[6], levels, 3, 0.25, 64, omega, 1, 4, 0.5)


def poisson_bench(n, levels):
    N = n ** 3
    cg = ConjugateGradientAmgGpu(N, 7, 0, 10, 0.0, levels=1, omega=OMEGA_STENCIL)       # (its own one-level hierarchy is not measured)
    cg.InitializePoisson((n, n, n))
    b = Bench(cg, randn_rhs(cg))
    count = (N,)
    b.setup("geometric", lambda L, *m: L.MgSetup(*m, n, n, n, levels, OMEGA_STENCIL, 1, 4, 0.5))
    maps = box_maps(n, levels)
    rows = np.asarray([N] + [int(m.max()) + 1 for m in maps], dtype=np.int32)
    flat = np.concatenate(maps)
    b.setup("box_aggregates", lambda L, *m: L.MgSetupAggregates(*m, *count, len(rows), _ptr(rows), _ptr(flat), OMEGA_STENCIL, 1, 4, 0.5))
    del maps, flat
    b.setup(f"own_aggregates_{levels}_levels", lambda L, *m: own(levels, OMEGA_STENCIL)(L, *m, *count))
    b.setup("own_aggregates_8_levels", lambda L, *m: own(8, OMEGA_STENCIL)(L, *m, *count))
    return b


def system_bench(s, omega, levels=(8,)):
    cg = ConjugateGradientAmgGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 10, 0.0, levels=1, omega=omega).load(s)
    cg.Initialize()
    b = Bench(cg, float(np.linalg.norm(s.b)))
    for lv in levels:
        b.setup(f"own_aggregates_{lv}_levels", lambda L, *m, lv=lv: own(lv, omega)(L, *m, s.Count))
    return b


def permuted_poisson(n, seed=7):
    """P A P^T of the n^3 7-point matrix for a seeded permutation, columns sorted, b ~ N(0,1)."""
    s = problems.poisson(n, n, n)
    A = s.to_scipy()
    perm = np.random.default_rng(seed).permutation(s.Count)
    A = A[perm][:, perm].tocsr()
    A.sort_indices()
    b = np.random.default_rng(20261019).standard_normal(s.Count)
    return problems.LinearSystem(A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32), np.zeros(s.Count), b, f"poisson{n}-permuted")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--n", type=int, nargs="*", default=[512, 256], help="n of the n^3 Poisson runs")
    ap.add_argument("--levels", type=int, default=3, help="levels of the geometric hierarchy and of its box-aggregate twin")
    ap.add_argument("--permuted", type=int, default=256, help="n of the permuted n^3 run (0: skip)")
    ap.add_argument("--random", type=int, default=10_000_000, help="rows of the random_spd run (0: skip)")
    ap.add_argument("--caps", type=int, nargs=2, default=[5, 25])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip", nargs="*", default=[], choices=["poisson", "drivers", "solution"])
    a = ap.parse_args()
    _lib.require_gpu()
    result = {}
    solution = "solution" not in a.skip

    def finish(name, b):
        result[name] = b.report(a.caps, a.repeats, solution)
        b.close()
        print(name, json.dumps(result[name]), flush=True)

    if "poisson" not in a.skip:
        for n in a.n:
            finish(f"poisson{n}", poisson_bench(n, a.levels))
    if a.permuted:
        finish(f"poisson{a.permuted}_permuted", system_bench(permuted_poisson(a.permuted), OMEGA_STENCIL, levels=(3, 8)))
    if a.random:
        finish(f"random_spd_{a.random}", system_bench(problems.random_spd(a.random), 0.8))
    if "drivers" not in a.skip:
        for name, make in (("mgcg_main", problems.mgcg_main), ("viennacl_main", problems.viennacl_main)):
            finish(name, system_bench(make(), 0.8))
    text = json.dumps(result, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
