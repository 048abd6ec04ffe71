"""Measurement only: what the device matrix product C = A B (MgcgCsrMultiply) costs on one GPU, phase by phase, next to a byte model, to
scipy.sparse on the host and -- for the Galerkin triple product -- to the one-lane Galerkin kernels the aggregation set-up runs today.  No
figure here is an acceptance threshold.

  poisson-squared    A A of the 7-point Poisson matrix of an n^3 grid (--grid, 256 by default: 16.8 M rows, 49 products a row)
  upwind-normal      A^T A of the n^3 upwind convection-diffusion matrix, c = (2, 1, .5); A^T comes from MgcgCsrTranspose
  random-squared     A A of random_nonsymmetric(--random-rows, 10^6 by default): 9 entries a row, columns uniform -- no locality in the gathered rows of B
  galerkin-triple    P^T (A P) of the n^3 Poisson matrix for the first-level map of the library's own matching (MgSetupAggregation): two
                     products and one transposition, against the set-up of the two-level hierarchy of the same map (MgSetupAggregates: the
                     one-lane Galerkin kernels, the diagonal pass and the upload of the map), in the same process

Per product, with both matrices resident on the device: the count-only call (the symbolic phase: checks, products per row, count pass) and
the full call (both phases); numeric = full - symbolic.  One call warms up, three follow; all three and their median are recorded.  Then
products per second of the full call, the share of rows in each class, the byte model (A once: 12 B an entry and 4 B a row; the gathered
rows of B: 12 B a product; C once: 12 B an entry and 4 B a row) with the bandwidth the full call reaches on it, and scipy.sparse's time for
the same product on the host (--no-scipy leaves it out).

Every leg is a child process of its own under a time limit of its own; the script ends at the first leg that fails.

    python -m conjugategradient_amd.tools.spgemm_run --out profiles/spgemm/spgemm_run.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

SYSTEMS = ("poisson-squared", "upwind-normal", "random-squared", "galerkin-triple")
LIMIT_S = 900                                                 # a leg's time limit
RUNS = 3


def median(v):
    return sorted(v)[len(v) // 2]


def products_per_row(a, b):
    """u_i of A B from the host copies (elements, columns, offsets)"""
    roa, rob = np.asarray(a[2], dtype=np.int64), np.asarray(b[2], dtype=np.int64)
    length = np.r_[0, np.cumsum(np.diff(rob)[np.asarray(a[1][: roa[-1]], dtype=np.int64)])]
    return length[roa[1:]] - length[roa[:-1]]


class Product:
    """A and B resident on the device; timed calls of MgcgCsrMultiply on them"""

    def __init__(self, a, b, columns):
        from conjugategradient_amd import _lib
        from conjugategradient_amd.solver import ConjugateGradientGpu, VectorDouble, VectorInt

        self.L, self.check = _lib.lib(), _lib.check
        self.kinds = (VectorDouble, VectorInt)
        self.a, self.b, self.columns = a, b, int(columns)
        self.rows, self.inner = len(a[2]) - 1, len(b[2]) - 1
        self.blas, self.sparse = ConjugateGradientGpu.CreateBlas(), ConjugateGradientGpu.CreateSparse()
        self.vectors = []
        args = []
        for e, c, ro in (a, b):
            nnz = int(ro[-1])
            for kind, host, dtype in ((VectorDouble, e[:nnz], np.float64), (VectorInt, ro, np.int32), (VectorInt, c[:nnz], np.int32)):
                v = kind(max(len(host), 1))
                if len(host):
                    v.CopyFrom(np.ascontiguousarray(host, dtype=dtype), len(host))
                self.vectors.append(v)
                args.append(v.Ptr)
            args.append(nnz)
        self.args = (self.blas, self.sparse, *args, self.rows, self.inner, self.columns)

    def timed(self, call):
        samples, got = [], None
        for rep in range(RUNS + 1):
            self.L.MgcgDeviceSynchronize()
            t = time.perf_counter()
            got = call()
            self.L.MgcgDeviceSynchronize()
            if rep:
                samples.append((time.perf_counter() - t) * 1e3)
            self.check("MgcgCsrMultiply")
            assert got >= 0, got
        return dict(samples_ms=samples, median_ms=median(samples)), got

    def measure(self, scipy_too, keep=False):
        from conjugategradient_amd import amg

        short, lds = amg.multiply_class_limits()
        u = products_per_row(self.a, self.b)
        out = dict(rows=self.rows, inner=self.inner, columns=self.columns, entries_a=int(self.a[2][-1]), entries_b=int(self.b[2][-1]), products=int(u.sum()),
                   most_products_in_a_row=int(u.max()),
                   rows_by_class=dict(register=float((u <= short).mean()), lds=float(((u > short) & (u <= lds)).mean()), global_scratch=float((u > lds).mean())))
        out["symbolic"], count = self.timed(lambda: self.L.MgcgCsrMultiply(*self.args, None, None, None, 0))
        VectorDouble, VectorInt = self.kinds
        outputs = [VectorDouble(max(count, 1)), VectorInt(self.rows + 1), VectorInt(max(count, 1))]
        out["full"], again = self.timed(lambda: self.L.MgcgCsrMultiply(*self.args, *(v.Ptr for v in outputs), count))
        assert again == count, (again, count)
        out["entries_c"] = int(count)
        out["numeric_ms"] = out["full"]["median_ms"] - out["symbolic"]["median_ms"]
        out["products_per_s"] = out["products"] / (out["full"]["median_ms"] * 1e-3)
        model = 12 * out["entries_a"] + 4 * self.rows + 12 * out["products"] + 12 * count + 4 * self.rows
        out["byte_model"] = dict(bytes=int(model), reached_gb_per_s=model / (out["full"]["median_ms"] * 1e-3) / 1e9)
        result = None
        if keep:
            result = (outputs[0].to_numpy(max(count, 1))[:count], outputs[2].to_numpy(max(count, 1))[:count], outputs[1].to_numpy(self.rows + 1))
        for v in outputs:
            v.Dispose()
        if scipy_too:
            import scipy.sparse as sp

            A = sp.csr_matrix((self.a[0][: self.a[2][-1]], self.a[1][: self.a[2][-1]], self.a[2]), shape=(self.rows, self.inner))
            B = sp.csr_matrix((self.b[0][: self.b[2][-1]], self.b[1][: self.b[2][-1]], self.b[2]), shape=(self.inner, self.columns))
            t = time.perf_counter()
            S = A @ B
            out["scipy_host_ms"] = (time.perf_counter() - t) * 1e3
            out["scipy_entries"] = int(S.nnz)
            out["scipy_over_full"] = out["scipy_host_ms"] / out["full"]["median_ms"]
        return out, result

    def dispose(self):
        for v in self.vectors:
            v.Dispose()
        self.L.DestroyBlas(self.blas)
        self.L.DestroySparse(self.sparse)


def csr_of(s):
    return np.asarray(s.Elements[: s.nnz], dtype=np.float64), np.asarray(s.ColumnIndeces[: s.nnz], dtype=np.int32), np.asarray(s.RowOffsets, dtype=np.int32)


def run_leg(name, grid, random_rows, scipy_too):
    from conjugategradient_amd import _lib, amg, problems

    _lib.require_gpu()
    t0 = time.perf_counter()
    out = {}
    if name == "poisson-squared":
        s = problems.poisson(grid, grid, grid)
        a = b = csr_of(s)
    elif name == "upwind-normal":
        s = problems.convection_diffusion(grid, grid, grid, (2.0, 1.0, 0.5), upwind=True)
        b = csr_of(s)
        a = amg.csr_transpose_gpu(*b, s.Count)
    elif name == "random-squared":
        s = problems.random_nonsymmetric(random_rows)
        a = b = csr_of(s)
    else:
        return run_triple(grid, scipy_too)
    out["host_build_s"] = time.perf_counter() - t0
    p = Product(a, b, s.Count)
    out["product"], _ = p.measure(scipy_too)
    p.dispose()
    return out


def run_triple(grid, scipy_too):
    from conjugategradient_amd import _lib, amg, problems

    L = _lib.lib()
    s = problems.poisson(grid, grid, grid)
    A = csr_of(s)
    cg = amg.ConjugateGradientAmgGpu(s.Count, 7, 0, 10, 1e-8, levels=2, rule=_lib.RULE_NATIVE).load(s)
    cg.Initialize()                                           # the library's own matching: its first-level map
    amap = cg.level_aggregates(0)
    cg.Dispose()
    nc = int(amap.max()) + 1
    P = (np.ones(s.Count), amap.astype(np.int32), np.arange(s.Count + 1, dtype=np.int32))
    out = dict(rows=s.Count, coarse_rows=nc)
    t = time.perf_counter()
    Pt = amg.csr_transpose_gpu(*P, nc)                        # (with its uploads and downloads: the product's legs below keep their matrices resident)
    out["transpose_with_copies_ms"] = (time.perf_counter() - t) * 1e3
    first = Product(A, P, nc)
    out["a_times_p"], AP = first.measure(scipy_too, keep=True)
    first.dispose()
    second = Product(Pt, AP, nc)
    out["pt_times_ap"], _ = second.measure(scipy_too)
    second.dispose()
    out["two_products_full_ms"] = out["a_times_p"]["full"]["median_ms"] + out["pt_times_ap"]["full"]["median_ms"]
    # the one-lane Galerkin kernels on the same map: the set-up of the two-level hierarchy (sigma = 1)
    two = amg.ConjugateGradientAmgGpu(s.Count, 7, 0, 10, 1e-8, sigma=1.0, aggregates=[amap], rule=_lib.RULE_NATIVE).load(s)
    two.Initialize()
    samples = []
    for rep in range(RUNS + 1):
        L.MgcgDeviceSynchronize()
        t = time.perf_counter()
        two.Setup()
        L.MgcgDeviceSynchronize()
        if rep:
            samples.append((time.perf_counter() - t) * 1e3)
    out["one_lane_galerkin_setup"] = dict(samples_ms=samples, median_ms=median(samples), coarse_entries=int(two.level_csr(1)[2][-1]))
    two.Dispose()
    out["products_over_one_lane_setup"] = out["two_products_full_ms"] / out["one_lane_galerkin_setup"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--systems", nargs="*", default=list(SYSTEMS), choices=list(SYSTEMS))
    ap.add_argument("--grid", type=int, default=256, help="n of the n^3 grids")
    ap.add_argument("--random-rows", type=int, default=1000000)
    ap.add_argument("--no-scipy", action="store_true", help="leave the host comparator out")
    ap.add_argument("--leg", default=None, help="run this system in this process")
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(run_leg(a.leg, a.grid, a.random_rows, not a.no_scipy)))
        return
    result = dict(grid=a.grid, random_rows=a.random_rows)
    for name in a.systems:
        command = [sys.executable, "-m", "conjugategradient_amd.tools.spgemm_run", "--leg", name, "--grid", str(a.grid), "--random-rows", str(a.random_rows)]
        child = subprocess.run(command + (["--no-scipy"] if a.no_scipy else []), stdout=subprocess.PIPE, timeout=LIMIT_S, check=True)      # a leg that fails or hangs ends the script
        result[name] = json.loads(child.stdout)
        print(json.dumps({name: result[name]}), file=sys.stderr, flush=True)
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
