"""Measurement only: the multicolour Gauss-Seidel smoother (MgSetSmoother(mg, 1)) against the weighted-Jacobi smoother ON THE SAME
HIERARCHY in the same process, and the one-level SSOR form against SolveEx and SolveJacobi on the same system.

Every system is a leg of its own: a child process under its own time limit, so that one leg's failure or timeout costs the others
nothing.  A leg builds the library's aggregates (MgSetupAggregation, 8 levels, the hierarchy's omega), measures the Jacobi cycle, switches
the same handle to mode 1 (the colouring set-up: wall time with the device drained either side), measures again, and then builds the
one-level hierarchy (MgSetupAggregates with levels = 1, nuCoarse = 2, omega = 1: SSOR).  Reported per form:

  ms_per_cycle      MgApply enqueued K times between two device synchronisations, median of the repeats
  ms_per_iteration  the loop at tolerance 0 under caps K1 < K2, (t2 - t1) / (K2 - K1) (amg_cg_run's measure), median of the repeats
  to_1e-8           one solve from x = 0 to || r || < 1e-8 || b ||: iterations and seconds
  bytes_model       per sweep: the level's matrix once (12 B per entry, 4 B per row of offsets), b, dinv and x read and x written (32 B per
                    row), plus -- Gauss-Seidel only -- 4 B per row of list; summed over the sweeps of one cycle on every level

  poisson256   256^3 7-point Poisson (device generator), N(0,1) right-hand side, omega 6/7
  permuted128  the 128^3 matrix with rows and columns permuted, omega 6/7
  random1m     problems.random_spd(1 000 000), omega 0.8
  graph64      the Laplacian of the 64^3 grid graph with edge weights 10^U(0,3) plus 1e-3 I, omega 0.8

    python -m conjugategradient_amd.tools.gs_smoother_run --out profiles/gs/gs_smoother_run.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.solver import _ptr
from conjugategradient_amd.tools.amg_cg_run import OMEGA_STENCIL, Bench, own, permuted_poisson, randn_rhs

LEGS = ("poisson256", "permuted128", "random1m", "graph64")


def graph_laplacian(n, seed=3, shift=1e-3):
    """The Laplacian of the n^3 grid graph with edge weights 10^U(0, 3), plus shift * I; b ~ N(0,1)."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    idx = np.arange(n ** 3).reshape(n, n, n)
    a = np.concatenate([idx[:-1].ravel(), idx[:, :-1].ravel(), idx[:, :, :-1].ravel()])
    b = np.concatenate([idx[1:].ravel(), idx[:, 1:].ravel(), idx[:, :, 1:].ravel()])
    w = 10.0 ** rng.uniform(0.0, 3.0, len(a))
    W = sp.coo_matrix((np.r_[w, w], (np.r_[a, b], np.r_[b, a])), shape=(n ** 3, n ** 3)).tocsr()
    A = (sp.diags(np.asarray(W.sum(axis=1)).ravel() + shift) - W).tocsr()
    A.sort_indices()
    rhs = np.random.default_rng(20261019).standard_normal(n ** 3)
    return problems.LinearSystem(A.data, A.indices.astype(np.int32), A.indptr.astype(np.int32), np.zeros(n ** 3), rhs, f"graph-laplacian-{n}")


def make_bench(leg):
    """(Bench, omega) of a leg: the matrix on the device, no hierarchy yet."""
    if leg == "poisson256":
        n = 256
        cg = ConjugateGradientAmgGpu(n ** 3, 7, 0, 10, 0.0, levels=1, omega=OMEGA_STENCIL)
        cg.InitializePoisson((n, n, n))
        return Bench(cg, randn_rhs(cg)), OMEGA_STENCIL
    s, omega = {"permuted128": lambda: (permuted_poisson(128), OMEGA_STENCIL), "random1m": lambda: (problems.random_spd(1_000_000), 0.8),
                "graph64": lambda: (graph_laplacian(64), 0.8)}[leg]()
    if leg == "random1m":
        s.b = np.random.default_rng(20261019).standard_normal(s.Count)
    cg = ConjugateGradientAmgGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 10, 0.0, levels=1, omega=omega).load(s)
    cg.Initialize()
    return Bench(cg, float(np.linalg.norm(s.b))), omega


def cycle_ms(b, mg, k, repeats):
    """MgApply k times between two synchronisations, per cycle; median of the repeats after one warm-up round."""
    L, cg = b.L, b.cg
    r, z = cg.vectorB.ToRawPtr(), cg.vectorZ.ToRawPtr()
    samples = []
    for rep in range(repeats + 1):
        L.MgcgDeviceSynchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            L.MgApply(mg, r, z)
        L.MgcgDeviceSynchronize()
        if rep:
            samples.append((time.perf_counter() - t0) * 1e3 / k)
    _lib.check("MgApply")
    return sorted(samples)[len(samples) // 2], samples


def bytes_model(b, mg, gs):
    """Bytes of the smoothing sweeps of one cycle by the docstring's model (the residual pass and the transfers are the same in both modes)."""
    L = b.L
    levels = L.MgLevels(mg)
    total = 0
    for l in range(levels):
        n, nnz = int(L.MgLevelRows(mg, l)), int(L.MgLevelNnz(mg, l))
        sweeps = 4 if l == levels - 1 else 2                     # nuCoarse = 4 on the last level (2 in the one-level form, see ssor), nu = 1 before and after
        total += sweeps * (12 * nnz + 4 * n + 32 * n + (4 * n if gs else 0))
    return total


def measure(b, form, mg, caps, repeats, gs, sweeps_last=None):
    out = dict(rows_per_level=b.mg[form][2])
    out["ms_per_cycle"], out["cycle_samples"] = cycle_ms(b, mg, 20, repeats)
    samples = []
    for rep in range(repeats + 1):
        (sa, _, ta), (sb, _, tb) = b.call(form, 0.0, caps[0]), b.call(form, 0.0, caps[1])
        if rep and sa == _lib.MAXIT_EXCEEDED and sb == _lib.MAXIT_EXCEEDED:
            samples.append((tb - ta) / (caps[1] - caps[0]))
    out["ms_per_iteration"] = sorted(samples)[len(samples) // 2] if samples else None
    st, it, ms = b.call(form, 1e-8 * b.bnorm, 20000)
    out["to_1e-8"] = dict(status=st, iterations=it, seconds=ms / 1e3, residual_over_b=b.res.value / b.bnorm)
    model = bytes_model(b, mg, gs)
    if sweeps_last is not None:                                   # the one-level form: sweeps_last sweeps in all
        n, nnz = b.N, b.nnz
        model = sweeps_last * (12 * nnz + 4 * n + 32 * n + (4 * n if gs else 0))
    out["sweep_bytes_model"] = model
    if gs:
        out["colours_per_level"] = [int(b.L.MgLevelColours(mg, l)) for l in range(b.L.MgLevels(mg))]
    return out


def run_leg(leg, caps, repeats):
    b, omega = make_bench(leg)
    L = b.L
    out = dict(rows=b.N, nnz=b.nnz, omega=omega)
    # plain and Jacobi CG on the same system
    for form in ("plain", "jacobi"):
        st, it, ms = b.call(form, 1e-8 * b.bnorm, 20000)
        out[form] = {"to_1e-8": dict(status=st, iterations=it, seconds=ms / 1e3)}
    b.setup("vcycle", lambda L_, *m: own(8, omega)(L_, *m, b.N))
    mg = b.mg["vcycle"][0]
    out["setup_seconds"] = b.mg["vcycle"][1]
    out["vcycle_jacobi"] = measure(b, "vcycle", mg, caps, repeats, gs=False)
    L.MgcgDeviceSynchronize()
    t0 = time.perf_counter()
    status = L.MgSetSmoother(mg, 1)
    L.MgcgDeviceSynchronize()
    out["colouring_seconds"] = time.perf_counter() - t0
    if status != 0:
        out["vcycle_gs"] = dict(refused=_lib.last_error())
        L.MgcgClearLastError()
    else:
        out["vcycle_gs"] = measure(b, "vcycle", mg, caps, repeats, gs=True)
        out["vcycle_gs"]["cycle_ratio_to_jacobi"] = out["vcycle_gs"]["ms_per_cycle"] / out["vcycle_jacobi"]["ms_per_cycle"]
        out["vcycle_gs"]["model_ratio_to_jacobi"] = out["vcycle_gs"]["sweep_bytes_model"] / out["vcycle_jacobi"]["sweep_bytes_model"]
    # one level, forward + backward sweep, omega = 1: SSOR
    rows = np.asarray([b.N], dtype=np.int32)
    none = np.zeros(1, dtype=np.int32)
    b.setup("ssor", lambda L_, *m: L_.MgSetupAggregates(*m, b.N, 1, _ptr(rows), _ptr(none), 1.0, 1, 2, 0.5))
    one = b.mg["ssor"][0]
    L.MgcgDeviceSynchronize()
    t0 = time.perf_counter()
    status = L.MgSetSmoother(one, 1)
    L.MgcgDeviceSynchronize()
    seconds = time.perf_counter() - t0
    if status != 0:
        out["ssor"] = dict(refused=_lib.last_error())
        L.MgcgClearLastError()
    else:
        out["ssor"] = measure(b, "ssor", one, caps, repeats, gs=True, sweeps_last=2)
        out["ssor"]["colouring_seconds"] = seconds
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--legs", nargs="*", default=list(LEGS), choices=LEGS)
    ap.add_argument("--leg", default=None, choices=LEGS, help="run this one leg in this process and print its JSON (what the parent starts)")
    ap.add_argument("--timeout", type=int, default=240, help="seconds a leg may take")
    ap.add_argument("--caps", type=int, nargs=2, default=[5, 25])
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        _lib.require_gpu()
        print("RESULT " + json.dumps(run_leg(a.leg, a.caps, a.repeats)), flush=True)
        return
    result = {}
    for leg in a.legs:
        cmd = [sys.executable, "-m", "conjugategradient_amd.tools.gs_smoother_run", "--leg", leg, "--caps", str(a.caps[0]), str(a.caps[1]), "--repeats", str(a.repeats)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.timeout)
        except subprocess.TimeoutExpired:
            result[leg] = dict(error=f"timed out after {a.timeout} s")
            print(leg, json.dumps(result[leg]), flush=True)
            break                                                 # a leg that hangs: start nothing more on the device
        lines = [ln for ln in done.stdout.splitlines() if ln.startswith("RESULT ")]
        if done.returncode != 0 or not lines:
            result[leg] = dict(error=f"exit status {done.returncode}", stderr=done.stderr[-2000:])
            print(leg, json.dumps(result[leg]), flush=True)
            if done.returncode < 0 or done.returncode in (134, 139):
                break                                             # a fault: start nothing more on the device
            continue
        result[leg] = json.loads(lines[-1][len("RESULT "):])
        print(leg, json.dumps(result[leg]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
