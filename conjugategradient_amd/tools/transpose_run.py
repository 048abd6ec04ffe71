"""Measurement only: what the device transposition (MgcgCsrTranspose) costs and what it takes off MgcgSymmetricPart and off the set-up of
MgSetupAggregationEx(strength = 1), on one GPU, against the library of the PARENT commit (whose MgcgSymmetricPart sorts the entries by
column on the host) in the same session.  No figure here is an acceptance threshold but one: the slowest of this library's three
MgcgSymmetricPart runs on the 256^3 stencil must be faster than the fastest of the parent's three (--check makes the script fail otherwise).

  upwind256        256^3 convection_diffusion, c = (2, 1, .5), first-order upwinding: 16.8 M rows, 117 M entries, every column stored 7 times or less
  random1000000    random_nonsymmetric(1 000 000): 9 entries a row, columns uniform -- no locality in the claim pass

Per leg, on one copy of the matrix on the device: MgcgCsrTranspose with values and source list (this commit's library alone: the parent has
no such export), MgcgSymmetricPart (count only: no output is copied) and the set-up of the class's default hierarchy with
strength = "symmetric".  One call warms up, three follow; all three and their median are recorded.

Every leg is a child process of its own under a time limit of its own, once with the library in the tree and once with --parent-lib (the
parent commit's libMgcgGpu.so, built from a checkout of that commit into a directory outside the tree, loaded through MGCG_LIB_PATH); the
script ends at the first leg that fails.

    python -m conjugategradient_amd.tools.transpose_run --parent-lib /somewhere/parent/libMgcgGpu.so --check --out profiles/transpose/transpose_run.json
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

SYSTEMS = ("upwind256", "random1000000")
LIMIT_S = 900                                                 # a leg's time limit
RUNS = 3
NEW_EXPORTS = ("MgcgCsrTranspose", "MgcgTransposeClassLimits")


def median(v):
    return sorted(v)[len(v) // 2]


def run_leg(name, parent):
    from conjugategradient_amd import _lib

    if parent:                                                # the parent's library lacks the new exports: do not ask it for them
        for export in NEW_EXPORTS:
            _lib.SIGNATURES.pop(export, None)
    from conjugategradient_amd import problems
    from conjugategradient_amd.amg import ConjugateGradientAmgGpu
    from conjugategradient_amd.solver import VectorDouble, VectorInt

    _lib.require_gpu()
    L = _lib.lib()
    t0 = time.perf_counter()
    s = problems.convection_diffusion(256, 256, 256, (2.0, 1.0, 0.5), upwind=True) if name == "upwind256" else problems.random_nonsymmetric(1000000)
    out = dict(library_of="parent_commit" if parent else "this_commit", rows=s.Count, nonzeros=s.nnz, host_build_s=time.perf_counter() - t0)

    def three(call):
        samples = []
        for rep in range(RUNS + 1):
            L.MgcgDeviceSynchronize()
            t = time.perf_counter()
            got = call()
            L.MgcgDeviceSynchronize()
            if rep:
                samples.append(time.perf_counter() - t)
            _lib.check(name)
        return dict(samples_s=samples, median_s=median(samples), fastest_s=min(samples), slowest_s=max(samples)), got

    agg = ConjugateGradientAmgGpu(s.Count, int(np.diff(s.RowOffsets).max()), 0, 10, 1e-8, rule=_lib.RULE_NATIVE).load(s)
    agg.Initialize()                                          # uploads the matrix (and builds the strength 0 hierarchy: not timed)
    matrix = (agg.cublas, agg.cusparse, agg.vectorA.Ptr, agg.vectorRowOffsets.Ptr, agg.vectorColumnIndeces.Ptr, s.nnz, s.Count)
    if not parent:
        outputs = [VectorDouble(s.nnz), VectorInt(s.Count + 1), VectorInt(s.nnz), VectorInt(s.nnz)]
        out["transpose"], count = three(lambda: L.MgcgCsrTranspose(*matrix, s.Count, *(v.Ptr for v in outputs)))
        assert count == s.nnz, count
        out["transpose"]["longest_column"] = int(np.diff(outputs[1].to_numpy(s.Count + 1)).max())
        for v in outputs:
            v.Dispose()
    out["symmetric_part"], count = three(lambda: L.MgcgSymmetricPart(*matrix, None, None, None, 0))
    out["symmetric_part"]["nonzeros"] = int(count)
    agg.strength = "symmetric"
    out["setup_strength1"], _ = three(agg.Setup)
    out["setup_strength1"]["level_rows"] = [int(L.MgLevelRows(agg.mg, l)) for l in range(agg.levels)]
    agg.Dispose()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the JSON here as well")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libMgcgGpu.so; without it only this commit's library is measured")
    ap.add_argument("--systems", nargs="*", default=list(SYSTEMS), choices=list(SYSTEMS))
    ap.add_argument("--check", action="store_true", help="fail unless this library's slowest MgcgSymmetricPart on upwind256 beats the parent's fastest")
    ap.add_argument("--leg", default=None, help="run this system in this process")
    ap.add_argument("--parent", action="store_true", help="with --leg: the library in MGCG_LIB_PATH is the parent's")
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(run_leg(a.leg, a.parent)))
        return
    result = {}
    for name in a.systems:
        result[name] = {}
        for which, path in (("this_commit", None), ("parent_commit", a.parent_lib)):
            if which == "parent_commit" and not path:
                continue
            env = dict(os.environ)
            env.pop("MGCG_LIB_PATH", None)
            if path:
                env["MGCG_LIB_PATH"] = os.path.abspath(path)
            child = subprocess.run([sys.executable, "-m", "conjugategradient_amd.tools.transpose_run", "--leg", name] + (["--parent"] if path else []),
                                   stdout=subprocess.PIPE, timeout=LIMIT_S, check=True, env=env)          # a leg that fails or hangs ends the script
            result[name][which] = json.loads(child.stdout)
            print(json.dumps({name: {which: result[name][which]}}), file=sys.stderr, flush=True)
        if "parent_commit" in result[name]:
            new, old = result[name]["this_commit"], result[name]["parent_commit"]
            result[name]["parent_over_this"] = {key: old[key]["median_s"] / new[key]["median_s"] for key in ("symmetric_part", "setup_strength1")}
            result[name]["slowest_of_this_below_fastest_of_parent"] = new["symmetric_part"]["slowest_s"] < old["symmetric_part"]["fastest_s"]
    text = json.dumps(result, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if a.check and not result.get("upwind256", {}).get("slowest_of_this_below_fastest_of_parent", False):
        sys.exit("the slowest MgcgSymmetricPart of this library on upwind256 does not beat the parent's fastest")


if __name__ == "__main__":
    main()
