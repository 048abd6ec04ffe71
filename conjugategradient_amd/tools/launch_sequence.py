#!/usr/bin/env python3
"""Which kernels the CG loop launches, and how often: one fixed set of solves that takes every variant of the loop's update step
(DESIGN.md section 5), to be run under the profiler at two commits whose launch sequences are meant to be equal.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python conjugategradient_amd/tools/launch_sequence.py run
    python conjugategradient_amd/tools/launch_sequence.py table OUT > counts.json

``run``: 64^3 SolveEx with x_defer 8 and 1, CgSteps(20), a 64^3 MGCG solve and a 64^3 Jacobi-preconditioned solve, two loopback ranks
plain, MGCG and Jacobi, four loopback ranks of which three hold no rows, plain and Jacobi.  The placement draw is off (its timing loops
launch SpMVs by the free memory of the moment).
``table``: per-kernel call counts of the run's *kernel_stats.csv, as one JSON object sorted by name."""
import csv
import glob
import json
import os
import sys
import threading

os.environ["MGCG_PLACEMENT"] = "0"
os.environ["MGCG_VIRTUAL_DEVICES"] = "4"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def ranks_in_threads(world, make_rank):
    from conjugategradient_amd import _lib

    L = _lib.lib()
    group = L.MgcgLoopbackCreate(world)
    errors = []

    def body(rank):
        try:
            L.SetDevice(rank)
            comm = L.MgcgCommInitLoopback(group, rank)
            assert comm, _lib.last_error()
            make_rank(rank, comm)
            L.MgcgCommDestroy(comm)
        except BaseException as e:      # noqa: BLE001 -- reported after the join
            errors.append(e)
            raise

    threads = [threading.Thread(target=body, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=600)
    L.MgcgLoopbackDestroy(group)
    if errors:
        raise errors[0]


def run():
    from conjugategradient_amd import _lib, problems
    from conjugategradient_amd.jacobi import ConjugateGradientJacobiGpu
    from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
    from conjugategradient_amd.parallel import ConjugateGradientMgRankGpu, ConjugateGradientRankGpu
    from conjugategradient_amd.solver import ConjugateGradientSingleGpu

    L = _lib.lib()
    s = problems.poisson(64, 64, 64)
    done = []
    for defer in (8, 1):                                        # one rank, plain: the ring, then one x term per iteration
        L.MgcgSetTuning(b"x_defer", defer)
        cg = ConjugateGradientSingleGpu(s.Count, 7, 0, 5000, 1e-8, rule=_lib.RULE_NATIVE).load(s)
        cg.Initialize()
        cg.Solve()
        done.append(("SolveEx x_defer %d" % defer, cg.Iteration))
        cg.Dispose()
    L.MgcgSetTuning(b"x_defer", 8)
    st = ConjugateGradientRankGpu(s.Count, 7, 0, 5000, 1e-8).load(s)
    st.Initialize()
    st.Steps(20)                                                # fixed length: no stop test, a short first group
    done.append(("CgSteps", 20))
    st.Dispose()
    mg = ConjugateGradientMgGpu(s.Count, 7, 0, 500, 1e-8, s.grid).load(s)      # one rank, preconditioned
    mg.Initialize()
    mg.Solve()
    done.append(("MGCG", mg.Iteration))
    mg.Dispose()
    jc = ConjugateGradientJacobiGpu(s.Count, 7, 0, 5000, 1e-8, rule=_lib.RULE_NATIVE).load(s)      # one rank, z = D^-1 r inside the vector passes
    jc.Initialize()
    jc.Solve()
    done.append(("Jacobi", jc.Iteration))
    jc.Dispose()

    t = problems.poisson(32, 32, 16)
    its = {}

    def plain(rank, comm):                                      # several ranks, plain
        cg = ConjugateGradientRankGpu(t.Count, 7, 0, 500, 1e-8, rank=rank, world=2, comm=comm, device=rank).load(t)
        cg.Initialize()
        cg.Solve()
        its["plain", rank] = cg.Iteration
        cg.Dispose()

    def precond(rank, comm):                                    # several ranks, preconditioned
        cg = ConjugateGradientMgRankGpu(t.Count, 7, 0, 400, 1e-8, t.grid, rank=rank, world=2, comm=comm, device=rank).load(t)
        cg.Initialize()
        cg.Setup()
        cg.Solve()
        its["mgcg", rank] = cg.Iteration
        cg.Dispose()

    def jacobi(rank, comm):                                     # several ranks, Jacobi
        cg = ConjugateGradientRankGpu(t.Count, 7, 0, 500, 1e-8, rank=rank, world=2, comm=comm, device=rank).load(t)
        cg.Initialize()
        cg.SetupJacobi()
        cg.SolveJacobi()
        its["jacobi", rank] = cg.Iteration
        cg.Dispose()

    ranks_in_threads(2, plain)
    ranks_in_threads(2, precond)
    ranks_in_threads(2, jacobi)
    done.append(("two ranks plain", its["plain", 0]))
    done.append(("two ranks MGCG", its["mgcg", 0]))
    done.append(("two ranks Jacobi", its["jacobi", 0]))

    e = problems.mgcg_main(3, 160)                              # 3 rows over 4 ranks: three ranks without rows
    assert problems.partition_offsets(e.Count, 4) == [0, 0, 0, 0, 3]

    def empty(rank, comm):
        cg = ConjugateGradientRankGpu(e.Count, 3, 0, 50, 1e-8, rank=rank, world=4, comm=comm, device=rank).load(e)
        cg.Initialize()
        cg.Solve()
        its["empty", rank] = cg.Iteration
        cg.Dispose()

    def empty_jacobi(rank, comm):
        cg = ConjugateGradientRankGpu(e.Count, 3, 0, 50, 1e-8, rank=rank, world=4, comm=comm, device=rank).load(e)
        cg.Initialize()
        cg.SetupJacobi()
        cg.SolveJacobi()
        its["empty jacobi", rank] = cg.Iteration
        cg.Dispose()

    ranks_in_threads(4, empty)
    ranks_in_threads(4, empty_jacobi)
    done.append(("four ranks, three empty", its["empty", 3]))
    done.append(("four ranks, three empty, Jacobi", its["empty jacobi", 3]))
    print(json.dumps({"iterations": dict(done)}))


def table(out):
    counts = {}
    for f in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(f) as fh:
            for row in csv.DictReader(fh):
                counts[row["Name"]] = counts.get(row["Name"], 0) + int(row["Calls"])
    print(json.dumps(dict(sorted(counts.items())), indent=1))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "table":
        table(sys.argv[2])
    else:
        sys.exit(__doc__)
