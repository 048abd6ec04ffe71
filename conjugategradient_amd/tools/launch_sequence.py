#!/usr/bin/env python3
"""Which kernels the CG loop launches, and how often: one fixed set of solves that takes every variant of the loop's update step
(DESIGN.md section 5), to be run under the profiler at two commits whose launch sequences are meant to be equal.

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python conjugategradient_amd/tools/launch_sequence.py run
    python conjugategradient_amd/tools/launch_sequence.py table OUT > counts.json

``run``: 64^3 SolveEx with x_defer 8 and 1, CgSteps(20), a 64^3 MGCG solve and a 64^3 Jacobi-preconditioned solve, two loopback ranks
plain, MGCG and Jacobi, four loopback ranks of which three hold no rows, plain and Jacobi; then one 64^3 solve of each one-column variant
(mixed precision, single reduction, MINRES with a shift that makes the system indefinite, BiCGStab, Jacobi-preconditioned MINRES, Chebyshev
CG of degree 4, BiCGStab(2), GMRES(8) with two orthogonalisation passes), one 32^3 BiCGStab solve with an aggregation hierarchy and, on two
loopback ranks at 32 x 32 x 16, the five of them that have a several-ranks form, with and without the diagonal where both exist.  The
placement draw is off (its timing loops launch SpMVs by the free memory of the moment).
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
    variants(done)
    print(json.dumps({"iterations": dict(done)}))


SHIFT = 0.1             # above the first eigenvalues of both grids below (64^3: from 0.007; 32 x 32 x 16: 0.052, 0.079, ...): A - SHIFT I is indefinite
BOUNDS = (0.4, 12.0)    # of the 7-point matrix; with the diagonal the same interval over 6


def variants(done):
    """One solve of each one-column variant on one rank, and of each several-ranks form on two loopback ranks."""
    from conjugategradient_amd import _lib, problems
    from conjugategradient_amd.amg import ConjugateGradientAmgGpu
    from conjugategradient_amd.bicgstab import (BiConjugateGradientStabGpu, BiConjugateGradientStabJacobiGpu, BiConjugateGradientStabLGpu,
                                                BiConjugateGradientStabLJacobiGpu)
    from conjugategradient_amd.chebyshev import ConjugateGradientChebyshevGpu
    from conjugategradient_amd.gmres import GeneralizedMinimalResidualGpu, GeneralizedMinimalResidualJacobiGpu
    from conjugategradient_amd.minres import MinimalResidualGpu, MinimalResidualJacobiGpu
    from conjugategradient_amd.mixed import ConjugateGradientMixedGpu
    from conjugategradient_amd.parallel import ConjugateGradientRankGpu
    from conjugategradient_amd.singlereduce import ConjugateGradientSingleReduceGpu
    from conjugategradient_amd.solver import ApplicationException

    def counted(solve):                                         # a run that meets its iteration cap counts too
        try:
            solve()
        except ApplicationException:
            pass

    s = problems.poisson(64, 64, 64)
    args = (s.Count, 7, 0, 5000, 1e-8)
    one_rank = [
        ("mixed", lambda: ConjugateGradientMixedGpu(*args, rule=_lib.RULE_CSHARP)),
        ("single reduction", lambda: ConjugateGradientSingleReduceGpu(*args, rule=_lib.RULE_CSHARP)),
        ("single reduction Jacobi", lambda: ConjugateGradientSingleReduceGpu(*args, rule=_lib.RULE_CSHARP, jacobi=True)),
        ("MINRES indefinite", lambda: MinimalResidualGpu(*args, rule=_lib.RULE_CSHARP, shift=SHIFT)),
        ("MINRES Jacobi indefinite", lambda: MinimalResidualJacobiGpu(*args, rule=_lib.RULE_CSHARP, shift=SHIFT)),
        ("BiCGStab", lambda: BiConjugateGradientStabGpu(*args, rule=_lib.RULE_CSHARP)),
        ("BiCGStab Jacobi", lambda: BiConjugateGradientStabJacobiGpu(*args, rule=_lib.RULE_CSHARP)),
        ("Chebyshev degree 4", lambda: ConjugateGradientChebyshevGpu(*args, rule=_lib.RULE_CSHARP, degree=4, bounds=BOUNDS)),
        ("Chebyshev degree 4 Jacobi", lambda: ConjugateGradientChebyshevGpu(*args, rule=_lib.RULE_CSHARP, degree=4, jacobi=True, bounds=(BOUNDS[0] / 6, BOUNDS[1] / 6))),
        ("BiCGStab(2)", lambda: BiConjugateGradientStabLGpu(*args, rule=_lib.RULE_CSHARP, ell=2)),
        ("BiCGStab(2) Jacobi", lambda: BiConjugateGradientStabLJacobiGpu(*args, rule=_lib.RULE_CSHARP, ell=2)),
        ("GMRES(8) orth 2", lambda: GeneralizedMinimalResidualGpu(*args, rule=_lib.RULE_CSHARP, m=8, orth=2)),
        ("GMRES(8) orth 2 Jacobi", lambda: GeneralizedMinimalResidualJacobiGpu(*args, rule=_lib.RULE_CSHARP, m=8, orth=2)),
    ]
    for name, make in one_rank:
        cg = make().load(s)
        cg.Initialize()
        counted(cg.Solve)
        done.append((name, cg.Iteration))
        cg.Dispose()

    c = problems.poisson(32, 32, 32)                            # the V-cycle of an aggregation hierarchy as BiCGStab's preconditioner
    amg = ConjugateGradientAmgGpu(c.Count, 7, 0, 500, 1e-8, rule=_lib.RULE_CSHARP).load(c)
    amg.Initialize()
    counted(amg.SolveBicgstab)
    done.append(("BiCGStab aggregation 32^3", amg.Iteration))
    amg.Dispose()

    t = problems.poisson(32, 32, 16)
    two_ranks = [
        ("single reduction", False, lambda cg: cg.SolveSingleReduce()),
        ("single reduction Jacobi", True, lambda cg: cg.SolveSingleReduce(jacobi=True)),
        ("MINRES indefinite", False, lambda cg: cg.SolveMinres(shift=SHIFT)),
        ("MINRES Jacobi indefinite", True, lambda cg: cg.SolveMinresJacobi(shift=SHIFT)),
        ("BiCGStab", False, lambda cg: cg.SolveBicgstab()),
        ("BiCGStab Jacobi", True, lambda cg: cg.SolveBicgstabJacobi()),
        ("Chebyshev degree 4", False, lambda cg: cg.SolveChebyshev(degree=4, bounds=BOUNDS)),
        ("Chebyshev degree 4 Jacobi", True, lambda cg: cg.SolveChebyshev(jacobi=True, degree=4, bounds=(BOUNDS[0] / 6, BOUNDS[1] / 6))),
    ]
    for name, diagonal, solve in two_ranks:
        its = {}

        def rank_body(rank, comm):
            cg = ConjugateGradientRankGpu(t.Count, 7, 0, 2000, 1e-8, rank=rank, world=2, comm=comm, device=rank).load(t)
            cg.Initialize()
            if diagonal:
                cg.SetupJacobi()
            counted(lambda: solve(cg))
            its[rank] = cg.Iteration
            cg.Dispose()

        ranks_in_threads(2, rank_body)
        assert its[0] == its[1], (name, its)
        done.append(("two ranks " + name, its[0]))


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
