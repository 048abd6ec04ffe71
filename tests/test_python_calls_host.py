"""What every one-column solver class of the Python layer hands to its native export and what it makes of the answer, compared with
tests/golden/python_calls.json (no GPU and no library needed: ``_lib._LIB`` is a fake that records).

A case is one method call on one object.  The fake answers every export; a ``Solve*`` export writes iteration 5, residual 0.25, a third
output of 0.5 (double) or 7 (int) and the trace 1, 1/2, 1/4, ... up to the capacity it was given, then returns the case's scripted status.
Recorded per case: the export, its whole argument tuple in normal form (a vector as the attribute that holds it and its size, a cell
as its type and starting value, the trace pointer as present or absent, numbers as they are), every library call between the method's
entry and its exit, the object's result attributes afterwards (the trace as its length) and the exception's type and whole message.  The file holds the record of
each config's ``plain-ok`` case whole and, for the config's other cases, what differs from it (``_difference`` / ``_whole``).

The golden file is a recorded result: ``python -m tests.test_python_calls_host --record`` writes it.  It was recorded ONCE, from the
package as it stood before the solver classes were moved onto one native-call path (``ConjugateGradientGpu._native_solve``), so that the
move could not change an argument, a default, an attribute or a message unnoticed -- the quirks that DESIGN.md lists as deliberate
included.  It is never recorded again to make a failing case pass; a new solver class adds cases, it does not rewrite old ones.
"""
import ctypes as C
import json
import math
import os
import re
import sys

import numpy as np
import pytest

from conjugategradient_amd import _lib, problems
from conjugategradient_amd.amg import ConjugateGradientAmgGpu
from conjugategradient_amd.bicgstab import (BiConjugateGradientStabGpu, BiConjugateGradientStabJacobiGpu, BiConjugateGradientStabLGpu,
                                            BiConjugateGradientStabLJacobiGpu)
from conjugategradient_amd.chebyshev import ConjugateGradientChebyshevGpu
from conjugategradient_amd.gmres import GeneralizedMinimalResidualGpu, GeneralizedMinimalResidualJacobiGpu
from conjugategradient_amd.jacobi import ConjugateGradientJacobiGpu
from conjugategradient_amd.minres import MinimalResidualGpu, MinimalResidualJacobiGpu
from conjugategradient_amd.mixed import ConjugateGradientMixedGpu
from conjugategradient_amd.multigrid import ConjugateGradientMgGpu
from conjugategradient_amd.parallel import ConjugateGradientMgRankGpu, ConjugateGradientRankGpu
from conjugategradient_amd.singlereduce import ConjugateGradientSingleReduceGpu
from conjugategradient_amd.solver import ConjugateGradientSingleGpu, VectorDouble, VectorInt
from conjugategradient_amd.ssor import ConjugateGradientSsorGpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "python_calls.json")
_BYREF = type(C.byref(C.c_int(0)))
_HANDLE0 = 0x40000000                                       # handles are far from every size and count of a case
STATUSES = {"ok": (_lib.OK, ""), "maxit": (_lib.MAXIT_EXCEEDED, "scripted: did not converge"), "nonfinite": (_lib.NONFINITE, ""),
            "error_said": (_lib.ERROR, "scripted: the library says why"), "error_silent": (_lib.ERROR, "")}


def _number(v):
    return ("nan" if math.isnan(v) else "inf" if v > 0 else "-inf") if isinstance(v, float) and not math.isfinite(v) else v


class FakeLibrary:
    """Stands where ``_lib._LIB`` does.  Every attribute is an export that records its call while ``recording`` is on."""

    def __init__(self, status="ok", jacobi_fails=False):
        self.status, self.message = STATUSES[status]
        self.jacobi_fails = jacobi_fails
        self.error = b""
        self.handles = {}                                   # handle -> "double[size]" / "int[size]" / the export that made it
        self.recording = False
        self.calls, self.solves = [], []

    def _new(self, label):
        h = _HANDLE0 + 16 * (len(self.handles) + 1)
        self.handles[h] = label
        return h

    def _plain(self, a):
        """An argument of any call but a solve: what it is, not where it lives."""
        if isinstance(a, (int, np.integer)) and int(a) in self.handles:
            return "<" + self.handles[int(a)] + ">"
        if isinstance(a, _BYREF):
            return "<cell>"
        if isinstance(a, (C.c_void_p, C.Array)):
            return "<pointer>"
        if isinstance(a, bytes):
            return a.decode()
        return _number(a)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def export(*args):
            if self.recording:
                solve = name == "Solve" or re.match(r"Solve[A-Z]", name)
                self.calls.append(name if solve or not args else f"{name}({', '.join(str(self._plain(a)) for a in args)})")
            return self._answer(name, args)
        return export

    def _answer(self, name, args):
        if name == "MgcgGetLastError":
            return self.error
        if name == "MgcgClearLastError":
            self.error = b""
            return None
        if name in ("GetDeviceCount", "MgcgAbiVersion"):
            return 1
        if name == "MgcgCommSize":
            return 2
        if name in ("MgcgCreateDouble64", "MgcgCreateInt64"):
            return self._new(("double" if "Double" in name else "int") + f"[{args[0]}]")
        if name in ("CreateBlas", "CreateSparse", "CreateMatDescr") or name.startswith("MgSetup"):
            return self._new(name)
        if name == "MgLevels":
            return 2
        if name == "Initialize":                            # the rank's column range, through its two cells
            args[11]._obj.value, args[12]._obj.value = 2, 13
        if name == "MgcgGershgorinBound":
            args[-1]._obj.value = 8.0
        if name == "MgcgJacobiSetup" and self.jacobi_fails:
            self.error = b"scripted: row 3 has no usable diagonal"
            return -1
        if name == "Solve" or re.match(r"Solve[A-Z]", name):
            return self._solve(name, args)
        return 0

    def _solve(self, name, args):
        """Keep the arguments as they came (cells by their starting value), then answer through them as the library would."""
        kept = []
        for a in args:
            if isinstance(a, _BYREF):
                kept.append(f"{type(a._obj).__name__}({_number(a._obj.value)})")
            elif isinstance(a, C.c_void_p):
                kept.append("<pointer>")
            else:
                kept.append(a)
        self.solves.append((name, kept))
        cells = [a._obj for a in args if isinstance(a, _BYREF)]
        doubles = iter((0.25, 0.5))
        ints = iter((5, 7))
        for c in cells:
            c.value = next(ints) if isinstance(c, C.c_int) else next(doubles)
        if name != "Solve":                                 # (the reference's own export takes no trace)
            pointer, cap = args[-2], args[-1]
            if pointer is not None:
                out = C.cast(pointer, C.POINTER(C.c_double))
                for i in range(cap):
                    out[i] = 0.5 ** i
        self.error = self.message.encode()
        return self.status


# --------------------------------------------------------------------------- the cases
ONE = problems.poisson(3, 3, 1)                             # 9 rows: an odd count, which the one-work-vector forms round up
SLAB = problems.poisson(2, 2, 4)                            # 16 rows in planes of 4: two ranks of two planes
STOP = (0, 10, 1e-8)


def _one(cls, **kw):
    def make(rule="default"):
        obj = cls(ONE.Count, 7, *STOP, **kw, **({} if rule == "default" else dict(rule=rule))).load(ONE)
        obj.Initialize()
        return obj
    return make


def _mg(cls, **kw):
    def make(rule="default"):
        args = (ONE.grid,) if cls is ConjugateGradientMgGpu else ()
        obj = cls(ONE.Count, 7, *STOP, *args, **kw, **({} if rule == "default" else dict(rule=rule))).load(ONE)
        obj.Initialize()
        return obj
    return make


def _rank(setup_jacobi=False, cls=ConjugateGradientRankGpu):
    def make(rule="default"):
        kw = {} if rule == "default" else dict(rule=rule)
        args = (SLAB.grid,) if cls is ConjugateGradientMgRankGpu else ()
        obj = cls(SLAB.Count, 7, *STOP, *args, rank=0, world=2, comm=_lib.lib()._new("comm"), **kw).load(SLAB)
        obj.Initialize()
        if cls is ConjugateGradientMgRankGpu:
            obj.Setup()
        if setup_jacobi:
            try:
                obj.SetupJacobi()
            except _lib.MgcgError:
                assert _lib.lib().jacobi_fails
        return obj
    return make


class _Other:
    """``hierarchy=``: the multigrid object whose hierarchy a call borrows."""


# name -> (make(rule), method, keywords, has traceCapacity, what runs on the object before the recorded call)
CONFIGS = {}


def _config(name, make, method="Solve", kw=None, capacity=False, before=()):
    assert name not in CONFIGS
    CONFIGS[name] = (make, method, kw or {}, capacity, before)


_config("single", _one(ConjugateGradientSingleGpu))
_config("jacobi", _one(ConjugateGradientJacobiGpu))
_config("mixed", _one(ConjugateGradientMixedGpu))
_config("sreduce", _one(ConjugateGradientSingleReduceGpu), capacity=True)
_config("sreduce_jacobi", _one(ConjugateGradientSingleReduceGpu, jacobi=True), capacity=True)
_config("chebyshev", _one(ConjugateGradientChebyshevGpu), capacity=True)
_config("chebyshev_jacobi_degree_bounds", _one(ConjugateGradientChebyshevGpu, jacobi=True, degree=6, bounds=(0.5, 9.0)), capacity=True)
_config("minres", _one(MinimalResidualGpu), capacity=True)
_config("minres_shift", _one(MinimalResidualGpu, shift=-1.5), capacity=True)
_config("minres_jacobi", _one(MinimalResidualJacobiGpu, shift=0.75), capacity=True)
_config("bicgstab", _one(BiConjugateGradientStabGpu), capacity=True)
_config("bicgstab_jacobi", _one(BiConjugateGradientStabJacobiGpu), capacity=True)
_config("bicgstabl", _one(BiConjugateGradientStabLGpu), capacity=True)
_config("bicgstabl_ell_raised", _one(BiConjugateGradientStabLGpu, ell=1), capacity=True, before=(("set", "ell", 4),))
_config("bicgstabl_ell_refused", _one(BiConjugateGradientStabLGpu, ell=1), capacity=True, before=(("set", "ell", 9),))
_config("bicgstabl_jacobi", _one(BiConjugateGradientStabLJacobiGpu, ell=3), capacity=True)
_config("gmres", _one(GeneralizedMinimalResidualGpu), capacity=True)
_config("gmres_m_orth", _one(GeneralizedMinimalResidualGpu, m=5, orth=1), capacity=True)
_config("gmres_m_raised", _one(GeneralizedMinimalResidualGpu, m=2), capacity=True, before=(("set", "m", 40),))
_config("gmres_jacobi", _one(GeneralizedMinimalResidualJacobiGpu, m=3), capacity=True)
for _name, _make in (("mg", _mg(ConjugateGradientMgGpu)), ("amg", _mg(ConjugateGradientAmgGpu)), ("ssor", _mg(ConjugateGradientSsorGpu))):
    _config(_name, _make)
    _config(_name + "_gmres_hierarchy_m_orth", _make, "SolveGmres", dict(hierarchy=_Other, m=4, orth=1))
    if _name == "mg":                                   # (the subclasses inherit the methods: they are pinned once, with every flag)
        _config(_name + "_minres", _make, "SolveMinres")
        _config(_name + "_bicgstab", _make, "SolveBicgstab")
        _config(_name + "_gmres", _make, "SolveGmres")
        _config(_name + "_minres_shift", _make, "SolveMinres", dict(shift=2.5))
        _config(_name + "_bicgstab_hierarchy", _make, "SolveBicgstab", dict(hierarchy=_Other))
        _config(_name + "_gmres_m_raised", _make, "SolveGmres", dict(m=40), before=(("call", "SolveGmres", dict(m=2)),))
        _config(_name + "_gmres_after_all", _make, "SolveGmres", dict(m=3),
                before=(("call", "SolveMinres", {}), ("call", "SolveBicgstab", {}), ("call", "SolveGmres", dict(m=6))))
_config("rank", _rank())
_config("rank_jacobi", _rank(True), "SolveJacobi")
_config("rank_jacobi_no_setup", _rank(), "SolveJacobi")
_config("rank_sreduce", _rank(), "SolveSingleReduce")
_config("rank_sreduce_jacobi", _rank(True), "SolveSingleReduce", dict(jacobi=True))
_config("rank_sreduce_jacobi_no_setup", _rank(), "SolveSingleReduce", dict(jacobi=True))
_config("rank_minres", _rank(), "SolveMinres")
_config("rank_minres_shift", _rank(), "SolveMinres", dict(shift=-0.5))
_config("rank_minres_again", _rank(), "SolveMinres", before=(("call", "SolveMinres", {}),))
_config("rank_minres_jacobi", _rank(True), "SolveMinresJacobi", dict(shift=0.25))
_config("rank_minres_jacobi_after_minres", _rank(True), "SolveMinresJacobi", before=(("call", "SolveMinres", {}),))
_config("rank_bicgstab", _rank(), "SolveBicgstab")
_config("rank_bicgstab_after_sreduce", _rank(), "SolveBicgstab", before=(("call", "SolveSingleReduce", {}),))     # vectorS grows
_config("rank_bicgstab_jacobi", _rank(True), "SolveBicgstab", dict(jacobi=True))
_config("rank_bicgstab_jacobi_method", _rank(True), "SolveBicgstabJacobi")
_config("rank_chebyshev", _rank(), "SolveChebyshev", dict(bounds=(0.5, 9.0)))
_config("rank_chebyshev_no_bounds", _rank(), "SolveChebyshev")
_config("rank_chebyshev_jacobi_degree", _rank(True), "SolveChebyshev", dict(jacobi=True, degree=7, bounds=(0.25, 2.0)))
_config("rank_chebyshev_jacobi_no_setup", _rank(), "SolveChebyshev", dict(jacobi=True, bounds=(0.25, 2.0)))
_config("rank_mg", _rank(cls=ConjugateGradientMgRankGpu))
# a rank whose SetupJacobi() failed: three methods still enter the native call with no dinv vector, two refuse
FAILED_SETUP = {"rank_jacobi": {}, "rank_minres_jacobi": {}, "rank_bicgstab_jacobi": {}, "rank_sreduce_jacobi": {}, "rank_chebyshev_jacobi_degree": {}}


# one config for each Solve body that the package had before they were folded (bicgstab.py's: one for each of its six exports)
COPIES = ("single", "jacobi", "mixed", "sreduce", "chebyshev", "minres", "minres_jacobi", "bicgstab", "bicgstab_jacobi", "bicgstabl",
          "bicgstabl_jacobi", "gmres", "gmres_jacobi", "mg", "mg_minres", "mg_bicgstab", "mg_gmres", "rank", "rank_jacobi", "rank_sreduce",
          "rank_minres", "rank_minres_jacobi", "rank_bicgstab", "rank_bicgstab_jacobi", "rank_chebyshev", "rank_mg")


def _cases():
    """id -> (config, rule, trace keywords, status, SetupJacobi() fails).  Every config with the trace off (status OK: the config's base
    record) and on (past MaxIteration).  Each of COPIES also under every status with the trace on, past MaxIteration with it off, with
    another rule and with none, and with the capacities 0 and 3 where the method takes one.  Then the failed set-up."""
    out = {}
    for name, (_, _, _, capacity, _) in CONFIGS.items():
        out[f"{name}-plain-ok"] = (name, "default", {}, "ok", False)
        out[f"{name}-trace-maxit"] = (name, "default", dict(trace=True), "maxit", False)
        if name not in COPIES:
            continue
        for status in STATUSES:
            out[f"{name}-trace-{status}"] = (name, "default", dict(trace=True), status, False)
        out[f"{name}-plain-maxit"] = (name, "default", {}, "maxit", False)
        out[f"{name}-rule_simple-ok"] = (name, _lib.RULE_SIMPLE, {}, "ok", False)
        out[f"{name}-rule_none_trace-ok"] = (name, None, dict(trace=True), "ok", False)
        if capacity:
            out[f"{name}-trace_capacity_0-ok"] = (name, "default", dict(trace=True, traceCapacity=0), "ok", False)
            out[f"{name}-trace_capacity_3-maxit"] = (name, "default", dict(trace=True, traceCapacity=3), "maxit", False)
            out[f"{name}-capacity_3_without_trace-ok"] = (name, "default", dict(traceCapacity=3), "ok", False)
    for name in FAILED_SETUP:
        for status in ("ok", "error_said"):
            out[f"{name}-failed_setup-{status}"] = (name, "default", {}, status, True)
    return out


CASES = _cases()


def _named(obj, other, fake, args):
    """The argument tuple with every handle named by the attribute that holds it."""
    names = {}
    for owner, prefix in ((other, "hierarchy."), (obj, "")):
        for key, value in (vars(owner).items() if owner is not None else ()):
            if isinstance(value, (VectorDouble, VectorInt)) and value.Ptr:
                names[value.Ptr] = f"{prefix}{key}[{value.size}]"
            elif isinstance(value, int) and not isinstance(value, bool) and value in fake.handles:
                names[value] = prefix + key
    return [names.get(a, "<" + fake.handles[a] + ">") if isinstance(a, int) and a in fake.handles else _number(a) for a in args]


def _dispose(obj):
    """Every vector of a case's object is deleted while the fake is still the library: a disposed object's finaliser calls nothing."""
    if obj is None:
        return
    try:
        obj.Dispose()
    finally:
        for value in vars(obj).values():
            if isinstance(value, (VectorDouble, VectorInt)):
                value.Dispose()


def run_case(case, patch):
    """One case against a fresh fake; ``patch(fake)`` puts it where ``_lib.lib()`` finds it."""
    name, rule, trace_kw, status, jacobi_fails = CASES[case]
    make, method, kw, _, before = CONFIGS[name]
    fake = FakeLibrary("ok", jacobi_fails)
    patch(fake)
    obj = other = None
    try:
        obj = make(rule)
        kw = dict(kw)
        if kw.get("hierarchy") is _Other:
            other = kw["hierarchy"] = make(rule)
        for step in before:
            if step[0] == "set":
                setattr(obj, step[1], step[2])
            else:
                getattr(obj, step[1])(**step[2])
        fake.status, fake.message = STATUSES[status]
        fake.solves.clear()
        fake.recording = True
        raised = None
        try:
            getattr(obj, method)(**kw, **trace_kw)
        except Exception as e:
            raised = [type(e).__name__, str(e)]
        fake.recording = False
        export, args = fake.solves[-1] if fake.solves else (None, [])
        assert len(fake.solves) <= 1
        after = {key: _number(getattr(obj, key, "<absent>")) for key in ("Iteration", "Residual", "TrueResidual", "ReliableUpdates", "status")}
        assert obj.trace is None or [float(v) for v in obj.trace] == [0.5 ** i for i in range(len(obj.trace))]
        after["trace"] = None if obj.trace is None else len(obj.trace)          # (the fake's 1, 1/2, 1/4, ...: its length says it all)
        return {"export": export, "args": _named(obj, other, fake, args), "calls": fake.calls, "after": after, "raised": raised}
    finally:
        fake.recording = False
        _dispose(obj)
        _dispose(other)


# --------------------------------------------------------------------------- the golden file: a base record per config, then differences
def _base(case):
    return case.split("-")[0] + "-plain-ok"


def _difference(base, record):
    """What ``record`` has that ``base`` has not: arguments by position, attributes by name, the library calls as the length of the
    common start and what follows it; ``export`` and ``raised`` whole."""
    out = {key: record[key] for key in ("export", "raised") if record[key] != base[key]}
    if len(record["args"]) != len(base["args"]):
        out["args"] = record["args"]
    elif record["args"] != base["args"]:
        out["args"] = {str(i): a for i, (a, b) in enumerate(zip(record["args"], base["args"])) if a != b}
    if record["calls"] != base["calls"]:
        same = next((i for i, (a, b) in enumerate(zip(record["calls"], base["calls"])) if a != b), min(len(record["calls"]), len(base["calls"])))
        out["calls"] = [same, record["calls"][same:]]
    after = {key: value for key, value in record["after"].items() if value != base["after"][key]}
    if after:
        out["after"] = after
    return out


def _whole(base, difference):
    """The record that ``_difference(base, record)`` was taken from."""
    args = difference.get("args", base["args"])
    if isinstance(args, dict):
        args = [args.get(str(i), a) for i, a in enumerate(base["args"])]
    calls = base["calls"][: difference["calls"][0]] + difference["calls"][1] if "calls" in difference else base["calls"]
    return {"export": difference.get("export", base["export"]), "args": args, "calls": calls,
            "after": dict(base["after"], **difference.get("after", {})), "raised": difference.get("raised", base["raised"])}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as fh:
        table = json.load(fh)
    return {case: entry if case == _base(case) else _whole(table[_base(case)], entry) for case, entry in table.items()}


def test_the_golden_file_holds_exactly_these_cases(recorded):
    assert sorted(recorded) == sorted(CASES)
    assert {name + "-plain-ok" for name in CONFIGS} <= set(CASES) and set(COPIES) <= set(CONFIGS)
    exports = {entry["export"] for entry in recorded.values()}
    assert exports >= {name for name in _lib.SIGNATURES if re.match(r"Solve[A-Z]", name) and name not in ("SolveBlockEx", "SolveBlockKrylov", "SolveShifted")}


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_native_call_and_what_becomes_of_it_are_unchanged(monkeypatch, recorded, case):
    got = run_case(case, lambda fake: monkeypatch.setattr(_lib, "_LIB", fake))
    assert json.loads(json.dumps(got)) == recorded[case]


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    if os.path.exists(GOLDEN):
        sys.exit(f"{GOLDEN} exists: it is recorded once (see this file's docstring)")
    table = {case: json.loads(json.dumps(run_case(case, lambda fake: setattr(_lib, "_LIB", fake)))) for case in sorted(CASES)}
    _lib._LIB = None
    short = {case: record if case == _base(case) else _difference(table[_base(case)], record) for case, record in table.items()}
    assert all(_whole(table[_base(case)], short[case]) == table[case] for case in table if case != _base(case))
    with open(GOLDEN, "w") as fh:
        fh.write("{\n" + ",\n".join(f" {json.dumps(case)}: {json.dumps(short[case])}" for case in sorted(short)) + "\n}\n")
    print(f"{len(table)} cases recorded in {GOLDEN}")
