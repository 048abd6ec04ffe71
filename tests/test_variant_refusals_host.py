"""Every refusal that the one-column variant solvers make on one rank before a device is asked for (no GPU needed), compared as WHOLE
messages with tests/golden/variant_refusals.json.  The substring assertions of tests/test_*_host.py say what a message must mention; this
file pins the text, so that a change of the shared entry path or of a message helper in csrc/solver.hip cannot alter one unnoticed.

The golden file is a recorded result: ``python -m tests.test_variant_refusals_host --record`` adds what the library in use (MGCG_LIB_PATH)
says for the cases the file does not hold yet and keeps every entry it holds.  Each entry was recorded from the commit before its export's
entry path was reshaped -- the older variants before they moved onto one entry path, SolveBicgstabMg and the work-vector forms before
theirs were folded -- and must not be recorded again to make a failing case pass."""
import ctypes as C
import json
import os
import sys

import pytest

from conjugategradient_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "variant_refusals.json")


class _VectorHead(C.Structure):
    """The head of the library's vector handle (csrc/common.hpp: data, size, device); the argument checks read the size only."""
    _fields_ = [("data", C.c_void_p), ("size", C.c_longlong), ("device", C.c_int), ("rest", C.c_char * 256)]


_handle = C.create_string_buffer(4096)                     # stands for every handle: a refused call looks at none (a zeroed MgcgMg: 0 ranks)
H = C.addressof(_handle)
_big, _small, _tiny = _VectorHead(None, 10, -1, b""), _VectorHead(None, 9, -1, b""), _VectorHead(None, 3, -1, b"")
VEC, SHORT, TINY = C.addressof(_big), C.addressof(_small), C.addressof(_tiny)
_sized = {n: _VectorHead(None, n, -1, b"") for n in (1000, 39, 49, 89, 99, -1)}     # work vectors: roomy, one entry short of each form, and short of nothing
ROOMY, WORK = C.addressof(_sized[1000]), {n: C.addressof(v) for n, v in _sized.items()}
IT, RES, TRUE, UP = C.c_int(0), C.c_double(0.0), C.c_double(0.0), C.c_int(0)
OUT2, OUT3 = (C.byref(IT), C.byref(RES)), (C.byref(IT), C.byref(RES), C.byref(TRUE))
EIGHT = (VEC,) * 8                                         # elements, rowOffsets, columnIndeces, x, b, Ap, p, r
ONE, RANKS = (28, 10), (10, 10, 0, 28, 0, 9)               # (elementsCount, count) ; (count, countForDevice, offset, elementsCount, minJ, maxJ)
STOP = (1e-8, 0, 10)
RULES = (("max_norm", _lib.RULE_HANDMADECL), ("rule_minus_1", -1), ("rule_5", 5))
SHIFTS = (C.c_double * 9)(*([1.0] * 9))
NOT_FINITE = (("shift_nan", float("nan")), ("shift_inf", float("inf")), ("shift_minus_inf", -float("inf")))


def _exports(L):
    """name -> (keyword defaults, call(**keywords)); the ...Parallel forms are called without a communicator: one rank."""
    def sreduce(par):
        def call(blas=H, sparse=H, s=VEC, dinv=None, rule=_lib.RULE_CSHARP):
            head = (None, blas, sparse, None) if par else (blas, sparse, None)
            fn = L.SolveSingleReduceParallel if par else L.SolveSingleReduce
            return fn(*head, *EIGHT, s, dinv, *(RANKS if par else ONE), *STOP, rule, *OUT2, None, 0)
        return call

    def minres(par):
        def call(blas=H, sparse=H, r=VEC, w1=VEC, w2=VEC, rule=_lib.RULE_CSHARP, shift=0.5):
            head = (None, blas, sparse, None) if par else (blas, sparse, None)
            fn = L.SolveMinresParallel if par else L.SolveMinres
            return fn(*head, *EIGHT[:7], r, w1, w2, *(RANKS if par else ONE), shift, *STOP, rule, *OUT3, None, 0)
        return call

    def bicgstab(par, jacobi):
        def call(blas=H, sparse=H, v=VEC, s=VEC, t=VEC, rhat=VEC, dinv=VEC, rule=_lib.RULE_CSHARP):
            head = (None, blas, sparse, None) if par else (blas, sparse, None)
            fn = getattr(L, "SolveBicgstab" + ("Jacobi" if jacobi else "") + ("Parallel" if par else ""))
            return fn(*head, *EIGHT, v, s, t, rhat, *((dinv,) if jacobi else ()), *(RANKS if par else ONE), *STOP, rule, *OUT3, None, 0)
        return call

    def pminres(par):
        def call(blas=H, sparse=H, r1=VEC, w1=VEC, w2=VEC, dinv=VEC, rule=_lib.RULE_CSHARP, shift=0.5):
            head = (None, blas, sparse, None) if par else (blas, sparse, None)
            fn = L.SolveMinresJacobiParallel if par else L.SolveMinresJacobi
            return fn(*head, *EIGHT, r1, w1, w2, dinv, *(RANKS if par else ONE), shift, *STOP, rule, *OUT3, None, 0)
        return call

    def pminres_mg(blas=H, sparse=H, mg=H, r1=VEC, w1=VEC, w2=VEC, z=VEC, rule=_lib.RULE_CSHARP, shift=0.5):
        return L.SolveMinresMg(blas, sparse, None, mg, *EIGHT, r1, w1, w2, z, *ONE, shift, *STOP, rule, *OUT3, None, 0)

    def chebyshev(par):
        def call(blas=H, sparse=H, dinv=None, z=VEC, z2=VEC, d=VEC, degree=4, lmin=0.4, lmax=12.0, rule=_lib.RULE_CSHARP):
            head = (None, blas, sparse, None) if par else (blas, sparse, None)
            fn = L.SolveChebyshevParallel if par else L.SolveChebyshev
            return fn(*head, *EIGHT, dinv, z, z2, d, *(RANKS if par else ONE), degree, lmin, lmax, *STOP, rule, *OUT2, None, 0)
        return call

    def mixed(blas=H, sparse=H, e32=VEC, nnz=14, count=10, rule=_lib.RULE_CSHARP):
        return L.SolveMixed(blas, sparse, None, *EIGHT, e32, nnz, count, *STOP, rule, *OUT2, C.byref(UP), None, 0)

    def shifted(blas=H, work=VEC, k=2, rule=_lib.RULE_CSHARP):
        return L.SolveShifted(blas, H, None, *EIGHT, work, *ONE, k, SHIFTS, *STOP, rule, None, None, None, None, 0)

    def bkrylov(blas=H, k=2, rule=_lib.RULE_CSHARP):
        return L.SolveBlockKrylov(blas, H, None, *EIGHT, *ONE, k, *STOP, rule, None, None, None, None, 0)

    def bicgstab_mg(blas=H, sparse=H, mg=H, v=VEC, s=VEC, t=VEC, rhat=VEC, count=10, rule=_lib.RULE_CSHARP):
        return L.SolveBicgstabMg(blas, sparse, None, mg, *EIGHT, v, s, t, rhat, 28, count, *STOP, rule, *OUT3, None, 0)

    def work_vector(name, jacobi):
        """SolveBicgstabL* (ell) and SolveGmres* (m, orth): one work vector, with `jacobi` the diagonal behind it"""
        def call(blas=H, sparse=H, work=ROOMY, dinv=VEC, ell=2, m=8, orth=2, count=10, rule=_lib.RULE_CSHARP):
            sizes = (ell,) if "Bicgstab" in name else (m, orth)
            return getattr(L, name)(blas, sparse, None, *EIGHT, work, *((dinv,) if jacobi else ()), *sizes, 28, count, *STOP, rule, *OUT3, None, 0)
        return call

    return {
        "SolveBicgstabMg": bicgstab_mg,
        "SolveBicgstabL": work_vector("SolveBicgstabL", False), "SolveBicgstabLJacobi": work_vector("SolveBicgstabLJacobi", True),
        "SolveGmres": work_vector("SolveGmres", False), "SolveGmresJacobi": work_vector("SolveGmresJacobi", True),
        "SolveShifted": shifted, "SolveBlockKrylov": bkrylov,
        "SolveSingleReduce": sreduce(False), "SolveSingleReduceParallel": sreduce(True),
        "SolveMinres": minres(False), "SolveMinresParallel": minres(True),
        "SolveBicgstab": bicgstab(False, False), "SolveBicgstabParallel": bicgstab(True, False),
        "SolveBicgstabJacobi": bicgstab(False, True), "SolveBicgstabJacobiParallel": bicgstab(True, True),
        "SolveMinresJacobi": pminres(False), "SolveMinresJacobiParallel": pminres(True), "SolveMinresMg": pminres_mg,
        "SolveChebyshev": chebyshev(False), "SolveChebyshevParallel": chebyshev(True),
        "SolveMixed": mixed,
    }


def _nulls(*names):
    return [("null_" + n, {n: None}) for n in names]


def _shorts(*names):
    return [("short_" + n, {n: SHORT}) for n in names]


def _rules():
    return [(label, dict(rule=rule)) for label, rule in RULES]


def _shifts():
    return [(label, dict(shift=v)) for label, v in NOT_FINITE]


# export -> [(label, keywords)]: each null handle, each bad rule, the shift, degree and bounds, each too-short vector; then pairs that
# show which refusal comes first
_SREDUCE = _nulls("blas", "sparse", "s") + _rules() + _shorts("s", "dinv") + [("max_norm_before_short_s", dict(rule=_lib.RULE_HANDMADECL, s=SHORT)),
                                                                             ("null_before_rule", dict(s=None, rule=5))]
_MINRES = (_nulls("blas", "sparse", "w1", "w2") + _shifts() + _rules() + _shorts("w1", "w2", "r")
           + [("shift_before_rule", dict(shift=float("nan"), rule=5)), ("w1_before_w2_before_r", dict(w1=SHORT, w2=TINY, r=TINY)), ("null_before_shift", dict(w2=None, shift=float("nan")))])
_BICGSTAB = (_nulls("blas", "sparse", "v", "s", "t", "rhat") + _rules() + _shorts("v", "t", "rhat", "s")
             + [("v_before_t_before_rhat_before_s", dict(v=SHORT, t=TINY, rhat=TINY, s=TINY)), ("rule_before_short_v", dict(rule=-1, v=SHORT))])
_BICGSTAB_JACOBI = _BICGSTAB + _nulls("dinv") + _shorts("dinv") + [("s_before_dinv", dict(s=SHORT, dinv=TINY))]
_PMINRES = (_nulls("blas", "sparse", "r1", "w1", "w2") + _shifts() + _rules() + _shorts("r1", "w1", "w2")
            + [("shift_before_rule", dict(shift=float("inf"), rule=-1)), ("r1_before_w1_before_w2", dict(r1=SHORT, w1=TINY, w2=TINY))])
_PMINRES_JACOBI = _PMINRES + _nulls("dinv") + _shorts("dinv") + [("w2_before_dinv", dict(w2=SHORT, dinv=TINY))]
_PMINRES_MG = _PMINRES + _nulls("mg", "z") + _shorts("z") + [("w2_before_z", dict(w2=SHORT, z=TINY)), ("hierarchy_of_no_ranks", dict())]
_CHEBYSHEV = (_nulls("blas", "sparse", "z", "z2", "d") + [("degree_0", dict(degree=0)), ("degree_17", dict(degree=17)), ("lmin_0", dict(lmin=0.0)),
                                                         ("lmin_above_lmax", dict(lmin=13.0)), ("lmax_inf", dict(lmax=float("inf"))), ("lmin_nan", dict(lmin=float("nan")))]
              + _rules() + _shorts("z", "z2", "d", "dinv")
              + [("degree_before_bounds_before_rule", dict(degree=0, lmin=0.0, rule=5)), ("z_before_z2_before_d_before_dinv", dict(z=SHORT, z2=TINY, d=TINY, dinv=TINY))])
_MIXED = (_nulls("blas", "sparse", "e32") + _rules() + [("no_rows", dict(count=0)), ("negative_nnz", dict(nnz=-1)), ("short_e32", dict(nnz=28, e32=SHORT)),
                                                        ("rule_before_no_rows", dict(rule=5, count=0))])
# the exports of the older variants that refuse through cg_variant_args before they ask for a device (SolveBlockEx asks for it first)
_SHIFTED = _nulls("blas", "work") + _rules()[1:] + [("k_0", dict(k=0)), ("k_9", dict(k=9)), ("k_before_rule", dict(k=0, rule=5))]
_BKRYLOV = _nulls("blas") + _rules() + [("k_0", dict(k=0)), ("k_9", dict(k=9)), ("k_before_rule", dict(k=0, rule=5))]
# the V-cycle form of BiCGStab: _handle is a zeroed hierarchy, so the call with every other argument in order is refused for it
_BICGSTAB_MG = _BICGSTAB + _nulls("mg") + [("hierarchy_of_no_ranks", dict()), ("count_0", dict(count=0))]


def _work_vector(sizes, first, short, jacobi):
    """The one-rank work-vector forms.  sizes: the refused ell, or m and orth; short: a work vector one entry short of this form (ell = 2:
    4 or 5 slices of 10; m = 8: 9 or 10).  No rows ask for no room, so count 0 alone is refused only with a device in hand: here
    it meets a work vector that holds less than nothing."""
    cases = (_nulls("blas", "sparse", "work") + sizes + _rules()
             + [("work_one_short", dict(work=WORK[short])), ("count_0_work_of_minus_1", dict(count=0, work=WORK[-1])),
                ("sizes_before_rule_before_work", dict(rule=5, work=WORK[short], **first))])
    if jacobi:
        cases += _nulls("dinv") + _shorts("dinv") + [("work_before_dinv", dict(work=WORK[short], dinv=TINY))]
    return cases


_ELL = [("ell_0", dict(ell=0)), ("ell_5", dict(ell=5))]
_M_ORTH = [("m_0", dict(m=0)), ("m_33", dict(m=33)), ("orth_0", dict(orth=0)), ("orth_3", dict(orth=3)), ("m_before_orth", dict(m=0, orth=0))]
CASES = {
    "SolveBicgstabMg": _BICGSTAB_MG,
    "SolveBicgstabL": _work_vector(_ELL, dict(ell=0), 39, False), "SolveBicgstabLJacobi": _work_vector(_ELL, dict(ell=0), 49, True),
    "SolveGmres": _work_vector(_M_ORTH, dict(orth=3), 89, False), "SolveGmresJacobi": _work_vector(_M_ORTH, dict(orth=3), 99, True),
    "SolveShifted": _SHIFTED, "SolveBlockKrylov": _BKRYLOV,
    "SolveSingleReduce": _SREDUCE, "SolveSingleReduceParallel": _SREDUCE,
    "SolveMinres": _MINRES, "SolveMinresParallel": _MINRES,
    "SolveBicgstab": _BICGSTAB, "SolveBicgstabParallel": _BICGSTAB,
    "SolveBicgstabJacobi": _BICGSTAB_JACOBI, "SolveBicgstabJacobiParallel": _BICGSTAB_JACOBI,
    "SolveMinresJacobi": _PMINRES_JACOBI, "SolveMinresJacobiParallel": _PMINRES_JACOBI, "SolveMinresMg": _PMINRES_MG,
    "SolveChebyshev": _CHEBYSHEV, "SolveChebyshevParallel": _CHEBYSHEV,
    "SolveMixed": _MIXED,
}
IDS = [f"{export}-{label}" for export, cases in CASES.items() for label, _ in cases]


def refusal(L, export, label):
    """[status, last_error()] of one refused call."""
    kw = dict(CASES[export])[label]
    L.MgcgClearLastError()
    st = _exports(L)[export](**kw)
    msg = _lib.last_error()
    L.MgcgClearLastError()
    return [st, msg]


def _other_exports(L):
    """The set-up exports that word a short dinv vector as the solvers do."""
    bound = C.c_double(0.0)
    out = {}
    for label, fn in (("MgcgJacobiSetup-short_dinv", lambda: L.MgcgJacobiSetup(H, VEC, VEC, VEC, 5, 9, 0, TINY)),
                      ("MgcgGershgorinBound-short_dinv", lambda: L.MgcgGershgorinBound(H, VEC, VEC, VEC, 5, 9, 0, TINY, C.byref(bound)))):
        L.MgcgClearLastError()
        st = fn()
        out[label] = [st, _lib.last_error()]
        L.MgcgClearLastError()
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_golden_file_holds_exactly_these_cases(recorded):
    assert len(set(IDS)) == len(IDS)
    assert sorted(recorded) == sorted(IDS + ["MgcgJacobiSetup-short_dinv", "MgcgGershgorinBound-short_dinv"])
    for key, (st, msg) in recorded.items():
        assert st in (_lib.ERROR, -1) and msg and "no HIP device" not in msg, key


@pytest.mark.parametrize("case", IDS)
def test_the_whole_message_of_a_refusal_is_unchanged(hiplib, recorded, case):
    export, label = case.split("-", 1)
    assert refusal(hiplib, export, label) == recorded[case]


def test_the_set_up_exports_word_a_short_dinv_vector_the_same_way(hiplib, recorded):
    for key, got in _other_exports(hiplib).items():
        assert got == recorded[key], key


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    lib = _lib.lib()
    with open(GOLDEN) as fh:
        table = json.load(fh)
    kept = len(table)
    fresh = {case: refusal(lib, *case.split("-", 1)) for case in IDS}
    fresh.update(_other_exports(lib))
    table.update({key: value for key, value in fresh.items() if key not in table})
    with open(GOLDEN, "w") as fh:
        json.dump(table, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(f"{len(table) - kept} refusals recorded in {GOLDEN}, {kept} kept as they were")
