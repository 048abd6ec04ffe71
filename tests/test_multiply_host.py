"""The CSR matrix product C = A B (MgcgCsrMultiply) on the host side: the numpy yardstick of its contract, checked against hand-worked cases,
against scipy, against dense products of integer-valued matrices and against the Galerkin yardstick of the aggregation multigrid; and the
library without a device -- the exports, and every refusal that is made before a device is asked for, with its whole message and with the
outputs left alone.

The contract (include/MgcgGpu.h): row i of A in stored order gives entries p with column k_p; each contributes the stored entries q of row
k_p of B in stored order; this numbers the products of row i as t = 0, 1, 2, ...  Row i of C stores column j exactly when some product lands
on it, columns ascending, each once, zero sums kept; c_ij = the serial sum from +0.0, in ascending t, of the rounded products a_p * b_q."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conjugategradient_amd import _lib, problems
from tests.test_amg_host import box_maps, csr_of, galerkin
from tests.test_amg_sym_host import NONSYMMETRIC
from tests.test_transpose_host import transpose_arrays


def expand_products(ca, roa, cb, rob):
    """(row of C, entry p of A, entry q of B) of every product, in the contract's order: by row, and t ascending inside a row."""
    roa, rob = np.asarray(roa, dtype=np.int64), np.asarray(rob, dtype=np.int64)
    ca = np.asarray(ca, dtype=np.int64)[: int(roa[-1])]
    length = np.diff(rob)[ca]                                  # the products of entry p
    total = int(length.sum())
    first = np.cumsum(length) - length
    p = np.repeat(np.arange(len(ca), dtype=np.int64), length)
    q = np.repeat(rob[ca] - first, length) + np.arange(total, dtype=np.int64)
    i = np.repeat(np.arange(len(roa) - 1, dtype=np.int64), np.diff(roa))[p]
    return i, p, q


def products_per_row(ca, roa, rob):
    """u_i: the products of every row of C"""
    roa, rob = np.asarray(roa, dtype=np.int64), np.asarray(rob, dtype=np.int64)
    length = np.r_[0, np.cumsum(np.diff(rob)[np.asarray(ca, dtype=np.int64)[: int(roa[-1])]])]
    return length[roa[1:]] - length[roa[:-1]]


def multiply_arrays(ea, ca, roa, eb, cb, rob, columns):
    """(elements, columns, offsets) of C = A B by the contract; ea and eb may both be None (pattern only: None comes back).  Entries beyond
    roa[-1] / rob[-1] are ignored."""
    rows = len(roa) - 1
    i, p, q = expand_products(ca, roa, cb, rob)
    j = np.asarray(cb, dtype=np.int64)[q]
    assert j.size == 0 or (j.min() >= 0 and j.max() < columns)
    order = np.lexsort((j, i))                                 # stable: t ascends inside one (i, j)
    i, j = i[order], j[order]
    head = np.r_[True, (i[1:] != i[:-1]) | (j[1:] != j[:-1])] if len(i) else np.zeros(0, dtype=bool)
    offsets = np.r_[0, np.cumsum(np.bincount(i[head], minlength=rows))].astype(np.int32)
    cols = j[head].astype(np.int32)
    if ea is None:
        assert eb is None
        return None, cols, offsets
    starts = np.nonzero(head)[0]
    run = np.cumsum(head) - 1
    rank = np.arange(len(i)) - starts[run] if len(i) else np.zeros(0, dtype=np.int64)
    by_rank = np.argsort(rank, kind="stable")
    bounds = np.r_[0, np.cumsum(np.bincount(rank))] if len(i) else [0]
    acc = np.zeros(len(starts))                                # +0.0
    with np.errstate(invalid="ignore", over="ignore"):         # (inf * 0 and inf - inf are NaN by the contract, not an error)
        prod = (np.asarray(ea, dtype=np.float64)[p] * np.asarray(eb, dtype=np.float64)[q])[order]    # every product rounded on its own
        for r in range(len(bounds) - 1):                       # the serial sums: one addition of every run that is long enough, per trip
            m = by_rank[bounds[r]:bounds[r + 1]]
            acc[run[m]] = acc[run[m]] + prod[m]
    return acc, cols, offsets


def _csr(rows, columns):
    """rows: a list of [(column, value), ...] in stored order"""
    ro = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    c = np.array([j for r in rows for j, _ in r], dtype=np.int32)
    e = np.array([v for r in rows for _, v in r], dtype=np.float64)
    return e, c, ro, columns


#      A (3 x 4), row 0 unsorted with column 1 twice      B (4 x 2), row 1 unsorted with column 1 twice
HAND_A = [[(1, 2.0), (3, 1.0), (1, 3.0)], [], [(0, 4.0), (2, -1.0)]]
HAND_B = [[(1, 5.0)], [(1, 1.0), (0, 2.0), (1, 0.5)], [(0, 7.0)], [(0, 10.0)]]


def hand_worked():
    ea, ca, roa, _ = _csr(HAND_A, 4)
    eb, cb, rob, _ = _csr(HAND_B, 2)
    return ea, ca, roa, eb, cb, rob, 2


def order_case(swapped=False):
    """A = [1e16, 1, -1e16] (1 x 3), or with its last two entries swapped; B = a column of ones"""
    a = [1e16, -1e16, 1.0] if swapped else [1e16, 1.0, -1e16]
    ea, ca, roa, _ = _csr([[(k, v) for k, v in enumerate(a)]], 3)
    eb, cb, rob, _ = _csr([[(0, 1.0)], [(0, 1.0)], [(0, 1.0)]], 1)
    return ea, ca, roa, eb, cb, rob, 1


# --------------------------------------------------------------------------- the yardstick
def test_a_hand_worked_3_by_4_times_4_by_2_example_with_a_duplicate_in_each():
    # row 0: t = 0..2 from (1: 2) -> (1: 2) (0: 4) (1: 1); t = 3 from (3: 1) -> (0: 10); t = 4..6 from (1: 3) -> (1: 3) (0: 6) (1: 1.5)
    #        column 0: (4 + 10) + 6 = 20; column 1: ((2 + 1) + 3) + 1.5 = 7.5
    # row 1: empty
    # row 2: (0: 4) -> (1: 20); (2: -1) -> (0: -7)
    e, c, ro = multiply_arrays(*hand_worked())
    assert ro.tolist() == [0, 2, 2, 4] and c.tolist() == [0, 1, 0, 1] and e.tolist() == [20.0, 7.5, -7.0, 20.0]
    ea, ca, roa, eb, cb, rob, columns = hand_worked()
    pe, pc, pro = multiply_arrays(None, ca, roa, None, cb, rob, columns)
    assert pe is None and pc.tolist() == c.tolist() and pro.tolist() == ro.tolist()
    assert products_per_row(ca, roa, rob).tolist() == [7, 0, 2]
    # entries beyond the end of the offsets are ignored
    e2, c2, ro2 = multiply_arrays(np.r_[ea, 9.0], np.r_[ca, 77], roa, np.r_[eb, 9.0, 9.0], np.r_[cb, -3, 5], rob, columns)
    assert (e2.tolist(), c2.tolist(), ro2.tolist()) == (e.tolist(), c.tolist(), ro.tolist())


def test_the_sum_runs_in_stored_order():
    e, c, ro = multiply_arrays(*order_case())
    assert ro.tolist() == [0, 1] and c.tolist() == [0] and e.tolist() == [0.0]           # (1e16 + 1) - 1e16: the 1 is lost; the zero is stored
    e, c, ro = multiply_arrays(*order_case(swapped=True))
    assert ro.tolist() == [0, 1] and c.tolist() == [0] and e.tolist() == [1.0]


def test_a_lone_negative_zero_product_gives_positive_zero():
    e, c, ro = multiply_arrays(np.array([-0.0]), [0], [0, 1], np.array([1.0]), [0], [0, 1], 1)
    assert e.tolist() == [0.0] and not np.signbit(e[0]) and ro.tolist() == [0, 1]


def _rectangular():
    s = problems.sparse_rectangular(900, 400)
    e, c, ro = s.Elements, s.ColumnIndeces, s.RowOffsets
    te, tc, tro, _ = transpose_arrays(e, c, ro, 400)
    return (e, c, ro, 400), (te, tc, tro, 900)


def pair(name):
    """((elements, columns, offsets, columns of the matrix) of A, the same of B)"""
    if name == "rectangular":
        return _rectangular()
    s = {"random1037": lambda: problems.random_nonsymmetric(1037), "poisson12": lambda: problems.poisson(12, 12, 12),
         "upwind12x10x8": NONSYMMETRIC["upwind12x10x8"]}[name]()
    m = csr_of(s) + (s.Count,)
    return m, m


PAIRS = ["random1037", "poisson12", "upwind12x10x8", "rectangular"]


@pytest.mark.parametrize("name", PAIRS)
def test_the_pattern_is_scipys_and_the_values_lie_within_the_rounding_of_the_sums(name):
    (ea, ca, roa, inner), (eb, cb, rob, columns) = pair(name)
    rows = len(roa) - 1
    e, c, ro = multiply_arrays(ea, ca, roa, eb, cb, rob, columns)
    A, B = sp.csr_matrix((ea, ca, roa), shape=(rows, inner)), sp.csr_matrix((eb, cb, rob), shape=(inner, columns))
    ones = sp.csr_matrix((np.ones(len(ca)), ca, roa), shape=A.shape) @ sp.csr_matrix((np.ones(len(cb)), cb, rob), shape=B.shape)
    ones.sort_indices()
    assert np.array_equal(ones.indptr, ro) and np.array_equal(ones.indices, c)
    assert np.all(np.diff(c)[np.setdiff1d(np.arange(len(c) - 1), ro[1:-1] - 1)] > 0)      # columns ascend inside every row, none twice
    S, bound = A @ B, abs(A) @ abs(B)
    S.sort_indices()
    bound.sort_indices()
    assert np.array_equal(S.indices, c) and np.array_equal(bound.indices, c)
    u = np.repeat(products_per_row(ca, roa, rob), np.diff(ro))
    assert np.all(np.abs(e - S.data) <= u * np.finfo(np.float64).eps * bound.data)
    print(f"{name}: {int(products_per_row(ca, roa, rob).sum())} products, {len(c)} entries, bit-equal to scipy: {e.tobytes() == S.data.tobytes()}")


def test_an_integer_valued_product_equals_the_dense_one_exactly():
    rng = np.random.default_rng(7)
    A = sp.random(61, 47, density=0.15, random_state=3, format="csr")
    B = sp.random(47, 53, density=0.2, random_state=4, format="csr")
    values = np.array([-3.0, -2.0, -1.0, 1.0, 2.0, 3.0])
    A.data, B.data = rng.choice(values, len(A.data)), rng.choice(values, len(B.data))
    e, c, ro = multiply_arrays(A.data, A.indices, A.indptr, B.data, B.indices, B.indptr, 53)
    dense = A.toarray() @ B.toarray()
    got = sp.csr_matrix((e, c, ro), shape=(61, 53)).toarray()
    assert np.array_equal(got, dense)
    pattern = abs(A).toarray() @ abs(B).toarray() > 0
    stored = np.zeros_like(pattern)
    stored[np.repeat(np.arange(61), np.diff(ro)), c] = True
    assert np.array_equal(stored, pattern) and np.any(e == 0.0)           # sums that come to zero are stored


def test_the_galerkin_triple_product_equals_the_aggregation_yardstick():
    s = problems.poisson(8, 8, 8)
    e, c, ro = csr_of(s)
    amap = box_maps(s.grid, 2)[0]
    nc = int(amap.max()) + 1
    P = (np.ones(s.Count), amap.astype(np.int32), np.arange(s.Count + 1, dtype=np.int32))
    pte, ptc, ptro, _ = transpose_arrays(*P, nc)
    ap = multiply_arrays(e, c, ro, *P, nc)
    ge, gc, gro = multiply_arrays(pte, ptc, ptro, *ap, nc)
    we, wc, wro = galerkin(e, c, ro, amap, nc, 1.0)
    assert np.array_equal(gro, wro) and np.array_equal(gc, wc) and ge.tobytes() == we.tobytes()


# --------------------------------------------------------------------------- the library without a device
def test_the_exports_are_there_and_declared(hiplib):
    for name in ("MgcgCsrMultiply", "MgcgMultiplyClassLimits"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    from conjugategradient_amd import amg

    short, lds = amg.multiply_class_limits()
    assert 1 <= short < lds
    only = C.c_int(0)
    hiplib.MgcgMultiplyClassLimits(None, C.byref(only))
    assert only.value == lds
    hiplib.MgcgMultiplyClassLimits(C.byref(only), None)
    assert only.value == short
    assert callable(amg.csr_multiply_gpu) and callable(amg.multiply_gpu)


class _VectorHead(C.Structure):
    """The head of the library's vector handle (csrc/common.hpp: data, size, device)."""
    _fields_ = [("data", C.c_void_p), ("size", C.c_longlong), ("device", C.c_int), ("rest", C.c_char * 256)]


def test_every_refusal_before_a_device_is_asked_for_has_its_message_and_leaves_the_outputs_alone(hiplib):
    L = hiplib
    handle = C.create_string_buffer(4096)                      # stands for the two handles: a refused call looks at neither
    h = C.addressof(handle)
    # A: 28 entries in 10 rows; B: 30 entries in 12 rows, 9 columns; room for 40 entries of C.  The output heads point at host arrays that a
    # refused call must not write; the input heads point nowhere, so every call below must be refused before a device is asked for.
    fill = {"oe": np.full(40, 7.0), "oro": np.full(11, -7, dtype=np.int32), "oc": np.full(40, -7, dtype=np.int32)}
    heads = {key: _VectorHead(a.ctypes.data, len(a), -1, b"") for key, a in fill.items()}
    heads.update(ea=_VectorHead(None, 28, -1, b""), roa=_VectorHead(None, 11, -1, b""), ca=_VectorHead(None, 28, -1, b""),
                 eb=_VectorHead(None, 30, -1, b""), rob=_VectorHead(None, 13, -1, b""), cb=_VectorHead(None, 30, -1, b""),
                 s10=_VectorHead(None, 10, -1, b""), s12=_VectorHead(None, 12, -1, b""), s27=_VectorHead(None, 27, -1, b""), s29=_VectorHead(None, 29, -1, b""),
                 s39=_VectorHead(None, 39, -1, b""))
    A = {key: C.addressof(v) for key, v in heads.items()}
    before = {key: bytes(v) for key, v in heads.items()}
    who = "MgcgCsrMultiply: "

    def call(blas=h, sparse=h, ea=A["ea"], roa=A["roa"], ca=A["ca"], nnzA=28, eb=A["eb"], rob=A["rob"], cb=A["cb"], nnzB=30, rows=10, inner=12, columns=9,
             oe=A["oe"], oro=A["oro"], oc=A["oc"], capacity=40):
        L.MgcgClearLastError()
        got = L.MgcgCsrMultiply(blas, sparse, ea, roa, ca, nnzA, eb, rob, cb, nnzB, rows, inner, columns, oe, oro, oc, capacity)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        assert np.all(fill["oe"] == 7.0) and all(np.all(fill[k] == -7) for k in ("oro", "oc"))
        assert {key: bytes(v) for key, v in heads.items()} == before
        assert got == -1
        return msg

    for kw in (dict(blas=None), dict(sparse=None), dict(roa=None), dict(ca=None), dict(rob=None), dict(cb=None)):
        assert call(**kw) == who + "null handle", kw
    together = who + "null handle (elementsA, elementsB and outElements are given together, or none of them)"
    for kw in (dict(ea=None), dict(eb=None), dict(oe=None), dict(ea=None, eb=None), dict(ea=None, oe=None), dict(eb=None, oe=None),
               dict(ea=None, oe=None, oro=None, oc=None), dict(eb=None, oe=None, oro=None, oc=None)):
        assert call(**kw) == together, kw
    outputs = who + "null handle (the output vectors are given together or not at all)"
    for kw in (dict(oro=None), dict(oc=None), dict(ea=None, eb=None, oe=None, oro=None), dict(ea=None, eb=None, oe=None, oc=None)):
        assert call(**kw) == outputs, kw
    bad = who + "bad parameters (rows %d, inner %d, columns %d, elementsCountA %d, elementsCountB %d, outCapacity %d)"
    assert call(rows=0) == bad % (0, 12, 9, 28, 30, 40)
    assert call(rows=-3) == bad % (-3, 12, 9, 28, 30, 40)
    assert call(inner=0) == bad % (10, 0, 9, 28, 30, 40)
    assert call(columns=0) == bad % (10, 12, 0, 28, 30, 40)
    assert call(nnzA=-1) == bad % (10, 12, 9, -1, 30, 40)
    assert call(nnzB=-2) == bad % (10, 12, 9, 28, -2, 40)
    assert call(capacity=-1) == bad % (10, 12, 9, 28, 30, -1)
    small = who + "vectors of %s too small (%d values, %d offsets, %d columns for %d entries in %d rows)"
    assert call(roa=A["s10"]) == small % ("A", 28, 10, 28, 28, 10)
    assert call(rows=11) == small % ("A", 28, 11, 28, 28, 11)
    assert call(nnzA=29) == small % ("A", 28, 11, 28, 29, 10)
    assert call(ca=A["s27"]) == small % ("A", 28, 11, 27, 28, 10)
    assert call(ea=A["s27"]) == small % ("A", 27, 11, 28, 28, 10)
    assert call(rob=A["s12"]) == small % ("B", 30, 12, 30, 30, 12)
    assert call(inner=13) == small % ("B", 30, 13, 30, 30, 13)
    assert call(nnzB=31) == small % ("B", 30, 13, 30, 31, 12)
    assert call(cb=A["s29"]) == small % ("B", 30, 13, 29, 30, 12)
    assert call(eb=A["s29"]) == small % ("B", 29, 13, 30, 30, 12)
    out = who + "output vectors too small (%d values, %d offsets, %d columns for a capacity of %d entries in %d rows)"
    assert call(oro=A["s10"]) == out % (40, 10, 40, 40, 10)
    assert call(oc=A["s39"]) == out % (40, 11, 39, 40, 10)
    assert call(oe=A["s39"]) == out % (39, 11, 40, 40, 10)
    assert call(capacity=41) == out % (40, 11, 40, 41, 10)
    # the pattern-only and the count-only forms pass the pairing checks and are refused by a later one (-1 stands for "no values")
    assert call(ea=None, eb=None, oe=None, roa=A["s10"]) == small % ("A", -1, 10, 28, 28, 10)
    assert call(ea=None, eb=None, oe=None, oc=A["s39"]) == out % (-1, 11, 39, 40, 10)
    assert call(oe=None, oro=None, oc=None, rob=A["s12"]) == small % ("B", 30, 12, 30, 30, 12)
    assert call(ea=None, eb=None, oe=None, oro=None, oc=None, inner=0) == bad % (10, 0, 9, 28, 30, 40)
    assert call(oe=None, oro=None, oc=None, capacity=-1, columns=0) == bad % (10, 12, 0, 28, 30, -1)     # (a count-only call's capacity is not looked at)
    # the order: handles, the pairing, the outputs, the counts, A, B, the outputs' sizes
    assert call(blas=None, ea=None) == who + "null handle"
    assert call(ea=None, oro=None) == together
    assert call(oro=None, rows=0) == outputs
    assert call(rows=0, roa=A["s10"]) == bad % (0, 12, 9, 28, 30, 40)
    assert call(roa=A["s10"], rob=A["s12"]) == small % ("A", 28, 10, 28, 28, 10)
    assert call(rob=A["s12"], oro=A["s10"]) == small % ("B", 30, 12, 30, 30, 12)
