"""CSR transposition (MgcgCsrTranspose) on the host side: the numpy yardstick of its contract, checked against a hand-worked example, against
scipy and against the entry order that the symmetric part's yardstick implies; and the library without a device -- the exports, and every
refusal that is made before a device is asked for, with its message and with the outputs left alone.

The contract (include/MgcgGpu.h): row c of A^T holds the stored entries of column c of A by ascending stored position k; source[q] = k; the
column of entry q is the row of A that stores k; values are bit copies.  A stable sort of the stored columns is exactly that."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from conjugategradient_amd import _lib, problems
from tests.test_amg_host import csr_of, reversed_rows, with_duplicates
from tests.test_amg_sym_host import NONSYMMETRIC, symmetric_part_arrays


def transpose_arrays(e, c, ro, columns):
    """(elements, columns, offsets, source) of A^T by the contract; e may be None (pattern only: None comes back).  Entries beyond ro[-1]
    are ignored."""
    ro = np.asarray(ro, dtype=np.int64)
    nnz = int(ro[-1])
    c = np.asarray(c, dtype=np.int64)[:nnz]
    source = np.argsort(c, kind="stable")
    row_of = np.repeat(np.arange(len(ro) - 1, dtype=np.int64), np.diff(ro))
    offsets = np.r_[0, np.cumsum(np.bincount(c, minlength=columns))]
    values = None if e is None else np.asarray(e, dtype=np.float64)[:nnz][source]
    return values, row_of[source].astype(np.int32), offsets.astype(np.int32), source.astype(np.int32)


def arrow(n, copies=1):
    """Row 0 stores column 0 alone; every other row stores its diagonal and column 0 (`copies` times, one after the other): column 0 is
    stored by every row."""
    cols, vals, offsets = [0], [float(n)], [0, 1]
    for i in range(1, n):
        cols += [i] + [0] * copies
        vals += [2.0 + i % 7] + [-(1.0 + (i + j) % 5) / 8.0 for j in range(copies)]
        offsets.append(len(cols))
    return np.array(vals), np.array(cols, dtype=np.int32), np.array(offsets, dtype=np.int32)


def arrow_fast(n, copies=1):
    """arrow() by numpy, for the long ones."""
    i = np.arange(1, n)
    per = 1 + copies
    cols = np.zeros(1 + per * (n - 1), dtype=np.int32)
    vals = np.empty(1 + per * (n - 1))
    vals[0] = float(n)
    cols[1::per] = i
    vals[1::per] = 2.0 + i % 7
    for j in range(copies):
        vals[2 + j::per] = -(1.0 + (i + j) % 5) / 8.0
    offsets = np.r_[0, 1 + per * np.arange(n)].astype(np.int32)
    return vals, cols, offsets


def merged_arrays(e, c, ro):
    """[A | A^T] of a square matrix as MgcgSymmetricPart forms it: (source, columns, offsets); row i = A's row i, then A^T's row i."""
    n = len(ro) - 1
    _, tc, tro, tsrc = transpose_arrays(None, c, ro, n)
    ro = np.asarray(ro, dtype=np.int64)
    mro = ro + tro
    source, cols = np.empty(2 * ro[-1], dtype=np.int64), np.empty(2 * ro[-1], dtype=np.int64)
    for i in range(n):
        a, t = slice(ro[i], ro[i + 1]), slice(tro[i], tro[i + 1])
        mid = mro[i] + ro[i + 1] - ro[i]
        source[mro[i]:mid], cols[mro[i]:mid] = np.arange(a.start, a.stop), np.asarray(c)[a]
        source[mid:mro[i + 1]], cols[mid:mro[i + 1]] = tsrc[t], tc[t]
    return source, cols, mro


# --------------------------------------------------------------------------- the yardstick
def test_a_hand_worked_3_by_4_example_with_a_duplicate():
    #      col 0   1   2   3
    # row 0  [ 1   .   2   . ]            stored: (0: 1) (2: 2)
    # row 1  [ .   .   .   . ]            empty
    # row 2  [ 5   .  3+4  . ]            stored unsorted, column 2 twice: (2: 3) (0: 5) (2: 4)
    e, c, ro = np.array([1.0, 2.0, 3.0, 5.0, 4.0]), np.array([0, 2, 2, 0, 2]), np.array([0, 2, 2, 5])
    te, tc, tro, src = transpose_arrays(e, c, ro, 4)
    assert tro.tolist() == [0, 2, 2, 5, 5]                     # columns 1 and 3 are stored by nobody
    assert src.tolist() == [0, 3, 1, 2, 4]                     # column 0: k = 0, 3; column 2: k = 1, 2, 4 (the duplicate in stored order)
    assert tc.tolist() == [0, 2, 0, 2, 2]
    assert te.tolist() == [1.0, 5.0, 2.0, 3.0, 4.0]
    pe, pc, pro, psrc = transpose_arrays(None, c, ro, 4)
    assert pe is None and (pc.tolist(), pro.tolist(), psrc.tolist()) == (tc.tolist(), tro.tolist(), src.tolist())
    # entries beyond ro[-1] are ignored
    te2, tc2, tro2, src2 = transpose_arrays(np.r_[e, 9.0], np.r_[c, 1], ro, 4)
    assert (te2.tolist(), tc2.tolist(), tro2.tolist(), src2.tolist()) == (te.tolist(), tc.tolist(), tro.tolist(), src.tolist())


@pytest.mark.parametrize("name", ["random1037", "upwind12x10x8", "upwind-reversed", "mgcg_main600", "arrow65", "arrow4097", "arrow70001", "rectangular"])
def test_the_yardstick_equals_scipy_on_matrices_without_duplicates(name):
    if name == "rectangular":
        A = sp.random(37, 91, density=0.08, random_state=5, format="csr")
        e, c, ro, columns = A.data, A.indices, A.indptr, 91
    elif name.startswith("arrow"):
        e, c, ro = arrow_fast(int(name[5:]))
        columns = len(ro) - 1
    else:
        s = {"random1037": lambda: problems.random_nonsymmetric(1037), "upwind12x10x8": NONSYMMETRIC["upwind12x10x8"],
             "upwind-reversed": lambda: reversed_rows(NONSYMMETRIC["upwind12x10x8"]()), "mgcg_main600": lambda: problems.mgcg_main(600)}[name]()
        e, c, ro = csr_of(s)
        columns = s.Count
    te, tc, tro, src = transpose_arrays(e, c, ro, columns)
    T = sp.csr_matrix((e, c, ro), shape=(len(ro) - 1, columns)).T.tocsr()
    T.sort_indices()                                           # (scipy's conversion keeps the source rows ascending already)
    assert np.array_equal(T.indptr, tro) and np.array_equal(T.indices, tc) and T.data.tobytes() == te.tobytes()
    assert np.array_equal(np.asarray(e)[src], te) and np.array_equal(np.sort(src), np.arange(ro[-1]))


def test_arrow_builders_agree():
    for n, copies in ((1, 1), (2, 1), (34, 1), (34, 2)):
        for a, b in zip(arrow(n, copies), arrow_fast(n, copies)):
            assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["upwind-duplicates", "random1500", "upwind-reversed"])
def test_the_merged_matrix_of_the_yardstick_sums_to_the_symmetric_part(name):
    s = {"upwind-duplicates": lambda: with_duplicates(NONSYMMETRIC["upwind12x10x8"]()), "random1500": NONSYMMETRIC["random1500"],
         "upwind-reversed": lambda: reversed_rows(NONSYMMETRIC["upwind12x10x8"]())}[name]()
    e, c, ro = csr_of(s)
    source, cols, mro = merged_arrays(e, c, ro)
    se, sc, sro = [], [], [0]
    for i in range(len(ro) - 1):                               # the order of the merged row is the order of the sums: A's entries, then A^T's
        acc = {}
        for p in range(mro[i], mro[i + 1]):
            acc[cols[p]] = acc.get(cols[p], 0.0) + e[source[p]]
        for j in sorted(acc):
            sc.append(j)
            se.append(0.5 * acc[j])
        sro.append(len(sc))
    we, wc, wro = symmetric_part_arrays(e, c, ro)
    assert np.array_equal(wro, sro) and np.array_equal(wc, sc) and we.tobytes() == np.array(se).tobytes()


# --------------------------------------------------------------------------- the library without a device
def test_the_exports_are_there_and_declared(hiplib):
    for name in ("MgcgCsrTranspose", "MgcgTransposeClassLimits"):
        assert hasattr(hiplib, name) and name in _lib.SIGNATURES
    from conjugategradient_amd import amg

    short, lds = amg.transpose_class_limits()
    assert 1 <= short < lds
    only = C.c_int(0)
    hiplib.MgcgTransposeClassLimits(None, C.byref(only))
    assert only.value == lds
    assert callable(amg.csr_transpose_gpu) and callable(amg.transpose_gpu)


class _VectorHead(C.Structure):
    """The head of the library's vector handle (csrc/common.hpp: data, size, device)."""
    _fields_ = [("data", C.c_void_p), ("size", C.c_longlong), ("device", C.c_int), ("rest", C.c_char * 256)]


def test_every_refusal_before_a_device_is_asked_for_has_its_message_and_leaves_the_outputs_alone(hiplib):
    L = hiplib
    handle = C.create_string_buffer(4096)                      # stands for the two handles: a refused call looks at neither
    h = C.addressof(handle)
    # 28 entries in 10 rows of 12 columns; the output heads point at host arrays that a refused call must not write
    fill = {"oe": np.full(28, 7.0), "oro": np.full(13, -7, dtype=np.int32), "oc": np.full(28, -7, dtype=np.int32), "os": np.full(28, -7, dtype=np.int32)}
    heads = {key: _VectorHead(a.ctypes.data, len(a), -1, b"") for key, a in fill.items()}
    heads.update(e=_VectorHead(None, 28, -1, b""), ro=_VectorHead(None, 11, -1, b""), c=_VectorHead(None, 28, -1, b""),
                 s10=_VectorHead(None, 10, -1, b""), s12=_VectorHead(None, 12, -1, b""), s27=_VectorHead(None, 27, -1, b""))
    A = {key: C.addressof(v) for key, v in heads.items()}
    before = {key: bytes(v) for key, v in heads.items()}

    def call(blas=h, sparse=h, e=A["e"], ro=A["ro"], c=A["c"], nnz=28, rows=10, columns=12, oe=A["oe"], oro=A["oro"], oc=A["oc"], os=A["os"]):
        L.MgcgClearLastError()
        got = L.MgcgCsrTranspose(blas, sparse, e, ro, c, nnz, rows, columns, oe, oro, oc, os)
        msg = _lib.last_error()
        L.MgcgClearLastError()
        assert np.all(fill["oe"] == 7.0) and all(np.all(fill[k] == -7) for k in ("oro", "oc", "os"))
        assert {key: bytes(v) for key, v in heads.items()} == before
        return got, msg

    for kw in (dict(blas=None), dict(sparse=None), dict(ro=None), dict(c=None), dict(oro=None), dict(oc=None)):
        got, msg = call(**kw)
        assert got == -1 and "MgcgCsrTranspose: null handle" in msg, (kw, msg)
    for kw in (dict(e=None), dict(oe=None)):
        got, msg = call(**kw)
        assert got == -1 and "MgcgCsrTranspose: null handle (elements and outElements are given together" in msg, (kw, msg)
    for kw, word in ((dict(rows=0), "rows 0"), (dict(rows=-3), "rows -3"), (dict(columns=0), "columns 0"), (dict(nnz=-1), "elementsCount -1")):
        got, msg = call(**kw)
        assert got == -1 and "MgcgCsrTranspose: bad parameters" in msg and word in msg, (kw, msg)
    for kw in (dict(ro=A["s10"]), dict(rows=11), dict(nnz=29), dict(c=A["s27"]), dict(e=A["s27"])):
        got, msg = call(**kw)
        assert got == -1 and "MgcgCsrTranspose: matrix vectors too small" in msg, (kw, msg)
    for kw in (dict(oro=A["s12"]), dict(columns=13), dict(oc=A["s27"]), dict(oe=A["s27"]), dict(os=A["s27"])):
        got, msg = call(**kw)
        assert got == -1 and "MgcgCsrTranspose: output vectors too small" in msg, (kw, msg)
    # the pattern-only forms pass these checks (what follows asks for a device: here there may be none, and nothing is written then either)
    got, msg = call(e=None, oe=None, ro=A["s10"])
    assert got == -1 and "matrix vectors too small" in msg
    # the order: handles, then the pairing, then the counts, then the sizes
    got, msg = call(blas=None, rows=0)
    assert "null handle" in msg
    got, msg = call(e=None, rows=0)
    assert "given together" in msg
    got, msg = call(rows=0, ro=A["s10"])
    assert "bad parameters" in msg
    got, msg = call(ro=A["s10"], oro=A["s12"])
    assert "matrix vectors too small" in msg
