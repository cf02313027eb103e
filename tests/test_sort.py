"""GxB_Matrix_sort / GxB_Vector_sort: ``A.ss.sort(op, order)`` / ``v.ss.sort(op)`` and the ``ss.compactify`` built on them -- the lane-group,
LDS and radix paths of grb_sort.hip on the GPU tier, the same sources under the SIMT emulator on the CPU tier.

1. the reference's own literals (tests/golden/sort_literals.json) through every spelling the host has;
2. seeded random parity, all 11 types x lt / gt, rowwise and columnwise, against an expectation computed HERE with numpy alone --
   per row ``np.lexsort((q, value_key, isnan))`` with the value cast to the operator's type, negated / complemented for gt, zeros equal --
   independent of the library and of the oracle; C and P compared as bit patterns;
3. the path limits, read from GrX_sort_limits: rows of every length around a lane-group width, around the LDS limit, hubs side by side,
   and GrX_sort_last against the counts the row lengths predict;
4. special values: NaN payloads, signed zeros, infinities, subnormals, integer extremes, BOOL, an iso matrix;
5. compactify against numpy;
6. the C ABI directly (ctypes) and the errors;
7. no growth of device memory over repeated calls (GPU tier).
"""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest

from tests.backend import DEVICES, ROOT, bind
from tests.test_select import NP_OF, _handle, _matrix_error, assert_coo, assert_vec, stored_iso
from tests.values import ALL_TYPES, rand_vals


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


@pytest.fixture(scope="module")
def literals():
    with open(os.path.join(ROOT, "tests", "golden", "sort_literals.json")) as f:
        return json.load(f)


def limits():
    from graphblas_amd import _lib

    w, l = ctypes.c_int64(), ctypes.c_int64()
    assert _lib.lib.GrX_sort_limits(ctypes.byref(w), ctypes.byref(l)) == 0
    return int(w.value), int(l.value)


def sort_last():
    from graphblas_amd import _lib

    out = (ctypes.c_int64 * 3)()
    assert _lib.lib.GrX_sort_last(out) == 0
    return list(out)


# ---- the expectation --------------------------------------------------------------------------------------------------------------------
def cast_like_library(vals, np_t):
    """cast_value of csrc/grb_ops.hpp with numpy: to BOOL ``x != 0``; floating point -> integer truncates and saturates, NaN -> 0."""
    np_t = np.dtype(np_t)
    vals = np.asarray(vals)
    if np_t == vals.dtype:
        return vals
    if np_t.kind == "b":
        return vals != 0
    if vals.dtype.kind == "f" and np_t.kind in "iu":
        info = np.iinfo(np_t)
        x = np.nan_to_num(vals.astype(np.float64), nan=0.0, posinf=np.inf, neginf=-np.inf)
        out = np.zeros(vals.shape, np_t)
        lo, hi = x <= float(info.min), x >= float(info.max)
        mid = ~(lo | hi)
        out[lo], out[hi] = info.min, info.max
        out[mid] = x[mid].astype(np_t)
        return out
    with np.errstate(all="ignore"):
        return vals.astype(np_t)


def np_sort(seg, vals, op, optype):
    """The order of the entries (given segment by segment, each in index order): for every segment ``np.lexsort((q, value_key, isnan))``.
    Returns the permutation of the entries, segment-major."""
    seg = np.asarray(seg, np.int64)
    key = cast_like_library(vals, NP_OF[optype])
    isnan = np.isnan(key) if key.dtype.kind == "f" else np.zeros(key.shape, bool)
    if key.dtype.kind == "f":
        k = np.where(isnan | (key == 0), key.dtype.type(0), key)  # (zeros equal; a NaN is placed by its flag)
        k = -k if op == "gt" else k
    elif key.dtype.kind == "b":
        k = key.astype(np.int8)
        k = 1 - k if op == "gt" else k
    else:
        k = ~key if op == "gt" else key
    q = np.arange(seg.size)  # (entries arrive in index order: the running number is the tie-break)
    return np.lexsort((q, k, isnan, seg))


def expected_sort(rows, cols, vals, op, optype, columnwise=False):
    """(rows, cols, C values in A's type, P) of the sort of the COO tuples, row-major."""
    rows, cols, vals = np.asarray(rows, np.int64), np.asarray(cols, np.int64), np.asarray(vals)
    seg, idx = (cols, rows) if columnwise else (rows, cols)
    base = np.lexsort((idx, seg))
    seg, idx, v = seg[base], idx[base], vals[base]
    order = np_sort(seg, v, op, optype)
    first = np.searchsorted(seg, seg)  # start of every entry's segment
    r = np.arange(seg.size) - first
    out_seg, out_r, out_c, out_p = seg, r, v[order], idx[order]
    er, ec = (out_r, out_seg) if columnwise else (out_seg, out_r)
    o = np.lexsort((ec, er))
    return er[o], ec[o], out_c[o], out_p[o]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind != "b" else a.astype(np.uint8)


def check_sorted(C, P, exp, where):
    er, ec, ev, ep = exp
    if C is not None:
        I, J, X = C.to_coo()
        assert I.tolist() == er.tolist() and J.tolist() == ec.tolist(), (where, "pattern of C")
        assert X.dtype == ev.dtype and bits(X).tolist() == bits(ev).tolist(), (where, "values of C")
    if P is not None:
        I, J, X = P.to_coo()
        assert I.tolist() == er.tolist() and J.tolist() == ec.tolist(), (where, "pattern of P")
        assert X.tolist() == ep.tolist(), (where, "values of P")


def matrix_of_lengths(gb, rng, deg, vals, tname, ncols=None):
    deg = np.asarray(deg)
    n = int(ncols or max(int(deg.max()), 1) + 3)
    rows = np.repeat(np.arange(deg.size), deg)
    cols = np.concatenate([np.sort(rng.choice(n, d, replace=False)) for d in deg]) if rows.size else np.zeros(0, np.int64)
    return gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=deg.size, ncols=n), rows, cols


# ---- 1. the reference's literals ------------------------------------------------------------------------------------------------------
def op_spellings(gb, name):
    return [getattr(gb.binary, name), {"lt": "<", "gt": ">"}[name], name]


def test_matrix_literals(gb, literals):
    lit = literals["matrix"]
    A = gb.Matrix.from_coo(lit["rows"], lit["cols"], lit["vals"], nrows=lit["nrows"], ncols=lit["ncols"])
    B = A.T.new()
    for case in lit["cases"]:
        for op, (permutation, values), nthreads in itertools.product(op_spellings(gb, case["op"]), itertools.product([True, False], repeat=2), [None, 4]):
            kw = dict(values=values, permutation=permutation, nthreads=nthreads)
            forms = [A.ss.sort(op, case["order"], **kw), B.T.ss.sort(op, case["order"], **kw)]  # (B.T is A: the library sorts B the other way)
            if case["op"] == "lt" and case["order"] == "rowwise" and not isinstance(op, str):
                forms.append(A.ss.sort(**kw))
            for k, (C, P) in enumerate(forms):
                where = (case["name"], repr(op), kw, k)
                assert (C is None) == (not values) and (P is None) == (not permutation), where
                if C is not None:
                    assert C.dtype.name == "INT64" and C.shape == A.shape, where
                    assert_coo(C, case["rows"], case["cols"], case["C"], where)
                if P is not None:
                    assert P.dtype.name == "UINT64" and P.shape == A.shape, where
                    assert_coo(P, case["rows"], case["cols"], case["P"], where)
    with pytest.raises(gb.exceptions.DomainMismatch):  # tests/test_matrix.py:4266
        A.ss.sort("+")


def test_vector_literals(gb, literals):
    lit = literals["vector"]
    v = gb.Vector.from_coo(lit["idx"], lit["vals"], size=lit["size"])
    for case in lit["cases"]:
        for op, (permutation, values), nthreads in itertools.product(op_spellings(gb, case["op"]), itertools.product([True, False], repeat=2), [None, 4]):
            w, p = v.ss.sort(op, values=values, permutation=permutation, nthreads=nthreads)
            assert (w is None) == (not values) and (p is None) == (not permutation)
            if w is not None:
                assert w.dtype.name == "INT64" and w.size == v.size
                assert_vec(w, case["idx"], case["w"], (case["name"], repr(op)))
            if p is not None and case["p"] is not None:
                assert p.dtype.name == "UINT64" and p.size == v.size
                assert_vec(p, case["idx"], case["p"], (case["name"], repr(op)))
    w, p = v.ss.sort()
    assert_vec(w, [0, 1, 2, 3], [0, 1, 1, 2], "default operator")
    with pytest.raises(gb.exceptions.DomainMismatch):  # tests/test_vector.py:2629
        v.ss.sort(gb.binary.plus)


# ---- 2. seeded random parity ------------------------------------------------------------------------------------------------------------
def draw_values(rng, k, tname):
    """Many ties, both signs, the full range, and -- floating point -- NaN, infinities and both zeros."""
    if tname == "BOOL":
        return rand_vals(rng, k, tname, "signed")
    if tname.startswith("FP"):
        return rand_vals(rng, k, tname, "exact" if rng.random() < 0.5 else "special")
    small = rand_vals(rng, k, tname, "small")
    return np.where(rng.random(k) < 0.5, small % 7, rand_vals(rng, k, tname, "signed")).astype(NP_OF[tname])


@pytest.mark.parametrize("op", ["lt", "gt"])
@pytest.mark.parametrize("tname", ALL_TYPES)
def test_sort_random(gb, tname, op):
    rng = np.random.default_rng(4100 + ALL_TYPES.index(tname) * 2 + (op == "gt"))
    m, n = 45, 150
    deg = rng.integers(0, 40, m)
    deg[rng.integers(0, m, 4)] = [0, 70, 130, 150]  # (rows for the LDS path too)
    vals = draw_values(rng, int(deg.sum()), tname)
    A, rows, cols = matrix_of_lengths(gb, rng, deg, vals, tname, ncols=n)
    for order in ("rowwise", "columnwise"):
        C, P = A.ss.sort(getattr(gb.binary, op), order)
        assert C.dtype.name == tname and P.dtype.name == "UINT64"
        check_sorted(C, P, expected_sort(rows, cols, vals, op, tname, order == "columnwise"), (tname, op, order))
    # on the transposed view the order flips
    C, P = A.T.ss.sort(getattr(gb.binary, op), "rowwise", values=False)
    assert C is None
    check_sorted(None, P, expected_sort(cols, rows, vals, op, tname), (tname, op, "A.T"))


@pytest.mark.parametrize("op", ["lt", "gt"])
def test_operator_of_another_type(gb, op):
    """An INT64 matrix under lt[FP32] / gt[FP32]: 2^24 + {0, 1, 2, 3} collide in FP32, so the tie-break decides; C keeps the INT64 values.
    And an FP64 matrix under an INT8 operator: truncation, saturation, NaN -> 0."""
    rng = np.random.default_rng(77)
    deg = np.array([0, 9, 33, 1, 80, 17])
    base = np.int64(1 << 24)
    vals = base * rng.integers(1, 4, int(deg.sum())) + rng.integers(0, 4, int(deg.sum()))
    A, rows, cols = matrix_of_lengths(gb, rng, deg, vals, "INT64")
    exp = expected_sort(rows, cols, vals, op, "FP32")
    assert exp[3].tolist() != expected_sort(rows, cols, vals, op, "INT64")[3].tolist()  # (the collisions matter)
    C, P = A.ss.sort(getattr(gb.binary, op)["FP32"])
    assert C.dtype.name == "INT64"
    check_sorted(C, P, exp, ("INT64 under FP32", op))
    fv = rand_vals(rng, int(deg.sum()), "FP64", "special", span=3)
    fv[::5] = np.resize([1.5, 1.25, -0.5, 300.7, -300.2], fv[::5].size)
    F, rows, cols = matrix_of_lengths(gb, rng, deg, fv, "FP64")
    C, P = F.ss.sort(getattr(gb.binary, op)["INT8"], "columnwise")
    check_sorted(C, P, expected_sort(rows, cols, fv, op, "INT8", True), ("FP64 under INT8", op))


# ---- 3. the path limits -------------------------------------------------------------------------------------------------------------------
def limit_lengths():
    wave_max, lds_max = limits()
    assert wave_max == 64 and lds_max >= 1024
    return [0, 0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, wave_max - 1, wave_max, wave_max + 1, lds_max - 1, lds_max, lds_max + 1, lds_max + 7, 3,
            lds_max + 5, 0, 0]


def pattern_values(pattern, deg, np_t):
    out = []
    for d in deg:
        k = np.arange(d)
        out.append({"ascending": k, "descending": d - k, "equal": np.full(d, 5), "alternating": 3 + 4 * (k % 2)}[pattern])
    return np.concatenate(out).astype(np_t)


@pytest.mark.parametrize("tname", ["FP32", "INT64"])
@pytest.mark.parametrize("pattern", ["ascending", "descending", "equal", "alternating"])
def test_path_limits(gb, pattern, tname):
    """Empty rows at both ends, every length around the lane-group widths and around the LDS limit, two hubs side by side, a short row,
    a third hub; 24 rows, of which 5 take 4-lane groups, 3 take 16 and 6 take 64: no multiple of the 16 / 4 / 1 rows of a wavefront."""
    wave_max, lds_max = limits()
    deg = np.array(limit_lengths())
    rng = np.random.default_rng(len(pattern))
    vals = pattern_values(pattern, deg, NP_OF[tname])
    A, rows, cols = matrix_of_lengths(gb, rng, deg, vals, tname)
    predicted = [int((deg <= wave_max).sum()), int(((deg > wave_max) & (deg <= lds_max)).sum()), int((deg > lds_max).sum())]
    assert predicted[1] == 3 and predicted[2] == 3
    for op in ("lt", "gt"):
        C, P = A.ss.sort(getattr(gb.binary, op))
        assert sort_last() == predicted, (pattern, tname, op)
        check_sorted(C, P, expected_sort(rows, cols, vals, op, tname), (pattern, tname, op))


def test_one_long_row_and_many_short(gb):
    """One hub alone (no second radix pass) and 150 short rows (several wavefronts of every lane-group width)."""
    wave_max, lds_max = limits()
    rng = np.random.default_rng(12)
    deg = np.concatenate([rng.integers(0, 6, 50), [lds_max + 300], rng.integers(5, 17, 50), rng.integers(17, 65, 50)])
    vals = rng.integers(-50, 50, int(deg.sum())).astype(np.int32)
    A, rows, cols = matrix_of_lengths(gb, rng, deg, vals, "INT32")
    C, P = A.ss.sort(">")
    assert sort_last() == [150, 0, 1]
    check_sorted(C, P, expected_sort(rows, cols, vals, "gt", "INT32"), "one hub")


def test_vector_paths(gb):
    wave_max, lds_max = limits()
    rng = np.random.default_rng(3)
    for nv, path in ((0, 0), (1, 0), (5, 0), (wave_max, 0), (wave_max + 1, 1), (lds_max, 1), (lds_max + 1, 2)):
        n = nv + 40
        idx = np.sort(rng.choice(n, nv, replace=False))
        vals = rand_vals(rng, nv, "FP32", "exact")
        u = gb.Vector.from_coo(idx, vals, dtype="FP32", size=n)
        for op in ("lt", "gt"):
            w, p = u.ss.sort(op)
            assert sort_last() == [int(path == k) if nv else int(k == 0) for k in range(3)], (nv, op)
            order = np_sort(np.zeros(nv, np.int64), vals, op, "FP32")
            I, X = w.to_coo()
            assert I.tolist() == list(range(nv)) and bits(X).tolist() == bits(vals[order]).tolist(), (nv, op)
            I, X = p.to_coo()
            assert I.tolist() == list(range(nv)) and X.tolist() == idx[order].tolist(), (nv, op)
            assert w.size == n and p.size == n and p.dtype.name == "UINT64"


# ---- 4. special values ----------------------------------------------------------------------------------------------------------------------
def special_values(tname):
    if tname == "FP32":
        nans = np.array([0x7fc00000, 0xffc00000, 0x7fc00001, 0x7fc12345, 0xffffffff], np.uint32).view(np.float32)
        fi = np.finfo(np.float32)
    elif tname == "FP64":
        nans = np.array([0x7ff8000000000000, 0xfff8000000000000, 0x7ff8000000000001, 0x7ff8123456789abc, 0xffffffffffffffff], np.uint64).view(np.float64)
        fi = np.finfo(np.float64)
    if tname.startswith("FP"):
        np_t = NP_OF[tname]
        reals = np.array([0.0, -0.0, np.inf, -np.inf, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny, fi.max, -fi.max, 1.0, -1.0, 0.0, -0.0], np_t)
        return np.concatenate([nans[:2], reals, nans[2:]])
    if tname == "BOOL":
        return np.array([True, False, True, True, False, False, True], bool)
    info = np.iinfo(NP_OF[tname])
    mid = (int(info.max) + int(info.min)) // 2
    return np.array([info.max, info.min, 0, 1, info.max - 1, info.min + 1, mid, mid + 1, info.max, info.min, -1 if info.min < 0 else (1 << (info.bits - 1)) + 5],
                    dtype=NP_OF[tname])


@pytest.mark.parametrize("tname", ["FP32", "FP64", "INT64", "UINT64", "INT8", "BOOL"])
def test_special_values(gb, tname):
    sv = special_values(tname)
    rng = np.random.default_rng(5)
    # the specials in three rows: as they are, reversed, shuffled -- the third row long enough for the LDS path
    row3 = np.concatenate([sv] * 6)[rng.permutation(sv.size * 6)]
    deg = np.array([sv.size, 0, sv.size, row3.size])
    vals = np.concatenate([sv, sv[::-1], row3])
    A, rows, cols = matrix_of_lengths(gb, rng, deg, vals, tname)
    for op in ("lt", "gt"):
        C, P = A.ss.sort(op)
        check_sorted(C, P, expected_sort(rows, cols, vals, op, tname), (tname, op))
        if tname.startswith("FP"):
            I, J, X = C.to_coo()
            for r in (0, 2, 3):
                x = X[I == r]
                nn = int(np.isnan(x).sum())
                assert nn > 0 and not np.isnan(x[: x.size - nn]).any() and np.isnan(x[x.size - nn:]).all(), (tname, op, r, "NaNs are last")
                real = x[: x.size - nn]
                assert (real[1:] >= real[:-1]).all() if op == "lt" else (real[1:] <= real[:-1]).all()


def test_iso_matrix(gb):
    rng = np.random.default_rng(8)
    deg = np.array([3, 0, 70, 20, 1])
    rows = np.repeat(np.arange(deg.size), deg)
    cols = np.concatenate([np.sort(rng.choice(90, d, replace=False)) for d in deg])
    indptr = np.concatenate([[0], np.cumsum(deg)])
    A = gb.Matrix.ss.import_csr(nrows=deg.size, ncols=90, indptr=indptr, values=np.array([2.5]), col_indices=cols, is_iso=True, sorted_cols=True, dtype="FP64")
    assert stored_iso(A)
    for op, order in (("lt", "rowwise"), ("gt", "rowwise"), ("lt", "columnwise")):
        C, P = A.ss.sort(op, order)
        check_sorted(C, P, expected_sort(rows, cols, np.full(rows.size, 2.5), op, "FP64", order == "columnwise"), ("iso", op, order))
        if order == "rowwise":
            assert stored_iso(C)
    I, J, X = A.ss.sort()[1].to_coo()
    assert X.tolist() == cols.tolist()  # (P is the identity per row)


# ---- 5. compactify ------------------------------------------------------------------------------------------------------------------------
def np_compactify(rows, cols, vals, shape, how, k, columnwise, reverse, asindex):
    er, ec, ev, ep = expected_sort(rows, cols, vals, "lt" if how == "smallest" else "gt", "FP64", columnwise)
    seg, r = (ec, er) if columnwise else (er, ec)
    x = ep.astype(np.uint64) if asindex else ev
    longest = int(r.max()) + 1 if r.size else 0
    k = longest if k is None else k
    keep = r < k
    seg, r, x = seg[keep], r[keep], x[keep]
    if reverse:
        cnt = np.bincount(seg, minlength=max(shape))
        r = cnt[seg] - 1 - r
    out_shape = (k, shape[1]) if columnwise else (shape[0], k)
    return ((r, seg) if columnwise else (seg, r)), x, out_shape


def test_matrix_compactify(gb):
    rng = np.random.default_rng(21)
    m, n = 13, 40
    deg = rng.integers(0, 12, m)
    deg[4] = 30
    vals = rng.integers(-6, 7, int(deg.sum())).astype(np.float64)
    vals[rng.random(vals.size) < 0.1] = np.nan
    A, rows, cols = matrix_of_lengths(gb, rng, deg, vals, "FP64", ncols=n)
    col_longest = int(np.bincount(cols, minlength=n).max())
    for columnwise in (False, True):
        longest = col_longest if columnwise else 30
        for how, k, reverse, asindex in itertools.product(("smallest", "largest"), (None, 0, 1, 3, longest - 1, longest, longest + 4), (False, True), (False, True)):
            if k is not None and k > (m if columnwise else n):
                continue
            R = A.ss.compactify(how, k, "columnwise" if columnwise else "rowwise", reverse=reverse, asindex=asindex)
            (er, ec), ex, shape = np_compactify(rows, cols, vals, (m, n), how, k, columnwise, reverse, asindex)
            where = (how, k, columnwise, reverse, asindex)
            assert R.shape == shape and R.dtype.name == ("UINT64" if asindex else "FP64"), (where, R.shape, shape)
            o = np.lexsort((ec, er))
            I, J, X = R.to_coo()
            assert I.tolist() == er[o].tolist() and J.tolist() == ec[o].tolist(), where
            assert bits(X).tolist() == bits(ex[o]).tolist(), where
    # on the transposed view; the k strongest entries of every row, the common use
    R = A.T.ss.compactify("largest", 2, "columnwise")
    (er, ec), ex, shape = np_compactify(cols, rows, vals, (n, m), "largest", 2, True, False, False)
    assert R.shape == shape
    o = np.lexsort((ec, er))
    I, J, X = R.to_coo()
    assert I.tolist() == er[o].tolist() and J.tolist() == ec[o].tolist() and bits(X).tolist() == bits(ex[o]).tolist()


def test_vector_compactify(gb):
    rng = np.random.default_rng(22)
    n, nv = 90, 37
    idx = np.sort(rng.choice(n, nv, replace=False))
    vals = rng.integers(-6, 7, nv).astype(np.float64)
    vals[[3, 20]] = np.nan
    u = gb.Vector.from_coo(idx, vals, size=n)
    for how, size, reverse, asindex in itertools.product(("smallest", "largest"), (None, 0, 1, 5, nv - 1, nv, nv + 6), (False, True), (False, True)):
        w = u.ss.compactify(how, size, reverse=reverse, asindex=asindex)
        order = np_sort(np.zeros(nv, np.int64), vals, "lt" if how == "smallest" else "gt", "FP64")
        k = nv if size is None else size
        x = (idx[order].astype(np.uint64) if asindex else vals[order])[:k]
        x = x[::-1] if reverse else x
        I, X = w.to_coo()
        where = (how, size, reverse, asindex)
        assert w.size == k and w.dtype.name == ("UINT64" if asindex else "FP64"), where
        assert I.tolist() == list(range(x.size)) and bits(X).tolist() == bits(x).tolist(), where
    for x in (u, gb.Matrix.from_coo([0], [1], [2.0], nrows=2, ncols=2)):
        for how in ("first", "last", "random"):
            with pytest.raises(gb.exceptions.NotImplementedException):
                x.ss.compactify(how)
        with pytest.raises(ValueError):
            x.ss.compactify("best")


# ---- 6. the C ABI directly and the errors --------------------------------------------------------------------------------------------------
def test_c_abi_and_errors(gb, literals):
    from graphblas_amd import _lib

    L = _lib.lib
    lit = literals["matrix"]
    r, c, x = (np.asarray(lit[k]) for k in ("rows", "cols", "vals"))
    case = lit["cases"][0]
    A = gb.Matrix.from_coo(r, c, x, nrows=7, ncols=7)
    lt, gt = _handle(L, "GrB_LT_INT64"), _handle(L, "GrB_GT_INT64")
    C, P = gb.Matrix(int, 7, 7), gb.Matrix("UINT64", 7, 7)
    # NULL C or NULL P; both NULL
    assert L.GxB_Matrix_sort(C._carg, None, lt, A._carg, None) == 0
    assert_coo(C, case["rows"], case["cols"], case["C"], "NULL P")
    assert L.GxB_Matrix_sort(None, P._carg, lt, A._carg, None) == 0
    assert_coo(P, case["rows"], case["cols"], case["P"], "NULL C")
    assert L.GxB_Matrix_sort(None, None, lt, A._carg, None) == -2  # GrB_NULL_POINTER
    assert L.GxB_Matrix_sort(C._carg, P._carg, None, A._carg, None) == -2
    assert L.GxB_Matrix_sort(C._carg, P._carg, lt, None, None) == -2
    # a C of another type: the original entry cast A -> C; a P of INT64; the old entries of the outputs are overwritten
    F, Pi = gb.Matrix.from_coo([6], [6], [1.5], nrows=7, ncols=7), gb.Matrix.from_coo([5], [6], [4], dtype="INT64", nrows=7, ncols=7)
    assert L.GxB_Matrix_sort(F._carg, Pi._carg, lt, A._carg, None) == 0
    assert F.dtype.name == "FP64"
    assert_coo(F, case["rows"], case["cols"], np.asarray(case["C"], np.float64), "FP64 C")
    assert_coo(Pi, case["rows"], case["cols"], case["P"], "INT64 P")
    B8 = gb.Matrix("INT8", 7, 7)
    big = gb.Matrix.from_coo([0, 0, 0], [1, 3, 5], [300, -2, 129], dtype="INT64", nrows=7, ncols=7)
    assert L.GxB_Matrix_sort(B8._carg, None, gt, big._carg, None) == 0
    assert_coo(B8, [0, 0, 0], [0, 1, 2], np.array([300, 129, -2]).astype(np.int8), "the value is cast, not the key")
    # a P of FP64; plus; operators that return BOOL but do not sort
    assert L.GxB_Matrix_sort(C._carg, F._carg, lt, A._carg, None) == -5  # GrB_DOMAIN_MISMATCH
    assert "INT64 or UINT64" in _matrix_error(L, C)
    assert L.GxB_Matrix_sort(C._carg, P._carg, _handle(L, "GrB_PLUS_INT64"), A._carg, None) == -5
    assert "BOOL" in _matrix_error(L, C)
    for name in ("GrB_LE_INT64", "GxB_PAIR_BOOL"):
        assert L.GxB_Matrix_sort(C._carg, P._carg, _handle(L, name), A._carg, None) == -8, name  # GrB_NOT_IMPLEMENTED
        assert "not implemented" in _matrix_error(L, C), name
    assert L.GxB_Matrix_sort(None, P._carg, _handle(L, "GrB_LE_INT64"), A._carg, None) == -8
    assert "not implemented" in _matrix_error(L, P)  # (the text goes to the first output that is not NULL)
    # wrong shapes, with and without T0
    R = gb.Matrix.from_coo([0, 2, 2], [1, 4, 0], [1, 2, 0], nrows=3, ncols=5)
    assert L.GxB_Matrix_sort(C._carg, None, lt, R._carg, None) == -6  # GrB_DIMENSION_MISMATCH
    assert "7 x 7" in _matrix_error(L, C) and "3 x 5" in _matrix_error(L, C)
    assert L.GxB_Matrix_sort(None, gb.Matrix("UINT64", 5, 3)._carg, lt, R._carg, _handle(L, "GrB_DESC_T0")) == -6  # (the shape stays A's)
    D, Q = gb.Matrix(int, 3, 5), gb.Matrix("UINT64", 3, 5)
    assert L.GxB_Matrix_sort(D._carg, Q._carg, lt, R._carg, _handle(L, "GrB_DESC_T0")) == 0
    assert_coo(D, [0, 0, 0], [0, 1, 4], [0, 1, 2], "T0 values")
    assert_coo(Q, [0, 0, 0], [0, 1, 4], [2, 0, 2], "T0 row indices")
    assert L.GxB_Matrix_sort(D._carg, Q._carg, lt, R._carg, _handle(L, "GrB_DESC_RSCT1")) == 0  # (every other field is ignored)
    assert_coo(D, [0, 2, 2], [0, 0, 1], [1, 0, 2], "other descriptor fields")
    # C aliased to A; P aliased to A
    E = A.dup()
    assert L.GxB_Matrix_sort(E._carg, P._carg, lt, E._carg, None) == 0
    assert_coo(E, case["rows"], case["cols"], case["C"], "C is A")
    assert_coo(P, case["rows"], case["cols"], case["P"], "C is A: P")
    E = A.dup(dtype="UINT64")
    assert L.GxB_Matrix_sort(C._carg, E._carg, lt, E._carg, _handle(L, "GrB_DESC_T0")) == 0
    col = lit["cases"][1]
    assert_coo(C, col["rows"], col["cols"], col["C"], "P is A, columnwise: C")
    assert_coo(E, col["rows"], col["cols"], col["P"], "P is A, columnwise")
    # the vector form
    v = gb.Vector.from_coo([1, 3, 4, 6], [1, 1, 2, 0], size=7)
    w, p = gb.Vector(int, 7), gb.Vector("UINT64", 7)
    assert L.GxB_Vector_sort(w._carg, p._carg, lt, v._carg, None) == 0
    assert_vec(w, [0, 1, 2, 3], [0, 1, 1, 2], "vector w")
    assert_vec(p, [0, 1, 2, 3], [6, 1, 3, 4], "vector p")
    assert L.GxB_Vector_sort(None, None, lt, v._carg, None) == -2
    assert L.GxB_Vector_sort(w._carg, gb.Vector(float, 7)._carg, lt, v._carg, None) == -5
    assert L.GxB_Vector_sort(w._carg, None, _handle(L, "GrB_PLUS_INT64"), v._carg, None) == -5
    assert L.GxB_Vector_sort(w._carg, None, _handle(L, "GrB_GE_INT64"), v._carg, None) == -8
    assert L.GxB_Vector_sort(gb.Vector(int, 8)._carg, None, lt, v._carg, None) == -6
    u = v.dup()
    assert L.GxB_Vector_sort(u._carg, None, gt, u._carg, None) == 0  # (w is u)
    assert_vec(u, [0, 1, 2, 3], [2, 1, 1, 0], "w is u")
    # an empty input empties the outputs
    assert L.GxB_Matrix_sort(C._carg, P._carg, lt, gb.Matrix(int, 7, 7)._carg, None) == 0
    assert C.nvals == 0 and P.nvals == 0


def test_host(gb, literals):
    lit = literals["matrix"]
    A = gb.Matrix.from_coo(lit["rows"], lit["cols"], lit["vals"], nrows=7, ncols=7)
    v = gb.Vector.from_coo([1, 3, 4, 6], [1, 1, 2, 0], size=7)
    assert A.ss.sort(values=False, permutation=False) == (None, None)
    with pytest.raises(gb.exceptions.NotImplementedException, match="not implemented"):
        A.ss.sort(gb.binary.le)
    with pytest.raises(gb.exceptions.NotImplementedException):
        v.ss.sort("<=")
    with pytest.raises(gb.exceptions.DomainMismatch):
        A.ss.sort(gb.monoid.plus)  # (a monoid stands for its binary operator)
    with pytest.raises(TypeError):
        A.ss.sort(gb.semiring.min_plus)
    with pytest.raises(ValueError):
        A.ss.sort(order="diagonal")
    with pytest.raises(gb.exceptions.NotImplementedException):
        A.ss.compactify("first")
    with pytest.raises(TypeError):
        gb.Matrix.ss.sort()
    calls = []
    gb.record_calls(calls)
    try:
        assert A.ss.sort(values=False, permutation=False) == (None, None)
        assert calls == []  # (asking for neither output makes no call)
        A.ss.sort()
        A.ss.sort(">", "columnwise", values=False)
        v.ss.sort()
    finally:
        gb.record_calls(None)
    names = [c.split("(")[0] for c in calls if "sort" in c]
    assert names == ["GxB_Matrix_sort", "GxB_Matrix_sort", "GxB_Vector_sort"], calls
    assert "GrB_LT_INT64" in calls[[c.startswith("GxB_Matrix_sort") for c in calls].index(True)], calls


# ---- 7. no growth ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_growth():
    """50 sorts per cycle on one R-MAT matrix (all three paths), both outputs, one output, columnwise, compactify; results freed.  The
    library keeps freed blocks in its size-class cache, so the first cycle may grow; free device memory after cycle 2 against after cycle 3."""
    import torch

    from graphblas_amd import synthetic

    gb = bind("gpu")
    scale = 12
    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, device="cpu")
    A = gb.Matrix.from_csr(ip.numpy(), col.numpy().astype(np.int64), synthetic.edge_weights(col, scale).numpy(), dtype="FP32", ncols=n)
    A.ss.sort()
    wave_max, lds_max = limits()
    assert min(sort_last()) > 0 or int(np.diff(ip.numpy()).max()) <= lds_max

    def free_bytes():
        gb.Matrix(int, 1, 1).wait()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        for k in range(50):
            r = [A.ss.sort(), A.ss.sort(">", values=False), A.ss.sort("<", "columnwise", permutation=False), A.ss.compactify("largest", 8)][k % 4]
            del r

    cycle()
    cycle()
    after2 = free_bytes()
    cycle()
    after3 = free_bytes()
    print(f"free after cycle 2: {after2 / 2**20:.1f} MiB, after cycle 3: {after3 / 2**20:.1f} MiB")
    assert after3 >= after2, (after2, after3)
