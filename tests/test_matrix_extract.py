"""Matrix extract: ``A[I, J]`` (GrB_Matrix_extract), ``A[i, J]`` / ``A[I, j]`` (GrB_Col_extract) and ``A[i, j]`` (GrB_Matrix_extractElement_<T>)
-- the kernels of grb_extract.hip on the GPU tier, the same sources under the SIMT emulator on the CPU tier.  Extract only moves and casts
values: every comparison is bit for bit.

1. the reference's own literals (tests/golden/extract_literals.json) through every spelling;
2. seeded random parity against an expectation computed HERE with numpy on the COO tuples (a stable argsort of J + searchsorted for the
   column map, a row loop for I, then the dense restatement of the write rule of tests/test_select.py), and against scipy;
3. the limits of the kernel: matrices built row by row from sorted column lists, so that units, methods and counts are known exactly;
4. GrB_Col_extract and the element forms;
5. the C ABI's errors through ctypes: the output stays bit for bit as it was;
6. (GPU tier) R-MAT scale 16 against scipy, and no growth of device memory.

Not testable at a small size: the GrB_NOT_IMPLEMENTED answer of method 12 for a result of 2^32 or more entries (its sort payload is 32 bits)."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.backend import DEVICES, ROOT, bind
from tests.test_select import NP_OF, OTHER_TYPE, TYPES, assert_coo, assert_vec, draw_coo, draw_matrix, np_write_rule, stored_iso
from tests.values import rand_vals, same_fp

UNIT = 8192  # entries of a unit (EXT_UNIT of grb_extract.hip)
CT_OF = {"BOOL": ctypes.c_bool, "INT8": ctypes.c_int8, "INT16": ctypes.c_int16, "INT32": ctypes.c_int32, "INT64": ctypes.c_int64,
         "UINT8": ctypes.c_uint8, "UINT16": ctypes.c_uint16, "UINT32": ctypes.c_uint32, "UINT64": ctypes.c_uint64, "FP32": ctypes.c_float,
         "FP64": ctypes.c_double}


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


@pytest.fixture(scope="module")
def literals():
    with open(os.path.join(ROOT, "tests", "golden", "extract_literals.json")) as f:
        return json.load(f)


def stats():
    from graphblas_amd import device

    return device.last_stats()


# ---- the numpy restatement -----------------------------------------------------------------------------------------------------
def np_extract(m, rows, cols, vals, I, J):
    """T(i', j') = A(I[i'], J[j']) on COO tuples sorted row-major.  Returns (rows, cols, vals) row-major with sorted columns."""
    I, J = np.asarray(I, np.int64), np.asarray(J, np.int64)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
    order = np.argsort(J, kind="stable")
    sJ = J[order]
    out_r, out_c, out_v = [], [], []
    for ip, i in enumerate(I):
        cs, vs = cols[indptr[i]:indptr[i + 1]], vals[indptr[i]:indptr[i + 1]]
        lb, ub = np.searchsorted(sJ, cs, "left"), np.searchsorted(sJ, cs, "right")
        mult = ub - lb
        t = np.repeat(lb, mult) + (np.arange(int(mult.sum())) - np.repeat(np.cumsum(mult) - mult, mult))
        jp, v = order[t], np.repeat(vs, mult)
        by_col = np.argsort(jp, kind="stable")
        out_r.append(np.full(jp.size, ip, np.int64))
        out_c.append(jp[by_col])
        out_v.append(v[by_col])
    if not out_r:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), vals[:0]
    return np.concatenate(out_r), np.concatenate(out_c), np.concatenate(out_v)


def np_units(m, n, rows, cols, I, J, size):
    """(method, units) the kernel must report: J None = GrB_ALL.  Units: every selected row's entries inside [min J, max J], in chunks of UNIT."""
    if I is not None and len(I) == 0 or J is not None and len(J) == 0 or rows.size == 0:
        return 6, 0
    if I is None and J is None:
        return 6, 0
    Iv = np.arange(m) if I is None else np.asarray(I, np.int64)
    lo, hi = (0, n - 1) if J is None else (int(np.min(J)), int(np.max(J)))
    inside = (cols >= lo) & (cols <= hi)
    per_row = np.bincount(rows[inside], minlength=m)[Iv]
    units, E = int(((per_row + UNIT - 1) // UNIT).sum()), int(per_row.sum())
    Jv = None if J is None else np.asarray(J, np.int64)
    if Jv is None or np.array_equal(Jv, Jv[0] + np.arange(Jv.size)):
        return 9, units
    if np.all(np.diff(Jv) > 0):
        return (10 if 4 * n <= (4 + size) * E else 11), units
    return 12, units


def from_rows(gb, rowcols, n, tname, rng=None, vals=None):
    """A matrix built row by row from sorted column lists; returns (A, rows, cols, vals)."""
    m = len(rowcols)
    deg = np.array([len(c) for c in rowcols], np.int64)
    rows = np.repeat(np.arange(m), deg)
    cols = np.concatenate([np.asarray(c, np.int64) for c in rowcols]) if deg.sum() else np.zeros(0, np.int64)
    if vals is None:
        vals = rand_vals(rng, rows.size, tname)
    indptr = np.concatenate([[0], np.cumsum(deg)])
    A = gb.Matrix.from_csr(indptr, cols, vals, dtype=tname, ncols=n) if rows.size else gb.Matrix(tname, m, n)
    assert A.shape == (m, n) and A.nvals == rows.size
    return A, rows, cols, vals


def same_matrix(C, er, ec, ev, where=""):
    I, J, X = C.to_coo()
    assert I.tolist() == np.asarray(er).tolist() and J.tolist() == np.asarray(ec).tolist(), where
    assert X.dtype == ev.dtype, where
    if ev.dtype.kind == "f":
        same_fp(X, ev, None, where)
    else:
        assert X.tolist() == ev.tolist(), where


def sel(key):
    return slice(None) if key is None else (key if isinstance(key, slice) else list(map(int, key)))


def check_extract(gb, A, m, n, rows, cols, vals, I, J, tname, where="", method=None):
    """A[I, J].new() against the restatement, with the method and the units the kernel must report."""
    Iv = np.arange(m) if I is None else np.asarray(I, np.int64)
    Jv = np.arange(n) if J is None else np.asarray(J, np.int64)
    C = A[sel(I), sel(J)].new()
    st = stats()
    assert C.shape == (Iv.size, Jv.size) and C.dtype == A.dtype, where
    er, ec, ev = np_extract(m, rows, cols, vals, Iv, Jv)
    same_matrix(C, er, ec, ev, where)
    want_method, want_units = np_units(m, n, rows, cols, I, J, NP_OF[tname]().itemsize)
    if method is not None:
        assert want_method == method, (where, want_method, method)
    assert (st["method"], st["tiles"], st["out_nvals"]) == (want_method, want_units, er.size), (where, st)
    assert st["kernel_launches"] > 0 or want_method == 6, (where, st)
    return C


# ---- 1. the reference's literals ------------------------------------------------------------------------------------------------
def lit_matrix(gb, literals, dtype=None):
    lit = literals["matrix"]
    return gb.Matrix.from_coo(lit["rows"], lit["cols"], lit["vals"], nrows=lit["nrows"], ncols=lit["ncols"], dtype=dtype)


def test_literal_values(gb, literals):
    lit = literals["matrix"]
    A = lit_matrix(gb, literals)
    assert_coo(A, lit["sorted_rows"], lit["sorted_cols"], lit["sorted_vals"], lit["source"])
    r, c, x = A.T.new().to_coo()
    assert_coo(A, c, r, x, "A.T")


def test_literal_extract(gb, literals):
    lit = literals["extract"]
    A = lit_matrix(gb, literals)
    I, J = lit["I"], lit["J"]
    si, sj, sjs = slice(*lit["I_slice"]), slice(*lit["J_slice"]), slice(*lit["J_slice_step"])
    spellings = [(I, J), (si, sj), (I, sjs), (np.array(I), np.array(J)), (np.array(I, np.uint64), J), (I, np.array(J, np.int32)), (si, J)]
    for k, (ki, kj) in enumerate(spellings):
        where = (lit["source"], k)
        C = gb.Matrix(A.dtype, lit["nrows"], lit["ncols"])
        C << A[ki, kj]
        assert_coo(C, lit["rows"], lit["cols"], lit["vals"], where)
        assert_coo(A[ki, kj].new(), lit["rows"], lit["cols"], lit["vals"], where)
        F = A[ki, kj].new(dtype=float)
        assert F.dtype == "FP64"
        assert_coo(F, lit["rows"], lit["cols"], [float(v) for v in lit["vals"]], where)
        # A.T[J, I] is the transpose of A[I, J]
        assert_coo(A.T[kj, ki].new(), lit["cols"], lit["rows"], lit["vals"], where)
        D = gb.Matrix(A.dtype, lit["ncols"], lit["nrows"])
        D << A.T[kj, ki]
        assert_coo(D, lit["cols"], lit["rows"], lit["vals"], where)
    # the updater forms
    C = gb.Matrix.from_coo([0, 1], [0, 0], [10, 20], nrows=3, ncols=4)
    C(accum=gb.binary.plus) << A[I, J]
    assert_coo(C, [0, 0, 1, 1, 2, 2, 2], [0, 2, 0, 1, 1, 2, 3], [12, 3, 20, 3, 5, 7, 3], "accum")
    M = gb.Matrix.from_coo([0, 2, 1], [2, 3, 0], [1, 1, 1], nrows=3, ncols=4)
    C(M.S, replace=True) << A[I, J]
    assert_coo(C, [0, 2], [2, 3], [3, 3], "mask, replace")
    assert_coo(A[I, J].new(mask=~M.S), [0, 1, 2, 2], [0, 1, 1, 2], [2, 3, 5, 7], ".new(mask=)")
    assert_coo(A[:, :].new(), literals["matrix"]["rows"], literals["matrix"]["cols"], literals["matrix"]["vals"], "[:, :]")
    assert not hasattr(gb.Matrix, "__setitem__") and not hasattr(gb.Matrix, "__delitem__")


def test_literal_row_and_column(gb, literals):
    A = lit_matrix(gb, literals)
    row, col = literals["extract_row"], literals["extract_column"]
    J, i = row["J"], row["row"]
    for k, expr in enumerate([lambda: A[i, J], lambda: A[i, slice(*row["J_slice"])], lambda: A.T[J, i], lambda: A[i, np.array(J)],
                              lambda: A.T[np.array(J), i]]):
        w = gb.Vector(A.dtype, row["size"])
        w << expr()
        assert_vec(w, row["idx"], row["vals"], (row["source"], k))
        assert_vec(expr().new(), row["idx"], row["vals"], (row["source"], k))
        f = expr().new(dtype=float)
        assert f.dtype == "FP64"
        assert_vec(f, row["idx"], [float(v) for v in row["vals"]], (row["source"], k))
    I, j = col["I"], col["col"]
    for k, expr in enumerate([lambda: A[I, j], lambda: A[slice(*col["I_slice"]), j], lambda: A.T[j, I], lambda: A[np.array(I), j]]):
        w = gb.Vector(A.dtype, col["size"])
        w << expr()
        assert_vec(w, col["idx"], col["vals"], (col["source"], k))
        assert_vec(expr().new(), col["idx"], col["vals"], (col["source"], k))
    # whole rows and columns (tests/test_matrix.py:35-43, the picture of A)
    assert_vec(A[6, :].new(), [2, 3, 4], [5, 7, 3], "A[6, :]")
    assert_vec(A[:, 2].new(), [3, 5, 6], [3, 1, 5], "A[:, 2]")
    assert_vec(A.T[:, 6].new(), [2, 3, 4], [5, 7, 3], "A.T[:, 6]")
    assert_vec(A.T[2, :].new(), [3, 5, 6], [3, 1, 5], "A.T[2, :]")
    assert_vec(A[-1, [0, -5, 4]].new(), row["idx"], row["vals"], "negative indices")


def test_literal_type_errors(gb, literals):
    A = lit_matrix(gb, literals)
    with pytest.raises(TypeError):  # tests/test_matrix.py:453-455: a list, not a tuple
        A[6, (0, 2, 4)]
    with pytest.raises(TypeError, match="Invalid dtype"):  # :458-459
        A[6, np.array([0, 2, 4], dtype=float)]
    with pytest.raises(TypeError, match="Invalid number of dimensions"):  # :460-461
        A[6, np.array([[0, 2, 4]])]
    with pytest.raises(TypeError, match="Invalid type for index"):  # :598-604 (test_extract_with_matrix)
        A[A.T, 1].new()
    with pytest.raises(TypeError, match="Invalid type for index"):
        A[A, [1]].new()
    with pytest.raises(TypeError, match="Invalid type for index"):
        A[[0], A.V].new()
    with pytest.raises(TypeError, match="Invalid type for index"):
        A[gb.Vector(int, 3), 1]
    with pytest.raises(TypeError):
        A[3]
    with pytest.raises(TypeError):
        A[1.0, 2]
    with pytest.raises(IndexError):
        A[7, 0]
    with pytest.raises(IndexError):
        A[[0], -8]
    with pytest.raises(gb.exceptions.IndexOutOfBound):
        A[[0, 7], [1]].new()
    with pytest.raises(gb.exceptions.DimensionMismatch):
        gb.Matrix(int, 2, 2) << A[[0, 1, 2], [1, 2]]
    with pytest.raises(TypeError):
        gb.Vector(int, 3) << A[[0, 1, 2], [1, 2, 3]]


def test_literal_element(gb, literals):
    lit = literals["extract_element"]
    A = lit_matrix(gb, literals)
    for case in lit["cases"]:
        expr = A.T[case["i"], case["j"]] if case["transposed"] else A[case["i"], case["j"]]
        s = expr.new()
        assert s.dtype == "INT64" and s.value == case["value"], case
        assert (expr == case["value"]) if case["value"] is not None else expr.new().is_empty, case
        assert expr.value == case["value"]
    f = lit["as_float"]
    s = A[f["i"], f["j"]].new(dtype=float)
    assert s.value == f["value"] and isinstance(s.value, float) and s.dtype == f["dtype"]
    assert A[-4, 0] == 3 and A[-4, -7] == 3


# ---- 2. seeded random parity ----------------------------------------------------------------------------------------------------
def draw_list(rng, kind, dim):
    """An index list over [0, dim): None = GrB_ALL."""
    if kind == 0:
        return None
    if kind == 1:  # a run
        lo = int(rng.integers(0, dim))
        return np.arange(lo, int(rng.integers(lo, dim)) + 1)
    if kind == 2:  # strictly increasing
        return np.flatnonzero(rng.random(dim) < 0.5) if dim > 1 else np.array([0])
    if kind == 3:  # shuffled, with duplicates
        return rng.integers(0, dim, int(rng.integers(1, dim + 40)))
    if kind == 4:  # a permutation
        return rng.permutation(dim)
    return np.zeros(0, np.int64)


@pytest.mark.parametrize("seed", range(21))
def test_extract_random(gb, seed):
    """Per seed 6 configurations: I and J each GrB_ALL / a run / increasing / shuffled with duplicates / a permutation / empty; T0; mask in
    {none, value, structural}, complement, replace, accum in {none, plus, min} (their full cross product: test_extract_write_rule); an output
    type that differs from the input's; C as its own mask (C aliasing A: test_extract_alias); empty, 1 x n, n x 1 matrices, the hub row, iso
    input.  No case is skipped."""
    rng = np.random.default_rng(9100 + seed)
    tname = TYPES[seed % 7]
    m, n, rows, cols, vals, iso = draw_matrix(rng, seed, tname)
    if iso:
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
        A = gb.Matrix.ss.import_csr(nrows=m, ncols=n, indptr=indptr, values=vals[:1], col_indices=cols, is_iso=True, sorted_cols=True, dtype=tname)
        assert stored_iso(A)
    else:
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
    compared = 0
    for k in range(6):
        cfg = seed * 6 + k
        t0 = (cfg // 5) % 2 == 1
        mask_kind, comp, repl = cfg % 3, (cfg // 3) % 2 == 1, (cfg // 6) % 2 == 1
        accum = [None, "plus", "min"][(cfg // 2) % 3]
        sm, sn = (n, m) if t0 else (m, n)
        if t0:
            o = np.lexsort((rows, cols))
            sr, sc, sv = cols[o], rows[o], vals[o]
        else:
            sr, sc, sv = rows, cols, vals
        alias_mask = cfg % 11 == 3
        ikind, jkind = (cfg // 2) % 6, (cfg + seed // 3) % 6
        I, J = draw_list(rng, ikind, sm), draw_list(rng, jkind, sn)
        Iv, Jv = (np.arange(sm) if I is None else I), (np.arange(sn) if J is None else J)
        om, on = Iv.size, Jv.size
        ctype = OTHER_TYPE[tname] if cfg % 5 == 1 else tname
        tr, tc, tv = np_extract(sm, sr, sc, sv, Iv, Jv)
        with np.errstate(all="ignore"):
            T = (tr, tc, tv.astype(NP_OF[ctype]))
        none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, NP_OF[ctype]))
        Cc = (draw_coo(rng, om, on, ctype, 0.3) if om * on else none) if (accum or mask_kind or alias_mask) else None
        C = gb.Matrix.from_coo(*Cc, dtype=ctype, nrows=om, ncols=on) if Cc is not None else gb.Matrix(ctype, om, on)
        Mc, kw = None, {}
        if alias_mask:
            mask_kind = 1 + cfg % 2
            Mc = Cc
            mm = C.S if mask_kind == 2 else C.V
            kw = dict(mask=~mm if comp else mm, replace=repl)
        elif mask_kind:
            Mc = draw_coo(rng, om, on, "INT8", 0.5) if om * on else (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int8))
            M = gb.Matrix.from_coo(*Mc, dtype="INT8", nrows=om, ncols=on)
            mm = M.S if mask_kind == 2 else M.V
            kw = dict(mask=~mm if comp else mm, replace=repl)
        if accum:
            kw["accum"] = accum
        C(**kw) << (A.T if t0 else A)[sel(I), sel(J)]
        st = stats()
        er, ec, ev = np_write_rule((om, on), ctype, Cc, T, Mc, mask_kind == 2, comp and mask_kind > 0, repl and mask_kind > 0, accum)
        where = (f"seed {seed}.{k} {tname}->{ctype} {m}x{n} I kind {ikind} J kind {jkind} t0={t0} mask={mask_kind} comp={comp} repl={repl} "
                 f"accum={accum} alias_mask={alias_mask} iso={iso}")
        Ig, Jg, X = C.to_coo()
        assert Ig.tolist() == er.tolist() and Jg.tolist() == ec.tolist(), where
        assert X.dtype == ev.dtype, where
        if ev.dtype.kind == "f":
            same_fp(X, ev, "min" if accum == "min" else None, where)
        else:
            assert X.tolist() == ev.tolist(), where
        want_method, want_units = np_units(sm, sn, sr, sc, I, J, NP_OF[tname]().itemsize)
        assert (st["method"], st["tiles"], st["out_nvals"]) == (want_method, want_units, tr.size), (where, st)
        if iso and not kw and tr.size and ctype == tname:
            assert stored_iso(C), where  # an iso input keeps one value unless the write rule needs one per entry
        compared += 1
    assert compared == 6


def same_coo_values(C, er, ec, ev, accum, where):
    Ig, Jg, X = C.to_coo()
    assert Ig.tolist() == er.tolist() and Jg.tolist() == ec.tolist(), where
    assert X.dtype == ev.dtype, where
    if ev.dtype.kind == "f":
        same_fp(X, ev, "min" if accum == "min" else None, where)
    else:
        assert X.tolist() == ev.tolist(), where


@pytest.mark.parametrize("jkind,tname", [(2, "INT32"), (3, "FP64")])
def test_extract_write_rule(gb, jkind, tname):
    """Every mask kind x complement x replace x accumulator on the matrix form: the 3 combinations without a mask and the 2 x 2 x 2 x 3 with
    one, on an increasing J and on a shuffled J with duplicates, against the dense restatement of the write rule."""
    rng = np.random.default_rng(9500 + jkind)
    m, n = 70, 90
    rowcols = [np.sort(rng.choice(n, int(rng.integers(0, 30)), replace=False)) for _ in range(m)]
    vals = rand_vals(rng, sum(len(c) for c in rowcols), tname, "exact") if tname.startswith("FP") else None
    A, rows, cols, vals = from_rows(gb, rowcols, n, tname, rng, vals=vals)
    I = rng.integers(0, m, 50)  # (shuffled, with repeats)
    J = draw_list(rng, 2, n) if jkind == 2 else rng.integers(0, n, 100)
    om, on = I.size, J.size
    T = np_extract(m, rows, cols, vals, I, J)
    assert T[0].size > 50
    seen = set()
    for mask_kind in (0, 1, 2):
        for comp in (False, True):
            for repl in (False, True):
                for accum in (None, "plus", "min"):
                    if not mask_kind and (comp or repl):
                        continue
                    Cc = draw_coo(rng, om, on, tname, 0.3)
                    C = gb.Matrix.from_coo(*Cc, dtype=tname, nrows=om, ncols=on)
                    Mc, kw = None, {}
                    if mask_kind:
                        Mc = draw_coo(rng, om, on, "INT8", 0.5)
                        M = gb.Matrix.from_coo(*Mc, dtype="INT8", nrows=om, ncols=on)
                        mm = M.S if mask_kind == 2 else M.V
                        kw = dict(mask=~mm if comp else mm, replace=repl)
                    if accum:
                        kw["accum"] = accum
                    C(**kw) << A[sel(I), sel(J)]
                    assert stats()["method"] in ((10, 11) if jkind == 2 else (12,))
                    er, ec, ev = np_write_rule((om, on), tname, Cc, T, Mc, mask_kind == 2, comp, repl, accum)
                    same_coo_values(C, er, ec, ev, accum, (jkind, mask_kind, comp, repl, accum))
                    seen.add((mask_kind, comp, repl, accum))
    assert len(seen) == 27


@pytest.mark.parametrize("t0", [False, True])
def test_extract_alias(gb, t0):
    """C is A: ``A(...) << A[I, J]`` on a square A with I, J permutations or GrB_ALL, without and with T0 -- T is then read from the transpose
    cached ON A, which the call has to drop before it writes --, plain, accumulated, under another matrix's mask and under A itself as the
    mask (C, A and the mask one object).  Afterwards A's transpose is the transpose of the new content."""
    rng = np.random.default_rng(9600 + t0)
    n = 130
    deg = rng.integers(0, 9, n)
    deg[7] = 100
    rows = np.repeat(np.arange(n), deg)
    cols = np.concatenate([np.sort(rng.choice(n, d, replace=False)) for d in deg])
    vals = rand_vals(rng, rows.size, "INT64")
    assert (vals == 0).any() and (vals != 0).any()  # (a valued mask of A's own values lets some entries through and stops others)
    o = np.lexsort((rows, cols))
    sr, sc, sv = (cols[o], rows[o], vals[o]) if t0 else (rows, cols, vals)
    Mc = draw_coo(rng, n, n, "INT8", 0.5)
    M = gb.Matrix.from_coo(*Mc, dtype="INT8", nrows=n, ncols=n)
    own = (rows, cols, vals)
    variants = {"plain": ({}, None, False, False, False, None),
                "accum": (dict(accum="plus"), None, False, False, False, "plus"),
                "mask": (dict(mask=M.V), Mc, False, False, False, None),
                "mask, replace, accum": (dict(mask=~M.S, replace=True, accum="min"), Mc, True, True, True, "min"),
                "own structure": (None, own, True, False, False, None),
                "own values, complemented, replace": (None, own, False, True, True, None)}
    runs = 0
    for ikind, jkind in ((4, 0), (0, 4), (4, 4), (2, 0)):
        for name, (kw, mc, structural, comp, repl, accum) in variants.items():
            A = gb.Matrix.from_coo(rows, cols, vals, dtype="INT64", nrows=n, ncols=n)
            if t0:
                A.T.new()  # (the transpose is cached on A before the call)
            if kw is None:
                mm = A.S if structural else A.V
                kw = dict(mask=~mm if comp else mm, replace=repl)
            I, J = draw_list(rng, ikind, n), draw_list(rng, jkind, n)
            if ikind == 2:  # a list of n rows with repeats: C keeps A's shape
                I = np.sort(rng.integers(0, n, n))
            T = np_extract(n, sr, sc, sv, np.arange(n) if I is None else I, np.arange(n) if J is None else J)
            A(**kw) << (A.T if t0 else A)[sel(I), sel(J)]
            assert stats()["method"] in (9, 12), name
            er, ec, ev = np_write_rule((n, n), "INT64", own, T, mc, structural, comp, repl, accum)
            where = (t0, ikind, jkind, name)
            same_coo_values(A, er, ec, ev, accum, where)
            tr, tc, tx = A.T.new().to_coo()
            o2 = np.lexsort((er, ec))
            assert tr.tolist() == ec[o2].tolist() and tc.tolist() == er[o2].tolist() and tx.tolist() == ev[o2].tolist(), where
            runs += 1
    assert runs == 24


@pytest.mark.parametrize("seed", range(6))
def test_extract_against_scipy(gb, seed):
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(9300 + seed)
    tname = ["INT64", "FP64", "INT32"][seed % 3]
    m, n, rows, cols, vals, _ = draw_matrix(rng, 3 + seed, tname)  # (the ragged shapes and the hub)
    vals = rng.integers(1, 100, rows.size).astype(NP_OF[tname])  # (no explicit zeros: scipy would keep them, but sums of duplicates must not cancel)
    A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
    G = sp.csr_matrix((vals, (rows, cols)), shape=(m, n))
    for ikind, jkind in ((3, 3), (2, 2), (3, 1), (4, 4), (1, 3)):
        I, J = draw_list(rng, ikind, m), draw_list(rng, jkind, n)
        ref = G[I][:, J].tocsr()
        ref.sort_indices()
        Cp, Cj, Cx = A[list(map(int, I)), list(map(int, J))].new().to_csr()
        where = (seed, ikind, jkind)
        if ref.nnz == 0:
            assert Cj.size == 0, where
            continue
        assert np.array_equal(Cp.astype(np.int64), ref.indptr) and np.array_equal(Cj.astype(np.int64), ref.indices), where
        assert np.array_equal(Cx, ref.data), where


# ---- 3. the limits of the kernel --------------------------------------------------------------------------------------------------
ROW_LENGTHS = [0, 1, 63, 64, 65, 127, 128, 129]


def test_limits_short_rows(gb):
    """Source rows of 0 .. 129 entries: every J class, I repeated / reversed / of empty rows only / of one row."""
    rng = np.random.default_rng(1)
    n = 300
    rowcols = [np.sort(rng.choice(n, k, replace=False)) for k in ROW_LENGTHS] + [np.zeros(0, np.int64)]
    m = len(rowcols)
    A, rows, cols, vals = from_rows(gb, rowcols, n, "INT32", rng)
    inc = np.unique(np.concatenate([[0, n - 1], np.flatnonzero(rng.random(n) < 0.4)]))
    shuffled = rng.integers(0, n, 333)
    for Jname, J in (("all", None), ("run", np.arange(17, 211)), ("increasing", inc), ("shuffled", shuffled), ("reversed", np.arange(n)[::-1])):
        for Iname, I in (("all", None), ("3 times", [4, 2, 4, 7, 4]), ("reversed", np.arange(m)[::-1]), ("empty rows only", [0, 8, 0]), ("one row", [5])):
            if I is None and J is None:
                continue
            check_extract(gb, A, m, n, rows, cols, vals, I, J, "INT32", (Jname, Iname))


@pytest.mark.parametrize("k,n", [(8192, 16385), (8193, 16385), (16384, 32769), (16385, 32769)])
def test_limits_long_rows(gb, k, n):
    """A source row of k entries beside short ones: the unit cuts of method 9's segments and of the source chunks of methods 10 - 12."""
    rng = np.random.default_rng(k)
    long_row = np.sort(rng.choice(n - 2, k - 2, replace=False) + 1)
    long_row = np.concatenate([[0], long_row, [n - 1]])  # (column 0 and column ncols - 1 hold entries)
    rowcols = [np.array([5, n - 1]), long_row, np.zeros(0, np.int64), np.array([0])]
    A, rows, cols, vals = from_rows(gb, rowcols, n, "FP32", rng)
    m = len(rowcols)
    I = [1, 3, 1, 0, 2]
    check_extract(gb, A, m, n, rows, cols, vals, I, None, "FP32", "all", method=9)
    assert stats()["tiles"] == 2 * -(-k // UNIT) + 2
    check_extract(gb, A, m, n, rows, cols, vals, I, np.arange(0, n), "FP32", "a run over every column", method=9)
    inc = np.unique(np.concatenate([[0, n - 1], long_row[::3], np.flatnonzero(rng.random(n) < 0.1)]))
    check_extract(gb, A, m, n, rows, cols, vals, I, inc, "FP32", "increasing", method=10)
    few = np.array([0, long_row[k // 2], n - 1])
    check_extract(gb, A, m, n, rows, cols, vals, [3, 0], few, "FP32", "increasing, search", method=11)
    check_extract(gb, A, m, n, rows, cols, vals, [1], rng.permutation(n)[: n // 2], "FP32", "shuffled", method=12)


def test_limits_runs(gb):
    """A run whose ends fall on a row's first / last entry, on lanes 63 / 64 of a chunk, one before and one after an entry; a run that selects
    nothing; columns 0 and ncols - 1."""
    n = 1000
    base = np.arange(100, 900, 4)  # 200 entries: entry 63 is column 352, entry 64 column 356
    rowcols = [base, np.array([0, n - 1]), np.zeros(0, np.int64), np.arange(n)]
    A, rows, cols, vals = from_rows(gb, rowcols, n, "INT64", np.random.default_rng(2))
    m = len(rowcols)
    ends = [100, 99, 101, 896, 895, 897, 352, 356, 351, 353, 355, 357, 0, n - 1]
    for lo in ends:
        for hi in ends:
            if lo <= hi:
                check_extract(gb, A, m, n, rows, cols, vals, [0, 1, 2, 3, 0], np.arange(lo, hi + 1), "INT64", ("run", lo, hi), method=9)
    # selects nothing from any row: a T without entries
    C = check_extract(gb, A, m, n, rows, cols, vals, [0, 1, 2], np.arange(897, 999), "INT64", "nothing", method=9)
    assert C.nvals == 0 and stats()["tiles"] == 0
    C = check_extract(gb, A, m, n, rows, cols, vals, [0, 2], np.array([101, 102, 103, 897]), "INT64", "nothing, increasing", method=11)
    assert C.nvals == 0
    C = check_extract(gb, A, m, n, rows, cols, vals, [0, 2], np.array([103, 101, 101]), "INT64", "nothing, shuffled", method=12)
    assert C.nvals == 0


@pytest.mark.parametrize("nj", [1, 64, 65, 4097])
def test_limits_increasing(gb, nj):
    n = 8200
    rng = np.random.default_rng(nj)
    rowcols = [np.arange(n), np.sort(rng.choice(n, 130, replace=False)), np.zeros(0, np.int64), np.arange(0, n, 2)]
    A, rows, cols, vals = from_rows(gb, rowcols, n, "UINT16", rng)
    J = np.array([n - 1]) if nj == 1 else np.unique(np.concatenate([[0, n - 1], rng.choice(np.arange(1, n - 1), nj - 2, replace=False)]))
    assert J.size == nj
    for I in ([0], [3, 1, 2, 0, 0], None):
        check_extract(gb, A, 4, n, rows, cols, vals, I, J, "UINT16", (nj, I))
    # (a list of one column is a run)
    assert nj > 1 or stats()["method"] == 9


def test_limits_table_or_search(gb):
    """The table is taken when 4 ncols <= (4 + sizeof T) E: both sides of the boundary by one entry of E, and the same J under BOOL and FP64."""
    n = 300  # FP64: 4 * 300 = 12 * E at E = 100
    J = np.unique(np.concatenate([np.arange(0, n, 2), [n - 1]]))  # (increasing, not a run, spans every column: nothing is narrowed away)
    rng = np.random.default_rng(3)
    results = {}
    for E in (99, 100, 101):
        rowcols = [np.sort(rng.choice(n, 60, replace=False)), np.sort(rng.choice(n, E - 60, replace=False)), np.arange(n)]
        fv = rng.integers(1, 9, E + n).astype(np.float64)
        for tname in ("FP64", "BOOL"):
            A, rows, cols, vals = from_rows(gb, rowcols, n, tname, vals=fv.astype(NP_OF[tname]))
            want = 10 if (tname == "FP64" and E >= 100) else 11
            C = check_extract(gb, A, 3, n, rows, cols, vals, [1, 0], J, tname, (E, tname), method=want)
            results[E, tname] = C.to_coo()
        # methods 10 and 11 give the identical pattern (the values differ only by the cast to BOOL)
        (r1, c1, x1), (r2, c2, x2) = results[E, "FP64"], results[E, "BOOL"]
        assert r1.tolist() == r2.tolist() and c1.tolist() == c2.tolist() and (x1 != 0).tolist() == x2.tolist()
    # ... and on one matrix: the rows [1, 0] hold 99 entries (search); with the full third row 399 (table)
    rowcols = [np.sort(rng.choice(n, 60, replace=False)), np.sort(rng.choice(n, 39, replace=False)), np.arange(n)]
    A, rows, cols, vals = from_rows(gb, rowcols, n, "FP64", rng)
    a = check_extract(gb, A, 3, n, rows, cols, vals, [1, 0, 2], J, "FP64", "table", method=10).to_coo()
    b = check_extract(gb, A, 3, n, rows, cols, vals, [1, 0], J, "FP64", "search", method=11).to_coo()
    first = a[0] < 2
    assert a[0][first].tolist() == b[0].tolist() and a[1][first].tolist() == b[1].tolist() and a[2][first].tolist() == b[2].tolist()


@pytest.mark.parametrize("ni", [1, 255, 256, 257])
def test_limits_row_counts(gb, ni):
    rng = np.random.default_rng(ni)
    m, n = 40, 90
    rowcols = [np.sort(rng.choice(n, int(rng.integers(0, 12)), replace=False)) for _ in range(m)]
    A, rows, cols, vals = from_rows(gb, rowcols, n, "INT8", rng)
    I = rng.integers(0, m, ni)
    for J in (None, np.arange(3, 80), np.arange(0, n, 3), rng.integers(0, n, 100)):
        check_extract(gb, A, m, n, rows, cols, vals, I, J, "INT8", (ni,))


def test_limits_duplicates(gb):
    """Method 12: one column 64 / 65 times (a run of duplicates across a block of 64 emits), J reversed, J a permutation of all columns of an
    8193-entry row, I and J both shuffled with duplicates."""
    rng = np.random.default_rng(4)
    n = 8193
    rowcols = [np.arange(n), np.array([7, 9, 4000]), np.zeros(0, np.int64), np.sort(rng.choice(n, 200, replace=False))]
    A, rows, cols, vals = from_rows(gb, rowcols, n, "INT64", rng)
    for reps in (64, 65):
        J = np.concatenate([[9], np.full(reps, 7), [4000, 8], np.full(reps, 4000)])
        check_extract(gb, A, 4, n, rows, cols, vals, [1, 0, 1, 3], J, "INT64", ("repeats", reps), method=12)
        check_extract(gb, A, 4, n, rows, cols, vals, [1], rng.permutation(J), "INT64", ("repeats, shuffled", reps), method=12)
    check_extract(gb, A, 4, n, rows, cols, vals, [0, 3], np.arange(n)[::-1], "INT64", "reversed", method=12)
    check_extract(gb, A, 4, n, rows, cols, vals, [0], rng.permutation(n), "INT64", "permutation of an 8193-entry row", method=12)
    check_extract(gb, A, 4, n, rows, cols, vals, rng.integers(0, 4, 9), rng.integers(0, n, 3000), "INT64", "both shuffled", method=12)


def test_short_cuts(gb):
    rng = np.random.default_rng(5)
    n = 50
    rowcols = [np.sort(rng.choice(n, 9, replace=False)) for _ in range(6)]
    A, rows, cols, vals = from_rows(gb, rowcols, n, "INT32", rng)
    for I, J in (([], None), ([], [1, 2]), (None, []), ([3, 3], []), ([], [])):
        C = check_extract(gb, A, 6, n, rows, cols, vals, I, J, "INT32", (I, J), method=6)
        assert C.nvals == 0
    Z = gb.Matrix("INT32", 6, n)
    none = (np.zeros(0, np.int64),) * 2 + (np.zeros(0, np.int32),)
    check_extract(gb, Z, 6, n, *none, [1, 5, 1], [4, 2], "INT32", "empty A", method=6)
    check_extract(gb, Z, 6, n, *none, None, None, "INT32", "empty A, all x all", method=6)
    F = A[:, :].new(dtype="FP64")  # ALL x ALL into another type: a cast copy
    assert stats()["method"] == 6 and stats()["out_nvals"] == rows.size
    same_matrix(F, rows, cols, vals.astype(np.float64), "all x all, cast")
    G = gb.Matrix("INT32", 6, n)
    G(accum="plus") << A[:, :]
    assert stats()["method"] == 6
    same_matrix(G, rows, cols, vals, "all x all, accum")


# ---- 4. GrB_Col_extract and elements --------------------------------------------------------------------------------------------
def dense_of(m, n, rows, cols, vals):
    has, val = np.zeros((m, n), bool), np.zeros((m, n), vals.dtype)
    has[rows, cols], val[rows, cols] = True, vals
    return has, val


def same_vector(w, has, val, where=""):
    I, X = w.to_coo()
    assert I.tolist() == np.flatnonzero(has).tolist(), where
    assert X.dtype == val.dtype and X.tolist() == val[has].tolist(), where


@pytest.mark.parametrize("k", [0, 1, 64, 65, 8193])
def test_row_extract(gb, k):
    """A[i, J] for a row of k entries: J with duplicates and out of order, a slice, all; A.T[J, i] is the same call."""
    rng = np.random.default_rng(100 + k)
    n = 8200
    rowcols = [np.array([1, 5]), np.sort(rng.choice(n, k, replace=False)), np.arange(0, n, 7)]
    A, rows, cols, vals = from_rows(gb, rowcols, n, "INT32", rng)
    has, val = dense_of(3, n, rows, cols, vals)
    own = rowcols[1][rng.integers(0, k, 30)] if k else np.zeros(0, np.int64)
    for J in (np.concatenate([own, rng.integers(0, n, 70)]).astype(np.int64), np.array([n - 1, 0, 0, n - 1]), np.arange(n)[::-1][:4097]):
        for expr in (A[1, list(map(int, J))], A.T[list(map(int, J)), 1]):
            same_vector(expr.new(), has[1, J], val[1, J], (k, "list"))
    same_vector(A[1, 3:8000:3].new(), has[1, 3:8000:3], val[1, 3:8000:3], (k, "slice"))
    whole = A[1, :].new()
    assert (stats()["kernel_launches"], stats()["method"]) == (1 if k else 0, 9)  # one scatter of the row, not ncols searches
    same_vector(whole, has[1], val[1], (k, "all"))
    same_vector(A.T[:, 1].new(), has[1], val[1], (k, "all, transposed"))
    same_vector(A[1, :].new(dtype="FP64"), has[1], val[1].astype(np.float64), (k, "all, cast"))


@pytest.mark.parametrize("size", [63, 64, 65, 4097])
def test_column_extract(gb, size):
    """A[I, j] and A[:, j] (with and without a cached transpose) at sizes around the last presence word; mask, accumulator, replace."""
    rng = np.random.default_rng(200 + size)
    m, n = size, 70
    rowcols = [np.sort(rng.choice(n, int(rng.integers(0, 9)), replace=False)) for _ in range(m)]
    rowcols[m - 1] = np.array([3, 69])
    rowcols[0] = np.array([0, 3])
    A, rows, cols, vals = from_rows(gb, rowcols, n, "INT64", rng)
    has, val = dense_of(m, n, rows, cols, vals)
    for j in (3, 0, 69, 20):
        plain = A[:, j].new()
        assert (stats()["kernel_launches"], stats()["method"]) == (1, 11)  # no transpose is cached (and none is built): a search per row
        same_vector(plain, has[:, j], val[:, j], (size, j, "no cached transpose"))
        I = rng.integers(0, m, size)
        same_vector(A[list(map(int, I)), j].new(), has[I, j], val[I, j], (size, j, "list"))
        same_vector(A.T[j, list(map(int, I))].new(), has[I, j], val[I, j], (size, j, "list, transposed"))
        same_vector(A[::-1, j].new(), has[::-1, j], val[::-1, j], (size, j, "reversed"))
    B = gb.Matrix.from_coo(rows, cols, vals, dtype="INT64", nrows=m, ncols=n)
    B.T.new()  # (caches the transpose: A[:, j] then reads row j of it)
    for j in (3, 0, 69, 20):
        cached = B[:, j].new()
        assert stats()["method"] == 9, "the cached transpose was not read"  # row j of B's transpose is copied
        same_vector(cached, has[:, j], val[:, j], (size, j, "cached transpose"))
        assert cached.isequal(A[:, j].new(), check_dtype=True) and cached.dtype == A.dtype
    # the write rule on the vector
    j = 3
    t_has, t_val = has[:, j], val[:, j]
    wi = np.flatnonzero(rng.random(m) < 0.5)
    wv = rng.integers(-50, 50, wi.size)
    mi = np.flatnonzero(rng.random(m) < 0.5)
    mv = rng.integers(0, 2, mi.size).astype(np.int8)
    zero = lambda a: np.zeros_like(a)  # noqa: E731
    T = (np.flatnonzero(t_has), zero(np.flatnonzero(t_has)), t_val[t_has])
    for mask_kind in (0, 1, 2):
        for comp in (False, True):
            for repl in (False, True):
                for accum in (None, "plus"):
                    if not mask_kind and (comp or repl):
                        continue
                    w = gb.Vector.from_coo(wi, wv, dtype="INT64", size=m)
                    mk = gb.Vector.from_coo(mi, mv, dtype="INT8", size=m)
                    kw = {}
                    if mask_kind:
                        mm = mk.S if mask_kind == 2 else mk.V
                        kw = dict(mask=~mm if comp else mm, replace=repl)
                    if accum:
                        kw["accum"] = accum
                    w(**kw) << A[:, j]
                    er, _, ev = np_write_rule((m, 1), "INT64", (wi, zero(wi), wv), T, (mi, zero(mi), mv) if mask_kind else None, mask_kind == 2,
                                              comp, repl, accum)
                    Ig, Xg = w.to_coo()
                    assert Ig.tolist() == er.tolist() and Xg.tolist() == ev.tolist(), (size, mask_kind, comp, repl, accum)


def test_element_positions(gb):
    """A[i, j]: first / middle / last entry of rows of 1 / 64 / 65 / 8193 entries, absent entries before / between / after, an empty row."""
    rng = np.random.default_rng(6)
    n = 20000
    lengths = [1, 64, 65, 8193, 0]
    rowcols = [np.sort(rng.choice(np.arange(2, n - 2, 2), k, replace=False)) for k in lengths]  # (even columns: the odd ones lie between)
    A, rows, cols, vals = from_rows(gb, rowcols, n, "INT32", rng)
    has, val = dense_of(len(lengths), n, rows, cols, vals)
    for i, rc in enumerate(rowcols):
        probes = [0, n - 1, 1]
        if rc.size:
            probes += [rc[0], rc[rc.size // 2], rc[-1], rc[0] - 1, rc[-1] + 1, rc[rc.size // 2] + 1, rc[min(63, rc.size - 1)], rc[min(64, rc.size - 1)]]
        for j in probes:
            got = A[i, int(j)].new()
            want = int(val[i, j]) if has[i, j] else None
            assert got.value == want, (i, j)
            assert A.T[int(j), i].value == want, (i, j, "transposed")


def test_element_types(gb):
    """Every matrix type into every GrB_Matrix_extractElement_<T> for a value both types hold; the _Scalar form present and absent."""
    from graphblas_amd import _lib

    L = _lib.lib
    names = list(CT_OF)
    for tname in names:
        A = gb.Matrix.from_coo([1, 2], [2, 0], [1, 1], dtype=tname, nrows=3, ncols=4)
        for oname in names:
            out = CT_OF[oname](0)
            assert getattr(L, f"GrB_Matrix_extractElement_{oname}")(ctypes.byref(out), A._carg, 1, 2) == 0, (tname, oname)
            assert out.value == 1 and type(out.value) is type(CT_OF[oname](1).value), (tname, oname)
            assert getattr(L, f"GrB_Matrix_extractElement_{oname}")(ctypes.byref(out), A._carg, 1, 3) == 1  # GrB_NO_VALUE
            assert getattr(L, f"GrB_Matrix_extractElement_{oname}")(ctypes.byref(out), A._carg, 3, 0) == -4  # GrB_INVALID_INDEX
            assert "(3, 0) is outside" in _error(L, A), _error(L, A)
            assert getattr(L, f"GrB_Matrix_extractElement_{oname}")(ctypes.byref(out), A._carg, 0, 4) == -4
            assert "(0, 4) is outside" in _error(L, A), _error(L, A)
            assert getattr(L, f"GrB_Matrix_extractElement_{oname}")(None, A._carg, 0, 0) == -2  # GrB_NULL_POINTER
            assert "NULL" in _error(L, A), _error(L, A)
    # values are cast by the typecast rules
    F = gb.Matrix.from_coo([0, 0, 0], [0, 1, 2], [-2.75, 300.0, np.nan], dtype="FP64", nrows=1, ncols=3)
    for j, want in ((0, -2), (1, 127), (2, 0)):
        out = ctypes.c_int8(5)
        assert L.GrB_Matrix_extractElement_INT8(ctypes.byref(out), F._carg, 0, j) == 0 and out.value == want
    out = ctypes.c_bool(False)
    assert L.GrB_Matrix_extractElement_BOOL(ctypes.byref(out), F._carg, 0, 0) == 0 and out.value is True
    # the _Scalar form
    L.GrB_Scalar_extractElement_FP64.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_void_p]
    s = ctypes.c_void_p()
    assert L.GrB_Scalar_new(ctypes.byref(s), ctypes.c_void_p(ctypes.c_void_p.in_dll(L, "GrB_FP64").value)) == 0
    try:
        x = ctypes.c_double(0)
        assert L.GrB_Matrix_extractElement_Scalar(s, F._carg, 0, 0) == 0
        assert L.GrB_Scalar_extractElement_FP64(ctypes.byref(x), s) == 0 and x.value == -2.75
        assert L.GrB_Matrix_extractElement_Scalar(s, gb.Matrix("INT64", 2, 2)._carg, 1, 1) == 0  # absent: the scalar is cleared
        assert L.GrB_Scalar_extractElement_FP64(ctypes.byref(x), s) == 1
        big = gb.Matrix.from_coo([0], [0], [np.uint64(2**64 - 1)], dtype="UINT64", nrows=1, ncols=1)
        assert L.GrB_Matrix_extractElement_Scalar(s, big._carg, 0, 0) == 0
        assert L.GrB_Scalar_extractElement_FP64(ctypes.byref(x), s) == 0 and x.value == float(2**64)
        def scalar_error():
            msg = ctypes.c_char_p()
            assert L.GrB_Scalar_error(ctypes.byref(msg), s) == 0
            return (msg.value or b"").decode()

        assert L.GrB_Matrix_extractElement_Scalar(s, F._carg, 1, 0) == -4
        assert "(1, 0) is outside" in scalar_error(), scalar_error()
        assert L.GrB_Scalar_extractElement_FP64(ctypes.byref(x), s) == 0 and x.value == float(2**64)  # (the scalar is as it was)
        assert L.GrB_Matrix_extractElement_Scalar(None, F._carg, 0, 0) == -2
        assert L.GrB_Matrix_extractElement_Scalar(s, None, 0, 0) == -2
        assert "NULL" in scalar_error(), scalar_error()
    finally:
        L.GrB_Scalar_free(ctypes.byref(s))
    # an iso matrix holds one value
    iso = gb.Matrix.ss.import_csr(nrows=2, ncols=3, indptr=[0, 2, 3], values=[7], col_indices=[0, 2, 1], is_iso=True, sorted_cols=True, dtype="INT16")
    assert stored_iso(iso) and iso[0, 2] == 7 and iso[1, 1] == 7 and iso[1, 0].new().is_empty
    assert_vec(iso[0, :].new(), [0, 2], [7, 7], "row of an iso matrix")
    assert_vec(iso[:, 1].new(), [1], [7], "column of an iso matrix")


# ---- 5. the C ABI's errors --------------------------------------------------------------------------------------------------------
def _handle(L, name):
    return ctypes.c_void_p(ctypes.c_void_p.in_dll(L, name).value)


def _error(L, obj, kind="Matrix"):
    s = ctypes.c_char_p()
    getattr(L, f"GrB_{kind}_error")(ctypes.byref(s), obj._carg)
    return (s.value or b"").decode()


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_c_abi_errors(gb, literals):
    from graphblas_amd import _lib

    L = _lib.lib
    ALL = _lib.all_indices()
    A = lit_matrix(gb, literals)
    before = ([0, 1, 2], [1, 0, 3], [11, 12, 13])
    C = gb.Matrix.from_coo(*before, nrows=3, ncols=4)
    M34, M22 = gb.Matrix("BOOL", 3, 4), gb.Matrix("BOOL", 2, 2)
    keepI, I = _u64([0, 3, 6])
    keepJ, J = _u64([1, 2, 3, 4])
    keepB, bad = _u64([0, 7, 6])
    T0, PLUS_FP32, EQ = _handle(L, "GrB_DESC_T0"), _handle(L, "GrB_PLUS_FP32"), _handle(L, "GrB_EQ_INT64")
    cases = [
        ((None, None, None, A._carg, I, 3, J, 4, None), -2, None),
        ((C._carg, None, None, None, I, 3, J, 4, None), -2, "A"),
        ((C._carg, None, None, A._carg, None, 3, J, 4, None), -2, "I"),
        ((C._carg, None, None, A._carg, I, 3, None, 4, None), -2, "J"),
        ((C._carg, None, None, A._carg, I, 2, J, 4, None), -6, "2 x 4"),
        ((C._carg, None, None, A._carg, I, 3, J, 3, None), -6, "3 x 3"),
        ((C._carg, None, None, A._carg, ALL, 3, J, 4, None), -6, "7 x 4"),  # (GrB_ALL counts as the full dimension)
        ((C._carg, None, None, A._carg, I, 3, ALL, 4, T0), -6, "3 x 7"),
        ((C._carg, M22._carg, None, A._carg, I, 3, J, 4, None), -6, "mask"),
        ((C._carg, None, None, A._carg, bad, 3, J, 4, None), -105, "index"),
        ((C._carg, None, None, A._carg, I, 3, bad, 3, None), -6, "3 x 3"),
        ((C._carg, None, PLUS_FP32, A._carg, I, 3, J, 4, None), -5, "accum"),
        ((C._carg, None, EQ, A._carg, I, 3, J, 4, None), -5, "accum"),
    ]
    keepJ7, J7 = _u64([1, 2, 7, 4])
    cases.append(((C._carg, None, None, A._carg, I, 3, J7, 4, None), -105, "index"))
    cases.append(((C._carg, M34._carg, _handle(L, "GrB_PLUS_INT64"), A._carg, I, 3, J7, 4, T0), -105, "index"))
    for args, want, text in cases:
        assert L.GrB_Matrix_extract(*args) == want, (args, want)
        assert_coo(C, *before, (args, "C was written"))
        if text is not None:
            assert text in _error(L, C) and _error(L, C), (args, _error(L, C))
    # ... and the call itself works; `!Mask && comp` writes nothing, with replace it clears
    assert L.GrB_Matrix_extract(C._carg, None, None, A._carg, I, 3, J, 4, _handle(L, "GrB_DESC_C")) == 0
    assert_coo(C, *before, "complemented absent mask")
    lit = literals["extract"]
    assert L.GrB_Matrix_extract(C._carg, None, None, A._carg, I, 3, J, 4, None) == 0
    assert_coo(C, lit["rows"], lit["cols"], lit["vals"], "GrB_Matrix_extract")
    assert L.GrB_Matrix_extract(C._carg, None, None, A._carg, I, 3, J, 4, _handle(L, "GrB_DESC_RC")) == 0
    assert C.nvals == 0
    # GrB_Col_extract
    wb = ([0, 2], [5, 6])
    w = gb.Vector.from_coo(*wb, size=3)
    m2, m3 = gb.Vector("BOOL", 2), gb.Vector("BOOL", 3)
    vcases = [
        ((None, None, None, A._carg, I, 3, 2, None), -2, None),
        ((w._carg, None, None, None, I, 3, 2, None), -2, "A"),
        ((w._carg, None, None, A._carg, None, 3, 2, None), -2, "I"),
        ((w._carg, None, None, A._carg, I, 2, 2, None), -6, "2"),
        ((w._carg, None, None, A._carg, ALL, 3, 2, None), -6, "7"),
        ((w._carg, m2._carg, None, A._carg, I, 3, 2, None), -6, "mask"),
        ((w._carg, None, None, A._carg, I, 3, 7, None), -4, "7"),  # GrB_INVALID_INDEX, as GrB_Vector_removeElement
        ((w._carg, None, None, A._carg, I, 3, 7, T0), -4, "7"),
        ((w._carg, None, None, A._carg, bad, 3, 2, None), -105, "index"),
        ((w._carg, m3._carg, None, A._carg, bad, 3, 2, T0), -105, "index"),
        ((w._carg, None, PLUS_FP32, A._carg, I, 3, 2, None), -5, "accum"),
        ((w._carg, None, EQ, A._carg, I, 3, 2, None), -5, "accum"),
    ]
    for args, want, text in vcases:
        assert L.GrB_Col_extract(*args) == want, (args, want)
        assert_vec(w, *wb, (args, "w was written"))
        if text is not None:
            assert text in _error(L, w, "Vector"), (args, _error(L, w, "Vector"))
    keep135, I135 = _u64([1, 3, 5])
    assert L.GrB_Col_extract(w._carg, None, None, A._carg, I135, 3, 2, None) == 0
    assert_vec(w, literals["extract_column"]["idx"], literals["extract_column"]["vals"], "GrB_Col_extract")
    keep024, J024 = _u64([0, 2, 4])
    assert L.GrB_Col_extract(w._carg, None, None, A._carg, J024, 3, 6, T0) == 0
    assert_vec(w, literals["extract_row"]["idx"], literals["extract_row"]["vals"], "GrB_Col_extract, T0")
    assert L.GrB_Col_extract(w._carg, None, None, A._carg, J024, 3, 6, _handle(L, "GrB_DESC_C")) == 0
    assert_vec(w, literals["extract_row"]["idx"], literals["extract_row"]["vals"], "complemented absent mask")


# ---- 6. GPU tier only -------------------------------------------------------------------------------------------------------------
def _rmat(gb, scale):
    import scipy.sparse as sp

    from graphblas_amd import synthetic

    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, device="cpu")
    w = synthetic.edge_weights(col, scale).numpy()
    G = sp.csr_matrix((w, col.numpy().astype(np.int64), ip.numpy()), shape=(n, n))
    G.sort_indices()
    return n, G, gb.Matrix.from_csr(G.indptr, G.indices, G.data, dtype="FP32", ncols=n)


@pytest.mark.gpu
def test_rmat16_gpu():
    """R-MAT scale 16: A[V, V] for a sorted and a shuffled half of the vertices, A[S, :] for 1024 random rows, against scipy."""
    gb = bind("gpu")
    n, G, A = _rmat(gb, 16)
    rng = np.random.default_rng(16)
    V = np.sort(rng.choice(n, n // 2, replace=False))
    Vs = rng.permutation(V)
    S = rng.integers(0, n, 1024)
    for name, I, J, method in (("sorted", V, V, None), ("shuffled", Vs, Vs, 12), ("rows", S, None, 9)):
        ref = (G[I] if J is None else G[I][:, J]).tocsr()
        ref.sort_indices()
        C = A[I, slice(None) if J is None else J].new()
        st = stats()
        assert method is None or st["method"] == method, (name, st)
        assert st["method"] in (9, 10, 11, 12) and st["out_nvals"] == ref.nnz, (name, st)
        Cp, Cj, Cx = C.to_csr()
        assert np.array_equal(Cp.astype(np.int64), ref.indptr) and np.array_equal(Cj.astype(np.int64), ref.indices), name
        assert np.array_equal(Cx, ref.data), name
    v = A[int(S[0]), :].new()
    row = G[int(S[0])]
    assert_vec(v, row.indices.tolist(), row.data.tolist(), "A[i, :]")


@pytest.mark.gpu
def test_no_growth_gpu():
    """100 extracts per cycle (every method, rows, columns, elements), results freed.  The library keeps freed blocks in its size-class
    cache, so the first cycle may grow: free device memory after the first 100 calls against after 3 x 100."""
    import torch

    gb = bind("gpu")
    n, _, A = _rmat(gb, 14)
    rng = np.random.default_rng(14)
    V = np.sort(rng.choice(n, n // 2, replace=False))
    Vs = rng.permutation(V)
    few = np.sort(rng.choice(n, 5, replace=False))
    S = rng.integers(0, n, 256)

    def free_bytes():
        gb.Matrix(int, 1, 1).wait()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        for k in range(10):
            for expr in (A[S, :], A[V, V], A[Vs, Vs], A[S, few], A[100:5000, 100:5000], A[:, :], A[int(S[k]), :], A[:, int(S[k])], A[S, int(S[k])],
                         A.T[V, few]):
                r = expr.new()
                del r
            A[int(S[k]), int(S[k])].new()

    cycle()
    after1 = free_bytes()
    cycle()
    cycle()
    after3 = free_bytes()
    print(f"free after 100 calls: {after1 / 2**20:.1f} MiB, after 300: {after3 / 2**20:.1f} MiB")
    assert after3 >= after1, (after1, after3)
