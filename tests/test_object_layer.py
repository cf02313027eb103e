"""The object layer (python-graphblas_amd/csrc/grb_object.hip) against numpy and the oracle: build and duplicate folding, the device
typecasts behind ``GrB_*_build_<X>`` / ``extractTuples_<X>``, CSR / CSC import and export, iso storage, the transpose and
``GrB_transpose`` with the write rule, the cached transpose, resize, typecast copies and the device-side isequal / isclose.  Both
tiers: the HIP library on the GPU, the same kernel sources under the CPU wave64 emulator.

Every expected value is numpy, a Python loop or the oracle -- never a second call into the library.  Floating-point values are
compared as bit patterns (``tests.values.same_fp``: NaN matches NaN, the zero sign counts), with the one exception that comparator
documents: under a min / max fold a zero matches a zero of either sign (IEEE minNum leaves min(-0, +0) open, and numpy's fmin and the
hardware's v_min answer it differently).  No tolerance appears anywhere but in the isclose cases, whose pairs are drawn a factor 8
inside or outside the bound and checked to be at least a factor 4 away from it.

Shapes are the smallest at which each piece can go wrong: keys are ``(row << cshift) | col`` with ``cshift = ceil_log2(ncols)``, so
ncols sits at 2^k and 2^k +- 1 (63 / 64 / 65, 4095 / 4096 / 4097) and at 1 and 2; nrows at 1, 2, 3 and 257 (more than one block of the
row-pointer search); first, last and a run of consecutive rows are empty; vectors sit at the 64-bit presence-word boundaries."""
import ctypes

import numpy as np
import pytest

from oracle import grb_oracle as O
from tests.backend import DEVICES, bind
from tests.values import ALL_TYPES, FP_TYPES, rand_vals, same_fp, same_values

NP_OF = O.NP_OF
NROWS = (1, 2, 3, 257)
NCOLS = (1, 2, 63, 64, 65, 4095, 4096, 4097)
SHAPES = [(m, n) for m in NROWS for n in NCOLS]
VEC_SIZES = (1, 63, 64, 65, 127, 128, 129, 4097)
GrB_INVALID_VALUE, GrB_NOT_IMPLEMENTED, GrB_OUTPUT_NOT_EMPTY, GrB_INSUFFICIENT_SPACE, GrB_INDEX_OUT_OF_BOUNDS = -3, -8, -7, -103, -105
CSR, CSC, COO = 0, 1, 2


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


# ---- numpy restatements ------------------------------------------------------------------------------------------------------
def same_arr(got, exp, where="", monoid=None):
    """Two value arrays of one dtype, floating point as bit patterns."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (where, got.dtype, exp.dtype, got.shape, exp.shape)
    if exp.dtype.kind == "f":
        same_fp(got, exp, monoid, where)
    else:
        assert got.tolist() == exp.tolist(), (where, got, exp)


def np_csr(r, c, x, m):
    o = np.lexsort((c, r))
    return np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))]).astype(np.int64), c[o], x[o]


def np_csc(r, c, x, n):
    o = np.lexsort((r, c))
    return np.concatenate([[0], np.cumsum(np.bincount(c, minlength=n))]).astype(np.int64), r[o], x[o]


def check_matrix(A, m, n, r, c, x, where=""):
    """Every egress form of a library Matrix against the tuples (r, c, x) it must hold."""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    assert (A.nrows, A.ncols, A.nvals) == (m, n, r.size), (where, A.shape, A.nvals, r.size)
    o = np.lexsort((c, r))
    I, J, X = A.to_coo()
    assert I.tolist() == r[o].tolist() and J.tolist() == c[o].tolist(), (where, "to_coo pattern")
    same_arr(X, x[o], where)
    ap, ai, ax = (ctypes.c_uint64() for _ in range(3))
    from graphblas_amd import _lib

    for fmt, (ep, ei, ex), (gp, gi, gx) in ((CSR, np_csr(r, c, x, m), A.to_csr()), (CSC, np_csc(r, c, x, n), A.to_csc())):
        assert _lib.lib.GrB_Matrix_exportSize(ctypes.byref(ap), ctypes.byref(ai), ctypes.byref(ax), fmt, A._handle) == 0
        assert (ap.value, ai.value, ax.value) == (ep.size, r.size, r.size), (where, fmt, "exportSize")
        assert gp.astype(np.int64).tolist() == ep.tolist() and gi.astype(np.int64).tolist() == ei.tolist(), (where, fmt, "pointers / indices")
        same_arr(gx, ex, (where, fmt))


def check_vector(v, size, idx, x, where=""):
    idx = np.asarray(idx, np.int64)
    o = np.argsort(idx, kind="stable")
    assert (v.size, v.nvals) == (size, idx.size), (where, v.size, v.nvals, idx.size)
    gi, gx = v.to_coo()
    assert gi.tolist() == idx[o].tolist(), (where, "pattern")
    same_arr(gx, np.asarray(x)[o], where)


def patterns(rng, m, n):
    """(name, rows, cols) from empty to full: no entry; the first cell; the last cell; a few hundred entries with the last column and the
    cells around 2^k occupied and -- from three rows on -- the first row, the last row and a run of consecutive rows empty; every cell."""
    z = np.zeros(0, np.int64)
    out = [("empty", z, z), ("first", np.array([0]), np.array([0])), ("last", np.array([m - 1]), np.array([n - 1]))]
    total = m * n
    flat = rng.integers(0, total, min(total, 400))
    lo = 1 if m >= 3 else 0  # (a row that stays occupied)
    forced = [lo * n + n - 1, lo * n, lo * n + n // 2, lo * n + max(n - 2, 0)]
    flat = np.unique(np.concatenate([flat, forced]))
    r, c = flat // n, flat % n
    if m >= 3:
        run0 = m // 3 + 1
        empty = np.concatenate([[0, m - 1], np.arange(run0, run0 + max(1, m // 8))])
        empty = empty[empty != lo]
        keep = ~np.isin(r, empty)
        r, c = r[keep], c[keep]
    out.append(("sparse", r, c))
    if total <= 4200:
        out.append(("full", np.repeat(np.arange(m), n), np.tile(np.arange(n), m)))
    return out


def domain_of(tname):
    return "exact" if tname in FP_TYPES else "signed"


def values_for(rng, k, tname, iso=False):
    x = np.asarray(rand_vals(rng, max(k, 1), tname, domain_of(tname)))[:k]
    if iso and k:
        x = np.full(k, x[0])
    return x


def ocast(x, tname):
    """``O.cast`` as an array, numpy's warnings about the out-of-range sources the cast is tested on silenced."""
    with np.errstate(all="ignore"):
        return np.asarray(O.cast(np.asarray(x), tname))


def shuffled(rng, *arrays):
    p = rng.permutation(arrays[0].size)
    return [a[p] for a in arrays]


def stored_iso(A):
    """Whether the library keeps ONE value for every entry of A (GrX_Matrix_export_CSR_device reports the stored form)."""
    from graphblas_amd import _lib

    dp, dj, dx, nv, iso = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    assert _lib.lib.GrX_Matrix_export_CSR_device(ctypes.byref(dp), ctypes.byref(dj), ctypes.byref(dx), ctypes.byref(nv), ctypes.byref(iso), A._carg) == 0
    return bool(iso.value)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ---- 1. build and duplicate folding --------------------------------------------------------------------------------------------
DUP_RUNS = (1, 2, 63, 64, 65, 300)  # 495 duplicates: the runs cross the 64-lane and the 256-thread boundaries of the sorted order
BOOL_AS = {"plus": "lor", "times": "land", "min": "land", "max": "lor", "minus": "lxor"}


def fold_runs(keys, vals, op, tname):
    """The documented fold: per key a LEFT fold in INPUT order, one element at a time, in the object's type.  The operator is the
    oracle's own evaluation of it (the one its accumulators use: fmin / fmax for floating-point min / max, C wrap-around for integers)."""
    f = O._NP_BINOP[BOOL_AS.get(op, op) if tname == "BOOL" else op]
    order = np.argsort(keys, kind="stable")
    ks, vs = keys[order], vals[order]
    out_k, out_v = [], []
    with np.errstate(all="ignore"):
        i = 0
        while i < ks.size:
            acc, j = vs[i], i + 1
            while j < ks.size and ks[j] == ks[i]:
                acc = vs.dtype.type(f(acc, vs[j]))
                j += 1
            out_k.append(ks[i])
            out_v.append(acc)
            i = j
    return np.asarray(out_k, np.int64), np.asarray(out_v, vals.dtype)


def dup_keys(rng, space, case):
    """Keys (flat positions below ``space``) in random order: the runs of DUP_RUNS plus single tuples, the first and the last position
    among the keys; or one key for every tuple; or one tuple."""
    if case == "same_key":
        return np.full(130, space - 1, np.int64)
    if case == "single":
        return np.array([space // 2], np.int64)
    k = min(space, 26)
    distinct = np.unique(np.concatenate([rng.choice(space, k, replace=False), [0, space - 1]]))
    distinct = rng.permutation(distinct)
    lens = np.ones(distinct.size, np.int64)
    lens[: min(len(DUP_RUNS), distinct.size)] = DUP_RUNS[: distinct.size]
    return rng.permutation(np.repeat(distinct, lens)).astype(np.int64)


def dup_ops(tname):
    return ("plus", "times", "min", "max", "first", "second", "minus") + (("lor", "land", "lxor") if tname == "BOOL" else ())


def fold_monoid(op, tname):
    return op if (op in ("min", "max") and tname in FP_TYPES) else None


@pytest.mark.parametrize("tname", ALL_TYPES)
def test_build_folds_duplicates_in_input_order(gb, tname):
    """Matrix and Vector build with every dup_op over runs of 1 / 2 / 63 / 64 / 65 / 300 equal keys in random input order.  ``minus``
    (``first`` / ``second`` for BOOL, whose minus is the order-blind lxor) fails if the fold is not a left fold in input order."""
    rng = np.random.default_rng(1100 + ALL_TYPES.index(tname))
    for (m, n), case in (((3, 65), "runs"), ((257, 4097), "runs"), ((2, 64), "same_key"), ((1, 1), "same_key"), ((2, 3), "single"),
                         ((1, 4096), "runs")):
        keys = dup_keys(rng, m * n, case)
        vals = values_for(rng, keys.size, tname)
        for op in dup_ops(tname):
            where = (tname, m, n, case, op)
            ek, ev = fold_runs(keys, vals, op, tname)
            A = gb.Matrix(tname, m, n)
            A.build(keys // n, keys % n, vals, dup_op=getattr(gb.binary, op))
            I, J, X = A.to_coo()
            assert (I.astype(np.int64) * n + J.astype(np.int64)).tolist() == ek.tolist(), where
            same_arr(X, ev, where, fold_monoid(op, tname))
            w = gb.Vector(tname, m * n)
            w.build(keys, vals, dup_op=getattr(gb.binary, op))
            gi, gx = w.to_coo()
            assert gi.tolist() == ek.tolist(), where
            same_arr(gx, ev, where, fold_monoid(op, tname))


def special_sources(xname):
    np_t = NP_OF[xname]
    if xname == "BOOL":
        return np.array([True, False, True])
    if xname in FP_TYPES:
        fi = np.finfo(np_t)
        with np.errstate(over="ignore"):
            return np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -0.5, 0.5, 255.5, -129, 2.0 ** 31, 2.0 ** 63, 2.0 ** 64, fi.max, -fi.max,
                             fi.smallest_subnormal, -fi.smallest_subnormal, 3.0, -7.0, 127.0, 128.0, 65535.0, 65536.0, -32769.0], np_t)
    info = np.iinfo(np_t)
    return np.array([info.min, info.max, 0, 1, 2, info.max - 1] + ([-1, -2, info.min + 1] if info.min < 0 else [info.max // 2 + 1]), np_t)


def raw_build(gb, kind, tname, shape, idx, X, xname, dup=None):
    """``GrB_<kind>_build_<xname>`` into a fresh object of type ``tname`` through the bound library: (object, return code)."""
    from graphblas_amd import _lib

    if kind == "Matrix":
        obj = gb.Matrix(tname, *shape)
        n = shape[1]
        I, J = np.ascontiguousarray(idx // n, np.uint64), np.ascontiguousarray(idx % n, np.uint64)
        rc = getattr(_lib.lib, f"GrB_Matrix_build_{xname}")(obj._handle, _p(I), _p(J), _p(X), X.size, dup)
    else:
        obj = gb.Vector(tname, shape[0] * shape[1])
        I = np.ascontiguousarray(idx, np.uint64)
        rc = getattr(_lib.lib, f"GrB_Vector_build_{xname}")(obj._handle, _p(I), _p(X), X.size, dup)
    return obj, rc


def raw_extract(obj, kind, xname, count):
    """``GrB_<kind>_extractTuples_<xname>``: (flat indices, values as ``xname``)."""
    from graphblas_amd import _lib

    I, J, X = np.empty(count, np.uint64), np.empty(count, np.uint64), np.empty(count, NP_OF[xname])
    cnt = ctypes.c_uint64(count)
    if kind == "Matrix":
        rc = getattr(_lib.lib, f"GrB_Matrix_extractTuples_{xname}")(_p(I), _p(J), _p(X), ctypes.byref(cnt), obj._handle)
        flat = I.astype(np.int64) * obj.ncols + J.astype(np.int64)
    else:
        rc = getattr(_lib.lib, f"GrB_Vector_extractTuples_{xname}")(_p(I), _p(X), ctypes.byref(cnt), obj._handle)
        flat = I.astype(np.int64)
    assert rc == 0 and cnt.value == count, (rc, cnt.value, count)
    return flat, X


@pytest.mark.parametrize("kind", ["Matrix", "Vector"])
@pytest.mark.parametrize("tname", ALL_TYPES)
def test_device_typecast_of_build_and_extract_tuples(gb, kind, tname):
    """``GrB_*_build_<X>`` into an object of type T and ``extractTuples_<X>`` out of it, all 11 x 11 pairs (``cast_array``): NaN, +-inf,
    +-0.0, fractions, values beyond every integer range, +-max and subnormals; the integer types' min / max / -1 -- against ``O.cast``."""
    shape = (3, 65)
    for xname in ALL_TYPES:
        src = np.ascontiguousarray(special_sources(xname))
        idx = np.arange(src.size, dtype=np.int64) * 7 + 1  # (3 * 65 = 195 cells; 23 sources at most)
        obj, rc = raw_build(gb, kind, tname, shape, idx, src, xname)
        assert rc == 0, (tname, xname, rc)
        stored = ocast(src, tname)
        flat, X = raw_extract(obj, kind, tname, src.size)
        assert flat.tolist() == idx.tolist(), (tname, xname)
        same_arr(X, stored, ("build", tname, "from", xname))
        # ... and out of an object of type `xname` as `tname`: the same 121 pairs of the egress cast
        src_obj, rc = raw_build(gb, kind, xname, shape, idx, src, xname)
        assert rc == 0
        flat, X = raw_extract(src_obj, kind, tname, src.size)
        assert flat.tolist() == idx.tolist(), (tname, xname)
        same_arr(X, stored, ("extractTuples", xname, "as", tname))


@pytest.mark.parametrize("kind", ["Matrix", "Vector"])
def test_failed_builds_leave_an_empty_usable_object(gb, kind):
    """An index out of bounds in the LAST tuple only, duplicates without a dup_op, and a second build into a non-empty object.  After
    the first two the object is empty (nvals == 0, no tuples) and a following valid build succeeds and is correct.  The third is an API
    error of the C API (GrB_OUTPUT_NOT_EMPTY): it leaves the object as it was -- checked against the tuples of the first build --, and
    after ``clear`` the object is empty and takes a valid build."""
    rng = np.random.default_rng(1300)
    m, n = 3, 65
    space = m * n
    idx = rng.permutation(space)[:100].astype(np.int64)
    for tname in ("INT64", "FP32", "BOOL", "UINT8"):
        vals = np.ascontiguousarray(values_for(rng, idx.size, tname))

        def holds(obj, keys, x, where):
            if kind == "Matrix":
                check_matrix(obj, m, n, keys // n, keys % n, x, where)
            else:
                check_vector(obj, space, keys, x, where)

        def py_build(obj, keys, x, **kw):
            if kind == "Matrix":
                obj.build(keys // n, keys % n, x, **kw)
            else:
                obj.build(keys, x, **kw)

        # (a) out of bounds, last tuple only: raw, then through the host API
        bad = idx.copy()
        bad[-1] = space if kind == "Vector" else (m - 1) * n + n  # (row m, column 0 as a flat position: row index out of range)
        obj, rc = raw_build(gb, kind, tname, (m, n), bad, vals, tname)
        assert rc == GrB_INDEX_OUT_OF_BOUNDS, (tname, rc)
        holds(obj, idx[:0], vals[:0], (tname, "after out-of-bounds"))
        py_build(obj, idx, vals)
        holds(obj, idx, vals, (tname, "valid build after out-of-bounds"))
        obj = gb.Matrix(tname, m, n) if kind == "Matrix" else gb.Vector(tname, space)
        with pytest.raises(gb.exceptions.IndexOutOfBound):
            if kind == "Matrix":
                obj.build(np.append(idx[:-1] // n, 0), np.append(idx[:-1] % n, n), vals)  # (column n)
            else:
                obj.build(bad, vals)
        holds(obj, idx[:0], vals[:0], (tname, "after out-of-bounds (host API)"))
        # (b) duplicates and no dup_op
        dup = idx.copy()
        dup[-1] = dup[0]
        obj, rc = raw_build(gb, kind, tname, (m, n), dup, vals, tname, None)
        assert rc == GrB_INVALID_VALUE, (tname, rc)
        holds(obj, idx[:0], vals[:0], (tname, "after duplicates"))
        py_build(obj, idx, vals)
        holds(obj, idx, vals, (tname, "valid build after duplicates"))
        obj = gb.Matrix(tname, m, n) if kind == "Matrix" else gb.Vector(tname, space)
        with pytest.raises(ValueError, match="Duplicate indices found"):
            py_build(obj, dup, vals)
        holds(obj, idx[:0], vals[:0], (tname, "after duplicates (host API)"))
        py_build(obj, idx, vals)
        # (c) a second build
        with pytest.raises(gb.exceptions.OutputNotEmpty):
            py_build(obj, idx[:5], vals[:5])
        holds(obj, idx, vals, (tname, "a refused second build changes nothing"))
        obj.clear()
        holds(obj, idx[:0], vals[:0], (tname, "cleared"))
        py_build(obj, idx[:5], vals[:5])
        holds(obj, idx[:5], vals[:5], (tname, "valid build after clear"))


# ---- 2. import and export ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", SHAPES)
def test_coo_csr_csc_round_trips_at_the_edge_shapes(gb, m, n):
    """Tuples in random order -> build -> to_coo / to_csr / to_csc / exportSize, and from_csr / from_csc with the indices inside a row /
    column NOT sorted -> the same egress, against a numpy restatement (lexsort + bincount).  Every pattern of ``patterns``; the types
    rotate over the patterns and the sparse pattern runs in all 11."""
    rng = np.random.default_rng(2000 + 17 * m + n)
    k = 0
    for name, r, c in patterns(rng, m, n):
        for tname in (ALL_TYPES if name == "sparse" else (ALL_TYPES[(k + m + n) % 11],)):
            k += 1
            x = values_for(rng, r.size, tname)
            where = (m, n, name, tname)
            sr, sc, sx = shuffled(rng, r, c, x)
            A = gb.Matrix.from_coo(sr, sc, sx, dtype=tname, nrows=m, ncols=n)
            check_matrix(A, m, n, r, c, x, where)
            # CSR / CSC whose minor indices are jumbled inside every row / column
            for fmt in (CSR, CSC):
                major, minor, nmaj = (r, c, m) if fmt == CSR else (c, r, n)
                o = np.lexsort((rng.random(major.size), major))  # (sorted by the major index only)
                indptr = np.concatenate([[0], np.cumsum(np.bincount(major, minlength=nmaj))])
                if fmt == CSR:
                    B = gb.Matrix.from_csr(indptr, minor[o], x[o], dtype=tname, ncols=n)
                else:
                    B = gb.Matrix.from_csc(indptr, minor[o], x[o], dtype=tname, nrows=m)
                check_matrix(B, m, n, r, c, x, (where, "from", fmt))


def test_to_coo_partial_forms_and_short_arrays(gb):
    """``to_coo(rows=False)`` & co. leave the other arrays as they are; arrays one element too short give the documented codes
    (extractTuples / export: GrB_INSUFFICIENT_SPACE; import: GrB_INVALID_VALUE); the COO format is declined with GrB_NOT_IMPLEMENTED."""
    from graphblas_amd import _lib

    L = _lib.lib
    rng = np.random.default_rng(2100)
    m, n, tname = 3, 65, "INT16"
    (_, r, c) = patterns(rng, m, n)[3]
    x = values_for(rng, r.size, tname)
    A = gb.Matrix.from_coo(r, c, x, dtype=tname, nrows=m, ncols=n)
    o = np.lexsort((c, r))
    for rows, columns, values in ((False, True, True), (True, False, True), (True, True, False), (False, False, True), (False, False, False)):
        I, J, X = A.to_coo(rows=rows, columns=columns, values=values)
        assert (I is None) == (not rows) and (J is None) == (not columns) and (X is None) == (not values)
        assert I is None or I.tolist() == r[o].tolist()
        assert J is None or J.tolist() == c[o].tolist()
        assert X is None or X.tolist() == x[o].tolist()
    nv = r.size
    I, J, X = np.empty(nv, np.uint64), np.empty(nv, np.uint64), np.empty(nv, NP_OF[tname])
    cnt = ctypes.c_uint64(nv - 1)
    assert L.GrB_Matrix_extractTuples_INT16(_p(I), _p(J), _p(X), ctypes.byref(cnt), A._handle) == GrB_INSUFFICIENT_SPACE
    v = gb.Vector.from_coo(r * n + c, x, dtype=tname, size=m * n)
    cnt = ctypes.c_uint64(nv - 1)
    assert L.GrB_Vector_extractTuples_INT16(_p(I), _p(X), ctypes.byref(cnt), v._handle) == GrB_INSUFFICIENT_SPACE
    for fmt, nvec in ((CSR, m), (CSC, n)):
        P = np.empty(nvec + 1, np.uint64)
        for short in range(3):
            lens = [ctypes.c_uint64(nvec + 1 - (short == 0)), ctypes.c_uint64(nv - (short == 1)), ctypes.c_uint64(nv - (short == 2))]
            rc = L.GrB_Matrix_export_INT16(_p(P), _p(I), _p(X), ctypes.byref(lens[0]), ctypes.byref(lens[1]), ctypes.byref(lens[2]), fmt, A._handle)
            assert rc == GrB_INSUFFICIENT_SPACE, (fmt, short, rc)
        ep, ei, ex = np_csr(r, c, x, m) if fmt == CSR else np_csc(r, c, x, n)
        ep, ei = np.ascontiguousarray(ep, np.uint64), np.ascontiguousarray(ei, np.uint64)
        typ = ctypes.c_void_p(_lib.handle("GrB_INT16"))
        for short in range(3):
            h = ctypes.c_void_p()
            rc = L.GrB_Matrix_import_INT16(ctypes.byref(h), typ, m, n, _p(ep), _p(ei), _p(ex), ep.size - (short == 0), nv - (short == 1),
                                           nv - (short == 2), fmt)
            assert rc == GrB_INVALID_VALUE and not h.value, (fmt, short, rc)
    # the COO format: declined by design
    lens = [ctypes.c_uint64(nv + m + n) for _ in range(3)]
    P = np.empty(nv + m + n, np.uint64)
    assert L.GrB_Matrix_exportSize(ctypes.byref(lens[0]), ctypes.byref(lens[1]), ctypes.byref(lens[2]), COO, A._handle) == GrB_NOT_IMPLEMENTED
    assert L.GrB_Matrix_export_INT16(_p(P), _p(I), _p(X), ctypes.byref(lens[0]), ctypes.byref(lens[1]), ctypes.byref(lens[2]), COO,
                                     A._handle) == GrB_NOT_IMPLEMENTED
    h = ctypes.c_void_p()
    assert L.GrB_Matrix_import_INT16(ctypes.byref(h), ctypes.c_void_p(_lib.handle("GrB_INT16")), m, n, _p(I), _p(J), _p(X), nv, nv, nv,
                                     COO) == GrB_NOT_IMPLEMENTED and not h.value


@pytest.mark.parametrize("tname", ALL_TYPES)
def test_iso_detection_is_by_bit_pattern(gb, tname):
    """All-equal bit patterns are kept as ONE value (all-NaN included); a +0.0 / -0.0 mix is not iso and comes back with its signs;
    two entries; one entry (never iso: nothing to share)."""
    rng = np.random.default_rng(2200 + ALL_TYPES.index(tname))
    np_t = NP_OF[tname]
    m, n = 3, 65
    (_, r, c) = patterns(rng, m, n)[3]
    cases = [("equal", np.full(r.size, values_for(rng, 1, tname)[0]), True)]
    if tname in FP_TYPES:
        cases.append(("all NaN", np.full(r.size, np.nan, np_t), True))
        cases.append(("all -0.0", np.full(r.size, -0.0, np_t), True))
        mix = np.where(rng.random(r.size) < 0.5, -0.0, 0.0).astype(np_t)
        mix[0], mix[-1] = 0.0, -0.0
        cases.append(("zeros of both signs", mix, False))
        cases.append(("NaN but the last", np.append(np.full(r.size - 1, np.nan, np_t), np_t(1)), False))
    if tname != "BOOL":
        x = np.full(r.size, np_t(5))
        x[-1] = np_t(6)
        cases.append(("last differs", x, False))
        x = np.full(r.size, np_t(5))
        x[0] = np_t(6)
        cases.append(("first differs", x, False))
    for name, x, iso in cases:
        sr, sc, sx = shuffled(rng, r, c, x)
        A = gb.Matrix.from_coo(sr, sc, sx, dtype=tname, nrows=m, ncols=n)
        assert stored_iso(A) == iso, (tname, name)
        check_matrix(A, m, n, r, c, x, (tname, name))
    two = np.array([values_for(rng, 1, tname)[0]] * 2)
    A = gb.Matrix.from_coo([2, 0], [64, 0], two, dtype=tname, nrows=m, ncols=n)
    assert stored_iso(A)
    check_matrix(A, m, n, np.array([0, 2]), np.array([0, 64]), two, (tname, "two equal"))
    if tname in FP_TYPES:
        pm = np.array([0.0, -0.0], np_t)
        A = gb.Matrix.from_coo([0, 2], [0, 64], pm, dtype=tname, nrows=m, ncols=n)
        assert not stored_iso(A)
        check_matrix(A, m, n, np.array([0, 2]), np.array([0, 64]), pm, (tname, "+0.0 and -0.0"))
    A = gb.Matrix.from_coo([2], [64], two[:1], dtype=tname, nrows=m, ncols=n)
    assert not stored_iso(A)
    check_matrix(A, m, n, np.array([2]), np.array([64]), two[:1], (tname, "one entry"))


@pytest.mark.parametrize("m,n", SHAPES)
def test_ss_import_and_pack_csr_iso_and_jumbled(gb, m, n):
    """``Matrix.ss.import_csr`` / ``A.ss.pack_csr`` with jumbled columns, with ``is_iso=True`` and with both, at the edge shapes."""
    rng = np.random.default_rng(2300 + 17 * m + n)
    for k, (name, r, c) in enumerate(patterns(rng, m, n)):
        tname = ALL_TYPES[(k + m + n) % 11]
        indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))])
        o = np.lexsort((rng.random(r.size), r))  # (columns jumbled inside every row)
        for iso in (False, True):
            if iso and r.size == 0:
                continue
            x = values_for(rng, r.size, tname, iso)
            where = (m, n, name, tname, iso)
            A = gb.Matrix.ss.import_csr(nrows=m, ncols=n, indptr=indptr, values=x[:1] if iso else x[o], col_indices=c[o], is_iso=iso,
                                        sorted_cols=False, dtype=tname)
            check_matrix(A, m, n, r, c, x, where)
            B = gb.Matrix.from_coo([m - 1], [0], values_for(rng, 1, tname), dtype=tname, nrows=m, ncols=n)
            B.ss.pack_csr(indptr=indptr, values=x[:1] if iso else x[o], col_indices=c[o], is_iso=iso, sorted_cols=False)
            check_matrix(B, m, n, r, c, x, (where, "pack"))
            if iso and r.size > 1:
                assert stored_iso(A) and stored_iso(B), where


# ---- 3. transpose --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", SHAPES)
def test_transpose_new_at_the_edge_shapes(gb, m, n):
    """``A.T.new()`` against numpy (the tuples with rows and columns swapped), iso and not; every type on the sparse pattern."""
    rng = np.random.default_rng(3000 + 17 * m + n)
    k = 0
    for name, r, c in patterns(rng, m, n):
        for tname in (ALL_TYPES if name == "sparse" else (ALL_TYPES[(k + m + n) % 11],)):
            k += 1
            for iso in (False, True):
                if iso and r.size < 2:
                    continue
                x = values_for(rng, r.size, tname, iso)
                A = gb.Matrix.from_coo(r, c, x, dtype=tname, nrows=m, ncols=n)
                B = A.T.new()
                check_matrix(B, n, m, c, r, x, (m, n, name, tname, iso))
                assert B.dtype.name == tname and (not iso or stored_iso(B))


def o_eye(n, tname):
    return O.OMat(n, n, np.arange(n + 1), np.arange(n), np.ones(n, NP_OF[tname]), tname)


def o_transposed_write(oa, oc, om, comp, struct, accum, replace):
    """The oracle's statement of ``C(mask, accum, replace) << A.T``: its mxm of an identity with its own transpose of A over
    (any, second) -- the product is A.T's entries untouched -- under the same mask / accumulator / replace, cast to C's type."""
    return O.mxm(o_eye(oa.ncols, oa.tname), oa.transpose(), "any_second", C=oc, mask=om, mask_comp=comp, mask_struct=struct, accum=accum,
                 replace=replace)


def same_omat(got, exp, where="", accum=None):
    """A library Matrix against an oracle OMat.  ``accum`` min / max: where the accumulator met +0.0 and -0.0 either zero is right (IEEE
    minNum leaves min(-0, +0) open: the C library's fmin of the oracle and the GPU's v_min answer it differently) -- the rule of
    ``tests.values.same_fp`` for a min / max fold; every other value is compared as a bit pattern."""
    assert (got.nrows, got.ncols) == (exp.nrows, exp.ncols), where
    Cp, Cj, Cx = got.to_csr()
    assert Cp.astype(np.int64).tolist() == exp.indptr.tolist(), (where, "row pointers differ")
    same_values(Cj.astype(np.int64), Cx, exp.indices, exp.values, accum if accum in ("min", "max") else None, where)


def dense_coo(rng, m, n, dens, tname, domain=None):
    r, c = np.nonzero(rng.random((m, n)) < dens)
    return r, c, np.asarray(rand_vals(rng, r.size, tname, domain or ("exact" if tname in FP_TYPES else "small")))


@pytest.mark.parametrize("a_type,c_type", [("INT64", "INT64"), ("FP64", "INT8"), ("INT8", "FP32"), ("BOOL", "UINT16"), ("FP32", "FP32"),
                                           ("UINT64", "BOOL")])
def test_masked_transpose_against_the_oracle(gb, a_type, c_type):
    """``C(mask, accum, replace) << A.T`` on 30 x 50 results, 20 % dense: value and structural masks, both complemented, no mask;
    accumulators plus / min / second / none; replace on and off; C of another type than A (the cast copy runs)."""
    rng = np.random.default_rng(3100 + ALL_TYPES.index(a_type) * 11 + ALL_TYPES.index(c_type))
    m, n = 50, 30  # (A; the result is 30 x 50)
    ar, ac, ax = dense_coo(rng, m, n, 0.2, a_type)
    cr, cc, cx = dense_coo(rng, n, m, 0.2, c_type)
    mr, mc, mx = dense_coo(rng, n, m, 0.3, "BOOL", "signed")
    A = gb.Matrix.from_coo(ar, ac, ax, dtype=a_type, nrows=m, ncols=n)
    M = gb.Matrix.from_coo(mr, mc, mx, dtype="BOOL", nrows=n, ncols=m)
    oa, om = O.OMat.from_coo(ar, ac, ax, m, n, a_type), O.OMat.from_coo(mr, mc, mx, n, m, "BOOL")
    oc = O.OMat.from_coo(cr, cc, cx, n, m, c_type)
    masks = {"none": (None, False, False), "V": (M.V, False, False), "S": (M.S, False, True), "~V": (~M.V, True, False), "~S": (~M.S, True, True)}
    for mname, (mask, comp, struct) in masks.items():
        for accum in (None, "plus", "min", "second"):
            for replace in ((False, True) if mask is not None else (False,)):
                C = gb.Matrix.from_coo(cr, cc, cx, dtype=c_type, nrows=n, ncols=m)
                kw = {} if accum is None else {"accum": getattr(gb.binary, accum)}
                if mask is not None:
                    kw.update(mask=mask, replace=replace)
                C(**kw) << A.T
                exp = o_transposed_write(oa, oc, om if mask is not None else None, comp, struct, accum, replace)
                same_omat(C, exp, (a_type, c_type, mname, accum, replace), accum)


def test_masked_transpose_with_aliased_output(gb):
    """C aliased with A (``A(M.S) << A.T``) and with A and the mask (``C(C.S) << C.T``), against the oracle."""
    rng = np.random.default_rng(3200)
    n = 41
    for tname in ("INT32", "FP64"):
        ar, ac, ax = dense_coo(rng, n, n, 0.2, tname)
        mr, mc, mx = dense_coo(rng, n, n, 0.3, "BOOL", "signed")
        oa, om = O.OMat.from_coo(ar, ac, ax, n, n, tname), O.OMat.from_coo(mr, mc, mx, n, n, "BOOL")
        M = gb.Matrix.from_coo(mr, mc, mx, dtype="BOOL", nrows=n, ncols=n)
        for accum in (None, "plus"):
            kw = {} if accum is None else {"accum": getattr(gb.binary, accum)}
            A = gb.Matrix.from_coo(ar, ac, ax, dtype=tname, nrows=n, ncols=n)
            A(M.S, **kw) << A.T
            same_omat(A, o_transposed_write(oa, oa, om, False, True, accum, False), (tname, accum, "C is A"))
            C = gb.Matrix.from_coo(ar, ac, ax, dtype=tname, nrows=n, ncols=n)
            C(C.S, **kw) << C.T
            same_omat(C, o_transposed_write(oa, oa, oa, False, True, accum, False), (tname, accum, "C is A is the mask"))
            D = gb.Matrix.from_coo(ar, ac, ax, dtype=tname, nrows=n, ncols=n)
            D(~D.S, replace=True, **kw) << D.T
            same_omat(D, o_transposed_write(oa, oa, oa, True, True, accum, True), (tname, accum, "complemented, replace"))


@pytest.mark.parametrize("change", ["resize", "clear_build", "pack_csr", "select", "mxm", "masked_transpose"])
def test_cached_transpose_is_dropped_by_every_in_place_change(gb, change):
    """``A.T`` in a product builds the cached transpose; every in-place change of A must drop it: afterwards ``A.T.mxv(u)`` and
    ``A.to_csc()`` equal the oracle / numpy on the NEW content."""
    rng = np.random.default_rng(3300)
    n, tname = 65, "INT64"
    ar, ac, ax = dense_coo(rng, n, n, 0.15, tname)
    br, bc, bx = dense_coo(rng, n, n, 0.1, tname)
    A = gb.Matrix.from_coo(ar, ac, ax, dtype=tname, nrows=n, ncols=n)
    oa = O.OMat.from_coo(ar, ac, ax, n, n, tname)

    def check_through_the_transpose(A, oa, where):
        ui = np.arange(0, oa.nrows, 2)
        uv = np.asarray(rand_vals(rng, ui.size, tname))
        u = gb.Vector.from_coo(ui, uv, dtype=tname, size=oa.nrows)
        exp = O.mxv(oa, O.OVec(oa.nrows, ui, uv, tname), "plus_times", transpose_a=True)
        gi, gv = A.T.mxv(u, gb.semiring.plus_times).new().to_coo()
        same_values(gi, gv, exp.idx, exp.vals, None, where)
        ot = oa.transpose()
        Cp, Ci, Cx = A.to_csc()
        assert Cp.astype(np.int64).tolist() == ot.indptr.tolist() and Ci.astype(np.int64).tolist() == ot.indices.tolist(), where
        same_arr(Cx, ot.values, where)

    check_through_the_transpose(A, oa, "before")  # (the cache exists now)
    if change == "resize":
        A.resize(40, 64)
        keep = (ar < 40) & (ac < 64)
        new = O.OMat.from_coo(ar[keep], ac[keep], ax[keep], 40, 64, tname)
    elif change == "clear_build":
        A.clear()
        A.build(br, bc, bx)
        new = O.OMat.from_coo(br, bc, bx, n, n, tname)
    elif change == "pack_csr":
        ip, cj, cx = np_csr(br, bc, bx, n)
        A.ss.pack_csr(indptr=ip, values=cx, col_indices=cj, sorted_cols=True)
        new = O.OMat(n, n, ip, cj, cx, tname)
    elif change == "select":
        A << A.select("tril", -1)
        keep = ac <= ar - 1
        new = O.OMat.from_coo(ar[keep], ac[keep], ax[keep], n, n, tname)
    elif change == "mxm":
        B = gb.Matrix.from_coo(br, bc, bx, dtype=tname, nrows=n, ncols=n)
        A << A.mxm(B, gb.semiring.plus_times)
        new = O.mxm(oa, O.OMat.from_coo(br, bc, bx, n, n, tname), "plus_times")
    else:
        M = gb.Matrix.from_coo(br, bc, np.ones(br.size, bool), dtype="BOOL", nrows=n, ncols=n)
        A(M.S) << A.T
        new = o_transposed_write(oa, oa, O.OMat.from_coo(br, bc, np.ones(br.size, bool), n, n, "BOOL"), False, True, None, False)
    same_omat(A, new, change)
    check_through_the_transpose(A, new, change)


# ---- 4. resize -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ALL_TYPES)
def test_matrix_resize_sequences(gb, tname):
    """Shrink rows only, columns only, both; grow, shrink, grow again; shrink to 0 rows, to 0 columns and to 1 x 1 -- iso and not,
    against the numpy restatement (drop what lies beyond the new bounds)."""
    rng = np.random.default_rng(4000 + ALL_TYPES.index(tname))
    for iso in (False, True):
        for (m, n), steps in (((3, 65), [(2, 65), (2, 64), (1, 63), (257, 4097), (2, 2), (3, 65)]),
                              ((257, 65), [(257, 64), (130, 64), (129, 4096), (1, 4096), (300, 1)]),
                              ((3, 65), [(0, 65)]), ((3, 65), [(3, 0)]), ((3, 65), [(1, 1)]), ((257, 2), [(86, 1), (0, 0), (5, 5)])):
            r, c = np.nonzero(rng.random((m, n)) < 0.4)
            r, c = np.append(r, [0, m - 1]), np.append(c, [0, n - 1])
            flat = np.unique(r * n + c)
            r, c = flat // n, flat % n
            x = values_for(rng, r.size, tname, iso)
            A = gb.Matrix.from_coo(r, c, x, dtype=tname, nrows=m, ncols=n)
            for m2, n2 in steps:
                A.resize(m2, n2)
                keep = (r < m2) & (c < n2)
                r, c, x = r[keep], c[keep], x[keep]
                check_matrix(A, m2, n2, r, c, x, (tname, iso, (m, n), "->", (m2, n2)))


@pytest.mark.parametrize("size", VEC_SIZES)
def test_vector_resize_across_presence_words(gb, size):
    """From every size of the list to every other one, the last index occupied: the entries below the new size stay, nothing else
    appears; then back to the old size: what was cut off must not come back."""
    rng = np.random.default_rng(4100 + size)
    for k, new in enumerate(VEC_SIZES + (0, size + 200)):
        tname = ALL_TYPES[(k + size) % 11]
        idx = np.unique(np.concatenate([rng.integers(0, size, min(size, 150)), [0, size - 1, max(size - 2, 0), size // 2]]))
        x = values_for(rng, idx.size, tname)
        v = gb.Vector.from_coo(idx, x, dtype=tname, size=size)
        v.resize(new)
        keep = idx < new
        check_vector(v, new, idx[keep], x[keep], (tname, size, new))
        v.resize(size)
        check_vector(v, size, idx[keep], x[keep], (tname, size, new, "and back"))


def _dev():
    import tests.backend as backend

    return "cpu" if backend._bound == "emu" else "cuda"


@pytest.mark.parametrize("writer", ["build", "assign_comp_mask", "mxv_comp_mask_replace", "mxv_full", "ewise_add", "select", "dup_dtype",
                                    "fill_absent", "import_dense"])
def test_no_writer_leaves_presence_bits_above_the_size(gb, writer):
    """``GrB_Vector_resize`` copies whole presence words when it grows, so every kernel that writes a vector must leave the bits above
    its size clear.  For sizes that are no multiple of 64, a vector made by each writer -- its content checked against numpy / the
    oracle -- is grown by 200: nvals, the tuples and a plus-reduction must be what they were.  A phantom entry fails."""
    from graphblas_amd import _lib
    from graphblas_amd.base import call_on

    rng = np.random.default_rng(4200)
    tname = "INT64"
    for n in (63, 65, 127, 129, 4097):
        idx = np.unique(np.concatenate([rng.integers(0, n, n // 3), [0, n - 1]]))
        x = np.asarray(rand_vals(rng, idx.size, tname))
        mi = np.unique(rng.integers(0, n - 1, n // 4))  # (the mask never holds the last index: its complement does)
        ov, om = O.OVec(n, idx, x, tname), O.OVec(n, mi, np.ones(mi.size, bool), "BOOL")
        v = gb.Vector.from_coo(idx, x, dtype=tname, size=n)
        mk = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=n)
        if writer == "build":
            w, exp = v, ov
        elif writer == "assign_comp_mask":
            w = gb.Vector(tname, n)
            w(~mk.S)[:] << 7
            exp = O.vec_assign_scalar(O.OVec.empty(n, tname), 7, mask=om, mask_comp=True, mask_struct=True)
        elif writer in ("mxv_comp_mask_replace", "mxv_full"):
            # a matrix with an entry in every row (the diagonal and a few more): the result reaches the last index
            r = np.concatenate([np.arange(n), rng.integers(0, n, n)])
            c = np.concatenate([np.arange(n), rng.integers(0, n, n)])
            flat = np.unique(r * n + c)
            r, c = flat // n, flat % n
            ax = np.asarray(rand_vals(rng, r.size, tname))
            A = gb.Matrix.from_coo(r, c, ax, dtype=tname, nrows=n, ncols=n)
            oa = O.OMat.from_coo(r, c, ax, n, n, tname)
            fx = np.asarray(rand_vals(rng, n, tname))
            full, ofull = gb.Vector.from_coo(np.arange(n), fx, dtype=tname, size=n), O.OVec(n, np.arange(n), fx, tname)
            if writer == "mxv_full":
                w = A.mxv(full, gb.semiring.plus_times).new()
                exp = O.mxv(oa, ofull, "plus_times")
            else:
                w = v.dup()
                w(~mk.S, replace=True) << A.mxv(full, gb.semiring.plus_times)
                exp = O.mxv(oa, ofull, "plus_times", w=ov, mask=om, mask_comp=True, mask_struct=True, replace=True)
        elif writer == "ewise_add":
            j2 = np.unique(np.concatenate([rng.integers(0, n, n // 3), [n - 1]]))
            y = np.asarray(rand_vals(rng, j2.size, tname))
            w = v.ewise_add(gb.Vector.from_coo(j2, y, dtype=tname, size=n), gb.binary.plus).new()
            exp = O.vec_ewise(ov, O.OVec(n, j2, y, tname), "plus", union=True)
        elif writer == "select":
            x[-1] = 50  # (the last index passes the selection)
            v = gb.Vector.from_coo(idx, x, dtype=tname, size=n)
            w = v.select(">=", 50).new()
            exp = O.OVec(n, idx[x >= 50], x[x >= 50], tname)
        elif writer == "dup_dtype":
            w = v.dup(dtype="INT8")
            exp = O.OVec(n, idx, O.cast(x, "INT8"), "INT8")
        elif writer == "fill_absent":
            w = v.dup()
            call_on(w, "GrX_Vector_fill_absent", [w._handle, gb.monoid.min[tname]._carg])
            exp = ov
        else:
            import torch

            vals = np.asarray(rand_vals(rng, n, tname))
            t = torch.from_numpy(vals).to(_dev())
            w = gb.Vector.__new__(gb.Vector)
            w.dtype, w._size, w.name, w._handle = gb.dtypes.lookup_dtype(tname), n, "w_dense", ctypes.c_void_p()
            call_on(None, "GrX_Vector_import_dense_device", [ctypes.byref(w._handle), w.dtype._carg, n, ctypes.c_void_p(t.data_ptr()), None])
            exp = O.OVec(n, np.arange(n), vals, tname)
        total = O.vec_reduce(exp, "plus")
        for grown in (False, True):
            if grown:
                w.resize(n + 200)
            where = (writer, n, "grown" if grown else "as written")
            check_vector(w, n + 200 * grown, exp.idx, exp.vals, where)
            assert w.reduce(gb.monoid.plus).new().value == total, where


# ---- 5. typecast copies --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ALL_TYPES)
def test_dup_dtype_casts_like_the_oracle(gb, src):
    """``Matrix.dup(dtype=...)`` and ``Vector.dup(dtype=...)`` into all 11 types, iso and not, over the special values of section 1."""
    x = special_sources(src)
    m, n = 3, 65
    flat = np.arange(x.size, dtype=np.int64) * 8 + 2
    r, c = flat // n, flat % n
    A = gb.Matrix.from_coo(r, c, x, dtype=src, nrows=m, ncols=n)
    v = gb.Vector.from_coo(flat, x, dtype=src, size=m * n)
    assert not stored_iso(A)
    for dst in ALL_TYPES:
        B = A.dup(dtype=dst)
        assert B.dtype.name == dst
        check_matrix(B, m, n, r, c, ocast(x, dst), (src, dst))
        w = v.dup(dtype=dst)
        assert w.dtype.name == dst
        check_vector(w, m * n, flat, ocast(x, dst), (src, dst))
    ir, ic = np.array([0, 1, 2, 2]), np.array([64, 0, 63, 64])
    for one in x:  # iso storage: ONE value is cast
        xi = np.full(4, one)
        Ai = gb.Matrix.from_coo(ir, ic, xi, dtype=src, nrows=m, ncols=n)
        assert stored_iso(Ai), (src, one)
        for dst in ALL_TYPES:
            Bi = Ai.dup(dtype=dst)
            assert stored_iso(Bi) and Bi.dtype.name == dst, (src, dst, one)
            I, J, X = Bi.to_coo()
            assert I.tolist() == ir.tolist() and J.tolist() == ic.tolist(), (src, dst, one)
            same_arr(X, ocast(xi, dst), (src, dst, one, "iso"))


# ---- 6. isequal / isclose ------------------------------------------------------------------------------------------------------
def np_isequal(xa, ta, xb, tb):
    """The reference's rule: values compared with ``==`` in ``unify(ta, tb)`` (numpy's promote_types)."""
    t = O.unify(ta, tb)
    with np.errstate(all="ignore"):
        return bool(np.all(ocast(np.asarray(xa, NP_OF[ta]), t) == ocast(np.asarray(xb, NP_OF[tb]), t)))


MIXED_PAIRS = [  # (type, values) x 2 and the verdict stated by the issue; `np_isequal` must agree with it
    ("INT8", [-1, 3], "UINT8", [255, 3], False),
    ("INT8", [-1, 3], "UINT16", [65535, 3], False),
    ("INT64", [-1, 3], "UINT64", [2 ** 64 - 1, 3], False),
    ("INT32", [5, 7], "FP32", [5.0, 7.0], True),
    ("BOOL", [True, False], "INT8", [1, 0], True),
    ("BOOL", [True, True], "INT8", [1, 2], False),
    ("INT8", [-1, 3], "INT8", [-1, 3], True),
    ("INT16", [-1, 3], "UINT16", [65535, 3], False),
    ("INT32", [-1, 3], "UINT32", [2 ** 32 - 1, 3], False),
    ("INT32", [-1, 3], "UINT8", [255, 3], False),
    ("INT16", [300, 3], "UINT8", [44, 3], False),
    ("UINT8", [200, 3], "INT8", [-56, 3], False),
    ("UINT8", [200, 3], "INT16", [200, 3], True),
    ("UINT32", [2 ** 31, 3], "INT64", [2 ** 31, 3], True),
    ("UINT64", [2 ** 63, 3], "INT64", [-2 ** 63, 3], False),
    ("FP32", [0.5, 3], "INT32", [0, 3], False),
    ("FP32", [16777216.0, 3], "INT32", [16777217, 3], False),
    ("FP64", [0.0, 3], "FP32", [-0.0, 3], True),
    ("UINT16", [65535, 3], "FP32", [65535.0, 3], True),
]


@pytest.mark.parametrize("ta,xa,tb,xb,verdict", MIXED_PAIRS)
def test_isequal_unifies_types_like_the_host(gb, ta, xa, tb, xb, verdict):
    """Mixed-type pairs are compared in ``dtypes.unify`` of the two types (numpy's promote_types: INT8 / UINT8 -> INT16, INT64 / UINT64
    -> FP64), not in the wider of the two: -1 and 2^k - 1 are different numbers."""
    assert np_isequal(xa, ta, xb, tb) == verdict
    r, c = np.array([0, 2]), np.array([64, 1])
    for iso_pad in (False, True):
        A = gb.Matrix.from_coo(r, c, np.asarray(xa, NP_OF[ta]), dtype=ta, nrows=3, ncols=65)
        B = gb.Matrix.from_coo(r, c, np.asarray(xb, NP_OF[tb]), dtype=tb, nrows=3, ncols=65)
        if iso_pad:  # the same claim through iso storage: one stored value each
            A = gb.Matrix.from_coo(r, c, np.asarray(xa[:1] * 2, NP_OF[ta]), dtype=ta, nrows=3, ncols=65)
            B = gb.Matrix.from_coo(r, c, np.asarray(xb[:1] * 2, NP_OF[tb]), dtype=tb, nrows=3, ncols=65)
            want = np_isequal(xa[:1], ta, xb[:1], tb)
        else:
            want = verdict
        assert A.isequal(B) == want and B.isequal(A) == want, (ta, tb, iso_pad)
        assert A.isclose(B, rel_tol=1e-12, abs_tol=0.0) == want and B.isclose(A, rel_tol=1e-12) == want, (ta, tb, iso_pad, "isclose")


def test_isequal_over_all_type_pairs(gb):
    """Every ordered pair of the 11 types, on values where the wrapping cast and the promotion disagree (the smaller type's min / max /
    -1 against the bit pattern the other type would wrap them to) and on small values every type holds."""
    r, c = np.array([0, 1, 2]), np.array([0, 64, 3])
    for ta in ALL_TYPES:
        for tb in ALL_TYPES:
            if ta == "BOOL":
                xa = np.array([True, False, True])
            elif ta in FP_TYPES:
                xa = np.array([-1.0, 3.0, 200.0], NP_OF[ta])
            else:
                info = np.iinfo(NP_OF[ta])
                xa = np.array([info.min, info.max, -1 if info.min < 0 else info.max // 2 + 1], NP_OF[ta])
            with np.errstate(all="ignore"):
                wrapped = ocast(xa, tb)  # (what a cast into B's type makes of A's values)
            for xb in (wrapped, ocast(np.array([1, 0, 1]), tb)):
                for xa_ in (xa, ocast(np.array([1, 0, 1]), ta)):
                    A = gb.Matrix.from_coo(r, c, xa_, dtype=ta, nrows=3, ncols=65)
                    B = gb.Matrix.from_coo(r, c, xb, dtype=tb, nrows=3, ncols=65)
                    assert A.isequal(B) == np_isequal(xa_, ta, xb, tb), (ta, xa_, tb, xb)


def test_isequal_patterns_and_storage(gb):
    """NaN is not equal to NaN; iso against expanded storage of the same values; the same column array and nvals under different row
    pointers; a difference in the last entry only and in the last row pointer only; nvals > nrows + 1 and nrows + 1 > nvals."""
    nan = np.array([np.nan, 1.0])
    A = gb.Matrix.from_coo([0, 1], [0, 1], nan, nrows=3, ncols=65)
    assert not A.isequal(gb.Matrix.from_coo([0, 1], [0, 1], nan, nrows=3, ncols=65)) and not A.isclose(A.dup())
    allnan = gb.Matrix.from_coo([0, 1], [0, 1], [np.nan, np.nan], nrows=3, ncols=65)
    assert stored_iso(allnan) and not allnan.isequal(allnan.dup())
    # iso vs expanded storage of the same values
    import torch

    from graphblas_amd import device

    rng = np.random.default_rng(6100)
    for m, n, dens in ((257, 3, 0.05), (3, 257, 0.5)):  # nrows + 1 > nvals; nvals > nrows + 1
        r, c = np.nonzero(rng.random((m, n)) < dens)
        assert (r.size < m + 1) == (m > n) and r.size > 2
        ones = np.full(r.size, 7, np.int64)
        iso = gb.Matrix.from_coo(r, c, ones, nrows=m, ncols=n)
        ip, cj, cx = np_csr(r, c, ones.astype(np.float64), m)
        # (every host ingress detects iso; a CSR adopted from device arrays keeps the storage it is given)
        full = device.matrix_from_device_csr(torch.from_numpy(ip).to(_dev()), torch.from_numpy(cj.astype(np.int32)).to(_dev()),
                                             torch.from_numpy(cx).to(_dev()), m, n, "FP64", copy=True)
        assert stored_iso(iso) and not stored_iso(full)
        assert iso.isequal(full) and full.isequal(iso) and iso.isclose(full)
        # the last entry only
        x = np.arange(r.size, dtype=np.int64)
        y = x.copy()
        y[np.lexsort((c, r))[-1]] += 1
        P, Q = gb.Matrix.from_coo(r, c, x, nrows=m, ncols=n), gb.Matrix.from_coo(r, c, y, nrows=m, ncols=n)
        assert P.isequal(P.dup()) and not P.isequal(Q) and not Q.isequal(P) and not P.isclose(Q, rel_tol=1e-9)
        assert iso.isequal(gb.Matrix.from_coo(r, c, ones, nrows=m, ncols=n)) and not iso.isequal(P)
        # the last row pointer that can differ (rowptr[nrows - 1]; rowptr[nrows] is nvals): rows up to nrows - 2 only, then the last
        # entry moves from (nrows - 2, ncols - 1) to (nrows - 1, ncols - 1) -- same column array, same nvals
        flat = np.unique(np.append((r * n + c)[r < m - 2], (m - 2) * n + n - 1))
        r1, c1 = flat // n, flat % n
        r2 = r1.copy()
        r2[-1] = m - 1
        x1 = np.arange(r1.size, dtype=np.int64)
        P, Q = gb.Matrix.from_coo(r1, c1, x1, nrows=m, ncols=n), gb.Matrix.from_coo(r2, c1, x1, nrows=m, ncols=n)
        ep, eq = np_csr(r1, c1, x1, m)[0], np_csr(r2, c1, x1, m)[0]
        assert np.flatnonzero(ep != eq).tolist() == [m - 1]
        assert not P.isequal(Q) and not Q.isequal(P) and not P.isclose(Q) and P.isequal(P.dup())
    # rows {0}, {1} against rows {0, 1}, {}: one column array, one nvals, two row-pointer arrays
    P = gb.Matrix.from_coo([0, 1], [0, 1], [5, 6], nrows=2, ncols=2)
    Q = gb.Matrix.from_coo([0, 0], [0, 1], [5, 6], nrows=2, ncols=2)
    assert not P.isequal(Q) and not Q.isequal(P) and not P.isclose(Q)
    P = gb.Matrix.from_coo([0, 2], [0, 1], [5, 6], nrows=3, ncols=2)
    Q = gb.Matrix.from_coo([0, 1], [0, 1], [5, 6], nrows=3, ncols=2)  # (only rowptr[2] differs: 1 against 2)
    assert not P.isequal(Q) and not Q.isequal(P)


def np_isclose_all(x, y, rel_tol, abs_tol):
    """The reference's formula in float64, and the margin of the least certain pair (how far |x - y| is from the bound, as a factor)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = np.abs(x - y)
    bound = np.maximum(rel_tol * np.maximum(np.abs(x), np.abs(y)), abs_tol)
    ok = (x == y) | (d <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(x == y, 0.0, d / bound)
        margin = np.where(ok, np.where(ratio == 0, np.inf, 1.0 / ratio), ratio)
    return bool(ok.all()), float(margin.min())


@pytest.mark.parametrize("ta,tb", [("FP64", "FP64"), ("FP32", "FP32"), ("FP32", "FP64"), ("INT32", "FP64"), ("INT64", "INT64")])
def test_isclose_follows_the_reference_formula(gb, ta, tb):
    """``x == y or |x - y| <= max(rel_tol * max(|x|, |y|), abs_tol)``, every pair drawn a factor 8 inside or outside the bound; the
    numpy restatement must classify every pair with a margin of at least 4, so no verdict rests on rounding at the boundary."""
    rng = np.random.default_rng(6200)
    m, n = 3, 257
    r, c = np.nonzero(rng.random((m, n)) < 0.5)
    k = r.size
    ints = "INT" in ta
    base = (rng.integers(1000, 100000, k) * np.where(rng.random(k) < 0.5, -1, 1)).astype(np.float64)
    if not ints:
        base = base + rng.random(k)
    xa = base.astype(NP_OF[ta])
    for rel_tol, abs_tol in ((1e-3, 0.0), (0.0, 40.0), (1e-3, 40.0)):
        bound = np.maximum(rel_tol * np.abs(xa.astype(np.float64)), abs_tol)
        for kind in ("inside", "last outside", "first outside", "all outside"):
            f = np.full(k, 1 / 8)
            if kind == "last outside":
                f[-1] = 8
            elif kind == "first outside":
                f[0] = 8
            elif kind == "all outside":
                f[:] = 8
            delta = bound * f * np.where(rng.random(k) < 0.5, -1, 1)
            if "INT" in tb:
                delta = np.where(f < 1, np.floor(np.abs(delta)), np.ceil(np.abs(delta))) * np.sign(delta)
            xb = (xa.astype(np.float64) + delta).astype(NP_OF[tb])
            t = O.unify(ta, tb)  # (the comparison runs on the values as the unified type holds them)
            want, margin = np_isclose_all(O.cast(xa, t), O.cast(xb, t), rel_tol, abs_tol)
            assert margin >= 4, (ta, tb, rel_tol, abs_tol, kind, margin)
            assert want == (kind == "inside"), (ta, tb, rel_tol, abs_tol, kind)
            A = gb.Matrix.from_coo(r, c, xa, dtype=ta, nrows=m, ncols=n)
            B = gb.Matrix.from_coo(r, c, xb, dtype=tb, nrows=m, ncols=n)
            assert A.isclose(B, rel_tol=rel_tol, abs_tol=abs_tol) == want, (ta, tb, rel_tol, abs_tol, kind)
            assert B.isclose(A, rel_tol=rel_tol, abs_tol=abs_tol) == want, (ta, tb, rel_tol, abs_tol, kind, "swapped")
