"""GrB_Matrix_diag / GxB_Vector_diag: ``v.diag(k)`` and ``A.diag(k)`` -- k_diag_popc / k_diag_fill / k_diag_extract of grb_diag.hip on the
GPU tier, the same sources under the SIMT emulator on the CPU tier.

The rules are restated HERE in numpy: ``C(i + max(-k, 0), i + max(k, 0)) = v(i)`` in a square matrix of order ``n + |k|`` whose row pointers
are checked whole (CSR export); ``v(i) = A(i + max(-k, 0), i + max(k, 0))`` over the diagonal's length ``min(m, n - k)`` / ``min(m + k, n)``.
Values are moved or cast by ``O.cast``, so everything compares bit for bit.  The reference's own test_diag
(tests/golden/union_diag_literals.json) comes first."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import grb_oracle as O
from tests.backend import DEVICES, ROOT, bind
from tests.test_cast_chain import compare_values
from tests.values import ALL_TYPES, rand_vals

NP_OF = O.NP_OF


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


@pytest.fixture(scope="module")
def literals():
    with open(os.path.join(ROOT, "tests", "golden", "union_diag_literals.json")) as f:
        return json.load(f)


def diag_len(m, n, k):
    return min(m, n - k) if 0 <= k < n else (min(m + k, n) if -m < k < 0 else 0)


def check_diag_matrix(C, idx, vals, n, k, tname, where):
    """C against the rule: shape, type, the WHOLE row-pointer array, columns, values"""
    order = n + abs(k)
    assert C.shape == (order, order) and C.dtype.name == tname, where
    Cp, Cj, Cx = C.to_csr()
    counts = np.zeros(order, np.int64)
    counts[idx + max(-k, 0)] = 1
    assert Cp.astype(np.int64).tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist(), (where, "row pointers")
    assert Cj.astype(np.int64).tolist() == (idx + max(k, 0)).tolist(), (where, "columns")
    compare_values(Cx, vals, None, where)
    assert C.nvals == idx.size, where


def check_vector(w, idx, vals, size, tname, where):
    assert w.size == size and w.dtype.name == tname, where
    I, X = w.to_coo()
    assert I.astype(np.int64).tolist() == np.asarray(idx).tolist() and w.nvals == len(idx), (where, "pattern")
    compare_values(X, vals, None, where)


# ---- 1. symbols, the reference's test_diag ------------------------------------------------------------------------------------------
def test_symbols_and_literals(gb, literals):
    from graphblas_amd import _lib

    L = _lib.lib
    header = open(os.path.join(ROOT, "include", "grb_mi355x.h")).read()
    assert hasattr(L, "GxB_Vector_diag") and "GrB_Info GxB_Vector_diag(" in header and "GrB_Info GrB_Matrix_diag(" in header
    assert L.GrB_Matrix_diag(None, None, 0) == -2  # GrB_NULL_POINTER
    out = ctypes.c_void_p()
    assert L.GrB_Matrix_diag(ctypes.byref(out), None, 0) == -2 and not out.value
    lit = literals["diag"]
    fx = lit["v"]
    idx, vals = np.asarray(fx["idx"], np.int64), np.asarray(fx["vals"], NP_OF[fx["dtype"]])
    v = gb.Vector.from_coo(idx, vals, size=fx["size"], dtype=fx["dtype"])
    assert [c["k"] for c in lit["matrices"]] == list(range(-5, 5))
    for case in lit["matrices"]:
        k, where = case["k"], f"recorded matrix k={case['k']}"
        for kk in (k, gb.Scalar.from_value(k)):  # an int, or a Scalar that holds one
            C = v.diag(kk)
            assert C.shape == (case["order"], case["order"]) and C.dtype.name == fx["dtype"], where
            I, J, X = C.to_coo()
            assert (I.tolist(), J.tolist(), X.tolist()) == (case["rows"], case["cols"], case["vals"]), where
            check_diag_matrix(C, idx, vals, fx["size"], k, fx["dtype"], where)  # (the recorded tuples and this file's rule agree)
        # and back out of the recorded matrix, built from its tuples: by a Scalar k in its own type, through the transpose as FP64
        R = gb.Matrix.from_coo(case["rows"], case["cols"], case["vals"], nrows=case["order"], ncols=case["order"], dtype=fx["dtype"])
        check_vector(R.diag(gb.Scalar.from_value(k)), idx, vals, fx["size"], lit["extracted_dtypes"]["same_k"], where + " extracted")
        check_vector(R.T.diag(-k, dtype=float), idx, vals.astype(np.float64), fx["size"], lit["extracted_dtypes"]["transposed_minus_k_as_float"],
                     where + " extracted through the transpose")
    with pytest.raises(TypeError):
        v.diag(1.5)
    with pytest.raises(ValueError):
        v.diag(gb.Scalar(int))


# ---- 2. vector -> matrix, and back ------------------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 4095, 4096, 4097]


def patterns(rng, n):
    corner = np.unique([i for i in (0, 63, 64, n - 1) if i < n])
    return {"empty": np.zeros(0, np.int64), "full": np.arange(n), "corners": corner.astype(np.int64),
            "random": np.flatnonzero(rng.random(n) < 0.3)}


@pytest.mark.parametrize("n", SIZES)
def test_vector_to_matrix_and_back(gb, n):
    from graphblas_amd import device

    rng = np.random.default_rng(8100 + n)
    ks = sorted({0, 1, -1, 64, -64, n - 1, -(n - 1)})
    types = ALL_TYPES  # (all 11 at every size; the k list is the full one for INT64 and up to n = 65)
    for tname in types:
        for kind, idx in patterns(rng, n).items():
            for iso in ((False, True) if kind == "random" else (False,)):
                vals = rand_vals(rng, idx.size, tname, "exact") if tname.startswith("FP") else rand_vals(rng, idx.size, tname)
                if iso and idx.size:
                    vals = np.full(idx.size, vals[0])
                v = gb.Vector.from_coo(idx, vals, dtype=tname, size=n)
                for k in ks if (tname == "INT64" or n <= 65) else (0, -1, 64):
                    where = f"n={n} {tname} {kind} iso={iso} k={k}"
                    C = v.diag(k)
                    assert device.last_stats()["method"] == (23 if idx.size else 6), where
                    check_diag_matrix(C, idx, vals, n, k, tname, where)
                    back = C.diag(k)
                    assert device.last_stats()["method"] == (24 if idx.size else 6), where
                    check_vector(back, idx, vals, n, tname, where + " round trip")
                    if k:  # the neighbouring diagonals of C hold nothing
                        assert C.diag(0).nvals == 0 and C.diag(-k).nvals == 0, where


@pytest.mark.parametrize("n,k", [(1, 100000), (1, -100000), (70, 300001), (70, -300001)])
def test_short_vector_far_off_the_main_diagonal(gb, n, k):
    """|k| much larger than n: the rows outside the diagonal's are most of Cp, written by more wavefronts than the vector has words."""
    from graphblas_amd import device

    idx = np.unique([0, n // 2, n - 1]).astype(np.int64)
    vals = np.arange(1, idx.size + 1, dtype=np.int32)
    C = gb.Vector.from_coo(idx, vals, dtype="INT32", size=n).diag(k)
    st = device.last_stats()
    assert st["method"] == 23 and st["tiles"] >= 32 > (n + 63) // 64 and st["out_nvals"] == idx.size, st
    check_diag_matrix(C, idx, vals, n, k, "INT32", f"n={n} k={k}")
    check_vector(C.diag(k), idx, vals, n, "INT32", f"n={n} k={k} round trip")
    assert device.last_stats()["method"] == 24 and device.last_stats()["out_nvals"] == -1


# ---- 3. matrix -> vector ----------------------------------------------------------------------------------------------------------------
def coo_diag(rows, cols, vals, m, n, k):
    """(indices, values) of diagonal k of the COO matrix"""
    on = cols - rows == k
    i = rows[on] - max(-k, 0)
    order = np.argsort(i)
    return i[order], vals[on][order]


def diagonals_of(m, n):
    """0, +-1, the last non-empty diagonal on each side, one past it (length 0), far outside"""
    return sorted({0, 1, -1, n - 1, n, -(m - 1), -m, 10 * n, -10 * m})


@pytest.mark.parametrize("shape", [(65, 130), (65, 65), (130, 65)])
def test_matrix_to_vector(gb, shape):
    rng = np.random.default_rng(8200 + shape[0] * 3 + shape[1])
    m, n = shape
    r, c = np.nonzero(rng.random(shape) < 0.35)
    for tname in ("INT64", "FP64", "BOOL"):
        vals = rand_vals(rng, r.size, tname, "exact") if tname.startswith("FP") else rand_vals(rng, r.size, tname)
        A = gb.Matrix.from_coo(r, c, vals, dtype=tname, nrows=m, ncols=n)
        for k in diagonals_of(m, n):
            idx, dv = coo_diag(r, c, vals, m, n, k)
            where = f"{shape} {tname} k={k}"
            check_vector(A.diag(k), idx, dv, diag_len(m, n, k), tname, where)
            check_vector(A.T.diag(-k), idx, dv, diag_len(m, n, k), tname, where + " through A.T")
    # dtype= other than A's: the FP64 -> INT8 cast saturates, NaN -> 0; FP64 -> BOOL; INT64 -> FP32
    vals = rand_vals(rng, r.size, "FP64", "special")
    on = np.flatnonzero(c == r)[:6]  # (on the main diagonal, where the casts are looked at)
    assert on.size == 6
    vals[on] = [300.7, -129.5, np.nan, np.inf, -np.inf, 127.9]
    A = gb.Matrix.from_coo(r, c, vals, dtype="FP64", nrows=m, ncols=n)
    for k in (0, 1, -1):
        idx, dv = coo_diag(r, c, vals, m, n, k)
        for to in ("INT8", "BOOL", "FP32", "UINT64"):
            with np.errstate(all="ignore"):
                check_vector(A.diag(k, dtype=to), idx, O.cast(dv, to), diag_len(m, n, k), to, f"{shape} FP64 -> {to} k={k}")


def test_row_shapes_and_iso(gb):
    """70 x 6000, k = 3 (the wanted column of row i is i + 3): rows of 0 / 1 / 64 / 65 / 5000 entries with the diagonal entry first in its
    row, last in its row, absent between two neighbours, absent beyond the row's last column."""
    from tests.test_matrix_ewise import stored_iso

    rng = np.random.default_rng(8300)
    m, n, k = 70, 6000, 3

    def others(i, count, lo, hi):
        pool = np.setdiff1d(np.arange(lo, hi), [i + k])
        return np.sort(rng.choice(pool, count, replace=False))

    rows = {
        1: np.array([1 + k]),                                               # 1 entry: the diagonal's
        2: np.array([2 + k + 1]),                                           # 1 entry: beside it
        3: np.concatenate([[3 + k], others(3, 63, 3 + k + 1, n)]),          # 64 entries, the diagonal entry first
        4: np.arange(4 + k + 1),                                            # 8 entries, the diagonal entry last
        5: np.concatenate([[5 + k - 1, 5 + k + 1], others(5, 63, 5 + k + 2, n)]),   # 65 entries, absent between two neighbours
        6: np.arange(6 + k),                                                # absent beyond the row's last column
        7: np.sort(np.concatenate([[7 + k], others(7, 4999, 0, n)])),       # 5000 entries, present
        8: others(8, 5000, 0, n),                                           # 5000 entries, absent
        66: np.concatenate([others(66, 64, 0, 66 + k), [66 + k]]),          # 65 entries, the diagonal entry last
        69: np.array([0, 69 + k, n - 1]),
    }
    r = np.concatenate([np.full(c.size, i, np.int64) for i, c in rows.items()])
    c = np.concatenate(list(rows.values())).astype(np.int64)
    vals = rng.integers(1, 1000, r.size)
    A = gb.Matrix.from_coo(r, c, vals, dtype="INT64", nrows=m, ncols=n)
    for kk in (k, 0, k + 1, k - 1, -1):
        idx, dv = coo_diag(r, c, vals, m, n, kk)
        check_vector(A.diag(kk), idx, dv, diag_len(m, n, kk), "INT64", f"rows k={kk}")
    assert A.diag(k).to_coo()[0].tolist() == [1, 3, 4, 7, 66, 69]
    order = np.lexsort((c, r))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))])
    Ai = gb.Matrix.ss.import_csr(nrows=m, ncols=n, indptr=indptr, values=np.array([2.5]), col_indices=c[order], is_iso=True, sorted_cols=True,
                                 dtype="FP64")
    assert stored_iso(Ai)
    idx, _ = coo_diag(r, c, vals, m, n, k)
    check_vector(Ai.diag(k), idx, np.full(idx.size, 2.5), diag_len(m, n, k), "FP64", "iso A")
    check_vector(Ai.diag(k, dtype="INT8"), idx, np.full(idx.size, 2, np.int8), diag_len(m, n, k), "INT8", "iso A, cast")


def test_c_abi_lengths_and_old_entries(gb):
    from graphblas_amd import _lib

    L = _lib.lib
    A = gb.Matrix.from_coo([0, 1, 2, 64], [0, 1, 5, 64], [10, 11, 12, 13], nrows=65, ncols=130)
    v = gb.Vector.from_coo([0, 3, 64], [1, 2, 3], size=65)
    for size, k in ((64, 0), (66, 0), (65, 66), (65, -1), (130, 0)):  # (diagonal 66 has 64 positions, diagonal -1 too)
        w = gb.Vector.from_coo([0, 1], [7, 8], size=size)
        assert L.GxB_Vector_diag(w._carg, A._carg, k, None) == -6, (size, k)  # GrB_DIMENSION_MISMATCH
        assert [x.tolist() for x in w.to_coo()] == [[0, 1], [7, 8]], (size, k)
    assert L.GxB_Vector_diag(None, A._carg, 0, None) == -2 and L.GxB_Vector_diag(v._carg, None, 0, None) == -2
    # entries of v beyond the new pattern go: positions 3 and 64 held entries, the diagonal holds 0, 1 and 64
    assert L.GxB_Vector_diag(v._carg, A._carg, 0, None) == 0
    assert v.nvals == 3 and [x.tolist() for x in v.to_coo()] == [[0, 1, 64], [10, 11, 13]]
    # ... also when the diagonal is empty, when A is, and when the length is 0; the descriptor is ignored
    desc = ctypes.c_void_p(ctypes.c_void_p.in_dll(L, "GrB_DESC_T0").value)
    w = gb.Vector.from_coo([0, 63], [7, 8], size=64)
    assert L.GxB_Vector_diag(w._carg, A._carg, 66, desc) == 0 and w.nvals == 0 and w.to_coo()[0].size == 0
    w = gb.Vector.from_coo([0, 64], [7, 8], size=65)
    assert L.GxB_Vector_diag(w._carg, gb.Matrix(int, 65, 130)._carg, 0, None) == 0 and w.nvals == 0
    w = gb.Vector(int, 0)
    assert L.GxB_Vector_diag(w._carg, A._carg, 130, None) == 0 and L.GxB_Vector_diag(w._carg, A._carg, -65, None) == 0 and w.nvals == 0
    # a vector grown afterwards shows no phantom entry (GrB_Vector_resize copies whole presence words)
    d = A.diag(0)
    d.resize(200)
    assert d.nvals == 3 and d.to_coo()[0].tolist() == [0, 1, 64]
    # a wider output type than A's
    f = gb.Vector(float, 65)
    assert L.GxB_Vector_diag(f._carg, A._carg, 0, None) == 0 and f.to_coo()[1].tolist() == [10.0, 11.0, 13.0]


# ---- 4. the Laplacian ---------------------------------------------------------------------------------------------------------------------
def test_laplacian(gb):
    rng = np.random.default_rng(8400)
    n = 200
    dense = np.triu(rng.random((n, n)) < 0.05, 1)
    dense = dense | dense.T
    dense[17] = dense[:, 17] = False  # an isolated vertex: no degree, no diagonal entry
    r, c = np.nonzero(dense)
    A = gb.Matrix.from_coo(r, c, np.ones(r.size, np.int64), dtype="INT64", nrows=n, ncols=n)
    d = A.reduce_rowwise().new()
    Lap = d.diag().ewise_union(A, gb.binary.minus, 0, 0).new()
    want = np.diag(dense.sum(1)).astype(np.int64) - dense.astype(np.int64)
    has = dense | np.diag(dense.any(1))
    I, J, X = Lap.to_coo()
    rr, cc = np.nonzero(has)
    assert I.tolist() == rr.tolist() and J.tolist() == cc.tolist() and X.tolist() == want[rr, cc].tolist()
    assert Lap.reduce_rowwise().new().reduce(gb.monoid.max).value == 0  # rows of a Laplacian sum to 0
    assert Lap.diag().isequal(d)
    # the convergence check of the issue: max |C - prev| through the union
    prev = Lap.dup()
    assert Lap.ewise_union(prev, gb.binary.minus, 0, 0).new().reduce_scalar(gb.monoid.max).new().value == 0
