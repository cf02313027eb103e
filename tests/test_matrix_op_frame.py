"""The frame the matrix operations share: descriptor, mask / accumulator checks, the rule that the complement of
no mask writes nothing, `T` held by an owner, the value helpers (operand casts, "T in the output type", iso expansion) and the write
rule -- driven through the C ABI of the five operations that end in it, on both tiers:

    GrB_mxm (plus_times)   GrB_Matrix_eWiseAdd_BinaryOp (plus; merged, and passed through beside an empty operand)
    GrB_Matrix_select_INT64 (TRIL)   GrB_Matrix_extract (strictly increasing J)   GrB_transpose

One matrix: 70 x 130 (130 x 130 where the operation needs a square one), one row of 100 entries -- more than a wavefront --, several
empty rows, no dimension a multiple of 64.  `T` is restated here with numpy on dense (value, present) arrays (the product by the
oracle), the write rule by oracle/dense_eval.py; every result is compared element for element, as tests/test_matrix_ewise.py does.
The kernels' own limits are the subject of the limit tests; these are the seams the shared helpers sit on.
"""
import ctypes

import numpy as np
import pytest

from oracle import dense_eval
from oracle import grb_oracle as O
from tests.backend import DEVICES, bind

OPS = ["mxm", "ewise_add", "ewise_add_pass", "select", "extract", "transpose"]
PREFIX = {"mxm": "mxm", "ewise_add": "eWise", "ewise_add_pass": "eWise", "select": "GrB_select", "extract": "GrB_Matrix_extract",
          "transpose": "GrB_transpose"}
KEEPS_ISO = {"ewise_add_pass", "select", "extract", "transpose"}  # T of an iso input is iso when nothing masks or accumulates
N = 130
A_VAL, B_VAL, TRIL_K = 3, 2, 10


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


def _handle(L, name):
    return ctypes.c_void_p(ctypes.c_void_p.in_dll(L, name).value)


def _error(L, C):
    s = ctypes.c_char_p()
    L.GrB_Matrix_error(ctypes.byref(s), C._carg)
    return (s.value or b"").decode()


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def stored_iso(A):
    from graphblas_amd import _lib

    dp, dj, dx, nv, iso = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    assert _lib.lib.GrX_Matrix_export_CSR_device(ctypes.byref(dp), ctypes.byref(dj), ctypes.byref(dx), ctypes.byref(nv), ctypes.byref(iso), A._carg) == 0
    return bool(iso.value)


def pattern(rng, m, n=N):
    """m x n: row 5 holds 100 entries, rows 0, 9, 10, 33 and the last are empty, the others 0 .. 12."""
    has = np.zeros((m, n), bool)
    for i in range(m):
        k = 100 if i == 5 else (0 if i in (0, 9, 10, 33, m - 1) else int(rng.integers(0, 13)))
        has[i, rng.choice(n, k, replace=False)] = True
    return has


def iso_matrix(gb, has, value, tname):
    r, c = np.nonzero(has)
    indptr = np.concatenate([[0], np.cumsum(has.sum(axis=1))])
    M = gb.Matrix.ss.import_csr(nrows=has.shape[0], ncols=has.shape[1], indptr=indptr, values=np.array([value], O.NP_OF[tname]), col_indices=c,
                                is_iso=True, sorted_cols=True, dtype=tname)
    assert stored_iso(M) and M.nvals == r.size
    return M


def matrix_of(gb, val, has, tname):
    r, c = np.nonzero(has)
    if r.size == 0:
        return gb.Matrix(tname, *has.shape)
    return gb.Matrix.from_coo(r, c, val[r, c], dtype=tname, nrows=has.shape[0], ncols=has.shape[1])


def draw(rng, shape, dens, lo, hi, np_t):
    has = rng.random(shape) < dens
    val = np.where(has, rng.integers(lo, hi, shape), 0).astype(np_t)
    return val, has


class Case:
    """One operation on A (iso INT8 with value 3, or -- `a_vals` -- INT64 with its own values): the C call, and T restated densely."""

    def __init__(self, gb, op, rng, square=False, a_vals=False):
        from graphblas_amd import _lib

        self.gb, self.op, self.L = gb, op, _lib.lib
        m = N if square else 70
        self.A_has = pattern(rng, m)
        if a_vals:
            self.A_val = np.where(self.A_has, rng.integers(1, 6, self.A_has.shape), 0).astype(np.int64)
            self.A = matrix_of(gb, self.A_val, self.A_has, "INT64")
        else:
            self.A_val = np.where(self.A_has, A_VAL, 0).astype(np.int64)
            self.A = iso_matrix(gb, self.A_has, A_VAL, "INT8")
        self.keep = []
        if op == "mxm":
            B_has = rng.random((N, N)) < 0.1
            B_has[:, 64] = False
            self.B = iso_matrix(gb, B_has, B_VAL, "INT8")
            oa = O.OMat.from_coo(*np.nonzero(self.A_has), self.A_val[self.A_has], m, N, "INT64")
            ob = O.OMat.from_coo(*np.nonzero(B_has), np.full(int(B_has.sum()), B_VAL, np.int64), N, N, "INT64")
            T = O.mxm_product(oa, ob, "plus_times")
            rows = np.repeat(np.arange(m), np.diff(T.indptr))
            self.T_has, self.T_val = np.zeros((m, N), bool), np.zeros((m, N), np.int64)
            self.T_has[rows, T.indices], self.T_val[rows, T.indices] = True, T.values
            count = self.A_has.astype(np.int64) @ B_has.astype(np.int64)  # (the oracle against plain numpy)
            assert np.array_equal(self.T_has, count > 0) and (a_vals or np.array_equal(self.T_val, A_VAL * B_VAL * count))
        elif op in ("ewise_add", "ewise_add_pass"):
            B_val, B_has = draw(rng, self.A_has.shape, 0.0 if op == "ewise_add_pass" else 0.08, 1, 10, np.int8)
            self.B = matrix_of(gb, B_val, B_has, "INT8")
            self.T_has, self.T_val = self.A_has | B_has, self.A_val + B_val
            assert op == "ewise_add_pass" or (self.A_has & B_has).any()
        elif op == "select":
            i, j = np.indices(self.A_has.shape)
            self.T_has = self.A_has & (j <= i + TRIL_K)
            self.T_val = np.where(self.T_has, self.A_val, 0)
        elif op == "extract":
            # C is A: every row, reversed, and the run of all columns; else 50 rows with repeats and 60 strictly increasing columns
            I = np.arange(m)[::-1] if square else rng.integers(0, m, 50)
            J = np.arange(N) if square else np.sort(rng.choice(N, 60, replace=False))
            self.T_has, self.T_val = self.A_has[np.ix_(I, J)], self.A_val[np.ix_(I, J)]
            self.keep = [_u64(I), _u64(J)]
        else:
            self.T_has, self.T_val = self.A_has.T.copy(), self.A_val.T.copy()
        self.shape = self.T_has.shape
        assert self.T_has.any() and not self.T_has.all()

    def call(self, C, Mask=None, accum=None, desc=None):
        L, A = self.L, self.A
        c, mk = C._carg, Mask._carg if Mask is not None else None
        acc, d = _handle(L, accum) if accum else None, _handle(L, desc) if desc else None
        if self.op == "mxm":
            return L.GrB_mxm(c, mk, acc, _handle(L, "GrB_PLUS_TIMES_SEMIRING_INT64"), A._carg, self.B._carg, d)
        if self.op in ("ewise_add", "ewise_add_pass"):
            return L.GrB_Matrix_eWiseAdd_BinaryOp(c, mk, acc, _handle(L, "GrB_PLUS_INT64"), A._carg, self.B._carg, d)
        if self.op == "select":
            return L.GrB_Matrix_select_INT64(c, mk, acc, _handle(L, "GrB_TRIL"), A._carg, TRIL_K, d)
        if self.op == "extract":
            (I, pI), (J, pJ) = self.keep
            return L.GrB_Matrix_extract(c, mk, acc, A._carg, pI, I.size, pJ, J.size, d)
        return L.GrB_transpose(c, mk, acc, A._carg, d)


def same(C, val, has, where):
    I, J, X = C.to_coo()
    r, c = np.nonzero(has)
    assert I.tolist() == r.tolist() and J.tolist() == c.tolist(), (where, "pattern")
    assert X.dtype == val.dtype and X.tolist() == val[r, c].tolist(), (where, "values")


@pytest.mark.parametrize("op", OPS)
def test_iso_input_masked_accumulated(gb, op):
    """(a) iso INT8 input, FP64 output, a valued mask and an accumulator: the operand cast, T with one value per entry, T in C's type."""
    rng = np.random.default_rng(7100 + OPS.index(op))
    k = Case(gb, op, rng)
    C_val, C_has = draw(rng, k.shape, 0.3, -9, 10, np.float64)
    M_val, M_has = draw(rng, k.shape, 0.6, 0, 3, np.int8)  # (a third of the mask's entries hold 0)
    assert (M_val[M_has] == 0).any() and (M_val[M_has] != 0).any()
    C, M = matrix_of(gb, C_val, C_has, "FP64"), matrix_of(gb, M_val, M_has, "INT8")
    assert k.call(C, M, "GrB_PLUS_FP64") == 0, _error(k.L, C)
    N_val, N_has = dense_eval.write(C_val, C_has, k.T_val.astype(np.float64), k.T_has, M_val, M_has, accum="plus", np_t=np.float64)
    same(C, N_val, N_has, op)
    assert not stored_iso(C)


@pytest.mark.parametrize("op", OPS)
def test_iso_input_plain(gb, op):
    """(b) the same without mask and accumulator: C takes T's storage (what it held goes away), an iso T stays iso."""
    rng = np.random.default_rng(7200 + OPS.index(op))
    k = Case(gb, op, rng)
    C_val, C_has = draw(rng, k.shape, 0.3, -9, 10, np.float64)
    C = matrix_of(gb, C_val, C_has, "FP64")
    assert k.call(C) == 0, _error(k.L, C)
    same(C, k.T_val.astype(np.float64), k.T_has, op)
    assert stored_iso(C) == (op in KEEPS_ISO), op


@pytest.mark.parametrize("op", OPS)
def test_output_is_an_input(gb, op):
    """(c) C is A, with A's transpose and pull layouts cached by earlier products: the result is right, and products on the new C --
    through its rows and through its transpose -- agree with the oracle, so the caches went with the old content."""
    rng = np.random.default_rng(7300 + OPS.index(op))
    k = Case(gb, op, rng, square=True, a_vals=True)
    A = k.A
    u_idx = np.flatnonzero(rng.random(N) < 0.7)
    u_val = rng.integers(1, 5, u_idx.size).astype(np.int64)
    u = gb.Vector.from_coo(u_idx, u_val, dtype="INT64", size=N)
    ou = O.OVec(N, u_idx, u_val, "INT64")

    def products(X, val, has, where):
        ox = O.OMat.from_coo(*np.nonzero(has), val[has], N, N, "INT64")
        for mat, tr in ((X, False), (X.T, True)):
            got = mat.mxv(u, gb.semiring.plus_times).new()
            exp = O.mxv(ox, ou, "plus_times", transpose_a=tr)
            gi, gv = got.to_coo()
            assert gi.tolist() == exp.idx.tolist() and gv.tolist() == exp.vals.tolist(), (where, tr)

    products(A, k.A_val, k.A_has, "before")  # (caches A's layouts and its transpose)
    M_val, M_has = draw(rng, (N, N), 0.6, 0, 3, np.int8)
    M = matrix_of(gb, M_val, M_has, "INT8")
    assert k.call(A, M, "GrB_PLUS_INT64") == 0, _error(k.L, A)
    N_val, N_has = dense_eval.write(k.A_val, k.A_has, k.T_val, k.T_has, M_val, M_has, accum="plus", np_t=np.int64)
    same(A, N_val, N_has, op)
    products(A, N_val, N_has, "after")


@pytest.mark.parametrize("op", OPS)
def test_complement_of_no_mask(gb, op):
    """(d) a complemented descriptor without a mask allows no position: C is unchanged, or emptied under replace."""
    rng = np.random.default_rng(7400 + OPS.index(op))
    k = Case(gb, op, rng)
    C_val, C_has = draw(rng, k.shape, 0.3, -9, 10, np.float64)
    C = matrix_of(gb, C_val, C_has, "FP64")
    for accum in (None, "GrB_PLUS_FP64"):
        assert k.call(C, None, accum, "GrB_DESC_C") == 0
        same(C, C_val, C_has, (op, accum, "complement"))
    assert k.call(C, None, None, "GrB_DESC_RC") == 0
    assert C.nvals == 0
    assert k.call(C) == 0  # (and the emptied C is a sound object)
    same(C, k.T_val.astype(np.float64), k.T_has, (op, "after replace"))


@pytest.mark.parametrize("op", OPS)
def test_mask_shape_check(gb, op):
    """(e) a mask of another shape than C: GrB_DIMENSION_MISMATCH, the operation's own prefix in the text, C unchanged; the same for an
    accumulator of another type than C's (GrB_DOMAIN_MISMATCH)."""
    rng = np.random.default_rng(7500 + OPS.index(op))
    k = Case(gb, op, rng)
    C_val, C_has = draw(rng, k.shape, 0.3, -9, 10, np.float64)
    C = matrix_of(gb, C_val, C_has, "FP64")
    for shape in ((k.shape[0] + 1, k.shape[1]), (k.shape[0], k.shape[1] - 1)):
        M = gb.Matrix("BOOL", *shape)
        assert k.call(C, M, "GrB_PLUS_FP64") == -6  # GrB_DIMENSION_MISMATCH
        assert _error(k.L, C) == PREFIX[op] + ": mask shape does not match the output"
        same(C, C_val, C_has, (op, shape))
    assert k.call(C, None, "GrB_PLUS_INT64") == -5  # GrB_DOMAIN_MISMATCH
    assert _error(k.L, C) == PREFIX[op] + ": accum operator type must equal the output type"
    same(C, C_val, C_has, (op, "accum"))
