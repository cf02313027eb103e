"""The frame the vector operations share (the vector half): descriptor, mask / accumulator checks, the rule that
the complement of no mask writes nothing, the mask's words (borrowed from a structural mask, a snapshot otherwise -- and always when the
mask is `w`), the value helpers (operand casts, "t in w's type") and the write rule -- driven through the C ABI of every operation that
ends in it, on both tiers:

    GrB_mxv / GrB_vxm (plus_times; vxm once more through the push direction)   GrB_mxv (GxB_MIN_SECONDI_INT64)
    GrB_Vector_eWiseAdd_BinaryOp / eWiseMult_BinaryOp (plus)   GxB_Vector_eWiseUnion
    GrB_Vector_select_INT64 (VALUEGT, ROWLE)   GrB_Vector_apply_BinaryOp2nd_INT64 (plus) / apply_IndexOp_INT64 (ROWINDEX)
    GrB_Vector_extract (a list with repeats)   GrB_Col_extract (a list, GrB_ALL, the row form under T0)
    GrB_Vector_assign (indexed)   GrB_Vector_assign_INT64 (GrB_ALL, indexed)

n = 1000: 15 full presence words and a tail of 40 bits, four workgroups of 256.  The matrix is 1000 x 1000, row 5 holds 100 entries --
more than a wavefront --, several rows are empty.  `t` is restated here with numpy on dense (value, present) arrays (the mxv product by
the oracle), the write rule by oracle/dense_eval.py; every result is compared element for element.  Every value is an integer that FP64
holds exactly.  The kernels' own limits are the subject of the limit tests; these are the seams the shared helpers sit on.
"""
import ctypes

import numpy as np
import pytest

from oracle import dense_eval
from oracle import grb_oracle as O
from tests.backend import DEVICES, bind

N = 1000
MXV_OPS = ["mxv", "vxm", "vxm_push", "mxv_posn"]
EWISE_OPS = ["ewise_add", "ewise_mult", "ewise_union"]
OPS = MXV_OPS + EWISE_OPS + ["select_value", "select_pos", "apply_2nd", "apply_index", "extract", "col_extract_list", "col_extract_all",
                             "col_extract_row", "assign", "assign_scalar_all", "assign_scalar_idx"]
OPS_WITH_U = [op for op in OPS if not op.startswith(("col_extract", "assign_scalar"))]
OPS_WITH_OPERAND = [op for op in OPS if not op.startswith("assign_scalar")]
USES_MATRIX = set(MXV_OPS) | {"col_extract_list", "col_extract_all", "col_extract_row"}
# the texts of the parent commit's sources (csrc/grb_mxv.hip, grb_mxv_posn.hip, grb_vecops.hip, grb_select.hip, grb_apply.hip, grb_extract.hip)
PREFIX = {"mxv": "mxv/vxm", "vxm": "mxv/vxm", "vxm_push": "mxv/vxm", "mxv_posn": "mxv/vxm", "ewise_add": "eWise", "ewise_mult": "eWise",
          "ewise_union": "eWise", "select_value": "GrB_select", "select_pos": "GrB_select", "apply_2nd": "GrB_apply", "apply_index": "GrB_apply",
          "extract": "extract", "col_extract_list": "GrB_Col_extract", "col_extract_all": "GrB_Col_extract", "col_extract_row": "GrB_Col_extract",
          "assign": "assign", "assign_scalar_all": "assign", "assign_scalar_idx": "assign"}
MASK_TEXT = {op: p + (": mask size does not match output size" if p == "mxv/vxm" else ": mask size does not match the output size")
             for op, p in PREFIX.items()}
ACCUM_TEXT = {op: p + ": accum operator type must equal the output type" for op, p in PREFIX.items()}
SR = "GrB_PLUS_TIMES_SEMIRING_INT64"
J_COL, J_ROW = 7, 5  # the column / (under T0) the row GrB_Col_extract takes: row 5 is the long one
GT_K, ROW_K, Y, X, ALPHA, BETA = 2, 700, 3, 4, 5, -6


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


def _handle(L, name):
    return ctypes.c_void_p(ctypes.c_void_p.in_dll(L, name).value)


def _error(L, w):
    s = ctypes.c_char_p()
    L.GrB_Vector_error(ctypes.byref(s), w._carg)
    return (s.value or b"").decode()


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def pattern(rng):
    """N x N: row 5 holds 100 entries, rows 0, 9, 10, 33 and the last are empty, the others 0 .. 12; column J_COL is not empty."""
    has = np.zeros((N, N), bool)
    for i in range(N):
        k = 100 if i == 5 else (0 if i in (0, 9, 10, 33, N - 1) else int(rng.integers(0, 13)))
        has[i, rng.choice(N, k, replace=False)] = True
    has[20:400:7, J_COL] = True
    return has


def draw(rng, n, dens, lo, hi, np_t):
    has = rng.random(n) < dens
    val = np.where(has, rng.integers(lo, hi, n), 0).astype(np_t)
    return val, has


def vec_of(gb, val, has, tname):
    idx = np.flatnonzero(has)
    if idx.size == 0:
        return gb.Vector(tname, has.size)
    return gb.Vector.from_coo(idx, val[idx], dtype=tname, size=has.size)


def dense_of(ov):
    has, val = ov.dense()
    return val.astype(np.int64), has.astype(bool)


class Case:
    """One operation on inputs of type `tname`: the C call, and `t` restated densely in INT64 (every operator here is an INT64 one).
    empty: "u" -- the vector operand holds no entry; "A" -- the matrix holds none.  alias: the index list of assign covers all of w,
    so that u can be w."""

    def __init__(self, gb, op, rng, tname="INT8", empty=None, alias=False):
        from graphblas_amd import _lib

        self.gb, self.op, self.L, self.tname = gb, op, _lib.lib, tname
        self.all = _lib.all_indices()
        self.ni = N if (alias or op != "assign") else 600
        self.u_val, self.u_has = draw(rng, self.ni, 0.01 if op == "vxm_push" else 0.7, -9, 10, np.int64)
        if op in MXV_OPS:
            self.u_val = np.abs(self.u_val) + self.u_has  # (1 .. 10)
        if op == "vxm_push":
            self.u_has[5], self.u_val[5] = True, 2  # (the long row is on the frontier)
        if empty == "u":
            self.u_val, self.u_has = np.zeros(self.ni, np.int64), np.zeros(self.ni, bool)
        self.u = vec_of(gb, self.u_val, self.u_has, tname)
        self.v_val, self.v_has = draw(rng, N, 0.5, -9, 10, np.int64)
        self.v = vec_of(gb, self.v_val, self.v_has, tname) if op in EWISE_OPS else None
        if op in USES_MATRIX:
            self.A_has = pattern(rng) if empty != "A" else np.zeros((N, N), bool)
            self.A_val = np.where(self.A_has, rng.integers(1, 6, (N, N)), 0).astype(np.int64)
            r, c = np.nonzero(self.A_has)
            self.A = gb.Matrix.from_coo(r, c, self.A_val[r, c], dtype=tname, nrows=N, ncols=N) if r.size else gb.Matrix(tname, N, N)
        if op in ("extract", "col_extract_list"):
            self.I = rng.integers(0, N, N)  # (with repeats)
            assert np.unique(self.I).size < N
        elif op in ("assign", "assign_scalar_idx"):
            self.I = rng.permutation(N)[: self.ni]
        else:
            self.I = np.zeros(0, np.int64)
        self.keep = _u64(self.I)
        self.scalars = []
        if op == "ewise_union":
            for x in (ALPHA, BETA):
                s = ctypes.c_void_p()
                assert self.L.GrB_Scalar_new(ctypes.byref(s), _handle(self.L, "GrB_INT64")) == 0
                assert self.L.GrB_Scalar_setElement_INT64(s, x) == 0
                self.scalars.append(s)
        self.T = self._t()

    def _t(self):
        op, u, uh, v, vh, i = self.op, self.u_val, self.u_has, self.v_val, self.v_has, np.arange(N)
        if op in MXV_OPS:
            r, c = np.nonzero(self.A_has)
            oa = O.OMat.from_coo(r, c, self.A_val[r, c], N, N, "INT64")
            ou = O.OVec(N, np.flatnonzero(uh), u[uh], "INT64")
            if op == "mxv":
                return dense_of(O.mxv(oa, ou, "plus_times"))
            if op == "mxv_posn":  # t(i) = min k over the entries A(i, k) that meet an entry u(k)
                P = self.A_has & uh[None, :]
                return np.where(P.any(axis=1), P.argmax(axis=1), 0).astype(np.int64), P.any(axis=1)
            T = dense_of(O.vxm(ou, oa, "plus_times"))
            assert np.array_equal(T[0], u @ self.A_val) and np.array_equal(T[1], (uh.astype(np.int64) @ self.A_has) > 0)  # (the oracle against numpy)
            return T
        if op == "ewise_add":
            return np.where(uh & vh, u + v, np.where(uh, u, v)), uh | vh
        if op == "ewise_mult":
            return np.where(uh & vh, u + v, 0), uh & vh
        if op == "ewise_union":
            return np.where(uh | vh, np.where(uh, u, ALPHA) + np.where(vh, v, BETA), 0), uh | vh
        if op == "select_value":
            return np.where(uh & (u > GT_K), u, 0), uh & (u > GT_K)
        if op == "select_pos":
            return np.where(uh & (i <= ROW_K), u, 0), uh & (i <= ROW_K)
        if op == "apply_2nd":
            return np.where(uh, u + Y, 0), uh
        if op == "apply_index":
            return np.where(uh, i + Y, 0), uh
        if op == "extract":
            return u[self.I], uh[self.I]
        if op == "col_extract_list":
            return self.A_val[self.I, J_COL], self.A_has[self.I, J_COL]
        if op == "col_extract_all":
            return self.A_val[:, J_COL].copy(), self.A_has[:, J_COL].copy()
        if op == "col_extract_row":
            return self.A_val[J_ROW, :].copy(), self.A_has[J_ROW, :].copy()
        if op == "assign_scalar_all":
            return np.full(N, X, np.int64), np.ones(N, bool)
        return None  # (indexed assign: Z depends on w)

    def _assigned(self, w_val, w_has, accum):
        """Z = w; Z(I) = accum ? accum(w(I), x) : x -- without accum a position of I that x does not fill loses its entry."""
        x_val, x_has = (self.u_val, self.u_has) if self.op == "assign" else (np.full(self.ni, X, np.int64), np.ones(self.ni, bool))
        Z_val, Z_has, I = w_val.copy(), w_has.copy(), self.I
        if accum:
            both, new = x_has & w_has[I], x_has & ~w_has[I]
            Z_val[I[both]] = w_val[I[both]] + x_val[both]
            Z_val[I[new]], Z_has[I[new]] = x_val[new], True
        else:
            Z_val[I], Z_has[I] = np.where(x_has, x_val, 0), x_has
        return Z_val, Z_has

    def expected(self, w_val, w_has, M=None, accum=False, comp=False, struct=False, replace=False):
        if self.T is None:
            T_val, T_has = self._assigned(w_val, w_has, accum)
            accum = False  # (GrB_assign accumulates into Z; the write rule then only masks)
        else:
            T_val, T_has = self.T
        M_val, M_has = M if M is not None else (None, None)
        return dense_eval.write(w_val, w_has, T_val.astype(w_val.dtype), T_has, M_val, M_has, comp=comp, struct=struct,
                                accum="plus" if accum else None, replace=replace, np_t=w_val.dtype.type)

    def call(self, w, mask=None, accum=None, flags="", u=None, v=None):
        L, op = self.L, self.op
        h = lambda name: _handle(L, name)  # noqa: E731
        u, v = self.u if u is None else u, self.v if v is None else v
        flags += "T0" if op == "col_extract_row" else ""
        c, mk, acc, d = w._carg, mask._carg if mask is not None else None, h(accum) if accum else None, h("GrB_DESC_" + flags) if flags else None
        plus, (I, pI) = h("GrB_PLUS_INT64"), self.keep
        if op == "mxv":
            return L.GrB_mxv(c, mk, acc, h(SR), self.A._carg, u._carg, d)
        if op == "mxv_posn":
            return L.GrB_mxv(c, mk, acc, h("GxB_MIN_SECONDI_INT64"), self.A._carg, u._carg, d)
        if op == "vxm":
            return L.GrB_vxm(c, mk, acc, h(SR), u._carg, self.A._carg, d)
        if op == "vxm_push":
            assert L.GrX_option_set(b"push_mode", 2) == 0
            try:
                return L.GrB_vxm(c, mk, acc, h(SR), u._carg, self.A._carg, d)
            finally:
                assert L.GrX_option_set(b"push_mode", 1) == 0
        if op == "ewise_add":
            return L.GrB_Vector_eWiseAdd_BinaryOp(c, mk, acc, plus, u._carg, v._carg, d)
        if op == "ewise_mult":
            return L.GrB_Vector_eWiseMult_BinaryOp(c, mk, acc, plus, u._carg, v._carg, d)
        if op == "ewise_union":
            return L.GxB_Vector_eWiseUnion(c, mk, acc, plus, u._carg, self.scalars[0], v._carg, self.scalars[1], d)
        if op == "select_value":
            return L.GrB_Vector_select_INT64(c, mk, acc, h("GrB_VALUEGT_INT64"), u._carg, GT_K, d)
        if op == "select_pos":
            return L.GrB_Vector_select_INT64(c, mk, acc, h("GrB_ROWLE"), u._carg, ROW_K, d)
        if op == "apply_2nd":
            return L.GrB_Vector_apply_BinaryOp2nd_INT64(c, mk, acc, plus, u._carg, Y, d)
        if op == "apply_index":
            return L.GrB_Vector_apply_IndexOp_INT64(c, mk, acc, h("GrB_ROWINDEX_INT64"), u._carg, Y, d)
        if op == "extract":
            return L.GrB_Vector_extract(c, mk, acc, u._carg, pI, I.size, d)
        if op == "col_extract_list":
            return L.GrB_Col_extract(c, mk, acc, self.A._carg, pI, I.size, J_COL, d)
        if op == "col_extract_all":
            return L.GrB_Col_extract(c, mk, acc, self.A._carg, self.all, N, J_COL, d)
        if op == "col_extract_row":
            return L.GrB_Col_extract(c, mk, acc, self.A._carg, self.all, N, J_ROW, d)
        if op == "assign":
            return L.GrB_Vector_assign(c, mk, acc, u._carg, pI, I.size, d)
        if op == "assign_scalar_all":
            return L.GrB_Vector_assign_INT64(c, mk, acc, X, self.all, N, d)
        return L.GrB_Vector_assign_INT64(c, mk, acc, X, pI, I.size, d)


def same(w, val, has, where):
    I, X = w.to_coo()
    assert I.tolist() == np.flatnonzero(has).tolist(), (where, "pattern")
    assert X.dtype == val.dtype and X.tolist() == val[has].tolist(), (where, "values")


def valued_mask(rng):
    M_val, M_has = draw(rng, N, 0.6, 0, 3, np.int8)  # (a third of the mask's entries hold 0)
    assert (M_val[M_has] == 0).any() and (M_val[M_has] != 0).any()
    return M_val, M_has


@pytest.mark.parametrize("op", OPS)
def test_cast_valued_mask_accum(gb, op):
    """(a) INT8 inputs, an FP64 w, a valued INT8 mask and GrB_PLUS_FP64: the operand cast, t in w's type, the value mask."""
    rng = np.random.default_rng(8100 + OPS.index(op))
    k = Case(gb, op, rng)
    w_val, w_has = draw(rng, N, 0.3, -9, 10, np.float64)
    M = valued_mask(rng)
    w, m = vec_of(gb, w_val, w_has, "FP64"), vec_of(gb, *M, "INT8")
    assert k.call(w, m, "GrB_PLUS_FP64") == 0, _error(k.L, w)
    if op == "vxm_push":
        from graphblas_amd import device

        assert device.last_stats()["method"] == 2, "the push direction did not run"
    same(w, *k.expected(w_val, w_has, M, accum=True), op)


@pytest.mark.parametrize("op", OPS)
def test_structural_mask_separate_and_aliased(gb, op):
    """(b) a structural mask -- S, SC, RSC -- whose structure and values disagree: a vector of its own (its words are borrowed), then
    w itself (its words are a snapshot): the aliased mask gives what a copy of it gives."""
    rng = np.random.default_rng(8200 + OPS.index(op))
    k = Case(gb, op, rng, tname="INT64")
    w_val, w_has = draw(rng, N, 0.5, -3, 4, np.int64)
    M = draw(rng, N, 0.6, 0, 3, np.int64)
    assert (M[0][M[1]] == 0).any() and (w_val[w_has] == 0).any()
    for flags in ("S", "SC", "RSC"):
        f = dict(comp="C" in flags, struct=True, replace="R" in flags)
        for accum in (None, "GrB_PLUS_INT64"):
            w, m = vec_of(gb, w_val, w_has, "INT64"), vec_of(gb, *M, "INT64")
            assert k.call(w, m, accum, flags) == 0, _error(k.L, w)
            same(w, *k.expected(w_val, w_has, M, accum=bool(accum), **f), (op, flags, accum, "separate"))
            same(m, *M, (op, flags, accum, "the mask is untouched"))
            exp = k.expected(w_val, w_has, (w_val, w_has), accum=bool(accum), **f)
            w = vec_of(gb, w_val, w_has, "INT64")
            assert k.call(w, w, accum, flags) == 0, _error(k.L, w)
            same(w, *exp, (op, flags, accum, "aliased"))
            w, m = vec_of(gb, w_val, w_has, "INT64"), vec_of(gb, w_val, w_has, "INT64")
            assert k.call(w, m, accum, flags) == 0, _error(k.L, w)
            same(w, *exp, (op, flags, accum, "a copy of w"))


@pytest.mark.parametrize("op", OPS_WITH_U)
def test_output_is_an_input(gb, op):
    """(c) w is u -- for eWise also v --, with a mask and an accumulator."""
    for which in (("u", "v") if op in EWISE_OPS else ("u",)):
        rng = np.random.default_rng(8300 + OPS.index(op))
        k = Case(gb, op, rng, tname="INT64", alias=True)
        w = k.u if which == "u" else k.v
        w_val, w_has = (k.u_val.copy(), k.u_has.copy()) if which == "u" else (k.v_val.copy(), k.v_has.copy())
        M = valued_mask(rng)
        m = vec_of(gb, *M, "INT8")
        assert k.call(w, m, "GrB_PLUS_INT64") == 0, _error(k.L, w)
        same(w, *k.expected(w_val, w_has, M, accum=True), (op, which))


@pytest.mark.parametrize("op", OPS)
def test_complement_of_no_mask(gb, op):
    """(d) a complemented descriptor without a mask allows no position: w is unchanged, or emptied under replace -- and the emptied w
    takes a plain call."""
    rng = np.random.default_rng(8400 + OPS.index(op))
    k = Case(gb, op, rng)
    w_val, w_has = draw(rng, N, 0.3, -9, 10, np.float64)
    w = vec_of(gb, w_val, w_has, "FP64")
    for accum in (None, "GrB_PLUS_FP64"):
        assert k.call(w, None, accum, "C") == 0
        same(w, w_val, w_has, (op, accum, "complement"))
    assert k.call(w, None, None, "RC") == 0
    assert w.nvals == 0
    assert k.call(w) == 0
    same(w, *k.expected(np.zeros(N), np.zeros(N, bool)), (op, "after replace"))


@pytest.mark.parametrize("op", OPS)
def test_mask_size_and_accum_type_checks(gb, op):
    """(e) a mask of size n + 1: GrB_DIMENSION_MISMATCH; an accumulator of another type than w's: GrB_DOMAIN_MISMATCH -- w unchanged,
    the text byte for byte the parent commit's."""
    rng = np.random.default_rng(8500 + OPS.index(op))
    k = Case(gb, op, rng)
    w_val, w_has = draw(rng, N, 0.3, -9, 10, np.float64)
    w = vec_of(gb, w_val, w_has, "FP64")
    m = gb.Vector("BOOL", N + 1)
    assert k.call(w, m, "GrB_PLUS_FP64") == -6  # GrB_DIMENSION_MISMATCH
    assert _error(k.L, w) == MASK_TEXT[op]
    same(w, w_val, w_has, (op, "mask"))
    assert k.call(w, None, "GrB_PLUS_INT64") == -5  # GrB_DOMAIN_MISMATCH
    assert _error(k.L, w) == ACCUM_TEXT[op]
    same(w, w_val, w_has, (op, "accum"))


@pytest.mark.parametrize("op", OPS_WITH_OPERAND)
def test_empty_operand(gb, op):
    """(f) an operand without entries (u; for mxv also the matrix), with and without mask and accumulator: the empty-T short cuts of
    mxv (GrX_Stats.method == 6) and every other operation's ordinary path over an empty t."""
    from graphblas_amd import device

    for empty in (("u", "A") if op in MXV_OPS else ("u",) if op in OPS_WITH_U else ("A",)):
        rng = np.random.default_rng(8600 + OPS.index(op))
        k = Case(gb, op, rng, empty=empty)
        w_val, w_has = draw(rng, N, 0.3, -9, 10, np.float64)
        M = valued_mask(rng)
        for masked in (False, True):
            w, m = vec_of(gb, w_val, w_has, "FP64"), vec_of(gb, *M, "INT8")
            assert k.call(w, m if masked else None, "GrB_PLUS_FP64" if masked else None) == 0, _error(k.L, w)
            if op in MXV_OPS:
                assert device.last_stats()["method"] == 6, (op, empty, masked)
            same(w, *k.expected(w_val, w_has, M if masked else None, accum=masked), (op, empty, masked))
