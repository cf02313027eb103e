"""GrB_Matrix_eWiseAdd / eWiseMult: ``A.ewise_add(B, op)`` / ``A.ewise_mult(B, op)`` -- the wavefront merge of grb_mxm_ewise.inc on the
GPU tier, the same sources under the SIMT emulator on the CPU tier.

1. the reference's own literals (tests/golden/ewise_literals.json) through ``.new()``, ``C << ...`` and ``C() << ...``;
2. the chunk boundaries of the merge (rows of 0, 1, 63, 64, 65, 127, 129, 200 entries; overlapping, disjoint and random columns; one
   list exhausted first) against an expectation computed HERE with numpy on linearised keys (union1d / intersect1d and ufuncs),
   cross-checked against the oracle's vec_ewise on the flattened matrices; compared bit for bit;
3. a row of 12000 entries cut into column pieces;
4. operands, operator and output of three types; iso operands on either side and on both;
5. the write rule (mask, complement, accumulator, replace; C aliasing A, C aliasing B, the mask aliasing A) against oracle.dense_eval;
6. transposed operands;
7. the C ABI directly (ctypes): the six matrix entry points, the two vector _Semiring forms, the error codes, GrX_last_stats;
8. GPU tier only: symmetrise an R-MAT graph on the device, count its triangles, no growth of device memory.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import dense_eval
from oracle import grb_oracle as O
from tests.backend import DEVICES, ROOT, bind
from tests.values import rand_vals, same_fp

NP_OF = O.NP_OF
TYPES = ["INT64", "FP32", "BOOL", "FP64", "INT8", "UINT16", "INT32"]  # (tests/test_select.py::TYPES)
# a second type that differs from the first and that numpy's astype casts like the library does (no float -> integer)
OTHER_TYPE = {"INT64": "FP64", "FP32": "FP64", "BOOL": "INT32", "FP64": "FP32", "INT8": "INT64", "UINT16": "FP32", "INT32": "INT64"}
ARITH = ["plus", "minus", "times", "min", "max", "first", "second"]
LOGICAL = ["lor", "land", "lxor"]  # (operators of BOOL: the operands are cast to BOOL first)
CMP = ["eq", "ne", "gt", "ge", "lt", "le"]
ORDERED = ["minus", "first", "second"]  # run with the operands swapped as well
ORACLE_OPS = ARITH + LOGICAL


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


@pytest.fixture(scope="module")
def literals():
    with open(os.path.join(ROOT, "tests", "golden", "ewise_literals.json")) as f:
        return json.load(f)


# ---- the expectation: numpy on linearised keys --------------------------------------------------------------------------------
class Coo:
    """COO tuples of one operand: keys = i * ncols + j."""

    def __init__(self, rows, cols, vals, tname, shape):
        self.rows, self.cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        self.vals, self.tname, self.shape = np.asarray(vals, NP_OF[tname]), tname, shape
        self.keys = self.rows * shape[1] + self.cols

    @property
    def T(self):
        return Coo(self.cols, self.rows, self.vals, self.tname, (self.shape[1], self.shape[0]))

    def matrix(self, gb):
        return gb.Matrix.from_coo(self.rows, self.cols, self.vals, dtype=self.tname, nrows=self.shape[0], ncols=self.shape[1])


def op_type(name, ta, tb):
    return "BOOL" if name in LOGICAL else O.unify(ta, tb)


def np_apply(name, a, b):
    """z = op(a, b) on two arrays of the operator's type."""
    with np.errstate(all="ignore"):
        if name in CMP:
            return {"eq": a == b, "ne": a != b, "gt": a > b, "ge": a >= b, "lt": a < b, "le": a <= b}[name]
        if a.dtype == np.bool_:
            return {"plus": a | b, "max": a | b, "lor": a | b, "times": a & b, "min": a & b, "land": a & b, "minus": a ^ b,
                    "lxor": a ^ b, "first": a, "second": b}[name]
        if name == "first":
            return a
        if name == "second":
            return b
        return {"plus": np.add, "minus": np.subtract, "times": np.multiply, "min": np.fmin, "max": np.fmax}[name](a, b)


def expect(union, name, A, B):
    """(keys, values) of A (op) B over the union / the intersection: operands cast to the operator's type, single entries pass
    through in it (cast to BOOL under a comparison)."""
    ot = op_type(name, A.tname, B.tname)
    av, bv = O.cast(A.vals, ot), O.cast(B.vals, ot)
    tt = np.bool_ if name in CMP else NP_OF[ot]
    both, ia, ib = np.intersect1d(A.keys, B.keys, return_indices=True)
    z = np.asarray(np_apply(name, av[ia], bv[ib])).astype(tt)
    if not union:
        return both, z
    keys = np.union1d(A.keys, B.keys)
    val = np.zeros(keys.size, tt)
    val[np.searchsorted(keys, A.keys)] = (av != 0) if name in CMP else av
    val[np.searchsorted(keys, B.keys)] = (bv != 0) if name in CMP else bv
    val[np.searchsorted(keys, both)] = z
    return keys, val


def same_vals(got, exp, name, where):
    assert got.dtype == exp.dtype, (where, got.dtype, exp.dtype)
    if exp.dtype.kind == "f":
        same_fp(got, exp, name if name in ("min", "max") else None, where)
    else:
        assert got.tolist() == exp.tolist(), where


def oracle_agrees(union, name, A, B, keys, vals, where):
    """The same expectation from the oracle's vec_ewise on the two matrices flattened to vectors, for the operators it knows."""
    if name not in ORACLE_OPS or (O.unify(A.tname, B.tname) == "BOOL" and name == "minus"):  # (numpy has no boolean subtract)
        return
    size = A.shape[0] * A.shape[1]
    with np.errstate(all="ignore"):
        ov = O.vec_ewise(O.OVec(size, A.keys, A.vals, A.tname), O.OVec(size, B.keys, B.vals, B.tname), name, union=union)
    assert ov.idx.tolist() == keys.tolist(), (where, "oracle pattern")
    if name in LOGICAL:  # (the oracle keeps the unified type; the operator is one of BOOL)
        assert (ov.vals != 0).tolist() == vals.tolist(), (where, "oracle values")
    else:
        same_vals(np.asarray(ov.vals), vals, name, where + " (oracle)")


def check(C, union, name, A, B, where, out_type=None, oracle=True):
    keys, vals = expect(union, name, A, B)
    if oracle:
        oracle_agrees(union, name, A, B, keys, vals, where)
    if out_type is not None:
        with np.errstate(all="ignore"):
            vals = vals.astype(NP_OF[out_type])
    I, J, X = C.to_coo()
    assert C.shape == A.shape, where
    assert (I.astype(np.int64) * A.shape[1] + J.astype(np.int64)).tolist() == keys.tolist(), (where, "pattern")
    same_vals(X, vals, name, where)
    return I.astype(np.int64), J.astype(np.int64)


def run(gb, a, b, union, name):
    return (a.ewise_add if union else a.ewise_mult)(b, getattr(gb.binary, name))


def values_for(rng, k, tname):
    return rand_vals(rng, k, tname, "exact") if tname.startswith("FP") else rand_vals(rng, k, tname)


# ---- 1. the reference's literals ------------------------------------------------------------------------------------------
def resolve(gb, dotted):
    ns, name = dotted.split(".")
    return getattr(getattr(gb, ns), name)


def test_literals(gb, literals):
    lit = literals
    m, n = lit["nrows"], lit["ncols"]
    A = gb.Matrix.from_coo(lit["A"]["rows"], lit["A"]["cols"], lit["A"]["vals"], nrows=m, ncols=n)
    B = gb.Matrix.from_coo(lit["B"]["rows"], lit["B"]["cols"], lit["B"]["vals"], nrows=m, ncols=n)
    for case in lit["cases"]:
        want = gb.Matrix.from_coo(case["rows"], case["cols"], case["vals"], nrows=m, ncols=n)
        order = np.lexsort((case["cols"], case["rows"]))
        for opname in case["ops"]:
            op = resolve(gb, opname)
            outs = [getattr(A, case["method"])(B, op).new()]
            C = gb.Matrix(A.dtype, m, n)
            C << getattr(A, case["method"])(B, op)
            outs.append(C)
            C = gb.Matrix.from_coo([1], [1], [99], nrows=m, ncols=n)  # (no mask, no accumulator: what C held goes away)
            C() << getattr(A, case["method"])(B, op)
            outs.append(C)
            for k, out in enumerate(outs):
                where = (case["source"], opname, k)
                I, J, X = out.to_coo()
                assert out.dtype == A.dtype and I.tolist() == np.asarray(case["rows"])[order].tolist(), where
                assert J.tolist() == np.asarray(case["cols"])[order].tolist() and X.tolist() == np.asarray(case["vals"])[order].tolist(), where
                assert out.isequal(want), where
    for case in lit["type_errors"]:
        with pytest.raises(TypeError, match=case["match"]):
            getattr(A, case["method"])(B, resolve(gb, case["op"]))
    with pytest.raises(TypeError, match="Expected type: Matrix; got Vector"):
        A.ewise_add(gb.Vector(int, 7), gb.binary.plus)
    with pytest.raises(gb.exceptions.DimensionMismatch):
        A.ewise_mult(gb.Matrix(int, 7, 8), gb.binary.times)
    assert A.ewise_add(B).new().isequal(A.ewise_add(B, gb.monoid.plus).new())  # the defaults: monoid.plus / binary.times
    assert A.ewise_mult(B).new().isequal(A.ewise_mult(B, gb.binary.times).new())


# ---- 2. chunk boundaries against numpy ------------------------------------------------------------------------------------
ROW_LENS = [(0, 0), (0, 1), (1, 0), (1, 1), (63, 64), (64, 64), (65, 1), (64, 65), (129, 127), (200, 200), (200, 0)]


def boundary_patterns(rng, variant, ncols=200):
    """12 x 200: rows 0..10 with the prescribed (A, B) lengths; row 11 with all of B's columns above all of A's (one list is
    exhausted first).  The disjoint variant takes A from the even and B from the odd columns, so its lengths stop at 100."""
    ra, ca, rb, cb = [], [], [], []
    for i, (la, lb) in enumerate(ROW_LENS):
        if variant == "overlap":  # the shorter row is a subset of the longer
            base = rng.permutation(ncols)
            a, b = np.sort(base[:la]), np.sort(base[:lb])
        elif variant == "disjoint":
            a = 2 * np.sort(rng.choice(ncols // 2, min(la, ncols // 2), replace=False))
            b = 2 * np.sort(rng.choice(ncols // 2, min(lb, ncols // 2), replace=False)) + 1
        else:
            a, b = np.sort(rng.choice(ncols, la, replace=False)), np.sort(rng.choice(ncols, lb, replace=False))
        ra.append(np.full(a.size, i)), ca.append(a), rb.append(np.full(b.size, i)), cb.append(b)
    a, b = np.sort(rng.choice(90, 70, replace=False)), 90 + np.sort(rng.choice(110, 90, replace=False))
    ra.append(np.full(a.size, 11)), ca.append(a), rb.append(np.full(b.size, 11)), cb.append(b)
    return (np.concatenate(ra), np.concatenate(ca)), (np.concatenate(rb), np.concatenate(cb))


@pytest.mark.parametrize("tname", TYPES)
@pytest.mark.parametrize("variant", ["overlap", "disjoint", "random"])
def test_chunk_boundaries(gb, variant, tname):
    rng = np.random.default_rng(4100 + TYPES.index(tname) * 3 + ["overlap", "disjoint", "random"].index(variant))
    shape = (12, 200)
    (ra, ca), (rb, cb) = boundary_patterns(rng, variant)
    A = Coo(ra, ca, values_for(rng, ra.size, tname), tname, shape)
    B = Coo(rb, cb, values_for(rng, rb.size, tname), tname, shape)
    a, b = A.matrix(gb), B.matrix(gb)
    compared = 0
    for name in ARITH + LOGICAL + CMP:
        for union in (True, False):
            pairs = [(a, b, A, B)] + ([(b, a, B, A)] if name in ORDERED else [])
            for x, y, X, Y in pairs:
                where = f"{variant} {tname} {'add' if union else 'mult'} {name} swapped={x is b}"
                C = run(gb, x, y, union, name).new()
                assert C.dtype.name == ("BOOL" if name in CMP else op_type(name, tname, tname)), where
                check(C, union, name, X, Y, where)
                compared += 1
    assert compared == 2 * (len(ARITH + LOGICAL + CMP) + len(ORDERED))


# ---- 3. a long row cut into pieces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["INT64", "FP32"])
def test_long_row_pieces(gb, tname):
    """Row 1 holds 6000 + 6000 entries (3000 shared) over 40000 columns: more than 8192 together, three column pieces."""
    rng = np.random.default_rng(4200 + len(tname))
    shape = (3, 40000)
    perm = rng.permutation(shape[1])
    a1, b1 = np.sort(perm[:6000]), np.sort(perm[3000:9000])
    a2, b2 = np.array([3, 70, 71, 20000, 39999]), np.array([0, 70, 9000, 20000, 20001, 39998, 39999])
    ra, ca = np.concatenate([np.full(a1.size, 1), np.full(a2.size, 2)]), np.concatenate([a1, a2])
    rb, cb = np.concatenate([np.full(b1.size, 1), np.full(b2.size, 2)]), np.concatenate([b1, b2])
    A = Coo(ra, ca, values_for(rng, ra.size, tname), tname, shape)
    B = Coo(rb, cb, values_for(rng, rb.size, tname), tname, shape)
    a, b = A.matrix(gb), B.matrix(gb)
    for union in (True, False):
        for name in ("plus", "minus"):
            where = f"long row {tname} {'add' if union else 'mult'} {name}"
            I, J = check(run(gb, a, b, union, name).new(), union, name, A, B, where)
            assert I.size == (9000 + 9 if union else 3000 + 3), where
            assert np.all(np.diff(J)[np.diff(I) == 0] > 0), (where, "columns must be strictly increasing within a row")


# ---- 4. three types; iso operands -------------------------------------------------------------------------------------------
def stored_iso(A):
    """Whether the library keeps ONE value for every entry of A (GrX_Matrix_export_CSR_device reports the stored form)."""
    from graphblas_amd import _lib

    dp, dj, dx, nv, iso = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    assert _lib.lib.GrX_Matrix_export_CSR_device(ctypes.byref(dp), ctypes.byref(dj), ctypes.byref(dx), ctypes.byref(nv), ctypes.byref(iso), A._carg) == 0
    return bool(iso.value)


def draw_coo(rng, shape, tname, dens, iso=False):
    r, c = np.nonzero(rng.random(shape) < dens)
    vals = values_for(rng, r.size, tname)
    if iso:
        vals = np.full(r.size, vals[vals != 0][0] if tname != "BOOL" else True)
    return Coo(r, c, vals, tname, shape)


def iso_matrix(gb, X):
    indptr = np.concatenate([[0], np.cumsum(np.bincount(X.rows, minlength=X.shape[0]))])
    M = gb.Matrix.ss.import_csr(nrows=X.shape[0], ncols=X.shape[1], indptr=indptr, values=X.vals[:1], col_indices=X.cols, is_iso=True,
                                sorted_cols=True, dtype=X.tname)
    assert stored_iso(M) and M.nvals == X.rows.size
    return M


@pytest.mark.parametrize("ta", TYPES)
def test_three_types(gb, ta):
    """A of one type, B of another, the operator in their unified type, the output in a third."""
    rng = np.random.default_rng(4300 + TYPES.index(ta))
    shape = (9, 150)
    tb = OTHER_TYPE[ta]
    ot = O.unify(ta, tb)
    tc = "FP32" if ot == "FP64" else "FP64"
    A, B = draw_coo(rng, shape, ta, 0.5), draw_coo(rng, shape, tb, 0.5)
    a, b = A.matrix(gb), B.matrix(gb)
    for name in ("plus", "minus", "times", "max", "second", "lt", "land"):
        for union in (True, False):
            where = f"{ta} {name} {tb} -> {tc} {'add' if union else 'mult'}"
            expr = run(gb, a, b, union, name)
            assert expr.dtype.name == ("BOOL" if name in CMP else op_type(name, ta, tb)), where
            check(expr.new(dtype=tc), union, name, A, B, where, out_type=tc)


@pytest.mark.parametrize("tname", ["INT64", "FP32", "BOOL"])
def test_iso_operands(gb, tname):
    rng = np.random.default_rng(4400 + len(tname))
    shape = (9, 150)
    A, B = draw_coo(rng, shape, tname, 0.5), draw_coo(rng, shape, tname, 0.5)
    Ai, Bi = draw_coo(rng, shape, tname, 0.5, iso=True), draw_coo(rng, shape, tname, 0.5, iso=True)
    a, b, ai, bi = A.matrix(gb), B.matrix(gb), iso_matrix(gb, Ai), iso_matrix(gb, Bi)
    scalar = gb.Matrix.from_coo(Ai.rows, Ai.cols, Ai.vals[0], dtype=tname, nrows=shape[0], ncols=shape[1])  # built with a scalar value
    for x, y, X, Y, side in ((ai, b, Ai, B, "A"), (a, bi, A, Bi, "B"), (ai, bi, Ai, Bi, "both"), (scalar, b, Ai, B, "scalar")):
        for name in ("plus", "minus", "second", "ge"):
            for union in (True, False):
                check(run(gb, x, y, union, name).new(), union, name, X, Y, f"iso {side} {tname} {name} {'add' if union else 'mult'}")
    # the pass-through short cut with an iso operand: under a mask the write rule reads one value per entry
    E = gb.Matrix(tname, *shape)
    C = b.dup()
    C(a.S) << ai.ewise_add(E, gb.binary.plus)
    keys, vals = expect(True, "plus", Ai, Coo([], [], [], tname, shape))
    allow = np.isin(np.arange(shape[0] * shape[1]), A.keys)
    has, val = np.zeros(allow.size, bool), np.zeros(allow.size, NP_OF[tname])
    has[B.keys], val[B.keys] = True, B.vals
    t_has = np.zeros(allow.size, bool)
    t_has[keys] = True
    has[allow] = t_has[allow]
    val[keys[allow[keys]]] = vals[allow[keys]]
    I, J, X = C.to_coo()
    assert (I.astype(np.int64) * shape[1] + J.astype(np.int64)).tolist() == np.flatnonzero(has).tolist()
    same_vals(X, val[has], None, "iso pass-through under a mask")


# ---- 5. the write rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["INT64", "FP32"])
def test_write_rule(gb, tname):
    rng = np.random.default_rng(4500 + len(tname))
    shape = (6, 70)
    np_t = NP_OF[tname]

    def dense(X, np_type=None):
        has, val = np.zeros(shape, bool), np.zeros(shape, np_type or NP_OF[X.tname])
        has[X.rows, X.cols], val[X.rows, X.cols] = True, X.vals
        return val, has

    def small(dens, t):
        r, c = np.nonzero(rng.random(shape) < dens)
        return Coo(r, c, rand_vals(rng, r.size, t), t, shape)

    compared = 0
    for alias in ("none", "C=A", "C=B", "M=A"):
        for mask_kind in (None, "S", "V", "~S", "~V"):
            if alias == "M=A" and mask_kind is None:
                continue
            for accum in (None, "plus"):
                for replace in ((False, True) if mask_kind else (False,)):
                    for union, name in ((True, "plus"), (False, "times")):
                        A, B = small(0.5, tname), small(0.5, tname)
                        Cc = {"none": small(0.4, tname), "C=A": A, "C=B": B, "M=A": small(0.4, tname)}[alias]
                        Mc = A if alias == "M=A" else small(0.5, "INT8")
                        a, b = A.matrix(gb), B.matrix(gb)
                        C = {"C=A": a, "C=B": b}.get(alias) or Cc.matrix(gb)
                        kw = {}
                        if mask_kind:
                            M = a if alias == "M=A" else Mc.matrix(gb)
                            mk = M.S if "S" in mask_kind else M.V
                            kw = dict(mask=~mk if "~" in mask_kind else mk, replace=replace)
                        if accum:
                            kw["accum"] = getattr(gb.binary, accum)
                        C(**kw) << run(gb, a, b, union, name)
                        keys, vals = expect(union, name, A, B)
                        T = Coo(keys // shape[1], keys % shape[1], vals, tname, shape)
                        Mval, Mhas = dense(Mc) if mask_kind else (None, None)
                        Nval, Nhas = dense_eval.write(*dense(Cc), *dense(T), Mval, Mhas, comp=bool(mask_kind) and "~" in mask_kind,
                                                      struct=bool(mask_kind) and "S" in mask_kind, accum=accum, replace=replace, np_t=np_t)
                        where = f"{tname} alias={alias} mask={mask_kind} accum={accum} replace={replace} {'add' if union else 'mult'}"
                        I, J, X = C.to_coo()
                        rr, cc = np.nonzero(Nhas)
                        assert I.tolist() == rr.tolist() and J.tolist() == cc.tolist(), where
                        same_vals(X, Nval[rr, cc], None, where)
                        compared += 1
    assert compared == 2 * (4 * 18 - 2)


# ---- 6. transposed operands ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["INT64", "FP64"])
def test_transposed(gb, tname):
    rng = np.random.default_rng(4600 + len(tname))
    shape = (50, 50)
    A, B = draw_coo(rng, shape, tname, 0.2), draw_coo(rng, shape, tname, 0.2)
    a, b = A.matrix(gb), B.matrix(gb)
    for name in ("minus", "plus", "second"):
        op = getattr(gb.binary, name)
        check(a.ewise_add(a.T, op).new(), True, name, A, A.T, f"A + A.T {name} {tname}")
        check(a.T.ewise_mult(b, op).new(), False, name, A.T, B, f"A.T * B {name} {tname}")
        check(a.T.ewise_add(b.T, op).new(), True, name, A.T, B.T, f"A.T + B.T {name} {tname}")
        check(a.ewise_mult(b.T, op).new(), False, name, A, B.T, f"A * B.T {name} {tname}")
    # the symmetrisation of a directed graph: the pattern equals its own transpose
    I, J, _ = a.ewise_add(a.T, gb.binary.any).new().to_coo()
    keys = I.astype(np.int64) * 50 + J.astype(np.int64)
    assert keys.tolist() == np.union1d(A.keys, A.T.keys).tolist()
    assert np.sort(J.astype(np.int64) * 50 + I.astype(np.int64)).tolist() == keys.tolist()
    # a rectangular matrix against its transpose is the library's DimensionMismatch
    R = gb.Matrix.from_coo([0, 2], [1, 4], [1, 2], nrows=3, ncols=5)
    with pytest.raises(gb.exceptions.DimensionMismatch):
        R.ewise_add(R.T, gb.binary.plus)
    assert R.T.ewise_add(R.T, gb.binary.plus).new().shape == (5, 3)


# ---- 7. the C ABI directly ----------------------------------------------------------------------------------------------------
def _handle(L, name):
    return ctypes.c_void_p(ctypes.c_void_p.in_dll(L, name).value)


def _matrix_error(L, C):
    s = ctypes.c_char_p()
    L.GrB_Matrix_error(ctypes.byref(s), C._carg)
    return (s.value or b"").decode()


def _coo(C):
    I, J, X = C.to_coo()
    return I.tolist(), J.tolist(), X.tolist()


def _sorted_case(case):
    order = np.lexsort((case["cols"], case["rows"]))
    return tuple(np.asarray(case[k])[order].tolist() for k in ("rows", "cols", "vals"))


def test_c_abi(gb, literals):
    from graphblas_amd import _lib, device

    L = _lib.lib
    lit = literals
    A = gb.Matrix.from_coo(lit["A"]["rows"], lit["A"]["cols"], lit["A"]["vals"], nrows=7, ncols=7)
    B = gb.Matrix.from_coo(lit["B"]["rows"], lit["B"]["cols"], lit["B"]["vals"], nrows=7, ncols=7)
    Ac = Coo(lit["A"]["rows"], lit["A"]["cols"], lit["A"]["vals"], "INT64", (7, 7))
    Bc = Coo(lit["B"]["rows"], lit["B"]["cols"], lit["B"]["vals"], "INT64", (7, 7))
    mult, add = (_sorted_case(c) for c in lit["cases"])
    C = gb.Matrix(int, 7, 7)
    for fn, op, want in (("GrB_Matrix_eWiseAdd_BinaryOp", "GrB_SECOND_INT64", add), ("GrB_Matrix_eWiseAdd_Monoid", "GrB_MAX_MONOID_INT64", add),
                         ("GrB_Matrix_eWiseMult_BinaryOp", "GrB_TIMES_INT64", mult), ("GrB_Matrix_eWiseMult_Monoid", "GrB_TIMES_MONOID_INT64", mult),
                         ("GrB_Matrix_eWiseMult_Semiring", "GrB_PLUS_TIMES_SEMIRING_INT64", mult)):
        assert getattr(L, fn)(C._carg, None, None, _handle(L, op), A._carg, B._carg, None) == 0, fn
        assert _coo(C) == want, fn
        st = device.last_stats()
        assert st["method"] == 8 and st["out_nvals"] == C.nvals == len(want[0]) and st["kernel_launches"] > 0, (fn, st)
    # the _Semiring form of eWiseAdd takes the additive monoid
    assert L.GrB_Matrix_eWiseAdd_Semiring(C._carg, None, None, _handle(L, "GrB_PLUS_TIMES_SEMIRING_INT64"), A._carg, B._carg, None) == 0
    check(C, True, "plus", Ac, Bc, "GrB_Matrix_eWiseAdd_Semiring")
    # ... and so do the vector forms
    u, v = gb.Vector.from_coo([1, 3, 4, 6], [1, 1, 2, 0], size=7), gb.Vector.from_coo([0, 3, 4], [5, 7, 9], size=7)
    w = gb.Vector(int, 7)
    assert L.GrB_Vector_eWiseAdd_Semiring(w._carg, None, None, _handle(L, "GrB_PLUS_TIMES_SEMIRING_INT64"), u._carg, v._carg, None) == 0
    assert [x.tolist() for x in w.to_coo()] == [[0, 1, 3, 4, 6], [5, 1, 8, 11, 0]]
    assert L.GrB_Vector_eWiseMult_Semiring(w._carg, None, None, _handle(L, "GrB_PLUS_TIMES_SEMIRING_INT64"), u._carg, v._carg, None) == 0
    assert [x.tolist() for x in w.to_coo()] == [[3, 4], [7, 18]]
    # the empty-operand short cuts skip the merge
    E = gb.Matrix(int, 7, 7)
    assert L.GrB_Matrix_eWiseMult_BinaryOp(C._carg, None, None, _handle(L, "GrB_TIMES_INT64"), A._carg, E._carg, None) == 0
    assert C.nvals == 0 and device.last_stats()["method"] == 6
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(C._carg, None, None, _handle(L, "GrB_PLUS_INT64"), E._carg, A._carg, None) == 0
    assert C.isequal(A) and device.last_stats()["method"] == 6 and device.last_stats()["out_nvals"] == A.nvals
    # handle-only operators stay outside
    D = gb.Matrix(float, 7, 7)
    assert L.GrB_Matrix_eWiseMult_BinaryOp(D._carg, None, None, _handle(L, "GrB_DIV_FP64"), A._carg, B._carg, None) == -8  # GrB_NOT_IMPLEMENTED
    assert _matrix_error(L, D) != ""
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(D._carg, None, None, _handle(L, "GxB_POW_FP64"), A._carg, B._carg, None) == -8
    # NULL arguments
    plus = _handle(L, "GrB_PLUS_INT64")
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(None, None, None, plus, A._carg, B._carg, None) == -2  # GrB_NULL_POINTER
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(C._carg, None, None, plus, None, B._carg, None) == -2
    assert L.GrB_Matrix_eWiseMult_BinaryOp(C._carg, None, None, plus, A._carg, None, None) == -2
    assert L.GrB_Matrix_eWiseMult_Monoid(C._carg, None, None, None, A._carg, B._carg, None) == -2
    # shapes, with T0 / T1 taken into account
    W = gb.Matrix.from_coo([0, 6], [1, 7], [1, 2], nrows=7, ncols=8)
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(C._carg, None, None, plus, A._carg, W._carg, None) == -6  # GrB_DIMENSION_MISMATCH
    assert "7 x 7" in _matrix_error(L, C) and "7 x 8" in _matrix_error(L, C)
    W2 = gb.Matrix(int, 7, 8)
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(W2._carg, None, None, plus, W._carg, W._carg, _handle(L, "GrB_DESC_T1")) == -6
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(C._carg, None, None, plus, W._carg, W._carg, None) == -6
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(W2._carg, A._carg, None, plus, W._carg, W._carg, None) == -6
    assert "mask" in _matrix_error(L, W2)
    W3 = gb.Matrix(int, 8, 7)
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(W3._carg, None, None, plus, W._carg, W._carg, _handle(L, "GrB_DESC_T0T1")) == 0
    assert _coo(W3) == ([1, 7], [0, 6], [2, 4])
    # the accumulator is of C's type and no comparison
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(C._carg, None, _handle(L, "GrB_PLUS_FP32"), plus, A._carg, B._carg, None) == -5  # GrB_DOMAIN_MISMATCH
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(C._carg, None, _handle(L, "GrB_EQ_INT64"), plus, A._carg, B._carg, None) == -5
    assert "accum" in _matrix_error(L, C)
    # a complemented absent mask writes nothing
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(W3._carg, None, None, plus, W._carg, W._carg, _handle(L, "GrB_DESC_T0T1")) == 0
    assert L.GrB_Matrix_eWiseMult_BinaryOp(W3._carg, None, None, plus, W3._carg, W3._carg, _handle(L, "GrB_DESC_C")) == 0
    assert _coo(W3) == ([1, 7], [0, 6], [2, 4])
    # a shape without rows returns at once
    Z = gb.Matrix(int, 0, 5)
    assert L.GrB_Matrix_eWiseAdd_BinaryOp(Z._carg, None, None, plus, Z._carg, Z._carg, None) == 0 and Z.nvals == 0


# ---- 8. GPU tier: a mid-size graph ----------------------------------------------------------------------------------------------
def _rmat(gb, scale):
    from graphblas_amd import synthetic

    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, device="cpu")
    ip, col = ip.numpy(), col.numpy().astype(np.int64)
    A = gb.Matrix.from_csr(ip, col, np.ones(col.size, np.int64), dtype="INT64", ncols=n)
    return n, A, Coo(np.repeat(np.arange(n), np.diff(ip)), col, np.ones(col.size, np.int64), "INT64", (n, n))


@pytest.mark.gpu
def test_symmetrise_and_count_triangles_gpu():
    gb = bind("gpu")
    n, A, Ac = _rmat(gb, 14)
    S = A.ewise_add(A.T, gb.binary.any).new()
    I, J, X = S.to_coo()
    union = np.union1d(Ac.keys, Ac.T.keys)
    assert np.array_equal(I.astype(np.int64) * n + J.astype(np.int64), union) and np.all(X == 1)
    I, J, X = A.ewise_mult(A.T, gb.binary.times).new().to_coo()
    assert np.array_equal(I.astype(np.int64) * n + J.astype(np.int64), np.intersect1d(Ac.keys, Ac.T.keys)) and np.all(X == 1)

    def triangles(S):
        L = S.select("tril", -1).new()
        C = gb.Matrix("INT64", n, n)
        C(L.S) << L.mxm(L.T, gb.semiring.plus_pair)
        return C.reduce_scalar("plus").new().value

    host = gb.Matrix.from_coo(union // n, union % n, np.ones(union.size, np.int64), dtype="INT64", nrows=n, ncols=n)
    got, want = triangles(S), triangles(host)
    print(f"scale 14: {S.nvals} entries in S, {got} triangles")
    assert got == want and got > 0


@pytest.mark.gpu
def test_no_growth():
    """100 calls per cycle on one graph, results freed.  The library keeps freed blocks in its size-class cache, so the first cycle may
    grow; free device memory after cycle 2 against after cycle 3 (the probe of tests/test_select.py::test_no_growth)."""
    import torch

    gb = bind("gpu")
    n, A, _ = _rmat(gb, 14)
    M = A.select("triu", 1).new()

    def free_bytes():
        gb.Matrix(int, 1, 1).wait()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        for k in range(25):
            for expr, mask in ((A.ewise_add(A.T, gb.binary.plus), None), (A.ewise_mult(A.T, gb.binary.times), M.S),
                               (A.ewise_add(M, gb.binary.lt), None), (M.T.ewise_add(A, gb.binary.minus), M.V)):
                r = expr.new(mask=mask) if mask is not None else expr.new()
                del r

    cycle()
    cycle()
    after2 = free_bytes()
    cycle()
    after3 = free_bytes()
    print(f"free after cycle 2: {after2 / 2**20:.1f} MiB, after cycle 3: {after3 / 2**20:.1f} MiB")
    assert after3 >= after2, (after2, after3)
