"""Matrix assign: ``C(mask, accum, replace)[I, J] << A`` / a scalar / a row / a column, ``setElement`` and ``removeElement`` (C API 2.0
section 4.3.7, GrB_assign -- the mask has C's shape --, not GxB_subassign; python-graphblas_amd/csrc/grb_assign.hip).

Every expectation is the DENSE numpy restatement below (``np_assign``): ``has`` / ``val`` arrays, step 1  Z = C; Z(I, J) = accum ? accum(C(I, J), A)
: A, step 2  C<Mask, replace> = Z  through ``np_write_rule`` of tests/test_select.py.  It knows nothing of the library or of the oracle; results
are compared bit for bit (``assert_coo``).  Values are small integers (floating-point types hold integer values too), so that every cast and every
accumulator is exact in every type and numpy's ``astype`` is the GraphBLAS typecast.

The constants the limits are built around are the library's: 2048 entries per placement unit (ASG_UNIT), 8192 entries of C(i, :) and S'(i, :)
together before a row is cut into column pieces (WR_LONG), 16384 columns per piece, 64-entry blocks, 8 blocks per walk of the mask filter.

Not testable at a small size: the scalar form's GrB_OUT_OF_MEMORY answer when the 4 ni nj bytes of a dense region do not fit the free device
memory (it needs a region of the order of the device's memory), and the GrB_NOT_IMPLEMENTED answer of an unsorted J at 2^32 entries."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.backend import DEVICES, ROOT, bind
from tests.test_select import assert_coo, np_write_rule

NP_OF = {"BOOL": np.bool_, "INT8": np.int8, "INT16": np.int16, "INT32": np.int32, "INT64": np.int64, "UINT8": np.uint8, "UINT16": np.uint16,
         "UINT32": np.uint32, "UINT64": np.uint64, "FP32": np.float32, "FP64": np.float64}
ALL_TYPES = list(NP_OF)
ASG_UNIT, WR_LONG, PIECE = 2048, 8192, 16384
ALL = slice(None)


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


@pytest.fixture(scope="module")
def lit():
    with open(os.path.join(ROOT, "tests", "golden", "assign_literals.json")) as f:
        return json.load(f)


# ---- the dense restatement ---------------------------------------------------------------------------------------------------------------
def np_acc(name, tname, c, t):
    with np.errstate(all="ignore"):
        if name == "second":
            return t
        if tname == "BOOL":
            return np.logical_or(c, t) if name == "plus" else np.logical_and(c, t)
        if name == "plus":
            return (c + t).astype(c.dtype)
        return np.minimum(c, t)


def dense_of(shape, coo, dt):
    has, val = np.zeros(shape, bool), np.zeros(shape, dt)
    if coo is not None and len(coo[0]):
        r, c = np.asarray(coo[0], np.int64), np.asarray(coo[1], np.int64)
        has[r, c] = True
        val[r, c] = np.asarray(coo[2]).astype(dt)
    return has, val


def np_assign(shape, tname, C, a_has, a_val, I, J, M=None, structural=False, comp=False, replace=False, accum=None):
    """C, M: (rows, cols, vals) or None.  a_has / a_val: the input as dense ni x nj arrays (a scalar: all present).  I, J: index arrays
    (None = every index).  Returns (rows, cols, vals) row-major."""
    dt = NP_OF[tname]
    I = np.arange(shape[0]) if I is None else np.asarray(I, np.int64)
    J = np.arange(shape[1]) if J is None else np.asarray(J, np.int64)
    c_has, c_val = dense_of(shape, C, dt)
    z_has, z_val = c_has.copy(), c_val.copy()
    if I.size and J.size:
        ix = np.ix_(I, J)
        a_val = np.asarray(a_val).astype(dt)
        if accum is None:
            z_has[ix], z_val[ix] = a_has, np.where(a_has, a_val, 0)
        else:
            ch, cv = c_has[ix], c_val[ix]
            z_val[ix] = np.where(ch & a_has, np_acc(accum, tname, cv, a_val), np.where(ch, cv, np.where(a_has, a_val, 0)))
            z_has[ix] = ch | a_has
    zr, zc = np.nonzero(z_has)
    if M is None and comp:
        return (np.zeros(0, int),) * 3 if replace else C
    return np_write_rule(shape, tname, C, (zr, zc, z_val[zr, zc]), M, structural, comp, replace, None)


def draw(rng, m, n, tname, dens, iso=False):
    k = rng.random((m, n)) < dens
    r, c = np.nonzero(k)
    if tname == "BOOL":
        v = rng.random(r.size) < 0.7
    else:
        v = rng.integers(1, 9, r.size).astype(NP_OF[tname])
    if iso and r.size:
        v[:] = v[0]
    return r, c, v


def mat(gb, coo, tname, m, n):
    return gb.Matrix.from_coo(coo[0], coo[1], coo[2], dtype=tname, nrows=m, ncols=n)


def mask_arg(Mm, structural, comp):
    mk = Mm.S if structural else Mm.V
    return ~mk if comp else mk


def updater(C, Mm, structural, comp, replace, accum):
    args = []
    if Mm is not None:
        args.append(mask_arg(Mm, structural, comp))
    if accum is not None:
        args.append(accum)
    return C(*args, replace=replace)


def index_list(rng, kind, dim, frac=0.6):
    """kind: all / run / sorted / shuffled -> (key for the host, index array or None)"""
    if kind == "all":
        return ALL, None
    if kind == "run":
        lo = int(rng.integers(0, max(dim // 3, 1)))
        a = np.arange(lo, lo + max(dim // 2, 1))
        return a, a
    a = np.sort(rng.choice(dim, max(int(dim * frac), 2), replace=False))
    if kind == "sorted":
        if a.size > 2 and np.all(np.diff(a) == 1):
            a = np.delete(a, 1)
        return a, a
    a = rng.permutation(a)
    if np.all(np.diff(a) > 0):
        a = a[::-1].copy()
    return a, a


def stats():
    from graphblas_amd import device

    return device.last_stats()


METHOD_OF_J = {"all": 15, "run": 15, "sorted": 16, "shuffled": 17}
MASKS = [(None, False, False, False)] + [("m", s, c, r) for s in (True, False) for c in (False, True) for r in (False, True)]
ACCUMS = [None, "plus", "min", "second"]


# ---- 1. the reference's literals --------------------------------------------------------------------------------------------------------------
def lit_A(gb, lit):
    a = lit["A"]
    return gb.Matrix.from_coo(a["rows"], a["cols"], a["vals"], dtype="INT64", nrows=a["nrows"], ncols=a["ncols"])


def lit_v(gb, lit):
    return gb.Vector.from_coo(lit["v"]["idx"], lit["v"]["vals"], dtype="INT64", size=lit["v"]["size"])


def expect(C, e, where=""):
    assert_coo(C, e["rows"], e["cols"], e["vals"], where)


def test_literals_assign(gb, lit):
    A, case = lit_A(gb, lit), lit["assign"]
    B = gb.Matrix.from_coo(case["B"]["rows"], case["B"]["cols"], case["B"]["vals"], dtype="INT64")
    I, J = case["I"], case["J"]
    for spell in range(6):
        C = A.dup()
        if spell == 0:
            C()[I, J] = B
        elif spell == 1:
            C()[I, J] << B
        elif spell == 2:
            C[:3:2, :6:5]() << B
        elif spell == 3:
            C[I, J] << B
        elif spell == 4:
            C[np.array(I), np.array(J)].update(B)
        else:
            C()[I, J] << B.T.new().T
        expect(C, case["expect"], spell)
    nvals = C.nvals
    C(C.S) << 1
    assert C.nvals == nvals and C.reduce_scalar().new() == nvals
    with pytest.raises(TypeError, match="Invalid type for index"):
        C()[C, [1]] = C
    C << 1
    assert C.nvals == C.nrows * C.ncols and C.reduce_scalar().new() == C.nrows * C.ncols
    with pytest.raises(gb.exceptions.DimensionMismatch):
        A()[lit["assign_wrong_dims"]["I"], lit["assign_wrong_dims"]["J"]] = B


def test_literals_row_column(gb, lit):
    A, v = lit_A(gb, lit), lit_v(gb, lit)
    C = A.dup()
    C()[lit["assign_row"]["row"], :] = v
    expect(C, lit["assign_row"]["expect"], "row")
    C = A.dup()
    C[0, :] << v
    expect(C, lit["assign_row"]["expect"], "row <<")
    C = A.dup()
    C()[:, lit["assign_column"]["col"]] = v
    expect(C, lit["assign_column"]["expect"], "column")
    # assign_row_scalar
    C, D = A.dup(), A.dup()
    C[0, :](v.S) << v
    D(v.S)[0, :] << v
    assert C.isequal(D)
    C(C.S)[:, :] << 1
    C[:, :](C.S) << 1
    assert C.reduce_scalar().new() == C.nvals
    with pytest.raises(TypeError, match="Unable to use Vector mask on Matrix assignment to a Matrix"):
        C[:, :](v.S) << 1
    with pytest.raises(TypeError, match="Unable to use Vector mask on single element assignment to a Matrix"):
        C[0, 0](v.S) << 1
    for bad in (lambda: C(v.S)[0, 0] << v, lambda: C(C.S)[0, 0] << v, lambda: C()[0, 0] << C):
        with pytest.raises(TypeError):
            bad()
    C = A.dup()
    C(v.S)[0, :] = lit["assign_row_scalar"]["value"]
    expect(C, lit["assign_row_scalar"]["expect"], "row scalar")
    # assign_column_scalar
    cs = lit["assign_column_scalar"]
    C, D = A.dup(), A.dup()
    C[:, 0](v.S) << v
    D(v.S)[:, 0] << v
    assert C.isequal(D)
    C = A.dup()
    C()[:, cs["col"]] = v
    C(v.S)[:, cs["col"]] = cs["value"]
    expect(C, cs["expect"], "column scalar")
    C(v.V, replace=True, accum=gb.binary.plus)[:, cs["col"]] = cs["value_accum"]
    expect(C, cs["expect_accum"], "column scalar accum")


def test_literals_scalar_list_element(gb, lit):
    A, sc = lit_A(gb, lit), lit["assign_scalar"]
    blk = sc["block"]
    for key in ((blk["I"], blk["J"]), (slice(*blk["I_slice"]), slice(*blk["J_slice"]))):
        for value in (sc["value"], gb.Scalar.from_value(sc["value"])):
            C = A.dup()
            C()[key] = value
            expect(C, blk["expect"], "block")
    for key in ((sc["row"]["i"], sc["row"]["J"]), (1, slice(2, 5, 2))):
        C = A.dup()
        C()[key] = sc["value"]
        expect(C, sc["row"]["expect"], "row")
    C = A.dup()
    C()[1, 2] = gb.Scalar.from_value(0)
    C[1, 4] << gb.Scalar.from_value(0)
    expect(C, sc["row"]["expect"], "elements")
    for key in ((sc["column"]["I"], sc["column"]["j"]), (slice(1, None, 2), 2)):
        C = A.dup()
        C()[key] = sc["value"]
        expect(C, sc["column"]["expect"], "column")
    es = sc["empty_scalar"]
    B = gb.Matrix.from_coo(es["B"]["rows"], es["B"]["cols"], es["B"]["vals"], dtype="INT64")
    B()[tuple(es["at"])] = gb.Scalar(B.dtype)
    expect(B, es["expect"], "empty scalar")
    # assign_list
    al = lit["assign_list"]
    L = gb.Matrix(int, al["nrows"], al["ncols"])
    for st in al["steps"]:
        rk = st["I"] if "I" in st else st["i"]
        ck = st["J"] if "J" in st else (slice(*st["J_slice"]) if "J_slice" in st else st["j"])
        L()[rk, ck] = st["value"] if "j" not in st else np.asarray(st["value"])
        expect(L, st["expect"], "list")
    for bad in (lambda: L()[0, 1] << [0],):
        with pytest.raises(TypeError):
            bad()
    for key, val in ((([0, 1], 1), [0]), (([0, 1], [1, 2]), [0]), (([0, 1], [1, 2]), [1, 2, 3, 4]), (([0, 1, 2], [1]), [1, 2, 3])):
        with pytest.raises(ValueError, match="shape mismatch"):
            L()[key] = val
    # set_element / remove_element
    se, re_ = lit["set_element"], lit["remove_element"]
    assert A[tuple(se["absent"])].new().value is None and A[tuple(se["present"])].new() == se["present_value"]
    A[1, 1].update(se["set"][0][2])
    A[3, 0] << se["set"][1][2]
    assert A[1, 1].new() == 21 and A[3, 0].new() == -5 and A.nvals == 13
    A(gb.binary.plus)[3, 0] << 7
    assert A[3, 0].new() == 2
    A = lit_A(gb, lit)
    assert A[tuple(re_["remove"])].new() == re_["removed_value"]
    A.remove_element(*re_["remove"])
    assert A[tuple(re_["remove"])].new().value is None and A[tuple(re_["kept"])].new() == re_["kept_value"] and A.nvals == 11
    A.remove_element(*re_["remove"])  # (absent: nothing happens)
    assert A.nvals == 11
    # assign_transpose
    C = gb.Matrix(A.dtype, A.ncols + 1, A.nrows + 1)
    C[: A.ncols, : A.nrows] << A.T
    assert C[: A.ncols, : A.nrows].new().isequal(A.T.new())
    with pytest.raises(TypeError, match="does not support item assignment"):
        C.T[:, :] << A


def test_host_errors(gb, lit):
    A, v = lit_A(gb, lit), lit_v(gb, lit)
    for key in ((0, 0), (ALL, 0), (0, ALL), (ALL, ALL)):
        with pytest.raises(TypeError, match="Bad type"):
            A()[key] = object()
    for key in ((0, 0), (ALL, 0), (0, ALL)):
        with pytest.raises(TypeError, match="Bad type"):
            A()[key] = A
    for key in ((0, 0), (ALL, ALL)):
        with pytest.raises(TypeError, match="Bad type"):
            A()[key] = v
    with pytest.raises(TypeError, match="SUBassign"):
        A[[0, 1], [0, 1]](mask=A.S) << 1
    with pytest.raises(TypeError, match="Invalid type for index"):
        A()[A.S, [1]] = 1
    with pytest.raises(TypeError):
        A()[0] = 1
    with pytest.raises(gb.exceptions.DimensionMismatch):
        A()[0, [1, 2, 3]] = v
    with pytest.raises(gb.exceptions.IndexOutOfBound):
        A()[np.array([1, 9]), :] << 1
    with pytest.raises(TypeError, match="replace"):
        A(replace=True)[[0], [0]] << 1
    assert not hasattr(gb.Matrix, "__setitem__") and not hasattr(gb.Matrix, "__delitem__")
    expect(A, lit["A"], "unchanged by the failed calls")


# ---- 2. seeded random parity ------------------------------------------------------------------------------------------------------------------
def check_matrix_form(gb, rng, m, n, tC, tA, ikind, jkind, Mcoo, structural, comp, replace, accum, *, t0=False, a_dens=0.4, c_dens=0.3, c_iso=False,
                      a_iso=False, where=""):
    Ccoo = draw(rng, m, n, tC, c_dens, c_iso)
    ikey, I = index_list(rng, ikind, m)
    jkey, J = index_list(rng, jkind, n)
    ni, nj = (m if I is None else I.size), (n if J is None else J.size)
    Acoo = draw(rng, ni, nj, tA, a_dens, a_iso)
    a_has, a_val = dense_of((ni, nj), Acoo, NP_OF[tA])
    C, A = mat(gb, Ccoo, tC, m, n), mat(gb, Acoo, tA, ni, nj)
    Mm = mat(gb, Mcoo, "INT32", m, n) if Mcoo is not None else None
    src = A.T.new().T if t0 else A
    updater(C, Mm, structural, comp, replace, accum)[ikey, jkey] << src
    st = stats()
    er, ec, ev = np_assign((m, n), tC, Ccoo, a_has, a_val, I, J, Mcoo, structural, comp, replace, accum)
    assert_coo(C, er, ec, ev, (where, ikind, jkind, structural, comp, replace, accum))
    if not (Mcoo is None and comp):
        full_copy = I is None and J is None and Mcoo is None and accum is None
        assert st["method"] == (6 if full_copy else METHOD_OF_J[jkind]), (st, where)
        assert st["out_nvals"] == len(er)
        if not full_copy and len(Acoo[0]):
            assert st["tiles"] == -(-len(Acoo[0]) // ASG_UNIT), st


@pytest.mark.parametrize("ikind", ["all", "sorted", "shuffled"])
@pytest.mark.parametrize("jkind", ["all", "run", "sorted", "shuffled"])
def test_matrix_form_random(gb, ikind, jkind):
    rng = np.random.default_rng(7 + 10 * ["all", "sorted", "shuffled"].index(ikind) + ["all", "run", "sorted", "shuffled"].index(jkind))
    for k, (mk, structural, comp, replace) in enumerate(MASKS):
        for accum in ACCUMS:
            m, n = int(rng.integers(20, 71)), int(rng.integers(20, 91))
            Mcoo = None
            if mk:
                Mcoo = draw(rng, m, n, "INT32", 0.5)
                Mcoo = (Mcoo[0], Mcoo[1], (Mcoo[2] % 2).astype(np.int32))  # (a valued mask with false entries)
            check_matrix_form(gb, rng, m, n, "INT64", "INT64", ikind, jkind, Mcoo, structural, comp, replace, accum, t0=(k % 3 == 0))


@pytest.mark.parametrize("tC", ALL_TYPES)
def test_matrix_form_types(gb, tC):
    """C and A in all 11 types on one geometry (70 x 90), with and without an accumulator; an iso C, an iso A."""
    rng = np.random.default_rng(ALL_TYPES.index(tC))
    for tA in ALL_TYPES:
        accum = [None, "plus", "min", "second"][ALL_TYPES.index(tA) % 4]
        Mcoo = draw(rng, 70, 90, "INT32", 0.5) if ALL_TYPES.index(tA) % 2 else None
        check_matrix_form(gb, rng, 70, 90, tC, tA, "shuffled", ["sorted", "shuffled", "run"][ALL_TYPES.index(tA) % 3], Mcoo, True, False, False, accum,
                          c_iso=tA == "INT8", a_iso=tA == "FP32", where=(tC, tA))


def test_matrix_form_special(gb):
    rng = np.random.default_rng(5)
    m, n = 40, 50
    # C aliases A: the rows permuted in place; C aliases the mask
    for accum in (None, "plus"):
        Ccoo = draw(rng, m, m, "FP64", 0.3)
        C = mat(gb, Ccoo, "FP64", m, m)
        perm = rng.permutation(m)
        updater(C, None, False, False, False, accum)[perm, :] << C
        a_has, a_val = dense_of((m, m), Ccoo, np.float64)
        assert_coo(C, *np_assign((m, m), "FP64", Ccoo, a_has, a_val, perm, None, accum=accum), ("alias A", accum))
        C = mat(gb, Ccoo, "FP64", m, m)
        Acoo = draw(rng, m, m, "FP64", 0.3)
        a_has, a_val = dense_of((m, m), Acoo, np.float64)
        updater(C, C, True, False, True, accum)[perm, perm] << mat(gb, Acoo, "FP64", m, m)
        assert_coo(C, *np_assign((m, m), "FP64", Ccoo, a_has, a_val, perm, perm, Ccoo, True, False, True, accum), ("alias mask", accum))
    # an empty A without an accumulator clears the region; with one it changes nothing
    Ccoo = draw(rng, m, n, "INT32", 0.5)
    I, J = np.array([3, 1, 39, 0]), np.array([49, 0, 7, 8, 20])
    none = (np.zeros((4, 5), bool), np.zeros((4, 5), np.int32))
    for accum in (None, "plus"):
        C = mat(gb, Ccoo, "INT32", m, n)
        updater(C, None, False, False, False, accum)[I, J] << gb.Matrix("INT32", 4, 5)
        assert_coo(C, *np_assign((m, n), "INT32", Ccoo, *none, I, J, accum=accum), ("empty A", accum))
        assert (C.nvals < len(Ccoo[0])) == (accum is None)
    # ni = 0 under a mask with replace: the entries outside the mask go; without a mask nothing happens
    Mcoo = draw(rng, m, n, "INT32", 0.5)
    C = mat(gb, Ccoo, "INT32", m, n)
    C(mat(gb, Mcoo, "INT32", m, n).S, replace=True)[np.zeros(0, np.int64), J] << gb.Matrix("INT32", 0, 5)
    assert stats()["method"] == 6
    assert_coo(C, *np_assign((m, n), "INT32", Ccoo, np.zeros((0, 5), bool), np.zeros((0, 5)), [], J, Mcoo, True, False, True), "ni = 0")
    C = mat(gb, Ccoo, "INT32", m, n)
    C()[I, np.zeros(0, np.int64)] << gb.Matrix("INT32", 4, 0)
    assert_coo(C, *Ccoo, "nj = 0")


def check_scalar_form(gb, rng, m, n, tC, ikind, jkind, Mcoo, structural, comp, replace, accum, value, *, c_iso=False, where=""):
    Ccoo = draw(rng, m, n, tC, 0.3, c_iso)
    ikey, I = index_list(rng, ikind, m)
    jkey, J = index_list(rng, jkind, n)
    ni, nj = (m if I is None else I.size), (n if J is None else J.size)
    C = mat(gb, Ccoo, tC, m, n)
    Mm = mat(gb, Mcoo, "INT32", m, n) if Mcoo is not None else None
    updater(C, Mm, structural, comp, replace, accum)[ikey, jkey] << value
    st = stats()
    v = value.value if hasattr(value, "value") else value
    er, ec, ev = np_assign((m, n), tC, Ccoo, np.ones((ni, nj), bool), np.full((ni, nj), v), I, J, Mcoo, structural, comp, replace, accum)
    assert_coo(C, er, ec, ev, (where, ikind, jkind, structural, comp, replace, accum))
    assert st["method"] == (18 if Mcoo is not None and not comp else 19), st
    assert st["out_nvals"] == len(er)


@pytest.mark.parametrize("ikind", ["all", "sorted", "shuffled"])
@pytest.mark.parametrize("jkind", ["all", "run", "sorted", "shuffled"])
def test_scalar_form_random(gb, ikind, jkind):
    rng = np.random.default_rng(111 + 10 * ["all", "sorted", "shuffled"].index(ikind) + ["all", "run", "sorted", "shuffled"].index(jkind))
    for k, (mk, structural, comp, replace) in enumerate(MASKS):
        for accum in ACCUMS:
            m, n = int(rng.integers(20, 71)), int(rng.integers(20, 91))
            Mcoo = None
            if mk:
                Mcoo = draw(rng, m, n, "INT32", 0.5)
                Mcoo = (Mcoo[0], Mcoo[1], (Mcoo[2] % 2).astype(np.int32))
            value = gb.Scalar.from_value(5) if k % 2 else 3
            check_scalar_form(gb, rng, m, n, "INT64", ikind, jkind, Mcoo, structural, comp, replace, accum, value)


@pytest.mark.parametrize("tC", ALL_TYPES)
def test_scalar_form_types(gb, tC):
    rng = np.random.default_rng(100 + ALL_TYPES.index(tC))
    Mcoo = draw(rng, 70, 90, "INT32", 0.5)
    for k, value in enumerate((1, 2.0, True, gb.Scalar.from_value(7, dtype="FP32"))):
        check_scalar_form(gb, rng, 70, 90, tC, "shuffled", "shuffled", Mcoo if k % 2 else None, False, False, False, ACCUMS[k], value, c_iso=k == 2,
                          where=(tC, k))


# ---- 3. limits: rows BUILT from sorted column lists ---------------------------------------------------------------------------------------------
def rows_to_coo(rows, base=0):
    """rows: list of column arrays -> (r, c, v) with values that name their position"""
    r = np.concatenate([np.full(len(cs), i) for i, cs in enumerate(rows)] or [np.zeros(0)]).astype(np.int64)
    c = np.concatenate([np.asarray(cs, np.int64) for cs in rows] or [np.zeros(0, np.int64)])
    v = ((r * 7 + c) % 50 + 1 + base).astype(np.int64)
    return r, c, v


def run_built(gb, m, n, Crows, Arows, ikey, I, jkey, J, *, accum=None, Mcoo=None, structural=True, comp=False, replace=False, where=""):
    Ccoo, Acoo = rows_to_coo(Crows), rows_to_coo(Arows, 100)
    ni, nj = (m if I is None else len(I)), (n if J is None else len(J))
    C, A = mat(gb, Ccoo, "INT64", m, n), mat(gb, Acoo, "INT64", ni, nj)
    Mm = mat(gb, Mcoo, "INT32", m, n) if Mcoo is not None else None
    updater(C, Mm, structural, comp, replace, accum)[ikey, jkey] << A
    st = stats()
    a_has, a_val = dense_of((ni, nj), Acoo, np.int64)
    assert_coo(C, *np_assign((m, n), "INT64", Ccoo, a_has, a_val, I, J, Mcoo, structural, comp, replace, accum), where)
    return st


LENS = [0, 1, 63, 64, 65, 127, 128, 129]


@pytest.mark.parametrize("accum", [None, "plus"])
@pytest.mark.parametrize("shape", ["interlocked", "identical"])
def test_limit_list_lengths(gb, accum, shape):
    """every length of C(i, :) against every length of A(i, :): the two lists interlocked (even / odd columns) and identical"""
    n = 300
    Crows = [np.arange(a) * 2 for a in LENS for _ in LENS]
    Arows = [np.arange(b) * 2 + (1 if shape == "interlocked" else 0) for _ in LENS for b in LENS]
    m = len(Crows)
    I = np.arange(m)
    st = run_built(gb, m, n, Crows, Arows, I, I, ALL, None, accum=accum, where=(accum, shape))
    assert st["method"] == 15 and st["tiles"] == -(-sum(len(a) for a in Arows) // ASG_UNIT)


def test_limit_region_edges(gb):
    """entries of C on J[0] - 1, J[0], J[nj - 1], J[nj - 1] + 1 and on rows I[0] - 1, I[ni - 1] + 1; I and J that hold 0 and the last index"""
    m, n = 12, 70
    full = [np.arange(n)] * m
    for jkey, J in ((np.arange(5, 66), np.arange(5, 66)), (np.array([5, 9, 65]), np.array([5, 9, 65])), (np.array([65, 5, 9]), np.array([65, 5, 9])),
                    (np.array([0, n - 1]), np.array([0, n - 1])), (np.array([n - 1, 0]), np.array([n - 1, 0]))):
        for I in (np.arange(3, 9), np.array([0, m - 1]), np.array([m - 1, 4, 0])):
            Arows = [np.arange(len(J))[:: (i % 2) + 1] for i in range(len(I))]  # (A leaves positions empty: they are cleared)
            for accum in (None, "second"):
                run_built(gb, m, n, full, Arows, I, I, jkey, J, accum=accum, where=(J[:3], I[:3], accum))


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_limit_bitmap_word_seam(gb, n):
    """J holds 63 and 64 (where the matrix has them), 0 and the last column: the word seam of the column bitmap"""
    m = 6
    J = np.array(sorted({0, 2, 62, 63, 64, 66, 127, 128, n - 1} & set(range(n))))
    assert not np.all(np.diff(J) == 1)
    full = [np.arange(n)] * m
    for jk in (J, J[::-1].copy()):
        st = run_built(gb, m, n, full, [[] for _ in range(3)], np.array([0, 2, 5]), np.array([0, 2, 5]), jk, jk, where=n)
        assert st["method"] == (16 if jk is J else 17)
        Mcoo = rows_to_coo(full)
        C = mat(gb, rows_to_coo(full), "INT64", m, n)
        C(mat(gb, Mcoo, "INT32", m, n).S)[np.array([0, 2, 5]), jk] << 9
        assert stats()["method"] == 18
        assert_coo(C, *np_assign((m, n), "INT64", rows_to_coo(full), np.ones((3, len(jk)), bool), np.full((3, len(jk)), 9), [0, 2, 5], jk, Mcoo, True),
                   ("scalar", n))


def test_limit_placement_units(gb):
    """rows of A of unit - 1 / unit / unit + 1 entries, a unit that ends on a row end, rows placed out of order"""
    n = ASG_UNIT + 60
    lens = [ASG_UNIT - 1, 1, ASG_UNIT, ASG_UNIT + 1, 0, ASG_UNIT - 1, 3]
    Arows = [np.arange(k) for k in lens]
    m = len(lens) + 2
    Crows = [np.arange(0, n, 97)] * m
    I = np.array([8, 0, 3, 5, 1, 7, 2])
    for jkey, J in ((ALL, None), (np.arange(n)[::-1].copy(), np.arange(n)[::-1].copy())):
        st = run_built(gb, m, n, Crows, Arows, I, I, jkey, J, where="units")
        assert st["tiles"] == -(-sum(lens) // ASG_UNIT) and st["method"] == (15 if J is None else 17)


@pytest.mark.parametrize("n", [PIECE, PIECE + 1])
def test_limit_column_pieces(gb, n):
    """a row long enough to be cut (more than 8192 entries of C and S' together) at 16384 columns (one piece) and 16385 (two pieces of 8193):
    entries on piece_cols - 1 / + 0 / + 1, and a piece that holds only S'"""
    pc = -(-n // (-(-n // PIECE)))
    edge = np.array([c for c in (pc - 1, pc, pc + 1) if c < n])
    Crows = [np.arange(0, pc - 1), np.concatenate([np.arange(0, WR_LONG + 10), edge[edge > WR_LONG + 10]]), np.arange(0, 100)]
    Arows = [np.concatenate([np.arange(0, 50), np.arange(pc, min(pc + 200, n))]), edge, np.arange(n - 70, n)]
    I = np.array([0, 1, 2])
    for accum in (None, "plus"):
        run_built(gb, 3, n, Crows, Arows, I, I, ALL, None, accum=accum, where=(n, accum))
    J = np.unique(np.concatenate([np.arange(0, pc - 1), [c for c in (pc, pc + 1) if c < n], [n - 1]])).astype(np.int64)
    run_built(gb, 3, n, Crows, [np.arange(len(J))[::3]] * 3, I, I, J, J, where=(n, "bitmap"))


def test_limit_unsorted_rows(gb):
    """class (c): rows of A of 1 / 64 / 65 entries, J reversed"""
    n = 80
    J = np.arange(n - 1, 7, -1)
    Arows = [np.arange(1), np.arange(64), np.arange(65), np.arange(len(J))]
    I = np.array([2, 0, 3, 1])
    st = run_built(gb, 5, n, [np.arange(0, n, 3)] * 5, Arows, I, I, J, J)
    assert st["method"] == 17


@pytest.mark.parametrize("ni,nj", [(1, 1), (64, 64), (65, 63), (0, 9)])
def test_limit_dense_scalar_regions(gb, ni, nj):
    m, n = 70, 70
    rng = np.random.default_rng(ni)
    Ccoo = draw(rng, m, n, "FP32", 0.2)
    Mcoo = draw(rng, m, n, "INT32", 0.5)
    I, J = rng.permutation(m)[:ni], rng.permutation(n)[:nj]
    for Mc, accum in ((None, None), (Mcoo, "plus")):
        C = mat(gb, Ccoo, "FP32", m, n)
        Mm = mat(gb, Mc, "INT32", m, n) if Mc is not None else None
        updater(C, Mm, False, Mc is not None, False, accum)[I, J] << 2.0
        st = stats()
        assert st["method"] == (19 if ni else 6) and (not ni or st["tiles"] == ni)
        assert_coo(C, *np_assign((m, n), "FP32", Ccoo, np.ones((ni, nj), bool), np.full((ni, nj), 2.0), I, J, Mc, False, Mc is not None, False, accum),
                   (ni, nj, accum))


def test_limit_mask_filter_blocks(gb):
    """the mask filter: a row of the mask that ends on the first and on the last lane of a 64-entry block, more than one walk of 8 blocks"""
    n = 200
    lens = [64, 1, 63, 65, 0, 127, 1, 128, 129, 0, 0, 190, 64, 64, 2] + [100] * 8
    Mrows = [np.arange(k) for k in lens]
    m = len(lens)
    Mcoo = rows_to_coo(Mrows)
    Mcoo = (Mcoo[0], Mcoo[1], (Mcoo[2] % 3 != 0).astype(np.int32))
    Ccoo = rows_to_coo([np.arange(0, n, 5)] * m)
    I = np.array([k for k in range(m) if k % 4 != 3])[::-1].copy()
    J = np.arange(1, 190)
    for structural in (True, False):
        for ikey, Iv in ((ALL, None), (I, I)):
            C = mat(gb, Ccoo, "INT64", m, n)
            C(mask_arg(mat(gb, Mcoo, "INT32", m, n), structural, False))[ikey, J] << 4
            st = stats()
            assert st["method"] == 18 and st["tiles"] == -(-(-(-len(Mcoo[0]) // 64)) // 8), st
            assert_coo(C, *np_assign((m, n), "INT64", Ccoo, np.ones((m if Iv is None else len(Iv), len(J)), bool),
                                     np.full((m if Iv is None else len(Iv), len(J)), 4), Iv, J, Mcoo, structural), (structural, Iv is None))
    # GrB_ALL x GrB_ALL under a structural mask: the mask's structure is the pattern, no filter (no unit)
    C = mat(gb, Ccoo, "INT64", m, n)
    C(mat(gb, Mcoo, "INT32", m, n).S) << 4
    assert stats()["method"] == 18 and stats()["tiles"] == 0
    assert_coo(C, *np_assign((m, n), "INT64", Ccoo, np.ones((m, n), bool), np.full((m, n), 4), None, None, Mcoo, True), "all x all")


# ---- 4. row / column assign ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [63, 64, 65])
def test_row_col_assign(gb, size):
    rng = np.random.default_rng(size)
    other = 9
    for row_form in (True, False):
        m, n = (other, size) if row_form else (size, other)
        for k, (mk, structural, comp, replace) in enumerate(MASKS):
            accum = ACCUMS[k % 4]
            Ccoo = draw(rng, m, n, "INT64", 0.5)
            idx = int(rng.integers(0, other))
            lkey, L = index_list(rng, ["all", "sorted", "shuffled"][k % 3], size)
            nl = size if L is None else L.size
            ui = np.flatnonzero(rng.random(nl) < 0.6)
            uv = rng.integers(1, 9, ui.size)
            u = gb.Vector.from_coo(ui, uv, dtype="INT64", size=nl)
            mi = np.flatnonzero(rng.random(size) < 0.5)
            mv = rng.integers(0, 2, mi.size)
            C = mat(gb, Ccoo, "INT64", m, n)
            mv_ = gb.Vector.from_coo(mi, mv, dtype="INT32", size=size) if mk else None
            key = (idx, lkey) if row_form else (lkey, idx)
            updater(C, mv_, structural, comp, replace, accum)[key] << u
            # the model: the mask vector laid on the addressed row / column; replace and the mask act there only
            a_has, a_val = np.zeros(nl, bool), np.zeros(nl, np.int64)
            a_has[ui], a_val[ui] = True, uv
            keep = [(r, c, v) for r, c, v in zip(*Ccoo) if (r if row_form else c) != idx]
            line = [(r, c, v) for r, c, v in zip(*Ccoo) if (r if row_form else c) == idx]
            lc = tuple(np.array(x, np.int64) for x in zip(*line)) if line else (np.zeros(0, np.int64),) * 3
            if row_form:
                sub = (np.zeros(len(lc[0]), np.int64), lc[1], lc[2])
                Mc = (np.zeros(mi.size, np.int64), mi, mv) if mk else None
                er, ec, ev = np_assign((1, size), "INT64", sub, a_has[None, :], a_val[None, :], [0], L, Mc, structural, comp, replace, accum)
                er = er + idx
            else:
                sub = (lc[0], np.zeros(len(lc[0]), np.int64), lc[2])
                Mc = (mi, np.zeros(mi.size, np.int64), mv) if mk else None
                er, ec, ev = np_assign((size, 1), "INT64", sub, a_has[:, None], a_val[:, None], L, [0], Mc, structural, comp, replace, accum)
                ec = ec + idx
            kr, kc, kv = (np.array(x, np.int64) for x in zip(*keep)) if keep else (np.zeros(0, np.int64),) * 3
            assert_coo(C, np.concatenate([kr, er]), np.concatenate([kc, ec]), np.concatenate([kv, ev]), (size, row_form, k))


# ---- 5. the C ABI directly ----------------------------------------------------------------------------------------------------------------------------
def _handle(L, name):
    return ctypes.c_void_p(ctypes.c_void_p.in_dll(L, name).value)


def _err(L, C):
    s = ctypes.c_char_p()
    L.GrB_Matrix_error(ctypes.byref(s), C._carg)
    return (s.value or b"").decode()


def _u64(a):
    a = np.ascontiguousarray(a, np.uint64)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def test_c_abi(gb, lit):
    from graphblas_amd import _lib

    L = _lib.lib
    ALLP = _lib.all_indices()
    A = lit_A(gb, lit)
    a = lit["A"]
    before = A.to_coo()

    def unchanged(where):
        assert_coo(A, *before, where)

    # every entry point once per type family
    for tname, ct, x in (("INT64", ctypes.c_int64, 4), ("UINT8", ctypes.c_uint8, 200), ("FP64", ctypes.c_double, 2.5), ("BOOL", ctypes.c_bool, True),
                         ("FP32", ctypes.c_float, -1.5), ("INT16", ctypes.c_int16, -7)):
        C = A.dup(dtype=tname)
        Ccoo = C.to_coo()
        Ia, Ip = _u64([6, 0])
        Ja, Jp = _u64([1, 2, 5])
        assert getattr(L, f"GrB_Matrix_assign_{tname}")(C._carg, None, None, ct(x), Ip, 2, Jp, 3, None) == 0, _err(L, C)
        ex = np_assign((7, 7), tname, Ccoo, np.ones((2, 3), bool), np.full((2, 3), x), [6, 0], [1, 2, 5])
        assert_coo(C, *ex, tname)
        assert getattr(L, f"GrB_Matrix_setElement_{tname}")(C._carg, ct(x), 4, 4) == 0
        ex = np_assign((7, 7), tname, ex, np.ones((1, 1), bool), np.full((1, 1), x), [4], [4])
        assert_coo(C, *ex, (tname, "setElement"))
        assert L.GrB_Matrix_removeElement(C._carg, 4, 4) == 0 and L.GrB_Matrix_removeElement(C._carg, 6, 1) == 0
        ex = np_assign((7, 7), tname, ex, np.zeros((1, 1), bool), np.zeros((1, 1)), [4], [4])
        ex = np_assign((7, 7), tname, ex, np.zeros((1, 1), bool), np.zeros((1, 1)), [6], [1])
        assert_coo(C, *ex, (tname, "removeElement"))
        s = ctypes.c_void_p()
        assert L.GrB_Scalar_new(ctypes.byref(s), _handle(L, f"GrB_{tname}")) == 0
        assert getattr(L, f"GrB_Scalar_setElement_{tname}")(s, ct(x)) == 0
        assert L.GrB_Matrix_assign_Scalar(C._carg, A._carg, None, s, ALLP, 7, ALLP, 7, None) == 0, _err(L, C)
        ex = np_assign((7, 7), tname, ex, np.ones((7, 7), bool), np.full((7, 7), x), None, None, before, False)
        assert_coo(C, *ex, (tname, "assign_Scalar"))
        assert L.GrB_Matrix_setElement_Scalar(C._carg, s, 0, 0) == 0
        assert L.GrB_Scalar_clear(s) == 0 and L.GrB_Matrix_setElement_Scalar(C._carg, s, 0, 1) == 0  # (an empty scalar removes the element)
        ex = np_assign((7, 7), tname, ex, np.ones((1, 1), bool), np.full((1, 1), x), [0], [0])
        ex = np_assign((7, 7), tname, ex, np.zeros((1, 1), bool), np.zeros((1, 1)), [0], [1])
        assert_coo(C, *ex, (tname, "setElement_Scalar"))
        assert L.GrB_Matrix_assign_Scalar(C._carg, None, None, s, ALLP, 7, ALLP, 7, None) == -8 and "EMPTY scalar" in _err(L, C)
        assert_coo(C, *ex, (tname, "empty scalar"))
        L.GrB_Scalar_free(ctypes.byref(s))
        # matrix, row and column forms
        B = gb.Matrix.from_coo([0, 1], [0, 2], [1, 1], dtype=tname, nrows=2, ncols=3)
        assert L.GrB_Matrix_assign(C._carg, None, _handle(L, f"GrB_PLUS_{tname}" if tname != "BOOL" else "GrB_LOR"), B._carg, Ip, 2, Jp, 3, None) == 0, _err(L, C)
        bh, bv = dense_of((2, 3), ([0, 1], [0, 2], [1, 1]), NP_OF[tname])
        ex = np_assign((7, 7), tname, ex, bh, bv, [6, 0], [1, 2, 5], accum="plus")
        assert_coo(C, *ex, (tname, "Matrix_assign"))
        u = gb.Vector.from_coo([0, 2], [1, 1], dtype=tname, size=3)
        assert L.GrB_Row_assign(C._carg, None, None, u._carg, 3, Jp, 3, None) == 0, _err(L, C)
        ex = np_assign((7, 7), tname, ex, np.array([[1, 0, 1]], bool), np.ones((1, 3)), [3], [1, 2, 5])
        assert L.GrB_Col_assign(C._carg, None, None, u._carg, Jp, 3, 6, None) == 0, _err(L, C)
        ex = np_assign((7, 7), tname, ex, np.array([[1], [0], [1]], bool), np.ones((3, 1)), [1, 2, 5], [6])
        assert_coo(C, *ex, (tname, "Row / Col assign"))
    # the error codes (GrB_INDEX_OUT_OF_BOUNDS -105, GrB_INVALID_VALUE -3, ...); after each failed call C is what it was
    B = gb.Matrix.from_coo([0, 1], [0, 2], [1, 1], dtype="INT64", nrows=2, ncols=3)
    u3 = gb.Vector.from_coo([0, 2], [1, 1], dtype="INT64", size=3)
    lists = {"ok_i": _u64([6, 0]), "ok_j": _u64([1, 2, 5]), "oob_i": _u64([6, 7]), "oob_j": _u64([1, 2, 7]), "dup_i": _u64([3, 3]), "dup_j": _u64([1, 5, 1])}
    P = {k: v[1] for k, v in lists.items()}
    for I_, J_, code, text in (("oob_i", "ok_j", -105, "I"), ("ok_i", "oob_j", -105, "J"), ("dup_i", "ok_j", -3, "list I"), ("ok_i", "dup_j", -3, "list J")):
        assert L.GrB_Matrix_assign(A._carg, None, None, B._carg, P[I_], 2, P[J_], 3, None) == code and text in _err(L, A), (I_, J_, _err(L, A))
        unchanged((I_, J_))
        assert L.GrB_Matrix_assign_INT64(A._carg, None, None, 5, P[I_], 2, P[J_], 3, None) == code and text in _err(L, A)
        unchanged((I_, J_, "scalar"))
    assert L.GrB_Matrix_assign(A._carg, None, None, B._carg, P["ok_j"], 3, P["ok_i"], 2, None) == -6  # GrB_DIMENSION_MISMATCH
    assert L.GrB_Matrix_assign(A._carg, B._carg, None, B._carg, P["ok_i"], 2, P["ok_j"], 3, None) == -6  # (the mask has the shape of C)
    assert L.GrB_Row_assign(A._carg, None, None, u3._carg, 7, P["ok_j"], 3, None) == -4 and "row 7" in _err(L, A)  # GrB_INVALID_INDEX
    assert L.GrB_Col_assign(A._carg, None, None, u3._carg, P["ok_j"], 3, 7, None) == -4 and "column 7" in _err(L, A)
    assert L.GrB_Row_assign(A._carg, None, None, u3._carg, 2, P["ok_i"], 2, None) == -6
    assert L.GrB_Row_assign(A._carg, None, None, u3._carg, 2, P["oob_j"], 3, None) == -105
    assert L.GrB_Row_assign(A._carg, u3._carg, None, u3._carg, 2, P["ok_j"], 3, None) == -6  # (the mask is a vector over the row)
    assert L.GrB_Matrix_setElement_INT64(A._carg, 1, 7, 0) == -4 and L.GrB_Matrix_setElement_INT64(A._carg, 1, 0, 7) == -4
    assert L.GrB_Matrix_removeElement(A._carg, 0, 7) == -4 and "(0, 7)" in _err(L, A)
    assert L.GrB_Matrix_assign(A._carg, None, None, B._carg, None, 2, P["ok_j"], 3, None) == -2  # GrB_NULL_POINTER
    unchanged("after the error cases")
    assert a["nrows"] == 7


# ---- 7. memory --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_growth():
    """50 calls of each form on one matrix after a warm-up of 5 (the library keeps freed blocks in its size-class cache, so the first calls
    may grow): free device memory before against after the 50 (tests/test_apply.py item 8)."""
    import torch

    from graphblas_amd import synthetic

    gb = bind("gpu")
    scale = 12
    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, device="cpu")
    A = gb.Matrix.from_csr(ip.numpy(), col.numpy().astype(np.int64), synthetic.edge_weights(col, scale).numpy(), dtype="FP32", ncols=n)
    rng = np.random.default_rng(0)
    V = rng.permutation(n)[: n // 2]
    Vs = np.sort(V)
    B, Bs = A[V, V].new(), A[Vs, :].new()
    v = A[5, :].new()

    def free_bytes():
        gb.Matrix(int, 1, 1).wait()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle(calls):
        C = A.dup()
        for k in range(calls):
            C()[V, V] << B
            C(A.S, "plus")[Vs, :] << Bs
            C(A.S) << 1.0
            C(~A.S)[Vs[:64], Vs[:64]] << 2.0
            C()[k, :] << v
            C(v.S, replace=True)[:, k] << v
            C()[k, k] << 3.0
            C.remove_element(k, k)

    cycle(5)
    before = free_bytes()
    cycle(50)
    after = free_bytes()
    print(f"free after the warm-up: {before / 2**20:.1f} MiB, after 50 more calls of each form: {after / 2**20:.1f} MiB")
    assert after >= before, (before, after)
