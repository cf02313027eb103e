"""GxB_Matrix_eWiseUnion / GxB_Vector_eWiseUnion: ``A.ewise_union(B, op, left_default, right_default)`` -- the DEFS variant of the wavefront
merge of grb_mxm_ewise.inc and k_ewise_union of grb_vecops.hip on the GPU tier, the same sources under the SIMT emulator on the CPU tier.

The expectation is computed HERE with numpy on linearised keys ``i * ncols + j`` (``np.union1d`` / ``np.isin``): with X the operator's
type, ``t = op((X) a, (X) b)`` where both hold an entry, ``op((X) a, (X) beta)`` where A alone does, ``op((X) alpha, (X) b)`` where B alone
does; every cast is a hop of ``O.cast``, every operator exact or IEEE, so results compare bit for bit.  The reference's own literals
(tests/golden/union_diag_literals.json) come first."""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import dense_eval
from oracle import grb_oracle as O
from tests.backend import DEVICES, ROOT, bind
from tests.test_cast_chain import chain, compare_values, np_op
from tests.values import rand_vals

NP_OF = O.NP_OF
CMP = ["eq", "ne", "gt", "lt", "ge", "le"]
WR_LONG = 8192  # (grb_mxm_write.inc: rows with more entries in both lists together are cut into column pieces)


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


@pytest.fixture(scope="module")
def literals():
    with open(os.path.join(ROOT, "tests", "golden", "union_diag_literals.json")) as f:
        return json.load(f)


class Coo:
    """COO tuples of one operand, sorted by key = i * ncols + j."""

    def __init__(self, rows, cols, vals, tname, shape):
        rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
        order = np.lexsort((cols, rows))
        self.rows, self.cols, self.vals = rows[order], cols[order], np.asarray(vals, NP_OF[tname])[order]
        self.tname, self.shape = tname, shape
        self.keys = self.rows * shape[1] + self.cols

    @property
    def T(self):
        return Coo(self.cols, self.rows, self.vals, self.tname, (self.shape[1], self.shape[0]))

    def matrix(self, gb):
        return gb.Matrix.from_coo(self.rows, self.cols, self.vals, dtype=self.tname, nrows=self.shape[0], ncols=self.shape[1])

    def vector(self, gb):
        assert self.shape[0] == 1
        return gb.Vector.from_coo(self.cols, self.vals, dtype=self.tname, size=self.shape[1])


def scalar_type(x):
    return O.NAME_OF_NP[np.asarray(x).dtype] if isinstance(x, np.generic) else {bool: "BOOL", int: "INT64", float: "FP64"}[type(x)]


def union_type(name, A, B, alpha, beta):
    """the rule of union_expression: op over unify(unify(A, beta), unify(alpha, B)); the logical operators are BOOL's"""
    if name in ("lor", "land", "lxor"):
        return "BOOL"
    return O.unify(O.unify(A.tname, scalar_type(beta)), O.unify(scalar_type(alpha), B.tname))


def expect_union(name, A, B, ot, alpha, beta):
    """(keys, values of the operator's result type) of the union with defaults; alpha / beta: numpy or Python scalars"""
    keys = np.union1d(A.keys, B.keys)
    in_a, in_b = np.isin(keys, A.keys), np.isin(keys, B.keys)
    x = np.repeat(chain(np.asarray([alpha], NP_OF[scalar_type(alpha)]), ot), keys.size)
    y = np.repeat(chain(np.asarray([beta], NP_OF[scalar_type(beta)]), ot), keys.size)
    x[in_a], y[in_b] = O.cast(A.vals, ot), O.cast(B.vals, ot)
    return keys, np.asarray(np_op(name, ot, x, y))


def check(C, name, A, B, alpha, beta, where, ot=None, out_type=None):
    ot = ot or union_type(name, A, B, alpha, beta)
    keys, vals = expect_union(name, A, B, ot, alpha, beta)
    tt = "BOOL" if name in CMP else ot
    if out_type is not None:
        vals = chain(vals, out_type)
    assert C.dtype.name == (out_type or tt), (where, C.dtype)
    if C.ndim == 1:
        I, X = C.to_coo()
        got = I.astype(np.int64)
    else:
        assert C.shape == A.shape, where
        I, J, X = C.to_coo()
        got = I.astype(np.int64) * A.shape[1] + J.astype(np.int64)
    assert got.tolist() == keys.tolist(), (where, "pattern")
    compare_values(X, vals, name if name in ("min", "max") else None, where)


def as_default(gb, x, scalar):
    return gb.Scalar.from_value(x, dtype=scalar_type(x)) if scalar else x


# ---- 1. the reference's literals, the exported symbols ----------------------------------------------------------------------------------
def resolve(gb, dotted):
    ns, name = dotted.split(".")
    return getattr(getattr(gb, ns), name)


def test_symbols_and_literals(gb, literals):
    from graphblas_amd import _lib

    header = open(os.path.join(ROOT, "include", "grb_mi355x.h")).read()
    for sym in ("GxB_Matrix_eWiseUnion", "GxB_Vector_eWiseUnion"):
        assert hasattr(_lib.lib, sym) and f"GrB_Info {sym}(" in header, sym
    lit = literals["matrix_union"]
    m, n = lit["nrows"], lit["ncols"]
    A1 = gb.Matrix.from_coo(lit["A1"]["rows"], lit["A1"]["cols"], lit["A1"]["vals"], nrows=m, ncols=n)
    A2 = gb.Matrix.from_coo(lit["A2"]["rows"], lit["A2"]["cols"], lit["A2"]["vals"], nrows=m, ncols=n)
    for case in lit["cases"]:
        left, right = (as_default(gb, case[k], case["scalars"]) for k in ("left", "right"))
        want = gb.Matrix.from_coo(case["rows"], case["cols"], case["vals"], nrows=m, ncols=n, dtype=case["dtype"])
        outs = [A1.ewise_union(A2, resolve(gb, case["op"]), left, right).new(),
                A1.ewise_union(A2.T.new().T, resolve(gb, case["op"]), left, right).new(),
                A1.T.ewise_union(A2.T.new(), resolve(gb, case["op"]), left, right).new().T.new()]
        for k, out in enumerate(outs):
            assert out.dtype.name == case["dtype"] and (out.isclose(want) if case["dtype"] == "FP64" else out.isequal(want)), (case["source"], k)
    with pytest.raises(gb.exceptions.DimensionMismatch):
        A1.ewise_union(gb.Matrix(int, lit["bad_shape"]["nrows"], lit["bad_shape"]["ncols"]), gb.binary.plus, 0, 0)
    for args in ((A2, 20), (10, A2)):
        with pytest.raises(TypeError, match=lit["type_error"]["match"]):
            A1.ewise_union(A2, gb.binary.plus, *args)
    lit = literals["vector_union"]
    v1 = gb.Vector.from_coo(lit["v1"]["idx"], lit["v1"]["vals"], size=lit["size"])
    v2 = gb.Vector.from_coo(lit["v2"]["idx"], lit["v2"]["vals"], size=lit["size"])
    for case in lit["cases"]:
        left, right = (as_default(gb, case[k], case["scalars"]) for k in ("left", "right"))
        want = gb.Vector.from_coo(case["idx"], case["vals"], size=lit["size"], dtype=case["dtype"])
        out = v1.ewise_union(v2, resolve(gb, case["op"]), left, right).new()
        assert out.dtype.name == case["dtype"] and (out.isclose(want) if case["dtype"] == "FP64" else out.isequal(want)), case["source"]
    with pytest.raises(gb.exceptions.DimensionMismatch):
        v1.ewise_union(gb.Vector(int, lit["bad_size"]["size"]), gb.binary.plus, 0, 0)
    for args in ((v2, 20), (10, v2)):
        with pytest.raises(TypeError, match=lit["type_error"]["match"]):
            v1.ewise_union(v2, gb.binary.plus, *args)
    # what ewise_add cannot do: an entry of B alone is 0 - b, not b
    assert v1.ewise_add(v2, gb.binary.minus).new().to_coo()[1].tolist() == [1, 2]
    assert v1.ewise_union(v2, gb.binary.minus, 0, 0).new().to_coo()[1].tolist() == [1, -2]


# ---- 2. chunk boundaries -----------------------------------------------------------------------------------------------------------
LENS = [0, 1, 63, 64, 65, 127, 128, 129, 200]
NCOLS = 420


def boundary_rows(rng):
    """One row per (len(A), len(B), relation): disjoint (even / odd columns), identical, interlocked (alternating runs of 1..3), nested
    (the shorter list inside the longer); then the two lane-63 rows: an A-single on lane 63 of the first chunk whose B neighbour is the
    first entry of B's next chunk, and the reverse."""
    rows_a, rows_b = [], []
    for la in LENS:
        for lb in LENS:
            for rel in ("disjoint", "identical", "interlocked", "nested"):
                if rel == "identical" and la != lb:
                    continue
                if rel == "disjoint":
                    a, b = 2 * np.sort(rng.choice(NCOLS // 2, la, replace=False)), 2 * np.sort(rng.choice(NCOLS // 2, lb, replace=False)) + 1
                elif rel == "identical":
                    a = b = np.sort(rng.choice(NCOLS, la, replace=False))
                elif rel == "interlocked":
                    cols = np.sort(rng.choice(NCOLS, la + lb, replace=False))
                    side = np.repeat(np.arange(la + lb) % 2, rng.integers(1, 4, la + lb))[: la + lb]
                    pick_a = np.zeros(la + lb, bool)
                    pick_a[np.concatenate([np.flatnonzero(side == 0), np.flatnonzero(side == 1)])[:la]] = True
                    a, b = cols[pick_a], cols[~pick_a]
                else:
                    big = np.sort(rng.choice(NCOLS, max(la, lb), replace=False))
                    small = np.sort(rng.choice(big, min(la, lb), replace=False))
                    a, b = (big, small) if la >= lb else (small, big)
                rows_a.append(a), rows_b.append(b)
    a = np.arange(0, 256, 2)  # 128 entries: lane 63 of the first chunk holds column 126, which the other list does not hold
    b = np.concatenate([[0], np.arange(1, 126, 2), np.arange(127, 267, 2)])  # 64 entries up to column 125, then 127 opens the next chunk
    assert a[63] == 126 and b[63] == 125 and b[64] == 127
    rows_a += [a, b]
    rows_b += [b, a]
    return rows_a, rows_b


def rows_to_coo(rng, lists, tname, ncols, domain=None):
    r = np.concatenate([np.full(c.size, i, np.int64) for i, c in enumerate(lists)])
    c = np.concatenate(lists).astype(np.int64)
    vals = rand_vals(rng, r.size, tname, domain) if domain else rand_vals(rng, r.size, tname)
    return Coo(r, c, vals, tname, (len(lists), ncols))


# (operator, type, alpha, beta): defaults that tell the three branches apart
BRANCH_CASES = [
    ("minus", "INT64", 7, -3), ("first", "INT64", 7, -3), ("second", "INT64", 7, -3), ("gt", "INT64", 50, 20),
    ("min", "FP32", np.float32(np.nan), np.float32(2)), ("min", "FP64", 3.0, float("nan")),
    ("plus", "FP32", np.float32(-0.0), np.float32(-0.0)), ("plus", "FP64", -0.0, -0.0),
    ("minus", "UINT8", np.uint8(3), np.uint8(250)), ("minus", "BOOL", True, False), ("le", "FP64", 1.0, float("nan")),
]


@pytest.fixture(scope="module")
def boundary_lists():
    return boundary_rows(np.random.default_rng(7100))


@pytest.mark.parametrize("name,tname,alpha,beta", BRANCH_CASES, ids=[f"{c[0]}-{c[1]}" for c in BRANCH_CASES])
def test_chunk_boundaries(gb, boundary_lists, name, tname, alpha, beta):
    from graphblas_amd import device

    rng = np.random.default_rng(7101)
    la, lb = boundary_lists
    assert len(la) > 200  # (more than 50 workgroups of four units)
    domain = "exact" if tname.startswith("FP") else None
    A, B = rows_to_coo(rng, la, tname, NCOLS, domain), rows_to_coo(rng, lb, tname, NCOLS, domain)
    a, b = A.matrix(gb), B.matrix(gb)
    C = a.ewise_union(b, getattr(gb.binary, name), alpha, beta).new()
    assert device.last_stats()["method"] == 21
    check(C, name, A, B, alpha, beta, f"{name} {tname}")
    if name in ("minus", "gt"):  # the operands swapped: the branches swap with them
        check(b.ewise_union(a, getattr(gb.binary, name), alpha, beta).new(), name, B, A, alpha, beta, f"{name} {tname} swapped")


@pytest.mark.parametrize("nrows", [255, 256, 257])
def test_row_counts_around_a_workgroup(gb, nrows):
    rng = np.random.default_rng(7200 + nrows)
    shape = (nrows, 90)
    ra, ca = np.nonzero(rng.random(shape) < 0.1)
    rb, cb = np.nonzero(rng.random(shape) < 0.1)
    A, B = Coo(ra, ca, rand_vals(rng, ra.size, "INT32"), "INT32", shape), Coo(rb, cb, rand_vals(rng, rb.size, "INT32"), "INT32", shape)
    check(A.matrix(gb).ewise_union(B.matrix(gb), gb.binary.minus, np.int32(1000), np.int32(-5)).new(), "minus", A, B, np.int32(1000),
          np.int32(-5), f"{nrows} rows")


def test_long_row_pieces(gb):
    """Row 1: 5000 + 4000 entries over 16385 columns (more than WR_LONG together): column pieces of which one holds A-singles only, one
    B-singles only, one nothing, the rest a mix; rows 0 and 2 are short."""
    rng = np.random.default_rng(7300)
    ncols = 16385
    a1 = np.concatenate([np.sort(rng.choice(np.arange(0, 3000), 2600, replace=False)), np.sort(rng.choice(np.arange(9000, 16385), 2400, replace=False))])
    b1 = np.concatenate([np.sort(rng.choice(np.arange(3000, 6000), 2500, replace=False)), np.sort(rng.choice(np.arange(9000, 16385), 1500, replace=False))])
    assert a1.size + b1.size > WR_LONG and not np.isin(np.arange(6000, 9000), np.concatenate([a1, b1])).any()
    la, lb = [np.array([0, 16384]), a1, np.array([5])], [np.array([16384]), b1, np.array([], np.int64)]
    for tname, alpha, beta in (("INT64", 11, -13), ("FP64", 0.5, -0.25)):
        A, B = rows_to_coo(rng, la, tname, ncols), rows_to_coo(rng, lb, tname, ncols)
        C = A.matrix(gb).ewise_union(B.matrix(gb), gb.binary.minus, alpha, beta).new()
        check(C, "minus", A, B, alpha, beta, f"long row {tname}")
        Cp = C.to_csr()[0]
        assert Cp.tolist() == [0, 2, 2 + np.union1d(a1, b1).size, 3 + np.union1d(a1, b1).size]


# ---- 3. types ----------------------------------------------------------------------------------------------------------------------
# (A, B, operator type, C, type of the Scalar defaults): lossy hops into the operator's type and out of it (tests/test_cast_chain.py)
TYPE_CASES = [("FP64", "INT64", "INT8", "INT32", "FP32"), ("FP32", "FP64", "UINT16", "UINT8", "INT64"), ("INT64", "UINT64", "FP32", "FP64", "INT8"),
              ("UINT64", "INT8", "INT32", "BOOL", "FP64"), ("INT8", "FP64", "BOOL", "INT16", "INT32"), ("FP64", "FP32", "UINT64", "INT8", "FP32")]


@pytest.mark.parametrize("ta,tb,ot,tc,ts", TYPE_CASES)
def test_type_chain(gb, ta, tb, ot, tc, ts):
    from tests.test_cast_chain import entry_values, source_values

    shape = (3, 70)
    rows_a = np.concatenate([np.zeros(70, np.int64), np.ones(24, np.int64), np.full(3, 2)])
    cols_a = np.concatenate([np.arange(70), np.arange(0, 70, 3), [1, 68, 69]])
    rows_b = np.concatenate([np.zeros(35, np.int64), np.ones(70, np.int64), np.full(3, 2)])
    cols_b = np.concatenate([np.arange(0, 70, 2), np.arange(70), [0, 1, 2]])
    A, B = Coo(rows_a, cols_a, entry_values(ta, rows_a.size), ta, shape), Coo(rows_b, cols_b, entry_values(tb, rows_b.size, 3), tb, shape)
    a, b = A.matrix(gb), B.matrix(gb)
    sv = source_values(ts)
    for name in ("minus", "second", "first", "lt", "max"):
        for alpha, beta in ((sv[1], sv[-1]), (sv[-2], sv[0])):
            expr = a.ewise_union(b, getattr(gb.binary, name)[ot], gb.Scalar.from_value(alpha, dtype=ts), gb.Scalar.from_value(beta, dtype=ts))
            check(expr.new(dtype=tc), name, A, B, alpha, beta, f"{ta} {name}[{ot}] {tb} -> {tc}, defaults {ts} {alpha} {beta}", ot=ot, out_type=tc)


@pytest.mark.parametrize("tname", ["INT64", "FP32", "BOOL"])
def test_iso_operands_and_aliases(gb, tname):
    from tests.test_matrix_ewise import draw_coo, iso_matrix

    rng = np.random.default_rng(7400 + len(tname))
    shape = (9, 150)
    alpha, beta = {"INT64": (5, -6), "FP32": (np.float32(5), np.float32(-6)), "BOOL": (True, False)}[tname]

    def draw(iso=False):
        X = draw_coo(rng, shape, tname, 0.5, iso=iso)
        return Coo(X.rows, X.cols, X.vals, tname, shape)

    A, B, Ai, Bi = draw(), draw(), draw(True), draw(True)
    a, b, ai, bi = A.matrix(gb), B.matrix(gb), iso_matrix(gb, Ai), iso_matrix(gb, Bi)
    for x, y, X, Y, side in ((ai, b, Ai, B, "A"), (a, bi, A, Bi, "B"), (ai, bi, Ai, Bi, "both")):
        for name in ("minus", "second", "ge"):
            check(x.ewise_union(y, getattr(gb.binary, name), alpha, beta).new(), name, X, Y, alpha, beta, f"iso {side} {tname} {name}")
    # A is B; C is A
    check(a.ewise_union(a, gb.binary.minus, alpha, beta).new(), "minus", A, A, alpha, beta, f"A is B {tname}")
    C = A.matrix(gb)
    C << C.ewise_union(b, gb.binary.minus, alpha, beta)
    check(C, "minus", A, B, alpha, beta, f"C is A {tname}")


# ---- 4. the write rule, the descriptor ----------------------------------------------------------------------------------------------
def test_write_rule(gb):
    rng = np.random.default_rng(7500)
    shape, tname, np_t = (6, 70), "INT64", np.int64

    def small(dens, t=tname):
        r, c = np.nonzero(rng.random(shape) < dens)
        return Coo(r, c, rand_vals(rng, r.size, t), t, shape)

    def dense(X):
        has, val = np.zeros(shape, bool), np.zeros(shape, NP_OF[X.tname])
        has[X.rows, X.cols], val[X.rows, X.cols] = True, X.vals
        return val, has

    compared = 0
    for mask_kind in (None, "S", "V", "~S", "~V"):
        for accum in (None, "plus"):
            for replace in ((False, True) if mask_kind else (False,)):
                A, B, Cc, Mc = small(0.5), small(0.5), small(0.4), small(0.5, "INT8")
                C = Cc.matrix(gb)
                kw = {}
                if mask_kind:
                    M = Mc.matrix(gb)
                    mk = M.S if "S" in mask_kind else M.V
                    kw = dict(mask=~mk if "~" in mask_kind else mk, replace=replace)
                if accum:
                    kw["accum"] = gb.binary.plus
                C(**kw) << A.matrix(gb).ewise_union(B.matrix(gb), gb.binary.minus, 100, 1000)
                keys, vals = expect_union("minus", A, B, tname, 100, 1000)
                T = Coo(keys // shape[1], keys % shape[1], vals, tname, shape)
                Mval, Mhas = dense(Mc) if mask_kind else (None, None)
                Nval, Nhas = dense_eval.write(*dense(Cc), *dense(T), Mval, Mhas, comp=bool(mask_kind) and "~" in mask_kind,
                                              struct=bool(mask_kind) and "S" in mask_kind, accum=accum, replace=replace, np_t=np_t)
                I, J, X = C.to_coo()
                rr, cc = np.nonzero(Nhas)
                where = f"mask={mask_kind} accum={accum} replace={replace}"
                assert I.tolist() == rr.tolist() and J.tolist() == cc.tolist() and X.tolist() == Nval[rr, cc].tolist(), where
                compared += 1
    assert compared == 18


def test_transposed(gb):
    rng = np.random.default_rng(7600)
    shape = (40, 40)
    ra, ca = np.nonzero(rng.random(shape) < 0.2)
    rb, cb = np.nonzero(rng.random(shape) < 0.2)
    A, B = Coo(ra, ca, rand_vals(rng, ra.size, "INT64"), "INT64", shape), Coo(rb, cb, rand_vals(rng, rb.size, "INT64"), "INT64", shape)
    a, b = A.matrix(gb), B.matrix(gb)
    op = gb.binary.minus
    check(a.T.ewise_union(b, op, 7, -3).new(), "minus", A.T, B, 7, -3, "T0")
    check(a.ewise_union(b.T, op, 7, -3).new(), "minus", A, B.T, 7, -3, "T1")
    check(a.T.ewise_union(b.T, op, 7, -3).new(), "minus", A.T, B.T, 7, -3, "T0 T1")
    check(a.ewise_union(a.T, op, 0, 0).new(), "minus", A, A.T, 0, 0, "A - A.T")


# ---- 5. empty operands, errors, stats -------------------------------------------------------------------------------------------------
def test_empty_operands_and_stats(gb):
    from graphblas_amd import device

    rng = np.random.default_rng(7700)
    shape = (5, 130)
    r, c = np.nonzero(rng.random(shape) < 0.4)
    A = Coo(r, c, rand_vals(rng, r.size, "FP64", "exact"), "FP64", shape)
    E = Coo([], [], [], "FP64", shape)
    a, e = A.matrix(gb), E.matrix(gb)
    for name in ("minus", "lt", "second", "first", "plus"):
        op = getattr(gb.binary, name)
        check(a.ewise_union(e, op, 2.5, -0.0).new(), name, A, E, 2.5, -0.0, f"B empty {name}")
        assert device.last_stats()["method"] == 22
        check(e.ewise_union(a, op, -0.0, 2.5).new(), name, E, A, -0.0, 2.5, f"A empty {name}")
        assert device.last_stats()["method"] == 22
    C = e.ewise_union(e, gb.binary.minus, 1.0, 2.0).new()
    assert C.nvals == 0 and device.last_stats()["method"] == 6
    # under a mask the short cut hands the write rule one value per entry
    M = Coo(r[::2], c[::2], np.ones(r[::2].size), "FP64", shape)
    C = a.ewise_union(e, gb.binary.second, 0.0, 9.0).new(mask=M.matrix(gb).S)
    I, J, X = C.to_coo()
    assert (I.astype(np.int64) * shape[1] + J.astype(np.int64)).tolist() == M.keys.tolist() and set(X.tolist()) == {9.0}
    check(a.ewise_union(a, gb.binary.minus, 1.0, 2.0).new(), "minus", A, A, 1.0, 2.0, "kernel path")
    st = device.last_stats()
    assert st["method"] == 21 and st["out_nvals"] == A.keys.size and st["kernel_launches"] > 0, st


@pytest.mark.parametrize("ta,tb,ot,tc,ts", TYPE_CASES)
def test_empty_operand_type_chain(gb, ta, tb, ot, tc, ts):
    """The one-operand-empty short cut (the bound-scalar stream of apply) makes the same hops as the merge: operand and default into the
    operator's type, the result (BOOL for a comparison) into C's type; a non-iso and an iso operand on either side."""
    from graphblas_amd import device
    from tests.test_cast_chain import entry_values, source_values
    from tests.test_matrix_ewise import iso_matrix

    shape = (3, 70)
    rows = np.concatenate([np.zeros(70, np.int64), np.ones(24, np.int64), np.full(3, 2)])
    cols = np.concatenate([np.arange(70), np.arange(0, 70, 3), [1, 68, 69]])
    sv = source_values(ts)
    for side, tx in (("B empty", ta), ("A empty", tb)):
        te = tb if side == "B empty" else ta  # the empty operand's type
        X = Coo(rows, cols, entry_values(tx, rows.size), tx, shape)
        E = Coo([], [], [], te, shape)
        for iso_value in (None, source_values(tx)[-1]):
            if iso_value is not None:
                X = Coo(rows, cols, np.full(rows.size, iso_value), tx, shape)
            x, e = (iso_matrix(gb, X) if iso_value is not None else X.matrix(gb)), E.matrix(gb)
            for name in ("minus", "second", "first", "lt", "min"):
                for alpha, beta in ((sv[1], sv[-1]), (sv[-2], sv[0])):
                    a, b, A, B = (x, e, X, E) if side == "B empty" else (e, x, E, X)
                    expr = a.ewise_union(b, getattr(gb.binary, name)[ot], gb.Scalar.from_value(alpha, dtype=ts), gb.Scalar.from_value(beta, dtype=ts))
                    C = expr.new(dtype=tc)
                    assert device.last_stats()["method"] == 22
                    check(C, name, A, B, alpha, beta, f"{side} iso={iso_value} {tx} {name}[{ot}] -> {tc}, defaults {ts} {alpha} {beta}", ot=ot,
                          out_type=tc)


@pytest.mark.parametrize("tname", ["FP32", "FP64"])
def test_empty_operand_nan_and_signed_zero_defaults(gb, tname):
    """``min`` with a NaN default (the operand wins, NaN against NaN stays NaN) and ``plus`` with -0.0 through the short cut."""
    from graphblas_amd import device

    rng = np.random.default_rng(7750)
    np_t, shape = NP_OF[tname], (4, 100)
    r, c = np.nonzero(rng.random(shape) < 0.5)
    A, E = Coo(r, c, rand_vals(rng, r.size, tname, "exact"), tname, shape), Coo([], [], [], tname, shape)
    a, e = A.matrix(gb), E.matrix(gb)
    for name, default in (("min", np_t(np.nan)), ("max", np_t(np.nan)), ("plus", np_t(-0.0)), ("minus", np_t(-0.0))):
        op = getattr(gb.binary, name)
        check(a.ewise_union(e, op, np_t(1), default).new(), name, A, E, np_t(1), default, f"B empty {name} {tname}")
        assert device.last_stats()["method"] == 22
        check(e.ewise_union(a, op, default, np_t(1)).new(), name, E, A, default, np_t(1), f"A empty {name} {tname}")
        assert device.last_stats()["method"] == 22


def _handle(L, name):
    return ctypes.c_void_p(ctypes.c_void_p.in_dll(L, name).value)


def test_errors_leave_the_output_unchanged(gb):
    from graphblas_amd import _lib
    from graphblas_amd.base import GrBScalarArg

    L = _lib.lib
    A = gb.Matrix.from_coo([0, 1], [1, 2], [3, 4], nrows=3, ncols=4)
    B = gb.Matrix.from_coo([0, 2], [1, 3], [5, 6], nrows=3, ncols=4)
    C = gb.Matrix.from_coo([2], [0], [77], nrows=3, ncols=4)
    before = [x.tolist() for x in C.to_coo()]
    with pytest.raises(gb.exceptions.EmptyObject, match="alpha"):
        C << A.ewise_union(B, gb.binary.minus, gb.Scalar(int), 0)
    with pytest.raises(gb.exceptions.EmptyObject, match="beta"):
        C << A.ewise_union(B, gb.binary.minus, 0, gb.Scalar(int))
    with pytest.raises(gb.exceptions.DimensionMismatch):
        C << A.ewise_union(gb.Matrix.from_coo([0], [0], [1], nrows=3, ncols=5).T.new().T.new(), gb.binary.minus, 0, 0)
    with pytest.raises(TypeError, match="Semiring"):
        A.ewise_union(B, gb.semiring.plus_times, 0, 0)
    with pytest.raises(TypeError):
        A.ewise_union(B, gb.binary.minus)  # both defaults are required
    zero = GrBScalarArg(gb.Scalar.from_value(0))
    D = gb.Matrix(float, 3, 4)
    assert L.GxB_Matrix_eWiseUnion(D._carg, None, None, _handle(L, "GrB_DIV_FP64"), A._carg, zero._carg, B._carg, zero._carg, None) == -8
    plus = _handle(L, "GrB_PLUS_INT64")
    assert L.GxB_Matrix_eWiseUnion(C._carg, None, None, plus, A._carg, None, B._carg, zero._carg, None) == -2   # GrB_NULL_POINTER
    assert L.GxB_Matrix_eWiseUnion(C._carg, None, None, None, A._carg, zero._carg, B._carg, zero._carg, None) == -2
    assert L.GxB_Matrix_eWiseUnion(C._carg, None, _handle(L, "GrB_PLUS_FP32"), plus, A._carg, zero._carg, B._carg, zero._carg, None) == -5
    assert L.GxB_Matrix_eWiseUnion(gb.Matrix(int, 4, 3)._carg, None, None, plus, A._carg, zero._carg, B._carg, zero._carg, None) == -6
    assert [x.tolist() for x in C.to_coo()] == before
    w = gb.Vector.from_coo([1], [5], size=4)
    u, v = gb.Vector.from_coo([0], [1], size=4), gb.Vector.from_coo([3], [2], size=4)
    with pytest.raises(gb.exceptions.EmptyObject):
        w << u.ewise_union(v, gb.binary.minus, gb.Scalar(int), 0)
    assert L.GxB_Vector_eWiseUnion(w._carg, None, None, _handle(L, "GxB_POW_INT64"), u._carg, zero._carg, v._carg, zero._carg, None) == -8
    assert [x.tolist() for x in w.to_coo()] == [[1], [5]]


# ---- 6. vectors ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 16383, 16384, 16385])
def test_vector_union(gb, n):
    rng = np.random.default_rng(7800 + n)
    last0 = ((n - 1) // 64) * 64  # first bit of the last presence word

    def draw(tname, forced, domain=None):
        idx = np.union1d(np.flatnonzero(rng.random(n) < 0.3), np.asarray(forced, np.int64))
        vals = rand_vals(rng, idx.size, tname, domain) if domain else rand_vals(rng, idx.size, tname)
        return Coo(np.zeros(idx.size, np.int64), idx, vals, tname, (1, n))

    for name, tname, alpha, beta in BRANCH_CASES:
        domain = "exact" if tname.startswith("FP") else None
        U, V = draw(tname, [last0], domain), draw(tname, [n - 1], domain)
        u, v = U.vector(gb), V.vector(gb)
        check(u.ewise_union(v, getattr(gb.binary, name), alpha, beta).new(), name, U, V, alpha, beta, f"n={n} {name} {tname}")
    E = Coo([], [], [], "INT64", (1, n))
    U = draw("INT64", [last0, n - 1])
    check(U.vector(gb).ewise_union(E.vector(gb), gb.binary.minus, 7, -3).new(), "minus", U, E, 7, -3, f"n={n} v empty")
    check(E.vector(gb).ewise_union(U.vector(gb), gb.binary.minus, 7, -3).new(), "minus", E, U, 7, -3, f"n={n} u empty")
    assert E.vector(gb).ewise_union(E.vector(gb), gb.binary.minus, 7, -3).new().nvals == 0
    # another operator type, Scalar defaults of a third, the output in a fourth; mask and accumulator
    U, V = draw("FP64", [0]), draw("INT64", [n - 1])
    expr = U.vector(gb).ewise_union(V.vector(gb), gb.binary.minus["INT8"], gb.Scalar.from_value(np.float32(300.5)), gb.Scalar.from_value(np.float32(-7)))
    check(expr.new(dtype="INT32"), "minus", U, V, np.float32(300.5), np.float32(-7), f"n={n} types", ot="INT8", out_type="INT32")
    w = U.vector(gb).dup(dtype="INT64")
    w(V.vector(gb).S, gb.binary.plus) << U.vector(gb).ewise_union(V.vector(gb), gb.binary.minus["INT64"], 1, 2)
    keys, t = expect_union("minus", U, V, "INT64", 1, 2)
    has, val = np.zeros(n, bool), np.zeros(n, np.int64)
    has[U.cols], val[U.cols] = True, O.cast(U.vals, "INT64")
    tv = np.zeros(n, np.int64)
    tv[keys] = t
    allow = np.zeros(n, bool)
    allow[V.cols] = True
    upd = allow & np.isin(np.arange(n), keys)
    val[upd] = np.where(has[upd], val[upd] + tv[upd], tv[upd])
    has |= upd
    I, X = w.to_coo()
    assert I.tolist() == np.flatnonzero(has).tolist() and X.tolist() == val[has].tolist(), f"n={n} mask + accum"
