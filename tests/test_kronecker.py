"""GrB_kronecker: ``C(M, accum) << A.kronecker(B, op)`` -- the closed-form row pointers and the entry-parallel fill of grb_kron.hip on
the GPU tier, the same sources under the SIMT emulator on the CPU tier.

1. the reference's own literal (tests/golden/kronecker_literals.json) through every spelling the host has and the three C entry points;
2. seeded random parity against an expectation computed HERE with numpy on the COO tuples (rows ``ra * mb + rb``, columns
   ``ca * nb + cb``, the operator in ``np.promote_types`` of the two dtypes, a cast, then the dense restatement of the write rule of
   tests/test_select.py) -- independent of the library and of the oracle; bit for bit;
3. the write rule on one compact grid;
4. the fill kernel at its limits, on operands built from lists of row lengths: a wavefront's unit is 8 blocks of 64 entries of T
   (SEL_BPW of grb_index_ops.hpp, the unit of GrB_apply by position), one search per unit, then the walk;
5. the short cuts (empty and iso products);
6. properties that do not go through the numpy restatement;
7. aliasing;
8. the C ABI and the errors;
9. no growth of device memory over repeated calls (GPU tier).

ANY may return either operand; the library returns the first, and the expectation here says so.  IEEE leaves min(-0, +0) open, so min /
max results are compared with a zero matching a zero of either sign (tests/values.py), everything else as bit patterns.  Integer
operands are drawn so that no product leaves the type's range: signed overflow pins nothing.

NOT reached at a test's size: nnz(A) * nnz(B) beyond int64 (GrB_OUT_OF_MEMORY by a checked multiplication before any allocation), row
pointers that cannot be allocated, and a row of T with 2^32 or more entries (the 64-bit branch of the fill's division) -- each needs
operands of more than 2^31 entries or a product of more than 2^32."""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.backend import DEVICES, ROOT, bind
from tests.test_select import NP_OF, TYPES, _handle, _matrix_error, assert_coo, draw_coo, np_write_rule, stored_iso
from tests.values import rand_vals, same_fp

ALL_TYPES = ["BOOL", "INT8", "INT16", "INT32", "INT64", "UINT8", "UINT16", "UINT32", "UINT64", "FP32", "FP64"]
assert set(TYPES) <= set(ALL_TYPES)
NAME_OF = {np.dtype(v): k for k, v in NP_OF.items()}
OPS = ["times", "plus", "min", "first", "second", "pair", "any", "gt", "eq"]
COMPARE = ("gt", "eq")
UNIT = 8 * 64  # entries of T one wavefront fills
FULL = 20  # GrX_last_stats method of the value fill; 6 = a short cut


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


@pytest.fixture(scope="module")
def literals():
    with open(os.path.join(ROOT, "tests", "golden", "kronecker_literals.json")) as f:
        return json.load(f)


def stats(gb):
    from graphblas_amd import device

    return device.last_stats()


def units_of(nnz):
    return -(-(-(-nnz // 64)) // 8)


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def np_kron(op, a, b, mb, nb):
    """T = A (x) B over COO tuples a = (ra, ca, va), b = (rb, cb, vb): (rows, cols, values in T's own type, the zero-sign freedom)."""
    (ra, ca, va), (rb, cb, vb) = (tuple(np.asarray(x) for x in a), tuple(np.asarray(x) for x in b))
    rows = (ra.astype(np.int64)[:, None] * mb + rb.astype(np.int64)[None, :]).ravel()
    cols = (ca.astype(np.int64)[:, None] * nb + cb.astype(np.int64)[None, :]).ravel()
    xt = np.promote_types(va.dtype, vb.dtype)
    shape = (ra.size, rb.size)
    with np.errstate(all="ignore"):
        p = np.broadcast_to(va.astype(xt)[:, None], shape).ravel()
        q = np.broadcast_to(vb.astype(xt)[None, :], shape).ravel()
        if xt == np.dtype(bool):
            table = {"times": np.logical_and, "plus": np.logical_or, "min": np.logical_and}
        else:
            fl = xt.kind == "f"
            table = {"times": lambda x, y: x * y, "plus": lambda x, y: x + y, "min": np.fmin if fl else np.minimum}
        table.update({"first": lambda x, y: x, "second": lambda x, y: y, "pair": lambda x, y: np.ones_like(x), "any": lambda x, y: x,
                      "gt": lambda x, y: x > y, "eq": lambda x, y: x == y})
        t = np.asarray(table[op](p, q)).astype(bool if op in COMPARE else xt)
    return rows, cols, t, ("min" if op == "min" else None)


def draw_vals(rng, k, tname):
    """Floating point: the "exact" domain (integers -8 .. 8, NaN, +-inf, +-0.0); integers small enough that no product or sum of two
    leaves the narrowest type."""
    if tname.startswith("FP"):
        return rand_vals(rng, k, tname, "exact")
    if tname == "BOOL":
        return rand_vals(rng, k, tname)
    lo = -9 if tname.startswith("INT") else 0
    return rng.integers(lo, 10, k).astype(NP_OF[tname])


def draw_operand(rng, m, n, tname, dens):
    has = rng.random((m, n)) < dens
    r, c = np.nonzero(has)
    return r, c, draw_vals(rng, r.size, tname)


def wider(tname):
    """An output type that differs from T's and that numpy's astype casts like the library does (no float -> integer)."""
    return "FP32" if tname == "FP64" else "FP64"


def compare_values(X, ev, free, where):
    assert X.dtype == ev.dtype, (where, X.dtype, ev.dtype)
    if ev.dtype.kind == "f":
        same_fp(X, ev, free, where)
    else:
        assert X.tolist() == ev.tolist(), where


def assert_product(C, rows, cols, vals, free, where):
    """A library Matrix against the COO tuples of the expectation, in any order."""
    I, J, X = C.to_coo()
    order = np.lexsort((cols, rows))
    assert I.tolist() == rows[order].tolist() and J.tolist() == cols[order].tolist(), where
    compare_values(X, vals[order], free, where)


def from_lengths(gb, rng, deg, n=None, tname="INT64"):
    """A matrix whose row i holds deg[i] entries at sorted random columns; values 1 .. 9."""
    deg = np.asarray(deg)
    n = int(max(deg.max(), 1)) + 2 if n is None else n
    rows = np.repeat(np.arange(deg.size), deg)
    cols = np.concatenate([np.sort(rng.choice(n, d, replace=False)) for d in deg]) if deg.sum() else np.zeros(0, np.int64)
    vals = rng.integers(1, 10, rows.size).astype(NP_OF[tname])
    A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=deg.size, ncols=n)
    return A, (rows, cols, vals)


# ---- 1. the reference's literal ------------------------------------------------------------------------------------------------------
def test_literals(gb, literals):
    from graphblas_amd import _lib

    L = _lib.lib
    a, b = literals["A"], literals["B"]
    A = gb.Matrix.from_coo(a["rows"], a["cols"], a["vals"], nrows=a["nrows"], ncols=a["ncols"])
    B = gb.Matrix.from_coo(b["rows"], b["cols"], b["vals"], nrows=b["nrows"], ncols=b["ncols"])
    for case in literals["cases"]:
        op = case["op"]
        forms = [A.kronecker(B, getattr(gb.binary, op)), A.kronecker(B, "*"), A.kronecker(B, op), A.kronecker(B, getattr(gb.monoid, op)),
                 A.kronecker(B)]
        for k, expr in enumerate(forms):
            assert expr.shape == (case["nrows"], case["ncols"])
            C = expr.new()
            assert C.shape == (case["nrows"], case["ncols"]) and C.dtype.name == "INT64", (k, C.shape, C.dtype)
            assert_coo(C, case["rows"], case["cols"], case["vals"], (case["source"], k))
            assert stats(gb)["method"] == FULL and stats(gb)["out_nvals"] == len(case["rows"])
        for fn, handle in (("GrB_Matrix_kronecker_BinaryOp", "GrB_TIMES_INT64"), ("GrB_Matrix_kronecker_Monoid", "GrB_TIMES_MONOID_INT64"),
                           ("GrB_Matrix_kronecker_Semiring", "GrB_PLUS_TIMES_SEMIRING_INT64")):  # (the semiring's multiply operator)
            C = gb.Matrix(int, case["nrows"], case["ncols"])
            assert getattr(L, fn)(C._carg, None, None, _handle(L, handle), A._carg, B._carg, None) == 0, fn
            assert_coo(C, case["rows"], case["cols"], case["vals"], (case["source"], fn))
    calls = []
    gb.record_calls(calls)
    try:
        A.kronecker(B, gb.binary.times).new()
        A.T.kronecker(B.T, gb.monoid.times).new()
    finally:
        gb.record_calls(None)
    names = [c.split("(")[0] for c in calls if "kronecker" in c]
    assert names == ["GrB_Matrix_kronecker_BinaryOp", "GrB_Matrix_kronecker_Monoid"], calls
    assert any("GrB_DESC_T0T1" in c for c in calls if "_Monoid" in c), calls


# ---- 2. seeded random parity against numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(22))
def test_kronecker_random(gb, seed):
    """All nine operators per seed over rectangular operands; the 11 types in turn, every other seed with a second operand of another
    type (the cast pass); A.T, B.T and both; an output type that differs from the operator's; mask in {none, value, structural} x
    complement x replace; accum in {none, plus}."""
    rng = np.random.default_rng(4400 + seed)
    ta = ALL_TYPES[seed % 11]
    tb = ALL_TYPES[(3 * seed + 1) % 11] if seed % 2 else ta
    ma, na, mb, nb = (int(rng.integers(1, 9)) for _ in range(4))
    if seed % 5 == 0:
        ma, nb = 1, 1
    a = draw_operand(rng, ma, na, ta, 0.5)
    b = draw_operand(rng, mb, nb, tb, 0.6)
    A = gb.Matrix.from_coo(*a, dtype=ta, nrows=ma, ncols=na)
    B = gb.Matrix.from_coo(*b, dtype=tb, nrows=mb, ncols=nb)
    for oi, op in enumerate(OPS):
        cfg = seed * len(OPS) + oi
        at, bt = (cfg // 2) % 2 == 1, (cfg // 4) % 2 == 1
        mask_kind = cfg % 3
        comp, repl = (cfg // 3) % 2 == 1, (cfg // 6) % 2 == 1
        accum = "plus" if (cfg // 5) % 2 else None
        ea, (ema, ena) = ((a[1], a[0], a[2]), (na, ma)) if at else (a, (ma, na))
        eb, (emb, enb) = ((b[1], b[0], b[2]), (nb, mb)) if bt else (b, (mb, nb))
        tr, tc, tv, free = np_kron(op, ea, eb, emb, enb)
        ttype = NAME_OF[tv.dtype]
        ctype = wider(ttype) if cfg % 4 == 1 else ttype
        om, on = ema * emb, ena * enb
        with np.errstate(all="ignore"):
            T = (tr, tc, tv.astype(NP_OF[ctype]))
        Cc = draw_coo(rng, om, on, ctype, 0.3) if (accum or mask_kind) else None
        if Cc is not None and not ctype.startswith("FP") and ctype != "BOOL":
            Cc = (Cc[0], Cc[1], draw_vals(rng, Cc[0].size, ctype))
        C = gb.Matrix.from_coo(*Cc, dtype=ctype, nrows=om, ncols=on) if Cc is not None else gb.Matrix(ctype, om, on)
        Mc, kw = None, {}
        if mask_kind:
            Mc = draw_coo(rng, om, on, "INT8", 0.5)
            M = gb.Matrix.from_coo(*Mc, dtype="INT8", nrows=om, ncols=on)
            mm = M.S if mask_kind == 2 else M.V
            kw = dict(mask=~mm if comp else mm, replace=repl)
        if accum:
            kw["accum"] = accum
        expr = (A.T if at else A).kronecker(B.T if bt else B, getattr(gb.binary, op))
        assert expr.dtype.name == ttype and expr.shape == (om, on), (op, expr.dtype, ttype)
        C(**kw) << expr
        er, ec, ev = np_write_rule((om, on), ctype, Cc, T, Mc, mask_kind == 2, comp and mask_kind > 0, repl and mask_kind > 0, accum)
        where = f"seed {seed} {op} {ta} x {tb} -> {ttype} -> {ctype} at={at} bt={bt} mask={mask_kind} comp={comp} repl={repl} accum={accum}"
        I, J, X = C.to_coo()
        assert I.tolist() == er.tolist() and J.tolist() == ec.tolist(), where
        compare_values(X, ev, free, where)


# ---- 3. the write rule, one grid ------------------------------------------------------------------------------------------------------
def test_write_rule_grid(gb):
    """No mask, structural, valued and complemented masks x replace x accum in {none, plus}, C non-empty beforehand; and the complement
    of no mask (C ABI: GrB_DESC_C keeps C, GrB_DESC_RC empties it)."""
    from graphblas_amd import _lib

    L = _lib.lib
    rng = np.random.default_rng(31)
    a, b = draw_operand(rng, 3, 4, "INT64", 0.6), draw_operand(rng, 4, 3, "INT64", 0.6)
    A = gb.Matrix.from_coo(*a, dtype="INT64", nrows=3, ncols=4)
    B = gb.Matrix.from_coo(*b, dtype="INT64", nrows=4, ncols=3)
    tr, tc, tv, _ = np_kron("times", a, b, 4, 3)
    Cc = draw_coo(rng, 12, 12, "INT64", 0.4)
    Mc = draw_coo(rng, 12, 12, "INT8", 0.5)
    M = gb.Matrix.from_coo(*Mc, dtype="INT8", nrows=12, ncols=12)
    assert (Mc[2] == 0).any() and (Mc[2] != 0).any()
    for mask_kind in (0, 1, 2):
        for comp in ((False,) if mask_kind == 0 else (False, True)):
            for repl in ((False,) if mask_kind == 0 else (False, True)):
                for accum in (None, "plus"):
                    C = gb.Matrix.from_coo(*Cc, dtype="INT64", nrows=12, ncols=12)
                    kw = {}
                    if mask_kind:
                        mm = M.S if mask_kind == 2 else M.V
                        kw = dict(mask=~mm if comp else mm, replace=repl)
                    if accum:
                        kw["accum"] = accum
                    C(**kw) << A.kronecker(B)
                    er, ec, ev = np_write_rule((12, 12), "INT64", Cc, (tr, tc, tv), Mc if mask_kind else None, mask_kind == 2, comp, repl, accum)
                    where = f"mask={mask_kind} comp={comp} repl={repl} accum={accum}"
                    I, J, X = C.to_coo()
                    assert I.tolist() == er.tolist() and J.tolist() == ec.tolist() and X.tolist() == ev.tolist(), where
                    assert stats(gb)["out_nvals"] == er.size, where
    times = _handle(L, "GrB_TIMES_INT64")
    C = gb.Matrix.from_coo(*Cc, dtype="INT64", nrows=12, ncols=12)
    assert L.GrB_Matrix_kronecker_BinaryOp(C._carg, None, None, times, A._carg, B._carg, _handle(L, "GrB_DESC_C")) == 0
    assert_coo(C, *Cc, "complemented absent mask")
    assert L.GrB_Matrix_kronecker_BinaryOp(C._carg, None, None, times, A._carg, B._carg, _handle(L, "GrB_DESC_RC")) == 0
    assert C.nvals == 0


# ---- 4. the fill kernel at its limits -------------------------------------------------------------------------------------------------
# (row lengths of A, row lengths of B): nnz(T) = sum(A) * sum(B); row ia * mb + ib of T holds A[ia] * B[ib] entries
LIMITS = {
    **{f"nnz(T) = {n}: A is 1 x 1": ([1], [n // 3, 0, n - n // 3]) for n in (63, 64, 65, UNIT - 1, UNIT, UNIT + 1, 2 * UNIT - 1, 2 * UNIT + 1)},
    "rows of T of 0 / 1 / 63 / 64 / 65 entries as 7 * 9, 8 * 8, 5 * 13": ([8, 7, 5, 0, 1], [8, 9, 13, 0, 1]),
    "row ends on the last (64, 128, 192, 256) and the first (65, 193) lane of a block": ([1, 1], [64, 1, 63]),
    "one row of T over 4 units, lenB = 40: several A entries inside one block": ([40], [40]),
    "one row of T over 118 units, lenB = 200: one A entry covers several blocks": ([300], [200]),
    **{f"quotient / remainder with lenB = {n}": ([5, 2], [n]) for n in (1, 3, 63, 64, 65, 1000)},
    "65 consecutive empty rows of T inside a unit (empty rows of B)": ([2], [3] + [0] * 65 + [2]),
    "130 consecutive empty rows of T inside a unit (empty rows of B)": ([2, 1], [3] + [0] * 130 + [2]),
    "an empty row of A, mb = 1": ([2, 0, 3], [2]),
    "an empty row of A, mb = 64: 64 empty rows of T": ([2, 0, 3], [1] * 64),
    "an empty row of A, mb = 65: 65 empty rows of T": ([2, 0, 3], [1] * 65),
    "empty first and last rows": ([0, 3, 0], [0, 2, 1, 0]),
    "many short rows across units": ([3, 0, 1] * 20, [2, 1, 0, 4] * 6),
}


@pytest.mark.parametrize("name", list(LIMITS))
def test_fill_kernel_limits(gb, name):
    """Each case names the limit it hits; the unit is 8 blocks of 64 entries of T."""
    dega, degb = LIMITS[name]
    rng = np.random.default_rng(len(name))
    A, a = from_lengths(gb, rng, dega)
    B, b = from_lengths(gb, rng, degb)
    nnz = int(np.sum(dega)) * int(np.sum(degb))
    C = A.kronecker(B, gb.binary.times).new()
    st = stats(gb)
    assert st["method"] == FULL and st["tiles"] == units_of(nnz) and st["out_nvals"] == nnz, (name, st)
    tr, tc, tv, _ = np_kron("times", a, b, B.nrows, B.ncols)
    assert_product(C, tr, tc, tv, None, name)
    Cp = C.to_csr()[0]
    assert np.diff(np.asarray(Cp).astype(np.int64)).tolist() == np.outer(dega, degb).ravel().tolist(), name
    if nnz <= 4096:  # a comparison (BOOL out) and the structure-only fill over the same seams
        G = A.kronecker(B, gb.binary.gt).new()
        gr, gc, gv, _ = np_kron("gt", a, b, B.nrows, B.ncols)
        assert_product(G, gr, gc, gv, None, name + " gt")
        P = A.kronecker(B, gb.binary.pair).new()
        assert stats(gb)["method"] == 6 and stats(gb)["tiles"] == units_of(nnz) and stored_iso(P)
        assert_product(P, tr, tc, np.ones(nnz, np.int64), None, name + " pair")


@pytest.mark.parametrize("shapes", [((1, 5), (4, 3)), ((5, 1), (4, 3)), ((4, 3), (1, 5)), ((4, 3), (5, 1)), ((1, 1), (6, 7)), ((6, 7), (1, 1)),
                                    ((1, 1), (1, 1)), ((1, 6), (6, 1))])
def test_unit_dimensions(gb, shapes):
    """ma = 1, mb = 1, na = 1, nb = 1, and 1 x 1 against anything."""
    (ma, na), (mb, nb) = shapes
    rng = np.random.default_rng(ma * 1000 + na * 100 + mb * 10 + nb)
    a, b = draw_operand(rng, ma, na, "INT32", 0.8), draw_operand(rng, mb, nb, "INT32", 0.8)
    if a[0].size == 0:
        a = (np.array([0]), np.array([0]), np.array([3], np.int32))
    if b[0].size == 0:
        b = (np.array([0]), np.array([0]), np.array([4], np.int32))
    A = gb.Matrix.from_coo(*a, dtype="INT32", nrows=ma, ncols=na)
    B = gb.Matrix.from_coo(*b, dtype="INT32", nrows=mb, ncols=nb)
    for op in ("times", "second"):
        C = A.kronecker(B, op).new()
        assert C.shape == (ma * mb, na * nb) and stats(gb)["method"] == FULL
        tr, tc, tv, _ = np_kron(op, a, b, mb, nb)
        assert_product(C, tr, tc, tv, None, (shapes, op))


def test_int32_column_edge(gb):
    """Columns at the int32 edge, computed in 64 bits: A 2 x 65536 with an entry at column 65535, B 2 x 32767 with one at column 32766
    give column 65535 * 32767 + 32766 = 2 147 418 111 of 2 147 418 112; B 2 x 32768 needs 2^31 columns: GrB_NOT_IMPLEMENTED, C unchanged."""
    a = (np.array([0, 1, 1]), np.array([3, 2, 65535]), np.array([2, 3, 5]))
    b = (np.array([0, 1, 1]), np.array([5, 0, 32766]), np.array([7, 1, 4]))
    A = gb.Matrix.from_coo(*a, nrows=2, ncols=65536)
    B = gb.Matrix.from_coo(*b, nrows=2, ncols=32767)
    C = A.kronecker(B).new()
    assert C.shape == (4, 65536 * 32767)
    tr, tc, tv, _ = np_kron("times", a, b, 2, 32767)
    assert int(tc.max()) == 2147418111
    assert_product(C, tr, tc, tv, None, "int32 edge")
    B2 = gb.Matrix.from_coo(*b, nrows=2, ncols=32768)
    C2 = gb.Matrix(int, 4, 65536 * 32768)
    with pytest.raises(gb.exceptions.NotImplementedException, match="int32 column indices"):
        C2 << A.kronecker(B2)
    assert C2.nvals == 0
    E = gb.Matrix(int, 2, 32768)
    C2 << A.kronecker(E)  # (nothing to index: an empty product of any width)
    assert C2.nvals == 0 and stats(gb)["method"] == 6


# ---- 5. the short cuts ----------------------------------------------------------------------------------------------------------------
def iso_matrix(gb, coo, m, n, value, tname="INT64"):
    r, c = coo[0], coo[1]
    order = np.lexsort((c, r))
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=m))])
    A = gb.Matrix.ss.import_csr(nrows=m, ncols=n, indptr=indptr, values=np.array([value], NP_OF[tname]), col_indices=c[order], is_iso=True,
                                sorted_cols=True, dtype=tname)
    assert stored_iso(A)
    return A


def test_short_cuts(gb):
    rng = np.random.default_rng(77)
    a, b = draw_operand(rng, 5, 6, "INT64", 0.5), draw_operand(rng, 4, 7, "INT64", 0.5)
    A = gb.Matrix.from_coo(*a, nrows=5, ncols=6)
    B = gb.Matrix.from_coo(*b, nrows=4, ncols=7)
    Ai, Bi = iso_matrix(gb, a, 5, 6, 3), iso_matrix(gb, b, 4, 7, -2)
    ai, bi = (a[0], a[1], np.full(a[0].size, 3)), (b[0], b[1], np.full(b[0].size, -2))
    nnz = a[0].size * b[0].size
    # empty operands: nothing is launched
    for X, Y in ((gb.Matrix(int, 5, 6), B), (A, gb.Matrix(int, 4, 7)), (gb.Matrix(int, 5, 6), gb.Matrix(int, 4, 7))):
        E = X.kronecker(Y).new()
        st = stats(gb)
        assert E.nvals == 0 and E.shape == (20, 42) and st["method"] == 6 and st["kernel_launches"] == 0 and st["out_nvals"] == 0, st
    # an empty product under replace still clears what the mask allows
    C = gb.Matrix.from_coo([0, 19], [0, 41], [1, 2], nrows=20, ncols=42)
    Mk = gb.Matrix.from_coo([0], [0], [1], nrows=20, ncols=42)
    C(Mk.S, replace=True) << A.kronecker(gb.Matrix(int, 4, 7))
    assert C.nvals == 0
    # iso products: one value computed on the host, the structure-only fill
    # (ANY may return either operand of a pair: the library returns the first, so it is iso with an iso A)
    for X, xa, Y, yb, op in ((Ai, ai, Bi, bi, "times"), (Ai, ai, Bi, bi, "gt"), (A, a, B, b, "pair"), (Ai, ai, B, b, "any"), (Ai, ai, B, b, "first"),
                             (A, a, Bi, bi, "second"), (Ai, ai, Bi, bi, "min")):
        C = X.kronecker(Y, getattr(gb.binary, op)).new()
        st = stats(gb)
        assert stored_iso(C) and st["method"] == 6 and st["out_nvals"] == nnz and st["tiles"] == units_of(nnz), (op, st)
        tr, tc, tv, free = np_kron(op, xa, yb, 4, 7)
        assert_product(C, tr, tc, tv, free, op)
    # FIRST and ANY of a non-iso A are the full path; so is SECOND of a non-iso B
    for X, xa, Y, yb, op in ((A, a, Bi, bi, "first"), (A, a, Bi, bi, "any"), (Ai, ai, B, b, "second"), (Ai, ai, B, b, "times")):
        C = X.kronecker(Y, getattr(gb.binary, op)).new()
        assert not stored_iso(C) and stats(gb)["method"] == FULL, op
        assert_product(C, *np_kron(op, xa, yb, 4, 7), op)
    # an iso result under a valued mask with an accumulator: the expansion runs, one value per entry again
    Cc = draw_coo(rng, 20, 42, "INT64", 0.3)
    Mc = draw_coo(rng, 20, 42, "INT8", 0.5)
    C = gb.Matrix.from_coo(*Cc, dtype="INT64", nrows=20, ncols=42)
    M = gb.Matrix.from_coo(*Mc, dtype="INT8", nrows=20, ncols=42)
    C(M.V, gb.binary.plus) << Ai.kronecker(Bi, gb.binary.times)
    assert stats(gb)["method"] == 6
    tr, tc, tv, _ = np_kron("times", ai, bi, 4, 7)
    er, ec, ev = np_write_rule((20, 42), "INT64", Cc, (tr, tc, tv), Mc, False, False, False, "plus")
    I, J, X = C.to_coo()
    assert I.tolist() == er.tolist() and J.tolist() == ec.tolist() and X.tolist() == ev.tolist()
    assert not stored_iso(C)
    # an iso product into another type keeps one value
    F = Ai.kronecker(Bi, gb.binary.times).new(dtype="FP32")
    assert stored_iso(F) and F.dtype.name == "FP32" and set(F.to_coo()[2].tolist()) == {-6.0}


# ---- 6. properties, independent of the numpy restatement ---------------------------------------------------------------------------------
def test_properties(gb):
    rng = np.random.default_rng(8)
    a, b, c = draw_operand(rng, 3, 4, "INT64", 0.6), draw_operand(rng, 4, 2, "INT64", 0.7), draw_operand(rng, 2, 5, "INT64", 0.6)
    A = gb.Matrix.from_coo(*a, nrows=3, ncols=4)
    B = gb.Matrix.from_coo(*b, nrows=4, ncols=2)
    Cm = gb.Matrix.from_coo(*c, nrows=2, ncols=5)
    # associativity
    left = A.kronecker(B).new().kronecker(Cm).new()
    right = A.kronecker(B.kronecker(Cm).new()).new()
    assert left.shape == right.shape == (24, 40) and left.nvals == a[0].size * b[0].size * c[0].size
    assert left.isequal(right, check_dtype=True)
    # kron(I_k, B): k diagonal copies of B
    k = 5
    Ik = gb.Matrix.from_coo(np.arange(k), np.arange(k), np.ones(k, np.int64), nrows=k, ncols=k)
    D = Ik.kronecker(B).new()
    assert_coo(D, np.concatenate([b[0] + 4 * i for i in range(k)]), np.concatenate([b[1] + 2 * i for i in range(k)]), np.tile(b[2], k), "kron(I, B)")
    # kron(A, ones): every entry of A becomes a block
    ones = gb.Matrix.from_coo([0, 0, 1, 1], [0, 1, 0, 1], [1, 1, 1, 1], nrows=2, ncols=2)
    Bl = A.kronecker(ones).new()
    dense = np.zeros((3, 4), np.int64)
    dense[a[0], a[1]] = a[2]
    has = np.zeros((3, 4), bool)
    has[a[0], a[1]] = True
    br, bc = np.nonzero(np.repeat(np.repeat(has, 2, 0), 2, 1))
    assert_coo(Bl, br, bc, np.repeat(np.repeat(dense, 2, 0), 2, 1)[br, bc], "kron(A, ones)")
    # kron(A, [[1]]) == A
    one = gb.Matrix.from_coo([0], [0], [1], nrows=1, ncols=1)
    assert A.kronecker(one).new().isequal(A, check_dtype=True) and one.kronecker(A).new().isequal(A, check_dtype=True)
    # a 2 x 2 seed raised four times: entry (i, j) is the product of seed[bit of i, bit of j] over the four bit positions
    seed = {(0, 0): 1, (0, 1): 2, (1, 0): 3}
    K = gb.Matrix.from_coo([0, 0, 1], [0, 1, 0], [1, 2, 3], nrows=2, ncols=2)
    P = K
    for _ in range(3):
        P = P.kronecker(K).new()
    er, ec, ev = [], [], []
    for i in range(16):
        for j in range(16):
            pairs = [((i >> s) & 1, (j >> s) & 1) for s in range(4)]
            if all(p in seed for p in pairs):
                er.append(i), ec.append(j), ev.append(int(np.prod([seed[p] for p in pairs])))
    assert P.shape == (16, 16) and P.nvals == 81
    assert_coo(P, er, ec, ev, "seed^4")
    # scipy.sparse.kron on FP64 times
    try:
        import scipy.sparse as sp
    except ImportError:
        return
    fa, fb = draw_operand(rng, 6, 5, "INT64", 0.5), draw_operand(rng, 3, 7, "INT64", 0.5)
    fa, fb = (fa[0], fa[1], fa[2].astype(np.float64) + 0.5), (fb[0], fb[1], fb[2].astype(np.float64) - 0.25)
    FA = gb.Matrix.from_coo(*fa, dtype="FP64", nrows=6, ncols=5)
    FB = gb.Matrix.from_coo(*fb, dtype="FP64", nrows=3, ncols=7)
    S = sp.kron(sp.coo_matrix((fa[2], (fa[0], fa[1])), shape=(6, 5)), sp.coo_matrix((fb[2], (fb[0], fb[1])), shape=(3, 7)), format="coo")
    keep = np.ones(S.nnz, bool)  # (scipy keeps explicit zeros of a product as entries: so does GraphBLAS)
    assert_product(FA.kronecker(FB).new(), S.row[keep].astype(np.int64), S.col[keep].astype(np.int64), S.data[keep], None, "scipy")


# ---- 7. aliasing ----------------------------------------------------------------------------------------------------------------------
def test_aliasing(gb):
    rng = np.random.default_rng(12)
    a = draw_operand(rng, 6, 9, "INT64", 0.5)
    A = gb.Matrix.from_coo(*a, nrows=6, ncols=9)
    one = gb.Matrix.from_coo([0], [0], [1], nrows=1, ncols=1)
    three = gb.Matrix.from_coo([0], [0], [3], nrows=1, ncols=1)
    assert_coo(A.T.kronecker(one).new(), a[1], a[0], a[2], "the transpose, now cached")
    A << A.kronecker(three)  # C is the first operand
    assert_coo(A, a[0], a[1], a[2] * 3, "A << A (x) [[3]]")
    assert_coo(A.T.kronecker(one).new(), a[1], a[0], a[2] * 3, "the cached transpose was rebuilt")
    A << three.kronecker(A)  # C is the second operand
    assert_coo(A, a[0], a[1], a[2] * 9, "A << [[3]] (x) A")
    assert_coo(A.T.kronecker(one).new(), a[1], a[0], a[2] * 9, "the cached transpose was rebuilt again")
    A(gb.binary.plus) << A.kronecker(one)
    assert_coo(A, a[0], a[1], a[2] * 18, "accumulating into an operand")
    # one matrix as both operands
    b = draw_operand(rng, 4, 5, "INT64", 0.6)
    B = gb.Matrix.from_coo(*b, nrows=4, ncols=5)
    assert_product(B.kronecker(B).new(), *np_kron("times", b, b, 4, 5), "B (x) B")
    assert_product(B.kronecker(B.T, "plus").new(), *np_kron("plus", b, (b[1], b[0], b[2]), 5, 4), "B (x) B'")
    three << three.kronecker(three)  # C is both operands
    assert_coo(three, [0], [0], [9], "O << O (x) O")


# ---- 8. the C ABI and the errors -------------------------------------------------------------------------------------------------------
def test_c_abi_errors(gb, literals):
    from graphblas_amd import _lib

    L = _lib.lib
    a, b = literals["A"], literals["B"]
    A = gb.Matrix.from_coo(a["rows"], a["cols"], a["vals"], nrows=2, ncols=2)
    B = gb.Matrix.from_coo(b["rows"], b["cols"], b["vals"], nrows=2, ncols=3)
    keep = ([0, 3], [5, 1], [11, 12])
    times = _handle(L, "GrB_TIMES_INT64")
    fns = ("GrB_Matrix_kronecker_BinaryOp", "GrB_Matrix_kronecker_Monoid", "GrB_Matrix_kronecker_Semiring")
    C = gb.Matrix.from_coo(*keep, nrows=4, ncols=6)
    for fn in fns:  # NULL operator, output and operands
        assert getattr(L, fn)(C._carg, None, None, None, A._carg, B._carg, None) == -2, fn  # GrB_NULL_POINTER
    assert L.GrB_Matrix_kronecker_BinaryOp(None, None, None, times, A._carg, B._carg, None) == -2
    assert L.GrB_Matrix_kronecker_BinaryOp(C._carg, None, None, times, None, B._carg, None) == -2
    assert L.GrB_Matrix_kronecker_BinaryOp(C._carg, None, None, times, A._carg, None, None) == -2
    # a wrong output shape: both shapes in the text
    W = gb.Matrix.from_coo([1], [2], [7], nrows=6, ncols=4)
    assert L.GrB_Matrix_kronecker_BinaryOp(W._carg, None, None, times, A._carg, B._carg, None) == -6  # GrB_DIMENSION_MISMATCH
    assert "6 x 4" in _matrix_error(L, W) and "4 x 6" in _matrix_error(L, W), _matrix_error(L, W)
    assert L.GrB_Matrix_kronecker_BinaryOp(W._carg, None, None, times, A._carg, B._carg, _handle(L, "GrB_DESC_T0")) == -6
    assert L.GrB_Matrix_kronecker_BinaryOp(C._carg, None, None, times, A._carg, B._carg, _handle(L, "GrB_DESC_T1")) == -6
    assert "4 x 6" in _matrix_error(L, C) and "6 x 4" in _matrix_error(L, C), _matrix_error(L, C)
    assert L.GrB_Matrix_kronecker_BinaryOp(W._carg, None, None, times, A._carg, B._carg, _handle(L, "GrB_DESC_T0T1")) == 0
    lit = literals["cases"][0]
    ar, ac = np.asarray(a["cols"]), np.asarray(a["rows"])  # A', B'
    tr, tc, tv, _ = np_kron("times", (ar, ac, np.asarray(a["vals"])), (np.asarray(b["cols"]), np.asarray(b["rows"]), np.asarray(b["vals"])), 3, 2)
    assert_product(W, tr, tc, tv, None, "T0T1")
    assert_coo(W.T.new(), lit["rows"], lit["cols"], lit["vals"], "(A' (x) B')' = A (x) B")
    # a mask of the wrong shape; a comparison as accumulator; a handle-only operator: C is unchanged every time
    with pytest.raises(gb.exceptions.DimensionMismatch):
        C(W.S) << A.kronecker(B)
    assert L.GrB_Matrix_kronecker_BinaryOp(C._carg, W._carg, None, times, A._carg, B._carg, None) == -6
    assert "mask" in _matrix_error(L, C)
    assert L.GrB_Matrix_kronecker_BinaryOp(C._carg, None, _handle(L, "GrB_EQ_INT64"), times, A._carg, B._carg, None) == -5  # GrB_DOMAIN_MISMATCH
    F = gb.Matrix.from_coo([2], [2], [0.5], dtype="FP64", nrows=4, ncols=6)
    assert L.GrB_Matrix_kronecker_BinaryOp(F._carg, None, None, _handle(L, "GrB_DIV_FP64"), A._carg, B._carg, None) == -8  # GrB_NOT_IMPLEMENTED
    assert "not implemented" in _matrix_error(L, F)
    assert_coo(F, [2], [2], [0.5], "C unchanged after GrB_DIV")
    assert L.GrB_Matrix_kronecker_BinaryOp(F._carg, None, None, _handle(L, "GrB_DIV_FP64"), A._carg, B._carg, _handle(L, "GrB_DESC_RC")) == -8
    assert_coo(F, [2], [2], [0.5], "C unchanged after GrB_DIV under a complemented absent mask with replace")
    assert_coo(C, *keep, "C unchanged after every failure")
    with pytest.raises(gb.exceptions.DimensionMismatch):
        gb.Matrix(int, 6, 4) << A.kronecker(B)
    # the host's own errors
    with pytest.raises(TypeError, match="Expected type: BinaryOp, Monoid"):  # reference core/matrix.py:2362-2363
        A.kronecker(B, gb.semiring.plus_times)
    with pytest.raises(TypeError, match="Expected type: Matrix"):
        A.kronecker(gb.Vector(int, 3))
    with pytest.raises(TypeError):
        A.kronecker(3)
    with pytest.raises(TypeError):
        A.T.kronecker(B, gb.semiring.min_plus)


# ---- 9. no growth ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_growth():
    """50 products per cycle (the value fill with and without a cast pass, an iso product, a comparison; with and without a mask) on one
    pair of operands, results freed.  The library keeps freed blocks in its size-class cache, so the first cycle may grow; free device
    memory after cycle 2 against after cycle 3."""
    import torch

    gb = bind("gpu")
    rng = np.random.default_rng(3)
    a = draw_operand(rng, 40, 40, "FP32", 0.25)
    A = gb.Matrix.from_coo(*a, dtype="FP32", nrows=40, ncols=40)
    Bi = gb.Matrix.from_coo(a[0], a[1], np.arange(a[0].size) % 7, dtype="INT64", nrows=40, ncols=40)
    K = A.kronecker(A).new()
    assert K.nvals == A.nvals ** 2 <= 200_000 and stats(gb)["method"] == FULL
    M = K.select("triu", 1).new()

    def free_bytes():
        gb.Matrix(int, 1, 1).wait()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        for k in range(13):
            for expr, mask in ((A.kronecker(A, "times"), None), (A.kronecker(Bi, "plus"), M.S), (A.T.kronecker(A, "pair"), M.V), (Bi.kronecker(A, ">"), None)):
                r = expr.new(mask=mask) if mask is not None else expr.new()
                del r

    cycle()
    cycle()
    after2 = free_bytes()
    cycle()
    after3 = free_bytes()
    print(f"free after cycle 2: {after2 / 2**20:.1f} MiB, after cycle 3: {after3 / 2**20:.1f} MiB")
    assert after3 >= after2, (after2, after3)
