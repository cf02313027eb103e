"""The typecast chain of the matrix operations: WHICH (from, to) pairs an operation hands to the cast, in which order, over lossy type
triples (source type, operator type, output type) -- float -> narrow integer saturates (NaN -> 0), integer -> integer wraps, anything ->
BOOL is x != 0.  The cast itself is tests/test_object_layer.py::test_dup_dtype_casts_like_the_oracle; here a skipped, swapped or doubled
hop shows.  (The operation suites -- test_select.py, test_matrix_ewise.py, test_apply.py, test_kronecker.py -- take their "other type"
from tables that numpy's astype casts like the library does, no float -> integer: the lossy pairs are here.)

The expectation is numpy plus ``O.cast``, one explicit call per hop (``chain``), compared bit for bit; it never comes from the library.
``O.cast`` is the authority because test_oracle_cast_follows_the_rule checks it against the rule of grb_ops.hpp (cast_value) in plain
Python first, and test_lossy_triples_are_distinguishable shows that for every lossy triple the value set tells the right chain from the
direct cast (both run without the library).

The chains, as read from the sources (s = the type of an operand, ot = the operator's type, tt = BOOL for a comparison else ot, ct = C's
type):

  select     predicate on (ot) a against (ot) thunk; a kept value goes s -> ct directly (grb_select.hip: values move in S's type,
             matrix_adopt(stype -> ctype)); a positional operator takes k = (INT64) thunk, saturated
  apply      op((ot) a, (ot) scalar) -> tt -> ct; ROWINDEX / COLINDEX / DIAGINDEX: int64 arithmetic that wraps, -> the operator's INT32 /
             INT64 -> ct; SECOND, PAIR, ANY and an iso A compute one value on the host (apply_values)
  eWiseMult  op((ot) a, (ot) b) -> tt -> ct
  eWiseAdd   the same where both hold an entry; an entry of one operand alone goes s -> ot -> tt -> ct, also when the other operand is
             empty (ewise_pass_through)
  kronecker  as eWiseMult; an iso T is one value computed on the host (kron_one_value)
  extract    s -> ct directly (a matrix, a row, a column, one element)
  assign     source -> ct, then the accumulator in ct on (ct) t
  mxm        operands -> the semiring's type, the fold in it, -> ct
  every one  the accumulator runs in ct on the already-cast t; a value mask is true where its value != 0 (NaN, a subnormal, 0.5 and -1
             are true, -0.0 is false)

ANY may return either operand: apply returns the bound scalar, kronecker the first operand, and the expectation says so.  IEEE leaves
min(-0, +0) open, so min / max results are compared with a zero matching a zero of either sign (tests/values.py).
"""
import ctypes
import math

import numpy as np
import pytest

from oracle import grb_oracle as O
from tests.backend import DEVICES, bind
from tests.test_select import np_keep, np_write_rule, stored_iso
from tests.values import same_fp

NP_OF = O.NP_OF
ALL_TYPES = ["BOOL", "INT8", "INT16", "INT32", "INT64", "UINT8", "UINT16", "UINT32", "UINT64", "FP32", "FP64"]
SOURCES = ["FP64", "FP32", "INT64", "UINT64", "INT8", "BOOL"]
OP_TYPES = ["INT8", "UINT16", "INT32", "UINT64", "BOOL", "FP32"]
OP_TYPES_ISO = ["INT8", "UINT16", "BOOL", "FP32"]  # the operator-type axis of the iso repeats (one matrix per value: the larger cross)
CMP = ["eq", "ne", "gt", "lt", "ge", "le"]
ARITH = ["plus", "minus", "times", "min", "max", "first", "second", "pair"]
VALUE = ["valueeq", "valuene", "valuegt", "valuege", "valuelt", "valuele"]
POSITIONAL = ["tril", "triu", "diag", "offdiag", "colle", "colgt", "rowle", "rowgt"]
INDEX = ["rowindex", "colindex", "diagindex"]
MASK_TYPES = ["FP64", "FP32", "INT8"]

# 3 x 70: row 0 is full (it crosses the block of 64 entries), row 1 holds every third column, row 2 three entries; 97 entries
M, N = 3, 70
ROWS = np.concatenate([np.zeros(70, np.int64), np.ones(24, np.int64), np.full(3, 2, np.int64)])
COLS = np.concatenate([np.arange(70), np.arange(0, 70, 3), [1, 68, 69]]).astype(np.int64)
NNZ = ROWS.size
INDPTR = np.array([0, 70, 94, 97], np.int64)
# the second operand of eWise: row 0 every second column, row 1 full, row 2 three entries -- entries of A alone, of B alone, of both
B_ROWS = np.concatenate([np.zeros(35, np.int64), np.ones(70, np.int64), np.full(3, 2, np.int64)])
B_COLS = np.concatenate([np.arange(0, 70, 2), np.arange(70), [0, 1, 2]]).astype(np.int64)


def source_values(tname):
    """The values of a source type.  Beyond the list of the issue: 300.5 (FP32 has no 300.7: through UINT16 into UINT8 it wraps to 44,
    directly it saturates to 255), 100.99999999 and 1e-60 (FP64: they round to 101 and to 0 in FP32), 200 and 16777217 (the 64-bit
    integers: through INT8 into a wider type, through FP32 into FP64)."""
    np_t = NP_OF[tname]
    if tname == "BOOL":
        return np.array([False, True])
    if tname.startswith("FP"):
        v = [np.nan, np.inf, -np.inf, 0.0, -0.0, 0.5, -0.5, 255.5, 300.5, -129, 127, 128, 65535, 65536, -32769, 2.0**31, 1e10, 2.0**63,
             2.0**64, 3, -7]
        if tname == "FP64":
            v += [300.7, 100.99999999, 1e-60]
        return np.array(v, np_t)
    info = np.iinfo(np_t)
    raw = [info.min, info.max, 0, 1, 2, -1, -2, info.max // 2 + 1] + ([200, 16777217] if info.bits == 64 else [])
    out = []
    for x in raw:  # (an unsigned type has no -1: it is the wrapped value, max)
        x = int(x) % (1 << info.bits)
        x -= (1 << info.bits) if x > info.max else 0
        if x not in out:
            out.append(x)
    return np.array(out, np_t)


def entry_values(tname, count=NNZ, shift=0):
    """``count`` values of a non-iso matrix: every special value occurs"""
    v = source_values(tname)
    assert count >= v.size
    return v[(np.arange(count) + shift) % v.size]


def scalars_of(tname):
    """Bound scalars / thunks in a source type."""
    np_t = NP_OF[tname]
    if tname == "BOOL":
        return [np.bool_(True), np.bool_(False)]
    if tname.startswith("FP"):
        return [np_t(255.5), np_t(0.5), np_t(1e10), np_t(np.nan), np_t(-7), np_t(300.5)]
    info = np.iinfo(np_t)
    return [np_t(info.max), np_t(1), np_t(info.max // 2 + 1), np_t(info.min), np.float64(2.5)]


def chain(x, *types):
    """x cast hop by hop with O.cast"""
    x = np.asarray(x)
    shape = x.shape
    x = x.reshape(-1)  # (O.cast takes arrays; a scalar goes as an array of one)
    for t in types:
        x = O.cast(x, t)
    return np.asarray(x).reshape(shape)


def np_op(name, ot, a, b):
    """op(a, b) element by element on operands already cast to ``ot``: values of ``ot``, BOOL for a comparison."""
    np_t = np.dtype(NP_OF[ot])
    a, b = np.broadcast_arrays(np.asarray(a), np.asarray(b))
    assert a.dtype == np_t and b.dtype == np_t, (name, ot, a.dtype, b.dtype)
    with np.errstate(all="ignore"):
        if name in CMP:
            return {"eq": a == b, "ne": a != b, "gt": a > b, "lt": a < b, "ge": a >= b, "le": a <= b}[name]
        if name in ("first", "second"):
            return (a if name == "first" else b).copy()
        if name == "pair":
            return np.ones(a.shape, np_t)
        if ot == "BOOL":
            return {"plus": a | b, "max": a | b, "lor": a | b, "times": a & b, "min": a & b, "land": a & b, "minus": a ^ b, "lxor": a ^ b,
                    "lxnor": a == b}[name]
        fl = np_t.kind == "f"
        out = {"plus": lambda: a + b, "minus": lambda: a - b, "times": lambda: a * b, "min": lambda: (np.fmin if fl else np.minimum)(a, b),
               "max": lambda: (np.fmax if fl else np.maximum)(a, b)}[name]()
        assert out.dtype == np_t
        return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_arr(a, b):
    """element-wise: equal bit patterns, NaN = NaN (so -0.0 != +0.0)"""
    assert a.dtype == b.dtype
    return (_bits(a) == _bits(b)) | ((np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else False)


def compare_values(X, ev, free, where):
    X, ev = np.asarray(X), np.asarray(ev)
    assert X.dtype == ev.dtype, (where, X.dtype, ev.dtype)
    if ev.dtype.kind == "f":
        same_fp(X, ev, free, where)
    else:
        assert X.tolist() == ev.tolist(), where


# ---- without the library: the oracle's cast against the rule, and the guard against a vacuous test -----------------------------------
def rule_cast(x, dst):
    """cast_value of grb_ops.hpp on ONE Python value (bool, int, or a float holding the source exactly): to BOOL x != 0; float ->
    integer NaN -> 0, x <= lowest -> lowest, x >= max -> max (both compared as doubles), else truncate; integer -> integer wraps; to a
    floating-point type the C conversion."""
    if dst == "BOOL":
        return bool(x != 0)
    if dst.startswith("FP"):
        with np.errstate(over="ignore"):
            return NP_OF[dst](x)
    info = np.iinfo(NP_OF[dst])
    lo, hi = int(info.min), int(info.max)
    if isinstance(x, float):
        if x != x:
            return 0
        if x <= float(lo):
            return lo
        if x >= float(hi):
            return hi
        return math.trunc(x)
    w = int(x) % (1 << info.bits)
    return w - (1 << info.bits) if w > hi else w


def cast_check_values(tname):
    v = source_values(tname)
    if tname.startswith("FP"):
        fi = np.finfo(NP_OF[tname])
        v = np.concatenate([v, np.array([fi.max, -fi.max, 2.0**31, 2.0**63, 2.0**64, -(2.0**31), -(2.0**63), 2147483520.0, 1.5, -1.5],
                                        NP_OF[tname])])
    return v


def test_oracle_cast_follows_the_rule():
    """O.cast element by element against rule_cast, every source value (and +-max, +-2^31, +-2^63, 2^64 for both floating-point
    types) into all 11 types."""
    checked = 0
    for s in ALL_TYPES:
        v = cast_check_values(s) if s in SOURCES else chain(source_values("INT64"), s)
        for d in ALL_TYPES:
            got = chain(v, d)
            assert got.dtype == np.dtype(NP_OF[d]) and got.shape == v.shape
            for x, g in zip(v.tolist(), got.tolist()):
                e = rule_cast(x, d)
                if d.startswith("FP"):
                    assert same_arr(np.array([g], NP_OF[d]), np.array([e], NP_OF[d])).all(), (s, d, x, g, e)
                else:
                    assert g == e and type(g) is type(e), (s, d, x, g, e)
                checked += 1
    assert checked > 1500


def is_lossy(s, ot):
    """the hop s -> ot loses something of a source value: it does not come back"""
    v = source_values(s)
    return not same_arr(chain(v, ot, s), v).all()


# The lossy triples whose right chain s -> ot -> ct and the direct cast s -> ct agree on EVERY value, not only on the values here:
_IDENTITY = "ct is ot: the second hop is the identity, both chains are the one cast s -> ot"
_MODULAR = "integer -> integer casts wrap, and ct is no wider than ot: both chains are x mod 2^bits(ct)"
_NONZERO = "a 64-bit integer -> FP32 keeps a non-zero value non-zero: both chains are x != 0"
NOT_DISTINGUISHABLE = {
    **{(s, t, t): _IDENTITY for s, ts in (("FP64", ["INT8", "UINT16", "INT32", "UINT64", "BOOL", "FP32"]),
                                           ("FP32", ["INT8", "UINT16", "INT32", "UINT64", "BOOL"]),
                                           ("INT64", ["INT8", "UINT16", "INT32", "BOOL", "FP32"]),
                                           ("UINT64", ["INT8", "UINT16", "INT32", "BOOL", "FP32"]),
                                           ("INT8", ["BOOL"])) for t in ts},
    **{(s, ot, ct): _MODULAR for s in ("INT64", "UINT64") for ot, cts in (("INT8", ["UINT8"]),
                                                                            ("UINT16", ["INT8", "UINT8", "INT16"]),
                                                                            ("INT32", ["INT8", "UINT8", "INT16", "UINT16", "UINT32"]))
       for ct in cts},
    ("INT64", "FP32", "BOOL"): _NONZERO,
    ("UINT64", "FP32", "BOOL"): _NONZERO,
}


def lossy_triples():
    return [(s, ot, ct) for s in SOURCES for ot in OP_TYPES if is_lossy(s, ot) for ct in ALL_TYPES]


def distinguishing(s, ot, ct):
    """the source values on which s -> ot -> ct and s -> ct differ"""
    v = source_values(s)
    return v[~same_arr(chain(v, ot, ct), chain(v, ct))]


def test_lossy_triples_are_distinguishable():
    """The guard against a vacuous test.  For every triple with a lossy middle hop, some value tells the chain through the operator's
    type (apply, eWise, kronecker, mxm; the one-hop-too-many mistake of select, extract, assign) from the direct cast (the rule of
    select, extract, assign; the skipped-hop mistake of the others).  The same inequality serves both directions."""
    lossy = lossy_triples()
    assert len(lossy) > 200
    for s in ("FP64", "FP32", "INT64"):
        for ot in ("INT8", "UINT16", "INT32", "BOOL"):
            assert is_lossy(s, ot), (s, ot)
    for tr in lossy:
        if tr in NOT_DISTINGUISHABLE:
            assert distinguishing(*tr).size == 0, ("listed as not distinguishable, but it is", tr, distinguishing(*tr))
        else:
            assert distinguishing(*tr).size > 0, ("no value tells the chains apart", tr)
    assert set(NOT_DISTINGUISHABLE) <= set(lossy)
    assert 5 * len(NOT_DISTINGUISHABLE) <= len(lossy), (len(NOT_DISTINGUISHABLE), len(lossy))
    # the examples of the issue
    assert chain(np.float64(1e10), "INT32", "INT64").item() == 2147483647 and chain(np.float64(1e10), "INT64").item() == 10**10
    assert chain(np.float64(0.5), "BOOL", "INT8").item() == 1 and chain(np.float64(0.5), "INT8").item() == 0
    assert chain(np.float64(300.7), "UINT8").item() == 255 and chain(np.float64(300.7), "UINT16", "UINT8").item() == 44


def test_counts():
    """What the operation tests below compare, for the record (``pytest -s``)."""
    lossy = lossy_triples()
    assert (len(lossy), len(NOT_DISTINGUISHABLE)) == (242, 42)
    assert sum(source_values(s).size for s in SOURCES) == 73  # iso matrices per operation
    print(f"triples per operation: {len(SOURCES) * len(OP_TYPES) * len(ALL_TYPES)} non-iso, {len(SOURCES) * len(OP_TYPES_ISO) * len(ALL_TYPES)} "
          f"per iso value; lossy {len(lossy)}, not distinguishable {len(NOT_DISTINGUISHABLE)}")


# ---- with the library ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


def stats(gb):
    from graphblas_amd import device

    return device.last_stats()


def matrix_of(gb, tname, vals, rows=ROWS, cols=COLS, shape=(M, N)):
    return gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=shape[0], ncols=shape[1])


def iso_matrix_of(gb, tname, value, indptr=INDPTR, cols=COLS, shape=(M, N)):
    A = gb.Matrix.ss.import_csr(nrows=shape[0], ncols=shape[1], indptr=indptr, values=np.array([value], NP_OF[tname]), col_indices=cols,
                                is_iso=True, sorted_cols=True, dtype=tname)
    assert stored_iso(A) and A.nvals == cols.size
    return A


def prefill(shape, ct):
    """what C holds before a masked, accumulating call"""
    r, c = np.nonzero((np.arange(shape[0])[:, None] + np.arange(shape[1])[None, :]) % 2 == 0)
    return r, c, chain(np.array([1, 2, 100, -3, 7], np.int64)[np.arange(r.size) % 5], ct)


def mask_coo(shape, mtype):
    """a value mask: NaN (true), -0.0 (false), a subnormal (true), 0.5 (true), +0.0 (false), 1 (true); INT8: -1 (true), 0, 1, -128"""
    r, c = np.nonzero((np.arange(shape[0])[:, None] * 7 + np.arange(shape[1])[None, :]) % 4 != 0)
    if mtype == "INT8":
        pool = np.array([-1, 0, 1, -128], np.int8)
    else:
        pool = np.array([np.nan, -0.0, np.finfo(NP_OF[mtype]).smallest_subnormal, 0.5, 0.0, 1.0], NP_OF[mtype])
    return r, c, pool[np.arange(r.size) % pool.size]


def finish(gb, expr, T, shape, ct, mode, where, free=None):
    """``C << expr`` (mode None) or ``C(M.V, plus) << expr`` on a C with entries (mode = the mask's type), against the dense restatement
    of the write rule (tests/test_select.py::np_write_rule) of T = (rows, cols, values ALREADY in ct)."""
    assert T[2].dtype == np.dtype(NP_OF[ct]), (where, T[2].dtype, ct)
    if mode is None:
        C = gb.Matrix(ct, *shape)
        C << expr
        er, ec, ev = np_write_rule(shape, ct, None, T, None, False, False, False, None)
    else:
        Cc, Mc = prefill(shape, ct), mask_coo(shape, mode)
        C = gb.Matrix.from_coo(*Cc, dtype=ct, nrows=shape[0], ncols=shape[1])
        Mk = gb.Matrix.from_coo(*Mc, dtype=mode, nrows=shape[0], ncols=shape[1])
        C(mask=Mk.V, accum=gb.binary.plus) << expr
        er, ec, ev = np_write_rule(shape, ct, Cc, T, Mc, False, False, False, "plus")
    I, J, X = C.to_coo()
    assert I.tolist() == er.tolist() and J.tolist() == ec.tolist(), where
    compare_values(X, ev, free, where)
    return X


def modes_for(k):
    """every call plain; every seventh under a value mask and accum=plus as well, the mask's type rotating"""
    return [None] + ([MASK_TYPES[(k // 7) % 3]] if k % 7 == 0 else [])


def free_of(op):
    return op if op in ("min", "max") else None


# ---- 1. select -------------------------------------------------------------------------------------------------------------------------
def select_T(op, ot, ct, vals, thunk, rows=ROWS, cols=COLS):
    keep = np_op(op[5:], ot, chain(vals, ot), chain(np.asarray(thunk), ot))  # the predicate in ot ...
    return rows[keep], cols[keep], chain(vals[keep], ct)  # ... the kept value s -> ct directly


@pytest.mark.parametrize("s", SOURCES)
def test_select_value(gb, s):
    vals = entry_values(s)
    A = matrix_of(gb, s, vals)
    thunks = scalars_of(s)
    k = compared = 0
    for ot in OP_TYPES:
        for ct in ALL_TYPES:
            op, thunk = VALUE[k % 6], thunks[k % len(thunks)]
            for mode in modes_for(k):
                where = f"select {s} -> {op}[{ot}] thunk {thunk!r} -> {ct} mode {mode}"
                finish(gb, A.select(getattr(gb.select, op)[ot], thunk), select_T(op, ot, ct, vals, thunk), (M, N), ct, mode, where)
            k += 1
            compared += 1
    assert compared == len(OP_TYPES) * len(ALL_TYPES)


@pytest.mark.parametrize("s", SOURCES)
def test_select_value_iso(gb, s):
    """iso A: one matrix per value; a kept iso result stays one value, cast s -> ct"""
    thunks = scalars_of(s)
    k = 0
    for vi, v in enumerate(source_values(s)):
        I = iso_matrix_of(gb, s, v)
        full = np.full(NNZ, v)
        for ot in OP_TYPES_ISO:
            for ct in ALL_TYPES:
                op, thunk = VALUE[k % 6], thunks[k % len(thunks)]
                where = f"select iso {s} {v!r} -> {op}[{ot}] thunk {thunk!r} -> {ct}"
                finish(gb, I.select(getattr(gb.select, op)[ot], thunk), select_T(op, ot, ct, full, thunk), (M, N), ct, None, where)
                k += 1
        finish(gb, I.select(gb.select.valuene[OP_TYPES_ISO[vi % 4]], thunks[0]), select_T("valuene", OP_TYPES_ISO[vi % 4], "UINT8", full, thunks[0]),
               (M, N), "UINT8", "FP32", f"select iso {s} {v!r} masked")


def test_select_kept_values_are_cast_directly(gb):
    """The examples of the issue, spelled out: 300.7 kept by a UINT16 operator reaches a UINT8 C as 255 (through UINT16 it would be
    44), 1e10 kept by an INT32 operator reaches an INT64 C as 10^10 (through INT32: 2147483647)."""
    vals = np.array([300.7, 1e10, 0.5, 7.0], np.float64)
    A = gb.Matrix.from_coo([0, 0, 1, 2], [0, 5, 5, 69], vals, dtype="FP64", nrows=M, ncols=N)
    C = A.select(gb.select.valuegt["UINT16"], np.float64(3.0)).new(dtype="UINT8")
    assert C.to_coo()[2].tolist() == [255, 255, 7]
    C = A.select(gb.select.valuege["INT32"], np.float64(300.0)).new(dtype="INT64")
    assert C.to_coo()[2].tolist() == [300, 10**10]
    C = A.select(gb.select.valueeq["BOOL"], True).new(dtype="INT8")  # 0.5 is true in BOOL, 0 in INT8
    assert C.to_coo()[2].tolist() == [127, 127, 0, 7]


@pytest.mark.parametrize("s", ["FP64", "INT8"])
def test_select_positional_thunks(gb, s):
    """Positional operators with thunks given as floating-point scalars, through GrB_Matrix_select_FP64 / _FP32 / _Scalar: the thunk
    becomes k = (INT64) thunk, saturated (1e30 -> 2^63 - 1, NaN -> 0, 2.5 -> 2), and sel_trivial / the predicate decide for that k."""
    vals = entry_values(s)
    A = matrix_of(gb, s, vals)
    u_idx = np.arange(NNZ) + 3 * (np.arange(NNZ) >= 64)
    u = gb.Vector.from_coo(u_idx, vals, dtype=s, size=100)
    calls = []
    k = 0
    for thunk in (1e30, -1e30, float("nan"), 2.5, -2.5, np.float32(1e30), np.float32(68.9), 2.0**63, -(2.0**63)):
        kk = int(chain(np.asarray(thunk), "INT64"))
        for op in POSITIONAL:
            ct = ALL_TYPES[k % 11]
            keep = np_keep(op, ROWS, COLS, None, kk)
            T = (ROWS[keep], COLS[keep], chain(vals[keep], ct))
            for form in (thunk, gb.Scalar.from_value(thunk)):
                gb.record_calls(calls)
                try:
                    finish(gb, A.select(op, form), T, (M, N), ct, None, f"select {op} thunk {thunk!r} (k = {kk}) {s} -> {ct}")
                finally:
                    gb.record_calls(None)
            # the vector form: a vector is a column, j = 0
            vkeep = np_keep(op, u_idx, np.zeros_like(u_idx), None, kk)
            w = gb.Vector(ct, 100)
            w << u.select(op, thunk)
            I, X = w.to_coo()
            assert I.tolist() == u_idx[vkeep].tolist(), (op, thunk, kk)
            compare_values(X, chain(vals[vkeep], ct), None, f"vector select {op} thunk {thunk!r} {s} -> {ct}")
            k += 1
    names = {c.split("(")[0] for c in calls if "_select_" in c}
    assert names == {"GrB_Matrix_select_FP64", "GrB_Matrix_select_FP32", "GrB_Matrix_select_Scalar"}, names


@pytest.mark.parametrize("s", SOURCES)
def test_vector_select_value(gb, s):
    vals = entry_values(s)
    idx = np.arange(NNZ) + 3 * (np.arange(NNZ) >= 64)
    u = gb.Vector.from_coo(idx, vals, dtype=s, size=100)
    thunks = scalars_of(s)
    k = 0
    for ot in OP_TYPES:
        for ct in ALL_TYPES:
            op, thunk = VALUE[k % 6], thunks[k % len(thunks)]
            keep = np_op(op[5:], ot, chain(vals, ot), chain(np.asarray(thunk), ot))
            w = gb.Vector(ct, 100)
            w << u.select(getattr(gb.select, op)[ot], thunk)
            I, X = w.to_coo()
            where = f"vector select {s} -> {op}[{ot}] thunk {thunk!r} -> {ct}"
            assert I.tolist() == idx[keep].tolist(), where
            compare_values(X, chain(vals[keep], ct), None, where)
            k += 1


# ---- 2. apply ---------------------------------------------------------------------------------------------------------------------------
def apply_T(op, side, ot, ct, vals, scalar):
    """op((ot) a, (ot) s) (the scalar bound second) / op((ot) s, (ot) a) (bound first) -> ot, BOOL for a comparison -> ct.  ANY: the scalar."""
    a, sc = chain(vals, ot), chain(np.asarray(scalar), ot)
    if op == "any":
        op = "second" if side == "right" else "first"
    t = np_op(op, ot, *((sc, a) if side == "left" else (a, sc)))
    return chain(t, ct)


def binary_ops_of(ot):
    return ARITH + ["any"] + CMP + (["lor", "land", "lxor", "lxnor"] if ot == "BOOL" else [])


@pytest.mark.parametrize("s", SOURCES)
def test_apply_bound_scalar(gb, s):
    vals = entry_values(s)
    A = matrix_of(gb, s, vals)
    scalars = scalars_of(s)
    k = 0
    for ot in OP_TYPES:
        ops = binary_ops_of(ot)
        for ct in ALL_TYPES:
            for rep in range(2):  # (two operators per triple: every operator meets every operator type)
                op, side, scalar = ops[k % len(ops)], ("right", "left")[(k // 3) % 2], scalars[k % len(scalars)]
                T = (ROWS, COLS, apply_T(op, side, ot, ct, vals, scalar))
                for mode in modes_for(k):
                    where = f"apply {s} -> {op}[{ot}] {side}={scalar!r} -> {ct} mode {mode}"
                    finish(gb, A.apply(getattr(gb.binary, op)[ot], **{side: scalar}), T, (M, N), ct, mode, where, free_of(op))
                    if mode is None and op in ("second", "pair", "any") and side == "right":
                        assert stats(gb)["method"] == 6, ("the one-value short cut did not run", where)
                k += 1


@pytest.mark.parametrize("s", SOURCES)
def test_apply_bound_scalar_iso(gb, s):
    """iso A: one value computed on the host; it must equal what the stream gave the same value in the non-iso matrix"""
    vals = entry_values(s)
    A = matrix_of(gb, s, vals)
    scalars = scalars_of(s)
    k = 0
    for vi, v in enumerate(source_values(s)):
        I = iso_matrix_of(gb, s, v)
        full = np.full(NNZ, v)
        for ot in OP_TYPES_ISO:
            ops = binary_ops_of(ot)
            for ct in ALL_TYPES:
                op, side, scalar = ops[k % len(ops)], ("right", "left")[(k // 3) % 2], scalars[k % len(scalars)]
                where = f"apply iso {s} {v!r} -> {op}[{ot}] {side}={scalar!r} -> {ct}"
                typed = getattr(gb.binary, op)[ot]
                X = finish(gb, I.apply(typed, **{side: scalar}), (ROWS, COLS, apply_T(op, side, ot, ct, full, scalar)), (M, N), ct, None, where,
                           free_of(op))
                assert stats(gb)["method"] == 6, ("iso A ran a value pass", where)
                if ct in ("UINT8", "INT64"):  # the stream on the same value, directly
                    Y = finish(gb, A.apply(typed, **{side: scalar}), (ROWS, COLS, apply_T(op, side, ot, ct, vals, scalar)), (M, N), ct, None, where,
                               free_of(op))
                    assert same_arr(X[:1], Y[vi:vi + 1]).all() or free_of(op), (where, X[0], Y[vi])
                k += 1
        ot = OP_TYPES_ISO[vi % 4]
        finish(gb, I.apply(gb.binary.plus[ot], right=scalars[0]), (ROWS, COLS, apply_T("plus", "right", ot, "INT16", full, scalars[0])), (M, N),
               "INT16", "FP64", f"apply iso {s} {v!r} masked")


def test_apply_examples(gb):
    """FP64 1e10 through an INT32 operator into an INT64 C is 2147483647 + 0 (not 10^10); 0.5 through a BOOL hop into INT8 is 1."""
    A = gb.Matrix.from_coo([0, 1], [0, 5], np.array([1e10, 0.5]), dtype="FP64", nrows=M, ncols=N)
    C = A.apply(gb.binary.plus["INT32"], right=0).new(dtype="INT64")
    assert C.to_coo()[2].tolist() == [2147483647, 0]
    C = A.apply(gb.binary.lor["BOOL"], right=False).new(dtype="INT8")
    assert C.to_coo()[2].tolist() == [1, 1]
    C = A.apply(gb.binary.ge["UINT8"], right=np.float64(300.7)).new(dtype="FP32")  # (UINT8) 1e10 = 255 >= (UINT8) 300.7 = 255
    assert C.to_coo()[2].tolist() == [1.0, 0.0]


@pytest.mark.parametrize("itype", ["INT32", "INT64"])
def test_apply_index(gb, itype):
    """ROWINDEX / COLINDEX / DIAGINDEX: i + k in int64 arithmetic that wraps -> the operator's INT32 / INT64 (an integer cast: it
    wraps) -> ct (INT8 wraps again, FP32 rounds), with thunks that push i + k past INT32 and past INT64.  The values of A are not read."""
    A = matrix_of(gb, "FP32", entry_values("FP32"))
    u_idx = np.arange(NNZ) + 3 * (np.arange(NNZ) >= 64)
    u = gb.Vector.from_coo(u_idx, entry_values("FP32"), dtype="FP32", size=100)

    def wrap64(x):
        return np.array([(int(t) + 2**63) % 2**64 - 2**63 for t in x], np.int64)

    k = 0
    for thunk in (0, -3, 2**31 - 2, -(2**31) - 1, 2**31 + 5, 2**40 + 5, 2**63 - 1, -(2**63), 125, np.int8(-128), np.uint64(2**64 - 1)):
        kk = int(chain(np.asarray(thunk), "INT64"))
        for op in INDEX:
            i, j = ROWS.astype(object), COLS.astype(object)
            t64 = wrap64({"rowindex": i + kk, "colindex": j + kk, "diagindex": j - i + kk}[op])
            for ct in ALL_TYPES:
                for mode in modes_for(k):
                    where = f"apply {op}[{itype}] thunk {thunk!r} -> {ct} mode {mode}"
                    finish(gb, A.apply(getattr(gb.indexunary, op)[itype], thunk), (ROWS, COLS, chain(t64, itype, ct)), (M, N), ct, mode, where)
                k += 1
            if op != "colindex":  # the vector form: a vector is a column, j = 0
                v64 = wrap64(u_idx.astype(object) * (1 if op == "rowindex" else -1) + kk)
                ct = ALL_TYPES[k % 11]
                w = gb.Vector(ct, 100)
                w << u.apply(getattr(gb.indexunary, op)[itype], thunk)
                I, X = w.to_coo()
                assert I.tolist() == u_idx.tolist()
                compare_values(X, chain(v64, itype, ct), None, f"vector apply {op}[{itype}] thunk {thunk!r} -> {ct}")


# ---- 3. eWiseAdd / eWiseMult -----------------------------------------------------------------------------------------------------------
def dense_of(rows, cols, vals, shape=(M, N)):
    has, val = np.zeros(shape, bool), np.zeros(shape, vals.dtype)
    has[rows, cols], val[rows, cols] = True, vals
    return has, val


def ewise_T(op, ot, ct, a, b, union, shape=(M, N)):
    """a, b = (rows, cols, values in their own types).  Both present: op((ot) a, (ot) b) -> tt; one present (eWiseAdd): s -> ot -> tt;
    then -> ct."""
    tt = "BOOL" if op in CMP else ot
    ha, va = dense_of(a[0], a[1], chain(a[2], ot), shape)
    hb, vb = dense_of(b[0], b[1], chain(b[2], ot), shape)
    both = np.asarray(np_op(op, ot, va, vb))
    t = np.where(ha & hb, both, np.where(ha, chain(va, tt), chain(vb, tt)))
    assert t.dtype == np.dtype(NP_OF[tt])
    has = (ha | hb) if union else (ha & hb)
    r, c = np.nonzero(has)
    return r, c, chain(t[r, c], ct)


@pytest.mark.parametrize("s", SOURCES)
def test_ewise(gb, s):
    vals = entry_values(s)
    A = matrix_of(gb, s, vals)
    a = (ROWS, COLS, vals)
    Bs, bs = {}, {}
    for sb in SOURCES:
        bv = entry_values(sb, B_ROWS.size, shift=5)
        bs[sb] = (B_ROWS, B_COLS, bv)
        Bs[sb] = matrix_of(gb, sb, bv, B_ROWS, B_COLS)
    ops = ARITH[:-1] + CMP
    k = 0
    for oi, ot in enumerate(OP_TYPES):
        for ct in ALL_TYPES:
            sb = SOURCES[(oi + k) % len(SOURCES)]
            op = ops[k % len(ops)]
            typed = getattr(gb.binary, op)[ot]
            for mode in modes_for(k):
                where = f"({s}, {sb}) -> {op}[{ot}] -> {ct} mode {mode}"
                finish(gb, A.ewise_add(Bs[sb], typed), ewise_T(op, ot, ct, a, bs[sb], True), (M, N), ct, mode, "eWiseAdd " + where, free_of(op))
                finish(gb, Bs[sb].ewise_mult(A, typed), ewise_T(op, ot, ct, bs[sb], a, False), (M, N), ct, mode, "eWiseMult " + where, free_of(op))
            # under a comparison the entries of one operand alone go ot -> BOOL -> ct
            cmp = CMP[k % 6]
            finish(gb, A.ewise_add(Bs[sb], getattr(gb.binary, cmp)[ot]), ewise_T(cmp, ot, ct, a, bs[sb], True), (M, N), ct, None,
                   f"eWiseAdd ({s}, {sb}) -> {cmp}[{ot}] -> {ct}")
            # the other operand empty: the pass-through, s -> ot -> tt -> ct, on either side
            E = gb.Matrix(sb, M, N)
            none = (ROWS[:0], COLS[:0], bs[sb][2][:0])
            for pop in (op, cmp):
                ptyped = getattr(gb.binary, pop)[ot]
                finish(gb, A.ewise_add(E, ptyped), ewise_T(pop, ot, ct, a, none, True), (M, N), ct, None, f"eWiseAdd with an empty B {s} -> {pop}[{ot}] -> {ct}")
                finish(gb, E.ewise_add(A, ptyped), ewise_T(pop, ot, ct, none, a, True), (M, N), ct, modes_for(k)[-1],
                       f"eWiseAdd with an empty A {s} -> {pop}[{ot}] -> {ct}")
            k += 1


@pytest.mark.parametrize("s", SOURCES)
def test_ewise_iso(gb, s):
    """iso A against a non-iso B (eWiseAdd, eWiseMult), and alone against an empty B (the pass-through of one value), in turn"""
    Bs, bs = {}, {}
    for sb in SOURCES:
        bv = entry_values(sb, B_ROWS.size, shift=5)
        bs[sb] = (B_ROWS, B_COLS, bv)
        Bs[sb] = matrix_of(gb, sb, bv, B_ROWS, B_COLS)
    ops = ARITH[:-1] + CMP
    k = 0
    for vi, v in enumerate(source_values(s)):
        I = iso_matrix_of(gb, s, v)
        ia = (ROWS, COLS, np.full(NNZ, v))
        E = gb.Matrix(s, M, N)
        none = (ROWS[:0], COLS[:0], ia[2][:0])
        for oi, ot in enumerate(OP_TYPES_ISO):
            for ct in ALL_TYPES:
                sb = SOURCES[(oi + k) % len(SOURCES)]
                op = ops[k % len(ops)]
                typed = getattr(gb.binary, op)[ot]
                where = f"iso {s} {v!r}, {sb} -> {op}[{ot}] -> {ct}"
                if k % 3 == 0:
                    finish(gb, I.ewise_add(Bs[sb], typed), ewise_T(op, ot, ct, ia, bs[sb], True), (M, N), ct, None, "eWiseAdd " + where, free_of(op))
                elif k % 3 == 1:
                    finish(gb, I.ewise_mult(Bs[sb], typed), ewise_T(op, ot, ct, ia, bs[sb], False), (M, N), ct, None, "eWiseMult " + where, free_of(op))
                else:
                    finish(gb, I.ewise_add(E, typed), ewise_T(op, ot, ct, ia, none, True), (M, N), ct, None, "eWiseAdd with an empty B " + where)
                k += 1
        ot = OP_TYPES_ISO[vi % 4]
        finish(gb, E.ewise_add(I, gb.binary.ge[ot]), ewise_T("ge", ot, "INT32", none, ia, True), (M, N), "INT32", "INT8",
               f"eWiseAdd iso {s} {v!r} with an empty A, masked")


# ---- 4. kronecker -------------------------------------------------------------------------------------------------------------------------
KB_ROWS, KB_COLS = np.array([0, 0, 1], np.int64), np.array([0, 1, 1], np.int64)  # 2 x 2, three entries
KB_INDPTR = np.array([0, 2, 3], np.int64)


def kron_T(op, ot, ct, a, b):
    """T[ia * 2 + ib, ja * 2 + jb] = op((ot) a, (ot) b) -> tt -> ct.  ANY: the first operand."""
    ea, eb = np.repeat(np.arange(a[0].size), b[0].size), np.tile(np.arange(b[0].size), a[0].size)
    rows, cols = a[0][ea] * 2 + b[0][eb], a[1][ea] * 2 + b[1][eb]
    t = np_op("first" if op == "any" else op, ot, chain(a[2], ot)[ea], chain(b[2], ot)[eb])
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], chain(t, ct)[order]


@pytest.mark.parametrize("s", SOURCES)
def test_kronecker(gb, s):
    vals = entry_values(s)
    A = matrix_of(gb, s, vals)
    a = (ROWS, COLS, vals)
    shape = (2 * M, 2 * N)
    ops = ARITH + ["any"] + CMP
    k = 0

    def b_of(sb, shift):
        sv = source_values(sb)
        bv = sv[(np.arange(3) * 5 + shift) % sv.size]
        return (KB_ROWS, KB_COLS, bv), matrix_of(gb, sb, bv, KB_ROWS, KB_COLS, (2, 2))

    for oi, ot in enumerate(OP_TYPES):
        for ct in ALL_TYPES:
            sb = SOURCES[(oi + k) % len(SOURCES)]
            b, B = b_of(sb, k)
            op = ops[k % len(ops)]
            for mode in modes_for(k):
                where = f"kronecker ({s}, {sb} {b[2].tolist()}) -> {op}[{ot}] -> {ct} mode {mode}"
                finish(gb, A.kronecker(B, getattr(gb.binary, op)[ot]), kron_T(op, ot, ct, a, b), shape, ct, mode, where, free_of(op))
            k += 1


@pytest.mark.parametrize("s", SOURCES)
def test_kronecker_iso(gb, s):
    """The iso T short cuts: both operands iso; FIRST / ANY of an iso A; SECOND of an iso B; PAIR -- one value, computed on the host
    (kron_one_value) from operands cast like every entry would be.  Every third case: an iso A against a B that is not iso (the kernel)."""
    vals = entry_values(s)
    A = matrix_of(gb, s, vals)
    a = (ROWS, COLS, vals)
    shape = (2 * M, 2 * N)
    ops = ARITH + ["any"] + CMP
    k = 0
    for vi, v in enumerate(source_values(s)):
        I = iso_matrix_of(gb, s, v)
        ia = (ROWS, COLS, np.full(NNZ, v))
        for oi, ot in enumerate(OP_TYPES_ISO):
            for ct in ALL_TYPES:
                sb = SOURCES[(oi + k) % len(SOURCES)]
                svb = source_values(sb)
                bval = svb[k % svb.size]
                IB = iso_matrix_of(gb, sb, bval, KB_INDPTR, KB_COLS, (2, 2))
                ib = (KB_ROWS, KB_COLS, np.full(3, bval))
                op = ops[k % len(ops)]
                typed = getattr(gb.binary, op)[ot]
                where = f"kronecker iso ({s} {v!r}, {sb} {bval!r}) -> {op}[{ot}] -> {ct}"
                if k % 3 == 0:
                    bv = svb[(np.arange(3) * 5 + k) % svb.size]
                    B = matrix_of(gb, sb, bv, KB_ROWS, KB_COLS, (2, 2))
                    finish(gb, I.kronecker(B, typed), kron_T(op, ot, ct, ia, (KB_ROWS, KB_COLS, bv)), shape, ct, None, where + " (B not iso)", free_of(op))
                elif k % 3 == 1:
                    finish(gb, A.kronecker(IB, gb.binary.second[ot]), kron_T("second", ot, ct, a, ib), shape, ct, None, where + " SECOND of an iso B")
                    assert stats(gb)["method"] == 6, where
                else:
                    finish(gb, I.kronecker(IB, typed), kron_T(op, ot, ct, ia, ib), shape, ct, None, where, free_of(op))
                    assert stats(gb)["method"] == 6, ("two iso operands ran a value pass", where)
                k += 1
        ot = OP_TYPES_ISO[vi % 4]
        finish(gb, I.kronecker(IB, gb.binary.times[ot]), kron_T("times", ot, "UINT16", ia, ib), shape, "UINT16", "FP32", f"kronecker iso {s} {v!r} masked")


# ---- 5. extract ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SOURCES)
def test_extract(gb, s):
    """A[I, J], a row, a column, one element: s -> ct directly, for a non-iso A and for an iso A of every value."""
    from graphblas_amd import _lib

    L = _lib.lib
    vals = entry_values(s)
    I_, J_ = np.array([2, 0]), np.array([69, 0, 5, 64, 3, 68, 1])
    k = 0
    mats = [(matrix_of(gb, s, vals), vals, "")] + [(iso_matrix_of(gb, s, v), np.full(NNZ, v), f" iso {v!r}") for v in source_values(s)]
    for A, av, tag in mats:
        has, val = dense_of(ROWS, COLS, av)
        for ct in ALL_TYPES:
            where = f"extract {s}{tag} -> {ct}"
            sub_h, sub_v = has[np.ix_(I_, J_)], val[np.ix_(I_, J_)]
            r, c = np.nonzero(sub_h)
            for mode in modes_for(k) if not tag else [None]:
                finish(gb, A[I_, J_], (r, c, chain(sub_v[r, c], ct)), (2, 7), ct, mode, where + " A[I, J]")
                finish(gb, A[:, :], (ROWS, COLS, chain(av, ct)), (M, N), ct, mode, where + " A[:, :]")
            for key, h, x in ((np.s_[0, :], has[0], val[0]), (np.s_[2, :], has[2], val[2]), (np.s_[:, 1], has[:, 1], val[:, 1])):
                w = gb.Vector(ct, h.size)
                w << A[key]
                wi, wx = w.to_coo()
                assert wi.tolist() == np.flatnonzero(h).tolist(), (where, key)
                compare_values(wx, chain(x[h], ct), None, f"{where} A[{key}]")
            # one element, through the typed entry point of ct: GrB_Matrix_extractElement_<ct> on a matrix of type s
            fn = getattr(L, f"GrB_Matrix_extractElement_{ct}")
            for e in ((0, 64), (1, 3), (2, 69), (0, k % 70)) if tag else zip(ROWS[:30].tolist(), COLS[:30].tolist()):
                out = np.ctypeslib.as_ctypes_type(NP_OF[ct])()
                rc = fn(ctypes.byref(out), A._handle, e[0], e[1])
                assert rc == 0, (where, e, rc)
                compare_values(np.array([out.value], NP_OF[ct]), chain(val[e[0], e[1]:e[1] + 1], ct), None, f"{where} element {e}")
            k += 1


# ---- 6. assign ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", SOURCES)
def test_assign(gb, s):
    """C(accum)[I, J] << A, a scalar (a Scalar and a plain number), a row, a column: the source -> ct, then the accumulator in ct on the
    cast value.  I is a permutation of the rows and J reverses the columns, so the region is all of C."""
    vals = entry_values(s)
    A = matrix_of(gb, s, vals)
    ha, va = dense_of(ROWS, COLS, vals)
    I_, J_ = np.array([2, 0, 1]), np.arange(N)[::-1].copy()
    scalars = scalars_of(s)
    row_v = entry_values(s, 70, shift=2)
    u_row = gb.Vector.from_coo(np.arange(70), row_v, dtype=s, size=70)
    col_v = entry_values(s, 3, shift=7) if source_values(s).size <= 3 else source_values(s)[[1, 5, 7]]
    u_col = gb.Vector.from_coo(np.arange(3), col_v, dtype=s, size=3)
    k = 0
    for ct in ALL_TYPES:
        Cc = prefill((M, N), ct)
        hc, vc = dense_of(*Cc)
        for accum in (None, "plus"):
            kw = {"accum": gb.binary.plus} if accum else {}

            def check(C, has, val, where):
                r, c = np.nonzero(has)
                Ci, Cj, Cx = C.to_coo()
                assert Ci.tolist() == r.tolist() and Cj.tolist() == c.tolist(), where
                compare_values(Cx, val[r, c], None, where)

            def merged(th, tv):
                """Z over a region (here a mask of positions) = T without an accumulator, accum(C, T) with one; tv is in ct"""
                if accum is None:
                    return th, tv
                return hc | th, np.where(hc & th, np_op("plus", ct, vc, tv), np.where(hc, vc, tv))

            where = f"assign {s} -> {ct} accum {accum}"
            # a matrix: A(i, j) lands at C(I[i], J[j])
            th, tv = np.zeros((M, N), bool), np.zeros((M, N), NP_OF[ct])
            th[np.ix_(I_, J_)], tv[np.ix_(I_, J_)] = ha, chain(va, ct)
            C = gb.Matrix.from_coo(*Cc, dtype=ct, nrows=M, ncols=N)
            C(**kw)[I_, J_] << A
            check(C, *merged(th, tv), where + " matrix")
            # a scalar into a block, as a Scalar (the library casts) and as a plain number
            sc = scalars[k % len(scalars)]
            region = np.zeros((M, N), bool)
            region[np.ix_([0, 2], [0, 5, 64, 69])] = True
            for form in (gb.Scalar.from_value(sc), sc):
                C = gb.Matrix.from_coo(*Cc, dtype=ct, nrows=M, ncols=N)
                C(**kw)[[0, 2], [0, 5, 64, 69]] << form
                zh, zv = merged(region, np.full((M, N), chain(np.asarray(sc), ct)))
                check(C, np.where(region, zh, hc), np.where(region, zv, vc), f"{where} scalar {sc!r} as {type(form).__name__}")
            # a row and a column
            for key, uvec, uv in ((np.s_[1, :], u_row, row_v), (np.s_[:, 5], u_col, col_v)):
                region = np.zeros((M, N), bool)
                region[key] = True
                tv = np.zeros((M, N), NP_OF[ct])
                tv[key] = chain(uv, ct)
                C = gb.Matrix.from_coo(*Cc, dtype=ct, nrows=M, ncols=N)
                C(**kw)[key] << uvec
                zh, zv = merged(region, tv)
                check(C, np.where(region, zh, hc), np.where(region, zv, vc), f"{where} {'row' if key[0] == 1 else 'column'}")
            k += 1
        # under a value mask, accumulating
        for mode in MASK_TYPES:
            Mc = mask_coo((M, N), mode)
            Mk = gb.Matrix.from_coo(*Mc, dtype=mode, nrows=M, ncols=N)
            C = gb.Matrix.from_coo(*Cc, dtype=ct, nrows=M, ncols=N)
            C(mask=Mk.V, accum=gb.binary.plus)[:, :] << A
            er, ec, ev = np_write_rule((M, N), ct, Cc, (ROWS, COLS, chain(vals, ct)), Mc, False, False, False, "plus")
            Ci, Cj, Cx = C.to_coo()
            assert Ci.tolist() == er.tolist() and Cj.tolist() == ec.tolist()
            compare_values(Cx, ev, None, f"assign {s} -> {ct} under a {mode} mask")


# ---- 7. mxm -------------------------------------------------------------------------------------------------------------------------------
# B is 70 x 3 with at most two entries per column that meet a row of A: a sum of two terms is the same in either order, so plus_times
# is exact in FP32 too
MB_ROWS, MB_COLS = np.array([1, 3, 40, 68, 69, 69], np.int64), np.array([0, 2, 0, 1, 1, 2], np.int64)


def mxm_T(sr, st, ct, a, b):
    monoid, mult = sr.split("_")
    ha, va = dense_of(a[0], a[1], chain(a[2], st))
    hb, vb = dense_of(b[0], b[1], chain(b[2], st), (N, 3))
    rows, cols, out = [], [], []
    for i in range(M):
        for j in range(3):
            ks = np.flatnonzero(ha[i] & hb[:, j])
            if ks.size == 0:
                continue
            assert ks.size <= 2
            p = np_op(mult, st, va[i, ks], vb[ks, j])
            acc = p[:1]
            for q in range(1, p.size):
                acc = np_op("first" if monoid == "any" else monoid, st, acc, p[q:q + 1])
            rows.append(i), cols.append(j), out.append(acc[0])
    return np.array(rows, np.int64), np.array(cols, np.int64), chain(np.array(out, NP_OF[st]), ct)


@pytest.mark.parametrize("s", SOURCES)
def test_mxm(gb, s):
    """plus_times, min_plus and any_pair in a semiring type narrower than (or just other than) an operand's: operands -> the semiring's
    type, multiply and fold in it, -> ct.  any_pair is 1 wherever a product exists."""
    vals = entry_values(s)
    A = matrix_of(gb, s, vals)
    a = (ROWS, COLS, vals)
    k = 0
    for oi, st in enumerate(OP_TYPES):
        for ct in ALL_TYPES:
            sb = SOURCES[(oi + k) % len(SOURCES)]
            svb = source_values(sb)
            b = (MB_ROWS, MB_COLS, svb[(np.arange(6) * 3 + k) % svb.size])
            B = matrix_of(gb, sb, b[2], MB_ROWS, MB_COLS, (N, 3))
            for sr in ("plus_times", ("min_plus", "any_pair")[k % 2]):  # (min_plus and any_pair in turn: each meets every st and ct)
                for mode in modes_for(k):
                    where = f"mxm ({s}, {sb} {b[2].tolist()}) {sr}[{st}] -> {ct} mode {mode}"
                    finish(gb, A.mxm(B, getattr(gb.semiring, sr)[st]), mxm_T(sr, st, ct, a, b), (M, 3), ct, mode, where,
                           "min" if sr == "min_plus" else None)
            k += 1
