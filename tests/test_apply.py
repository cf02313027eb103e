"""GrB_apply with a bound scalar or an index-unary operator: ``A.apply(op, right=, left=)`` / ``v.apply(...)`` -- the by-value stream
and the by-position kernel of grb_apply.hip on the GPU tier, the same sources under the SIMT emulator on the CPU tier.

1. the reference's own literals (tests/golden/apply_literals.json) through every spelling the host has;
2. seeded random parity against an expectation computed HERE with numpy on the COO tuples (the operator in its own dtype, a cast, then
   the dense restatement of the write rule of tests/test_select.py) -- independent of the library and of the oracle; bit for bit;
3. the by-value kernel at its pack, wavefront and workgroup limits, for 1-, 2-, 4- and 8-byte types, and on an array that is not
   16-byte aligned;
4. the by-position kernel on matrices built from lists of row lengths: the seams of its blocks, its 64-row-end walk, its shares;
5. the short cuts (iso results without a value pass);
6. the C ABI directly (ctypes);
7. the host's errors;
8. no growth of device memory over repeated calls (GPU tier).

ANY may return either operand; the library returns the bound scalar, and the expectation here says so.  IEEE leaves min(-0, +0) open, so
min / max results are compared with a zero matching a zero of either sign (tests/values.py), everything else as bit patterns.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.backend import DEVICES, ROOT, bind
from tests.test_select import (NP_OF, TYPES, _handle, _matrix_error, assert_coo, assert_vec, draw_coo, draw_matrix, np_keep, np_write_rule,
                               stored_iso)
from tests.values import rand_vals, same_fp

NAME_OF = {np.dtype(v): k for k, v in NP_OF.items()}
ARITH = ["first", "second", "pair", "plus", "minus", "times", "min", "max", "any", "lor", "land", "lxor", "lxnor"]
COMPARE = ["eq", "ne", "gt", "lt", "ge", "le"]
BINARY = ARITH + COMPARE
BOOL_ONLY = ("lor", "land", "lxor", "lxnor")
INDEX = ["rowindex", "colindex", "diagindex"]
POSITIONAL = ["tril", "triu", "diag", "offdiag", "colle", "colgt", "rowle", "rowgt"]
VALUE = ["valueeq", "valuene", "valuegt", "valuege", "valuelt", "valuele"]
THUNKS = [-3, 0, 2]  # (+ one beyond the dimensions, per matrix)


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


@pytest.fixture(scope="module")
def literals():
    with open(os.path.join(ROOT, "tests", "golden", "apply_literals.json")) as f:
        return json.load(f)


def stats(gb):
    from graphblas_amd import device

    return device.last_stats()


# ---- the expectation ------------------------------------------------------------------------------------------------------------------
def np_binary(op, side, vals, scalar):
    """op(a, s) (side "right") or op(s, a) (side "left") over the values, in the operator's dtype X = unify(A.dtype, scalar dtype) --
    BOOL for lor / land / lxor / lxnor.  Returns the values of T in T's own type (BOOL for a comparison, else X)."""
    xt = np.dtype(bool) if op in BOOL_ONLY else np.promote_types(vals.dtype, np.asarray(scalar).dtype)
    with np.errstate(all="ignore"):
        a = vals.astype(xt)
        s = np.full(a.shape, np.asarray(scalar).astype(xt), xt)
        x, y = (s, a) if side == "left" else (a, s)
        if xt == np.dtype(bool):
            table = {"plus": np.logical_or, "max": np.logical_or, "lor": np.logical_or, "times": np.logical_and, "min": np.logical_and,
                     "land": np.logical_and, "minus": np.logical_xor, "lxor": np.logical_xor, "lxnor": lambda p, q: p == q}
        else:
            fl = xt.kind == "f"
            table = {"plus": lambda p, q: p + q, "minus": lambda p, q: p - q, "times": lambda p, q: p * q,
                     "min": np.fmin if fl else np.minimum, "max": np.fmax if fl else np.maximum}
        table.update({"first": lambda p, q: p, "second": lambda p, q: q, "pair": lambda p, q: np.ones_like(p), "any": lambda p, q: s,
                      "eq": lambda p, q: p == q, "ne": lambda p, q: p != q, "gt": lambda p, q: p > q, "lt": lambda p, q: p < q,
                      "ge": lambda p, q: p >= q, "le": lambda p, q: p <= q})
        t = np.asarray(table[op](x, y))
        return t.astype(bool if op in COMPARE else xt)


def np_index(op, itype, r, c, thunk):
    i, j = r.astype(np.int64), c.astype(np.int64)
    with np.errstate(all="ignore"):
        t = {"rowindex": i + np.int64(thunk), "colindex": j + np.int64(thunk), "diagindex": j - i + np.int64(thunk)}[op]
        return t.astype(NP_OF[itype])


def wider(tname):
    """An output type that differs from T's and that numpy's astype casts like the library does (no float -> integer)."""
    return "FP32" if tname == "FP64" else "FP64"


def scalar_for(rng, pick, tname, vals):
    np_t = NP_OF[tname]
    if pick == 0 and vals.size:
        return vals[rng.integers(0, vals.size)]  # a value of the matrix, in the matrix's type
    if pick == 1:
        return np_t(np.nan) if tname.startswith("FP") else np_t(0)
    if pick == 2:
        return 3  # a Python int: the operator runs in unify(A.dtype, INT64) -- a cast pass for every narrower type
    if pick == 3:
        return np.float64(2.5) if not tname.startswith("FP") else (np.float64(-0.0) if tname == "FP32" else np.float32(1.0))  # another dtype: the cast pass
    return np_t(-0.0) if tname.startswith("FP") else (np_t(1) if tname != "BOOL" else np.bool_(False))


def cases_for(span):
    out = [("binary", op, side) for op in BINARY for side in ("right", "left")]
    out += [("index", op, it) for op in INDEX for it in ("INT32", "INT64")]
    out += [("pred", op, None) for op in POSITIONAL + VALUE]
    return out


def expected_T(kind, op, extra, sr, sc, vals, scalar):
    """(values of T, the zero-sign freedom same_fp gets)."""
    if kind == "binary":
        return np_binary(op, extra, vals, scalar), (op if op in ("min", "max") else None)
    if kind == "index":
        return np_index(op, extra, sr, sc, scalar), None
    return np_keep(op, sr, sc, vals, scalar), None


def compare_values(X, ev, free, where):
    assert X.dtype == ev.dtype, (where, X.dtype, ev.dtype)
    if ev.dtype.kind == "f":
        same_fp(X, ev, free, where)
    else:
        assert X.tolist() == ev.tolist(), where


# ---- 1. the reference's literals ----------------------------------------------------------------------------------------------------
def literal_forms(gb, x, case):
    """Every spelling of one literal case: method form, string form, Scalar and plain-number thunk, the monoid for the binary operator."""
    s = case["scalar"]
    if case["kind"] == "binary":
        ops = [getattr(gb.binary, case["op"]), case["op"], *case["spellings"]] + ([getattr(gb.monoid, case["op"])] if case["monoid"] else [])
        return [x.apply(o, **{case["side"]: v}) for o in ops for v in (s, gb.Scalar.from_value(s))]
    op = getattr(gb.indexunary, case["op"])
    ops = [op, getattr(gb.select, case["op"]), case["op"], *case["spellings"]]
    if s is None:
        forms = [x.apply(o) for o in ops] + ([op(x)] if case["callable"] else [])
    else:
        forms = [x.apply(o, v) for o in ops for v in (s, gb.Scalar.from_value(s, gb.dtypes.INT64))]
        forms += [op(x, thunk=s)] if case["callable"] else []
    return forms


def test_matrix_literals(gb, literals):
    lit = literals["matrix"]
    A = gb.Matrix.from_coo(lit["rows"], lit["cols"], lit["vals"], nrows=lit["nrows"], ncols=lit["ncols"])
    for case in lit["cases"]:
        for k, expr in enumerate(literal_forms(gb, A, case)):
            C = expr.new()
            assert C.dtype.name == case["dtype"] and C.shape == A.shape, (case["name"], k, C.dtype)
            assert_coo(C, lit["rows"], lit["cols"], np.asarray(case["vals"], NP_OF[case["dtype"]]), (case["name"], case["source"], k))


def test_vector_literals(gb, literals):
    lit = literals["vector"]
    v = gb.Vector.from_coo(lit["idx"], lit["vals"], size=lit["size"])
    for case in lit["cases"]:
        for k, expr in enumerate(literal_forms(gb, v, case)):
            w = expr.new()
            assert w.dtype.name == case["dtype"] and w.size == v.size, (case["name"], k, w.dtype)
            assert_vec(w, lit["idx"], np.asarray(case["vals"], NP_OF[case["dtype"]]).tolist(), (case["name"], case["source"], k))


# ---- 2. seeded random parity against numpy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("seed", range(14))
def test_apply_random(gb, seed, part):
    """Every implemented binary operator x bind side, rowindex / colindex / diagindex in INT32 and INT64 and every select operator per seed;
    scalars of A's type and of another (the cast pass); thunks -3, 0, 2 and one beyond the dimensions; T0; mask in {none, value,
    structural} x complement x replace; accum in {none, plus, min}; C aliasing A; an output type that differs from T's; empty, 1 x n,
    n x 1 matrices; the hub row; iso input.  A seed's cases are dealt to four tests (``part``); the hub matrix, whose every call walks
    8000 entries under the emulator, takes every twelfth case."""
    rng = np.random.default_rng(9900 + seed)
    tname = TYPES[seed % 7]
    m, n, rows, cols, vals, iso = draw_matrix(rng, seed, tname)
    if iso:
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
        A = gb.Matrix.ss.import_csr(nrows=m, ncols=n, indptr=indptr, values=vals[:1], col_indices=cols, is_iso=True, sorted_cols=True, dtype=tname)
        assert stored_iso(A) and A.nvals == rows.size
    else:
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
    cases = cases_for(max(m, n))
    for ci, (kind, op, extra) in enumerate(cases):
        if ci % 4 != part or (seed % 6 == 5 and (ci // 4) % 3 != seed // 6):
            continue
        cfg = seed * len(cases) + ci
        t0 = (cfg // 5) % 2 == 1
        mask_kind = cfg % 3  # 0 none, 1 value, 2 structural
        comp, repl = (cfg // 3) % 2 == 1, (cfg // 6) % 2 == 1
        accum = [None, "plus", "min"][(cfg // 2) % 3]
        om, on = (n, m) if t0 else (m, n)
        sr, sc = (cols, rows) if t0 else (rows, cols)
        if kind == "binary":
            scalar = scalar_for(rng, (seed + ci) % 5, tname, vals)
        elif kind == "pred" and op in VALUE:
            scalar = scalar_for(rng, (seed + ci) % 5, tname, vals)
        else:
            scalar = (THUNKS + [max(om, on) + 3, -(max(om, on) + 3)])[(seed + ci) % 5]
        tv, free = expected_T(kind, op, extra, sr, sc, vals, scalar)
        ttype = NAME_OF[tv.dtype]
        alias = cfg % 7 == 0 and om == m and on == n and (tv.dtype.kind != "f" or tname.startswith("FP"))
        ctype = tname if alias else (wider(ttype) if cfg % 5 == 1 else ttype)
        with np.errstate(all="ignore"):
            T = (sr, sc, tv.astype(NP_OF[ctype]))
        if alias:
            Cc, C = (rows, cols, vals), A.dup()
            src = C
        else:
            Cc = draw_coo(rng, om, on, ctype, 0.3) if (accum or mask_kind) else None
            C = gb.Matrix.from_coo(*Cc, dtype=ctype, nrows=om, ncols=on) if Cc is not None else gb.Matrix(ctype, om, on)
            src = A
        Mc = draw_coo(rng, om, on, "INT8", 0.5) if mask_kind else None
        kw = {}
        if mask_kind:
            M = gb.Matrix.from_coo(*Mc, dtype="INT8", nrows=om, ncols=on)
            mm = M.S if mask_kind == 2 else M.V
            kw = dict(mask=~mm if comp else mm, replace=repl)
        if accum:
            kw["accum"] = accum
        x = src.T if t0 else src
        if kind == "binary":
            expr = x.apply(getattr(gb.binary, op), **{extra: scalar})
        elif kind == "index":
            expr = x.apply(getattr(gb.indexunary, op)[extra], scalar)
        else:
            expr = x.apply(getattr(gb.select, op), scalar)
        assert expr.dtype.name == ttype, (op, extra, expr.dtype, ttype)
        C(**kw) << expr
        er, ec, ev = np_write_rule((om, on), ctype, Cc, T, Mc, mask_kind == 2, comp and mask_kind > 0, repl and mask_kind > 0, accum)
        where = f"seed {seed} {kind} {op} {extra} scalar {scalar!r} {tname}->{ttype}->{ctype} t0={t0} mask={mask_kind} comp={comp} repl={repl} accum={accum} alias={alias} iso={iso}"
        I, J, X = C.to_coo()
        assert I.tolist() == er.tolist() and J.tolist() == ec.tolist(), where
        compare_values(X, ev, "min" if accum == "min" else free, where)


@pytest.mark.parametrize("seed", range(7))
def test_vector_apply_random(gb, seed):
    rng = np.random.default_rng(6600 + seed)
    tname = TYPES[seed % 7]
    n = [1, 63, 64, 65, 700, 4100, 257][seed % 7]
    idx = np.flatnonzero(rng.random(n) < [0.5, 1.0, 0.0][seed % 3])
    vals = rand_vals(rng, idx.size, tname, "exact") if tname.startswith("FP") else rand_vals(rng, idx.size, tname)
    u = gb.Vector.from_coo(idx, vals, dtype=tname, size=n)
    zero = np.zeros_like(idx)
    cases = cases_for(n)
    for ci, (kind, op, extra) in enumerate(cases):
        cfg = seed * len(cases) + ci
        mask_kind, comp, repl = cfg % 3, (cfg // 3) % 2 == 1, (cfg // 6) % 2 == 1
        accum = [None, "plus", "min"][(cfg // 2) % 3]
        if kind == "binary" or op in VALUE:
            scalar = scalar_for(rng, (seed + ci) % 5, tname, vals)
        else:
            scalar = (THUNKS + [n + 3, -(n + 3)])[(seed + ci) % 5]
        tv, free = expected_T(kind, op, extra, idx, zero, vals, scalar)
        ttype = NAME_OF[tv.dtype]
        alias = cfg % 7 == 0 and (tv.dtype.kind != "f" or tname.startswith("FP"))
        ctype = tname if alias else (wider(ttype) if cfg % 5 == 1 else ttype)
        with np.errstate(all="ignore"):
            T = (idx, zero, tv.astype(NP_OF[ctype]))
        if alias:
            Cc, w = (idx, zero, vals), u.dup()
            src = w
        else:
            ci_ = np.flatnonzero(rng.random(n) < 0.4)
            Cc = (ci_, np.zeros_like(ci_), rand_vals(rng, ci_.size, ctype))
            w = gb.Vector.from_coo(ci_, Cc[2], dtype=ctype, size=n)
            src = u
        Mc, kw = None, {}
        if mask_kind:
            mi = np.flatnonzero(rng.random(n) < 0.5)
            Mc = (mi, np.zeros_like(mi), rand_vals(rng, mi.size, "INT8"))
            mk = gb.Vector.from_coo(mi, Mc[2], dtype="INT8", size=n)
            mm = mk.S if mask_kind == 2 else mk.V
            kw = dict(mask=~mm if comp else mm, replace=repl)
        if accum:
            kw["accum"] = accum
        if kind == "binary":
            expr = src.apply(getattr(gb.binary, op), **{extra: scalar})
        elif kind == "index":
            expr = src.apply(getattr(gb.indexunary, op)[extra], scalar)
        else:
            expr = src.apply(getattr(gb.select, op), scalar)
        w(**kw) << expr
        er, _, ev = np_write_rule((n, 1), ctype, Cc, T, Mc, mask_kind == 2, comp and mask_kind > 0, repl and mask_kind > 0, accum)
        where = f"seed {seed} {kind} {op} {extra} scalar {scalar!r} {tname}->{ttype}->{ctype} mask={mask_kind} comp={comp} repl={repl} accum={accum} alias={alias}"
        I, X = w.to_coo()
        assert I.tolist() == er.tolist(), where
        compare_values(X, ev, "min" if accum == "min" else free, where)


# ---- 3. the by-value kernel at its limits ------------------------------------------------------------------------------------------
def value_sizes(V):
    """A lane's pack of V values, a wavefront's load of 64 V, a workgroup's 256 V (beyond it: the second workgroup); the kernel has no loop."""
    return sorted({V - 1, V, V + 1, 64 * V - 1, 64 * V, 64 * V + 1, 256 * V - 1, 256 * V, 256 * V + 1, 512 * V + 1} - {0})


@pytest.mark.parametrize("tname", ["INT8", "UINT16", "FP32", "INT64"])
def test_value_kernel_limits(gb, tname):
    np_t = NP_OF[tname]
    V = 16 // np.dtype(np_t).itemsize
    rng = np.random.default_rng(V)
    for nnz in value_sizes(V):
        vals = rand_vals(rng, nnz, tname, "exact") if tname == "FP32" else rand_vals(rng, nnz, tname, "signed")
        m = 1 if nnz % 2 else 3  # (the stream does not look at the rows)
        rows = np.sort(rng.integers(0, m, nnz))
        cols = np.concatenate([np.arange(c) for c in np.bincount(rows, minlength=m)])
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=nnz)
        for op, scalar in (("times", np_t(3)), ("gt", np_t(1)), ("minus", np_t(2))):
            C = A.apply(op, left=scalar).new() if op == "minus" else A.apply(op, right=scalar).new()
            st = stats(gb)
            assert st["method"] == 13 and st["tiles"] == -(-nnz // (64 * V)) and st["out_nvals"] == nnz, (tname, nnz, op, st)
            I, J, X = C.to_coo()
            assert I.tolist() == rows.tolist() and J.tolist() == cols.tolist(), (tname, nnz, op)
            compare_values(X, np_binary(op, "left" if op == "minus" else "right", vals, scalar), None, f"{tname} nnz {nnz} {op}")


@pytest.mark.parametrize("dev", DEVICES)
@pytest.mark.parametrize("tname", ["UINT16", "FP32", "INT64"])
def test_value_kernel_unaligned(dev, tname):
    """A value array that starts one element past a 16-byte boundary (an adopted device CSR): the per-element form."""
    import torch

    from graphblas_amd import device

    gb = bind(dev)
    where = "cpu" if dev == "emu" else "cuda"
    np_t = NP_OF[tname]
    V = 16 // np.dtype(np_t).itemsize
    rng = np.random.default_rng(5)
    for nnz in (V + 1, 256 * V - 1, 256 * V + 1):
        vals = rand_vals(rng, nnz, tname, "exact") if tname == "FP32" else rand_vals(rng, nnz, tname, "signed")
        store = np.zeros(nnz + 1, np_t)
        store[1:] = vals
        tstore = torch.from_numpy(store.view(np.int16) if tname == "UINT16" else store).to(where)
        tv = tstore[1:]
        assert tstore.data_ptr() % 16 == 0 and tv.data_ptr() % 16 != 0
        A = device.matrix_from_device_csr(torch.tensor([0, nnz], dtype=torch.int64, device=where),
                                          torch.arange(nnz, dtype=torch.int32, device=where), tv, 1, nnz, tname, copy=False)
        C = A.apply("plus", right=np_t(5)).new()
        st = stats(gb)
        assert st["method"] == 13 and st["tiles"] == -(-nnz // (64 * V)), st
        compare_values(C.to_coo()[2], np_binary("plus", "right", vals, np_t(5)), None, f"unaligned {tname} nnz {nnz}")
        del C, A


# ---- 4. the by-position kernel at its limits -----------------------------------------------------------------------------------------
SHARE = 8 * 64  # entries of one wavefront: SEL_BPW blocks of 64

ROW_LENGTHS = {
    "row ends on entry 63 of a block": [63, 5, 60],
    "row ends on entry 64 of a block": [64, 5, 59],
    "row starts on a block's first entry": [30, 34, 70, 2],
    "row spans several blocks": [3, 200, 1],
    "row spans more than a wavefront's share": [10, SHARE + 300, 7],
    "65 empty rows between two entries": [1] + [0] * 65 + [1],
    "129 empty rows between two entries": [2] + [0] * 129 + [3],
    "empty first and last rows": [0] * 70 + [5, 0, 9] + [0] * 66,
    "one row": [100],
    "63 entries": [20, 43],
    "64 entries": [64],
    "65 entries": [1, 0, 64],
    "a share less one": [SHARE - 1],
    "a share": [100] * 5 + [12],
    "a share and one": [SHARE, 1],
    "m + 1 no multiple of 64": [1] * 100,
    "many short rows across a share": [3, 0, 1] * 400,
}


@pytest.mark.parametrize("name", list(ROW_LENGTHS))
def test_position_kernel_limits(gb, name):
    deg = np.asarray(ROW_LENGTHS[name])
    m, n = deg.size, int(max(deg.max(), 2)) + 3
    rng = np.random.default_rng(len(name))
    rows = np.repeat(np.arange(m), deg)
    cols = np.concatenate([np.sort(rng.choice(n, d, replace=False)) for d in deg])
    A = gb.Matrix.from_coo(rows, cols, np.ones(rows.size, np.int64), dtype="INT64", nrows=m, ncols=n)
    nnz = rows.size
    for op, thunk in (("rowindex", 0), ("diagindex", 1), ("tril", -1)):
        C = A.apply(op, thunk).new()
        st = stats(gb)
        assert st["method"] == 14 and st["tiles"] == -(-(-(-nnz // 64)) // 8) and st["out_nvals"] == nnz, (name, op, st)
        I, J, X = C.to_coo()
        assert I.tolist() == rows.tolist() and J.tolist() == cols.tolist(), (name, op)
        exp = np_keep(op, rows, cols, None, thunk) if op == "tril" else np_index(op, "INT64", rows, cols, thunk)
        assert C.dtype.name == ("BOOL" if op == "tril" else "INT64")
        assert X.tolist() == exp.tolist(), (name, op)


# ---- 5. the short cuts ---------------------------------------------------------------------------------------------------------------
def test_short_cuts(gb, literals):
    lit = literals["matrix"]
    r, c, x = (np.asarray(lit[k]) for k in ("rows", "cols", "vals"))
    A = gb.Matrix.from_coo(r, c, x, nrows=7, ncols=7)
    for expr, val in ((A.apply(gb.binary.second, right=1), 1), (A.apply(gb.binary.first, left=4), 4), (A.apply(gb.binary.pair, right=9), 1),
                      (A.apply(gb.binary.pair, left=9), 1), (A.apply(gb.binary.any, right=6), 6)):
        C = expr.new()
        assert stats(gb)["method"] == 6 and stats(gb)["out_nvals"] == r.size and stored_iso(C)
        assert_coo(C, r, c, np.full(r.size, val), "iso short cut")
    # the same calls under a mask and an accumulator: one value per entry again
    M = gb.Matrix.from_coo([0, 3, 6, 2], [3, 0, 4, 2], [1, 0, 1, 1], nrows=7, ncols=7)
    C = A.dup()
    C(M.V, gb.binary.plus) << A.apply(gb.binary.second, right=10)
    hit = np.isin(r * 7 + c, [0 * 7 + 3, 6 * 7 + 4])
    assert_coo(C, r, c, np.where(hit, x + 10, x), "second under mask + accum")
    C = gb.Matrix(int, 7, 7)
    C(~M.S) << A.apply(gb.binary.pair, left=3)
    keep = ~np.isin(r * 7 + c, [0 * 7 + 3, 3 * 7 + 0, 6 * 7 + 4, 2 * 7 + 2])
    assert_coo(C, r[keep], c[keep], np.ones(int(keep.sum()), np.int64), "pair under a complemented mask")
    # an iso A under a by-value operator stays iso; an empty A runs no value pass
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=7))])
    order = np.lexsort((c, r))
    I = gb.Matrix.ss.import_csr(nrows=7, ncols=7, indptr=indptr, values=np.array([5], np.int64), col_indices=c[order], is_iso=True, sorted_cols=True,
                                dtype="INT64")
    C = I.apply(gb.binary.times, right=3).new()
    assert stored_iso(C) and stats(gb)["method"] == 6
    assert_coo(C, r, c, np.full(r.size, 15), "iso A under times")
    C = I.apply(gb.binary.gt, left=7).new()
    assert stored_iso(C) and C.dtype.name == "BOOL"
    assert_coo(C, r, c, np.ones(r.size, bool), "iso A under gt")
    E = gb.Matrix(int, 5, 4).apply(gb.binary.times, right=3).new()
    assert E.nvals == 0 and stats(gb)["method"] == 6 and stats(gb)["kernel_launches"] == 0


# ---- 6. the C ABI directly -------------------------------------------------------------------------------------------------------------
def test_c_abi(gb, literals):
    from graphblas_amd import _lib

    L = _lib.lib
    lit = literals["matrix"]
    r, c, x = (np.asarray(lit[k]) for k in ("rows", "cols", "vals"))
    A = gb.Matrix.from_coo(r, c, x, nrows=7, ncols=7)
    C = gb.Matrix(int, 7, 7)
    B = gb.Matrix(bool, 7, 7)
    v = gb.Vector.from_coo([1, 3, 4, 6], [1, 1, 2, 0], size=7)
    w = gb.Vector(int, 7)
    # typed forms of all three kinds
    assert L.GrB_Matrix_apply_BinaryOp2nd_INT64(C._carg, None, None, _handle(L, "GrB_TIMES_INT64"), A._carg, 3, None) == 0
    assert_coo(C, r, c, x * 3, "BinaryOp2nd_INT64")
    assert L.GrB_Matrix_apply_BinaryOp1st_INT64(C._carg, None, None, _handle(L, "GrB_MINUS_INT64"), 8, A._carg, None) == 0
    assert_coo(C, r, c, 8 - x, "BinaryOp1st_INT64")
    assert L.GrB_Matrix_apply_BinaryOp2nd_FP64(B._carg, None, None, _handle(L, "GrB_GT_INT64"), A._carg, 2.0, None) == 0  # (the scalar is cast to the operator's type)
    assert_coo(B, r, c, x > 2, "BinaryOp2nd_FP64 with GrB_GT_INT64")
    assert L.GrB_Matrix_apply_IndexOp_INT64(C._carg, None, None, _handle(L, "GrB_ROWINDEX_INT64"), A._carg, 1, None) == 0
    assert_coo(C, r, c, r + 1, "IndexOp_INT64 ROWINDEX")
    assert L.GrB_Matrix_apply_IndexOp_INT32(C._carg, None, None, _handle(L, "GrB_DIAGINDEX_INT32"), A._carg, 0, None) == 0
    assert_coo(C, r, c, c - r, "IndexOp_INT32 DIAGINDEX")
    assert L.GrB_Matrix_apply_IndexOp_BOOL(B._carg, None, None, _handle(L, "GrB_TRIL"), A._carg, False, None) == 0
    assert_coo(B, r, c, c <= r, "IndexOp_BOOL TRIL")
    assert L.GrB_Vector_apply_BinaryOp2nd_INT64(w._carg, None, None, _handle(L, "GrB_PLUS_INT64"), v._carg, 5, None) == 0
    assert_vec(w, [1, 3, 4, 6], [6, 6, 7, 5], "Vector BinaryOp2nd")
    assert L.GrB_Vector_apply_BinaryOp1st_INT64(w._carg, None, None, _handle(L, "GrB_MINUS_INT64"), 2, v._carg, None) == 0
    assert_vec(w, [1, 3, 4, 6], [1, 1, 0, 2], "Vector BinaryOp1st")
    assert L.GrB_Vector_apply_IndexOp_INT64(w._carg, None, None, _handle(L, "GrB_ROWINDEX_INT64"), v._carg, 10, None) == 0
    assert_vec(w, [1, 3, 4, 6], [11, 13, 14, 16], "Vector IndexOp")
    # the _Scalar forms; an empty scalar
    L.GrB_Scalar_setElement_INT64.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    s = ctypes.c_void_p()
    assert L.GrB_Scalar_new(ctypes.byref(s), _handle(L, "GrB_INT64")) == 0
    try:
        for fn, args in (("GrB_Matrix_apply_BinaryOp2nd_Scalar", (_handle(L, "GrB_PLUS_INT64"), A._carg, s)),
                         ("GrB_Matrix_apply_BinaryOp1st_Scalar", (_handle(L, "GrB_PLUS_INT64"), s, A._carg)),
                         ("GrB_Matrix_apply_IndexOp_Scalar", (_handle(L, "GrB_COLINDEX_INT64"), A._carg, s))):
            assert getattr(L, fn)(C._carg, None, None, *args, None) == -106, fn  # GrB_EMPTY_OBJECT
            assert "empty" in _matrix_error(L, C), fn
        assert L.GrB_Vector_apply_BinaryOp2nd_Scalar(w._carg, None, None, _handle(L, "GrB_PLUS_INT64"), v._carg, s, None) == -106
        assert L.GrB_Vector_apply_BinaryOp1st_Scalar(w._carg, None, None, _handle(L, "GrB_PLUS_INT64"), s, v._carg, None) == -106
        assert L.GrB_Vector_apply_IndexOp_Scalar(w._carg, None, None, _handle(L, "GrB_ROWINDEX_INT64"), v._carg, s, None) == -106
        assert L.GrB_Scalar_setElement_INT64(s, 2) == 0
        assert L.GrB_Matrix_apply_BinaryOp2nd_Scalar(C._carg, None, None, _handle(L, "GrB_PLUS_INT64"), A._carg, s, None) == 0
        assert_coo(C, r, c, x + 2, "BinaryOp2nd_Scalar")
        assert L.GrB_Matrix_apply_BinaryOp1st_Scalar(C._carg, None, None, _handle(L, "GrB_MINUS_INT64"), s, A._carg, None) == 0
        assert_coo(C, r, c, 2 - x, "BinaryOp1st_Scalar")
        assert L.GrB_Matrix_apply_IndexOp_Scalar(C._carg, None, None, _handle(L, "GrB_COLINDEX_INT64"), A._carg, s, None) == 0
        assert_coo(C, r, c, c + 2, "IndexOp_Scalar")
        assert L.GrB_Vector_apply_BinaryOp2nd_Scalar(w._carg, None, None, _handle(L, "GrB_TIMES_INT64"), v._carg, s, None) == 0
        assert_vec(w, [1, 3, 4, 6], [2, 2, 4, 0], "Vector BinaryOp2nd_Scalar")
        assert L.GrB_Vector_apply_BinaryOp1st_Scalar(w._carg, None, None, _handle(L, "GrB_MINUS_INT64"), s, v._carg, None) == 0
        assert_vec(w, [1, 3, 4, 6], [1, 1, 0, 2], "Vector BinaryOp1st_Scalar")
        assert L.GrB_Vector_apply_IndexOp_Scalar(w._carg, None, None, _handle(L, "GrB_DIAGINDEX_INT64"), v._carg, s, None) == 0
        assert_vec(w, [1, 3, 4, 6], [1, -1, -2, -4], "Vector IndexOp_Scalar")
    finally:
        L.GrB_Scalar_free(ctypes.byref(s))
    # NULL output, input and operator
    plus = _handle(L, "GrB_PLUS_INT64")
    assert L.GrB_Matrix_apply_BinaryOp2nd_INT64(None, None, None, plus, A._carg, 1, None) == -2  # GrB_NULL_POINTER
    assert L.GrB_Matrix_apply_BinaryOp2nd_INT64(C._carg, None, None, plus, None, 1, None) == -2
    assert L.GrB_Matrix_apply_BinaryOp2nd_INT64(C._carg, None, None, None, A._carg, 1, None) == -2
    assert L.GrB_Matrix_apply_BinaryOp1st_INT64(C._carg, None, None, None, 1, A._carg, None) == -2
    assert L.GrB_Matrix_apply_IndexOp_INT64(C._carg, None, None, None, A._carg, 1, None) == -2
    assert L.GrB_Vector_apply_BinaryOp2nd_INT64(None, None, None, plus, v._carg, 1, None) == -2
    assert L.GrB_Vector_apply_BinaryOp2nd_INT64(w._carg, None, None, plus, None, 1, None) == -2
    assert L.GrB_Vector_apply_IndexOp_INT64(w._carg, None, None, None, v._carg, 1, None) == -2
    # shapes, with and without T0
    R = gb.Matrix.from_coo([0, 2], [1, 4], [1, 2], nrows=3, ncols=5)
    D = gb.Matrix(int, 3, 5)
    assert L.GrB_Matrix_apply_BinaryOp2nd_INT64(C._carg, None, None, plus, R._carg, 1, None) == -6  # GrB_DIMENSION_MISMATCH
    assert "7 x 7" in _matrix_error(L, C) and "3 x 5" in _matrix_error(L, C)
    assert L.GrB_Matrix_apply_BinaryOp2nd_INT64(D._carg, None, None, plus, R._carg, 1, _handle(L, "GrB_DESC_T0")) == -6
    assert L.GrB_Matrix_apply_IndexOp_INT64(D._carg, None, None, _handle(L, "GrB_ROWINDEX_INT64"), R._carg, 1, _handle(L, "GrB_DESC_T0")) == -6
    Dt = gb.Matrix(int, 5, 3)
    assert L.GrB_Matrix_apply_IndexOp_INT64(Dt._carg, None, None, _handle(L, "GrB_ROWINDEX_INT64"), R._carg, 0, _handle(L, "GrB_DESC_T0")) == 0
    assert_coo(Dt, [1, 4], [0, 2], [1, 4], "T0")
    assert L.GrB_Matrix_apply_BinaryOp2nd_INT64(D._carg, None, None, plus, R._carg, 1, _handle(L, "GrB_DESC_T1")) == 0  # (T1 is ignored)
    assert_coo(D, [0, 2], [1, 4], [2, 3], "T1")
    assert L.GrB_Vector_apply_BinaryOp2nd_INT64(gb.Vector(int, 5)._carg, None, None, plus, v._carg, 1, None) == -6
    # a comparison is no accumulator; GrB_DIV is a handle only
    assert L.GrB_Matrix_apply_BinaryOp2nd_INT64(D._carg, None, _handle(L, "GrB_EQ_INT64"), plus, R._carg, 1, None) == -5  # GrB_DOMAIN_MISMATCH
    F = gb.Matrix("FP64", 3, 5)
    assert L.GrB_Matrix_apply_BinaryOp2nd_FP64(F._carg, None, None, _handle(L, "GrB_DIV_FP64"), R._carg, 2.0, None) == -8  # GrB_NOT_IMPLEMENTED
    assert "not implemented" in _matrix_error(L, F)
    assert F.nvals == 0
    # a complemented absent mask writes nothing
    assert L.GrB_Matrix_apply_BinaryOp2nd_INT64(D._carg, None, None, plus, R._carg, 1, _handle(L, "GrB_DESC_C")) == 0
    assert_coo(D, [0, 2], [1, 4], [2, 3], "complemented absent mask")
    # the unary form stays outside the path
    L.GrB_Matrix_apply.argtypes = [ctypes.c_void_p] * 6
    assert L.GrB_Matrix_apply(C._carg, None, None, _handle(L, "GrB_AINV_INT64"), A._carg, None) == -8
    assert "outside" in _matrix_error(L, C)


# ---- 7. the host's errors ------------------------------------------------------------------------------------------------------------
def test_host_errors(gb, literals):
    lit = literals["matrix"]
    A = gb.Matrix.from_coo(lit["rows"], lit["cols"], lit["vals"], nrows=7, ncols=7)
    v = gb.Vector.from_coo(literals["vector"]["idx"], literals["vector"]["vals"], size=7)
    for x in (A, v):
        with pytest.raises(TypeError):  # tests/test_matrix.py:1188-1191, tests/test_vector.py:686-689
            x.apply(gb.binary.plus, left=x)
        with pytest.raises(TypeError):
            x.apply(gb.binary.plus, right=x)
        with pytest.raises(TypeError, match="Cannot provide both"):  # tests/test_matrix.py:1192-1193
            x.apply(gb.binary.plus, left=1, right=1)
        with pytest.raises(TypeError):
            x.apply(gb.binary.plus)
        with pytest.raises(TypeError, match="left"):  # tests/test_matrix.py:1232-1233
            x.apply(gb.select.valueeq, left=gb.Scalar.from_value(3))
        with pytest.raises(TypeError, match="left"):
            x.apply(gb.indexunary.rowindex, left=1)
        with pytest.raises(TypeError, match="apply only accepts UnaryOp with no scalars or BinaryOp"):  # tests/test_vector.py:671-672
            x.apply(gb.semiring.min_plus)
        with pytest.raises(gb.exceptions.EmptyObject):  # tests/test_vector.py:700-703
            x.apply(gb.binary.plus, gb.Scalar(int)).new()
        with pytest.raises(gb.exceptions.NotImplementedException, match="outside"):
            x.apply(gb.unary.ainv).new()
        with pytest.raises(gb.exceptions.DomainMismatch, match="BOOL"):  # an apply operator does not select
            x.select(gb.indexunary.rowindex).new()
    assert gb.indexunary.rowindex is gb.select.rowindex and A.apply("rowindex").dtype.name == "INT64"
    assert A.apply(gb.indexunary.rowindex["INT32"]).new().dtype.name == "INT32"
    calls = []
    gb.record_calls(calls)
    try:
        A.apply(gb.binary.times, right=gb.Scalar.from_value(2)).new()
        A.T.apply(gb.binary.times, left=2.0).new()
        v.apply("index", 1).new()
    finally:
        gb.record_calls(None)
    names = [c.split("(")[0] for c in calls if "_apply_" in c]
    assert names == ["GrB_Matrix_apply_BinaryOp2nd_Scalar", "GrB_Matrix_apply_BinaryOp1st_FP64", "GrB_Vector_apply_IndexOp_INT64"], calls
    assert any("GrB_DESC_T0" in c for c in calls if "BinaryOp1st" in c), calls


# ---- 8. no growth ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_growth():
    """200 applies per cycle (by value with and without a cast pass, by position, a short cut; with and without a mask) on one matrix,
    results freed.  The library keeps freed blocks in its size-class cache, so the first cycle may grow; free device memory after cycle 2
    against after cycle 3."""
    import torch

    from graphblas_amd import synthetic

    gb = bind("gpu")
    scale = 14
    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, device="cpu")
    A = gb.Matrix.from_csr(ip.numpy(), col.numpy().astype(np.int64), synthetic.edge_weights(col, scale).numpy(), dtype="FP32", ncols=n)
    M = A.select("triu", 1).new()

    def free_bytes():
        gb.Matrix(int, 1, 1).wait()
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    def cycle():
        for k in range(50):
            for expr, mask in ((A.apply("times", right=np.float32(0.85)), None), (A.apply(">", right=100), M.S), (A.apply("rowindex", k), None),
                               (A.apply("second", right=np.float32(1)), M.V)):
                r = expr.new(mask=mask) if mask is not None else expr.new()
                del r

    cycle()
    cycle()
    after2 = free_bytes()
    cycle()
    after3 = free_bytes()
    print(f"free after cycle 2: {after2 / 2**20:.1f} MiB, after cycle 3: {after3 / 2**20:.1f} MiB")
    assert after3 >= after2, (after2, after3)
