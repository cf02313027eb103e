"""GrB_select: ``A.select(op, thunk)`` / ``v.select(op, thunk)`` with the builtin index-unary operators (tril, triu, diag, offdiag,
rowle, rowgt, colle, colgt, value{eq,ne,gt,ge,lt,le}) -- the entry-parallel flag / scan / rows / fill kernel of grb_select.hip on the
GPU tier, the same sources under the SIMT emulator on the CPU tier.

1. the reference's own literals (tests/golden/select_literals.json), through the method form, the functional form and every string
   spelling the literals use;
2. seeded random parity against an expectation computed HERE with numpy on the COO tuples (a boolean filter, then a dense
   restatement of the write rule) -- independent of the library and of the oracle; compared bit for bit;
3. the C ABI directly (ctypes);
4. triangle counting end to end against scipy;
5. no growth of device memory over repeated calls (GPU tier).
"""
import ctypes
import json
import os

import numpy as np
import pytest

from tests.backend import DEVICES, ROOT, bind
from tests.values import rand_vals, same_fp

NP_OF = {"BOOL": np.bool_, "INT8": np.int8, "INT16": np.int16, "INT32": np.int32, "INT64": np.int64, "UINT8": np.uint8,
         "UINT16": np.uint16, "UINT32": np.uint32, "UINT64": np.uint64, "FP32": np.float32, "FP64": np.float64}
TYPES = ["INT64", "FP32", "BOOL", "FP64", "INT8", "UINT16", "INT32"]  # (tests/test_random_parity.py::TYPES)
POSITIONAL = ["tril", "triu", "diag", "offdiag", "colle", "colgt", "rowle", "rowgt"]
VALUE = ["valueeq", "valuene", "valuegt", "valuege", "valuelt", "valuele"]
OPS = POSITIONAL + VALUE
# an output type that differs from the input's and that numpy's astype casts like the library does (no float -> integer)
OTHER_TYPE = {"INT64": "FP64", "FP32": "FP64", "BOOL": "INT32", "FP64": "FP32", "INT8": "INT64", "UINT16": "FP32", "INT32": "INT64"}


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


@pytest.fixture(scope="module")
def literals():
    with open(os.path.join(ROOT, "tests", "golden", "select_literals.json")) as f:
        return json.load(f)


def assert_coo(got, rows, cols, vals, where=""):
    """A library Matrix against COO tuples in any order."""
    I, J, X = got.to_coo()
    order = np.lexsort((np.asarray(cols), np.asarray(rows)))
    assert I.tolist() == np.asarray(rows)[order].tolist() and J.tolist() == np.asarray(cols)[order].tolist(), where
    assert X.tolist() == np.asarray(vals)[order].tolist(), where


def assert_vec(got, idx, vals, where=""):
    I, X = got.to_coo()
    assert I.tolist() == list(idx) and X.tolist() == list(vals), (where, I, X)


# ---- 1. the reference's literals ------------------------------------------------------------------------------------------
def test_matrix_literals(gb, literals):
    lit = literals["matrix"]
    A = gb.Matrix.from_coo(lit["rows"], lit["cols"], lit["vals"], nrows=lit["nrows"], ncols=lit["ncols"])
    for case in lit["cases"]:
        args = () if case["thunk"] is None else (case["thunk"],)
        op = getattr(gb.select, case["op"])
        forms = [A.select(op, *args), A.select(getattr(gb.indexunary, case["op"]), *args), op(A, *args), A.select(case["op"], *args)]
        forms += [A.select(s, *args) for s in case["spellings"]]
        for k, expr in enumerate(forms):
            C = expr.new()
            assert C.dtype == A.dtype and C.shape == A.shape
            assert_coo(C, case["rows"], case["cols"], case["vals"], (case["name"], case["source"], k))
    with pytest.raises(TypeError, match="thunk"):  # tests/test_matrix.py:1262-1263
        A.select(gb.select.valueeq, object())


def test_vector_literals(gb, literals):
    lit = literals["vector"]
    v = gb.Vector.from_coo(lit["idx"], lit["vals"], size=lit["size"])
    for case in lit["cases"]:
        args = () if case["thunk"] is None else (case["thunk"],)
        op = getattr(gb.select, case["op"])
        forms = [v.select(op, *args), op(v, *args), v.select(case["op"], *args)] + [v.select(s, *args) for s in case["spellings"]]
        for k, expr in enumerate(forms):
            w = expr.new()
            assert w.dtype == v.dtype and w.size == v.size
            assert_vec(w, case["idx"], case["vals"], (case["name"], case["source"], k))
    with pytest.raises(TypeError, match="thunk"):  # tests/test_vector.py:745-746
        v.select(gb.select.valueeq, object())


def test_vector_mask_sequence(gb, literals):
    """tests/test_vector.py:765-802 restated with the syntax the host has (``w << 1``, ``w[i] = x``, ``del w[i]``)."""
    lit, seq = literals["vector"], literals["mask_sequence"]
    v = gb.Vector.from_coo(lit["idx"], lit["vals"], size=lit["size"])
    w7 = gb.Vector.from_coo(seq["w7"]["idx"], seq["w7"]["vals"], size=lit["size"])
    res = seq["result"]
    assert_vec(v.select(w7.S).new(), [1, 3, 4], [1, 1, 2], "structural mask")
    assert_vec(v.select(gb.Vector.from_coo(res["idx"], res["vals"], size=lit["size"]).S).new(), res["idx"], res["vals"], "w8")
    w9 = v.select(w7.V).new()
    assert_vec(w9, res["idx"], res["vals"], "w9")
    with pytest.raises(TypeError, match="thunk"):
        v.select(w7.V, 777)
    with pytest.raises(TypeError):
        v.select(gb.Matrix(int, 7, 7).S)
    # replace is used
    w9 << 1
    w9 << v.select(w7.V)
    assert_vec(w9, res["idx"], res["vals"], "replace")
    # ... and with masks
    w9 << 1
    w9[1] = 0
    w9(w9.V) << v.select(w7.V)
    assert_vec(w9, seq["result2"]["idx"], seq["result2"]["vals"], "result2")
    w9 << 1
    w9[1] = 0
    w9(w9.V, replace=True) << v.select(w7.V)
    assert_vec(w9, seq["result2_replace"]["idx"], seq["result2_replace"]["vals"], "result2 with replace")
    w9 << 1
    w9[1] = 0
    w9(w9.V, gb.binary.plus) << v.select(w7.V)
    w8 = gb.Vector(v.dtype, v.size)
    w8 << 1
    w8[1] = 0
    w8(w8.V, gb.binary.plus) << v.dup(mask=w7.V)
    assert w8.isequal(w9)
    assert_vec(w9, seq["masked_plus"]["idx"], seq["masked_plus"]["vals"], "mask + accum")
    w9 << 1
    w9(gb.binary.plus) << v.select(w7.V)
    w8 << 1
    w8(gb.binary.plus) << v.dup(mask=w7.V)
    assert w8.isequal(w9)
    assert_vec(w9, seq["plus"]["idx"], seq["plus"]["vals"], "accum")


def test_matrix_mask_select_and_strings(gb, literals):
    lit = literals["matrix"]
    A = gb.Matrix.from_coo(lit["rows"], lit["cols"], lit["vals"], nrows=7, ncols=7)
    M = gb.Matrix.from_coo([0, 3, 6, 2], [3, 0, 4, 2], [1, 0, 1, 1], nrows=7, ncols=7)
    assert_coo(A.select(M.S).new(), [0, 3, 6], [3, 0, 4], [3, 3, 3], "M.S")
    assert_coo(A.select(M.V).new(), [0, 6], [3, 4], [3, 3], "M.V")
    with pytest.raises(TypeError, match="thunk"):
        A.select(M.S, 1)
    with pytest.raises(ValueError):
        A.select("no such operator")
    with pytest.raises(TypeError):
        A.select(gb.binary.plus, 1)
    with pytest.raises(TypeError):
        A(accum=gb.select.tril)
    # a Scalar thunk goes through the _Scalar entry point; an empty one is the library's GrB_EMPTY_OBJECT
    calls = []
    gb.record_calls(calls)
    try:
        C = A.select(">=", gb.Scalar.from_value(7)).new()
    finally:
        gb.record_calls(None)
    assert any(c.startswith("GrB_Matrix_select_Scalar(") for c in calls), calls
    assert_coo(C, [6, 1, 4], [3, 4, 5], [7, 8, 7], ">= Scalar(7)")
    with pytest.raises(gb.exceptions.EmptyObject):
        A.select(">=", gb.Scalar(int)).new()
    # offdiag / diag / tril with a thunk, transposed input (descriptor T0)
    r, c, x = (np.asarray(lit[k]) for k in ("rows", "cols", "vals"))
    keep = r <= c - 2  # (A.T)(i, j) = A(j, i): tril(A.T, -2) keeps i' - 2 >= j', i.e. col - 2 >= row of A
    assert_coo(A.T.select(gb.select.tril, -2).new(), c[keep], r[keep], x[keep], "T0")
    assert A.select("offdiag").new().isequal(A) and A.select("diag").new().nvals == 0


# ---- 2. seeded random parity against numpy ------------------------------------------------------------------------------------
def np_keep(op, r, c, vals, thunk):
    """The boolean filter of a select operator over COO tuples, restated with numpy."""
    if op in POSITIONAL:
        k = int(np.int64(thunk)) if not isinstance(thunk, int) else thunk
        i, j = r.astype(object), c.astype(object)  # (python integers: no i + k can overflow)
        keep = {"tril": lambda: j <= i + k, "triu": lambda: j >= i + k, "diag": lambda: j == i + k, "offdiag": lambda: j != i + k,
                "colle": lambda: j <= k, "colgt": lambda: j > k, "rowle": lambda: i <= k, "rowgt": lambda: i > k}[op]()
        return np.asarray(keep, bool).reshape(r.shape)
    ot = np.promote_types(vals.dtype, np.asarray(thunk).dtype)  # entry and thunk are compared in unify(A.dtype, thunk dtype)
    with np.errstate(all="ignore"):
        a, y = vals.astype(ot), np.asarray(thunk).astype(ot)
        return {"valueeq": a == y, "valuene": a != y, "valuegt": a > y, "valuege": a >= y, "valuelt": a < y, "valuele": a <= y}[op]


def np_accum(name, tname, c, t):
    with np.errstate(all="ignore"):
        if tname == "BOOL":
            return np.logical_or(c, t) if name == "plus" else np.logical_and(c, t)
        if name == "plus":
            return (c + t).astype(c.dtype)
        return np.fmin(c, t) if c.dtype.kind == "f" else np.minimum(c, t)


def np_write_rule(shape, tname, C, T, M, structural, comp, replace, accum):
    """C<M, replace> = accum(C, T), dense: C, T, M are (rows, cols, vals) or None.  Returns (rows, cols, vals) row-major."""
    np_t = NP_OF[tname]

    def dense(coo, dt):
        has, val = np.zeros(shape, bool), np.zeros(shape, dt)
        if coo is not None and len(coo[0]):
            has[coo[0], coo[1]] = True
            val[coo[0], coo[1]] = coo[2]
        return has, val

    c_has, c_val = dense(C, np_t)
    t_has, t_val = dense(T, np_t)
    if accum is None:
        z_has, z_val = t_has, t_val
    else:
        z_has = c_has | t_has
        z_val = np.where(c_has & t_has, np_accum(accum, tname, c_val, t_val), np.where(c_has, c_val, t_val))
    if M is None:
        allow = np.ones(shape, bool)
    else:
        m_has, m_val = dense(M, np.asarray(M[2]).dtype)
        allow = m_has if structural else (m_has & (m_val != 0))
        if comp:
            allow = ~allow
    out_has = np.where(allow, z_has, False if replace else c_has)
    out_val = np.where(allow, z_val, c_val)
    rr, cc = np.nonzero(out_has)
    return rr, cc, out_val[rr, cc]


def draw_matrix(rng, seed, tname):
    """Shapes: empty, 1 x n, n x 1, a hub row longer than 8192 entries (not a multiple of 64), ragged rows with empty ones."""
    kind = seed % 9
    iso = seed % 6 == 4
    if iso:
        kind = 3  # (an iso matrix needs entries: never one of the empty / single-entry shapes)
    if seed % 6 == 5:  # the hub: block seams of the flag pass, WR_LONG of the write rule
        m, n = 6, 9001
        deg = np.array([3, 0, 8192 + 45, 70, 0, 1])
    elif kind == 0:
        m, n = int(rng.integers(1, 40)), int(rng.integers(1, 40))
        deg = np.zeros(m, np.int64)
    elif kind == 1:
        m, n = 1, int(rng.integers(1, 300))
        deg = np.array([rng.integers(0, n + 1)])
    elif kind == 2:
        m, n = int(rng.integers(1, 300)), 1
        deg = rng.integers(0, 2, m)
    else:
        m, n = int(rng.integers(2, 260)), int(rng.integers(2, 260))
        deg = rng.integers(0, 9, m)
        deg[rng.random(m) < 0.3] = 0
        deg[rng.integers(0, m)] = rng.integers(n // 2, n + 1)
        deg = np.minimum(deg, n)
    rows = np.repeat(np.arange(m), deg)
    cols = np.concatenate([np.sort(rng.choice(n, d, replace=False)) for d in deg]) if deg.sum() else np.zeros(0, np.int64)
    if tname.startswith("FP"):
        vals = rand_vals(rng, rows.size, tname, "exact")  # integers -8..8 with NaN, +-inf and +-0.0 among them
    else:
        vals = rand_vals(rng, rows.size, tname)
    if iso:
        vals = np.full(rows.size, vals[0])
    return m, n, rows.astype(np.int64), cols.astype(np.int64), vals, iso


def stored_iso(A):
    """Whether the library keeps ONE value for every entry of A (GrX_Matrix_export_CSR_device reports the stored form)."""
    from graphblas_amd import _lib

    dp, dj, dx, nv, iso = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    assert _lib.lib.GrX_Matrix_export_CSR_device(ctypes.byref(dp), ctypes.byref(dj), ctypes.byref(dx), ctypes.byref(nv), ctypes.byref(iso), A._carg) == 0
    return bool(iso.value)


def draw_coo(rng, m, n, tname, dens):
    has = rng.random((m, n)) < dens if m * n <= 70000 else np.zeros((m, n), bool)
    if m * n > 70000:
        has[rng.integers(0, m, 6000), rng.integers(0, n, 6000)] = True
        has[2, ::2] = True  # (a long row of the mask / of C against the hub)
    r, c = np.nonzero(has)
    return r, c, rand_vals(rng, r.size, tname)


def thunk_for(rng, seed, opi, op, tname, vals, m, n):
    if op in POSITIONAL:
        span = max(m, n)
        ks = [-3, -1, 0, 1, 2, span + 3, -(span + 3), 1 << 40, -(1 << 40), int(rng.integers(-span, span + 1))]
        return ks[(seed + opi) % len(ks)]
    np_t = NP_OF[tname]
    pick = (seed + opi) % 4
    if pick == 0 and vals.size:  # a value of the matrix, in the matrix's type
        return vals[rng.integers(0, vals.size)]
    if pick == 1:
        return np_t(np.nan) if tname.startswith("FP") else np_t(0)
    if pick == 2:
        return 3  # a Python int: the comparison runs in unify(A.dtype, INT64)
    return np_t(-0.0) if tname.startswith("FP") else (np_t(1) if tname != "BOOL" else np.bool_(False))


@pytest.mark.parametrize("seed", range(28))
def test_select_random(gb, seed):
    """All 14 operators per seed; thunks with negatives, 0, +-(n + 3), +-2^40; T0; mask in {none, value, structural} x complement x
    replace; accum in {none, plus, min}; C aliasing A; an output type that differs from the input's; empty, 1 x n, n x 1 matrices; the
    hub row; iso input.  No case is skipped: every (seed, operator) pair is compared."""
    rng = np.random.default_rng(7700 + seed)
    tname = TYPES[seed % 7]
    m, n, rows, cols, vals, iso = draw_matrix(rng, seed, tname)
    if iso:  # an iso matrix by construction: one value handed over with is_iso
        assert rows.size > 1
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m))])
        A = gb.Matrix.ss.import_csr(nrows=m, ncols=n, indptr=indptr, values=vals[:1], col_indices=cols, is_iso=True, sorted_cols=True, dtype=tname)
        assert stored_iso(A) and A.nvals == rows.size
    else:
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
    compared = 0
    for opi, op in enumerate(OPS):
        cfg = seed * len(OPS) + opi
        t0 = (cfg // 5) % 2 == 1
        mask_kind = cfg % 3  # 0 none, 1 value, 2 structural
        comp, repl = (cfg // 3) % 2 == 1, (cfg // 6) % 2 == 1
        accum = [None, "plus", "min"][(cfg // 2) % 3]
        om, on = (n, m) if t0 else (m, n)
        alias = cfg % 7 == 0 and om == m and on == n
        ctype = OTHER_TYPE[tname] if (cfg % 5 == 1 and not alias) else tname
        thunk = thunk_for(rng, seed, opi, op, tname, vals, om, on)
        sr, sc = (cols, rows) if t0 else (rows, cols)
        keep = np_keep(op, sr, sc, vals, thunk)
        with np.errstate(all="ignore"):
            T = (sr[keep], sc[keep], vals[keep].astype(NP_OF[ctype]))
        if alias:
            Cc = (rows, cols, vals)
            C = A.dup()
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
        C(**kw) << (src.T if t0 else src).select(op, thunk)
        er, ec, ev = np_write_rule((om, on), ctype, Cc, T, Mc, mask_kind == 2, comp and mask_kind > 0, repl and mask_kind > 0, accum)
        where = f"seed {seed} {op} thunk {thunk!r} {tname}->{ctype} t0={t0} mask={mask_kind} comp={comp} repl={repl} accum={accum} alias={alias}"
        I, J, X = C.to_coo()
        assert I.tolist() == er.tolist() and J.tolist() == ec.tolist(), where
        assert X.dtype == ev.dtype, where
        if ev.dtype.kind == "f":
            same_fp(X, ev, "min" if accum == "min" else None, where)
        else:
            assert X.tolist() == ev.tolist(), where
        compared += 1
    assert compared == len(OPS)


@pytest.mark.parametrize("seed", range(12))
def test_vector_select_random(gb, seed):
    rng = np.random.default_rng(8800 + seed)
    tname = TYPES[seed % 7]
    n = [1, 63, 64, 65, 700, 4100][seed % 6]
    idx = np.flatnonzero(rng.random(n) < [0.0, 0.5, 1.0][seed % 3])
    vals = rand_vals(rng, idx.size, tname, "exact") if tname.startswith("FP") else rand_vals(rng, idx.size, tname)
    u = gb.Vector.from_coo(idx, vals, dtype=tname, size=n)
    for opi, op in enumerate(OPS):
        cfg = seed * len(OPS) + opi
        mask_kind, comp, repl = cfg % 3, (cfg // 3) % 2 == 1, (cfg // 6) % 2 == 1
        accum = [None, "plus", "min"][(cfg // 2) % 3]
        alias = cfg % 7 == 0
        ctype = OTHER_TYPE[tname] if (cfg % 5 == 1 and not alias) else tname
        thunk = thunk_for(rng, seed, opi, op, tname, vals, n, 1)
        keep = np_keep(op, idx, np.zeros_like(idx), vals, thunk)
        zero = np.zeros(int(keep.sum()), np.int64)
        with np.errstate(all="ignore"):
            T = (idx[keep], zero, vals[keep].astype(NP_OF[ctype]))
        if alias:
            Cc = (idx, np.zeros_like(idx), vals)
            w = u.dup()
            src = w
        else:
            ci = np.flatnonzero(rng.random(n) < 0.4)
            Cc = (ci, np.zeros_like(ci), rand_vals(rng, ci.size, ctype))
            w = gb.Vector.from_coo(ci, Cc[2], dtype=ctype, size=n)
            src = u
        Mc = None
        kw = {}
        if mask_kind:
            mi = np.flatnonzero(rng.random(n) < 0.5)
            Mc = (mi, np.zeros_like(mi), rand_vals(rng, mi.size, "INT8"))
            mk = gb.Vector.from_coo(mi, Mc[2], dtype="INT8", size=n)
            mm = mk.S if mask_kind == 2 else mk.V
            kw = dict(mask=~mm if comp else mm, replace=repl)
        if accum:
            kw["accum"] = accum
        w(**kw) << src.select(op, thunk)
        er, _, ev = np_write_rule((n, 1), ctype, Cc, T, Mc, mask_kind == 2, comp and mask_kind > 0, repl and mask_kind > 0, accum)
        where = f"seed {seed} {op} thunk {thunk!r} {tname}->{ctype} mask={mask_kind} comp={comp} repl={repl} accum={accum} alias={alias}"
        I, X = w.to_coo()
        assert I.tolist() == er.tolist(), where
        assert X.dtype == ev.dtype, where
        if ev.dtype.kind == "f":
            same_fp(X, ev, "min" if accum == "min" else None, where)
        else:
            assert X.tolist() == ev.tolist(), where


# ---- 3. the C ABI directly ------------------------------------------------------------------------------------------------
def _handle(L, name):
    return ctypes.c_void_p(ctypes.c_void_p.in_dll(L, name).value)


def _matrix_error(L, C):
    s = ctypes.c_char_p()
    L.GrB_Matrix_error(ctypes.byref(s), C._carg)
    return (s.value or b"").decode()


def test_c_abi(gb, literals):
    from graphblas_amd import _lib, device

    L = _lib.lib
    lit = literals["matrix"]
    r, c, x = (np.asarray(lit[k]) for k in ("rows", "cols", "vals"))
    A = gb.Matrix.from_coo(r, c, x, nrows=7, ncols=7)
    # python-graphblas's default thunk: GrB_Matrix_select_BOOL with a positional operator and y = false
    C = gb.Matrix(int, 7, 7)
    assert L.GrB_Matrix_select_BOOL(C._carg, None, None, _handle(L, "GrB_TRIL"), A._carg, False, None) == 0
    assert_coo(C, r[c <= r], c[c <= r], x[c <= r], "GrB_TRIL, false")
    flag_launches = device.last_stats()["kernel_launches"]
    assert flag_launches > 0
    # the ROWLE short cut: a slice of the row pointers, no flag pass
    assert L.GrB_Matrix_select_INT64(C._carg, None, None, _handle(L, "GrB_ROWLE"), A._carg, 2, None) == 0
    assert_coo(C, r[r <= 2], c[r <= 2], x[r <= 2], "GrB_ROWLE, 2")
    assert 0 < device.last_stats()["kernel_launches"] < flag_launches
    # every typed entry point takes every operator: y is cast to the operator's thunk type
    assert L.GrB_Matrix_select_FP64(C._carg, None, None, _handle(L, "GrB_VALUEGE_INT64"), A._carg, 7.0, None) == 0
    assert_coo(C, r[x >= 7], c[x >= 7], x[x >= 7], "GrB_VALUEGE_INT64, 7.0")
    assert L.GrB_Matrix_select_INT8(C._carg, None, None, _handle(L, "GrB_VALUELT_FP32"), A._carg, 3, None) == 0
    assert_coo(C, r[x < 3], c[x < 3], x[x < 3], "GrB_VALUELT_FP32, 3")
    # the _Scalar forms
    L.GrB_Scalar_setElement_INT64.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    s = ctypes.c_void_p()
    assert L.GrB_Scalar_new(ctypes.byref(s), _handle(L, "GrB_INT64")) == 0
    try:
        assert L.GrB_Matrix_select_Scalar(C._carg, None, None, _handle(L, "GrB_TRIU"), A._carg, s, None) == -106  # GrB_EMPTY_OBJECT
        assert "empty" in _matrix_error(L, C)
        v = gb.Vector.from_coo([1, 3, 4, 6], [1, 1, 2, 0], size=7)
        w = gb.Vector(int, 7)
        assert L.GrB_Vector_select_Scalar(w._carg, None, None, _handle(L, "GrB_ROWGT"), v._carg, s, None) == -106
        assert L.GrB_Scalar_setElement_INT64(s, 3) == 0
        assert L.GrB_Matrix_select_Scalar(C._carg, None, None, _handle(L, "GrB_COLGT"), A._carg, s, None) == 0
        assert_coo(C, r[c > 3], c[c > 3], x[c > 3], "GrB_COLGT, Scalar 3")
        assert L.GrB_Vector_select_Scalar(w._carg, None, None, _handle(L, "GrB_ROWGT"), v._carg, s, None) == 0
        assert_vec(w, [4, 6], [2, 0], "GrB_ROWGT, Scalar 3")
        assert L.GrB_Vector_select_INT64(w._carg, None, None, _handle(L, "GrB_VALUEEQ_INT64"), v._carg, 1, None) == 0
        assert_vec(w, [1, 3], [1, 1], "GrB_VALUEEQ_INT64, 1")
    finally:
        L.GrB_Scalar_free(ctypes.byref(s))
    # apply operators do not return BOOL
    assert L.GrB_Matrix_select_INT64(C._carg, None, None, _handle(L, "GrB_ROWINDEX_INT64"), A._carg, 0, None) == -5  # GrB_DOMAIN_MISMATCH
    assert "BOOL" in _matrix_error(L, C)
    # shapes, with T0 taken into account
    B = gb.Matrix.from_coo([0, 2], [1, 4], [1, 2], nrows=3, ncols=5)
    D = gb.Matrix(int, 3, 5)
    assert L.GrB_Matrix_select_INT64(C._carg, None, None, _handle(L, "GrB_TRIL"), B._carg, 0, None) == -6  # GrB_DIMENSION_MISMATCH
    assert "7 x 7" in _matrix_error(L, C) and "3 x 5" in _matrix_error(L, C)
    assert L.GrB_Matrix_select_INT64(D._carg, None, None, _handle(L, "GrB_TRIL"), B._carg, 0, _handle(L, "GrB_DESC_T0")) == -6
    assert L.GrB_Matrix_select_INT64(D._carg, A._carg, None, _handle(L, "GrB_TRIL"), B._carg, 0, None) == -6
    assert "mask" in _matrix_error(L, D)
    assert L.GrB_Matrix_select_INT64(D._carg, None, None, _handle(L, "GrB_TRIL"), B._carg, 5, _handle(L, "GrB_DESC_T1")) == 0  # (T1 is ignored)
    assert_coo(D, [0, 2], [1, 4], [1, 2], "T1")
    assert L.GrB_Matrix_select_INT64(D._carg, None, _handle(L, "GrB_PLUS_FP32"), _handle(L, "GrB_TRIL"), B._carg, 5, None) == -5
    assert L.GrB_Matrix_select_INT64(None, None, None, _handle(L, "GrB_TRIL"), B._carg, 5, None) == -2  # GrB_NULL_POINTER
    assert L.GrB_Matrix_select_INT64(D._carg, None, None, None, B._carg, 5, None) == -2
    # a complemented absent mask writes nothing
    assert L.GrB_Matrix_select_INT64(D._carg, None, None, _handle(L, "GrB_DIAG"), B._carg, 0, _handle(L, "GrB_DESC_C")) == 0
    assert_coo(D, [0, 2], [1, 4], [1, 2], "complemented absent mask")


# ---- 4. triangle counting end to end -----------------------------------------------------------------------------------------
def _symmetric_rmat(gb, scale):
    import scipy.sparse as sp

    from graphblas_amd import synthetic

    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, device="cpu")
    G = sp.csr_matrix((np.ones(col.numel(), np.int64), col.numpy().astype(np.int64), ip.numpy()), shape=(n, n))
    G = ((G + G.T) > 0).astype(np.int64).tocsr()  # symmetrised; the self-loops stay in for select("offdiag") to remove
    G.sort_indices()
    return n, G


def _triangles(gb, scale, want_entries=None, want_triangles=None):
    import scipy.sparse as sp

    n, G = _symmetric_rmat(gb, scale)
    S0 = gb.Matrix.from_csr(G.indptr, G.indices, G.data, dtype="INT64", ncols=n)
    S = S0.select("offdiag").new()
    Ssp = (G - sp.diags(G.diagonal(), dtype=np.int64, format="csr")).tocsr()
    Ssp.eliminate_zeros()
    L = S.select("tril", -1).new()
    Lsp = sp.tril(Ssp, -1, format="csr")
    Lsp.sort_indices()
    Lp, Lj, Lx = L.to_csr()
    assert np.array_equal(Lp.astype(np.int64), Lsp.indptr) and np.array_equal(Lj.astype(np.int64), Lsp.indices)
    assert np.array_equal(Lx, Lsp.data)
    C = gb.Matrix("INT64", n, n)
    C(L.S) << L.mxm(L.T, gb.semiring.plus_pair)
    got = C.reduce_scalar("plus").new().value
    want = int((Lsp @ Lsp.T).multiply(Lsp).sum())
    print(f"scale {scale}: {L.nvals} entries in L, longest row {int(np.diff(Lsp.indptr).max())}, {got} triangles")
    assert got == want
    if want_entries is not None:
        assert (L.nvals, got) == (want_entries, want_triangles)


def test_triangle_count_emu():
    gb = bind("emu")
    _triangles(gb, 10, 10438, 75630)


@pytest.mark.gpu
def test_triangle_count_gpu():
    gb = bind("gpu")
    _triangles(gb, 16, 909612, 15691680)


@pytest.mark.gpu
def test_select_scale20_gpu():
    """select alone at scale 20 against scipy.sparse.tril / triu, and a >= threshold on the U{1..255} weights."""
    import scipy.sparse as sp

    from graphblas_amd import synthetic

    gb = bind("gpu")
    scale = 20
    n = 1 << scale
    ip, col = synthetic.rmat_csr(scale, device="cpu")
    w = synthetic.edge_weights(col, scale).numpy()
    G = sp.csr_matrix((w, col.numpy().astype(np.int64), ip.numpy()), shape=(n, n))
    A = gb.Matrix.from_csr(G.indptr, G.indices, G.data, dtype="FP32", ncols=n)
    for name, k, ref in (("tril", -1, sp.tril(G, -1, format="csr")), ("triu", 1, sp.triu(G, 1, format="csr")), ("tril", 0, sp.tril(G, 0, format="csr"))):
        ref.sort_indices()
        Cp, Cj, Cx = A.select(name, k).new().to_csr()
        assert np.array_equal(Cp.astype(np.int64), ref.indptr) and np.array_equal(Cj.astype(np.int64), ref.indices), (name, k)
        assert np.array_equal(Cx, ref.data), (name, k)
    thr = np.float32(128)
    keep = G.data >= thr
    rows = np.repeat(np.arange(n), np.diff(G.indptr))
    Cp, Cj, Cx = A.select(">=", thr).new().to_csr()
    assert np.array_equal(Cp.astype(np.int64), np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]))
    assert np.array_equal(Cj.astype(np.int64), G.indices[keep]) and np.array_equal(Cx, G.data[keep])


# ---- 5. no growth ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_no_growth():
    """200 selects per cycle (flag-pass and short-cut forms, with and without a mask) on one matrix, results freed.  The library keeps
    freed blocks in its size-class cache, so the first cycle may grow; free device memory after cycle 2 against after cycle 3."""
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
            for expr, mask in ((A.select("tril", -1), None), (A.select(">=", 100.0), M.S), (A.select("rowle", n // 2), None),
                               (A.select("colgt", k), M.V)):
                r = expr.new(mask=mask) if mask is not None else expr.new()
                del r

    cycle()
    cycle()
    after2 = free_bytes()
    cycle()
    after3 = free_bytes()
    print(f"free after cycle 2: {after2 / 2**20:.1f} MiB, after cycle 3: {after3 / 2**20:.1f} MiB")
    assert after3 >= after2, (after2, after3)
