"""The positional semirings of mxv / vxm (python-graphblas_amd/csrc/grb_mxv_posn.hip): GxB_{MIN,MAX,ANY,PLUS}_
{FIRSTI,FIRSTI1,FIRSTJ,FIRSTJ1,SECONDI,SECONDI1,SECONDJ,SECONDJ1}_{INT32,INT64}.

The reference is a numpy restatement written here (the oracle has no positional operator): per output index o the set
K(o) = row(o) of the matrix AS MULTIPLIED (after T0 / T1)  intersected with  pattern(u); then the index rule
    mxv (w = M u):    firsti = o   firstj = secondi = k   secondj = 0
    vxm (w' = u' M):  firsti = 0   firstj = secondi = k   secondj = o          (the ...1 forms one more)
in int64, the monoid over k in K(o) in the semiring's type (PLUS wraps), the cast to w's type by the library's cast_value (integer to
integer keeps the low bits, to FP64 is exact here), and the write rule.  min / max / plus are compared for exact equality of pattern
and values; any_* for the exact pattern and membership of every value in the admissible set.

The reference project's own tests hold no literal mxv / vxm case for these operators (its only uses are a Vector @ Vector inner product
and an element-wise call, graphblas/tests/test_vector.py:2123-2126, both outside what is implemented here), so there is no
tests/golden/positional_literals.json.

Witnesses (GrX_last_stats): method 25 = the pull kernel, 26 = the push kernel, 6 = an operand without entries; tiles = wavefront units:
the pull kernel gives a row a lane group of G = 4 / 8 / 16 / 64 lanes for nnz // nrows <= 4 / 8 / 16 / above, so tiles = ceil(m G / 64)."""
import ctypes

import numpy as np
import pytest

from tests.backend import DEVICES, bind

OPS = ("firsti", "firsti1", "firstj", "firstj1", "secondi", "secondi1", "secondj", "secondj1")
MONOIDS = ("min", "max", "plus", "any")
NP = {"INT32": np.int32, "INT64": np.int64, "FP64": np.float64, "INT8": np.int8}
PULL, PUSH, EMPTY = 25, 26, 6


@pytest.fixture(params=DEVICES)
def gb(request):
    g = bind(request.param)
    yield g
    _opts(())  # (every test leaves the option table as it found it)


def _opts(opts):
    from graphblas_amd import _lib

    assert _lib.lib.GrX_options_reset() == 0
    for name, val in opts:
        assert _lib.lib.GrX_option_set(name, val) == 0, name


def _stats():
    from graphblas_amd import device

    return device.last_stats()


# ---- the numpy restatement ------------------------------------------------------------------------------------------------------
def ref_product(M, u_has, vxm, op, tname):
    """Per output: the list of candidate values (int64), in rising k.  M: dense bool pattern of the matrix as multiplied."""
    off = 1 if op.endswith("1") else 0
    base = op.rstrip("1")
    n_out = M.shape[1] if vxm else M.shape[0]
    out = []
    for o in range(n_out):
        line = M[:, o] if vxm else M[o, :]
        ks = np.flatnonzero(line & u_has).astype(np.int64)
        if base in ("firstj", "secondi"):
            z = ks
        elif (base == "firsti") != vxm:  # firsti of mxv / secondj of vxm: the output index
            z = np.full(ks.size, o, np.int64)
        else:
            z = np.zeros(ks.size, np.int64)
        out.append(z + off)
    return out


def ref_fold(cands, monoid, tname):
    """(has, val) of T in the semiring's type for min / max / plus."""
    t = NP[tname]
    has = np.array([c.size > 0 for c in cands])
    val = np.zeros(len(cands), t)
    for o, c in enumerate(cands):
        if c.size:
            c = c.astype(t)
            val[o] = c.min() if monoid == "min" else (c.max() if monoid == "max" else c.sum(dtype=t))
    return has, val


def ref_write(w_has, w_val, t_has, t_val, allow, replace, accum):
    """w<allow, replace> = accum(w, t); allow = None: no mask; t already in w's type."""
    if accum is None:
        z_has, z_val = t_has, t_val
    else:
        z_has = w_has | t_has
        z_val = np.where(w_has & t_has, accum(w_val, t_val), np.where(t_has, t_val, w_val))
    if allow is None:
        return z_has, z_val
    return np.where(allow, z_has, False if replace else w_has), np.where(allow, z_val, w_val)


def vec(gb, has, val=None, dtype="INT64"):
    idx = np.flatnonzero(has)
    vals = np.ones(idx.size, NP.get(dtype, np.int64)) if val is None else np.asarray(val)[idx]
    return gb.Vector.from_coo(idx, vals, dtype=dtype, size=len(has))


def check_exact(w, has, val, where=""):
    gi, gv = w.to_coo()
    assert gi.tolist() == np.flatnonzero(has).tolist(), (where, gi, np.flatnonzero(has))
    assert gv.tolist() == np.asarray(val)[has].tolist(), (where, gv, np.asarray(val)[has])


def check_any(w, cands, tname, where=""):
    gi, gv = w.to_coo()
    assert gi.tolist() == [o for o, c in enumerate(cands) if c.size], (where, gi)
    for o, v in zip(gi.tolist(), gv.tolist()):
        assert v in cands[o].astype(NP[tname]).tolist(), (where, o, v, cands[o])


def matrix_of(gb, M, dtype="INT64"):
    r, c = np.nonzero(M)
    return gb.Matrix.from_coo(r, c, np.arange(1, r.size + 1), dtype=dtype, nrows=M.shape[0], ncols=M.shape[1])


def product(gb, A, u, vxm, tr, sr):
    """The delayed expression of one of the four orientations."""
    if vxm:
        return u.vxm(A.T if tr else A, sr)
    return (A.T if tr else A).mxv(u, sr)


# ---- 1. the semantics table -----------------------------------------------------------------------------------------------------
LIT = np.zeros((7, 5), bool)  # 7 x 5: i, k, j and 0 cannot be confused
for _i, _j in ((0, 1), (0, 3), (1, 0), (1, 1), (1, 4), (2, 2), (3, 0), (3, 3), (3, 4), (5, 1), (5, 2), (5, 3), (6, 4), (6, 0)):
    LIT[_i, _j] = True


@pytest.mark.parametrize("mode", ["mxv", "vxm", "mxv_T0", "vxm_T1"])
@pytest.mark.parametrize("tname", ["INT32", "INT64"])
def test_semantics_table(gb, tname, mode):
    vxm, tr = mode.startswith("vxm"), "_T" in mode
    A = matrix_of(gb, LIT)
    Mm = LIT.T if tr else LIT                      # the matrix as multiplied
    n_in = Mm.shape[0] if vxm else Mm.shape[1]
    u_has = np.zeros(n_in, bool)
    u_has[[0, 3, 4] if n_in == 5 else [1, 3, 6]] = True  # 3 entries
    u = vec(gb, u_has)
    for push_mode in (0, 2):
        _opts(((b"push_mode", push_mode),))
        for op in OPS:
            cands = ref_product(Mm, u_has, vxm, op, tname)
            for mon in MONOIDS:
                sr = getattr(gb.semiring, f"{mon}_{op}")[tname]
                w = product(gb, A, u, vxm, tr, sr).new()
                assert w.dtype.name == tname and _stats()["method"] in (PULL, PUSH)
                if mon == "any":
                    check_any(w, cands, tname, (mode, op, push_mode))
                else:
                    check_exact(w, *ref_fold(cands, mon, tname), (mode, mon, op, push_mode))


def test_spellings_and_types(gb):
    A = matrix_of(gb, LIT, dtype="FP32")
    q_has = np.zeros(7, bool)
    q_has[[1, 3, 6]] = True
    q = vec(gb, q_has, dtype="INT32")
    cands = ref_product(LIT, q_has, True, "secondi", "INT64")
    exp = ref_fold(cands, "min", "INT64")
    forms = [q.vxm(A, gb.semiring.min_secondi), gb.semiring.min_secondi(q @ A), q.vxm(A, "min_secondi"), q.vxm(A, gb.op.min_secondi)]
    for k, expr in enumerate(forms):
        w = expr.new()
        assert w.dtype.name == "INT64", k  # INT64 whatever the operands' dtypes are
        check_exact(w, *exp, k)
    assert q.vxm(A, gb.semiring.min_secondi["INT32"]).new().dtype.name == "INT32"
    assert gb.binary.firsti["FP32"].type.name == "INT64" and gb.binary.secondj1["INT32"].type.name == "INT32"
    assert gb.op.firstj is gb.binary.firstj
    for op in OPS:
        assert not hasattr(gb.semiring, f"times_{op}")
        for mon in MONOIDS:
            assert getattr(gb.op, f"{mon}_{op}") is getattr(gb.semiring, f"{mon}_{op}")
    u_has = np.array([True, False, False, True, True])
    check_exact(A.mxv(vec(gb, u_has), gb.semiring.min_firstj).new(), *ref_fold(ref_product(LIT, u_has, False, "firstj", "INT64"), "min", "INT64"))


# ---- 2. pull: chunk limits, lane groups ---------------------------------------------------------------------------------------------
LENS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
WHICH = ("first", "64th", "65th", "last", "none")


def _rows_matrix(m_total):
    """45 rows (every length x every choice of the operand's one column), each over a column block of its own with gaps, spread over
    m_total rows (the others empty).  Returns (row lists, u_has, ncols, row numbers)."""
    step = max(1, m_total // 45)
    rows, marks, base = {}, [], 0
    for n, (ln, which) in enumerate((ln, wh) for wh in WHICH for ln in LENS):
        cols = base + 2 * np.arange(ln) + (n % 2)
        pick = {"first": 0, "64th": 63, "65th": 64, "last": ln - 1, "none": -1}[which]
        if 0 <= pick < ln:
            marks.append(int(cols[pick]))
        rows[n * step] = cols
        base += 2 * 200 + 2
    u_has = np.zeros(base, bool)
    u_has[marks] = True
    return rows, u_has, base


@pytest.mark.parametrize("G,m_total", [(4, 800), (8, 450), (16, 240), (64, 45)])
def test_pull_chunk_limits(gb, G, m_total):
    rows, u_one, ncols = _rows_matrix(m_total)
    r = np.concatenate([np.full(c.size, i) for i, c in rows.items()])
    c = np.concatenate(list(rows.values()))
    A = gb.Matrix.from_coo(r, c, np.ones(r.size, np.int64), dtype="INT64", nrows=m_total, ncols=ncols)
    nnz = r.size
    assert {4: nnz // m_total <= 4, 8: 4 < nnz // m_total <= 8, 16: 8 < nnz // m_total <= 16, 64: nnz // m_total > 16}[G]
    _opts(((b"push_mode", 0),))
    every_second = np.arange(m_total) % 2 == 0
    vmask_val = np.ones(m_total, bool)
    vmask_val[::3] = False  # a value mask holding false entries
    for u_has in (u_one, np.ones(ncols, bool)):  # one column per row; a full operand
        cands = [np.zeros(0, np.int64)] * m_total
        for i, cols in rows.items():
            cands[i] = cols[u_has[cols]].astype(np.int64)
        u = vec(gb, u_has)
        for mon in MONOIDS:
            sr = getattr(gb.semiring, f"{mon}_secondi")
            w = A.mxv(u, sr).new()
            st = _stats()
            assert st["method"] == PULL and st["tiles"] == -(-m_total * G // 64) and st["flops"] == nnz, st
            t_has, t_val = ref_fold(cands, "min" if mon == "any" else mon, "INT64")
            if mon == "any":
                check_any(w, cands, "INT64", (G, "any"))
                continue
            check_exact(w, t_has, t_val, (G, mon))
            # a complemented structural mask that excludes every second row, with replace, over old content
            w_has, w_val = np.ones(m_total, bool), np.full(m_total, -7, np.int64)
            w = vec(gb, w_has, w_val)
            mk = vec(gb, every_second, dtype="BOOL")
            w(~mk.S, replace=True) << A.mxv(u, sr)
            check_exact(w, *ref_write(w_has, w_val, t_has, t_val, ~every_second, True, None), (G, mon, "comp mask"))
            # a value mask with false entries, no replace
            w = vec(gb, w_has, w_val)
            mv = gb.Vector.from_coo(np.arange(m_total), vmask_val, dtype="BOOL", size=m_total)
            w(mv.V) << A.mxv(u, sr)
            check_exact(w, *ref_write(w_has, w_val, t_has, t_val, vmask_val, False, None), (G, mon, "value mask"))


CYCLES = {4: (0, 1, 3, 4, 5, 7), 8: (5, 8, 9, 0, 12, 7), 16: (16, 17, 1, 15, 20, 9), 64: (64, 65, 1, 30, 100)}


@pytest.mark.parametrize("G", [4, 8, 16, 64])
@pytest.mark.parametrize("m", [63, 64, 65, 257])
def test_pull_short_last_group(gb, m, G):
    rng = np.random.default_rng(100 * G + m)
    ncols = 300
    M = np.zeros((m, ncols), bool)
    for i in range(m):
        M[i, rng.choice(ncols, CYCLES[G][i % len(CYCLES[G])], replace=False)] = True
    A = matrix_of(gb, M)
    u_has = rng.random(ncols) < 0.5
    u = vec(gb, u_has)
    _opts(((b"push_mode", 0),))
    for name in ("min_secondi", "max_secondi", "plus_secondi", "any_secondi", "plus_firsti", "min_firsti1", "plus_secondj1", "max_firstj1"):
        mon, op = name.split("_")
        w = A.mxv(u, getattr(gb.semiring, name)).new()
        st = _stats()
        assert st["method"] == PULL and st["tiles"] == -(-m * G // 64), st
        cands = ref_product(M, u_has, False, op, "INT64")
        if mon == "any":
            check_any(w, cands, "INT64", name)
        else:
            check_exact(w, *ref_fold(cands, mon, "INT64"), name)


# ---- 3. push limits ------------------------------------------------------------------------------------------------------------------
HUB, CONTESTED = 4097, 7


def _push_graph():
    """P = A for vxm.  Row 0: a hub of 4097 entries; rows 1 .. 65: one entry each, all on the contested output 7; rows 66, 67 empty;
    row 68: one entry of its own."""
    ncols = 2 * HUB
    lists = {0: 2 * np.arange(HUB) + 1}
    for k in range(1, 66):
        lists[k] = np.array([CONTESTED])
    lists[68] = np.array([100])
    return lists, 70, ncols


FRONTIERS = {"hub alone": [0], "two on one output": [1, 2], "64": list(range(1, 65)), "65 on one output": list(range(1, 66)),
             "hub + 64": list(range(0, 65)), "hub, empty rows, a single": [0, 66, 67, 68], "all rows empty": [66, 67]}


@pytest.mark.parametrize("fname", list(FRONTIERS))
def test_push_limits(gb, fname):
    lists, nrows, ncols = _push_graph()
    r = np.concatenate([np.full(c.size, i) for i, c in lists.items()])
    c = np.concatenate(list(lists.values()))
    A = gb.Matrix.from_coo(r, c, np.ones(r.size, np.int64), dtype="INT64", nrows=nrows, ncols=ncols)
    M = np.zeros((nrows, ncols), bool)
    M[r, c] = True
    q_has = np.zeros(nrows, bool)
    q_has[FRONTIERS[fname]] = True
    q = vec(gb, q_has)
    work = int(sum(lists[k].size for k in FRONTIERS[fname] if k in lists))
    excl = np.zeros(ncols, bool)
    excl[CONTESTED] = True
    mk = vec(gb, excl, dtype="BOOL")
    for name in ("min_secondi", "max_secondi", "plus_secondi", "any_secondi", "plus_secondj", "max_firsti1"):
        mon, op = name.split("_")
        cands = ref_product(M, q_has, True, op, "INT64")
        got = {}
        for push_mode in (2, 0):
            _opts(((b"push_mode", push_mode),))
            w = q.vxm(A, getattr(gb.semiring, name)).new()
            st = _stats()
            if push_mode == 2:
                assert st["method"] == PUSH and st["flops"] == work and st["tiles"] == -(-work // 512), st
            else:
                assert st["method"] == PULL, st
            if mon == "any":
                check_any(w, cands, "INT64", (name, push_mode))
            else:
                check_exact(w, *ref_fold(cands, mon, "INT64"), (name, push_mode))
                got[push_mode] = tuple(x.tolist() for x in w.to_coo())
            # a mask that excludes the contested output
            w = gb.Vector("INT64", size=ncols)
            w(~mk.S) << q.vxm(A, getattr(gb.semiring, name))
            gi, _ = w.to_coo()
            assert CONTESTED not in gi.tolist() and gi.tolist() == [o for o, cd in enumerate(cands) if cd.size and o != CONTESTED]
        if mon != "any":
            assert got[0] == got[2], name  # bit-identical in both directions


def test_push_last_of_65537_outputs(gb):
    n = 65537
    A = gb.Matrix.from_coo([0, 2, 2], [n - 1, 5, n - 1], [1, 1, 1], dtype="INT64", nrows=3, ncols=n)
    q = gb.Vector.from_coo([0, 2], [1, 1], dtype="INT64", size=3)
    for push_mode, method in ((2, PUSH), (0, PULL)):
        _opts(((b"push_mode", push_mode),))
        for name, exp in (("min_secondi", [2, 0]), ("max_secondi", [2, 2]), ("plus_secondi", [2, 2]), ("max_secondj", [5, n - 1])):
            w = q.vxm(A, getattr(gb.semiring, name)).new()
            assert _stats()["method"] == method
            gi, gv = w.to_coo()
            assert gi.tolist() == [5, n - 1] and gv.tolist() == exp, (name, push_mode, gi, gv)


# ---- 4. write rule and types --------------------------------------------------------------------------------------------------------
def test_write_rule_and_types(gb):
    from graphblas_amd import _lib

    L = _lib.lib
    A = matrix_of(gb, LIT)
    q_has = np.zeros(7, bool)
    q_has[[1, 3, 6]] = True
    q = vec(gb, q_has)
    cands = ref_product(LIT, q_has, True, "secondi1", "INT64")
    t_has, t_val = ref_fold(cands, "max", "INT64")
    sr = gb.semiring.max_secondi1
    w0_has, w0_val = np.array([True, True, False, True, False]), np.array([0, 50, 0, 3, 0], np.int64)
    m_has = np.array([True, False, True, True, False])
    for push_mode in (0, 2):
        _opts(((b"push_mode", push_mode),))
        # accum = min into an existing INT64 w
        w = vec(gb, w0_has, w0_val)
        w(accum=gb.binary.min) << q.vxm(A, sr)
        check_exact(w, *ref_write(w0_has, w0_val, t_has, t_val, None, False, np.minimum), "accum")
        # w of type FP64 and INT8 (T is cast; a PLUS of large indices keeps its low bits in INT8)
        for wt in ("FP64", "INT8"):
            w = q.vxm(A, sr).new(dtype=wt)
            assert w.dtype.name == wt
            check_exact(w, t_has, t_val.astype(NP[wt]), wt)
        # replace with and without a mask
        mk = vec(gb, m_has, dtype="BOOL")
        for mask_on in (True, False):
            for comp in ((False, True) if mask_on else (False,)):
                w = vec(gb, w0_has, w0_val)
                allow = (~m_has if comp else m_has) if mask_on else None
                arg = (~mk.S if comp else mk.S) if mask_on else None
                if mask_on:
                    w(arg, replace=True) << q.vxm(A, sr)
                else:  # (the Python layer refuses replace without a mask: through the C ABI)
                    assert L.GrB_vxm(w._carg, None, None, sr["INT64"]._carg, q._carg, A._carg, ctypes.c_void_p.in_dll(L, "GrB_DESC_R")) == 0
                check_exact(w, *ref_write(w0_has, w0_val, t_has, t_val, allow, True, None), ("replace", mask_on, comp))
        # the mask aliasing w (structural and by value: w holds a zero), u aliasing w
        for by_value in (False, True):
            w = vec(gb, w0_has, w0_val)
            allow = w0_has & (w0_val != 0) if by_value else w0_has
            w(w.V if by_value else w.S, replace=True) << q.vxm(A, sr)
            check_exact(w, *ref_write(w0_has, w0_val, t_has, t_val, allow, True, None), ("mask is w", by_value))
        sq = np.zeros((7, 7), bool)
        sq[:, :5] = LIT
        S = matrix_of(gb, sq)
        w = vec(gb, q_has)
        w << w.vxm(S, gb.semiring.min_secondi)
        check_exact(w, *ref_fold(ref_product(sq, q_has, True, "secondi", "INT64"), "min", "INT64"), "u is w")
        # an iso BOOL matrix; FP32 operands holding NaN (values are never read)
        r, c = np.nonzero(LIT)
        indptr = np.concatenate([[0], np.cumsum(LIT.sum(1))])
        B = gb.Matrix.ss.import_csr(nrows=7, ncols=5, indptr=indptr, values=np.array([True]), col_indices=c, is_iso=True, sorted_cols=True, dtype="BOOL")
        check_exact(q.vxm(B, sr).new(), t_has, t_val, "iso BOOL")
        F = gb.Matrix.from_coo(r, c, np.full(r.size, np.nan, np.float32), dtype="FP32", nrows=7, ncols=5)
        qf = gb.Vector.from_coo(np.flatnonzero(q_has), np.full(3, np.nan, np.float32), dtype="FP32", size=7)
        w = qf.vxm(F, sr).new()
        assert w.dtype.name == "INT64"
        check_exact(w, t_has, t_val, "NaN operands")
    # PLUS wraps in the semiring's type and INT8 keeps the low bits of T
    big = np.zeros((3, 70000), bool)
    big[0, [65535, 69999]] = big[1, 69999] = True
    Bm = matrix_of(gb, big)
    u_has = np.zeros(70000, bool)
    u_has[[65535, 69999]] = True
    w = Bm.mxv(vec(gb, u_has), gb.semiring.plus_secondi).new(dtype="INT8")
    check_exact(w, np.array([True, True, False]), np.array([65535 + 69999, 69999, 0], np.int64).astype(np.int8), "INT8 of a sum")
    # !mask && comp writes nothing; with replace it empties w
    none, repl = ctypes.c_void_p.in_dll(L, "GrB_DESC_C"), ctypes.c_void_p.in_dll(L, "GrB_DESC_RC")
    sr_h = gb.semiring.max_secondi1["INT64"]._carg
    w = vec(gb, w0_has, w0_val)
    assert L.GrB_vxm(w._carg, None, None, sr_h, q._carg, A._carg, none) == 0
    check_exact(w, w0_has, w0_val, "comp of no mask")
    assert L.GrB_vxm(w._carg, None, None, sr_h, q._carg, A._carg, repl) == 0
    assert w.nvals == 0
    # an operand without entries: the write rule alone
    w = vec(gb, w0_has, w0_val)
    assert L.GrB_vxm(w._carg, None, None, sr_h, gb.Vector("INT64", size=7)._carg, A._carg, ctypes.c_void_p.in_dll(L, "GrB_DESC_R")) == 0
    assert _stats()["method"] == EMPTY and w.nvals == 0
    # dimension mismatches: -6, the message on w, w unchanged
    w = vec(gb, w0_has, w0_val)
    bad_u, bad_w, bad_m = gb.Vector("INT64", size=6), gb.Vector("INT64", size=4), gb.Vector("BOOL", size=6)
    err = ctypes.c_char_p()
    for args in ((w._carg, None, None, sr_h, bad_u._carg, A._carg, None), (bad_w._carg, None, None, sr_h, q._carg, A._carg, None),
                 (w._carg, bad_m._carg, None, sr_h, q._carg, A._carg, None)):
        assert L.GrB_vxm(*args) == -6
        assert L.GrB_Vector_error(ctypes.byref(err), args[0]) == 0 and b"mxv/vxm" in err.value, err.value
    assert L.GrB_mxv(w._carg, None, None, sr_h, A._carg, q._carg, None) == -6  # (A is 7 x 5: u has 7 entries, w 5)
    check_exact(w, w0_has, w0_val, "after the refused calls")
    with pytest.raises(gb.exceptions.DimensionMismatch):
        bad_u.vxm(A, sr).new()


# ---- 5. BFS parents end to end -------------------------------------------------------------------------------------------------------
def _graphs():
    from graphblas_amd import synthetic

    indptr, col = synthetic.rmat_csr(10, device="cpu")  # (host tensors on both tiers: the graph reaches the library through from_coo)
    ip, cj = indptr.cpu().numpy().astype(np.int64), col.cpu().numpy().astype(np.int64)
    n = ip.size - 1
    adj = np.zeros((n, n), bool)
    adj[np.repeat(np.arange(n), np.diff(ip)), cj] = True
    adj |= adj.T
    path = np.zeros((9, 9), bool)
    path[np.arange(8), np.arange(1, 9)] = True
    path |= path.T
    return {"rmat10": (adj, int(np.argmax(adj.sum(1)))), "path9": (path, 3)}


def _np_bfs(adj, src):
    """Levels and smallest-parent tree."""
    n = adj.shape[0]
    level, parent = np.full(n, -1), np.full(n, -1)
    level[src], parent[src] = 0, src
    frontier, d = np.array([src]), 0
    while frontier.size:
        d += 1
        reach = adj[frontier].any(0) & (level < 0)
        new = np.flatnonzero(reach)
        for v in new:
            parent[v] = frontier[adj[frontier, v]].min()
        level[new] = d
        frontier = new
    return level, parent


@pytest.fixture(scope="module")
def bfs_refs():
    return {}


@pytest.mark.parametrize("push_mode", [0, 1, 2])
@pytest.mark.parametrize("gname", ["rmat10", "path9"])
def test_bfs_parents(gb, bfs_refs, gname, push_mode):
    if "graphs" not in bfs_refs:  # (computed once, shared, never changed)
        bfs_refs["graphs"] = _graphs()
        bfs_refs["np"] = {k: _np_bfs(*g) for k, g in bfs_refs["graphs"].items()}
    adj, src = bfs_refs["graphs"][gname]
    level, parent_ref = bfs_refs["np"][gname]
    n = adj.shape[0]
    r, c = np.nonzero(adj)
    A = gb.Matrix.from_coo(r, c, np.ones(r.size, bool), dtype="BOOL", nrows=n, ncols=n)
    _opts(((b"push_mode", push_mode),))
    # the level BFS of this library (lor_land): the reached set
    q = gb.Vector.from_coo([src], [True], dtype="BOOL", size=n)
    visited = q.dup()
    while q.nvals:
        q(~visited.S, replace=True) << q.vxm(A, gb.semiring.lor_land)
        visited(q.S) << q
    reached = visited.to_coo()[0].tolist()
    assert reached == np.flatnonzero(level >= 0).tolist()
    for name in ("min_secondi", "any_secondi"):
        sr = getattr(gb.semiring, name)
        parent = gb.Vector.from_coo([src], [src], dtype="INT64", size=n)
        q = gb.Vector.from_coo([src], [src], dtype="INT64", size=n)
        methods = set()
        while q.nvals:
            q(~parent.S, replace=True) << q.vxm(A, sr)
            methods.add(_stats()["method"])
            parent(q.S) << q
        assert methods <= {PULL, PUSH, EMPTY} and (push_mode != 0 or PUSH not in methods) and (push_mode != 2 or PULL not in methods), methods
        pi, pv = parent.to_coo()
        assert pi.tolist() == reached, name
        if name == "min_secondi":
            assert pv.tolist() == parent_ref[pi].tolist()
        else:
            for v, p in zip(pi.tolist(), pv.tolist()):
                assert (v == src and p == src) or (adj[p, v] and level[p] == level[v] - 1), (v, p)


# ---- 6. the boundary ----------------------------------------------------------------------------------------------------------------
def _err(L, obj, matrix):
    s = ctypes.c_char_p()
    (L.GrB_Matrix_error if matrix else L.GrB_Vector_error)(ctypes.byref(s), obj._carg)
    return (s.value or b"").decode()


def test_boundary(gb):
    from graphblas_amd import _lib

    L = _lib.lib
    h = lambda name: ctypes.c_void_p(ctypes.c_void_p.in_dll(L, name).value)
    r, c, x = [0, 1, 2, 2], [1, 2, 0, 2], [4, 5, 6, 7]
    A = gb.Matrix.from_coo(r, c, x, dtype="INT64", nrows=3, ncols=3)
    B = gb.Matrix.from_coo(r, c, x, dtype="INT64", nrows=3, ncols=3)
    u = gb.Vector.from_coo([0, 2], [1, 2], dtype="INT64", size=3)
    L.GrB_Matrix_apply_BinaryOp2nd_INT64.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_int64, ctypes.c_void_p]
    L.GrX_mxm_streamed.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_uint64] + [ctypes.c_void_p] * 4
    s = ctypes.c_void_p()
    assert L.GrB_Scalar_new(ctypes.byref(s), h("GrB_INT64")) == 0
    L.GrB_Scalar_setElement_INT64.argtypes = [ctypes.c_void_p, ctypes.c_int64]
    assert L.GrB_Scalar_setElement_INT64(s, 1) == 0
    bop, sr, plus, pt = h("GxB_SECONDI1_INT64"), h("GxB_ANY_SECONDI1_INT64"), h("GrB_PLUS_INT64"), h("GrB_PLUS_TIMES_SEMIRING_INT64")

    def fresh():
        return gb.Matrix.from_coo([0, 1], [0, 1], [9, 8], dtype="INT64", nrows=3, ncols=3)

    matrix_calls = {
        "GrB_mxm": lambda C: L.GrB_mxm(C._carg, None, None, sr, A._carg, B._carg, None),
        "GrB_mxm, accum": lambda C: L.GrB_mxm(C._carg, None, bop, pt, A._carg, B._carg, None),
        "eWiseAdd_BinaryOp": lambda C: L.GrB_Matrix_eWiseAdd_BinaryOp(C._carg, None, None, bop, A._carg, B._carg, None),
        "eWiseMult_BinaryOp": lambda C: L.GrB_Matrix_eWiseMult_BinaryOp(C._carg, None, None, bop, A._carg, B._carg, None),
        "eWiseMult_Semiring": lambda C: L.GrB_Matrix_eWiseMult_Semiring(C._carg, None, None, sr, A._carg, B._carg, None),
        "eWiseAdd, accum": lambda C: L.GrB_Matrix_eWiseAdd_BinaryOp(C._carg, None, bop, plus, A._carg, B._carg, None),
        "eWiseUnion": lambda C: L.GxB_Matrix_eWiseUnion(C._carg, None, None, bop, A._carg, s, B._carg, s, None),
        "apply_BinaryOp2nd": lambda C: L.GrB_Matrix_apply_BinaryOp2nd_INT64(C._carg, None, None, bop, A._carg, 1, None),
        "kronecker_BinaryOp": lambda C: L.GrB_Matrix_kronecker_BinaryOp(gb.Matrix("INT64", 9, 9)._carg if C is None else C._carg, None, None, bop, A._carg, B._carg, None),
    }
    try:
        for name, call in matrix_calls.items():
            C = gb.Matrix.from_coo([0, 1], [0, 1], [9, 8], dtype="INT64", nrows=9, ncols=9) if name.startswith("kron") else fresh()
            assert call(C) == -8, name
            assert "SECONDI1" in _err(L, C, True), (name, _err(L, C, True))
            ci, cj, cx = C.to_coo()
            assert (ci.tolist(), cj.tolist(), cx.tolist()) == ([0, 1], [0, 1], [9, 8]), name
        w = gb.Vector.from_coo([1], [5], dtype="INT64", size=3)
        vector_calls = {
            "reduce_BinaryOp": lambda: L.GrB_Matrix_reduce_BinaryOp(w._carg, None, None, bop, A._carg, None),
            "reduce_Monoid, accum": lambda: L.GrB_Matrix_reduce_Monoid(w._carg, None, bop, h("GrB_PLUS_MONOID_INT64"), A._carg, None),
            "mxv, accum": lambda: L.GrB_mxv(w._carg, None, bop, pt, A._carg, u._carg, None),
            "vxm, accum on a positional semiring": lambda: L.GrB_vxm(w._carg, None, bop, sr, u._carg, A._carg, None),
            "Vector eWiseMult": lambda: L.GrB_Vector_eWiseMult_BinaryOp(w._carg, None, None, bop, u._carg, u._carg, None),
        }
        for name, call in vector_calls.items():
            assert call() == -8, name
            assert "SECONDI1" in _err(L, w, False), (name, _err(L, w, False))
            assert [a.tolist() for a in w.to_coo()] == [[1], [5]], name
        out = [ctypes.c_uint64() for _ in range(4)]
        assert L.GrX_mxm_streamed(sr, A._carg, B._carg, 1 << 30, *[ctypes.byref(o) for o in out]) == -8
        # an ordinary accumulator with a positional semiring is allowed
        assert L.GrB_vxm(w._carg, None, h("GrB_MIN_INT64"), sr, u._carg, A._carg, None) == 0
    finally:
        L.GrB_Scalar_free(ctypes.byref(s))
    # the Python spellings
    NI = gb.exceptions.NotImplementedException
    with pytest.raises(NI, match="SECONDI"):
        A.mxm(B, gb.semiring.any_secondi).new()
    with pytest.raises(NI, match="FIRSTI"):
        A.ewise_mult(B, gb.binary.firsti).new()
    with pytest.raises(NI):
        A.ewise_add(B, gb.binary.firstj1).new()
    with pytest.raises(NI):
        A.kronecker(B, gb.binary.secondj).new()
    with pytest.raises(NI):
        A.apply(gb.binary.secondi, right=1).new()
    with pytest.raises(NI):
        w(accum=gb.binary.firsti) << A.mxv(u, gb.semiring.plus_times)
    with pytest.raises(NI):
        gb.Matrix.from_coo([0, 0], [1, 1], [1, 2], dtype="INT64", nrows=2, ncols=2, dup_op=gb.binary.firsti)
