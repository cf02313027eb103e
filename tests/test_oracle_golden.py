"""Pins the CPU oracle (oracle/grb_oracle.c) against every known-answer literal the reference's own
tests/docs hold for mxm / mxv / vxm (tests/golden/reference_literals.json), and cross-checks it
against the independent dense brute-force evaluator (oracle/dense_eval.py)."""
import json
import os

import numpy as np
import pytest

from oracle import dense_eval as D
from oracle import grb_oracle as O
from tests.helpers import o_obj, oracle_case, same
from tests.values import rand_vals, same_values

_G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "reference_literals.json")))


@pytest.mark.parametrize("case", _G["cases"], ids=[c["name"] for c in _G["cases"]])
def test_reference_literal(case):
    got = oracle_case(case, _G["inputs"])
    if "expect_shape" in case:
        assert [got.nrows, got.ncols] == case["expect_shape"]
    else:
        same(got, case["expect"])


@pytest.mark.parametrize("case", _G["vector_ops"], ids=[c["name"] for c in _G["vector_ops"]])
def test_reference_literal_vector_ops(case):
    """The operations around the path (assign, reduce, eWise, row reduce, resize): oracle vs the reference's literals."""
    def get(x):
        return o_obj(_G["inputs"][x] if isinstance(x, str) else x)

    op = case["op"]
    if op == "assign_scalar":
        got = O.vec_assign_scalar(get(case["w"]), case["value"], mask=get(case["mask"]) if "mask" in case else None,
                                  mask_comp=case.get("mask_comp", False))
        same(got, case["expect"])
    elif op == "reduce":
        assert O.vec_reduce(get(case["u"]), case["monoid"]) == case["expect_scalar"]
    elif op in ("ewise_mult", "ewise_add"):
        same(O.vec_ewise(get(case["u"]), get(case["v"]), case["binop"], union=op == "ewise_add"), case["expect"])
    elif op in ("reduce_rowwise", "reduce_columnwise"):
        same(O.mat_reduce_rows(get(case["A"]), case["monoid"], columns=op == "reduce_columnwise"), case["expect"])
    elif op in ("agg_matvec", "agg_matvec_scalar"):
        # count / exists: semiring(A @ init) with a dense iso INT64 operand (reference core/operator/agg.py:264-283)
        A = get(case["A"])
        size = A.nrows if case.get("columns") else A.ncols
        init = O.OVec(size, np.arange(size), np.ones(size, np.int64), "INT64")
        got = O.vxm(init, A, case["semiring"]) if case.get("columns") else O.mxv(A, init, case["semiring"])
        if op == "agg_matvec":
            same(got, case["expect"])
        else:
            assert O.vec_reduce(got, "plus") == case["expect_scalar"]
    elif op == "reduce_scalar":
        assert O.vec_reduce(O.mat_reduce_rows(get(case["A"]), case["monoid"]), case["monoid"]) == case["expect_scalar"]
    elif op == "resize":
        src = get(case["A"] if "A" in case else case["w"])
        if "A" in case:
            nr, nc = case["to"]
            r = np.repeat(np.arange(src.nrows), np.diff(src.indptr))
            keep = (r < nr) & (src.indices < nc)
            got = O.OMat.from_coo(r[keep], src.indices[keep], src.values[keep], nr, nc, src.tname)
        else:
            keep = src.idx < case["to"][0]
            got = O.OVec(case["to"][0], src.idx[keep], src.vals[keep], src.tname)
        same(got, case["expect"])
    elif op == "extract_element":  # (element access is the vector's own content: the oracle's dense view)
        has, val = get(case["u"]).dense()
        for i, want in case["probes"]:
            assert (int(val[i]) if has[i] else None) == want
    elif op == "set_element":  # GrB_Vector_setElement = assign of a scalar at one index
        w = get(case["w"])
        for i, x in case["sets"]:
            w = O.vec_assign(w, x, [i])
        same(w, case["expect"])
    elif op == "remove_element":  # GrB_Vector_removeElement: the entry leaves the pattern
        w = get(case["w"])
        keep = w.idx != case["index"]
        same(O.OVec(w.size, w.idx[keep], w.vals[keep], w.tname), case["expect"])
    elif op == "extract":
        u = get(case["u"])
        same(O.vec_extract(O.OVec.empty(len(case["indices"]), u.tname), u, case["indices"]), case["expect"])
    elif op == "assign_vector":
        same(O.vec_assign(get(case["w"]), get(case["u"]), case["indices"]), case["expect"])
    elif op == "assign_scalar_at":
        same(O.vec_assign(get(case["w"]), case["value"], case["indices"]), case["expect"])
    elif op == "transpose":
        same(get(case["A"]).transpose(), case["expect"])
    elif op == "agg_exists_scalar":  # exists = any_pair over the whole object (reference core/operator/agg.py:264-283): 1 iff it holds an entry
        x = get(case["A"] if "A" in case else case["u"])
        nvals = x.nvals if "A" in case else len(x.idx)
        assert (1 if nvals else None) == case["expect_scalar"]
    else:
        raise AssertionError(op)


def test_primer_sssp():
    s = _G["sssp"]
    G = o_obj(_G["inputs"][s["G"]])
    v = o_obj(s["start"])
    for _ in range(10):
        w = O.vxm(v, G, "min_plus", w=v, accum="min")
        if w.idx.tolist() == v.idx.tolist() and w.vals.tolist() == v.vals.tolist():
            break
        v = w
    same(v, s["expect"])


def _rand_dense(rng, shape, density, tname):
    has = rng.random(shape) < density
    np_t = O.NP_OF[tname]
    if tname == "BOOL":
        val = rng.random(shape) < 0.6
    elif tname.startswith("FP"):
        val = rng.integers(-8, 9, shape).astype(np_t)  # exact in fp => order independent
    elif tname.startswith("U"):
        val = rng.integers(0, np.iinfo(np_t).max, shape, dtype=np.uint64).astype(np_t)
    else:
        info = np.iinfo(np_t)
        val = rng.integers(info.min, info.max, shape, dtype=np.int64).astype(np_t)
    val = np.where(has, val, 0).astype(np_t)
    return val, has


def _omat(val, has, tname):
    r, c = np.nonzero(has)
    return O.OMat.from_coo(r, c, val[r, c], has.shape[0], has.shape[1], tname)


def _ovec(val, has, tname):
    (i,) = np.nonzero(has)
    return O.OVec(len(has), i, val[i], tname)


SEMIRINGS = ["plus_times", "min_plus", "lor_land", "any_pair", "max_plus", "plus_plus", "min_second",
             "max_first", "plus_pair", "min_max", "lxor_land", "land_lor"]


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("semiring", SEMIRINGS)
def test_oracle_vs_dense_bruteforce(semiring, seed):
    rng = np.random.default_rng(1000 * seed + hash(semiring) % 997)
    monoid, mult = semiring.split("_", 1)
    boolish = monoid in ("lor", "land", "lxor", "lxnor")
    tname = "BOOL" if boolish else ["INT64", "INT8", "FP64", "UINT16", "FP32", "INT32"][seed]
    if semiring == "any_pair":
        tname = ["BOOL", "INT64", "FP32", "UINT8", "INT16", "FP64"][seed]
    np_t = O.NP_OF[tname]
    m, k, n = rng.integers(1, 9, 3)
    Av, Ah = _rand_dense(rng, (m, k), 0.5, tname)
    Bv, Bh = _rand_dense(rng, (k, n), 0.5, tname)
    Cv, Ch = _rand_dense(rng, (m, n), 0.4, tname)
    Mv, Mh = _rand_dense(rng, (m, n), 0.6, "INT8")
    comp, struct, replace = (bool(x) for x in rng.integers(0, 2, 3))
    use_mask = bool(rng.integers(0, 3))
    accum = [None, "plus", "min", "second", "first", "max"][rng.integers(0, 6)]
    # --- mxm
    Tv, Th = D.matmul(Av, Ah, Bv, Bh, monoid, mult, np_t)
    Nv, Nh = D.write(Cv, Ch, Tv, Th, Mv if use_mask else None, Mh if use_mask else None, comp=comp,
                     struct=struct, accum=accum, replace=replace and use_mask, np_t=np_t)
    got = O.mxm(_omat(Av, Ah, tname), _omat(Bv, Bh, tname), semiring, C=_omat(Cv, Ch, tname),
                mask=_omat(Mv, Mh, "INT8") if use_mask else None, mask_comp=comp and use_mask,
                mask_struct=struct, accum=accum, replace=replace and use_mask)
    exp = _omat(Nv, Nh, tname)
    assert got.indptr.tolist() == exp.indptr.tolist() and got.indices.tolist() == exp.indices.tolist()
    assert got.values.tolist() == exp.values.tolist()
    # --- mxv / vxm on column 0 / row 0
    uv, uh = Bv[:, 0], Bh[:, 0]
    Tv1, Th1 = D.matmul(Av, Ah, uv[:, None], uh[:, None], monoid, mult, np_t)
    wv, wh = Cv[:, 0], Ch[:, 0]
    mv, mh = Mv[:, 0], Mh[:, 0]
    Nv1, Nh1 = D.write(wv, wh, Tv1[:, 0], Th1[:, 0], mv if use_mask else None, mh if use_mask else None,
                       comp=comp, struct=struct, accum=accum, replace=replace and use_mask, np_t=np_t)
    got = O.mxv(_omat(Av, Ah, tname), _ovec(uv, uh, tname), semiring, w=_ovec(wv, wh, tname),
                mask=_ovec(mv, mh, "INT8") if use_mask else None, mask_comp=comp and use_mask,
                mask_struct=struct, accum=accum, replace=replace and use_mask)
    exp = _ovec(Nv1, Nh1, tname)
    assert got.idx.tolist() == exp.idx.tolist() and got.vals.tolist() == exp.vals.tolist()
    # vxm(u, A') must equal mxv(A, u) when mult is commutative; with first/second swapped otherwise
    if mult not in ("first", "second"):
        got2 = O.vxm(_ovec(uv, uh, tname), _omat(Av, Ah, tname), semiring, transpose_b=True,
                     w=_ovec(wv, wh, tname), mask=_ovec(mv, mh, "INT8") if use_mask else None,
                     mask_comp=comp and use_mask, mask_struct=struct, accum=accum, replace=replace and use_mask)
        assert got2.idx.tolist() == exp.idx.tolist() and got2.vals.tolist() == exp.vals.tolist()
    # row vector times matrix: u' B
    rv, rh = Av[0, :], Ah[0, :]
    Tv2, Th2 = D.matmul(rv[None, :], rh[None, :], Bv, Bh, monoid, mult, np_t)
    got3 = O.vxm(_ovec(rv, rh, tname), _omat(Bv, Bh, tname), semiring)
    exp3 = _ovec(Tv2[0], Th2[0], tname)
    assert got3.idx.tolist() == exp3.idx.tolist() and got3.vals.tolist() == exp3.vals.tolist()


def _rand_dense_domain(rng, shape, density, tname, domain):
    has = rng.random(shape) < density
    val = np.zeros(shape, O.NP_OF[tname])
    val[has] = rand_vals(rng, int(has.sum()), tname, domain)
    return val, has


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("domain", ["signed", "special"])
@pytest.mark.parametrize("semiring", SEMIRINGS)
def test_oracle_vs_dense_bruteforce_value_domains(semiring, domain, seed):
    """The C oracle against the naive dense restatement over the value domains of tests/values.py: full-range integers, and for the
    floating-point types NaN, +-inf, +-0.0, subnormals and +-MAX (both fold in column order, so even inexact sums agree bit for bit),
    with a floating-point value mask (-0.0 false, NaN true) -- compared with the strict comparator."""
    rng = np.random.default_rng(5000 + 1000 * seed + sum(map(ord, semiring + domain)))
    monoid, mult = semiring.split("_", 1)
    if monoid in ("lor", "land", "lxor", "lxnor"):
        tname = "BOOL"
    elif domain == "special":
        tname = ["FP32", "FP64"][seed % 2]
    else:
        tname = ["INT8", "UINT64", "INT16", "UINT32", "INT32", "UINT8", "INT64", "UINT16", "FP32", "FP64"][(seed + len(semiring)) % 10]
    np_t = O.NP_OF[tname]
    dom = "signed" if tname == "BOOL" else domain
    m, k, n = (int(x) for x in rng.integers(1, 9, 3))
    Av, Ah = _rand_dense_domain(rng, (m, k), 0.6, tname, dom)
    Bv, Bh = _rand_dense_domain(rng, (k, n), 0.6, tname, dom)
    Cv, Ch = _rand_dense_domain(rng, (m, n), 0.4, tname, dom)
    Mv, Mh = _rand_dense_domain(rng, (m, n), 0.6, "FP32", "special")
    comp, struct, replace = (bool(x) for x in rng.integers(0, 2, 3))
    accum = [None, "plus", "min", "max", "second"][seed % 5] if tname != "BOOL" else [None, "lor", "land"][seed % 3]
    Tv, Th = D.matmul(Av, Ah, Bv, Bh, monoid, mult, np_t)
    Nv, Nh = D.write(Cv, Ch, Tv, Th, Mv, Mh, comp=comp, struct=struct, accum=accum, replace=replace, np_t=np_t)
    got = O.mxm(_omat(Av, Ah, tname), _omat(Bv, Bh, tname), semiring, C=_omat(Cv, Ch, tname), mask=_omat(Mv, Mh, "FP32"),
                mask_comp=comp, mask_struct=struct, accum=accum, replace=replace)
    exp = _omat(Nv, Nh, tname)
    assert got.indptr.tolist() == exp.indptr.tolist()
    same_values(got.indices, got.values, exp.indices, exp.values, None, ("mxm", tname, semiring, domain))
    uv, uh = Bv[:, 0], Bh[:, 0]
    Tv1, Th1 = D.matmul(Av, Ah, uv[:, None], uh[:, None], monoid, mult, np_t)
    Nv1, Nh1 = D.write(Cv[:, 0], Ch[:, 0], Tv1[:, 0], Th1[:, 0], Mv[:, 0], Mh[:, 0], comp=comp, struct=struct, accum=accum,
                       replace=replace, np_t=np_t)
    got = O.mxv(_omat(Av, Ah, tname), _ovec(uv, uh, tname), semiring, w=_ovec(Cv[:, 0], Ch[:, 0], tname),
                mask=_ovec(Mv[:, 0], Mh[:, 0], "FP32"), mask_comp=comp, mask_struct=struct, accum=accum, replace=replace)
    exp = _ovec(Nv1, Nh1, tname)
    same_values(got.idx, got.vals, exp.idx, exp.vals, None, ("mxv", tname, semiring, domain))
    # the oracle's reduce against the dense fold (no identity for a non-empty set)
    if tname != "BOOL" and Ah[0].any():
        for mon in ("plus", "times", "min", "max"):
            acc = None
            for x in Av[0][Ah[0]]:
                acc = x if acc is None else D.binop(mon, acc, x, np_t)
            ref = O.vec_reduce(_ovec(Av[0], Ah[0], tname), mon)
            same_values([0], np.array([ref], np_t), [0], np.array([acc], np_t), None, ("reduce", tname, mon, domain))


def test_scipy_crosscheck_plus_times():
    sp = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(7)
    A = sp.random(200, 150, 0.05, format="csr", random_state=rng, data_rvs=lambda n: rng.integers(1, 9, n).astype(float))
    B = sp.random(150, 120, 0.05, format="csr", random_state=rng, data_rvs=lambda n: rng.integers(1, 9, n).astype(float))
    A.sort_indices(); B.sort_indices()
    oa = O.OMat(200, 150, A.indptr, A.indices, A.data, "FP64")
    ob = O.OMat(150, 120, B.indptr, B.indices, B.data, "FP64")
    C = (A @ B).tocsr(); C.sort_indices()
    got = O.mxm(oa, ob, "plus_times")
    assert got.indptr.tolist() == C.indptr.tolist() and got.indices.tolist() == C.indices.tolist()
    np.testing.assert_allclose(got.values, C.data, rtol=1e-12)
    x = rng.integers(1, 5, 150).astype(float)
    y = O.mxv(oa, O.OVec(150, np.arange(150), x, "FP64"), "plus_times")
    ref = A @ x
    nz = np.diff(A.indptr) > 0
    assert y.idx.tolist() == np.flatnonzero(nz).tolist()
    np.testing.assert_allclose(y.vals, ref[nz], rtol=1e-12)


def test_oracle_assign_extract_literals():
    """The oracle's restatement of GrB_Vector_assign / GrB_Vector_extract reproduces the reference's literals
    (graphblas/tests/test_vector.py:428-443, 505-541)."""
    from oracle import grb_oracle as O

    v = O.OVec(7, [1, 3, 4, 6], np.array([1, 1, 2, 0], np.int64), "INT64")
    w = O.vec_extract(O.OVec.empty(3, "INT64"), v, [1, 3, 5])
    assert w.idx.tolist() == [0, 1] and w.vals.tolist() == [1, 1]
    u = O.OVec(3, [0, 2], np.array([9, 8], np.int64), "INT64")
    w = O.vec_assign(v, u, [0, 2, 4])
    assert w.idx.tolist() == [0, 1, 3, 4, 6] and w.vals.tolist() == [9, 1, 1, 8, 0]
    w = O.vec_assign(v, 9, [1, 3, 5])
    assert w.idx.tolist() == [1, 3, 4, 5, 6] and w.vals.tolist() == [9, 9, 2, 9, 0]


@pytest.mark.parametrize("tname,sr", [("INT64", "plus_times"), ("INT64", "min_plus"), ("FP32", "min_plus"), ("FP64", "plus_times"),
                                      ("BOOL", "lor_land"), ("INT32", "any_pair")])
def test_oracle_mxv_balanced_partition_and_split_hub_rows(tname, sr):
    """Round 6: the oracle's mxv cuts the rows into chunks of equal weight and folds a row heavier than a chunk in fixed blocks
    (only for monoids that are exactly associative in the type).  Whatever the partition, the result must be the row-by-row
    definition: checked against numpy on a matrix with one 300 000-entry hub row among 40 000 short ones, with several threads."""
    from oracle import grb_oracle as O

    rng = np.random.default_rng(11)
    n, m = 400_000, 40_001
    lens = rng.integers(0, 6, m)
    lens[17] = 300_000
    indptr = np.zeros(m + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    col = np.concatenate([np.sort(rng.choice(n, int(k), replace=False)) for k in lens]).astype(np.int64)
    npt = O.NP_OF[tname]
    vals = (rng.integers(1, 7, col.size) if tname != "BOOL" else rng.integers(0, 2, col.size)).astype(npt)
    A = O.OMat(m, n, indptr, col, vals, tname)
    ui = np.flatnonzero(rng.random(n) < 0.6)
    uv = (rng.integers(1, 9, ui.size) if tname != "BOOL" else rng.integers(0, 2, ui.size)).astype(npt)
    u = O.OVec(n, ui, uv, tname)
    O.lib()  # (loads the library: _MAX_THREADS is known afterwards)
    saved = O._MAX_THREADS
    try:
        O._MAX_THREADS = max(4, saved or 1)  # (several chunks and the block phase even on a small host)
        got = O.mxv(A, u, sr)
    finally:
        O._MAX_THREADS = saved
    u_has = np.zeros(n, bool); u_has[ui] = True
    u_val = np.zeros(n, npt); u_val[ui] = uv
    rows = np.repeat(np.arange(m), lens)
    keep = u_has[col]
    r, a, x = rows[keep], vals[keep], u_val[col[keep]]
    mon, mul = sr.split("_")
    prod = {"times": lambda: a * x, "plus": lambda: a + x, "land": lambda: a & x, "pair": lambda: np.ones_like(a)}[mul]()
    exp_rows = np.unique(r)
    assert got.idx.tolist() == exp_rows.tolist()
    if mon == "plus":
        exp = np.zeros(m, np.float64 if tname.startswith("FP") else npt); np.add.at(exp, r, prod)
    elif mon == "min":
        exp = np.full(m, np.inf if tname.startswith("FP") else np.iinfo(npt).max, npt); np.minimum.at(exp, r, prod)
    elif mon == "lor":
        exp = np.zeros(m, npt); np.logical_or.at(exp, r, prod)
    else:  # any_pair: every product is 1
        exp = np.ones(m, npt)
    if tname == "FP64" and mon == "plus":
        np.testing.assert_allclose(got.vals, exp[exp_rows], rtol=1e-12)
    else:
        assert got.vals.tolist() == exp[exp_rows].astype(npt).tolist()


def test_oracle_mxv_full_operand_without_presence_bytes():
    """A full operand may be handed to the C oracle without presence bytes (u_has = NULL; bench.py's CPU baseline does): the result
    must be the one with an explicit all-ones presence array, for the specialised loops and the generic one."""
    import ctypes

    from oracle import grb_oracle as O

    rng = np.random.default_rng(5)
    m, n = 3000, 2500
    lens = rng.integers(0, 12, m)
    indptr = np.zeros(m + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    col = np.concatenate([np.sort(rng.choice(n, int(k), replace=False)) for k in lens]).astype(np.int64)
    L = O.lib()
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    for tname, mon, mul in (("FP32", "min", "plus"), ("INT64", "plus", "times"), ("FP64", "max", "plus"), ("INT32", "min", "second"), ("BOOL", "lor", "land")):
        npt = O.NP_OF[tname]
        vals = (rng.integers(1, 50, col.size) if tname != "BOOL" else rng.integers(0, 2, col.size)).astype(npt)
        u_val = (rng.integers(1, 50, n) if tname != "BOOL" else rng.integers(0, 2, n)).astype(npt)
        out = []
        for u_has in (np.ones(n, np.uint8), None):
            t_has, t_val = np.zeros(m, np.uint8), np.zeros(m, npt)
            assert L.grbo_mxv(O.TYPE_CODES[tname], O.OP_CODES[mon], O.OP_CODES[mul], ctypes.c_int64(m), p(indptr), p(col), p(vals), 0, p(u_has), p(u_val),
                              None, p(t_has), p(t_val)) == 0
            out.append((t_has.copy(), np.where(t_has != 0, t_val, 0)))
        assert out[0][0].tolist() == out[1][0].tolist() and out[0][1].tolist() == out[1][1].tolist(), tname
        assert out[1][0].tolist() == (lens > 0).astype(np.uint8).tolist()
