"""Kernels against the oracle on the values where kernels go wrong: NaN, +-inf, signed zeros, subnormals, the types' extremes,
negative values and full-range integers (the value domains of tests/values.py), on every kernel path of mxv / vxm / mxm the
options can force, all 11 types, compared with the strict comparator (bit patterns; NaN matches NaN; the zero sign counts except
under min / max / any).  Each forced path is checked through GrX_Stats, so a silent fallback cannot leave a case untested."""
import numpy as np
import pytest

from oracle import grb_oracle as O
from tests.backend import DEVICES, bind
from tests.values import ALL_TYPES, FP_TYPES, plus_within_bound, rand_vals, same_fp, same_mat, same_vec, shape_rows

DEFAULT_LONG_KERNEL = 5

SPLIT = ((b"split_min_nnz", 1), (b"split_min_len", 8), (b"push_mode", 0))
ORDER_OPTS = ((b"order_min_nnz", 1), (b"lean_min_nnz", 1), (b"split_min_nnz", 1), (b"split_min_len", 8), (b"push_mode", 0), (b"hot_min_cols", 8),
              (b"lazy_layout", 0), (b"vec_pad_min_bytes", 0), (b"rows_head_min_groups", 1), (b"order_mode", 1), (b"hot_k", 256),
              (b"hub_min_len", 200))


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


def set_opts(opts):
    from graphblas_amd import _lib

    for name, val in opts:
        assert _lib.lib.GrX_option_set(name, val) == 0, name


def reset_opts():
    from graphblas_amd import _lib

    assert _lib.lib.GrX_options_reset() == 0


def semirings_for(tname):
    if tname == "BOOL":
        return ["lor_land", "land_lor", "lxor_land", "any_pair"]
    return ["min_plus", "max_plus", "min_second", "max_first", "plus_times", "plus_plus", "any_pair"]


def domain_for(tname, sr):
    """The value domain a semiring is compared bit for bit under: the plus monoid of a floating-point type over 'exact' values (their
    sums do not depend on the order of the fold), every other floating-point semiring over 'special', integers over their full range."""
    if tname in FP_TYPES:
        return "exact" if sr.startswith("plus_") else "special"
    return "signed"


def skewed(rng, m, n, tname, domain, lens=(8, 9, 15, 16, 17, 63, 64, 65, 300, 513, 1030), hubs=0):
    """Short rows and long rows over skewed columns (a tenth of the columns take 3/4 of the references), values from ``domain`` with
    all-NaN, all -0.0 and +inf / -inf rows.  ``hubs``: that many more rows of 100..600 entries (the ordered layouts want the long rows
    to hold a good share of the entries, as tests/test_vertex_order.py's skewed_square builds them)."""
    deg = rng.integers(0, 6, m)
    deg[rng.random(m) < 0.3] = 0
    for ln in tuple(lens) + tuple(int(x) for x in rng.integers(100, 600, hubs)):
        deg[rng.integers(0, m)] = min(ln, n)
    hot = rng.permutation(n)[: max(1, n // 10)]
    rows = np.repeat(np.arange(m), deg)
    cols = np.where(rng.random(rows.size) < 0.75, hot[rng.integers(0, hot.size, rows.size)], rng.integers(0, n, rows.size))
    key = np.unique(rows * n + cols)
    rows, cols = key // n, key % n
    vals = shape_rows(rng, rows, rand_vals(rng, rows.size, tname, domain), tname)
    return rows, cols, vals


def rand_vec(rng, n, dens, tname, domain):
    idx = np.flatnonzero(rng.random(n) < dens)
    return idx, rand_vals(rng, idx.size, tname, domain)


def zero_sign_rule(monoid, accum):
    """The monoid whose zero-sign rule a write of ``accum(w, A (monoid.x) u)`` is compared under: a min / max / any anywhere in the chain
    leaves the sign of a zero open (min(-0, +0) is either, and a later sum carries that on)."""
    return "min" if monoid in ("min", "max", "any") or accum in ("min", "max") else "plus"


def long_want(forced, tname):
    return {3: 1 if tname == "BOOL" else 2, 5: 1 if tname == "BOOL" else 2}.get(forced, forced)


MXV_PATHS = {
    "default": (),
    "short0": SPLIT + ((b"short_kernel", 0),),
    "short1": SPLIT + ((b"short_kernel", 1),),
    "short5": SPLIT + ((b"short_kernel", 5),),
    "short6": SPLIT + ((b"short_kernel", 6),),
    "long1": SPLIT + ((b"long_kernel", 1), (b"long_sub", 2), (b"long_sub_min_len", 8)),
    "long2": SPLIT + ((b"long_kernel", 2), (b"long_classes", 8)),
    "long3": SPLIT + ((b"long_kernel", 3),),
    "long4": SPLIT + ((b"long_kernel", 4), (b"long_classes", 32)),
    "long5": SPLIT + ((b"long_kernel", 5),),
    "hot_cold": SPLIT + ((b"hot_min_cols", 8), (b"hot_k", 256), (b"long_kernel", 4), (b"long_classes", 16), (b"short_kernel", 5),
                         (b"vec_pad_min_bytes", 0)),
    "cold_tiles": ((b"split_min_nnz", 1), (b"split_min_len", 2), (b"push_mode", 0), (b"hot_min_cols", 8), (b"hot_k", 128), (b"long_kernel", 4),
                   (b"long_sub", 2), (b"vec_pad_min_bytes", 0)),
    "ordered": ORDER_OPTS,
}


def check_path(path, st, tname, full_pair, reads_u):
    """What GrX_Stats must show for the forced path (``full_pair``: (monoid, pair) over a full operand is computed from the row
    lengths alone, method 5; ``reads_u``: the multiply reads the operand's values, so the hot-column table is built).
    No statistic tells the short-row kernels (short_kernel 0 / 1 / 5 / 6) apart: for them only the split itself -- long rows on the
    long-row kernels, long_entries > 0 -- is asserted.  Nor does one tell the cold tiles from the cold strips: "cold_tiles" asserts the
    hot / cold layout (long_kernel 4) with a hot table in use."""
    if path == "default" or full_pair and st["method"] == 5:
        return
    assert st["method"] != 5, (path, st)
    if path == "ordered":
        assert st["ordered"] == 1, (path, st)
        return
    forced = {"long1": 1, "long2": 2, "long3": 3, "long4": 4, "long5": 5, "hot_cold": 4, "cold_tiles": 4}.get(path, DEFAULT_LONG_KERNEL)
    assert st["long_kernel"] == long_want(forced, tname) and st["long_entries"] > 0, (path, st)
    if path in ("hot_cold", "cold_tiles") and reads_u:
        assert st["hot_k"] > 0, (path, st)  # (the hot-column table really was in use)


@pytest.mark.parametrize("tname", ALL_TYPES)
@pytest.mark.parametrize("path", list(MXV_PATHS))
def test_mxv_paths(gb, path, tname):
    """Every semiring of the type on one forced mxv path: a plain product, and a masked one with an accumulator (over an old w of the
    same domain), against the oracle; the operand full for the ordered layouts' row tiles, sparse otherwise."""
    from graphblas_amd import device

    seed = list(MXV_PATHS).index(path) * 16 + ALL_TYPES.index(tname)
    rng = np.random.default_rng(5100 + seed)
    m, n = 300, 2600
    square = path == "ordered"
    if square:
        m = n
    try:
        set_opts(MXV_PATHS[path])
        srs = semirings_for(tname)
        if square:  # (the ordered layouts of a 2600-vertex graph take seconds per semiring under the emulator: a rotating half of them)
            srs = srs[seed % 2::2]
        for k, sr in enumerate(srs):
            monoid = sr.split("_", 1)[0]
            dom = domain_for(tname, sr)
            rows, cols, vals = skewed(rng, m, n, tname, dom, hubs=6 + n // 150 if square else 0)
            ui, uv = rand_vec(rng, n, [1.0, 0.5, 0.08][(seed + k) % 3], tname, dom)
            wi, wv = rand_vec(rng, m, 0.5, tname, dom)
            mi, mv = rand_vec(rng, m, 0.5, tname, "special" if tname in FP_TYPES else "signed")
            oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
            ou = O.OVec(n, ui, uv, tname)
            A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
            u = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
            S = getattr(gb.semiring, sr)
            for call in range(2):  # (the second call finds the layouts built)
                got = A.mxv(u, S).new()
                check_path(path, device.last_stats(), tname, ui.size == n and sr.endswith("pair"),
                           not sr.endswith(("pair", "first")))
                same_vec(got, O.mxv(oa, ou, sr), monoid, (path, tname, sr, call))
            # a value mask of the type (-0.0 false, NaN and negatives true), complemented or not, and an accumulator
            accum = {"BOOL": "lor"}.get(tname, ["min", "max", "plus"][(seed + k) % 3])
            comp = bool((seed + k) & 1)
            w = gb.Vector.from_coo(wi, wv, dtype=tname, size=m)
            mk = gb.Vector.from_coo(mi, mv, dtype=tname, size=m)
            w(~mk.V if comp else mk.V, accum=accum) << A.mxv(u, S)
            exp = O.mxv(oa, ou, sr, w=O.OVec(m, wi, wv, tname), mask=O.OVec(m, mi, mv, tname), mask_comp=comp, accum=accum)
            same_vec(w, exp, zero_sign_rule(monoid, accum), (path, tname, sr, "masked"))
    finally:
        reset_opts()


@pytest.mark.parametrize("tname", FP_TYPES)
def test_mxv_plus_over_reals_within_bound(gb, tname):
    """plus_times / plus_plus over normal reals of both signs (magnitudes 1e-15 .. 1e15, so no partial sum overflows): every row within
    the error bound of its exact sum, on the default path and on the split kernels."""
    rng = np.random.default_rng(77 + FP_TYPES.index(tname))
    m, n = 300, 2600
    rows, cols, _ = skewed(rng, m, n, tname, "signed")
    vals = rand_vals(rng, rows.size, tname, "signed", span=15)
    ui = np.flatnonzero(rng.random(n) < 0.6)
    uv = rand_vals(rng, ui.size, tname, "signed", span=15)
    oa, ou = O.OMat.from_coo(rows, cols, vals, m, n, tname), O.OVec(n, ui, uv, tname)
    try:
        for opts in ((), SPLIT + ((b"long_kernel", 4), (b"hot_min_cols", 8), (b"hot_k", 256))):
            set_opts(opts)
            A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
            u = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
            for mult in ("times", "plus"):
                gi, gv = A.mxv(u, getattr(gb.semiring, f"plus_{mult}")).new().to_coo()
                plus_within_bound(gi, gv, oa, ou, mult, (tname, mult, opts))
    finally:
        reset_opts()


def test_value_dictionary_and_fill_with_negatives(gb):
    """FP32 min_plus on the ordered layouts: a matrix of <= 256 distinct values with negatives and -0.0 takes the value dictionary (on and
    off); a NaN or an infinity in the matrix switches the dictionary off.  The absorbing fill runs with negative, near-limit operands and
    is switched off by an infinite or NaN operand value.  All against the oracle."""
    from graphblas_amd import device

    rng = np.random.default_rng(4242)
    n = 2600
    rows, cols, _ = skewed(rng, n, n, "FP32", "small", hubs=6 + n // 150)
    palette = np.concatenate([np.arange(-100, 100, dtype=np.float32) * np.float32(0.75), np.float32([-0.0, 0.0, -3e30, 3e30])])
    vals = palette[rng.integers(0, palette.size, rows.size)]
    ui = np.flatnonzero(rng.random(n) < 0.3)
    uv = rand_vals(rng, ui.size, "FP32", "signed")
    try:
        for vd in (1, 0):
            for bad in (None, np.nan, np.inf):
                v = vals.copy()
                if bad is not None:
                    v[::97] = np.float32(bad)
                set_opts(ORDER_OPTS + ((b"hot_k", 1 << 20), (b"value_dict", vd)))
                A = gb.Matrix.from_coo(rows, cols, v, dtype="FP32", nrows=n, ncols=n)
                oa = O.OMat.from_coo(rows, cols, v, n, n, "FP32")
                for sr in ("min_plus", "max_plus"):
                    for uvals in (uv, np.where(np.arange(ui.size) % 50 == 0, np.float32(np.nan), uv).astype(np.float32),
                                  np.where(np.arange(ui.size) % 50 == 0, np.float32(np.inf), uv).astype(np.float32)):
                        u = gb.Vector.from_coo(ui, uvals, dtype="FP32", size=n)
                        got = A.mxv(u, getattr(gb.semiring, sr)).new()
                        st = device.last_stats()
                        where = (vd, bad, sr, uvals is uv)
                        assert st["ordered"] == 1, (where, st)
                        want_vd = (np.unique(v.view(np.uint32)).size if bad is None else 0) if vd else 0  # (distinct bit patterns: -0.0 is a value of its own)
                        assert st["value_dict"] == want_vd, (where, st)
                        # the fill needs finite matrix values (known from the dictionary) and a finite, bounded operand
                        assert st["fill_absent"] == (1 if (vd and bad is None and uvals is uv) else 0), (where, st)
                        same_vec(got, O.mxv(oa, O.OVec(n, ui, uvals, "FP32"), sr), sr.split("_")[0], where)
    finally:
        reset_opts()


@pytest.mark.parametrize("tname", ALL_TYPES)
@pytest.mark.parametrize("push", ["pull", "push_small", "push_whole"])
def test_vxm_paths(gb, tname, push):
    """vxm on the pull kernels over the cached transpose and on the push kernels (forced): a frontier of a few entries, and one of
    thousands (whole workgroups of it), masked with a complement and an accumulator."""
    from graphblas_amd import _lib, device

    rng = np.random.default_rng(6100 + 16 * ["pull", "push_small", "push_whole"].index(push) + ALL_TYPES.index(tname))
    m, n = 2600, 400
    try:
        if push != "pull":
            _lib.lib.GrX_option_set(b"push_mode", 2)
        for k, sr in enumerate(semirings_for(tname)):
            monoid = sr.split("_", 1)[0]
            dom = domain_for(tname, sr)
            rows, cols, vals = skewed(rng, m, n, tname, dom, lens=(9, 64, 65, 300))
            dens = {"pull": 0.5, "push_small": 0.003, "push_whole": 0.9}[push]
            ui, uv = rand_vec(rng, m, dens, tname, dom)
            oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
            ou = O.OVec(m, ui, uv, tname)
            A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
            u = gb.Vector.from_coo(ui, uv, dtype=tname, size=m)
            got = u.vxm(A, getattr(gb.semiring, sr)).new()
            if push != "pull":
                assert device.last_stats()["method"] == (2 if ui.size and rows.size else 6), device.last_stats()
            else:
                assert device.last_stats()["method"] not in (2, 6), device.last_stats()  # (pulled: not pushed, not the write rule alone)
            same_vec(got, O.vxm(ou, oa, sr), monoid, (push, tname, sr))
            wi, wv = rand_vec(rng, n, 0.5, tname, dom)
            mi, mv = rand_vec(rng, n, 0.5, "BOOL", "small")
            accum = {"BOOL": "lor"}.get(tname, ["min", "max", "plus"][k % 3])
            w = gb.Vector.from_coo(wi, wv, dtype=tname, size=n)
            mk = gb.Vector.from_coo(mi, mv, dtype="BOOL", size=n)
            w(~mk.S, accum=accum) << u.vxm(A, getattr(gb.semiring, sr))
            exp = O.vxm(ou, oa, sr, w=O.OVec(n, wi, wv, tname), mask=O.OVec(n, mi, mv, "BOOL"), mask_comp=True, mask_struct=True, accum=accum)
            same_vec(w, exp, zero_sign_rule(monoid, accum), (push, tname, sr, "masked"))
    finally:
        reset_opts()


MXM_PATHS = ("rows", "mask_driven", "mask_units", "comp_mask", "units")


@pytest.mark.parametrize("tname", ALL_TYPES)
@pytest.mark.parametrize("path", MXM_PATHS)
def test_mxm_paths(gb, tname, path):
    """mxm: the row kernels, the mask-driven product (row kernels and (row, window) units), the complemented mask fused into the
    product, and heavy rows as unit classes with a limited bitmap pool."""
    from graphblas_amd import device

    rng = np.random.default_rng(7100 + 16 * MXM_PATHS.index(path) + ALL_TYPES.index(tname))
    try:
        if path == "mask_driven":
            set_opts(((b"mxm_mask_mode", 2), (b"mxm_masked_units_min_flops", 64 << 20)))
        elif path == "mask_units":
            set_opts(((b"mxm_mask_mode", 2), (b"mxm_masked_units_min_flops", 0)))
        elif path == "units":
            set_opts(((b"mxm_bitmap_pool_cap", 3),))
        for sr in semirings_for(tname):
            monoid = sr.split("_", 1)[0]
            dom = domain_for(tname, sr)
            if path == "units":
                m, k, n = 9, 220, 40_000
                br = np.repeat(np.arange(k), 193)
                bc = np.concatenate([np.sort(np.concatenate([rng.choice(16384, 150, replace=False), 16384 + rng.choice(16384, 40, replace=False),
                                                             32768 + rng.choice(n - 32768, 3, replace=False)])) for _ in range(k)])
                deg = np.array([100, 0, 25, 3, 180, 1, 60, 0, 26])
                ar = np.repeat(np.arange(m), deg)
                ac = np.concatenate([np.sort(rng.choice(k, d, replace=False)) for d in deg])
            else:
                m, k, n = 200, 150, 180
                ar, ac, _ = skewed(rng, m, k, tname, dom, lens=(40, 100))
                br, bc, _ = skewed(rng, k, n, tname, dom, lens=(60, 150))
            av = shape_rows(rng, ar, rand_vals(rng, ar.size, tname, dom), tname)
            bv = rand_vals(rng, br.size, tname, dom)
            oa, ob = O.OMat.from_coo(ar, ac, av, m, k, tname), O.OMat.from_coo(br, bc, bv, k, n, tname)
            A = gb.Matrix.from_coo(ar, ac, av, dtype=tname, nrows=m, ncols=k)
            B = gb.Matrix.from_coo(br, bc, bv, dtype=tname, nrows=k, ncols=n)
            S = getattr(gb.semiring, sr)
            if path in ("rows", "units"):
                got = A.mxm(B, S).new()
                # (method 3: the unmasked product.  No statistic tells the (row, window) units or the bitmap pool from the row kernels;
                #  "units" builds the rows test_random_parity.py's test_mxm_unit_classes checks the classes of)
                assert device.last_stats()["method"] == 3, device.last_stats()
                same_mat(got, O.mxm(oa, ob, sr), monoid, (path, tname, sr))
                continue
            mr = rng.integers(0, m, 3000)
            mc = rng.integers(0, n, 3000)
            mval = rand_vals(rng, mr.size, "FP32", "special")
            M = gb.Matrix.from_coo(mr, mc, mval, dtype="FP32", nrows=m, ncols=n, dup_op=gb.binary.first)
            om = O.OMat.from_coo(mr, mc, mval, m, n, "FP32", dup_op="first")
            if path == "comp_mask":
                got = A.mxm(B, S).new(mask=~M.S)
                assert device.last_stats()["method"] == 7, device.last_stats()  # the complemented mask was fused into the product
                same_mat(got, O.mxm(oa, ob, sr, mask=om, mask_comp=True, mask_struct=True), monoid, (path, tname, sr))
            else:
                got = A.mxm(B, S).new(mask=M.S)
                # the mask-driven path really ran (no statistic tells its (row, window) units -- mask_units -- from its row kernels)
                assert device.last_stats()["method"] == 4, device.last_stats()
                same_mat(got, O.mxm(oa, ob, sr, mask=om, mask_struct=True), monoid, (path, tname, sr))
                # a value mask of FP32: -0.0 is false, NaN and negatives are true
                got = A.mxm(B, S).new(mask=M.V)
                same_mat(got, O.mxm(oa, ob, sr, mask=om), monoid, (path, tname, sr, "value mask"))
    finally:
        reset_opts()


@pytest.mark.parametrize("tname", [t for t in ALL_TYPES if t not in ("BOOL",) + FP_TYPES])
def test_mxm_streamed_row_batches(gb, tname):
    """GrX_mxm_streamed over full-range integers: count and checksum of the product in row batches (budgets down to one row per
    batch) against the oracle's product.  (The checksum adds a floating-point value's integer part, which cannot see NaN or a zero's
    sign: the floating-point types are left to the materialised products above.)"""
    import ctypes

    from graphblas_amd import _lib

    rng = np.random.default_rng(7700 + ALL_TYPES.index(tname))
    m, k, n = 24, 120, 200
    ar, ac, av = skewed(rng, m, k, tname, "signed", lens=(40, 100))
    br, bc, bv = skewed(rng, k, n, tname, "signed", lens=(60, 150))
    A = gb.Matrix.from_coo(ar, ac, av, dtype=tname, nrows=m, ncols=k)
    B = gb.Matrix.from_coo(br, bc, bv, dtype=tname, nrows=k, ncols=n)
    oa, ob = O.OMat.from_coo(ar, ac, av, m, k, tname), O.OMat.from_coo(br, bc, bv, k, n, tname)
    for sr in ("plus_times", "min_plus", "max_plus"):
        ref = O.mxm(oa, ob, sr)
        want = sum(int(x) for x in ref.values.tolist()) & 0xFFFFFFFFFFFFFFFF  # (a signed value enters sign-extended)
        for budget in (1, 4096, 1 << 30):
            nv, cs, fl, nb = (ctypes.c_uint64(0) for _ in range(4))
            rc = _lib.lib.GrX_mxm_streamed(getattr(gb.semiring, sr)[tname]._carg, A._carg, B._carg, budget, ctypes.byref(nv), ctypes.byref(cs),
                                           ctypes.byref(fl), ctypes.byref(nb))
            assert rc == 0
            assert nb.value >= 1 and (budget > 1 or nb.value > m // 4), (sr, budget, nb.value)  # (really in row batches)
            assert nv.value == ref.nvals and cs.value == want, (tname, sr, budget, nv.value, ref.nvals, cs.value, want)


def test_value_dictionary_padding_under_plus_times(gb):
    """The fast hot-strip kernel over dictionary-coded FP32 values under plus_times: a padding entry takes code 0, whose value may be
    negative or -0.0 -- its product must still be -0.0, the sum's seed, or a row of -0.0 products comes back as +0.0.  Every matrix value
    here is negative or -0.0, so code 0 is one of them; long rows of -0.0 against a full, positive operand must sum to -0.0."""
    from graphblas_amd import device

    rng = np.random.default_rng(4343)
    n = 2600
    rows, cols, _ = skewed(rng, n, n, "FP32", "small", hubs=6 + n // 150)
    palette = np.concatenate([-np.arange(1, 120, dtype=np.float32) * np.float32(0.5), np.float32([-0.0])])
    vals = palette[rng.integers(0, palette.size, rows.size)]
    lens = np.bincount(rows, minlength=n)
    negzero = rng.permutation(np.flatnonzero(lens >= 65))[:8]  # (long rows: they run on the hot strips; lengths leave padding)
    vals[np.isin(rows, negzero)] = np.float32(-0.0)
    u = gb.Vector.from_coo(np.arange(n), rng.integers(1, 9, n).astype(np.float32), dtype="FP32", size=n)
    ou = O.OVec(n, np.arange(n), u.to_coo()[1], "FP32")
    oa = O.OMat.from_coo(rows, cols, vals, n, n, "FP32")
    try:
        set_opts(ORDER_OPTS + ((b"hot_k", 1 << 20), (b"value_dict", 1)))
        A = gb.Matrix.from_coo(rows, cols, vals, dtype="FP32", nrows=n, ncols=n)
        got = A.mxv(u, gb.semiring.plus_times).new()
        st = device.last_stats()
        assert st["ordered"] == 1 and st["value_dict"] > 0 and st["long_kernel"] == 4 and st["hot_k"] > 0, st
        same_vec(got, O.mxv(oa, ou, "plus_times"), "plus", "dictionary padding")
        gi, gv = got.to_coo()
        at = np.searchsorted(gi, negzero)
        assert np.array_equal(gi[at], negzero) and np.all(gv[at] == 0) and np.all(np.signbit(gv[at])), gv[at]
    finally:
        reset_opts()


def test_fill_limit(gb):
    """The absorbing fill's bound on the operand (FLT_MAX - the largest matrix magnitude, so no finite product overflows to the
    identity): an operand just under the bound takes the fill, one just over it does not -- both against the oracle, with negative values."""
    from graphblas_amd import device

    rng = np.random.default_rng(4545)
    n = 2600
    rows, cols, _ = skewed(rng, n, n, "FP32", "small", hubs=6 + n // 150)
    palette = np.arange(-100, 101, dtype=np.float32) * np.float32(0.5)
    vals = palette[rng.integers(0, palette.size, rows.size)]
    absmax = float(np.abs(vals).max())
    limit = float(np.finfo(np.float32).max) - absmax
    ui = np.flatnonzero(rng.random(n) < 0.3)
    base = rand_vals(rng, ui.size, "FP32", "signed")
    oa = O.OMat.from_coo(rows, cols, vals, n, n, "FP32")
    try:
        set_opts(ORDER_OPTS + ((b"hot_k", 1 << 20), (b"value_dict", 1), (b"fill_absent", 1)))
        A = gb.Matrix.from_coo(rows, cols, vals, dtype="FP32", nrows=n, ncols=n)
        for sr, sign in (("min_plus", 1.0), ("max_plus", -1.0)):
            for near, want in ((limit * 0.999, 1), (float(np.finfo(np.float32).max), 0)):  # (the kernel admits up to limit * (1 - 1e-6))
                uv = base.copy()
                uv[:: 40] = np.float32(sign * near)  # (one operand value in forty at the magnitude under test)
                u = gb.Vector.from_coo(ui, uv, dtype="FP32", size=n)
                got = A.mxv(u, getattr(gb.semiring, sr)).new()
                st = device.last_stats()
                assert st["ordered"] == 1 and st["fill_absent"] == want, (sr, near, st)
                same_vec(got, O.mxv(oa, O.OVec(n, ui, uv, "FP32"), sr), sr.split("_")[0], (sr, near))
    finally:
        reset_opts()


@pytest.mark.parametrize("tname", ALL_TYPES)
def test_vector_ops(gb, tname):
    """reduce (against the oracle's fold: fmin / fmax, left-to-right sums with no seed), ewise_add / ewise_mult with min / max / plus,
    the scalar assign with the accumulators, where the old w holds NaN, +-inf, -0.0 or the type's extremes."""
    rng = np.random.default_rng(8100 + ALL_TYPES.index(tname))
    n = 700
    fp = tname in FP_TYPES
    for dom in (("special", "exact") if fp else ("signed",)):
        ui, uv = rand_vec(rng, n, 0.5, tname, dom)
        vi, vv = rand_vec(rng, n, 0.5, tname, dom)
        ou, ov = O.OVec(n, ui, uv, tname), O.OVec(n, vi, vv, tname)
        U = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
        V = gb.Vector.from_coo(vi, vv, dtype=tname, size=n)
        mons = ["lor", "land", "lxor"] if tname == "BOOL" else (["min", "max"] if dom == "special" else ["plus", "min", "max", "times"])
        if not fp and tname != "BOOL":
            mons = ["plus", "times", "min", "max"]
        for mon in mons:
            got = U.reduce(getattr(gb.monoid, mon)).new().value
            ref = O.vec_reduce(ou, mon)
            if fp:
                if mon == "times" and np.isfinite(ref):
                    # (a product of thousands of small integers rounds: the order of the fold changes the last bits)
                    assert np.isclose(got, ref, rtol=1e-5 if tname == "FP32" else 1e-12), (dom, mon, got, ref)
                else:
                    same_fp(np.array([got], O.NP_OF[tname]), np.array([ref], O.NP_OF[tname]), mon, (tname, dom, mon))
            else:
                assert got == ref, (tname, mon, got, ref)
        # the findings themselves: an all-NaN vector under min / max reduces to NaN, a sum of -0.0 to -0.0
        if fp:
            nan2 = gb.Vector.from_coo([1, 5], np.array([np.nan, np.nan], O.NP_OF[tname]), dtype=tname, size=n)
            for mon in ("min", "max"):
                assert np.isnan(nan2.reduce(getattr(gb.monoid, mon)).new().value), mon
            nz = gb.Vector.from_coo([1, 5, 9], np.array([-0.0] * 3, O.NP_OF[tname]), dtype=tname, size=n)
            z = nz.reduce(gb.monoid.plus).new().value
            assert z == 0 and np.signbit(z), z
        ops = ["lor", "land", "lxor"] if tname == "BOOL" else ["min", "max", "plus"]
        for op in ops:
            sem = op if op in ("min", "max") else "plus"
            same_vec(U.ewise_add(V, getattr(gb.binary, op)).new(), O.vec_ewise(ou, ov, op, union=True), sem, (tname, dom, op, "add"))
            same_vec(U.ewise_mult(V, getattr(gb.binary, op)).new(), O.vec_ewise(ou, ov, op, union=False), sem, (tname, dom, op, "mult"))
        scalars = rand_vals(rng, 4, tname, dom)
        for s in scalars:
            for accum in ((None, "lor") if tname == "BOOL" else (None, "min", "max", "plus")):
                W = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
                W(accum=accum)[:] << s.item()
                same_vec(W, O.vec_assign_scalar(ou, s, accum=accum), accum if accum in ("min", "max") else "plus", (tname, dom, s, accum))


@pytest.mark.parametrize("tname", FP_TYPES)
def test_findings_minimal(gb, tname):
    """The minimal cases: a row whose every product is NaN under a min / max monoid is a present NaN (not the identity +-inf); a sum of
    -0.0 products is -0.0 -- in mxv, vxm and mxm."""
    np_t = O.NP_OF[tname]
    nan, nz = np_t(np.nan), np_t(-0.0)
    rows, cols = np.array([0, 0, 1, 1, 2]), np.array([0, 1, 0, 1, 1])
    vals = np.array([nan, nan, nz, nz, 3], np_t)
    A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=3, ncols=2)
    u = gb.Vector.from_coo([0, 1], np.ones(2, np_t), dtype=tname, size=2)
    for sr in ("min_plus", "max_plus", "max_first", "plus_times"):
        gi, gv = A.mxv(u, getattr(gb.semiring, sr)).new().to_coo()
        assert gi.tolist() == [0, 1, 2], (sr, gi)
        assert np.isnan(gv[0]), (sr, gv)
        if sr == "plus_times":
            assert gv[1] == 0 and np.signbit(gv[1]), (sr, gv)
        # (u' A': the multiply's operands swap -- max_first of mxv is max_second here)
        gi, gv = u.vxm(A.T, getattr(gb.semiring, sr.replace("first", "second"))).new().to_coo()
        assert np.isnan(gv[0]), ("vxm", sr, gv)
        if sr == "plus_times":
            assert gv[1] == 0 and np.signbit(gv[1]), ("vxm", sr, gv)
        B = gb.Matrix.from_coo([0, 1], [0, 0], np.ones(2, np_t), dtype=tname, nrows=2, ncols=1)
        cp, cj, cx = A.mxm(B, getattr(gb.semiring, sr)).new().to_csr()
        assert np.isnan(cx[0]), ("mxm", sr, cx)
        if sr == "plus_times":
            assert cx[1] == 0 and np.signbit(cx[1]), ("mxm", sr, cx)


@pytest.mark.gpu
@pytest.mark.parametrize("tname", [t for t in ALL_TYPES if t != "BOOL"])
def test_rmat_special_values_gpu(tname):
    """One scale-16 R-MAT graph per type, values from the 'special' (floating point) / 'signed' (integer) domain with shaped rows,
    min_plus and max_first (plus plus_times for the integers, which wrap exactly) against the oracle."""
    import torch

    gb = bind("gpu")
    from graphblas_amd import synthetic

    scale = 16
    n = 1 << scale
    indptr, col = synthetic.rmat_csr(scale, device="cuda")
    ip, cj = indptr.cpu().numpy(), col.cpu().numpy().astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(ip))
    rng = np.random.default_rng(16)
    dom = "special" if tname in FP_TYPES else "signed"
    vals = shape_rows(rng, rows, rand_vals(rng, rows.size, tname, dom), tname)
    ui = np.flatnonzero(rng.random(n) < 0.5)
    uv = rand_vals(rng, ui.size, tname, dom)
    oa, ou = O.OMat.from_coo(rows, cj, vals, n, n, tname), O.OVec(n, ui, uv, tname)
    A = gb.Matrix.from_coo(rows, cj, vals, dtype=tname, nrows=n, ncols=n)
    u = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
    for sr in ("min_plus", "max_first") + (() if tname in FP_TYPES else ("plus_times",)):
        same_vec(A.mxv(u, getattr(gb.semiring, sr)).new(), O.mxv(oa, ou, sr), sr.split("_")[0], (tname, sr))
    torch.cuda.synchronize()
