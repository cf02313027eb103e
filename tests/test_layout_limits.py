"""The cached layouts of the pull mxv at the limits of their packed fields.

Every layout of an ordered matrix packs indices into narrow fields, gives one bit pattern a second meaning as padding and falls back
to a wider form when a field cannot hold the matrix.  The random suites never come near those limits; the matrices here are built
so that one entry sits exactly ON each limit and one just behind it.  They carry GrX_Matrix_hint_ranked, so the layouts are built
in the caller's own index order and the test decides which column code, which long-row slot and which tile row an entry gets.

Every case compares with the oracle element for element (small integer values: plus_times and min_plus are exact), three ways: the
plain product, the product under a complemented structural mask with an accumulator, and a second call on the cached layouts.  An
entry on a limit carries a value no other entry of its row has.  Two witnesses show that the layout under test was really built:
GrX_last_stats, and GrX_Matrix_cache_bytes of the same matrix with the narrow form switched on and off -- smaller where the narrow
form fits, equal where the builder fell back.

What the geometry rests on (python-graphblas_amd/csrc):
* a SLOT is the rank of a row among the LONG rows (k_split_fill: lidx, the scan of the "row has >= split_min_len entries" flags) --
  not its row index: short and empty rows in between do not count;
* the entries of the long rows are sorted by (class, slot); a SEGMENT is one (class, row) run, padded to whole lanes of 8 entries;
  64 consecutive lanes of a class are one chunk (k_strip_place), every class is padded to whole chunks;
* the class of a resident column code c is strip_cls_of_line(c >> 5, ncls): lines of 32 codes dealt boustrophedon to the classes;
  codes below cls_lds_lim = min(hot_k, LONG_LDS_WORDS * 4 / max(4, sizeof(T)) * ncls) are resident, the others are cold;
* cold column ranges (ensure_ordered) are whole blocks of 4096 codes from cls_lds_lim on; a range closes at 2 MiB of operand
  (2^19 FP32 codes, 2^18 FP64), or -- ctile_pack on -- at 2^19 - 4096 codes if that is less, or earlier when it has collected
  1/32 of the cold references;
* the cold tiles number their long-row slots inside blocks of ct_slots = 8192 (packed words, any type), else 16384 (8-byte
  types: 8192);
* the sorted row tiles cut the short part by groups of 64 rows: a tile closes at rows_cap = rtile_rows (8-byte types: half) rows or
  at rtile_entries entries; its entries go, sorted by column code, into lane-transposed blocks of 256, padded with word
  0xffffffff / tag rows_cap."""
import numpy as np
import pytest

from oracle import grb_oracle as O
from tests.backend import DEVICES, bind
from tests.test_vertex_order import ORDER_OPTS, reset_opts, set_opts
from tests.values import same_vec

# (LONG_LDS_WORDS, grb_mxv_long.inc: words of the operand's head a workgroup of the strip kernels keeps in LDS.  Should the library's value
#  change, test_last_resident_code_of_a_class_head fails on its cache_bytes relations: the boundary would no longer lie where it builds it.)
LDS_WORDS = 39936
RT_BLOCK_ENTRIES = 256  # (a sorted row tile's entries are stored in whole blocks of 256: RT_EPL * 64 lanes, grb_mxv_rtile.inc)
RT_TILE_RECORD = 36     # (bytes GrX_Matrix_cache_bytes counts per sorted row tile: its record and its place in the hand-out order)
CT_EPL = 4              # (a cold tile's entries are padded to units of 4, grb_mxv_ctile.inc)
CT_MAX_ENTRIES = 16384  # (a (column range, slot block) pair with more cold entries is cut into equal pieces)


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


def _np(tname):
    return O.NP_OF[tname]


def _coo(parts, tname):
    """[(row, cols, vals), ...] -> sorted COO arrays (no duplicates allowed)."""
    rows = np.concatenate([np.full(len(c), r, np.int64) for r, c, _ in parts])
    cols = np.concatenate([np.asarray(c, np.int64) for _, c, _ in parts])
    vals = np.concatenate([np.asarray(v) for _, _, v in parts]).astype(_np(tname))
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    assert rows.size == np.unique(rows * (int(cols.max()) + 1) + cols).size, "duplicate entries"
    return rows, cols, vals


def _operand(n, tname):
    """A full operand of small integers that differ between neighbouring columns (an entry read at the wrong column shows)."""
    if tname == "BOOL":
        return np.arange(n), np.ones(n, bool)
    return np.arange(n), (1 + (np.arange(n) * 5 + np.arange(n) // 32) % 11).astype(_np(tname))


def _build(gb, rows, cols, vals, m, n, tname, ranked=True):
    from graphblas_amd import device

    A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
    if ranked:
        device.matrix_hint_ranked(A)
    return A


def _check(gb, A, oa, tname, keep_rows, stats, srs=None, operand=None):
    """The plain product, the product under a complemented structural mask with an accumulator, and the same call again on the
    cached layouts -- each against the oracle, each with the statistics the case names.  The rows of `keep_rows` are never in the
    mask (complemented: they are computed)."""
    from graphblas_amd import device

    m, n = oa.nrows, oa.ncols
    rng = np.random.default_rng(12345)
    ui, uv = operand if operand is not None else _operand(n, tname)
    u = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
    ou = O.OVec(n, ui, uv, tname)
    in_mask = rng.random(m) < 0.5
    in_mask[np.asarray(keep_rows, np.int64)] = False
    mi = np.flatnonzero(in_mask)
    mk = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=m)
    om = O.OVec(m, mi, np.ones(mi.size, bool), "BOOL")
    wi = np.flatnonzero(rng.random(m) < 0.6)
    wv = np.ones(wi.size, bool) if tname == "BOOL" else (1 + wi % 9).astype(_np(tname))
    ow = O.OVec(m, wi, wv, tname)
    for sr in srs or (("lor_land",) if tname == "BOOL" else ("plus_times", "min_plus")):
        accum = {"plus_times": "plus", "min_plus": "min", "lor_land": "lor"}[sr]
        exp_plain = O.mxv(oa, ou, sr)
        exp_masked = O.mxv(oa, ou, sr, w=ow, mask=om, mask_comp=True, mask_struct=True, accum=accum)
        for rep in range(2):  # (the second round runs on the cached layouts and the operands the library kept)
            got = A.mxv(u, getattr(gb.semiring, sr)).new()
            st = device.last_stats()
            for k, want in stats.items():
                assert (st[k] in want if isinstance(want, tuple) else st[k] == want), (sr, rep, k, st)
            same_vec(got, exp_plain, where=f"{sr} plain, call {rep}")
            w = gb.Vector.from_coo(wi, wv, dtype=tname, size=m)
            w(~mk.S, accum=getattr(gb.binary, accum)) << A.mxv(u, getattr(gb.semiring, sr))
            st = device.last_stats()
            for k, want in stats.items():
                assert (st[k] in want if isinstance(want, tuple) else st[k] == want), (sr, rep, k, st)
            same_vec(w, exp_masked, where=f"{sr} masked, call {rep}")


def _first_bytes(gb, A, n, tname, ordered=1):
    """Bytes of the layouts the library has cached for A after ONE product of a full operand (the layouts are built at first use).  Every
    byte count of this file is taken here: the figures that are compared come from the same call on matrices built the same way."""
    from graphblas_amd import device

    ui, uv = _operand(n, tname)
    u = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
    A.mxv(u, gb.semiring.lor_land if tname == "BOOL" else gb.semiring.min_plus).new()
    assert device.last_stats()["ordered"] == ordered, device.last_stats()
    return device.matrix_cache_bytes(A)


def _cache_bytes(gb, rows, cols, vals, m, n, tname, opts, ordered=1, ranked=True):
    """Bytes of the cached layouts of the matrix built under `opts`."""
    set_opts(opts)
    A = _build(gb, rows, cols, vals, m, n, tname, ranked)
    return _first_bytes(gb, A, n, tname, ordered)


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. hot strips: 16-bit slot offsets
# ------------------------------------------------------------------------------------------------------------------------------------
def _strip_matrix(dist, kind):
    """Long rows (8 entries each) whose slots run 0 .. dist + 5; hot_k = 256 makes the codes 0 .. 255 resident, 16 classes of one
    line each: class 0 = codes 0 .. 31, class 1 = codes 32 .. 63.  Rows NEAR (slot 2), NEAR + 1 and FAR (slot 2 + dist) hold 8-40
    entries of class 0 and nothing else does: their segments are 1 + 1 + 4 lanes of the ONE chunk of class 0, whose other 58 lanes
    are padding (slot -1 -> 0xffff) -- the chunk's smallest slot is 2, its largest 2 + dist.  All other long rows have their 8 entries
    in class 1 (1026 full chunks).  Short and empty rows lie between the long ones: they take no slot."""
    tname = "FP64" if kind == "fp64" else "FP32"
    n = 2048
    near, far = 2, 2 + dist
    n_long = far + 4
    # (row index of slot s: one empty row before every 64 long rows, one short row behind them -- slots do not count them)
    row_of = lambda s: s + 2 * (s // 64) + 1
    m = row_of(n_long - 1) + 3
    nvals = 257 if kind == "fp32_257" else 200
    slots = np.arange(n_long)
    fill = np.setdiff1d(slots, [near, near + 1, far])
    fr = np.repeat(row_of(fill), 8)
    fc = np.tile(32 + np.arange(8), fill.size) + np.repeat(fill % 3, 8) * 8  # (class 1: codes 32 .. 63)
    fv = 1 + (np.arange(fr.size) * 7 + fr) % nvals
    rows_l, cols_l, vals_l = [fr], [fc], [fv]
    # NEAR: 8 entries; NEAR + 1: 8 entries; FAR: 32 entries (4 lanes) -- codes of class 0 only
    for s, cc, v0 in ((near, np.arange(8), 300), (near + 1, np.arange(4, 12), 310), (far, np.arange(32), 320)):
        rows_l.append(np.full(cc.size, row_of(s)))
        cols_l.append(cc)
        vals_l.append((v0 + np.arange(cc.size)) if kind != "fp32_dict" else 201 + np.arange(cc.size) % 50 + (s % 5))
    # the short rows (1-2 entries, any column)
    sr_rows = np.array([row_of(s) + 1 for s in range(63, n_long, 64)])
    rows_l.append(sr_rows)
    cols_l.append(700 + sr_rows % 900)
    vals_l.append(1 + sr_rows % 7)
    rows = np.concatenate(rows_l).astype(np.int64)
    cols = np.concatenate(cols_l).astype(np.int64)
    vals = np.concatenate(vals_l).astype(_np(tname))
    if kind == "fp32_dict":
        assert np.unique(vals).size <= 256
    elif kind == "fp32_257":
        assert np.unique(vals).size > 256
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order], m, n, tname, [row_of(near), row_of(near + 1), row_of(far)]


def _strip_case(gb, dist, kind):
    from graphblas_amd import device

    rows, cols, vals, m, n, tname, special = _strip_matrix(dist, kind)
    oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
    opts = ORDER_OPTS + ((b"hot_k", 256), (b"hub_min_len", 0), (b"long_classes", 16))
    try:
        set_opts(opts + ((b"strip_slot16", 1),))
        A = _build(gb, rows, cols, vals, m, n, tname)
        narrow = _first_bytes(gb, A, n, tname)
        _check(gb, A, oa, tname, special, {"ordered": 1, "long_kernel": 4, "reorders": 0})
        vd = device.last_stats()["value_dict"]
        assert (vd > 0) == (kind == "fp32_dict"), vd
        wide = _cache_bytes(gb, rows, cols, vals, m, n, tname, opts + ((b"strip_slot16", 0),))
        assert (narrow < wide) if dist == 65534 else (narrow == wide), (narrow, wide)
    finally:
        reset_opts()


@pytest.mark.parametrize("dist", [65534, 65535])
def test_strip_slot16_offset_limit(gb, dist):
    """k_strip_slot16 (grb_mxv_strip.inc: `hi - lo >= 0xffff` raises too_wide): a chunk of class 0 whose real lanes belong to the long
    rows of slots 2, 3 and 2 + dist.  dist = 65534 is offset 0xfffe, the largest one that is not the padding pattern 0xffff: the 16-bit
    slots are kept (cache_bytes smaller than with strip_slot16 = 0); dist = 65535 must fall back to 32-bit slots (equal bytes).  The
    far row's products must arrive either way -- with `>` in place of `>=` its lanes would read as padding.  The chunk's trailing 58
    lanes are padding.  A chunk of padding ONLY -- the `lo == 0x7fffffff` branch of k_strip_slot16 -- cannot be built: ensure_split gives
    class c ceil((raw[c + 1] - raw[c]) / 64) chunks (grb_mxv.hip, the loop over `c < nvc` that fills h_cb / h_shift), nothing for a class
    without lanes, and the real lanes of a class are shifted to the front of its chunks (h_shift), so the first lane of every chunk is a
    real one.  nvc counts the 16 / 8 classes of the rows below the hub level AND the 64 classes of the hub level (own class numbers
    ncls .. ncls + 63: a row's lanes lie in the classes of its own level only), so this holds for both levels; the branch guards the
    builder against a layout it does not make.  FP32 with a value dictionary: k_mxv_hstrip<.., DICT, SLOT16>."""
    _strip_case(gb, dist, "fp32_dict")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fp32_257", "fp64"])
@pytest.mark.parametrize("dist", [65534, 65535])
def test_strip_slot16_offset_limit_other_records(dist, kind):
    """The same for FP32 with 257 distinct values (no dictionary: records with full values) and FP64 (half the LDS slots).  GPU tier
    only: the 65 540 long rows take the emulator 50-57 s per case (measured: 50.1 / 53.5 s fp32_257, 49.7 / 47.8 s fp64); the
    dictionary case above runs there."""
    _strip_case(bind("gpu"), dist, kind)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. sorted row tiles: the word that is padding and an entry at once; the pack / no-pack switch at 2^24 column codes
# ------------------------------------------------------------------------------------------------------------------------------------
def _pack_matrix(n, natural=False):
    """n columns, exactly 256 distinct FP32 values (1 .. 256).  Rows 0 .. 11 are long (64 entries on the first codes: the split is
    built).  256 short rows hold value k + 1 at column TOP, whose code is 2^24 - 1 (row base + k): whichever value the dictionary numbers 255,
    one of them is stored as the word 0xffffffff when TOP has the code 2^24 - 1.  TOP is the largest code of the (one) tile -- with one
    column more the second largest --, so these entries fill the END of the tile's last block of 256, next to its padding words (the tile
    has 1000-odd entries: no multiple of 256).  Every fourth of them also has entries at columns 0, 1 and TOP - 1; with one column more
    the rows base + 3 k also hold column TOP + 1, whose code is 2^24: it must not alias code 0.

    natural: the layouts of the matrix in its natural order (order_mode 0, rows_tile 2) code a column through the hot table -- the
    hot_k = 256 most referred-to columns get the codes below 256 (k_hot_rank), column c of the others the code 256 + c (k_hot_recode).
    The long rows are then 300 rows that hold ALL of the columns 0 .. 255: each of these is referred to 300 times or more, TOP 256 times,
    so the table is exactly the columns 0 .. 255 and TOP = 2^24 - 257 has the code 2^24 - 1."""
    top = (1 << 24) - 1 - (256 if natural else 0)  # (the column whose code is 2^24 - 1)
    n_long, base, m = (300, 400, 2000) if natural else (12, 100, 1500)
    rows_l, cols_l, vals_l = [], [], []
    for r in range(n_long):
        cc = np.arange(256) if natural else np.arange(64) * 3 + r
        rows_l.append(np.full(cc.size, r)); cols_l.append(cc); vals_l.append(1 + (cc * 5 + r) % 256)
    k = np.arange(256)
    rows_l.append(base + k); cols_l.append(np.full(256, top)); vals_l.append(k + 1)
    q = k[::4]
    for c, dv in ((0, 17), (1, 101), (top - 1, 203)):
        rows_l.append(base + q); cols_l.append(np.full(q.size, c)); vals_l.append(1 + (q + dv) % 256)
    if n > top + 1:
        q3 = k[::3]
        rows_l.append(base + q3); cols_l.append(np.full(q3.size, top + 1)); vals_l.append(1 + (q3 + 59) % 256)
    # other short rows
    o = np.arange(base + 300, m, 3)
    rows_l.append(o); cols_l.append(5000 + o * 7); vals_l.append(1 + o % 256)
    rows, cols = np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64)
    vals = np.concatenate(vals_l).astype(np.float32)
    if natural:  # (the hot table is the columns 0 .. 255: nothing else is referred to as often as the least of them)
        cnt = np.bincount(cols, minlength=n)
        assert cnt[:256].min() > cnt[256:].max()
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order], m, n, list(range(base, base + 256))


def _pack_case(gb, n, natural=False):
    from graphblas_amd import device

    rows, cols, vals, m, n, special = _pack_matrix(n, natural)
    assert np.unique(vals).size == 256
    tname = "FP32"
    n_codes = n + (256 if natural else 0)
    top = (1 << 24) - 1 - (256 if natural else 0)  # (the column whose code is 2^24 - 1)
    assert (cols == top).sum() == 256 and cols.max() == n - 1
    oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
    opts = ORDER_OPTS + ((b"hot_k", 256), (b"hub_min_len", 0), (b"lazy_tagged", 1))
    if natural:
        opts += ((b"order_mode", 0), (b"rows_tile", 2))
    ordered = 0 if natural else 1
    try:
        set_opts(opts + ((b"rtile_pack", 1),))
        A = _build(gb, rows, cols, vals, m, n, tname, ranked=not natural)
        narrow = _first_bytes(gb, A, n, tname, ordered)
        stats = {"ordered": ordered, "reorders": 0, "value_dict": 256, "fused_epilogue": 3}
        if natural:
            stats["hot_k"] = 256
        else:
            stats["long_kernel"] = 4
        _check(gb, A, oa, tname, special, stats)
        # a call the tiles do not take (a sparse operand under plus_times): the tagged row groups, whose entries are built now -- from
        # the packed tiles (k_tag_from_tiles, vmode -1: code and column taken apart again; padding told by its tag)
        ui = np.unique(np.concatenate([np.array([0, 1, top - 1, top, n - 1]), np.arange(0, 6000, 5), np.arange(5000, 16000, 7)]))
        uv = (1 + ui % 9).astype(np.float32)
        u = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
        got = A.mxv(u, gb.semiring.plus_times).new()
        st = device.last_stats()
        assert st["ordered"] == ordered and st["fused_epilogue"] == 1, st
        same_vec(got, O.mxv(oa, O.OVec(n, ui, uv, tname), "plus_times"), where="tagged row groups from the tiles")
        wide = _cache_bytes(gb, rows, cols, vals, m, n, tname, opts + ((b"rtile_pack", 0),), ordered, ranked=not natural)
        assert (narrow < wide) if n_codes == 1 << 24 else (narrow == wide), (narrow, wide)
    finally:
        reset_opts()


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_rtile_packed_word_at_2_pow_24_columns(extra):
    """ensure_rtile (`n_codes <= 1 << 24`), k_rtile_place, k_mxv_rtile<.., PACK>, k_tag_from_tiles: with exactly 2^24 columns a
    dictionary-coded matrix keeps code << 24 | column in one word, and the entry (column 2^24 - 1, code 255) IS the padding word
    0xffffffff -- told from padding by its tag alone; with 2^24 + 1 columns the codes go to a stream of their own (equal cache_bytes
    with rtile_pack on and off) and column 2^24 must not lose its top bit.  See _pack_matrix for the geometry.  GPU tier only: the
    16.8 M-entry operand and the per-column passes of the layout build take the emulator 140.3 s (2^24 columns) and 127.9 s
    (2^24 + 1), measured once; both passed there."""
    _pack_case(bind("gpu"), (1 << 24) + extra)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_rtile_packed_word_at_2_pow_24_codes_natural_order(extra):
    """The `+ hot_k` term of n_codes in ensure_rtile: the sorted row tiles of a hot-coded matrix in its natural order (order_mode 0,
    rows_tile 2 -- the ranked hint plays no part there: an ordered twin has hot_identity and n_codes = ncols) number ncols + hot_k codes,
    so the switch lies at 2^24 - 256 columns: there the last column has the code 2^24 - 1 and, with dictionary code 255, the word
    0xffffffff; with one column more its code is 2^24 and the codes leave the word.  See _pack_matrix.  GPU tier only, as the case above
    (the same operand size: the emulator took 263 s and 243 s, measured once on a busy machine; both passed there)."""
    _pack_case(bind("gpu"), (1 << 24) - 256 + extra, natural=True)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. sorted row tiles: row tags at rows_cap
# ------------------------------------------------------------------------------------------------------------------------------------
def _rows_cap_matrix(cap, tname):
    """3 cap + 70 rows, 4096 columns.  Rows 1 .. 16 are long (1200 entries each: more than 30 % of all entries, so the split is built);
    they are empty rows of the short part.  Every other row i holds (0, 0, 1, 1, 2)[i % 5] entries -- fewer than 0.8 (3 cap + 70) <
    rtile_entries = 49152 in all, so only the ROW cap closes tiles: tile t = rows [t cap, (t + 1) cap), the last one 70 rows.  For
    t = 1, 2, 3: row t cap - 1 (tag cap - 1, the largest real one) and row t cap (tag 0 of the next tile) hold two entries with values
    of their own, row t cap - 2 is empty; the last row of the matrix, in the partly filled last tile next to its tag padding, holds two
    such entries too."""
    m, n = 3 * cap + 70, 4096
    is_bool = tname == "BOOL"
    rows_l, cols_l, vals_l = [], [], []
    for r in range(1, 17):
        rows_l.append(np.full(1200, r)); cols_l.append((np.arange(1200) * 3 + r) % n); vals_l.append(1 + (np.arange(1200) + r) % 200)
    special = [m - 1]
    for t in (1, 2, 3):
        special += [t * cap - 1, t * cap]
    empty = [t * cap - 2 for t in (1, 2, 3)]
    i = np.arange(17, m)
    i = i[~np.isin(i, special + empty)]
    cnt = np.array([0, 0, 1, 1, 2])[i % 5]
    rr = np.repeat(i, cnt)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    kth = np.arange(rr.size) - np.repeat(first, cnt)
    rows_l.append(rr); cols_l.append((rr * 13 + kth * 1777) % n); vals_l.append(1 + (rr + kth) % 200)
    for j, r in enumerate(special):
        rows_l.append(np.full(2, r)); cols_l.append(np.array([(r * 13) % n, (r * 13 + 2048) % n])); vals_l.append(np.array([201 + 2 * j, 202 + 2 * j]))
    rows, cols = np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64)
    vals = np.ones(rows.size, bool) if is_bool else np.concatenate(vals_l).astype(_np(tname))
    order = np.lexsort((cols, rows))
    assert (np.diff(rows[order] * n + cols[order]) > 0).all()
    short = rows.size - 16 * 1200
    assert short < 49152 and 16 * 1200 > 0.3 * rows.size
    return rows[order], cols[order], vals[order], m, n, special


@pytest.mark.parametrize("tname", ["FP32", "FP64", "INT64", "BOOL"])
@pytest.mark.parametrize("rtile_rows", [8192, 16384])
def test_rtile_row_tags_at_rows_cap(gb, rtile_rows, tname):
    """k_rtile_heads / k_rtile_keys / k_rtile_pad_tags (grb_mxv_rtile.inc), k_mxv_rtile and k_mxv_rtile_bool: tiles that the row cap
    closes -- rows_cap = rtile_rows, half of it for the 8-byte types FP64 and INT64 -- so that a u16 row tag reaches rows_cap - 1 while rows_cap itself is the tag
    of padding.  See _rows_cap_matrix.  Afterwards a call the tiles do not take (max_second) builds the tagged row groups from the
    tiles (k_tag_from_tiles: `tag >= rows_cap` is padding).

    Witness that the row cap -- this rtile_rows, halved for this type -- closed the tiles: the same matrix under the OTHER rtile_rows.
    The 3 cap + 70 rows make 4 tiles here and 2 tiles (cap doubled) or 7 tiles (cap halved) there.  GrX_Matrix_cache_bytes counts a
    tile's entries in whole blocks of 256 and 36 bytes per tile, and nothing else in it depends on rtile_rows: the two byte counts
    differ, modulo 256, by 36 times the difference of the tile counts.  A cap that ignored rtile_rows (difference 0) or the halving
    (2 and 1 tiles, or 2 and 4) gives another residue."""
    from graphblas_amd import device

    cap = rtile_rows // 2 if tname in ("FP64", "INT64") else rtile_rows
    rows, cols, vals, m, n, special = _rows_cap_matrix(cap, tname)
    oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
    try:
        set_opts(ORDER_OPTS + ((b"hot_k", 256), (b"hub_min_len", 0), (b"rtile_rows", rtile_rows), (b"lazy_tagged", 1)))
        A = _build(gb, rows, cols, vals, m, n, tname)
        here = _first_bytes(gb, A, n, tname)
        # (k_mxv_rtile_bool takes the operand as presence / value pairs: a BOOL operand that is not full)
        operand = (np.flatnonzero(np.arange(n) % 7 != 3), np.ones(n - (n + 3) // 7, bool)) if tname == "BOOL" else None
        _check(gb, A, oa, tname, special, {"ordered": 1, "long_kernel": 1 if tname == "BOOL" else 4, "reorders": 0, "fused_epilogue": 3},
                            operand=operand)
        if tname != "BOOL":
            ui, uv = _operand(n, tname)
            u = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
            got = A.mxv(u, gb.semiring.max_second).new()
            assert device.last_stats()["fused_epilogue"] == 1, device.last_stats()
            same_vec(got, O.mxv(oa, O.OVec(n, ui, uv, tname), "max_second"), where="tagged row groups from the tiles")
        other = 8192 + 16384 - rtile_rows
        tiles_there = -(-m // (cap * other // rtile_rows))
        assert tiles_there == (2 if other > rtile_rows else 7)
        opts = ORDER_OPTS + ((b"hot_k", 256), (b"hub_min_len", 0), (b"lazy_tagged", 1))
        there = _cache_bytes(gb, rows, cols, vals, m, n, tname, opts + ((b"rtile_rows", other),))
        assert (here - there) % RT_BLOCK_ENTRIES == (RT_TILE_RECORD * (4 - tiles_there)) % RT_BLOCK_ENTRIES, (here, there)
    finally:
        reset_opts()


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. cold tiles: packed words
# ------------------------------------------------------------------------------------------------------------------------------------
CT_HOT = 256  # (hot_k of the case: the codes 0 .. 255 are resident, the cold column ranges begin at code 256)


def _ctile_geometry(tname):
    """(W, bounds, n): with ctile_pack on, ensure_ordered closes a column range at W = min(2 MiB / sizeof(T), 2^19 - 4096) codes -- 127
    blocks of 4096 for the 4-byte types, 64 for the 8-byte ones -- unless the range has collected 1/32 of the cold references before.
    _ctile_matrix refers to the first two ranges 12 times each and to the block behind them 20 000 times, so the bounds are
    256, 256 + W, 256 + 2 W (closed by their width), 256 + 2 W + 4096 (closed by its references) and n = that + 1000."""
    vb = np.dtype(_np(tname)).itemsize
    w = min((2 << 20) // vb, (1 << 19) - 4096)
    bounds = [CT_HOT, CT_HOT + w, CT_HOT + 2 * w, CT_HOT + 2 * w + 4096, CT_HOT + 2 * w + 4096 + 1000]
    return w, bounds, bounds[-1]


def _ctile_matrix(kind):
    """16 408 long rows (rows 0 .. 16 407: a row's slot is its index), 200 short rows behind them.  Every long row has 8 entries on the
    resident codes 0 .. 255.  The rows of the slots 0, 8191, 8192, 16383, 16384 and 16407 -- first and last slot of a block of 8192
    (packed words, and FP64 / INT64 in any mode) and of 16384 (FP32, three streams) -- also hold the FIRST and the LAST code of the
    ranges 0 and 1, the first code of the ranges 2 and 3 and the last column.  Offset W - 1 = 2^19 - 4097 (FP32) is the largest the
    builder makes, in slot 8191 of a block the packed word is 8191 << 19 | W - 1: the one closest to the padding word 0xffffffff.  The
    rows 3 .. 7 hold 4000 codes each of range 2 -- the SAME codes: 20 002 entries in the pair (range 2, slot block 0), more than
    CT_MAX_ENTRIES = 16384, so the pair is cut into two pieces.  (One hub row alone cannot fill a pair: a range closes as soon as it
    holds 1/32 of the cold references, a row refers to a code once, and 32 x 16384 cold entries are too many for a quick test.)"""
    tname = "FP64" if kind == "fp64" else "FP32"
    w, bounds, n = _ctile_geometry(tname)
    n_long = 16384 + 24
    m = n_long + 200
    nvals = 900 if kind == "fp32_257" else 150
    s = np.arange(n_long)
    rows_l = [np.repeat(s, 8)]
    cols_l = [(np.repeat(s * 8, 8) + np.tile(np.arange(8), n_long)) % CT_HOT]
    vals_l = [1 + (np.arange(8 * n_long) * 7 + np.repeat(s, 8)) % nvals]
    special = [0, 8191, 8192, 16383, 16384, n_long - 1]
    on_limits = np.array([bounds[0], bounds[1] - 1, bounds[1], bounds[2] - 1, bounds[2], bounds[3], n - 1])
    for j, r in enumerate(special):
        rows_l.append(np.full(on_limits.size, r)); cols_l.append(on_limits); vals_l.append(nvals + 1 + 7 * j + np.arange(on_limits.size))
    hubs = list(range(3, 8))
    for r in hubs:
        cc = bounds[2] + 1 + np.arange(4000)
        rows_l.append(np.full(cc.size, r)); cols_l.append(cc); vals_l.append(1 + (cc + r) % 50)
    o = np.arange(n_long, m)  # short rows
    rows_l.append(o); cols_l.append((o * 4099) % n); vals_l.append(1 + o % 50)
    rows, cols = np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64)
    vals = np.concatenate(vals_l).astype(_np(tname))
    assert kind == "fp64" or (np.unique(vals).size <= 256) == (kind == "fp32_dict")
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order], m, n, tname, special + hubs, n_long


def _ctile_units(rows, cols, n_long, bounds, ct_slots):
    """Units of 4 entries of the cold tiles, as ensure_split cuts them: the cold entries of the long rows by (column range, slot block)
    pair, a pair of more than CT_MAX_ENTRIES entries in equal pieces, every piece padded to whole units."""
    cold = (rows < n_long) & (cols >= bounds[0])
    rng = np.searchsorted(np.asarray(bounds), cols[cold], side="right") - 1
    pair, cnt = np.unique(rng * 64 + rows[cold] // ct_slots, return_counts=True)
    units = 0
    for c in cnt.tolist():
        pieces = -(-c // CT_MAX_ENTRIES)
        per = -(-c // pieces)
        units += sum(-(-min(per, c - q * per) // CT_EPL) for q in range(pieces))
    assert cnt.max() > CT_MAX_ENTRIES
    return units


def _ctile_case(gb, kind):
    from graphblas_amd import device

    rows, cols, vals, m, n, tname, keep, n_long = _ctile_matrix(kind)
    w, bounds, _ = _ctile_geometry(tname)
    oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
    opts = ORDER_OPTS + ((b"hot_k", CT_HOT), (b"hub_min_len", 0), (b"long_classes", 16))
    bytes_of = {}
    try:
        for mode in (1, 2, 0):
            set_opts(opts + ((b"ctile_pack", mode),))
            A = _build(gb, rows, cols, vals, m, n, tname)
            bytes_of[mode] = _first_bytes(gb, A, n, tname)
            _check(gb, A, oa, tname, keep, {"ordered": 1, "long_kernel": 4, "reorders": 0})
            assert (device.last_stats()["value_dict"] > 0) == (kind == "fp32_dict")
        assert bytes_of[2] <= bytes_of[1] < bytes_of[0], bytes_of
        # the geometry: the stream that differs between two modes is counted per padded entry of the cold tiles
        units = _ctile_units(rows, cols, n_long, bounds, 8192)
        if kind == "fp32_dict":  # (mode 2: one-byte value codes in place of 4-byte values, everything else as in mode 1)
            assert bytes_of[1] - bytes_of[2] == units * CT_EPL * 3, (bytes_of, units)
        else:
            assert bytes_of[1] == bytes_of[2], bytes_of  # (no dictionary: mode 2 is mode 1)
        if kind == "fp64":  # (8-byte types: the same ranges and blocks of 8192 slots in mode 0 -- only the 16-bit slot stream goes)
            assert bytes_of[0] - bytes_of[1] == units * CT_EPL * 2, (bytes_of, units)
    finally:
        reset_opts()


def test_ctile_packed_words_at_range_and_slot_limits(gb):
    """ensure_ordered (the column ranges), ensure_split (ct_mode, ct_slots, the pieces of a pair), k_ctile_place and k_mxv_ctile
    (`w == 0xffffffffu` is padding): the cold tiles with slot << 19 | column offset in one word (ctile_pack 1), with one-byte value codes
    too (2) and as three streams (0), each against the oracle.  See _ctile_matrix for the entries on the limits.  cache_bytes orders the
    modes 2 <= 1 < 0, and -- the witness that the ranges, slot blocks and pieces are the ones the matrix was built for -- the bytes mode 2
    saves over mode 1 are exactly 3 per padded entry of the tiles as _ctile_units cuts them.  FP32 with a value dictionary.  (The three
    builds of 16 408 long rows and the 24 products take the emulator 53 s, measured once.)"""
    _ctile_case(gb, "fp32_dict")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["fp32_257", "fp64"])
def test_ctile_packed_words_other_records(kind):
    """The same for FP32 without a dictionary (mode 2 falls back to mode 1: equal bytes) and FP64 (ranges of 2^18 codes, blocks of 8192 slots
    in every mode: mode 0 costs exactly the two bytes of its slot stream per padded entry more)."""
    _ctile_case(bind("gpu"), kind)


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. hot / cold boundary of a class head
# ------------------------------------------------------------------------------------------------------------------------------------
def _head_matrix(tname, move_low=None, move_hub=None):
    """700 rows, HUB + 50 000 columns.  20 long rows below the hub level (14 + j entries) hold LIM - 1, LIM, LIM + 1, the first code of
    LIM - 1's line, codes of the line before and codes of other classes; 4 hub rows (120-odd entries) hold HUB - 1, HUB, HUB + 1, the first
    code of HUB - 1's line, LIM - 1 and LIM (both resident there).  The entries ON the limits carry values of their own.  move_low /
    move_hub = (from, to) renames one column in the rows of that level (for the witnesses: see the test)."""
    vb = np.dtype(_np(tname)).itemsize
    lim = LDS_WORDS * 4 // vb * 16
    hub = 4 * lim
    n, m = hub + 50000, 700
    rows_l, cols_l, vals_l = [], [], []
    special = []

    def put(r, cc, vv, move):
        # (the values go with the entries ON the limits before a column is renamed: a variant keeps its values)
        for k, c in enumerate((lim - 1, lim, hub - 1, hub)):
            vv = np.where(cc == c, 200 + k, vv)
        if move:
            assert move[1] not in cc
            cc = np.where(cc == move[0], move[1], cc)
        rows_l.append(np.full(cc.size, r)); cols_l.append(cc); vals_l.append(vv)
        special.append(r)

    for j, r in enumerate(range(3, 43, 2)):  # 20 long rows of 14 + j entries (below the hub level)
        cc = np.unique(np.concatenate([[lim - 1, lim, lim - 32, lim - 33, lim + 1, 0, 31, 32], 64 + j + 97 * np.arange(6 + j)]))
        put(r, cc, 1 + (np.arange(cc.size) * 3 + j) % 150, move_low)
    for j, r in enumerate(range(50, 62, 3)):  # 4 hub rows of 120-odd entries
        cc = np.unique(np.concatenate([[hub - 1, hub, hub - 32, hub + 1, lim - 1, lim, 0], 100 + j + 1009 * np.arange(115)]))
        put(r, cc, 1 + (np.arange(cc.size) * 7 + j) % 150, move_hub)
    o = np.arange(100, m, 2)  # short rows
    rows_l.append(o); cols_l.append((o * 3571) % n); vals_l.append(1 + o % 150)
    rows, cols = np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64)
    vals = np.concatenate(vals_l).astype(_np(tname))
    order = np.lexsort((cols, rows))
    return rows[order], cols[order], vals[order], m, n, special, lim, hub


@pytest.mark.parametrize("dev, tname", [pytest.param("emu", "FP64")] + [pytest.param("gpu", t, marks=pytest.mark.gpu) for t in ("FP32", "FP64", "INT32", "INT64")])
def test_last_resident_code_of_a_class_head(dev, tname):
    """ensure_split (lds_lim4, hub_lim), k_long_keys, k_strip_place (long_tcode_n) and hot_pad_code: with 16 classes the codes below
    LIM = LONG_LDS_WORDS * 4 / sizeof(T) * 16 are resident (4-byte types 638 976, 8-byte types 319 488), for the hub rows -- 64 classes,
    rows from hub_min_len = 100 entries -- the codes below HUB = 4 LIM.  Code LIM - 1 (HUB - 1) is the last code of the last line of its
    class: LDS slot LDS_SLOTS - 1, right in front of the padding slot LDS_SLOTS (hot_pad_code) that every padding entry of a lane record
    points at; code LIM (HUB) is the first cold one and goes to the cold tiles.  See _head_matrix.  Both levels run in the one launch of
    k_mxv_hstrip (hub_min_len > 0, full operand, min_plus / plus_times).

    Witnesses that the boundary lies between LIM - 1 and LIM (HUB - 1 and HUB) and nowhere else -- cls_lds_lim is min(hot_k, LIM): the
    statistics show hot_k = LIM + 4096 (set so: the LDS limit decides, not the table), and GrX_Matrix_cache_bytes of two variants per level.  Renaming column LIM to LIM - 2 in the rows of the
    level takes 20 (4) entries out of one cold tile -- 5 units (1 unit) less -- and adds no hot lane: LIM - 2 joins the lane that holds
    LIM - 32 and LIM - 1.  Fewer bytes: LIM was cold, LIM - 2 is resident.  Renaming LIM - 1 to LIM + 2 takes nothing from that lane's count
    and adds 20 (4) entries to the cold tile of LIM and LIM + 1 (the same block of 4096 codes, hence the same column range).  More bytes:
    LIM - 1 was resident.  With a boundary elsewhere at least one of the four relations is an equality.

    The emulator tier runs FP64 alone (the five layout builds over 1.3 M columns take it 42 s; FP32 / INT32, 2.6 M columns: 76 / 79 s,
    INT64 41 s, measured once, all passed there); the GPU tier runs the four types."""
    gb = bind(dev)
    rows, cols, vals, m, n, special, lim, hub = _head_matrix(tname)
    oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
    # (a hot table LARGER than the heads: the heads end at the LDS limit, not where the table ends)
    opts = ORDER_OPTS + ((b"long_classes", 16), (b"hub_min_len", 100), (b"hot_k", lim + 4096))
    try:
        set_opts(opts)
        A = _build(gb, rows, cols, vals, m, n, tname)
        base = _first_bytes(gb, A, n, tname)
        from graphblas_amd import device

        assert device.last_stats()["hot_k"] == lim + 4096, device.last_stats()
        _check(gb, A, oa, tname, special, {"ordered": 1, "long_kernel": 4, "reorders": 0})
        for level, b in (("low", lim), ("hub", hub)):
            for move, more in (((b, b - 2), False), ((b - 1, b + 2), True)):
                r2, c2, v2 = _head_matrix(tname, **{"move_" + level: move})[:3]
                assert r2.size == rows.size
                got = _cache_bytes(gb, r2, c2, v2, m, n, tname, opts)
                assert (got > base) if more else (got < base), (level, move, got, base)
    finally:
        reset_opts()


# ------------------------------------------------------------------------------------------------------------------------------------
# 6. the lifetime of the cached layouts: built, extended, rebuilt, dropped, built again
# ------------------------------------------------------------------------------------------------------------------------------------
def _lifecycle_matrix():
    """300 rows, 2048 columns, FP32 values from 1 .. 200 (a dictionary is built).  Rows 0 .. 23 are long: 96 entries each, 48 on the
    resident codes below hot_k = 256 (hot strips) and 48 behind them (cold tiles) -- 2304 entries, more than 30 % of all, so the split
    is built.  The other rows hold 0 .. 3 entries anywhere (the short part: tagged row groups and sorted row tiles)."""
    m, n = 300, 2048
    rows_l, cols_l = [], []
    for r in range(24):
        cc = np.concatenate([(np.arange(48) * 5 + r) % 256, 256 + (np.arange(48) * 37 + r * 3) % (n - 256)])
        rows_l.append(np.full(cc.size, r)); cols_l.append(cc)
    i = np.arange(24, m)
    cnt = np.array([0, 1, 2, 3, 1])[i % 5]
    rr = np.repeat(i, cnt)
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    kth = np.arange(rr.size) - np.repeat(first, cnt)
    rows_l.append(rr); cols_l.append((rr * 29 + kth * 683) % n)
    rows, cols = np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64)
    order = np.lexsort((cols, rows))
    rows, cols = rows[order], cols[order]
    assert (np.diff(rows * n + cols) > 0).all()
    vals = (1 + (rows * 7 + cols * 3) % 200).astype(np.float32)
    return rows, cols, vals, m, n


def test_layouts_are_built_extended_rebuilt_dropped_and_built_again(gb):
    """Every cached layout of one matrix through its whole life, with GrX_Matrix_cache_bytes as the witness that what was dropped was
    released and what was rebuilt is what was there before -- a layout that one of the steps forgets to drop, or keeps half of, shows as
    a byte count that does not return.  The matrix (see _lifecycle_matrix) carries the ranked hint and gets the ordered twin with a value
    dictionary, hot strips, cold tiles, the index of the tagged row groups and sorted row tiles.  Every product is compared with the
    oracle element for element (small integer values: exact).

    1. three min_plus products of a full operand: the layouts are built at the first; the bytes are recorded;
    2. a plus_times product of a sparse operand, which the row tiles do not take: the ENTRIES of the tagged row groups are built now, from
       the tiles (lazy_tagged) -- the bytes grow by exactly those: 4 (column) + 1 (row tag) + 1 (value code) bytes per entry, the entries of
       every group of 64 rows padded to a multiple of 4;
    3. long_classes 16 -> 32 and back: each change rebuilds the twin and its split; after the way back the bytes are those of step 2;
    4. ONE value is changed in place, which drops every cached layout: 0 bytes; three products against the oracle; the bytes of step 1.
       (GrB_Matrix_setElement is not implemented by this library; the in-place element-wise update A = A (+) D with `second` and a D
       of one entry sets that one value and invalidates the caches like any other write to A.)"""
    from graphblas_amd import device

    rows, cols, vals, m, n = _lifecycle_matrix()
    tname = "FP32"
    oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
    fi, fv = _operand(n, tname)
    si = np.unique(np.concatenate([np.arange(0, n, 3), np.arange(1, 256, 7)]))
    sv = (1 + si % 9).astype(np.float32)
    full, ofull = gb.Vector.from_coo(fi, fv, dtype=tname, size=n), O.OVec(n, fi, fv, tname)
    sparse, osparse = gb.Vector.from_coo(si, sv, dtype=tname, size=n), O.OVec(n, si, sv, tname)
    # (the short part: the rows with fewer than split_min_len = 8 entries)
    deg = np.bincount(rows, minlength=m)
    short = np.where(deg < 8, deg, 0)
    per_group = np.add.reduceat(short, np.arange(0, m, 64))
    tagged_entry_bytes = int(((per_group + 3) // 4).sum()) * 4 * 6

    def full_products(oa, where):
        exp = O.mxv(oa, ofull, "min_plus")
        for call in range(3):
            same_vec(A.mxv(full, gb.semiring.min_plus).new(), exp, where=f"{where}, full operand, call {call}")
            st = device.last_stats()
            assert st["ordered"] == 1 and st["long_kernel"] == 4 and st["fused_epilogue"] == 3 and st["value_dict"] > 0, (where, call, st)

    def sparse_product(oa, where):
        same_vec(A.mxv(sparse, gb.semiring.plus_times).new(), O.mxv(oa, osparse, "plus_times"), where=f"{where}, sparse operand")
        st = device.last_stats()
        assert st["ordered"] == 1 and st["fused_epilogue"] == 1, (where, st)

    opts = ORDER_OPTS + ((b"hot_k", 256), (b"hub_min_len", 0), (b"long_classes", 16), (b"lazy_tagged", 1))
    try:
        set_opts(opts)
        A = _build(gb, rows, cols, vals, m, n, tname)
        assert device.matrix_cache_bytes(A) == 0
        # 1
        full_products(oa, "step 1")
        built = device.matrix_cache_bytes(A)
        assert built > 0
        # 2
        sparse_product(oa, "step 2")
        extended = device.matrix_cache_bytes(A)
        assert extended - built == tagged_entry_bytes, (built, extended, tagged_entry_bytes)
        # 3
        set_opts(((b"long_classes", 32),))
        full_products(oa, "step 3, 32 classes")
        sparse_product(oa, "step 3, 32 classes")
        set_opts(((b"long_classes", 16),))
        full_products(oa, "step 3, 16 classes again")
        sparse_product(oa, "step 3, 16 classes again")
        assert device.matrix_cache_bytes(A) == extended, (device.matrix_cache_bytes(A), extended)
        # 4
        k = int(np.flatnonzero(rows == 5)[50])  # (a cold entry of a long row)
        new_val = np.float32(7 if vals[k] != 7 else 8)
        D = gb.Matrix.from_coo(rows[k : k + 1], cols[k : k + 1], np.array([new_val], np.float32), dtype=tname, nrows=m, ncols=n)
        A << A.ewise_add(D, gb.binary.second)
        assert device.matrix_cache_bytes(A) == 0
        vals2 = vals.copy()
        vals2[k] = new_val
        oa2 = O.OMat.from_coo(rows, cols, vals2, m, n, tname)
        full_products(oa2, "step 4")
        assert device.matrix_cache_bytes(A) == built, (device.matrix_cache_bytes(A), built)
    finally:
        reset_opts()
