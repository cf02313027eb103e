"""Cold tiles with the value code in the column word (option ctile_code = 1, the default; cold-tile mode 3).

A dictionary-coded 4-byte matrix whose operand image has at most 2^24 codes keeps a cold entry as the word code << 24 | column code
plus a 16-bit slot -- 6 instead of 10 bytes -- and k_mxv_ctile<.., CODEW> takes the value from the dictionary in LDS.  Every other
matrix keeps the three streams of mode 0 without the caller noticing.

Every case runs the same calls on the same matrix built with the code words on (ctile_pack = 0, then ctile_code = 1: setting ctile_pack
names a layout and switches the code words off) and under ctile_pack = 0 alone, the three streams, and
* compares every result with the oracle (tests/values.py: bit patterns; the values are small integers unless the case says otherwise),
* compares the results of the two builds with each other bit for bit,
* asserts through GrX_Stats.cold_tile_mode that mode 3 -- or the fallback, mode 0 -- is what k_mxv_ctile ran on, and through
  GrX_Matrix_cache_bytes that mode 3 dropped exactly the value stream: 4 bytes per padded entry, a multiple of 16 per tile.

The matrices with the ranked hint (GrX_Matrix_hint_ranked) are laid out in the caller's own index order: with hot_k = 256 the column codes
0 .. 255 are LDS-resident and every other column is cold; a row's slot is its rank among the rows with at least split_min_len = 8 entries."""
import numpy as np
import pytest

from oracle import grb_oracle as O
from tests.backend import DEVICES, bind
from tests.test_layout_limits import CT_EPL, CT_MAX_ENTRIES, _operand
from tests.test_vertex_order import ORDER_OPTS, reset_opts, set_opts, skewed_square
from tests.values import same_vec

CT_SLOTS = 16384  # (long rows per cold tile, 4-byte accumulators: grb_mxv_ctile.inc)
HOT = 256
OPTS = ORDER_OPTS + ((b"hot_k", HOT), (b"hub_min_len", 0), (b"long_classes", 16))
# (semiring, mask, accumulator, replace): the headline's shape, a plain product, a product that replaces
CALLS = (("min_plus", "comp_struct", "min", False), ("plus_times", None, None, False), ("max_plus", "value", None, True))


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[v.dtype.itemsize]).tolist()


def _run_calls(gb, A, oa, tname, calls, want_mode, operand=None, reps=2, dict_expected=None):
    """Every call of `calls`, `reps` times (the second on the cached layouts), against the oracle; returns the raw results."""
    from graphblas_amd import device

    m, n = oa.nrows, oa.ncols
    rng = np.random.default_rng(777)
    ui, uv = operand if operand is not None else _operand(n, tname)
    u, ou = gb.Vector.from_coo(ui, uv, dtype=tname, size=n), O.OVec(n, ui, uv, tname)
    mi = np.flatnonzero(rng.random(m) < 0.5)
    mk, om = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=m), O.OVec(m, mi, np.ones(mi.size, bool), "BOOL")
    wi = np.flatnonzero(rng.random(m) < 0.6)
    wv = (1 + wi % 9).astype(O.NP_OF[tname])
    out = []
    for sr, mask, accum, repl in calls:
        kw = {} if mask is None else {"mask": om, "mask_comp": mask == "comp_struct", "mask_struct": mask == "comp_struct"}
        exp = O.mxv(oa, ou, sr, w=O.OVec(m, wi, wv, tname), accum=accum, replace=repl, **kw)
        for rep in range(reps):
            w = gb.Vector.from_coo(wi, wv, dtype=tname, size=m)
            sel = () if mask is None else ((~mk.S,) if mask == "comp_struct" else (mk.V,))
            w(*sel, accum=None if accum is None else getattr(gb.binary, accum), replace=repl) << A.mxv(u, getattr(gb.semiring, sr))
            st = device.last_stats()
            assert st["long_kernel"] == 4 and st["cold_tile_mode"] == want_mode, (sr, rep, want_mode, st)
            if dict_expected is not None:
                assert (st["value_dict"] > 0) == dict_expected, st
            monoid = sr.split("_")[0]
            same_vec(w, exp, monoid if monoid in ("min", "max") else None, where=f"{sr} mode {want_mode} call {rep}")
            out.append(w.to_coo())
    return out


def _ab(gb, rows, cols, vals, m, n, tname, want, calls=CALLS, opts=OPTS, ranked=True, setup=None, operand=None, dict_expected=None, units=None):
    """The matrix built with the code words on (`want` = the mode that must run: 3, or 0 for a fallback) and under ctile_pack = 0 alone."""
    from graphblas_amd import device

    oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
    got, nbytes = {}, {}
    try:
        for pack in (3, 0):
            set_opts(opts + ((b"ctile_pack", 0),) + (((b"ctile_code", 1),) if pack == 3 else ()))
            A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
            if ranked:
                device.matrix_hint_ranked(A)
            if setup is not None:
                setup(A)
            got[pack] = _run_calls(gb, A, oa, tname, calls, want if pack == 3 else 0, operand=operand, dict_expected=dict_expected)
            nbytes[pack] = device.matrix_cache_bytes(A)
    finally:
        reset_opts()
    for (i3, v3), (i0, v0) in zip(got[3], got[0]):
        assert i3.tolist() == i0.tolist() and _bits(v3) == _bits(v0), "code words and three streams differ"
    saved = nbytes[0] - nbytes[3]
    if want == 3:  # (the value stream is gone: 4 bytes per padded entry)
        assert saved > 0 and saved % (4 * CT_EPL) == 0, nbytes
        if units is not None:
            assert saved == 4 * CT_EPL * units, (nbytes, units)
    else:
        assert saved == 0, nbytes


def _units(counts):
    """Padded units of 4 entries of (column range, slot block) pairs with these entry counts, cut the way ensure_split cuts them."""
    units = 0
    for c in counts:
        pieces = -(-c // CT_MAX_ENTRIES)
        per = -(-c // pieces)
        units += sum(-(-min(per, c - q * per) // CT_EPL) for q in range(pieces))
    return units


def _sorted(rows, cols, vals):
    order = np.lexsort((cols, rows))
    rows, cols, vals = rows[order], cols[order], vals[order]
    assert (np.diff(rows * (int(cols.max()) + 1) + cols) > 0).all(), "duplicate entries"
    return rows, cols, vals


def _small(n_long=24, n=2048, m=300, extra_cold=1, nvals=256, hot_per_row=48, cold_per_row=48):
    """`n_long` long rows of hot_per_row resident and cold_per_row cold codes (row 0: `extra_cold` more), short rows behind them; the value
    of entry k is 1 + k % nvals.  With n = 2048 the cold codes are ONE column range (a range is whole blocks of 4096 codes), with at
    most 16384 long rows one slot block: all cold entries are one tile of n_long * cold_per_row + extra_cold entries."""
    rows_l, cols_l = [], []
    for r in range(n_long):
        k = cold_per_row + (extra_cold if r == 0 else 0)
        cc = np.concatenate([(np.arange(hot_per_row) * 5 + r) % HOT, HOT + (np.arange(k) * 37 + r * 3) % (n - HOT)])
        rows_l.append(np.full(cc.size, r)); cols_l.append(cc)
    i = np.arange(n_long, m)
    cnt = np.array([0, 1, 2, 3, 1])[i % 5]
    rr = np.repeat(i, cnt)
    kth = np.arange(rr.size) - np.repeat(np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt)
    rows_l.append(rr); cols_l.append((rr * 29 + kth * 683) % n)
    rows, cols = np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64)
    rows, cols, _ = _sorted(rows, cols, np.zeros(rows.size))
    vals = 1 + np.arange(rows.size) % nvals
    return rows, cols, vals, m, n


# ------------------------------------------------------------------------------------------------------------------------------------
def test_option_ctile_code_and_its_coupling_to_ctile_pack(gb):
    """ctile_code is 1 by default and takes 0 and 1; setting ctile_pack -- to 0 too -- names the layout of the cold tiles and stores 0 in
    ctile_code; ctile_code set behind it holds; GrX_options_reset returns both to what GrB_init left."""
    import ctypes

    from graphblas_amd import _lib

    def get(name):
        v = ctypes.c_int64(-1)
        assert _lib.lib.GrX_option_get(name, ctypes.byref(v)) == 0
        return v.value

    reset_opts()
    first = (get(b"ctile_pack"), get(b"ctile_code"))
    try:
        for bad in (-1, 2):
            assert _lib.lib.GrX_option_set(b"ctile_code", bad) != 0 and get(b"ctile_code") == first[1]
        for pack in (0, 1, 2):
            set_opts(((b"ctile_code", 1), (b"ctile_pack", pack)))
            assert (get(b"ctile_pack"), get(b"ctile_code")) == (pack, 0)
            assert _lib.lib.GrX_option_set(b"ctile_pack", 3) != 0 and (get(b"ctile_pack"), get(b"ctile_code")) == (pack, 0)  # (a rejected value changes nothing)
        set_opts(((b"ctile_pack", 0), (b"ctile_code", 1)))
        assert (get(b"ctile_pack"), get(b"ctile_code")) == (0, 1)
    finally:
        reset_opts()
    assert (get(b"ctile_pack"), get(b"ctile_code")) == first
    import os

    if "GRB_CTILE_PACK" not in os.environ and "GRB_CTILE_CODE" not in os.environ:
        assert first == (0, 1)


def test_skewed_square_three_semirings(gb):
    """A skewed square FP32 graph of 3000 vertices in the library's own popularity order (no hint): its long rows have cold entries
    behind the 256 resident codes.  The headline's call (min_plus, complemented structural mask, accumulator min), plus_times without
    a mask, max_plus with replace; 8 distinct values."""
    rng = np.random.default_rng(2407)
    n = 3000
    rows, cols, vals = skewed_square(rng, n, "FP32")
    _ab(gb, rows, cols, vals, n, n, "FP32", 3, ranked=False, dict_expected=True)


@pytest.mark.parametrize("nvals", [256, 257])
def test_dictionary_of_256_values_beside_padding(gb, nvals):
    """Exactly 256 distinct values: code 255 is in use, in a tile of 24 x 48 + 1 = 1153 entries -- no multiple of 4, so three padding
    entries (word 0xffffffff = column 2^24 - 1 with code 255, slot CT_SLOTS) follow the last entry; they must stay no-ops.  The saving is
    exactly the one tile's 289 units.  257 distinct values: no dictionary, the three streams of mode 0."""
    rows, cols, vals, m, n = _small(nvals=nvals)
    vals = vals.astype(np.float32)
    cold = (rows < 24) & (cols >= HOT)
    assert cold.sum() == 1153 and np.unique(vals).size == nvals and np.unique(vals[cold]).size == nvals
    _ab(gb, rows, cols, vals, m, n, "FP32", 3 if nvals == 256 else 0, dict_expected=nvals == 256, units=_units([1153]))


@pytest.mark.parametrize("kind", ["fp32_zeros", "fp32_nonfinite", "int32_bits"])
def test_special_bit_patterns(gb, kind):
    """The dictionary returns the stored bits.  fp32_zeros: -0.0 and +0.0 are two codes (a dictionary holds bit patterns) next to small
    integers of both signs -- mode 3.  fp32_nonfinite: +inf, -inf and a NaN with a payload among the values -- the library builds no
    dictionary for an FP32 matrix with a non-finite value (ensure_vdict), so the tiles keep full values: the fallback, and the same
    results.  int32_bits: the bit patterns of -0.0, +inf, -inf and of the NaN 0x7fc12345 as INT32 values, which a dictionary does code:
    mode 3, and max_first / min_first hand the stored words through.  Operand of ones, so a product is the matrix value itself."""
    rows, cols, vals, m, n = _small(nvals=13)
    if kind == "int32_bits":
        tname = "INT32"
        pal = np.array([0x80000000, 0x7f800000, 0xff800000, 0x7fc12345, 0, 1, 7, 0x7fffffff], np.uint32).view(np.int32)
        calls = (("max_first", "comp_struct", "max", False), ("min_first", None, None, False), ("max_first", "value", None, True))
    else:
        tname = "FP32"
        pal = np.array([-0.0, 0.0, 1.0, -2.0, 3.0, -4.0, 5.0, 8.0], np.float32)
        if kind == "fp32_nonfinite":
            pal = np.concatenate([pal, np.array([0x7f800000, 0xff800000, 0x7fc12345], np.uint32).view(np.float32)])
        calls = (("min_plus", "comp_struct", "min", False), ("max_first", None, None, False), ("plus_times", "value", None, True))
    vals = pal[(np.arange(rows.size) * 7) % pal.size]
    cold = (rows < 24) & (cols >= HOT)
    assert np.unique(_bits(vals[cold])).size == pal.size
    operand = (np.arange(n), np.ones(n, O.NP_OF[tname]))
    finite = kind != "fp32_nonfinite"
    _ab(gb, rows, cols, vals, m, n, tname, 3 if finite else 0, calls=calls, operand=operand, dict_expected=finite)


def _wide_matrix(n):
    """256 long rows (row k: the resident codes 8 k' .. and three cold ones) whose entry at column TOP = 2^24 - 1 carries value k + 1: all
    256 values, so whichever of them the dictionary numbers 255 is stored as the word 0xffffffff, the padding pattern, when n = 2^24.
    256 x 3 + 1 cold entries (row 0 holds one more): padding follows.  With n = 2^24 + 1 the rows 3 k also hold column 2^24."""
    top = (1 << 24) - 1
    k = np.arange(256)
    rows_l = [np.repeat(k, 8), k, k, k, np.array([0])]
    cols_l = [(np.repeat(k * 8, 8) + np.tile(np.arange(8), 256)) % HOT, np.full(256, top), np.full(256, top - 1), 5000 + k * 4099, np.array([777777])]
    vals_l = [1 + (np.arange(2048) * 5) % 256, k + 1, 1 + (k + 101) % 256, 1 + (k + 17) % 256, np.array([9])]
    if n > top + 1:
        rows_l.append(k[::3]); cols_l.append(np.full(k[::3].size, top + 1)); vals_l.append(1 + (k[::3] + 59) % 256)
    o = np.arange(300, 1500, 3)  # short rows
    rows_l.append(o); cols_l.append(6000 + o * 7); vals_l.append(1 + o % 256)
    rows, cols, vals = _sorted(np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64), np.concatenate(vals_l).astype(np.float32))
    return rows, cols, vals, 1500, n


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [0, 1])
def test_code_word_at_2_pow_24_columns(extra):
    """ensure_split (`codes_total <= 1 << 24`), k_ctile_place, k_mxv_ctile<.., CODEW>: with exactly 2^24 columns the entry (column
    2^24 - 1, code 255) IS the word 0xffffffff and is told from the padding beside it by its slot alone; with 2^24 + 1 columns the tiles
    keep the three streams and column 2^24 keeps its top bit.  GPU tier only, as test_rtile_packed_word_at_2_pow_24_columns: the
    16.8 M-entry operand and the per-column passes of the layout build take the emulator minutes."""
    gb = bind("gpu")
    rows, cols, vals, m, n = _wide_matrix((1 << 24) + extra)
    assert np.unique(vals).size == 256 and (cols == (1 << 24) - 1).sum() == 256 and cols.max() == n - 1
    _ab(gb, rows, cols, vals, m, n, "FP32", 0 if extra else 3, dict_expected=True, calls=CALLS[:2])


def test_pair_cut_into_several_tiles(gb):
    """Five rows that hold the SAME 4000 cold codes: 20 000 entries in the one (column range, slot block) pair of the matrix, more than
    CT_MAX_ENTRIES = 16384 -- cut into two tiles of 10 000 (the saving is exactly their 5000 units).  n = 256 + 4096: one column range."""
    n, m = HOT + 4096, 400
    rows_l, cols_l = [], []
    for r in range(5):
        cc = np.concatenate([(np.arange(8) + 8 * r) % HOT, HOT + 1 + np.arange(4000)])
        rows_l.append(np.full(cc.size, r)); cols_l.append(cc)
    o = np.arange(5, m)  # short rows
    rows_l.append(o); cols_l.append((o * 131) % n)
    rows, cols = np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64)
    rows, cols, _ = _sorted(rows, cols, np.zeros(rows.size))
    vals = (1 + (rows * 3 + cols) % 50).astype(np.float32)
    assert 20000 > CT_MAX_ENTRIES
    _ab(gb, rows, cols, vals, m, n, "FP32", 3, dict_expected=True, units=_units([20000]))


def test_slot_block_boundary(gb):
    """CT_SLOTS + 1 long rows: the last one is slot 0 of a second slot block.  Every long row has 8 resident entries; the rows of the
    slots 0, 1, CT_SLOTS - 1 and CT_SLOTS (and every 97th) also hold cold entries with values of their own -- slot CT_SLOTS - 1 is the
    largest 16-bit slot a real entry carries, CT_SLOTS is the padding's.  Two tiles: 3 x 174-odd entries and the last row's 3."""
    n_long = CT_SLOTS + 1
    n, m = HOT + 4096, n_long + 40
    s = np.arange(n_long)
    rows_l = [np.repeat(s, 8)]
    cols_l = [(np.repeat(s * 8, 8) + np.tile(np.arange(8), n_long)) % HOT]
    vals_l = [1 + (np.arange(8 * n_long) * 7 + np.repeat(s, 8)) % 100]
    special = np.unique(np.concatenate([[0, 1, CT_SLOTS - 1, CT_SLOTS], s[::97]]))
    for j, c in enumerate((HOT, HOT + 1000, n - 1)):
        rows_l.append(special); cols_l.append(np.full(special.size, c)); vals_l.append(101 + (special + j) % 100)
    o = np.arange(n_long, m)
    rows_l.append(o); cols_l.append((o * 131) % n); vals_l.append(1 + o % 50)
    rows, cols, vals = _sorted(np.concatenate(rows_l).astype(np.int64), np.concatenate(cols_l).astype(np.int64), np.concatenate(vals_l).astype(np.float32))
    in_block0 = int((special < CT_SLOTS).sum()) * 3
    _ab(gb, rows, cols, vals, m, n, "FP32", 3, dict_expected=True, calls=CALLS[:2], units=_units([in_block0, 3]))


@pytest.mark.parametrize("kind", ["fp64", "iso"])
def test_fp64_and_iso_fall_back(gb, kind):
    """An 8-byte type has no dictionary and an iso matrix has no value stream to drop: both keep mode 0."""
    rows, cols, vals, m, n = _small(nvals=50)
    tname = "FP64" if kind == "fp64" else "FP32"
    vals = np.full(rows.size, 3, O.NP_OF[tname]) if kind == "iso" else vals.astype(np.float64)
    _ab(gb, rows, cols, vals, m, n, tname, 0, dict_expected=False)


def test_row_block_after_shard_setup(gb):
    """A NON-square row block of a skewed graph whose column order comes from GrX_Matrix_shard_setup (the global reference counts): its
    long rows have cold tiles too, and they take the code words."""
    from graphblas_amd import device

    rng = np.random.default_rng(2408)
    n = 4000
    rows, cols, vals = skewed_square(rng, n, "FP32")
    counts = np.bincount(cols, minlength=n).astype(np.uint32)
    hi = n // 2 // 64 * 64
    keep = rows < hi
    _ab(gb, rows[keep], cols[keep], vals[keep], hi, n, "FP32", 3, ranked=False, setup=lambda A: device.matrix_shard_setup(A, counts), dict_expected=True,
        calls=CALLS[:2])
