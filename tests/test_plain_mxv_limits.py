"""The plain path of mxv / vxm at the limits of its tiles, seams and work items.

Every matrix below split_min_nnz (4 Mi entries) is multiplied by k_mxv_pull + k_mxv_seams (grb_mxv_pull.inc, grb_mxv_write.inc) when it
is pulled and by k_push_frontier + k_push_small / k_push_pass, or the dense k_push, when it is pushed (grb_mxv_push.inc).  The random
suites put hub rows across tile seams but never an entry, a row start or a row end ON a boundary; the matrices here are built from
lists of row lengths so that they are.  Every comparison is element for element against the oracle; the values are small integers, so
plus_times and min_plus are exact in every type and nothing has a tolerance.  The operand differs between neighbouring columns, and an
entry ON a boundary carries a value no other entry of its row has (BOOL: the only true entry of its row).

Geometry of the merge path (python-graphblas_amd/csrc):
* merge positions (k_tile_table, grb_mxv_common.inc): the entries of row i sit at i + rowptr[i] .. i + rowptr[i + 1] - 1, its row end
  at i + rowptr[i + 1] -- m + nnz positions in all;
* tile t is the positions [t TILE, (t + 1) TILE), n_tiles = ceil((m + nnz) / TILE) (ensure_tile_table, grb_mxv.hip); tile_row[t] is
  the number of row ends in front of position t TILE: the row whose end is the first one in tile t;
* TILE = PULL_BLOCK * IPT = 256 IPT (k_mxv_pull); IPT is 8 for types of at most 4 bytes (TILE 2048) and 4 for the 8-byte types
  (TILE 1024) (PullIPT, grb_mxv.hip); option pull_ipt 4 / 16 gives TILE 1024 / 4096 to the specialised semirings of the types of at
  most 4 bytes -- FP32 min_plus, plus_times, any_pair; BOOL lor_land, any_pair (launch_pull, pull_dispatch);
* a tile OWNS the rows whose end lies in it, except its first row when that row began in an earlier tile (own_lo): that row is a SEAM,
  written by k_mxv_seams from the carries of the tiles [t_s, t) -- t_s = (row + rowptr[row]) / TILE, the tile of its first entry --
  and the tile's own first partial (first_has bit 0; bit 1 = there is a seam).
_tile_rows computes tile_row[] from rowptr by this definition; every case asserts with it that its boundary lies where the matrix was
built to put it, and with GrX_last_stats that the plain path ran (method 1, long_kernel -1) over that many tiles.

Every pull case runs plain, under a complemented structural mask with an accumulator and old content in w, under that mask with
replace (both with its special rows admitted and with them masked out, an old entry of w under each), and with w aliased to u (the
`fresh` buffers; the matrices are square, or get a square twin with empty rows behind the last one).  Afterwards each result is grown
by 200: a presence bit left above the size would show as a phantom entry.

The push cases run u' A (vxm: A's own rows are the frontier's) under push_mode 2."""
import numpy as np
import pytest

from oracle import grb_oracle as O
from tests.backend import DEVICES, bind
from tests.test_layout_limits import _operand
from tests.test_vertex_order import ORDER_OPTS, reset_opts, set_opts
from tests.values import same_values, same_vec

PUSH_Q = 1024            # (entries of a work item of the thin push path, grb_mxv_push.inc)
PUSH_SMALL_CHUNKS = 64   # (k_push_small takes at most this many work items ...)
PUSH_SMALL_FCOUNT = 4096  # (... of at most this many frontier vertices: push_thin, grb_mxv.hip)
PUSH_F_CAP = 1 << 16     # (f_cap = max(n / 64 + 64, 2^16): push_thin)
PUSH_CHUNK = 8           # (consecutive work items of a thread of the dense k_push)
FILL = (0, 1, 0, 2, 1, 0, 3, 0)  # (row lengths of the filler rows)


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


def _np(tname):
    return O.NP_OF[tname]


def _tile(tname, ipt=0):
    """TILE of a specialised semiring of this type under option pull_ipt."""
    small = np.dtype(_np(tname)).itemsize <= 4
    return 256 * (ipt if ipt and small else (8 if small else 4))


def _tile_rows(rowptr, tile):
    """tile_row[0 .. n_tiles] by the definition of the module docstring -- the reference for the witnesses."""
    rowptr = np.asarray(rowptr, np.int64)
    m, nnz = rowptr.size - 1, int(rowptr[-1])
    n_tiles = -(-(m + nnz) // tile)
    ends = np.arange(m) + rowptr[1:]
    diag = np.minimum(np.arange(n_tiles + 1) * tile, m + nnz)
    return np.searchsorted(ends, diag, side="left")


class _Lay:
    """Row lengths laid along the merge path: `pos` is the position the next row's first entry (or, if it is empty, its end) gets."""

    def __init__(self, lead=0):
        self.lens, self.pos = [], 0
        for _ in range(lead):
            self.row(0)

    def row(self, ln):
        self.lens.append(int(ln))
        self.pos += ln + 1
        return len(self.lens) - 1

    def fill_to(self, p):
        """Filler rows until the next row starts at position p."""
        assert p >= self.pos, (p, self.pos)
        while p - self.pos > 9:
            self.row(FILL[len(self.lens) % len(FILL)])
        if p > self.pos:
            self.row(p - self.pos - 1)
        assert self.pos == p

    def fill_tiles(self, k, tile):
        self.fill_to((self.pos // tile + k) * tile + 17)

    def align(self, residue, tile, off=0):
        """Filler rows until the next row has an index = residue (mod 64) AND starts `off` positions in front of a tile boundary."""
        k = (residue - len(self.lens)) % 64
        if k < 2:
            k += 64
        p = -(-(self.pos + k + off + 1) // tile) * tile - off
        e = p - self.pos - k
        for j in range(k):
            self.row(e // k + (e % k if j == k - 1 else 0))
        assert self.pos == p and len(self.lens) % 64 == residue
        return p

    def rowptr(self):
        return np.concatenate([[0], np.cumsum(self.lens)]).astype(np.int64)


def _first(rp, i):
    return i + int(rp[i])      # (merge position of row i's first entry)


def _end(rp, i):
    return i + int(rp[i + 1])  # (merge position of row i's end)


def _matrix(lens, n, tname, marks=(), pin_last=()):
    """COO arrays of the matrix with these row lengths: row i holds the ascending columns s_i, s_i + 1, ..; values 3 .. 9 (BOOL: a third
    of them true), except the k-th entry of row r for (r, k) in marks: 1, 2, 10, 11, .. in the order given (BOOL: the only true entries
    of their rows).  The last entry of the rows of pin_last is moved to the last column."""
    lens = np.asarray(lens, np.int64)
    m = lens.size
    assert lens.max() <= n
    rp = np.concatenate([[0], np.cumsum(lens)])
    rows = np.repeat(np.arange(m), lens)
    kth = np.arange(rows.size) - rp[rows]
    cols = (rows * 37) % (n - lens[rows] + 1) + kth
    for r in pin_last:
        cols[rp[r + 1] - 1] = n - 1
    if tname == "BOOL":
        vals = (cols + rows) % 3 == 0
        for r in {r for r, _ in marks}:
            vals[rp[r]:rp[r + 1]] = False
        for r, k in marks:
            vals[rp[r] + k % lens[r]] = True
    else:
        vals = (3 + (cols * 3 + rows) % 7).astype(_np(tname))
        seen = {}
        for r, k in marks:
            vals[rp[r] + k % lens[r]] = (1, 2, 10, 11, 12, 13)[seen.setdefault(r, 0)]
            seen[r] += 1
    return rows, cols, vals


def _bool_operand(n, full):
    """BOOL operand whose values differ between neighbouring columns; not full: every fifth column absent."""
    c = np.arange(n)
    val = (c * 3 + c // 16) % 2 == 0
    if full:
        return c, val
    keep = c % 5 != 2
    return c[keep], val[keep]


def _grown_equals(w, exp, where):
    """No presence bit above the size: grown by 200, the vector holds what it held."""
    w.resize(w.size + 200)
    gi, gv = w.to_coo()
    same_values(gi, gv, exp.idx, exp.vals, None, where + ", grown by 200")


def _plain_path(where, want_tiles):
    """The witness of every pull call: the plain path ran (method 1, no split) over the tiles the host function counts."""
    from graphblas_amd import device

    st = device.last_stats()
    assert st["method"] == 1 and st["long_kernel"] == -1 and st["tiles"] == want_tiles, (where, want_tiles, st)


ACCUM = {"plus_times": "plus", "min_plus": "min", "lor_land": "lor", "any_pair": "lor", "plus_pair": "plus", "lxor_pair": "lor"}


def _pull_ways(gb, lens, tname, tile, special, marks=(), srs=None, operand=None, n_min=0, wtype=None, alias=True, opts=(), pin_last=()):
    """Build the matrix of these row lengths (square when the longest row allows it, else with a square twin that has empty rows behind the
    last one) and run every semiring of `srs` the ways the module docstring names, each against the oracle and each with the statistics
    of the plain path and the tile count of _tile_rows.  `special` rows: admitted in one masked round, masked out in the other; w holds an
    old entry under each of them.  Returns the row pointers."""
    from graphblas_amd import device

    lens = np.asarray(lens, np.int64)
    m = lens.size
    n = max(int(lens.max()), n_min) if n_min else max(int(lens.max()), m)
    rows, cols, vals = _matrix(lens, n, tname, marks, pin_last)
    rp = np.concatenate([[0], np.cumsum(lens)])
    tiles = _tile_rows(rp, tile).size - 1
    oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
    wt = wtype or tname
    special = np.asarray(sorted(set(special)), np.int64)
    rng = np.random.default_rng(m * 7 + n)
    ui, uv = operand if operand is not None else (_bool_operand(n, False) if tname == "BOOL" else _operand(n, tname))
    ou = O.OVec(n, ui, uv, tname)
    wi = np.union1d(np.flatnonzero(rng.random(m) < 0.6), special)
    wv = (wi % 2 == 0) if wt == "BOOL" else (1 + wi % 9).astype(_np(wt))
    ow = O.OVec(m, wi, wv, wt)
    try:
        set_opts(((b"push_mode", 0),) + tuple(opts))
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
        u = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)

        def plain_path(where, want_tiles=tiles):
            _plain_path(where, want_tiles)

        for sr in srs or (("lor_land",) if tname == "BOOL" else ("plus_times", "min_plus")):
            semi, accum = getattr(gb.semiring, sr), ACCUM[sr]
            got = A.mxv(u, semi).new(dtype=wt)
            plain_path((sr, "plain"))
            exp = O.mxv(oa, ou, sr, out_type=wt)
            same_vec(got, exp, where=f"{sr} plain")
            _grown_equals(got, exp, f"{sr} plain")
            for admitted in (True, False):
                in_mask = rng.random(m) < 0.5
                in_mask[special] = not admitted
                mi = np.flatnonzero(in_mask)
                mk = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=m)
                om = O.OVec(m, mi, np.ones(mi.size, bool), "BOOL")
                for kw, okw in ((dict(accum=getattr(gb.binary, accum)), dict(accum=accum)), (dict(replace=True), dict(replace=True))):
                    where = f"{sr} special rows {'admitted' if admitted else 'masked out'} {sorted(okw)}"
                    w = gb.Vector.from_coo(wi, wv, dtype=wt, size=m)
                    w(~mk.S, **kw) << A.mxv(u, semi)
                    plain_path(where)
                    exp = O.mxv(oa, ou, sr, w=ow, mask=om, mask_comp=True, mask_struct=True, **okw)
                    same_vec(w, exp, where=where)
                    _grown_equals(w, exp, where)
        if alias and wtype is None:
            # w IS u: the tiles write into fresh buffers (PullArgs::fresh), every kept entry is copied
            big = max(m, n)
            r2, c2, v2 = (rows, cols, vals) if m == n else _matrix(np.concatenate([lens, np.zeros(big - m, np.int64)]), n, tname, marks, pin_last)
            rp2 = np.concatenate([rp, np.full(big - m, rp[-1])])
            osq = O.OMat.from_coo(r2, c2, v2, big, big, tname)
            Asq = A if m == n else gb.Matrix.from_coo(r2, c2, v2, dtype=tname, nrows=big, ncols=big)
            in_mask = rng.random(big) < 0.5
            in_mask[special] = False
            mi = np.flatnonzero(in_mask)
            mk = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=big)
            om = O.OVec(big, mi, np.ones(mi.size, bool), "BOOL")
            for sr in srs or (("lor_land",) if tname == "BOOL" else ("plus_times", "min_plus")):
                q = gb.Vector.from_coo(ui, uv, dtype=tname, size=big)
                q(~mk.S, replace=True) << Asq.mxv(q, getattr(gb.semiring, sr))
                plain_path((sr, "aliased"), _tile_rows(rp2, tile).size - 1)
                oq = O.OVec(big, ui, uv, tname)
                exp = O.mxv(osq, oq, sr, w=oq, mask=om, mask_comp=True, mask_struct=True, replace=True)
                same_vec(q, exp, where=f"{sr} w aliased to u")
                _grown_equals(q, exp, f"{sr} w aliased to u")
    finally:
        reset_opts()
    return rp


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. a row end split from its row; 8. the same through the unfused write rule
# ------------------------------------------------------------------------------------------------------------------------------------
def _row_end_layout(tile):
    """Rows RA, RB, RC in filler: RA's 5 entries are the last 5 items of a tile, its end the first item of the next one; RB's end is the
    last item of a tile and RC's first entry opens the next tile, which RC (TILE + 5 entries) fills: RC is the seam of the tile after."""
    lay = _Lay()
    lay.fill_tiles(1, tile)
    ta = lay.pos // tile + 1
    lay.fill_to((ta + 1) * tile - 5)
    ra = lay.row(5)
    lay.fill_tiles(1, tile)
    tb = lay.pos // tile + 1
    lay.fill_to((tb + 1) * tile - 4)
    rb = lay.row(3)
    rc = lay.row(tile + 5)
    lay.fill_tiles(1, tile)
    lay.row(2)
    if len(lay.lens) % 64 == 0:
        lay.row(0)
    rp = lay.rowptr()
    tr = _tile_rows(rp, tile)
    # RA: last entry = last item of tile ta, end = first item of tile ta + 1, whose first row it therefore is -- with no entry there
    assert _end(rp, ra) == (ta + 1) * tile and tr[ta + 1] == ra and tr[ta] < ra and _first(rp, ra) // tile == ta
    # RB: end = last item of tile tb (owned by tb: no seam); RC: first entry = first item of tile tb + 1 (t_s an exact quotient), seam of tb + 2
    assert _end(rp, rb) == (tb + 1) * tile - 1 and tr[tb + 1] == rc == rb + 1
    assert _first(rp, rc) == (tb + 1) * tile and tr[tb + 2] == rc and _end(rp, rc) == (tb + 2) * tile + 5
    return lay.lens, (ra, rb, rc), ((ra, 4), (ra, 0), (rb, 2), (rc, 0), (rc, tile - 1), (rc, tile))


@pytest.mark.parametrize("tname", ["FP32", "INT64", "BOOL"])
def test_row_end_on_a_tile_boundary(gb, tname):
    """k_mxv_pull: `se ? 2 | (s_thas[0] ? 1 : 0)` -- a row whose last entry is the last item of a tile leaves the next tile a seam without a
    partial of its own (first_has == 2), which k_mxv_seams must fold from the carry alone; a row end ON the last item (`start < nnz_t`,
    own_lo 0 in the next tile: no seam at all); a row whose first entry opens a tile (k_mxv_seams: `t_s = (row + rowptr[row]) / TILE` an
    exact quotient).  Each with the row admitted, masked out, and masked out under replace with an old entry in w.  BOOL: lor_land over
    presence / value pairs (u_pv)."""
    tile = _tile(tname)
    lens, special, marks = _row_end_layout(tile)
    _pull_ways(gb, lens, tname, tile, special, marks)


@pytest.mark.parametrize("tname, wtype", [("FP32", "FP64"), ("INT64", "INT32")])
def test_row_end_on_a_tile_boundary_unfused_write(gb, tname, wtype):
    """mxv_core, `fused = (w->type->code == st)` false: the same seams into a temporary of the semiring's type (no mask, no accumulator in
    the tiles), then k_vec_write with the typecast, mask, accumulator and replace."""
    tile = _tile(tname)
    lens, special, marks = _row_end_layout(tile)
    _pull_ways(gb, lens, tname, tile, special, marks, wtype=wtype)


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. a row over more than 64 tiles
# ------------------------------------------------------------------------------------------------------------------------------------
def _long_row_layout(tile):
    """Row H begins 100 items into tile t_s and ends 50 items into tile t_s + 66: 66 carries, the last two on the second trip of the fold."""
    lay = _Lay()
    lay.fill_tiles(1, tile)
    ts = lay.pos // tile + 1
    lay.fill_to(ts * tile + 100)
    h = lay.row(66 * tile - 50)
    for _ in range(40):
        lay.row(FILL[len(lay.lens) % len(FILL)])
    rp = lay.rowptr()
    tr = _tile_rows(rp, tile)
    assert _first(rp, h) // tile == ts and _end(rp, h) == (ts + 66) * tile + 50 and (tr[ts + 1:ts + 67] == h).all() and tr[ts + 67] > h
    return lay.lens, h, ts


def _in_tile(rp, h, tile, t):
    """The entry numbers of row h that lie in tile t."""
    k0 = max(0, t * tile - _first(rp, h))
    k1 = min(int(rp[h + 1] - rp[h]), (t + 1) * tile - _first(rp, h))
    return k0, k1


@pytest.mark.parametrize("tname, ipt", [("INT64", 0), ("FP64", 0), ("FP32", 4)])
def test_row_over_more_than_64_tiles(gb, tname, ipt):
    """k_mxv_seams: `for (t = t_s + lane; t < tile; t += 64)` -- a row of 66 tiles of 1024 puts the carries of t_s + 64 and t_s + 65 on the
    second trip of lanes 0 and 1.  Under min_plus the unique minimum sits in the carry of t_s, of t_s + 64 and in the last tile's own
    first partial (first_has bit 0) in turn; then a sparse operand meets the row in tile t_s + 65 alone (every other carry has
    carry_has == 0) and one meets it nowhere (the row is absent although it has entries)."""
    from graphblas_amd import device

    tile = _tile(tname, ipt)
    assert tile == 1024
    lens, h, ts = _long_row_layout(tile)
    opts = ((b"pull_ipt", ipt),) if ipt else ()
    m, n = len(lens), int(max(lens)) + 500
    rp = _pull_ways(gb, lens, tname, tile, [h], ((h, 0),), opts=opts, n_min=n)
    rows, cols, vals = _matrix(lens, n, tname)
    ui, uv = _operand(n, tname)
    hcols = cols[rp[h]:rp[h + 1]]
    try:
        set_opts(((b"push_mode", 0),) + opts)
        u = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
        ou = O.OVec(n, ui, uv, tname)
        for t in (ts, ts + 64, ts + 66):
            k0, k1 = _in_tile(rp, h, tile, t)
            k = k0 + int(np.flatnonzero(uv[hcols[k0:k1]] == 1)[0])  # (an entry of that tile under an operand value of 1)
            v2 = vals.copy()
            v2[rp[h] + k] = 1  # (1 + 1: every other product of the row is at least 3 + 1)
            A = gb.Matrix.from_coo(rows, cols, v2, dtype=tname, nrows=m, ncols=n)
            got = A.mxv(u, gb.semiring.min_plus).new()
            _plain_path(f"minimum in tile t_s + {t - ts}", _tile_rows(rp, tile).size - 1)
            exp = O.mxv(O.OMat.from_coo(rows, cols, v2, m, n, tname), ou, "min_plus")
            assert exp.vals[np.searchsorted(exp.idx, h)] == 2
            same_vec(got, exp, where=f"minimum in tile t_s + {t - ts}")
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
        oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
        k0, k1 = _in_tile(rp, h, tile, ts + 65)
        for name, si in (("tile t_s + 65 alone", hcols[k0 + 3:k1:97]), ("nowhere", np.setdiff1d(np.arange(n), hcols)[::7])):
            assert si.size > 0
            sv = (1 + si % 9).astype(_np(tname))
            s = gb.Vector.from_coo(si, sv, dtype=tname, size=n)
            for sr in ("min_plus", "plus_times"):
                got = A.mxv(s, getattr(gb.semiring, sr)).new()
                _plain_path((sr, name), _tile_rows(rp, tile).size - 1)
                exp = O.mxv(oa, O.OVec(n, si, sv, tname), sr)
                assert (h in exp.idx) == (name != "nowhere")
                same_vec(got, exp, where=f"{sr}, a sparse operand that meets the row {name}")
    finally:
        reset_opts()


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. tiles made of row ends only; 4. a 64-row group shared by two tiles and a seam; 6. no active row in a tile
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["FP32", "INT64"])
def test_tile_of_row_ends_only(gb, tname):
    """k_mxv_pull, `s_act[TILE / 32 + 3]`, `abase = i0 & 31`, `nw = (last_row >> 5) - (i0 >> 5) + 1`: TILE + 70 empty rows from a row i0 with
    i0 % 64 == 63 whose end is the first item of a tile -- that tile is TILE row ends, nrows_t = TILE, abase = 31, and ROW_ACTIVE reads
    word (31 + TILE) >> 5 = TILE / 32 of s_act: nw = TILE / 32 + 1, the most a tile can need (i1 - i0 <= TILE, so (i1 >> 5) - (i0 >> 5)
    <= TILE / 32; a tile never loads TILE / 32 + 2 words).  The mask differs from row to row and w holds old entries there; with an
    accumulator and without one under replace.  The first and the last 64-row group of the tile are partly owned (atomicAnd / atomicOr
    on the presence word), the others wholly (the plain store): the presence must equal the oracle's."""
    tile = _tile(tname)
    lay = _Lay()
    lay.fill_tiles(1, tile)
    p = lay.align(63, tile)
    i0 = len(lay.lens)
    for _ in range(tile + 70):
        lay.row(0)
    lay.fill_tiles(1, tile)
    lay.row(3)
    rp = lay.rowptr()
    tr = _tile_rows(rp, tile)
    t = p // tile
    assert i0 % 64 == 63 and i0 % 32 == 31 and tr[t] == i0 and tr[t + 1] == i0 + tile and rp[i0] == rp[i0 + tile + 70]
    assert ((i0 + tile) >> 5) - (i0 >> 5) + 1 == tile // 32 + 1
    _pull_ways(gb, lay.lens, tname, tile, [i0, i0 + 1, i0 + 64, i0 + tile - 1, i0 + tile])


@pytest.mark.parametrize("residue", [0, 63, 20])
@pytest.mark.parametrize("tname", ["FP32", "INT64"])
def test_row_group_shared_by_two_tiles_and_a_seam(gb, tname, residue):
    """k_mxv_pull, `own_lo`, `row_lo = i0 + own_lo`, `if (om == ~0ull) .. else atomicAnd / atomicOr`; k_mxv_seams' atomicOr / atomicAnd on the
    same word: a tile boundary inside a 64-row group of short rows, through the seam row itself (3 of its 6 entries on either side).  The
    group's presence word is written by the tile in front (rows below the seam), the tile behind (rows above it) and the seams kernel
    (its one bit).  residue 20: the seam in the middle of the group; 0: the seam is the group's first row, the tile in front owns
    nothing of it; 63: row_lo is a multiple of 64, the tile behind owns the next group wholly."""
    tile = _tile(tname)
    lay = _Lay()
    lay.fill_tiles(1, tile)
    p = lay.align(residue, tile, off=3)
    s = lay.row(6)
    lay.fill_tiles(1, tile)
    lay.row(1)
    rp = lay.rowptr()
    tr = _tile_rows(rp, tile)
    t = (p + 3) // tile
    assert (p + 3) % tile == 0 and _first(rp, s) == t * tile - 3 and tr[t] == s and s % 64 == residue and tr[t + 1] > s + 64 - residue
    _pull_ways(gb, lay.lens, tname, tile, [s - 1, s, s + 1], ((s, 2), (s, 3)))


@pytest.mark.parametrize("tname", ["FP32", "INT64"])
def test_tile_without_an_admitted_row(gb, tname):
    """k_mxv_pull, `s_any` / `any_active`: a tile none of whose rows [i0, min(i1, m - 1)] the mask admits skips its gathers and folds but
    still applies the write rule and leaves carry_has = 0, first_has as the seam needs it.  Tile t here begins inside row L (which began
    in tile t - 1) and ends inside row R (which goes on into tile t + 1).  Round 1 admits everything but the rows of tile t (L, R and the
    rows between): L's and R's seams must be written as masked-out rows although their other tiles ran.  Round 2 admits, of those rows,
    R alone (the open row: `last_row = i1` counts it), round 3 L alone (the tile's first row, whose partial goes to first_val)."""
    from graphblas_amd import device

    tile = _tile(tname)
    lay = _Lay()
    lay.fill_tiles(1, tile)
    t = lay.pos // tile + 1
    lay.fill_to(t * tile - 40)
    left = lay.row(90)
    lay.fill_to((t + 1) * tile - 30)
    right = lay.row(70)
    lay.fill_tiles(1, tile)
    lay.row(2)
    lens = np.asarray(lay.lens, np.int64)
    rp = lay.rowptr()
    tr = _tile_rows(rp, tile)
    assert tr[t] == left and tr[t + 1] == right and _first(rp, left) < t * tile < _end(rp, left) and _first(rp, right) < (t + 1) * tile < _end(rp, right)
    m = n = lens.size
    rows, cols, vals = _matrix(lens, n, tname, ((left, 39), (left, 40), (right, 29), (right, 30)))
    oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
    ui, uv = _operand(n, tname)
    rng = np.random.default_rng(5)
    wi = np.union1d(np.flatnonzero(rng.random(m) < 0.6), [left, right, left + 1])
    wv = (1 + wi % 9).astype(_np(tname))
    try:
        set_opts(((b"push_mode", 0),))
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
        u, ou = gb.Vector.from_coo(ui, uv, dtype=tname, size=n), O.OVec(n, ui, uv, tname)
        for admitted in ((), (right,), (left,)):
            in_mask = rng.random(m) < 0.4
            in_mask[left:right + 1] = True
            in_mask[np.asarray(admitted, np.int64)] = False
            mi = np.flatnonzero(in_mask)
            # (the rows k_mxv_pull tests for `s_any` in tile t are [tile_row[t], min(tile_row[t + 1], m - 1)]: the complemented mask admits
            #  exactly the rows of `admitted` there -- none in round 1 -- and rows on both sides of them in the neighbouring tiles)
            assert np.flatnonzero(~in_mask[tr[t]:min(tr[t + 1], m - 1) + 1]).tolist() == [r - tr[t] for r in sorted(admitted)]
            assert (~in_mask[tr[t - 1]:tr[t]]).any() and (~in_mask[tr[t + 1] + 1:tr[t + 2] + 1]).any()
            mk, om = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=m), O.OVec(m, mi, np.ones(mi.size, bool), "BOOL")
            for sr, accum in (("plus_times", "plus"), ("min_plus", "min")):
                for kw, okw in ((dict(accum=getattr(gb.binary, accum)), dict(accum=accum)), (dict(replace=True), dict(replace=True))):
                    w = gb.Vector.from_coo(wi, wv, dtype=tname, size=m)
                    w(~mk.S, **kw) << A.mxv(u, getattr(gb.semiring, sr))
                    st = device.last_stats()
                    assert st["method"] == 1 and st["long_kernel"] == -1 and st["tiles"] == tr.size - 1, st
                    same_vec(w, O.mxv(oa, ou, sr, w=O.OVec(m, wi, wv, tname), mask=om, mask_comp=True, mask_struct=True, **okw),
                             where=f"{sr} {sorted(okw)}, admitted of tile {t}: {admitted}")
    finally:
        reset_opts()


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. the end of the arrays
# ------------------------------------------------------------------------------------------------------------------------------------
def _array_end_layout(tile, tail):
    """tail 1 .. 4: the last row opens a tile and holds TILE + tail entries -- that tile has `left = nnz - j0` = TILE + tail (the 16-byte
    loads run only from TILE + 4 on), the last tile `left` = tail, and the last row is a seam.  "exact" / "exact+1": the last row (7
    entries) ends on the last item of the last tile / is followed by one empty row whose end is a tile of its own (left = 0)."""
    for lead in range(4):
        lay = _Lay(lead)
        lay.fill_tiles(2 if tile <= 1024 else 1, tile)
        if isinstance(tail, int):
            t = lay.pos // tile + 1
            lay.fill_to(t * tile)
            last = lay.row(tile + tail)
        else:
            t = lay.pos // tile + 1
            lay.fill_to((t + 1) * tile - 8)
            last = lay.row(7)
            if tail == "exact+1":
                lay.row(0)
        if len(lay.lens) % 64 and max(lay.lens) <= len(lay.lens):
            break
    rp = lay.rowptr()
    tr = _tile_rows(rp, tile)
    m, nnz = len(lay.lens), int(rp[-1])
    assert m % 64 != 0
    if isinstance(tail, int):
        assert _first(rp, last) == t * tile and tr.size - 1 == t + 2 and tr[t + 1] == last == m - 1 and nnz - (t * tile - tr[t]) == tile + tail
        assert nnz - ((t + 1) * tile - tr[t + 1]) == tail
    else:
        assert (m + nnz) % tile == (0 if tail == "exact" else 1) and _end(rp, last) == (t + 1) * tile - 1 and tr.size - 1 == t + 1 + (tail != "exact")
    return lay.lens, last


@pytest.mark.parametrize("tail", [1, 2, 3, 4, "exact", "exact+1"])
@pytest.mark.parametrize("tname", ["FP32", "INT64", "BOOL"])
def test_end_of_the_arrays(gb, tname, tail):
    """k_mxv_pull, `whole = left >= TILE + 4` and the buffer descriptors `make_rsrc(a.col + j0, left * 4)`: with fewer than TILE + 4 entries
    left a tile reads entry by entry and what lies past the end of the arrays reads as 0 through the descriptor; `d1 = min(d0 + TILE,
    total)`, `i0 + tid < a.m`, `last_row = i1 < m ? i1 : m - 1` at the last tile; m is no multiple of 64 (`(pre_g << 6) < a.m`, the
    partly owned last group): no presence bit above m may be left (every result is grown by 200).  See _array_end_layout.  BOOL: lor_land
    over presence / value pairs (u_pv), over a full operand (u_valbits), and any_pair over a sparse operand that holds the columns of the
    last row's marked entries."""
    tile = _tile(tname)
    lens, last = _array_end_layout(tile, tail)
    k = len(lens) - 1
    marks = ((last, 0), (last, lens[last] - 1)) + (((last, tile - 1), (last, tile)) if isinstance(tail, int) else ())
    _pull_ways(gb, lens, tname, tile, [last, k, k - 1], marks)
    if tname == "BOOL":
        n = len(lens)  # (square: _array_end_layout makes no row longer than m)
        _pull_ways(gb, lens, tname, tile, [last, k, k - 1], marks, operand=_bool_operand(n, True), alias=False)
        c0 = (last * 37) % (n - lens[last] + 1)  # (first column of the last row, see _matrix)
        c = np.arange(n)
        sparse = np.union1d(c[c % 7 == 3], [c0 + kk for _, kk in marks])
        _pull_ways(gb, lens, tname, tile, [last, k, k - 1], marks, srs=("any_pair",), operand=(sparse, np.ones(sparse.size, bool)))


# ------------------------------------------------------------------------------------------------------------------------------------
# 7. BOOL operands
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_u", [16 * 300 - 1, 16 * 300, 16 * 300 + 1])
def test_bool_operand_words(gb, n_u):
    """bool_pv_gather (`cc >> 4`, 16 codes of presence / value pairs per word, descriptor of ((x_len + 15) >> 4) * 4 bytes) with operands
    of 16 k - 1, 16 k and 16 k + 1 entries whose last column is referred to; the full operand (u_valbits, `cc >> 5`) and any_pair over
    a sparse operand (presence alone) on the same matrix -- the row-end layout of case 1 with the last column in the marked rows."""
    tile = _tile("BOOL")
    lens, special, marks = _row_end_layout(tile)
    kw = dict(n_min=n_u, alias=False, pin_last=special)  # (the last entry of RA, RB and RC -- RA's is marked -- is at the last column)
    _pull_ways(gb, lens, "BOOL", tile, special, marks, **kw)
    _pull_ways(gb, lens, "BOOL", tile, special, marks, operand=_bool_operand(n_u, True), **kw)
    c = np.arange(n_u)
    sparse = c[(c % 7 == 3) | (c == n_u - 1)]
    _pull_ways(gb, lens, "BOOL", tile, special, marks, srs=("any_pair",), operand=(sparse, np.ones(sparse.size, bool)), **kw)


@pytest.mark.parametrize("form", ["pairs", "full", "any_pair"])
def test_bool_row_over_more_than_64_tiles(gb, form):
    """Case 2 for BOOL under pull_ipt 4 (TILE 1024): lor_land with the only true entry of the 66-tile row in the carry of t_s + 64, the
    operand as presence / value pairs and full; any_pair over a sparse operand that meets the row in that one entry alone (the carry of
    t_s + 64 is the only one with carry_has set: the second trip of the fold decides whether the row exists)."""
    tile = _tile("BOOL", 4)
    lens, h, ts = _long_row_layout(tile)
    rp = np.concatenate([[0], np.cumsum(lens)])
    k0, k1 = _in_tile(rp, h, tile, ts + 64)
    assert k0 + 5 < k1
    n = int(max(lens)) + 500
    c0 = (h * 37) % (n - lens[h] + 1)  # (first column of row h, see _matrix)
    col = c0 + k0 + 5
    if form == "any_pair":
        outside = np.setdiff1d(np.arange(n), np.arange(c0, c0 + lens[h]))
        ui = np.union1d(outside[::3], [col])
        _pull_ways(gb, lens, "BOOL", tile, [h], ((h, k0 + 5),), srs=("any_pair",), operand=(ui, np.ones(ui.size, bool)),
                   opts=((b"pull_ipt", 4),), n_min=n)
        return
    ui, uv = _bool_operand(n, form == "full")
    uv = uv.copy()
    if col in ui:
        uv[np.searchsorted(ui, col)] = True
    else:
        at = np.searchsorted(ui, col)
        ui, uv = np.insert(ui, at, col), np.insert(uv, at, True)
    _pull_ways(gb, lens, "BOOL", tile, [h], ((h, k0 + 5),), operand=(ui, uv), opts=((b"pull_ipt", 4),), alias=form == "pairs", n_min=n)


# ------------------------------------------------------------------------------------------------------------------------------------
# 9. the tile table follows the tile size
# ------------------------------------------------------------------------------------------------------------------------------------
def test_tile_table_follows_the_tile_size(gb):
    """ensure_tile_table (`A->tile.tile_items == tile_items`): the cached table is rebuilt when a call comes with another TILE -- one FP32
    matrix under pull_ipt 0, 4, 16, 0; one INT32 matrix under an INT32 semiring (TILE 2048) and an INT64 one (1024) -- and dropped with
    the matrix's content: after a resize that cuts rows and entries off and after an element-wise update that adds one, the count is
    that of the new m + nnz.  Each product against the oracle, each with the tile count of its TILE."""
    from graphblas_amd import device

    lay = _Lay()
    lay.fill_tiles(5, 1024)
    lay.row(1500)
    lay.fill_tiles(1, 1024)
    lens = np.asarray(lay.lens, np.int64)
    m = n = lens.size
    assert lens.max() <= n
    rp = lay.rowptr()
    try:
        set_opts(((b"push_mode", 0),))
        rows, cols, vals = _matrix(lens, n, "FP32")
        A, oa = gb.Matrix.from_coo(rows, cols, vals, dtype="FP32", nrows=m, ncols=n), O.OMat.from_coo(rows, cols, vals, m, n, "FP32")
        ui, uv = _operand(n, "FP32")
        u, ou = gb.Vector.from_coo(ui, uv, dtype="FP32", size=n), O.OVec(n, ui, uv, "FP32")
        counts = []
        for ipt in (0, 4, 16, 0):
            set_opts(((b"pull_ipt", ipt),))
            for sr in ("min_plus", "plus_times"):
                got = A.mxv(u, getattr(gb.semiring, sr)).new()
                st = device.last_stats()
                assert st["method"] == 1 and st["tiles"] == _tile_rows(rp, _tile("FP32", ipt)).size - 1, (ipt, st)
                same_vec(got, O.mxv(oa, ou, sr), where=f"pull_ipt {ipt} {sr}")
            counts.append(st["tiles"])
        assert counts[0] == counts[3] and len(set(counts[:3])) == 3, counts
        # content changes: rows and entries cut off, then one entry added
        m2 = m - 300
        A.resize(m2, n)
        keep = rows < m2
        r2, c2, v2 = rows[keep], cols[keep], vals[keep]
        for step in ("resize", "one entry more"):
            if step != "resize":
                e = int(np.flatnonzero(lens[:m2] == 0)[3])  # (an empty row gets an entry)
                D = gb.Matrix.from_coo([e], [5], np.array([4], np.float32), dtype="FP32", nrows=m2, ncols=n)
                A << A.ewise_add(D, gb.binary.second)
                r2, c2, v2 = np.append(r2, e), np.append(c2, 5), np.append(v2, np.float32(4))
            oa2 = O.OMat.from_coo(r2, c2, v2, m2, n, "FP32")
            got = A.mxv(u, gb.semiring.plus_times).new()
            st = device.last_stats()
            assert st["method"] == 1 and st["tiles"] == -(-(m2 + r2.size) // 2048) == _tile_rows(oa2.indptr, 2048).size - 1, (step, st)
            same_vec(got, O.mxv(oa2, ou, "plus_times"), where=step)
        # one INT32 matrix, two semiring types
        rows, cols, vals = _matrix(lens, n, "INT32")
        B, ob = gb.Matrix.from_coo(rows, cols, vals, dtype="INT32", nrows=m, ncols=n), O.OMat.from_coo(rows, cols, vals, m, n, "INT32")
        ui, uv = _operand(n, "INT32")
        x = gb.Vector.from_coo(ui, uv, dtype="INT32", size=n)
        for st_name, tile in (("INT32", 2048), ("INT64", 1024), ("INT32", 2048)):
            got = B.mxv(x, gb.semiring.plus_times[st_name]).new()
            st = device.last_stats()
            assert st["method"] == 1 and st["tiles"] == _tile_rows(rp, tile).size - 1, (st_name, st)
            exp = O.mxv(ob.astype(st_name), O.OVec(n, ui, uv.astype(_np(st_name)), st_name), "plus_times")
            same_vec(got, exp, where=f"INT32 matrix under a {st_name} semiring")
    finally:
        reset_opts()


# ------------------------------------------------------------------------------------------------------------------------------------
# 10. the row-length kernel
# ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname", ["INT8", "UINT8", "INT64", "BOOL"])
@pytest.mark.parametrize("m", [63, 64, 65, 257])
def test_rowlen_kernel(gb, tname, m):
    """k_mxv_rowlen (method 5; pull_dispatch: `mul == OP_PAIR && a.u_full`): plus_pair, lxor_pair (a BOOL semiring: the BOOL matrix) and
    any_pair over a full operand are functions of the row length -- `(T)len` wraps in INT8 / UINT8 like the oracle's sum of ones (rows
    of 200 and 300 entries), `len & 1`, 1.  m = 63, 64, 65, 257: `g < (a.m + 63) >> 6` and the bits of the last word above m.  With and without a mask, accumulator and
    replace."""
    from graphblas_amd import device

    n = 300
    lens = np.array([(0, 1, 200, 300, 2, 0, 255, 256, 128, 3)[i % 10] for i in range(m)], np.int64)
    lens[m - 1] = 300
    rows, cols, vals = _matrix(lens, n, tname)
    oa = O.OMat.from_coo(rows, cols, vals, m, n, tname)
    ui, uv = _operand(n, tname)
    rng = np.random.default_rng(m)
    wi = np.flatnonzero(rng.random(m) < 0.6)
    wv = (wi % 2 == 0) if tname == "BOOL" else (1 + wi % 9).astype(_np(tname))
    mi = np.flatnonzero(rng.random(m) < 0.5)
    try:
        set_opts(((b"push_mode", 0),))
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=m, ncols=n)
        u, ou = gb.Vector.from_coo(ui, uv, dtype=tname, size=n), O.OVec(n, ui, uv, tname)
        mk, om = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=m), O.OVec(m, mi, np.ones(mi.size, bool), "BOOL")
        for sr in ("lxor_pair", "any_pair") if tname == "BOOL" else ("plus_pair", "any_pair"):
            semi = getattr(gb.semiring, sr)
            accum = "lor" if tname == "BOOL" else "plus"
            got = A.mxv(u, semi).new()
            assert device.last_stats()["method"] == 5, device.last_stats()
            exp = O.mxv(oa, ou, sr)
            same_vec(got, exp, where=f"{sr} plain")
            _grown_equals(got, exp, f"{sr} plain")
            for kw, okw in ((dict(accum=getattr(gb.binary, accum)), dict(accum=accum)), (dict(replace=True), dict(replace=True)),
                            (dict(accum=getattr(gb.binary, accum), replace=True), dict(accum=accum, replace=True))):
                w = gb.Vector.from_coo(wi, wv, dtype=tname, size=m)
                w(~mk.S, **kw) << A.mxv(u, semi)
                assert device.last_stats()["method"] == 5, device.last_stats()
                exp = O.mxv(oa, ou, sr, w=O.OVec(m, wi, wv, tname), mask=om, mask_comp=True, mask_struct=True, **okw)
                same_vec(w, exp, where=f"{sr} {sorted(okw)}")
                _grown_equals(w, exp, f"{sr} {sorted(okw)}")
            w = gb.Vector.from_coo(wi, wv, dtype=tname, size=m)
            w(accum=getattr(gb.binary, accum)) << A.mxv(u, semi)
            assert device.last_stats()["method"] == 5
            same_vec(w, O.mxv(oa, ou, sr, w=O.OVec(m, wi, wv, tname), accum=accum), where=f"{sr} accumulated, no mask")
    finally:
        reset_opts()


# ------------------------------------------------------------------------------------------------------------------------------------
# push direction: u' A under push_mode 2
# ------------------------------------------------------------------------------------------------------------------------------------
def _push_matrix(lens, n, tname):
    rows, cols, vals = _matrix(lens, n, tname)
    return rows, cols, vals, O.OMat.from_coo(rows, cols, vals, n, n, tname)


def _frontier(fi, tname):
    fi = np.asarray(sorted(fi), np.int64)
    return fi, ((fi % 3 != 1) if tname == "BOOL" else (1 + fi % 9).astype(_np(tname)))


def _srs(tname):
    return ("lor_land",) if tname == "BOOL" else ("plus_times", "min_plus")


def _pushed(gb, A, oa, fi, tname, sr, mk, om, lk, work, where):
    """One level step two ways -- into an empty w, and with w the frontier itself -- under ~m.S, replace: each against the oracle, each
    with method 2, the form `lk` of GrX_Stats.long_kernel (-2 one workgroup, -1 a kernel per pass, 0 the dense path) and the work."""
    from graphblas_amd import device

    n = oa.nrows
    fi, fv = _frontier(fi, tname)
    of = O.OVec(n, fi, fv, tname)
    semi = getattr(gb.semiring, sr)
    f = gb.Vector.from_coo(fi, fv, dtype=tname, size=n)
    w = gb.Vector(tname, n)
    w(~mk.S, replace=True) << f.vxm(A, semi)
    st = device.last_stats()
    assert st["method"] == 2 and st["long_kernel"] == lk and st["flops"] == work, (where, lk, work, st)
    same_vec(w, O.vxm(of, oa, sr, mask=om, mask_comp=True, mask_struct=True, replace=True), where=f"{where} {sr}, w empty")
    f(~mk.S, replace=True) << f.vxm(A, semi)
    st = device.last_stats()
    assert st["method"] == 2 and st["long_kernel"] == lk and st["flops"] == work, (where, lk, work, st)
    same_vec(f, O.vxm(of, oa, sr, w=of, mask=om, mask_comp=True, mask_struct=True, replace=True), where=f"{where} {sr}, w the frontier")


def _small_limit_matrix():
    """n = 66 000.  Row 10: 64 x 1024 entries (64 work items); rows 100 .. 4299: one entry each; rows 5000 .. 9299: empty."""
    n = 66000
    lens = np.zeros(n, np.int64)
    lens[10] = PUSH_SMALL_CHUNKS * PUSH_Q
    lens[100:4300] = 1
    return lens, n


@pytest.mark.parametrize("tname", ["INT64", "FP32", "BOOL"])
def test_push_one_workgroup_or_a_kernel_per_pass(gb, tname):
    """push_thin (grb_mxv.hip): `small = n_chunks <= PUSH_SMALL_CHUNKS && fcount <= 4096 && ..` -- frontiers of exactly 64 and 65 work items
    of 1024 entries (k_push_frontier: `(len + PUSH_Q - 1) / PUSH_Q`): one row of 64 x 1024 entries, and that row with a one-entry row;
    64 rows of one entry, and 65.  The bound on fcount is reached with 64 work items only by vertices WITHOUT entries: 4096 and 4097
    vertices of which 64 hold one entry.  long_kernel is -2 for the first of each pair, -1 for the second.  (4096 and 4097 vertices of one
    entry EACH are 4096 and 4097 work items: both a kernel per pass, by the first bound -- run too.)"""
    lens, n = _small_limit_matrix()
    rows, cols, vals, oa = _push_matrix(lens, n, tname)
    one, empty = np.arange(100, 4300), np.arange(5000, 9300)
    mi = np.flatnonzero(np.arange(n) % 3 == 1)
    try:
        set_opts(((b"push_mode", 2),))
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=n, ncols=n)
        mk, om = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=n), O.OVec(n, mi, np.ones(mi.size, bool), "BOOL")
        for sr in _srs(tname):
            for where, fi, lk in (("64 work items of one row", [10], -2), ("65 work items", [10, 100], -1),
                                  ("64 rows of one entry", one[:64], -2), ("65 rows of one entry", one[:65], -1),
                                  ("4096 vertices, 64 work items", np.concatenate([one[:64], empty[:PUSH_SMALL_FCOUNT - 64]]), -2),
                                  ("4097 vertices, 64 work items", np.concatenate([one[:64], empty[:PUSH_SMALL_FCOUNT - 63]]), -1),
                                  ("4096 rows of one entry", one[:4096], -1), ("4097 rows of one entry", one[:4097], -1)):
                _pushed(gb, A, oa, fi, tname, sr, mk, om, lk, int(lens[np.asarray(fi)].sum()), where)
    finally:
        reset_opts()


@pytest.mark.parametrize("tname", ["INT64", "FP32"])
def test_push_thin_path_to_dense_path(gb, tname):
    """push_thin: `if (fcount > a.f_cap || n_chunks > a.c_cap) return -1` with f_cap = max(n / 64 + 64, 2^16); k_push_frontier:
    `if (i >= a.f_cap) break`.  n = 70 000, every row one or two entries: a frontier of 65 536 vertices is the last the thin path takes
    (long_kernel -1), one of 65 537 goes to push_core (long_kernel stays 0) after k_push_frontier stopped writing its list at f_cap --
    still method 2 and the oracle's product.  The small thin call behind it must be right (the counters were left clean), and a call
    whose operand is of another type than the semiring's returns from push_thin at once and runs push_core."""
    from graphblas_amd import device

    n = 70000
    lens = 1 + (np.arange(n) % 2)
    rows, cols, vals, oa = _push_matrix(lens, n, tname)
    mi = np.flatnonzero(np.arange(n) % 3 == 1)
    assert max(n // 64 + 64, 1 << 16) == PUSH_F_CAP
    try:
        set_opts(((b"push_mode", 2),))
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=n, ncols=n)
        mk, om = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=n), O.OVec(n, mi, np.ones(mi.size, bool), "BOOL")
        pick = np.flatnonzero(np.arange(n) % 17 != 3)
        for sr in _srs(tname):
            for count, lk in ((PUSH_F_CAP, -1), (PUSH_F_CAP + 1, 0)):
                fi = pick[:count]
                _pushed(gb, A, oa, fi, tname, sr, mk, om, lk, int(lens[fi].sum()), f"{count} vertices")
                _pushed(gb, A, oa, [5, 77, 69999], tname, sr, mk, om, -2, int(lens[[5, 77, 69999]].sum()), f"a small call behind {count} vertices")
        # an operand of another type: no thin path
        fi = pick[:300]
        fv = (1 + fi % 9).astype(np.int32)
        f = gb.Vector.from_coo(fi, fv, dtype="INT32", size=n)
        w = gb.Vector(tname, n)
        w(~mk.S, replace=True) << f.vxm(A, gb.semiring.plus_times[tname])
        st = device.last_stats()
        assert st["method"] == 2 and st["long_kernel"] == 0, st
        same_vec(w, O.vxm(O.OVec(n, fi, fv.astype(_np(tname)), tname), oa, "plus_times", mask=om, mask_comp=True, mask_struct=True, replace=True),
                 where="INT32 operand")
    finally:
        reset_opts()


@pytest.mark.parametrize("tname", ["INT64", "FP32"])
def test_push_dense_chunks(gb, tname):
    """k_push (reached through a typecast: an INT32 operand): `x0 = thread * PUSH_CHUNK`, the binary search `pre[mid] <= x0` for the last
    frontier entry at or before x0, `x1 = x0 + PUSH_CHUNK < work ? .. : work`, `while (x >= next)`.  Frontier rows of 8, 0, 8, 7, 0, 1,
    0, 0, 9, 17, 0, 1, 7 .. entries: a thread's 8 items are exactly one row (first entry to last); begin behind an empty frontier row
    (the search must land on the LAST entry with pre <= x0); run from a row of 7 over an empty row into a row of 1 (two steps of the
    while loop); a row of 17 shared by three threads.  One-entry rows behind the pattern make the total work 8 k - 1, 8 k and 8 k + 1
    (the last thread's x1); a frontier of ONE vertex has f == 1 (no search step).  Mask complemented and not, with an accumulator."""
    from graphblas_amd import device

    pattern = (8, 0, 8, 7, 0, 1, 0, 0, 9, 17, 0, 1, 7, 8, 0, 0, 17, 9, 1, 0, 7)
    n = 3000
    lens = np.zeros(n, np.int64)
    lens[:len(pattern) * 20] = np.tile(pattern, 20)
    lens[1000:1100] = 1
    rows, cols, vals, oa = _push_matrix(lens, n, tname)
    pre = np.concatenate([[0], np.cumsum(lens)])
    # (what the pattern is for: threads whose first item is a row's first entry and whose last item is that row's last; one that starts
    #  right behind an empty frontier row; one that crosses an empty frontier row)
    starts = pre[:len(pattern)]
    assert pre[1] == PUSH_CHUNK and lens[1] == 0 and starts[2] % PUSH_CHUNK == 0 and lens[2] == 8
    assert lens[3] == 7 and lens[4] == 0 and lens[5] == 1 and pre[3] % PUSH_CHUNK == 0 and pre[6] % PUSH_CHUNK == 0
    mi = np.flatnonzero(np.arange(n) % 3 == 1)
    wi = np.flatnonzero(np.arange(n) % 4 < 2)
    wv = (1 + wi % 9).astype(_np(tname))
    try:
        set_opts(((b"push_mode", 2),))
        A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=n, ncols=n)
        mk, om = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=n), O.OVec(n, mi, np.ones(mi.size, bool), "BOOL")
        base = np.arange(len(pattern) * 20)
        w0 = int(lens[base].sum())
        frontiers = [("one vertex", np.array([9]))]
        for target in (-1, 0, 1):
            extra = (target - w0) % PUSH_CHUNK
            fi = np.concatenate([base, 1000 + np.arange(extra)])
            assert (int(lens[fi].sum()) - target) % PUSH_CHUNK == 0
            frontiers.append((f"work = 8 k {target:+d}", fi))
        for where, fi in frontiers:
            fv = (1 + fi % 9).astype(np.int32)
            f = gb.Vector.from_coo(fi, fv, dtype="INT32", size=n)
            of = O.OVec(n, fi, fv.astype(_np(tname)), tname)
            for sr, accum in (("plus_times", "plus"), ("min_plus", "min")):
                semi = getattr(gb.semiring, sr)[tname]
                for comp in (True, False):
                    for kw, okw in ((dict(accum=getattr(gb.binary, accum)), dict(accum=accum)), (dict(replace=True), dict(replace=True))):
                        w = gb.Vector.from_coo(wi, wv, dtype=tname, size=n)
                        w(~mk.S if comp else mk.S, **kw) << f.vxm(A, semi)
                        st = device.last_stats()
                        assert st["method"] == 2 and st["long_kernel"] == 0 and st["flops"] == int(lens[fi].sum()), (where, st)
                        same_vec(w, O.vxm(of, oa, sr, w=O.OVec(n, wi, wv, tname), mask=om, mask_comp=comp, mask_struct=True, **okw),
                                 where=f"{where} {sr} comp={comp} {sorted(okw)}")
    finally:
        reset_opts()


def test_push_work_item_limit_in_a_vertex_order(gb):
    """push_thin's `in_map` / `out_map` (k_push_frontier, push_chunk): the 64 / 65 work-item pair on a matrix with a vertex order of its
    own (ORDER_OPTS), after a pulled call has left the frontier and the mask in that order -- the pushed call converts nothing
    (reorders == 0) and equals the oracle."""
    from graphblas_amd import device
    from tests.test_vertex_order import skewed_square

    tname, sr = "FP32", "min_plus"
    rng = np.random.default_rng(77)
    n = 2400
    rows, cols, vals = skewed_square(rng, n, tname)
    oa = O.OMat.from_coo(rows, cols, vals, n, n, tname)
    deg = np.bincount(rows, minlength=n)
    cand = np.flatnonzero((deg >= 1) & (deg <= PUSH_Q))
    assert cand.size >= 65
    mi = np.flatnonzero(np.arange(n) % 3 == 1)
    om = O.OVec(n, mi, np.ones(mi.size, bool), "BOOL")
    try:
        for count, lk in ((PUSH_SMALL_CHUNKS, -2), (PUSH_SMALL_CHUNKS + 1, -1)):
            set_opts(ORDER_OPTS + ((b"hot_k", 256),))
            A = gb.Matrix.from_coo(rows, cols, vals, dtype=tname, nrows=n, ncols=n)
            mk = gb.Vector.from_coo(mi, np.ones(mi.size, bool), dtype="BOOL", size=n)
            fi, fv = _frontier(cand[:count], tname)
            f, of = gb.Vector.from_coo(fi, fv, dtype=tname, size=n), O.OVec(n, fi, fv, tname)
            w = gb.Vector(tname, n)
            w(~mk.S, replace=True) << f.vxm(A, getattr(gb.semiring, sr))  # pulled: f, mk and w are in the matrix's order now
            st = device.last_stats()
            assert st["method"] == 1 and st["ordered"] == 1, st
            exp = O.vxm(of, oa, sr, mask=om, mask_comp=True, mask_struct=True, replace=True)
            set_opts(((b"push_mode", 2),))
            w2 = gb.Vector(tname, n)
            w2(~mk.S, replace=True) << f.vxm(A, getattr(gb.semiring, sr))
            st = device.last_stats()
            assert st["method"] == 2 and st["long_kernel"] == lk and st["reorders"] == 0 and st["flops"] == int(deg[fi].sum()), (count, st)
            same_vec(w2, exp, where=f"{count} work items pushed in the matrix's order, w empty")
            same_vec(w, exp, where="pulled")
            f(~mk.S, replace=True) << f.vxm(A, getattr(gb.semiring, sr))
            st = device.last_stats()
            assert st["method"] == 2 and st["long_kernel"] == lk and st["reorders"] == 0, (count, st)
            same_vec(f, O.vxm(of, oa, sr, w=of, mask=om, mask_comp=True, mask_struct=True, replace=True), where=f"{count} work items, w the frontier")
    finally:
        reset_opts()
