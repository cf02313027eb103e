"""The SpGEMM kernels at the limits of their bins, units and windows (python-graphblas_amd/csrc/grb_mxm.hip).

The random mxm suites draw rows of B of 20 .. 600 entries and class limits from a few fixed values: they reach none of the limits
below except by luck.  Here the matrices are BUILT: a row of A is the list of the rows of B it selects, a row of B the list of its
columns, so the flops and nnz of every row of the product, the entries of every (row, window) unit and group and the first product
number of every entry of a batch are known exactly.  One entry sits ON each limit and one just behind it.

Every case compares with the oracle element for element (same_mat: row pointers, columns, values).  The values are small integers
(plus_times and min_plus are exact); the columns whose rank in their unit is limit - 1, limit and limit + 1 carry values no other
column of the row sums to (_special), under plus_pair they are reached by 2, 3 and 4 products while every other column is reached by
one per repetition (Rows.marks): a misplaced rank or a dropped pass shows as a value.  Two witnesses show that the path under test
ran: the line launch_unit_classes prints under GRB_MXM_TRACE (compared with the class counts _expected_units computes from the
pattern product) -- or its absence, where the case is about the hash bins --, and method / flops / out_nvals of device.last_stats().

What the geometry rests on:
* a WINDOW is 16384 columns (MM_WIN); the units of a row walk groups of F windows, F = mxm_window_groups or, left at 0, 1 up to 64
  windows and 2 beyond; a group whose entries exceed lim[2] = mxm_unit_dense falls back to its single windows (unit_class_of);
* a row is a unit row when its products exceed sym_b3 = min(4096, max(mxm_unit_min_flops, mxm_unit_min_per_window * groups)) AND
  1024 (bin_of tests 128 and 1024 before sym_b3, so a row of up to 1024 products never is one);
* the other rows are counted by k_spgemm_hash<256 / 2048 / 32768> by flops (bin_of at 128 / 1024 / sym_b3) and computed by
  k_spgemm_hash<256 / 2048 / 8192> by nnz (128 / 1024 / 4096); s_sorted holds TABLE / 2 keys; a fused complemented mask adds its
  forbidden columns to either size;
* unit classes by entries: <= 512 one wavefront (CAP 512), <= 1024 four wavefronts (CAP 1024), <= mxm_unit_dense four wavefronts
  with CAP 4096 (single windows) or 3968 (groups), beyond that k_spgemm_unit_dense; a unit of more than CAP entries takes
  ceil(entries / CAP) passes, and stores its columns through the accumulators' LDS only up to CAP * sizeof(W) / 4 entries;
* a wavefront deals the products of a batch of 64 entries of A: the numeric one-wavefront class by search, every other unit by rank
  in segments of MU_SEG = 2048 products, 64 * MU_ILP = 256 products per trip; wavefront s of a four-wavefront unit holds the entries
  s, s + 4, ... of the row."""
import ctypes
import re

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import grb_oracle as O
from tests.backend import DEVICES, bind
from tests.values import same_mat

WIN = 16384       # (MM_WIN)
GROUP_CAP = 3968  # (accumulators of the densest compact GROUP class; single windows: 4096)
TYPES = [("INT64", "plus_times"), ("FP32", "min_plus"), ("UINT16", "plus_pair")]  # (8-byte, 4-byte and 4-byte widened accumulators)
TRACE = re.compile(r"\[mxm\] (numeric|masked) units: (\d+) rows x (\d+) windows, groups of (\d+); group classes (\d+) (\d+) (\d+), "
                   r"window classes (\d+) (\d+) (\d+), dense (\d+)")


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


def _special(sr, r):
    """The value of B on the r-th special column of a row: beyond every sum of ordinary products (plus_times), below every one
    (min_plus)."""
    return -(100 + 10 * r) if sr == "min_plus" else 10007 * (r + 1)


class Rows:
    """B by its rows' columns, A by the rows of B each of its rows selects.  Rows of B are numbered as they are made: the entries of
    a row of A lie in that order."""

    def __init__(self, n, tname, sr):
        self.n, self.tname, self.sr = n, tname, sr
        self.bcols, self.bvals, self.arows = [], [], []

    def brow(self, cols, special=()):
        cols = np.asarray(cols, np.int64)
        assert cols.size == np.unique(cols).size and (cols.size == 0 or (0 <= cols.min() and cols.max() < self.n))
        cols = np.sort(cols)
        vals = 1 + (cols * 5 + cols // 64) % 7
        for r, c in enumerate(special):
            vals[cols == c] = _special(self.sr, r)
        self.bcols.append(cols)
        self.bvals.append(vals)
        return len(self.bcols) - 1

    def deal(self, cols, nb, special=()):
        """nb new rows of B that hold `cols` round-robin (disjoint: nnz = flops)."""
        cols = np.sort(np.asarray(cols, np.int64))
        return [self.brow(cols[r::nb], special) for r in range(nb)]

    def marks(self, special):
        """Rows of B that hold special[r:], r = 0 ..: special column r is reached by r + 1 products more (plus_pair counts them)."""
        return [self.brow(np.asarray(special[r:], np.int64)) for r in range(len(special))]

    def unit(self, cols, nb, limits=(), reps=1, marks=True):
        """The rows of B for one unit (or hash row) with the columns `cols`: `reps` times nb rows that hold them round-robin
        (repeated column sets: nnz < flops); the columns of rank limit - 1, limit, limit + 1 are special."""
        cols = np.sort(np.asarray(cols, np.int64))
        special = [int(cols[r]) for lim in limits for r in (lim - 1, lim, lim + 1) if 0 <= r < cols.size]
        ids = [i for _ in range(reps) for i in self.deal(cols, nb, special)]
        if marks and self.sr == "plus_pair" and special:
            ids += self.marks(special)
        return ids

    def arow(self, ids):
        assert len(set(ids)) == len(ids)
        self.arows.append(np.sort(np.asarray(ids, np.int64)))
        return len(self.arows) - 1

    def coo(self):
        np_t = O.NP_OF[self.tname]
        br = np.concatenate([np.full(c.size, r, np.int64) for r, c in enumerate(self.bcols)])
        bc, bv = np.concatenate(self.bcols), np.concatenate(self.bvals)
        ar = np.concatenate([np.full(k.size, i, np.int64) for i, k in enumerate(self.arows)])
        ac = np.concatenate(self.arows)
        av = 1 + ac % 3
        if self.tname == "UINT16":  # (plus_pair reads no value)
            av, bv = np.ones_like(av), np.ones_like(bv)
        return (ar, ac, av.astype(np_t)), (br, bc, bv.astype(np_t)), len(self.arows), len(self.bcols)

    def pattern(self):
        """The pattern product (entry = number of products) and the flops of every row."""
        (ar, ac, _), (br, bc, _), m, k = self.coo()
        P = (sp.csr_matrix((np.ones(ar.size, np.int64), (ar, ac)), shape=(m, k)) @
             sp.csr_matrix((np.ones(br.size, np.int64), (br, bc)), shape=(k, self.n))).tocsr()
        P.sort_indices()
        blen = np.array([c.size for c in self.bcols], np.int64)
        return P, np.bincount(ar, weights=blen[ac], minlength=m).astype(np.int64)


def _spread(w, count, off=0):
    """`count` columns of window w, spread over all its bitmap words (the window's first column among them when off = 0)."""
    assert count + off <= WIN
    return w * WIN + off + (np.arange(count, dtype=np.int64) * (WIN - off)) // max(count, 1)


def _nwin(n):
    return -(-n // WIN)


def _groups_of(opts, n):
    return opts.get("mxm_window_groups", 0) or (1 if _nwin(n) <= 64 else 2)


def _class_counts(rows_window_counts, nwin, F, lim):
    """unit_class_of over the windows of the unit rows: [three group classes, three window classes, dense]."""
    cnt = [0] * 7
    for wc in rows_window_counts:
        wc = np.concatenate([wc, np.zeros(-(-nwin // F) * F - nwin, np.int64)])
        for g in range(0, nwin, F):
            grp = wc[g:g + F]
            tot = int(grp.sum())
            if F > 1 and tot <= lim[2]:
                if tot:
                    cnt[0 if tot <= lim[0] else (1 if tot <= lim[1] else 2)] += 1
            else:
                for c in grp.tolist():
                    if c:
                        cnt[3 + (0 if c <= lim[0] else (1 if c <= lim[1] else (2 if c <= lim[2] else 3)))] += 1
    return cnt


def _limits(opts, masked=False):
    l0 = min(512, opts.get("mxm_unit_small", 512))
    l1 = max(l0, opts.get("mxm_unit_mid", 1024))
    return l0, l1, (1 << 31) - 1 if masked else max(l1, opts.get("mxm_unit_dense", 4096))


def _expected_units(n, opts, T, flops, extra=None):
    """The trace line of the numeric pass of a plain (or fused) product whose pattern is T: None when no row is a unit row."""
    nwin, F = _nwin(n), _groups_of(opts, n)
    if opts.get("mxm_heavy_kernel", 1) == 0:
        return None
    # (bin_of tests 128 and 1024 before sym_b3: a row of up to 1024 products stays with the hash kernels whatever the options say)
    b3 = max(1024, min(4096, max(opts.get("mxm_unit_min_flops", 1024), opts.get("mxm_unit_min_per_window", 16) * -(-nwin // F))))
    size = flops + (extra if extra is not None else 0) * (flops > 0)
    urows = np.flatnonzero(size > b3)
    if urows.size == 0:
        return None
    wcs = [np.bincount(T.indices[T.indptr[i]:T.indptr[i + 1]] // WIN, minlength=nwin) for i in urows]
    return ("numeric", int(urows.size), nwin, F, _class_counts(wcs, nwin, F, _limits(opts)))


def _expected_masked_units(n, opts, M, flops):
    """The trace line of a mask-driven product: the units are the mask rows' windows (single windows, no dense class)."""
    nwin = _nwin(n)
    thr = max(opts.get("mxm_unit_min_flops", 1024), opts.get("mxm_unit_min_per_window", 16) * nwin)
    urows = np.flatnonzero((flops > thr) & (np.diff(M.indptr) > 0))
    wcs = [np.bincount(M.indices[M.indptr[i]:M.indptr[i + 1]] // WIN, minlength=nwin) for i in urows]
    return ("masked", int(urows.size), nwin, 1, _class_counts(wcs, nwin, 1, _limits(opts, True)))


def _traces(err):
    return [(t[0], int(t[1]), int(t[2]), int(t[3]), [int(x) for x in t[4:]]) for t in TRACE.findall(err)]


def _set(opts):
    from graphblas_amd import _lib

    for name, val in opts.items():
        assert _lib.lib.GrX_option_set(name.encode(), val) == 0, name


def _reset():
    from graphblas_amd import _lib

    assert _lib.lib.GrX_options_reset() == 0


def _product(gb, bd, opts, capfd, monkeypatch, mask=None, comp=False):
    """C = A (+.x) B, C<M.S> (mask-driven) or C<!M.S> (fused) under `opts`: checked against the oracle and against both witnesses.
    Returns (statistics, trace lines, expected product, pattern product, flops per row)."""
    from graphblas_amd import device

    (ar, ac, av), (br, bc, bv), m, k = bd.coo()
    n, tname, sr = bd.n, bd.tname, bd.sr
    P, flops = bd.pattern()
    monkeypatch.setenv("GRB_MXM_TRACE", "1")
    try:
        _set(opts)
        A = gb.Matrix.from_coo(ar, ac, av, dtype=tname, nrows=m, ncols=k)
        B = gb.Matrix.from_coo(br, bc, bv, dtype=tname, nrows=k, ncols=n)
        C = gb.Matrix(tname, m, n)
        capfd.readouterr()
        if mask is None:
            C << A.mxm(B, getattr(gb.semiring, sr))
        else:
            M = gb.Matrix.from_coo(mask[0], mask[1], np.ones(len(mask[0]), bool), dtype="BOOL", nrows=m, ncols=n)
            if comp:
                C(~M.S) << A.mxm(B, getattr(gb.semiring, sr))
            else:
                C(M.S) << A.mxm(B, getattr(gb.semiring, sr))
        st = device.last_stats()
        traces = _traces(capfd.readouterr().err)
    finally:
        _reset()
    om = None if mask is None else O.OMat.from_coo(mask[0], mask[1], np.ones(len(mask[0]), bool), m, n, "BOOL")
    exp = O.mxm(O.OMat.from_coo(ar, ac, av, m, k, tname), O.OMat.from_coo(br, bc, bv, k, n, tname), sr, mask=om, mask_comp=comp,
                mask_struct=True)
    same_mat(C, exp, where=f"{tname} {sr} {opts}")
    assert st["flops"] == int(flops.sum()) and st["out_nvals"] == exp.nvals, (st, int(flops.sum()), exp.nvals)
    Mp = None if mask is None else sp.csr_matrix((np.ones(len(mask[0]), np.int64), mask), shape=(m, n))
    if mask is None:
        assert st["method"] == 3, st
        want = _expected_units(n, opts, P, flops)
    elif comp:
        assert st["method"] == 7, st
        T = (P - P.multiply(Mp)).tocsr()
        T.eliminate_zeros()
        T.sort_indices()
        want = _expected_units(n, opts, T, flops, np.diff(Mp.tocsr().indptr))
    else:
        assert st["method"] == 4, st
        Mc = Mp.tocsr()
        Mc.sort_indices()
        want = _expected_masked_units(n, opts, Mc, flops)
    assert traces == ([] if want is None else [want]), (traces, want)
    return st, traces, exp, P, flops


POOLS = ["keep", "none", "short"]


def _pool(pool, F):
    """The bitmap pool of a case: kept (no limit), recomputed (a pool of 0: the numeric pass runs its own pass A before the passes
    over the accumulators) or short -- F - 1 slots, fewer than one group needs (`got + F <= cap` fails for every unit); with single
    windows (F = 1, where that is 0 again) two slots: the first two units that ask keep their bitmaps, every later one
    recomputes."""
    return {"keep": {}, "none": {"mxm_bitmap_pool_cap": 0}, "short": {"mxm_bitmap_pool_cap": F - 1 if F > 1 else 2}}[pool]


# ----------------------------------------------------------------------------------------------------------------------------------
# A. row bins and LDS hash tables
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tname, sr", TYPES)
def test_symbolic_bins_distinct_columns(gb, tname, sr, capfd, monkeypatch):
    """k_row_bins / bin_of by flops, k_spgemm_hash<256 / 2048 / 32768, false> and -- all columns distinct, nnz = flops -- the
    numeric tables <256 / 2048 / 8192, true> filled to exactly TABLE / 2 keys (s_sorted full) and one key more in the next table:
    rows of 128 | 129, 1024 | 1025 and 4096 | 4097 products.  mxm_unit_min_flops = 4096: the row of 4096 is the last one the 32768
    table counts, the row of 4097 the one unit row (two windows of 2049 and 2048 entries: the trace line shows one row, window
    classes 0 0 2).  The column of rank limit - 1 (and limit, where it exists) carries a value of its own."""
    n = 2 * WIN
    bd = Rows(n, tname, sr)
    sizes = [128, 129, 1024, 1025, 4096, 4097]
    for i, s in enumerate(sizes):
        cols = i + (np.arange(s, dtype=np.int64) * (n - 8)) // s
        bd.arow(bd.unit(cols, 8, limits=(sizes[i & ~1],), marks=False))
    opts = {"mxm_unit_min_flops": 4096}
    st, traces, exp, P, flops = _product(gb, bd, opts, capfd, monkeypatch)
    assert flops.tolist() == sizes and np.diff(exp.indptr).tolist() == sizes
    assert traces == [("numeric", 1, 2, 1, [0, 0, 0, 0, 0, 2, 0])], traces


@pytest.mark.parametrize("heavy", [1, 0])
@pytest.mark.parametrize("tname, sr", TYPES)
def test_numeric_bins_from_more_flops_than_nnz(gb, tname, sr, heavy, capfd, monkeypatch):
    """The numeric bins by nnz where they differ from the symbolic bins by flops: repeated column sets.  heavy = 1: nnz 128 from
    1024 flops (counted in table 2048, computed in 256), 129 from 1032 (32768 / 2048), 1024 from 4096 (32768 / 2048), 1025 from 3075
    (32768 / 8192), 4096 from 4096; no row beyond sym_b3 = 4096 flops: no unit runs, no trace line.  heavy = 0 (mxm_heavy_kernel 0:
    sym_b3 = 16384, no units at all): nnz 4096 from 8192 flops -- the last row of hash table 8192 -- against 4097 from 8194, the
    first row of the window walk k_spgemm_win, and 4097 from 20485 flops, counted by k_spgemm_sym_lds."""
    n = 2 * WIN
    bd = Rows(n, tname, sr)
    rows = [(128, 8), (129, 8), (1024, 4), (1025, 3), (4096, 1)] if heavy else [(1024, 8), (4096, 2), (4097, 2), (4097, 5)]
    for i, (nnz, reps) in enumerate(rows):
        cols = i + (np.arange(nnz, dtype=np.int64) * (n - 8)) // nnz
        lim = 128 if nnz < 200 else (1024 if nnz < 2000 else 4096)
        bd.arow(bd.unit(cols, 4, limits=(lim,), reps=reps, marks=False))
    opts = {"mxm_unit_min_flops": 4096} if heavy else {"mxm_heavy_kernel": 0}
    st, traces, exp, P, flops = _product(gb, bd, opts, capfd, monkeypatch)
    assert np.diff(exp.indptr).tolist() == [r[0] for r in rows] and flops.tolist() == [r[0] * r[1] for r in rows]
    assert traces == []


def _hash_col(c, table):
    return ((np.asarray(c, np.int64) * 2654435761) & 0xFFFFFFFF) & (table - 1)  # (hash_col)


@pytest.mark.parametrize("tname, sr", TYPES)
def test_hash_probe_chains_wrap_the_table_end(gb, tname, sr, capfd, monkeypatch):
    """Linear probing of k_spgemm_hash (`h = (h + 1) & (TABLE - 1)`): for each numeric table 256 / 2048 / 8192 one row with 40
    columns whose hash is one of the table's LAST four slots -- the chain runs over the end into the first slots -- and one row with
    12 columns of ONE slot; the rows are filled with ordinary columns up to the bin of their table (100, 340 and 1540 | 72, 312 and
    1512 entries).  The rows of the 8192 bin are counted in the symbolic table 32768: they also hold the 16 columns of its last four
    slots.  All columns distinct; the last three columns of every chain carry values of their own."""
    n = 8 * WIN
    allc = np.arange(n, dtype=np.int64)
    bd = Rows(n, tname, sr)
    want = []
    last32k = allc[_hash_col(allc, 32768) >= 32768 - 4]
    assert last32k.size == 16
    for table, fill in ((256, 60), (2048, 300), (8192, 1500)):
        h = _hash_col(allc, table)
        for chain in (allc[h >= table - 4][:40], allc[h == 5][:12]):
            assert chain.size in (40, 12)
            if table == 8192:
                chain = np.union1d(chain, last32k)
            rest = np.setdiff1d(7 + (np.arange(fill + 60, dtype=np.int64) * (n - 8)) // (fill + 60), chain)[:fill]
            cols = np.union1d(chain, rest)
            special = [int(c) for c in chain[-3:]]
            bd.arow(bd.deal(cols, 4, special))
            want.append(cols.size)
            assert (cols.size <= 128) == (table == 256) and (cols.size <= 1024) == (table <= 2048) and cols.size <= 4096
    st, traces, exp, P, flops = _product(gb, bd, {"mxm_unit_min_flops": 4096}, capfd, monkeypatch)
    assert np.diff(exp.indptr).tolist() == want and traces == []


@pytest.mark.parametrize("tname, sr", TYPES)
def test_fused_complemented_mask_adds_forbidden_columns_to_the_bin(gb, tname, sr, capfd, monkeypatch):
    """C<!M.S>, fused (method 7): k_row_bins adds the row's forbidden columns to its size (extra_ptr), because they take slots of
    the hash table beside the row's own.  Three rows of 100 products on distinct columns with 28, 29 and 30 forbidden columns, ONE
    of which is also produced (it must not appear: 99 entries): symbolic sizes 128 | 129 | 130 (table 256, then 2048), numeric sizes
    127 | 128 | 129 (table 256 with exactly 128 keys, then 2048).  No unit row: no trace line."""
    n = WIN
    bd = Rows(n, tname, sr)
    mr, mc = [], []
    for i, forb in enumerate((28, 29, 30)):
        own = _spread(0, 100, off=i)
        bd.arow(bd.unit(own, 4, limits=(99,), marks=False))
        cols = np.concatenate([[own[50]], own[:forb - 1] + 3])
        assert np.intersect1d(cols, own).size == 1
        mr.append(np.full(forb, i))
        mc.append(np.sort(cols))
    mask = (np.concatenate(mr), np.concatenate(mc))
    st, traces, exp, P, flops = _product(gb, bd, {}, capfd, monkeypatch, mask=mask, comp=True)
    assert flops.tolist() == [100] * 3 and np.diff(exp.indptr).tolist() == [99] * 3 and traces == []


@pytest.mark.parametrize("tname, sr", TYPES)
def test_foreach_product_blocks_of_256_entries(gb, tname, sr, capfd, monkeypatch):
    """foreach_product takes the entries of a row of A BLOCK = 256 at a time: rows of A with 256 and 257 entries whose flops stay in
    the hash bins.  Row 0: 256 single-entry rows of B (one full block).  Row 1: 257 entries -- 255 EMPTY rows of B, then one of 100
    entries (every product of the first block comes from the block's last entry), then a single entry alone in the second block. Row
    2: 257 single entries.  Row 3: 256 entries, the FIRST brings 100 products, the others none."""
    n = WIN
    bd = Rows(n, tname, sr)
    bd.arow([bd.brow([37 * e % n]) for e in range(256)])
    hundred = _spread(0, 100, off=11)
    bd.arow([bd.brow([]) for _ in range(255)] + [bd.brow(hundred, special=[int(hundred[-1])]), bd.brow([5])])
    bd.arow([bd.brow([(41 * e + 3) % n]) for e in range(257)])
    bd.arow([bd.brow(hundred + 1, special=[int(hundred[0]) + 1])] + [bd.brow([]) for _ in range(255)])
    st, traces, exp, P, flops = _product(gb, bd, {}, capfd, monkeypatch)
    assert flops.tolist() == [256, 101, 257, 100] and np.diff(exp.indptr).tolist() == [256, 101, 257, 100] and traces == []
    assert [a.size for a in bd.arows] == [256, 257, 257, 256]


# ----------------------------------------------------------------------------------------------------------------------------------
# B. unit classes and accumulator passes
# ----------------------------------------------------------------------------------------------------------------------------------
def _window_units_problem(tname, sr):
    """Rows 0 / 1 / 2: window 0 holds 512 / 1024 / 4096 entries, window 1 holds 513 / 1025 / 4097 (every set twice: nnz < flops)."""
    bd = Rows(2 * WIN, tname, sr)
    for i, lim in enumerate((512, 1024, 4096)):
        bd.arow(bd.unit(_spread(0, lim, off=i), 4, limits=(lim,), reps=2) +
                bd.unit(_spread(1, lim + 1, off=i), 4, limits=(lim,), reps=2))
    return bd


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("tname, sr", TYPES)
def test_single_window_units_at_the_class_limits(gb, tname, sr, pool, capfd, monkeypatch):
    """unit_class_of / k_spgemm_unit<.., 1, 512> | <.., 4, 1024> | <.., 4, 4096> / k_spgemm_unit_dense with mxm_window_groups = 1:
    units of 512 | 513, 1024 | 1025 and 4096 | 4097 entries -- window classes 1 2 2, dense 1.  The unit of 512 entries fills the
    one-wavefront class's accumulators, 4096 the last compact class's in ONE pass; 4097 is the first dense unit.  Bitmaps (_pool):
    kept, recomputed, and a pool of two slots that runs out.  With the pool kept the symbolic unit keeps a bitmap from
    mxm_bitmap_min_cnt + 1 = 513 entries on (`cnt > bm_min_cnt`): the unit of 512 entries recomputes, the one of 513 does not.  THIS
    limit has no witness: kept or recomputed, the product is the same, and neither the trace line nor the statistics tell which
    happened -- the case pins only that both sides of it compute the right values."""
    bd = _window_units_problem(tname, sr)
    opts = dict({"mxm_window_groups": 1}, **_pool(pool, 1))
    st, traces, exp, P, flops = _product(gb, bd, opts, capfd, monkeypatch)
    assert traces == [("numeric", 3, 2, 1, [0, 0, 0, 1, 2, 2, 1])], traces


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("tname, sr", TYPES)
def test_single_window_units_of_several_passes(gb, tname, sr, pool, capfd, monkeypatch):
    """The pass loop of k_spgemm_unit<.., 4, 4096, 1> (`for (r0 = 0; r0 < cnt; r0 += CAP)`), reached with mxm_unit_dense = 16384:
    compact units of 4097 (two passes, the second for ONE rank), 8192 (two full passes), 8193 (three) and 16384 entries (four: every
    column of the window).  The staged column store ends at CAP * sizeof(W) / 4 entries: 4096 | 4097 for the 4-byte accumulators,
    8192 | 8193 for INT64.  The columns of rank 4095 .. 4097, 8191 .. 8193 and 12287 .. 12289 carry values of their own.  Bitmaps
    (_pool) kept, recomputed -- the numeric unit then runs pass A itself, and the batches it pre-fetched there serve every pass over
    the accumulators -- and a pool of two slots for the four units."""
    bd = Rows(WIN, tname, sr)
    sizes = [4097, 8192, 8193, 16384]
    for i, s in enumerate(sizes):
        bd.arow(bd.unit(_spread(0, s, off=min(i, WIN - s)), 8, limits=(4096, 8192, 12288)))
    opts = dict({"mxm_window_groups": 1, "mxm_unit_dense": 16384}, **_pool(pool, 1))
    st, traces, exp, P, flops = _product(gb, bd, opts, capfd, monkeypatch)
    assert np.diff(exp.indptr).tolist() == sizes
    assert traces == [("numeric", 4, 1, 1, [0, 0, 0, 0, 0, 4, 0])], traces


def _group_cols(g, F, tot, where="even"):
    """`tot` columns of group g of F windows: spread evenly over its windows, or all in its first / last window."""
    if where != "even":
        return _spread(g * F + (0 if where == "first" else F - 1), tot, off=3)
    per = [tot // F + (1 if f < tot % F else 0) for f in range(F)]
    return np.concatenate([_spread(g * F + f, c, off=f) for f, c in enumerate(per)])


def _group_units_problem(F, tname, sr, pairs=((512, 513), (1024, 1025), (GROUP_CAP, GROUP_CAP + 1), (4096, 4097))):
    """2 F + 1 windows (n is no multiple of 16384): every row holds group 0, group 1 and the SHORT last group (one window, with the
    column n - 1).  Rows 0 .. 3: the groups' totals are the pairs on a limit; the last row: a group with all its entries in its
    first window and one with all of them in its last."""
    n = (2 * F + 1) * WIN - 5
    bd = Rows(n, tname, sr)
    for i, (a, b) in enumerate(pairs):
        lims = (a,) if a != 4096 else (GROUP_CAP, 4096)
        tail = np.array([2 * F * WIN + 7 + i, n - 40 + i, n - 1])
        bd.arow(bd.unit(_group_cols(0, F, a), 4, limits=lims, reps=2) + bd.unit(_group_cols(1, F, b), 4, limits=lims, reps=2) +
                bd.unit(tail, 2, limits=(2,), reps=2))
    bd.arow(bd.unit(_group_cols(0, F, 700, "first"), 4, limits=(512,), reps=2) +
            bd.unit(_group_cols(1, F, 700, "last"), 4, limits=(512,), reps=2) +
            bd.unit(np.array([n - 3, n - 1]), 2, reps=2))
    return bd


@pytest.mark.parametrize("pool", POOLS)
@pytest.mark.parametrize("F", [2, 4, 8])
@pytest.mark.parametrize("tname, sr", TYPES)
def test_group_units_at_the_class_limits(gb, tname, sr, F, pool, capfd, monkeypatch):
    """Groups of F = 2 / 4 / 8 windows (k_spgemm_unit<.., F>, unit_class_of): group totals of 512 | 513, 1024 | 1025, 3968 | 3969
    and 4096 | 4097 entries.  The densest group class has CAP = 3968 accumulators but takes groups of up to lim[2] = 4096 entries:
    3969 .. 4096 entries are a SECOND pass, and the 4-byte accumulators leave the staged column store there (INT64: staged up to
    7936). The group of 4097 entries falls back to its single windows.  A group whose entries all lie in its first window, one with
    all in its last; every row's last group is short (`fspan` = 1 < F: window 2 F alone) and holds the column n - 1.  Bitmaps
    (_pool) kept, recomputed and with a pool of F - 1 slots."""
    bd = _group_units_problem(F, tname, sr)
    opts = dict({"mxm_window_groups": F}, **_pool(pool, F))
    st, traces, exp, P, flops = _product(gb, bd, opts, capfd, monkeypatch)
    (kind, nrows, nwin, f, cnt), = traces
    assert (nrows, nwin, f) == (5, 2 * F + 1, F)
    # group classes: <= 512: the five short last groups and the group of 512; <= 1024: 513, 1024 and the two of 700; <= 4096: 1025,
    # 3968, 3969, 4096; the group of 4097 as F single windows
    assert cnt[:3] == [6, 4, 4] and sum(cnt[3:]) == F and cnt[6] == 0, cnt


@pytest.mark.parametrize("pool", POOLS)
def test_default_group_choice_beyond_64_windows(gb, pool, capfd, monkeypatch):
    """mxm_window_groups left at 0 with 66 windows: groups of TWO windows are what ships (spgemm: `n_win <= 64 ? 1 : 2`).  Row 0: a
    group of 3969 entries (second pass of the CAP = 3968 class), one of 600 and the last group with 100 entries up to column n - 1;
    row 1: a group of 5000 entries, which falls back to two windows of 2500.  Trace: groups of 2; group classes 1 1 1, window
    classes 0 0 2, dense 0.  Bitmaps (_pool) kept, recomputed (the group of 3969 entries runs pass A and both passes over the
    accumulators in the numeric unit) and a pool of one slot, fewer than a pair needs."""
    n = 66 * WIN - 3
    bd = Rows(n, "INT64", "plus_times")
    last = np.concatenate([_spread(65, 99, off=5)[:99] - 10, [n - 1]])
    bd.arow(bd.unit(_group_cols(0, 2, GROUP_CAP + 1), 4, limits=(GROUP_CAP,)) + bd.unit(_group_cols(5, 2, 600), 4, limits=(512,)) +
            bd.unit(np.unique(last), 2))
    bd.arow(bd.unit(_group_cols(3, 2, 5000), 4, limits=(2500,)))
    st, traces, exp, P, flops = _product(gb, bd, _pool(pool, 2), capfd, monkeypatch)
    assert traces == [("numeric", 2, 66, 2, [1, 1, 1, 0, 0, 2, 0])], traces


@pytest.mark.parametrize("case", ["group_3969", "window_8193"])
def test_streamed_checksum_through_the_second_pass(gb, case, capfd, monkeypatch):
    """GrX_mxm_streamed: csum_mine of k_spgemm_unit is added to in EVERY pass over the accumulators.  The group of 3969 entries (F =
    2, CAP = 3968: the second pass stores one value) and the single window of 8193 entries (mxm_unit_dense = 16384, CAP = 4096:
    three passes); count and checksum against the oracle's product, folded into the stores (mxm_checksum_pass 0) and by the pass of
    its own (1)."""
    from graphblas_amd import _lib, device

    if case == "group_3969":
        bd = _group_units_problem(2, "INT64", "plus_times", pairs=((GROUP_CAP, GROUP_CAP + 1),))
        opts = {"mxm_window_groups": 2}
    else:
        bd = Rows(WIN, "INT64", "plus_times")
        bd.arow(bd.unit(_spread(0, 8193), 8, limits=(4096, 8192)))
        opts = {"mxm_window_groups": 1, "mxm_unit_dense": 16384}
    (ar, ac, av), (br, bc, bv), m, k = bd.coo()
    P, flops = bd.pattern()
    exp = O.mxm(O.OMat.from_coo(ar, ac, av, m, k, "INT64"), O.OMat.from_coo(br, bc, bv, k, bd.n, "INT64"), "plus_times")
    want = _expected_units(bd.n, opts, P, flops)
    assert want[4][2 if case == "group_3969" else 5] >= 1
    monkeypatch.setenv("GRB_MXM_TRACE", "1")
    try:
        A = gb.Matrix.from_coo(ar, ac, av, dtype="INT64", nrows=m, ncols=k)
        B = gb.Matrix.from_coo(br, bc, bv, dtype="INT64", nrows=k, ncols=bd.n)
        for sum_pass in (0, 1):
            _set(dict(opts, mxm_checksum_pass=sum_pass))
            capfd.readouterr()
            nv, cs, fl, nb = (ctypes.c_uint64(0) for _ in range(4))
            assert _lib.lib.GrX_mxm_streamed(gb.semiring.plus_times["INT64"]._carg, A._carg, B._carg, 1 << 30, ctypes.byref(nv),
                                             ctypes.byref(cs),
                                             ctypes.byref(fl), ctypes.byref(nb)) == 0
            st = device.last_stats()
            assert _traces(capfd.readouterr().err) == [want]
            assert (nv.value, fl.value, nb.value) == (exp.nvals, int(flops.sum()), 1)
            assert cs.value == int(exp.values.sum()) & 0xFFFFFFFFFFFFFFFF, (sum_pass, cs.value, int(exp.values.sum()))
            assert st["flops"] == int(flops.sum()) and st["out_nvals"] == exp.nvals, st
    finally:
        _reset()


@pytest.mark.parametrize("tname, sr", TYPES)
def test_mask_driven_units_at_the_class_limits(gb, tname, sr, capfd, monkeypatch):
    """k_spgemm_unit<.., MU_MASKED, ..> (mxm_mask_mode = 2, mxm_masked_units_min_flops = 0): the unit's bitmap is the MASK row's
    part of the window, the accumulators are keyed by the mask entry.  Mask rows with 512 | 513, 1024 | 1025 and 4096 | 4097 entries
    in window 0 (4097: a second pass of the CAP = 4096 class), each with the column 16383, and the column 16384 with four more
    entries in window 1. B holds every column of window 0 except a few HOLES, which are mask entries no product reaches: they must
    stay absent."""
    n = 2 * WIN + 10
    sizes = [512, 513, 1024, 1025, 4096, 4097]
    mr, mc, holes, special = [], [], [], []
    for i, t in enumerate(sizes):
        cols = np.unique(np.concatenate([(np.arange(t - 1, dtype=np.int64) * (WIN - 2 - i)) // (t - 1) + i, [WIN - 1]]))
        assert cols.size == t
        lim = sizes[i & ~1]
        special += [int(cols[r]) for r in (lim - 1, lim, lim + 1) if r < t]
        holes += [int(cols[r]) for r in (3, 100, t - 10)]
        w1 = np.array([WIN, WIN + 2 + i, WIN + 9, 2 * WIN + 1, n - 1])
        mr.append(np.full(t + w1.size, i))
        mc.append(np.concatenate([cols, w1]))
    holes = np.setdiff1d(np.unique(holes), special + [WIN - 1])
    bd = Rows(n, tname, sr)
    reach = np.setdiff1d(np.concatenate([np.arange(WIN), [WIN, WIN + 9, n - 1]]), holes)
    ids = bd.deal(reach, 40, special[:12])
    for _ in sizes:
        bd.arow(ids)
    opts = {"mxm_mask_mode": 2, "mxm_masked_units_min_flops": 0}
    st, traces, exp, P, flops = _product(gb, bd, opts, capfd, monkeypatch, mask=(np.concatenate(mr), np.concatenate(mc)))
    # (window 0: 512 | 513 1024 | 1025 4096 4097; windows 1 and 2: three and two entries in each of the six rows)
    assert traces == [("masked", 6, 3, 1, [0, 0, 0, 13, 2, 3, 0])], traces
    got = set(exp.indices.tolist())
    assert WIN - 1 in got and WIN in got and not (got & set(holes.tolist())) and WIN + 2 not in got


# ----------------------------------------------------------------------------------------------------------------------------------
# C. product dealing (visit / process of k_spgemm_unit)
# ----------------------------------------------------------------------------------------------------------------------------------
DEAL = {"mxm_window_groups": 1}


@pytest.mark.parametrize("symw", [1, 8])
@pytest.mark.parametrize("tname, sr", TYPES)
def test_row_lengths_of_a_at_the_batch_limits(gb, tname, sr, symw, capfd, monkeypatch):
    """Rows of A with 64 | 65, 128 | 129 (MU_SYM_PLEN: up to 128 entries a symbolic unit walks mxm_sym_windows windows, longer rows
    come from the list launch; and the NB = 2 pre-fetched batches of a one-wavefront unit), 256 | 257 and 512 | 513 entries (the two
    pre-fetched batches of a four-wavefront unit: 64 * 4 * 2).  Row r of B holds 2 columns of window 0 and 15 of window 1, so a row
    of L entries has units of 2 L and 15 L entries (more than 1024 products: a unit row): one-wavefront and four-wavefront units of
    every compact class, the densest with up to two passes (mxm_unit_dense = 16384)."""
    n, lens = 2 * WIN, [64, 65, 128, 129, 256, 257, 512, 513]
    bd = Rows(n, tname, sr)
    ends = (63, 64, 127, 128, 255, 256, 511, 512)  # (the last entry of every row of A, and the one before it: a value of its own)
    ids = [bd.brow(np.concatenate([2 * r + np.arange(2), WIN + 15 * r + np.arange(15)]), special=[2 * r + 1] if r in ends else ())
           for r in range(513)]
    for L in lens:
        bd.arow(ids[:L])
    st, traces, exp, P, flops = _product(gb, bd, dict(DEAL, mxm_sym_windows=symw, mxm_unit_dense=16384), capfd, monkeypatch)
    assert np.diff(exp.indptr).tolist() == [17 * L for L in lens]
    # 2 L: 128 130 256 258 512 | 514 1024 | 1026;  15 L: 960 975 | 1920 1935 3840 3855 7680 7695
    assert traces == [("numeric", 8, 2, 1, [0, 0, 0, 5, 4, 7, 0])], traces


@pytest.mark.parametrize("pos", [0, 130, 255])
@pytest.mark.parametrize("tname, sr", TYPES)
def test_a_long_row_of_b_spans_whole_segments(gb, tname, sr, pos, capfd, monkeypatch):
    """A row of B with 5000 entries inside one window: more than two segments of MU_SEG = 2048 products, so the rank dealing of
    `process` meets a segment in which NO entry starts (recm empty, every rank from recb = before - 1).  The row of A has 256
    entries (a third of them with an empty range in window 0, the others with one or two columns); the long row is its first, a
    middle or its last non-empty entry -- lane 0 of wavefront 0, lane 32 of wavefront 2, lane 63 of wavefront 3 of a four-wavefront
    unit.  Plain with mxm_unit_dense = 16384: the symbolic unit (one wavefront, rank dealing) and the numeric CAP = 4096 unit (four
    wavefronts, rank dealing, two passes).  Mask-driven: a mask row of 300 entries (one wavefront: SEARCH dealing) and one of 700
    (four wavefronts)."""
    n = 2 * WIN
    bd = Rows(n, tname, sr)
    longc = np.arange(5000, dtype=np.int64)
    ids = []
    for e in range(256):
        if e == pos:
            ids.append(bd.brow(longc, special=[2047, 2048, 2049, 4095, 4096, 4097, 4999]))
        else:
            ids.append(bd.brow(([] if e % 3 == 0 else [5000 + 2 * e] + ([5001 + 2 * e] if e % 3 == 2 else [])) + [WIN + e]))
    bd.arow(ids)
    bd.arow(ids)
    opts = dict(DEAL, mxm_unit_dense=16384)
    st, traces, exp, P, flops = _product(gb, bd, opts, capfd, monkeypatch)
    (kind, nrows, nwin, f, cnt), = traces
    assert cnt == [0, 0, 0, 2, 0, 2, 0], cnt  # (window 0: 5000 + 255 entries, window 1: 255)
    # (5002, 5003 and 5101 belong to the entries 1 and 50 of the row: produced unless the long row took their place)
    on = np.array([0, 2047, 2048, 4096, 4999, 5002, 5003, 5101])
    m0 = np.union1d(on, np.setdiff1d(np.arange(400, dtype=np.int64) * 41 + 1, on)[:292])
    m1 = np.union1d(on, np.setdiff1d(np.arange(700, dtype=np.int64) * 23 + 1, on)[:692])
    assert m0.size == 300 and m1.size == 700
    mask = (np.concatenate([np.zeros(300, np.int64), np.ones(700, np.int64)]), np.concatenate([m0, m1]))
    opts = dict(opts, mxm_mask_mode=2, mxm_masked_units_min_flops=0)
    st, traces, exp, P, flops = _product(gb, bd, opts, capfd, monkeypatch, mask=mask)
    assert traces == [("masked", 2, 2, 1, [0, 0, 0, 1, 1, 0, 0])], traces


@pytest.mark.parametrize("tname, sr", TYPES)
def test_entries_that_start_on_a_segment_boundary(gb, tname, sr, capfd, monkeypatch):
    """`rel >= 0 && rel < MU_SEG` in `process`: entries of a batch whose first product number is exactly 2047 (the last bit of a
    segment's recm), 2048 (the first of the next) and 2049.  Row X, for one wavefront over 64 consecutive entries (the symbolic
    unit): ranges of 2047, 1, 1, 5, ... products.  Row Y, for a four-wavefront unit (wavefront s holds the entries s, s + 4, ...):
    wavefront 0 sees 2047, 1, 1, 5, wavefront 1 2048, 1, 1, 5, wavefront 2 2049, 1, 1, wavefront 3 2046, 1, 1, 1 -- and, walked by
    consecutive entries in the symbolic pass, starts of 2047, 4095 and 6144.  The long ranges share the columns 0 .. 2048 (nnz <
    flops: a compact four-wavefront unit); the columns 2046 .. 2048 carry values of their own."""
    n = WIN
    bd = Rows(n, tname, sr)
    nxt = [3000]

    def fresh(c):
        nxt[0] += c
        return np.arange(nxt[0] - c, nxt[0], dtype=np.int64)

    sp_ = [2046, 2047, 2048]
    bd.arow([bd.brow(np.arange(2047), special=sp_)] + [bd.brow(fresh(c)) for c in [1, 1, 5] + [(e % 3) for e in range(60)]])
    first = {0: [2047, 1, 1, 5], 1: [2048, 1, 1, 5], 2: [2049, 1, 1], 3: [2046, 1, 1, 1]}
    ids = []
    for p in range(64):
        s, lane = p % 4, p // 4
        c = first[s][lane] if lane < len(first[s]) else 1
        ids.append(bd.brow(np.arange(c) if c > 1000 else fresh(c), special=sp_))
    bd.arow(ids)
    st, traces, exp, P, flops = _product(gb, bd, DEAL, capfd, monkeypatch)
    assert np.diff(exp.indptr).tolist() == [2047 + 7 + 60, 2049 + 68] and flops.tolist() == [2114, 2047 + 2048 + 2049 + 2046 + 68]
    assert traces == [("numeric", 2, 1, 1, [0, 0, 0, 0, 0, 2, 0])], traces


@pytest.mark.parametrize("tname, sr", TYPES)
def test_batch_totals_at_trip_and_segment_limits(gb, tname, sr, capfd, monkeypatch):
    """The products of a batch: 255 | 256 | 257 (one trip of 64 * MU_ILP = 256 products, and one product more) and 2048 | 2049 (one
    segment, and one product more).  Rows 0 .. 4: 63 entries of A whose ranges in window 0 add up to exactly that (one wavefront:
    the symbolic unit by rank, the numeric one-wavefront unit of the first three by search); 17 columns per entry in window 1 make
    every row a unit row (more than 1024 products).  Rows 5 | 6: 64 entries dealt to the four wavefronts of a CAP = 4096 unit with
    255, 256, 257, 2048 | 2049, 2047, 256, 1 products per wavefront (rank dealing: a segment and one product more in wavefront 0 of
    row 6).  Row 6 has 4353 entries in window 0: mxm_unit_dense = 16384 keeps it a compact unit of two passes -- at the default 4096
    it would be a dense unit, which deals its products another way (deal_products_2) and never sees these batches."""
    n = 2 * WIN
    bd = Rows(n, tname, sr)
    totals = [255, 256, 257, 2048, 2049]
    for i, t in enumerate(totals):
        cols = _spread(0, t, off=i)
        lens = [t // 63 + (1 if e < t % 63 else 0) for e in range(63)]
        cut = np.concatenate([[0], np.cumsum(lens)])
        bd.arow([bd.brow(np.concatenate([cols[cut[e]:cut[e + 1]], WIN + 17 * e + np.arange(17)]), special=[int(cols[-1])])
                 for e in range(63)])
    for per_wave in ([255, 256, 257, 2048], [2049, 2047, 256, 1]):
        cols, at, ids = _spread(0, sum(per_wave), off=9), 0, [None] * 64
        for s, t in enumerate(per_wave):
            for lane in range(16):
                c = t // 16 + (1 if lane < t % 16 else 0)
                ids[4 * lane + s] = bd.brow(cols[at:at + c], special=[int(cols[at + c - 1])] if c and lane == 15 else ())
                at += c
        bd.arow(ids)
    st, traces, exp, P, flops = _product(gb, bd, dict(DEAL, mxm_unit_dense=16384), capfd, monkeypatch)
    assert flops.tolist() == [t + 1071 for t in totals] + [2816, 4353] and np.diff(exp.indptr).tolist() == flops.tolist()
    # (window 0: 255 256 257 | 2048 2049 2816 4353; window 1: five times 1071 -- no dense unit)
    assert traces == [("numeric", 7, 2, 1, [0, 0, 0, 3, 0, 9, 0])], traces


@pytest.mark.parametrize("tname, sr", TYPES)
def test_a_batch_with_one_non_empty_range(gb, tname, sr, capfd, monkeypatch):
    """A batch in which only ONE of the 64 entries of A has a range inside the window (the first, the 38th or the last): the other
    63 rows of B lie in window 1 only (14 columns each: more than 1024 products, a unit row).  With 200 columns a one-wavefront unit
    (search dealing: scan[] of 63 equal numbers), with 600 a four-wavefront unit (rank dealing: one bit in recm, the other
    wavefronts' batches empty)."""
    n = 2 * WIN
    bd = Rows(n, tname, sr)
    for count in (200, 600):
        for pos in (0, 37, 63):
            cols = _spread(0, count, off=pos)
            in_w1 = lambda e: WIN + 14 * e + np.arange(14)
            bd.arow([bd.brow(np.concatenate([cols if e == pos else [], in_w1(e)]).astype(np.int64), special=[int(cols[-1])])
                     for e in range(64)])
    st, traces, exp, P, flops = _product(gb, bd, DEAL, capfd, monkeypatch)
    assert np.diff(exp.indptr).tolist() == [200 + 896] * 3 + [600 + 896] * 3
    assert traces == [("numeric", 6, 2, 1, [0, 0, 0, 3, 9, 0, 0])], traces


# ----------------------------------------------------------------------------------------------------------------------------------
# D. windows
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [WIN, WIN + 1, 2 * WIN])
@pytest.mark.parametrize("tname, sr", TYPES)
def test_window_geometry_at_multiples_of_16384(gb, tname, sr, n, capfd, monkeypatch):
    """n_win = ceil(n / 16384) and the window of a column (k_window_offsets_hist: `Bj / MM_WIN`): n = 16384 is ONE window whose last
    column 16383 is produced; n = 16385 has a second window of one column, 16384; n = 32768 two full windows with 16383, 16384 and n
    - 1 produced.  1500 entries in window 0; the columns 16382 .. 16384 carry values of their own."""
    bd = Rows(n, tname, sr)
    cols = np.unique(np.concatenate([_spread(0, 1497), [WIN - 3, WIN - 2, WIN - 1]]))
    assert cols.size == 1500
    more = [] if n == WIN else ([WIN] if n == WIN + 1 else np.unique(np.concatenate([[WIN, n - 1], _spread(1, 798, off=1)])))
    cols = np.concatenate([cols, more]).astype(np.int64)
    bd.arow(bd.deal(cols, 6, special=[WIN - 2, WIN - 1, WIN]))
    st, traces, exp, P, flops = _product(gb, bd, {}, capfd, monkeypatch)
    want = {WIN: [0, 0, 0, 0, 0, 1, 0], WIN + 1: [0, 0, 0, 1, 0, 1, 0], 2 * WIN: [0, 0, 0, 0, 1, 1, 0]}[n]
    assert traces == [("numeric", 1, _nwin(n), 1, want)], traces
    assert exp.indices[-1] == n - 1


@pytest.mark.parametrize("nwin", [2047, 2048])
def test_window_offsets_histogram_to_search_switch(gb, nwin, capfd, monkeypatch):
    """launch_window_offsets: up to WO_MAX_WIN = 2047 windows k_window_offsets_hist (an LDS histogram of 2048 numbers per wavefront,
    its last one the entry n_win), beyond that k_window_offsets_wave (a binary search per window).  Two rows of A over 40 rows of B
    with 30-odd entries each: ten in the windows 0 and 1 (with the columns 16383 and 16384), ten in the last two windows (with n -
    1), ten in ten windows in between; default groups (pairs); mxm_unit_min_per_window = 1 makes rows of more than 1024 products
    unit rows. Plain, and under a structural mask, mask-driven (the MASK rows' offsets come from the same launcher, classified on
    the way)."""
    n = nwin * WIN - 3
    bd = Rows(n, "INT64", "plus_times")
    ids = []
    for r in range(40):
        cols = np.concatenate([WIN - 40 + 7 * np.arange(10) + r % 7, n - 2 * WIN + 1600 * np.arange(10) + 31 * r,
                               (200 * np.arange(1, 11) + 7) * WIN + 401 * r])
        extra = {0: [n - 1], 1: [WIN - 1, WIN], 2: [n - WIN + 5]}.get(r, [])
        ids.append(bd.brow(np.unique(np.concatenate([cols, extra]).astype(np.int64)), special=[WIN - 1, WIN, n - 1]))
    bd.arow(ids)
    bd.arow(ids[1:38])
    opts = {"mxm_unit_min_per_window": 1}
    st, traces, exp, P, flops = _product(gb, bd, opts, capfd, monkeypatch)
    # (the exact class line is asserted in _product; here: both rows are unit rows of nwin windows, every unit a pair of windows.
    #  The trace does not tell the histogram from the search kernel: the witness of the switch is n_win itself, with the values)
    assert traces[0][1:4] == (2, nwin, 2) and sum(traces[0][4][3:]) == 0, traces
    assert {WIN - 1, WIN, n - 1} <= set(exp.indices.tolist())
    # the mask: every second entry of the product, and entries no product reaches (among them window 0 and the last window)
    er, ec, _ = exp.to_coo()
    mr = np.concatenate([er[::2], [0, 0, 1, 1]])
    mc = np.concatenate([ec[::2], [3, n - 2, WIN + 1, n - 2]])
    key = np.unique(mr * n + mc)
    opts = {"mxm_mask_mode": 2, "mxm_masked_units_min_flops": 0, "mxm_unit_min_per_window": 0}
    st, traces, exp, P, flops = _product(gb, bd, opts, capfd, monkeypatch, mask=(key // n, key % n))
    assert traces[0][:4] == ("masked", 2, nwin, 1) and sum(traces[0][4][4:]) == 0, traces
