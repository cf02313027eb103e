"""The matrix write rule C<M, replace> = accum(C, T) at the limits of its chunks, column pieces and searches.

Every masked or accumulated matrix result ends in matrix_apply_write_rule (grb_mxm.hip), by default in k_mat_write_wave
(grb_mxm_write.inc).  Its geometry:
* a UNIT is a row, or -- for a row with more than WR_LONG = 8192 entries in C_old and T together -- a (row, column piece) pair; a matrix
  has pieces = min(WR_MAX_PIECES = 256, ceil(ncols / 16384)) pieces of piece_cols = ceil(ncols / pieces) columns, so nothing is cut
  below 16385 columns; a piece's part of each list is found with wave_lower_bound, a 64-ary search that needs one round for lists of
  up to 4160 entries (the range left after a round is ceil(n / 64) - 1 long, and the loop ends at 64), two up to 266 304, three beyond;
* the three lists are merged 64 entries at a time under a BOUND, the smallest last-loaded column over the lists that still have
  unloaded entries (`e - p > 64`); an entry finds its partner by a 6-step search of the other chunk in LDS; a false mask entry is kept
  in place as -1 - column; an output position is two popcounts of ballots;
* four units share a workgroup; a count pass, a scan and a fill pass run the same walk; k_write_units_per_row / k_write_rowptr take
  256 rows per workgroup.
The random suite draws its rows; the rows here are built from explicit sorted column lists, so every limit is hit by construction, with
one entry on the limit and one just behind it.

How a case runs: T is given exactly -- ``C(mask, accum, replace) << T`` with T a plain matrix of C's type is GrB_transpose's copy
branch straight into the write rule -- under mat_write_kernel 1 (the wavefront kernel) and 0 (the thread-per-row k_mat_write), each
compared with the expectation, never with the other.  The expectation is `_expect`: the rule restated in numpy on the linearised keys
row * ncols + col (isin / union1d / intersect1d and the accumulator's ufunc on sparse arrays: one case has 5 M columns); it shares
nothing with the library or the oracle.  Up to ORACLE_MAX_COLS columns the restatement must first agree with the oracle's
``mxm(identity, T, "any_second", C=..., mask=...)``.  Row pointers, columns and values are compared exactly; no case has a tolerance.
Values: C_old in [1, 1000), T in [1000, 2 10^6), so C, T and plus(C, T) differ pairwise at every position and a misplaced entry or a
swapped source shows as a value (the 8- and 16-bit types get narrower ranges with the same property: 1 .. 15 / 16 .. 99 and 1 .. 999 /
1000 .. 29999; BOOL has two values for three sources, so its values are drawn per position instead).  second(C, T) is T and, with
these ranges, min(C, T) is C: the bound rows and the type rows therefore swap the two ranges in their odd rows, where min(C, T) is
T's value, so that a source taken from the wrong side shows under min in one half or the other.  Floating-point values are compared
as bit patterns."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from oracle import grb_oracle as O
from tests.backend import DEVICES, bind
from tests.values import ALL_TYPES, FP_TYPES, same_fp

WR_LONG = 8192            # (entries of C_old(i,:) + T(i,:) above which a row is cut: grb_mxm_write.inc)
WR_MAX_PIECES = 256
PIECE_MIN_COLS = 16384    # (pieces = ceil(ncols / 16384), at most 256: matrix_apply_write_rule)
ONE_ROUND = 65 * 64       # (wave_lower_bound leaves its loop after one round up to this many entries ...)
TWO_ROUNDS = (ONE_ROUND + 1) * 64  # (... and after two up to this many)
ORACLE_MAX_COLS = 40_000  # (the second reference runs up to here)

Mode = namedtuple("Mode", "mask comp replace accum")  # mask: "none" / "S" (structural) / "V" (valued)
ACCUMS = (None, "plus", "second", "min")
ALL_MODES = [Mode("none", False, False, a) for a in ACCUMS[1:]] + \
            [Mode(k, c, r, a) for k in "SV" for c in (False, True) for r in (False, True) for a in ACCUMS]
FEW_MODES = [Mode("none", False, False, "plus"), Mode("S", False, False, None), Mode("S", True, False, "plus"),
             Mode("S", False, True, "second"), Mode("S", True, True, "min"), Mode("V", False, False, "plus"),
             Mode("V", True, False, None), Mode("V", False, True, "min"), Mode("V", True, True, "second"),
             Mode("V", False, True, None), Mode("V", True, True, "plus")]
TWO_MODES = [Mode("V", False, False, "plus"), Mode("V", True, True, None)]


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


def _name(mode):
    return f"{mode.mask}{'~' if mode.comp else ''}{'r' if mode.replace else ''}-{mode.accum}"


def _pieces(ncols):
    """(pieces, piece_cols) of a matrix with this many columns."""
    pieces = min(WR_MAX_PIECES, max(1, -(-ncols // PIECE_MIN_COLS)))
    return pieces, -(-ncols // pieces)


# ---- operands from explicit column lists -----------------------------------------------------------------------------------
def _list(rng, n, lo, hi, at=None):
    """n ascending distinct columns of [lo, hi); ``at`` = {index: column} pins entries, the others are drawn in between."""
    out = np.empty(n, np.int64)
    prev_i, prev_c = -1, lo - 1
    for i, c in sorted((at or {}).items()) + [(n, hi)]:
        k, span = i - prev_i - 1, c - prev_c - 1
        assert 0 <= k <= span, (n, lo, hi, at)
        out[prev_i + 1:i] = prev_c + 1 + np.sort(rng.choice(span, k, replace=False))
        if i < n:
            out[i] = c
        prev_i, prev_c = i, c
    return out


def _but(cols, drop=(), add=()):
    """The sorted list without the columns of ``drop`` and with those of ``add``."""
    cols = np.setdiff1d(np.asarray(cols, np.int64), np.asarray(drop, np.int64))
    return np.union1d(cols, np.asarray(add, np.int64))


class Rows:
    """The rows of C_old, T and M of one case, as sorted column lists; ``truth``: which mask entries hold a true value."""

    def __init__(self, ncols):
        self.ncols, self.c, self.t, self.m, self.truth = int(ncols), [], [], [], []

    def row(self, c=(), t=(), m=(), truth=None):
        lists = [np.asarray(x, np.int64).reshape(-1) for x in (c, t, m)]
        for x in lists:
            assert x.size == 0 or (x[0] >= 0 and x[-1] < self.ncols and (np.diff(x) > 0).all())
        if truth is None:  # (a fixed mix: about two entries of three are true)
            truth = (lists[2] * 2654435761 >> 5) % 3 != 0
        truth = np.asarray(truth, bool).reshape(-1)
        assert truth.size == lists[2].size
        self.c.append(lists[0]); self.t.append(lists[1]); self.m.append(lists[2]); self.truth.append(truth)
        return len(self.c) - 1

    @property
    def nrows(self):
        return len(self.c)

    @staticmethod
    def _csr(lists):
        ptr = np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64)
        return ptr, (np.concatenate(lists) if lists else np.zeros(0)).astype(np.int64)

    def operands(self, rng, tname, mask_type="INT8", swap_odd=False):
        """(C, T, M) as (indptr, cols, vals) triples, M's values true / false by ``truth``.  ``swap_odd``: in the odd rows C_old takes
        the values of T's range and T those of C_old's, so that min(C, T) is T's value there and C's in the even rows."""
        (cp, cj), (tp, tj), (mp, mj) = self._csr(self.c), self._csr(self.t), self._csr(self.m)
        cv, tv = _draw(rng, cj.size, tname, False), _draw(rng, tj.size, tname, True)
        if swap_odd and tname != "BOOL":
            c_odd, t_odd = (np.repeat(np.arange(self.nrows), np.diff(ptr)) % 2 == 1 for ptr in (cp, tp))
            cv[c_odd], tv[t_odd] = _draw(rng, int(c_odd.sum()), tname, True), _draw(rng, int(t_odd.sum()), tname, False)
        truth = np.concatenate(self.truth) if self.truth else np.zeros(0, bool)
        mv = np.where(truth, rng.integers(1, 100, mj.size), 0).astype(O.NP_OF[mask_type])
        return (cp, cj, cv), (tp, tj, tv), (mp, mj, mv)


def _draw(rng, k, tname, of_t):
    """Values of C_old (1 .. 999) or of T (1000 .. 2 10^6 - 1): see the module docstring for the narrow types."""
    np_t = np.dtype(O.NP_OF[tname])
    if tname == "BOOL":
        return rng.random(k) < 0.5
    if np_t.itemsize == 1:
        lo, hi = ((16, 100) if of_t else (1, 16))
    elif np_t.itemsize == 2:
        lo, hi = ((1000, 30000) if of_t else (1, 1000))
    else:
        lo, hi = ((1000, 2_000_000) if of_t else (1, 1000))
    return rng.integers(lo, hi, k).astype(np_t)


# ---- the expectation -------------------------------------------------------------------------------------------------------
def _ufunc(accum, tname):
    if accum == "second":
        return lambda a, b: b
    if tname == "BOOL":  # (the BOOL spellings of plus / min are lor / land)
        return {"plus": np.logical_or, "min": np.logical_and}[accum]
    return {"plus": np.add, "min": np.minimum}[accum]


def _keys(ptr, cols, ncols):
    return np.repeat(np.arange(ptr.size - 1, dtype=np.int64), np.diff(ptr)) * ncols + cols


def _expect(nrows, ncols, C, T, M, truth, mode, tname):
    """C<M, replace> = accum(C, T) on linearised keys: Z = T, or accum over the union of C and T; the mask admits the keys of its true
    entries (all of them when structural), or the others when complemented; the result is Z where admitted and, unless replace, C
    elsewhere.  Returns (indptr, cols, vals)."""
    kc, vc = _keys(C[0], C[1], ncols), C[2]
    kt, vt = _keys(T[0], T[1], ncols), T[2]
    if mode.accum is None:
        kz, vz = kt, vt
    else:
        kz = np.union1d(kc, kt)
        vz = np.empty(kz.size, vt.dtype)
        vz[np.searchsorted(kz, kc)] = vc
        vz[np.searchsorted(kz, kt)] = vt
        both, ic, it = np.intersect1d(kc, kt, assume_unique=True, return_indices=True)
        with np.errstate(all="ignore"):
            vz[np.searchsorted(kz, both)] = _ufunc(mode.accum, tname)(vc[ic], vt[it]).astype(vt.dtype)
    if mode.mask == "none":
        kr, vr = kz, vz
    else:
        km = _keys(M[0], M[1], ncols)
        if mode.mask == "V":
            km = km[truth]
        admit_z = np.isin(kz, km, assume_unique=True) != mode.comp
        kr, vr = kz[admit_z], vz[admit_z]
        if not mode.replace:
            keep_c = np.isin(kc, km, assume_unique=True) == mode.comp
            kr, vr = np.concatenate([kr, kc[keep_c]]), np.concatenate([vr, vc[keep_c]])
            order = np.argsort(kr, kind="stable")
            kr, vr = kr[order], vr[order]
            assert (np.diff(kr) > 0).all()
    ptr = np.searchsorted(kr, np.arange(nrows + 1, dtype=np.int64) * ncols).astype(np.int64)
    return ptr, kr % ncols, vr


def _same_arrays(got, exp, where):
    (gp, gj, gx), (ep, ej, ex) = got, exp
    gp, gj = np.asarray(gp).astype(np.int64), np.asarray(gj).astype(np.int64)
    if not np.array_equal(gp, ep):
        bad = np.flatnonzero(gp != ep)[:4] if gp.size == ep.size else []
        raise AssertionError(f"{where}: row pointers differ at {list(bad)}: got {gp[bad].tolist()} expected {ep[bad].tolist()} "
                             f"({gp.size} / {ep.size} pointers)")
    if not np.array_equal(gj, ej):
        bad = np.flatnonzero(gj != ej)[:4]
        raise AssertionError(f"{where}: columns differ at positions {bad.tolist()} (rows {(np.searchsorted(ep, bad, 'right') - 1).tolist()}): "
                             f"got {gj[bad].tolist()} expected {ej[bad].tolist()}")
    gx, ex = np.asarray(gx), np.asarray(ex)
    assert gx.dtype == ex.dtype, (where, gx.dtype, ex.dtype)
    if ex.dtype.kind == "f":
        same_fp(gx, ex, None, where)
    elif not np.array_equal(gx, ex):
        bad = np.flatnonzero(gx != ex)[:4]
        raise AssertionError(f"{where}: values differ at positions {bad.tolist()} (rows {(np.searchsorted(ep, bad, 'right') - 1).tolist()}, "
                             f"columns {ej[bad].tolist()}): got {gx[bad].tolist()} expected {ex[bad].tolist()}")


def _omat(nrows, ncols, csr, tname):
    return O.OMat(nrows, ncols, csr[0], csr[1], csr[2], tname)


def _oracle_agrees(nrows, ncols, C, T, M, mode, tname, mask_type, exp, where):
    """The second reference: the oracle's write rule behind an identity product (T = I any.second T)."""
    eye = np.arange(nrows + 1, dtype=np.int64)
    I = O.OMat(nrows, nrows, eye, eye[:-1], np.ones(nrows, O.NP_OF[tname]), tname)
    accum = mode.accum
    if tname == "BOOL" and accum in ("plus", "min"):
        accum = {"plus": "lor", "min": "land"}[accum]
    got = O.mxm(I, _omat(nrows, ncols, T, tname), "any_second", C=_omat(nrows, ncols, C, tname),
                mask=_omat(nrows, ncols, M, mask_type) if mode.mask != "none" else None, mask_comp=mode.comp,
                mask_struct=mode.mask == "S", accum=accum, replace=mode.replace)
    _same_arrays((got.indptr, got.indices, got.values), exp, where + " [restatement against the oracle]")


# ---- the library -----------------------------------------------------------------------------------------------------------
def _stored_iso(A):
    from graphblas_amd import _lib

    dp, dj, dx, nv, iso = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_int()
    assert _lib.lib.GrX_Matrix_export_CSR_device(ctypes.byref(dp), ctypes.byref(dj), ctypes.byref(dx), ctypes.byref(nv), ctypes.byref(iso), A._carg) == 0
    return bool(iso.value)


def _matrix(gb, nrows, ncols, csr, tname, iso=False):
    ptr, cols, vals = csr
    if cols.size == 0:
        return gb.Matrix(tname, nrows, ncols)  # (no storage at all: a null row pointer)
    if iso:
        assert (vals == vals[0]).all()
        A = gb.Matrix.ss.import_csr(nrows=nrows, ncols=ncols, indptr=ptr, values=vals[:1], col_indices=cols, is_iso=True, sorted_cols=True,
                                    dtype=tname)
        assert _stored_iso(A) and A.nvals == cols.size
        return A
    return gb.Matrix.from_csr(ptr, cols, vals, dtype=tname, ncols=ncols)


def _output_params(gb, M, mode):
    kw = {}
    if mode.mask != "none":
        mk = M.S if mode.mask == "S" else M.V
        kw = dict(mask=~mk if mode.comp else mk, replace=mode.replace)
    if mode.accum:
        kw["accum"] = getattr(gb.binary, mode.accum)
    return kw


def _set(name, value):
    from graphblas_amd import _lib

    assert _lib.lib.GrX_option_set(name, value) == 0, name


def _reset():
    from graphblas_amd import _lib

    assert _lib.lib.GrX_options_reset() == 0


def _got(C):
    return C.to_csr()


def _run(gb, rows, modes, where, *, tname="INT64", mask_type="INT8", seed=0, iso_c=False, iso_m=None, operands=None, specials=False,
         swap_odd=False, update=None):
    """Every mode under both kernels.  ``update(C, T, M, kw)`` replaces the plain ``C(**kw) << T`` (other producers of T).
    ``specials``: a floating-point T carries -0.0, NaN and the infinities in every mode but those that accumulate with min (what min
    gives with a NaN operand belongs to the suite of the special values; the min modes run on the plain values)."""
    rng = np.random.default_rng(9100 + seed)
    nrows, ncols = rows.nrows, rows.ncols
    C, T, M = operands or rows.operands(rng, tname, mask_type, swap_odd)
    T_special = None
    if specials and tname in FP_TYPES:
        tv = T[2].copy()
        tv[:: max(1, tv.size // 8)][:4] = [-0.0, np.nan, np.inf, -np.inf]
        T_special = (T[0], T[1], tv)
    truth = M[2] != 0  # (NaN is true, either zero false)
    if iso_c:
        C = (C[0], C[1], np.full_like(C[2], C[2][0]))
    if iso_m is not None:
        M = (M[0], M[1], np.full_like(M[2], iso_m))
        truth = M[2] != 0
    try:
        T_plain, Tm_plain = T, _matrix(gb, nrows, ncols, T, tname)
        Tm_special = _matrix(gb, nrows, ncols, T_special, tname) if T_special else None
        Mm = _matrix(gb, nrows, ncols, M, mask_type, iso=iso_m is not None)
        for mode in modes:
            T, Tm = (T_special, Tm_special) if T_special and mode.accum != "min" else (T_plain, Tm_plain)
            w = f"{where} {_name(mode)}"
            exp = _expect(nrows, ncols, C, T, M, truth, mode, tname)
            if ncols <= ORACLE_MAX_COLS:
                _oracle_agrees(nrows, ncols, C, T, M, mode, tname, mask_type, exp, w)
            for kernel in (1, 0):
                _set(b"mat_write_kernel", kernel)
                Cm = _matrix(gb, nrows, ncols, C, tname, iso=iso_c)
                kw = _output_params(gb, Mm, mode)
                if update:
                    update(Cm, Tm, Mm, kw)
                else:
                    Cm(**kw) << Tm
                _same_arrays(_got(Cm), exp, f"{w} kernel {kernel}")
    finally:
        _reset()


# ---- 1. chunk lengths ------------------------------------------------------------------------------------------------------
LENS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
N_CHUNK = 640


def _chunk_rows(arrangement):
    """One row per (len C_old, len T, len M) of LENS^3, and per (len C_old, len T) under a full mask row: 810 rows."""
    rng = np.random.default_rng(31)
    rows = Rows(N_CHUNK)
    for lc in LENS:
        for lt in LENS:
            for lm in LENS + (N_CHUNK,):
                if arrangement == "interleaved":  # C on multiples of 3, T on multiples of 2
                    c, t, m = 3 * np.arange(lc), 2 * np.arange(lt), _list(rng, lm, 0, N_CHUNK)
                elif arrangement == "c_below_t":
                    c, t, m = _list(rng, lc, 0, 300), _list(rng, lt, 300, N_CHUNK), (np.arange(lm) * N_CHUNK) // max(lm, 1)
                elif arrangement == "t_below_c":
                    c, t, m = _list(rng, lc, 320, N_CHUNK), _list(rng, lt, 0, 320), (np.arange(lm) * N_CHUNK) // max(lm, 1)
                else:
                    c, t, m = _list(rng, lc, 0, N_CHUNK), _list(rng, lt, 0, N_CHUNK), _list(rng, lm, 0, N_CHUNK)
                rows.row(c, t, m, truth=rng.random(lm) < 0.6)
    return rows


@pytest.mark.parametrize("group", range(3))
@pytest.mark.parametrize("arrangement", ["interleaved", "c_below_t", "t_below_c", "random"])
def test_chunk_lengths(gb, arrangement, group):
    """Lists of 0, 1, 63, 64, 65, 127, 128, 129 and 200 entries against each other (and a full mask row): a chunk that is empty, one
    short of full, full, and one entry into the next, in every list independently; every arrangement under every mask kind,
    complement, replace and accumulator (the 35 modes in three groups: one run of all of them takes the emulator two minutes).  The
    rows with nothing in C_old and T but a mask row are rows without a unit between working ones."""
    _run(gb, _chunk_rows(arrangement), ALL_MODES[group::3], f"chunks {arrangement}")


# ---- 2. the bound ----------------------------------------------------------------------------------------------------------
N_BOUND = 4096


def _bound_rows():
    rng = np.random.default_rng(32)
    rows = Rows(N_BOUND)
    n = N_BOUND
    # a list with exactly 64 / 65 entries (left) while another has hundreds: short at the start, at the end, and spread over the row
    for short in (64, 65, 128, 129):
        for which in range(3):
            for lo, hi in ((0, 400), (n - 400, n), (0, n)):
                lists = [_list(rng, 300, 0, n) for _ in range(3)]
                lists[which] = _list(rng, short, lo, hi)
                # the last column of the short list -- its 64th / 65th (128th / 129th) -- is taken in both other lists: an entry
                # that is wrong as soon as the short list is held to be loaded one entry too early or too late
                last = lists[which][-1]
                for other in range(3):
                    if other != which:
                        lists[other] = _but(lists[other], add=[last])
                k = rows.row(*lists)
                rows.truth[k][np.searchsorted(rows.m[k], last)] = (lo, hi) != (0, 400)  # (that mask entry: false in one row, true in two)
    # the column on lane 63 of one list = a column of another list at lane 0, at lane 63, and in the next chunk (64, 100)
    X = 1500
    for a in range(3):
        for b in range(3):
            if a != b:
                for at in (0, 63, 64, 100):
                    lists = [_list(rng, 150, 0, n) for _ in range(3)]
                    lists[a] = _list(rng, 200, 0, n, {63: X})
                    lists[b] = _list(rng, 200, 0, n, {at: X})
                    k = rows.row(*lists)
                    if 2 in (a, b):  # (the mask entry on the bound: false in every second row)
                        rows.truth[k][np.searchsorted(rows.m[k], X)] = bool(at & 64)
    # the mask far denser than C_old and T: steps where only the mask advances
    for lm in (3000, n):
        rows.row(_list(rng, 100, 0, n), _list(rng, 100, 0, n), _list(rng, lm, 0, n))
        rows.row(_list(rng, 70, 2000, n), _list(rng, 3, 3000, n), _list(rng, lm, 0, n))
    # all mask entries below the first C / T column, and all above the last
    for lm in (10, 64, 65, 200):
        rows.row(_list(rng, 150, 1000, 2000), _list(rng, 150, 1000, 2000), _list(rng, lm, 0, 1000))
        rows.row(_list(rng, 150, 1000, 2000), _list(rng, 150, 1000, 2000), _list(rng, lm, 2000, n))
    # a false valued-mask entry exactly on the bound (lane 63 of a mask with more to load) and at column 0 (code -1), with an entry
    # of C_old and of T, of C_old only, and of T only under it
    for c0, t0 in ((True, True), (True, False), (False, True)):
        m = _list(rng, 200, 0, n, {0: 0, 63: X})
        c = _but(_list(rng, 150, 1, n), drop=[X], add=[0, X] if c0 else [])
        t = _but(_list(rng, 150, 1, n), drop=[X], add=[0, X] if t0 else [])
        truth = rng.random(200) < 0.6
        truth[[0, 63]] = False
        rows.row(c, t, m, truth)
    # C_old and T identical: every entry has a partner
    for ln in (64, 65, 200):
        same = _list(rng, ln, 0, n)
        rows.row(same, same, _list(rng, 150, 0, n))
    # interlocked: every C-only entry between two T entries of the same step (both popcount terms of its position non-zero), and the
    # reverse; runs of two C-only entries between T entries
    ev = 2 * np.arange(200)
    rows.row(ev + 1, ev, _list(rng, 250, 0, 400))
    rows.row(ev, ev + 1, _list(rng, 250, 0, 400))
    rows.row(_but(np.arange(600), drop=3 * np.arange(200)), 3 * np.arange(200), _list(rng, 400, 0, 600))
    rows.row(3 * np.arange(200), _but(np.arange(600), drop=3 * np.arange(200)), _list(rng, 400, 0, 600))
    return rows


@pytest.mark.parametrize("group", range(3))
def test_the_bound(gb, group):
    """The step's bound: a list with exactly 64 and 65 entries left while another has hundreds; the column on lane 63 of one list met
    by another list's lane 0, lane 63 and next chunk; a mask far denser than C_old and T; all mask entries below / above C_old and T; a
    false valued-mask entry on the bound and at column 0; identical lists; interlocked lists."""
    _run(gb, _bound_rows(), ALL_MODES[group::3], "bound", swap_odd=True)


# ---- 3. the row cut --------------------------------------------------------------------------------------------------------
def _boundary_cols(ncols):
    """k piece_cols - 1, k piece_cols, k piece_cols + 1 for every piece boundary, column 0 and the last column."""
    pieces, pc = _pieces(ncols)
    b = [0, ncols - 1] + [k * pc + d for k in range(1, pieces) for d in (-1, 0, 1)]
    return np.unique([x for x in b if 0 <= x < ncols])


def _cut_rows(ncols):
    rng = np.random.default_rng(33 + ncols)
    rows = Rows(ncols)
    pieces, pc = _pieces(ncols)
    # len(C_old) + len(T) at 8192 and 8193
    for lc, lt in ((8192, 0), (8193, 0), (0, 8192), (0, 8193), (4096, 4096), (4096, 4097)):
        rows.row(_list(rng, lc, 0, ncols), _list(rng, lt, 0, ncols), _list(rng, 5000, 0, ncols))
    # entries on the piece boundaries in each of C_old, T and M separately, and in all three
    B = _boundary_cols(ncols)
    for which in ((0,), (1,), (2,), (0, 1, 2)):
        lists = [_but(_list(rng, 5000, 0, ncols), drop=B) for _ in range(3)]
        for w in which:
            lists[w] = _but(lists[w], add=B)
        rows.row(*lists)
    if pieces > 1:
        last = (pieces - 1) * pc
        # everything in the first piece: the last holds only mask entries, or nothing
        rows.row(_list(rng, 4500, 0, pc), _list(rng, 4500, 0, pc), _list(rng, 3000, 0, ncols))
        rows.row(_list(rng, 4500, 0, pc), _list(rng, 4500, 0, pc), _list(rng, 3000, 0, pc))
        # everything in the last piece, the last column taken
        rows.row(_list(rng, 4500, last, ncols, {4499: ncols - 1}), _list(rng, 4500, last, ncols), _list(rng, 3000, 0, ncols))
        rows.row(_list(rng, 4500, last, ncols), _list(rng, 4500, last, ncols, {4499: ncols - 1}), _list(rng, 3000, last, ncols, {2999: ncols - 1}))
        # pieces with entries of one list only
        rows.row(_list(rng, 5000, 0, pc), _list(rng, 5000, last, ncols), _list(rng, 3000, 0, ncols))
        rows.row(_list(rng, 5000, last, ncols), _list(rng, 5000, 0, pc), _list(rng, 3000, 0, ncols))
        rows.row(_list(rng, 8300, 0, ncols), [], _list(rng, 3000, 0, pc))
    if pieces > 2:  # a middle piece that holds nothing, and one that holds only mask entries
        outer = np.concatenate([np.arange(pc), np.arange(2 * pc, ncols)])
        rows.row(outer[_list(rng, 4500, 0, outer.size)], outer[_list(rng, 4500, 0, outer.size)], outer[_list(rng, 3000, 0, outer.size)])
        rows.row(outer[_list(rng, 4500, 0, outer.size)], outer[_list(rng, 4500, 0, outer.size)], _list(rng, 3000, pc, 2 * pc))
    return rows


@pytest.mark.parametrize("ncols", [16384, 16385, 32768, 32769])
def test_row_cut(gb, ncols):
    """Rows at the cut: 8192 and 8193 entries in C_old and T together (8192 + 0, 0 + 8193, 4096 + 4097 and their neighbours) on 16384,
    16385, 32768 and 32769 columns -- one, two, two and three pieces; entries on k piece_cols - 1, k piece_cols, k piece_cols + 1, column
    0 and the last column in each list; pieces that hold nothing, only mask entries, or entries of one list; an empty first and an empty
    last piece.  No statistic exposes the number of units, so the 8192 / 8193 pair is a VALUE test on both sides of the cut: the row of
    8192 is merged by one wavefront, the row of 8193 by one per piece, and both must give the restated result."""
    assert _pieces(ncols)[0] == {16384: 1, 16385: 2, 32768: 2, 32769: 3}[ncols]
    _run(gb, _cut_rows(ncols), FEW_MODES, f"cut {ncols}", seed=ncols)


@pytest.mark.parametrize("ncols", [16385, 32769])
def test_row_cut_without_old_content(gb, ncols):
    """T rows of 8192 and 8193 entries into a C without storage (a null row pointer: every row's C_old is empty)."""
    rng = np.random.default_rng(34)
    rows = Rows(ncols)
    for lt in (8192, 8193, 0, 8193, 70):
        rows.row([], _list(rng, lt, 0, ncols), _list(rng, 5000, 0, ncols))
    rows.row([], _but(_list(rng, 9000, 0, ncols), add=_boundary_cols(ncols)), _but(_list(rng, 5000, 0, ncols), add=_boundary_cols(ncols)))
    _run(gb, rows, FEW_MODES, f"cut {ncols}, C empty")


# ---- 4. the piece cap ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows", [1, 2])
@pytest.mark.parametrize("ncols", [256 * 16384, 256 * 16384 + 1, 5_000_000])
def test_piece_cap(gb, ncols, nrows):
    """256 pieces and no more: 256 * 16384 columns (piece_cols 16384), one more (16385: the last piece is short) and 5 000 000 (19532).
    One cut row has entries on the boundaries of pieces 1, 2, 128 and 255, on column 0 and on the last column: C_old on k piece_cols - 1
    and k piece_cols, T on k piece_cols and k piece_cols + 1, M on all three."""
    pieces, pc = _pieces(ncols)
    assert pieces == WR_MAX_PIECES and pc == {256 * 16384: 16384, 256 * 16384 + 1: 16385, 5_000_000: 19532}[ncols]
    rng = np.random.default_rng(35)
    ks = np.array([1, 2, 128, 255]) * pc
    B = np.concatenate([ks - 1, ks, ks + 1, [0, ncols - 1]])
    rows = Rows(ncols)
    for _ in range(nrows - 1):  # (an uncut row in front of the cut one)
        rows.row(_list(rng, 100, 0, ncols), _list(rng, 100, 0, ncols), _list(rng, 100, 0, ncols))
    c = _but(_list(rng, 4500, 0, ncols), drop=B, add=np.concatenate([ks - 1, ks, [0]]))
    t = _but(_list(rng, 4500, 0, ncols), drop=B, add=np.concatenate([ks, ks + 1, [ncols - 1]]))
    m = _but(_list(rng, 6000, 0, ncols), add=B)
    assert c.size + t.size > WR_LONG
    k = rows.row(c, t, m)
    rows.truth[k][np.searchsorted(m, ks)] = [True, False, True, False]
    _run(gb, rows, FEW_MODES, f"cap {ncols} x {nrows}")


# ---- 5. the rounds of the 64-ary search ------------------------------------------------------------------------------------
def _with_key(rng, n, ncols, key, where):
    """A list of n columns whose relation to the piece boundary ``key`` is ``where``: the key is the element at a probed index
    (a multiple of the first round's step), absent and strictly between two probes, below every entry, above every entry, or the last
    entry."""
    step = -(-n // 64)
    base = (n * key // ncols) // step * step
    if where == "probe":
        return _list(rng, n, 0, ncols, {base: key})
    if where == "between":
        return _but(_list(rng, n + 1, 0, ncols, {base + step // 2: key}), drop=[key])
    if where == "below":
        return _list(rng, n, key + 1, ncols)
    if where == "above":
        return _list(rng, n, 0, key)
    assert where == "last"
    return _list(rng, n, 0, key + 1, {n - 1: key})


KEY_POSITIONS = ("probe", "between", "below", "above", "last")


@pytest.mark.parametrize("n", [4096, 4097, ONE_ROUND, ONE_ROUND + 1])
def test_search_one_and_two_rounds(gb, n):
    """A cut row with 4096, 4097, 4160 and 4161 entries of one list (C_old, T, M in turn; 4160 is the most the search settles in one
    round), the first piece boundary equal to a probed element, between two probes, below every entry, above every entry and equal to
    the last entry."""
    ncols = 32769
    pc = _pieces(ncols)[1]
    rng = np.random.default_rng(36 + n)
    rows = Rows(ncols)
    for which in range(3):
        for where in KEY_POSITIONS:
            lists = [_list(rng, 4300, 0, ncols), _list(rng, 4300, 0, ncols), _list(rng, 3000, 0, ncols)]
            lists[which] = _with_key(rng, n, ncols, pc, where)
            rows.row(*lists)
    _run(gb, rows, TWO_MODES, f"search {n}")


N_THREE = 270_000


def _three_round_rows():
    ncols, n = 300_000, N_THREE
    pieces, pc = _pieces(ncols)
    assert pieces == 19 and n > TWO_ROUNDS
    rng = np.random.default_rng(37)
    step = -(-n // 64)

    def near_full(kind):
        """All columns of [lo, hi) but hi - lo - n: as many are left out below 5 pc that 5 pc sits at a probed index of the first
        round, as many between 5 pc and 9 pc (7 pc among them: an absent key) that 9 pc sits a third of a step behind a probe.
        ``kind``: the list starts above the first boundary / ends below the last one / ends on the last one."""
        lo, hi = {"below": (pc + 3, ncols), "above": (0, 18 * pc - 3), "last": (0, 18 * pc + 1)}[kind]
        out_n = hi - lo - n
        r1 = (5 * pc - lo) % step
        r2 = ((9 * pc - lo) - r1 - step // 3) % step or step
        assert r1 + r2 <= out_n
        drop = np.concatenate([lo + 1 + rng.choice(5 * pc - lo - 1, r1, replace=False),
                               rng.choice(np.setdiff1d(np.arange(5 * pc + 1, 9 * pc), [7 * pc]), r2 - 1, replace=False), [7 * pc],
                               9 * pc + 1 + rng.choice(hi - 1 - (9 * pc + 1), out_n - r1 - r2, replace=False)])
        out = np.setdiff1d(np.arange(lo, hi), drop)
        assert out.size == n and np.searchsorted(out, 5 * pc) % step == 0 and out[np.searchsorted(out, 5 * pc)] == 5 * pc
        assert np.searchsorted(out, 9 * pc) % step == step // 3 and out[np.searchsorted(out, 9 * pc)] == 9 * pc and 7 * pc not in out
        assert out[-1] == hi - 1
        return out

    rows = Rows(ncols)
    rows.row(_list(rng, 9000, 0, ncols), near_full("below"), near_full("above"))
    rows.row(near_full("last"), _list(rng, 300, 0, ncols), _list(rng, 9000, 0, ncols))
    return rows


@pytest.mark.parametrize("mode", TWO_MODES, ids=_name)
def test_search_three_rounds(gb, mode):
    """270 000 entries of one list in a cut row (more than 266 304: three rounds of the search), on 300 000 columns and 19 pieces: T
    starting above the first boundary, M ending below the last, C_old ending on the last; boundaries on a probed element, absent, and
    present between two probes."""
    _run(gb, _three_round_rows(), [mode], "search 270000")


# ---- 6. the unit tables ----------------------------------------------------------------------------------------------------
def _cut_lists(rng, ncols, nm=3000):
    return _list(rng, 4200, 0, ncols), _list(rng, 4200, 0, ncols), _list(rng, nm, 0, ncols)


def _short_lists(rng, ncols):
    return _list(rng, 70, 0, ncols), _list(rng, 65, 0, ncols), _list(rng, 90, 0, ncols)


@pytest.mark.parametrize("layout", ["1", "3", "4", "5", "cut", "cut+1", "cut+2", "cut,empty,1", "1,cut,1"])
def test_unit_counts(gb, layout):
    """n_units of 1, 3, 4 and 5 -- the tail wavefronts of the last workgroup leave early --, made of uncut rows, or of a row cut in three
    with uncut ones behind it; rows without a unit (nothing in C_old and T, a mask row) in front, behind and in runs between the
    working rows; a cut row directly followed by an uncut one and by an empty one."""
    ncols = 32769
    rng = np.random.default_rng(38)
    rows = Rows(ncols)
    no_unit = lambda: rows.row([], [], _list(rng, 40, 0, ncols))
    no_unit()
    if layout.isdigit():
        for i in range(int(layout)):
            rows.row(*_short_lists(rng, ncols))
            for _ in range(i):
                no_unit()
        units = int(layout)
    else:
        units = 0
        for part in layout.replace("+", ",").split(","):
            if part == "cut":
                rows.row(*_cut_lists(rng, ncols))
                units += 3
            elif part == "empty":
                rows.row()
            else:
                for _ in range(int(part)):
                    rows.row(*_short_lists(rng, ncols))
                    units += 1
        if layout == "cut":
            no_unit()
    lens = np.array([c.size + t.size for c, t in zip(rows.c, rows.t)])
    assert np.where(lens > WR_LONG, 3, lens > 0).sum() == units
    _run(gb, rows, FEW_MODES, f"units {layout}")


@pytest.mark.parametrize("nrows", [255, 256, 257])
def test_rows_past_one_workgroup(gb, nrows):
    """255, 256 and 257 rows: the unit counts and the row pointers are written by 256 threads per workgroup, and the entry behind the
    last row belongs to the second one from 256 rows on.  The last rows work; runs of rows without a unit lie in front of them."""
    ncols = 300
    rng = np.random.default_rng(39)
    rows = Rows(ncols)
    for i in range(nrows):
        if i >= 253 or i % 11 == 0:
            rows.row(_list(rng, 1 + i % 70, 0, ncols), _list(rng, 1 + (i * 7) % 67, 0, ncols), _list(rng, 50, 0, ncols))
        else:
            rows.row([], [], _list(rng, i % 5, 0, ncols))
    _run(gb, rows, FEW_MODES, f"{nrows} rows")


@pytest.mark.parametrize("kernel", [1, 0])
def test_results_without_entries(gb, kernel):
    """A result with no entries -- everything masked out under replace; C_old and T both empty under a mask; T empty and C_old masked
    out -- is read (nvals, to_coo, to_csr) and then used as the output of a second update."""
    ncols, nrows = 32769, 3
    rng = np.random.default_rng(40)
    rows = Rows(ncols)
    rows.row(_list(rng, 4200, 0, 20000), _list(rng, 4200, 0, 20000), _list(rng, 500, 20000, ncols))  # (a cut row)
    rows.row(_list(rng, 100, 0, 20000), _list(rng, 65, 0, 20000), _list(rng, 64, 20000, ncols))
    rows.row([], [], _list(rng, 10, 0, ncols))
    C, T, M = rows.operands(rng, "INT64")
    empty = (np.zeros(nrows + 1, np.int64), np.zeros(0, np.int64), np.zeros(0, np.int64))
    second = Rows(ncols)
    for i in range(nrows):
        second.row([], rows.t[i], _list(rng, 6000, 0, ncols))
    _, T2, M2 = second.operands(rng, "INT64")
    mode2 = Mode("V", False, False, "plus")
    exp2 = _expect(nrows, ncols, empty, T2, M2, M2[2] != 0, mode2, "INT64")
    try:
        _set(b"mat_write_kernel", kernel)
        for name, c_in, t_in, mode in (("all masked out", C, T, Mode("S", False, True, "plus")),
                                       ("C and T empty", empty, empty, Mode("S", False, False, "plus")),
                                       ("T empty, C masked out", C, empty, Mode("V", False, True, None))):
            exp = _expect(nrows, ncols, c_in, t_in, M, M[2] != 0, mode, "INT64")
            assert exp[1].size == 0
            Cm, Tm, Mm = _matrix(gb, nrows, ncols, c_in, "INT64"), _matrix(gb, nrows, ncols, t_in, "INT64"), _matrix(gb, nrows, ncols, M, "INT8")
            Cm(**_output_params(gb, Mm, mode)) << Tm
            assert Cm.nvals == 0, name
            I, J, X = Cm.to_coo()
            assert I.size == 0 and J.size == 0 and X.size == 0, name
            Cp, Cj, Cx = Cm.to_csr()
            assert not np.asarray(Cp).any() and np.asarray(Cj).size == 0 and np.asarray(Cx).size == 0, name
            Cm(**_output_params(gb, _matrix(gb, nrows, ncols, M2, "INT8"), mode2)) << _matrix(gb, nrows, ncols, T2, "INT64")
            _same_arrays(_got(Cm), exp2, f"second update after '{name}' kernel {kernel}")
    finally:
        _reset()


# ---- 7. types --------------------------------------------------------------------------------------------------------------
def _type_rows():
    rng = np.random.default_rng(41)
    rows = Rows(700)
    for lc, lt, lm in ((65, 129, 64), (200, 200, 128), (0, 70, 300), (70, 0, 300), (64, 64, 700), (1, 1, 1), (129, 63, 0), (0, 0, 9),
                       (300, 310, 320)):
        rows.row(_list(rng, lc, 0, 700), _list(rng, lt, 0, 700), _list(rng, lm, 0, 700))
    same = _list(rng, 130, 0, 700)
    rows.row(same, same, _list(rng, 200, 0, 700))
    return rows


@pytest.mark.parametrize("tname", ALL_TYPES)
def test_value_types(gb, tname):
    """C_old and T in every type: the value chunk in LDS at 1, 2, 4 and 8 bytes; floating-point T values include -0.0, NaN and the
    infinities (bit patterns compared)."""
    _run(gb, _type_rows(), FEW_MODES, f"type {tname}", tname=tname, specials=True, swap_odd=True)


@pytest.mark.parametrize("tname", ["INT8", "UINT16", "FP32", "INT64"])
def test_iso_old_content(gb, tname):
    """C_old stored as one value."""
    _run(gb, _type_rows(), FEW_MODES, f"iso C {tname}", tname=tname, iso_c=True)


@pytest.mark.parametrize("mask_type,value", [("INT8", 1), ("INT8", 0), ("FP64", 2.5), ("FP64", -0.0), ("UINT16", 256), ("BOOL", False)])
def test_iso_valued_mask(gb, mask_type, value):
    """A valued mask stored as one value, true and false."""
    modes = [m for m in FEW_MODES if m.mask == "V"]
    _run(gb, _type_rows(), modes, f"iso M {mask_type} {value}", tname="INT32", mask_type=mask_type, iso_m=O.NP_OF[mask_type](value))


def _mask_values(mask_type):
    """Values whose truth changes when they are read at another width or as another type."""
    np_t = np.dtype(O.NP_OF[mask_type])
    if mask_type in FP_TYPES:
        sub = np.finfo(np_t).smallest_subnormal
        sub32 = np.finfo(np.float32).smallest_subnormal
        return np.array([0.0, -0.0, np.nan, sub, -sub, sub32, -sub32, np.inf, -np.inf, 1.0], np_t)
    if mask_type == "BOOL":
        return np.array([False, True, True, False, False], np_t)
    bits, signed = np_t.itemsize * 8, np_t.kind == "i"
    raw = {8: [0, 1, 128, 255, 0], 16: [0, 256, -256, -32768, 1, 0], 32: [0, 1 << 16, 1 << 31, 1, 0],
           64: [0, 1 << 32, 1 << 40, 1 << 63, 1, 0]}[bits]
    return np.array([v % (1 << bits) for v in raw], np.dtype(f"u{bits // 8}")).view(np_t) if signed else \
        np.array([v % (1 << bits) for v in raw], np_t)


MASK_MODES = [Mode("V", False, False, "plus"), Mode("V", True, False, None), Mode("V", False, True, None), Mode("V", True, True, "plus"),
              Mode("V", False, False, None)]


@pytest.mark.parametrize("mask_type", ALL_TYPES)
def test_valued_mask_types(gb, mask_type):
    """A valued mask in every type, with values that are true only at the type's own width: +-0.0, NaN, subnormals and infinities;
    256, -256, -32768 in 16 bits; 1 << 16, 1 << 31 in 32; 1 << 32, 1 << 40, INT64_MIN in 64.  Through the plain update, and through mxm
    under mxm_mask_mode 0 (full product, then the write rule), 1 and 2 (mask-driven where it pays / always, or fused with the
    complement: its own truth table in true_pattern) against the same expectation."""
    rows = _type_rows()
    rng = np.random.default_rng(42)
    C, T, M = rows.operands(rng, "INT32", mask_type)
    vals = _mask_values(mask_type)
    M = (M[0], M[1], vals[np.arange(M[1].size) % vals.size])
    _run(gb, rows, MASK_MODES, f"mask {mask_type}", tname="INT32", mask_type=mask_type, operands=(C, T, M))
    eye = np.arange(rows.nrows)
    I = gb.Matrix.from_coo(eye, eye, np.ones(rows.nrows, np.int32), dtype="INT32", nrows=rows.nrows, ncols=rows.nrows)
    from graphblas_amd import device

    for mask_mode in (0, 1, 2):
        def product(Cm, Tm, Mm, kw):
            _set(b"mxm_mask_mode", mask_mode)
            Cm(**kw) << I.mxm(Tm, gb.semiring.plus_times)
            # the witness of the path: 3 the full product, 4 the mask-driven one, 7 the product with the complement fused in.  With an
            # identity on the left the flops are nnz(T), below the threshold of mode 1: only mode 2 drives the product by the mask
            comp = kw["mask"].complement
            want = 3 if mask_mode == 0 else (7 if comp else (4 if mask_mode == 2 else 3))
            assert device.last_stats()["method"] == want, (mask_type, mask_mode, comp, device.last_stats()["method"])

        _run(gb, rows, MASK_MODES, f"mask {mask_type} mxm mode {mask_mode}", tname="INT32", mask_type=mask_type, operands=(C, T, M),
             update=product)


# ---- 8. producers of T and aliasing ----------------------------------------------------------------------------------------
def _producer_rows():
    ncols = 32769
    rng = np.random.default_rng(43)
    rows = Rows(ncols)
    rows.row(*_cut_lists(rng, ncols, 6000))
    rows.row(*_short_lists(rng, ncols))
    rows.row()
    rows.row(_but(_list(rng, 5000, 0, ncols), add=_boundary_cols(ncols)), _but(_list(rng, 5000, 0, ncols), add=_boundary_cols(ncols)),
             _but(_list(rng, 5000, 0, ncols), add=_boundary_cols(ncols)))
    return rows


@pytest.mark.parametrize("producer", ["mxm", "transpose", "transpose_iso", "select"])
def test_producers_hand_over(gb, producer):
    """A cut row through each producer of T: an identity product under mxm_mask_mode 0, a masked A.T with T built by the transpose
    (iso and not), a masked, accumulated select that keeps everything."""
    rows = _producer_rows()
    nrows, ncols = rows.nrows, rows.ncols
    rng = np.random.default_rng(44)
    C, T, M = rows.operands(rng, "INT64")
    if producer == "transpose_iso":
        T = (T[0], T[1], np.full_like(T[2], 1500))
    t_rows = np.repeat(np.arange(nrows), np.diff(T[0]))
    eye = np.arange(nrows)
    I = gb.Matrix.from_coo(eye, eye, np.ones(nrows, np.int64), dtype="INT64", nrows=nrows, ncols=nrows)
    A = gb.Matrix.from_coo(T[1], t_rows, T[2], dtype="INT64", nrows=ncols, ncols=nrows)  # (T's transpose)
    if producer == "transpose_iso":
        assert _stored_iso(A)

    def update(Cm, Tm, Mm, kw):
        if producer == "mxm":
            _set(b"mxm_mask_mode", 0)
            Cm(**kw) << I.mxm(Tm, gb.semiring.plus_times)
        elif producer == "select":
            Cm(**kw) << Tm.select("valuege", 0)
        else:
            Cm(**kw) << A.T

    modes = [m for m in FEW_MODES if m.mask != "none" and (producer != "select" or m.accum)]
    _run(gb, rows, modes, f"producer {producer}", operands=(C, T, M), update=update)


@pytest.mark.parametrize("kernel", [1, 0])
def test_aliased_operands(gb, kernel):
    """C(C.S) << T, C(C.V, replace) << T, C(accum) << C, and the mask being T (structural, and valued with zeros among T's values)."""
    rows = _producer_rows()
    nrows, ncols = rows.nrows, rows.ncols
    rng = np.random.default_rng(45)
    C, T, _ = rows.operands(rng, "INT64")
    C[2][::3] = 0  # (false entries of a valued mask)
    T[2][::4] = 0
    new = lambda csr: _matrix(gb, nrows, ncols, csr, "INT64")
    try:
        _set(b"mat_write_kernel", kernel)
        for name, mode, mask, src in (("C(C.S, plus) << T", Mode("S", False, False, "plus"), "C", "T"),
                                      ("C(~C.V, replace) << T", Mode("V", True, True, None), "C", "T"),
                                      ("C(C.V, min) << T", Mode("V", False, False, "min"), "C", "T"),
                                      ("C(plus) << C", Mode("none", False, False, "plus"), None, "C"),
                                      ("C(C.S, plus, replace) << C", Mode("S", False, True, "plus"), "C", "C"),
                                      ("C(T.S, second) << T", Mode("S", False, False, "second"), "T", "T"),
                                      ("C(T.V, replace) << T", Mode("V", False, True, None), "T", "T"),
                                      ("C(~T.V, plus) << T", Mode("V", True, False, "plus"), "T", "T")):
            m_csr, t_csr = {"C": C, "T": T, None: C}[mask], {"C": C, "T": T}[src]
            exp = _expect(nrows, ncols, C, t_csr, m_csr, m_csr[2] != 0, mode, "INT64")
            if ncols <= ORACLE_MAX_COLS:
                _oracle_agrees(nrows, ncols, C, t_csr, m_csr, mode, "INT64", "INT64", exp, name)
            Cm, Tm = new(C), new(T)
            objs = {"C": Cm, "T": Tm, None: None}
            Cm(**_output_params(gb, objs[mask], mode)) << objs[src]
            _same_arrays(_got(Cm), exp, f"{name} kernel {kernel}")
    finally:
        _reset()
