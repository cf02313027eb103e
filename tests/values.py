"""Value domains for the parity tests and the strict comparator they are checked with.

``rand_vals(rng, k, tname, domain)`` draws the values of a matrix or a vector:

* ``"small"``: what the parity suite has always used -- floating-point values are the integers 1..8, integers 0..99, BOOL is
  true with probability 0.8.  Every sum of them is exact, so every semiring compares bit for bit.
* ``"signed"``: integers over the whole range of the type, with its min / max, 0 and 1 (and -1 for signed types, 2^(bits-1) for
  unsigned ones) forced in; floating-point values are normal reals of both signs, magnitudes 10^-span .. 10^span (``span`` 30 by
  default: min / max semirings; the plus semirings pass a span that keeps every partial sum finite).
* ``"special"`` (floating point): the ``"signed"`` mix plus NaN, +-inf, +-0.0, subnormals and +-FLT_MAX / DBL_MAX.
* ``"exact"`` (floating point): integers -8..8 (with -0.0) plus NaN, +-inf and +-0.0 -- the values whose sums, products and folds
  are exact and whose non-finite results do not depend on the order of a fold, so the plus semirings can be compared bit for bit
  over negative values, signed zeros and infinities.

``shape_rows`` turns some rows of a COO matrix into rows whose products are all NaN, all -0.0, or meet +inf with -inf.

``same_values`` is the comparator: equal patterns, equal integer / BOOL values, floating-point values equal as BIT PATTERNS except
that any NaN matches any NaN and, under min / max / any, a zero matches a zero of either sign (IEEE minNum leaves min(-0, +0) open).
``plus_within_bound`` checks a floating-point sum of real values of mixed sign against its exact value under an error bound.
"""
import math

import numpy as np

from oracle import grb_oracle as O

FP_TYPES = ("FP32", "FP64")
INT_TYPES = ("INT8", "INT16", "INT32", "INT64", "UINT8", "UINT16", "UINT32", "UINT64")
ALL_TYPES = ("BOOL",) + INT_TYPES + FP_TYPES


def _force(rng, out, forced):
    """Put the values ``forced`` at random distinct positions of ``out`` (as many as fit)."""
    k = min(len(out), len(forced))
    if k:
        out[rng.choice(len(out), k, replace=False)] = np.asarray(forced[:k], out.dtype)
    return out


def _fp_reals(rng, k, np_t, span):
    mag = 10.0 ** rng.uniform(-span, span, k)
    sign = np.where(rng.random(k) < 0.5, -1.0, 1.0)
    return (sign * mag).astype(np_t)


def rand_vals(rng, k, tname, domain="small", span=30):
    np_t = O.NP_OF[tname]
    if tname == "BOOL":
        return rng.random(k) < 0.8 if domain == "small" else rng.random(k) < 0.5
    fp = tname in FP_TYPES
    if domain == "small":
        return rng.integers(1, 9, k).astype(np_t) if fp else rng.integers(0, 100, k).astype(np_t)
    if domain == "signed":
        if fp:
            return _force(rng, _fp_reals(rng, k, np_t, span), [1.0, -1.0])
        info = np.iinfo(np_t)
        out = rng.integers(int(info.min), int(info.max), k, dtype=np_t, endpoint=True)
        forced = [info.min, info.max, 0, 1] + ([-1] if info.min < 0 else [1 << (info.bits - 1), (1 << (info.bits - 1)) + 1])
        return _force(rng, out, forced)
    if not fp:
        raise ValueError(f"domain {domain!r} is floating-point only")
    fi = np.finfo(np_t)
    if domain == "special":
        out = _fp_reals(rng, k, np_t, span)
        sub = fi.smallest_subnormal
        specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, sub, -sub, 3 * sub, fi.max, -fi.max], np_t)
        pick = rng.random(k) < 0.3
        out[pick] = specials[rng.integers(0, specials.size, int(pick.sum()))]
        return _force(rng, out, specials)
    if domain == "exact":
        out = rng.integers(-8, 9, k).astype(np_t)
        out[out == 0] = np.where(rng.random(int((out == 0).sum())) < 0.5, -0.0, 0.0).astype(np_t)
        specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], np_t)
        pick = rng.random(k) < 0.1
        out[pick] = specials[rng.integers(0, specials.size, int(pick.sum()))]
        return _force(rng, out, specials)
    raise ValueError(domain)


def shape_rows(rng, rows, vals, tname, frac=0.05):
    """Make about ``frac`` of the non-empty rows all NaN, as many all -0.0 and as many alternate +inf / -inf (floating point only;
    returns a new value array).  Under any multiply that reads the matrix value an all-NaN row has only NaN products; an all -0.0 row
    has -0.0 products under times with a positive operand value; the +inf / -inf row gives a NaN sum."""
    vals = np.array(vals, copy=True)
    if tname not in FP_TYPES or rows.size == 0:
        return vals
    np_t = O.NP_OF[tname]
    uniq = np.unique(rows)
    pick = rng.permutation(uniq)
    n = max(1, int(frac * uniq.size))
    for kind, sel in (("nan", pick[:n]), ("negzero", pick[n:2 * n]), ("infs", pick[2 * n:3 * n])):
        at = np.isin(rows, sel)
        if kind == "nan":
            vals[at] = np_t(np.nan)
        elif kind == "negzero":
            vals[at] = np_t(-0.0)
        else:
            idx = np.flatnonzero(at)
            vals[idx] = np.where(np.arange(idx.size) % 2 == 0, np.inf, -np.inf).astype(np_t)
    return vals


def _zero_sign_free(monoid):
    return monoid in ("min", "max", "any")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_fp(gv, ev, monoid=None, where=""):
    """Floating-point values equal as bit patterns; NaN matches NaN; a zero matches either zero under min / max / any."""
    gv, ev = np.asarray(gv), np.asarray(ev)
    assert gv.dtype == ev.dtype, (gv.dtype, ev.dtype, where)
    ok = _bits(gv) == _bits(ev)
    ok |= np.isnan(gv) & np.isnan(ev)
    if _zero_sign_free(monoid):
        ok |= (gv == 0) & (ev == 0)
    if not ok.all():
        bad = np.flatnonzero(~ok)[:8]
        raise AssertionError(f"{where}: {bad.size}+ values differ, positions {bad.tolist()}: got {gv[bad].tolist()} expected "
                             f"{ev[bad].tolist()}")


def same_values(got_idx, got_vals, exp_idx, exp_vals, monoid=None, where=""):
    """The strict comparator: the same indices, integer / BOOL values equal, floating-point values compared by ``same_fp``."""
    got_idx, exp_idx = np.asarray(got_idx), np.asarray(exp_idx)
    assert got_idx.tolist() == exp_idx.tolist(), (where, "patterns differ")
    gv, ev = np.asarray(got_vals), np.asarray(exp_vals)
    if ev.dtype.kind == "f":
        same_fp(gv.astype(ev.dtype, copy=False) if gv.dtype != ev.dtype else gv, ev, monoid, where)
    else:
        assert gv.dtype == ev.dtype, (where, gv.dtype, ev.dtype)
        assert gv.tolist() == ev.tolist(), (where, gv, ev)


def same_vec(got, exp, monoid=None, where=""):
    """A library Vector against an oracle OVec."""
    gi, gv = got.to_coo()
    same_values(gi, gv, exp.idx, exp.vals, monoid, where)


def same_mat(got, exp, monoid=None, where=""):
    """A library Matrix against an oracle OMat."""
    Cp, Cj, Cx = got.to_csr()
    assert np.asarray(Cp).astype(np.int64).tolist() == exp.indptr.tolist(), (where, "row pointers differ")
    same_values(np.asarray(Cj).astype(np.int64), Cx, exp.indices, exp.values, monoid, where)


PLUS_BOUND_C = 2.0
"""The scale factor of the error bound of a floating-point sum: |got - exact| <= PLUS_BOUND_C * n * eps * sum |products|.  Any order
of summation (left-to-right, a tree of lane partials, atomics in any order) stays within n * eps * sum |p| to first order; the factor
2 covers the second-order terms and the rounding of the products' own conversion."""


def plus_within_bound(got_idx, got_vals, A, u, mult, where=""):
    """Check an unmasked ``A (plus.mult) u`` of real floating-point values against the exact sums: the pattern must be exact; a row
    whose products hold a NaN, or +inf and -inf, must give NaN; a row with infinities of one sign must give that infinity; every
    other row must lie within the bound above of the exact sum (float64 sums of FP32 products, math.fsum for FP64).  A row whose
    sum of magnitudes exceeds the type's max may overflow in one order and not in another: there only the pattern is checked."""
    np_t = O.NP_OF[A.tname]
    eps = float(np.finfo(np_t).eps)
    big = float(np.finfo(np_t).max)
    u_has, u_val = u.dense()
    got = dict(zip(np.asarray(got_idx).tolist(), np.asarray(got_vals).tolist()))
    exp_rows = []
    for i in range(A.nrows):
        p0, p1 = int(A.indptr[i]), int(A.indptr[i + 1])
        cols = A.indices[p0:p1]
        keep = u_has[cols].astype(bool)
        if not keep.any():
            continue
        exp_rows.append(i)
        a, x = A.values[p0:p1][keep], u_val[cols[keep]]
        with np.errstate(all="ignore"):
            prod = {"times": a * x, "plus": a + x, "first": a, "second": x}[mult].astype(np_t)
        g = got.get(i)
        assert g is not None, (where, "row missing", i)
        if np.isnan(prod).any() or (np.isposinf(prod).any() and np.isneginf(prod).any()):
            assert math.isnan(g), (where, i, g)
            continue
        if np.isinf(prod).any():
            assert g == float(prod[np.isinf(prod)][0]), (where, i, g)
            continue
        absum = float(np.abs(prod.astype(np.float64)).sum())
        if absum > big:
            continue
        exact = math.fsum(prod.astype(np.float64).tolist())
        bound = PLUS_BOUND_C * prod.size * eps * absum
        assert math.isfinite(g) and abs(g - exact) <= bound, (where, i, g, exact, bound)
    assert sorted(got) == exp_rows, (where, "patterns differ")
