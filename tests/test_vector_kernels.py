"""The vector kernels of python-graphblas_amd/csrc/grb_vecops.hip past one workgroup, against the oracle and plain numpy, on both
tiers (the HIP library on the GPU, the same kernel sources under the CPU wave64 emulator).

``k_reduce`` gives one thread one 64-bit presence word: a wavefront covers 4096 elements, a 256-thread workgroup 16384, the grid is
capped at 4 workgroups per compute unit.  The cases below put values where each stage of the kernel has to carry them -- a high lane
of the shuffle tree, wavefronts 1..3 of the LDS combine, a second / third / last workgroup of the cross-workgroup atomic, the second
trip of the grid-stride loop -- and choose the values so that a dropped lane, wavefront or workgroup changes the answer (distinct
powers of two under plus, distinct primes under times, the extreme moved through every position under min / max, one True / one
False moved through every position under lor / land / lxor / lxnor).

The element-wise kernels: the comparison operators (``k_ewise_cmp``) in every type at the presence-word boundaries, operands and an
output of three different types (the ``cast_array`` branches of ``ewise_core``), ``GrB_Vector_reduce_<T>`` with a monoid of another
type than the vector (the ``cast_buf`` branch and the host-side accumulator of ``reduce_to``), and indexed assign / extract with
index lists that cross a workgroup and crowd into a few presence words.

Every expected value is the oracle or numpy, never a second call into the library.  Integers and BOOL compare exactly; floating-point
values as bit patterns through ``tests.values.same_fp`` (NaN matches NaN; under min / max / any a zero matches a zero of either
sign).  The one tolerance is the floating-point ``times`` fold, whose rounding depends on the order: rtol 1e-5 (FP32) / 1e-12 (FP64),
the bound tests/test_random_parity.py::test_vector_assign_reduce_random uses for the same fold."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import grb_oracle as O
from tests.backend import DEVICES, ROOT, bind
from tests.values import ALL_TYPES, FP_TYPES, INT_TYPES, rand_vals, same_fp, same_vec

NP_OF = O.NP_OF
WORD, WAVE, WG = 64, 4096, 16384  # elements per presence word (one thread), per wavefront, per 256-thread workgroup
N3 = 3 * WG + 65  # three whole workgroups and a fourth of two words, the last word holding ONE element
BOUNDARY_SIZES = (4095, 4096, 4097, 16383, 16384, 16385, N3)


@pytest.fixture(params=DEVICES)
def gb(request):
    return bind(request.param)


def monoids_of(tname):
    return ("lor", "land", "lxor", "lxnor") if tname == "BOOL" else ("plus", "times", "min", "max")


def reduce_value(gb, v, mon):
    return v.reduce(getattr(gb.monoid, mon)).new().value


def check_scalar(got, ref, tname, mon, where):
    """One reduced value against its reference: integers / BOOL exactly, floating point through ``same_fp``."""
    assert got is not None, (where, "empty result", ref)
    if tname in FP_TYPES:
        same_fp(np.array([got], NP_OF[tname]), np.array([ref], NP_OF[tname]), mon, where)
    else:
        assert got == ref and type(got) is type(ref), (where, got, ref)


def check_reduce(gb, tname, n, pos, vals, mon, where):
    """``reduce(mon)`` of the vector holding ``vals`` at ``pos`` against the oracle's fold."""
    vals = np.asarray(vals, NP_OF[tname])
    v = gb.Vector.from_coo(pos, vals, dtype=tname, size=n)
    check_scalar(reduce_value(gb, v, mon), O.vec_reduce(O.OVec(n, pos, vals, tname), mon), tname, mon, where)


# ---- 1. k_reduce, stage by stage ---------------------------------------------------------------------------------------------
def elems(words):
    """One element in each presence word of ``words``, at a bit that differs from word to word."""
    return np.array([WORD * g + (7 * g + 3) % WORD for g in words], np.int64)


PLACED = [  # (name, n, positions)
    ("lanes", WAVE, elems([0, 31, 32, 63])),  # every shuffle distance of wavefront 0
    ("wavefronts 1-3", WG, elems([64, 128, 192, 255])),  # wavefront 0 empty: the first-taker branch of the LDS combine
    ("wavefronts 0-3", WG, elems([0, 64, 128, 192])),
    ("workgroups 0-2", N3, elems([5, 256 + 17, 512 + 200])),
    ("last workgroup", N3, np.array([768 * WORD + 3, 768 * WORD + 40, N3 - 1], np.int64)),
    ("partial last word", N3, np.array([N3 - 1], np.int64)),
    ("last element 4097", 4097, np.array([4096], np.int64)),
    ("last element 16385", 16385, np.array([16384], np.int64)),
]


def placed_values(tname, mon, k):
    """The value sets of one monoid over ``k`` placed entries: (name, values).  Every position changes the answer."""
    np_t = NP_OF[tname]
    if tname == "BOOL":
        if mon in ("lor", "lxor"):  # one True moved through every position (an odd count for lxor), and none
            out = [(f"true at {p}", np.arange(k) == p) for p in range(k)] + [("all false", np.zeros(k, bool))]
            if mon == "lxor":
                odd = np.ones(k, bool)
                odd[: (k + 1) % 2] = False  # (an odd number of True)
                out.append(("odd count", odd))
            return out
        return [(f"false at {p}", np.arange(k) != p) for p in range(k)] + [("all true", np.ones(k, bool))]
    if mon == "plus":
        out = [("powers of two", (1 << np.arange(k)).astype(np_t))]
        if tname in INT_TYPES:  # 2^(bits-2) + 2^i each: with three or four of them the sum leaves the type and wraps as numpy's does
            out.append(("wrapping", ((1 << (np.iinfo(np_t).bits - 2)) + (1 << np.arange(k))).astype(np_t)))
        return out
    if mon == "times":
        return [("primes", np.array([2, 3, 5, 7][:k], np_t))]
    signed = tname in FP_TYPES or np.iinfo(np_t).min < 0
    out = []
    for p in range(k):  # the extreme at position p
        x = (50 + 10 * np.arange(k)).astype(np_t)
        x[p] = np_t((-3 if signed else 3) if mon == "min" else 120)
        out.append((f"extreme at {p}", x))
    return out


@pytest.mark.parametrize("tname", ALL_TYPES)
def test_reduce_placed_entries(gb, tname):
    """A handful of entries at chosen presence words: the lanes {0, 31, 32, 63} of wavefront 0; one wavefront each, with and without
    wavefront 0; one workgroup each; the last workgroup alone; the partial last word alone; the last element of n = 4097 / 16385.
    Every monoid of the type, and ``any``, whose result must be one of the stored values."""
    for name, n, pos in PLACED:
        for mon in monoids_of(tname):
            for vname, vals in placed_values(tname, mon, pos.size):
                check_reduce(gb, tname, n, pos, vals, mon, (tname, name, mon, vname))
        stored = [np.ones(pos.size, bool), np.zeros(pos.size, bool)] if tname == "BOOL" else [(10 + np.arange(pos.size)).astype(NP_OF[tname])]
        for vals in stored:
            got = reduce_value(gb, gb.Vector.from_coo(pos, vals, dtype=tname, size=n), "any")
            assert got is not None and got in vals.tolist(), (tname, name, "any", got, vals)


# ---- 2. seeds and NaN across workgroups --------------------------------------------------------------------------------------
PER_WG = np.array([WG * w + 64 * (9 + 50 * w) + 11 * w + 1 for w in range(3)] + [N3 - 2], np.int64)  # one element in each of the 4 workgroups


@pytest.mark.parametrize("tname", FP_TYPES)
def test_reduce_seeds_and_nan_across_workgroups(gb, tname):
    """The accumulator seeds (-0.0 for plus, NaN for min / max) against the partials of four workgroups: a sum of -0.0 alone keeps
    its sign; NaN alone gives NaN; NaN in some workgroups and finite values in ONE other give the finite extreme (the NaN slot is
    replaced exactly once); +inf and -inf in different workgroups."""
    np_t = NP_OF[tname]
    nan, inf = np_t(np.nan), np_t(np.inf)
    v = gb.Vector.from_coo(PER_WG, np.full(4, -0.0, np_t), dtype=tname, size=N3)
    z = reduce_value(gb, v, "plus")
    assert z == 0 and np.signbit(z), (tname, "sum of -0.0", z)
    check_reduce(gb, tname, N3, PER_WG, np.full(4, -0.0, np_t), "plus", (tname, "sum of -0.0"))
    for mon in ("min", "max"):
        got = reduce_value(gb, gb.Vector.from_coo(PER_WG, np.full(4, nan), dtype=tname, size=N3), mon)
        assert got is not None and np.isnan(got), (tname, mon, "NaN in every workgroup", got)
    finite = np.array([5, -7, 3, 0.5], np_t)
    in_wg = lambda w, whole, last: WG * w + np.array(last if w == 3 else whole, np.int64)  # (workgroup 3 holds 65 elements)
    for where_finite, nan_wgs in ((1, (0, 2)), (3, (0, 2)), (3, (0, 1, 2)), (0, (1, 2, 3)), (2, (0, 1, 3))):
        fpos = in_wg(where_finite, [70, WAVE + 5, 9000, WG - 1], [1, 30, 63, 64])
        npos = np.concatenate([in_wg(w, [77, WAVE + 130], [5, 62]) for w in nan_wgs])
        pos = np.concatenate([fpos, npos])
        vals = np.concatenate([finite, np.full(npos.size, nan)])
        for mon, want in (("min", -7.0), ("max", 5.0)):
            got = reduce_value(gb, gb.Vector.from_coo(pos, vals, dtype=tname, size=N3), mon)
            assert got == want, (tname, mon, "finite in workgroup", where_finite, "NaN in", nan_wgs, got)
            check_reduce(gb, tname, N3, pos, vals, mon, (tname, mon, where_finite, nan_wgs))
    for order in ((inf, -inf, np_t(1), np_t(2)), (np_t(1), inf, np_t(2), -inf), (-inf, np_t(3), inf, np_t(4))):
        vals = np.array(order, np_t)
        u = gb.Vector.from_coo(PER_WG, vals, dtype=tname, size=N3)
        assert np.isnan(reduce_value(gb, u, "plus")), (tname, "+inf + -inf", order)
        assert reduce_value(gb, u, "min") == -inf and reduce_value(gb, u, "max") == inf, (tname, order)
        for mon in ("plus", "min", "max"):
            check_reduce(gb, tname, N3, PER_WG, vals, mon, (tname, mon, order))


@pytest.mark.parametrize("tname", ["INT64", "UINT64"])
def test_reduce_full_range_64_bit_across_workgroups(gb, tname):
    """The 64-bit atomics go through ``unsigned long long`` / ``long long``: values over the whole range (above 2^63 for UINT64), one
    per workgroup with the extreme in every workgroup in turn, and forty of the 'signed' domain spread over all four workgroups."""
    np_t = NP_OF[tname]
    info = np.iinfo(np_t)
    base = [info.max, info.min, 3, (1 << 63) + 5 if tname == "UINT64" else -5]
    for rot in range(4):
        vals = np.array(base[rot:] + base[:rot], np_t)
        for mon in ("min", "max", "plus"):
            check_reduce(gb, tname, N3, PER_WG, vals, mon, (tname, mon, "rotation", rot))
    if tname == "UINT64":  # every value above 2^63: a signed comparison would order them as negatives
        vals = np.array([(1 << 63) + 9, (1 << 64) - 2, (1 << 63), (1 << 63) + 70], np_t)
        for mon in ("min", "max", "plus"):
            check_reduce(gb, tname, N3, PER_WG, vals, mon, (tname, mon, "above 2^63"))
    rng = np.random.default_rng(2100 + ALL_TYPES.index(tname))
    for seed in range(3):
        pos = np.unique(np.concatenate([rng.integers(0, N3, 36), PER_WG]))
        vals = rand_vals(rng, pos.size, tname, "signed")
        for mon in ("min", "max", "plus"):
            check_reduce(gb, tname, N3, pos, vals, mon, (tname, mon, "signed domain", seed))


# ---- 3. random reduce at the boundary sizes ----------------------------------------------------------------------------------
def random_values(rng, k, tname, finite):
    """'exact' for floating point (its sums do not depend on the order), with the non-finite values replaced by small integers when
    ``finite``; the whole range for the integers."""
    if tname not in FP_TYPES:
        return np.asarray(rand_vals(rng, k, tname, "signed"))
    x = np.asarray(rand_vals(rng, k, tname, "exact"))
    if finite:
        x = np.where(np.isfinite(x), x, rng.integers(-8, 9, k).astype(x.dtype))
    return x


@pytest.mark.parametrize("tname", ALL_TYPES)
def test_reduce_random_at_boundary_sizes(gb, tname):
    """n at 4096 / 16384 +- 1 and at three workgroups and a partial one; half full and with about 64 entries (a sparse frontier).
    Floating point in the 'exact' domain (NaN, +-inf, signed zeros) and in its finite part, so plus / min / max compare bit for bit;
    ``times`` over about 40 entries (floating point: 1..8, the product stays finite, within the rtol of the module docstring; integers:
    odd values of the whole range, whose product wraps and is never zero)."""
    rng = np.random.default_rng(3100 + ALL_TYPES.index(tname))
    fp = tname in FP_TYPES
    for n in BOUNDARY_SIZES:
        for dens in (0.5, 64.0 / n):
            for finite in ((False, True) if fp else (False,)):
                pos = np.unique(np.concatenate([np.flatnonzero(rng.random(n) < dens), [n - 1]]))
                vals = random_values(rng, pos.size, tname, finite)
                ou = O.OVec(n, pos, vals, tname)
                v = gb.Vector.from_coo(pos, vals, dtype=tname, size=n)
                for mon in monoids_of(tname):
                    if mon == "times" and fp:
                        continue
                    check_scalar(reduce_value(gb, v, mon), O.vec_reduce(ou, mon), tname, mon, (tname, n, dens, finite, mon))
        if tname == "BOOL":
            continue
        pos = np.unique(np.concatenate([rng.integers(0, n, 38), [0, n - 1]]))
        vals = rng.integers(1, 9, pos.size).astype(NP_OF[tname]) if fp else np.asarray(rand_vals(rng, pos.size, tname, "signed")) | NP_OF[tname](1)
        got = reduce_value(gb, gb.Vector.from_coo(pos, vals, dtype=tname, size=n), "times")
        ref = O.vec_reduce(O.OVec(n, pos, vals, tname), "times")
        if fp:
            assert np.isfinite(ref) and np.isclose(got, ref, rtol=1e-5 if tname == "FP32" else 1e-12, atol=0), (tname, n, "times", got, ref)
        else:
            assert got == ref and ref != 0, (tname, n, "times", got, ref)


def test_matrix_reduce_scalar_past_one_workgroup(gb):
    """``Matrix.reduce_scalar`` ends in the vector reduce of the row results: 16385 rows are two workgroups of it, the second holding
    the last row alone.  Against numpy over the entries."""
    rng = np.random.default_rng(3200)
    m, n = 16385, 5
    for tname in ("INT64", "FP64"):
        flat = np.unique(np.concatenate([rng.integers(0, m * n, 9000), [0, (m - 1) * n + 2]]))
        r, c = flat // n, flat % n
        x = rng.integers(-50, 51, flat.size).astype(NP_OF[tname])
        x[-1] = 1 << 20  # (the last row: the largest value and a bit of the sum no other entry sets)
        x[0] = -(1 << 21)
        A = gb.Matrix.from_coo(r, c, x, dtype=tname, nrows=m, ncols=n)
        for mon, ref in (("plus", x.sum()), ("max", x.max()), ("min", x.min())):
            got = A.reduce_scalar(getattr(gb.monoid, mon)).new().value
            assert got == ref.item() and type(got) is type(ref.item()), (tname, mon, got, ref)


def test_vector_isequal_past_one_workgroup(gb):
    """``Vector.isequal`` is ``ewise_mult(eq)`` and ``reduce(land)``: two vectors of size 16385 that differ in ONE element -- the only
    element of workgroup 1, the last lane of a wavefront, the first of the next -- are not equal; the same vectors are."""
    rng = np.random.default_rng(3300)
    n = 16385
    for tname in ("INT32", "FP32", "BOOL"):
        x = np.asarray(rand_vals(rng, n, tname, "small"))
        a = gb.Vector.from_coo(np.arange(n), x, dtype=tname, size=n)
        assert a.isequal(gb.Vector.from_coo(np.arange(n), x, dtype=tname, size=n)), tname
        for at in (n - 1, 0, WAVE - 1, WAVE, WG - 1, 3 * WAVE + 17):
            y = x.copy()
            y[at] = (not y[at]) if tname == "BOOL" else y[at] + 1
            assert not a.isequal(gb.Vector.from_coo(np.arange(n), y, dtype=tname, size=n)), (tname, "differs at", at)


# ---- 4. the grid-stride loop -------------------------------------------------------------------------------------------------
def compute_units():
    """The number of compute units the bound library sizes its grids by: the device's on the GPU tier, the emulator's constant (the
    value its ``hipDeviceGetAttribute`` returns) on the CPU tier."""
    import tests.backend as backend

    if backend._bound == "gpu":
        import torch

        return int(torch.cuda.get_device_properties(0).multi_processor_count)
    with open(os.path.join(ROOT, "tests", "emu", "hip", "hip_runtime.h")) as f:
        found = re.search(r"hipDeviceGetAttribute\([^)]*\)\s*\{\s*\*v\s*=\s*(\d+)\s*;", f.read())
    assert found, "the emulator's compute-unit count was not found in tests/emu/hip/hip_runtime.h"
    return int(found.group(1))


@pytest.mark.parametrize("tname", ["INT32", "FP32"])
def test_reduce_grid_stride_second_trip(gb, tname):
    """The grid is capped at 4 workgroups per compute unit, so the loop of ``k_reduce`` takes a second trip only when the vector has
    more than 256 * 4 * num_cus presence words.  A sparse vector six words past that: a few hundred entries in the first trip, some
    in the words of the second trip -- among them the smallest value, the largest one and a bit of the sum that no other entry sets
    -- and one in the last, partial word."""
    cap_words = 256 * 4 * compute_units()
    n = (cap_words + 5) * WORD + 1
    nwords = (n + 63) >> 6
    assert nwords > cap_words and n - 1 == (nwords - 1) * WORD, (n, nwords, cap_words)  # a second trip, and a last word of one element
    rng = np.random.default_rng(4100)
    np_t = NP_OF[tname]
    first = np.unique(np.concatenate([rng.integers(0, cap_words * WORD, 300), np.arange(6) * WORD + 9]))  # (words 0..5: the threads that come back)
    second = np.array([cap_words * WORD + 2, (cap_words + 1) * WORD + 63, (cap_words + 3) * WORD + 31, (cap_words + 4) * WORD, n - 1], np.int64)
    pos = np.concatenate([first, second])
    vals = np.concatenate([rng.integers(-100, 101, first.size), [-1000, 1 << 12, 1 << 13, 1000, 1 << 14]]).astype(np_t)
    v = gb.Vector.from_coo(pos, vals, dtype=tname, size=n)
    for mon, ref in (("plus", vals.astype(np.int64).sum()), ("min", -1000), ("max", 1 << 14)):
        check_scalar(reduce_value(gb, v, mon), np_t(ref).item(), tname, mon, (tname, n, mon))


# ---- 5a. comparison operators ------------------------------------------------------------------------------------------------
CMP = {"eq": np.equal, "ne": np.not_equal, "gt": np.greater, "lt": np.less, "ge": np.greater_equal, "le": np.less_equal}


def dense_of(n, idx, vals, np_t):
    has, val = np.zeros(n, bool), np.zeros(n, np_t)
    has[idx], val[idx] = True, vals
    return has, val


def write_rule(ow, t_has, t_val, om, comp, struct, accum, replace):
    """The oracle's ``grbo_vec_write``: w<mask, replace> = accum(w, T) with T dense and already in w's type."""
    n, wt = ow.size, ow.tname
    w_has, w_val = ow.dense()
    mt = O._dense_mask(om, struct, n)
    t_val = np.ascontiguousarray(t_val, NP_OF[wt])
    rc = O.lib().grbo_vec_write(O.TYPE_CODES[wt], ctypes.c_int64(n), O._p(w_has), O._p(w_val), O._p(np.ascontiguousarray(t_has, np.uint8)),
                                O._p(t_val), O._p(mt), int(comp and om is not None), O.OP_CODES[accum] if accum else -1,
                                int(replace and om is not None))
    assert rc == 0
    return O.OVec.from_dense(w_has, w_val, wt)


def ocast(x, tname):
    with np.errstate(all="ignore"):
        return np.asarray(O.cast(np.asarray(x), tname))


@pytest.mark.parametrize("tname", ALL_TYPES)
def test_ewise_comparison_operators(gb, tname):
    """``ewise_mult`` / ``ewise_add`` with eq, ne, gt, lt, ge, le at n = 63, 64, 65, 257 against numpy: the comparison on the
    intersection, a single entry of ``ewise_add`` passed through as ``x != 0``.  Floating point in the 'special' domain (NaN compares
    false except under ne, -0.0 equals +0.0), with equal pairs, NaN pairs and zeros of both signs forced in.  The result as a BOOL
    vector, and cast into an INT32 output under a mask with ``accum=plus``."""
    rng = np.random.default_rng(5100 + ALL_TYPES.index(tname))
    np_t = NP_OF[tname]
    dom = "special" if tname in FP_TYPES else ("signed" if tname != "BOOL" else "small")
    for n in (63, 64, 65, 257):
        ui = np.unique(np.concatenate([np.flatnonzero(rng.random(n) < 0.6), [0, 1, 2, n - 1]]))
        vi = np.unique(np.concatenate([np.flatnonzero(rng.random(n) < 0.6), [0, 1, 2, n - 1]]))
        uv, vv = np.asarray(rand_vals(rng, ui.size, tname, dom)), np.asarray(rand_vals(rng, vi.size, tname, dom))
        hu, du = dense_of(n, ui, uv, np_t)
        hv, dv = dense_of(n, vi, vv, np_t)
        same = np.flatnonzero(hu & hv)[::3]  # a third of the common entries hold equal values
        dv[same] = du[same]
        if tname in FP_TYPES:
            du[0], dv[0] = np.nan, np.nan
            du[1], dv[1] = -0.0, 0.0
            du[2], dv[2] = np.nan, 1.0
        uv, vv = du[ui], dv[vi]
        U = gb.Vector.from_coo(ui, uv, dtype=tname, size=n)
        V = gb.Vector.from_coo(vi, vv, dtype=tname, size=n)
        wi = np.flatnonzero(rng.random(n) < 0.5)
        wv = rng.integers(-5, 6, wi.size).astype(np.int32)
        mi = np.flatnonzero(rng.random(n) < 0.6)
        mv = rng.integers(0, 2, mi.size).astype(np.int8)
        ow, om = O.OVec(n, wi, wv, "INT32"), O.OVec(n, mi, mv, "INT8")
        M = gb.Vector.from_coo(mi, mv, dtype="INT8", size=n)
        for k, (opname, f) in enumerate(CMP.items()):
            with np.errstate(invalid="ignore"):
                both = f(du, dv)
            for is_add in (False, True):
                t_has = (hu | hv) if is_add else (hu & hv)
                t_val = np.where(hu & hv, both, np.where(hu, du != 0, dv != 0)) & t_has
                where = (tname, n, opname, "add" if is_add else "mult")
                op = getattr(gb.binary, opname)
                expr = (lambda: U.ewise_add(V, op)) if is_add else (lambda: U.ewise_mult(V, op))
                got = expr().new()
                assert got.dtype.name == "BOOL" and got.size == n, where
                same_vec(got, O.OVec.from_dense(t_has, t_val, "BOOL"), None, where)
                comp, struct, repl = bool(k & 1), bool(k & 2), is_add
                W = gb.Vector.from_coo(wi, wv, dtype="INT32", size=n)
                mm = M.S if struct else M.V
                W(~mm if comp else mm, accum=gb.binary.plus, replace=repl) << expr()
                same_vec(W, write_rule(ow, t_has, t_val.astype(np.int32), om, comp, struct, "plus", repl), None, (where, "into INT32"))


# ---- 5b. operands and output of three different types ------------------------------------------------------------------------
TRIPLES = [  # (u, v, w): signed / unsigned pairs, integer / floating-point pairs, a floating-point result into INT8 (saturates, NaN -> 0)
    ("INT8", "UINT8", "INT32"), ("UINT16", "INT16", "UINT64"), ("INT32", "UINT32", "INT8"), ("INT64", "UINT64", "FP32"),
    ("INT32", "FP32", "FP64"), ("FP64", "INT16", "INT8"), ("FP32", "UINT8", "INT8"), ("UINT64", "FP64", "INT64"),
    ("BOOL", "INT8", "FP32"), ("FP32", "FP64", "UINT16"), ("INT16", "INT64", "BOOL"), ("UINT8", "BOOL", "INT16"),
]
MIXED_OPS = ("plus", "times", "min", "max", "minus", "first", "second")


@pytest.mark.parametrize("seed", range(len(TRIPLES)))
def test_ewise_mixed_types(gb, seed):
    """``w(mask, accum, replace) << u.ewise_add / ewise_mult(v, op)`` with u, v and w of three different types: the operands are cast
    to the operator's type (the unified type of u and v), the result to w's.  Expected: ``O.vec_ewise`` in the unified type, the
    oracle's cast to w's type, ``grbo_vec_write``.  No mask, value / structural masks and their complements; accumulators and none;
    replace on and off.  Arithmetic operators of a floating-point type draw from the 'exact' domain (a single operation on NaN, +-inf
    and small integers is the same everywhere), min / max / first / second from 'special', integers from their whole range."""
    ut, vt, wt = TRIPLES[seed]
    rng = np.random.default_rng(5200 + seed)
    n = (257, 300, 129, 65)[seed % 4]
    wi = np.flatnonzero(rng.random(n) < 0.4)
    wv = np.asarray(rand_vals(rng, wi.size, wt, "small"))
    mi = np.flatnonzero(rng.random(n) < 0.6)
    mv = rng.integers(0, 3, mi.size).astype(np.int8)
    ow, om = O.OVec(n, wi, wv, wt), O.OVec(n, mi, mv, "INT8")
    M = gb.Vector.from_coo(mi, mv, dtype="INT8", size=n)
    accums = (None, "lor", "second", "land") if wt == "BOOL" else (None, "plus", "min", "second")
    k = 0
    for opname in MIXED_OPS:
        def draw(t):
            idx = np.unique(np.concatenate([np.flatnonzero(rng.random(n) < 0.5), [0, n - 1]]))
            dom = "small" if t == "BOOL" else ("signed" if t not in FP_TYPES else ("exact" if opname in ("plus", "times", "minus") else "special"))
            return idx, np.asarray(rand_vals(rng, idx.size, t, dom))

        (ui, uv), (vi, vv) = draw(ut), draw(vt)
        U = gb.Vector.from_coo(ui, uv, dtype=ut, size=n)
        V = gb.Vector.from_coo(vi, vv, dtype=vt, size=n)
        ou, ov = O.OVec(n, ui, uv, ut), O.OVec(n, vi, vv, vt)
        op = getattr(gb.binary, opname)
        for is_add in (True, False):
            with np.errstate(all="ignore"):
                t = O.vec_ewise(ou, ov, opname, union=is_add)
            assert t.tname == O.unify(ut, vt)
            t_has, t_val = dense_of(n, t.idx, ocast(t.vals, wt), NP_OF[wt])
            for mname in ("none", "V", "S", "~V", "~S"):
                for repl in ((False,) if mname == "none" else (False, True)):
                    accum = accums[k % 4]
                    k += 1
                    W = gb.Vector.from_coo(wi, wv, dtype=wt, size=n)
                    kw = {} if accum is None else {"accum": getattr(gb.binary, accum)}
                    if mname != "none":
                        mm = M.S if "S" in mname else M.V
                        kw.update(mask=~mm if "~" in mname else mm, replace=repl)
                    W(**kw) << (U.ewise_add(V, op) if is_add else U.ewise_mult(V, op))
                    exp = write_rule(ow, t_has, t_val, None if mname == "none" else om, "~" in mname, "S" in mname, accum, repl)
                    zero_free = "min" if opname in ("min", "max") or accum == "min" else None
                    same_vec(W, exp, zero_free, (ut, vt, wt, opname, "add" if is_add else "mult", mname, accum, repl))


# ---- 5c. reduce in a monoid type other than the vector's ---------------------------------------------------------------------
CT = {"BOOL": ctypes.c_bool, "INT8": ctypes.c_int8, "INT16": ctypes.c_int16, "INT32": ctypes.c_int32, "INT64": ctypes.c_int64,
      "UINT8": ctypes.c_uint8, "UINT16": ctypes.c_uint16, "UINT32": ctypes.c_uint32, "UINT64": ctypes.c_uint64, "FP32": ctypes.c_float,
      "FP64": ctypes.c_double}


def raw_reduce(gb, out_t, start, accum, accum_t, mon, mon_t, v):
    """``GrB_Vector_reduce_<out_t>(&val, accum, monoid, v)`` through the bound library, ``val`` holding ``start`` before the call."""
    from graphblas_amd import _lib

    out = CT[out_t](start)
    acc = None if accum is None else ctypes.c_void_p(getattr(gb.binary, accum)[accum_t]._carg)
    rc = getattr(_lib.lib, f"GrB_Vector_reduce_{out_t}")(ctypes.byref(out), acc, ctypes.c_void_p(getattr(gb.monoid, mon)[mon_t]._carg), v._handle, None)
    assert rc == 0, (rc, out_t, mon, mon_t)
    return NP_OF[out_t](out.value)


def host_accum(start, t, accum, accum_t, out_t):
    """val = accum(val, t) in the accumulator's type, cast back to the scalar's (the C API's rule for a scalar output)."""
    if accum is None:
        return NP_OF[out_t](t)
    a, b = ocast(np.array([start], NP_OF[out_t]), accum_t), ocast(np.array([t], NP_OF[out_t]), accum_t)
    with np.errstate(all="ignore"):
        z = np.asarray(O._NP_BINOP[accum](a, b)).astype(NP_OF[accum_t])
    return ocast(z, out_t)[0]


def test_reduce_in_another_monoid_type(gb):
    """The values are cast to the MONOID's type before the fold: an INT8 vector under an INT64 plus does not wrap; an FP64 vector under
    an INT32 min / max saturates (NaN -> 0).  Over 16385 elements (two workgroups of the cast copy), without an accumulator and with
    one into a scalar that holds a value, in the scalar's type and in another."""
    rng = np.random.default_rng(5300)
    n = 16385
    pos = np.unique(np.concatenate([np.flatnonzero(rng.random(n) < 0.5), [0, n - 1]]))
    x8 = rng.integers(90, 128, pos.size).astype(np.int8)  # (thousands of them: far beyond INT8, and beyond INT16 and INT32's wrap of it)
    v8 = gb.Vector.from_coo(pos, x8, dtype="INT8", size=n)
    total = int(x8.astype(np.int64).sum())
    assert total > 1 << 17 and total != int(x8.sum(dtype=np.int8))
    for out_t, start, accum, accum_t in (("INT64", 0, None, None), ("INT64", 1000, "plus", "INT64"), ("INT64", 77, "min", "INT64"),
                                         ("INT64", -9, "second", "INT64"), ("FP32", 0.5, "plus", "FP32"), ("INT64", 1 << 40, "plus", "FP64"),
                                         ("INT32", 5, "plus", "INT8")):
        got = raw_reduce(gb, out_t, start, accum, accum_t, "plus", "INT64", v8)
        ref = host_accum(start, ocast(np.array([total], np.int64), out_t)[0], accum, accum_t, out_t)
        assert got == ref and got.dtype == ref.dtype, ("INT8 under INT64 plus", out_t, start, accum, accum_t, got, ref)
    # ... and the same vector under the INT8 monoid wraps, as numpy's INT8 sum does
    assert raw_reduce(gb, "INT8", 0, None, None, "plus", "INT8", v8) == x8.sum(dtype=np.int8)
    sets = {"huge": [1e30, -1e30, 3.7, np.nan], "nan and negatives": [np.nan, -5.5, -1e30, -2.5], "fractions": [-0.75, 0.25, 7.99, -7.99],
            "infinities": [np.inf, -np.inf, np.nan, 12.0]}
    for name, specials in sets.items():
        x = rng.integers(-1000, -10, pos.size).astype(np.float64) if name == "nan and negatives" else rng.integers(-6, 7, pos.size).astype(np.float64)
        at = np.array([0, pos.size // 2, pos.size - 2, pos.size - 1])  # (the first and the last element among them: both workgroups)
        x[at] = specials
        v = gb.Vector.from_coo(pos, x, dtype="FP64", size=n)
        as32 = ocast(x, "INT32")
        for mon, fold in (("max", as32.max()), ("min", as32.min()), ("plus", as32.sum(dtype=np.int32))):
            for start, accum, accum_t in ((0, None, None), (41, "max", "INT32"), (-(1 << 31), "plus", "INT32"), (100, "times", "FP64")):
                got = raw_reduce(gb, "INT32", start, accum, accum_t, mon, "INT32", v)
                ref = host_accum(start, fold, accum, accum_t, "INT32")
                assert got == ref and got.dtype == ref.dtype, ("FP64 under INT32", name, mon, start, accum, accum_t, got, ref)


# ---- 5d. indexed assign and extract ------------------------------------------------------------------------------------------
def index_lists(rng, n, ni):
    """(name, I): ``ni`` distinct indices spread over the vector with its first and last element and both sides of the workgroup
    boundary among them; and a shuffled run of ``ni`` consecutive indices around that boundary (every presence word it touches is
    updated by up to 64 lanes at once)."""
    forced = np.array([0, n - 1, WG - 1, WG - 2])
    spread = rng.permutation(np.concatenate([forced, np.setdiff1d(rng.choice(n, ni, replace=False), forced)[: ni - forced.size]]))
    lo = n - ni  # (the run ends in the vector's last element: the partial last word, the only one of workgroup 1)
    return [("spread", spread.astype(np.int64)), ("clustered", rng.permutation(np.arange(lo, lo + ni)).astype(np.int64))]


ASSIGN_TYPES = [("INT32", "INT32"), ("FP64", "INT8"), ("BOOL", "BOOL"), ("UINT16", "INT64"), ("FP32", "FP32"), ("INT8", "FP64")]


@pytest.mark.parametrize("wt,st", ASSIGN_TYPES)
@pytest.mark.parametrize("ni", [255, 256, 257])
def test_indexed_assign_and_extract_past_one_workgroup(gb, ni, wt, st):
    """``w(mask, accum, replace)[I] << u``, ``... << scalar`` and ``x << u[J]`` with 255 / 256 / 257 indices (one workgroup of the
    scatter, and one element more) into a vector of 16385, spread and clustered.  u lacks entries: without an accumulator an absent
    u(k) deletes w(I[k]).  No duplicate indices in assign; extract repeats some.  The aliased form ``w[I] << w`` with I a
    permutation.  Against ``O.vec_assign`` / ``O.vec_extract``; w of type ``wt``, u of type ``st`` (cast on the way in)."""
    rng = np.random.default_rng(5400 + 16 * ni + ASSIGN_TYPES.index((wt, st)))
    n = 16385
    with np.errstate(all="ignore"):  # (the oracle's numpy restatement adds NaN and infinities of the 'exact' domain)
        dom = lambda t: "small" if t == "BOOL" else ("exact" if t in FP_TYPES else "signed")
        for lname, I in index_lists(rng, n, ni):
            wi = np.unique(np.concatenate([np.flatnonzero(rng.random(n) < 0.5), I[::2]]))
            wv = np.asarray(rand_vals(rng, wi.size, wt, dom(wt)))
            ui = np.flatnonzero(rng.random(ni) < 0.6)
            uv = np.asarray(rand_vals(rng, ui.size, st, dom(st)))
            mi = np.flatnonzero(rng.random(n) < 0.5)
            mv = rng.random(mi.size) < 0.5
            ow, ou, om = O.OVec(n, wi, wv, wt), O.OVec(ni, ui, uv, st), O.OVec(n, mi, mv, "BOOL")
            mk = gb.Vector.from_coo(mi, mv, dtype="BOOL", size=n)
            forms = [(None, False, False, False), (mk.V, False, False, False), (~mk.S, True, True, True)]
            for accum in ((None, "lor") if wt == "BOOL" else (None, "plus", "min")):
                for mask, comp, struct, repl in forms:
                    kw = dict(mask=om if mask is not None else None, mask_comp=comp, mask_struct=struct, accum=accum, replace=repl)
                    where = (ni, wt, st, lname, accum, comp, struct, repl)
                    zero_free = "min" if accum == "min" else None

                    def target(w):
                        return w(accum=accum) if mask is None else w(mask, accum=accum, replace=repl)

                    w = gb.Vector.from_coo(wi, wv, dtype=wt, size=n)
                    target(w)[I] << gb.Vector.from_coo(ui, uv, dtype=st, size=ni)
                    same_vec(w, O.vec_assign(ow, ou, I, **kw), zero_free, (where, "vector"))
                    w = gb.Vector.from_coo(wi, wv, dtype=wt, size=n)
                    s = np.asarray(rand_vals(rng, 1, wt, "small"))[0]
                    target(w)[I] << s
                    same_vec(w, O.vec_assign(ow, s, I, **kw), zero_free, (where, "scalar"))
                    # extract: x of size ni from a source of size n (in the source type `st`), some indices twice
                    J = I.copy()
                    J[rng.integers(0, ni, 20)] = I[rng.integers(0, ni, 20)]
                    xi = np.flatnonzero(rng.random(ni) < 0.5)
                    xv = np.asarray(rand_vals(rng, xi.size, wt, dom(wt)))
                    m2i = np.flatnonzero(rng.random(ni) < 0.5)
                    m2v = rng.random(m2i.size) < 0.5
                    sv = ocast(wv, st)
                    x = gb.Vector.from_coo(xi, xv, dtype=wt, size=ni)
                    src = gb.Vector.from_coo(wi, sv, dtype=st, size=n)
                    mk2 = gb.Vector.from_coo(m2i, m2v, dtype="BOOL", size=ni)
                    if mask is None:
                        x(accum=accum) << src[J]
                    else:
                        x(~mk2.S if comp else mk2.V, accum=accum, replace=repl) << src[J]
                    exp = O.vec_extract(O.OVec(ni, xi, xv, wt), O.OVec(n, wi, sv, st), J, mask=O.OVec(ni, m2i, m2v, "BOOL") if mask is not None else None,
                                        mask_comp=comp, mask_struct=struct, accum=accum, replace=repl)
                    same_vec(x, exp, zero_free, (where, "extract"))
        # w[P] << w with P a permutation of all of w's indices: the input is the output
        P = rng.permutation(ni).astype(np.int64)
        ai = np.flatnonzero(rng.random(ni) < 0.6)
        av = np.asarray(rand_vals(rng, ai.size, wt, dom(wt)))
        oa = O.OVec(ni, ai, av, wt)
        for accum in ((None, "lor") if wt == "BOOL" else (None, "plus")):
            a = gb.Vector.from_coo(ai, av, dtype=wt, size=ni)
            a(accum=accum)[P] << a
            same_vec(a, O.vec_assign(oa, oa, P, accum=accum), None, (ni, wt, "aliased", accum))
