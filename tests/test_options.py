"""The option table (python-graphblas_amd/csrc/grb_context.hip): GrX_option_set / GrX_option_get / GrX_options_reset and the derived
GRB_<NAME> environment names.  For every option: its current value is accepted, `get` returns what `set` stored, a rejected value
returns GrB_INVALID_VALUE and leaves the option alone, and the values that are clamped, snapped or floored are stored as the
if / else chain this table replaced stored them (the cases below are taken from that chain, one per distinct rule per option)."""
import ctypes
import os
import subprocess
import sys

import pytest

from tests.backend import DEVICES, EMU_SO, ROOT, bind

GrB_INVALID_VALUE = -3
P30, P40 = 1 << 30, 1 << 40


def any_int(name):  # stored in an int: the value is cast
    return name, [(7, 7), (-3, -3), ((1 << 32) + 5, 5)], []


def any_i64(name):
    return name, [(7, 7), (-3, -3), (P40 + 5, P40 + 5)], []


def clamp30(name):  # moved into [0, 2^30]
    return name, [(-5, 0), (12, 12), (P30, P30), (P30 + 1, P30), (P40, P30)], []


def floor0(name):  # a negative value becomes 0
    return name, [(-1, 0), (0, 0), (5, 5), (P40, P40)], []


def within(name, lo, hi):  # rejected outside [lo, hi]
    return name, [(lo, lo), (hi, hi)], [lo - 1, hi + 1, (1 << 32) + lo]


# (name, [(value given, value stored)], [values rejected])
OPTIONS = [
    ("debug_flags", [(0, 0), (128, 128), (256, 256), (2048, 2048), (65536, 65536), (128 | 256 | 2048 | 65536, 128 | 256 | 2048 | 65536),
                     ((1 << 32) + 128, 128)], [1, 4, 128 | 1, -1]),  # (the kernel ablation bits exist in -DGRB_ABLATE builds only)
    any_int("pull_ipt"), any_i64("hot_min_cols"), any_i64("hot_k"), any_int("push_mode"), any_i64("split_min_nnz"), clamp30("split_min_len"),
    ("short_kernel", [(0, 0), (1, 1), (5, 5), (6, 6)], [-1, 2, 3, 4, 7]),
    any_int("lazy_layout"), any_i64("lazy_min_nnz"), floor0("lean_min_nnz"), any_int("long_kernel"),
    ("long_classes", [(8, 8), (16, 16), (32, 32), (64, 64), (12, 8), (0, 8), (128, 8), (-1, 8)], []),
    ("long_sub", [(-1, 0), (0, 0), (3, 3), (16, 16), (17, 16), (P40, 16)], []),
    any_int("long_sub_min_len"), any_int("mxm_mask_mode"), within("mat_write_kernel", 0, 1), any_int("mxm_heavy_kernel"), any_int("drop_hot_cols"),
    any_i64("mxm_unit_min_flops"), any_i64("mxm_unit_min_per_window"), any_i64("mxm_masked_units_min_flops"),
    within("mxm_unit_small", 1, P30), within("mxm_unit_mid", 1, P30), within("mxm_unit_dense", 1, P30), within("mxm_sym_windows", 1, 64),
    ("mxm_window_groups", [(0, 0), (1, 1), (2, 2), (4, 4), (8, 8)], [-1, 3, 5, 6, 7, 9, 16]),
    within("mxm_xcd_map", 0, 1), within("mxm_checksum_pass", 0, 1), any_i64("mxm_bitmap_pool_mb"), any_int("mxm_bitmap_min_cnt"),
    any_i64("mxm_bitmap_pool_cap"), any_i64("vec_pad_min_bytes"), clamp30("hub_min_len"), within("fill_absent", 0, 1), within("rows_tile", 0, 2),
    within("lazy_tagged", 0, 1), within("ctile_pack", 0, 2), within("strip_slot16", 0, 1), within("rtile_pack", 0, 1), clamp30("cold_in_rows"),
    floor0("stream_nt_min_nnz"), within("bool_probe", 0, 16),
    ("rtile_rows", [(8192, 8192), (16384, 16384)], [0, 8191, 12288, 32768]),
    within("rtile_entries", 256, 1 << 24), within("rows_head", 0, 1), floor0("rows_head_min_groups"), within("push_small", 0, 1),
    within("value_dict", 0, 1), within("order_mode", 0, 1), floor0("order_min_nnz"),
    ("alloc_cache", [(0, 0), (1, 1), (5, 5)], []),  # (0 releases the block cache on the way)
]
NAMES = [o[0] for o in OPTIONS]
UNKNOWN = ("mxv_overlap", "strip_wgs", "no_such_option", "", "Pull_ipt")  # (the first two were options once)


@pytest.fixture(params=DEVICES)
def L(request):
    bind(request.param)
    from graphblas_amd import _lib

    yield _lib.lib
    assert _lib.lib.GrX_options_reset() == 0


def get(L, name):
    v = ctypes.c_int64(-12345)
    assert L.GrX_option_get(name.encode(), ctypes.byref(v)) == 0, name
    return v.value


def test_the_table_lists_every_option_once():
    assert len(NAMES) == len(set(NAMES)) == 52


@pytest.mark.parametrize("name,stored,rejected", OPTIONS, ids=NAMES)
def test_set_get_and_rules(L, name, stored, rejected):
    first = get(L, name)
    assert L.GrX_option_set(name.encode(), first) == 0 and get(L, name) == first  # (the default, or the environment's value, is a valid value)
    for given, kept in stored:
        assert L.GrX_option_set(name.encode(), given) == 0, (name, given)
        assert get(L, name) == kept, (name, given)
        for bad in rejected:
            assert L.GrX_option_set(name.encode(), bad) == GrB_INVALID_VALUE, (name, bad)
            assert get(L, name) == kept, (name, bad)
    assert L.GrX_options_reset() == 0 and get(L, name) == first


def test_unknown_names_and_null_pointers(L):
    before = {n: get(L, n) for n in NAMES}
    v = ctypes.c_int64(77)
    for name in UNKNOWN:
        assert L.GrX_option_set(name.encode(), 1) == GrB_INVALID_VALUE, name
        assert L.GrX_option_get(name.encode(), ctypes.byref(v)) == GrB_INVALID_VALUE and v.value == 77, name
    assert L.GrX_option_set(None, 1) == -2 and L.GrX_option_get(None, ctypes.byref(v)) == -2 and L.GrX_option_get(b"hot_k", None) == -2  # GrB_NULL_POINTER
    assert {n: get(L, n) for n in NAMES} == before


def test_reset_returns_every_option_to_its_initial_value(L):
    assert L.GrX_options_reset() == 0
    first = {n: get(L, n) for n in NAMES}
    for name, stored, _ in OPTIONS:
        for given, kept in stored:
            if kept != first[name]:
                assert L.GrX_option_set(name.encode(), given) == 0
                break
    changed = [n for n in NAMES if get(L, n) != first[n]]
    assert len(changed) == len(NAMES), sorted(set(NAMES) - set(changed))
    assert L.GrX_options_reset() == 0
    assert {n: get(L, n) for n in NAMES} == first
    assert L.GrX_options_reset() == 0 and {n: get(L, n) for n in NAMES} == first  # (twice is once)


_ENV_CHILD = """
import ctypes, sys
import graphblas_amd as gb
from graphblas_amd import _lib
gb.init(**({"lib_path": sys.argv[1]} if sys.argv[1] else {}))
def get(name):
    v = ctypes.c_int64()
    assert _lib.lib.GrX_option_get(name, ctypes.byref(v)) == 0
    return v.value
got = [get(n) for n in (b"split_min_nnz", b"lazy_min_nnz", b"vec_pad_min_bytes", b"mxm_masked_units_min_flops", b"mxm_bitmap_pool_cap",
                        b"hot_k", b"long_classes", b"short_kernel", b"debug_flags")]
assert got == [11, 12, 13, 14, 15, 16, 8, 6, 128], got
assert _lib.lib.GrX_option_set(b"hot_k", 99) == 0 and _lib.lib.GrX_options_reset() == 0 and get(b"hot_k") == 16  # (reset: the environment's value)
print("env ok")
"""


@pytest.mark.parametrize("dev", DEVICES)
def test_every_option_has_its_environment_name(dev):
    """GRB_<NAME> is derived from the option's name: the five options that had none before are read too, a rejected value leaves the default
    (with a line on stderr), GRB_DEBUG_FLAGS drops unknown bits instead, and GrX_options_reset returns to what the environment set."""
    if dev == "emu":
        bind("emu")  # (builds the emulator library when it is stale; a process bound to the GPU library skips)
    env = dict(os.environ, GRB_SPLIT_MIN_NNZ="11", GRB_LAZY_MIN_NNZ="12", GRB_VEC_PAD_MIN_BYTES="13", GRB_MXM_MASKED_UNITS_MIN_FLOPS="14",
               GRB_MXM_BITMAP_POOL_CAP="15", GRB_HOT_K="16", GRB_LONG_CLASSES="12", GRB_SHORT_KERNEL="3", GRB_DEBUG_FLAGS="129", GRB_EMU_PREBUILT="1",
               PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, "-c", _ENV_CHILD, EMU_SO if dev == "emu" else ""], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "env ok" in r.stdout, (r.stdout, r.stderr)
    assert 'GRB_SHORT_KERNEL=3 rejected (not a valid value of option "short_kernel")' in r.stderr, r.stderr
