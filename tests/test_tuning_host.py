"""
The library's tuning switches and the launch shapes they decide (csrc/sp_tuning.cpp), without a GPU.

  * sp_debug_planned_shape -- what sp_lnlike_ensemble_planned launches for a plan of a given shape under given switches
    -- reproduces every row of tests/golden/planned_shape.json, recorded from the driver's inline logic as it stood
    before the switches had one table;
  * the parse rules: what every switch reads from the strings a user may put in its environment variable;
  * a process-wide setter followed by -1 is back at the environment's value.

The library reads the process-wide switches once, so every environment setting gets a fresh child process (which loads
the library alone: no torch, no device).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN
from starry_process_amd import _lib

# the table's order (csrc/sp_tuning.cpp): name, default, parse rule
SWITCHES = [
    ("SP_GROUPS", 1, "int"), ("SP_DEFER_NORM", 1, "int"), ("SP_LAZY_COV", 1, "int"), ("SP_PANEL_LA", 1, "int"),
    ("SP_PANEL_LAYOUT", 1, "int"), ("SP_FUSE_REDUCE", 1, "int"), ("SP_SUPER", 0, "min0"),
    ("SP_SMALL_K", 1, "onoff"), ("SP_PLAN_RIDING_LAZY", 1, "onoff"), ("SP_PLAN_PANEL_LAZY", 1, "onoff"),
    ("SP_PLAN_TEMPORAL_LAZY", 1, "onoff"), ("SP_PLAN_DIAG_LAZY", 1, "onoff"), ("SP_PLAN_FUSE0", 1, "onoff"),
    ("SP_SYRK_SYMDIAG", 1, "onoff"), ("SP_SYRK128_FROM", 17, "min0"), ("SP_ASM_TILES", 17, "min1"),
    ("SP_PLAN_TILES", 0, "int"),
]
# What a switch of each rule holds for the strings unset, "", "0", "1", "-3", "17", "abc" (D: its default).  By hand
# from the reads these rules replace: `e ? atoi(e) : D` (int; SP_SUPER and SP_SYRK128_FROM then `< 0 -> 0`, SP_ASM_TILES
# `< 1 -> 1`) and `!(e && atoi(e) == 0)` (on / off) -- atoi gives 0 for "" and "abc".
STRINGS = [None, "", "0", "1", "-3", "17", "abc"]
EXPECT = {
    "int": ["D", 0, 0, 1, -3, 17, 0],
    "min0": ["D", 0, 0, 1, 0, 17, 0],
    "min1": ["D", 1, 1, 1, 1, 17, 1],
    "onoff": [1, 0, 0, 1, 1, 1, 0],
}

CHILD = r"""
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
def values():
    out = (ctypes.c_int32 * 17)()
    assert L.sp_debug_tuning(out) == 0
    return list(out)
res = [values()]
for name, arg in json.loads(sys.argv[2]):
    fn = getattr(L, name)
    fn.argtypes = [ctypes.c_int]
    assert fn(arg) == 0
    res.append(values())
print(json.dumps(res))
"""


def child(env_switches, calls=()):
    """the switches' values in a fresh process with these variables set: at the start and after each setter call"""
    env = {k: v for k, v in os.environ.items() if k not in {n for n, _, _ in SWITCHES}}
    env.update(env_switches)
    import torch

    tl = os.path.join(os.path.dirname(torch.__file__), "lib")
    env["LD_LIBRARY_PATH"] = tl + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    out = subprocess.run([sys.executable, "-c", CHILD, _lib.LIB_PATH, json.dumps(list(calls))], check=True,
                         capture_output=True, text=True, env=env, timeout=120)
    return json.loads(out.stdout)


def test_planned_shape_reproduces_the_recorded_decisions():
    with open(os.path.join(GOLDEN, "planned_shape.json")) as f:
        fix = json.load(f)
    assert fix["switch_order"] == [n for n, _, _ in SWITCHES] and fix["defaults"] == [d for _, d, _ in SWITCHES]
    L = _lib.lib()
    rows = fix["rows"]
    assert len(rows) > 300
    seen_K, seen_t, seen_sw = set(), set(), set()
    for r in rows:
        # (a switch at its default is passed as -1: the library's own default must be the recorded one)
        sw = [r["switches"].get(n, -1) for n, _, _ in SWITCHES]
        a = np.array(r["in"] + sw, np.int32)
        o = np.full(13, -7, np.int32)
        assert L.sp_debug_planned_shape(_lib.hptr(a), _lib.hptr(o)) == 0
        assert o.tolist() == r["out"], (r, o.tolist())
        seen_K.add(r["in"][1])
        seen_t.add(r["in"][4])
        seen_sw.update(r["switches"])
    assert seen_K == {2, 63, 64, 65, 127, 128, 129, 200, 256, 512, 700, 960, 1000, 1024, 1345, 2488}
    assert seen_t == {0, 1, 2}
    assert seen_sw >= {n for n, _, rule in SWITCHES if rule == "onoff"} | {"SP_SUPER", "SP_LAZY_COV", "SP_FUSE_REDUCE"}
    bad = np.zeros(23, np.int32)
    assert L.sp_debug_planned_shape(None, _lib.hptr(o)) == -1 and L.sp_debug_planned_shape(_lib.hptr(bad), _lib.hptr(o)) == -1


SHAPE_OUT = ("lazy_nfull", "ncolw", "no_panels", "riding", "nrid", "dlazy", "dfrom", "fuse0", "use_ptab", "small_k",
             "superpanel", "fuses_reduce", "can_form_diag")


def planned_shape(ydeg, K, covpts, M=1, temporal=0, has_diag=0, **switches):
    """sp_debug_planned_shape's outputs by name, every switch at the library's default unless given"""
    assert set(switches) <= {n for n, _, _ in SWITCHES}
    a = np.array([ydeg, K, M, covpts, temporal, has_diag] + [switches.get(n, -1) for n, _, _ in SWITCHES], np.int32)
    o = np.full(len(SHAPE_OUT), -7, np.int32)
    assert _lib.lib().sp_debug_planned_shape(_lib.hptr(a), _lib.hptr(o)) == 0
    return dict(zip(SHAPE_OUT, o.tolist()))


def test_planned_shape_over_the_lag_grid_size():
    """The three decisions of sp_planned_shape that depend on covpts, each on either side of its threshold.  The
    thresholds are derived here from the documented budgets, in doubles, of a table of 4 (covpts + 4) coefficients:
      * the one-workgroup kernel keeps it in a region of 64 * BLD doubles, BLD = 66 the padded row of a 64 x 64 block
        (csrc/sp_internal.h, sp_small_k_serves);
      * the kernels that form tiles at first touch stage it, with a tile's 64 column phases behind it, in the smallest
        of their scratch areas, SP_TILE_LDS_MIN = 4544 doubles (csrc/sp_internal.h);
      * the stars' packed tables live in the design-matrix region, Kr * N doubles per star, Kr = K rounded up to 64
        and N = (ydeg + 1)^2."""
    nb, bld, tile_lds_min = 64, 66, 4544
    # small_k (K = 100 <= 128): 4 (covpts + 4) <= 64 BLD
    last = (64 * bld) // 4 - 4
    assert last == 1052
    for K in (100, 60):
        assert planned_shape(5, K, last)["small_k"] == 1 and planned_shape(5, K, last + 1)["small_k"] == 0
        assert planned_shape(5, K, last, SP_SMALL_K=0)["small_k"] == 0
    # tiles at first touch (K = 330, ydeg 5): 4 (covpts + 4) + 64 <= SP_TILE_LDS_MIN; the packed tables fit either way
    last = (tile_lds_min - 64) // 4 - 4
    assert last == 1116 and 4 * (last + 4) + 64 == tile_lds_min      # (full to the last double)
    K, N = 330, 36
    Kr, Kp = -(-K // nb) * nb, -(-(K + 1 + 2) // nb) * nb           # (the system: K cadences, one residual row, two of the normalisation)
    assert 4 * (last + 1 + 4) <= Kr * N
    a, b = planned_shape(5, K, last), planned_shape(5, K, last + 1)
    assert a["use_ptab"] == 1 and b["use_ptab"] == 1
    assert a["riding"] == 1 and a["lazy_nfull"] == Kp // nb == 6    # (every row tile, those of the riding rows included)
    assert b["riding"] == 0 and b["lazy_nfull"] == 0 and b["dlazy"] == 0
    assert planned_shape(5, K, 300)["lazy_nfull"] == 6 and planned_shape(5, K, last, SP_LAZY_COV=0)["lazy_nfull"] == 0
    # (with a temporal kernel the assembly writes the first super-panel of four block columns, the rest is formed)
    at = planned_shape(5, K, last, temporal=1)
    assert at["lazy_nfull"] == 6 and at["ncolw"] == 4 and at["no_panels"] == 1
    assert planned_shape(5, K, last + 1, temporal=1)["lazy_nfull"] == 0
    # packed tables (ydeg 5, K = 130): 4 (covpts + 4) <= Kr N
    K = 130
    Kr = -(-K // nb) * nb
    assert Kr * N == 6912
    last = (Kr * N) // 4 - 4
    assert last == 1724
    assert planned_shape(5, K, last)["use_ptab"] == 1 and planned_shape(5, K, last + 1)["use_ptab"] == 0
    # (ydeg 15 has room for both)
    assert planned_shape(15, K, last + 1)["use_ptab"] == 1


@pytest.mark.parametrize("k", range(len(STRINGS)))
def test_parse_rules(k):
    s = STRINGS[k]
    got = child({} if s is None else {n: s for n, _, _ in SWITCHES})[0]
    want = [d if EXPECT[rule][k] == "D" else EXPECT[rule][k] for _, d, rule in SWITCHES]
    assert got == want, (s, dict(zip([n for n, _, _ in SWITCHES], zip(got, want))))


def test_a_process_wide_setter_then_minus_one_is_the_environments_value():
    names = [n for n, _, _ in SWITCHES]
    i_small, i_sym, i_from = names.index("SP_SMALL_K"), names.index("SP_SYRK_SYMDIAG"), names.index("SP_SYRK128_FROM")
    calls = [("sp_debug_set_small_k", 1), ("sp_debug_set_small_k", -1), ("sp_debug_set_syrk_symdiag", 7),
             ("sp_debug_set_syrk_symdiag", -1), ("sp_debug_set_syrk128_from", 9), ("sp_debug_set_syrk128_from", 0),
             ("sp_debug_set_syrk128_from", -1)]
    for env, base in (({"SP_SMALL_K": "0", "SP_SYRK_SYMDIAG": "0", "SP_SYRK128_FROM": "5"}, (0, 0, 5)), ({}, (1, 1, 17))):
        v = child(env, calls if env else [(n, 0 if a > 0 else a) for n, a in calls])
        pick = [(r[i_small], r[i_sym], r[i_from]) for r in v]
        b = base
        if env:
            assert pick == [b, (1, b[1], b[2]), b, (b[0], 1, b[2]), b, (b[0], b[1], 9), (b[0], b[1], 0), b]
        else:
            assert pick == [b, (0, b[1], b[2]), b, (b[0], 0, b[2]), b, (b[0], b[1], 0), (b[0], b[1], 0), b]
        # (no setter touches another switch)
        others = [[x for i, x in enumerate(r) if i not in (i_small, i_sym, i_from)] for r in v]
        assert all(o == others[0] for o in others)
