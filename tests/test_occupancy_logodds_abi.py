"""CPU checks of log-odds grid sets (ABI 0.7.14): the seven symbols and two structs are declared by include/lsm2d_logodds.h (the extension of lsm2d.h), bound by the Python mirror and laid out
as gcc lays them out; the new kernels are in the library's code object beside the old ones; the mirrors exist and the new C++ sources compile.
occupancy_logodds_cases.reference -- what the GPU tests hold the device to -- is pinned to what is pinned already: for every case and two grid sizes the
counts references run on each scan ALONE give H_s = hits > 0 and M_s = misses > 0 and not H_s, the clamped votes applied in numpy in list order, and value
and observed agree bit for bit.  Then what the cases claim, the decay, and lsm2d_logodds_render_table (host only: it runs here) against its definition."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import abi_checks
import cpp_build
import occupancy_logodds_cases as lc
import occupancy_scan_cases as sc
from conftest import ROOT
from srrg2_laser_slam_2d_amd import api

W, H = lc.W, lc.H
P = lc.PARAMS
SCAN_CASES = lc.scan_cases()
CLOUD_CASES = lc.cloud_cases()
SYMBOLS = {"lsm2d_gridset_create_logodds": 5, "lsm2d_gridset_set_logodds": 2, "lsm2d_gridset_upload_logodds": 4, "lsm2d_gridset_download_logodds": 4,
           "lsm2d_occupancy_decay": 5, "lsm2d_logodds_render_table": 2, "lsm2d_occupancy_render_logodds": 5}


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_structs_declared_bound_and_exported():
    base, header = abi_checks.header(), abi_checks.header("lsm2d_logodds.h")
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = abi_checks.bound_symbols("LOGODDS_SYMBOLS")
    assert sorted(bound) == sorted(set(re.findall(r"\b(lsm2d_[a-z0-9_]+)\s*\(", plain))) == sorted(SYMBOLS)      # the extension declares these seven and no other
    assert not set(bound) & set(abi_checks.bound_symbols()) and '#include "lsm2d.h"' in header and "lsm2d_logodds.h" in base
    for name, n_args in SYMBOLS.items():
        assert plain.count(name + "(") == 1, name
        abi_checks.assert_declared_bound_exported(name, n_args, "lsm2d_logodds.h", "LOGODDS_SYMBOLS")
    assert "} lsm2d_logodds_params;" in header and "} lsm2d_logodds_render_params;" in header
    assert "0.7.14" in base and "0.7.14" in header
    block = header[header.index("log-odds grid sets (0.7.14)"):header.index("} lsm2d_logodds_params;")]
    for text in ("item 17e", "items 17c / 17d", "ascending position", "the hit", "clamp((int64) value + l_hit, l_min, l_max)", "saturating", "keeps its bits",
                 "n calls of one scan each", "count rays, not votes", "2^20", "2^30", "THE TABLE IS THE DEFINITION", "ceil(log((j - 0.5) / (100.5 - j)) / unit)",
                 "no exponential", "k_occ_tiles_logodds", "k_occ_decay", "k_occ_render_logodds", "no grid mapper", "NOT BUILT", "asynchronous form",
                 "per-grid geometry", "per-scan sensor parameters", "several workgroups", "multi-echo", "once-per-scan rule for counts sets"):
        assert text in block, text
    # the two older NOT BUILT lists have moved on
    for start, end in (("occupancy grids on the device (0.7.12)", "#define LSM2D_OCCUPANCY_MAX_SIDE"), ("occupancy grids from raw scans (0.7.13)", "} lsm2d_occupancy_scan_params;")):
        old = base[base.index(start):base.index(end)]
        lst = old[old.index("NOT BUILT"):]
        assert "log-odds with decay;" not in lst and "once-per-scan rule for counts sets" in lst and "0.7.14" in lst, start


def test_struct_layouts_match_the_c_compiler(tmp_path):
    from srrg2_laser_slam_2d_amd import _capi
    structs = {"lsm2d_logodds_params": (_capi.LogOddsParamsC, 16), "lsm2d_logodds_render_params": (_capi.LogOddsRenderParamsC, 8)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsm2d_logodds.h"', 'int main(void) {']
    for cname, (st, _) in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('printf(" %s=%%zu", offsetof(%s, %s));' % (fname, cname, fname))
        lines.append('printf("\\n");')
    lines += ['return 0; }']
    src = tmp_path / "layout.c"; src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines():
        parts = line.split(); st, size = structs[parts[0]]
        assert int(parts[1]) == C.sizeof(st) == size, parts[0]
        for kv in parts[2:]:
            k, v = kv.split("=")
            assert getattr(st, k).offset == int(v), (parts[0], k)
    assert [f.name for f in dataclasses.fields(api.LogOddsParams)] == ["l_hit", "l_miss", "l_min", "l_max"]
    p = api.LogOddsParams(85, -40, -200, 350).struct()
    assert (p.l_hit, p.l_miss, p.l_min, p.l_max) == (85, -40, -200, 350)


def test_kernels_are_in_the_code_object_beside_the_old_ones():
    abi_checks.assert_kernels_in_code_object((b"k_occ_tiles_logoddsILb0EE", b"k_occ_tiles_logoddsILb1EE", b"k_occ_decay", b"k_occ_render_logodds", b"k_occ_tilesILb0EE",
                                              b"k_occ_tilesILb1EE", b"k_occ_put"))
    csrc = os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "csrc")
    src = open(os.path.join(csrc, "lsm2d_k_occupancy.h")).read()
    assert src.index("void k_occ_tiles_logodds(") > src.index("void k_occ_put(")      # the new kernels come LAST
    for text in ("void k_occ_decay(", "void k_occ_render_logodds(", "__ballot(keep)"):
        assert text in src, text
    inc = open(os.path.join(csrc, "lsm2d_capi_occupancy.inc")).read()
    for name in SYMBOLS:
        assert 'extern "C" int %s(' % name in inc, name


def test_mirrors_exist():
    abi_checks.assert_mirrors_have(("occupancy_render_logodds", "logodds_values", "logodds_render_table"),
                                   ("struct LogOddsParams", "lsm2d_gridset_create_logodds(", "setLogOdds(", "uploadLogOdds(", "downloadLogOdds(", "occupancyDecay(",
                                    "occupancyRenderLogOdds(", "lsm2d_occupancy_decay(", "lsm2d_occupancy_render_logodds("), "lsm2d_occupancy.hpp")
    for m in ("set_logodds", "upload_logodds", "download_logodds", "decay"):
        assert callable(getattr(api.GridSet, m)), m


@pytest.mark.parametrize("source", ["occupancy_logodds_ref.cpp", "occupancy_logodds_driver.cpp", "occupancy_logodds_bench.cpp"])
def test_cpp_sources_compile(source):
    r = cpp_build.syntax_only(source)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the restatement is pinned to the counts references ------------------------------------------------------------------------------------------------------
def _pin(case, w, h, params=P, value=None, observed=None):
    gv, go = lc.reference(case, w, h, params, value, observed)
    wv, wo = lc.pinned(case, w, h, params, value, observed)
    assert gv.dtype == np.int32 and go.dtype == np.uint32
    assert gv.tobytes() == wv.tobytes(), np.argwhere(gv != wv)[:5].tolist()
    assert go.tobytes() == wo.tobytes(), np.argwhere(go != wo)[:5].tolist()
    return gv, go


@pytest.mark.parametrize("size", [(W, H), (65, 63)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(SCAN_CASES))
def test_reference_is_the_votes_of_the_scans_references_one_scan_at_a_time(name, size):
    _pin(SCAN_CASES[name], *size)


@pytest.mark.parametrize("size", [(W, H), (65, 63)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(CLOUD_CASES))
def test_reference_is_the_votes_of_the_clouds_references_one_input_at_a_time(name, size):
    _pin(CLOUD_CASES[name], *size)


def test_reference_over_uploaded_cells_and_with_tight_clamps():
    rng = np.random.default_rng(3)
    case = SCAN_CASES["random"]
    value = rng.integers(-400, 400, (2, H, W)).astype(np.int32); observed = rng.integers(0, 9, (2, H, W)).astype(np.uint32)
    _pin(case, W, H, P, value, observed)
    _pin(case, W, H, api.LogOddsParams(1, -1, 0, 0), value, observed)                            # both clamps at zero: every voted cell reads 0
    _pin(case, W, H, api.LogOddsParams(1 << 20, -(1 << 20), -(1 << 30), 1 << 30), value, observed)      # the widest parameters
    _pin(lc.order_case(300), 64, 64, lc.ORDER_PARAMS)


# ---- what the cases claim ------------------------------------------------------------------------------------------------------------------------------------
def test_own_cell_gets_one_vote_however_many_beams_cross_it():
    for case, own in ((SCAN_CASES["fan"], P.l_miss), (SCAN_CASES["fan_with_returns"], P.l_miss)):
        h, m = sc.reference(case, W, H)[:2]
        assert m[0, 31, 33] > 800 and h[0, 31, 33] == 0      # every live beam crosses the sensor's own cell ...
        v, o = lc.reference(case, W, H)
        assert v[0, 31, 33] == own and o[0, 31, 33] == 1      # ... and it gets ONE vote
        assert o.max() == 1 and set(np.unique(v).tolist()) <= {0, P.l_hit, P.l_miss}
        assert ((o == 0) == ((h[0] == 0) & (m[0] == 0))).all()


def test_a_cell_hit_and_crossed_in_one_scan_gets_l_hit():
    case = SCAN_CASES["sheaf"]
    rays, kind, _ = sc.case_rays(case)
    assert (kind[0, 0::2] == sc.HIT).all() and (kind[0, 1::2] == sc.CLEAR).all()      # a CLEAR beam beside every HIT beam
    h, m = sc.reference(case, W, H)[:2]
    both = (h[0] > 0) & (m[0] > 0)
    assert both.sum() >= 1 and both[30, 30] and m[0, 30, 30] >= 1000      # the end cell of the returns, crossed by the thousand beams without one
    v, o = lc.reference(case, W, H)
    assert (v[0][both] == P.l_hit).all() and (o[0][both] == 1).all()
    assert (v[0][(m[0] > 0) & ~both] == P.l_miss).all()
    # and across scans of a case with HIT rays only: a cloud's end cell crossed by another ray of the same input
    cv, co = lc.reference(CLOUD_CASES["random"], W, H)
    ch, cm = lc.oc.reference(CLOUD_CASES["random"], W, H)[:2]
    assert ((ch > 0) & (cm > 0)).sum() > 50 and (co <= np.bincount(lc.grids_of(CLOUD_CASES["random"]), minlength=2)[:, None, None]).all() and cv.max() > 0


def test_clamps_uploads_and_saturation_on_single_cells():
    value, observed, checks, hit, miss = lc.stress_start()
    case = lc.fan_with_returns_case()
    v, o = _pin(case, W, H, P, value[None], observed[None])
    assert len(checks) == 64
    seen = set()
    for what, (y, x), want_v, want_o in checks:
        assert v[0, y, x] == want_v and o[0, y, x] == want_o, (what, int(v[0, y, x]), want_v, int(o[0, y, x]), want_o)
        seen.add(want_v)
    # the clamps reached exactly, exceeded by one (pulled in), missed by one, at both ends; values far outside pulled in; INT32 ends do not wrap
    assert {P.l_max, P.l_max - 1, P.l_min, P.l_min + 1, P.l_hit, P.l_miss} <= seen
    wants = {w: (a, b) for w, _, a, b in checks}
    assert wants["hit cell, INT32_MAX, observed 0"] == (P.l_max, 1) and wants["hit cell, INT32_MIN, observed 0"] == (P.l_min, 1)
    assert wants["miss cell, INT32_MIN, observed 0"] == (P.l_min, 1) and wants["miss cell, INT32_MAX, observed 0"] == (P.l_max, 1)
    assert wants["hit cell, far below, observed 5"] == (P.l_min, 6) and wants["miss cell, far above, observed 5"] == (P.l_max, 6)
    assert wants["hit cell, zero, observed %d" % (lc.U32_MAX - 1)][1] == lc.U32_MAX and wants["hit cell, zero, observed %d" % lc.U32_MAX][1] == lc.U32_MAX
    rest = ~(hit | miss)
    assert rest.sum() > 1000 and (v[0][rest] == value[rest]).all() and (o[0][rest] == observed[rest]).all()      # every other cell keeps its bits
    # observed from 2^32 - 2 over three scans: 2^32 - 1 and no further
    v3, o3 = lc.reference(lc.repeat_case(3), W, H, P, value[None], observed[None])
    y, x = np.argwhere(hit & (observed == lc.U32_MAX - 1))[0]
    assert o3[0, y, x] == lc.U32_MAX


def test_repeated_scan_has_the_known_answer():
    hit, miss = lc.scan_sets(lc.fan_with_returns_case(), W, H)[0]
    assert hit.sum() > 100 and miss.sum() > 500
    for n in (1, 2, 40):
        v, o = lc.reference(lc.repeat_case(n), W, H)
        assert (v[0][hit] == min(n * P.l_hit, P.l_max)).all() and (v[0][miss] == max(n * P.l_miss, P.l_min)).all()
        assert (o[0][hit | miss] == n).all() and not v[0][~(hit | miss)].any() and not o[0][~(hit | miss)].any()


def test_one_call_over_n_scans_equals_n_calls_of_one_scan():
    for case in (SCAN_CASES["random"], SCAN_CASES["interleaved"], CLOUD_CASES["random"]):
        want = lc.reference(case, W, H)
        scans, grids = lc.scan_list(case), lc.grids_of(case)
        v = o = None
        for k in range(len(scans)):
            v, o = lc.reference_of(scans[k:k + 1], grids[k:k + 1], case["n_grids"], W, H, P, v, o)
        assert v.tobytes() == want[0].tobytes() and o.tobytes() == want[1].tobytes()
    # the order matters once a clamp is met: the reversed list gives another grid
    a = lc.reference(lc.order_case(6), 64, 64, lc.ORDER_PARAMS)[0]
    b = lc.reference(lc.order_case(6, reverse=True), 64, 64, lc.ORDER_PARAMS)[0]
    x, y = lc.HIT_CELL
    assert a[0, y, x] != b[0, y, x]


def test_order_cases_are_decided_by_the_last_scan():
    x, y = lc.HIT_CELL
    p = lc.ORDER_PARAMS
    assert p.l_max == p.l_hit and p.l_min == p.l_miss
    for n in (256, 300):
        for reverse in (False, True):
            case = lc.order_case(n, reverse)
            sets = lc.scan_sets(case, 64, 64)
            assert all(s[0][y, x] != s[1][y, x] for s in sets)      # every scan votes on the cell: a hit or a miss
            last_is_hit = bool(sets[-1][0][y, x])
            assert last_is_hit == reverse      # (scan n - 1 is odd: it clears; reversed, the list ends with scan 0, which hits)
            v, o = lc.reference(case, 64, 64, p)
            assert v[0, y, x] == (p.l_hit if last_is_hit else p.l_hit + p.l_miss) and o[0, y, x] == n
        far = lc.order_case(n, far_every_third=True)
        sets = lc.scan_sets(far, 64, 64)
        assert sum(1 for s in sets if not s[0].any() and not s[1].any()) == n // 3      # every third scan misses the tile altogether
        assert lc.reference(far, 64, 64, p)[1][0, y, x] == n - n // 3


def test_interleaved_grids_and_a_dropped_scan_between_two_live_ones():
    case = SCAN_CASES["interleaved"]
    assert case["grids"].tolist() == [0, 1, 0, 1, 2, 1, 0]
    v, o = lc.reference(case, W, H)
    assert all(1 <= int(o[g].max()) <= n for g, n in enumerate((3, 3, 1))) and all(v[g].any() for g in range(3))
    case = SCAN_CASES["dropped_between"]
    _, kind, _ = sc.case_rays(case)
    assert (kind[1] == sc.DROPPED).all() and (kind[0] != sc.DROPPED).all() and (kind[2] != sc.DROPPED).all() and case["n_grids"] == 1
    two = dict(case); two["ranges"] = case["ranges"][[0, 2]]; two["poses"] = case["poses"][[0, 2]]
    a, b = lc.reference(case, W, H), lc.reference(two, W, H)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and 1 <= a[1].max() <= 2
    # the edge case ends where it says
    rays, kind, _ = sc.case_rays(SCAN_CASES["edge"])
    assert [tuple(int(c) for c in rays[k, 2, 2:]) for k in range(4)] == [(63, 10), (64, 12), (5, 63), (6, 64)] and (kind[:, 2] == sc.HIT).all()


def test_decay():
    value = np.array([[-7, -3, -1, 0, 1, 3, 7, lc.I32_MAX, lc.I32_MIN, 5, -5, 9]], np.int32)
    observed = np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, lc.U32_MAX]], np.uint32)
    assert lc.decay(value, observed, 0).tolist() == value.tolist()
    assert lc.decay(value, observed, 3).tolist() == [[-4, 0, 0, 0, 0, 0, 4, lc.I32_MAX - 3, lc.I32_MIN + 3, 5, -5, 6]]      # toward zero, never past it; unknown cells stay
    assert lc.decay(value, observed, lc.I32_MAX).tolist() == [[0, 0, 0, 0, 0, 0, 0, 0, -1, 5, -5, 0]]


# ---- the render table ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit", [0.01, 0.125, 1.0])
def test_render_table_is_its_definition(unit):
    t = api.logodds_render_table(unit).astype(np.int64)
    assert len(t) == 100 and (np.diff(t) >= 0).all()
    u = float(np.float32(unit))
    j = np.arange(1, 101, dtype=np.float64)
    x = np.log((j - 0.5) / (100.5 - j))
    assert t.tolist() == np.ceil(x / u).astype(np.int64).tolist()
    for jj in range(1, 101):      # threshold 101 - j mirrors threshold j
        assert t[100 - jj] == -np.floor(x[jj - 1] / u), jj
    one = lambda v: int(api.logodds_values(np.array([v], np.int32), np.array([1], np.uint32), unit)[0])      # noqa: E731
    assert one(0) == 50 and one(lc.I32_MAX) == 100 and one(lc.I32_MIN) == 0
    v = np.arange(int(t[0]) - 50, int(t[-1]) + 51, dtype=np.int64)
    away = np.abs(v[:, None] - t[None, :]).min(1) >= 2
    assert away.sum() > 20
    got = api.logodds_values(v[away].astype(np.int32), np.ones(int(away.sum()), np.uint32), unit)
    want = np.round(100.0 / (1.0 + np.exp(-u * v[away].astype(np.float64))))
    assert got.tolist() == want.astype(np.int64).tolist()
    # min_scans: unknown below it, never below one
    vals = api.logodds_values(np.zeros(4, np.int32), np.array([0, 1, 2, 3], np.uint32), unit, 2)
    assert vals.tolist() == [-1, -1, 50, 50] and api.logodds_values(np.zeros(2, np.int32), np.array([0, 1], np.uint32), unit, 0).tolist() == [-1, 50]


def test_render_table_refuses_a_bad_unit():
    for unit in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(api.Lsm2dError):
            api.logodds_render_table(unit)
    from srrg2_laser_slam_2d_amd import _capi
    assert _capi.load().lsm2d_logodds_render_table(C.c_float(1.0), None) == _capi.BAD_ARGUMENT
