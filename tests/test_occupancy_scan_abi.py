"""CPU checks of lsm2d_occupancy_update_scans (ABI 0.7.13): the symbol and its struct are declared by include/lsm2d.h, bound by the Python mirror and laid
out as gcc lays them out; the limits are 0.7.12's macros, reused; both new kernels are in the library's code object; the mirrors exist and the new C++
sources compile.  occupancy_scan_cases.reference -- what the GPU tests hold the device to -- is pinned to what is pinned already: over the clouds of its
HIT and of its CLEAR end points occupancy_cases.reference gives hits == H_hit and misses == M_hit + M_clear + H_clear, the counts likewise; its end points
are the oracle preprocessor's bit for bit.  Saturation on hand-made counts; and the cases the GPU tests run contain what they claim, asserted on the
reference's own classification."""
import ctypes as C
import dataclasses
import os
import re
import subprocess

import numpy as np
import pytest

import abi_checks
import cpp_build
import occupancy_cases as oc
import occupancy_scan_cases as sc
from conftest import ROOT
from srrg2_laser_slam_2d_amd import api

F32 = np.float32
W, H, T, CAP = sc.W, sc.H, oc.TILE, sc.CAP
CASES = sc.all_cases()
_RAYS = {}


def _rays(name):
    if name not in _RAYS:
        _RAYS[name] = sc.case_rays(CASES[name])
    return _RAYS[name]


# ---- the ABI -------------------------------------------------------------------------------------------------------------------------------------------------
def test_symbol_struct_and_macros_declared_bound_and_exported():
    name = "lsm2d_occupancy_update_scans"
    abi_checks.assert_declared_bound_exported(name, 10)
    header = abi_checks.header()
    assert re.sub(r"/\*.*?\*/", "", header, flags=re.S).count(name + "(") == 1      # ONE new symbol
    assert len([s for s in abi_checks.bound_symbols() if "occupancy" in s or "gridset" in s]) == 8      # 0.7.12's seven and this one
    assert "} lsm2d_occupancy_scan_params;" in header and header.index("lsm2d_occupancy_update_scans(") > header.index("int lsm2d_occupancy_render(")
    # the limits are 0.7.12's: no new macro, the number stays
    assert len(re.findall(r"#define LSM2D_OCCUPANCY_\w+", header)) == 4 and "LSM2D_VERSION 160" in header and "0.7.13" in header
    block = header[header.index("occupancy grids from raw scans (0.7.13)"):header.index("} lsm2d_occupancy_scan_params;")]
    for text in ("item 17d", "item 17c.1", "xf_point", "LSM2D_OCCUPANCY_MAX_RAYS", "LSM2D_OCCUPANCY_MAX_RAY_CELLS", "LSM2D_CAPACITY_EXCEEDED", "no grid mapper",
                 "NOT BUILT", "asynchronous form", "per-grid geometry", "once-per-scan", "several workgroups", "log-odds", "k_occ_beams", "k_occ_tiles<true>",
                 "TWO launches", "ONE copy down", "ONE wait"):
        assert text in block, text
    # 0.7.12's block says where the truncation and the clearing went
    old = header[header.index("occupancy grids on the device (0.7.12)"):header.index("#define LSM2D_OCCUPANCY_MAX_SIDE")]
    assert "maximum-range truncation" in old and "lsm2d_occupancy_update_scans" in old and "0.7.13" in old


def test_struct_layout_matches_the_c_compiler(tmp_path):
    from srrg2_laser_slam_2d_amd import _capi
    st = _capi.OccupancyScanParamsC
    assert [f for f, _ in st._fields_] == ["n_beams", "angle_min", "angle_max", "range_min", "range_max", "trace_range", "clear_no_return"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsm2d.h"', 'int main(void) {', 'printf("%zu", sizeof(lsm2d_occupancy_scan_params));']
    for fname, _ in st._fields_:
        lines.append('printf(" %s=%%zu:%%zu", offsetof(lsm2d_occupancy_scan_params, %s), sizeof(((lsm2d_occupancy_scan_params*) 0)->%s));' % (fname, fname, fname))
    lines += ['printf("\\n");', 'return 0; }']
    src = tmp_path / "layout.c"; src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    parts = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert int(parts[0]) == C.sizeof(st) == 28 and len(parts) == 8
    for kv in parts[1:]:
        k, v = kv.split("=")
        off, size = (int(x) for x in v.split(":"))
        assert getattr(st, k).offset == off and getattr(st, k).size == size == 4, k
    p = api.OccupancyScanParams(1081, -2.0, 2.5, 0.25, 30.0, 20.0, False).struct()
    assert (p.n_beams, p.angle_min, p.angle_max, p.range_min, p.range_max, p.trace_range, p.clear_no_return) == (1081, -2.0, 2.5, 0.25, 30.0, 20.0, 0)


def test_kernels_are_in_the_code_object_and_in_the_last_parts():
    abi_checks.assert_kernels_in_code_object((b"k_occ_beams", b"k_occ_tilesILb1EE", b"k_occ_rays", b"k_occ_tilesILb0EE"))
    csrc = os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "csrc")
    assert "void k_occ_beams(" in open(os.path.join(csrc, "lsm2d_k_occupancy.h")).read() and "void k_occ_tiles(" in open(os.path.join(csrc, "lsm2d_k_occupancy.h")).read()
    assert 'extern "C" int lsm2d_occupancy_update_scans(' in open(os.path.join(csrc, "lsm2d_capi_occupancy.inc")).read()


def test_mirrors_exist():
    abi_checks.assert_mirrors_have("occupancy_update_scans", ("struct OccupancyScanParams", "occupancyUpdateScans(", "lsm2d_occupancy_update_scans("), "lsm2d_occupancy.hpp")
    assert [f.name for f in dataclasses.fields(api.OccupancyScanParams)] == ["n_beams", "angle_min", "angle_max", "range_min", "range_max", "trace_range", "clear_no_return"]
    assert "lsm2d_occupancy" not in abi_checks.assert_mirrors_have((), ())


@pytest.mark.parametrize("source", ["occupancy_scan_ref.cpp", "occupancy_scan_driver.cpp", "occupancy_scan_bench.cpp"])
def test_cpp_sources_compile(source):
    r = cpp_build.syntax_only(source)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the reference is pinned to what is pinned already -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(W, H), (65, 63)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_is_occupancy_cases_reference_over_its_end_points(name, size):
    """hits == H_hit and misses == M_hit + M_clear + H_clear, where (H, M) is occupancy_cases.reference of the cloud of HIT end points and of the cloud of
    CLEAR end points alone: exact wherever no counter saturates (none does: every count here is far below 2^32)"""
    w, h = size
    case = CASES[name]
    hits, misses, n_hit, n_clear, n_drop = sc.reference(case, w, h)
    Hh, Mh, rays_h, drop_h = oc.reference(sc.clouds_of(case, sc.HIT), w, h)
    Hc, Mc, rays_c, drop_c = oc.reference(sc.clouds_of(case, sc.CLEAR), w, h)
    assert int(max(Hh.max(), Mh.max(), Hc.max(), Mc.max())) < 1 << 30
    assert hits.tobytes() == Hh.tobytes(), np.argwhere(hits != Hh)[:5].tolist()
    want_m = Mh + Mc + Hc
    assert misses.tobytes() == want_m.tobytes(), np.argwhere(misses != want_m)[:5].tolist()
    assert n_hit.tolist() == rays_h.tolist() and n_clear.tolist() == rays_c.tolist()
    # dropped: by the class, or by the cell tests (which occupancy_cases.reference counts)
    _, kind, cls = _rays(name)
    grids = np.zeros(len(case["ranges"]), np.int32) if case["grids"] is None else case["grids"]
    by_class = np.zeros(case["n_grids"], np.int64)
    for k, scan in enumerate(case["ranges"]):
        by_class[grids[k]] += int((sc.points(case["params"], scan)[1] == sc.DROPPED).sum())
    assert n_drop.tolist() == (by_class + drop_h + drop_c).tolist()
    beams = np.bincount(grids, minlength=case["n_grids"]) * case["params"].n_beams
    assert (n_hit + n_clear + n_drop).tolist() == beams.tolist()
    # and case_rays agrees with it
    for g in range(case["n_grids"]):
        assert int((kind[grids == g] == sc.HIT).sum()) == n_hit[g] and int((kind[grids == g] == sc.CLEAR).sum()) == n_clear[g]


def test_end_points_are_the_oracle_preprocessors_bit_for_bit(po):
    """a scan with every beam in class 1 or 2 and trace_range == range_max: the oracle's preprocessor at normal_min_points 1, voxelize_resolution 0 keeps
    every valid beam in beam order, and its points are l * dir.  (It keeps a beam whose window has a direction -- oracle/lsm2d_oracle.c:278 drops an
    isotropic window, a lone point among them --, so normal_point_distance is sc.WHOLE_SCAN: every window is the whole scan; the count is asserted.)"""
    cases = [CASES["returns_only"], sc.returns_only_case(seed=5, n_scans=2, n_beams=1081), sc.returns_only_case(seed=6, n_scans=2, n_beams=64)]
    for case in cases:
        prm = case["params"]
        assert prm.trace_range == prm.range_max
        pp = po.Preprocessor(prm.n_beams, prm.angle_min, prm.angle_max, prm.range_min, prm.range_max, sc.WHOLE_SCAN, 1, 0.0)
        for scan in case["ranges"]:
            cls, kind, xy = sc.points(prm, scan)
            assert set(cls.tolist()) <= {1, 2} and (cls == 2).sum() > prm.n_beams // 2 and (cls == 1).sum() > 0
            want = po.preprocess_scan(pp, scan)
            assert len(want) == int((kind == sc.HIT).sum())
            assert xy[kind == sc.HIT].tobytes() == np.ascontiguousarray(want[:, :2]).tobytes()


def test_reference_counts_by_hand_and_saturation():
    """four beams from cell (2, 1) of a 12 x 8 grid: a hit ray of 3 cells along +x, a clear ray of 4 cells along +y, two dropped, twice;
    then the same over counters at 2^32 - 2"""
    prm = sc.four_beams(0.25, 3.0, 2.0, True)
    case = sc._case(prm, [[sc.NAN, sc.NAN, 1.5, 2.5], [sc.NAN, sc.NAN, 1.5, sc.INF]], poses=[sc._sensor(2, 1), sc._sensor(2, 1)])
    h, m, n_hit, n_clear, n_drop = sc.reference(case, 12, 8)
    want_h = np.zeros((8, 12), np.uint32); want_m = np.zeros((8, 12), np.uint32)
    want_h[1, 5] = 2                                     # the hit rays' last cell
    want_m[1, 2:5] += 2                                  # ... and the cells before it
    want_m[1:6, 2] += 2                                  # the clear rays: EVERY cell, the last one too, and no hit
    assert np.array_equal(h[0], want_h) and np.array_equal(m[0], want_m), (h[0], m[0])
    assert (n_hit.tolist(), n_clear.tolist(), n_drop.tolist()) == ([2], [2], [4])
    full = np.full((1, 8, 12), 0xFFFFFFFE, np.uint32)
    h2, m2, _, _, _ = sc.reference(case, 12, 8, full, full)
    assert m2[0, 1, 2] == 0xFFFFFFFF and m2[0, 5, 2] == 0xFFFFFFFF and m2[0, 1, 3] == 0xFFFFFFFF and h2[0, 1, 5] == 0xFFFFFFFF and h2[0, 5, 2] == 0xFFFFFFFE
    assert m2[0, 0, 0] == 0xFFFFFFFE and m2[0, 2, 2] == 0xFFFFFFFF
    one = np.full((1, 8, 12), 0xFFFFFFFF, np.uint32)
    h3, m3, _, _, _ = sc.reference(case, 12, 8, one, one)
    assert h3.tobytes() == one.tobytes() and m3.tobytes() == one.tobytes()


# ---- the cases contain what they claim -----------------------------------------------------------------------------------------------------------------------
def test_cases_contain_what_they_claim():
    inside = lambda x, y: 0 <= x < W and 0 <= y < H      # noqa: E731
    # every class at its thresholds, one ulp either side; the non-finite values, zero, a negative range
    r, want_cls = sc.threshold_ranges()
    for name, clear in (("classes_clear", True), ("classes_drop", False)):
        case = CASES[name]
        assert case["params"].clear_no_return == clear and np.array_equal(case["ranges"][0], r, equal_nan=True) and np.array_equal(case["ranges"][1], r[::-1], equal_nan=True)
        cls, kind, _ = sc.points(case["params"], case["ranges"][0])
        assert cls.tolist() == want_cls.tolist()
        assert kind.tolist() == [{1: -1, 2: 0, 3: 1, 4: 1 if clear else -1}[c] for c in want_cls.tolist()]
        rays, kd, _ = _rays(name)
        assert np.array_equal(kd[0], kind) and np.array_equal(kd[1], kind[::-1])      # none dropped by the cell tests
    assert np.array_equal(CASES["classes_clear"]["ranges"], CASES["classes_drop"]["ranges"], equal_nan=True)      # the same scans at both settings
    up, down = F32(np.inf), F32(-np.inf)
    for v, c in ((sc.RMIN, 2), (np.nextafter(sc.RMIN, down), 1), (sc.TRACE, 2), (np.nextafter(sc.TRACE, up), 3), (sc.RMAX, 3), (np.nextafter(sc.RMAX, up), 4),
                 (sc.INF, 4), (-sc.INF, 1), (F32(0.0), 1), (F32(-1.0), 1)):
        assert want_cls[np.flatnonzero(r == v)[0]] == c, v
    assert want_cls[np.flatnonzero(np.isnan(r))[0]] == 1
    # trace_range == range_max: no class 3
    case = CASES["trace_is_max"]
    cls, _, _ = sc.points(case["params"], case["ranges"][0])
    assert case["params"].trace_range == case["params"].range_max and 3 not in cls.tolist() and {1, 2, 4} <= set(cls.tolist())
    # scans of clear rays only: hits stay 0 everywhere, the misses are there, in both grids
    rays, kind, cls = _rays("clear_only")
    assert (kind == sc.CLEAR).all() and {3, 4} == set(cls.ravel().tolist())
    h, m, n_hit, n_clear, n_drop = sc.reference(CASES["clear_only"], W, H)
    assert not h.any() and m[0].sum() > 100 and m[1].sum() > 100 and n_hit.tolist() == [0, 0] and n_clear.tolist() == [130, 65] and n_drop.tolist() == [0, 0]
    # a scan wholly dropped, alone in its grid
    rays, kind, cls = _rays("dropped_scan")
    assert (kind[1] == sc.DROPPED).all() and {1, 4} == set(cls[1].tolist()) and (kind[0] != sc.DROPPED).all()
    h, m, n_hit, n_clear, n_drop = sc.reference(CASES["dropped_scan"], W, H)
    assert n_drop.tolist() == [0, 40, 0] and not h[1].any() and not m[1].any() and h[0].sum() > 0 and h[2].sum() > 0
    # a clear ray with L = 0: one miss in the sensor's cell, no hit
    rays, kind, _ = _rays("clear_zero_length")
    zero = (kind == sc.CLEAR) & ((rays[..., 2:] == rays[..., :2]).all(-1))
    assert zero.sum() == 5 and (kind[~zero] != sc.CLEAR).all()
    h, m, _, n_clear, _ = sc.reference(CASES["clear_zero_length"], W, H)
    assert m[0, 9, 7] == 3 and m[0, 63, 64] == 2 and h[0, 9, 7] == 1 and h[0, 63, 64] == 1 and n_clear.tolist() == [5]      # (the two short returns are hits there)
    # clear rays against the grid and the tile edge; a hit ray and a clear ray of different scans ending in one cell
    rays, kind, _ = _rays("geometry")
    scans = sc.geometry_scans()
    beam2 = lambda k: (tuple(int(v) for v in rays[k, 2]), int(kind[k, 2]))      # noqa: E731
    assert beam2(0) == ((-17, 10, 63, 10), sc.CLEAR) and beam2(1) == ((-16, 12, 64, 12), sc.CLEAR)
    assert beam2(2) == ((5, -17, 5, 63), sc.CLEAR) and beam2(3) == ((6, -16, 6, 64), sc.CLEAR)
    assert T == 64 and len(scans) == len(rays)
    r4, k4 = beam2(4)
    assert k4 == sc.CLEAR and not inside(r4[0], r4[1]) and not inside(r4[2], r4[3]) and sum(inside(int(x), int(y)) for x, y in oc.walk(r4)) == H      # crosses
    r5, k5 = beam2(5)
    assert k5 == sc.CLEAR and inside(r5[0], r5[1]) and not inside(r5[2], r5[3])      # ends outside
    assert beam2(6) == ((33, 10, 63, 10), sc.HIT)
    h, m, _, _, _ = sc.reference(CASES["geometry"], W, H)
    assert h[0, 10, 63] == 1 and m[0, 10, 63] == 1 and m[0, 10, 62] == 2      # the clear ray's end is a miss, the hit ray's a hit, in one cell
    r7, k7 = beam2(7)
    assert k7 == sc.CLEAR and r7[2] - r7[0] == sc.TRACE_CELLS and not any(inside(int(x), int(y)) for x, y in oc.walk(r7))      # a return beyond the cut
    assert (kind[8] == sc.HIT).all()
    # L = 32767 kept and 32768 dropped, through the resolution
    rays, kind, cls = _rays("long")
    assert CASES["long"]["resolution"] == 2.0 ** -10 and CASES["long"]["params"].trace_range < 32.0
    assert kind[:, 2].tolist() == [sc.CLEAR, sc.DROPPED] and cls[:, 2].tolist() == [4, 4]
    assert tuple(int(v) for v in rays[0, 2]) == (67 - sc.MAX_RAY, 10, 67, 10)
    h, m, _, n_clear, n_drop = sc.reference(CASES["long"], W, H)
    assert n_clear.tolist() == [1] and n_drop.tolist() == [7] and m[0, 10, :68].tolist() == [1] * 68 and m.sum() == 68 and not h.any()
    # an end cell at +-2^20
    rays, kind, _ = _rays("cap")
    assert [int(kind[0, 2]), int(kind[1, 2]), int(kind[2, 0]), int(kind[3, 0])] == [sc.CLEAR, sc.DROPPED, sc.CLEAR, sc.DROPPED]
    assert rays[0, 2, 2] == CAP - 1 and rays[2, 0, 2] == -CAP
    # realistic numbers: every class present, two grids used, a share of the beams without a return
    for name in ("random", "random_drop"):
        rays, kind, cls = _rays(name)
        assert {1, 2, 3, 4} == set(cls.ravel().tolist()) and 0.15 < (cls == 4).mean() < 0.35
        h, m, n_hit, n_clear, n_drop = sc.reference(CASES[name], W, H)
        assert n_hit.min() > 0 and h[0].sum() > 0 and h[1].sum() > 0 and m.max() > 5
    assert sc.reference(CASES["random"], W, H)[3].sum() > sc.reference(CASES["random_drop"], W, H)[3].sum() > 0
    assert CASES["no_pose"]["poses"] is None and CASES["no_pose"]["grids"] is None
    # the shapes of the GPU test
    for n in (1, 63, 64, 65, 257, 1081, 2048):
        c = sc.beams_case(n)
        assert c["ranges"].shape == (3, n)
    for n in (1, 3, 256, 257, 300):
        assert sc.many_scans_case(n)["ranges"].shape == (n, 5)
    assert oc.BLOCK == 256
    fan = sc.fan_case()
    rays, kind, _ = sc.case_rays(fan)
    assert (kind == sc.CLEAR).all() and kind.shape == (1, 1081) and (rays[0, :, :2] == (33, 31)).all()
