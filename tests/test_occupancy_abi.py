"""CPU checks of the occupancy grids (ABI 0.7.12): the seven symbols, the two structs and the four limits are declared by include/lsm2d.h, bound by the
Python mirror and laid out as gcc lays them out; the new kernels are in the library's code object; the mirrors exist and the C++ sources compile;
occupancy_cases.reference -- what the GPU tests hold the device to -- has voxelize_cases.transform's transform bit for bit (that one is pinned to the
oracle's merger), and its walk equals an independent incremental walk, has L + 1 cells, the right ends, 8-connected steps and stays within half a cell of
the ideal line in exact rationals; the cases the GPU tests run contain what they claim; api.occupancy_values on hand-made counts."""
import ctypes as C
import dataclasses
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import abi_checks
import cpp_build
import occupancy_cases as oc
import voxelize_cases as vc
from conftest import ROOT
from srrg2_laser_slam_2d_amd import api

F32 = np.float32
SYMBOLS = {"lsm2d_gridset_create": 4, "lsm2d_gridset_clear": 3, "lsm2d_gridset_upload": 4, "lsm2d_gridset_download": 4, "lsm2d_gridset_destroy": 1,
           "lsm2d_occupancy_update": 9, "lsm2d_occupancy_render": 5}
CASES = oc.all_cases()
_RAYS = {}


def _rays(name):
    if name not in _RAYS:
        _RAYS[name] = oc.case_rays(CASES[name])
    return _RAYS[name]


def test_symbols_structs_and_macros_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi
    for name, n_args in SYMBOLS.items():
        abi_checks.assert_declared_bound_exported(name, n_args)
    header = abi_checks.header()
    assert "} lsm2d_grid_geometry;" in header and "} lsm2d_occupancy_render_params;" in header
    for macro, value, mirror in (("LSM2D_OCCUPANCY_MAX_SIDE", "16384", _capi.OCCUPANCY_MAX_SIDE), ("LSM2D_OCCUPANCY_MAX_CELLS", "(1 << 28)", _capi.OCCUPANCY_MAX_CELLS),
                                 ("LSM2D_OCCUPANCY_MAX_RAYS", "(1 << 24)", _capi.OCCUPANCY_MAX_RAYS), ("LSM2D_OCCUPANCY_MAX_RAY_CELLS", "32767", _capi.OCCUPANCY_MAX_RAY_CELLS)):
        assert re.search(r"#define %s\s+%s\s" % (macro, re.escape(value)), header), macro
        assert mirror == eval(value)
    assert "0.7.12" in header
    # the meaning is cited where it is declared, and so are the limits of what is built
    block = header[header.index("occupancy grids on the device (0.7.12)"):header.index("#define LSM2D_OCCUPANCY_MAX_SIDE")]
    for text in ("item 17c", "item 11b", "xf_point", "lsm2d_merge_scene", "no grid mapper", "NOT BUILT", "asynchronous form", "per-grid geometry", "maximum-range truncation",
                 "once-per-scan", "several workgroups", "log-odds"):
        assert text in block, text


def test_struct_layouts_match_the_c_compiler(tmp_path):
    from srrg2_laser_slam_2d_amd import _capi
    structs = {"lsm2d_grid_geometry": (_capi.GridGeometryC, 20), "lsm2d_occupancy_render_params": (_capi.OccupancyRenderParamsC, 4)}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsm2d.h"', 'int main(void) {']
    for cname, (st, _) in structs.items():
        lines.append('printf("%s %%zu", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            lines.append('printf(" %s=%%zu", offsetof(%s, %s));' % (fname, cname, fname))
        lines.append('printf("\\n");')
    lines += ['printf("limits %d %d %d %d\\n", LSM2D_OCCUPANCY_MAX_SIDE, LSM2D_OCCUPANCY_MAX_CELLS, LSM2D_OCCUPANCY_MAX_RAYS, LSM2D_OCCUPANCY_MAX_RAY_CELLS);', 'return 0; }']
    src = tmp_path / "layout.c"; src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    for line in out[:-1]:
        parts = line.split(); st, size = structs[parts[0]]
        assert int(parts[1]) == C.sizeof(st) == size, parts[0]
        for kv in parts[2:]:
            k, v = kv.split("=")
            assert getattr(st, k).offset == int(v), (parts[0], k)
    assert [int(v) for v in out[-1].split()[1:]] == [_capi.OCCUPANCY_MAX_SIDE, _capi.OCCUPANCY_MAX_CELLS, _capi.OCCUPANCY_MAX_RAYS, _capi.OCCUPANCY_MAX_RAY_CELLS]


def test_kernels_are_in_the_code_object_and_the_tile_is_the_sources():
    from srrg2_laser_slam_2d_amd import _capi
    abi_checks.assert_kernels_in_code_object((b"k_occ_rays", b"k_occ_tilesILb0EE", b"k_occ_render", b"k_occ_put", b"occupancy_tile"))
    csrc = os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "csrc")
    src = open(os.path.join(csrc, "lsm2d_k_occupancy.h")).read()
    assert int(re.search(r"kOccTile = (\d+);", src).group(1)) == _capi.OCCUPANCY_TILE == oc.TILE == 64
    assert int(re.search(r"kOccBlock = (\d+);", src).group(1)) == _capi.OCCUPANCY_BLOCK == oc.BLOCK
    # the new parts come LAST: every older kernel keeps its place in the code object
    assert re.findall(r'#include "(lsm2d_k_\w+\.h)"', open(os.path.join(csrc, "lsm2d_kernels.h")).read())[-1] == "lsm2d_k_occupancy.h"
    assert re.findall(r'#include "(lsm2d_capi_\w+\.inc)"', open(os.path.join(csrc, "lsm2d_capi.hip")).read())[-1] == "lsm2d_capi_occupancy.inc"


def test_mirrors_exist():
    abi_checks.assert_mirrors_have(("occupancy_update", "occupancy_render", "occupancy_values"),
                                   ("class GridSet", "occupancyUpdate(", "occupancyRender(", "lsm2d_occupancy_update(", "lsm2d_occupancy_render(", "lsm2d_gridset_destroy(",
                                    '#include "lsm2d.hpp"'), "lsm2d_occupancy.hpp")
    assert [f.name for f in dataclasses.fields(api.GridGeometry)] == ["origin_x", "origin_y", "resolution", "width", "height"]
    for m in ("clear", "upload", "download", "close"):
        assert callable(getattr(api.GridSet, m)), m
    first = abi_checks.assert_mirrors_have((), ())
    assert "lsm2d_occupancy" not in first and "lsm2d_gridset" not in first


@pytest.mark.parametrize("source", ["occupancy_driver.cpp", "occupancy_bench.cpp", "occupancy_ref.cpp"])
def test_cpp_sources_compile(source):
    r = cpp_build.syntax_only(source)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the reference's transform is the voxeliser's, which is the oracle's merger ----------------------------------------------------------------------------
def test_reference_transform_is_voxelize_cases_transform_bit_for_bit():
    rng = np.random.default_rng(6)
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for th in (-2.5, -0.4, 0.0, 0.7, 3.0):
                pose = np.array([sx * 1.25, sy * 0.75, th], F32)
                pts = np.stack([rng.uniform(-9, 9, 300), rng.uniform(-9, 9, 300), np.ones(300), np.zeros(300)], 1).astype(F32)
                assert oc.transform(pts, pose)[:, :2].tobytes() == vc.transform(pts, pose)[:, :2].tobytes(), pose.tolist()
    # ... and it is what the rays are made from: the cells of the transformed points, start at the pose's translation
    case = CASES["random"]
    for k, cloud in enumerate(case["clouds"]):
        rays, live = oc.rays_of(cloud, case["poses"][k], case["origin"], case["resolution"])
        t = vc.transform(cloud, case["poses"][k])
        inv = F32(1.0) / F32(case["resolution"]); o = np.array(case["origin"], F32)
        want = np.floor((t[:, :2] - o) * inv).astype(np.int32)
        start = np.floor((case["poses"][k][:2] - o) * inv).astype(np.int32)
        assert live.all() and np.array_equal(rays[:, 2:], want) and np.all(rays[:, :2] == start)


# ---- the walk ----------------------------------------------------------------------------------------------------------------------------------------------
def _incremental_walk(x0, y0, x1, y1):
    """the error-term walk, written independently of the closed form: the minor coordinate steps when twice the accumulated minor extent passes L"""
    dx, dy = x1 - x0, y1 - y0
    ax, ay = abs(dx), abs(dy)
    sx, sy = (-1 if dx < 0 else 1), (-1 if dy < 0 else 1)
    cells = []
    if ax >= ay:
        err, y = ax, y0
        for i in range(ax + 1):
            cells.append((x0 + sx * i, y))
            err += 2 * ay
            if ax and err >= 2 * ax:
                err -= 2 * ax; y += sy
    else:
        err, x = ay, x0
        for i in range(ay + 1):
            cells.append((x, y0 + sy * i))
            err += 2 * ax
            if err >= 2 * ay:
                err -= 2 * ay; x += sx
    return cells


@pytest.mark.parametrize("name", sorted(CASES))
def test_walk_of_every_ray_of_every_case(name):
    rays, live = _rays(name)
    n_checked = 0
    for r in rays[live]:
        x0, y0, x1, y1 = (int(v) for v in r)
        cells = [tuple(int(v) for v in c) for c in oc.walk(r)]
        L = max(abs(x1 - x0), abs(y1 - y0))
        assert len(cells) == L + 1 and cells[0] == (x0, y0) and cells[-1] == (x1, y1), r
        assert cells == _incremental_walk(x0, y0, x1, y1), r
        xm = abs(x1 - x0) >= abs(y1 - y0)
        a = abs(y1 - y0) if xm else abs(x1 - x0)
        for i in range(1, L + 1):
            assert max(abs(cells[i][0] - cells[i - 1][0]), abs(cells[i][1] - cells[i - 1][1])) == 1, (r, i)      # 8-connected, no repeated cell
        step = 1 if L <= 2048 else 997      # (the two 32767-cell rays: every 997th step and the last ones)
        for i in list(range(0, L + 1, step)) + list(range(max(L - 3, 0), L + 1)):
            minor = (cells[i][1] - y0) * (1 if y1 >= y0 else -1) if xm else (cells[i][0] - x0) * (1 if x1 >= x0 else -1)
            major = abs(cells[i][0] - x0) if xm else abs(cells[i][1] - y0)
            assert major == i
            ideal = Fraction(i * a, L) if L else Fraction(0)
            assert abs(Fraction(minor) - ideal) <= Fraction(1, 2), (r, i)
        n_checked += 1
    assert n_checked == int(live.sum())


def test_cases_contain_what_they_claim():
    W, H, T, CAP = oc.W, oc.H, oc.TILE, oc.CAP
    inside = lambda x, y: 0 <= x < W and 0 <= y < H      # noqa: E731
    # the builder gives exactly the cells asked for
    for name, want in (("octants", oc.octant_rays()), ("borders", oc.border_rays()), ("long", oc.long_rays()), ("cap", oc.cap_rays())):
        rays, live = _rays(name)
        assert len(rays) == len(want), name
        for r, l, w in zip(rays, live, want):
            ok = all(-CAP <= v < CAP for v in w) and max(abs(w[2] - w[0]), abs(w[3] - w[1])) <= oc.MAX_RAY
            assert l == ok and (not ok or tuple(int(v) for v in r) == tuple(w)), (name, w)
    # octants, axes, ties
    rays, live = _rays("octants")
    d = rays[:, 2:] - rays[:, :2]
    octs = {(int(np.sign(x)), int(np.sign(y)), abs(int(x)) > abs(int(y))) for x, y in d if x and y and abs(x) != abs(y)}
    assert len(octs) == 8 and live.all()
    for v in ((9, 0), (-9, 0), (0, 9), (0, -9)):
        assert any((d == v).all(1))
    assert sum(1 for x, y in d if abs(x) == abs(y) and x) >= 4                      # ax == ay
    assert sum(1 for x, y in d if max(abs(x), abs(y)) == 2 * min(abs(x), abs(y)) and x and y) >= 8      # a / L = 1 / 2
    assert any((d == (0, 0)).all(1)) and sum(1 for x, y in d if max(abs(x), abs(y)) == 1) >= 3           # L = 0, L = 1
    # the tie rule: ax == ay walks the diagonal
    assert [tuple(c) for c in oc.walk([0, 0, 3, -3]).tolist()] == [(0, 0), (1, -1), (2, -2), (3, -3)]
    # a rounding tie goes up (away from the start): (2 i a + L) / (2 L) at a / L = 1 / 2, i = 1 is exactly 1
    assert [tuple(c) for c in oc.walk([0, 0, 4, 2]).tolist()] == [(0, 0), (1, 1), (2, 1), (3, 2), (4, 2)]
    # negative cells, and an origin that is not zero
    rays, live = _rays("negative")
    assert live.all() and (rays < 0).any(axis=1).sum() > 20 and CASES["negative"]["origin"] == (-1.25, 0.75)
    # enter, leave, cross, miss; last row and column; the tile edge
    rays, live = _rays("borders")
    kinds = set()
    for r in rays:
        cells = oc.walk(r)
        touched = any(inside(int(x), int(y)) for x, y in cells)
        kinds.add((inside(int(r[0]), int(r[1])), inside(int(r[2]), int(r[3])), touched))
        assert len(cells) > 1
    assert {(False, True, True), (True, False, True), (False, False, True), (False, False, False), (True, True, True)} <= kinds
    assert any(r[1] == H - 1 and r[3] == H - 1 and abs(r[2] - r[0]) > 100 for r in rays) and any(r[0] == W - 1 and r[2] == W - 1 and abs(r[3] - r[1]) > 60 for r in rays)
    crossings = set()
    for r in rays:
        xm = abs(r[2] - r[0]) >= abs(r[3] - r[1])
        cells = oc.walk(r)
        for (xa, ya), (xb, yb) in zip(cells[:-1], cells[1:]):
            if {int(xa), int(xb)} == {T - 1, T}:
                crossings.add(("x", "major" if xm else "minor"))
            if {int(ya), int(yb)} == {T - 1, T}:
                crossings.add(("y", "minor" if xm else "major"))
    assert crossings == {("x", "major"), ("x", "minor"), ("y", "major"), ("y", "minor")}
    # L at the cap of a ray's length
    rays, live = _rays("long")
    L = np.abs(rays[:, 2:] - rays[:, :2]).max(1)
    assert live.tolist() == [True, False, True, False] and L[live].tolist() == [oc.MAX_RAY, oc.MAX_RAY]
    for r in rays[live]:
        cells = oc.walk(r)
        n_in = sum(1 for x, y in cells if inside(int(x), int(y)))
        assert 0 < n_in < 200 and len(cells) == oc.MAX_RAY + 1      # almost all of it outside
    # a cell coordinate at the cap, both sides, both axes
    rays, live = _rays("cap")
    assert live.tolist() == [True, False, True, False, True, False, True, False, False, False]
    assert rays[live].max() == CAP - 1 and rays[live].min() == -CAP
    # cell edges and one ulp either side
    pts, cells = oc.edge_points()
    rays, live = _rays("edges")
    assert live.all() and np.all(rays[:, :2] == 0) and np.array_equal(rays[:, 2:], cells)
    assert len({tuple(c) for c in cells.tolist()}) >= 20
    # NaN and Inf
    pts, ok = oc.nonfinite_points()
    rays, live = _rays("nonfinite")
    assert np.array_equal(live, ok) and np.isnan(pts[:, :2]).any() and np.isposinf(pts[:, :2]).any() and np.isneginf(pts[:, :2]).any() and ok.sum() == 3
    # an empty input, a wholly dropped input, and a grid that only the dropped one feeds
    c = CASES["empty_and_dropped"]
    assert [len(x) for x in c["clouds"]] == [40, 0, 25, 40]
    _, _, n_rays, dropped = oc.reference(c, W, H)
    assert n_rays.tolist() == [80, 0, 0] and dropped.tolist() == [0, 0, 25]
    # realistic numbers: all live, two grids used
    c = CASES["random"]
    h, m, n_rays, dropped = oc.reference(c, W, H)
    assert dropped.sum() == 0 and n_rays.min() > 0 and h[0].sum() > 0 and h[1].sum() > 0 and m.max() > 5
    # the fans and the many-input cases of the GPU test
    for n in (1, 63, 64, 65, 257, 1081):
        f = oc.fan_case(n)
        assert len(f["clouds"]) == 1 and len(f["clouds"][0]) == n
    for n in (1, 3, 256, 257, 300):
        assert len(oc.many_inputs_case(n)["clouds"]) == n
    assert oc.BLOCK == 256


def test_reference_counts_by_hand():
    """one ray, cell by cell: misses on steps 0 .. L - 1, a hit on step L, nothing outside the grid; and saturation"""
    case = oc.cell_rays([(1, 1, 5, 3), (1, 1, 1, 1), (1, 1, 8, 1)])
    h, m, n_rays, dropped = oc.reference(case, 6, 4)
    want_m = np.zeros((4, 6), np.uint32); want_h = np.zeros((4, 6), np.uint32)
    for x, y in ((1, 1), (2, 2), (3, 2), (4, 3)):
        want_m[y, x] += 1
    want_h[3, 5] += 1
    want_h[1, 1] += 1                      # L = 0: the single cell is the hit
    for x in range(1, 6):
        want_m[1, x] += 1                  # ends at (8, 1) outside: its hit is not counted
    assert np.array_equal(h[0], want_h) and np.array_equal(m[0], want_m) and n_rays.tolist() == [3] and dropped.tolist() == [0]
    full = np.full((1, 4, 6), 0xFFFFFFFE, np.uint32)
    h2, m2, _, _ = oc.reference(case, 6, 4, full, full)
    assert m2[0, 1, 1] == 0xFFFFFFFF and m2[0, 1, 2] == 0xFFFFFFFF and h2[0, 1, 1] == 0xFFFFFFFF and h2[0, 0, 0] == 0xFFFFFFFE


def test_occupancy_values_on_hand_made_counts():
    v = api.occupancy_values
    assert v([0, 5, 1, 3], [5, 0, 7, 5]).tolist() == [0, 100, 12, 38]      # 0, 100, 12.5 -> 12, 37.5 -> 38: ties to even
    assert v([0], [0]).tolist() == [-1] and v([0], [0], 0).tolist() == [-1]      # never visited: unknown whatever min_visits says
    assert v([1, 1], [1, 2], 3).tolist() == [-1, 33]                      # min_visits one above and at a cell's visits
    assert v([1], [2], 4).tolist() == [-1]
    big = 0xFFFFFFFF
    assert v([big, big, 0, big], [big, 0, big, 1]).tolist() == [50, 100, 0, 100]      # saturated counters: the sum is formed in 64 bits
    out = v(np.array([[1, 0], [2, 2]], np.uint32), np.array([[0, 0], [2, 6]], np.uint32), 1)
    assert out.dtype == np.int8 and out.tolist() == [[100, -1], [50, 25]]
