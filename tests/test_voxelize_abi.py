"""CPU checks of lsm2d_voxelize (ABI 0.7.11): the symbol, the parameter struct and the two limits are declared by include/lsm2d.h, bound by the Python mirror
and laid out as gcc lays them out; the new kernels are in the library's code object; the mirrors exist and the C++ sources compile; voxelize_cases.reference
-- what the GPU tests hold the device to -- is pinned to the CPU ORACLE bit for bit (the clipper's voxelisation, the preprocessor's, the merger's transform);
and the cases the GPU tests run contain what they claim."""
import ctypes as C
import dataclasses
import math
import os
import re
import subprocess

import numpy as np
import pytest

import abi_checks
import cpp_build
import voxelize_cases as vc
from conftest import ROOT
from srrg2_laser_slam_2d_amd import api

F32 = np.float32
T = vc.TILE


def test_symbol_struct_and_macros_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi
    abi_checks.assert_declared_bound_exported("lsm2d_voxelize", 12)
    header = abi_checks.header()
    assert "int lsm2d_voxelize(" in header and "} lsm2d_voxelize_params;" in header and "0.7.11" in header
    assert "#define LSM2D_VOXELIZE_MAX_POINTS (1 << 24)" in header and "#define LSM2D_VOXELIZE_MAX_GROUPS (1 << 16)" in header
    assert (_capi.VOXELIZE_MAX_POINTS, _capi.VOXELIZE_MAX_GROUPS) == (1 << 24, 1 << 16)
    assert _capi.VOXELIZE_MAX_POINTS >= 1 << 24 and _capi.VOXELIZE_MAX_GROUPS >= 1 << 16
    # the reference lines the call restates are cited where it is declared
    assert "raw_data_preprocessor_projective_2d.cpp:38-41" in header and "scene_clipper_projective_2d.cpp:44-48" in header


def test_params_layout_matches_the_c_compiler(tmp_path):
    from srrg2_laser_slam_2d_amd import _capi
    st, cname = _capi.VoxelizeParamsC, "lsm2d_voxelize_params"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsm2d.h"', 'int main(void) {', 'printf("%%zu", sizeof(%s));' % cname]
    for fname, _ in st._fields_:
        lines.append('printf(" %s=%%zu", offsetof(%s, %s));' % (fname, cname, fname))
    lines += ['printf(" points=%d groups=%d\\n", LSM2D_VOXELIZE_MAX_POINTS, LSM2D_VOXELIZE_MAX_GROUPS);', 'return 0; }']
    src = tmp_path / "layout.c"; src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    parts = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert int(parts[0]) == C.sizeof(st) == 8
    seen = dict(kv.split("=") for kv in parts[1:])
    for fname, _ in st._fields_:
        assert getattr(st, fname).offset == int(seen[fname]), fname
    assert (int(seen["points"]), int(seen["groups"])) == (_capi.VOXELIZE_MAX_POINTS, _capi.VOXELIZE_MAX_GROUPS)


def test_kernels_are_in_the_code_object_and_the_tile_is_the_sources():
    from srrg2_laser_slam_2d_amd import _capi
    abi_checks.assert_kernels_in_code_object((b"k_vox_keys", b"k_vox_hist", b"k_vox_scan", b"k_vox_scatter", b"k_vox_head_count", b"k_vox_head_write", b"k_vox_sum",
                                              b"k_vox_verdict", b"k_vox_write", b"k_vox_finish", b"voxelize_tile", b"voxelize_scan_tiles"))
    src = open(os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "csrc", "lsm2d_k_voxelize.h")).read()
    assert int(re.search(r"kVoxTile = (\d+);", src).group(1)) == _capi.VOXELIZE_TILE == T
    block = int(re.search(r"kVoxScanBlock = (\d+);", src).group(1))
    assert "kVoxScanTiles = 4 * kVoxScanBlock / 256;" in src and 4 * block // 256 == _capi.VOXELIZE_SCAN_TILES == vc.SCAN_TILES


def test_mirrors_exist():
    abi_checks.assert_mirrors_have("voxelize", ("voxelize(", "lsm2d_voxelize(", '#include "lsm2d.hpp"'), "lsm2d_voxelize.hpp")
    assert [f.name for f in dataclasses.fields(api.VoxelizeParams)] == ["resolution", "normal_resolution"]
    assert api.VoxelizeParams.clipper(0.05).normal_resolution == 0.1 and api.VoxelizeParams.preprocessor(0.05).normal_resolution == 1.0


@pytest.mark.parametrize("source", ["voxelize_driver.cpp", "voxelize_bench.cpp", "voxelize_ref.cpp"])
def test_cpp_sources_compile(source):
    r = cpp_build.syntax_only(source)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the reference, pinned to the oracle ----------------------------------------------------------------------------------------------------------------
def _ring(n_cols, columns, radius, rng):
    """one point per chosen column of a (-pi, pi) projector of n_cols columns, on a circle round the origin, ascending column; normals face the origin"""
    a = (-math.pi + (np.asarray(columns, np.float64) + 0.5) * (2.0 * math.pi / n_cols))
    r = radius + rng.uniform(-0.01, 0.01, len(a))
    return np.stack([r * np.cos(a), r * np.sin(a), -np.cos(a), -np.sin(a)], 1).astype(F32)


def test_reference_is_the_oracles_clipper_voxelisation(po):
    rng = np.random.default_rng(5)
    cols = 720
    pr = po.Projector(cols, -math.pi, math.pi, 0.3, 30.0, 0.0)
    n_shared = 0
    for radius, res in ((2.0, 0.05), (4.0, 0.1), (1.0, 0.05), (8.0, 0.5)):
        columns = np.sort(rng.choice(cols, 600, replace=False))      # runs of neighbouring columns among them
        scene = _ring(cols, columns, radius, rng)
        plain, src = po.clip_scene(pr, scene, np.zeros(3, F32))
        assert len(plain) == len(scene) and np.array_equal(src, np.arange(len(scene)))      # one unoccluded point per column, in the scene's order
        want = po.clip_scene_voxelized(pr, scene, np.zeros(3, F32), (0.0, 0.0, 0.0), res)
        got, counts, dropped = vc.reference([scene], params=(res, 0.1))
        assert counts[0] == len(want) and dropped[0] == 0
        assert got[0].tobytes() == want.tobytes(), (radius, res)
        n_shared += len(scene) - len(want)
    assert n_shared > 100      # neighbouring columns did share voxels


def test_reference_is_the_oracles_preprocessor_voxelisation(po):
    from srrg2_laser_slam_2d_amd import synth
    world = synth.make_world(6)
    poses = synth.sample_poses(world, 3, seed=21)
    ranges = synth.make_scan_ranges(world, poses, n_beams=721, angle_min=-2.35, angle_max=2.35, noise_sigma=0.004, seed=7)
    merged = 0
    for r in ranges:
        for res in (0.02, 0.1):
            points = po.preprocess_scan(po.Preprocessor(721, -2.35, 2.35, 0.3, 20.0, 0.3, 5, 0.0), r)
            want = po.preprocess_scan(po.Preprocessor(721, -2.35, 2.35, 0.3, 20.0, 0.3, 5, res), r)
            got, counts, dropped = vc.reference([points], params=(res, 1.0))
            assert len(points) > 200 and counts[0] == len(want) and dropped[0] == 0
            assert got[0].tobytes() == want.tobytes(), res
            merged += len(points) - len(want)
    assert merged > 100


def test_reference_transform_is_the_oracles_merge_into_an_empty_scene(po):
    rng = np.random.default_rng(6)
    cols = 720
    pr = po.Projector(cols, -math.pi, math.pi, 0.3, 30.0, 0.0)
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for th in (-2.5, -0.4, 0.7, 3.0):
                pose = np.array([sx * 1.25, sy * 0.75, th], F32)
                meas = _ring(cols, np.sort(rng.choice(np.arange(2, cols - 2, 2), 300, replace=False)), 5.0, rng)      # at most one point per column, far inside 0.9 x range_max
                want, counts = po.merge_scene(pr, np.zeros((0, 4), F32), meas, pose)
                assert counts == (len(meas), 0, 0)
                assert vc.transform(meas, pose).tobytes() == want.tobytes(), pose.tolist()


# ---- the cases contain what they claim ------------------------------------------------------------------------------------------------------------------
def _sorted_keys(case):
    assert case["poses"] is None and len(case["clouds"]) == 1
    k = vc.keys(case["clouds"][0], *case["params"])
    return k, np.sort(k[k >= 0], kind="stable")


def _runs(sorted_keys):
    """(start, length) of every run of equal keys"""
    if len(sorted_keys) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    starts = np.flatnonzero(np.concatenate([[True], sorted_keys[1:] != sorted_keys[:-1]]))
    return starts, np.diff(np.concatenate([starts, [len(sorted_keys)]]))


def test_cases_contain_what_they_claim():
    sizes = vc.size_cases()
    assert sorted(len(c["clouds"][0]) for c in sizes.values()) == [0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5]
    for name, c in sizes.items():
        _, counts, dropped = vc.case_reference(c)
        n = len(c["clouds"][0])
        assert counts[0] + dropped[0] <= n and (n < 50 or (dropped[0] > 0 and 0 < counts[0] < n - dropped[0])), name      # equal keys and dropped points among them
    s = vc.structure_cases()
    # a run of equal keys across a tile boundary of the sorted order
    _, sk = _sorted_keys(s["straddle"])
    starts, lens = _runs(sk)
    assert len(sk) == 2 * T + 1 and any(b < T < b + n for b, n in zip(starts, lens))
    # a run longer than a tile, among others
    _, sk = _sorted_keys(s["long_run"])
    starts, lens = _runs(sk)
    assert lens.max() > T and len(lens) > 50 and len(sk) > 2 * T
    # one voxel
    k, sk = _sorted_keys(s["one_voxel"])
    assert len(k) == 2 * T + 1 and np.all(k == k[0]) and k[0] >= 0
    # all distinct, ascending and descending in input order
    k, _ = _sorted_keys(s["distinct_sorted"])
    assert len(k) == 3 * T + 5 and np.all(np.diff(k) > 0)
    k, _ = _sorted_keys(s["distinct_reversed"])
    assert len(k) == 3 * T + 5 and np.all(np.diff(k) < 0)
    # the ends of the ranges, one ulp outside each, NaN and Inf
    e, ok = vc.edge_points()
    k = vc.keys(e, vc.RES, 1.0)
    assert np.array_equal(k >= 0, ok)
    kx, ky, knx, kny = (k >> 26) - 32768, ((k >> 10) & 0xFFFF) - 32768, ((k >> 5) & 31) - 16, (k & 31) - 16
    good = k >= 0
    for comp, lo, hi in ((kx, -32768, 32767), (ky, -32768, 32767), (knx, -16, 15), (kny, -16, 15)):
        assert lo in comp[good] and hi in comp[good]
    for c in range(4):      # one ulp outside each bound: the neighbour float inside has a key
        col = e[:, c]
        for v_out, toward in ((np.nextafter(F32(-16384.0 if c < 2 else -16.0), F32(-np.inf)), F32(np.inf)), (F32(16384.0 if c < 2 else 16.0), F32(-np.inf))):
            i = np.flatnonzero(col == v_out)
            assert len(i) >= 1 and not np.any(ok[i])
            assert np.any((col == np.nextafter(v_out, toward)) & ok)
        assert np.any(np.isnan(col)) and np.any(col == np.inf) and np.any(col == -np.inf)
    assert np.all(np.isin(e.view(np.uint32), s["edges"]["clouds"][0].view(np.uint32)).all(axis=1))
    g = vc.group_cases()
    assert [len(g[n]["clouds"]) for n in ("inputs3_group1", "inputs7_groups3")] == [3, 7] and g["inputs7_groups3"]["n_groups"] == 3
    c = g["inputs7_groups3"]
    per_group = [sum(len(c["clouds"][k]) for k in range(7) if c["groups"][k] == gi) for gi in range(3)]
    assert per_group[0] > 2 * T and sum(per_group[:2]) % T != 0 and min(per_group) > 0      # groups that cross tiles
    clouds, counts, dropped = vc.case_reference(g["empty_and_dropped"])
    assert counts[1] == 0 and dropped[1] == 0                                   # an empty group
    assert counts[2] == 0 and dropped[2] == 40                                  # a group that is dropped entirely
    assert counts[0] == counts[3] > 0                                           # the same keys in two groups, never merged
    k0 = vc.keys(g["empty_and_dropped"]["clouds"][0], vc.RES, 1.0); k3 = vc.keys(g["empty_and_dropped"]["clouds"][3], vc.RES, 1.0)
    assert set(k0.tolist()) == set(k3.tolist())
    assert g["clipper_coefficients"]["params"][1] == 0.1 and g["preprocessor_coefficients"]["params"][1] == 1.0
    # just past the tiles one pass of the scan takes, every key its own
    k, _ = _sorted_keys(vc.scan_boundary_case())
    assert len(k) == vc.SCAN_TILES * T + 5 and len(set(k.tolist())) == len(k) and k.min() >= 0 and np.any(np.diff(k) < 0)
    a = vc.assembly_case()
    assert len(a["clouds"]) == 5 and {(np.sign(p[0]), np.sign(p[1]), np.sign(p[2])) for p in a["poses"][:4]} == {(1, -1, 1), (-1, 1, -1), (1, 1, 1), (-1, -1, -1)}


def test_reference_orders_equal_keys_by_concatenation_index():
    """fp32 sums depend on their order: a voxel of three points whose sum differs between orders comes out in the order of the list"""
    a, b, c = F32(1.0e-3), F32(0.24999999), F32(0.2)
    pts = np.array([[a, 0.1, 0.5, 0.5], [b, 0.1, 0.5, 0.5], [c, 0.1, 0.5, 0.5]], F32)
    fwd = F32(F32(F32(F32(0.0) + a) + b) + c) * (F32(1.0) / F32(3.0)); rev = F32(F32(F32(F32(0.0) + c) + b) + a) * (F32(1.0) / F32(3.0))
    assert vc.reference([pts])[0][0][0, 0] == F32(fwd)
    assert vc.reference([pts[::-1].copy()])[0][0][0, 0] == F32(rev)
    # two inputs: list position first
    assert vc.reference([pts[2:], pts[:2]])[0][0][0, 0] == F32(F32(F32(F32(F32(0.0) + c) + a) + b) * (F32(1.0) / F32(3.0)))
