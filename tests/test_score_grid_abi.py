"""CPU checks of lsm2d_score_grid_select (ABI 0.7.10): the symbol, the descriptor and the two limits are declared by include/lsm2d.h, bound by the Python
mirror with the right argument count and laid out as gcc lays them out; the new kernels are in the library's code object; the Python and C++ mirrors exist
and the C++ sources compile; api.grid_level_poses gives the known answers of the formulas the header states; and -- on the CPU oracle, no GPU -- the cases
the GPU tests run are such that those tests cannot pass vacuously (score_grid_cases)."""
import ctypes as C
import dataclasses
import os
import subprocess

import numpy as np
import pytest

import abi_checks
import cpp_build
import score_grid_cases as gc
from conftest import ROOT
from srrg2_laser_slam_2d_amd import api

F32 = np.float32


def test_symbol_struct_and_macros_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi
    abi_checks.assert_declared_bound_exported("lsm2d_score_grid_select", 20)      # the declaration's parameters, counted: ctx .. out_level_counts
    header = abi_checks.header()
    assert "int lsm2d_score_grid_select(" in header and "} lsm2d_pose_grid;" in header and "0.7.10" in header
    assert "#define LSM2D_GRID_MAX_LEVELS 4" in header and "#define LSM2D_GRID_MAX_ITEMS  (1 << 18)" in header
    assert (_capi.GRID_MAX_LEVELS, _capi.GRID_MAX_ITEMS) == (4, 1 << 18)


def test_pose_grid_layout_matches_the_c_compiler(tmp_path):
    """sizeof / offsetof of lsm2d_pose_grid as gcc lays include/lsm2d.h out, against the ctypes mirror field by field"""
    from srrg2_laser_slam_2d_amd import _capi
    st, cname = _capi.PoseGridC, "lsm2d_pose_grid"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsm2d.h"', 'int main(void) {', 'printf("%%zu", sizeof(%s));' % cname]
    for fname, _ in st._fields_:
        lines.append('printf(" %s=%%zu", offsetof(%s, %s));' % (fname, cname, fname))
    lines += ['printf(" levels=%d items=%d\\n", LSM2D_GRID_MAX_LEVELS, LSM2D_GRID_MAX_ITEMS);', 'return 0; }']
    src = tmp_path / "layout.c"; src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    parts = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert int(parts[0]) == C.sizeof(st) == 56
    seen = dict(kv.split("=") for kv in parts[1:])
    for fname, _ in st._fields_:
        assert getattr(st, fname).offset == int(seen[fname]), fname
    assert (int(seen["levels"]), int(seen["items"])) == (_capi.GRID_MAX_LEVELS, _capi.GRID_MAX_ITEMS)


def test_kernels_are_in_the_code_object():
    abi_checks.assert_kernels_in_code_object((b"k_grid_level0", b"k_grid_children", b"k_grid_mask_padsINS_7CombRow", b"k_grid_finish"))


def test_mirrors_exist():
    abi_checks.assert_mirrors_have(("score_grid_select", "relocalize_grid", "grid_level_poses"),
                                   ("scoreGridSelect(", "relocalizeGrid(", "lsm2d_score_grid_select(", '#include "lsm2d.hpp"'), "lsm2d_score_grid.hpp")
    fields = [f.name for f in dataclasses.fields(api.ScoreGridResult)]
    assert fields == ["pose", "origin", "H", "b", "stats", "active", "n_accepted", "level_counts", "kernel_ms"]
    assert [f.name for f in dataclasses.fields(api.PoseGrid)] == ["center", "step", "count", "n_levels", "refine", "k_parents"]
    assert "two" in api.relocalize_grid.__doc__.lower() and "0.4 %" in api.relocalize_grid.__doc__


@pytest.mark.parametrize("source", ["score_grid_driver.cpp", "score_grid_bench.cpp"])
def test_cpp_sources_compile(source):
    r = cpp_build.syntax_only(source)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- api.grid_level_poses: known answers ------------------------------------------------------------------------------------------------------------------------
def test_level0_known_answers_and_order():
    g = api.PoseGrid(center=(1.0, 1.0, 1.0), step=(0.5, 0.5, 0.5), count=(4, 1, 1))
    p = api.grid_level_poses(g, 0)
    assert p.dtype == np.float32 and p.shape == (4, 3)
    assert p[:, 0].tolist() == [0.25, 0.75, 1.25, 1.75] and np.all(p[:, 1:] == 1.0)
    # item (it * ny + iy) * nx + ix
    g = api.PoseGrid(center=(0.0, 10.0, 100.0), step=(1.0, 2.0, 4.0), count=(2, 3, 2))
    p = api.grid_level_poses(g, 0)
    assert len(p) == 12
    for it in range(2):
        for iy in range(3):
            for ix in range(2):
                assert p[(it * 3 + iy) * 2 + ix].tolist() == [ix - 0.5, 10.0 + 2.0 * (iy - 1), 100.0 + 4.0 * (it - 0.5)]


def test_children_known_answers_and_order():
    parents = np.array([[0.1, -0.7, 3.0], [5.0, 6.0, -7.0]], F32)
    one = api.PoseGrid(step=(0.3, 0.3, 0.3), count=(2, 1, 1), n_levels=2, refine=(1, 1, 1), k_parents=2)
    assert api.grid_level_poses(one, 1, parents).tobytes() == parents.tobytes()      # refine 1: the parent's bits
    g = api.PoseGrid(step=(0.3, 0.3, 0.3), count=(2, 1, 1), n_levels=3, refine=(3, 1, 2), k_parents=2)
    s1 = g.spacing(1)
    assert s1.dtype == np.float32 and s1.tobytes() == np.array([F32(0.3) / F32(3.0), F32(0.3), F32(0.3) / F32(2.0)], F32).tobytes()
    assert g.spacing(2).tobytes() == (s1 / np.array([3, 1, 2], F32)).astype(F32).tobytes()      # division after division
    p = api.grid_level_poses(g, 1, parents)
    assert p.shape == (12, 3)
    for j in range(2):
        for ct in range(2):
            for cx in range(3):
                want = [F32(parents[j, 0] + F32(F32(cx - 1.0) * s1[0])), parents[j, 1], F32(parents[j, 2] + F32(F32(ct - 0.5) * s1[2]))]
                assert p[j * 6 + (ct * 1 + 0) * 3 + cx].tolist() == want, (j, ct, cx)
        assert p[j * 6 + 1, 0] == parents[j, 0] and p[j * 6 + 4, 0] == parents[j, 0]      # refine 3: the parent in the middle
    # the product is rounded before the sum: a case where a fused multiply-add gives another float
    g = api.PoseGrid(center=(1.0, 0.0, 0.0), step=(0.8645471334457397,) * 3, count=(1, 1, 1), n_levels=2, refine=(4, 1, 1), k_parents=1)
    s = g.spacing(1)[0]; base = F32(4.560959339141846)
    o = F32(1.5)
    two_ops = F32(base + F32(o * s)); fused = F32(np.float64(base) + np.float64(o) * np.float64(s))
    assert two_ops != fused
    assert api.grid_level_poses(g, 1, [[base, 0.0, 0.0]])[3, 0] == two_ops


# ---- the GPU tests' cases, on the oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pyramids(po):
    c = gc.make_cases()
    cache, out = {}, {}
    for name, (g, coarse, last, k) in gc.cases(c).items():
        st0, act0, _ = gc.oracle_rows(po, c, api.grid_level_poses(g, 0), cache)
        mid = gc.mid_of(st0, act0)
        r, levels = gc.oracle_pyramid(po, c, g, gc.select_of(coarse, mid), gc.select_of(last, mid), k, cache)
        print(name, "counts", r.level_counts.tolist(), "k_parents", g.k_parents, "k", k)
        out[name] = (g, k, r, levels)
    return out


def test_cases_cannot_pass_vacuously(pyramids):
    cnt = {name: v[2].level_counts for name, v in pyramids.items()}
    kp = {name: v[0].k_parents for name, v in pyramids.items()}
    # a level with 0 < m < k_parents: pads beside real children at the next level
    assert 0 < cnt["some"][0, 1] == cnt["some"][0, 0] < kp["some"] and cnt["some"][1, 1] == kp["some"] < cnt["some"][1, 0] and cnt["some"][2, 1] > 0
    # m == k_parents < accepted
    assert cnt["two"][0, 1] == kp["two"] < cnt["two"][0, 0] and cnt["two"][1, 1] > 0
    assert cnt["one_parent"][0, 1] == 1 < cnt["one_parent"][0, 0] and cnt["two_parents"][0, 1] == 2
    # m == 0 at level 0, and first at a deeper level
    assert cnt["none_at_0"].tolist() == [[0, 0], [0, 0], [0, 0]]
    assert cnt["none_deeper"].tolist() == [[1, 1], [0, 0], [0, 0]]
    # a last level where k exceeds the accepted count
    g, k, r, _ = pyramids["four"]
    assert 0 < r.n_accepted == len(r.pose) < k
    # every level count of the cases meant to go all the way down is positive
    for name in ("single", "two", "three", "four", "one_cell", "big_level0", "big_children", "duplicates"):
        assert np.all(cnt[name][:, 1] > 0), name
    # past one select tile at level 0 and below it
    assert int(np.prod(pyramids["big_level0"][0].count)) == 2197 > api.SELECT_TILE
    g = pyramids["big_children"][0]
    assert g.k_parents * int(np.prod(g.refine)) == 2400 > api.SELECT_TILE and cnt["big_children"][0, 1] == 300


def test_duplicates_are_ranked_by_index(pyramids):
    g, k, r, levels = pyramids["duplicates"]
    poses0, _, idx0 = levels[0][:3]
    assert poses0[0].tobytes() == poses0[1].tobytes()      # a zero step with count 2: cells 2 i and 2 i + 1 are one pose
    st0 = levels[0][5]
    order = idx0.tolist()
    for a in range(0, 6, 2):
        if a in order and a + 1 in order:
            assert order.index(a) + 1 == order.index(a + 1)      # equal keys: adjacent, the lower index first
    assert any(a in order and a + 1 in order for a in range(0, 6, 2))
    assert st0[0].tobytes() == st0[1].tobytes() or order[0] % 2 == 0
    # refine (1, 1, 1): every level's hypotheses are the parents again, origins are kept
    assert levels[1][0].tobytes() == poses0[idx0].tobytes() and np.array_equal(levels[1][1], idx0)
    assert np.array_equal(r.origin, levels[2][1][levels[2][2]])
