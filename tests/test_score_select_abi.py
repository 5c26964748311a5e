"""CPU checks of lsm2d_score_select's ABI and of its restatement api.score_rank: the symbol is declared by include/lsm2d.h, bound by the Python mirror with its
sixteen arguments and exported by the gfx950 build; the three k_select_* kernels are in the library's code object; lsm2d_select_params has the layout gcc
gives it; the C++ mirror has its entries; score_rank applies the acceptance test and the ranking the header states, on hand-made statistics; and the workload
the GPU tests select from exercises every condition of the test (the oracle's statistics, no GPU)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import abi_checks
import score_select_cases as cases
import cpp_build
from conftest import ROOT

NAME = "lsm2d_score_select"


def test_score_select_symbol_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi, api
    abi_checks.assert_declared_bound_exported(NAME, 16)
    header = abi_checks.header()
    m = re.search(r"#define\s+LSM2D_SELECT_MAX_K\s+(\d+)", header)
    assert m and int(m.group(1)) == _capi.SELECT_MAX_K == api.SELECT_MAX_K
    # the tile the tests read: a power of two, at least two selections
    assert api.SELECT_TILE >= 2 * api.SELECT_MAX_K and api.SELECT_TILE & (api.SELECT_TILE - 1) == 0
    ksrc = open(os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "csrc", "lsm2d_k_select.h")).read()
    assert re.search(r"kSelectMaxK\s*=\s*%d\s*;" % api.SELECT_MAX_K, ksrc) and api.SELECT_TILE == 2 * api.SELECT_MAX_K
    assert re.search(r"kSelectTile\s*=\s*2\s*\*\s*kSelectMaxK\s*;", ksrc)


def test_score_select_kernels_are_in_the_code_object():
    abi_checks.assert_kernels_in_code_object((b"k_select_keys", b"k_select_tile", b"k_select_gather"))


def test_select_params_layout_matches_the_c_compiler(tmp_path):
    from srrg2_laser_slam_2d_amd import _capi
    st, cname = _capi.SelectParamsC, "lsm2d_select_params"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lsm2d.h"', 'int main(void) {', 'printf("%%zu", sizeof(%s));' % cname]
    lines += ['printf(" %s=%%zu", offsetof(%s, %s));' % (f, cname, f) for f, _ in st._fields_]
    lines += ['printf("\\n"); return 0; }']
    src = tmp_path / "layout.c"; src.write_text("\n".join(lines))
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    parts = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert int(parts[0]) == C.sizeof(st) == 12
    assert len(parts) == 4
    for kv in parts[1:]:
        k, v = kv.split("=")
        assert getattr(st, k).offset == int(v), (k, v)


def test_mirrors_have_score_select():
    from srrg2_laser_slam_2d_amd import api
    abi_checks.assert_mirrors_have(("score_select", "score_rank", "relocalize"), ("scoreSelect(", "lsm2d_score_select(", "relocalize("))
    d, r = api.SelectParams(), api.SelectParams.relocalizer()
    assert (d.min_inliers, d.max_chi_per_inlier, d.min_inlier_ratio) == (500, 0.1, 0.8)
    assert (r.min_inliers, r.max_chi_per_inlier, r.min_inlier_ratio) == (700, 0.01, 0.75)


def test_cpp_mirror_compiles():
    r = cpp_build.syntax_only("score_select_driver.cpp")
    assert r.returncode == 0, r.stderr[-3000:]


# ---- api.score_rank on hand-made statistics ----------------------------------------------------------------------------------------------------------------
def _stats(rows):
    """rows of (n_inliers, n_outliers, chi_inliers) as a structured array"""
    from srrg2_laser_slam_2d_amd import api
    st = np.zeros(len(rows), api.STATS_DTYPE)
    for i, (n_in, n_out, chi) in enumerate(rows):
        st[i] = (n_in + n_out, n_in, n_out, chi, 0.0, 0, 0)
    return st


def _list_of_structs(st):
    from srrg2_laser_slam_2d_amd._capi import IterationStats
    out = []
    for r in st:
        s = IterationStats()
        s.n_correspondences, s.n_inliers, s.n_outliers, s.chi_inliers = int(r["n_correspondences"]), int(r["n_inliers"]), int(r["n_outliers"]), float(r["chi_inliers"])
        out.append(s)
    return out


def _rank(st, sel, k):
    """score_rank on the structured array and on the list of structs: the same answer"""
    from srrg2_laser_slam_2d_amd import api
    idx, n_acc = api.score_rank(st, sel, k)
    idx2, n_acc2 = api.score_rank(_list_of_structs(st), sel, k)
    assert idx.dtype == np.int32 and np.array_equal(idx, idx2) and n_acc == n_acc2
    return idx.tolist(), n_acc


def test_score_rank_each_condition_rejects_one_item_and_passes_one():
    from srrg2_laser_slam_2d_amd import api
    sel = api.SelectParams(500, 0.1, 0.8)
    #            passes all      too few inliers  chi per inlier    inlier ratio      nothing found
    st = _stats([(600, 100, 30.0), (499, 0, 1.0), (600, 100, 61.0), (600, 151, 30.0), (0, 0, 0.0)])
    assert _rank(st, sel, 8) == ([0], 1)
    assert _rank(st, api.SelectParams(400, 0.2, 0.75), 8) == ([0, 3, 2, 1], 4)      # 600 inliers: chi 30 (index 0, then 3), then chi 61; then 499 inliers
    assert _rank(st, api.SelectParams(400, 0.2, 0.75), 2) == ([0, 3], 4)


def test_score_rank_thresholds_at_equality_accept():
    from srrg2_laser_slam_2d_amd import api
    st = _stats([(7, 2, 0.3), (3, 4, 0.7)])
    q = np.float32(0.3) / np.float32(7.0); r = np.float32(7.0) / np.float32(9.0)
    assert float(q) != 0.3 / 7.0 and float(r) != 7.0 / 9.0      # the fp32 quotients are not the fp64 ones: the test is in fp32
    assert _rank(st, api.SelectParams(7, float(q), float(r)), 4) == ([0], 1)
    below = float(np.nextafter(q, np.float32(0.0))); above = float(np.nextafter(r, np.float32(2.0)))
    assert _rank(st, api.SelectParams(7, below, float(r)), 4) == ([], 0)
    assert _rank(st, api.SelectParams(7, float(q), above), 4) == ([], 0)
    assert _rank(st, api.SelectParams(8, float(q), float(r)), 4) == ([], 0)
    # the other item's own fp32 quotient as the threshold: both pass, the one with more inliers first
    q2 = np.float32(0.7) / np.float32(3.0)
    assert _rank(st, api.SelectParams(3, float(q2), 0.0), 4)[0] == [0, 1]


def test_score_rank_nan_is_rejected_even_by_the_open_thresholds():
    from srrg2_laser_slam_2d_amd import api
    everything = api.SelectParams(0, float("inf"), 0.0)
    st = _stats([(5, 0, float("nan")), (5, 0, float("inf")), (0, 0, 0.0), (9, 90, 1e30)])
    assert _rank(st, everything, 8) == ([3, 1, 2], 3)
    assert _rank(st, api.SelectParams(0, float("nan"), 0.0), 8) == ([], 0)      # a NaN threshold: every comparison is false
    assert _rank(st, api.SelectParams(0, float("inf"), float("nan")), 8) == ([], 0)


def test_score_rank_ties_k_beyond_the_accepted_and_nothing_accepted():
    from srrg2_laser_slam_2d_amd import api
    everything = api.SelectParams(0, float("inf"), 0.0)
    lo = float(np.nextafter(np.float32(2.0), np.float32(0.0)))
    st = _stats([(8, 0, 2.0), (9, 0, 5.0), (8, 0, lo), (9, 0, 5.0), (8, 0, 2.0), (9, 1, 4.0)])
    # 9 inliers first: chi 4 (index 5), then the two chi 5 by index; then 8 inliers: the chi one ulp below 2 first, then the two chi 2 by index
    assert _rank(st, everything, 6) == ([5, 1, 3, 2, 0, 4], 6)
    assert _rank(st, everything, 100) == ([5, 1, 3, 2, 0, 4], 6)      # k beyond the accepted count
    assert _rank(st, everything, 1) == ([5], 6)
    assert _rank(st, api.SelectParams(10, float("inf"), 0.0), 3) == ([], 0)
    assert _rank(_stats([]), everything, 3) == ([], 0)
    with pytest.raises(ValueError):
        api.score_rank(st, everything, 0)


# ---- the GPU tests' workload, on the CPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_workload_exercises_every_condition(po, kind):
    """the thresholds test_gpu_score_select.py derives from the oracle's statistics make every condition alone reject and pass at least one hypothesis, and
    the selection is neither empty nor everything (the finder kinds the GPU file runs beyond these two assert the same there)"""
    from srrg2_laser_slam_2d_amd import api
    c = cases.make_cases()
    pairs = cases.oracle_pairs(po, c, kind)
    for robust in (po.ROBUST_NONE, po.ROBUST_CAUCHY):
        for order in (0, 1):
            _, _, st = cases.oracle_rows(po, c, kind, robust, order, pairs)
            sel = cases.middle_thresholds(st)
            cond = cases.conditions(st, sel)
            assert np.all(cond.any(axis=1)) and not np.any(cond.all(axis=1)), (kind, robust, order, sel)
            idx, n_acc = api.score_rank(st, sel, 64)
            assert 0 < n_acc < len(st) and n_acc == int(np.all(cond, axis=0).sum()), (kind, robust, order, n_acc)
