"""The three grouped select calls from C++, built with plain g++ and run on the GPU (tests/cpp/select_grouped_driver.cpp): through the bare C ABI and through
the host mirror's extension header (srrg2_laser_slam_2d_amd/host/lsm2d_grouped.hpp).  Per group, both routes' counts, indices and every row word equal what
the Python calls return on the same inputs, bit for bit."""
import math

import numpy as np
import pytest

import align_select_cases as cases
import cpp_build
import select_grouped_cases as gc
from cpp_driver import f32_bits_arg, run_json, write_bins
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu

K = gc.K_MIXED


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("select_grouped_cpp")
    c = cases.make_cases()
    files = write_bins(d, scan=c.scan, map=c.map, poses=c.poses, groups=gc.offsets(gc.SIZES_MIXED))
    return cpp_build.build("select_grouped_driver.cpp", d, flags=("-O2", "-pthread")), files, c


def _words(*parts):
    """rows of equal length [m, ...] side by side as one flat list of 32-bit words"""
    m = len(parts[0])
    if m == 0:
        return []
    cols = [np.ascontiguousarray(p).view(np.uint32).reshape(m, -1) for p in parts]
    return np.concatenate(cols, axis=1).ravel().tolist()


def _same(blocks, index, n_acc, n_suc, words, tag):
    assert len(blocks) == len(index), tag
    for g, blk in enumerate(blocks):
        assert blk["n_accepted"] == int(n_acc[g]) and blk["n_success"] == (-1 if n_suc is None else int(n_suc[g])), (tag, g)
        assert blk["index"] == index[g].tolist() and blk["words"] == words[g], (tag, g)


def test_cpp_grouped_calls(ctx, driver):
    exe, f, c = driver
    off = gc.offsets(gc.SIZES_MIXED)
    finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cases.COLS, -math.pi, math.pi, 0.3, 30.0))
    al = api.MultiAligner2D(ctx, max_iterations=cases.ITERATIONS, min_num_inliers=0)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, robustifier=api.RobustifierCauchy(cases.TAU), min_num_correspondences=cases.MIN_CORR))
    first = al.compute_batch([c.scan], [c.map], c.poses, want_stats=True)
    n_in = first.last_stats()["n_inliers"][first.status == 0]
    al.param_min_num_inliers = int(np.sort(n_in)[len(n_in) // 2])      # the middle of the inlier counts: some candidates end NotEnoughInliers
    res = al.compute_batch([c.scan], [c.map], c.poses, want_stats=True)
    sel = cases.middle_thresholds(res.last_stats()[res.status == 0])
    sp = al.param_slice_processors[0].slice_params()
    scan_set, map_set = api.CloudSet(ctx, c.scan), api.CloudSet(ctx, c.map)
    # (the unaligned hypotheses pass other thresholds than the aligned candidates: the middle ones of their own rows)
    sel_score = cases.middle_thresholds(api._stats_array(api.score_batch(ctx, sp, scan_set, map_set, c.poses)[2]))
    s_index, s_H, s_b, s_st, s_acc = api.score_select_grouped(ctx, sp, scan_set, map_set, c.poses, off, sel_score, K)
    a_index, a_H, a_b, a_st, a_act, a_acc = api.score_aligner_select_grouped(al, [scan_set], [map_set], c.poses, off, sel_score, K)
    got = api.align_select_grouped(al, [scan_set], [map_set], c.poses, off, sel, K)
    assert any(len(i) == K for i in got.index) and any(0 < len(i) < K for i in got.index) and np.any(got.n_accepted < got.n_success)
    assert int(s_acc.sum()) > 0 and int(a_acc.sum()) > 0
    r = run_json(exe, [f["scan"], f["map"], f["poses"], f["groups"], cases.COLS, repr(cases.TAU), cases.ITERATIONS, al.param_min_num_inliers, sel.min_inliers,
                       f32_bits_arg(sel.max_chi_per_inlier), f32_bits_arg(sel.min_inlier_ratio), K, sel_score.min_inliers, f32_bits_arg(sel_score.max_chi_per_inlier),
                       f32_bits_arg(sel_score.min_inlier_ratio)])
    G = len(off) - 1
    assert r["n"] == len(c.poses) and r["n_groups"] == G
    s_words = [_words(s_H[g], s_b[g], s_st[g]) for g in range(G)]
    a_words = [_words(a_H[g], a_b[g], a_st[g], a_act[g]) for g in range(G)]
    g_words = [_words(got.pose[g], got.information[g], got.iterations[g], got.last_stats[g]) for g in range(G)]
    for route in ("abi", "mirror"):
        _same(r["score_" + route], s_index, s_acc, None, s_words, "score_" + route)
        _same(r["score_aligner_" + route], a_index, a_acc, None, a_words, "score_aligner_" + route)
        _same(r["align_" + route], got.index, got.n_accepted, got.n_success, g_words, "align_" + route)
