"""relocalizeSelect of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d_relocalize.hpp), built with plain g++ and run on the GPU against the existing
relocalize() of lsm2d.hpp on the same inputs: the driver restates relocalize()'s verdict and compares every output byte for byte; what it prints is also
api.relocalize_select's answer on the same inputs, bit for bit -- in both orders of summation."""
import math

import numpy as np
import pytest

import align_select_cases as cases
import cpp_build
from cpp_driver import f32_bits, f32_bits_arg, run_json, stats_json, write_bins
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("relocalize_select_cpp")
    c = cases.make_cases()
    return cpp_build.build("relocalize_select_driver.cpp", d, flags=("-O2", "-pthread")), write_bins(d, scan=c.scan, map=c.map, poses=c.poses), c


@pytest.mark.parametrize("order", [0, 1])
def test_cpp_relocalize_select(ctx, driver, order):
    exe, f, c = driver
    k_score, k = 64, 5
    ctx.set_option("sum_order", order)
    try:
        finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cases.COLS, -math.pi, math.pi, 0.3, 30.0))
        al = api.MultiAligner2D(ctx, max_iterations=cases.ITERATIONS, min_num_inliers=0)
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, robustifier=api.RobustifierCauchy(cases.TAU), min_num_correspondences=cases.MIN_CORR))
        first = al.compute_batch([c.scan], [c.map], c.poses, want_stats=True)
        n_in = first.last_stats()["n_inliers"][first.status == 0]
        al.param_min_num_inliers = int(np.sort(n_in)[len(n_in) // 2])      # the middle of the inlier counts: some hypotheses end NotEnoughInliers
        # ONE set of thresholds judges both stages here: a quarter of the way up the hypotheses' own first-iteration rows (align_select_cases.status_thresholds
        # on api.score_aligner's rows), so that plenty pass the scoring and the aligned rows of the selected are judged by values from the same scale
        _, _, st, active = api.score_aligner(al, [c.scan], [c.map], c.poses)
        sel = cases.status_thresholds(st[active > 0])
        got = api.relocalize_select(al, [c.scan], [c.map], c.poses, sel, k_score, None, k)
    finally:
        ctx.set_option("sum_order", 0)
    print("scored", got.n_scored_accepted, len(got.scored_index), "aligned", got.n_success, got.n_accepted, len(got.index))
    assert 0 < len(got.scored_index) and len(got.index) == min(k, got.n_accepted) and 0 < got.n_accepted
    r = run_json(exe, [f["scan"], f["map"], f["poses"], cases.COLS, repr(cases.TAU), cases.ITERATIONS, al.param_min_num_inliers, order, sel.min_inliers,
                       f32_bits_arg(sel.max_chi_per_inlier), f32_bits_arg(sel.min_inlier_ratio), k_score, k])
    assert r["n"] == len(c.poses) and r["n_empty"] == 0
    assert r["scored_equal"] == 1 and r["aligned_equal"] == 1      # relocalizeSelect against relocalize(), inside the driver
    assert r["scored_index"] == got.scored_index.tolist() and r["n_scored_accepted"] == got.n_scored_accepted
    assert r["index"] == got.index.tolist() and (r["n_accepted"], r["n_success"]) == (got.n_accepted, got.n_success)
    for j, row in enumerate(r["rows"]):
        assert row["pose"] == f32_bits(got.pose[j]) and row["H"] == f32_bits(got.information[j]) and row["iterations"] == int(got.iterations[j]), j
        assert {key: row[key] for key in ("counts", "chi", "digest")} == stats_json(got.last_stats[j]), j
