"""alignSelect and LoopClosureSweep::computeSelect of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d.hpp), built with plain g++ and run on the GPU:
the selection, the counts and every row equal api.align_select on the same inputs, bit for bit -- alignSelect in both orders of summation, computeSelect (two
shards on one device, merged on the host) in the default order, the only one a sweep's contexts run in."""
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
    d = tmp_path_factory.mktemp("align_select_cpp")
    c = cases.make_cases()
    return cpp_build.build("align_select_driver.cpp", d, flags=("-O2", "-pthread")), write_bins(d, scan=c.scan, map=c.map, poses=c.poses), c


def _same(block, got):
    assert block["n_accepted"] == got.n_accepted and block["n_success"] == got.n_success and block["index"] == got.index.tolist()
    assert len(block["rows"]) == len(got.index)
    for j, row in enumerate(block["rows"]):
        assert row["pose"] == f32_bits(got.pose[j]) and row["H"] == f32_bits(got.information[j]) and row["iterations"] == int(got.iterations[j]), j
        assert {key: row[key] for key in ("counts", "chi", "digest")} == stats_json(got.last_stats[j]), j


@pytest.mark.parametrize("order", [0, 1])
def test_cpp_align_select(ctx, driver, order):
    exe, f, c = driver
    k = 9
    ctx.set_option("sum_order", order)
    try:
        finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cases.COLS, -math.pi, math.pi, 0.3, 30.0))
        al = api.MultiAligner2D(ctx, max_iterations=cases.ITERATIONS, min_num_inliers=0)
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, robustifier=api.RobustifierCauchy(cases.TAU), min_num_correspondences=cases.MIN_CORR))
        first = al.compute_batch([c.scan], [c.map], c.poses, want_stats=True)
        n_in = first.last_stats()["n_inliers"][first.status == 0]
        al.param_min_num_inliers = int(np.sort(n_in)[len(n_in) // 2])      # the middle of the inlier counts: some candidates end NotEnoughInliers
        res = al.compute_batch([c.scan], [c.map], c.poses, want_stats=True)
        sel = cases.middle_thresholds(res.last_stats()[res.status == 0])
        got = api.align_select(al, [c.scan], [c.map], c.poses, sel, k)
    finally:
        ctx.set_option("sum_order", 0)
    assert len(got.index) == k and k < got.n_accepted < got.n_success < len(c.poses)      # a selection that is cut at k; the status term and the thresholds both reject
    r = run_json(exe, [f["scan"], f["map"], f["poses"], cases.COLS, repr(cases.TAU), cases.ITERATIONS, al.param_min_num_inliers, order, sel.min_inliers,
                       f32_bits_arg(sel.max_chi_per_inlier), f32_bits_arg(sel.min_inlier_ratio), k])
    assert r["n"] == len(c.poses) and r["n_empty"] == 0
    _same(r["align_select"], got)
    if order == 0:
        _same(r["compute_select"], got)
    else:
        assert r["compute_select"] is None
