"""scoreSelect and relocalize of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d.hpp), built with plain g++ and run on the GPU: the selection, its rows
and the relocalisation's results equal api.score_select / api.relocalize on the same inputs, bit for bit, and every selected row equals the mirror's own
scoreBatch row (checked inside the driver)."""
import math

import pytest

import score_select_cases as cases
import cpp_build
from cpp_driver import f32_bits, f32_bits_arg, run_json, stats_json, write_bins
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_select_cpp")
    c = cases.make_cases()
    return cpp_build.build("score_select_driver.cpp", d), write_bins(d, scan=c.scan, map=c.map, poses=c.poses), c


@pytest.mark.parametrize("order", [0, 1])
def test_cpp_score_select(ctx, driver, order):
    exe, f, c = driver
    k = 9
    ctx.set_option("sum_order", order)
    try:
        finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cases.COLS, -math.pi, math.pi, 0.3, 30.0))
        al = api.MultiAligner2D(ctx, max_iterations=8, min_num_inliers=10)
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, robustifier=api.RobustifierCauchy(cases.TAU), min_num_correspondences=10))
        sp = al.param_slice_processors[0].slice_params()
        _, _, st = api.score_batch(ctx, sp, c.scan, c.map, c.poses)
        sel = cases.middle_thresholds(api._stats_array(st))
        index, H, b, sst, n_acc = api.score_select(ctx, sp, c.scan, c.map, c.poses, sel, k)
        rel = api.relocalize(al, c.scan, c.map, c.poses, sel, k)
    finally:
        ctx.set_option("sum_order", 0)
    r = run_json(exe, [f["scan"], f["map"], f["poses"], cases.COLS, repr(cases.TAU), order, sel.min_inliers, f32_bits_arg(sel.max_chi_per_inlier),
                       f32_bits_arg(sel.min_inlier_ratio), k])
    assert r["n"] == len(c.poses) and r["rows_equal_score_batch"] == 1 and r["n_empty"] == 0
    assert len(index) == k and n_acc > k      # a selection that is cut at k
    assert r["n_accepted"] == n_acc and r["index"] == index.tolist()
    for j, row in enumerate(r["rows"]):
        assert row["H"] == f32_bits(H[j]) and row["b"] == f32_bits(b[j]), j
        assert {key: row[key] for key in ("counts", "chi", "digest")} == stats_json(sst[j]), j
    rr = r["relocalize"]
    assert rr["n_accepted"] == rel.n_accepted and rr["index"] == rel.index.tolist() and len(rr["items"]) == len(rel.index)
    last = rel.result.last_stats()
    for j, it in enumerate(rr["items"]):
        assert it["pose"] == f32_bits(rel.result.pose[j]) and it["status"] == int(rel.result.status[j]) and it["iterations"] == int(rel.result.iterations[j]), j
        assert it["accepted"] == int(rel.accepted[j]), j
        assert {key: it[key] for key in ("counts", "chi", "digest")} == stats_json(last[j]), j
    assert any(it["status"] == 0 for it in rr["items"])
