"""scoreGridSelect and relocalizeGrid of the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d_score_grid.hpp), built with plain g++ and run on the GPU:
what the driver prints is api.score_grid_select's and api.relocalize_grid's answer on the same inputs, bit for bit -- in both orders of summation."""
import math

import pytest

import align_select_cases as ac
import cpp_build
import score_grid_cases as gc
from cpp_driver import f32_bits, f32_bits_arg, run_json, stats_json, write_bins
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_grid_cpp")
    c = gc.make_cases()
    return cpp_build.build("score_grid_driver.cpp", d, flags=("-O2", "-pthread")), write_bins(d, scan=c.scan, map=c.map), c


def _sel_args(sel):
    return [int(sel.min_inliers), f32_bits_arg(sel.max_chi_per_inlier), f32_bits_arg(sel.min_inlier_ratio)]


@pytest.mark.parametrize("order", [0, 1])
def test_cpp_score_grid(ctx, driver, order):
    exe, f, c = driver
    g, _, _, _ = gc.cases(c)["some"]      # three levels, 0 < m < k_parents at level 0: pads
    k, k_align = 32, 5
    ctx.set_option("sum_order", order)
    try:
        finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(ac.COLS, -math.pi, math.pi, 0.3, 30.0))
        al = api.MultiAligner2D(ctx, max_iterations=ac.ITERATIONS, min_num_inliers=0)
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, robustifier=api.RobustifierCauchy(ac.TAU), min_num_correspondences=ac.MIN_CORR))
        _, _, st, active = api.score_aligner(al, [c.scan], [c.map], api.grid_level_poses(g, 0))
        mid = gc.mid_of(st, active)
        got = api.score_grid_select(al, [c.scan], [c.map], g, mid, mid, k)
        rel = api.relocalize_grid(al, [c.scan], [c.map], g, mid, mid, k, None, k_align)
    finally:
        ctx.set_option("sum_order", 0)
    print("counts", got.level_counts.tolist(), "aligned", rel.aligned.n_success, rel.aligned.n_accepted, len(rel.aligned.index))
    assert 0 < got.level_counts[0, 1] < g.k_parents and len(got.pose) > 0 and len(rel.aligned.index) > 0
    args = [f["scan"], f["map"], ac.COLS, repr(ac.TAU), order] + f32_bits(g.center) + f32_bits(g.step)
    args += list(g.count) + [g.n_levels] + list(g.refine) + [g.k_parents] + _sel_args(mid) + _sel_args(mid) + [k, ac.ITERATIONS, k_align]
    r = run_json(exe, args)
    assert r["scored_again_equal"] == 1
    assert r["level_counts"] == got.level_counts.tolist() and r["n_accepted"] == got.n_accepted and r["origin"] == got.origin.tolist()
    assert len(r["rows"]) == len(got.pose)
    for j, row in enumerate(r["rows"]):
        assert row["pose"] == f32_bits(got.pose[j]) and row["H"] == f32_bits(got.H[j]) and row["b"] == f32_bits(got.b[j]) and row["active"] == int(got.active[j]), j
        assert {key: row[key] for key in ("counts", "chi", "digest")} == stats_json(got.stats[j]), j
    a = r["aligned"]
    assert (a["n_accepted"], a["n_success"]) == (rel.aligned.n_accepted, rel.aligned.n_success) and a["index"] == rel.aligned.index.tolist()
    assert a["pose"] == [f32_bits(p) for p in rel.aligned.pose]
