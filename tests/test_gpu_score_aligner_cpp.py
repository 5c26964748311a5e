"""lsm2d_score_aligner_batch through the bare C ABI, and scoreAligner / scoreAlignerSelect / the two-slice relocalize of the C++ host mirror
(srrg2_laser_slam_2d_amd/host/lsm2d.hpp), built with plain g++ and run on the GPU: every row, the selection and the relocalisation's results equal
api.score_aligner / api.score_aligner_select / api.relocalize on the same inputs, bit for bit; inside the driver the mirror equals the ABI, every selected
row equals scoreAligner's, and relocalize equals the entry points called by hand."""
import math

import numpy as np
import pytest

import score_aligner_cases as cases
import cpp_build
from cpp_driver import f32_bits, f32_bits_arg, run_json, stats_json, write_bins
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("score_aligner_cpp")
    exe = cpp_build.build("score_aligner_driver.cpp", d)
    c = cases.make_inputs()
    rng = np.random.default_rng(4)
    c.scan = (np.arange(24) % c.n).astype(np.int32)      # 24 hypotheses over the four scans, some of them far from everything
    c.hyp = (c.poses[c.scan] + rng.uniform(-0.03, 0.03, (24, 3)).astype(np.float32)).astype(np.float32)
    c.hyp[5::9, :2] += np.float32(500.0)
    c.which = [0, 2]      # the two projective slices, with the offsets S0 and S1
    c.sensors = [cases.S_OFF[0], cases.S_OFF[1]]
    c.fixed_h = [[c.fixed[0][i] for i in c.scan], [c.fixed[1][i] for i in c.scan]]      # one cloud per hypothesis, moved by the slice's S^-1
    for s in range(2):
        off = np.zeros(25, np.int32); off[1:] = np.cumsum([len(a) for a in c.fixed_h[s]])
        write_bins(d, **{"fixed%d" % s: np.concatenate(c.fixed_h[s]), "off%d" % s: off, "moving%d" % s: c.moving[c.which[s]]})
    c.priors = [cases.asym_prior(X, seed=2) for X in c.hyp]
    write_bins(d, priors=np.concatenate([np.concatenate([z, om.ravel()]) for z, om in c.priors]).astype(np.float32), poses=c.hyp)
    return exe, d, c


def _same_row(row, H, b, st, active, tag):
    assert row["H"] == f32_bits(H) and row["b"] == f32_bits(b) and row["active"] == int(active), tag
    assert {key: row[key] for key in ("counts", "chi", "digest")} == stats_json(st), tag


@pytest.mark.parametrize("with_prior", [0, 1], ids=["plain", "prior"])
@pytest.mark.parametrize("order", [0, 1], ids=["tree", "reference"])
def test_cpp_score_aligner(ctx, driver, order, with_prior):
    exe, d, c = driver
    k = 6
    sel = api.SelectParams(300, 0.05, 0.5)
    priors = c.priors if with_prior else None
    ctx.set_option("sum_order", order)
    try:
        al = api.MultiAligner2D(ctx, max_iterations=8, min_num_inliers=10)
        for s in range(2):
            _, cols, _, tau = cases.SLICES[c.which[s]]
            al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(
                api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, 30.0)), sensor_in_robot=c.sensors[s],
                robustifier=api.RobustifierCauchy(tau), min_num_correspondences=10))
        fixed = [api.CloudSet(ctx, np.concatenate(c.fixed_h[s]), np.concatenate([[0], np.cumsum([len(a) for a in c.fixed_h[s]])]).astype(np.int32)) for s in range(2)]
        moving = [api.CloudSet(ctx, c.moving[c.which[s]]) for s in range(2)]
        H, b, st, active = api.score_aligner(al, fixed, moving, c.hyp, priors)
        index, sH, sb, sst, sact, n_acc = api.score_aligner_select(al, fixed, moving, c.hyp, sel, k, priors)
        rel = api.relocalize(al, fixed, moving, c.hyp, sel, k, priors=priors)
        by_hand = al.compute_batch(fixed, moving, c.hyp[index], priors=None if priors is None else [priors[int(i)] for i in index],
                                   fixed_index=np.stack([index, index]), want_stats=True)
    finally:
        ctx.set_option("sum_order", 0)
    r = run_json(exe, [d, order, sel.min_inliers, f32_bits_arg(sel.max_chi_per_inlier), f32_bits_arg(sel.min_inlier_ratio), k, with_prior])
    assert r["n"] == len(c.hyp) and r["mirror_equals_abi"] == 1 and r["rows_equal_score_aligner"] == 1 and r["relocalize_equals_by_hand"] == 1 and r["n_empty"] == 0
    assert np.any(active == 0) and np.any(active == 2)
    for i, row in enumerate(r["all"]):
        _same_row(row, H[i], b[i], st[i], active[i], ("all", i))
    assert len(index) == k and n_acc > k      # a selection that is cut at k
    assert r["n_accepted"] == n_acc and r["index"] == index.tolist()
    for j, row in enumerate(r["rows"]):
        _same_row(row, sH[j], sb[j], sst[j], sact[j], ("selected", j))
    # the two-slice relocalize: the Python route is its own entry points called by hand, and the C++ route gives its bytes
    assert np.array_equal(rel.index, index) and rel.n_accepted == n_acc
    assert by_hand.pose.tobytes() == rel.result.pose.tobytes() and np.array_equal(by_hand.status, rel.result.status)
    rr = r["relocalize"]
    assert rr["n_accepted"] == rel.n_accepted and len(rr["items"]) == len(rel.index)
    last = rel.result.last_stats()
    for j, it in enumerate(rr["items"]):
        assert it["pose"] == f32_bits(rel.result.pose[j]) and it["status"] == int(rel.result.status[j]) and it["iterations"] == int(rel.result.iterations[j]), j
        assert it["accepted"] == int(rel.accepted[j]), j
        assert {key: it[key] for key in ("counts", "chi", "digest")} == stats_json(last[j]), j
    assert any(it["status"] == 0 for it in rr["items"])


def test_one_slice_relocalize_takes_todays_path(ctx, driver):
    """a one-slice aligner with single sets and no prior: relocalize is score_select + compute_batch as before -- not the aligner scoring"""
    _, _, c = driver
    al = api.MultiAligner2D(ctx, max_iterations=4, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(
        api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)), robustifier=api.RobustifierCauchy(0.05),
        min_num_correspondences=10))
    fixed = api.CloudSet(ctx, np.concatenate(c.fixed[2]), np.concatenate([[0], np.cumsum([len(a) for a in c.fixed[2]])]).astype(np.int32))
    moving = api.CloudSet(ctx, c.moving[0])
    sel = api.SelectParams(300, 0.05, 0.5)
    rel = api.relocalize(al, fixed, moving, c.poses, sel, 3)
    index, _, _, sst, n_acc = api.score_select(ctx, al.param_slice_processors[0].slice_params(), fixed, moving, c.poses, sel, 3)
    assert np.array_equal(rel.index, index) and rel.n_accepted == n_acc and rel.score_stats.tobytes() == sst.tobytes()
    # ... and as lists of one set it goes through the aligner scoring: the same selection, the digest being salted with slice 0 in both
    rel2 = api.relocalize(al, [fixed], [moving], c.poses, sel, 3)
    assert np.array_equal(rel2.index, index) and rel2.score_stats.tobytes() == sst.tobytes() and rel2.result.pose.tobytes() == rel.result.pose.tobytes()
