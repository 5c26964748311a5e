"""GPU tests of the latency kernel in the reference's order of summation (k_align_pair<true>, "sum_order" 1): the live tracker's call -- one alignment, one
or two projective slices -- runs on the latency kernel with H, b and the chi^2 statistics added pair after pair, and equals both the sequential fp32
oracle (lsmo_align_f, device_order = 0) and k_align_seq (align_path 1) BIT FOR BIT: status, iteration count, pose, information matrix, every iteration's
counts, chi^2 sums and pair digest.  No tolerance appears in this file."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import cpp_build

from srrg2_laser_slam_2d_amd import api, synth

pytestmark = pytest.mark.gpu


@pytest.fixture()
def seq_ctx(ctx):
    ctx.set_option("sum_order", 1)
    try:
        yield ctx
    finally:
        ctx.set_option("sum_order", 0)
        ctx.set_option("align_path", 0)


def _projector(cols, rmax=20.0):
    return api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, rmax)


def _oslice(po, sl):
    sp = sl.slice_params()
    return po.slice_params(finder=sp.finder, canvas_cols=sp.projector.canvas_cols, angle_min=sp.projector.angle_min, angle_max=sp.projector.angle_max,
                           range_min=sp.projector.range_min, range_max=sp.projector.range_max, col_offset=sp.projector.col_offset,
                           point_distance=sp.point_distance, normal_cos=sp.normal_cos, max_distance=sp.max_distance, resolution=sp.resolution,
                           robustifier=sp.robustifier, chi_threshold=sp.chi_threshold, min_num_correspondences=sp.min_num_correspondences,
                           sensor_in_robot=tuple(sp.sensor_in_robot))


def _assert_bitwise(res, i, ro, tag):
    assert int(res.status[i]) == ro["status"] and int(res.iterations[i]) == ro["iterations"], (tag, int(res.status[i]), ro["status"], int(res.iterations[i]), ro["iterations"])
    assert np.array_equal(res.pose[i], ro["pose"]), (tag, "pose", res.pose[i].tolist(), ro["pose"].tolist())
    assert np.array_equal(res.information[i], ro["H"]), (tag, "H")
    if res.stats is not None:
        for k in range(ro["iterations"]):
            g, o = res.stats[i][k], ro["stats"][k]
            assert (int(g["n_correspondences"]), int(g["n_inliers"]), int(g["n_outliers"])) == (o.n_corr, o.n_in, o.n_out), (tag, "counts", k)
            assert np.float32(g["chi_inliers"]) == np.float32(o.chi_in) and np.float32(g["chi_outliers"]) == np.float32(o.chi_out), (tag, "chi", k)
            assert (int(g["pair_digest_hi"]) << 32 | int(g["pair_digest_lo"])) == (o.pair_digest_hi << 32 | o.pair_digest_lo), (tag, "pair digest", k)


def _assert_same(a, b, tag):
    """two device results, field for field"""
    assert np.array_equal(a.status, b.status) and np.array_equal(a.iterations, b.iterations), tag
    assert np.array_equal(a.pose, b.pose) and np.array_equal(a.information, b.information), tag
    if a.stats is not None:
        assert np.array_equal(a.stats, b.stats), tag
    if a.pairs is not None:
        for pa, pb in zip(a.pairs, b.pairs):
            assert all(np.array_equal(x, y) for x, y in zip(pa, pb)), tag


class Scene:
    """a world, a map (the moving cloud) and scans of every slice from one robot pose (the fixed clouds)"""

    def __init__(self, seed, map_points, beams, sensors, n=1):
        self.world = synth.make_world(seed)
        self.map = synth.make_map(self.world, map_points, noise_sigma=0.003, seed=seed + 1)
        robots = synth.sample_poses(self.world, n, seed=seed + 2)
        rng = np.random.default_rng(seed)
        self.x0 = synth.invert_poses(synth.compose_poses(robots, rng.uniform(-0.04, 0.04, (n, 3)))).astype(np.float32)
        self.scans = []
        for s, (nb, S) in enumerate(zip(beams, sensors)):
            pts, offs = synth.make_scans(self.world, synth.compose_poses(robots, np.tile(np.asarray(S, np.float64)[None, :], (n, 1))), n_beams=nb,
                                         noise_sigma=0.003, seed=seed + 10 + s)
            self.scans.append((pts, offs))

    def fixed_np(self, s, i=0):
        pts, offs = self.scans[s]
        return pts[offs[i]:offs[i + 1]]


def _aligner(ctx, cols, sensors, cauchy, min_corr=5, its=8, **kw):
    al = api.MultiAligner2D(ctx, max_iterations=its, min_num_inliers=10, termination_chi_epsilon=kw.get("eps", 0.0))
    al.param_enable_inlier_only_runs = bool(kw.get("inlier_runs", False))
    al.param_keep_only_inlier_correspondences = bool(kw.get("keep_inliers", False))
    for s, c in enumerate(cols):
        f = api.CorrespondenceFinderProjective2f(ctx, _projector(c), 0.6, 0.7)
        rob = api.RobustifierCauchy(0.02) if cauchy[s] else None
        mc = min_corr[s] if isinstance(min_corr, (list, tuple)) else min_corr
        S = np.float32(sensors[s])
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(f, sensor_in_robot=S, robustifier=rob, min_num_correspondences=mc) if S.any()
                                         else api.AlignerSliceProcessorLaser2D(f, robustifier=rob, min_num_correspondences=mc))
    return al


def _check_case(ctx, po, al, fixed_sets, moving_sets, x0, priors, fixed_np, moving_np, tag, want_pairs=False):
    """align_path 3 (the new kernel) against align_path 1 (k_align_seq) and the sequential oracle"""
    ctx.set_option("align_path", 3)
    r3 = al.compute_batch(fixed_sets, moving_sets, x0, priors=priors, want_stats=True, want_pairs=want_pairs)
    assert ctx.get_option("last_align_path") == 3, tag
    ctx.set_option("align_path", 1)
    r1 = al.compute_batch(fixed_sets, moving_sets, x0, priors=priors, want_stats=True, want_pairs=want_pairs)
    assert ctx.get_option("last_align_path") == 1, tag
    ctx.set_option("align_path", 0)
    _assert_same(r3, r1, (tag, "latency kernel != k_align_seq"))
    oslices = [_oslice(po, sl) for sl in al.param_slice_processors]
    for i in range(len(x0)):
        kw = dict(prior_z=priors[i][0], prior_omega=priors[i][1]) if priors else {}
        ap = po.aligner_params(al.param_max_iterations, min_num_inliers=al.param_min_num_inliers, termination_chi_epsilon=al.param_termination_chi_epsilon,
                               enable_inlier_only_runs=al.param_enable_inlier_only_runs, keep_only_inlier_correspondences=al.param_keep_only_inlier_correspondences, **kw)
        ro = po.align(ap, oslices, [f[i] for f in fixed_np], moving_np, x0[i], want_pairs=want_pairs)
        _assert_bitwise(r3, i, ro, (tag, i))
        if want_pairs:
            for s in range(len(oslices)):
                assert np.array_equal(r3.pairs[i][s], ro["pairs"][s]), (tag, "pairs", i, s)
    return r3


def test_path_automatic_single_alignment_and_explicit_path_3(seq_ctx, po):
    """With "sum_order" 1 a two-slice single alignment (the tracker's call) takes the latency kernel by itself; align_path 3 takes it for any n
    (here 1, 2, 17 and 256), all bit-identical to k_align_seq.  Automatic selection for n >= 2 stays on k_align_seq."""
    ctx = seq_ctx
    sensors = [(0.2, 0.1, 0.1), (-0.3, 0.0, math.pi)]
    sc = Scene(5, 900, (721, 721), sensors, n=4)
    al = _aligner(ctx, (721, 721), sensors, (True, False))
    mv = api.CloudSet(ctx, sc.map)
    fixed = [api.CloudSet(ctx, *sc.scans[s]) for s in range(2)]
    pri = [(sc.x0[0].copy(), np.diag([100.0, 100.0, 100.0]).astype(np.float32))]
    f1 = [api.CloudSet(ctx, sc.fixed_np(s, 0)) for s in range(2)]
    r_auto = al.compute_batch(f1, [mv, mv], sc.x0[:1], priors=pri, want_stats=True)
    assert ctx.get_option("last_align_path") == 3
    ctx.set_option("align_path", 1)
    r_seq = al.compute_batch(f1, [mv, mv], sc.x0[:1], priors=pri, want_stats=True)
    ctx.set_option("align_path", 0)
    _assert_same(r_auto, r_seq, "automatic n = 1")
    r4 = al.compute_batch(fixed, [mv, mv], sc.x0, want_stats=True)
    assert ctx.get_option("last_align_path") == 1      # n = 4, automatic: k_align_seq
    for n in (1, 2, 17, 256):
        idx = (np.arange(n, dtype=np.int32) % 4)
        fi = np.stack([idx, idx])
        x0 = sc.x0[idx].copy(); x0[:, 0] += np.linspace(-0.01, 0.01, n, dtype=np.float32)
        ctx.set_option("align_path", 3)
        r3 = al.compute_batch(fixed, [mv, mv], x0, fixed_index=fi, want_stats=True)
        assert ctx.get_option("last_align_path") == 3, n
        ctx.set_option("align_path", 1)
        r1 = al.compute_batch(fixed, [mv, mv], x0, fixed_index=fi, want_stats=True)
        ctx.set_option("align_path", 0)
        _assert_same(r3, r1, ("explicit path 3", n))
        oslices = [_oslice(po, sl) for sl in al.param_slice_processors]
        for i in sorted({0, n - 1}):
            ro = po.align(po.aligner_params(8, min_num_inliers=10), oslices, [sc.fixed_np(s, int(idx[i])) for s in range(2)], [sc.map, sc.map], x0[i])
            _assert_bitwise(r3, i, ro, ("explicit path 3", n, i))
    assert r4.status.shape == (4,)


@pytest.mark.parametrize("cols", [(300,), (512,), (513,), (721,), (1081,), (1500,), (721, 721), (721, 1081), (1500, 300), (513, 512)])
def test_widths_one_and_two_slices(seq_ctx, po, cols):
    """Canvases of 300 .. 1500 columns (one to three trips of 512), mixed widths across the two slices (the narrower slice joins the wider one's extra
    trips with no records); Cauchy on slice 0 only, sensor offsets, a prior on every other width; a clipped-scene-sized moving cloud (on chip)."""
    ctx = seq_ctx
    ns = len(cols)
    sensors = [(0.2, -0.1, 0.5), (-0.25, 0.05, -2.9)][:ns]
    sc = Scene(20 + sum(cols) % 97, 950, tuple(min(c, 1081) for c in cols), sensors)
    al = _aligner(ctx, cols, sensors, (True, False)[:ns])
    mv = api.CloudSet(ctx, sc.map)
    fixed = [api.CloudSet(ctx, sc.fixed_np(s)) for s in range(ns)]
    pri = [(sc.x0[0].copy(), np.diag([30.0, 20.0, 50.0]).astype(np.float32))] if cols[0] % 2 else None
    _check_case(ctx, po, al, fixed, [mv] * ns, sc.x0, pri, [[sc.fixed_np(s)] for s in range(ns)], [sc.map] * ns, ("widths", cols))


def test_big_moving_cloud_cauchy_both_slices_no_sensor(seq_ctx, po):
    """moving clouds of more than kPairMovCap (1024) points: gathered from global memory; 1025 points and a 20 000-point map; Cauchy on both slices"""
    ctx = seq_ctx
    for pts, cols in ((1025, (721, 721)), (20000, (1081, 721))):
        sc = Scene(31, pts, (721, 541), [(0.0, 0.0, 0.0), (0.0, 0.0, 0.0)])
        al = _aligner(ctx, cols, [(0, 0, 0), (0, 0, 0)], (True, True))
        mv = api.CloudSet(ctx, sc.map)
        fixed = [api.CloudSet(ctx, sc.fixed_np(s)) for s in range(2)]
        _check_case(ctx, po, al, fixed, [mv, mv], sc.x0, None, [[sc.fixed_np(s)] for s in range(2)], [sc.map, sc.map], ("big moving", pts))


def test_skipped_and_empty_slices_and_failure_statuses(seq_ctx, po):
    """a slice skipped by min_num_correspondences; a slice with zero pairs (its scan far outside the map); NOT_ENOUGH_CORRESPONDENCES (a start pose
    far away); SINGULAR_H (one straight wall: nothing constrains the motion along it)."""
    ctx = seq_ctx
    sensors = [(0.2, -0.1, 0.5), (-0.25, 0.05, -2.9)]
    sc = Scene(41, 900, (721, 721), sensors)
    mv = api.CloudSet(ctx, sc.map)
    fnp = [sc.fixed_np(0), sc.fixed_np(1)]
    fixed = [api.CloudSet(ctx, f) for f in fnp]
    al = _aligner(ctx, (721, 721), sensors, (True, False), min_corr=(5, 100000))
    _check_case(ctx, po, al, fixed, [mv, mv], sc.x0, None, [[f] for f in fnp], [sc.map] * 2, "slice 1 skipped")
    far = fnp[1].copy(); far[:, :2] += 1000.0
    fixed_far = [fixed[0], api.CloudSet(ctx, far)]
    al = _aligner(ctx, (721, 721), sensors, (True, False))
    r = _check_case(ctx, po, al, fixed_far, [mv, mv], sc.x0, None, [[fnp[0]], [far]], [sc.map] * 2, "slice 1 without pairs")
    assert all(int(st["n_correspondences"]) > 0 for st in r.stats[0][: r.iterations[0]])
    x_far = sc.x0.copy(); x_far[:, 0] += 500.0
    r = _check_case(ctx, po, al, fixed, [mv, mv], x_far, None, [[f] for f in fnp], [sc.map] * 2, "not enough correspondences")
    assert int(r.status[0]) == 1      # LSM2D_NOT_ENOUGH_CORRESPONDENCES
    # one straight wall, normals all (-1, 0): H's row of the translation along the wall is zero
    ys = np.linspace(-1.0, 1.0, 300, dtype=np.float32)
    wall = np.stack([np.full_like(ys, 2.0), ys, np.full_like(ys, -1.0), np.zeros_like(ys)], axis=1).astype(np.float32)
    al = _aligner(ctx, (721,), [(0, 0, 0)], (False,))
    r = _check_case(ctx, po, al, [api.CloudSet(ctx, wall)], [api.CloudSet(ctx, wall)], np.zeros((1, 3), np.float32), None, [[wall]], [wall], "singular")
    assert int(r.status[0]) == 3


def test_termination_inlier_runs_and_kept_pairs(seq_ctx, po):
    """termination_chi_epsilon; enable_inlier_only_runs (records carry the 0 / 1 weights) with keep_only_inlier_correspondences through
    lsm2d_align_batch_pairs (the correspondences the aligner leaves in its slices)"""
    ctx = seq_ctx
    sensors = [(0.2, 0.1, 0.1), (-0.3, 0.0, math.pi)]
    sc = Scene(53, 1000, (721, 721), sensors)
    mv = api.CloudSet(ctx, sc.map)
    fnp = [sc.fixed_np(0), sc.fixed_np(1)]
    fixed = [api.CloudSet(ctx, f) for f in fnp]
    pri = [(sc.x0[0].copy(), np.diag([100.0, 100.0, 100.0]).astype(np.float32))]
    for kw in (dict(eps=1e-3), dict(inlier_runs=True, keep_inliers=True), dict(eps=1e-3, inlier_runs=True, keep_inliers=True)):
        al = _aligner(ctx, (721, 721), sensors, (True, True), its=10, **kw)
        _check_case(ctx, po, al, fixed, [mv, mv], sc.x0, pri, [[f] for f in fnp], [sc.map] * 2, ("options", kw), want_pairs=True)


def test_begin_wait_and_deferred_unpack(seq_ctx, po):
    """the begin / wait form; a fixed set still in its pinned upload (n = 1: the kernel's prologue unpacks it), in both slices"""
    ctx = seq_ctx
    sensors = [(0.2, 0.1, 0.1), (-0.3, 0.0, math.pi)]
    sc = Scene(61, 900, (721, 721), sensors)
    mv = api.CloudSet(ctx, sc.map)
    fnp = [sc.fixed_np(0), sc.fixed_np(1)]
    al = _aligner(ctx, (721, 721), sensors, (True, False), its=10)
    oslices = [_oslice(po, sl) for sl in al.param_slice_processors]
    pri = [(sc.x0[0].copy(), np.diag([100.0, 100.0, 100.0]).astype(np.float32))]
    ro = po.align(po.aligner_params(10, min_num_inliers=10, prior_z=pri[0][0], prior_omega=pri[0][1]), oslices, fnp, [sc.map] * 2, sc.x0[0])
    fixed = [api.CloudSet(ctx, f) for f in fnp]
    prep = al.prepare_batch(fixed, [mv, mv], sc.x0, priors=pri, want_stats=True)
    prep.begin(); res = prep.wait(copy=True)
    assert ctx.get_option("last_align_path") == 3
    _assert_bitwise(res, 0, ro, "begin / wait")
    sets = [api.CloudSet.reserved(ctx, 1024), api.CloudSet.reserved(ctx, 1024)]
    for s in range(2):
        sets[s].upload(fnp[s])
    res = al.compute_batch(sets, [mv, mv], sc.x0, priors=pri, want_stats=True)
    assert ctx.get_option("last_align_path") == 3
    _assert_bitwise(res, 0, ro, "deferred unpack")
    for s in range(2):
        assert np.array_equal(sets[s].download(), fnp[s])


def test_tracker_chains_in_the_reference_order(ctx):
    """tests/golden/tracker_chain_seq.json and tracker_replay_seq_1000.json (the sequential oracle's digests, tests/golden/make_tracker_chain_seq.py): the
    device with "sum_order" 1 reproduces both field for field, every step's aligner call on the latency kernel"""
    import tracker_chain
    from conftest import golden_path
    for name, kw in (("tracker_chain_seq.json", {}), ("tracker_replay_seq_1000.json", dict(record_every=50, map_capacity=60000))):
        g = json.load(open(golden_path(name)))
        c = api.Context(0, kernel_timing=False)
        try:
            c.set_option("sum_order", 1)
            got = tracker_chain.run_device(api, c, g.get("steps_total", len(g["steps"])), **kw)
            assert c.get_option("last_align_path") == 3
        finally:
            c.close()
        assert [r["step"] for r in got] == [r["step"] for r in g["steps"]], name
        for a, b in zip(got, g["steps"]):
            assert a == b, (name, a["step"], {k: (a[k], b[k]) for k in b if a[k] != b[k]})


def test_tree_order_two_slices_on_path_3_unchanged(ctx, po):
    """"sum_order" 0 on align_path 3 (k_align_pair<false>): still the device-order oracle's bits"""
    sensors = [(0.2, 0.1, 0.1), (-0.3, 0.0, math.pi)]
    sc = Scene(71, 900, (721, 721), sensors)
    mv = api.CloudSet(ctx, sc.map)
    fnp = [sc.fixed_np(0), sc.fixed_np(1)]
    al = _aligner(ctx, (721, 721), sensors, (True, False), its=10)
    pri = [(sc.x0[0].copy(), np.diag([100.0, 100.0, 100.0]).astype(np.float32))]
    ctx.set_option("align_path", 3)
    try:
        res = al.compute_batch([api.CloudSet(ctx, f) for f in fnp], [mv, mv], sc.x0, priors=pri, want_stats=True)
        assert ctx.get_option("last_align_path") == 3
    finally:
        ctx.set_option("align_path", 0)
    oslices = [_oslice(po, sl) for sl in al.param_slice_processors]
    rt = po.align(po.aligner_params(10, min_num_inliers=10, prior_z=pri[0][0], prior_omega=pri[0][1], device_order=True), oslices, fnp, [sc.map] * 2, sc.x0[0])
    _assert_bitwise(res, 0, rt, "tree order, path 3")


def test_adapter_hip_context_follows_its_sum_order_param(tmp_path):
    """adapters/srrg HipContext: a change of its sum_order PARAM after the first handle() reaches the context (lsm2d_get_option), both ways; a failed
    apply throws and leaves no context behind (tests/cpp/adapter_sum_order_driver.cpp)"""
    from conftest import ROOT
    exe = cpp_build.build("adapter_sum_order_driver.cpp", tmp_path, flags=("-O1", "-Wall"), link_flags=("-ldl",),
                          include_dirs=(os.path.join(ROOT, "adapters", "srrg"), os.path.join(cpp_build.CPP, "adapter_shim")))
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    r = json.loads(out.strip().splitlines()[-1])
    assert r == {"first": 0, "after_on": 1, "after_off": 0, "same_context": 1, "threw": 1, "after_failure": 1}, r
