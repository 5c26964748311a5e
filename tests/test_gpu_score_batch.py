"""GPU tests of lsm2d_score_batch (k_find_*_batch, then k_score_partial_batch / k_score_final_batch / k_score_seq_batch on the pairs where they lie).  Per
item the call must return exactly what lsm2d_find_correspondences_batch followed by lsm2d_linearize_batch returns -- H, b, the counts, the chi^2 sums and
the pair digest -- in both orders of summation, so every batch here is compared with that two-call sequence, with single find + linearize calls AND with the
CPU oracle (po.find, then po.linearize_device_order for "sum_order" 0, the sequential po.linearize for "sum_order" 1).  No tolerance appears in this file."""
import ctypes as C
import math

import numpy as np
import pytest

from srrg2_laser_slam_2d_amd import api, synth
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT, IterationStats

pytestmark = pytest.mark.gpu

PAIR_BUDGET = 1 << 21      # pair slots per launch group (kBatchPairBudget, lsm2d_capi_finder.inc)
TAU = 0.01
MD = 0.3
# where an item's lin_blocks(count) = clamp(ceil(count / 256), 1, 1024) steps, where a trip of kAlignBlock = 512 and a half-trip of kSeqHalf = 256 end; the
# slot is the largest (1025, no multiple of 256: five virtual blocks per item, most of which exit)
EDGE_COUNTS = [0, 1, 255, 256, 257, 511, 512, 513, 1025]
EDGE_POSE = np.float32([0.001, -0.0007, 0.0005])
N_BIG = 270000             # more pairs than 1024 workgroups x 256 threads take in one trip (262 144)


class _Fx:
    pass


def _multi(ctx, clouds):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    return api.CloudSet(ctx, np.ascontiguousarray(np.concatenate(clouds), np.float32), offs if len(clouds) > 1 else None)


@pytest.fixture(scope="module")
def fx(ctx, po):
    f = _Fx()
    wl = synth.make_workload(3, 3000, seed=5, map_noise=0.004, scan_noise=0.004)
    f.wl = wl
    f.scans = [wl.scan_points[wl.scan_offsets[i]:wl.scan_offsets[i + 1]] for i in range(3)]
    f.map = wl.map_points
    f.x0 = np.ascontiguousarray(wl.x0, np.float32)
    f.scan_set = api.CloudSet(ctx, wl.scan_points, wl.scan_offsets)
    f.map_set = api.CloudSet(ctx, f.map)
    f.prefixes = [np.ascontiguousarray(f.map[:c]) for c in EDGE_COUNTS]
    f.prefix_set = _multi(ctx, f.prefixes)
    return f


@pytest.fixture()
def order_ctx(ctx, request):
    ctx.set_option("sum_order", request.param)
    try:
        yield ctx
    finally:
        ctx.set_option("sum_order", 0)


def _finder(ctx, kind, cols=1081):
    if kind == "proj":
        return api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, 30.0))
    if kind == "nn":
        return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=MD, search="exact")
    if kind == "kd":
        return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=MD, search="kdtree")
    return api.CorrespondenceFinderNN2D(ctx, max_distance_m=MD)


def _osp(po, kind, robust, cols=1081):
    if kind == "proj":
        return po.slice_params(canvas_cols=cols, robustifier=robust, chi_threshold=TAU)
    fk = dict(nn=po.FINDER_NN, kd=po.FINDER_KDTREE_APPROX, dm=po.FINDER_DISTMAP)[kind]
    return po.slice_params(finder=fk, max_distance=MD, robustifier=robust, chi_threshold=TAU)


def _key(H, b, st):
    """everything an item returns, as bytes and integers: equality of keys is bitwise equality"""
    return (np.asarray(H, np.float32).tobytes(), np.asarray(b, np.float32).tobytes(), int(st.n_correspondences), int(st.n_inliers), int(st.n_outliers),
            np.float32(st.chi_inliers).tobytes(), np.float32(st.chi_outliers).tobytes(), int(st.pair_digest))


def _okey(H, b, ost):
    return (np.asarray(H, np.float32).tobytes(), np.asarray(b, np.float32).tobytes(), int(ost.n_corr), int(ost.n_in), int(ost.n_out),
            np.float32(ost.chi_in).tobytes(), np.float32(ost.chi_out).tobytes(), int(ost.pair_digest))


def _batch_keys(res):
    H, b, st = res
    assert H.shape == (len(st), 3, 3) and b.shape == (len(st), 3)
    return [_key(H[i], b[i], st[i]) for i in range(len(st))]


def _three_ways(ctx, po, finder, sp, osp, fixed, fclouds, fixed_index, moving, mclouds, moving_index, poses, oracle_items=None, single_items=None, tag=""):
    """score_batch against (a) find_correspondences_batch -> linearize_batch, (b) single find + linearize calls, (c) the oracle; returns the batch's result,
    its keys and the oracle's pair vectors (None where the oracle was not asked)"""
    n = len(poses)
    order = ctx.get_option("sum_order")
    fi = (np.arange(n) if len(fclouds) > 1 else np.zeros(n, int)) if fixed_index is None else np.asarray(fixed_index)
    mi = (np.arange(n) if len(mclouds) > 1 else np.zeros(n, int)) if moving_index is None else np.asarray(moving_index)
    res = api.score_batch(ctx, sp, fixed, moving, poses, fixed_index=fixed_index, moving_index=moving_index)
    got = _batch_keys(res)
    vecs = finder.compute_batch(fixed, moving, poses, fixed_index=fixed_index, moving_index=moving_index)
    two = _batch_keys(api.linearize_batch(ctx, sp, fixed, moving, vecs, poses, fixed_index=fixed_index, moving_index=moving_index))
    for k in range(n):
        assert got[k] == two[k], (tag, "score_batch vs find_batch -> linearize_batch", order, k, len(vecs[k]))
    for k in (range(n) if single_items is None else single_items):
        finder.setFixed(fixed, int(fi[k])); finder.setMoving(moving, int(mi[k])); finder.setLocalMapInSensor(poses[k])
        v = finder.compute().copy()
        one = _key(*api.linearize(ctx, sp, fixed, moving, v, poses[k], fixed_index=int(fi[k]), moving_index=int(mi[k])))
        assert got[k] == one, (tag, "score_batch vs single calls", order, k, len(v))
    oracle = po.linearize if order else po.linearize_device_order
    ovecs = [None] * n
    for k in (range(n) if oracle_items is None else oracle_items):
        fcl, mcl = fclouds[int(fi[k])], mclouds[int(mi[k])]
        ovecs[k] = po.find(osp, fcl, mcl, poses[k])
        assert res[2][k].n_correspondences == len(ovecs[k]), (tag, "pair count vs po.find", k)
        assert got[k] == _okey(*oracle(osp, fcl, mcl, ovecs[k], poses[k])), (tag, "score_batch vs oracle", order, k, len(ovecs[k]))
    return res, got, ovecs


def _with_robust(sp, robust):
    sp.robustifier = robust; sp.chi_threshold = TAU
    return sp


# ---- 1. shape edges of the factor's launch form, point-query finders -----------------------------------------------------------------------------------
@pytest.mark.parametrize("robust", [api.ROBUST_NONE, api.ROBUST_CAUCHY], ids=["plain", "cauchy"])
@pytest.mark.parametrize("kind", ["nn", "kd", "dm"])
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_shape_edges_point_query(order_ctx, po, fx, kind, robust):
    ctx = order_ctx
    order = ctx.get_option("sum_order")
    finder = _finder(ctx, kind)
    sp, osp = _with_robust(finder.slice_params(), robust), _osp(po, kind, robust)
    n = len(EDGE_COUNTS)
    poses = np.tile(EDGE_POSE, (n, 1))
    (H, b, st), got, ovecs = _three_ways(ctx, po, finder, sp, osp, fx.map_set, [fx.map], None, fx.prefix_set, fx.prefixes, None, poses, tag=(kind, robust))
    for k, c in enumerate(EDGE_COUNTS):
        assert len(ovecs[k]) == c and st[k].n_correspondences == c, (kind, k, c)      # po.find itself: every query finds its pair
        assert st[k].pair_digest == po.pair_digest(ovecs[k])
    assert np.all(H[0] == 0) and np.all(b[0] == 0) and st[0].n_correspondences == 0 and st[0].chi_inliers == 0 and st[0].chi_outliers == 0
    assert np.any(b[-1] != 0) and st[-1].chi_inliers + st[-1].chi_outliers > 0
    # the other order gives other bits for every count >= 255: a kernel summing in the wrong order cannot have passed
    other = po.linearize_device_order if order else po.linearize
    for k, c in enumerate(EDGE_COUNTS):
        if c >= 255:
            assert got[k][:2] != _okey(*other(osp, fx.map, fx.prefixes[k], ovecs[k], poses[k]))[:2], (order, kind, robust, k)


# ---- 2. past the 1024-block clamp, over several launch groups -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(ctx, po, fx):
    f = _Fx()
    f.cloud = synth.make_map(fx.wl.world, N_BIG, seed=7)
    f.set = api.CloudSet(ctx, f.cloud)
    # the large item between two small ones (ragged block bases), then six more small ones: a launch group takes PAIR_BUDGET // N_BIG = 7 items, so the nine
    # items are two launch groups queued behind each other with one wait
    f.mclouds = [np.ascontiguousarray(f.cloud[:300]), f.cloud, np.ascontiguousarray(f.cloud[1000:1700])] + \
                [np.ascontiguousarray(f.cloud[5000 * j: 5000 * j + 257 + 100 * j]) for j in range(1, 7)]
    f.mset = _multi(ctx, f.mclouds)
    f.poses = np.tile(EDGE_POSE, (len(f.mclouds), 1))
    f.poses[1] = 0.0      # the large item: identity pose, moving = fixed
    f.osp_find = po.slice_params(finder=po.FINDER_NN, max_distance=MD)
    f.ovecs = [po.find(f.osp_find, f.cloud, m, f.poses[k]) for k, m in enumerate(f.mclouds)]      # once, for both orders
    assert len(f.ovecs[1]) > 262144
    assert len(f.mclouds) > PAIR_BUDGET // N_BIG and len(f.mclouds) * N_BIG > PAIR_BUDGET
    return f


@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_past_the_block_clamp_over_two_launch_groups(order_ctx, po, big):
    ctx = order_ctx
    order = ctx.get_option("sum_order")
    finder = _finder(ctx, "nn")
    sp, osp = _with_robust(finder.slice_params(), api.ROBUST_CAUCHY), _osp(po, "nn", po.ROBUST_CAUCHY)
    n = len(big.mclouds)
    H, b, st = api.score_batch(ctx, sp, big.set, big.mset, big.poses)
    got = _batch_keys((H, b, st))
    assert [s.n_correspondences for s in st] == [len(v) for v in big.ovecs]
    vecs = finder.compute_batch(big.set, big.mset, big.poses)
    assert got == _batch_keys(api.linearize_batch(ctx, sp, big.set, big.mset, vecs, big.poses))
    oracle = po.linearize if order else po.linearize_device_order
    for k in range(n):
        assert np.array_equal(vecs[k], big.ovecs[k]), k
        finder.setFixed(big.set, 0); finder.setMoving(big.mset, k); finder.setLocalMapInSensor(big.poses[k])
        v = finder.compute().copy()
        assert got[k] == _key(*api.linearize(ctx, sp, big.set, big.mset, v, big.poses[k], fixed_index=0, moving_index=k)), ("single calls", order, k)
        assert got[k] == _okey(*oracle(osp, big.cloud, big.mclouds[k], big.ovecs[k], big.poses[k])), ("oracle", order, k)
    assert np.any(H[1] != 0) and np.any(b[0] != 0) and np.any(b[n - 1] != 0)      # items of both launch groups did their work


# ---- 3. projective finder ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [1081, 257])
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_projective(order_ctx, po, fx, cols):
    ctx = order_ctx
    finder = _finder(ctx, "proj", cols)
    sp, osp = _with_robust(finder.slice_params(), api.ROBUST_CAUCHY), _osp(po, "proj", po.ROBUST_CAUCHY, cols)
    fi = np.int32([0, 1, 2, 2, 0, 1, 1])
    poses = np.concatenate([fx.x0, fx.x0[[2, 0, 1]], np.float32([[1000.0, 1000.0, 0.3]])]).astype(np.float32)
    poses[3:6] += np.float32([[0.02, -0.01, 0.005], [-0.01, 0.02, -0.004], [0.015, 0.01, 0.003]])
    (H, b, st), got, ovecs = _three_ways(ctx, po, finder, sp, osp, fx.scan_set, fx.scans, fi, fx.map_set, [fx.map], None, poses, tag=cols)
    assert min(len(v) for v in ovecs[:6]) > 50 and len(ovecs[6]) == 0
    assert got[2] != got[3] and got[0] != got[4]
    assert np.all(H[6] == 0) and np.all(b[6] == 0) and bytes(st[6]) == bytes(IterationStats())      # the item that finds no pair: exact zeros
    assert any(s.n_inliers > 0 and s.n_outliers > 0 for s in st)
    # the scans in their own order through NULL indices
    _three_ways(ctx, po, finder, sp, osp, fx.scan_set, fx.scans, None, fx.map_set, [fx.map], None, fx.x0, tag=(cols, "NULL indices"))


# ---- 4. set states and index rules ---------------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Out:
    def __init__(self, n):
        self.H = np.full((max(n, 1), 9), -7.0, np.float32); self.b = np.full((max(n, 1), 3), -7.0, np.float32)
        self.st = (IterationStats * max(n, 1))()
        C.memset(self.st, 0x5A, C.sizeof(self.st))

    def untouched(self):
        return bool(np.all(self.H == -7.0) and np.all(self.b == -7.0) and bytes(self.st) == b"\x5a" * C.sizeof(self.st))

    def keys(self, n):
        return [_key(self.H[i].reshape(3, 3), self.b[i], self.st[i]) for i in range(n)]


def _raw(ctx, sp, fixed, fi, moving, mi, poses, n=None, stats=True):
    poses = None if poses is None else np.ascontiguousarray(poses, np.float32)
    n = len(poses) if n is None else n
    out = _Out(n)
    rc = ctx._lib.lsm2d_score_batch(ctx.handle, C.byref(sp), fixed.handle, _ptr(fi), moving.handle, _ptr(mi), n, _ptr(poses), _ptr(out.H), _ptr(out.b),
                                    out.st if stats else None)
    return rc, out


def _raw_two_calls(ctx, sp, fixed, fi, moving, mi, poses, cap):
    """lsm2d_find_correspondences_batch, then lsm2d_linearize_batch on what it wrote, untouched"""
    poses = np.ascontiguousarray(poses, np.float32)
    n = len(poses)
    pairs = np.full((n, cap, 2), -7, np.int32); cnt = np.full(n, -7, np.int32)
    rc = ctx._lib.lsm2d_find_correspondences_batch(ctx.handle, C.byref(sp), fixed.handle, _ptr(fi), moving.handle, _ptr(mi), n, _ptr(poses), _ptr(pairs), cap, _ptr(cnt))
    assert rc == 0
    out = _Out(n)
    rc = ctx._lib.lsm2d_linearize_batch(ctx.handle, C.byref(sp), fixed.handle, _ptr(fi), moving.handle, _ptr(mi), n, _ptr(pairs), cap, _ptr(cnt), _ptr(poses),
                                        _ptr(out.H), _ptr(out.b), out.st)
    assert rc == 0
    return out, [pairs[i, : cnt[i]].copy() for i in range(n)]


def test_set_states_and_index_rules(ctx, po, fx):
    cols, beams = 721, 721
    pr = api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, 30.0)
    finder = api.CorrespondenceFinderProjective2f(ctx, pr)
    sp = _with_robust(finder.slice_params(), api.ROBUST_CAUCHY)
    osp = po.slice_params(canvas_cols=cols, robustifier=po.ROBUST_CAUCHY, chi_threshold=TAU)
    # a fixed set whose sizes only the device knows: lsm2d_preprocess_scans, then lsm2d_preprocess_scans_refill with fresh ranges
    sensors = synth.sample_poses(fx.wl.world, 3, seed=21)
    first = synth.make_scan_ranges(fx.wl.world, synth.sample_poses(fx.wl.world, 3, seed=22), n_beams=beams, angle_min=-2.0, angle_max=2.0, noise_sigma=0.004, seed=8)
    fresh = np.ascontiguousarray(synth.make_scan_ranges(fx.wl.world, sensors, n_beams=beams, angle_min=-2.0, angle_max=2.0, noise_sigma=0.004, seed=9), np.float32)
    pre = api.RawDataPreprocessorProjective2D(ctx, range_min=0.3, range_max=30.0, voxelize_resolution=0.02, normal_point_distance=0.3, normal_min_points=5)
    pre.setRawData(first, -2.0, 2.0, 0.0, 40.0)
    scans = pre.compute()
    pre.setRawData(fresh, -2.0, 2.0, 0.0, 40.0)
    pre.refill(scans)
    scans._set_pending()      # (the Python object's sizes are the first batch's: whoever reads them asks the library)
    # a moving set written by an asynchronous lsm2d_clip_scene
    clipper = api.SceneClipperProjective2D(ctx, pr, asynchronous=True, voxelize_resolution=0.0)
    clipper.setFullScene(fx.map_set); clipper.setRobotInLocalMap(sensors[0].astype(np.float32))
    clipped = clipper.compute()
    # clipped is in the robot frame of sensors[0]: scan i sees it under inverse(sensors[i]) * sensors[0], a little off
    rel = synth.compose_poses(synth.invert_poses(sensors), np.tile(sensors[[0]], (3, 1)))
    poses = synth.compose_poses(rel, np.array([[0.03, -0.02, 0.01]] * 3)).astype(np.float32)
    # NULL fixed index over a set of n_items clouds, NULL moving index over a one-cloud set -- before anybody has resolved a size
    rc, out = _raw(ctx, sp, scans, None, clipped, None, poses)
    assert rc == 0
    got = out.keys(3)
    two, vecs = _raw_two_calls(ctx, sp, scans, None, clipped, None, poses, cols)
    assert got == two.keys(3)
    fclouds = [scans.download(i) for i in range(3)]
    mcloud = clipped.download(0)
    pp = po.Preprocessor(beams, -2.0, 2.0, 0.3, 30.0, 0.3, 5, 0.02)
    for i in range(3):
        assert np.array_equal(fclouds[i], po.preprocess_scan(pp, fresh[i])), i
        v = po.find(osp, fclouds[i], mcloud, poses[i])
        assert np.array_equal(vecs[i], v), i
        assert got[i] == _okey(*po.linearize_device_order(osp, fclouds[i], mcloud, v, poses[i])), i
    assert len(vecs[0]) > 100
    # NULL fixed index over a one-cloud set with an index array on the other side (the roles swapped), repeats included
    inv = synth.invert_poses(poses.astype(np.float64)).astype(np.float32)
    mi = np.int32([2, 0, 0, 1])
    rc, out = _raw(ctx, sp, clipped, None, scans, mi, inv[mi])
    assert rc == 0
    two, vecs = _raw_two_calls(ctx, sp, clipped, None, scans, mi, inv[mi], cols)
    assert out.keys(4) == two.keys(4) and out.keys(4)[1] == out.keys(4)[2]
    for k in range(4):
        v = po.find(osp, mcloud, fclouds[mi[k]], inv[mi[k]])
        assert out.keys(4)[k] == _okey(*po.linearize_device_order(osp, mcloud, fclouds[mi[k]], v, inv[mi[k]])), k
    # a NULL index over a set of neither 1 nor n_items clouds
    rc, out = _raw(ctx, sp, scans, None, clipped, None, poses[:2])
    assert rc == BAD_ARGUMENT and out.untouched()


# ---- 5. argument checks through raw calls ----------------------------------------------------------------------------------------------------------------------
def _aligner(ctx):
    al = api.MultiAligner2D(ctx, max_iterations=8, min_num_inliers=10)
    finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0))
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, min_num_correspondences=10))
    return al


def test_argument_checks(ctx, po, fx):
    lib = ctx._lib
    sp = _with_robust(_finder(ctx, "proj").slice_params(), api.ROBUST_CAUCHY)
    rc, ok = _raw(ctx, sp, fx.scan_set, None, fx.map_set, None, fx.x0)
    assert rc == 0
    want = ok.keys(3)
    osp = _osp(po, "proj", po.ROBUST_CAUCHY)
    assert want == [_okey(*po.linearize_device_order(osp, fx.scans[i], fx.map, po.find(osp, fx.scans[i], fx.map, fx.x0[i]), fx.x0[i])) for i in range(3)]
    # n_items 0: a successful no-op that writes nothing, whatever the item arrays are
    rc, out = _raw(ctx, sp, fx.scan_set, None, fx.map_set, None, None, n=0)
    assert rc == 0 and out.untouched()
    H, b, st = api.score_batch(ctx, sp, fx.scan_set, fx.map_set, np.zeros((0, 3), np.float32))
    assert H.shape == (0, 3, 3) and b.shape == (0, 3) and st == []
    # a cloud index out of range in item k: the text names k, nothing is written
    for fi, k in ((np.int32([0, 1, 3]), 2), (np.int32([0, -1, 2]), 1)):
        rc, out = _raw(ctx, sp, fx.scan_set, fi, fx.map_set, None, fx.x0)
        assert rc == BAD_ARGUMENT and out.untouched()
        assert "item %d" % k in lib.lsm2d_last_error(ctx.handle).decode()
    rc, out = _raw(ctx, sp, fx.scan_set, None, fx.map_set, np.int32([0, 0, 1]), fx.x0)
    assert rc == BAD_ARGUMENT and out.untouched() and "item 2" in lib.lsm2d_last_error(ctx.handle).decode()
    # out_stats NULL
    rc, out = _raw(ctx, sp, fx.scan_set, None, fx.map_set, None, fx.x0, stats=False)
    assert rc == 0 and np.array_equal(out.H.view(np.uint32), ok.H.view(np.uint32)) and np.array_equal(out.b.view(np.uint32), ok.b.view(np.uint32))
    assert bytes(out.st) == b"\x5a" * C.sizeof(out.st)
    # a set from another context
    other = api.Context(0)
    try:
        foreign = api.CloudSet(other, fx.map)
        rc, out = _raw(ctx, sp, fx.scan_set, None, foreign, None, fx.x0)
        assert rc == BAD_ARGUMENT and out.untouched()
        rc, out = _raw(ctx, sp, foreign, np.zeros(3, np.int32), fx.map_set, None, fx.x0)
        assert rc == BAD_ARGUMENT and out.untouched()
        del foreign
    finally:
        other.close()
    # one batch begun: the call works and gives the same bits, and so does the batch
    al = _aligner(ctx)
    want_al = al.compute_batch([fx.scan_set], [fx.map_set], fx.x0)
    prep = al.prepare_batch([fx.scan_set], [fx.map_set], fx.x0)
    prep.begin()
    rc, out = _raw(ctx, sp, fx.scan_set, None, fx.map_set, None, fx.x0)
    res = prep.wait(copy=True)
    assert rc == 0 and out.keys(3) == want
    assert np.array_equal(res.pose.view(np.uint32), want_al.pose.view(np.uint32)) and np.array_equal(res.status, want_al.status)
    # two begun: refused like every call that moves data, nothing written; both are still waited for cleanly and the call works again
    a, b = al.prepare_batch([fx.scan_set], [fx.map_set], fx.x0), al.prepare_batch([fx.scan_set], [fx.map_set], fx.x0[::-1].copy(), fixed_index=np.int32([[2, 1, 0]]))
    a.begin(); b.begin()
    try:
        rc, out = _raw(ctx, sp, fx.scan_set, None, fx.map_set, None, fx.x0)
        assert rc == BAD_ARGUMENT and out.untouched()
    finally:
        ra, rb = a.wait(copy=True), b.wait(copy=True)
    assert np.array_equal(ra.pose.view(np.uint32), want_al.pose.view(np.uint32)) and np.array_equal(ra.pose.view(np.uint32), rb.pose[::-1].view(np.uint32))
    rc, out = _raw(ctx, sp, fx.scan_set, None, fx.map_set, None, fx.x0)
    assert rc == 0 and out.keys(3) == want


# ---- 6. the lane's scratch is the caller's again afterwards -----------------------------------------------------------------------------------------------------
def test_align_batch_after_score_batch_keeps_its_bits(ctx, fx):
    al = _aligner(ctx)
    before = al.compute_batch([fx.scan_set], [fx.map_set], fx.x0, want_stats=True)
    sp = _with_robust(_finder(ctx, "nn").slice_params(), api.ROBUST_CAUCHY)
    inv = synth.invert_poses(fx.x0.astype(np.float64)).astype(np.float32)
    H, b, st = api.score_batch(ctx, sp, fx.map_set, fx.scan_set, inv)      # writes items, counts, pairs, rows into the lane's scratch
    assert min(s.n_correspondences for s in st) > 100
    after = al.compute_batch([fx.scan_set], [fx.map_set], fx.x0, want_stats=True)      # the same inputs again: the aligner may not trust what lay there
    for k in ("pose", "information", "status", "iterations"):
        x, y = getattr(before, k), getattr(after, k)
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), k
    assert np.array_equal(api.pair_digests(before.stats), api.pair_digests(after.stats))
    assert np.all(before.status == 0)
