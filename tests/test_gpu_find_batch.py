"""GPU tests of lsm2d_find_correspondences_batch (k_find_projective_batch / k_find_nn_batch) and of lsm2d_align_batch_pairs through it.  Per item the
batched call must return exactly what lsm2d_find_correspondences returns -- the same pairs in the same order -- and that call is held bit for bit to the
CPU oracle, so every batch here is compared with single calls AND with po.find.  No tolerance appears in this file."""
import ctypes as C
import math

import numpy as np
import pytest

import mixed_batches as mb
from srrg2_laser_slam_2d_amd import api, synth
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT, CAPACITY_EXCEEDED

pytestmark = pytest.mark.gpu

RMAX = 25.0
MD, RES, NCOS = 0.4, 0.1, 0.7
PAIR_BUDGET = 1 << 21      # pairs per launch (kBatchPairBudget, lsm2d_capi_finder.inc)


class _Fx:
    pass


@pytest.fixture(scope="module")
def fx(ctx):
    f = _Fx()
    world = synth.make_world(4)
    f.world = world
    f.m = synth.make_map(world, 6000, seed=2)
    f.small = np.ascontiguousarray(f.m[::6])
    f.big = synth.make_map(world, 40000, seed=3)
    f.robots = synth.sample_poses(world, 6, seed=8)
    pts, offs = synth.make_scans(world, f.robots, n_beams=1081, noise_sigma=0.01, seed=5)
    f.scans = [pts[offs[i]:offs[i + 1]] for i in range(6)]
    assert [len(s) for s in f.scans] == [1081, 970, 1006, 973, 1011, 1081]
    x0 = synth.invert_poses(synth.compose_poses(f.robots, np.array([[0.12, -0.08, 0.04]] * 6))).astype(np.float32)
    x0[5] = np.float32([500.0, 500.0, 1.0])      # forms no pair
    f.x0 = x0
    f.inv = synth.invert_poses(x0.astype(np.float64)).astype(np.float32)      # role B: the scan moves, the map is fixed
    f.scan_set = api.CloudSet(ctx, pts, offs)
    f.m_set = api.CloudSet(ctx, f.m)
    f.small_set = api.CloudSet(ctx, f.small)
    f.three = _multi(ctx, [f.m, f.small, f.big])
    f.three_clouds = [f.m, f.small, f.big]
    return f


def _multi(ctx, clouds):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    pts = np.concatenate(clouds) if offs[-1] else np.zeros((0, 4), np.float32)
    return api.CloudSet(ctx, np.ascontiguousarray(pts, np.float32), offs if len(clouds) > 1 else None)


def _proj(cols):
    return api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, RMAX)


def _finder(ctx, kind, cols=1081):
    if kind == "proj":
        return api.CorrespondenceFinderProjective2f(ctx, _proj(cols))
    if kind == "nn":
        return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=MD, normal_cos=NCOS, search="exact")
    if kind == "kd":
        return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=MD, normal_cos=NCOS, search="kdtree")
    return api.CorrespondenceFinderNN2D(ctx, max_distance_m=MD, resolution=RES, normal_cos=NCOS)


def _osp(po, kind, cols=1081):
    if kind == "proj":
        return po.slice_params(canvas_cols=cols, range_max=RMAX)
    fk = dict(nn=po.FINDER_NN, kd=po.FINDER_KDTREE_APPROX, dm=po.FINDER_DISTMAP)[kind]
    return po.slice_params(finder=fk, max_distance=MD, resolution=RES, normal_cos=NCOS)


def _singles(f, fixed, fi, moving, mi, poses):
    out = []
    for k in range(len(poses)):
        f.setFixed(fixed, int(fi[k])); f.setMoving(moving, int(mi[k])); f.setLocalMapInSensor(poses[k])
        out.append(f.compute().copy())
    return out


def _run_and_compare(po, osp, f, fixed, fclouds, fixed_index, moving, mclouds, moving_index, poses, oracle_items=None, tag=""):
    n = len(poses)
    fi = (np.arange(n) if len(fclouds) > 1 else np.zeros(n, int)) if fixed_index is None else np.asarray(fixed_index)
    mi = (np.arange(n) if len(mclouds) > 1 else np.zeros(n, int)) if moving_index is None else np.asarray(moving_index)
    got = f.compute_batch(fixed, moving, poses, fixed_index=fixed_index, moving_index=moving_index)
    assert len(got) == n
    one = _singles(f, fixed, fi, moving, mi, poses)
    for k in range(n):
        assert np.array_equal(got[k], one[k]), (tag, "batch vs single call", k, len(got[k]), len(one[k]))
    for k in (range(n) if oracle_items is None else oracle_items):
        want = po.find(osp, fclouds[int(fi[k])], mclouds[int(mi[k])], poses[k])
        assert np.array_equal(got[k], want), (tag, "batch vs oracle", k, len(got[k]), len(want))
    return got


# ---- 1. the projective finder: less than one trip of 1024 columns, two trips, three trips with one column in the last ------------------------------------
ORACLE_COUNTS = {1081: [404, 516, 404, 430, 466, 0], 2049: [327, 535, 446, 491, 413, 0]}


@pytest.mark.parametrize("cols", [64, 721, 1081, 2049])
def test_projective_batch_equals_single_calls_and_oracle(ctx, po, fx, cols):
    got = _run_and_compare(po, _osp(po, "proj", cols), _finder(ctx, "proj", cols), fx.scan_set, fx.scans, None, fx.m_set, [fx.m], None, fx.x0, tag=cols)
    assert len(got[5]) == 0
    if cols in ORACLE_COUNTS:
        assert [len(g) for g in got] == ORACLE_COUNTS[cols]


# ---- 2. index forms --------------------------------------------------------------------------------------------------------------------------------------
def test_index_forms(ctx, po, fx):
    f, osp = _finder(ctx, "proj"), _osp(po, "proj")
    # NULL indices, `moving` one shared cloud: the first test.  A permuted fixed_index with scan 2 used twice under different poses
    fi = np.int32([3, 2, 0, 2, 4, 1, 5])
    poses = np.concatenate([fx.x0[fi[:3]], fx.x0[[1]], fx.x0[fi[4:]]]).astype(np.float32)      # item 3: scan 2 under scan 1's pose
    got = _run_and_compare(po, osp, f, fx.scan_set, fx.scans, fi, fx.m_set, [fx.m], None, poses, tag="permuted fixed_index")
    assert not np.array_equal(got[1], got[3])
    # `moving` the three-cloud set {m, small, big} through moving_index: the 40 000-point cloud is z-buffered inside the item's workgroup
    mi = np.int32([2, 0, 1, 2, 1, 0])
    got = _run_and_compare(po, osp, f, fx.scan_set, fx.scans, None, fx.three, fx.three_clouds, mi, fx.x0, tag="moving_index")
    assert len(got[0]) == 572
    # ... and as the FIXED side, with both index arrays
    _run_and_compare(po, osp, f, fx.three, fx.three_clouds, np.int32([2, 1, 0, 2]), fx.scan_set, fx.scans, np.int32([0, 1, 1, 3]), fx.inv[[0, 1, 1, 3]], tag="big fixed cloud")
    # NULL moving index over a set of n_items clouds
    six = _multi(ctx, [fx.m, fx.small, fx.m[::2], fx.big[::3], fx.small[::2], fx.m])
    _run_and_compare(po, osp, f, fx.scan_set, fx.scans, None, six, [fx.m, fx.small, fx.m[::2], fx.big[::3], fx.small[::2], fx.m], None, fx.x0, tag="n_items moving clouds")


# ---- 3. the point-query finders, both roles ----------------------------------------------------------------------------------------------------------------
ROLE_A_COUNTS = dict(nn=[176, 200, 268, 229, 144, 0], kd=[175, 199, 260, 217, 143, 0])


@pytest.mark.parametrize("kind", ["nn", "kd", "dm"])
def test_point_query_batch_both_roles(ctx, po, fx, kind):
    f, osp = _finder(ctx, kind), _osp(po, kind)
    got = _run_and_compare(po, osp, f, fx.scan_set, fx.scans, None, fx.small_set, [fx.small], None, fx.x0, tag=(kind, "role A"))
    if kind in ROLE_A_COUNTS:
        assert [len(g) for g in got] == ROLE_A_COUNTS[kind]
    assert len(got[5]) == 0
    _run_and_compare(po, osp, f, fx.m_set, [fx.m], None, fx.scan_set, fx.scans, None, fx.inv, tag=(kind, "role B"))
    # one batch, both search forms: items against m (6000 >= 4 x 1081) search cooperatively, items against small (1000) do not
    two = _multi(ctx, [fx.m, fx.small])
    _run_and_compare(po, osp, f, two, [fx.m, fx.small], np.int32([0, 1, 1, 0, 0, 1]), fx.scan_set, fx.scans, None, fx.inv, tag=(kind, "mixed group widths"))
    # moving clouds at the trip boundaries of both group widths (1024 and 256 queries per trip); from three trips on (2049, 3073 with one lane per query) the
    # single call spreads the queries over many workgroups (k_find_nn_multi): all three kernels that share the match, against each other and the oracle
    sizes = [0, 1, 255, 256, 257, 1023, 1024, 1025, 2049, 3073]
    prefixes = [np.ascontiguousarray(fx.m[:k]) for k in sizes]
    pset = _multi(ctx, prefixes)
    poses = np.tile(fx.x0[0], (len(sizes), 1))
    _run_and_compare(po, osp, f, fx.scan_set, fx.scans, np.zeros(len(sizes), np.int32), pset, prefixes, None, poses, tag=(kind, "prefixes, one lane per query"))
    big_fixed = _multi(ctx, [fx.big, fx.m])      # 40000 >= 4 x 1025: kNNGroup lanes per query
    poses_b = np.tile(fx.inv[0], (len(sizes), 1))
    _run_and_compare(po, osp, f, big_fixed, [fx.big, fx.m], np.zeros(len(sizes), np.int32), pset, prefixes, None, poses_b, tag=(kind, "prefixes, cooperative"))


# ---- 4. item counts: 600 workgroups of 1024 threads are more than one dispatch round on 256 CUs -----------------------------------------------------------
def _perturbed(fx, n, seed):
    rng = np.random.default_rng(seed)
    which = np.arange(n) % 6
    d = rng.uniform(-1.0, 1.0, (n, 3)) * np.array([0.05, 0.05, 0.02])
    poses = synth.invert_poses(synth.compose_poses(synth.compose_poses(fx.robots[which], np.array([[0.12, -0.08, 0.04]] * n)), d)).astype(np.float32)
    poses[which == 5] = np.float32([500.0, 500.0, 1.0])
    return which.astype(np.int32), poses


@pytest.mark.parametrize("n", [1, 2, 600])
def test_item_counts(ctx, po, fx, n):
    which, poses = _perturbed(fx, n, 17)
    got = _run_and_compare(po, _osp(po, "proj"), _finder(ctx, "proj"), fx.scan_set, fx.scans, which, fx.m_set, [fx.m], None, poses, tag=n)
    if n == 600:
        assert len({g.tobytes() for g in got}) > 400      # the perturbations matter: the items are not copies of six


# ---- raw calls (capacities and pointers chosen by the test) ---------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(ctx, sp, fixed, fi, moving, mi, poses, cap, n=None, out=None, cnt=None):
    poses = None if poses is None else np.ascontiguousarray(poses, np.float32)
    n = len(poses) if n is None else n
    out = np.full((max(n, 1), max(cap, 1), 2), -7, np.int32) if out is None else out
    cnt = np.full(max(n, 1), -7, np.int32) if cnt is None else cnt
    rc = ctx._lib.lsm2d_find_correspondences_batch(ctx.handle, C.byref(sp), fixed.handle, _ptr(fi), moving.handle, _ptr(mi), n, _ptr(poses), _ptr(out), cap, _ptr(cnt))
    return rc, out, cnt


# ---- 5. sizes only the device knows -------------------------------------------------------------------------------------------------------------------------
def test_moving_set_just_written_by_an_asynchronous_batched_clip(ctx, po, fx):
    cols = 721
    pr = _proj(cols)
    clipper = api.SceneClipperProjective2D(ctx, pr, asynchronous=True, voxelize_resolution=0.0)
    guess = synth.compose_poses(fx.robots, np.array([[0.03, -0.02, 0.02]] * 6)).astype(np.float32)
    clipped = api.CloudSet.reserved_many(ctx, 6, cols)
    clipper.compute_batch(fx.m_set, guess, clipped, scene_index=np.zeros(6, np.int32))      # nothing waits: the six sizes stay on the device
    poses = np.tile(np.float32([0.02, -0.01, 0.01]), (6, 1))
    res = {}
    for kind in ("proj", "nn"):
        sp = _finder(ctx, kind, cols).slice_params()
        rc, out, cnt = _raw(ctx, sp, fx.scan_set, None, clipped, None, poses, cols)
        assert rc == 0, (kind, rc)
        res[kind] = [out[i, : cnt[i]].copy() for i in range(6)]
        if kind == "proj":      # the next round reads sizes nobody has resolved yet, again
            clipper.compute_batch(fx.m_set, guess, clipped, scene_index=np.zeros(6, np.int32))
    clouds = [clipped.download(i) for i in range(6)]
    assert min(len(c) for c in clouds) > 100
    copies = _multi(ctx, clouds)
    for kind in ("proj", "nn"):
        f, osp = _finder(ctx, kind, cols), _osp(po, kind, cols)
        one = _singles(f, fx.scan_set, np.arange(6), copies, np.arange(6), poses)
        for i in range(6):
            assert np.array_equal(res[kind][i], one[i]), (kind, i)
            assert np.array_equal(res[kind][i], po.find(osp, fx.scans[i], clouds[i], poses[i])), (kind, i)
        assert sum(len(r) for r in res[kind]) > 300


# ---- 6. a batch beyond the device buffer's budget: several launches over consecutive items ------------------------------------------------------------------------
def test_budget_crossing(ctx, po, fx):
    n_map = 100000
    per_launch = PAIR_BUDGET // n_map
    n = per_launch + 4
    assert per_launch >= 2 and n * n_map > PAIR_BUDGET
    huge = synth.make_map(fx.world, n_map, seed=4)
    hset = api.CloudSet(ctx, huge)
    which, poses = _perturbed(fx, n, 23)
    f = _finder(ctx, "dm")
    got = _run_and_compare(po, _osp(po, "dm"), f, fx.scan_set, fx.scans, which, hset, [huge], None, poses, oracle_items=(0, per_launch - 1, per_launch + 1), tag="budget")
    assert which[n - 1] == 5 and len(got[n - 1]) == 0      # (the last item is a scan-5 item: no pair)
    assert len(got[per_launch]) > 0 and len(got[n - 2]) > 0      # items of the second launch


# ---- 7. lsm2d_align_batch_pairs through the batch kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", ["S1", "S2", "S3"])
def test_align_batch_pairs_equals_single_alignment_calls_and_oracle(ctx, po, setting):
    n = 300
    spec = mb.batch(2024, n, setting)
    ns = spec["ns"]
    fixed = [api.CloudSet(ctx, sl["pts"], sl["offs"]) for sl in spec["slices"]]
    moving = api.CloudSet(ctx, spec["map"])
    al = mb.aligner(ctx, spec)
    assert al.param_keep_only_inlier_correspondences == (setting == "S2")
    r = al.compute_batch(fixed, [moving] * ns, spec["x0"], priors=spec["priors"], fixed_index=spec["fixed_index"], want_stats=True, want_pairs=True)
    plain = al.compute_batch(fixed, [moving] * ns, spec["x0"], priors=spec["priors"], fixed_index=spec["fixed_index"], want_stats=True)
    for k in ("pose", "information", "status", "iterations"):
        assert np.array_equal(getattr(r, k).view(np.uint32) if getattr(r, k).dtype == np.float32 else getattr(r, k),
                              getattr(plain, k).view(np.uint32) if getattr(plain, k).dtype == np.float32 else getattr(plain, k)), k
    kinds = spec["kinds"]
    assert np.any(r.iterations == 0) or np.any(kinds == "empty")
    assert set(np.unique(kinds)) >= {"empty", "nan", "inf", "far", "converge"}
    # one alignment per call: those calls keep the single finder calls, so the check is independent of the batch kernels
    for i in range(n):
        r1 = al.compute_batch(fixed, [moving] * ns, spec["x0"][i:i + 1], priors=None if spec["priors"] is None else [spec["priors"][i]],
                              fixed_index=np.ascontiguousarray(spec["fixed_index"][:, i:i + 1]), want_pairs=True)
        assert int(r1.iterations[0]) == int(r.iterations[i]) and np.array_equal(r1.pose[0].view(np.uint32), r.pose[i].view(np.uint32)), (i, kinds[i])
        for s in range(ns):
            assert np.array_equal(r.pairs[i][s], r1.pairs[0][s]), ("batch vs one alignment per call", i, s, kinds[i], len(r.pairs[i][s]), len(r1.pairs[0][s]))
        if int(r.iterations[i]) < 1:
            assert all(len(p) == 0 for p in r.pairs[i]), (i, kinds[i])
    for i in range(0, n, 10):
        w = mb.oracle_align(po, spec, i, device_order=True, want_pairs=True)
        for s in range(ns):
            assert np.array_equal(r.pairs[i][s], w["pairs"][s]), ("batch vs oracle", i, s, kinds[i])
    if not spec["keep_only_inlier"]:      # every returned vector set IS the last iteration's correspondence set: the in-kernel digest says so
        dg = api.pair_digests(r.stats)
        for i in range(n):
            its = int(r.iterations[i])
            if its < 1:
                continue
            host = sum(po.pair_digest(r.pairs[i][s], s) for s in range(ns)) & 0xFFFFFFFFFFFFFFFF
            assert host == int(dg[i][its - 1]), ("digest", i, kinds[i])
    assert sum(len(p) for row in r.pairs for p in row) > 10000


# ---- 8. one batch in flight -----------------------------------------------------------------------------------------------------------------------------------------
def test_with_one_batch_in_flight(ctx, po, fx):
    al = api.MultiAligner2D(ctx, max_iterations=10, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(_finder(ctx, "proj"), min_num_correspondences=10))
    x0 = fx.x0[:5]
    scans5 = _multi(ctx, fx.scans[:5])
    want = al.compute_batch([scans5], [fx.m_set], x0)
    f = _finder(ctx, "nn")
    want_pairs = f.compute_batch(fx.scan_set, fx.small_set, fx.x0)
    prep = al.prepare_batch([scans5], [fx.m_set], x0)
    prep.begin()
    got_pairs = f.compute_batch(fx.scan_set, fx.small_set, fx.x0)
    got = prep.wait(copy=True)
    assert np.array_equal(got.pose.view(np.uint32), want.pose.view(np.uint32)) and np.array_equal(got.status, want.status)
    for k in range(6):
        assert np.array_equal(got_pairs[k], want_pairs[k]), k
        assert np.array_equal(got_pairs[k], po.find(_osp(po, "nn"), fx.scans[k], fx.small, fx.x0[k])), k


# ---- 9. errors ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_errors(ctx, fx):
    sp = _finder(ctx, "proj").slice_params()
    # capacity one short: refused before anything is launched, nothing written
    rc, out, cnt = _raw(ctx, sp, fx.scan_set, None, fx.m_set, None, fx.x0, 1080)
    assert rc == CAPACITY_EXCEEDED and np.all(out == -7) and np.all(cnt == -7)
    spn = _finder(ctx, "nn").slice_params()
    rc, out, cnt = _raw(ctx, spn, fx.scan_set, None, fx.three, np.int32([1] * 6), fx.x0, len(fx.big) - 1)      # the LARGEST moving cloud counts
    assert rc == CAPACITY_EXCEEDED and np.all(out == -7) and np.all(cnt == -7)
    rc, out, cnt = _raw(ctx, sp, fx.scan_set, None, fx.m_set, None, fx.x0, 1081)
    assert rc == 0 and cnt.tolist() == ORACLE_COUNTS[1081]
    # indices out of range; NULL index over a set of neither 1 nor n_items clouds
    for fi, mi in ((np.int32([0, 1, 2, 3, 4, 6]), None), (np.int32([0, 1, 2, 3, 4, -1]), None), (None, np.int32([0, 0, 0, 0, 0, 1]))):
        rc, out, cnt = _raw(ctx, sp, fx.scan_set, fi, fx.m_set, mi, fx.x0, 1081)
        assert rc == BAD_ARGUMENT and np.all(cnt == -7)
    rc, _, cnt = _raw(ctx, sp, fx.scan_set, None, fx.m_set, None, fx.x0[:4], 1081)
    assert rc == BAD_ARGUMENT and np.all(cnt == -7)
    # a set from another context
    other = api.Context(0)
    try:
        foreign = api.CloudSet(other, fx.m)
        rc, _, cnt = _raw(ctx, sp, fx.scan_set, None, foreign, None, fx.x0, 1081)
        assert rc == BAD_ARGUMENT and np.all(cnt == -7)
        rc, _, cnt = _raw(ctx, sp, foreign, np.zeros(6, np.int32), fx.m_set, None, fx.x0, 1081)
        assert rc == BAD_ARGUMENT and np.all(cnt == -7)
        del foreign
    finally:
        other.close()
    # NULL arguments
    lib = ctx._lib
    p = np.ascontiguousarray(fx.x0); out = np.empty((6, 1081, 2), np.int32); cnt = np.empty(6, np.int32)
    good = [ctx.handle, C.byref(sp), fx.scan_set.handle, None, fx.m_set.handle, None, 6, _ptr(p), _ptr(out), 1081, _ptr(cnt)]
    for k in (0, 1, 2, 4, 7, 8, 10):
        a = list(good); a[k] = None
        assert lib.lsm2d_find_correspondences_batch(*a) == BAD_ARGUMENT, k
    a = list(good); a[6] = -1
    assert lib.lsm2d_find_correspondences_batch(*a) == BAD_ARGUMENT
    # n_items 0: a successful no-op, whatever the item arrays are
    rc, out, cnt = _raw(ctx, sp, fx.scan_set, None, fx.m_set, None, None, 1081, n=0)
    assert rc == 0 and np.all(out == -7) and np.all(cnt == -7)
    # two batches in flight: refused like every call that moves data; with both waited for it works again
    al = api.MultiAligner2D(ctx, max_iterations=5, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(_finder(ctx, "proj"), min_num_correspondences=10))
    a, b = al.prepare_batch([fx.scan_set], [fx.m_set], fx.x0), al.prepare_batch([fx.scan_set], [fx.m_set], fx.x0[::-1].copy(), fixed_index=np.int32([[5, 4, 3, 2, 1, 0]]))
    a.begin(); b.begin()
    try:
        rc, out, cnt = _raw(ctx, sp, fx.scan_set, None, fx.m_set, None, fx.x0, 1081)
        assert rc == BAD_ARGUMENT and np.all(out == -7) and np.all(cnt == -7)
    finally:
        ra, rb = a.wait(copy=True), b.wait(copy=True)
    assert np.array_equal(ra.pose.view(np.uint32), rb.pose[::-1].view(np.uint32))
    rc, _, cnt = _raw(ctx, sp, fx.scan_set, None, fx.m_set, None, fx.x0, 1081)
    assert rc == 0 and cnt.tolist() == ORACLE_COUNTS[1081]
