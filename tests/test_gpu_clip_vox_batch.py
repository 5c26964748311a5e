"""GPU tests of the batched clipper's voxelised form: lsm2d_clip_scene_voxelized_batch (k_clip_vox_batch), SceneClipperProjective2D.compute_batch
with voxelize_resolution > 0 and api.TrackerBatch(clip_voxelize_resolution=...).  Every tracker's cloud and count must be the bits of
lsm2d_clip_scene_voxelized for the same scene, pose, offset and resolution, and of the fp32 oracle's clip_scene_voxelized; a voxelising fleet
must equal the oracle's chain per seed in both orders of summation.  Every comparison is np.array_equal (or == on digests): no tolerance
appears in this file."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import tracker_chain as tc
import tracker_chain_seq
import tracker_fleet_vox as tfv
from srrg2_laser_slam_2d_amd import api
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT, CAPACITY_EXCEEDED

pytestmark = pytest.mark.gpu

COLS = 721
RMIN, RMAX = 0.3, 20.0
SENSOR = np.float32([0.2, 0.1, 0.1])


def _proj(cols=COLS):
    return api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, RMIN, RMAX)


def _oproj(po, cols=COLS):
    return po.Projector(cols, -math.pi, math.pi, RMIN, RMAX, 0.0)


# the recipe of tests/test_gpu_tracker_batch.py, restated
def _cloud(rng, n, rmax=20.0):
    r = rng.uniform(0.5, rmax, n); a = rng.uniform(-math.pi, math.pi, n); b = rng.uniform(-math.pi, math.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a), np.cos(b), np.sin(b)], 1).astype(np.float32)


def _multi(ctx, clouds):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    pts = np.concatenate(clouds) if offs[-1] else np.zeros((0, 4), np.float32)
    return api.CloudSet(ctx, pts, offs if len(clouds) > 1 else None)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _poses(rng, n):
    return np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.uniform(-math.pi, math.pi, (n, 1))], 1).astype(np.float32)


def _vox_batch(ctx, pr, scenes, poses, sensor, res, clipped, scene_index=None, sync=True):
    n = len(poses); out = np.empty(n, np.int32) if sync else None
    p = np.ascontiguousarray(poses, np.float32)
    rc = ctx._lib.lsm2d_clip_scene_voxelized_batch(ctx.handle, C.byref(pr.struct()), scenes.handle, n, _ptr(scene_index), _ptr(p),
                                                   _ptr(np.ascontiguousarray(sensor, np.float32)), float(res), clipped.handle, _ptr(out))
    return rc, out


def _plain_batch(ctx, pr, scenes, poses, sensor, clipped, scene_index=None, sync=True):
    n = len(poses); out = np.empty(n, np.int32) if sync else None
    p = np.ascontiguousarray(poses, np.float32)
    rc = ctx._lib.lsm2d_clip_scene_batch(ctx.handle, C.byref(pr.struct()), scenes.handle, n, _ptr(scene_index), _ptr(p),
                                         _ptr(np.ascontiguousarray(sensor, np.float32)), clipped.handle, _ptr(out))
    return rc, out


def _own_set(ctx, cloud):
    """a copy of one scene in a single-cloud set of its own (what lsm2d_clip_scene_voxelized takes)"""
    if len(cloud) == 0:
        return api.CloudSet.reserved(ctx, 16)
    return api.CloudSet(ctx, np.array(cloud, np.float32, copy=True))


class _Single:
    """lsm2d_clip_scene_voxelized, one call per tracker, synchronous, into one reserved set"""

    def __init__(self, ctx, pr):
        self.ctx, self.pr = ctx, pr
        self.out = api.CloudSet.reserved(ctx, pr.param_canvas_cols)

    def __call__(self, own, pose, sensor, res):
        n = C.c_int32(0)
        rc = self.ctx._lib.lsm2d_clip_scene_voxelized(self.ctx.handle, C.byref(self.pr.struct()), own.handle, 0, _ptr(np.ascontiguousarray(pose, np.float32)),
                                                      _ptr(np.ascontiguousarray(sensor, np.float32)), float(res), self.out.handle, C.byref(n), None)
        assert rc == 0
        self.out._set_count(n.value)
        return self.out.download()


def _check_batch(ctx, po, pr, opr, clouds, scenes, poses, sensor, res, n_extra=2, rng=None):
    """synchronous into a reserved-many set of n + n_extra clouds (the extra ones filled beforehand, untouched afterwards), then asynchronous with
    the scenes permuted, into a fresh set: tracker i == the single call on a copy of its scene == the oracle.  Returns the voxelised and the plain sizes."""
    n = len(poses); cols = pr.param_canvas_cols
    owns = [_own_set(ctx, c) for c in clouds]
    single = _Single(ctx, pr)
    clipped = api.CloudSet.reserved_many(ctx, n + n_extra, cols)
    before = []
    if n_extra:
        filler = _multi(ctx, [_cloud(np.random.default_rng(3 + j), 400) for j in range(n + n_extra)])
        rc, _ = _plain_batch(ctx, pr, filler, np.zeros((n + n_extra, 3), np.float32), sensor, clipped)
        assert rc == 0
        clipped._set_pending()
        before = [clipped.download(n + j) for j in range(n_extra)]
        assert all(len(b) > 100 for b in before)
    rc, got_n = _vox_batch(ctx, pr, scenes, poses, sensor, res, clipped)
    assert rc == 0
    clipped._set_pending()
    sizes, plain_sizes = [], []
    for i in range(n):
        want = po.clip_scene_voxelized(opr, clouds[i], poses[i], sensor, res)
        one = single(owns[i], poses[i], sensor, res)
        got = clipped.download(i)
        assert got_n[i] == len(want) == len(one) == len(got), (i, got_n[i], len(want), len(one), len(got))
        assert np.array_equal(got, one), i
        assert np.array_equal(got, want), i
        sizes.append(len(want)); plain_sizes.append(len(po.clip_scene(opr, clouds[i], poses[i], sensor)[0]))
    for j in range(n_extra):
        assert np.array_equal(clipped.download(n + j), before[j]), j
    if rng is not None:
        perm = rng.permutation(n).astype(np.int32)
        clipped2 = api.CloudSet.reserved_many(ctx, n, cols)
        rc, _ = _vox_batch(ctx, pr, scenes, poses, sensor, res, clipped2, scene_index=perm, sync=False)
        assert rc == 0
        clipped2._set_pending()
        want_p = [po.clip_scene_voxelized(opr, clouds[perm[i]], poses[i], sensor, res) for i in range(n)]
        assert clipped2.counts.tolist() == [len(w) for w in want_p]
        for i in range(n):
            got = clipped2.download(i)
            assert np.array_equal(got, want_p[i]), i
            assert np.array_equal(got, single(owns[perm[i]], poses[i], sensor, res)), i
    return sizes, plain_sizes


# ---- 1. batch == single calls == oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [0.1, 2.0])
@pytest.mark.parametrize("n", [1, 5, 300])
def test_vox_batch_equals_single_calls_and_oracle(ctx, po, n, res):
    rng = np.random.default_rng(100 + n)
    sizes = [[0, 3, 700, 40000, 1500][i % 5] if n > 1 else 40000 for i in range(n)]
    clouds = [_cloud(rng, s) for s in sizes]
    scenes = _multi(ctx, clouds)
    poses = _poses(rng, n)
    vox, plain = _check_batch(ctx, po, _proj(), _oproj(po), clouds, scenes, poses, SENSOR, res, rng=rng)
    print("n %d res %g: voxelised %s plain %s" % (n, res, vox[:5], plain[:5]))
    assert all(v <= p for v, p in zip(vox, plain))
    assert any(v < p for v, p in zip(vox, plain))            # really voxelised: the test cannot pass on the plain path
    assert max(plain) == COLS                                # the 40000-point scenes fill the canvas (k at its limit)


# ---- 2. the sort at its limits --------------------------------------------------------------------------------------------------------------
def _fan(m, pose, sensor, cols):
    """m points on m distinct columns as seen from pose * sensor: each on the centre bearing of its column (float64, then rounded: the rounding moves
    a bearing by ~1e-7 rad, a column is 2 pi / cols wide), ranges 2 .. 10 m"""
    from srrg2_laser_slam_2d_amd import synth
    cam = synth.compose_poses(np.asarray(pose, np.float64)[None, :], np.asarray(sensor, np.float64)[None, :])[0]
    col = (np.arange(m) * (cols // m if m <= cols // 2 else 1)).astype(np.float64)      # spread over the circle while there is room, else the first m columns
    ang = -math.pi + (col + 0.5) * (2.0 * math.pi / cols)
    r = 2.0 + 8.0 * ((np.arange(m) * 37) % 101) / 101.0
    x, y = r * np.cos(ang), r * np.sin(ang)
    c, s = math.cos(cam[2]), math.sin(cam[2])
    wx, wy = cam[0] + c * x - s * y, cam[1] + s * x + c * y
    nb = ang + cam[2] + math.pi      # normals towards the sensor
    return np.stack([wx, wy, np.cos(nb), np.sin(nb)], 1).astype(np.float32)


FAN_SIZES = [64, 65, 1024, 1025]


@pytest.mark.parametrize("res", [0.25, 5e-4])
def test_vox_batch_sort_limits(ctx, po, res):
    cols = 2048
    rng = np.random.default_rng(2048)
    pr, opr = _proj(cols), _oproj(po, cols)
    poses = _poses(rng, 2 + len(FAN_SIZES))
    clouds = [_cloud(rng, 40000), _cloud(rng, 1500)] + [_fan(m, poses[2 + j], SENSOR, cols) for j, m in enumerate(FAN_SIZES)]
    plain = [len(po.clip_scene(opr, c, p, SENSOR)[0]) for c, p in zip(clouds, poses)]
    assert plain[0] == cols                                   # k = kVoxMax: the full bitonic network
    assert 1024 < plain[1] < 2048                             # np2 = 2048 with k well below it
    assert plain[2:] == FAN_SIZES                             # the edges of np2, of a wave's 128-element block, of one pass of the head scan
    scenes = _multi(ctx, clouds)
    vox, _ = _check_batch(ctx, po, pr, opr, clouds, scenes, poses, SENSOR, res, rng=rng)
    print("res %g: plain %s voxelised %s" % (res, plain, vox))
    assert vox[0] <= plain[0] and (res < 0.01 or vox[0] < plain[0])


def test_vox_batch_refuses_more_than_2048_columns(ctx):
    cols = 2049
    rng = np.random.default_rng(2049)
    pr = _proj(cols)
    clouds = [_cloud(rng, 3000) for _ in range(3)]
    scenes = _multi(ctx, clouds); poses = _poses(rng, 3)
    clipped = api.CloudSet.reserved_many(ctx, 3, cols)
    rc, before_n = _plain_batch(ctx, pr, scenes, poses, SENSOR, clipped)
    assert rc == 0 and before_n.min() > 100
    clipped._set_pending()
    before = [clipped.download(i) for i in range(3)]
    for sync in (True, False):
        rc, _ = _vox_batch(ctx, pr, scenes, poses[::-1].copy(), SENSOR, 0.1, clipped, sync=sync)
        assert rc == CAPACITY_EXCEEDED and b"2048" in ctx._lib.lsm2d_last_error(ctx.handle)
    ctx.synchronize()
    clipped._set_pending()
    assert clipped.counts.tolist() == before_n.tolist()
    for i in range(3):
        assert np.array_equal(clipped.download(i), before[i]), i


# ---- 3. degenerate merges --------------------------------------------------------------------------------------------------------------------
def _wall():
    y = np.linspace(-3.0, 3.0, 5000)
    return np.stack([np.full_like(y, 2.0), y, np.full_like(y, -1.0), np.zeros_like(y)], 1).astype(np.float32)


@pytest.mark.parametrize("res,want_n", [(0.1, 60), (1.0, 6), (100.0, 2)])
def test_vox_batch_long_runs_and_an_empty_clip(ctx, po, res, want_n):
    rng = np.random.default_rng(33)
    pr, opr = _proj(), _oproj(po)
    zero = np.zeros(3, np.float32)
    far = _cloud(rng, 900); far[:, :2] *= np.float32(30.0) / np.hypot(far[:, 0], far[:, 1]).astype(np.float32)[:, None]      # every point 30 m out: beyond the range gate
    clouds = [_cloud(rng, 700), _wall(), far, _wall()]
    poses = np.zeros((4, 3), np.float32)
    assert len(po.clip_scene(opr, _wall(), zero, zero)[0]) == 227 and len(po.clip_scene(opr, far, zero, zero)[0]) == 0
    scenes = _multi(ctx, clouds)
    vox, plain = _check_batch(ctx, po, pr, opr, clouds, scenes, poses, zero, res, rng=rng)      # zero offset: the s_identity path
    assert vox[1] == vox[3] == want_n and plain[1] == 227
    assert vox[2] == 0 and vox[0] > 0


# ---- 4. sizes only the device knows --------------------------------------------------------------------------------------------------------
def test_vox_batch_reads_pending_sizes(ctx, po):
    rng = np.random.default_rng(7)
    n, res = 6, 0.1
    traj, ranges, _ = tc.scenario(2, 4)
    pre = api.RawDataPreprocessorProjective2D(ctx, range_min=tc.RMIN, range_max=tc.RMAX, voxelize_resolution=0.02)
    rr = np.stack([ranges[i % 2][i % 3] for i in range(n)]).astype(np.float32)
    pre.setRawData(rr[::-1].copy(), tc.A0, tc.A1, 0.0, 30.0); scans = pre.compute()
    pre.setRawData(rr, tc.A0, tc.A1, 0.0, 30.0); pre.refill(scans)           # sizes pending now
    pr = _proj(); sensor = np.float32([-0.3, 0.0, math.pi])
    single = _Single(ctx, pr)
    poses = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-1, 1, (n, 1))], 1).astype(np.float32)
    clipped = api.CloudSet.reserved_many(ctx, n, COLS)
    rc, got_n = _vox_batch(ctx, pr, scans, poses, sensor, res, clipped)
    assert rc == 0
    scans._set_pending(); clipped._set_pending()
    copies = [scans.download(i) for i in range(n)]
    for i in range(n):
        want = single(_own_set(ctx, copies[i]), poses[i], sensor, res)
        assert got_n[i] == len(want) and len(want) > 50 and np.array_equal(clipped.download(i), want), i
        assert np.array_equal(want, po.clip_scene_voxelized(_oproj(po), copies[i], poses[i], sensor, res)), i
    # a reserved-many scene set filled by an asynchronous batched merge
    maps = api.CloudSet.reserved_many(ctx, n, 8000)
    mg = api.MergerProjective2D(ctx, pr, 0.2, asynchronous=True)
    meas = _multi(ctx, [_cloud(rng, 600) for _ in range(n)])
    mg.compute_batch(maps, [meas, meas], np.zeros((n, 2, 3), np.float32) + np.float32([0.1, 0.0, 0.3]))
    rc, _ = _vox_batch(ctx, pr, maps, poses, sensor, res, clipped, sync=False)
    assert rc == 0
    clipped._set_pending(); maps._set_pending()
    copies = [maps.download(i) for i in range(n)]          # (the single clipper refuses a reserved-many set: each map's rows go into a set of its own)
    want = [single(_own_set(ctx, copies[i]), poses[i], sensor, res) for i in range(n)]
    assert clipped.counts.tolist() == [len(w) for w in want]
    for i in range(n):
        assert len(want[i]) > 50 and np.array_equal(clipped.download(i), want[i]), i


# ---- 5. voxelize_resolution <= 0 is the plain batched clip ---------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [0.0, -1.0])
def test_vox_batch_without_resolution_is_the_plain_batch(ctx, res):
    rng = np.random.default_rng(50)
    n = 5
    clouds = [_cloud(rng, s) for s in [0, 3, 700, 40000, 1500]]
    scenes = _multi(ctx, clouds); poses = _poses(rng, n); pr = _proj()
    a = api.CloudSet.reserved_many(ctx, n, COLS); b = api.CloudSet.reserved_many(ctx, n, COLS)
    rc_a, n_a = _vox_batch(ctx, pr, scenes, poses, SENSOR, res, a)
    rc_b, n_b = _plain_batch(ctx, pr, scenes, poses, SENSOR, b)
    assert rc_a == 0 and rc_b == 0 and n_a.tolist() == n_b.tolist() and n_a.max() == COLS
    a._set_pending(); b._set_pending()
    for i in range(n):
        assert np.array_equal(a.download(i), b.download(i)), i
    rc, _ = _vox_batch(ctx, pr, scenes, poses, SENSOR, res, a, sync=False)
    assert rc == 0
    a._set_pending()
    assert a.counts.tolist() == n_b.tolist()
    for i in range(n):
        assert np.array_equal(a.download(i), b.download(i)), i


# ---- 6. bad arguments ------------------------------------------------------------------------------------------------------------------------
def test_vox_batch_bad_arguments(ctx, po):
    rng = np.random.default_rng(9)
    pr = _proj(); lib = ctx._lib; prs = C.byref(pr.struct())
    many = api.CloudSet.reserved_many(ctx, 4, 2 * COLS)
    single = api.CloudSet.reserved(ctx, 2 * COLS)
    small_many = api.CloudSet.reserved_many(ctx, 4, COLS - 1)
    three = api.CloudSet.reserved_many(ctx, 3, COLS)
    scenes = _multi(ctx, [_cloud(rng, 50) for _ in range(4)])
    poses = np.zeros((4, 3), np.float32); s0 = np.zeros(3, np.float32)

    def clip(sc, n, idx, out, ctx_h=ctx.handle, pr_=prs, poses_=_ptr(poses), s_=_ptr(s0)):
        return lib.lsm2d_clip_scene_voxelized_batch(ctx_h, pr_, None if sc is None else sc.handle, n, _ptr(idx), poses_, s_, 0.1, None if out is None else out.handle, None)

    assert clip(scenes, 4, None, many) == 0
    assert clip(scenes, 4, None, many, ctx_h=None) == BAD_ARGUMENT               # a NULL for each required pointer
    assert clip(scenes, 4, None, many, pr_=None) == BAD_ARGUMENT
    assert clip(None, 4, None, many) == BAD_ARGUMENT
    assert clip(scenes, 4, None, many, poses_=None) == BAD_ARGUMENT
    assert clip(scenes, 4, None, many, s_=None) == BAD_ARGUMENT
    assert clip(scenes, 4, None, None) == BAD_ARGUMENT
    assert clip(scenes, 0, None, many) == BAD_ARGUMENT and clip(scenes, -1, None, many) == BAD_ARGUMENT      # n_trackers < 1
    assert clip(scenes, 4, None, single) == BAD_ARGUMENT                        # clipped: not a reserved-many set
    assert clip(many, 4, None, many) == BAD_ARGUMENT                            # clipped is the scenes' set
    assert clip(scenes, 4, None, three) == BAD_ARGUMENT                         # clipped holds fewer than n clouds
    assert clip(scenes, 4, np.int32([0, 1, 2, 4]), many) == BAD_ARGUMENT        # scene index out of range
    assert clip(scenes, 4, np.int32([0, 1, 2, -1]), many) == BAD_ARGUMENT
    assert clip(scenes, 4, None, small_many) == CAPACITY_EXCEEDED               # clouds smaller than canvas_cols
    assert b"canvas_cols" in lib.lsm2d_last_error(ctx.handle)
    # the context is still usable: case 1 with n = 1 again
    ctx.synchronize()
    rng = np.random.default_rng(101)
    cloud = _cloud(rng, 40000); poses1 = _poses(rng, 1)
    vox, plain = _check_batch(ctx, po, pr, _oproj(po), [cloud], _multi(ctx, [cloud]), poses1, SENSOR, 0.1, rng=rng)
    assert vox[0] < plain[0] == COLS


# ---- the Python classes ------------------------------------------------------------------------------------------------------------------------
def test_scene_clipper_compute_batch_voxelises(ctx, po):
    rng = np.random.default_rng(77)
    n = 4
    clouds = [_cloud(rng, s) for s in [40000, 700, 1500, 40000]]
    scenes = _multi(ctx, clouds); poses = _poses(rng, n); pr = _proj()
    for asynchronous in (False, True):
        clipper = api.SceneClipperProjective2D(ctx, pr, voxelize_resolution=0.1, asynchronous=asynchronous)
        clipper.setSensorInRobot(SENSOR)
        clipped = api.CloudSet.reserved_many(ctx, n, COLS)
        got_n = clipper.compute_batch(scenes, poses, clipped)
        want = [po.clip_scene_voxelized(_oproj(po), clouds[i], poses[i], SENSOR, 0.1) for i in range(n)]
        assert (got_n is None) == asynchronous
        assert clipped.counts.tolist() == [len(w) for w in want] and (asynchronous or got_n.tolist() == [len(w) for w in want])
        for i in range(n):
            assert np.array_equal(clipped.download(i), want[i]), i
        assert len(want[0]) < COLS


# ---- 7. a voxelised fleet against the oracle -------------------------------------------------------------------------------------------------
FLEET_RES, FLEET_STEPS = 0.1, 4
DEVICE_FIELDS = ("step", "status", "pose_hex", "information", "scans", "scan_points", "clip_points", "clip", "map_points", "map")


def _fleet_seeds():
    seeds = tfv.fleet_seeds(5, FLEET_STEPS)
    assert seeds == [1, 2, 3, 4, 5]
    return seeds


@functools.lru_cache(maxsize=None)
def _oracle_record(sequential: bool, seed: int, steps: int):
    """one oracle chain per (order of summation, seed, length): tracker_chain.scenario(steps, seed) depends on its length"""
    from oracle import pyoracle as po
    return tfv.run_oracle(tracker_chain_seq._SequentialOracle(po) if sequential else po, seed, steps, FLEET_RES)


def _check_fleet(got, seeds, sequential, steps=FLEET_STEPS):
    for j, s in enumerate(seeds):
        w = _oracle_record(sequential, s, steps)
        assert len(got[j]) == len(w) == steps
        for a, b in zip(got[j], w):
            assert set(a) == set(DEVICE_FIELDS)
            assert all(a[f] == b[f] for f in DEVICE_FIELDS), (s, a["step"], {f: (a[f], b[f]) for f in DEVICE_FIELDS if a[f] != b[f]})
            assert a["clip_points"] < b["plain_clip_points"], (s, a["step"])      # every step really voxelised: the fleet cannot pass on the plain path
            assert b["status"] == 0, (s, b)                                           # the oracle's own chain: every alignment ends Success


def test_vox_fleet_equals_the_oracle(ctx):
    seeds = _fleet_seeds()
    got = tfv.run_fleet(api, ctx, seeds, FLEET_STEPS, FLEET_RES)
    assert ctx.get_option("last_align_path") == 3                      # k_align_pair (n <= 256)
    _check_fleet(got, seeds, False)


def test_vox_fleet_sum_order_1(ctx):
    seeds = _fleet_seeds()
    ctx.set_option("sum_order", 1)
    try:
        got = tfv.run_fleet(api, ctx, seeds, FLEET_STEPS, FLEET_RES)
    finally:
        ctx.set_option("sum_order", 0)
    _check_fleet(got, seeds, True)


@pytest.mark.parametrize("sum_order", [0, 1])
def test_vox_fleet_above_256(ctx, sum_order):
    seeds = [_fleet_seeds()[i % 5] for i in range(260)]
    ctx.set_option("sum_order", sum_order)
    try:
        got = tfv.run_fleet(api, ctx, seeds, 2, FLEET_RES)
        if sum_order == 0:
            assert ctx.get_option("last_align_path") == 1                  # k_align (n > 256)
    finally:
        ctx.set_option("sum_order", 0)
    _check_fleet(got, seeds, bool(sum_order), steps=2)
