"""GPU tests of N independent trackers per call: reserved-many sets, lsm2d_clip_scene_batch (k_clip_batch), lsm2d_merge_scene_batch
(k_merge_batch) and api.TrackerBatch.  Every tracker's output must be the bits the single-tracker calls produce -- clip and merge against N
single calls, whole tracker chains against the CPU oracle per seed and against the committed single-tracker goldens.  No tolerance
appears in this file."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import tracker_chain as tc
import tracker_chain_seq
import tracker_fleet
from conftest import golden_path
from srrg2_laser_slam_2d_amd import api
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT, CAPACITY_EXCEEDED

pytestmark = pytest.mark.gpu

COLS = 721


def _proj(cols=COLS, rmax=20.0):
    return api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, rmax)


def _cloud(rng, n, rmax=20.0):
    r = rng.uniform(0.5, rmax, n); a = rng.uniform(-math.pi, math.pi, n); b = rng.uniform(-math.pi, math.pi, n)
    return np.stack([r * np.cos(a), r * np.sin(a), np.cos(b), np.sin(b)], 1).astype(np.float32)


def _multi(ctx, clouds):
    offs = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    pts = np.concatenate(clouds) if offs[-1] else np.zeros((0, 4), np.float32)
    return api.CloudSet(ctx, pts, offs if len(clouds) > 1 else None)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _clip_batch(ctx, pr, scenes, poses, sensor, clipped, scene_index=None, sync=True):
    n = len(poses); out = np.empty(n, np.int32) if sync else None
    p = np.ascontiguousarray(poses, np.float32)
    rc = ctx._lib.lsm2d_clip_scene_batch(ctx.handle, C.byref(pr.struct()), scenes.handle, n, _ptr(scene_index), _ptr(p),
                                         _ptr(np.ascontiguousarray(sensor, np.float32)), clipped.handle, _ptr(out))
    return rc, out


def _single_clips(ctx, pr, scenes, poses, sensor, scene_index=None):
    out = []
    ctx._lib.lsm2d_cloudset_num_points(scenes.handle)          # sizes the device knows resolved first: the single call then takes them by value
    single = api.CloudSet.reserved(ctx, pr.param_canvas_cols)
    for i, pose in enumerate(poses):
        n = C.c_int32(0)
        rc = ctx._lib.lsm2d_clip_scene(ctx.handle, C.byref(pr.struct()), scenes.handle, int(scene_index[i]) if scene_index is not None else i,
                                       _ptr(np.ascontiguousarray(pose, np.float32)), _ptr(np.ascontiguousarray(sensor, np.float32)), single.handle, C.byref(n), None)
        assert rc == 0
        single._set_count(n.value)
        out.append(single.download())
    return out


@pytest.mark.parametrize("n", [1, 5, 300])
def test_clip_batch_equals_single_calls(ctx, n):
    rng = np.random.default_rng(100 + n)
    sizes = [[0, 3, 700, 40000, 1500][i % 5] if n > 1 else 40000 for i in range(n)]
    scenes = _multi(ctx, [_cloud(rng, s) for s in sizes])
    pr = _proj()
    poses = np.concatenate([rng.uniform(-1, 1, (n, 2)), rng.uniform(-math.pi, math.pi, (n, 1))], 1).astype(np.float32)
    sensor = np.float32([0.2, 0.1, 0.1])
    want = _single_clips(ctx, pr, scenes, poses, sensor)
    clipped = api.CloudSet.reserved_many(ctx, n + 2, COLS)
    rc, got_n = _clip_batch(ctx, pr, scenes, poses, sensor, clipped)
    assert rc == 0 and got_n.tolist() == [len(w) for w in want]
    clipped._set_pending()
    for i in range(n):
        assert np.array_equal(clipped.download(i), want[i]), i
    # asynchronous, scenes permuted through the index array, into a fresh set: nothing waits, the sizes are the device's until asked for
    perm = rng.permutation(n).astype(np.int32)
    clipped2 = api.CloudSet.reserved_many(ctx, n, COLS)
    rc, _ = _clip_batch(ctx, pr, scenes, poses, sensor, clipped2, scene_index=perm, sync=False)
    assert rc == 0
    clipped2._set_pending()
    want_p = _single_clips(ctx, pr, scenes, poses, sensor, scene_index=perm)
    assert clipped2.counts.tolist() == [len(w) for w in want_p]
    for i in range(n):
        assert np.array_equal(clipped2.download(i), want_p[i]), i


def test_clip_batch_reads_pending_sizes(ctx):
    """scenes whose sizes only the device knows (a refilled scan set; a reserved-many set after an asynchronous batched merge)"""
    rng = np.random.default_rng(7)
    n = 6
    traj, ranges, _ = tc.scenario(2, 4)
    pre = api.RawDataPreprocessorProjective2D(ctx, range_min=tc.RMIN, range_max=tc.RMAX, voxelize_resolution=0.02)
    rr = np.stack([ranges[i % 2][i % 3] for i in range(n)]).astype(np.float32)
    pre.setRawData(rr[::-1].copy(), tc.A0, tc.A1, 0.0, 30.0); scans = pre.compute()
    pre.setRawData(rr, tc.A0, tc.A1, 0.0, 30.0); pre.refill(scans)           # sizes pending now
    pr = _proj(); sensor = np.float32([-0.3, 0.0, math.pi])
    poses = np.concatenate([rng.uniform(-0.5, 0.5, (n, 2)), rng.uniform(-1, 1, (n, 1))], 1).astype(np.float32)
    clipped = api.CloudSet.reserved_many(ctx, n, COLS)
    rc, got_n = _clip_batch(ctx, pr, scans, poses, sensor, clipped)
    assert rc == 0
    scans._set_pending(); clipped._set_pending()
    want = _single_clips(ctx, pr, scans, poses, sensor)       # (the single calls read resolved sizes)
    assert got_n.tolist() == [len(w) for w in want]
    for i in range(n):
        assert np.array_equal(clipped.download(i), want[i]), i
    # a reserved-many scene set filled by an asynchronous batched merge
    maps = api.CloudSet.reserved_many(ctx, n, 8000)
    mg = api.MergerProjective2D(ctx, pr, 0.2, asynchronous=True)
    meas = _multi(ctx, [_cloud(rng, 600) for _ in range(n)])
    mg.compute_batch(maps, [meas, meas], np.zeros((n, 2, 3), np.float32) + np.float32([0.1, 0.0, 0.3]))
    rc, got_n = _clip_batch(ctx, pr, maps, poses, sensor, clipped, sync=False)
    assert rc == 0
    clipped._set_pending(); maps._set_pending()
    # (the single clipper refuses a reserved-many set: each map's rows go into a set of its own)
    copies = _multi(ctx, [maps.download(i) for i in range(n)])
    want = _single_clips(ctx, pr, copies, poses, sensor)
    assert clipped.counts.tolist() == [len(w) for w in want]
    for i in range(n):
        assert np.array_equal(clipped.download(i), want[i]), i


@pytest.mark.parametrize("n,k", [(1, 2), (5, 1), (5, 3), (64, 4), (300, 2)])
def test_merge_batch_equals_merge_scenes(ctx, n, k):
    rng = np.random.default_rng(1000 * n + k)
    pr = _proj()
    # measurement clouds of mixed size (empty ones included), points out to range_max (beyond 0.9 * range_max: ignored)
    meas = [_multi(ctx, [_cloud(rng, [0, 5, 700, 300][(i + j) % 4]) for i in range(n)]) for j in range(k)]
    midx = np.stack([rng.permutation(n) for _ in range(k)]).astype(np.int32)
    cap = 4 * k * COLS + 64
    maps = api.CloudSet.reserved_many(ctx, n, cap)
    singles = [api.CloudSet.reserved(ctx, cap) for _ in range(n)]
    lib = ctx._lib
    for rnd in range(3):
        poses = np.concatenate([rng.uniform(-0.3, 0.3, (n, k, 2)), rng.uniform(-0.5, 0.5, (n, k, 1))], 2).astype(np.float32)
        sync = rnd != 1
        sizes = np.empty(n, np.int32); counts = np.empty((n, k, 3), np.int32)
        handles = (C.c_void_p * k)(*[m.handle.value for m in meas])
        rc = lib.lsm2d_merge_scene_batch(ctx.handle, C.byref(pr.struct()), maps.handle, n, None, k, handles, _ptr(midx), _ptr(poses), 0.2,
                                         _ptr(sizes) if sync else None, _ptr(counts) if sync else None)
        assert rc == 0
        for i in range(n):
            sz = C.c_int32(0); cn = np.empty((k, 3), np.int32)
            idx = (C.c_int32 * k)(*[int(midx[j, i]) for j in range(k)])
            assert lib.lsm2d_merge_scenes(ctx.handle, C.byref(pr.struct()), singles[i].handle, k, handles, idx, _ptr(np.ascontiguousarray(poses[i])), 0.2,
                                          C.byref(sz), _ptr(cn)) == 0
            singles[i]._set_count(sz.value)
            if sync:
                assert sizes[i] == sz.value and np.array_equal(counts[i], cn), (rnd, i)
    maps._set_pending()
    assert maps.counts.tolist() == [int(s.n_points) for s in singles]
    for i in range(n):
        assert np.array_equal(maps.download(i), singles[i].download()), i


def _check_fleet(got, seeds, want_of):
    for j, s in enumerate(seeds):
        w = want_of(s)
        assert len(got[j]) == len(w)
        for a, b in zip(got[j], w):
            assert a == b, (s, a["step"], {f: (a[f], b[f]) for f in b if a[f] != b[f]})


def test_fleet_chains_equal_the_oracle_small_batch(ctx, po):
    seeds = [4, 1, 2, 3, 5, 6, 7]
    got = tracker_fleet.run_fleet(api, ctx, seeds, 8)
    assert ctx.get_option("last_align_path") == 3                      # k_align_pair (n <= 256)
    g = json.load(open(golden_path("tracker_chain.json")))
    assert got[0] == g["steps"]
    _check_fleet(got, seeds, lambda s: tracker_fleet.run_oracle(po, s, 8))


def test_fleet_chains_equal_the_oracle_above_256(ctx, po):
    seeds = tracker_fleet.fleet_seeds(300)
    assert 4 in seeds
    got = tracker_fleet.run_fleet(api, ctx, seeds, 8)
    assert ctx.get_option("last_align_path") == 1                      # k_align (n > 256)
    g = json.load(open(golden_path("tracker_chain.json")))
    assert got[seeds.index(4)] == g["steps"]
    _check_fleet(got, seeds, lambda s: tracker_fleet.run_oracle(po, s, 8))


def test_fleet_sum_order_1(ctx, po):
    ctx.set_option("sum_order", 1)
    try:
        seeds = [4, 9, 11]
        got = tracker_fleet.run_fleet(api, ctx, seeds, 8)
    finally:
        ctx.set_option("sum_order", 0)
    g = json.load(open(golden_path("tracker_chain_seq.json")))
    assert got[0] == g["steps"]
    _check_fleet(got, seeds, lambda s: tracker_fleet.run_oracle(tracker_chain_seq._SequentialOracle(po), s, 8))


def test_fleet_replay_1000_steps(ctx):
    g = json.load(open(golden_path("tracker_replay_1000.json")))
    assert g["steps_total"] == 1000 and g["record_every"] == 50 and len(g["steps"]) == 20
    quiet = api.Context(0, kernel_timing=False)
    try:
        got = tracker_fleet.run_fleet(api, quiet, [4, 4, 4], 1000, record_every=50, map_capacity=60000)
    finally:
        quiet.close()
    for j in range(3):
        assert got[j] == g["steps"], j


def test_capacity_all_or_nothing_and_reset(ctx):
    rng = np.random.default_rng(5)
    pr = _proj(); lib = ctx._lib
    n, k = 3, 2
    cap = k * COLS + 100
    maps = api.CloudSet.reserved_many(ctx, n, cap)
    big = _cloud(rng, 700, 15.0)
    meas = _multi(ctx, [big, np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32)])
    handles = (C.c_void_p * k)(meas.handle.value, meas.handle.value)
    poses = np.zeros((n, k, 3), np.float32); poses[:, 1, 2] = 0.05
    assert lib.lsm2d_merge_scene_batch(ctx.handle, C.byref(pr.struct()), maps.handle, n, None, k, handles, None, _ptr(poses), 0.2, None, None) == 0
    maps._set_pending()
    before = [maps.download(i) for i in range(n)]
    assert len(before[0]) > 100 and len(before[1]) == 0
    # the host's bounds say "no room" for every scene; the real sizes leave room for trackers 1 and 2 only: nothing is launched
    rc = lib.lsm2d_merge_scene_batch(ctx.handle, C.byref(pr.struct()), maps.handle, n, None, k, handles, None, _ptr(poses), 0.2, None, None)
    assert rc == CAPACITY_EXCEEDED and b"tracker 0" in lib.lsm2d_last_error(ctx.handle)
    ctx.synchronize()
    for i in range(n):
        assert np.array_equal(maps.download(i), before[i]), i
    # a tracker that starts a new local map: clear, then merge == a fresh single map
    assert lib.lsm2d_cloudset_clear_clouds(maps.handle, 1, _ptr(np.int32([0]))) == 0
    maps.clear([2])
    sizes = np.empty(1, np.int32)
    assert lib.lsm2d_merge_scene_batch(ctx.handle, C.byref(pr.struct()), maps.handle, 1, _ptr(np.int32([0])), k, handles, None, _ptr(poses[:1]), 0.2,
                                       _ptr(sizes), None) == 0
    fresh = api.CloudSet.reserved(ctx, cap)
    mg = api.MergerProjective2D(ctx, pr, 0.2)
    mg.setScene(fresh)
    assert mg.compute_all([meas, meas], poses[0], [0, 0]) == sizes[0]
    maps._set_pending()
    assert np.array_equal(maps.download(0), fresh.download())
    assert np.array_equal(maps.download(1), before[1]) and len(maps.download(2)) == 0


def test_bad_arguments(ctx):
    rng = np.random.default_rng(9)
    pr = _proj(); lib = ctx._lib; prs = C.byref(pr.struct())
    many = api.CloudSet.reserved_many(ctx, 4, 2 * COLS)
    one_many = api.CloudSet.reserved_many(ctx, 1, 2 * COLS)
    single = api.CloudSet.reserved(ctx, 2 * COLS)
    small_many = api.CloudSet.reserved_many(ctx, 4, COLS - 1)
    scenes = _multi(ctx, [_cloud(rng, 50) for _ in range(4)])
    poses = np.zeros((4, 3), np.float32); s0 = np.zeros(3, np.float32)
    mp = np.zeros((4, 4, 3), np.float32)
    h1 = (C.c_void_p * 1)(scenes.handle.value)
    h5 = (C.c_void_p * 5)(*([scenes.handle.value] * 5))
    hself = (C.c_void_p * 1)(many.handle.value)

    def clip(sc, n, idx, out):
        return lib.lsm2d_clip_scene_batch(ctx.handle, prs, sc.handle, n, _ptr(idx), _ptr(poses), _ptr(s0), out.handle, None)

    def merge(sc, n, idx, k, hs, midx=None):
        return lib.lsm2d_merge_scene_batch(ctx.handle, prs, sc.handle, n, _ptr(idx), k, hs, _ptr(midx), _ptr(mp), 0.2, None, None)

    assert clip(scenes, 4, None, many) == 0 and merge(many, 4, None, 1, h1) == 0
    assert clip(scenes, 4, None, single) == BAD_ARGUMENT                        # clipped: not a reserved-many set
    assert clip(scenes, 5, None, many) == BAD_ARGUMENT                          # more trackers than clipped clouds
    assert clip(scenes, 4, np.int32([0, 1, 2, 4]), many) == BAD_ARGUMENT        # scene index out of range
    assert clip(scenes, 4, np.int32([0, 1, 2, -1]), many) == BAD_ARGUMENT
    assert clip(many, 4, None, many) == BAD_ARGUMENT                            # scene == clipped
    assert clip(scenes, 0, None, many) == BAD_ARGUMENT
    assert clip(scenes, 4, None, small_many) == CAPACITY_EXCEEDED               # clouds smaller than canvas_cols
    assert merge(single, 1, None, 1, h1) == BAD_ARGUMENT                        # scenes: not a reserved-many set
    assert merge(many, 4, np.int32([0, 1, 1, 2]), 1, h1) == BAD_ARGUMENT        # duplicate scene index
    assert merge(many, 4, np.int32([0, 1, 2, 4]), 1, h1) == BAD_ARGUMENT        # out of range
    assert merge(many, 4, None, 0, h1) == BAD_ARGUMENT and merge(many, 4, None, 5, h5) == BAD_ARGUMENT     # n_measurements outside 1..4
    assert merge(many, 4, None, 1, hself) == BAD_ARGUMENT                       # measurement == scenes
    assert merge(many, 4, None, 1, h1, np.int32([0, 1, 2, 7])) == BAD_ARGUMENT  # measurement index out of range
    assert merge(many, 5, None, 1, h1) == BAD_ARGUMENT                          # more trackers than scenes
    assert lib.lsm2d_merge_scene_batch(ctx.handle, prs, many.handle, 4, None, 1, h1, None, _ptr(mp), 0.2, None, _ptr(np.empty(12, np.int32))) == BAD_ARGUMENT
    assert lib.lsm2d_cloudset_clear_clouds(single.handle, 0, None) == BAD_ARGUMENT
    assert lib.lsm2d_cloudset_clear_clouds(many.handle, 1, _ptr(np.int32([4]))) == BAD_ARGUMENT
    assert lib.lsm2d_cloudset_create_reserved_many(ctx.handle, 0, 10, C.byref(C.c_void_p())) == BAD_ARGUMENT
    assert lib.lsm2d_cloudset_create_reserved_many(ctx.handle, 2, 0, C.byref(C.c_void_p())) == BAD_ARGUMENT
    # a reserved-many set is never taken for a single reserved cloud, even with one cloud
    pts = _cloud(rng, 10)
    from srrg2_laser_slam_2d_amd import _capi
    pp = _capi.Preprocessor(721, tc.A0, tc.A1, tc.RMIN, tc.RMAX, 0.3, 5, 0.02)
    rr = np.full(721, 5.0, np.float32)
    for m in (many, one_many):
        assert lib.lsm2d_cloudset_upload(m.handle, _ptr(pts), len(pts)) == BAD_ARGUMENT
        assert lib.lsm2d_clip_scene(ctx.handle, prs, scenes.handle, 0, _ptr(s0), _ptr(s0), m.handle, None, None) == BAD_ARGUMENT
        assert lib.lsm2d_clip_scene(ctx.handle, prs, m.handle, 0, _ptr(s0), _ptr(s0), single.handle, None, None) == BAD_ARGUMENT
        assert lib.lsm2d_merge_scene(ctx.handle, prs, m.handle, scenes.handle, 0, _ptr(s0), 0.2, None, None) == BAD_ARGUMENT
        assert lib.lsm2d_merge_scenes(ctx.handle, prs, m.handle, 1, h1, None, _ptr(s0), 0.2, None, None) == BAD_ARGUMENT
        assert lib.lsm2d_preprocess_scan_into(ctx.handle, C.byref(pp), _ptr(rr), m.handle) == BAD_ARGUMENT
        assert lib.lsm2d_preprocess_scans_refill(ctx.handle, C.byref(pp), _ptr(rr), m.n_clouds, m.handle) == BAD_ARGUMENT
    # ... while the readers take it like any multi-cloud set
    ctx.synchronize()
    many._set_pending()
    assert many.counts.sum() > 0
    src = np.empty(COLS, np.int32)
    assert lib.lsm2d_project(ctx.handle, prs, many.handle, 3, _ptr(s0), _ptr(src), None, None) == 0


def test_cpp_fleet_step_through_the_bare_c_abi():
    """tests/cpp/track_batch_driver.cpp: the batched step against its own one-tracker-at-a-time loop, poses, statuses and local maps bit for bit
    (N = 5 on 3 scenarios, two episodes per side)"""
    import os
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "bench"))
    import track_batch_bench as tbb
    with tempfile.TemporaryDirectory() as d:
        tc_ = tbb.write_inputs(d, 3, 8)
        exe = tbb.build_driver(d)
        out = tbb.run(exe, d, tc_, 3, 8, 5, 2, timeout=300)
    assert out["bitwise_equal"] is True and out["differing_words"] == 0 and out["differing_maps"] == 0, out
    assert out["status_ok"] == 5 * 8
