"""lsm2d_voxelize on the GPU (ABI 0.7.11): every output -- clouds, counts, dropped counts -- is voxelize_cases.reference's, bit for bit (the reference is pinned
to the CPU oracle by tests/test_voxelize_abi.py).  Sizes round the sort tile, runs across and beyond a tile, the ends of the key's ranges, several inputs and
groups, poses, in place over a reserved-many set, assembly into one of the inputs, both coefficient sets, the two existing callers of voxelize_lds, the
capacity verdict (all or nothing), every refusal, determinism, and the voxelised set as input of the aligner and of a KD-tree finder.
The scan of the device side is ONE workgroup that takes "voxelize_scan_tiles" (16) tiles' counters a pass and carries its running sum from pass to pass: the
case `scan_boundary` lies just past 16 tiles, and the fleet of 40 clouds (more than 32 groups: a seventh digit, the sorted keys end in the other buffer)
crosses it too, in place.  Both are held to the reference like every other case."""
import ctypes as C
import math

import numpy as np
import pytest

import voxelize_cases as vc
from gpu_helpers import _aligner, _kd_finder
from srrg2_laser_slam_2d_amd import _capi, api, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
T = vc.TILE
CASES = vc.all_cases()
_REF = {}


def _ref(name):
    if name not in _REF:
        _REF[name] = vc.case_reference(CASES[name])
    return _REF[name]


def _source(ctx, clouds):
    offs = np.zeros(len(clouds) + 1, np.int32); offs[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.ascontiguousarray(np.concatenate(clouds), F32).reshape(-1, 4)
    return api.CloudSet(ctx, pts, offs if len(clouds) > 1 else None)


def _clouds(cs, n=None):
    return [cs.download(i) for i in range(cs.n_clouds if n is None else n)]


def _assert_equal(got_set, counts, dropped, want, tag=""):
    w_clouds, w_counts, w_dropped = want
    assert counts.tolist() == w_counts.tolist() and dropped.tolist() == w_dropped.tolist(), (tag, counts.tolist(), w_counts.tolist(), dropped.tolist(), w_dropped.tolist())
    assert got_set.counts[:len(w_counts)].tolist() == w_counts.tolist(), tag
    for g, w in enumerate(w_clouds):
        got = got_set.download(g)
        assert got.shape == w.shape and got.tobytes() == w.tobytes(), (tag, g, len(w), int(np.flatnonzero((got.view(np.uint32) != w.view(np.uint32)).any(axis=1))[0]) if got.shape == w.shape else -1)


def _run(ctx, case, dst=None):
    src = _source(ctx, case["clouds"])
    p = api.VoxelizeParams(*case["params"])
    return api.voxelize(ctx, p, src, None, case["poses"], case["groups"], case["n_groups"], dst)


def test_tiling_constants(ctx):
    assert ctx.get_option("voxelize_tile") == T == _capi.VOXELIZE_TILE
    assert ctx.get_option("voxelize_scan_tiles") == vc.SCAN_TILES == _capi.VOXELIZE_SCAN_TILES == 16      # tiles a pass of the one-workgroup scan takes
    assert len(CASES["scan_boundary"]["clouds"][0]) == vc.SCAN_TILES * T + 5
    with pytest.raises(api.Lsm2dError):
        ctx.set_option("voxelize_tile", 512)


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_the_reference_bit_for_bit(ctx, name):
    dst, counts, dropped = _run(ctx, CASES[name])
    print(name, "inputs", [len(c) for c in CASES[name]["clouds"]], "counts", counts.tolist(), "dropped", dropped.tolist(), "kernel ms %.3f" % ctx.last_kernel_ms())
    _assert_equal(dst, counts, dropped, _ref(name), name)


def test_two_runs_agree_bitwise(ctx):
    a = _run(ctx, CASES["long_run"]); b = _run(ctx, CASES["long_run"])
    assert a[1].tolist() == b[1].tolist() and a[0].download().tobytes() == b[0].download().tobytes()


# ---- in place over a reserved-many set; assembly into one of the inputs ----------------------------------------------------------------------------------
def _fleet(ctx, n_clouds=6, capacity=2 * T + 64):
    """a reserved-many set filled by the call itself (group k = input k): (set, its clouds as the reference gives them)"""
    rng = np.random.default_rng(21)
    clouds = []
    for k in range(n_clouds):
        n = [T + 40, 300, 0, 2 * T + 1, 5, 900][k % 6]
        a = rng.uniform(-np.pi, np.pi, n); r = rng.uniform(1.0, 9.0, n)
        clouds.append(np.stack([r * np.cos(a), r * np.sin(a), -np.cos(a), -np.sin(a)], 1).astype(F32))
    many = api.CloudSet.reserved_many(ctx, n_clouds, capacity)
    p = api.VoxelizeParams(0.02, 1.0)
    got = api.voxelize(ctx, p, _source(ctx, clouds), None, None, np.arange(n_clouds), n_clouds, many)
    want = vc.reference(clouds, None, np.arange(n_clouds), n_clouds, (0.02, 1.0))
    _assert_equal(*got, want, "fleet fill")
    return many, want[0]


def test_fleet_decimated_in_place(ctx):
    many, first = _fleet(ctx)
    n = many.n_clouds
    assert max(len(c) for c in first) > T      # a group that crosses a tile
    want = vc.reference(first, None, np.arange(n), n, (0.25, 1.0))
    dst, counts, dropped = api.voxelize(ctx, api.VoxelizeParams(0.25, 1.0), many, None, None, np.arange(n), n, many)
    assert dst is many and counts.sum() < sum(len(c) for c in first)      # coarser cells: it decimates
    _assert_equal(many, counts, dropped, want, "in place")


def test_fleet_of_forty_groups_in_place(ctx):
    """more than 32 groups: 42 + 6 + 1 sort bits are SEVEN digits, so the sorted keys end in the second buffer; 29 000 points: past the scan's first pass"""
    many, first = _fleet(ctx, 40)      # (the fill is itself a call with 40 groups, held to the reference there)
    assert sum(len(c) for c in first) > vc.SCAN_TILES * T
    want = vc.reference(first, None, np.arange(40), 40, (0.25, 1.0))
    dst, counts, dropped = api.voxelize(ctx, api.VoxelizeParams(0.25, 1.0), many, None, None, np.arange(40), 40, many)
    assert dst is many and 0 < counts.sum() < sum(len(c) for c in first)
    _assert_equal(many, counts, dropped, want, "forty in place")


def test_assembly_with_poses_into_one_of_the_inputs(ctx):
    many, first = _fleet(ctx, 5, 5 * T)
    poses = CASES["assembly"]["poses"]
    want = vc.reference(first, poses, None, 1, (0.1, 1.0))
    dst, counts, dropped = api.voxelize(ctx, api.VoxelizeParams(0.1, 1.0), many, None, poses, None, 1, many, [3])
    assert counts.tolist() == want[1].tolist() and dropped.tolist() == want[2].tolist() and counts[0] > T
    got = _clouds(many)
    assert got[3].tobytes() == want[0][0].tobytes() and many.counts[3] == counts[0]
    for k in (0, 1, 2, 4):      # the other inputs are as they were
        assert got[k].tobytes() == first[k].tobytes(), k


# ---- the two existing callers of voxelize_lds -------------------------------------------------------------------------------------------------------------
def test_equals_the_voxelising_clipper(ctx):
    rng = np.random.default_rng(31)
    cols = 1440
    proj = api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, 30.0)
    columns = np.sort(rng.choice(cols, 1300, replace=False))
    a = -math.pi + (columns + 0.5) * (2.0 * math.pi / cols); r = 3.0 + rng.uniform(-0.01, 0.01, len(a))
    scene = np.stack([r * np.cos(a), r * np.sin(a), -np.cos(a), -np.sin(a)], 1).astype(F32)
    for res in (0.05, 0.2):
        outs = []
        for vox in (0.0, res):
            clipper = api.SceneClipperProjective2D(ctx, proj, voxelize_resolution=vox)
            clipper.setFullScene(api.CloudSet(ctx, scene)); clipper.setRobotInLocalMap(np.zeros(3, F32)); clipper.setSensorInRobot(np.zeros(3, F32))
            outs.append(clipper.compute())
        plain, voxelised = outs
        assert plain.n_points == len(scene) <= 2048      # one point per column
        dst, counts, _ = api.voxelize(ctx, api.VoxelizeParams.clipper(res), plain)
        assert counts[0] == voxelised.n_points < len(scene)
        assert dst.download().tobytes() == voxelised.download().tobytes(), res


def test_equals_the_voxelising_preprocessor(ctx):
    world = synth.make_world(6)
    poses = synth.sample_poses(world, 3, seed=21)
    ranges = synth.make_scan_ranges(world, poses, n_beams=721, angle_min=-2.35, angle_max=2.35, noise_sigma=0.004, seed=7)
    for res in (0.02, 0.1):
        sets = []
        for vox in (0.0, res):
            pre = api.RawDataPreprocessorProjective2D(ctx, range_min=0.3, range_max=20.0, voxelize_resolution=vox)
            pre.setRawData(ranges, -2.35, 2.35, 0.0, 30.0); sets.append(pre.compute())
        plain, voxelised = sets
        dst, counts, dropped = api.voxelize(ctx, api.VoxelizeParams.preprocessor(res), plain, None, None, np.arange(3), 3)
        assert counts.tolist() == voxelised.counts.tolist() and dropped.tolist() == [0, 0, 0] and counts.sum() < plain.n_points
        for k in range(3):
            assert dst.download(k).tobytes() == voxelised.download(k).tobytes(), (res, k)


# ---- all or nothing ---------------------------------------------------------------------------------------------------------------------------------------
def _four_distinct(ctx, capacity):
    """a reserved-many set of four clouds with keys of their own, filled by the call; cloud g: 300 + 10 g voxels"""
    rng = np.random.default_rng(41)
    d = vc.distinct(4 * 400, rng)
    clouds = [d[400 * g:400 * g + 300 + 10 * g] for g in range(4)]
    many = api.CloudSet.reserved_many(ctx, 4, capacity)
    api.voxelize(ctx, api.VoxelizeParams(vc.RES, 1.0), _source(ctx, clouds), None, None, np.arange(4), 4, many)
    before = _clouds(many)
    assert [len(c) for c in before] == [300, 310, 320, 330]
    return many, before


@pytest.mark.parametrize("room", [-1, 0])
def test_capacity_one_voxel_short_changes_nothing_and_exact_fits(ctx, room):
    # group 0 = clouds 0, 1, 2 into cloud 0 (one of its inputs), group 1 = cloud 3 into cloud 3 (in place): 930 and 330 voxels
    many, before = _four_distinct(ctx, 930 + room)
    want = vc.reference(before, None, [0, 0, 0, 1], 2, (vc.RES, 1.0))
    assert want[1].tolist() == [930, 330]
    p = api.VoxelizeParams(vc.RES, 1.0)
    if room < 0:
        with pytest.raises(api.Lsm2dError) as e:
            api.voxelize(ctx, p, many, None, None, [0, 0, 0, 1], 2, many, [0, 3])
        assert e.value.code == _capi.CAPACITY_EXCEEDED and e.value.counts.tolist() == [930, 330]      # what would have been needed
        assert many.counts.tolist() == [300, 310, 320, 330]
        after = _clouds(many)
        for k in range(4):
            assert after[k].tobytes() == before[k].tobytes(), k      # every destination cloud bitwise unchanged, the in-place one too
    else:
        _, counts, dropped = api.voxelize(ctx, p, many, None, None, [0, 0, 0, 1], 2, many, [0, 3])
        assert counts.tolist() == [930, 330] and dropped.tolist() == [0, 0]
        after = _clouds(many)
        assert after[0].tobytes() == want[0][0].tobytes() and after[3].tobytes() == want[0][1].tobytes()
        assert after[1].tobytes() == before[1].tobytes() and after[2].tobytes() == before[2].tobytes()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, params, src, n_inputs, src_index, pose, group, n_groups, dst, dst_index, counts, dropped):
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)      # noqa: E731
    si, gr, di = i32(src_index), i32(group), i32(dst_index)
    ps = None if pose is None else np.ascontiguousarray(pose, F32)
    p = None if params is None else params.struct()
    return _capi.load().lsm2d_voxelize(ctx.handle if ctx else None, None if p is None else C.byref(p), None if src is None else src.handle, n_inputs, api._ptr(si),
                                   api._ptr(ps), api._ptr(gr), n_groups, None if dst is None else dst.handle, api._ptr(di), api._ptr(counts), api._ptr(dropped))


def test_refusals_launch_nothing_and_change_nothing(ctx):
    many, before = _four_distinct(ctx, 1000)
    plain = _source(ctx, before)
    ok = api.VoxelizeParams(vc.RES, 1.0)
    BAD = _capi.BAD_ARGUMENT
    sentinel = np.full(4, -77, np.int32)

    def refused(**kw):
        a = dict(params=ok, src=many, n_inputs=4, src_index=None, pose=None, group=[0, 1, 2, 3], n_groups=4, dst=many, dst_index=None)
        a.update(kw)
        counts, dropped = sentinel.copy(), sentinel.copy()
        uploads = ctx.get_option("uploads")
        code = _raw(None if kw.get("no_ctx") else ctx, a["params"], a["src"], a["n_inputs"], a["src_index"], a["pose"], a["group"], a["n_groups"], a["dst"], a["dst_index"],
                    None if kw.get("no_counts") else counts, dropped)
        assert code == BAD, (kw, code)
        assert counts.tolist() == sentinel.tolist() and dropped.tolist() == sentinel.tolist() and ctx.get_option("uploads") == uploads
        assert many.counts.tolist() == [300, 310, 320, 330]

    refused(no_ctx=True); refused(params=None); refused(src=None); refused(dst=None); refused(no_counts=True)
    # a set that belongs to another context, as source and as destination
    ctx2 = api.Context(0)
    try:
        other = api.CloudSet.reserved_many(ctx2, 4, 1000)
        refused(src=other); refused(dst=other)
    finally:
        ctx2.close()
    for res in (0.0, -1.0, float("nan"), float("inf")):
        refused(params=api.VoxelizeParams(res, 1.0)); refused(params=api.VoxelizeParams(0.5, res))
    refused(n_inputs=0); refused(n_groups=0)
    refused(src_index=[0, 1, 2, 4]); refused(src_index=[0, -1, 2, 3]); refused(n_inputs=5, group=[0, 1, 2, 3, 0])      # an index outside the source set
    refused(dst_index=[0, 1, 2, 4]); refused(n_groups=5, group=[0, 1, 2, 4])                                           # ... outside the destination set
    refused(group=[0, 1, 2, 4]); refused(group=[0, -1, 2, 3])
    refused(dst_index=[0, 1, 1, 2])                                                                                    # a destination twice
    refused(dst=plain)                                                                                                 # not a reserved set
    refused(n_groups=_capi.VOXELIZE_MAX_GROUPS + 1, group=[0, 1, 2, 3])
    # more input points than the limit: the same cloud named again and again
    reps = _capi.VOXELIZE_MAX_POINTS // 330 + 1
    refused(n_inputs=reps, src_index=np.full(reps, 3), group=np.zeros(reps))
    # two batches in flight
    wl = synth.make_workload(16, 4000, seed=3)
    al = _aligner(ctx)
    fx = [api.CloudSet(ctx, wl.scan_points[:wl.scan_offsets[8]], wl.scan_offsets[:9])]; mv = [api.CloudSet(ctx, wl.map_points)]
    p1 = al.prepare_batch(fx, mv, wl.x0[:8]); p2 = al.prepare_batch(fx, mv, wl.x0[:8])
    p1.begin(); p2.begin()
    try:
        refused()
    finally:
        p1.wait(); p2.wait()
    after = _clouds(many)
    for k in range(4):
        assert after[k].tobytes() == before[k].tobytes(), k
    # the context is usable and the call still right
    _, counts, _ = api.voxelize(ctx, ok, many, None, None, [0, 1, 2, 3], 4, many)
    assert counts.tolist() == [300, 310, 320, 330]


# ---- the voxelised set is a set like any other ------------------------------------------------------------------------------------------------------------
def test_voxelised_set_feeds_the_aligner_and_a_kd_tree_finder(ctx):
    wl = synth.make_workload(4, 20000, seed=2)
    scans = api.CloudSet(ctx, wl.scan_points, wl.scan_offsets)
    dst = api.CloudSet.reserved(ctx, len(wl.map_points))
    dst.upload(wl.map_points)
    scan0 = wl.scan_points[wl.scan_offsets[0]:wl.scan_offsets[1]]
    kd = _kd_finder(ctx, 0.5)
    scan_in_map = synth.invert_poses(wl.x0[:1].astype(np.float64))[0].astype(F32)
    kd.setFixed(dst); kd.setMoving(api.CloudSet(ctx, scan0)); kd.setLocalMapInSensor(scan_in_map)
    old_pairs = kd.compute()      # the set carries a KD-tree of its OLD points now (and the aligner's row copies below)
    al = _aligner(ctx)
    al.compute_batch([scans], [dst], wl.x0)
    _, counts, _ = api.voxelize(ctx, api.VoxelizeParams(0.02, 1.0), api.CloudSet(ctx, wl.map_points), dst=dst)
    print("map", len(wl.map_points), "->", counts.tolist())
    assert 100 < counts[0] < len(wl.map_points) and dst.n_points == counts[0]      # it decimated, and a map is left
    fresh = api.CloudSet(ctx, dst.download())
    a, b = al.compute_batch([scans], [dst], wl.x0), al.compute_batch([scans], [fresh], wl.x0)
    assert np.array_equal(a.status, b.status) and a.pose.tobytes() == b.pose.tobytes() and a.information.tobytes() == b.information.tobytes()
    assert np.any(a.status == 0)
    pairs = kd.compute()      # must rebuild its tree
    kd2 = _kd_finder(ctx, 0.5)
    kd2.setFixed(fresh); kd2.setMoving(api.CloudSet(ctx, scan0)); kd2.setLocalMapInSensor(scan_in_map)
    want = kd2.compute()
    assert len(want) > 100 and np.array_equal(pairs, want) and not np.array_equal(pairs, old_pairs)
