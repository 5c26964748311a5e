"""lsm2d_occupancy_update / lsm2d_occupancy_render on the GPU (ABI 0.7.12): every output -- hits, misses, rays walked, points dropped -- is
occupancy_cases.reference's, bit for bit (tests/test_occupancy_abi.py pins that reference), on grids of 1 x 1, 64 x 64, 65 x 63 and 130 x 70 cells.  Inputs
round the workgroup's stride (1 .. 1081 rays) and the round of 256 box tests (1 .. 300 inputs to one grid), 1, 3 and 40 grids with every optional array
given and NULL, 1081 rays of one origin (contention on one LDS word), accumulation over calls, clear / upload / download, saturation, the render against
api.occupancy_values, eight realistic scans into a 400 x 300 grid, clouds from the preprocessor and from an asynchronous merge (the size fetch), every
refusal, and two runs that agree bytewise.  Integer sums have no order: there is no tolerance anywhere."""
import ctypes as C
import math

import numpy as np
import pytest

import occupancy_cases as oc
from gpu_helpers import _aligner
from srrg2_laser_slam_2d_amd import _capi, api, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = oc.W, oc.H
CASES = oc.all_cases()
_REF = {}


def _ref(name, w, h):
    if (name, w, h) not in _REF:
        _REF[(name, w, h)] = oc.reference(CASES[name], w, h)
    return _REF[(name, w, h)]


def _source(ctx, clouds):
    offs = np.zeros(len(clouds) + 1, np.int32); offs[1:] = np.cumsum([len(c) for c in clouds])
    pts = np.ascontiguousarray(np.concatenate(clouds), F32).reshape(-1, 4)
    return api.CloudSet(ctx, pts, offs if len(clouds) > 1 else None)


def _grids(ctx, case, w, h):
    return api.GridSet(ctx, api.GridGeometry(case["origin"][0], case["origin"][1], case["resolution"], w, h), case["n_grids"])


def _download(gs):
    hm = [gs.download(g) for g in range(gs.n_grids)]
    return np.stack([x[0] for x in hm]), np.stack([x[1] for x in hm])


def _run(ctx, case, w, h, gs=None):
    gs = _grids(ctx, case, w, h) if gs is None else gs
    rays, dropped = api.occupancy_update(ctx, gs, _source(ctx, case["clouds"]), None, case["poses"], case["grids"])
    return gs, rays, dropped


def _assert_equal(gs, rays, dropped, want, tag=""):
    wh, wm, wr, wd = want
    assert rays.tolist() == wr.tolist() and dropped.tolist() == wd.tolist(), (tag, rays.tolist(), wr.tolist(), dropped.tolist(), wd.tolist())
    gh, gm = _download(gs)
    assert gh.dtype == np.uint32 and gh.shape == wh.shape
    assert gh.tobytes() == wh.tobytes(), (tag, "hits", np.argwhere(gh != wh)[:5].tolist())
    assert gm.tobytes() == wm.tobytes(), (tag, "misses", np.argwhere(gm != wm)[:5].tolist())


def test_tiling_constants(ctx):
    assert ctx.get_option("occupancy_tile") == oc.TILE == _capi.OCCUPANCY_TILE == 64
    with pytest.raises(api.Lsm2dError):
        ctx.set_option("occupancy_tile", 32)


@pytest.mark.parametrize("size", oc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_the_reference_bit_for_bit(ctx, name, size):
    w, h = size
    gs, rays, dropped = _run(ctx, CASES[name], w, h)
    print(name, size, "rays", rays.tolist(), "dropped", dropped.tolist(), "kernel ms %.3f" % ctx.last_kernel_ms())
    _assert_equal(gs, rays, dropped, _ref(name, w, h), (name, size))
    gs.close()


# ---- the workgroup's stride over an input's rays, and its rounds of 256 box tests -----------------------------------------------------------------------------
@pytest.mark.parametrize("n_rays", [1, 63, 64, 65, 257, 1081])
def test_one_input_of_n_rays(ctx, n_rays):
    case = oc.fan_case(n_rays)
    gs, rays, dropped = _run(ctx, case, W, H)
    _assert_equal(gs, rays, dropped, oc.reference(case, W, H), n_rays)
    assert rays.tolist() == [n_rays]
    gs.close()


@pytest.mark.parametrize("n_inputs", [1, 3, 256, 257, 300])
def test_n_inputs_to_one_grid(ctx, n_inputs):
    """300 inputs exceed one round of box tests; 256 fill it exactly"""
    case = oc.many_inputs_case(n_inputs)
    assert len(case["clouds"]) == n_inputs and oc.BLOCK == 256
    gs, rays, dropped = _run(ctx, case, W, H)
    _assert_equal(gs, rays, dropped, oc.reference(case, W, H), n_inputs)
    gs.close()


@pytest.mark.parametrize("n_grids", [1, 3, 40])
@pytest.mark.parametrize("given", ["none", "grid", "src_index", "pose", "all"])
def test_grids_and_optional_arrays(ctx, n_grids, given):
    """1, 3 and 40 grids; `grid`, `src_index` and `pose` each given and NULL"""
    rng = np.random.default_rng(100 + n_grids)
    n_clouds = max(2 * n_grids, 4)
    clouds = []
    for _ in range(n_clouds):
        a = rng.uniform(-np.pi, np.pi, 50); r = rng.uniform(0.0, 12.0, 50)
        clouds.append(np.stack([r * np.cos(a), r * np.sin(a), np.ones(50), np.zeros(50)], 1).astype(F32))
    src = _source(ctx, clouds)
    idx = rng.permutation(n_clouds)[:n_clouds - 1].astype(np.int32) if given in ("src_index", "all") else None      # a subset, out of order
    used = list(range(n_clouds)) if idx is None else idx.tolist()
    poses = np.stack([rng.uniform(-3, 3, len(used)), rng.uniform(-3, 3, len(used)), rng.uniform(-3, 3, len(used))], 1).astype(F32) if given in ("pose", "all") else None
    grid = rng.integers(0, n_grids, len(used)).astype(np.int32) if given in ("grid", "all") else None
    case = oc._case([clouds[k] for k in used], poses, grid, n_grids, origin=(-6.35, -3.45), resolution=0.1)
    gs = _grids(ctx, case, W, H)
    rays, dropped = api.occupancy_update(ctx, gs, src, idx, poses, grid)
    want = oc.reference(case, W, H)
    _assert_equal(gs, rays, dropped, want, (n_grids, given))
    assert want[0].sum() > 0 and (grid is None or n_grids == 1 or np.count_nonzero(want[2]) > 1)
    gs.close()


def test_contention_1081_rays_of_one_origin(ctx):
    case = oc.fan_case(1081, seed=8)
    gs, rays, dropped = _run(ctx, case, W, H)
    want = oc.reference(case, W, H)
    _assert_equal(gs, rays, dropped, want, "fan")
    r, live = oc.case_rays(case)
    longer = int((live & (np.abs(r[:, 2:] - r[:, :2]).max(1) > 0)).sum())
    assert longer > 1000 and gs.download(0)[1][31, 33] == longer      # the origin cell's misses: every live ray with L > 0
    gs.close()


# ---- accumulation and storage ------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_equal_one_call_with_both_inputs(ctx):
    a, b = CASES["octants"], CASES["borders"]
    both = oc._case(a["clouds"] + b["clouds"], np.concatenate([a["poses"], b["poses"]]))
    one, rays, dropped = _run(ctx, both, W, H)
    two, ra, da = _run(ctx, a, W, H)
    _, rb, db = _run(ctx, b, W, H, two)
    assert (ra + rb).tolist() == rays.tolist() and (da + db).tolist() == dropped.tolist()
    h1, m1 = _download(one); h2, m2 = _download(two)
    assert h1.tobytes() == h2.tobytes() and m1.tobytes() == m2.tobytes() and h1.sum() > 0
    _assert_equal(two, rays, dropped, oc.reference(both, W, H), "both")
    one.close(); two.close()


def test_clear_of_some_grids_leaves_the_others(ctx):
    case = oc.random_case(seed=23, n_inputs=8, n_points=100, n_grids=4)
    case["grids"] = np.arange(8, dtype=np.int32) % 4
    gs, _, _ = _run(ctx, case, W, H)
    wh, wm, _, _ = oc.reference(case, W, H)
    assert all(wh[g].sum() > 0 for g in range(4))
    gs.clear([1, 3])
    gh, gm = _download(gs)
    for g in range(4):
        if g in (1, 3):
            assert not gh[g].any() and not gm[g].any()
        else:
            assert gh[g].tobytes() == wh[g].tobytes() and gm[g].tobytes() == wm[g].tobytes()
    gs.clear()
    gh, gm = _download(gs)
    assert not gh.any() and not gm.any()
    gs.close()


def test_upload_then_download_round_trips(ctx):
    rng = np.random.default_rng(5)
    gs = api.GridSet(ctx, api.GridGeometry(0.0, 0.0, 0.5, 65, 63), 3)
    h = rng.integers(0, 1 << 32, (63, 65), dtype=np.uint64).astype(np.uint32); m = rng.integers(0, 1 << 32, (63, 65), dtype=np.uint64).astype(np.uint32)
    gs.upload(1, h, m)
    gh, gm = gs.download(1)
    assert gh.tobytes() == h.tobytes() and gm.tobytes() == m.tobytes()
    for g in (0, 2):
        a, b = gs.download(g)
        assert not a.any() and not b.any()
    gs.upload(1, None, h)      # a NULL array leaves that counter
    gh, gm = gs.download(1)
    assert gh.tobytes() == h.tobytes() and gm.tobytes() == h.tobytes()
    gs.upload(1, m, None)
    gh, gm = gs.download(1)
    assert gh.tobytes() == m.tobytes() and gm.tobytes() == h.tobytes()
    gs.close()


def test_counters_saturate(ctx):
    """a cell uploaded at 2^32 - 2 and crossed three times reads 2^32 - 1; so does a cell hit three times"""
    case = oc.cell_rays([(2, 3, 9, 3), (2, 3, 9, 4), (2, 3, 9, 5), (0, 0, 9, 3), (1, 1, 9, 3), (2, 2, 9, 3)])
    start = np.full((8, 12), 0xFFFFFFFE, np.uint32)
    gs = _grids(ctx, case, 12, 8)
    gs.upload(0, start, start)
    rays, dropped = api.occupancy_update(ctx, gs, _source(ctx, case["clouds"]), None, case["poses"], None)
    want = oc.reference(case, 12, 8, start[None], start[None])
    _assert_equal(gs, rays, dropped, want, "saturation")
    gh, gm = gs.download(0)
    assert gm[3, 2] == 0xFFFFFFFF and gh[3, 9] == 0xFFFFFFFF and gm[3, 9] == 0xFFFFFFFE and gh[0, 11] == 0xFFFFFFFE
    gs.close()


# ---- the render --------------------------------------------------------------------------------------------------------------------------------------------
def test_render_is_occupancy_values_of_the_downloaded_counts(ctx):
    case = CASES["random"]
    gs, _, _ = _run(ctx, case, W, H)
    _run(ctx, CASES["random"], W, H, gs)
    rng = np.random.default_rng(7)
    # hand-made counters in a grid set of their own: every small pair (ties among them), large and saturated values
    gs2 = api.GridSet(ctx, api.GridGeometry(0.0, 0.0, 0.5, W, H), 1)
    h = rng.integers(0, 40, (H, W)).astype(np.uint32); m = rng.integers(0, 40, (H, W)).astype(np.uint32)
    h[:8, :8] = np.arange(8, dtype=np.uint32)[:, None]; m[:8, :8] = np.arange(8, dtype=np.uint32)[None, :]
    h[10, :6] = [0xFFFFFFFF, 0xFFFFFFFF, 0, 0xFFFFFFFF, 1 << 31, 3]; m[10, :6] = [0xFFFFFFFF, 0, 0xFFFFFFFF, 1, 1 << 31, 0xFFFFFFFD]
    h[12:20] = rng.integers(0, 1 << 32, (8, W), dtype=np.uint64).astype(np.uint32); m[12:20] = rng.integers(0, 1 << 32, (8, W), dtype=np.uint64).astype(np.uint32)
    gs2.upload(0, h, m)
    for grids, g in ((gs, 0), (gs, 1), (gs2, 0)):
        dh, dm = grids.download(g)
        for min_visits in (0, 1, 2, 5):
            got = api.occupancy_render(ctx, grids, g, min_visits)
            want = api.occupancy_values(dh, dm, min_visits)
            assert got.dtype == np.int8 and got.shape == (H, W) and got.tobytes() == want.tobytes(), (g, min_visits, np.argwhere(got != want)[:5].tolist())
            assert got.min() >= -1 and got.max() <= 100
    got = api.occupancy_render(ctx, gs2, 0, 1)
    assert got[1, 7] == 12 and got[3, 5] == 38 and got[0, 0] == -1 and got[10, 0] == 50 and got[10, 1] == 100 and got[10, 2] == 0      # 12.5 -> 12, 37.5 -> 38
    gs.close(); gs2.close()


# ---- realistic scans ---------------------------------------------------------------------------------------------------------------------------------------
def _distance_to_segments(p, a, b):
    d = b - a
    t = np.clip(((p[:, None, :] - a[None]) * d[None]).sum(2) / (d * d).sum(1)[None], 0.0, 1.0)
    return np.linalg.norm(p[:, None, :] - (a[None] + t[..., None] * d[None]), axis=2).min(1)


def test_eight_scans_of_the_synthetic_world(ctx):
    world = synth.make_world(6)
    poses = synth.sample_poses(world, 8, seed=21)
    pts, offs = synth.make_scans(world, poses, n_beams=1081)
    clouds = [pts[offs[k]:offs[k + 1]] for k in range(8)]
    case = oc._case(clouds, poses.astype(F32), None, 1, origin=(-20.0, -15.0), resolution=0.1)
    gs = _grids(ctx, case, 400, 300)
    rays, dropped = api.occupancy_update(ctx, gs, api.CloudSet(ctx, pts, offs), None, case["poses"], None)
    print("rays", rays.tolist(), "dropped", dropped.tolist(), "kernel ms %.3f" % ctx.last_kernel_ms())
    want = oc.reference(case, 400, 300)
    _assert_equal(gs, rays, dropped, want, "world")
    assert rays[0] > 8 * 900 and dropped[0] == 0
    # on the CPU side, the reference alone: every cell rendered >= 50 lies within one cell diagonal of a wall segment (its centre does); no cell excluded
    img = api.occupancy_values(want[0][0], want[1][0], 1)
    cy, cx = np.nonzero(img >= 50)
    assert len(cx) > 100
    centres = np.stack([-20.0 + 0.1 * (cx + 0.5), -15.0 + 0.1 * (cy + 0.5)], 1)
    assert _distance_to_segments(centres, world.a, world.b).max() <= 0.1 * math.sqrt(2.0)
    assert (img == 0).sum() > 10 * len(cx)      # and free space was cleared
    assert api.occupancy_render(ctx, gs, 0, 1).tobytes() == img.tobytes()
    gs.close()


# ---- sources -----------------------------------------------------------------------------------------------------------------------------------------------
def test_clouds_of_the_preprocessor_and_of_an_asynchronous_merge(ctx):
    world = synth.make_world(6)
    poses = synth.sample_poses(world, 3, seed=21)
    ranges = synth.make_scan_ranges(world, poses, n_beams=721, angle_min=-2.35, angle_max=2.35, noise_sigma=0.004, seed=7)
    pre = api.RawDataPreprocessorProjective2D(ctx, range_min=0.3, range_max=20.0, voxelize_resolution=0.0)
    pre.setRawData(ranges, -2.35, 2.35, 0.0, 30.0)
    scans = pre.compute()      # lsm2d_preprocess_scans: three clouds made on the device
    gs = api.GridSet(ctx, api.GridGeometry(-20.0, -15.0, 0.1, 400, 300), 1)
    rays, dropped = api.occupancy_update(ctx, gs, scans, None, poses.astype(F32), None)
    clouds = [scans.download(k) for k in range(3)]
    case = oc._case(clouds, poses.astype(F32), None, 1, origin=(-20.0, -15.0), resolution=0.1)
    _assert_equal(gs, rays, dropped, oc.reference(case, 400, 300), "preprocessor")
    assert rays[0] == sum(len(c) for c in clouds) > 1000
    # an asynchronous merge leaves the scene's size known to the device only: the call fetches it
    proj = api.PointNormal2fProjectorPolar(721, -math.pi, math.pi, 0.3, 30.0)
    scene = api.CloudSet.reserved(ctx, 4096)
    merger = api.MergerProjective2D(ctx, proj, asynchronous=True)
    merger.setScene(scene)
    for k in range(2):
        merger.setMeasurement(scans, k); merger.setMeasurementInScene(synth.compose_poses(synth.invert_poses(poses[:1]), poses[k:k + 1])[0].astype(F32))
        assert merger.compute() == -1
    assert scene._pending
    gs.clear()
    rays, dropped = api.occupancy_update(ctx, gs, scene, None, poses[:1].astype(F32), None)
    merged = scene.download()
    assert len(merged) > len(clouds[0]) and rays[0] + dropped[0] == len(merged)
    case = oc._case([merged], poses[:1].astype(F32), None, 1, origin=(-20.0, -15.0), resolution=0.1)
    _assert_equal(gs, rays, dropped, oc.reference(case, 400, 300), "asynchronous merge")
    gs.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------
def _raw_update(ctx, gs, src, n_inputs, src_index, pose, grid, rays, dropped):
    i32 = lambda a: None if a is None else np.ascontiguousarray(a, np.int32)      # noqa: E731
    si, gr = i32(src_index), i32(grid)
    ps = None if pose is None else np.ascontiguousarray(pose, F32)
    return _capi.load().lsm2d_occupancy_update(ctx.handle if ctx else None, None if gs is None else gs.handle, None if src is None else src.handle, n_inputs,
                                               api._ptr(si), api._ptr(ps), api._ptr(gr), api._ptr(rays), api._ptr(dropped))


def test_refusals_launch_nothing_and_change_nothing(ctx):
    lib = _capi.load()
    BAD = _capi.BAD_ARGUMENT
    case = oc.random_case(seed=31, n_inputs=4, n_points=83, n_grids=2)
    gs, _, _ = _run(ctx, case, W, H)
    src = _source(ctx, case["clouds"])
    before = _download(gs)
    sentinel = np.full(2, -77, np.int32)

    def refused(**kw):
        a = dict(gs=gs, src=src, n_inputs=4, src_index=None, pose=case["poses"], grid=case["grids"])
        a.update({k: v for k, v in kw.items() if k != "no_ctx"})
        rays, dropped = sentinel.copy(), sentinel.copy()
        uploads = ctx.get_option("uploads")
        code = _raw_update(None if kw.get("no_ctx") else ctx, a["gs"], a["src"], a["n_inputs"], a["src_index"], a["pose"], a["grid"], rays, dropped)
        assert code == BAD, (kw, code)
        assert rays.tolist() == sentinel.tolist() and dropped.tolist() == sentinel.tolist() and ctx.get_option("uploads") == uploads

    refused(no_ctx=True); refused(gs=None); refused(src=None)
    refused(n_inputs=0); refused(n_inputs=-1)
    refused(src_index=[0, 1, 2, 4]); refused(src_index=[0, -1, 2, 3]); refused(n_inputs=5, grid=[0, 1, 0, 1, 0], pose=np.zeros((5, 3), F32))      # an index outside the set
    refused(grid=[0, 1, 2, 0]); refused(grid=[0, -1, 1, 0])
    reps = _capi.OCCUPANCY_MAX_RAYS // 83 + 1      # more input points than the limit: the same cloud named again and again
    refused(n_inputs=reps, src_index=np.zeros(reps), pose=np.zeros((reps, 3), F32), grid=np.zeros(reps))
    ctx2 = api.Context(0)      # a set of another context, as source and as grids
    try:
        refused(src=api.CloudSet(ctx2, case["clouds"][0])); refused(gs=api.GridSet(ctx2, gs.geometry, 2))
    finally:
        ctx2.close()
    # the grid set's own refusals
    h = C.c_void_p()
    def create(geo, n_grids=1, with_ctx=True, with_geo=True, with_out=True):      # noqa: E306
        g = geo.struct()
        return lib.lsm2d_gridset_create(ctx.handle if with_ctx else None, C.byref(g) if with_geo else None, n_grids, C.byref(h) if with_out else None)
    ok = api.GridGeometry(0.0, 0.0, 0.1, 64, 64)
    assert create(ok, with_ctx=False) == BAD and create(ok, with_geo=False) == BAD and create(ok, with_out=False) == BAD
    for res in (0.0, -1.0, float("nan"), float("inf")):
        assert create(api.GridGeometry(0.0, 0.0, res, 64, 64)) == BAD
    for o in (float("nan"), float("inf"), float("-inf")):
        assert create(api.GridGeometry(o, 0.0, 0.1, 64, 64)) == BAD and create(api.GridGeometry(0.0, o, 0.1, 64, 64)) == BAD
    for side in (0, -1, _capi.OCCUPANCY_MAX_SIDE + 1):
        assert create(api.GridGeometry(0.0, 0.0, 0.1, side, 64)) == BAD and create(api.GridGeometry(0.0, 0.0, 0.1, 64, side)) == BAD
    assert create(ok, 0) == BAD and create(ok, -3) == BAD
    assert create(api.GridGeometry(0.0, 0.0, 0.1, 16384, 16384), 2) == BAD and create(ok, _capi.OCCUPANCY_MAX_CELLS // 4096 + 1) == BAD      # the cells of the set
    assert not h.value
    assert lib.lsm2d_gridset_clear(None, 0, None) == BAD and lib.lsm2d_gridset_clear(gs.handle, 1, api._ptr(np.array([2], np.int32))) == BAD
    z = np.zeros((H, W), np.uint32)
    assert lib.lsm2d_gridset_upload(gs.handle, 2, api._ptr(z), api._ptr(z)) == BAD and lib.lsm2d_gridset_upload(gs.handle, -1, api._ptr(z), api._ptr(z)) == BAD
    assert lib.lsm2d_gridset_download(gs.handle, 2, api._ptr(z), api._ptr(z)) == BAD and lib.lsm2d_gridset_download(None, 0, api._ptr(z), api._ptr(z)) == BAD
    img = np.full((H, W), 55, np.int8); rp = _capi.OccupancyRenderParamsC(1)
    for args in ((None, gs.handle, 0, C.byref(rp), api._ptr(img)), (ctx.handle, None, 0, C.byref(rp), api._ptr(img)), (ctx.handle, gs.handle, 2, C.byref(rp), api._ptr(img)),
                 (ctx.handle, gs.handle, -1, C.byref(rp), api._ptr(img)), (ctx.handle, gs.handle, 0, None, api._ptr(img)), (ctx.handle, gs.handle, 0, C.byref(rp), None)):
        assert lib.lsm2d_occupancy_render(*args) == BAD
    assert np.all(img == 55)
    # two batches in flight
    wl = synth.make_workload(16, 4000, seed=3)
    al = _aligner(ctx)
    fx = [api.CloudSet(ctx, wl.scan_points[:wl.scan_offsets[8]], wl.scan_offsets[:9])]; mv = [api.CloudSet(ctx, wl.map_points)]
    p1 = al.prepare_batch(fx, mv, wl.x0[:8]); p2 = al.prepare_batch(fx, mv, wl.x0[:8])
    p1.begin(); p2.begin()
    try:
        refused()
        assert lib.lsm2d_occupancy_render(ctx.handle, gs.handle, 0, C.byref(rp), api._ptr(img)) == BAD and np.all(img == 55)
    finally:
        p1.wait(); p2.wait()
    after = _download(gs)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    # the context is usable and the call still right
    rays, dropped = api.occupancy_update(ctx, gs, src, None, case["poses"], case["grids"])
    want = oc.reference(case, W, H, *before)
    _assert_equal(gs, rays, dropped, want, "after the refusals")
    gs.close()


def test_two_runs_agree_bitwise(ctx):
    outs = []
    for _ in range(2):
        gs, rays, dropped = _run(ctx, CASES["random"], W, H)
        outs.append((rays.tobytes(), dropped.tobytes(), _download(gs)[0].tobytes(), _download(gs)[1].tobytes(), api.occupancy_render(ctx, gs, 0, 2).tobytes()))
        gs.close()
    assert outs[0] == outs[1]
