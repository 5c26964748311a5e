"""lsm2d_occupancy_update_scans on the GPU (ABI 0.7.13): every output -- hits, misses, hit rays, clear rays, dropped beams -- is
occupancy_scan_cases.reference's, bit for bit (tests/test_occupancy_scan_abi.py pins that reference), on grids of 1 x 1, 64 x 64, 65 x 63 and 130 x 70
cells.  Scans of 1 .. 2048 beams (65 and 257 make a wave straddle two scans), 1 .. 300 scans to one grid (the rounds of 256 box tests), 1, 3 and 40 grids
with `pose` and `grid` given and NULL, ranges from pageable, pinned and device memory with the handle count balanced, 1081 clear rays of one origin,
accumulation, a clear-only scan over uploaded counters, saturation by clear rays, the composition with lsm2d_preprocess_scans + lsm2d_occupancy_update on
returns-only scans, the parent's call after the new one, the render, every refusal, and two runs that agree bytewise.  Integer sums have no order: there
is no tolerance anywhere."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import occupancy_cases as oc
import occupancy_scan_cases as sc
from gpu_helpers import _aligner
from srrg2_laser_slam_2d_amd import _capi, api, synth

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = sc.W, sc.H
CASES = sc.all_cases()
_REF = {}


def _ref(name, w, h):
    if (name, w, h) not in _REF:
        _REF[(name, w, h)] = sc.reference(CASES[name], w, h)
    return _REF[(name, w, h)]


def _grids(ctx, case, w, h):
    return api.GridSet(ctx, api.GridGeometry(case["origin"][0], case["origin"][1], case["resolution"], w, h), case["n_grids"])


def _download(gs):
    hm = [gs.download(g) for g in range(gs.n_grids)]
    return np.stack([x[0] for x in hm]), np.stack([x[1] for x in hm])


def _run(ctx, case, w, h, gs=None, ranges=None):
    gs = _grids(ctx, case, w, h) if gs is None else gs
    counts = api.occupancy_update_scans(ctx, gs, case["params"], case["ranges"] if ranges is None else ranges, case["poses"], case["grids"])
    return gs, counts


def _assert_equal(gs, counts, want, tag=""):
    wh, wm = want[0], want[1]
    for got, w, what in zip(counts, want[2:], ("hit rays", "clear rays", "dropped")):
        assert got.dtype == np.int32 and got.tolist() == w.tolist(), (tag, what, got.tolist(), w.tolist())
    gh, gm = _download(gs)
    assert gh.dtype == np.uint32 and gh.shape == wh.shape
    assert gh.tobytes() == wh.tobytes(), (tag, "hits", np.argwhere(gh != wh)[:5].tolist())
    assert gm.tobytes() == wm.tobytes(), (tag, "misses", np.argwhere(gm != wm)[:5].tolist())


@pytest.mark.parametrize("size", sc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_the_reference_bit_for_bit(ctx, name, size):
    w, h = size
    gs, counts = _run(ctx, CASES[name], w, h)
    print(name, size, "hit", counts[0].tolist(), "clear", counts[1].tolist(), "dropped", counts[2].tolist(), "kernel ms %.3f" % ctx.last_kernel_ms())
    _assert_equal(gs, counts, _ref(name, w, h), (name, size))
    beams = np.bincount(np.zeros(len(CASES[name]["ranges"]), np.int32) if CASES[name]["grids"] is None else CASES[name]["grids"], minlength=gs.n_grids)
    assert (counts[0] + counts[1] + counts[2]).tolist() == (beams * CASES[name]["params"].n_beams).tolist()
    gs.close()


# ---- a thread per beam over scans of any width, and the tile workgroup's rounds of 256 box tests -------------------------------------------------------------
@pytest.mark.parametrize("n_beams", [1, 63, 64, 65, 257, 1081, 2048])
def test_three_scans_of_n_beams(ctx, n_beams):
    """65 and 257 are no multiple of the wave: a wave holds beams of two scans, which the per-(wave, scan) reduction keeps apart"""
    case = sc.beams_case(n_beams)
    gs, counts = _run(ctx, case, W, H)
    _assert_equal(gs, counts, sc.reference(case, W, H), n_beams)
    assert int(sum(c.sum() for c in counts)) == 3 * n_beams
    gs.close()


@pytest.mark.parametrize("n_scans", [1, 3, 256, 257, 300])
def test_n_scans_to_one_grid(ctx, n_scans):
    """300 scans exceed one round of box tests; 256 fill it exactly"""
    case = sc.many_scans_case(n_scans)
    gs, counts = _run(ctx, case, W, H)
    _assert_equal(gs, counts, sc.reference(case, W, H), n_scans)
    gs.close()


@pytest.mark.parametrize("n_grids", [1, 3, 40])
@pytest.mark.parametrize("given", ["none", "grid", "pose", "all"])
def test_grids_and_optional_arrays(ctx, n_grids, given):
    case = sc.random_case(seed=100 + n_grids, n_scans=max(2 * n_grids, 4), n_beams=50, n_grids=n_grids, poses=given in ("pose", "all"), grids=given in ("grid", "all"))
    assert (case["poses"] is None) == (given in ("none", "grid")) and (case["grids"] is None) == (given in ("none", "pose") or n_grids == 1)
    gs, counts = _run(ctx, case, W, H)
    want = sc.reference(case, W, H)
    _assert_equal(gs, counts, want, (n_grids, given))
    assert want[1].sum() > 0 and (case["grids"] is None or np.count_nonzero(want[2] + want[3]) > 1)
    gs.close()


# ---- where the ranges live -----------------------------------------------------------------------------------------------------------------------------------
def test_pageable_pinned_and_device_ranges_give_the_same_bytes_and_leave_no_handle(ctx):
    import torch
    case = CASES["random"]
    want = _ref("random", W, H)
    live = lambda: ctx.get_option("live_handles")      # noqa: E731  (the process's count, read through the session's context)
    for where in ("pageable", "pinned", "device"):
        src = {"pageable": lambda: case["ranges"], "pinned": lambda: torch.from_numpy(case["ranges"]).pin_memory(),
               "device": lambda: torch.from_numpy(case["ranges"]).to("cuda:0")}[where]()
        before = live()
        own = api.Context(0)
        gs, counts = _run(own, case, W, H, ranges=src)
        moved = own.get_option("last_h2d_bytes")
        assert moved == (0 if where == "device" else case["ranges"].nbytes), (where, moved)
        _assert_equal(gs, counts, want, where)
        assert live() > before
        gs.close(); own.close()
        assert live() == before, (where, before, live())      # create -> call -> destroy: the call owns nothing outside the context


def test_contention_1081_clear_rays_of_one_origin(ctx):
    case = sc.fan_case(1081)
    gs, counts = _run(ctx, case, W, H)
    want = sc.reference(case, W, H)
    _assert_equal(gs, counts, want, "fan")
    assert counts[0].tolist() == [0] and counts[1][0] + counts[2][0] == 1081 and counts[1][0] > 1000
    h, m = gs.download(0)
    assert m[31, 33] == counts[1][0] and not h.any()      # the origin cell's misses: EVERY live ray, for a clear ray's every step is a miss
    gs.close()


# ---- accumulation and storage --------------------------------------------------------------------------------------------------------------------------------
def test_two_calls_equal_one_call_with_both_scans(ctx):
    a = sc.random_case(seed=41, n_scans=3, n_beams=129, n_grids=2)
    b = sc.random_case(seed=42, n_scans=4, n_beams=129, n_grids=2)
    both = sc._case(a["params"], np.concatenate([a["ranges"], b["ranges"]]), np.concatenate([a["poses"], b["poses"]]), np.concatenate([a["grids"], b["grids"]]), 2,
                    a["origin"], a["resolution"])
    one, c1 = _run(ctx, both, W, H)
    two, ca = _run(ctx, a, W, H)
    _, cb = _run(ctx, b, W, H, two)
    for x, y, z in zip(c1, ca, cb):
        assert x.tolist() == (y + z).tolist()
    h1, m1 = _download(one); h2, m2 = _download(two)
    assert h1.tobytes() == h2.tobytes() and m1.tobytes() == m2.tobytes() and h1.sum() > 0
    _assert_equal(two, c1, sc.reference(both, W, H), "both")
    one.close(); two.close()


def test_clear_only_scan_leaves_uploaded_hits_byte_identical(ctx):
    rng = np.random.default_rng(5)
    case = CASES["clear_only"]
    gs = _grids(ctx, case, W, H)
    hits = rng.integers(0, 1 << 32, (2, H, W), dtype=np.uint64).astype(np.uint32); misses = rng.integers(0, 1 << 20, (2, H, W)).astype(np.uint32)
    for g in range(2):
        gs.upload(g, hits[g], misses[g])
    _, counts = _run(ctx, case, W, H, gs)
    gh, gm = _download(gs)
    assert gh.tobytes() == hits.tobytes() and counts[0].tolist() == [0, 0]
    _assert_equal(gs, counts, sc.reference(case, W, H, hits, misses), "over uploaded counters")
    assert (gm != misses).sum() > 100
    gs.close()


def test_misses_saturate_by_clear_rays(ctx):
    """cells uploaded at 2^32 - 2 and crossed by three clear rays read 2^32 - 1, their ends too; the hits, at 2^32 - 2, stay"""
    prm = sc.four_beams(0.25, 60.0, 4.0, True)
    case = sc._case(prm, [[sc.NAN, sc.NAN, sc.INF, sc.NAN]] * 3, poses=[sc._sensor(1, 3), sc._sensor(1, 3), sc._sensor(2, 3)])
    start = np.full((8, 12), 0xFFFFFFFE, np.uint32)
    gs = _grids(ctx, case, 12, 8)
    gs.upload(0, start, start)
    _, counts = _run(ctx, case, 12, 8, gs)
    _assert_equal(gs, counts, sc.reference(case, 12, 8, start[None], start[None]), "saturation")
    gh, gm = gs.download(0)
    assert counts[1].tolist() == [3] and gm[3, 1] == 0xFFFFFFFF and gm[3, 2] == 0xFFFFFFFF and gm[3, 9] == 0xFFFFFFFF and gm[3, 10] == 0xFFFFFFFF
    assert gm[3, 11] == 0xFFFFFFFE and gm[2, 5] == 0xFFFFFFFE and (gh == 0xFFFFFFFE).all()
    gs.close()


# ---- composition with what the parent has --------------------------------------------------------------------------------------------------------------------
def test_returns_only_scans_equal_preprocess_scans_then_occupancy_update(ctx):
    """class-1/2-only scans, trace_range == range_max: the preprocessor at normal_min_points 1, resolution 0 (and a normal window that is the whole scan: it
    drops a beam whose window has no direction) keeps every valid beam, and the parent's two calls trace the same rays"""
    case = CASES["returns_only"]
    prm = case["params"]
    one, counts = _run(ctx, case, 200, 120)
    pre = api.RawDataPreprocessorProjective2D(ctx, range_min=prm.range_min, range_max=prm.range_max, voxelize_resolution=0.0, normal_point_distance=sc.WHOLE_SCAN,
                                              normal_min_points=1)
    pre.setRawData(case["ranges"], prm.angle_min, prm.angle_max, 0.0, float("inf"))
    clouds = pre.compute()
    two = _grids(ctx, case, 200, 120)
    rays, dropped = api.occupancy_update(ctx, two, clouds, None, case["poses"], None)
    h1, m1 = _download(one); h2, m2 = _download(two)
    assert h1.tobytes() == h2.tobytes() and m1.tobytes() == m2.tobytes() and h1.sum() > 1000
    assert counts[0].tolist() == rays.tolist() and counts[1].tolist() == [0] and dropped.tolist() == [0]
    assert counts[0][0] + counts[2][0] == case["ranges"].size and counts[2][0] > 0
    _assert_equal(one, counts, sc.reference(case, 200, 120), "returns only")
    one.close(); two.close()


def test_the_cloud_call_is_unchanged_after_the_scan_call(ctx):
    gs, _ = _run(ctx, CASES["random"], W, H)      # the new call has run in this process, on this context
    gs.close()
    cases = oc.all_cases()
    for name in ("borders", "random", "empty_and_dropped"):
        case = cases[name]
        offs = np.zeros(len(case["clouds"]) + 1, np.int32); offs[1:] = np.cumsum([len(c) for c in case["clouds"]])
        src = api.CloudSet(ctx, np.ascontiguousarray(np.concatenate(case["clouds"]), F32).reshape(-1, 4), offs)
        g2 = api.GridSet(ctx, api.GridGeometry(case["origin"][0], case["origin"][1], case["resolution"], W, H), case["n_grids"])
        rays, dropped = api.occupancy_update(ctx, g2, src, None, case["poses"], case["grids"])
        wh, wm, wr, wd = oc.reference(case, W, H)
        gh, gm = _download(g2)
        assert rays.tolist() == wr.tolist() and dropped.tolist() == wd.tolist() and gh.tobytes() == wh.tobytes() and gm.tobytes() == wm.tobytes(), name
        g2.close()


def test_render_after_a_mixed_scan_is_occupancy_values_of_the_references_counters(ctx):
    gs, _ = _run(ctx, CASES["random"], W, H)
    wh, wm = _ref("random", W, H)[:2]
    for g in range(2):
        for min_visits in (1, 3):
            got = api.occupancy_render(ctx, gs, g, min_visits)
            want = api.occupancy_values(wh[g], wm[g], min_visits)
            assert got.tobytes() == want.tobytes(), (g, min_visits)
            assert (got == 0).sum() > 100 and (got > 0).sum() > 10 and (got == -1).sum() > 10
    gs.close()


def test_workgroup_stamps_work_for_the_scan_call(ctx):
    assert ctx.kernel_timing      # (the Python context turns it on)
    gs, _ = _run(ctx, CASES["random"], W, H)
    med, top = ctx.get_option("last_occupancy_wg_median_ns"), ctx.get_option("last_occupancy_wg_max_ns")
    assert 0 < med <= top and ctx.last_kernel_ms() > 0.0
    gs.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_change_nothing(ctx):
    import torch
    lib = _capi.load()
    BAD, CAPACITY = _capi.BAD_ARGUMENT, _capi.CAPACITY_EXCEEDED
    case = sc.random_case(seed=31, n_scans=4, n_beams=83, n_grids=2)
    gs, _ = _run(ctx, case, W, H)
    before = _download(gs)
    sentinel = np.full(2, -77, np.int32)
    nan, inf = float("nan"), float("inf")

    def refused(code=BAD, no_ctx=False, no_params=False, **kw):
        a = dict(gs=gs, params=case["params"], ranges=case["ranges"], n_scans=4, pose=case["poses"], grid=case["grids"])
        a.update(kw)
        outs = [sentinel.copy() for _ in range(3)]
        uploads = ctx.get_option("uploads")
        p = a["params"].struct()
        gr = None if a["grid"] is None else np.ascontiguousarray(a["grid"], np.int32)
        ps = None if a["pose"] is None else np.ascontiguousarray(a["pose"], F32)
        got = lib.lsm2d_occupancy_update_scans(None if no_ctx else ctx.handle, None if a["gs"] is None else a["gs"].handle, None if no_params else C.byref(p),
                                               api._ptr(a["ranges"]), a["n_scans"], api._ptr(ps), api._ptr(gr), *(api._ptr(o) for o in outs))
        assert got == code, (kw, got)
        assert all(o.tolist() == sentinel.tolist() for o in outs) and ctx.get_option("uploads") == uploads, kw
        dh, dm = _download(gs)      # nothing was written: the counters downloaded after EVERY refusal are the ones from before
        assert dh.tobytes() == before[0].tobytes() and dm.tobytes() == before[1].tobytes(), kw

    with_ = lambda **kw: dataclasses.replace(case["params"], **kw)      # noqa: E731
    refused(no_ctx=True); refused(gs=None); refused(no_params=True); refused(ranges=None)      # a NULL the call needs
    refused(n_scans=0); refused(n_scans=-1)
    big = _capi.OCCUPANCY_MAX_RAYS // 83 + 1      # n_scans * n_beams above the limit (refused before the ranges are read)
    refused(n_scans=big, pose=None, grid=None)
    refused(code=CAPACITY, params=with_(n_beams=0)); refused(code=CAPACITY, params=with_(n_beams=2049)); refused(code=CAPACITY, params=with_(n_beams=-5))
    refused(params=with_(angle_max=case["params"].angle_min)); refused(params=with_(angle_min=1.0, angle_max=-1.0)); refused(params=with_(angle_max=nan))
    for field in ("range_min", "range_max", "trace_range"):
        for v in (nan, inf, -inf):
            refused(params=with_(**{field: v}))
    refused(params=with_(range_min=-0.5)); refused(params=with_(range_min=13.0))                      # range_min < 0, range_min > range_max
    refused(params=with_(trace_range=0.0)); refused(params=with_(trace_range=-1.0))                   # !(trace_range > 0)
    refused(params=with_(trace_range=0.2)); refused(params=with_(trace_range=12.5))                   # trace_range < range_min, > range_max
    p = case["params"].struct()
    for v in (2, -1):      # clear_no_return outside {0, 1}
        p.clear_no_return = v
        outs = [sentinel.copy() for _ in range(3)]
        assert lib.lsm2d_occupancy_update_scans(ctx.handle, gs.handle, C.byref(p), api._ptr(case["ranges"]), 4, api._ptr(case["poses"]), api._ptr(case["grids"]),
                                                *(api._ptr(o) for o in outs)) == BAD
        assert all(o.tolist() == sentinel.tolist() for o in outs)
    refused(grid=[0, 1, 2, 0]); refused(grid=[0, -1, 1, 0])
    ctx2 = api.Context(0)      # a set of another context, and one whose context is gone (made through the bare ABI: the Python context closes its own sets)
    orphan = C.c_void_p()
    try:
        refused(gs=api.GridSet(ctx2, gs.geometry, 2))
        geo = gs.geometry.struct()
        assert lib.lsm2d_gridset_create(ctx2.handle, C.byref(geo), 2, C.byref(orphan)) == 0
    finally:
        ctx2.close()
    try:
        refused(gs=type("Orphan", (), {"handle": orphan})())
    finally:
        lib.lsm2d_gridset_destroy(orphan)
    if torch.cuda.device_count() > 1:      # device-resident ranges on another device
        refused(ranges=torch.from_numpy(case["ranges"]).to("cuda:1"))
    # two batches in flight
    wl = synth.make_workload(16, 4000, seed=3)
    al = _aligner(ctx)
    fx = [api.CloudSet(ctx, wl.scan_points[:wl.scan_offsets[8]], wl.scan_offsets[:9])]; mv = [api.CloudSet(ctx, wl.map_points)]
    p1 = al.prepare_batch(fx, mv, wl.x0[:8]); p2 = al.prepare_batch(fx, mv, wl.x0[:8])
    p1.begin(); p2.begin()
    try:
        outs = [sentinel.copy() for _ in range(3)]
        p = case["params"].struct()
        assert lib.lsm2d_occupancy_update_scans(ctx.handle, gs.handle, C.byref(p), api._ptr(case["ranges"]), 4, api._ptr(case["poses"]), api._ptr(case["grids"]),
                                                *(api._ptr(o) for o in outs)) == BAD
        assert all(o.tolist() == sentinel.tolist() for o in outs)
    finally:
        p1.wait(); p2.wait()
    after = _download(gs)
    assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes()
    # the context is usable and the call still right
    _, counts = _run(ctx, case, W, H, gs)
    _assert_equal(gs, counts, sc.reference(case, W, H, *before), "after the refusals")
    gs.close()


def test_two_runs_agree_bitwise(ctx):
    outs = []
    for _ in range(2):
        gs, counts = _run(ctx, CASES["random"], W, H)
        outs.append((tuple(c.tobytes() for c in counts), _download(gs)[0].tobytes(), _download(gs)[1].tobytes(), api.occupancy_render(ctx, gs, 0, 2).tobytes()))
        gs.close()
    assert outs[0] == outs[1]
