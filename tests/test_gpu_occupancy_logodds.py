"""Log-odds grid sets on the GPU (ABI 0.7.14): value and observed after lsm2d_occupancy_update_scans and lsm2d_occupancy_update into a log-odds set are
occupancy_logodds_cases.reference's, bit for bit, with no tolerance and nothing excluded (tests/test_occupancy_logodds_abi.py pins that reference), on grids
of 1 x 1, 64 x 64, 65 x 63 and 130 x 70 cells.  A known answer that needs no restatement (one scan n times), the ORDER of the scans (256 and 300 alternating
scans to one tile, reversed, with every third scan's box missing the tile), 1 / 3 / 40 grids with the optional arrays, where the ranges live, 1 .. 2048 beams,
rays ending either side of the tile edge, accumulation, set_logodds between calls, a counts set beside a log-odds set, decay, render, upload / download,
clear, the workgroup stamps, the handle count, every refusal, two runs, and clouds made by lsm2d_preprocess_scans through the cloud call."""
import ctypes as C

import numpy as np
import pytest

import occupancy_cases as oc
import occupancy_logodds_cases as lc
import occupancy_scan_cases as sc
from srrg2_laser_slam_2d_amd import _capi, api

pytestmark = pytest.mark.gpu
F32 = np.float32
W, H = lc.W, lc.H
P = lc.PARAMS
SCAN_CASES = lc.scan_cases()
CLOUD_CASES = lc.cloud_cases()
_REF = {}


def _ref(kind, name, w, h):
    if (kind, name, w, h) not in _REF:
        _REF[(kind, name, w, h)] = lc.reference((SCAN_CASES if kind == "scan" else CLOUD_CASES)[name], w, h)
    return _REF[(kind, name, w, h)]


def _grids(ctx, case, w, h, params=P):
    return api.GridSet(ctx, api.GridGeometry(case["origin"][0], case["origin"][1], case["resolution"], w, h), case["n_grids"], params)


def _download(gs):
    vo = [gs.download_logodds(g) for g in range(gs.n_grids)]
    return np.stack([x[0] for x in vo]), np.stack([x[1] for x in vo])


def _cloudset(ctx, case):
    offs = np.zeros(len(case["clouds"]) + 1, np.int32); offs[1:] = np.cumsum([len(c) for c in case["clouds"]])
    return api.CloudSet(ctx, np.ascontiguousarray(np.concatenate(case["clouds"]), F32).reshape(-1, 4), offs)


def _run(ctx, case, w, h, gs=None, params=P, ranges=None):
    """a case of either call into a log-odds set: -> (set, the call's counts)"""
    gs = _grids(ctx, case, w, h, params) if gs is None else gs
    if lc.is_scan_case(case):
        return gs, api.occupancy_update_scans(ctx, gs, case["params"], case["ranges"] if ranges is None else ranges, case["poses"], case["grids"])
    src = _cloudset(ctx, case)
    counts = api.occupancy_update(ctx, gs, src, None, case["poses"], case["grids"])
    src.close()
    return gs, counts


def _assert_cells(gs, want, tag=""):
    gv, go = _download(gs)
    assert gv.dtype == np.int32 and go.dtype == np.uint32 and gv.shape == want[0].shape
    assert gv.tobytes() == want[0].tobytes(), (tag, "value", np.argwhere(gv != want[0])[:5].tolist())
    assert go.tobytes() == want[1].tobytes(), (tag, "observed", np.argwhere(go != want[1])[:5].tolist())


# ---- every case through both update calls ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", lc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(SCAN_CASES))
def test_scan_case_is_the_reference_bit_for_bit(ctx, name, size):
    w, h = size
    case = SCAN_CASES[name]
    gs, counts = _run(ctx, case, w, h)
    _assert_cells(gs, _ref("scan", name, w, h), (name, size))
    want = sc.reference(case, w, h)[2:]      # the counts keep their meaning: rays, not votes
    assert [c.tolist() for c in counts] == [c.tolist() for c in want], (name, size)
    gs.close()


@pytest.mark.parametrize("size", lc.SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(CLOUD_CASES))
def test_cloud_case_is_the_reference_bit_for_bit(ctx, name, size):
    w, h = size
    case = CLOUD_CASES[name]
    gs, counts = _run(ctx, case, w, h)
    _assert_cells(gs, _ref("cloud", name, w, h), (name, size))
    want = oc.reference(case, w, h)[2:]
    assert [c.tolist() for c in counts] == [c.tolist() for c in want], (name, size)
    gs.close()


@pytest.mark.parametrize("name", ["returns_only", "random", "classes_clear", "fan_with_returns"])
def test_clouds_made_by_preprocess_scans_through_the_cloud_call(ctx, name):
    """the scans' returns as lsm2d_preprocess_scans makes them (normal_min_points 1, resolution 0, the full-scan normal window: every valid beam kept), a
    cloud per scan, through lsm2d_occupancy_update: the restatement over the rays of the clouds as downloaded"""
    case = SCAN_CASES[name]
    prm = case["params"]
    pre = api.RawDataPreprocessorProjective2D(ctx, range_min=prm.range_min, range_max=prm.range_max, voxelize_resolution=0.0, normal_point_distance=sc.WHOLE_SCAN,
                                              normal_min_points=1)
    pre.setRawData(case["ranges"], prm.angle_min, prm.angle_max, 0.0, float("inf"))
    clouds = pre.compute()
    assert clouds.n_clouds == len(case["ranges"])
    as_clouds = oc._case([clouds.download(k) for k in range(clouds.n_clouds)], case["poses"], case["grids"], case["n_grids"], case["origin"], case["resolution"])
    assert sum(len(c) for c in as_clouds["clouds"]) > 10
    gs = _grids(ctx, case, W, H)
    rays, dropped = api.occupancy_update(ctx, gs, clouds, None, case["poses"], case["grids"])
    _assert_cells(gs, lc.reference(as_clouds, W, H), name)
    assert rays.sum() + dropped.sum() == sum(len(c) for c in as_clouds["clouds"])
    if name == "returns_only":      # trace_range == range_max and no beam without a return: the scan call votes the same
        _assert_cells(gs, _ref("scan", name, W, H), "the scan call's")
    gs.close(); clouds.close()


# ---- a known answer that needs no restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 40])
def test_one_scan_n_times_in_one_list(ctx, n):
    base = lc.fan_with_returns_case()
    cs, (ch, cm) = _run_counts(ctx, base)
    hit, miss = ch > 0, (cm > 0) & ~(ch > 0)      # H and M of the scan, from a COUNTS set on the device (held to its reference elsewhere)
    assert hit.sum() > 100 and miss.sum() > 500
    gs, counts = _run(ctx, lc.repeat_case(n, base), W, H)
    v, o = gs.download_logodds(0)
    assert (v[hit] == min(n * P.l_hit, P.l_max)).all(), np.unique(v[hit]).tolist()
    assert (v[miss] == max(n * P.l_miss, P.l_min)).all(), np.unique(v[miss]).tolist()
    assert (o[hit | miss] == n).all() and not v[~(hit | miss)].any() and not o[~(hit | miss)].any()
    assert int(sum(c.sum() for c in counts)) == n * 1081
    gs.close(); cs.close()


def _run_counts(ctx, case, w=W, h=H):
    cs = api.GridSet(ctx, api.GridGeometry(case["origin"][0], case["origin"][1], case["resolution"], w, h), case["n_grids"])
    api.occupancy_update_scans(ctx, cs, case["params"], case["ranges"], case["poses"], case["grids"])
    return cs, cs.download(0)


# ---- the order of the scans ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("far_every_third", [False, True], ids=["all", "far_every_third"])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("n", [256, 300])
def test_the_last_scan_decides(ctx, n, reverse, far_every_third):
    """l_max = l_hit and l_min = l_miss: the cell's value says which scan came last (300 scans make a second round of box tests)"""
    p = lc.ORDER_PARAMS
    case = lc.order_case(n, reverse, far_every_third)
    gs, _ = _run(ctx, case, 64, 64, params=p)
    _assert_cells(gs, lc.reference(case, 64, 64, p), (n, reverse, far_every_third))
    x, y = lc.HIT_CELL
    v, o = gs.download_logodds(0)
    if not far_every_third:
        assert v[y, x] == (p.l_hit if reverse else p.l_hit + p.l_miss) and o[y, x] == n      # forward the list ends with a clearing scan, reversed with a hit
    else:
        assert o[y, x] == n - n // 3
    gs.close()


# ---- grids, optional arrays, where the ranges live, beams ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_grids", [1, 3, 40])
@pytest.mark.parametrize("given", ["none", "grid", "pose", "all"])
def test_grids_and_optional_arrays(ctx, n_grids, given):
    case = sc.random_case(seed=100 + n_grids, n_scans=max(2 * n_grids, 4), n_beams=50, n_grids=n_grids, poses=given in ("pose", "all"), grids=given in ("grid", "all"))
    gs, counts = _run(ctx, case, W, H)
    want = lc.reference(case, W, H)
    _assert_cells(gs, want, (n_grids, given))
    assert want[1].sum() > 0 and (case["grids"] is None or np.count_nonzero(want[1].reshape(n_grids, -1).sum(1)) > 1)
    gs.close()


def test_pageable_pinned_and_device_ranges_give_the_same_bytes_and_leave_no_handle(ctx):
    import torch
    case = SCAN_CASES["random"]
    want = _ref("scan", "random", W, H)
    live = lambda: ctx.get_option("live_handles")      # noqa: E731
    for where in ("pageable", "pinned", "device"):
        src = {"pageable": lambda: case["ranges"], "pinned": lambda: torch.from_numpy(case["ranges"]).pin_memory(),
               "device": lambda: torch.from_numpy(case["ranges"]).to("cuda:0")}[where]()
        before = live()
        own = api.Context(0)
        gs, _ = _run(own, case, W, H, ranges=src)
        _assert_cells(gs, want, where)
        gs.decay(10); api.occupancy_render_logodds(own, gs, 0, lc.UNIT)
        assert live() > before
        gs.close(); own.close()
        assert live() == before, (where, before, live())      # "live_handles" balanced: the new calls own nothing outside the context


@pytest.mark.parametrize("n_beams", [1, 63, 64, 65, 257, 1081, 2048])
def test_three_scans_of_n_beams(ctx, n_beams):
    case = sc.beams_case(n_beams)
    gs, counts = _run(ctx, case, W, H)
    _assert_cells(gs, lc.reference(case, W, H), n_beams)
    assert int(sum(c.sum() for c in counts)) == 3 * n_beams
    gs.close()


def test_rays_ending_on_cell_63_and_on_cell_64(ctx):
    gs, _ = _run(ctx, SCAN_CASES["edge"], W, H)
    v, o = gs.download_logodds(0)
    for x, y in ((63, 10), (64, 12), (5, 63), (6, 64)):
        assert v[y, x] == P.l_hit and o[y, x] == 1, (x, y)
    assert v[10, 64] == 0 and v[12, 65] == 0 and v[10, 62] == P.l_miss and v[12, 63] == P.l_miss and v[62, 5] == P.l_miss and v[63, 6] == P.l_miss
    _assert_cells(gs, _ref("scan", "edge", W, H), "edge")
    gs.close()


# ---- accumulation, parameters, the old path ----------------------------------------------------------------------------------------------------------------------
def test_two_calls_equal_one_call_and_set_logodds_between_calls(ctx):
    a = sc.random_case(seed=41, n_scans=3, n_beams=129, n_grids=2)
    b = sc.random_case(seed=42, n_scans=4, n_beams=129, n_grids=2)
    both = sc._case(a["params"], np.concatenate([a["ranges"], b["ranges"]]), np.concatenate([a["poses"], b["poses"]]), np.concatenate([a["grids"], b["grids"]]), 2,
                    a["origin"], a["resolution"])
    tight = api.LogOddsParams(100, -100, -150, 150)      # clamps that are met: the order of the scans matters
    one, _ = _run(ctx, both, W, H, params=tight)
    two, _ = _run(ctx, a, W, H, params=tight)
    _run(ctx, b, W, H, two)
    want = lc.reference(both, W, H, tight)
    _assert_cells(one, want, "one call"); _assert_cells(two, want, "two calls")
    assert (np.abs(want[0]) == 150).sum() > 10
    # other parameters for the second call
    other = api.LogOddsParams(7, -300, -1000, 20)
    three, _ = _run(ctx, a, W, H, params=tight)
    three.set_logodds(other)
    _run(ctx, b, W, H, three)
    va, oa = lc.reference(a, W, H, tight)
    _assert_cells(three, lc.reference(b, W, H, other, va, oa), "set_logodds between calls")
    for gs in (one, two, three):
        gs.close()


def test_a_counts_set_beside_a_logodds_set_is_byte_identical_to_its_reference(ctx):
    """the same scans into both kinds of set in one process, the log-odds call first and last: the old path is untouched"""
    case = SCAN_CASES["random"]
    lo, _ = _run(ctx, case, W, H)
    cs = api.GridSet(ctx, api.GridGeometry(case["origin"][0], case["origin"][1], case["resolution"], W, H), case["n_grids"])
    counts = api.occupancy_update_scans(ctx, cs, case["params"], case["ranges"], case["poses"], case["grids"])
    _run(ctx, case, W, H, lo)
    wh, wm, n_hit, n_clear, n_drop = sc.reference(case, W, H)
    for g in range(case["n_grids"]):
        gh, gm = cs.download(g)
        assert gh.tobytes() == wh[g].tobytes() and gm.tobytes() == wm[g].tobytes(), g
        assert api.occupancy_render(ctx, cs, g, 1).tobytes() == api.occupancy_values(wh[g], wm[g], 1).tobytes()
    assert [c.tolist() for c in counts] == [n_hit.tolist(), n_clear.tolist(), n_drop.tolist()]
    cloud = CLOUD_CASES["random"]
    cc = api.GridSet(ctx, api.GridGeometry(cloud["origin"][0], cloud["origin"][1], cloud["resolution"], W, H), cloud["n_grids"])
    src = _cloudset(ctx, cloud)
    api.occupancy_update(ctx, cc, src, None, cloud["poses"], cloud["grids"])
    ch, cm = oc.reference(cloud, W, H)[:2]
    for g in range(cloud["n_grids"]):
        gh, gm = cc.download(g)
        assert gh.tobytes() == ch[g].tobytes() and gm.tobytes() == cm[g].tobytes(), g
    v, o = lc.reference(case, W, H)
    _assert_cells(lo, lc.reference(case, W, H, P, v, o), "twice")
    for s in (lo, cs, cc, src):
        s.close()


# ---- clamps, uploads, saturation ---------------------------------------------------------------------------------------------------------------------------------
def test_clamps_uploaded_values_and_saturation(ctx):
    value, observed, checks, hit, miss = lc.stress_start()
    case = lc.fan_with_returns_case()
    gs = _grids(ctx, case, W, H)
    gs.upload_logodds(0, value, observed)
    v0, o0 = gs.download_logodds(0)
    assert v0.tobytes() == value.tobytes() and o0.tobytes() == observed.tobytes()      # the round trip, INT32_MIN .. INT32_MAX and 0 .. 2^32 - 1
    _run(ctx, case, W, H, gs)
    v, o = gs.download_logodds(0)
    for what, (y, x), want_v, want_o in checks:
        assert v[y, x] == want_v and o[y, x] == want_o, (what, int(v[y, x]), want_v, int(o[y, x]), want_o)
    _assert_cells(gs, lc.reference(case, W, H, P, value[None], observed[None]), "over uploaded cells")
    rest = ~(hit | miss)
    assert (v[rest] == value[rest]).all() and (o[rest] == observed[rest]).all()
    # one array at a time: the other word stays
    gs.upload_logodds(0, value=np.full((H, W), 7, np.int32))
    v1, o1 = gs.download_logodds(0)
    assert (v1 == 7).all() and o1.tobytes() == o.tobytes()
    gs.upload_logodds(0, observed=np.full((H, W), 9, np.uint32))
    v2, o2 = gs.download_logodds(0)
    assert (v2 == 7).all() and (o2 == 9).all()
    gs.close()


# ---- decay, render, clear ----------------------------------------------------------------------------------------------------------------------------------------
def test_decay_render_and_clear(ctx):
    case = SCAN_CASES["random"]
    gs, _ = _run(ctx, case, W, H)
    _run(ctx, case, W, H, gs)
    v, o = lc.reference(case, W, H, P, *_ref("scan", "random", W, H))
    for unit in (lc.UNIT, 0.125):
        for min_scans in (0, 1, 3):
            for g in range(2):
                got = api.occupancy_render_logodds(ctx, gs, g, unit, min_scans)
                assert got.dtype == np.int8 and got.tobytes() == api.logodds_values(v[g], o[g], unit, min_scans).tobytes(), (unit, min_scans, g)
    got = api.occupancy_render_logodds(ctx, gs, 0, lc.UNIT, 1)
    assert (got == -1).sum() > 10 and (got > 50).sum() > 10 and ((got >= 0) & (got < 50)).sum() > 100 and ctx.last_kernel_ms() > 0.0
    gs.decay(0)
    _assert_cells(gs, (v, o), "amount 0")
    gs.decay(30, [1])      # one grid
    v[1] = lc.decay(v[1], o[1], 30)
    _assert_cells(gs, (v, o), "one grid")
    gs.decay(55)           # every grid; past zero for the cells within 55 of it
    v = lc.decay(v, o, 55)
    _assert_cells(gs, (v, o), "every grid")
    assert (v > 0).any() and (v < 0).any() and ((v == 0) & (o > 0)).any()
    gs.decay(2 ** 31 - 1)
    _assert_cells(gs, (np.zeros_like(v), o), "all the way")
    # unknown cells with a value (uploaded) do not decay; observed ones do, from INT32_MIN and INT32_MAX too
    val = np.full((H, W), -9, np.int32); val[0, 0] = lc.I32_MAX; val[0, 1] = lc.I32_MIN
    obs = np.zeros((H, W), np.uint32); obs[0, :4] = 1
    gs.upload_logodds(0, val, obs)
    gs.decay(5)
    v0, o0 = gs.download_logodds(0)
    assert v0.tobytes() == lc.decay(val, obs, 5).tobytes() and o0.tobytes() == obs.tobytes() and v0[0, 0] == lc.I32_MAX - 5 and v0[0, 1] == lc.I32_MIN + 5 and v0[1, 1] == -9
    gs.clear([0])
    v0, o0 = gs.download_logodds(0)
    v1, o1 = gs.download_logodds(1)
    assert not v0.any() and not o0.any() and o1.tobytes() == o[1].tobytes()
    gs.clear()
    assert not gs.download_logodds(1)[1].any()
    _run(ctx, case, W, H, gs)
    _assert_cells(gs, _ref("scan", "random", W, H), "after a clear")
    gs.close()


def test_workgroup_stamps_with_kernel_timing_on(ctx):
    assert ctx.kernel_timing
    gs, _ = _run(ctx, SCAN_CASES["random"], W, H)
    med, top = ctx.get_option("last_occupancy_wg_median_ns"), ctx.get_option("last_occupancy_wg_max_ns")
    assert 0 < med <= top and ctx.last_kernel_ms() > 0.0
    gs.close()
    gs, _ = _run(ctx, CLOUD_CASES["random"], W, H)
    med, top = ctx.get_option("last_occupancy_wg_median_ns"), ctx.get_option("last_occupancy_wg_max_ns")
    assert 0 < med <= top and ctx.last_kernel_ms() > 0.0
    gs.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing_and_change_nothing(ctx):
    lib = _capi.load()
    BAD = _capi.BAD_ARGUMENT
    case = SCAN_CASES["random"]
    lo, _ = _run(ctx, case, W, H)
    cs = api.GridSet(ctx, lo.geometry, 2)
    api.occupancy_update_scans(ctx, cs, case["params"], case["ranges"], case["poses"], case["grids"])
    before_lo, before_cs = _download(lo), [cs.download(g) for g in range(2)]

    def unchanged(what):
        v, o = _download(lo)
        assert v.tobytes() == before_lo[0].tobytes() and o.tobytes() == before_lo[1].tobytes(), what
        for g in range(2):
            h, m = cs.download(g)
            assert h.tobytes() == before_cs[g][0].tobytes() and m.tobytes() == before_cs[g][1].tobytes(), what

    def refused(what, code):
        assert code == BAD, (what, code)
        unchanged(what)

    geo = lo.geometry.struct()
    good = P.struct()
    # a parameter outside the constraints, at create and at set
    for field, bad in (("l_hit", 0), ("l_hit", -1), ("l_hit", (1 << 20) + 1), ("l_miss", 0), ("l_miss", 1), ("l_miss", -(1 << 20) - 1), ("l_min", 1),
                       ("l_min", -(1 << 30) - 1), ("l_max", -1), ("l_max", (1 << 30) + 1)):
        p = P.struct(); setattr(p, field, bad)
        out = C.c_void_p(0x1234)
        refused((field, bad, "create"), lib.lsm2d_gridset_create_logodds(ctx.handle, C.byref(geo), 2, C.byref(p), C.byref(out)))
        assert out.value is None      # (*out is NULL after a refusal)
        refused((field, bad, "set"), lib.lsm2d_gridset_set_logodds(lo.handle, C.byref(p)))
    for field, ok in (("l_hit", 1), ("l_hit", 1 << 20), ("l_miss", -1), ("l_miss", -(1 << 20)), ("l_min", 0), ("l_min", -(1 << 30)), ("l_max", 0), ("l_max", 1 << 30)):
        p = P.struct(); setattr(p, field, ok)
        assert lib.lsm2d_gridset_set_logodds(lo.handle, C.byref(p)) == 0, (field, ok)      # the ends of the constraints are inside
    assert lib.lsm2d_gridset_set_logodds(lo.handle, C.byref(good)) == 0
    # a NULL the call needs
    out = C.c_void_p()
    refused("create: no ctx", lib.lsm2d_gridset_create_logodds(None, C.byref(geo), 2, C.byref(good), C.byref(out)))
    refused("create: no geometry", lib.lsm2d_gridset_create_logodds(ctx.handle, None, 2, C.byref(good), C.byref(out)))
    refused("create: no params", lib.lsm2d_gridset_create_logodds(ctx.handle, C.byref(geo), 2, None, C.byref(out)))
    refused("create: no out", lib.lsm2d_gridset_create_logodds(ctx.handle, C.byref(geo), 2, C.byref(good), None))
    refused("create: n_grids 0", lib.lsm2d_gridset_create_logodds(ctx.handle, C.byref(geo), 0, C.byref(good), C.byref(out)))
    refused("set: no set", lib.lsm2d_gridset_set_logodds(None, C.byref(good)))
    refused("set: no params", lib.lsm2d_gridset_set_logodds(lo.handle, None))
    val = np.zeros((H, W), np.int32); obs = np.zeros((H, W), np.uint32); img = np.full((H, W), 77, np.int8)
    rp = _capi.LogOddsRenderParamsC(1, lc.UNIT)
    refused("upload: no set", lib.lsm2d_gridset_upload_logodds(None, 0, api._ptr(val), api._ptr(obs)))
    refused("download: no set", lib.lsm2d_gridset_download_logodds(None, 0, api._ptr(val), api._ptr(obs)))
    refused("decay: no ctx", lib.lsm2d_occupancy_decay(None, lo.handle, 0, None, 1))
    refused("decay: no set", lib.lsm2d_occupancy_decay(ctx.handle, None, 0, None, 1))
    refused("render: no ctx", lib.lsm2d_occupancy_render_logodds(None, lo.handle, 0, C.byref(rp), api._ptr(img)))
    refused("render: no set", lib.lsm2d_occupancy_render_logodds(ctx.handle, None, 0, C.byref(rp), api._ptr(img)))
    refused("render: no params", lib.lsm2d_occupancy_render_logodds(ctx.handle, lo.handle, 0, None, api._ptr(img)))
    refused("render: no out", lib.lsm2d_occupancy_render_logodds(ctx.handle, lo.handle, 0, C.byref(rp), None))
    # the wrong kind of set
    refused("set on counts", lib.lsm2d_gridset_set_logodds(cs.handle, C.byref(good)))
    refused("upload_logodds on counts", lib.lsm2d_gridset_upload_logodds(cs.handle, 0, api._ptr(val), api._ptr(obs)))
    refused("download_logodds on counts", lib.lsm2d_gridset_download_logodds(cs.handle, 0, api._ptr(val), api._ptr(obs)))
    refused("decay on counts", lib.lsm2d_occupancy_decay(ctx.handle, cs.handle, 0, None, 1))
    refused("render_logodds on counts", lib.lsm2d_occupancy_render_logodds(ctx.handle, cs.handle, 0, C.byref(rp), api._ptr(img)))
    cnt = np.zeros((H, W), np.uint32)
    refused("upload on log-odds", lib.lsm2d_gridset_upload(lo.handle, 0, api._ptr(cnt), api._ptr(cnt)))
    refused("download on log-odds", lib.lsm2d_gridset_download(lo.handle, 0, api._ptr(cnt), api._ptr(cnt)))
    crp = _capi.OccupancyRenderParamsC(1)
    refused("render on log-odds", lib.lsm2d_occupancy_render(ctx.handle, lo.handle, 0, C.byref(crp), api._ptr(img)))
    assert (img == 77).all() and not val.any() and not cnt.any()      # nothing was written to the host either
    # a negative amount; an index outside the set; a unit that is not > 0 or not finite
    refused("decay: amount -1", lib.lsm2d_occupancy_decay(ctx.handle, lo.handle, 0, None, -1))
    for idx in ([2], [0, -1], [0, 1, 2]):
        a = np.array(idx, np.int32)
        refused(("decay index", idx), lib.lsm2d_occupancy_decay(ctx.handle, lo.handle, len(a), api._ptr(a), 1))
    refused("decay: n -1", lib.lsm2d_occupancy_decay(ctx.handle, lo.handle, -1, api._ptr(np.zeros(1, np.int32)), 1))
    for g in (-1, 2):
        refused(("upload index", g), lib.lsm2d_gridset_upload_logodds(lo.handle, g, api._ptr(val), api._ptr(obs)))
        refused(("download index", g), lib.lsm2d_gridset_download_logodds(lo.handle, g, api._ptr(val), api._ptr(obs)))
        refused(("render index", g), lib.lsm2d_occupancy_render_logodds(ctx.handle, lo.handle, g, C.byref(rp), api._ptr(img)))
    for unit in (0.0, -0.5, float("nan"), float("inf")):
        bad = _capi.LogOddsRenderParamsC(1, unit)
        refused(("render unit", unit), lib.lsm2d_occupancy_render_logodds(ctx.handle, lo.handle, 0, C.byref(bad), api._ptr(img)))
    # a set of another context
    ctx2 = api.Context(0)
    try:
        other = api.GridSet(ctx2, lo.geometry, 2, P)
        refused("decay: another context", lib.lsm2d_occupancy_decay(ctx.handle, other.handle, 0, None, 1))
        refused("render: another context", lib.lsm2d_occupancy_render_logodds(ctx.handle, other.handle, 0, C.byref(rp), api._ptr(img)))
    finally:
        ctx2.close()
    assert (img == 77).all()
    # the context is usable and the calls still right
    _run(ctx, case, W, H, lo)
    _assert_cells(lo, lc.reference(case, W, H, P, *before_lo), "after the refusals")
    lo.close(); cs.close()


def test_two_runs_agree_bitwise(ctx):
    outs = []
    for _ in range(2):
        gs, counts = _run(ctx, SCAN_CASES["random"], W, H)
        gs.decay(17)
        outs.append((tuple(c.tobytes() for c in counts), _download(gs)[0].tobytes(), _download(gs)[1].tobytes(), api.occupancy_render_logodds(ctx, gs, 0, lc.UNIT, 2).tobytes()))
        gs.close()
    assert outs[0] == outs[1]
