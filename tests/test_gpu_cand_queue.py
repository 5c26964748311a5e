"""The candidate lists' queue of maybes (csrc/lsm2d_device_cand.h: project_point_stream_blk<., true>, project_cloud_list_blkq_t, cand_collect_queue_t): with
"cand_queue" 1 the build iteration's stream tests every interior point against the PROVISIONAL blocker of its column -- the word its atomic minimum returns -- and
queues the index of every point that test does not settle; the collect then classifies the queue's points alone, against the final blockers, instead of the whole
unit list.  A build whose maybes outgrow the queue's room ("cand_queue_cap" entries per alignment) makes its list from the unit list as "cand_queue" 0 does.  The
list is the same SET either way, so every canvas, pair, sum and pose keeps its bits and the books a caller can read keep their values.

Every case is four-way bitwise -- the device-order oracle, "cand_lists" 0, "cand_queue" 0 and "cand_queue" 1: pose, information, status, iterations and every
statistics row -- and "builds", served "iterations" and "overflows" are equal between "cand_queue" 0 and 1.  The set-up is that of tests/test_gpu_cand_collect.py,
restated here: 8 scans x 1081 beams of synth's world 2 at 20 iterations, "align_path" 1, "zero_copy_max" 0, every option a case depends on set explicitly and put
back to the library's default behind the run; every case runs with "fast_forward" 0 and 2.

The shapes are the smallest at which the new code can go wrong (a cloud of n points: 512 chunks of T = ceil(n / 1024) steps, blocks of B = 2 ceil(T / 14) steps):
 * the chunk's last block is one step (3 000, 17 000), an odd number of steps (19 000, cloud 1 of two) or full (20 000); a single block (2 000); T < B behind a
   larger cloud (1 000 behind 20 000): the fused stream runs on the collect pass's wave-owned unit loop, with its look-ahead and its lanes without a unit;
 * a unit longer than the 32-bit mask of maybes (120 000 points, B = 18, a 361-column canvas): the unit's maybes reach the queue in two segments;
 * many points outside the stream's own gates -- maybes whose class only the collect knows: a canvas of a quarter circle, and "range_max" 4 m;
 * both instantiations of the bearing's guard ("range_min" 0.3 and 1e-5);
 * the queue's room: 0 (every build falls back), the default (none does: the queue path made the lists), 512 and 2 048 (some of the eight may, others not);
 * repeated builds ("cand_first_it" 1, "cand_max_builds" 16): the counter and the region are used again and again;
 * an empty unit list (start poses 200 m away): no maybes, no list;
 * "cand_cap" 64: every list overflows behind the queue path."""
import math

import numpy as np
import pytest

import ff_finish_cases as fc
from srrg2_laser_slam_2d_amd import api, synth

pytestmark = pytest.mark.gpu

ITS, N = 20, 8
FULL = (1081, -math.pi, math.pi, 0.3, 30.0)
GUARDED = (1081, -math.pi, math.pi, 1e-5, 30.0)
NARROW = (361, -math.pi, math.pi, 0.3, 30.0)
QUARTER = (271, -math.pi / 4, math.pi / 4, 0.3, 30.0)
SHORT = (1081, -math.pi, math.pi, 0.3, 4.0)
QCAP = 16384
# the library's defaults, restored behind every run
DEFAULTS = dict(cand_lists=1, cand_queue=1, cand_queue_cap=QCAP, cand_margin_um=30, cand_margin_urad=3, cand_cap=3328, cand_first_it=3, cand_max_builds=2, fast_forward=2,
                sum_order=0, align_path=0, align_width=0, zero_copy_max=256)
_CACHE = {}


def _layout(n):
    """(T, B, steps of a chunk's last block) of an n-point cloud in the lane-chunked copy (ensure_lane_layout, cull_block_steps)"""
    T = ((n + 1) // 2 + 511) // 512
    B = 2 * ((T + 13) // 14)
    return T, B, T - (-(-T // B) - 1) * B


def _world(ctx):
    if "wl" not in _CACHE:
        wl = synth.make_workload(N, 20000, seed=2)
        scans = [wl.scan_points[wl.scan_offsets[i]:wl.scan_offsets[i + 1]] for i in range(N)]
        _CACHE["wl"] = (wl, scans, api.CloudSet(ctx, wl.scan_points, wl.scan_offsets))
    return _CACHE["wl"]


def _points(ctx, n):
    wl, _, _ = _world(ctx)
    if ("points", n) not in _CACHE:
        _CACHE["points", n] = wl.map_points if n == 20000 else synth.make_map(wl.world, n, seed=2)
    return _CACHE["points", n]


def _map(ctx, n, behind):
    """(moving set, moving_index) of the n-point map: a set of its own, or cloud 1 of a set behind a 20 000-point cloud"""
    wl, _, _ = _world(ctx)
    key = ("map", n, behind)
    if key not in _CACHE:
        m = _points(ctx, n)
        if behind:
            both = np.concatenate([wl.map_points, m])
            _CACHE[key] = (api.CloudSet(ctx, both, np.array([0, len(wl.map_points), len(both)], np.int32)), np.ones((1, N), np.int32))
        else:
            _CACHE[key] = (api.CloudSet(ctx, m), None)
    return _CACHE[key]


def _x0(ctx, far):
    x0 = _world(ctx)[0].x0.copy()
    if far:
        x0[:, 0] += 200.0
    return x0


def _oracle(po, ctx, n, proj, far):
    key = ("oracle", n, proj, far)
    if key not in _CACHE:
        _, scans, _ = _world(ctx)
        m = _points(ctx, n)
        sl = po.slice_params(canvas_cols=proj[0], angle_min=proj[1], angle_max=proj[2], range_min=proj[3], range_max=proj[4])
        runs = [po.align(po.aligner_params(ITS, device_order=True), [sl], [s], [m], x) for s, x in zip(scans, _x0(ctx, far))]
        _CACHE[key] = fc.as_arrays(runs, ITS)
    return _CACHE[key]


def _run(ctx, al, fixed, moving, x0, moving_index, **opts):
    """one batch with statistics under exactly `opts` on top of the defaults; returns (bit patterns, books)"""
    opts = dict(DEFAULTS, **opts)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        r = al.compute_batch([fixed], [moving], x0, moving_index=moving_index, want_stats=True)
        assert ctx.get_option("last_align_path") == 1 and ctx.get_option("last_align_width") == 512
        n = len(r.status)
        bits = dict(pose=r.pose.view(np.uint32), information=r.information.reshape(n, 9).view(np.uint32), status=r.status, iterations=r.iterations,
                    stats=np.ascontiguousarray(r.stats).view(np.uint8).reshape(n, -1))
        return bits, dict(builds=ctx.get_option("last_cand_builds"), iterations=ctx.get_option("last_cand_iterations"), overflows=ctx.get_option("last_cand_overflows"),
                          fallbacks=ctx.get_option("last_cand_fallbacks"))
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


def _assert_same(got, want, tag, what):
    for k in got:
        a, b = got[k].reshape(len(got[k]), -1), want[k].reshape(len(want[k]), -1)
        assert a.shape == b.shape, (tag, k, what, a.shape, b.shape)
        d = np.flatnonzero(np.any(a != b, axis=1))
        assert len(d) == 0, (tag, k, what, "alignments", d[:8].tolist())


def _four_way(ctx, po, tag, n, proj=FULL, behind=False, far=False, **opts):
    """the device-order oracle, lists off, the collect over the unit list, the collect over the queue: all equal, bit for bit, and the two collects' books equal.
    Returns (books with the queue, its bit patterns)."""
    _, _, fixed = _world(ctx)
    moving, mi = _map(ctx, n, behind)
    want = _oracle(po, ctx, n, proj, far)
    al = api.MultiAligner2D(ctx, max_iterations=ITS, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(*proj)), min_num_correspondences=10))
    opts = dict(dict(align_path=1, zero_copy_max=0), **opts)
    off, c_off = _run(ctx, al, fixed, moving, _x0(ctx, far), mi, **dict(opts, cand_lists=0))
    q0, c_q0 = _run(ctx, al, fixed, moving, _x0(ctx, far), mi, **dict(opts, cand_lists=1, cand_queue=0))
    q1, c_q1 = _run(ctx, al, fixed, moving, _x0(ctx, far), mi, **dict(opts, cand_lists=1, cand_queue=1))
    print(tag, "cand_queue 0:", c_q0, "cand_queue 1:", c_q1)
    assert (c_off["builds"], c_off["iterations"], c_off["overflows"], c_off["fallbacks"]) == (0, 0, 0, 0), (tag, c_off)
    _assert_same(off, want, tag, "cand_lists 0 against the oracle")
    _assert_same(q0, want, tag, "cand_queue 0 against the oracle")
    _assert_same(q1, want, tag, "cand_queue 1 against the oracle")
    _assert_same(q1, q0, tag, "cand_queue 1 against 0")
    _assert_same(q1, off, tag, "cand_queue 1 against cand_lists 0")
    assert c_q0["fallbacks"] == 0, (tag, c_q0)      # (no queue, nothing to fall back from)
    assert all(c_q1[k] == c_q0[k] for k in ("builds", "iterations", "overflows")), (tag, c_q0, c_q1)
    assert 0 <= c_q1["fallbacks"] <= c_q1["builds"], (tag, c_q1)
    return c_q1, q1


def _ran_all(on):
    """the alignments that ran every iteration (under "fast_forward" 0 each of them had the chance to build a list in front of iteration `cand_first_it` + 1)"""
    return int(np.sum(on["iterations"] == ITS))


# ---- 1. block shapes: the chunk's last block one step, an odd number, full; a single block; T below B ------------------------------------------------------------
BLOCKS = [  # n, (T, B, last block), cloud 1 of two, cand_first_it
    (2000, (2, 2, 2), False, 1),
    (3000, (3, 2, 1), False, 2),
    (17000, (17, 4, 1), False, 2),
    (19000, (19, 4, 3), True, 2),
    (20000, (20, 4, 4), False, 1),
    (1000, (1, 2, 1), True, 1),
]


@pytest.mark.parametrize("ff", [0, 2])
@pytest.mark.parametrize("case", BLOCKS, ids=[str(c[0]) for c in BLOCKS])
def test_block_shapes(ctx, po, case, ff):
    n, layout, behind, first_it = case
    assert _layout(n) == layout, (n, _layout(n))
    c, on = _four_way(ctx, po, ("blocks", n, ff), n, behind=behind, fast_forward=ff, cand_first_it=first_it)
    assert c["overflows"] == 0, c
    if ff == 0:
        assert c["builds"] >= max(_ran_all(on), 1) and c["iterations"] > 0, (c, on["iterations"])


# ---- 2. a unit longer than the mask of maybes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
def test_unit_longer_than_the_mask(ctx, po, ff):
    n = 120000
    T, B, last = _layout(n)
    assert (T, B, last) == (118, 18, 10) and B > 16
    c, on = _four_way(ctx, po, ("segments", n, ff), n, proj=NARROW, fast_forward=ff, cand_first_it=2)
    if ff == 0:
        assert c["builds"] >= max(_ran_all(on), 1) and c["builds"] > c["overflows"] and c["iterations"] > 0, (c, on["iterations"])


# ---- 3. many points outside the stream's gates: maybes whose class only the collect knows -------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
@pytest.mark.parametrize("proj", [QUARTER, SHORT], ids=["quarter_circle", "range_max_4m"])
def test_points_outside_the_gates(ctx, po, proj, ff):
    c, on = _four_way(ctx, po, ("outside the gates", proj, ff), 20000, proj=proj, fast_forward=ff, cand_first_it=2)
    if ff == 0:
        assert c["builds"] >= _ran_all(on), (c, on["iterations"])


# ---- 4. the bearing's guard, on and off ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
@pytest.mark.parametrize("proj", [FULL, GUARDED], ids=["tiny_ok", "guarded"])
def test_bearing_guard(ctx, po, proj, ff):
    """ProjK::tiny_ok (make_projk) is true when 2.1e-12 / (0.7 range_min) < 2.5e-8: 0.3 m runs the <false> instantiations of the stream and the collect, 1e-5 m the <true> ones."""
    assert 2.1e-12 / (0.7 * FULL[3]) < 2.5e-8 <= 2.1e-12 / (0.7 * GUARDED[3])
    c, on = _four_way(ctx, po, ("guard", proj[3], ff), 19000, proj=proj, fast_forward=ff, cand_first_it=2)
    assert c["overflows"] == 0, c
    if ff == 0:
        assert c["builds"] >= _ran_all(on) >= 1 and c["iterations"] > 0, (c, on["iterations"])


# ---- 5. the queue's room ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
@pytest.mark.parametrize("qcap", [0, 512, 2048, QCAP])
def test_queue_room(ctx, po, qcap, ff):
    c, on = _four_way(ctx, po, ("cand_queue_cap", qcap, ff), 20000, fast_forward=ff, cand_queue_cap=qcap, cand_first_it=2)
    assert c["overflows"] == 0, c
    if qcap == 0:
        assert c["fallbacks"] == c["builds"], c
    elif qcap == QCAP:      # the queue path, not the fallback, made the lists
        assert c["fallbacks"] == 0 and c["builds"] > 0, c
    if ff == 0:
        assert c["builds"] >= _ran_all(on) >= 1 and c["iterations"] > 0, (c, on["iterations"])


# ---- 6. repeated builds: the counter and the region are used again --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
def test_repeated_builds(ctx, po, ff):
    c, on = _four_way(ctx, po, ("repeated builds", ff), 20000, fast_forward=ff, cand_first_it=1, cand_max_builds=16)
    assert c["overflows"] == 0, c
    if ff == 0:
        assert c["builds"] > N and c["iterations"] > 0, c


# ---- 7. an empty unit list ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
def test_empty_unit_list(ctx, po, ff):
    c, on = _four_way(ctx, po, ("empty unit list", ff), 20000, far=True, fast_forward=ff, cand_first_it=1)
    assert np.all(on["status"] != 0) and not on["information"].any(), (on["status"], c)      # (the oracle's, by the four-way comparison: no pairs, zero matrices)
    assert c["overflows"] == 0 and c["fallbacks"] == 0, c


# ---- 8. "cand_cap" 64: every list overflows behind the queue path ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
def test_every_list_overflows(ctx, po, ff):
    c, on = _four_way(ctx, po, ("cand_cap 64", ff), 20000, fast_forward=ff, cand_cap=64, cand_first_it=2)
    assert c["overflows"] == c["builds"] and c["iterations"] == 0 and c["fallbacks"] == 0, c
    if ff == 0:
        assert c["builds"] >= _ran_all(on) >= 1, (c, on["iterations"])
