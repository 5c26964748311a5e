"""The candidate lists' collect pass (csrc/lsm2d_device_cand.h: cand_for_each_pair, cand_collect_t): the build iteration's second pass over the unit list's points
walks each unit with the stream's two-buffer look-ahead and appends a wave's keeps once per unit -- a lane notes its keeps in a 32-bit mask (two bits per step),
and behind the unit's last step the wave scans the popcounts, adds their total to the LDS counter once and writes the indices.  The list is the same SET as
before (its order is free), so every canvas, pair, sum and pose keeps its bits, and the counters a caller can read keep their values.

Every case is three-way bitwise -- the device-order oracle, "cand_lists" 0 and "cand_lists" 1: pose, information, status, iterations and every statistics row --
on 8 scans x 1081 beams of synth's world 2 at 20 iterations, with "align_path" 1 and "zero_copy_max" 0 (tests/test_gpu_candidate_lists.py, whose comparison
this file restates for itself).  Every option a case depends on is set explicitly and put back to the library's default behind the run.

The shapes are the smallest at which the walk can go wrong.  A cloud of n points is cut into 512 chunks of T = ceil(n / 1024) steps (two points a step) and a chunk
into blocks of B = cull_block_steps(T) = 2 ceil(T / 14) steps; a unit is one block of one chunk.
 * the last block of a chunk: one step (n = 3 000: T 3, B 2; n = 17 000: T 17, B 4), an even number short of B (18 000: 2 of 4), an odd number above one (19 000: 3
   of 4), a full one (20 000; 2 000: T = B = 2, a single block) -- the look-ahead's tail step and its read of one row past the block;
 * T below B: only a cloud of at most 1 024 points has it (T 1, B 2), and it gets the lane-chunked layout only in a set with a larger cloud: a 1 000-point
   cloud behind a 20 000-point one;
 * the moving cloud is the LAST cloud of its set in every case (the only one, or cloud 1 of two: a chunk row that does not start at the copy's first byte), so
   the look-ahead of the last block reads the spare rows behind the copy;
 * more than 16 steps in a unit (n = 120 000: T 118, B 18; a 361-column canvas leaves the list its room): the mask is flushed after 16 steps and the rest of the unit
   is a segment of its own;
 * thread coverage: at n = 2 000 and 3 000 there are at most 512 and 1 024 units before culling, so whole waves and single lanes of the 512 threads have no unit
   in a trip (a unit list's length is not visible to a caller: eight alignments at eight poses give eight lengths per case); a far start pose leaves the
   unit list empty;
 * "cand_cap" 64: every list overflows, the count past the capacity is still formed ("overflows" == "builds", no served iteration); 1024 and the default;
 * both instantiations of the bearing's guard (ProjK::tiny_ok: range_min 0.3 and 1e-5, tests/test_gpu_cand_fused_build.py);
 * "fast_forward" 0 (every iteration runs: lists are built and served many times, "cand_first_it" 1 - 2, "cand_max_builds" up to 16) and 2."""
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
# the library's defaults (tests/test_gpu_candidate_lists.py pins them), restored behind every run
DEFAULTS = dict(cand_lists=1, cand_margin_um=30, cand_margin_urad=3, cand_cap=3328, cand_first_it=3, cand_max_builds=2, fast_forward=2, sum_order=0,
                align_path=0, align_width=0, zero_copy_max=256)
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


def _oracle(po, ctx, n, proj, far):
    key = ("oracle", n, proj, far)
    if key not in _CACHE:
        wl, scans, _ = _world(ctx)
        m = _points(ctx, n)
        sl = po.slice_params(canvas_cols=proj[0], angle_min=proj[1], angle_max=proj[2], range_min=proj[3], range_max=proj[4])
        runs = [po.align(po.aligner_params(ITS, device_order=True), [sl], [s], [m], x) for s, x in zip(scans, _x0(ctx, far))]
        _CACHE[key] = fc.as_arrays(runs, ITS)
    return _CACHE[key]


def _x0(ctx, far):
    x0 = _world(ctx)[0].x0.copy()
    if far:
        x0[:, 0] += 200.0
    return x0


def _run(ctx, al, fixed, moving, x0, moving_index, **opts):
    """one batch with statistics under exactly `opts` on top of the defaults; returns (bit patterns, counters)"""
    opts = dict(DEFAULTS, **opts)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        r = al.compute_batch([fixed], [moving], x0, moving_index=moving_index, want_stats=True)
        assert ctx.get_option("last_align_path") == 1 and ctx.get_option("last_align_width") == 512
        n = len(r.status)
        bits = dict(pose=r.pose.view(np.uint32), information=r.information.reshape(n, 9).view(np.uint32), status=r.status, iterations=r.iterations,
                    stats=np.ascontiguousarray(r.stats).view(np.uint8).reshape(n, -1))
        return bits, dict(builds=ctx.get_option("last_cand_builds"), iterations=ctx.get_option("last_cand_iterations"), overflows=ctx.get_option("last_cand_overflows"))
    finally:
        for k, v in DEFAULTS.items():
            ctx.set_option(k, v)


def _assert_same(got, want, tag, what):
    for k in got:
        a, b = got[k].reshape(len(got[k]), -1), want[k].reshape(len(want[k]), -1)
        assert a.shape == b.shape, (tag, k, what, a.shape, b.shape)
        d = np.flatnonzero(np.any(a != b, axis=1))
        assert len(d) == 0, (tag, k, what, "alignments", d[:8].tolist())


def _three_way(ctx, po, tag, n, proj=FULL, behind=False, far=False, **opts):
    """lists off, lists on, the device-order oracle: all equal, bit for bit.  Returns (counters with the lists on, its bit patterns)."""
    _, _, fixed = _world(ctx)
    moving, mi = _map(ctx, n, behind)
    want = _oracle(po, ctx, n, proj, far)
    al = api.MultiAligner2D(ctx, max_iterations=ITS, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(*proj)), min_num_correspondences=10))
    opts = dict(dict(align_path=1, zero_copy_max=0), **opts)
    off, c_off = _run(ctx, al, fixed, moving, _x0(ctx, far), mi, **dict(opts, cand_lists=0))
    on, c_on = _run(ctx, al, fixed, moving, _x0(ctx, far), mi, **dict(opts, cand_lists=1))
    print(tag, "lists on:", c_on)
    assert (c_off["builds"], c_off["iterations"], c_off["overflows"]) == (0, 0, 0), (tag, c_off)
    _assert_same(off, want, tag, "cand_lists 0 against the oracle")
    _assert_same(on, want, tag, "cand_lists 1 against the oracle")
    _assert_same(on, off, tag, "cand_lists 1 against 0")
    return c_on, on


def _ran_all(on):
    """the alignments that ran every iteration (under "fast_forward" 0 each of them had the chance to build a list in front of iteration `cand_first_it` + 1)"""
    return int(np.sum(on["iterations"] == ITS))


# ---- 1. the last block of a chunk: one step, an even number short of B, an odd number, full; a single block; T below B ----------------------------------------------
BLOCKS = [  # n, (T, B, last block), cloud 1 of two, cand_first_it, cand_max_builds
    (2000, (2, 2, 2), False, 1, 2),
    (3000, (3, 2, 1), False, 2, 2),
    (17000, (17, 4, 1), False, 2, 2),
    (18000, (18, 4, 2), False, 1, 2),
    (19000, (19, 4, 3), True, 2, 2),
    (20000, (20, 4, 4), False, 1, 16),
    (1000, (1, 2, 1), True, 1, 2),
]


@pytest.mark.parametrize("ff", [0, 2])
@pytest.mark.parametrize("case", BLOCKS, ids=[str(c[0]) for c in BLOCKS])
def test_block_lengths(ctx, po, case, ff):
    n, layout, behind, first_it, max_builds = case
    assert _layout(n) == layout, (n, _layout(n))
    c, on = _three_way(ctx, po, ("blocks", n, ff), n, behind=behind, fast_forward=ff, cand_first_it=first_it, cand_max_builds=max_builds)
    assert c["overflows"] == 0, c
    if ff == 0:
        assert c["builds"] >= max(_ran_all(on), 1) and c["iterations"] > 0, (c, on["iterations"])


# ---- 2. a unit of more than 16 steps: the mask's segments -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
def test_unit_longer_than_the_mask(ctx, po, ff):
    n = 120000
    T, B, last = _layout(n)
    assert (T, B, last) == (118, 18, 10) and B > 16
    c, on = _three_way(ctx, po, ("segments", n, ff), n, proj=NARROW, fast_forward=ff, cand_first_it=2)
    if ff == 0:
        assert c["builds"] >= max(_ran_all(on), 1) and c["builds"] > c["overflows"] and c["iterations"] > 0, (c, on["iterations"])


# ---- 3. an empty unit list ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
def test_empty_unit_list(ctx, po, ff):
    c, on = _three_way(ctx, po, ("empty unit list", ff), 20000, far=True, fast_forward=ff, cand_first_it=1)
    assert np.all(on["status"] != 0) and not on["information"].any(), (on["status"], c)      # (the oracle's, by the three-way comparison: no pairs, zero matrices)
    assert c["overflows"] == 0, c


# ---- 4. the capacity: every list overflows, a smaller room, the default ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
@pytest.mark.parametrize("cap", [64, 1024, DEFAULTS["cand_cap"]])
def test_capacity(ctx, po, cap, ff):
    c, on = _three_way(ctx, po, ("cand_cap", cap, ff), 20000, fast_forward=ff, cand_cap=cap, cand_first_it=2)
    if ff == 0:
        assert c["builds"] >= _ran_all(on) >= 1, (c, on["iterations"])
    if cap == 64:      # (a 20 000-point map's list has several hundred entries: the counter must have gone on counting past the 64)
        assert c["overflows"] == c["builds"] and c["iterations"] == 0, c
    elif cap == DEFAULTS["cand_cap"]:
        assert c["overflows"] == 0, c
        if ff == 0:
            assert c["iterations"] > 0, c
    else:
        assert c["overflows"] <= c["builds"], c


# ---- 5. the bearing's guard, on and off -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
@pytest.mark.parametrize("proj", [FULL, GUARDED], ids=["tiny_ok", "guarded"])
def test_bearing_guard(ctx, po, proj, ff):
    """ProjK::tiny_ok (make_projk) is true when 2.1e-12 / (0.7 range_min) < 2.5e-8: 0.3 m runs cand_collect_t<false>, 1e-5 m cand_collect_t<true>."""
    assert 2.1e-12 / (0.7 * FULL[3]) < 2.5e-8 <= 2.1e-12 / (0.7 * GUARDED[3])
    c, on = _three_way(ctx, po, ("guard", proj[3], ff), 19000, proj=proj, fast_forward=ff, cand_first_it=2)
    assert c["overflows"] == 0, c
    if ff == 0:
        assert c["builds"] >= _ran_all(on) >= 1 and c["iterations"] > 0, (c, on["iterations"])
