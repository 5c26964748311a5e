"""Candidate lists (csrc/lsm2d_device.h, "candidate lists"; align_body in csrc/lsm2d_k_align.h; options "cand_lists", "cand_margin_um", "cand_margin_urad",
"cand_cap", "cand_first_it", "cand_max_builds"): once the pose has settled, an iteration of k_align<1,0,0,0,5> gathers the few thousand map
points that can still win a column instead of streaming the kept unit list.  The moving canvas keeps its bits, so everything a caller can see does.

Every case compares three things for bitwise equality -- the oracle (device order; sequential for "sum_order" 1), the call with "cand_lists" 0 and the call with
the lists on: pose, information matrix, status, iterations and every statistics row (chi, inliers, pair_digest) of every iteration -- and asserts through the
read-only options "last_cand_builds" / "last_cand_iterations" / "last_cand_overflows" that the path under test really ran (or, where the lists have no room, that
it did not).  All batches are small, so "zero_copy_max" 0 sends them the way bench.py's batch goes (copies, fast-forward available) and "align_path" 1 to k_align."""
import math

import numpy as np
import pytest

import ff_finish_cases as fc
from srrg2_laser_slam_2d_amd import api, synth

pytestmark = pytest.mark.gpu

ITS = 20
# the library's defaults, restored behind every run
DEFAULTS = dict(cand_lists=1, cand_margin_um=30, cand_margin_urad=3, cand_cap=3328, cand_first_it=3, cand_max_builds=2, fast_forward=2, sum_order=0,
                align_path=0, align_width=0, zero_copy_max=256)
MARGIN_MAX = (100000, 50000)      # the largest margins the option table admits
_CACHE = {}


def test_defaults_are_the_librarys(ctx):
    for k, v in DEFAULTS.items():
        assert ctx.get_option(k) == v, (k, ctx.get_option(k), v)
    with pytest.raises(Exception):
        ctx.set_option("cand_margin_um", MARGIN_MAX[0] + 1)
    with pytest.raises(Exception):
        ctx.set_option("cand_margin_urad", MARGIN_MAX[1] + 1)
    with pytest.raises(Exception):
        ctx.set_option("last_cand_builds", 1)
    assert ctx.get_option("cand_margin_um") == DEFAULTS["cand_margin_um"]


def _aligner(ctx, projs, its=ITS, **kw):
    al = api.MultiAligner2D(ctx, max_iterations=its, min_num_inliers=10, **kw)
    for proj in projs:
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(api.CorrespondenceFinderProjective2f(ctx, proj), min_num_correspondences=10))
    return al


def _run(ctx, al, fixed, moving, x0, fixed_index=None, **opts):
    """one batch with statistics; returns (bit patterns, counters)"""
    opts = dict(dict(align_path=1, zero_copy_max=0), **opts)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        r = al.compute_batch(fixed, moving, x0, fixed_index=fixed_index, want_stats=True)
        assert ctx.get_option("last_align_path") == 1
        n = len(r.status)
        bits = dict(pose=r.pose.view(np.uint32), information=r.information.reshape(n, 9).view(np.uint32), status=r.status, iterations=r.iterations,
                    stats=np.ascontiguousarray(r.stats).view(np.uint8).reshape(n, -1))
        return bits, dict(builds=ctx.get_option("last_cand_builds"), iterations=ctx.get_option("last_cand_iterations"), overflows=ctx.get_option("last_cand_overflows"),
                          width=ctx.get_option("last_align_width"))
    finally:
        for k in opts:
            ctx.set_option(k, DEFAULTS[k])


def _assert_same(got, want, tag, what, rows=None):
    for k in got:
        a, b = got[k].reshape(len(got[k]), -1), want[k].reshape(len(want[k]), -1)
        if rows is not None:
            b = b[rows]
        assert a.shape == b.shape, (tag, k, what, a.shape, b.shape)
        d = np.flatnonzero(np.any(a != b, axis=1))
        assert len(d) == 0, (tag, k, what, "alignments", d[:8].tolist())


def _three_way(ctx, al, fixed, moving, x0, want, tag, fixed_index=None, rows=None, **opts):
    """lists off, lists on, the oracle: all equal.  Returns the counters of the run with the lists on."""
    off, c_off = _run(ctx, al, fixed, moving, x0, fixed_index=fixed_index, **dict(opts, cand_lists=0))
    on, c_on = _run(ctx, al, fixed, moving, x0, fixed_index=fixed_index, **dict(opts, cand_lists=1))
    print(tag, "lists on:", c_on)
    assert (c_off["builds"], c_off["iterations"], c_off["overflows"]) == (0, 0, 0), (tag, c_off)
    _assert_same(off, want, tag, "cand_lists 0 against the oracle", rows=rows)
    _assert_same(on, want, tag, "cand_lists 1 against the oracle", rows=rows)
    _assert_same(on, off, tag, "cand_lists 1 against 0")
    return c_on


def _oracle(po, key, scans, maps, x0, slices, its=ITS, device_order=True, **ap):
    if key not in _CACHE:
        runs = [po.align(po.aligner_params(its, device_order=device_order, **ap), slices, [s] * len(slices), [maps] * len(slices), x) for s, x in zip(scans, x0)]
        _CACHE[key] = fc.as_arrays(runs, its)
    return _CACHE[key]


# ---- 1. bench.py's own three stragglers -----------------------------------------------------------------------------------------------------------------------
BENCH_ROWS = [26, 75, 523, 0, 1, 2, 3, 4]


def _bench_case(ctx):
    if "bench" not in _CACHE:
        world = synth.make_world(0)
        wl = synth.make_workload(1000, 100000, seed=0, n_beams=1081, world=world, map_points=np.zeros((0, 4), np.float32))
        m = synth.make_map(world, 100000, seed=0)
        scans = [wl.scan_points[wl.scan_offsets[i]:wl.scan_offsets[i + 1]] for i in BENCH_ROWS]
        offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
        _CACHE["bench"] = (scans, m, wl.x0[BENCH_ROWS].copy(), api.CloudSet(ctx, np.concatenate(scans), offs), api.CloudSet(ctx, m))
    return _CACHE["bench"]


@pytest.mark.parametrize("ff", [0, 2])
def test_bench_stragglers(ctx, po, ff):
    scans, m, x0, fixed, moving = _bench_case(ctx)
    want = _oracle(po, "bench_oracle", scans, m, x0, [po.slice_params()])
    al = _aligner(ctx, [api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)])
    c = _three_way(ctx, al, [fixed], [moving], x0, want, ("bench stragglers", ff), fast_forward=ff)
    assert c["width"] == 512
    assert c["iterations"] > 0 and c["overflows"] == 0, c


# ---- 2. smoke()'s size, three margins ----------------------------------------------------------------------------------------------------------------------------
def _small_case(ctx):
    if "small" not in _CACHE:
        wl = synth.make_workload(6, 20000, seed=2)
        scans = [wl.scan_points[wl.scan_offsets[i]:wl.scan_offsets[i + 1]] for i in range(6)]
        _CACHE["small"] = (scans, wl.map_points, wl.x0, api.CloudSet(ctx, wl.scan_points, wl.scan_offsets), api.CloudSet(ctx, wl.map_points))
    return _CACHE["small"]


@pytest.mark.parametrize("margins", [(30, 3), (1000, 100), MARGIN_MAX])
def test_margins(ctx, po, margins):
    scans, m, x0, fixed, moving = _small_case(ctx)
    want = _oracle(po, "small_oracle", scans, m, x0, [po.slice_params()])
    al = _aligner(ctx, [api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)])
    # (ff 0: every iteration runs, so a list built in iteration 2 has iterations to serve)
    c = _three_way(ctx, al, [fixed], [moving], x0, want, ("margins", margins), fast_forward=0, cand_margin_um=margins[0], cand_margin_urad=margins[1], cand_first_it=2)
    assert c["builds"] >= len(x0), c
    if margins != MARGIN_MAX:      # (the widest margins keep nearly every point: whether the lists fit is not this test's business)
        assert c["iterations"] > 0, c


# ---- 3. slow convergence: lists built and invalidated ---------------------------------------------------------------------------------------------------------------
def test_slow_convergence(ctx, po):
    scans, m, x0, fixed, moving = _small_case(ctx)
    want = _oracle(po, "small_oracle_damped", scans, m, x0, [po.slice_params()], damping=50.0)
    al = _aligner(ctx, [api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)], damping=50.0)
    # damping 50: the steps shrink by a factor of about seven per iteration, from 0.1 m to below a micrometre over eight iterations -- a list built behind every one
    # of them is left by the next step until the steps are within the margins
    c = _three_way(ctx, al, [fixed], [moving], x0, want, "slow convergence", fast_forward=0, cand_first_it=1, cand_max_builds=16)
    assert c["builds"] >= 3 * len(x0) and c["iterations"] > 0 and c["overflows"] == 0, c


# ---- 4. a partial canvas --------------------------------------------------------------------------------------------------------------------------------------------
def test_partial_canvas(ctx, po):
    scans, m, x0, fixed, moving = _small_case(ctx)
    r = np.hypot(m[:, 0] - x0[0, 0], m[:, 1] - x0[0, 1])
    th = np.arctan2(m[:, 1] - x0[0, 1], m[:, 0] - x0[0, 0]) - x0[0, 2]
    assert np.any(r > 21.0) and np.any(np.abs(np.arctan2(np.sin(th), np.cos(th))) > 2.5), "the map has points beyond range_max and outside the field of view"
    sl = po.slice_params(canvas_cols=721, angle_min=-0.75 * np.pi, angle_max=0.75 * np.pi, range_max=20.0)
    want = _oracle(po, "partial_oracle", scans, m, x0, [sl])
    al = _aligner(ctx, [api.PointNormal2fProjectorPolar(721, -0.75 * math.pi, 0.75 * math.pi, 0.3, 20.0)])
    c = _three_way(ctx, al, [fixed], [moving], x0, want, "partial canvas", fast_forward=0, cand_first_it=2)
    assert c["builds"] >= len(x0) and c["iterations"] > 0, c


# ---- 5. every list overflows ----------------------------------------------------------------------------------------------------------------------------------------
def test_overflow_falls_back(ctx, po):
    scans, m, x0, fixed, moving = _small_case(ctx)
    want = _oracle(po, "small_oracle", scans, m, x0, [po.slice_params()])
    al = _aligner(ctx, [api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)])
    c = _three_way(ctx, al, [fixed], [moving], x0, want, "cand_cap 64", fast_forward=0, cand_cap=64, cand_first_it=2)
    assert c["builds"] >= len(x0) and c["overflows"] == c["builds"] and c["iterations"] == 0, c


# ---- 6. batches without room ----------------------------------------------------------------------------------------------------------------------------------------
def test_two_slices_have_no_room(ctx, po):
    scans, m, x0, fixed, moving = _small_case(ctx)
    want = _oracle(po, "small_oracle_two", scans, m, x0, [po.slice_params(), po.slice_params()])
    proj = api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)
    al = _aligner(ctx, [proj, proj])
    c = _three_way(ctx, al, [fixed, fixed], [moving, moving], x0, want, "two slices", fast_forward=0, cand_first_it=2)
    assert (c["builds"], c["iterations"], c["overflows"]) == (0, 0, 0), c


def test_sum_order_1_has_no_room(ctx, po):
    scans, m, x0, fixed, moving = _small_case(ctx)
    want = _oracle(po, "small_oracle_seq", scans, m, x0, [po.slice_params()], device_order=False)
    al = _aligner(ctx, [api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)])
    c = _three_way(ctx, al, [fixed], [moving], x0, want, "sum_order 1", fast_forward=0, sum_order=1, cand_first_it=2)
    assert (c["builds"], c["iterations"], c["overflows"]) == (0, 0, 0), c


# ---- 7. the packed and the narrow form ------------------------------------------------------------------------------------------------------------------------------
# (... and a batch of two full dispatch rounds in the wide form: more than one round has no tail for the lists to shorten, the host offers none)
@pytest.mark.parametrize("form", [("k_align_two", 1040, 1024), ("k_align_narrow", 1100, 256), ("k_align", 512, 512), ("k_align, two rounds", 2048, 512)])
def test_launch_forms(ctx, po, form):
    name, n, width = form
    if "ff_sets" not in _CACHE:
        m, wl = fc.workload()
        _CACHE["ff_sets"] = (api.CloudSet(ctx, wl.scan_points, wl.scan_offsets), api.CloudSet(ctx, m), wl)
    fixed, moving, wl = _CACHE["ff_sets"]
    want = fc.oracle_arrays(po, ITS, True)
    idx = np.arange(n) % fc.N
    al = _aligner(ctx, [api.PointNormal2fProjectorPolar(fc.COLS, -math.pi, math.pi, 0.3, 30.0)])
    opts = dict(align_width=width) if width != 512 or n > 1024 else {}
    c = _three_way(ctx, al, [fixed], [moving], wl.x0[idx], want, name, fixed_index=idx.astype(np.int32)[None, :], rows=idx, fast_forward=0, cand_first_it=2, **opts)
    assert c["width"] == width, c
    if width == 512 and n <= 1024:
        assert c["builds"] >= n and c["iterations"] > 0, c      # the wide kernel carries the lists
    else:
        assert (c["builds"], c["iterations"], c["overflows"]) == (0, 0, 0), c      # the packed and the narrow form, and batches of several rounds, do not: same bits all the same
