"""The candidate lists' build with the blockers made inside the stream (csrc/lsm2d_device.h: project_point_stream_blk, cand_classify_polar; align_body's
`cst == 2` branch in csrc/lsm2d_k_align.h): the iteration that builds a list clears the blockers, streams the unit list once -- the canvas update and, from the
r, th, u and column just computed, the column's blocker -- and collects behind it.  The blockers, hence the list, hence every canvas, pair, sum and pose keep
their bits; the cases below put the build where its bookkeeping and its edges are: in the alignment's last iteration, one before it, across unit-list
rebuilds, with a list that overflows, on a partial canvas, over an empty unit list, with the bearing's guard on and off, with and without the fast-forward.

Every case is three-way bitwise, as in tests/test_gpu_candidate_lists.py (whose helpers, small case and oracle cache this file shares): the device-order
oracle, "cand_lists" 0 and "cand_lists" 1 -- pose, information, status, iterations and every statistics row -- on that file's small case (6 scans x 1081
beams, a 20 000-point map, seed 2) with "align_path" 1 and "zero_copy_max" 0.

Bookkeeping: a build is booked behind the iteration that made its blockers, the alignment's last iteration included (so `max_iterations = cand_first_it + 1`
books one build per alignment that nothing ever uses); an overflow is booked with it."""
import math

import numpy as np
import pytest

import test_gpu_candidate_lists as cl
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu

N = 6      # alignments of the small case
FULL = (1081, -math.pi, math.pi, 0.3, 30.0)


def _run(ctx, al, fixed, moving, x0, **opts):
    """cl._run for any option: what an option was before the call is what it is behind it"""
    opts = dict(dict(align_path=1, zero_copy_max=0), **opts)
    before = {k: ctx.get_option(k) for k in opts}
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        r = al.compute_batch(fixed, moving, x0, want_stats=True)
        assert ctx.get_option("last_align_path") == 1
        n = len(r.status)
        bits = dict(pose=r.pose.view(np.uint32), information=r.information.reshape(n, 9).view(np.uint32), status=r.status, iterations=r.iterations,
                    stats=np.ascontiguousarray(r.stats).view(np.uint8).reshape(n, -1))
        return bits, dict(builds=ctx.get_option("last_cand_builds"), iterations=ctx.get_option("last_cand_iterations"), overflows=ctx.get_option("last_cand_overflows"),
                          width=ctx.get_option("last_align_width"))
    finally:
        for k, v in before.items():
            ctx.set_option(k, v)


def _three_way(ctx, al, fixed, moving, x0, want, tag, **opts):
    off, c_off = _run(ctx, al, fixed, moving, x0, **dict(opts, cand_lists=0))
    on, c_on = _run(ctx, al, fixed, moving, x0, **dict(opts, cand_lists=1))
    print(tag, "lists on:", c_on)
    assert (c_off["builds"], c_off["iterations"], c_off["overflows"]) == (0, 0, 0), (tag, c_off)
    cl._assert_same(off, want, tag, "cand_lists 0 against the oracle")
    cl._assert_same(on, want, tag, "cand_lists 1 against the oracle")
    cl._assert_same(on, off, tag, "cand_lists 1 against 0")
    assert c_on["width"] == 512, (tag, c_on)
    return c_on, on


def _case(ctx, po, its, proj=FULL, x0=None, key=None, **ap):
    """(aligner, fixed set, moving set, start poses, oracle arrays) of the small case at max_iterations `its`"""
    scans, m, x0s, fixed, moving = cl._small_case(ctx)
    x0 = x0s if x0 is None else x0
    sl = po.slice_params(canvas_cols=proj[0], angle_min=proj[1], angle_max=proj[2], range_min=proj[3], range_max=proj[4])
    want = cl._oracle(po, ("fused", key, proj, its, tuple(sorted(ap.items()))), scans, m, x0, [sl], its=its, **ap)
    al = cl._aligner(ctx, [api.PointNormal2fProjectorPolar(*proj)], its=its, **ap)
    return al, fixed, moving, x0, want


# ---- 1. the build is the alignment's last iteration -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
@pytest.mark.parametrize("first_it", [1, 2, 3])
def test_build_in_the_last_iteration(ctx, po, first_it, ff):
    al, fixed, moving, x0, want = _case(ctx, po, first_it + 1)
    c, _ = _three_way(ctx, al, [fixed], [moving], x0, want, ("build last", first_it, ff), fast_forward=ff, cand_first_it=first_it)
    assert (c["builds"], c["iterations"], c["overflows"]) == (N, 0, 0), c


# ---- 2. the list is collected, and decided about, for the alignment's last iteration ---------------------------------------------------------------------------
@pytest.mark.parametrize("ff", [0, 2])
@pytest.mark.parametrize("first_it", [1, 2, 3])
def test_list_decided_for_the_last_iteration(ctx, po, first_it, ff):
    """One list per alignment ("cand_max_builds" 1: with the default of two, an alignment whose pose has left the first list's margins builds a second one in
    its last iteration, which is booked like any other -- that run is held to the bits and to between one and two builds per alignment)."""
    al, fixed, moving, x0, want = _case(ctx, po, first_it + 2)
    c, _ = _three_way(ctx, al, [fixed], [moving], x0, want, ("decided last", first_it, ff, 1), fast_forward=ff, cand_first_it=first_it, cand_max_builds=1)
    assert c["builds"] == N and c["overflows"] == 0, c
    c2, _ = _three_way(ctx, al, [fixed], [moving], x0, want, ("decided last", first_it, ff, 2), fast_forward=ff, cand_first_it=first_it)
    assert N <= c2["builds"] <= 2 * N and c2["overflows"] == 0, c2


# ---- 3. lists built while every iteration rebuilds the unit list ----------------------------------------------------------------------------------------------
def test_build_across_unit_list_rebuilds(ctx, po):
    """damping 50 (test_slow_convergence: the steps shrink by about seven per iteration), the unit list's keep margins at their smallest admitted values (0, 0):
    the unit list is rebuilt in front of every iteration whose pose differs from the one it was built at, in front of every build among them"""
    scans, m, x0, fixed, moving = cl._small_case(ctx)
    want = cl._oracle(po, "small_oracle_damped", scans, m, x0, [po.slice_params()], damping=50.0)
    al = cl._aligner(ctx, [api.PointNormal2fProjectorPolar(*FULL)], damping=50.0)
    c, _ = _three_way(ctx, al, [fixed], [moving], x0, want, "rebuilds", fast_forward=0, cand_first_it=1, cand_max_builds=16, cull_margin_um=0, cull_margin_urad=0)
    assert c["builds"] >= 3 * N and c["iterations"] > 0 and c["overflows"] == 0, c


# ---- 4. a list that overflows -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("its", [None, 20])
@pytest.mark.parametrize("first_it", [1, 2, 3])
def test_overflow(ctx, po, first_it, its):
    its = first_it + 2 if its is None else its
    al, fixed, moving, x0, want = _case(ctx, po, its)
    c, _ = _three_way(ctx, al, [fixed], [moving], x0, want, ("cand_cap 64", first_it, its), fast_forward=0, cand_cap=64, cand_first_it=first_it)
    assert c["builds"] >= N and c["overflows"] == c["builds"] and c["iterations"] == 0, c


# ---- 5. a partial canvas; a blocker array whose length is no multiple of four ------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_it", [1, 2, 3])
@pytest.mark.parametrize("proj", [(721, -0.75 * math.pi, 0.75 * math.pi, 0.3, 20.0), FULL], ids=["721", "1081"])
def test_canvases(ctx, po, proj, first_it):
    scans, m, x0, _, _ = cl._small_case(ctx)
    r = np.hypot(m[:, 0] - x0[0, 0], m[:, 1] - x0[0, 1])
    th = np.arctan2(m[:, 1] - x0[0, 1], m[:, 0] - x0[0, 0]) - x0[0, 2]
    th = np.abs(np.arctan2(np.sin(th), np.cos(th)))
    assert np.any(r > 21.0) and np.any(th > 2.5) and np.any(th > math.pi - 0.01), "the map has points beyond range_max, outside the field of view and at the wrap"
    assert proj[0] % 4 == 1
    al, fixed, moving, x0, want = _case(ctx, po, cl.ITS, proj=proj)
    c, _ = _three_way(ctx, al, [fixed], [moving], x0, want, ("canvas", proj[0], first_it), fast_forward=0, cand_first_it=first_it)
    assert c["builds"] >= N and c["iterations"] > 0, c


# ---- 6. an empty unit list --------------------------------------------------------------------------------------------------------------------------------------
def test_empty_unit_list(ctx, po):
    scans, m, x0, _, _ = cl._small_case(ctx)
    far = x0.copy(); far[:, 0] += 200.0
    al, fixed, moving, far, want = _case(ctx, po, cl.ITS, x0=far, key="far")
    c, on = _three_way(ctx, al, [fixed], [moving], far, want, "empty unit list", fast_forward=0, cand_first_it=1)
    assert np.all(on["status"] != 0) and not on["information"].any(), (on["status"], c)      # (the oracle's, by the three-way comparison: no pairs, zero matrices)


# ---- 7. the bearing's guard, on and off ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("range_min", [0.3, 1e-5], ids=["tiny_ok", "guarded"])
def test_bearing_guard(ctx, po, range_min):
    """ProjK::tiny_ok (make_projk) is true when 2.1e-12 / (0.7 range_min) < 2.5e-8, i.e. range_min above 1.2e-4 m: 0.3 m runs the stream without the guard in
    front of the short quotient, 1e-5 m the one with it -- both instantiations of the fused stream and of the collect."""
    assert 2.1e-12 / (0.7 * 0.3) < 2.5e-8 <= 2.1e-12 / (0.7 * 1e-5)
    al, fixed, moving, x0, want = _case(ctx, po, cl.ITS, proj=(1081, -math.pi, math.pi, range_min, 30.0))
    c, _ = _three_way(ctx, al, [fixed], [moving], x0, want, ("guard", range_min), fast_forward=0, cand_first_it=2)
    assert c["builds"] >= N and c["iterations"] > 0 and c["overflows"] == 0, c


# ---- 8. fast-forward ----------------------------------------------------------------------------------------------------------------------------------------------
def test_fast_forward(ctx, po):
    al, fixed, moving, x0, want = _case(ctx, po, cl.ITS)
    c2, on2 = _three_way(ctx, al, [fixed], [moving], x0, want, ("ff", 2), fast_forward=2, cand_first_it=2)
    c0, on0 = _three_way(ctx, al, [fixed], [moving], x0, want, ("ff", 0), fast_forward=0, cand_first_it=2)
    cl._assert_same(on2, on0, "ff", "fast_forward 2 against 0")
    assert c2["builds"] <= c0["builds"] and c0["builds"] >= N, (c2, c0)
