"""GPU tests of lsm2d_relocalize_select: the scoring's selection, the gather of the selected hypotheses and the aligner chained on the device.  Every output
must be, bit for bit, what lsm2d_score_aligner_select followed by lsm2d_align_select over the selected hypotheses gives on the same context
(relocalize_cases.two_calls) -- across finders, both orders of summation, one slice and two WithSensor slices with priors and index arrays, batch sizes, k_score
(1: a single slot without the inline start pose; 257: past the latency kernel; against a map-sized cloud: onto the placement estimate), k, every align_path and fast_forward -- and, for
"sum_order" 1, the CPU restatement end to end.  No tolerance appears in this file."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import align_select_cases as ac
import relocalize_cases as rc
from srrg2_laser_slam_2d_amd import api, synth
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT

pytestmark = pytest.mark.gpu

MAX_K = api.SELECT_MAX_K
EVERYTHING, NOTHING = rc.EVERYTHING, rc.NOTHING


def _finder(ctx, kind):
    if kind == "proj":
        return api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(ac.COLS, -math.pi, math.pi, 0.3, 30.0))
    return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=ac.MD, search="exact")


def _aligner(ctx, kind="proj", min_num_inliers=10, sensors=None):
    al = api.MultiAligner2D(ctx, max_iterations=ac.ITERATIONS, min_num_inliers=min_num_inliers)
    kw = dict(robustifier=api.RobustifierCauchy(ac.TAU), min_num_correspondences=ac.MIN_CORR)
    if sensors is None:
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(_finder(ctx, kind), **kw))
    else:
        for S in sensors:
            al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(_finder(ctx, kind), sensor_in_robot=S, **kw))
    return al


@pytest.fixture(scope="module")
def cs(ctx):
    c = rc.make_cases()
    c.scan_set = api.CloudSet(ctx, c.scan); c.map_set = api.CloudSet(ctx, c.map)
    fixed, moving, c.fixed_index, c.priors = rc.two_slice_inputs(c)
    c.fixed2 = [api.CloudSet(ctx, p, o) for p, o in fixed]; c.moving2 = [api.CloudSet(ctx, m) for m in moving]
    c.pair_set = api.CloudSet(ctx, np.ascontiguousarray(np.concatenate([c.scan, c.scan[::2]])), np.int32([0, len(c.scan), len(c.scan) + len(c.scan[::2])]))
    c.min_inliers = {}      # (kind, variant) -> the median of the device's own last-row inlier counts: some candidates end NotEnoughInliers
    return c


@pytest.fixture()
def order_ctx(ctx, request):
    ctx.set_option("sum_order", request.param)
    try:
        yield ctx
    finally:
        ctx.set_option("sum_order", 0)


def _setup(ctx, cs, kind, variant):
    """(aligner, fixed, moving, keyword arguments) of a variant: "one" slice without priors, or "two" WithSensor slices with priors and index arrays"""
    two = variant == "two"
    fx, mv = (cs.fixed2, cs.moving2) if two else ([cs.scan_set], [cs.map_set])
    kw = dict(priors=cs.priors, fixed_index=cs.fixed_index) if two else {}
    al = _aligner(ctx, kind, 0, rc.S_OFF if two else None)
    if (kind, variant) not in cs.min_inliers:
        first = al.compute_batch(fx, mv, cs.poses, want_stats=True, **kw)
        n_in = first.last_stats()["n_inliers"][first.status == 0]
        cs.min_inliers[(kind, variant)] = int(np.sort(n_in)[len(n_in) // 2])
    al.param_min_num_inliers = cs.min_inliers[(kind, variant)]
    return al, fx, mv, kw


def _thresholds(al, fx, mv, poses, kw):
    """the middle of the device's own first-iteration rows (stage 1) and of its aligned Success rows (stage 2): every threshold an item's own fp32 value"""
    _, _, st, active = api.score_aligner(al, fx, mv, poses, kw.get("priors"), kw.get("fixed_index"))
    res = al.compute_batch(fx, mv, poses, want_stats=True, **kw)
    ok = res.status == 0      # (a batch of one or two hypotheses may hold no Success: everything passes then)
    return ac.middle_thresholds(st[active > 0]), ac.middle_thresholds(res.last_stats()[ok]) if np.any(ok) else EVERYTHING


def _both(al, fx, mv, poses, s1, k_score, s2, k, tag, **kw):
    want = rc.two_calls(al, fx, mv, poses, s1, k_score, s2, k, **kw)
    got = api.relocalize_select(al, fx, mv, poses, s1, k_score, s2, k, **kw)
    print(tag, "k_score", k_score, "k", k, "scored", got.n_scored_accepted, len(got.scored_index), "aligned", got.n_success, got.n_accepted, len(got.index))
    rc.assert_same(got, want, (tag, k_score, k))
    return got


# ---- 1. the fused call equals the two calls ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["one", "two"])
@pytest.mark.parametrize("kind", ["proj", "nn"])
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_fused_equals_two_calls(order_ctx, cs, kind, variant):
    ctx = order_ctx
    al, fx, mv, kw = _setup(ctx, cs, kind, variant)
    mid1, mid2 = _thresholds(al, fx, mv, cs.poses, kw)
    seen_m = set()
    for s1, s2 in ((mid1, mid2), (EVERYTHING, mid2), (mid1, None)):
        for k_score in rc.K_SCORES:
            for k in sorted({1, k_score, MAX_K}):
                if s1 is EVERYTHING and k not in (k_score,):
                    continue
                got = _both(al, fx, mv, cs.poses, s1, k_score, s2, k, (kind, variant, ctx.get_option("sum_order")), **kw)
                seen_m.add((len(got.scored_index) < k_score, got.n_accepted > 0, got.n_accepted < got.n_success))
    assert any(t[0] for t in seen_m) and any(not t[0] for t in seen_m) and any(t[1] and t[2] for t in seen_m)
    assert ctx.last_kernel_ms() > 0.0


@pytest.mark.parametrize("n", [1, 2, 2049])
def test_batch_sizes(ctx, cs, n):
    """one hypothesis, two (a two-cloud fixed set without an index array: "cloud i" spelled out on the device), and 2049 -- the 300 tiled, so that stage 1's
    selection needs a second tile and the duplicates' ties cross it"""
    al, fx, mv, kw = _setup(ctx, cs, "proj", "one")
    poses = ac.cyclic(cs, n)
    if n == 2:
        fx = [cs.pair_set]; poses = np.ascontiguousarray(cs.poses[[8, 14]])
    mid1, mid2 = _thresholds(al, fx, mv, poses, kw)
    for s1 in (mid1, EVERYTHING):
        for k_score in rc.K_SCORES:
            for k in sorted({1, k_score, MAX_K}):
                got = _both(al, fx, mv, poses, s1, k_score, mid2, k, ("n", n), **kw)
    assert len(got.scored_index) == min(n if n != 2049 else 2049 - 7, rc.K_SCORES[-1])      # EVERYTHING: all but the copies of the pose that finds nothing


@pytest.mark.parametrize("options", [dict(align_path=0), dict(align_path=1), dict(align_path=2), dict(align_path=3), dict(fast_forward=0), dict(fast_forward=2)],
                         ids=lambda o: "%s=%d" % next(iter(o.items())))
@pytest.mark.parametrize("variant", ["one", "two"])
def test_every_path_and_option(ctx, cs, variant, options):
    al, fx, mv, kw = _setup(ctx, cs, "proj", variant)
    mid1, mid2 = _thresholds(al, fx, mv, cs.poses, kw)
    defaults = dict(align_path=0, fast_forward=2)
    try:
        for key, v in options.items():
            ctx.set_option(key, v)
        for k_score in rc.K_SCORES:
            _both(al, fx, mv, cs.poses, mid1, k_score, mid2, k_score, (variant, options), **kw)
            if options.get("align_path"):
                assert ctx.get_option("last_align_path") == options["align_path"]
        _both(al, fx, mv, cs.poses, EVERYTHING, 257, mid2, 64, (variant, options), **kw)
    finally:
        for key, v in defaults.items():
            ctx.set_option(key, v)


# ---- 2. "sum_order" 1 against the CPU, end to end -----------------------------------------------------------------------------------------------------------------
def test_reference_order_against_the_cpu(ctx, po, cs):
    rows1, active, M, full = rc.oracle_stages(po, cs)
    tc = rc.threshold_cases(rows1, active, full)
    al = _aligner(ctx, "proj", M)
    ctx.set_option("sum_order", 1)
    try:
        for name, (s1, k_score, s2) in tc.items():
            for k in (1024, 7):
                got = api.relocalize_select(al, [cs.scan_set], [cs.map_set], cs.poses, s1, k_score, s2, k)
                want = rc.restate(rows1, active, full, s1, k_score, s2, k)
                print(name, k, "m", len(got.scored_index), "accepted", got.n_accepted, "success", got.n_success)
                rc.assert_same(got, want, (name, k))
    finally:
        ctx.set_option("sum_order", 0)


# ---- 3. pads never show ---------------------------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, al, fx, mv, poses, s1, k_score, s2, k, fill=-77):
    """the bare C call into buffers of k_score / k rows filled with a pattern"""
    bd, keep = al._batch(fx, mv, poses)
    ap = al._aligner_params()
    s_index = np.full(k_score, fill, np.int32); s_st = np.full(k_score * 7, fill, np.int32)
    index = np.full(k, fill, np.int32); pose = np.full((k, 3), fill, np.float32); H = np.full((k, 9), fill, np.float32); its = np.full(k, fill, np.int32)
    st = np.full(k * 7, fill, np.int32)
    cnt = [C.c_int32(fill) for _ in range(5)]
    sel1 = s1.struct(); sel2 = s2.struct()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    rc_ = ctx._lib.lsm2d_relocalize_select(ctx.handle, C.byref(ap), C.byref(bd), C.byref(sel1), k_score, C.byref(sel2), k, p(s_index), p(s_st), C.byref(cnt[0]),
                                           C.byref(cnt[1]), p(index), p(pose), p(H), p(its), p(st), C.byref(cnt[2]), C.byref(cnt[3]), C.byref(cnt[4]))
    return rc_, [c_.value for c_ in cnt], (s_index, s_st.reshape(k_score, 7), index, pose, H, its, st.reshape(k, 7))


def test_pads_never_show(ctx, cs):
    al, fx, mv, kw = _setup(ctx, cs, "proj", "one")
    mid1, mid2 = _thresholds(al, fx, mv, cs.poses, kw)
    fill = -77
    swapped = cs.poses.copy(); swapped[[0, 1]] = swapped[[1, 0]]      # hypothesis 0 finds nothing: with m = 0 every pad ends NotEnoughCorrespondences
    for poses, s1, k_score in ((cs.poses, NOTHING, 64), (swapped, NOTHING, 64), (swapped, NOTHING, 257), (cs.poses, mid1, 257), (swapped, mid1, 64)):
        code, (n_ssel, n_sacc, n_sel, n_acc, n_suc), bufs = _raw(ctx, al, fx, mv, poses, s1, k_score, EVERYTHING, k_score, fill)
        assert code == 0
        assert n_ssel == min(n_sacc, k_score) and n_ssel < k_score and n_suc <= n_ssel and n_acc <= n_suc and n_sel == min(n_acc, k_score)
        if s1 is NOTHING:
            assert (n_ssel, n_sacc, n_sel, n_acc, n_suc) == (0, 0, 0, 0, 0)
        else:
            assert n_ssel > 0 and n_sel > 0
        s_index, s_st, index, pose, H, its, st = bufs
        assert np.all(s_index[n_ssel:] == fill) and np.all(s_st[n_ssel:] == fill)
        assert np.all(index[n_sel:] == fill) and np.all(its[n_sel:] == fill) and np.all(st[n_sel:] == fill)
        assert np.all(pose[n_sel:] == np.float32(fill)) and np.all(H[n_sel:] == np.float32(fill))
        assert set(index[:n_sel].tolist()) <= set(s_index[:n_ssel].tolist())      # every output is a real selected hypothesis


# ---- 4. the lanes' caches are honest afterwards -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(ctx, cs):
    """the same world with a 3000-point map: a moving cloud past 1024 points gets the lane-chunked copy without which no placement estimate is made"""
    wl = synth.make_workload(1, 3000, seed=5, n_beams=ac.COLS, map_noise=ac.NOISE, scan_noise=ac.NOISE)
    assert np.array_equal(wl.x0[0], cs.wl.x0[0])
    return types.SimpleNamespace(scan_set=api.CloudSet(ctx, np.ascontiguousarray(wl.scan_points)), map_set=api.CloudSet(ctx, np.ascontiguousarray(wl.map_points)))


def _same_result(a, b):
    return (np.array_equal(rc.u32(a.pose), rc.u32(b.pose)) and np.array_equal(rc.u32(a.information), rc.u32(b.information)) and
            np.array_equal(a.status, b.status) and np.array_equal(a.iterations, b.iterations) and a.stats.tobytes() == b.stats.tobytes())


@pytest.mark.parametrize("k_score", [257, 300])
def test_placement_estimate_reads_the_device_poses(ctx, cs, big, k_score):
    """past 256 slots, against a map-sized cloud, stage 2 makes a balanced placement: k_cull_estimate reads the poses k_reloc_items has just written"""
    al = _aligner(ctx, "proj", 10)
    fx, mv = [big.scan_set], [big.map_set]
    mid1, mid2 = _thresholds(al, fx, mv, cs.poses, {})
    for s1 in (EVERYTHING, mid1):
        got = _both(al, fx, mv, cs.poses, s1, k_score, mid2, 64, ("estimate", k_score))
        assert ctx.get_option("last_cull_estimate") == 1 and ctx.get_option("last_align_path") == 1
    assert 0 < len(got.scored_index) < k_score      # mid1: pads were placed and aligned too


@pytest.mark.parametrize("n", [4, 300])
def test_align_batch_is_unchanged_around_the_call(ctx, cs, big, n):
    """lsm2d_align_batch, the fused call, the same lsm2d_align_batch with byte-identical inputs ON THE LANE STAGE 2 USED.  The batch is a prepared one run
    through begin / wait, which moves the context on to the other lane each time: after six runs BOTH lanes hold its input block with the host's shadow of
    it (n = 4: "zero_copy_max" 0, or a batch that small keeps no block on the device) and, at n = 300 with "balance" on, a placement kept with notes.  The
    fused call then scores on the current lane and aligns on the other one, overwriting that lane's input block and placement with data the host never saw.
    The second run afterwards lands on that lane: it must upload its inputs again (else it aligns the fused call's hypotheses) and, where the fused call
    made a placement of the same shape (k_score = n = 300), make its placement again."""
    assert ctx.get_option("balance") == 1
    al = _aligner(ctx, "proj", 10)
    fx, mv = [big.scan_set], [big.map_set]
    poses = np.ascontiguousarray(cs.poses[:n])
    others = np.ascontiguousarray(cs.poses[::-1])      # the fused call's hypotheses: slot j of its aligner never holds poses[j]
    ctx.set_option("zero_copy_max", 0 if n <= 256 else 256)
    try:
        ref = al.compute_batch(fx, mv, poses, want_stats=True)
        pb = al.prepare_batch(fx, mv, poses, want_stats=True)

        def run():
            pb.begin()
            return pb.wait(copy=True)

        for _ in range(6):
            assert _same_result(ref, run())
        if n > 256:
            assert ctx.get_option("last_cull_estimate") == 0      # the kept placement is in use: a stale one would be, too
        for k_score in (max(n, 2), 257):
            for flip in (0, 1):      # ... whichever lane is the current one
                if flip:
                    assert _same_result(ref, run())
                api.relocalize_select(al, fx, mv, others, EVERYTHING, k_score, EVERYTHING, k_score)
                estimates = []
                for _ in range(4):      # the current lane, stage 2's lane, and both once more
                    assert _same_result(ref, run()), (n, k_score, flip)
                    estimates.append(ctx.get_option("last_cull_estimate"))
                if n > 256 and k_score == n:
                    assert estimates[1] == 1 and estimates[3] == 0, estimates      # made again on stage 2's lane, and kept again from then on
    finally:
        ctx.set_option("zero_copy_max", 256)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_context_alone(ctx, cs):
    al, fx, mv, kw = _setup(ctx, cs, "proj", "one")
    fill = -77
    for k_score, k in ((0, 4), (MAX_K + 1, 4), (4, 0), (4, MAX_K + 1)):
        code, counts, bufs = _raw_bad_k(ctx, al, fx, mv, cs.poses, k_score, k, fill)
        assert code == BAD_ARGUMENT and all(v == fill for v in counts) and all(np.all(b == fill) for b in bufs)
    # a NULL the call needs
    bd, keep = al._batch(fx, mv, cs.poses)
    ap = al._aligner_params(); sel = EVERYTHING.struct()
    n1 = C.c_int32(fill)
    idx = np.full(4, fill, np.int32); pose = np.full((4, 3), fill, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    code = ctx._lib.lsm2d_relocalize_select(ctx.handle, C.byref(ap), C.byref(bd), C.byref(sel), 4, None, 4, None, None, C.byref(n1), C.byref(n1), p(idx), p(pose), None,
                                            None, None, C.byref(n1), C.byref(n1), None)
    assert code == BAD_ARGUMENT and n1.value == fill and np.all(idx == fill)
    # a cloud index out of range: refused by stage 1's rules before anything is launched
    bad = np.zeros((1, len(cs.poses)), np.int32); bad[0, 17] = 5
    with pytest.raises(Exception):
        api.relocalize_select(al, fx, mv, cs.poses, EVERYTHING, 4, None, 4, fixed_index=bad)
    # a batch in flight
    pending = al.prepare_batch(fx, mv, cs.poses[:8])
    pending.begin()
    try:
        code, counts, bufs = _raw(ctx, al, fx, mv, cs.poses, EVERYTHING, 4, EVERYTHING, 4, fill)
        assert code == BAD_ARGUMENT and all(v == fill for v in counts) and all(np.all(b == fill) for b in bufs)
    finally:
        pending.wait()
    # the context is usable and the call still right
    mid1, mid2 = _thresholds(al, fx, mv, cs.poses, kw)
    _both(al, fx, mv, cs.poses, mid1, 64, mid2, 7, "after refusals")
    # no hypotheses at all: success, zeros
    empty = api.relocalize_select(al, fx, mv, np.zeros((0, 3), np.float32), EVERYTHING, 4, None, 4)
    assert len(empty.index) == 0 and len(empty.scored_index) == 0 and (empty.n_scored_accepted, empty.n_accepted, empty.n_success) == (0, 0, 0)


def _raw_bad_k(ctx, al, fx, mv, poses, k_score, k, fill):
    """_raw with buffers of at least one row, whatever the (refused) k_score and k are"""
    bd, keep = al._batch(fx, mv, poses)
    ap = al._aligner_params(); sel = EVERYTHING.struct()
    rows = 4
    s_index = np.full(rows, fill, np.int32); index = np.full(rows, fill, np.int32); pose = np.full((rows, 3), fill, np.float32)
    cnt = [C.c_int32(fill) for _ in range(5)]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    code = ctx._lib.lsm2d_relocalize_select(ctx.handle, C.byref(ap), C.byref(bd), C.byref(sel), k_score, C.byref(sel), k, p(s_index), None, C.byref(cnt[0]),
                                            C.byref(cnt[1]), p(index), p(pose), None, None, None, C.byref(cnt[2]), C.byref(cnt[3]), C.byref(cnt[4]))
    return code, [c_.value for c_ in cnt], (s_index, index, pose)
