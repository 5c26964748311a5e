"""GPU tests of lsm2d_score_select (lsm2d_score_batch's scoring, then k_select_keys / k_select_tile / k_select_gather on the rows where they lie).  The call
must return exactly what api.score_rank -- the acceptance test and the ranking restated in numpy float32 / integer arithmetic -- selects from the statistics
of the same hypotheses, and for every selected hypothesis the bits lsm2d_score_batch returns.  The statistics come from the CPU oracle (po.find, then
po.linearize_device_order for "sum_order" 0, the sequential po.linearize for "sum_order" 1) where the batch is small, and from api.score_batch -- unchanged
code, itself held to the oracle by test_gpu_score_batch.py -- where it is large.  No tolerance appears in this file."""
import ctypes as C
import math

import numpy as np
import pytest

import score_select_cases as cases
from srrg2_laser_slam_2d_amd import api
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT

pytestmark = pytest.mark.gpu

T = api.SELECT_TILE        # entries a workgroup of k_select_tile sorts: where the selection takes another pass
MAX_K = api.SELECT_MAX_K
PAIR_BUDGET = 1 << 21      # pair slots per launch group (kBatchPairBudget, lsm2d_capi_finder.inc)
EVERYTHING = api.SelectParams(0, float("inf"), 0.0)
NOTHING = api.SelectParams(10 ** 9, 0.0, 2.0)


@pytest.fixture(scope="module")
def cs(ctx, po):
    c = cases.make_cases()
    c.scan_set = api.CloudSet(ctx, c.scan)
    c.map_set = api.CloudSet(ctx, c.map)
    c.pairs = {}      # the oracle's correspondence vectors per finder kind: found once, shared by every case of that kind
    return c


@pytest.fixture()
def order_ctx(ctx, request):
    ctx.set_option("sum_order", request.param)
    try:
        yield ctx
    finally:
        ctx.set_option("sum_order", 0)


def _finder(ctx, kind):
    if kind == "proj":
        return api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cases.COLS, -math.pi, math.pi, 0.3, 30.0))
    if kind == "nn":
        return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=cases.MD, search="exact")
    if kind == "kd":
        return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=cases.MD, search="kdtree")
    return api.CorrespondenceFinderNN2D(ctx, max_distance_m=cases.MD)


def _slice(ctx, kind="proj", robust=api.ROBUST_CAUCHY):
    sp = _finder(ctx, kind).slice_params()
    sp.robustifier = robust; sp.chi_threshold = cases.TAU
    return sp


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _batch_rows(ctx, sp, fixed, moving, poses, **kw):
    """api.score_batch's results with the statistics as one structured array"""
    H, b, st = api.score_batch(ctx, sp, fixed, moving, poses, **kw)
    return H, b, api._stats_array(st)


def _check_against(got, H, b, st, sel, k, tag):
    """got = api.score_select's return; (H, b, st) the rows of ALL hypotheses: the selection is score_rank's, the rows are theirs, bit for bit"""
    index, gH, gb, gst, n_acc = got
    want, want_acc = api.score_rank(st, sel, k)
    print(tag, "k", k, "accepted", n_acc, "/", len(st), "selected", len(index), "expected", want_acc, len(want))
    assert n_acc == want_acc, tag
    assert index.dtype == np.int32 and np.array_equal(index, want), (tag, index[:16], want[:16])
    assert gH.shape == (len(want), 3, 3) and gb.shape == (len(want), 3) and gst.shape == (len(want),) and gst.dtype == api.STATS_DTYPE
    assert np.array_equal(_u32(gH), _u32(H[want])) and np.array_equal(_u32(gb), _u32(b[want])), tag
    assert gst.tobytes() == np.ascontiguousarray(st[want]).tobytes(), tag
    return want, want_acc


# ---- 1. against the oracle, small ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust", [api.ROBUST_NONE, api.ROBUST_CAUCHY], ids=["plain", "cauchy"])
@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_against_the_oracle(order_ctx, po, cs, kind, robust):
    ctx = order_ctx
    order = ctx.get_option("sum_order")
    if kind not in cs.pairs:
        cs.pairs[kind] = cases.oracle_pairs(po, cs, kind)
    H, b, st = cases.oracle_rows(po, cs, kind, po.ROBUST_CAUCHY if robust == api.ROBUST_CAUCHY else po.ROBUST_NONE, order, cs.pairs[kind])
    sel = cases.middle_thresholds(st)
    cond = cases.conditions(st, sel)
    assert np.all(cond.any(axis=1)) and not np.any(cond.all(axis=1)), (kind, robust, order, sel)      # each condition alone passes and rejects somebody
    sp = _slice(ctx, kind, robust)
    for k in (64, 7):
        got = api.score_select(ctx, sp, cs.scan_set, cs.map_set, cs.poses, sel, k)
        want, n_acc = _check_against(got, H, b, st, sel, k, (kind, robust, order))
        assert 0 < n_acc < len(st) and len(want) == min(k, n_acc)
    assert ctx.last_kernel_ms() > 0.0      # "kernel_timing": the last launch group and the selection


# ---- 2. thresholds at equality ---------------------------------------------------------------------------------------------------------------------------------
def test_thresholds_at_equality(ctx, po, cs):
    if "proj" not in cs.pairs:
        cs.pairs["proj"] = cases.oracle_pairs(po, cs, "proj")
    H, b, st = cases.oracle_rows(po, cs, "proj", po.ROBUST_CAUCHY, 0, cs.pairs["proj"])
    sp = _slice(ctx)
    per_inlier, ratio = cases.quotients(st)
    mid = api.score_rank(st, cases.middle_thresholds(st), MAX_K)[0]
    mid = [int(i) for i in mid if st["n_outliers"][i] > 0 and per_inlier[i] > 0]
    j = mid[len(mid) // 2]      # a hypothesis from the middle of the ranking, with inliers and outliers
    at = (int(st["n_inliers"][j]), float(per_inlier[j]), float(ratio[j]))
    for sel in (api.SelectParams(*at), api.SelectParams(at[0], float("inf"), 0.0), api.SelectParams(0, at[1], 0.0), api.SelectParams(0, float("inf"), at[2])):
        got = api.score_select(ctx, sp, cs.scan_set, cs.map_set, cs.poses, sel, MAX_K)
        want, n_acc = _check_against(got, H, b, st, sel, MAX_K, ("equality", sel))
        assert j in got[0].tolist() and n_acc < len(st), sel      # >= and <= at equality accept; somebody else is rejected
    # one ulp to the wrong side of each threshold and the hypothesis is gone
    tight = (api.SelectParams(at[0] + 1, at[1], at[2]), api.SelectParams(at[0], float(np.nextafter(np.float32(at[1]), np.float32(0.0))), at[2]),
             api.SelectParams(at[0], at[1], float(np.nextafter(np.float32(at[2]), np.float32(2.0)))))
    for sel in tight:
        got = api.score_select(ctx, sp, cs.scan_set, cs.map_set, cs.poses, sel, MAX_K)
        _check_against(got, H, b, st, sel, MAX_K, ("one ulp off", sel))
        assert j not in got[0].tolist(), sel


# ---- 3. tile and pass edges -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large(ctx, cs):
    """3 T + 1 hypotheses (three selection passes at k = MAX_K: 4 tiles, 2 tiles, 1 tile) scored once by api.score_batch; the smaller batches are its prefixes"""
    n = 3 * T + 1
    poses = cases.many_poses(cs, n)
    H, b, st = _batch_rows(ctx, _slice(ctx), cs.scan_set, cs.map_set, poses)
    return poses, H, b, st, cases.middle_thresholds(st)


@pytest.mark.parametrize("n", [1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T + 1])
def test_tile_and_pass_edges(ctx, cs, large, n):
    poses, H, b, st, mid = large
    assert math.ceil(math.ceil((3 * T + 1) / T) * MAX_K / T) > 1      # the largest batch at k = MAX_K needs a third pass
    sp = _slice(ctx)
    # an item's row does not depend on the batch it is scored in: the prefix of the large batch IS score_batch's result for the first n poses
    Hn, bn, stn = _batch_rows(ctx, sp, cs.scan_set, cs.map_set, poses[:n]) if n <= T + 1 else (H[:n], b[:n], st[:n])
    assert stn.tobytes() == np.ascontiguousarray(st[:n]).tobytes() and np.array_equal(_u32(Hn), _u32(H[:n]))
    for k in sorted({1, 2, min(n, MAX_K), min(n + 1, MAX_K), MAX_K}):
        for sel in (mid, EVERYTHING):
            got = api.score_select(ctx, sp, cs.scan_set, cs.map_set, poses[:n], sel, k)
            _, n_acc = _check_against(got, Hn, bn, stn, sel, k, ("edges", n))
            if sel is EVERYTHING:
                assert n_acc == n
    if n > T:
        assert api.score_rank(stn, mid, MAX_K)[1] > 0


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_ties_come_out_in_ascending_index(ctx, cs):
    sp = _slice(ctx)
    n = T + 700
    poses = cases.many_poses(cs, n, seed=12)
    _, _, st0 = _batch_rows(ctx, sp, cs.scan_set, cs.map_set, poses)
    best = int(api.score_rank(st0, EVERYTHING, 1)[0][0])
    same = np.arange(T - 301, T + 299, 2)      # 300 copies of the best pose of all, every other item across the tile boundary
    same = same[same != best]
    poses[same] = poses[best]
    H, b, st = _batch_rows(ctx, sp, cs.scan_set, cs.map_set, poses)
    tied = np.sort(np.append(same, best))
    assert len(tied) >= 300 and len(set(st[i].tobytes() for i in tied)) == 1 and st["n_inliers"][best] > 0      # equal keys
    for k in (MAX_K, 100):
        got = api.score_select(ctx, sp, cs.scan_set, cs.map_set, poses, EVERYTHING, k)
        _check_against(got, H, b, st, EVERYTHING, k, "ties")
        m = min(k, len(tied))
        assert np.array_equal(got[0][:m], tied[:m])      # the copies lead the ranking, by index
    # identical poses only: the ranking is the index
    poses[:] = poses[best]
    for k in (MAX_K, 3):
        index, _, _, gst, n_acc = api.score_select(ctx, sp, cs.scan_set, cs.map_set, poses, EVERYTHING, k)
        assert n_acc == n and np.array_equal(index, np.arange(k)) and gst.tobytes() == st[best].tobytes() * k


# ---- 5. several launch groups -------------------------------------------------------------------------------------------------------------------------------------
def test_several_launch_groups(ctx, cs):
    sp = _slice(ctx, "nn")
    slot = len(cs.map)      # a point-query item's slot: the largest moving cloud
    per_group = PAIR_BUDGET // slot
    n = per_group + 400
    assert n * slot > PAIR_BUDGET and n > T
    poses = cases.many_poses(cs, n, seed=13)
    H, b, st = _batch_rows(ctx, sp, cs.scan_set, cs.map_set, poses)
    for sel in (cases.middle_thresholds(st), EVERYTHING):
        got = api.score_select(ctx, sp, cs.scan_set, cs.map_set, poses, sel, MAX_K)
        want, n_acc = _check_against(got, H, b, st, sel, MAX_K, "two launch groups")
        assert np.any(want < per_group) and np.any(want >= per_group) and n_acc > 0      # selected items of both groups


# ---- 6. nothing and everything ---------------------------------------------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Out:
    def __init__(self, k):
        m = max(min(k, MAX_K + 1), 1)
        self.index = np.full(m, -7, np.int32); self.H = np.full((m, 9), -7.0, np.float32); self.b = np.full((m, 3), -7.0, np.float32)
        self.st = np.full(m * 7, 0x5A5A5A5A, np.uint32).view(api.STATS_DTYPE)
        self.n_sel = C.c_int32(-7); self.n_acc = C.c_int32(-7)

    def untouched(self, start=0, counts=True):
        return bool(np.all(self.index[start:] == -7) and np.all(self.H[start:] == -7.0) and np.all(self.b[start:] == -7.0) and
                    np.all(self.st[start:].view(np.uint32) == 0x5A5A5A5A) and (not counts or (self.n_sel.value == -7 and self.n_acc.value == -7)))


def _raw(ctx, sp, fixed, fi, moving, mi, poses, sel, k, n=None, want=(True, True, True), null_select=False, null_index=False):
    poses = None if poses is None else np.ascontiguousarray(poses, np.float32)
    n = len(poses) if n is None else n
    out = _Out(k)
    s = sel.struct()
    rc = ctx._lib.lsm2d_score_select(ctx.handle, C.byref(sp), fixed.handle, _ptr(fi), moving.handle, _ptr(mi), n, _ptr(poses),
                                     None if null_select else C.byref(s), k, None if null_index else _ptr(out.index), _ptr(out.H) if want[0] else None,
                                     _ptr(out.b) if want[1] else None, _ptr(out.st) if want[2] else None, C.byref(out.n_sel), C.byref(out.n_acc))
    return rc, out


def test_nothing_accepted(ctx, cs):
    rc, out = _raw(ctx, _slice(ctx), cs.scan_set, None, cs.map_set, None, cs.poses, NOTHING, 64)
    assert rc == 0 and out.n_sel.value == 0 and out.n_acc.value == 0 and out.untouched(counts=False)
    index, H, b, st, n_acc = api.score_select(ctx, _slice(ctx), cs.scan_set, cs.map_set, cs.poses, NOTHING, 64)
    assert n_acc == 0 and index.shape == (0,) and H.shape == (0, 3, 3) and b.shape == (0, 3) and st.shape == (0,)
    # n_items == 0: both counts are set, nothing else is written
    rc, out = _raw(ctx, _slice(ctx), cs.scan_set, None, cs.map_set, None, None, EVERYTHING, 64, n=0)
    assert rc == 0 and out.n_sel.value == 0 and out.n_acc.value == 0 and out.untouched(counts=False)


def test_everything_accepted_but_a_nan(ctx, po, cs):
    """{0, +Inf, 0} accepts every hypothesis whose chi_inliers is not NaN.  The hypothesis scored against a scan with a NaN normal sums a NaN (no robustifier:
    every pair is an inlier) and must be absent; the one given a NaN pose finds no pair at all, sums exact zeros, and is ranked last like every empty item."""
    sp = _slice(ctx, "proj", api.ROBUST_NONE)
    v = po.find(cases.oracle_slice(po, "proj", po.ROBUST_NONE), cs.scan, cs.map, cs.poses[0])
    bad = cs.scan.copy(); bad[v[0][0], 2:] = np.nan      # the normal of a point that is paired at poses[0]
    offs = np.int32([0, len(cs.scan), 2 * len(cs.scan)])
    two = api.CloudSet(ctx, np.ascontiguousarray(np.concatenate([cs.scan, bad])), offs)
    n = 40
    poses = cs.poses[:n].copy(); poses[5] = cs.poses[0]; poses[9] = np.nan
    fi = np.zeros(n, np.int32); fi[5] = 1
    H, b, st = _batch_rows(ctx, sp, two, cs.map_set, poses, fixed_index=fi)
    nan = np.isnan(st["chi_inliers"])
    assert nan[5] and nan.sum() == 1 and st["n_correspondences"][9] == 0 and st["n_correspondences"][1] == 0
    got = api.score_select(ctx, sp, two, cs.map_set, poses, EVERYTHING, MAX_K, fixed_index=fi)
    want, n_acc = _check_against(got, H, b, st, EVERYTHING, MAX_K, "everything")
    sel_list = got[0].tolist()
    assert n_acc == n - 1 and 5 not in sel_list and sel_list.index(1) < sel_list.index(9)      # the two empty items tie: by index


# ---- 7. outputs beyond n_selected, NULL outputs -----------------------------------------------------------------------------------------------------------------
def test_outputs_beyond_n_selected_are_untouched_and_may_be_null(ctx, cs):
    sp = _slice(ctx)
    H, b, st = _batch_rows(ctx, sp, cs.scan_set, cs.map_set, cs.poses)
    sel = cases.middle_thresholds(st)
    want, n_acc = api.score_rank(st, sel, MAX_K)
    assert 0 < n_acc < 200
    rc, full = _raw(ctx, sp, cs.scan_set, None, cs.map_set, None, cs.poses, sel, 200)
    assert rc == 0 and full.n_sel.value == n_acc == full.n_acc.value and full.untouched(start=n_acc, counts=False)
    assert np.array_equal(full.index[:n_acc], want) and np.array_equal(_u32(full.H[:n_acc]), _u32(H[want]).reshape(-1, 9))
    assert np.array_equal(_u32(full.b[:n_acc]), _u32(b[want])) and full.st[:n_acc].tobytes() == np.ascontiguousarray(st[want]).tobytes()
    for wanted in ((False, True, True), (True, False, True), (True, True, False), (False, False, False)):
        rc, out = _raw(ctx, sp, cs.scan_set, None, cs.map_set, None, cs.poses, sel, 200, want=wanted)
        assert rc == 0 and out.n_sel.value == n_acc and np.array_equal(out.index, full.index), wanted
        assert np.array_equal(_u32(out.H), _u32(full.H)) if wanted[0] else np.all(out.H == -7.0), wanted
        assert np.array_equal(_u32(out.b), _u32(full.b)) if wanted[1] else np.all(out.b == -7.0), wanted
        assert out.st.tobytes() == full.st.tobytes() if wanted[2] else np.all(out.st.view(np.uint32) == 0x5A5A5A5A), wanted


# ---- 8. argument errors ----------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx, cs):
    lib = ctx._lib
    sp = _slice(ctx)
    args = (ctx, sp, cs.scan_set, None, cs.map_set, None, cs.poses[:8])

    def refused(rc, out, text):
        assert rc == BAD_ARGUMENT and out.untouched(), text
        assert text in lib.lsm2d_last_error(ctx.handle).decode(), lib.lsm2d_last_error(ctx.handle)

    refused(*_raw(*args, EVERYTHING, 0), "score_select: k outside")
    refused(*_raw(*args, EVERYTHING, -3), "score_select: k outside")
    refused(*_raw(*args, EVERYTHING, MAX_K + 1), "score_select: k outside")
    refused(*_raw(*args, EVERYTHING, 4, null_select=True), "score_select: null argument")
    refused(*_raw(*args, EVERYTHING, 4, null_index=True), "score_select: null argument")
    s = EVERYTHING.struct(); out = _Out(4); poses = np.ascontiguousarray(cs.poses[:8])
    for n_sel, n_acc in ((None, C.byref(out.n_acc)), (C.byref(out.n_sel), None)):      # a NULL count pointer
        rc = lib.lsm2d_score_select(ctx.handle, C.byref(sp), cs.scan_set.handle, None, cs.map_set.handle, None, 8, _ptr(poses), C.byref(s), 4, _ptr(out.index),
                                    _ptr(out.H), _ptr(out.b), _ptr(out.st), n_sel, n_acc)
        refused(rc, out, "score_select: null argument")
    for fi, item in ((np.int32([0, 0, 1, 0, 0, 0, 0, 0]), 2), (np.int32([0, 0, 0, 0, 0, -1, 0, 0]), 5)):      # a cloud index out of range: the text names the item
        refused(*_raw(ctx, sp, cs.scan_set, fi, cs.map_set, None, cs.poses[:8], EVERYTHING, 4), "score_select: item %d" % item)
    refused(*_raw(ctx, sp, cs.scan_set, None, cs.map_set, None, None, EVERYTHING, 4, n=8), "score_select: null argument")      # NULL poses
    with pytest.raises(api.Lsm2dError):
        api.score_select(ctx, sp, cs.scan_set, cs.map_set, cs.poses[:8], EVERYTHING, MAX_K + 1)
    rc, out = _raw(*args, EVERYTHING, 4)      # ... and the call still works
    assert rc == 0 and out.n_sel.value == 4 and out.n_acc.value == 8


# ---- 9. score_batch is unchanged by calls to score_select -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_score_batch_returns_the_same_bytes_after_score_select(order_ctx, cs):
    ctx = order_ctx
    sp = _slice(ctx)
    raw = lambda r: (_u32(r[0]).tobytes(), _u32(r[1]).tobytes(), r[2].tobytes())
    before = raw(_batch_rows(ctx, sp, cs.scan_set, cs.map_set, cs.poses))
    big = cases.many_poses(cs, T + 9, seed=14)
    before_big = raw(_batch_rows(ctx, sp, cs.scan_set, cs.map_set, big))
    for poses, k in ((cs.poses, 5), (big, MAX_K), (cs.poses[:3], 1)):      # the shared scratch holds keys, indices and a selection behind the rows
        api.score_select(ctx, sp, cs.scan_set, cs.map_set, poses, EVERYTHING, k)
        assert raw(_batch_rows(ctx, sp, cs.scan_set, cs.map_set, cs.poses)) == before, (len(poses), k)
    assert raw(_batch_rows(ctx, sp, cs.scan_set, cs.map_set, big)) == before_big


# ---- 10. the relocalise helper ------------------------------------------------------------------------------------------------------------------------------------------
def test_relocalize_equals_the_two_entry_points_by_hand(ctx, cs):
    al = api.MultiAligner2D(ctx, max_iterations=8, min_num_inliers=10)
    finder = _finder(ctx, "proj")
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, robustifier=api.RobustifierCauchy(cases.TAU), min_num_correspondences=10))
    sp = al.param_slice_processors[0].slice_params()
    H, b, st = _batch_rows(ctx, sp, cs.scan_set, cs.map_set, cs.poses)
    sel = cases.middle_thresholds(st)
    two = api.CloudSet(ctx, np.ascontiguousarray(np.concatenate([cs.scan[:90], cs.scan])), np.int32([0, 90, 90 + len(cs.scan)]))
    fi = (np.arange(len(cs.poses)) % 2).astype(np.int32)
    for fixed, index_arg in ((cs.scan_set, None), (two, fi)):
        r = api.relocalize(al, fixed, cs.map_set, cs.poses, sel, 6, fixed_index=index_arg)
        index, _, _, sst, n_acc = api.score_select(ctx, sp, fixed, cs.map_set, cs.poses, sel, 6, fixed_index=index_arg)
        assert len(index) == min(6, n_acc) > 0 and np.array_equal(r.index, index) and r.n_accepted == n_acc and r.score_stats.tobytes() == sst.tobytes()
        hand = al.compute_batch([fixed], [cs.map_set], cs.poses[index], fixed_index=None if index_arg is None else index_arg[index][None, :], want_stats=True)
        assert np.array_equal(_u32(r.result.pose), _u32(hand.pose)) and np.array_equal(_u32(r.result.information), _u32(hand.information))
        assert np.array_equal(r.result.status, hand.status) and np.array_equal(r.result.iterations, hand.iterations)
        assert r.result.stats.tobytes() == hand.stats.tobytes()
        last = hand.last_stats()
        assert np.array_equal(r.accepted, (hand.status == 0) & np.all(cases.conditions(last, sel), axis=0))
        assert np.any(hand.status == 0) and np.any(_u32(hand.pose) != _u32(cs.poses[index]))      # the aligner ran
    r = api.relocalize(al, cs.scan_set, cs.map_set, cs.poses, NOTHING, 6)
    assert r.n_accepted == 0 and len(r.index) == 0 and len(r.result.pose) == 0 and len(r.accepted) == 0
