"""GPU tests of lsm2d_align_select / lsm2d_sweep_align_select (lsm2d_align_batch's alignment with its results kept on the device, then k_align_rows and the
selection's kernels on one row per candidate).  The call must return exactly what api.align_rank -- the verdict restated in numpy float32 / integer
arithmetic -- selects from the results of the same candidates, and for every selected candidate the bits lsm2d_align_batch returns.  The results come from
the CPU oracle (po.align per candidate: the sequential one for "sum_order" 1, its device-order mirror for the default order) where the batch is small, and
from aligner.compute_batch(..., want_stats=True) -- unchanged code, itself held to the oracle by the aligner's own tests -- on the same context everywhere
else.  No tolerance appears in this file.

Thresholds: align_select_cases.middle_thresholds of the Success candidates' last rows, and status_thresholds (taken from all candidates' rows: the ones under
which the status term alone rejects candidates -- test_align_select_abi.py says why the first set cannot show that)."""
import ctypes as C
import math

import numpy as np
import pytest

import align_select_cases as cases
from srrg2_laser_slam_2d_amd import api, synth
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT, AlignerParams

pytestmark = pytest.mark.gpu

T = api.SELECT_TILE        # entries a workgroup of k_select_tile sorts: where the selection takes another pass
MAX_K = api.SELECT_MAX_K
EVERYTHING = api.SelectParams(0, float("inf"), 0.0)
NOTHING = api.SelectParams(10 ** 9, 0.0, 2.0)
SMALL_COLS, SMALL_MAP, SMALL_ITS = 64, 300, 3


def _finder(ctx, kind, cols=cases.COLS):
    if kind == "proj":
        return api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, 30.0))
    return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=cases.MD, search="exact")


def _aligner(ctx, kind="proj", robust=True, iterations=cases.ITERATIONS, min_num_inliers=10, cols=cases.COLS):
    al = api.MultiAligner2D(ctx, max_iterations=iterations, min_num_inliers=min_num_inliers)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(_finder(ctx, kind, cols), robustifier=api.RobustifierCauchy(cases.TAU) if robust else None,
                                                                      min_num_correspondences=cases.MIN_CORR))
    return al


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check(got, pose, H, status, iterations, stats, sel, k, tag):
    """got = api.align_select's result; the arrays are the results of ALL candidates: the selection is align_rank's, the rows are theirs, bit for bit"""
    want, want_acc, want_suc = api.align_rank(status, iterations, stats, sel, k)
    print(tag, "k", k, "accepted", got.n_accepted, "success", got.n_success, "/", len(status), "selected", len(got.index), "expected", want_acc, want_suc, len(want))
    assert (got.n_accepted, got.n_success) == (want_acc, want_suc), tag
    assert got.index.dtype == np.int32 and np.array_equal(got.index, want), (tag, got.index[:16], want[:16])
    m = len(want)
    assert got.pose.shape == (m, 3) and got.information.shape == (m, 3, 3) and got.iterations.shape == (m,) and got.last_stats.shape == (m,)
    assert np.array_equal(_u32(got.pose), _u32(pose[want])) and np.array_equal(_u32(got.information), _u32(np.asarray(H).reshape(-1, 3, 3)[want])), tag
    assert np.array_equal(got.iterations, np.asarray(iterations)[want]), tag
    assert got.last_stats.tobytes() == np.ascontiguousarray(api.last_stats_rows(iterations, stats)[want]).tobytes(), tag
    return want, want_acc, want_suc


def _check_result(got, res, sel, k, tag):
    return _check(got, res.pose, res.information, res.status, res.iterations, res.stats, sel, k, tag)


@pytest.fixture(scope="module")
def cs(ctx):
    c = cases.make_cases()
    c.scan_set = api.CloudSet(ctx, c.scan)
    c.map_set = api.CloudSet(ctx, c.map)
    c.oracle = {}      # (kind, robust, device_order) -> (min_num_inliers, Results): computed once, shared, never changed
    return c


@pytest.fixture()
def order_ctx(ctx, request):
    ctx.set_option("sum_order", request.param)
    try:
        yield ctx
    finally:
        ctx.set_option("sum_order", 0)


def _oracle(po, c, kind, robust, device_order):
    key = (kind, robust, device_order)
    if key not in c.oracle:
        rb = po.ROBUST_CAUCHY if robust else po.ROBUST_NONE
        M = cases.middle_min_inliers(po, c, kind, rb, device_order)
        c.oracle[key] = (M, cases.oracle_results(po, c, kind, rb, device_order, M))
    return c.oracle[key]


# ---- 1. against the oracle, both orders ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust", [False, True], ids=["plain", "cauchy"])
@pytest.mark.parametrize("kind", ["proj", "nn"])
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_against_the_oracle(order_ctx, po, cs, kind, robust):
    ctx = order_ctx
    order = ctx.get_option("sum_order")
    M, r = _oracle(po, cs, kind, robust, 0 if order else 1)
    last = r.last(); ok = r.status == 0
    al = _aligner(ctx, kind, robust, min_num_inliers=M)
    if robust:
        assert all(np.any(r.status == s) for s in (0, 1, 2))
    for sel in (cases.middle_thresholds(last[ok]), cases.status_thresholds(last[r.iterations >= 1]), EVERYTHING):
        for k in (64, 7):
            got = api.align_select(al, [cs.scan_set], [cs.map_set], cs.poses, sel, k)
            want, n_acc, n_suc = _check(got, r.pose, r.H, r.status, r.iterations, r.stats, sel, k, (kind, robust, order, sel))
            assert 0 < n_acc <= n_suc and len(want) == min(k, n_acc)
            if robust and sel is not EVERYTHING:
                assert n_acc < n_suc < len(cs.poses)
    assert ctx.last_kernel_ms() > 0.0


# ---- 2. bitwise against compute_batch across the launch forms ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(ctx, cs):
    """64-beam scan, 300-point map, 3 iterations: milliseconds per call.  The start poses are the workload's (the same world and true pose: the same seed),
    repeated cyclically; min_num_inliers is the median of the device's own last-row inlier counts."""
    class S:
        pass
    s = S()
    wl = synth.make_workload(1, SMALL_MAP, seed=5, n_beams=SMALL_COLS, map_noise=cases.NOISE, scan_noise=cases.NOISE)
    assert np.array_equal(wl.x0[0], cs.wl.x0[0])
    s.scan_set = api.CloudSet(ctx, np.ascontiguousarray(wl.scan_points)); s.map_set = api.CloudSet(ctx, np.ascontiguousarray(wl.map_points))
    first = _aligner(ctx, iterations=SMALL_ITS, min_num_inliers=0, cols=SMALL_COLS).compute_batch([s.scan_set], [s.map_set], cs.poses, want_stats=True)
    n_in = first.last_stats()["n_inliers"][first.status == 0]
    s.M = int(np.sort(n_in)[len(n_in) // 2])
    s.aligner = lambda **kw: _aligner(ctx, iterations=SMALL_ITS, min_num_inliers=s.M, cols=SMALL_COLS, **kw)
    return s


def _both(al, s, poses, sel, ks, tag, **kw):
    """compute_batch with statistics, then align_select for every k: the same context, the same candidates"""
    res = al.compute_batch([s.scan_set], [s.map_set], poses, want_stats=True, **kw)
    ok = res.status == 0
    sels = [EVERYTHING] if sel is None else [sel]
    if sel is None and np.any(ok):
        sels.append(cases.middle_thresholds(res.last_stats()[ok]))
    for se in sels:
        for k in ks:
            got = api.align_select(al, [s.scan_set], [s.map_set], poses, se, k, **kw)
            _check_result(got, res, se, k, (tag, len(poses)))
    return res


@pytest.mark.parametrize("n", [1, 2, 192, 193, 256, 257, 1024, 1025, 1049, T - 1, T, T + 1, 2 * T + 1])
def test_bitwise_against_compute_batch(ctx, cs, small, n):
    """n crosses the zero-copy and latency-kernel limit (256), the split-path limit (192), the packed and narrow widths (1025, 1049), the single-tile launch
    (T) and one and two tile passes"""
    poses = cases.cyclic(cs, n)
    res = _both(small.aligner(), small, poses, None, sorted({1, 2, 7, min(n, MAX_K), MAX_K}), "forms")
    if n >= 192:
        assert all(np.any(res.status == s) for s in (0, 1, 2))


@pytest.mark.parametrize("options", [dict(align_path=0), dict(align_path=1), dict(align_path=2), dict(align_path=3), dict(fast_forward=0), dict(fast_forward=2),
                                     dict(inlier_only_runs=1)], ids=lambda o: "%s=%d" % next(iter(o.items())))
def test_bitwise_under_every_path_and_option(ctx, cs, small, options):
    n = 300
    al = small.aligner()
    if options.get("inlier_only_runs"):
        al.param_enable_inlier_only_runs = True      # two phases: the last row's index moves past max_iterations
    defaults = dict(align_path=0, fast_forward=2)
    try:
        for key, v in options.items():
            if key in defaults:
                ctx.set_option(key, v)
        res = _both(al, small, cases.cyclic(cs, n), None, (7, MAX_K), options)
        if options.get("inlier_only_runs"):
            assert res.stats.shape[1] == 2 * SMALL_ITS and np.any(res.iterations > SMALL_ITS)
        if "align_path" in options and options["align_path"]:
            assert ctx.get_option("last_align_path") == options["align_path"]
    finally:
        for key, v in defaults.items():
            ctx.set_option(key, v)


# ---- 3. ordering ------------------------------------------------------------------------------------------------------------------------------------------------
def test_ties_come_out_in_ascending_index(ctx, cs, small):
    al = small.aligner()
    n = T + 700
    poses = cases.cyclic(cs, n)
    res0 = al.compute_batch([small.scan_set], [small.map_set], poses, want_stats=True)
    best = int(api.align_rank(res0.status, res0.iterations, res0.stats, EVERYTHING, 1)[0][0])
    same = np.arange(T - 301, T + 299, 2)      # 300 copies of the best candidate's start pose, every other candidate across the tile boundary
    poses[same] = poses[best]
    res = al.compute_batch([small.scan_set], [small.map_set], poses, want_stats=True)
    last = res.last_stats()
    tied = np.flatnonzero((res.status == 0) & (last["n_inliers"] == last["n_inliers"][best]) & (_u32(last["chi_inliers"]) == _u32(last["chi_inliers"])[best]))
    assert set(same.tolist()) <= set(tied.tolist()) and np.any(tied < T) and np.any(tied >= T)      # equal keys on either side of the tile boundary
    for k in (MAX_K, 100):
        got = api.align_select(al, [small.scan_set], [small.map_set], poses, EVERYTHING, k)
        _check_result(got, res, EVERYTHING, k, "ties")
        m = min(k, len(tied))
        assert np.array_equal(got.index[:m], tied[:m])      # the copies lead the ranking, by index


# ---- 4. thresholds at equality, counts -----------------------------------------------------------------------------------------------------------------------------
def test_thresholds_at_equality_and_counts(ctx, po, cs):
    M, r = _oracle(po, cs, "proj", True, 1)
    al = _aligner(ctx, "proj", True, min_num_inliers=M)
    last = r.last(); ok = r.status == 0
    per_inlier, ratio = cases.sc.quotients(last)
    mid = [int(i) for i in api.align_rank(r.status, r.iterations, r.stats, cases.middle_thresholds(last[ok]), MAX_K)[0] if last["n_outliers"][i] > 0 and per_inlier[i] > 0]
    j = mid[len(mid) // 2]      # an accepted candidate from the middle of the ranking, with inliers and outliers
    at = (int(last["n_inliers"][j]), float(per_inlier[j]), float(ratio[j]))
    args = ([cs.scan_set], [cs.map_set], cs.poses)
    rows = (r.pose, r.H, r.status, r.iterations, r.stats)
    for sel in (api.SelectParams(*at), api.SelectParams(at[0], float("inf"), 0.0), api.SelectParams(0, at[1], 0.0), api.SelectParams(0, float("inf"), at[2])):
        got = api.align_select(al, *args, sel, MAX_K)
        _, n_acc, n_suc = _check(got, *rows, sel, MAX_K, ("equality", sel))
        assert j in got.index.tolist() and n_acc < n_suc, sel      # >= and <= at equality accept; a Success candidate is rejected
    tight = (api.SelectParams(at[0] + 1, at[1], at[2]), api.SelectParams(at[0], float(np.nextafter(np.float32(at[1]), np.float32(0.0))), at[2]),
             api.SelectParams(at[0], at[1], float(np.nextafter(np.float32(at[2]), np.float32(2.0)))))
    for sel in tight:      # one ulp to the wrong side of each threshold and the candidate is gone
        got = api.align_select(al, *args, sel, MAX_K)
        _check(got, *rows, sel, MAX_K, ("one ulp off", sel))
        assert j not in got.index.tolist(), sel
    # {0, +Inf, 0} accepts exactly the Success candidates that started an iteration
    got = api.align_select(al, *args, EVERYTHING, MAX_K)
    _check(got, *rows, EVERYTHING, MAX_K, "everything")
    assert got.n_accepted == got.n_success == int((ok & (r.iterations >= 1)).sum()) < len(cs.poses)
    assert set(got.index.tolist()) == set(np.flatnonzero(ok).tolist())
    # ... and an aligner that starts no iteration: whatever its statuses are, no candidate is accepted
    al0 = _aligner(ctx, "proj", True, iterations=0)
    res0 = al0.compute_batch(*args, want_stats=True)
    got0 = api.align_select(al0, *args, EVERYTHING, 8)
    assert np.all(res0.iterations == 0)
    assert (got0.n_accepted, got0.n_success, len(got0.index)) == (0, int((res0.status == 0).sum()), 0)


# ---- 5. outputs beyond n_selected, NULL outputs, nothing accepted ------------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _Out:
    def __init__(self, k):
        m = max(min(k, MAX_K + 1), 1)
        self.index = np.full(m, -7, np.int32); self.pose = np.full((m, 3), -7.0, np.float32); self.H = np.full((m, 9), -7.0, np.float32)
        self.its = np.full(m, -7, np.int32); self.st = np.full(m * 7, 0x5A5A5A5A, np.uint32).view(api.STATS_DTYPE)
        self.n_sel = C.c_int32(-7); self.n_acc = C.c_int32(-7); self.n_suc = C.c_int32(-7)

    def untouched(self, start=0, counts=True):
        return bool(np.all(self.index[start:] == -7) and np.all(self.pose[start:] == -7.0) and np.all(self.H[start:] == -7.0) and np.all(self.its[start:] == -7) and
                    np.all(self.st[start:].view(np.uint32) == 0x5A5A5A5A) and
                    (not counts or (self.n_sel.value == -7 and self.n_acc.value == -7 and self.n_suc.value == -7)))


def _raw(al, fixed, moving, poses, sel, k, want=(True, True, True, True), null=(), fixed_index=None, n=None, n_slices=None):
    """lsm2d_align_select through ctypes: want = (out_H, out_iterations, out_last_stats, out_n_success); null names the required pointers to pass as NULL"""
    ctx = al._ctx
    bd, keep = al._batch([fixed], [moving], poses, None, fixed_index, None)
    if n is not None:
        bd.n_alignments = n
    if n_slices is not None:
        bd.n_slices = n_slices
    ap = al._aligner_params()
    out = _Out(k)
    s = sel.struct()
    p = lambda name, v: None if name in null else v
    rc = ctx._lib.lsm2d_align_select(p("ctx", ctx.handle), p("aligner", C.byref(ap)), p("batch", C.byref(bd)), p("select", C.byref(s)), k, p("index", _ptr(out.index)),
                                     p("pose", _ptr(out.pose)), _ptr(out.H) if want[0] else None, _ptr(out.its) if want[1] else None,
                                     _ptr(out.st) if want[2] else None, p("n_sel", C.byref(out.n_sel)), p("n_acc", C.byref(out.n_acc)),
                                     C.byref(out.n_suc) if want[3] else None)
    return rc, out


def test_outputs_beyond_n_selected_are_untouched_and_may_be_null(ctx, po, cs):
    M, r = _oracle(po, cs, "proj", True, 1)
    al = _aligner(ctx, "proj", True, min_num_inliers=M)
    last = r.last()
    sel = cases.middle_thresholds(last[r.status == 0])
    want, n_acc, n_suc = api.align_rank(r.status, r.iterations, r.stats, sel, MAX_K)
    assert 0 < n_acc < 200
    rc, full = _raw(al, cs.scan_set, cs.map_set, cs.poses, sel, 200)
    assert rc == 0 and (full.n_sel.value, full.n_acc.value, full.n_suc.value) == (n_acc, n_acc, n_suc) and full.untouched(start=n_acc, counts=False)
    assert np.array_equal(full.index[:n_acc], want) and np.array_equal(_u32(full.pose[:n_acc]), _u32(r.pose[want]))
    assert np.array_equal(_u32(full.H[:n_acc]), _u32(r.H[want]).reshape(-1, 9)) and np.array_equal(full.its[:n_acc], r.iterations[want])
    assert full.st[:n_acc].tobytes() == np.ascontiguousarray(last[want]).tobytes()
    for wanted in ((False, True, True, True), (True, False, True, True), (True, True, False, True), (True, True, True, False), (False, False, False, False)):
        rc, out = _raw(al, cs.scan_set, cs.map_set, cs.poses, sel, 200, want=wanted)
        assert rc == 0 and out.n_sel.value == n_acc and np.array_equal(out.index, full.index) and np.array_equal(_u32(out.pose), _u32(full.pose)), wanted
        assert np.array_equal(_u32(out.H), _u32(full.H)) if wanted[0] else np.all(out.H == -7.0), wanted
        assert np.array_equal(out.its, full.its) if wanted[1] else np.all(out.its == -7), wanted
        assert out.st.tobytes() == full.st.tobytes() if wanted[2] else np.all(out.st.view(np.uint32) == 0x5A5A5A5A), wanted
        assert out.n_suc.value == (n_suc if wanted[3] else -7), wanted
    # nothing accepted: the counts are right, no row is touched
    rc, out = _raw(al, cs.scan_set, cs.map_set, cs.poses, NOTHING, 64)
    assert rc == 0 and (out.n_sel.value, out.n_acc.value, out.n_suc.value) == (0, 0, n_suc) and out.untouched(counts=False)
    got = api.align_select(al, [cs.scan_set], [cs.map_set], cs.poses, NOTHING, 64)
    assert got.index.shape == (0,) and got.pose.shape == (0, 3) and got.information.shape == (0, 3, 3) and got.last_stats.shape == (0,)
    # n_alignments == 0: all counts are set to 0, nothing else is written
    rc, out = _raw(al, cs.scan_set, cs.map_set, np.zeros((0, 3), np.float32), EVERYTHING, 64)
    assert rc == 0 and (out.n_sel.value, out.n_acc.value, out.n_suc.value) == (0, 0, 0) and out.untouched(counts=False)


# ---- 6. refusals, lanes ----------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(ctx, cs):
    lib = ctx._lib
    al = _aligner(ctx)
    args = (al, cs.scan_set, cs.map_set, cs.poses[:8])

    def refused(rc, out, text, handle=ctx.handle):
        assert rc == BAD_ARGUMENT and out.untouched(), text
        assert text in lib.lsm2d_last_error(handle).decode(), lib.lsm2d_last_error(handle)

    for k in (0, -3, MAX_K + 1):
        refused(*_raw(*args, EVERYTHING, k), "align_select: k outside")
    for name in ("aligner", "batch", "select", "index", "pose", "n_sel", "n_acc"):
        refused(*_raw(*args, EVERYTHING, 4, null=(name,)), "align_select: null argument")
    refused(*_raw(*args, EVERYTHING, 4, null=("ctx",)), "align_select: null argument", handle=None)
    refused(*_raw(*args, EVERYTHING, 4, n_slices=0), "align_batch: bad batch descriptor")      # lsm2d_align_batch's own refusals
    refused(*_raw(*args, EVERYTHING, 4, n=-1), "align_batch: bad batch descriptor")
    refused(*_raw(*args, EVERYTHING, 4, n_slices=0, n=0), "align_batch: bad batch descriptor")      # an empty batch's descriptor is checked too
    refused(*_raw(*args, EVERYTHING, 4, fixed_index=np.int32([[0, 0, 1, 0, 0, 0, 0, 0]])), "align_batch: fixed_index out of range")
    other = api.Context(0)
    try:
        foreign = api.CloudSet(other, cs.scan)
        refused(*_raw(al, foreign, cs.map_set, cs.poses[:8], EVERYTHING, 4), "align_batch: cloud set missing or from another context")
        del foreign
    finally:
        other.close()
    with pytest.raises(api.Lsm2dError):
        api.align_select(al, [cs.scan_set], [cs.map_set], cs.poses[:8], EVERYTHING, MAX_K + 1)
    rc, out = _raw(*args, EVERYTHING, 4)      # ... and the call still works
    assert rc == 0 and out.n_sel.value == min(4, out.n_acc.value) and out.n_acc.value <= out.n_suc.value <= 8


def test_one_batch_in_flight_works_two_are_refused(ctx, po, cs):
    M, r = _oracle(po, cs, "proj", True, 1)
    al = _aligner(ctx, "proj", True, min_num_inliers=M)
    sel = cases.middle_thresholds(r.last()[r.status == 0])
    rows = (r.pose, r.H, r.status, r.iterations, r.stats)
    a = al.prepare_batch([cs.scan_set], [cs.map_set], cs.poses, want_stats=True)
    b = al.prepare_batch([cs.scan_set], [cs.map_set], cs.poses[::-1].copy())
    a.begin()
    try:
        got = api.align_select(al, [cs.scan_set], [cs.map_set], cs.poses, sel, 64)      # the free lane
        _check(got, *rows, sel, 64, "one in flight")
        b.begin()
        try:
            rc, out = _raw(al, cs.scan_set, cs.map_set, cs.poses, sel, 64)
            assert rc == BAD_ARGUMENT and out.untouched() and "two batches are in flight" in ctx._lib.lsm2d_last_error(ctx.handle).decode()
            rc, out = _raw(al, cs.scan_set, cs.map_set, np.zeros((0, 3), np.float32), sel, 64)      # an empty batch is a no-op only on a context that could run it
            assert rc == BAD_ARGUMENT and out.untouched()
        finally:
            ra = a.wait(copy=True)
            a = None
            b.wait(copy=True)
    finally:
        if a is not None:
            ra = a.wait(copy=True)
    assert np.array_equal(_u32(ra.pose), _u32(r.pose)) and np.array_equal(ra.status, r.status)      # the batch in flight was not disturbed
    got = api.align_select(al, [cs.scan_set], [cs.map_set], cs.poses, sel, 64)
    _check(got, *rows, sel, 64, "after both")


# ---- 7. state: lsm2d_align_batch is unchanged by calls to lsm2d_align_select ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_align_batch_returns_the_same_bytes_after_align_select(order_ctx, cs, small):
    ctx = order_ctx
    al = small.aligner()
    raw = lambda res: (_u32(res.pose).tobytes(), _u32(res.information).tobytes(), res.status.tobytes(), res.iterations.tobytes(), res.stats.tobytes())
    run = lambda poses: raw(al.compute_batch([small.scan_set], [small.map_set], poses, want_stats=True))
    big = cases.cyclic(cs, T + 9)
    before, before_big = run(cs.poses), run(big)
    cand = [ctx.get_option(key) for key in ("last_cand_builds", "last_cand_iterations", "last_cand_overflows")]
    for poses, k in ((cs.poses, 5), (big, MAX_K), (cs.poses[:3], 1)):      # the shared scratch holds rows, keys, indices and a selection behind the results
        api.align_select(al, [small.scan_set], [small.map_set], poses, EVERYTHING, k)
        assert [ctx.get_option(key) for key in ("last_cand_builds", "last_cand_iterations", "last_cand_overflows")] == cand      # the previous call's values
        assert run(cs.poses) == before, (len(poses), k)
        cand = [ctx.get_option(key) for key in ("last_cand_builds", "last_cand_iterations", "last_cand_overflows")]
    assert run(big) == before_big


def test_last_kernel_ms_covers_launch_and_selection(ctx, cs, small):
    """documented in include/lsm2d.h: the bracket is begun in front of the aligner's launch and ended behind the selection, so it is at least the launch"""
    al = small.aligner()
    poses = cases.cyclic(cs, 2 * T + 1)
    res = al.compute_batch([small.scan_set], [small.map_set], poses, want_stats=True)
    got = api.align_select(al, [small.scan_set], [small.map_set], poses, EVERYTHING, MAX_K)
    assert res.kernel_ms > 0.0 and got.kernel_ms > 0.0 and got.kernel_ms == ctx.last_kernel_ms()
    assert got.kernel_ms > 0.5 * res.kernel_ms      # (the launch is in it: a selection alone of 4097 rows is a small fraction of 4097 alignments)
    ctx.set_option("kernel_timing", 0)
    try:
        assert api.align_select(al, [small.scan_set], [small.map_set], poses, EVERYTHING, 4).n_accepted == got.n_accepted
    finally:
        ctx.set_option("kernel_timing", 1)


# ---- 8. the sweep ------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]], ids=["G1", "G2", "G3"])
def test_sweep_equals_the_single_device_call(ctx, po, cs, devices):
    M, r = _oracle(po, cs, "proj", True, 1)
    al = _aligner(ctx, "proj", True, min_num_inliers=M)
    last = r.last()
    lib = ctx._lib
    sw = C.c_void_p()
    assert lib.lsm2d_sweep_create(_ptr(np.int32(devices)), len(devices), C.byref(sw)) == 0
    try:
        assert lib.lsm2d_sweep_set_map(sw, _ptr(cs.map), len(cs.map)) == 0
        assert lib.lsm2d_sweep_set_scans(sw, _ptr(cs.scan), _ptr(np.int32([0, len(cs.scan)])), 1) == 0
        ap = al._aligner_params(); sp = al.param_slice_processors[0].slice_params()
        poses = np.ascontiguousarray(cs.poses)
        for sel, k in ((cases.middle_thresholds(last[r.status == 0]), 64), (cases.status_thresholds(last[r.iterations >= 1]), 7), (EVERYTHING, MAX_K), (NOTHING, 5)):
            one = api.align_select(al, [cs.scan_set], [cs.map_set], poses, sel, k)
            out = _Out(k); s = sel.struct()
            rc = lib.lsm2d_sweep_align_select(sw, C.byref(ap), C.byref(sp), len(poses), None, _ptr(poses), C.byref(s), k, _ptr(out.index), _ptr(out.pose), _ptr(out.H),
                                              _ptr(out.its), _ptr(out.st), C.byref(out.n_sel), C.byref(out.n_acc), C.byref(out.n_suc))
            assert rc == 0, lib.lsm2d_sweep_last_error(sw)
            m = len(one.index)
            assert (out.n_sel.value, out.n_acc.value, out.n_suc.value) == (m, one.n_accepted, one.n_success) and out.untouched(start=m, counts=False), (devices, sel)
            assert np.array_equal(out.index[:m], one.index) and np.array_equal(_u32(out.pose[:m]), _u32(one.pose)), (devices, sel)
            assert np.array_equal(_u32(out.H[:m]).reshape(-1, 3, 3), _u32(one.information)) and np.array_equal(out.its[:m], one.iterations)
            assert out.st[:m].tobytes() == one.last_stats.tobytes()
        out = _Out(4); s = EVERYTHING.struct()      # refusals write nothing
        rc = lib.lsm2d_sweep_align_select(sw, C.byref(ap), C.byref(sp), len(poses), None, _ptr(poses), C.byref(s), MAX_K + 1, _ptr(out.index), _ptr(out.pose),
                                          _ptr(out.H), _ptr(out.its), _ptr(out.st), C.byref(out.n_sel), C.byref(out.n_acc), C.byref(out.n_suc))
        assert rc == BAD_ARGUMENT and out.untouched()
    finally:
        lib.lsm2d_sweep_destroy(sw)
