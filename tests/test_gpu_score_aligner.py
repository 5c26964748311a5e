"""GPU tests of lsm2d_score_aligner_batch / lsm2d_score_aligner_select: pose hypotheses scored against a whole aligner -- its slices with their sensor
offsets and skip thresholds, the optional prior -- and ranked on the device.

Yardsticks (tests/score_aligner_cases.py; the combination itself is pinned against the sequential oracle's align(max_iterations=1) on the CPU by
tests/test_score_aligner_abi.py): with "sum_order" 1 an item IS po.align(max_iterations=1) -- H, first statistics row, digest, status -- and
po.solve_update on the device's H and b gives its pose; in the default order it is the numpy combination over po.find + po.linearize_device_order per
slice.  Larger batches are held to the parent's route: api.score_batch per slice at the host-composed effective pose -- unchanged code, itself held to the
oracle by test_gpu_score_batch.py -- combined in numpy.  Everything is compared bit for bit: no tolerance appears in this file."""
import ctypes as C
import math

import numpy as np
import pytest

import fuzz_cases
import score_aligner_cases as cases
from srrg2_laser_slam_2d_amd import api
from srrg2_laser_slam_2d_amd._capi import BAD_ARGUMENT, CAPACITY_EXCEEDED

pytestmark = pytest.mark.gpu

EVERYTHING = api.SelectParams(0, float("inf"), 0.0)
u32 = cases.u32


@pytest.fixture(scope="module")
def cs(ctx):
    c = cases.make_inputs()
    c.fixed_sets = []
    for s in range(4):
        off = np.zeros(c.n + 1, np.int32); off[1:] = np.cumsum([len(a) for a in c.fixed[s]])
        c.fixed_sets.append(api.CloudSet(ctx, np.concatenate(c.fixed[s]), off))
    c.moving_sets = [api.CloudSet(ctx, m) for m in c.moving]
    c.oracle_rows = {}      # (order, slice, item) -> the oracle's row at the item's effective pose: computed once, shared
    return c


@pytest.fixture()
def order_ctx(ctx, request):
    ctx.set_option("sum_order", request.param)
    try:
        yield ctx
    finally:
        ctx.set_option("sum_order", 0)


def _finder(ctx, s):
    kind, cols, md, _ = cases.SLICES[s]
    if kind == "proj":
        return api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, 30.0))
    if kind == "nn":
        return api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=md, search="exact")
    return api.CorrespondenceFinderNN2D(ctx, max_distance_m=md)


def _aligner(ctx, which, min_corr=None, sensors=None):
    """an aligner over the slices `which` (indices into cases.SLICES), in that order"""
    al = api.MultiAligner2D(ctx, max_iterations=1, min_num_inliers=10)
    for j, s in enumerate(which):
        tau = cases.SLICES[s][3]
        mc = cases.MIN_CORR if min_corr is None else min_corr[j]
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(
            _finder(ctx, s), sensor_in_robot=cases.S_OFF[s] if sensors is None else sensors[j], robustifier=None if tau is None else api.RobustifierCauchy(tau),
            min_num_correspondences=int(mc)))
    return al


def _oracle_rows(po, cs, order, which, i):
    rows = []
    for j, s in enumerate(which):
        key = (order, s, j, i)
        if key not in cs.oracle_rows:
            sp = fuzz_cases.oracle_slice(po, _aligner(None, [s]).param_slice_processors[0].slice_params())
            Xe = cases.effective_pose(po, cases.S_OFF[s], cs.poses[i])
            cs.oracle_rows[key] = cases.oracle_row(po, sp, j, cs.fixed[s][i], cs.moving[s], Xe, order)
        rows.append(cs.oracle_rows[key])
    return rows


def _assert_item(got, i, want, tag):
    """got = api.score_aligner's return; want = cases.combine's dict for item i"""
    H, b, st, active = got
    g = st[i]
    assert int(active[i]) == want["active"], (tag, i, int(active[i]), want["active"])
    assert (int(g["n_correspondences"]), int(g["n_inliers"]), int(g["n_outliers"])) == (want["n_corr"], want["n_in"], want["n_out"]), (tag, i, g, want)
    assert (int(g["pair_digest_hi"]) << 32 | int(g["pair_digest_lo"])) == want["digest"], (tag, i, "digest")
    assert u32(g["chi_inliers"]) == u32(want["chi_in"]) and u32(g["chi_outliers"]) == u32(want["chi_out"]), (tag, i, "chi")
    assert np.array_equal(u32(H[i]), u32(want["H"])), (tag, i, "H", H[i], want["H"])
    assert np.array_equal(u32(b[i]), u32(want["b"])), (tag, i, "b", b[i], want["b"])


def _assert_item_is_po_align(po, got, i, want, X, tag):
    """"sum_order" 1: the item is the sequential oracle's align(max_iterations=1)"""
    H, b, st, active = got
    o = want["stats"][0]; g = st[i]
    assert (int(g["n_correspondences"]), int(g["n_inliers"]), int(g["n_outliers"])) == (o.n_corr, o.n_in, o.n_out), (tag, i)
    assert u32(g["chi_inliers"]) == u32(o.chi_in) and u32(g["chi_outliers"]) == u32(o.chi_out), (tag, i)
    assert (int(g["pair_digest_hi"]) << 32 | int(g["pair_digest_lo"])) == o.pair_digest, (tag, i)
    if want["status"] == po.NOT_ENOUGH_CORRESPONDENCES:
        assert int(active[i]) == 0 and not H[i].any() and not b[i].any(), (tag, i)
        return
    assert int(active[i]) > 0 and np.array_equal(u32(H[i]), u32(want["H"])), (tag, i, H[i], want["H"])
    _, pose, _ = po.solve_update(H[i], b[i], X, 0.0)
    assert np.array_equal(u32(pose), u32(want["pose"])), (tag, i, pose, want["pose"])


def _po_align(po, cs, which, i, min_corr=None, prior=None):
    sl = []
    for j, s in enumerate(which):
        sp = fuzz_cases.oracle_slice(po, _aligner(None, [s], None if min_corr is None else [min_corr[j]]).param_slice_processors[0].slice_params())
        sl.append(sp)
    ap = po.aligner_params(1, prior_z=None if prior is None else prior[0], prior_omega=None if prior is None else prior[1])
    return po.align(ap, sl, [cs.fixed[s][i] for s in which], [cs.moving[s] for s in which], cs.poses[i])


def _sets(cs, which):
    return [cs.fixed_sets[s] for s in which], [cs.moving_sets[s] for s in which]


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [1, 2, 3, 4])
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_against_the_oracle(order_ctx, po, cs, ns):
    ctx = order_ctx; order = ctx.get_option("sum_order")
    which = list(range(ns))
    fx, mv = _sets(cs, which)
    got = api.score_aligner(_aligner(ctx, which), fx, mv, cs.poses)
    assert got[0].shape == (cs.n, 3, 3) and got[1].shape == (cs.n, 3) and got[2].dtype == api.STATS_DTYPE and got[3].dtype == np.int32
    for i in range(cs.n):
        want = cases.combine(po, _oracle_rows(po, cs, order, which, i), [cases.MIN_CORR] * ns, cs.poses[i])
        assert want["active"] == ns
        _assert_item(got, i, want, ("oracle rows", order, ns))
        if order:
            r = _po_align(po, cs, which, i)
            assert r["status"] == 0
            _assert_item_is_po_align(po, got, i, r, cs.poses[i], ("po.align", ns))
    assert ctx.last_kernel_ms() > 0.0      # "kernel_timing": the last launch group of the last slice, the combination


# ---- 2. equal to the parent's route ---------------------------------------------------------------------------------------------------------------------------------
def _parent_rows(ctx, po, al, fx, mv, poses, fixed_index=None, moving_index=None):
    """per slice j and item i: api.score_batch at the host-composed effective pose, its digest re-salted with the slice index (the pairs behind the re-salted
    digest are the batch finder's own: finder.compute_batch at the same poses)"""
    rows = []
    for j, spr in enumerate(al.param_slice_processors):
        sp = spr.slice_params()
        Xe = np.stack([cases.effective_pose(po, tuple(sp.sensor_in_robot), X) for X in poses])
        fi = None if fixed_index is None else fixed_index[j]; mi = None if moving_index is None else moving_index[j]
        H, b, st = api.score_batch(ctx, sp, fx[j], mv[j], Xe, fi, mi)
        if j == 0:
            dig = [s_.pair_digest for s_ in st]
        else:
            pairs = spr.param_finder.compute_batch(fx[j], mv[j], Xe, fixed_index=fi, moving_index=mi)
            assert [po.pair_digest(p, 0) for p in pairs] == [s_.pair_digest for s_ in st]
            dig = [po.pair_digest(p, j) for p in pairs]
        rows.append([(H[i], b[i], st[i].n_correspondences, st[i].n_inliers, st[i].n_outliers, st[i].chi_inliers, st[i].chi_outliers, dig[i]) for i in range(len(poses))])
    return rows


def _assert_parents_route(ctx, po, al, fx, mv, poses, priors=None, fixed_index=None, moving_index=None, tag=""):
    got = api.score_aligner(al, fx, mv, poses, priors, fixed_index, moving_index)
    rows = _parent_rows(ctx, po, al, fx, mv, poses, fixed_index, moving_index)
    mc = [spr.param_min_num_correspondences for spr in al.param_slice_processors]
    for i in range(len(poses)):
        want = cases.combine(po, [r[i] for r in rows], mc, poses[i], None if priors is None else priors[i])
        _assert_item(got, i, want, tag)
    return got


@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_equal_to_the_parents_route(order_ctx, po, cs):
    ctx = order_ctx
    for s in range(4):      # every slice's own contribution: the slice alone (salt 0), score_batch's bits with -0 turned +0
        fx, mv = _sets(cs, [s])
        al = _aligner(ctx, [s])
        got = _assert_parents_route(ctx, po, al, fx, mv, cs.poses, tag=("alone", s))
        sp = al.param_slice_processors[0].slice_params()
        Xe = np.stack([cases.effective_pose(po, cases.S_OFF[s], X) for X in cs.poses])
        H, b, st = api.score_batch(ctx, sp, fx[0], mv[0], Xe)
        assert np.array_equal(u32(got[0]), u32(H + np.float32(0.0))) and np.array_equal(u32(got[1]), u32(b + np.float32(0.0)))
        assert got[2].tobytes() == api._stats_array(st).tobytes() and np.all(got[3] == 1)
    which = [0, 1, 2, 3]
    fx, mv = _sets(cs, which)
    _assert_parents_route(ctx, po, _aligner(ctx, which), fx, mv, cs.poses, tag="four slices")
    which = [3, 2, 1]      # another order: the salts follow the slice index, not the finder
    fx, mv = _sets(cs, which)
    _assert_parents_route(ctx, po, _aligner(ctx, which), fx, mv, cs.poses, tag="reordered")


# ---- 3. the skip rule -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_skip_rule(order_ctx, po, cs):
    ctx = order_ctx; order = ctx.get_option("sum_order")
    which = [0, 1, 2]; i0 = 1
    fx, mv = _sets(cs, which)
    counts = [r[2] for r in _oracle_rows(po, cs, order, which, i0)]
    priors = [cases.asym_prior(X, seed=7) for X in cs.poses]
    for s in range(3):
        for delta, active in ((0, 2), (-1, 3)):      # a threshold equal to the slice's own pair count skips it; one less keeps it
            mc = [cases.MIN_CORR] * 3; mc[s] = counts[s] + delta
            got = api.score_aligner(_aligner(ctx, which, mc), fx, mv, cs.poses, priors)
            for i in range(cs.n):
                want = cases.combine(po, _oracle_rows(po, cs, order, which, i), mc, cs.poses[i], priors[i])
                _assert_item(got, i, want, ("skip", s, delta))
            assert int(got[3][i0]) == active and int(got[2][i0]["n_correspondences"]) == sum(counts)      # the skipped slice's pairs are still counted
            if order:
                _assert_item_is_po_align(po, got, i0, _po_align(po, cs, which, i0, mc, priors[i0]), cs.poses[i0], ("skip, po.align", s, delta))
    # all slices skipped: zeros, active 0, no prior; counts and digest still reported
    mc = [100000] * 3
    got = api.score_aligner(_aligner(ctx, which, mc), fx, mv, cs.poses, priors)
    for i in range(cs.n):
        want = cases.combine(po, _oracle_rows(po, cs, order, which, i), mc, cs.poses[i], priors[i])
        assert want["active"] == 0 and want["n_corr"] > 900 and want["digest"] != 0
        _assert_item(got, i, want, "all skipped")
        assert not got[0][i].any() and not got[1][i].any() and np.all(u32(got[0][i]) == 0) and int(got[2][i]["n_inliers"]) == 0
    if order:
        r = _po_align(po, cs, which, i0, mc, priors[i0])
        assert r["status"] == po.NOT_ENOUGH_CORRESPONDENCES
        _assert_item_is_po_align(po, got, i0, r, cs.poses[i0], "all skipped, po.align")


# ---- 4. the prior ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_prior(order_ctx, po, cs):
    ctx = order_ctx; order = ctx.get_option("sum_order")
    which = [0, 1, 2]
    fx, mv = _sets(cs, which)
    priors = [cases.asym_prior(X, seed=i) for i, X in enumerate(cs.poses)]
    assert all(om[0, 2] != om[2, 0] for _, om in priors)
    al = _aligner(ctx, which)
    got = api.score_aligner(al, fx, mv, cs.poses, priors)
    plain = api.score_aligner(al, fx, mv, cs.poses)
    for i in range(cs.n):
        want = cases.combine(po, _oracle_rows(po, cs, order, which, i), [cases.MIN_CORR] * 3, cs.poses[i], priors[i])
        _assert_item(got, i, want, ("prior", order))
        assert not np.array_equal(got[0][i], plain[0][i]) and not np.array_equal(got[0][i], got[0][i].T)      # it is in, asymmetric as given
        assert got[2][i].tobytes() == plain[2][i].tobytes()
        if order:
            _assert_item_is_po_align(po, got, i, _po_align(po, cs, which, i, None, priors[i]), cs.poses[i], "prior, po.align")


# ---- 5. the sensor offset's identity shortcut ---------------------------------------------------------------------------------------------------------------------------
def test_zero_sensor_offset_keeps_the_poses_bits(ctx, po, cs):
    """(0, 0, 0) and (-0.0, 0, 0) both compare equal to zero: Xe has X's bits -- also for an angle outside (-pi, pi], which a composition would wrap"""
    which = [2, 0]
    fx, mv = _sets(cs, which)
    poses = cs.poses.copy()
    poses[0, 2] = np.float32(poses[0, 2] + np.float32(2.0 * math.pi)); poses[3, 2] = np.float32(poses[3, 2] - np.float32(2.0 * math.pi))
    assert abs(poses[0, 2]) > math.pi and abs(poses[3, 2]) > math.pi
    res = []
    for zero in ((0.0, 0.0, 0.0), (-0.0, 0.0, 0.0), (0.0, -0.0, -0.0)):
        al = _aligner(ctx, which, sensors=[zero, cases.S_OFF[0]])
        res.append(_assert_parents_route(ctx, po, al, fx, mv, poses, tag=("zero offset", zero)))
        sp = al.param_slice_processors[0].slice_params()
        assert cases.effective_pose(po, tuple(sp.sensor_in_robot), poses[0]).tobytes() == poses[0].tobytes()
    for r in res[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(r, res[0]))
    # ... and the shortcut is observable: composing with the identity instead wraps the angle and gives other bits somewhere
    wrapped = cases.compose(po, cases.inverse(po, (0.0, 0.0, 0.0)), poses[0])
    assert wrapped[2] != poses[0, 2]


# ---- 6. shapes --------------------------------------------------------------------------------------------------------------------------------------------------------
def _many(cs, n, seed):
    """n hypotheses over the four scans: scan i % 4 (a repeated index), its start pose moved by a few centimetres"""
    rng = np.random.default_rng(seed)
    scan = (np.arange(n) % cs.n).astype(np.int32)
    poses = (cs.poses[scan] + rng.uniform(-0.03, 0.03, (n, 3)).astype(np.float32)).astype(np.float32)
    return scan, poses


@pytest.mark.parametrize("n", [1, 2, 256, 257])
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_batch_sizes_and_index_rules(order_ctx, po, cs, n):
    """per-slice index tables, repeated indices, a one-cloud moving set shared by all items; a prior per item"""
    ctx = order_ctx
    which = [0, 1]
    fx, mv = _sets(cs, which)
    scan, poses = _many(cs, n, seed=n)
    fidx = np.stack([scan, scan[::-1].copy()])      # slice 1 pairs the hypotheses with the scans in another order
    priors = [cases.asym_prior(X, seed=3) for X in poses]
    got = _assert_parents_route(ctx, po, _aligner(ctx, which), fx, mv, poses, priors, fixed_index=fidx, tag=("n", n))
    assert np.all(got[3] >= 1)


def test_two_launch_groups_with_slices_of_unequal_slot(ctx, po, cs):
    """a 2048-column canvas takes 1024 items to a launch group, so 1025 items are two groups -- for the 64-column slice next to it too, which alone would be one"""
    n = 1025
    small = [np.ascontiguousarray(a[::5]) for a in cs.fixed[2]]      # ~200-point clouds
    off = np.zeros(cs.n + 1, np.int32); off[1:] = np.cumsum([len(a) for a in small])
    fixed = api.CloudSet(ctx, np.concatenate(small), off)
    moving = api.CloudSet(ctx, np.ascontiguousarray(cs.moving[2][::30]))
    assert all(150 <= len(a) <= 250 for a in small)
    al = api.MultiAligner2D(ctx, max_iterations=1)
    for cols, S in ((2048, (0.0, 0.0, 0.0)), (64, (0.05, 0.0, 0.1))):
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(
            api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, 30.0)), sensor_in_robot=S,
            robustifier=api.RobustifierCauchy(0.05), min_num_correspondences=5))
    scan, poses = _many(cs, n, seed=5)
    got = _assert_parents_route(ctx, po, al, [fixed, fixed], [moving, moving], poses, fixed_index=np.stack([scan, scan]), tag="two groups")
    assert set(np.unique(got[3]).tolist()) <= {0, 1, 2} and np.any(got[3] == 2)
    assert got[2][1024].tobytes() != got[2][0].tobytes()      # the last item, alone in its group, has its own result


# ---- 7. select --------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_select(al, fx, mv, poses, sel, k, tag, **kw):
    H, b, st, active = api.score_aligner(al, fx, mv, poses, **kw)
    index, gH, gb, gst, gact, n_acc = api.score_aligner_select(al, fx, mv, poses, sel, k, **kw)
    want, want_acc = api.score_rank(st, sel, k, active)
    print(tag, "k", k, "accepted", n_acc, "/", len(st), "selected", len(index), "inactive", int(np.sum(active == 0)))
    assert n_acc == want_acc and index.dtype == np.int32 and np.array_equal(index, want), (tag, index[:16], want[:16])
    assert np.array_equal(u32(gH), u32(H[want])) and np.array_equal(u32(gb), u32(b[want])), tag
    assert gst.tobytes() == np.ascontiguousarray(st[want]).tobytes() and np.array_equal(gact, active[want]), tag
    return want, want_acc, st, active


def _select_batch(cs, n, seed):
    """hypotheses of every kind: good ones, exact repeats (ties), and some far from everything (no pairs: active 0)"""
    scan, poses = _many(cs, n, seed)
    poses[5::7] = poses[4::7][: len(poses[5::7])]; scan[5::7] = scan[4::7][: len(scan[5::7])]      # ties: item 7 m + 5 repeats item 7 m + 4
    poses[3::11, :2] += np.float32(500.0)                                                                   # nothing in reach
    return scan, poses


@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_select_is_score_rank_on_the_combined_statistics(order_ctx, cs):
    ctx = order_ctx
    which = [0, 1]
    fx, mv = _sets(cs, which)
    al = _aligner(ctx, which)
    scan, poses = _select_batch(cs, 300, seed=11)
    kw = dict(fixed_index=np.stack([scan, scan]))
    want, n_acc, st, active = _check_select(al, fx, mv, poses, EVERYTHING, 64, "everything", **kw)
    n_inactive = int(np.sum(active == 0))
    assert n_inactive >= 20 and n_acc == 300 - n_inactive      # {0, +Inf, 0} accepts all but the items no slice contributed to
    ties = [j for j in range(len(want) - 1) if st[want[j]].tobytes() == st[want[j + 1]].tobytes()]
    assert ties and all(want[j] < want[j + 1] for j in ties)      # equal statistics: the lower index first
    _check_select(al, fx, mv, poses, EVERYTHING, 1024, "k > n_accepted", **kw)
    mid = api.SelectParams(int(np.median(st["n_inliers"][active > 0])), 0.015, 0.9)
    _, n_mid, _, _ = _check_select(al, fx, mv, poses, mid, 16, "middle", **kw)
    assert 0 < n_mid < n_acc
    assert ctx.last_kernel_ms() > 0.0
    _, n_none, _, _ = _check_select(al, fx, mv, poses, api.SelectParams(10 ** 9, 0.0, 2.0), 5, "nothing", **kw)
    assert n_none == 0


def test_select_past_one_tile_with_a_prior(ctx, cs):
    which = [2, 0]
    fx, mv = _sets(cs, which)
    al = _aligner(ctx, which)
    n = api.SELECT_TILE + 1
    scan, poses = _select_batch(cs, n, seed=13)
    priors = [cases.asym_prior(X, seed=1) for X in poses]
    kw = dict(fixed_index=np.stack([scan, scan]), priors=priors)
    for k in (1, 100, api.SELECT_MAX_K):
        _check_select(al, fx, mv, poses, EVERYTHING, k, ("past one tile", k), **kw)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
class _Out:
    def __init__(self, k):
        self.index = np.full(k, -7, np.int32); self.H = np.full((k, 9), np.float32(-7.0)); self.b = np.full((k, 3), np.float32(-7.0))
        self.st = np.full(k, 0x55, np.uint8).repeat(api.STATS_DTYPE.itemsize).view(api.STATS_DTYPE); self.active = np.full(k, -7, np.int32)
        self.n_sel = C.c_int32(-7); self.n_acc = C.c_int32(-7)
        self._ref = [a.copy() for a in (self.index, self.H, self.b, self.st, self.active)]

    def untouched(self):
        return all(a.tobytes() == r.tobytes() for a, r in zip((self.index, self.H, self.b, self.st, self.active), self._ref)) and self.n_sel.value == -7 and self.n_acc.value == -7


def _raw_batch(ctx, bd, out, null_H=False):
    return ctx._lib.lsm2d_score_aligner_batch(ctx.handle, C.byref(bd) if bd is not None else None, None if null_H else api._ptr(out.H), api._ptr(out.b),
                                              api._ptr(out.st), api._ptr(out.active))


def _raw_select(ctx, bd, out, k, sel=EVERYTHING, null_index=False):
    s = sel.struct() if sel is not None else None
    return ctx._lib.lsm2d_score_aligner_select(ctx.handle, C.byref(bd), C.byref(s) if s is not None else None, k, None if null_index else api._ptr(out.index),
                                               api._ptr(out.H), api._ptr(out.b), api._ptr(out.st), api._ptr(out.active), C.byref(out.n_sel), C.byref(out.n_acc))


def test_refusals_leave_the_outputs_untouched(ctx, cs):
    which = [0, 1]
    fx, mv = _sets(cs, which)
    al = _aligner(ctx, which)
    both = lambda bd, o: (_raw_batch(ctx, bd, o), _raw_select(ctx, bd, o, 4))
    err = lambda: ctx._lib.lsm2d_last_error(ctx.handle).decode()
    # n_slices outside [1, 4]
    for ns in (0, 5, -1):
        bd, keep = al._batch(fx, mv, cs.poses); bd.n_slices = ns
        o = _Out(8)
        assert both(bd, o) == (BAD_ARGUMENT, BAD_ARGUMENT) and o.untouched(), ns
    # a NULL the call needs
    o = _Out(8)
    bd, keep = al._batch(fx, mv, cs.poses)
    assert _raw_batch(ctx, None, o) == BAD_ARGUMENT and _raw_batch(ctx, bd, o, null_H=True) == BAD_ARGUMENT and o.untouched()
    assert _raw_select(ctx, bd, o, 4, sel=None) == BAD_ARGUMENT and _raw_select(ctx, bd, o, 4, null_index=True) == BAD_ARGUMENT and o.untouched()
    bd.init_pose = None
    assert both(bd, o) == (BAD_ARGUMENT, BAD_ARGUMENT) and o.untouched()
    bd, keep = al._batch(fx, mv, cs.poses); bd.slices = None
    assert both(bd, o) == (BAD_ARGUMENT, BAD_ARGUMENT) and o.untouched()
    # k outside [1, LSM2D_SELECT_MAX_K]
    bd, keep = al._batch(fx, mv, cs.poses)
    for k in (0, -1, api.SELECT_MAX_K + 1):
        assert _raw_select(ctx, bd, o, k) == BAD_ARGUMENT and o.untouched(), k
    # a cloud index out of range: the message names item and slice
    fidx = np.zeros((2, cs.n), np.int32); fidx[1, 2] = cs.n
    bd, keep = al._batch(fx, mv, cs.poses, fixed_index=fidx)
    assert both(bd, o) == (BAD_ARGUMENT, BAD_ARGUMENT) and o.untouched()
    assert "item 2" in err() and "slice 1" in err(), err()
    midx = np.zeros((2, cs.n), np.int32); midx[0, 3] = -1
    bd, keep = al._batch(fx, mv, cs.poses, moving_index=midx)
    assert both(bd, o) == (BAD_ARGUMENT, BAD_ARGUMENT) and o.untouched() and "item 3" in err() and "slice 0" in err()
    # a set without index must hold 1 or n clouds
    bd, keep = al._batch(fx, mv, cs.poses[:3])
    assert both(bd, o) == (BAD_ARGUMENT, BAD_ARGUMENT) and o.untouched()
    # canvases that do not fit LDS (2 x 8 bytes x columns)
    big = api.MultiAligner2D(ctx, max_iterations=1)
    big.param_slice_processors.append(al.param_slice_processors[0])
    big.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(
        api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(1 << 16, -math.pi, math.pi, 0.3, 30.0))))
    assert (1 << 16) * 16 > ctx.get_option("max_dyn_lds")
    bd, keep = big._batch(fx, mv, cs.poses)
    assert both(bd, o) == (CAPACITY_EXCEEDED, CAPACITY_EXCEEDED) and o.untouched()
    # n == 0 succeeds; the select form sets both counts to 0
    bd, keep = al._batch(fx, mv, np.zeros((0, 3), np.float32))
    assert _raw_batch(ctx, bd, o) == 0 and _raw_select(ctx, bd, o, 4) == 0 and (o.n_sel.value, o.n_acc.value) == (0, 0)
    o.n_sel.value = o.n_acc.value = -7
    assert o.untouched()
    # two batches in flight: refused as lsm2d_score_batch refuses; with one the call works and gives the same bits
    want = api.score_aligner(al, fx, mv, cs.poses)
    one = _aligner(ctx, [2])
    a = one.prepare_batch([cs.fixed_sets[2]], [cs.moving_sets[2]], cs.poses); b = one.prepare_batch([cs.fixed_sets[2]], [cs.moving_sets[2]], cs.poses[::-1].copy())
    a.begin()
    try:
        got = api.score_aligner(al, fx, mv, cs.poses)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))
        b.begin()
        try:
            bd, keep = al._batch(fx, mv, cs.poses)
            assert both(bd, o) == (BAD_ARGUMENT, BAD_ARGUMENT) and o.untouched() and "in flight" in err()
        finally:
            a.wait(); a = None
            b.wait()
    finally:
        if a is not None:
            a.wait()
    got = api.score_aligner(al, fx, mv, cs.poses)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))


# ---- 9. the old calls are what they were ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order_ctx", [0, 1], ids=["tree", "reference"], indirect=True)
def test_no_side_effect_on_score_batch_and_score_select(order_ctx, po, cs):
    ctx = order_ctx
    sp = _aligner(ctx, [0]).param_slice_processors[0].slice_params()
    scan, poses = _many(cs, 40, seed=2)
    sel = api.SelectParams(300, 0.05, 0.5)

    def old():
        H, b, st = api.score_batch(ctx, sp, cs.fixed_sets[0], cs.moving_sets[0], poses, scan)
        r = api.score_select(ctx, sp, cs.fixed_sets[0], cs.moving_sets[0], poses, sel, 8, scan)
        return [H.tobytes(), b.tobytes(), api._stats_array(st).tobytes()] + [np.asarray(x).tobytes() for x in r]

    before = old()
    # the old call's digest is still salted with slice 0, whatever the new call hashed with in between
    H, b, st = api.score_batch(ctx, sp, cs.fixed_sets[0], cs.moving_sets[0], poses[:1], scan[:1])
    pairs = po.find(fuzz_cases.oracle_slice(po, sp), cs.fixed[0][scan[0]], cs.moving[0], poses[0])
    assert st[0].pair_digest == po.pair_digest(pairs, 0) != po.pair_digest(pairs, 1)
    which = [1, 0, 2]
    fx, mv = _sets(cs, which)
    api.score_aligner(_aligner(ctx, which), fx, mv, cs.poses, [cases.asym_prior(X) for X in cs.poses])
    api.score_aligner_select(_aligner(ctx, which), fx, mv, cs.poses, EVERYTHING, 3)
    assert old() == before
