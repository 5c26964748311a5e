"""Gauss-Newton damping and general prior information matrices on every aligner path, bit for bit against the fp32 oracle.

Two inputs of the step reach the device by routes of their own: the damping goes to three different 3x3 solves (solve_update in k_align and its narrow, packed,
seq and first-iteration forms; k_split_finish; solve_flat in the latency kernel k_align_pair), the prior's matrix to prior_apply and to the latency kernel's
per-lane copy of it (prior_term_lane).  Here every one of them runs with a damping of 50 and with priors whose matrices are full (L L^T), or not even
symmetric, and whose means are turned away from the start pose, and every finite alignment must equal the oracle in status, iterations, pose, all nine
information entries and every iteration's statistics and digest: the device-order mirror for "sum_order" 0, the sequential oracle for "sum_order" 1.
tests/test_damping_and_prior_cpu.py pins that oracle, and the contrasts asserted here on the device's own results (damping 0, diagonal matrices, a matrix
against its transpose), so that a path that ignores the input cannot pass.  No tolerance appears in the bitwise parts; the fp64 comparison uses gpu_helpers' bars."""
import collections
import ctypes as C
import math
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mixed_batches as mb
from gpu_helpers import POSE_TOL_M, POSE_TOL_RAD, _Envelope, _assert_bitwise_equal_to_device_order_oracle, _oracle_slice, _pose_diff, _same_correspondence_sets, assert_same_bits, result_bits
from srrg2_laser_slam_2d_amd import _capi, api, synth
from mixed_batches import MIN_DIFFERENT as MIXED_MIN_DIFFERENT, WALL_OFFSET_START, WALL_OFFSET_TOL, WALL_ROWS, wall_cloud

pytestmark = pytest.mark.gpu

SEED, DAMPING = mb.DAMPING_SEED, mb.DAMPING
N_SMALL, N_PACKED = mb.DAMPING_N, 1040
_BASE = {}        # (setting, full_omega) -> the batch of N_PACKED alignments: every smaller one is a prefix of it
_DEVICE = {}      # setting -> the cloud sets of its slices and of the map
_ORACLE = {}      # (sum_order, setting, full_omega, damping, i) -> po.align's result


@pytest.fixture(params=[0, 1], ids=["tree", "reference"])
def order_ctx(ctx, request):
    ctx.set_option("sum_order", request.param)
    try:
        yield ctx
    finally:
        for k in ("sum_order", "align_path", "align_width"):
            ctx.set_option(k, 0)
        ctx.set_option("cull", 1); ctx.set_option("balance", 1)


def _spec(n, setting, damping=DAMPING, full=False):
    """the first n alignments of a setting's batch (mixed_batches: a prefix of the larger one), with its damping"""
    if (setting, full) not in _BASE:
        _BASE[(setting, full)] = mb.batch(SEED, N_PACKED, setting, full_omega=full)
    b = _BASE[(setting, full)]
    return dict(b, n=n, damping=float(damping), full=full, all_slices=b["slices"], kinds=b["kinds"][:n], x0=b["x0"][:n], fixed_index=np.ascontiguousarray(b["fixed_index"][:, :n]),
                priors=None if b["priors"] is None else b["priors"][:n])


def _sets(ctx, spec):
    if spec["setting"] not in _DEVICE:
        _DEVICE[spec["setting"]] = ([api.CloudSet(ctx, sl["pts"], sl["offs"]) for sl in spec["all_slices"]], api.CloudSet(ctx, spec["map"]))
    return _DEVICE[spec["setting"]]


def _run(ctx, spec, want_pairs=False, **opts):
    """compute_batch of a batch under context options.  Returns (result, last_align_path, last_align_width)."""
    fixed, moving = _sets(ctx, spec)
    al = mb.aligner(ctx, spec)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        r = al.compute_batch(fixed[:spec["ns"]], [moving] * spec["ns"], spec["x0"], priors=spec["priors"], fixed_index=spec["fixed_index"], want_stats=True, want_pairs=want_pairs)
        return r, ctx.get_option("last_align_path"), ctx.get_option("last_align_width")
    finally:
        for k in opts:
            ctx.set_option(k, 1 if k in ("cull", "balance") else 0)


def _finite(spec):
    return np.flatnonzero(~np.isin(spec["kinds"], mb.NON_FINITE))


def _assert_oracle_bits(po, res, spec, sum_order, tag, want_pairs=False):
    """EVERY finite alignment of the batch against the oracle in the device's order of summation.  Returns the number checked."""
    rows = [int(i) for i in _finite(spec)]
    key = lambda i: (sum_order, spec["setting"], spec["full"], spec["damping"], i)
    todo = [i for i in rows if key(i) not in _ORACLE]
    with ThreadPoolExecutor(16) as ex:
        for i, r in zip(todo, ex.map(lambda i: mb.oracle_align(po, spec, i, device_order=not sum_order), todo)):
            _ORACLE[key(i)] = r
    for i in rows:
        _assert_bitwise_equal_to_device_order_oracle(res, i, _ORACLE[key(i)], (tag, spec["setting"], "sum_order", sum_order, i, spec["kinds"][i]))
    bad = np.isin(spec["kinds"], mb.NON_FINITE)
    assert np.all(res.status[bad] != 0), res.status[bad]
    return len(rows)


def _count_different(a, b, spec, n=N_SMALL):
    """finite alignments among the first n whose pose bits or status differ between two device results; how many were compared"""
    rows = _finite(spec); rows = rows[rows < n]
    d = (a.status[rows] != b.status[rows]) | np.any(a.pose[rows].view(np.uint32) != b.pose[rows].view(np.uint32), axis=1)
    return int(d.sum()), len(rows)


def _assert_contrasts(ctx, res, spec, tag, **opts):
    """part 1's contrasts (tests/test_damping_and_prior_cpu.py) on the device's own results, the first 120 alignments: the batch without damping has a singular H,
    the damped one none, and at least 95 of the 114 finite alignments differ; with full prior matrices at least 95 of 114 differ from the diagonal ones"""
    n = spec["n"]
    diag = res if not spec["full"] else _run(ctx, _spec(n, spec["setting"], spec["damping"], False), **opts)[0]
    plain = _run(ctx, _spec(n, spec["setting"], 0.0, False), **opts)[0]
    rows = _finite(spec); rows = rows[rows < N_SMALL]
    assert np.sum(plain.status[rows] == 3) >= 1 and np.sum(diag.status[rows] == 3) == 0 and np.sum(res.status[rows] == 3) == 0, (tag, plain.status[rows], diag.status[rows])
    d_lambda, k = _count_different(diag, plain, spec)
    assert k == 114 and d_lambda >= MIXED_MIN_DIFFERENT, (tag, d_lambda, k)
    d_omega = None
    if spec["full"]:
        d_omega, k = _count_different(res, diag, spec)
        assert k == 114 and d_omega >= MIXED_MIN_DIFFERENT, (tag, d_omega, k)
    return d_lambda, d_omega


CASES = [("S1", False), ("S3", True)]      # S1 with damping 50; S3 (two slices, one with a sensor offset, priors) with damping 50 and full prior matrices
IDS = ["S1", "S3-full-omega"]


@pytest.mark.parametrize("setting,full", CASES, ids=IDS)
def test_k_align_wide_narrow_and_seq(order_ctx, po, setting, full):
    """n = 120: k_align (512 threads), k_align_narrow<256> and, with "sum_order" 1, k_align_seq -- forced by align_path 1 and align_width; the automatic call (in the
    tree order the latency kernel, at this size) gives the same bits"""
    ctx = order_ctx; so = ctx.get_option("sum_order"); t0 = time.time()
    spec = _spec(N_SMALL, setting, DAMPING, full)
    ref, path0, _ = _run(ctx, spec)
    forms = [("automatic", path0, None)]
    for w in (512, 256):
        r, path, width = _run(ctx, spec, align_path=1, align_width=w)
        assert path == 1 and width == (512 if (so and w == 256) else w), (setting, so, w, path, width)      # (no narrow reference-order kernel: 256 launches 512)
        assert_same_bits(result_bits(r), result_bits(ref), labels=spec["kinds"], tag=("align_width", w))
        forms.append(("align_path 1, align_width %d" % w, path, width))
    r, path, width = _run(ctx, spec, align_path=1, cull=0, balance=0)      # (the stream without culling has no narrow form)
    assert path == 1 and width == 512, (setting, so, path, width)
    assert_same_bits(result_bits(r), result_bits(ref), labels=spec["kinds"], tag="cull 0, balance 0")
    forms.append(("align_path 1, cull 0, balance 0", path, width))
    checked = _assert_oracle_bits(po, ref, spec, so, "n 120")
    d_lambda, d_omega = _assert_contrasts(ctx, ref, spec, (setting, so), align_path=1)
    print("damping and prior, %s, sum_order %d, n %d: forms (name, last_align_path, last_align_width) %s; statuses %s; %d alignments equal the oracle bit for bit; %d of 114 "
          "differ from damping 0%s; %.1f s" % (IDS[CASES.index((setting, full))], so, N_SMALL, forms, dict(sorted(collections.Counter(ref.status.tolist()).items())), checked, d_lambda,
                                              "" if d_omega is None else ", %d of 114 from diagonal prior matrices" % d_omega, time.time() - t0))


@pytest.mark.parametrize("sum_order,setting,full", [(0, "S1", False), (1, "S1", False), (0, "S3", True)], ids=["tree-S1", "reference-S1", "tree-S3-full-omega"])
def test_packed_workgroups(ctx, po, sum_order, setting, full):
    """n = 1040: k_align_two / k_align_seq_two, two alignments in a workgroup one after the other -- the second must see the same damping and its own prior"""
    t0 = time.time()
    ctx.set_option("sum_order", sum_order)
    try:
        spec = _spec(N_PACKED, setting, DAMPING, full)
        ref, path, width = _run(ctx, spec)
        assert path == 1 and width == 1024, (setting, sum_order, path, width)
        r, path_w, width_w = _run(ctx, spec, align_width=512)
        assert path_w == 1 and width_w == 512, (path_w, width_w)
        assert_same_bits(result_bits(r), result_bits(ref), labels=spec["kinds"], tag="align_width 512")
        checked = _assert_oracle_bits(po, ref, spec, sum_order, "n 1040")
        d_lambda, d_omega = _assert_contrasts(ctx, ref, spec, (setting, sum_order))
    finally:
        ctx.set_option("sum_order", 0)
    print("damping and prior, packed, %s%s, sum_order %d, n %d: last_align_path %d, last_align_width %d (forced 512: %d); statuses %s; %d alignments equal the oracle bit for bit; "
          "of the first 120, %d of 114 differ from damping 0%s; %.1f s" % (setting, ", full prior matrices" if full else "", sum_order, N_PACKED, path, width, width_w,
                                                                           dict(sorted(collections.Counter(ref.status.tolist()).items())), checked, d_lambda,
                                                                           "" if d_omega is None else ", %d of 114 from diagonal prior matrices" % d_omega, time.time() - t0))


def _wall_aligner(ctx, damping):
    al = api.MultiAligner2D(ctx, max_iterations=8, min_num_inliers=10, damping=damping)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)),
                                                                      min_num_correspondences=0))
    return al


def _assert_wall_rows(ctx, po, sum_order, path, rows, want_path=None):
    """the wall of tests/test_damping_and_prior_cpu.py on one aligner path (path 0: the one the library takes by itself, which must be want_path): the table's status
    and iterations, the oracle's bits, a failed step discarded"""
    want_path = path if want_path is None else want_path
    wall = wall_cloud(); ws = api.CloudSet(ctx, wall)
    ctx.set_option("align_path", path)
    try:
        for start, lam, status, its in rows:
            al = _wall_aligner(ctx, lam)
            x0 = np.float32([start])
            r = al.compute_batch([ws], [ws], x0, want_stats=True)
            assert ctx.get_option("last_align_path") == want_path, (path, lam)
            o = po.align(po.aligner_params(8, damping=lam, device_order=not sum_order), [_oracle_slice(po, al.param_slice_processors[0].slice_params())], [wall], [wall], x0[0])
            assert (o["status"], o["iterations"]) == (status, its), (lam, o["status"], o["iterations"])
            _assert_bitwise_equal_to_device_order_oracle(r, 0, o, ("wall", "path", path, "sum_order", sum_order, "damping", lam, start))
            if status == 3:
                assert r.pose[0].tobytes() == x0[0].tobytes(), (lam, r.pose[0])      # what was computed behind the failed pivot is discarded: the start pose's bits
            elif not any(start):
                assert np.all(r.pose[0] == 0.0), (lam, r.pose[0])
            else:
                d = np.abs(r.pose[0].astype(np.float64) - [start[0], 0.0, 0.0])
                assert d.max() <= WALL_OFFSET_TOL, (lam, r.pose[0])
    finally:
        ctx.set_option("align_path", 0)


def test_split_path(order_ctx, po):
    """k_split_project + k_split_finish (align_path 2): the first 8 alignments of the S3 batch with damping 50 and full prior matrices, and the wall"""
    ctx = order_ctx; so = ctx.get_option("sum_order")
    spec = _spec(8, "S3", DAMPING, True)
    r2, path, _ = _run(ctx, spec, align_path=2)
    assert path == 2
    r1, path, _ = _run(ctx, spec, align_path=1)
    assert path == 1
    assert_same_bits(result_bits(r2), result_bits(r1), "split path against k_align", spec["kinds"])
    checked = _assert_oracle_bits(po, r2, spec, so, "split")
    diag = _run(ctx, _spec(8, "S3", DAMPING, False), align_path=2)[0]; plain = _run(ctx, _spec(8, "S3", 0.0, True), align_path=2)[0]
    ok = np.flatnonzero(r2.status == 0)
    # (this seed's first eight, measured on both oracles in test_damping_and_prior_cpu.py::test_small_contrasts_the_gpu_tests_rely_on: five succeed; all five differ
    # from their diagonal-matrix result, four from their undamped one -- the fifth has converged)
    d_omega = sum(r2.pose[i].tobytes() != diag.pose[i].tobytes() for i in ok); d_lambda = sum(r2.pose[i].tobytes() != plain.pose[i].tobytes() for i in ok)
    assert len(ok) == 5 and d_omega >= 3 and d_lambda >= 3, (r2.status, d_omega, d_lambda)
    _assert_wall_rows(ctx, po, so, 2, [row for row in WALL_ROWS if row[1] in (0.0, 1.0)])
    print("damping and prior, split path, sum_order %d: last_align_path 2; statuses %s; %d alignments and the wall (damping 1: Success, 0: SingularH) equal the oracle bit for bit"
          % (so, r2.status.tolist(), checked))


def test_latency_kernel(order_ctx, po):
    """k_align_pair<false> / <true>: align_path 3 on a batch and the single-alignment call (its prior travels in the kernel's arguments), one slice and two slices
    (721 + 541 columns, the second with a sensor offset), crossed with {no prior, full Omega with the turned mean, an asymmetric Omega, its transpose} and damping
    {0, 50}; then the wall with every damping of the table -- solve_flat computes past a failed pivot and must discard what it computed"""
    ctx = order_ctx; so = ctx.get_option("sum_order"); t0 = time.time()
    base = _spec(8, "S3", DAMPING, True)
    i0 = int(np.flatnonzero(base["kinds"] == "converge")[0])
    variants = mb.prior_variants(base)
    runs = 0
    for ns in (1, 2):
        poses = {}
        for name, priors in variants.items():
            for lam in (0.0, DAMPING):
                spec = mb.with_slices(base, ns, priors=priors, damping=lam, full=(name, ns))
                r, path, _ = _run(ctx, spec, align_path=3)
                assert path == 3, (ns, name, lam, path)
                _assert_oracle_bits(po, r, spec, so, ("latency kernel, batch of 8", ns, name, lam))
                one = dict(spec, n=1, kinds=spec["kinds"][i0:i0 + 1], x0=spec["x0"][i0:i0 + 1], fixed_index=np.ascontiguousarray(spec["fixed_index"][:, i0:i0 + 1]),
                           priors=None if priors is None else priors[i0:i0 + 1])
                r1, path, _ = _run(ctx, one)
                assert path == 3 and r1.status[0] == 0, (ns, name, lam, path, r1.status)      # automatic: a single alignment takes the latency kernel in both orders
                assert_same_bits(result_bits(r1), result_bits(r), ("single alignment against the batch's", ns, name, lam), one["kinds"], rows=[i0])
                poses[(name, lam)] = r1.pose[0].tobytes() + r1.information[0].tobytes()
                runs += 2
        # every input is seen: no two of the eight (prior, damping) combinations give the same pose and information matrix -- the asymmetric Omega and its transpose
        # included (a property of this seed's alignment, measured on both oracles: test_damping_and_prior_cpu.py::test_small_contrasts_the_gpu_tests_rely_on)
        assert len(set(poses.values())) == len(poses), (ns, [k for k in poses])
    for path in (3, 0):      # forced, and the automatic single-alignment call
        _assert_wall_rows(ctx, po, so, path, WALL_ROWS + [(WALL_OFFSET_START, 1.0, 0, 8)], want_path=3)
    print("damping and prior, latency kernel, sum_order %d: last_align_path 3 in %d calls (batch of 8 and single alignment; 1 and 2 slices; no / full / asymmetric / transposed "
          "prior matrix; damping 0 and 50) and on the wall with damping %s: all equal the oracle bit for bit; %.1f s" % (so, runs, [row[1] for row in WALL_ROWS] + [1.0], time.time() - t0))


def test_point_query_finders(order_ctx, po, small_workload):
    """the instantiations of k_align without a projective stream (and one with both): exact NN, KD-tree, distance map, projective + NN; role B (the map is the
    fixed cloud, the scans are the queries), damping 50, a full prior matrix with a turned mean"""
    ctx = order_ctx; so = ctx.get_option("sum_order")
    wl = small_workload; n = 3
    xb = synth.invert_poses(wl.x0[:n].astype(np.float64)).astype(np.float32)
    rng = np.random.default_rng([SEED, 7])
    priors = []
    for i in range(n):
        L = np.tril(rng.uniform(-3.0, 3.0, (3, 3)), -1) + np.diag(rng.uniform(3.0, 8.0, 3))
        z = synth.compose_poses(xb[i:i + 1].astype(np.float64), np.array([[0.02, -0.01, rng.uniform(0.1, 0.4)]]))[0].astype(np.float32)
        priors.append((z, (L @ L.T).astype(np.float32)))
    scans = [wl.scan_points[wl.scan_offsets[i]:wl.scan_offsets[i + 1]] for i in range(n)]
    fixed = api.CloudSet(ctx, wl.map_points); moving = api.CloudSet(ctx, wl.scan_points[:wl.scan_offsets[n]], wl.scan_offsets[:n + 1])
    finders = dict(exact=lambda: [api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.3, normal_cos=0.8, search="exact")],
                   kdtree=lambda: [api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.3, normal_cos=0.8, search="kdtree")],
                   distmap=lambda: [api.CorrespondenceFinderNN2D(ctx, max_distance_m=0.3, resolution=0.05, normal_cos=0.8)],
                   mixed=lambda: [api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)),
                                  api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.3, normal_cos=0.8, search="exact")])
    for kind, make in finders.items():
        got = {}
        for lam, pri in ((DAMPING, priors), (0.0, priors), (DAMPING, None)):
            al = api.MultiAligner2D(ctx, max_iterations=3, min_num_inliers=10, damping=lam)      # (three iterations: short of convergence, where the damping no longer shows)
            for f in make():
                al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(f, min_num_correspondences=10))
            ns = len(al.param_slice_processors)
            r = al.compute_batch([fixed] * ns, [moving] * ns, xb, priors=pri, want_stats=True)
            assert ctx.get_option("last_align_path") == 1, kind
            osl = [_oracle_slice(po, s.slice_params()) for s in al.param_slice_processors]
            for i in range(n):
                kw = {} if pri is None else dict(prior_z=pri[i][0], prior_omega=pri[i][1])
                o = po.align(po.aligner_params(3, min_num_inliers=10, damping=lam, device_order=not so, **kw), osl, [wl.map_points] * ns, [scans[i]] * ns, xb[i])
                _assert_bitwise_equal_to_device_order_oracle(r, i, o, (kind, "sum_order", so, "damping", lam, "prior", pri is not None, i))
            got[(lam, pri is not None)] = r
        full = got[(DAMPING, True)]
        assert np.all(full.status == 0), (kind, full.status)
        for other in ((0.0, True), (DAMPING, False)):
            assert all(full.pose[i].tobytes() != got[other].pose[i].tobytes() for i in range(n)), (kind, other)
    print("damping and prior, point-query finders %s, sum_order %d: last_align_path 1; 3 alignments each with (damping, prior) = (50, full), (0, full), (50, none) equal the oracle "
          "bit for bit" % (list(finders), so))


def test_forms_that_only_carry_state(ctx, po):
    """a prepared batch run three times, begin / wait and the pairs call on the S3 batch (n = 120, damping 50, full prior matrices); one device through lsm2d_sweep_align
    with damping 50 (S1: one slice, no prior)"""
    spec = _spec(N_SMALL, "S3", DAMPING, True)
    fixed, moving = _sets(ctx, spec)
    ref, path, _ = _run(ctx, spec)
    checked = _assert_oracle_bits(po, ref, spec, 0, "automatic")
    al = mb.aligner(ctx, spec)
    prep = al.prepare_batch(fixed, [moving] * 2, spec["x0"], priors=spec["priors"], fixed_index=spec["fixed_index"], want_stats=True)
    for k in range(3):
        assert_same_bits(result_bits(prep.run(copy=True)), result_bits(ref), labels=spec["kinds"], tag=("prepared", k))
    prep.begin(); assert_same_bits(result_bits(prep.wait(copy=True)), result_bits(ref), labels=spec["kinds"], tag="begin / wait")
    pairs, _, _ = _run(ctx, spec, want_pairs=True)
    assert_same_bits(result_bits(pairs), result_bits(ref), labels=spec["kinds"], tag="want_pairs")
    for i in _finite(spec)[:16]:
        w = mb.oracle_align(po, spec, int(i), device_order=True, want_pairs=True)
        assert all(np.array_equal(pairs.pairs[i][s], w["pairs"][s]) for s in range(2)), ("pairs", int(i), spec["kinds"][i])
    # ---- the sweep
    s1 = _spec(N_SMALL, "S1", DAMPING, False)
    want, path1, _ = _run(ctx, s1)
    _assert_oracle_bits(po, want, s1, 0, "S1 automatic")
    lib = _capi.load(); P = lambda a: a.ctypes.data_as(C.c_void_p)
    sw = C.c_void_p()
    assert lib.lsm2d_sweep_create((C.c_int32 * 1)(0), 1, C.byref(sw)) == 0
    try:
        sl = s1["slices"][0]
        scans = np.ascontiguousarray(sl["pts"]); offs = np.ascontiguousarray(sl["offs"], np.int32); mp = np.ascontiguousarray(s1["map"])
        assert lib.lsm2d_sweep_set_scans(sw, P(scans), P(offs), len(offs) - 1) == 0 and lib.lsm2d_sweep_set_map(sw, P(mp), len(mp)) == 0
        n = s1["n"]
        x0 = np.ascontiguousarray(s1["x0"], np.float32); idx = np.ascontiguousarray(s1["fixed_index"][0], np.int32)
        pose = np.zeros((n, 3), np.float32); H = np.zeros((n, 9), np.float32); status = np.full(n, -7, np.int32); iters = np.zeros(n, np.int32)
        sp = mb.aligner(None, s1).param_slice_processors[0].slice_params()
        for lam, other in ((DAMPING, want), (0.0, _run(ctx, _spec(N_SMALL, "S1", 0.0, False))[0])):
            ap = _capi.AlignerParams(s1["max_iterations"], s1["min_num_inliers"], lam)
            assert lib.lsm2d_sweep_align(sw, C.byref(ap), C.byref(sp), n, P(idx), P(x0), P(pose), P(H), P(status), P(iters), None) == 0, lib.lsm2d_sweep_last_error(sw)
            fin = _finite(s1)
            assert np.array_equal(status[fin], other.status[fin]) and np.array_equal(iters[fin], other.iterations[fin]), lam
            assert np.array_equal(pose[fin].view(np.uint32), other.pose[fin].view(np.uint32)), lam
            assert np.array_equal(H[fin].view(np.uint32), other.information[fin].reshape(-1, 9).view(np.uint32)), lam
    finally:
        lib.lsm2d_sweep_destroy(sw)
    d, k = _count_different(want, _run(ctx, _spec(N_SMALL, "S1", 0.0, False))[0], s1)
    assert k == 114 and d >= MIXED_MIN_DIFFERENT, (d, k)
    print("damping and prior, state-carrying forms: prepared x 3, begin / wait, pairs (S3, full prior matrices, last_align_path %d), lsm2d_sweep_align (S1, against last_align_path %d) "
          "with damping 50: the automatic call's bits; %d alignments of it equal the oracle bit for bit" % (path, path1, checked))


def test_against_the_fp64_oracle(ctx, po):
    """the `converge` alignments of the S3 batch (n = 120, damping 50, full prior matrices with turned means): the device's pose within gpu_helpers' bars of the fp64
    oracle wherever it used the sequential fp32 oracle's pairs in every iteration (digests); gpu_helpers._Envelope's rule for the others, nothing named, nothing new"""
    spec = _spec(N_SMALL, "S3", DAMPING, True)
    res, _, _ = _run(ctx, spec)
    rows = [int(i) for i in np.flatnonzero(spec["kinds"] == "converge")]
    with ThreadPoolExecutor(16) as ex:
        seq = list(ex.map(lambda i: mb.oracle_align(po, spec, i), rows)); dbl = list(ex.map(lambda i: mb.oracle_align(po, spec, i, double=True), rows))
    env = _Envelope("damping_and_prior", SEED)
    strict, worst = 0, 0.0
    for i, r, rd in zip(rows, seq, dbl):
        assert rd["status"] == 0 and res.status[i] == 0, (i, rd["status"], res.status[i])
        dm, dr = _pose_diff(res.pose[i], rd["pose"])
        if res.iterations[i] == r["iterations"] and _same_correspondence_sets(res.stats[i], r["stats"], r["iterations"]):
            assert dm <= POSE_TOL_M and dr <= POSE_TOL_RAD, (i, dm, dr)
            strict += 1; worst = max(worst, dm, dr)
        else:
            rr = mb.oracle_align(po, spec, i, double="ref")
            env.check((0, i, "pair sets differ"), res.pose[i], int(res.status[i]), r, rd, rr,
                      perturbed=lambda: [mb.oracle_align(po, dict(spec, x0=np.tile(xp, (spec["n"], 1))), i) for xp in _Envelope.one_ulp_starts(spec["x0"][i])])
    env.assert_only_named_exceptions()
    # (not vacuous: with the device-order oracle in the device's place, 49 of this seed's 54 are in the strict class -- test_small_contrasts_the_gpu_tests_rely_on;
    # the device equals that oracle bit for bit, so the count is the same here)
    assert strict == 49 and len(rows) == 54, (strict, len(rows))
    print("damping and prior against fp64: %d converge alignments, %d with the sequential oracle's pairs in every iteration within %.1e of the fp64 oracle (bar %.0e); the others: %s"
          % (len(rows), strict, worst, POSE_TOL_M, env.summary()))
