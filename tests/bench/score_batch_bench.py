#!/usr/bin/env python3
"""lsm2d_score_batch (finder, then factor, pairs kept on the device: one copy down and one wait) against lsm2d_find_correspondences_batch followed by
lsm2d_linearize_batch on the same items in the same process.  The two-call sequence is what a caller with N pose hypotheses had before the fused call
existed, so it is the baseline.  Medians over --steps timed calls after --warmup, the two routes ALTERNATING call by call, wall clock around calls that end
in their wait, kernel timing off; `*_kernel_ms` is lsm2d_last_kernel_ms of one more call with kernel timing on (the fused call: its last launch group, finder
and factor together; the two-call route: the finder's launch plus the factor's).  One JSON line per part, finder role and order of summation.

Part a: 1000 items of BASELINE configs[1] geometry -- 1000 scans of 1081 beams, a 100 000-point map, Cauchy tau 0.05 -- with the projective finder (scan
fixed, map moving) and, as a second line, role B with the exact NN finder (map fixed, scans moving, max_distance 0.5).
Part b: a relocalisation grid -- 65 536 hypotheses (64 x 64 x 16 in x, y, theta around its start pose) of ONE scan against the map, projective finder, fused
call only: the two-call route would move 567 MB of pair slots down and again up.  A recorded figure, nothing to compare against.

Parity gate, inside the run and before any timing: every item of the fused call equals the two-call route in H, b and the statistics, byte for byte, and
every 50th item (part b: sixteen spread over all launch groups) equals the CPU oracle -- po.find, then linearize_device_order / the sequential linearize.

    python tests/bench/score_batch_bench.py [--n 1000] [--map 100000] [--grid 65536] [--steps 20] [--warmup 3] [--parts a,b] [--workdir DIR]

Measured on an MI355X (gfx950), medians of 20, every item byte-equal to the two-call route:
    part a, projective (scan fixed, map moving; 638 011 pairs, 583 816 inliers / 54 195 outliers), run 1 / run 2:
        sum_order 0: fused 0.229 / 0.226 ms (0.22 .. 0.24) against 1.390 / 1.291 ms (1.22 .. 1.49) for the two calls: 6.1 / 5.7 x
        sum_order 1: fused 0.225 / 0.224 ms (0.22 .. 0.23) against 1.312 / 1.273 ms (1.25 .. 1.37): 5.8 / 5.7 x
        lsm2d_last_kernel_ms: 0.17 ms for the fused call (finder and factor), 0.17 .. 0.18 ms summed over the two calls
      The bar -- the fused median below the two-call median by more than the two-call route's own spread over two runs -- is met: the two-call medians of the
      two runs differ by 0.10 ms (sum_order 1: 0.04 ms), the fused call lies 1.06 .. 1.16 ms below them.  The fused call is device-bound (0.17 of its 0.23 ms);
      what it saves is the 8.6 MB copy down, the host's index check and packing, the 5 MB copy up and the second wait.
    part a, role B, exact NN (map fixed, scans moving; 941 540 pairs): fused 1.613 / 1.615 ms against 2.888 / 2.890 ms (1.8 x), sum_order 1: 1.614 / 1.621 against
      2.880 / 2.880 ms; lsm2d_last_kernel_ms 1.56 ms (the finder's kernel is all but 0.03 ms of it)
    part b, 65 536 hypotheses of one scan (13 994 453 pairs), 34 launch groups of 1940 items, one wait:
        sum_order 0: 10.434 / 10.436 ms per call (10.39 .. 10.53), 0.159 us per hypothesis; the last launch group (1516 items) 0.207 ms on the device
        sum_order 1: 10.634 / 10.639 ms per call (10.56 .. 10.72), 0.162 us per hypothesis; 0.21 ms
      The two-call route at this size: not measured."""
import argparse
import ctypes as C
import math
import statistics
import sys
import time

import numpy as np

import bench_common
from bench_common import HERE_ROOT

TAU = 0.05
COLS = 1081
BUDGET = 1 << 21      # pair slots per launch group


def _stats(t):
    return [round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)]


def _alternating_ms(fns, steps, warmup):
    """every function once per round, round after round: what drifts (clocks, other tenants) drifts for all of them"""
    for _ in range(warmup):
        for f in fns:
            f()
    t = [[] for _ in fns]
    for _ in range(steps):
        for k, f in enumerate(fns):
            t0 = time.perf_counter(); f(); t[k].append((time.perf_counter() - t0) * 1e3)
    return [_stats(x) for x in t]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _oracle_check(po, osp, order, fcloud, mcloud, pose, H, b, st, tag):
    v = po.find(osp, fcloud, mcloud, pose)
    oH, ob, ost = (po.linearize if order else po.linearize_device_order)(osp, fcloud, mcloud, v, pose)
    assert np.array_equal(H.view(np.uint32), oH.ravel().view(np.uint32)) and np.array_equal(b.view(np.uint32), ob.view(np.uint32)), ("oracle", tag)
    assert (st.n_correspondences, st.n_inliers, st.n_outliers, st.pair_digest) == (ost.n_corr, ost.n_in, ost.n_out, ost.pair_digest), ("oracle", tag)
    assert np.float32(st.chi_inliers) == np.float32(ost.chi_in) and np.float32(st.chi_outliers) == np.float32(ost.chi_out), ("oracle", tag)


def part_a(api, capi, po, synth, ctx, wl, role, order, args):
    pts, offs, m, x0 = wl
    n = len(x0)
    lib = ctx._lib
    ctx.set_option("sum_order", order)
    scans = api.CloudSet(ctx, pts, offs); mp = api.CloudSet(ctx, m)
    if role == "projective":      # scan fixed, map moving
        finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(COLS, -math.pi, math.pi, 0.3, 30.0))
        osp = po.slice_params(robustifier=po.ROBUST_CAUCHY, chi_threshold=TAU)
        fixed, moving, poses, cap = scans, mp, np.ascontiguousarray(x0, np.float32), COLS
        clouds = lambda i: (pts[offs[i]:offs[i + 1]], m)
    else:                         # role B: map fixed, scans moving, exact nearest neighbour
        finder = api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.5, search="exact")
        osp = po.slice_params(finder=po.FINDER_NN, max_distance=0.5, robustifier=po.ROBUST_CAUCHY, chi_threshold=TAU)
        fixed, moving, poses, cap = mp, scans, synth.invert_poses(np.asarray(x0, np.float64)).astype(np.float32), int(np.diff(offs).max())
        clouds = lambda i: (m, pts[offs[i]:offs[i + 1]])
    sp = finder.slice_params()
    sp.robustifier = api.ROBUST_CAUCHY; sp.chi_threshold = TAU
    pairs = np.empty((n, cap, 2), np.int32); cnt = np.empty(n, np.int32)
    H = np.empty((n, 9), np.float32); b = np.empty((n, 3), np.float32); st = (capi.IterationStats * n)()
    H2 = np.empty((n, 9), np.float32); b2 = np.empty((n, 3), np.float32); st2 = (capi.IterationStats * n)()
    two_kernel_ms = [0.0]

    def fused():
        rc = lib.lsm2d_score_batch(ctx.handle, C.byref(sp), fixed.handle, None, moving.handle, None, n, _p(poses), _p(H), _p(b), st)
        assert rc == 0, rc

    def two_calls(timed=False):
        rc = lib.lsm2d_find_correspondences_batch(ctx.handle, C.byref(sp), fixed.handle, None, moving.handle, None, n, _p(poses), _p(pairs), cap, _p(cnt))
        assert rc == 0, rc
        if timed:
            two_kernel_ms[0] = ctx.last_kernel_ms()
        rc = lib.lsm2d_linearize_batch(ctx.handle, C.byref(sp), fixed.handle, None, moving.handle, None, n, _p(pairs), cap, _p(cnt), _p(poses), _p(H2), _p(b2), st2)
        assert rc == 0, rc
        if timed:
            two_kernel_ms[0] += ctx.last_kernel_ms()

    # ---- parity gate
    fused(); two_calls()
    assert np.array_equal(H.view(np.uint32), H2.view(np.uint32)) and np.array_equal(b.view(np.uint32), b2.view(np.uint32)), "parity: H, b"
    assert bytes(st) == bytes(st2), "parity: statistics"
    checked = 0
    for i in range(0, n, 50):
        fc, mc = clouds(i)
        _oracle_check(po, osp, order, fc, mc, poses[i], H[i], b[i], st[i], i)
        checked += 1
    # ---- wall clock, kernel timing off, the two routes alternating
    ctx.set_option("kernel_timing", 0)
    tf, tt = _alternating_ms([fused, two_calls], args.steps, args.warmup)
    # ---- device time of one more call each
    ctx.set_option("kernel_timing", 1)
    fused(); fused_kernel_ms = ctx.last_kernel_ms()
    two_calls(timed=True)
    ctx.set_option("kernel_timing", 0)
    groups = int(math.ceil(n / max(1, min(BUDGET // max(cap, 1), 1 << 16))))
    return dict(bench="score_batch", part="a", role=role, sum_order=order, n_items=n, slot=cap, pairs=int(cnt.sum()), steps=args.steps,
                fused_ms=tf[0], two_call_ms=tt[0], two_call_over_fused=round(tt[0] / tf[0], 2), fused_ms_min_max=tf[1:], two_call_ms_min_max=tt[1:],
                fused_us_per_item=round(tf[0] * 1e3 / n, 3), two_call_us_per_item=round(tt[0] * 1e3 / n, 3), fused_kernel_ms=round(fused_kernel_ms, 4),
                two_call_kernel_ms=round(two_kernel_ms[0], 4), launch_groups=groups, inliers=int(sum(s.n_inliers for s in st)),
                outliers=int(sum(s.n_outliers for s in st)), parity_items=n, oracle_items=checked, parity="ok")


def part_b(api, capi, po, synth, ctx, wl, order, args):
    pts, offs, m, x0 = wl
    lib = ctx._lib
    ctx.set_option("sum_order", order)
    scan = np.ascontiguousarray(pts[offs[0]:offs[1]])
    fixed = api.CloudSet(ctx, scan); moving = api.CloudSet(ctx, m)
    n = args.grid
    nt = 16; nxy = int(round(math.sqrt(n / nt)))
    assert nxy * nxy * nt == n, "--grid must be 16 x a square"
    gx, gy, gt = np.meshgrid(np.linspace(-1.0, 1.0, nxy), np.linspace(-1.0, 1.0, nxy), np.linspace(-0.2, 0.2, nt), indexing="ij")
    delta = np.stack([gx.ravel(), gy.ravel(), gt.ravel()], 1)
    poses = np.ascontiguousarray(synth.compose_poses(np.tile(np.asarray(x0[:1], np.float64), (n, 1)), delta), np.float32)
    finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(COLS, -math.pi, math.pi, 0.3, 30.0))
    sp = finder.slice_params()
    sp.robustifier = api.ROBUST_CAUCHY; sp.chi_threshold = TAU
    osp = po.slice_params(robustifier=po.ROBUST_CAUCHY, chi_threshold=TAU)
    H = np.empty((n, 9), np.float32); b = np.empty((n, 3), np.float32); st = (capi.IterationStats * n)()

    def fused():
        rc = lib.lsm2d_score_batch(ctx.handle, C.byref(sp), fixed.handle, None, moving.handle, None, n, _p(poses), _p(H), _p(b), st)
        assert rc == 0, rc

    fused()
    per_group = max(1, min(BUDGET // COLS, 1 << 16))
    groups = int(math.ceil(n / per_group))
    picks = sorted({0, per_group - 1, per_group, n - 1} | set(int(v) for v in np.linspace(0, n - 1, 12)))
    for i in picks:
        if 0 <= i < n:
            _oracle_check(po, osp, order, scan, m, poses[i], H[i], b[i], st[i], i)
    # the first launch group's items against the two-call route
    k = min(n, per_group)
    pairs = np.empty((k, COLS, 2), np.int32); cnt = np.empty(k, np.int32)
    H2 = np.empty((k, 9), np.float32); b2 = np.empty((k, 3), np.float32); st2 = (capi.IterationStats * k)()
    assert lib.lsm2d_find_correspondences_batch(ctx.handle, C.byref(sp), fixed.handle, None, moving.handle, None, k, _p(poses), _p(pairs), COLS, _p(cnt)) == 0
    assert lib.lsm2d_linearize_batch(ctx.handle, C.byref(sp), fixed.handle, None, moving.handle, None, k, _p(pairs), COLS, _p(cnt), _p(poses), _p(H2), _p(b2), st2) == 0
    assert np.array_equal(H[:k].view(np.uint32), H2.view(np.uint32)) and np.array_equal(b[:k].view(np.uint32), b2.view(np.uint32)), "parity: H, b"
    assert bytes(st)[: C.sizeof(st2)] == bytes(st2), "parity: statistics"
    ctx.set_option("kernel_timing", 0)
    (tf,) = _alternating_ms([fused], args.steps, args.warmup)
    ctx.set_option("kernel_timing", 1)
    fused(); kernel_ms = ctx.last_kernel_ms()
    ctx.set_option("kernel_timing", 0)
    nc = np.array([s.n_correspondences for s in st])
    return dict(bench="score_batch", part="b", role="projective", sum_order=order, n_items=n, slot=COLS, pairs=int(nc.sum()), steps=args.steps, fused_ms=tf[0],
                fused_ms_min_max=tf[1:], fused_us_per_item=round(tf[0] * 1e3 / n, 3), launch_groups=groups, last_group_kernel_ms=round(kernel_ms, 4),
                items_in_last_group=n - (groups - 1) * per_group, best_item=int(np.argmax([s.n_inliers for s in st])), parity_items=k, oracle_items=len(picks),
                parity="ok")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--grid", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--orders", default="0,1")
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, HERE_ROOT)
    from oracle import pyoracle as po
    from srrg2_laser_slam_2d_amd import _capi as capi, api, synth
    po.lib()
    ctx = api.Context(0)
    wl = bench_common.workload(synth, args.workdir, args.n, args.map)
    parts = args.parts.split(",")

    def emit(ln):
        bench_common.emit(ln, args.label)

    for order in [int(v) for v in args.orders.split(",")]:
        if "a" in parts:
            for role in ("projective", "exact_nn_role_b"):
                emit(part_a(api, capi, po, synth, ctx, wl, role, order, args))
        if "b" in parts:
            emit(part_b(api, capi, po, synth, ctx, wl, order, args))
    ctx.close()


if __name__ == "__main__":
    main()
