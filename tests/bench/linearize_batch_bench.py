#!/usr/bin/env python3
"""lsm2d_linearize_batch against the same items through lsm2d_linearize one after another, in one process.  BASELINE configs[1] geometry: 1000 scans of
1081 beams against a 100 000-point map, every item's pairs those of the projective finder (scan fixed, map moving) at its start pose, Cauchy robustifier.
The loop of single calls is the baseline: it is what a caller with 1000 hypotheses had before the batch call existed.  One JSON line per order of summation
("sum_order" 0: trees, 1: the reference's), medians over --steps timed calls after --warmup, wall clock with kernel timing off; `*_kernel_ms` is
lsm2d_last_kernel_ms of one more call with kernel timing on (the batch: its launches; the loop: the sum over its 1000 calls).

Parity gate, inside the run and before any timing: every item of the batch equals the single call on that item in H, b, counts, chi^2 sums and digest, bit
for bit, and every 50th item equals the CPU oracle in the order asked for (linearize_device_order / the sequential linearize).

    python tests/bench/linearize_batch_bench.py [--n 1000] [--map 100000] [--steps 20] [--warmup 3] [--workdir DIR]

Measured on an MI355X (gfx950), 1000 items, 638 011 pairs (583 816 inliers / 54 195 outliers at tau 0.05), medians of 20, every item bit-equal to its single call:
    sum_order 0: batch 0.527 ms (0.51 .. 0.54), loop 23.25 ms (23.20 .. 23.52): 44 x; lsm2d_last_kernel_ms 0.026 ms (two launches) against 13.6 ms summed over the loop
    sum_order 1: batch 0.522 ms (0.50 .. 0.58), loop 27.47 ms (27.39 .. 27.54): 53 x; lsm2d_last_kernel_ms 0.030 ms (one launch) against 18.2 ms summed over the loop
  a second run of the same command: 0.472 against 23.21 ms (49 x) and 0.482 against 27.35 ms (57 x)
The batch call is host-bound: the device works for 0.03 of its 0.5 ms; the rest is the host's check of 638 011 index pairs, their packing into pinned memory,
the 5 MB copy to the device and the wait.  The loop pays a staging copy, one or two launches and a wait per item (23 us each)."""
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


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def run_order(api, capi, po, ctx, wl, order, args):
    pts, offs, m, x0 = wl
    n = len(x0)
    lib = ctx._lib
    ctx.set_option("sum_order", order)
    fixed = api.CloudSet(ctx, pts, offs); moving = api.CloudSet(ctx, m)
    cols = 1081
    finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(cols, -math.pi, math.pi, 0.3, 30.0))
    spf = finder.slice_params()
    poses = np.ascontiguousarray(x0, np.float32)
    pairs = np.empty((n, cols, 2), np.int32); cnt = np.empty(n, np.int32)
    rc = lib.lsm2d_find_correspondences_batch(ctx.handle, C.byref(spf), fixed.handle, None, moving.handle, None, n, _p(poses), _p(pairs), cols, _p(cnt))
    assert rc == 0, rc
    sp = api.make_slice_params(robustifier=api.ROBUST_CAUCHY, chi_threshold=TAU)
    H = np.empty((n, 9), np.float32); b = np.empty((n, 3), np.float32); st = (capi.IterationStats * n)()
    H1 = np.empty((n, 9), np.float32); b1 = np.empty((n, 3), np.float32); st1 = (capi.IterationStats * n)()

    def batch():
        rc = lib.lsm2d_linearize_batch(ctx.handle, C.byref(sp), fixed.handle, None, moving.handle, None, n, _p(pairs), cols, _p(cnt), _p(poses), _p(H), _p(b), st)
        assert rc == 0, rc

    # the loop's arguments marshalled once: what is timed is the calls
    single_args = [(ctx.handle, C.byref(sp), fixed.handle, i, moving.handle, 0, C.c_void_p(pairs[i].ctypes.data), int(cnt[i]), C.c_void_p(poses[i].ctypes.data),
                    C.c_void_p(H1[i].ctypes.data), C.c_void_p(b1[i].ctypes.data), C.byref(st1[i])) for i in range(n)]
    fn1 = lib.lsm2d_linearize

    def loop():
        for a in single_args:
            if fn1(*a) != 0:
                raise RuntimeError("lsm2d_linearize failed")

    # ---- parity gate
    batch(); loop()
    assert np.array_equal(H.view(np.uint32), H1.view(np.uint32)) and np.array_equal(b.view(np.uint32), b1.view(np.uint32)), "parity: H, b"
    assert bytes(st) == bytes(st1), "parity: statistics"
    osp = po.slice_params(robustifier=po.ROBUST_CAUCHY, chi_threshold=TAU)
    oracle = po.linearize if order else po.linearize_device_order
    checked = 0
    for i in range(0, n, 50):
        oH, ob, ost = oracle(osp, pts[offs[i]:offs[i + 1]], m, pairs[i, : cnt[i]], poses[i])
        assert np.array_equal(H[i].view(np.uint32), oH.ravel().view(np.uint32)) and np.array_equal(b[i].view(np.uint32), ob.view(np.uint32)), ("oracle", i)
        assert (st[i].n_correspondences, st[i].n_inliers, st[i].n_outliers, st[i].pair_digest) == (ost.n_corr, ost.n_in, ost.n_out, ost.pair_digest), ("oracle", i)
        assert np.float32(st[i].chi_inliers) == np.float32(ost.chi_in) and np.float32(st[i].chi_outliers) == np.float32(ost.chi_out), ("oracle", i)
        checked += 1
    # ---- wall clock, kernel timing off
    ctx.set_option("kernel_timing", 0)
    tb = _median_ms(batch, args.steps, args.warmup)
    tl = _median_ms(loop, args.steps, args.warmup)
    # ---- device time of one more call each
    ctx.set_option("kernel_timing", 1)
    batch(); batch_kernel_ms = ctx.last_kernel_ms()
    loop_kernel_ms = 0.0
    for a in single_args:
        assert fn1(*a) == 0
        loop_kernel_ms += ctx.last_kernel_ms()
    budget = 1 << 21
    return dict(bench="linearize_batch", sum_order=order, n_items=n, pairs=int(cnt.sum()), steps=args.steps, batch_ms=round(tb[0], 4), loop_ms=round(tl[0], 4),
                loop_over_batch=round(tl[0] / tb[0], 2), batch_ms_min_max=[round(tb[1], 4), round(tb[2], 4)], loop_ms_min_max=[round(tl[1], 4), round(tl[2], 4)],
                batch_us_per_item=round(tb[0] * 1e3 / n, 3), loop_us_per_item=round(tl[0] * 1e3 / n, 3), batch_kernel_ms=round(batch_kernel_ms, 4),
                loop_kernel_ms=round(loop_kernel_ms, 4), launches_per_batch_call=int(math.ceil(n / max(1, budget // cols))) * (1 if order else 2),
                inliers=int(sum(s.n_inliers for s in st)), outliers=int(sum(s.n_outliers for s in st)), parity_items=n, oracle_items=checked, parity="ok")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--orders", default="0,1")
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
    for order in [int(v) for v in args.orders.split(",")]:
        bench_common.emit(run_order(api, capi, po, ctx, wl, order, args), args.label)
    ctx.close()


if __name__ == "__main__":
    main()
