#!/usr/bin/env python3
"""What the aligner's correspondence vectors cost at batch scale, and the batched finder alone.  BASELINE configs[1] geometry (1000 scans of 1081 beams
against a 100 000-point map, 20 iterations).  One JSON line per part, medians over --steps timed calls after --warmup, every part parity-gated inside the
run (the batch's pairs against single calls):

  a  lsm2d_align_batch_pairs against lsm2d_align_batch, both at n = 1000: what the pairs add to a step
  b  lsm2d_find_correspondences_batch alone at 1000 items: the projective finder (scan fixed, map moving) and the exact NN finder in role B
     (map fixed, scan moving): us per item, launches per call
  c  the tracker's shape: ONE alignment, two 721-column slices (one with a sensor offset) and a prior, with pairs

    python tests/bench/pairs_batch_bench.py [--parts a,b,c] [--steps 20] [--warmup 3] [--root TREE] [--workdir DIR]

--root TREE imports the package (and its built library) from another checkout of the project -- parts a and c use nothing this checkout added, so the
same script times the parent commit next to this one (alternate the two in one job).  --workdir keeps the synthetic workload between invocations."""
import argparse
import ctypes as C
import math
import os
import statistics
import sys
import time

import numpy as np

import bench_common
from bench_common import HERE_ROOT


def _median_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t), max(t)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class _AlignCall:
    """an aligner call marshalled once: run(pairs) calls lsm2d_align_batch_pairs (pairs) or lsm2d_align_batch"""

    def __init__(self, api, al, fixed, moving, x0, priors=None, cap=1081):
        self.lib, self.ctx = al._ctx._lib, al._ctx
        self.b, self.keep = al._batch(fixed, moving, x0, priors, None, None)
        self.ap = api.AlignerParams(al.param_max_iterations, al.param_min_num_inliers, al.param_damping, al.param_termination_chi_epsilon,
                                    1 if al.param_enable_inlier_only_runs else 0, 1 if al.param_keep_only_inlier_correspondences else 0)
        n, ns = self.b.n_alignments, self.b.n_slices
        self.n, self.ns, self.cap = n, ns, cap
        self.pose = np.empty((n, 3), np.float32); self.H = np.empty((n, 9), np.float32)
        self.status = np.empty(n, np.int32); self.its = np.empty(n, np.int32)
        self.pbuf = np.empty((n, ns, cap, 2), np.int32); self.pcnt = np.zeros((n, ns), np.int32)

    def run(self, pairs):
        if pairs:
            rc = self.lib.lsm2d_align_batch_pairs(self.ctx.handle, C.byref(self.ap), C.byref(self.b), _p(self.pose), _p(self.H), _p(self.status), _p(self.its), None,
                                                  _p(self.pbuf), self.cap, _p(self.pcnt))
        else:
            rc = self.lib.lsm2d_align_batch(self.ctx.handle, C.byref(self.ap), C.byref(self.b), _p(self.pose), _p(self.H), _p(self.status), _p(self.its), None)
        assert rc == 0, rc

    def pairs(self, i, s):
        return self.pbuf[i, s, : self.pcnt[i, s]].copy()


def part_a(api, ctx, wl, args):
    pts, offs, m, x0 = wl
    n = len(x0)
    al = api.MultiAligner2D(ctx, max_iterations=20, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(
        api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)), min_num_correspondences=10))
    fixed = api.CloudSet(ctx, pts, offs); moving = api.CloudSet(ctx, m)
    call = _AlignCall(api, al, [fixed], [moving], x0)
    call.run(True)
    # parity gate: every 50th alignment's vector against a call with that alignment alone (one alignment keeps the single finder calls)
    scans = [pts[offs[i]:offs[i + 1]] for i in range(n)]
    checked = 0
    for i in range(0, n, 50):
        one = al.compute_batch([api.CloudSet(ctx, scans[i])], [moving], x0[i:i + 1], want_pairs=True)
        assert int(one.iterations[0]) == int(call.its[i]) and np.array_equal(one.pairs[0][0], call.pairs(i, 0)), ("parity", i)
        checked += 1
    total_pairs = int(call.pcnt.sum())
    plain = _median_ms(lambda: call.run(False), args.steps, args.warmup)
    withp = _median_ms(lambda: call.run(True), args.steps, args.warmup)
    return dict(part="a", n=n, steps=args.steps, align_batch_ms=round(plain[0], 4), align_batch_pairs_ms=round(withp[0], 4),
                pairs_cost_ms=round(withp[0] - plain[0], 4), align_batch_ms_min_max=[round(plain[1], 4), round(plain[2], 4)],
                align_batch_pairs_ms_min_max=[round(withp[1], 4), round(withp[2], 4)], pairs_returned=total_pairs, parity_checked=checked, parity="ok")


def part_b(api, ctx, wl, args):
    pts, offs, m, x0 = wl
    n = len(x0)
    from srrg2_laser_slam_2d_amd import synth
    fixed = api.CloudSet(ctx, pts, offs); mset = api.CloudSet(ctx, m)
    inv = synth.invert_poses(x0.astype(np.float64)).astype(np.float32)
    budget = 1 << 21
    out = []
    cases = (("projective", api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)), fixed, mset, x0, 1081),
             ("exact_nn_role_b", api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.5, normal_cos=0.8, search="exact"), mset, fixed, inv, 1081))
    for name, f, fx, mv, poses, cap in cases:
        got = f.compute_batch(fx, mv, poses)
        for i in range(0, n, 50):      # parity gate: single calls
            f.setFixed(fx, i if fx.n_clouds > 1 else 0); f.setMoving(mv, i if mv.n_clouds > 1 else 0); f.setLocalMapInSensor(poses[i])
            assert np.array_equal(f.compute(), got[i]), ("parity", name, i)
        sp = f.slice_params()
        buf = np.empty((n, cap, 2), np.int32); cnt = np.empty(n, np.int32); p = np.ascontiguousarray(poses, np.float32)
        lib = ctx._lib

        def call():
            rc = lib.lsm2d_find_correspondences_batch(ctx.handle, C.byref(sp), fx.handle, None, mv.handle, None, n, _p(p), _p(buf), cap, _p(cnt))
            assert rc == 0, rc
        med = _median_ms(call, args.steps, args.warmup)
        f.setFixed(fx, 0); f.setMoving(mv, 0); f.setLocalMapInSensor(poses[0])
        single = _median_ms(lambda: f.compute(), max(args.steps, 50), args.warmup)
        out.append(dict(part="b", finder=name, n_items=n, steps=args.steps, call_ms=round(med[0], 4), us_per_item=round(med[0] * 1e3 / n, 3),
                        launches_per_call=int(math.ceil(n / max(1, budget // cap))), pairs_returned=int(cnt.sum()),
                        single_call_us_python=round(single[0] * 1e3, 2), parity="ok"))
    return out


def part_c(api, ctx, args):
    from srrg2_laser_slam_2d_amd import synth
    world = synth.make_world(6)
    S = [np.float32([0.2, 0.1, 0.1]), np.float32([-0.3, 0.0, math.pi])]
    robot = synth.sample_poses(world, 1, seed=12)[0]
    sensors = [synth.compose_poses(robot[None, :], s[None, :].astype(np.float64)) for s in S]
    scans = [synth.make_scans(world, sp, n_beams=721, noise_sigma=0.004, seed=40 + i)[0] for i, sp in enumerate(sensors)]
    proj = api.PointNormal2fProjectorPolar(721, -math.pi, math.pi, 0.3, 20.0)
    m = synth.make_map(world, 20000, noise_sigma=0.004, seed=2)
    guess = synth.compose_poses(robot[None, :], np.array([[0.03, -0.02, 0.02]]))[0].astype(np.float32)
    clipper = api.SceneClipperProjective2D(ctx, proj, asynchronous=False, voxelize_resolution=0.0)
    clipper.setFullScene(api.CloudSet(ctx, m)); clipper.setRobotInLocalMap(guess); clipper.setSensorInRobot(S[0])
    clipped = clipper.compute()
    al = api.MultiAligner2D(ctx, max_iterations=10, min_num_inliers=10)
    for s in S:
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(api.CorrespondenceFinderProjective2f(ctx, proj, 0.5, 0.8), sensor_in_robot=s,
                                                                                  min_num_correspondences=5))
    fixed = [api.CloudSet(ctx, sc) for sc in scans]
    priors = [(np.zeros(3, np.float32), np.diag(np.float32([20.0, 20.0, 40.0])))]
    call = _AlignCall(api, al, fixed, [clipped, clipped], np.zeros((1, 3), np.float32), priors=priors, cap=721)
    call.run(True)
    assert int(call.status[0]) == 0 and int(call.pcnt.min()) > 100, (call.status, call.pcnt)
    # parity gate: the two vectors against the finder's single calls at the pose the last iteration started from is what the library does itself; here the
    # vectors of two consecutive calls must agree and the pose must be the pairless call's
    first = [call.pairs(0, s) for s in range(2)]; pose = call.pose.copy()
    call.run(False); assert np.array_equal(pose.view(np.uint32), call.pose.view(np.uint32))
    call.run(True); assert all(np.array_equal(first[s], call.pairs(0, s)) for s in range(2))
    steps = max(args.steps, 300)
    plain = _median_ms(lambda: call.run(False), steps, 20)
    withp = _median_ms(lambda: call.run(True), steps, 20)
    return dict(part="c", shape="1 alignment, 2 slices of 721 columns, prior", steps=steps, align_us=round(plain[0] * 1e3, 2), align_pairs_us=round(withp[0] * 1e3, 2),
                pairs_cost_us=round((withp[0] - plain[0]) * 1e3, 2), pairs_returned=int(call.pcnt.sum()), parity="ok")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--root", default=HERE_ROOT, help="checkout whose package and library are timed")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, os.path.abspath(args.root))
    from srrg2_laser_slam_2d_amd import api, synth
    parts = args.parts.split(",")
    ctx = api.Context(0)
    wl = bench_common.workload(synth, args.workdir, args.n, args.map) if ("a" in parts or "b" in parts) else None
    lines = []
    if "a" in parts:
        lines.append(part_a(api, ctx, wl, args))
    if "b" in parts:
        lines += part_b(api, ctx, wl, args)
    if "c" in parts:
        lines.append(part_c(api, ctx, args))
    for ln in lines:
        bench_common.emit(ln, args.label)
    ctx.close()


if __name__ == "__main__":
    main()
