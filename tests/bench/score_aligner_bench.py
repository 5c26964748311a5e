#!/usr/bin/env python3
"""lsm2d_score_aligner_batch / lsm2d_score_aligner_select for a two-slice aligner (front and rear laser, WithSensor offsets) against the route a caller had
before them: one lsm2d_score_batch per slice at the effective pose the caller composes itself (two waits, two full row copies), the rows added and the skip
rule applied on the host, and for the select form the acceptance test and a partial sort on the host.  All four routes run through the bare C ABI from one
C++ program (tests/cpp/score_aligner_bench.cpp, built here with g++), alternating call by call.  Medians over --steps timed calls after --warmup, wall clock
around calls that end in their wait, kernel timing off; `*_kernel_ms` is lsm2d_last_kernel_ms of one more call with kernel timing on (the new calls: the last
launch group of the last slice, the combination and the selection; the baseline: the last launch group of its second lsm2d_score_batch).  One JSON line per
part.  Run the command twice: how far the BASELINE's own median moves between the two runs is the margin a difference has to exceed.

Part a: 1000 items of BASELINE configs[1] geometry -- 1000 scans of 1081 beams, a 100 000-point map, Cauchy tau 0.05, projective finders -- seen by a front
        laser at (0.2, 0.1, 0.1) and a rear laser at (-0.3, 0, pi) in the robot frame (the tracker benches' offsets): slice s's fixed cloud is the scan moved
        by S_s^-1.
Part b: a relocalisation grid -- 65 536 hypotheses (64 x 64 x 16 in x, y, theta around its start pose) of ONE scan pair against the map.

Parity gate, inside every run and before any time is reported: the new call's rows equal the old route's byte for byte (H, b, counts, chi^2 sums, active;
the digest apart: the old route cannot salt it with the slice index), and both selections are the same items in the same order.

    python tests/bench/score_aligner_bench.py [--n 1000] [--map 100000] [--grid 65536] [--k 64] [--steps 20] [--warmup 3] [--parts a,b] [--workdir DIR]

Measured figures: README.md, DESIGN.md section 8 and profiles/r18/."""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

import bench_common
from bench_common import HERE_ROOT, bits_arg

TAU = 0.05
COLS = 1081
MIN_CORR = 10
SENSORS = [(0.2, 0.1, 0.1), (-0.3, 0.0, math.pi)]


def run_part(api, po, cases, synth, exe, tmp, part, scans, offs, m, poses, order, args):
    n = len(poses)
    files = {k: os.path.join(tmp, "%s_%s.bin" % (part, k)) for k in ("fixed0", "off0", "fixed1", "off1", "map", "poses", "sinv")}
    sinv = np.zeros((2, 8), np.float32)
    for s, S in enumerate(SENSORS):
        S32 = np.float32(S)
        inv = synth.invert_poses(np.array([S32], np.float64))[0]
        cases._move(np.ascontiguousarray(scans, np.float32), inv).tofile(files["fixed%d" % s]); np.ascontiguousarray(offs, np.int32).tofile(files["off%d" % s])
        si = cases.inverse(po, S32); sn, cs = po.sincos(si[2])
        sinv[s, :3] = S32; sinv[s, 3:6] = si; sinv[s, 6] = cs[0]; sinv[s, 7] = sn[0]
    sinv.tofile(files["sinv"])
    np.ascontiguousarray(m, np.float32).tofile(files["map"]); np.ascontiguousarray(poses, np.float32).tofile(files["poses"])
    # thresholds read off a sample of the batch's own statistics, so that a good part of it is accepted and k cuts the ranking
    ctx = api.Context(0)
    ctx.set_option("sum_order", order)
    al = api.MultiAligner2D(ctx, max_iterations=1)
    for S in SENSORS:
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(
            api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(COLS, -math.pi, math.pi, 0.3, 30.0)), sensor_in_robot=tuple(np.float32(S).tolist()),
            robustifier=api.RobustifierCauchy(TAU), min_num_correspondences=MIN_CORR))
    fixed = [api.CloudSet(ctx, np.fromfile(files["fixed%d" % s], np.float32).reshape(-1, 4), offs if len(offs) > 2 else None) for s in range(2)]
    moving = api.CloudSet(ctx, m)
    _, _, st, active = api.score_aligner(al, fixed, [moving, moving], poses)
    ctx.close()
    ok = active > 0
    n_in = st["n_inliers"].astype(np.float32)
    per_inlier = st["chi_inliers"] / np.maximum(n_in, np.float32(1.0)); ratio = n_in / np.maximum(st["n_correspondences"], 1).astype(np.float32)
    sel = api.SelectParams(int(np.median(st["n_inliers"][ok])), float(np.quantile(per_inlier[ok], 0.9).astype(np.float32)), float(np.quantile(ratio[ok], 0.1).astype(np.float32)))
    out = subprocess.run([exe] + [files[k] for k in ("fixed0", "off0", "fixed1", "off1", "map", "poses", "sinv")] +
                         [str(COLS), repr(TAU), str(order), str(MIN_CORR), str(sel.min_inliers), bits_arg(sel.max_chi_per_inlier), bits_arg(sel.min_inlier_ratio), str(args.k),
                          str(args.steps), str(args.warmup)], check=True, capture_output=True, text=True).stdout
    r = json.loads(out)
    # ---- parity gate
    assert r["rows_equal"] == 1, "parity: the new call's rows against the per-slice route combined on the host"
    assert r["select_equal"] == 1, "parity: the new selection against the host's test and partial sort"
    want, n_acc = api.score_rank(st, sel, args.k, active)
    assert r["n_accepted"] == n_acc and r["n_selected"] == len(want) and r["best_item"] == (int(want[0]) if len(want) else -1), "parity: the selection against score_rank"
    line = dict(bench="score_aligner", part=part, sum_order=order, n_items=n, n_slices=2, k=args.k, steps=args.steps)
    for key in ("batch_ms", "baseline_batch_ms", "select_ms", "baseline_select_ms"):
        line[key] = r[key][0]; line[key + "_min_max"] = r[key][1:]
    line.update(baseline_over_batch=round(r["baseline_batch_ms"][0] / r["batch_ms"][0], 3), baseline_over_select=round(r["baseline_select_ms"][0] / r["select_ms"][0], 3),
                batch_kernel_ms=r["batch_kernel_ms"], select_kernel_ms=r["select_kernel_ms"], baseline_kernel_ms=r["baseline_kernel_ms"], n_accepted=n_acc,
                n_selected=len(want), n_inactive=r["n_inactive"], thresholds=[sel.min_inliers, sel.max_chi_per_inlier, sel.min_inlier_ratio], parity="ok")
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--grid", type=int, default=65536)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--orders", default="0")
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, HERE_ROOT); sys.path.insert(0, os.path.join(HERE_ROOT, "tests"))
    import score_aligner_cases as cases
    from oracle import pyoracle as po
    from srrg2_laser_slam_2d_amd import api, synth
    po.lib()
    pts, offs, m, x0 = bench_common.workload(synth, args.workdir, args.n, args.map)
    parts = args.parts.split(",")
    with tempfile.TemporaryDirectory() as tmp:
        exe = bench_common.build("score_aligner_bench.cpp", tmp)
        for order in [int(v) for v in args.orders.split(",")]:
            lines = []
            if "a" in parts:
                lines.append(run_part(api, po, cases, synth, exe, tmp, "a", pts, offs, m, np.ascontiguousarray(x0, np.float32), order, args))
            if "b" in parts:
                n = args.grid
                nt = 16; nxy = int(round(math.sqrt(n / nt)))
                assert nxy * nxy * nt == n, "--grid must be 16 x a square"
                gx, gy, gt = np.meshgrid(np.linspace(-1.0, 1.0, nxy), np.linspace(-1.0, 1.0, nxy), np.linspace(-0.2, 0.2, nt), indexing="ij")
                delta = np.stack([gx.ravel(), gy.ravel(), gt.ravel()], 1)
                poses = np.ascontiguousarray(synth.compose_poses(np.tile(np.asarray(x0[:1], np.float64), (n, 1)), delta), np.float32)
                scan = np.ascontiguousarray(pts[offs[0]:offs[1]])
                lines.append(run_part(api, po, cases, synth, exe, tmp, "b", scan, np.int32([0, len(scan)]), m, poses, order, args))
            for ln in lines:
                bench_common.emit(ln, args.label)


if __name__ == "__main__":
    main()
