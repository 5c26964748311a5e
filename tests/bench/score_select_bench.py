#!/usr/bin/env python3
"""lsm2d_score_select with k = 64 (scoring, acceptance test and ranking on the device: 64 rows come down) against the route a caller had before it:
lsm2d_score_batch followed by the same acceptance test and a partial sort on the host.  Both routes run through the bare C ABI from one C++ program
(tests/cpp/score_select_bench.cpp, built here with g++), alternating call by call, so Python's per-item structs flatter neither.  Medians over --steps timed
calls after --warmup, wall clock around calls that end in their wait, kernel timing off; `*_kernel_ms` is lsm2d_last_kernel_ms of one more call of each with
kernel timing on (the new call: its last launch group plus the selection; the baseline: its last launch group).  One JSON line per part.

Part a: 1000 items of BASELINE configs[1] geometry -- 1000 scans of 1081 beams, a 100 000-point map, Cauchy tau 0.05, projective finder.
Part b: a relocalisation grid -- 65 536 hypotheses (64 x 64 x 16 in x, y, theta around its start pose) of ONE scan against the map.
The thresholds are read off the batch's own statistics (api.score_batch, before the C++ program runs): the median inlier count, the 0.9 quantile of chi per
inlier and the 0.1 quantile of the inlier ratio, so that a good part of the batch is accepted and k cuts the ranking.

Parity gate, inside every run and before any time is reported: the new call's selection and the host route's both equal api.score_rank on the statistics
the C++ program's lsm2d_score_batch returned, and the new call's rows equal that call's rows for the selected items, byte for byte.

    python tests/bench/score_select_bench.py [--n 1000] [--map 100000] [--grid 65536] [--k 64] [--steps 20] [--warmup 3] [--parts a,b] [--workdir DIR]

Measured figures: README.md, DESIGN.md section 8 and profiles/r14/."""
import argparse
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

import bench_common
from bench_common import HERE_ROOT

TAU = 0.05
COLS = 1081


def run_part(api, ctx, exe, tmp, part, scans, offs, m, poses, order, args):
    n = len(poses)
    finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(COLS, -math.pi, math.pi, 0.3, 30.0))
    sp = finder.slice_params()
    sp.robustifier = api.ROBUST_CAUCHY; sp.chi_threshold = TAU
    ctx.set_option("sum_order", order)
    fixed = api.CloudSet(ctx, scans, offs if len(offs) > 2 else None); moving = api.CloudSet(ctx, m)
    st = api._stats_array(api.score_batch(ctx, sp, fixed, moving, poses)[2])
    n_in = st["n_inliers"].astype(np.float32)
    per_inlier = st["chi_inliers"] / np.maximum(n_in, np.float32(1.0)); ratio = n_in / np.maximum(st["n_correspondences"], 1).astype(np.float32)
    sel = api.SelectParams(int(np.median(st["n_inliers"])), float(np.quantile(per_inlier, 0.9).astype(np.float32)), float(np.quantile(ratio, 0.1).astype(np.float32)))
    del fixed, moving
    files = {k: os.path.join(tmp, "%s_%s.bin" % (part, k)) for k in ("scans", "offsets", "map", "poses", "stats")}
    np.ascontiguousarray(scans, np.float32).tofile(files["scans"]); np.ascontiguousarray(offs, np.int32).tofile(files["offsets"])
    np.ascontiguousarray(m, np.float32).tofile(files["map"]); np.ascontiguousarray(poses, np.float32).tofile(files["poses"])
    out = subprocess.run([exe, files["scans"], files["offsets"], files["map"], files["poses"], str(COLS), repr(TAU), str(order), str(sel.min_inliers),
                          bench_common.bits_arg(sel.max_chi_per_inlier), bench_common.bits_arg(sel.min_inlier_ratio), str(args.k), str(args.steps), str(args.warmup),
                          files["stats"]],
                         check=True, capture_output=True, text=True).stdout
    r = json.loads(out)
    # ---- parity gate: both selections are score_rank's on the statistics that run returned; they are also the ones this process scored
    st_run = np.fromfile(files["stats"], api.STATS_DTYPE)
    assert st_run.tobytes() == st.tobytes(), "parity: the C++ program's lsm2d_score_batch against api.score_batch"
    want, n_acc = api.score_rank(st_run, sel, args.k)
    assert r["rows_equal"] == 1, "parity: the selected rows against lsm2d_score_batch's"
    assert r["n_accepted"] == [n_acc, n_acc] and r["index_select"] == want.tolist() and r["index_baseline"] == want.tolist(), "parity: the selection against score_rank"
    new, base = r["select_ms"], r["baseline_ms"]
    return dict(bench="score_select", part=part, sum_order=order, n_items=n, k=args.k, steps=args.steps, select_ms=new[0], baseline_ms=base[0],
                baseline_over_select=round(base[0] / new[0], 3), select_ms_min_max=new[1:], baseline_ms_min_max=base[1:], select_kernel_ms=r["select_kernel_ms"],
                baseline_kernel_ms=r["baseline_kernel_ms"], n_accepted=n_acc, n_selected=len(want), thresholds=[sel.min_inliers, sel.max_chi_per_inlier, sel.min_inlier_ratio],
                best_item=int(want[0]) if len(want) else -1, parity="ok")


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
    sys.path.insert(0, HERE_ROOT)
    from srrg2_laser_slam_2d_amd import api, synth
    ctx = api.Context(0)
    pts, offs, m, x0 = bench_common.workload(synth, args.workdir, args.n, args.map)
    parts = args.parts.split(",")
    with tempfile.TemporaryDirectory() as tmp:
        exe = bench_common.build("score_select_bench.cpp", tmp)
        for order in [int(v) for v in args.orders.split(",")]:
            lines = []
            if "a" in parts:
                lines.append(run_part(api, ctx, exe, tmp, "a", pts, offs, m, np.ascontiguousarray(x0, np.float32), order, args))
            if "b" in parts:
                n = args.grid
                nt = 16; nxy = int(round(math.sqrt(n / nt)))
                assert nxy * nxy * nt == n, "--grid must be 16 x a square"
                gx, gy, gt = np.meshgrid(np.linspace(-1.0, 1.0, nxy), np.linspace(-1.0, 1.0, nxy), np.linspace(-0.2, 0.2, nt), indexing="ij")
                delta = np.stack([gx.ravel(), gy.ravel(), gt.ravel()], 1)
                poses = np.ascontiguousarray(synth.compose_poses(np.tile(np.asarray(x0[:1], np.float64), (n, 1)), delta), np.float32)
                scan = np.ascontiguousarray(pts[offs[0]:offs[1]])
                lines.append(run_part(api, ctx, exe, tmp, "b", scan, np.int32([0, len(scan)]), m, poses, order, args))
            for ln in lines:
                bench_common.emit(ln, args.label)
    ctx.close()


if __name__ == "__main__":
    main()
