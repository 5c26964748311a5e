#!/usr/bin/env python3
"""The grouped select calls -- a fleet's candidates, the best k per robot, in one call with one wait -- against the two routes a fleet server had before them:
(b) one ungrouped select call per robot, one after another, and (c) ONE batch call with everything coming down (lsm2d_align_batch with every iteration's
statistics; lsm2d_score_batch's rows) followed by the same test and a partial sort per robot on the host.  All three run through the bare C ABI from one C++
program (tests/cpp/select_grouped_bench.cpp, built here with g++), alternating call by call.  Medians over --steps timed calls after --warmup, wall clock
around calls that end in their wait, kernel timing off; `grouped_kernel_ms` is lsm2d_last_kernel_ms of one more grouped call with kernel timing on.  One JSON
line per part.

Align parts: the loop detector's aligner (30 iterations, Cauchy 0.05, projective finder: MULTI.json:602-630) and its thresholds (500 / 0.1 / 0.8:
MULTI.json:964-986) and, because this small geometry cannot reach 500 inliers, again with min_inliers 230 and 100
(--min-inliers: aligned candidates end with 200 to 300 inliers here), k = 8; G robots x 64 candidates each, G in --robots (16, 256, 1024); 721-column scans (16
distinct ones, robot g's is scan g % 16) against an 800-point map, tests/bench/clip_vox_batch_bench.py's geometry.  Every group fits one tile: ONE selection launch behind the aligner's.
Score part: lsm2d_score_select_grouped with one relocalisation grid of 4096 hypotheses per robot at G = 16, the same slice and thresholds: every group is
two tiles, so the segmented passes are what is timed.

Parity gate, inside every run and before any time is reported: the C++ program finds the three routes' verdicts equal group by group and the grouped call's
rows equal to the batch call's rows of the selected items byte for byte; here the grouped call's counts and indices are held to api.align_rank_grouped /
api.score_rank_grouped on what that run's batch call returned.

    python tests/bench/select_grouped_bench.py [--robots 16,256,1024] [--per-robot 64] [--grid 4096] [--k 8] [--steps 20] [--warmup 2] [--parts align,score]

Measured figures: README.md, DESIGN.md section 8 and profiles/r27/."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import bench_common
from bench_common import HERE_ROOT, bits_arg

TAU = 0.05
COLS = 721
MAP_POINTS = 800
DISTINCT = 16
ITERATIONS = 30


def run_part(api, exe, tmp, mode, wl, x0, idx, groups, sel, args):
    n = len(x0); G = len(groups) - 1
    tag = "%s_%d" % (mode, G)
    files = {k: os.path.join(tmp, "%s_%s.bin" % (tag, k)) for k in ("scans", "offsets", "map", "poses", "index", "groups", "out")}
    np.ascontiguousarray(wl.scan_points, np.float32).tofile(files["scans"]); np.ascontiguousarray(wl.scan_offsets, np.int32).tofile(files["offsets"])
    np.ascontiguousarray(wl.map_points, np.float32).tofile(files["map"]); np.ascontiguousarray(x0, np.float32).tofile(files["poses"])
    np.ascontiguousarray(idx, np.int32).tofile(files["index"]); np.ascontiguousarray(groups, np.int32).tofile(files["groups"])
    out = subprocess.run([exe, mode, files["scans"], files["offsets"], files["map"], files["poses"], files["index"], files["groups"], str(COLS), repr(TAU),
                          str(ITERATIONS), str(sel.min_inliers), bits_arg(sel.max_chi_per_inlier), bits_arg(sel.min_inlier_ratio), str(args.k), str(args.steps),
                          str(args.warmup), files["out"]],
                         check=True, capture_output=True, text=True).stdout
    r = json.loads(out)
    # ---- parity gate
    assert r["grouped_is_host"] == 1 and r["per_group_calls_is_host"] == 1, "parity: the three routes' verdicts"
    assert r["rows_equal"] == 1, "parity: the grouped call's rows against the batch call's"
    raw = open(files["out"], "rb").read()
    at = 0
    if mode == "align":
        status = np.frombuffer(raw, np.int32, n, 0); its = np.frombuffer(raw, np.int32, n, 4 * n); at = 8 * n
    last = np.frombuffer(raw, api.STATS_DTYPE, n, at); at += 28 * n
    n_acc = np.frombuffer(raw, np.int32, G, at); n_sel = np.frombuffer(raw, np.int32, G, at + 4 * G); index = np.frombuffer(raw, np.int32, G * args.k, at + 8 * G)
    want = api.align_rank_grouped(status, its, last, groups, sel, args.k) if mode == "align" else api.score_rank_grouped(last, groups, sel, args.k)
    assert np.array_equal(n_acc, want[1]), "parity: the accepted counts against the restatement"
    for g in range(G):
        assert n_sel[g] == len(want[0][g]) and np.array_equal(index[g * args.k: g * args.k + n_sel[g]], want[0][g]), "parity: group %d's selection" % g
    a, b, c = r["grouped_ms"], r["per_group_calls_ms"], r["batch_and_host_ms"]
    return dict(bench="select_grouped", mode=mode, n_groups=G, n_items=n, k=args.k, steps=args.steps, grouped_ms=a[0], per_group_calls_ms=b[0], batch_and_host_ms=c[0],
                per_group_calls_over_grouped=round(b[0] / a[0], 3), batch_and_host_over_grouped=round(c[0] / a[0], 3), grouped_ms_min_max=a[1:],
                per_group_calls_ms_min_max=b[1:], batch_and_host_ms_min_max=c[1:], grouped_kernel_ms=r["grouped_kernel_ms"],
                batch_down_bytes=int(n) * int(r["stats_rows_per_item"]) * 28, grouped_down_bytes=G * (16 + 4 * args.k + 4 * (24 if mode == "align" else 17) * args.k),
                n_accepted=int(r["n_accepted"]), n_selected=int(r["n_selected"]), groups_with_a_winner=int(np.count_nonzero(n_sel)),
                thresholds=[sel.min_inliers, sel.max_chi_per_inlier, sel.min_inlier_ratio], parity="ok")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--robots", default="16,256,1024")
    ap.add_argument("--per-robot", type=int, default=64)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--grid-robots", type=int, default=16)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--min-inliers", default="500,230,100", help="min_inliers thresholds to run every part with: the loop detector's, one that some robots' candidates meet, one that all do")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="align,score")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, HERE_ROOT)
    from srrg2_laser_slam_2d_amd import api, synth
    # the loop detector's thresholds; an 800-point map cannot give a 721-column scan 500 inliers, so under them every group reports "nothing accepted" -- the
    # selection still runs in full, the gather moves no row.  Every part therefore runs again with min_inliers lowered until some, then all, groups have winners.
    sels = [api.SelectParams(min_inliers=int(v)) for v in args.min_inliers.split(",")]
    parts = args.parts.split(",")
    world = synth.make_world(1)
    wl = synth.make_workload(DISTINCT, MAP_POINTS, seed=1, n_beams=COLS, world=world)

    def candidates(G, per_robot, spread, salt):
        """robot g: scan g % DISTINCT, per_robot start poses within +-spread of its true pose"""
        n = G * per_robot
        idx = ((np.arange(n) // per_robot) % DISTINCT).astype(np.int32)
        delta = synth.Stream(1001 + G, salt=salt).uniform(3 * n, -spread, spread).reshape(n, 3)
        x0 = synth.invert_poses(synth.compose_poses(synth.invert_poses(wl.x_true)[idx], delta)).astype(np.float32)
        return x0, idx, (np.arange(G + 1) * per_robot).astype(np.int32)

    with tempfile.TemporaryDirectory() as tmp:
        exe = bench_common.build("select_grouped_bench.cpp", tmp)
        lines = []
        for sel in sels:
            if "align" in parts:
                for G in [int(v) for v in args.robots.split(",")]:
                    lines.append(run_part(api, exe, tmp, "align", wl, *candidates(G, args.per_robot, 0.05, 9), sel, args))
            if "score" in parts:      # a relocalisation grid per robot: hypotheses within +-0.25 of the truth
                lines.append(run_part(api, exe, tmp, "score", wl, *candidates(args.grid_robots, args.grid, 0.25, 10), sel, args))
        for ln in lines:
            bench_common.emit(ln, args.label)


if __name__ == "__main__":
    main()
