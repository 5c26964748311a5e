#!/usr/bin/env python3
"""lsm2d_relocalize_select (scoring, selection, gather, alignment and verdict chained on the device: one upload, one copy down, one wait) against the route a
caller had before it: lsm2d_score_aligner_select, the host's gather of the selected hypotheses, lsm2d_align_select.  Both routes run through the bare C ABI
from one C++ program (tests/cpp/relocalize_bench.cpp, built here with g++), alternating call by call.  Medians over --steps timed calls after --warmup, wall
clock around calls that end in their wait, kernel timing off; `*_kernel_ms` is lsm2d_last_kernel_ms of one more call of each with kernel timing on (the
two-call route: its two calls' brackets, which do not cover the gap between them).  One JSON line per part.

The aligner is the loop detector's (30 iterations, Cauchy 0.05, projective finder: MULTI.json:602-630), the thresholds are the loop detector's (500 / 0.1 /
0.8: MULTI.json:964-986) unless --min-inliers lowers the first: the synthetic scans do not all reach 500 inliers at a perturbed pose.
Part a: 1000 hypotheses of BASELINE configs[1] geometry -- 1000 scans of 1081 beams, one each, against a 100 000-point map; k_score = 64.
Part b: the 65 536-hypothesis grid of ONE scan (256 x 256 translations within +-0.5 m of the truth) against the same map; k_score = 64.
Part c: part a with thresholds nobody passes: the fused call still aligns k_score pads, the two calls stop after the scoring -- the pad cost.

Parity gate, inside every run and before any time is reported: every output of the two routes is equal byte for byte.

    python tests/bench/relocalize_bench.py [--n 1000] [--map 100000] [--grid 256] [--k-score 64] [--k 64] [--steps 20] [--warmup 2] [--parts a,b,c]

Measured figures: README.md and profiles/r28/."""
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
COLS = 1081
ITERATIONS = 30


def run_part(exe, tmp, part, scans, offs, m, poses, sel, args):
    files = {k: os.path.join(tmp, "%s_%s.bin" % (part, k)) for k in ("scans", "offsets", "map", "poses")}
    np.ascontiguousarray(scans, np.float32).tofile(files["scans"]); np.ascontiguousarray(offs, np.int32).tofile(files["offsets"])
    np.ascontiguousarray(m, np.float32).tofile(files["map"]); np.ascontiguousarray(poses, np.float32).tofile(files["poses"])
    out = subprocess.run([exe, files["scans"], files["offsets"], files["map"], files["poses"], str(COLS), repr(TAU), str(ITERATIONS), str(sel.min_inliers),
                          bits_arg(sel.max_chi_per_inlier), bits_arg(sel.min_inlier_ratio), str(args.k_score), str(args.k), str(args.steps), str(args.warmup)],
                         check=True, capture_output=True, text=True).stdout
    r = json.loads(out)
    assert r["outputs_equal"] == 1, "parity: the fused call's outputs against the two calls'"
    fused, two = r["fused_ms"], r["two_call_ms"]
    return dict(bench="relocalize", part=part, n_hypotheses=r["n_hypotheses"], k_score=args.k_score, k=args.k, steps=args.steps, iterations=ITERATIONS,
                fused_ms=fused[0], two_call_ms=two[0], two_call_over_fused=round(two[0] / fused[0], 3), fused_ms_min_max=fused[1:], two_call_ms_min_max=two[1:],
                fused_kernel_ms=r["fused_kernel_ms"], two_call_kernel_ms=r["two_call_kernel_ms"], n_scored_accepted=r["n_scored_accepted"],
                n_scored_selected=r["n_scored_selected"], n_success=r["n_success"], n_accepted=r["n_accepted"], n_selected=r["n_selected"], best=r["best"],
                thresholds=[sel.min_inliers, sel.max_chi_per_inlier, sel.min_inlier_ratio], parity="ok")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--k-score", type=int, default=64)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--min-inliers", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, HERE_ROOT)
    from srrg2_laser_slam_2d_amd import api, synth
    sel = api.SelectParams()      # the loop detector's thresholds
    if args.min_inliers is not None:
        sel.min_inliers = args.min_inliers
    nobody = api.SelectParams(10 ** 9, 0.0, 2.0)
    parts = args.parts.split(",")
    with tempfile.TemporaryDirectory() as tmp:
        exe = bench_common.build("relocalize_bench.cpp", tmp)
        wl = synth.make_workload(args.n, args.map, seed=1)
        x0 = np.ascontiguousarray(wl.x0, np.float32)
        lines = []
        if "a" in parts:
            lines.append(run_part(exe, tmp, "a", wl.scan_points, wl.scan_offsets, wl.map_points, x0, sel, args))
        if "b" in parts:
            g = args.grid
            t = np.linspace(-0.5, 0.5, g, dtype=np.float64)
            d = np.stack([np.repeat(t, g), np.tile(t, g), np.zeros(g * g)], axis=1)
            grid = np.ascontiguousarray(x0[0][None, :].astype(np.float64) + d, np.float32)
            lo, hi = int(wl.scan_offsets[0]), int(wl.scan_offsets[1])
            lines.append(run_part(exe, tmp, "b", wl.scan_points[lo:hi], np.int32([0, hi - lo]), wl.map_points, grid, sel, args))
        if "c" in parts:
            lines.append(run_part(exe, tmp, "c", wl.scan_points, wl.scan_offsets, wl.map_points, x0, nobody, args))
        for ln in lines:
            bench_common.emit(ln, args.label)


if __name__ == "__main__":
    main()
