#!/usr/bin/env python3
"""lsm2d_align_select with k = 64 (alignment, acceptance test -- status term included -- and ranking on the device: 64 rows come down) against the route a
caller had before it: lsm2d_align_batch with every iteration's statistics, followed by the same test on each candidate's last row and a partial sort on the
host.  Both routes run through the bare C ABI from one C++ program (tests/cpp/align_select_bench.cpp, built here with g++), alternating call by call.
Medians over --steps timed calls after --warmup, wall clock around calls that end in their wait, kernel timing off; `*_kernel_ms` is lsm2d_last_kernel_ms of
one more call of each with kernel timing on (the new call: the aligner's launch plus the packing and the selection; the baseline: the aligner's launch).
One JSON line per part.

The aligner is the loop detector's (30 iterations, Cauchy 0.05, projective finder: MULTI.json:602-630), the thresholds are the loop detector's (500 / 0.1 /
0.8: MULTI.json:964-986).
Part a: 1000 candidates of BASELINE configs[1] geometry -- 1000 scans of 1081 beams, one each, against a 100 000-point map.
Part b: 65 536 candidates of BASELINE configs[3] geometry -- 2048 distinct scans x 32 perturbed guesses each, against the 100 000-point submap.

Parity gate, inside every run and before any time is reported: the new call's verdict and the host route's both equal api.align_rank on the statuses,
iteration counts and last rows the C++ program's lsm2d_align_batch returned, and the new call's rows equal that call's rows for the selected candidates, byte
for byte.

    python tests/bench/align_select_bench.py [--n 1000] [--map 100000] [--unique 2048] [--per-scan 32] [--k 64] [--steps 20] [--warmup 2] [--parts a,b]

Measured figures: README.md, DESIGN.md section 8 and profiles/r25/."""
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


def run_part(api, exe, tmp, part, scans, offs, m, poses, index, sel, args):
    n = len(poses)
    files = {k: os.path.join(tmp, "%s_%s.bin" % (part, k)) for k in ("scans", "offsets", "map", "poses", "index", "out")}
    np.ascontiguousarray(scans, np.float32).tofile(files["scans"]); np.ascontiguousarray(offs, np.int32).tofile(files["offsets"])
    np.ascontiguousarray(m, np.float32).tofile(files["map"]); np.ascontiguousarray(poses, np.float32).tofile(files["poses"])
    (np.zeros(0, np.int32) if index is None else np.ascontiguousarray(index, np.int32)).tofile(files["index"])
    out = subprocess.run([exe, files["scans"], files["offsets"], files["map"], files["poses"], files["index"], str(COLS), repr(TAU), str(ITERATIONS),
                          str(sel.min_inliers), bits_arg(sel.max_chi_per_inlier), bits_arg(sel.min_inlier_ratio), str(args.k), str(args.steps), str(args.warmup), files["out"]],
                         check=True, capture_output=True, text=True).stdout
    r = json.loads(out)
    # ---- parity gate: both verdicts are align_rank's on what that run's lsm2d_align_batch returned
    raw = open(files["out"], "rb").read()
    status = np.frombuffer(raw, np.int32, n, 0); its = np.frombuffer(raw, np.int32, n, 4 * n); last = np.frombuffer(raw, api.STATS_DTYPE, n, 8 * n)
    want, n_acc, n_suc = api.align_rank(status, its, last, sel, args.k)
    assert r["rows_equal"] == 1, "parity: the selected rows against lsm2d_align_batch's"
    assert r["n_accepted"] == [n_acc, n_acc] and r["n_success"] == [n_suc, n_suc], "parity: the counts against align_rank"
    assert r["index_select"] == want.tolist() and r["index_baseline"] == want.tolist(), "parity: the selection against align_rank"
    new, base = r["select_ms"], r["baseline_ms"]
    return dict(bench="align_select", part=part, n_candidates=n, k=args.k, steps=args.steps, iterations=ITERATIONS, select_ms=new[0], baseline_ms=base[0],
                baseline_over_select=round(base[0] / new[0], 3), select_ms_min_max=new[1:], baseline_ms_min_max=base[1:], select_kernel_ms=r["select_kernel_ms"],
                baseline_kernel_ms=r["baseline_kernel_ms"], baseline_stats_bytes=int(n) * int(r["stats_rows_per_candidate"]) * 28, n_accepted=n_acc, n_success=n_suc,
                n_selected=len(want), thresholds=[sel.min_inliers, sel.max_chi_per_inlier, sel.min_inlier_ratio], best_candidate=int(want[0]) if len(want) else -1,
                parity="ok")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--unique", type=int, default=2048)
    ap.add_argument("--per-scan", type=int, default=32)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="a,b")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, HERE_ROOT)
    from srrg2_laser_slam_2d_amd import api, synth
    sel = api.SelectParams()      # the loop detector's thresholds
    parts = args.parts.split(",")
    with tempfile.TemporaryDirectory() as tmp:
        exe = bench_common.build("align_select_bench.cpp", tmp)
        lines = []
        if "a" in parts:
            wl = synth.make_workload(args.n, args.map, seed=1)
            lines.append(run_part(api, exe, tmp, "a", wl.scan_points, wl.scan_offsets, wl.map_points, np.ascontiguousarray(wl.x0, np.float32), None, sel, args))
        if "b" in parts:      # bench.py's configs[3]: distinct scans x perturbed guesses each, start poses within 0.05 of the truth
            n_cand = args.unique * args.per_scan
            world = synth.make_world(1)
            wl = synth.make_workload(args.unique, args.map, seed=1, world=world, map_points=np.zeros((0, 4), np.float32))
            m = synth.make_map(world, args.map, seed=1)
            idx = (np.arange(n_cand) % args.unique).astype(np.int32)
            delta = synth.Stream(1001, salt=9).uniform(3 * n_cand, -0.05, 0.05).reshape(n_cand, 3)
            x0 = synth.invert_poses(synth.compose_poses(synth.invert_poses(wl.x_true)[idx], delta)).astype(np.float32)
            lines.append(run_part(api, exe, tmp, "b", wl.scan_points, wl.scan_offsets, m, x0, idx, sel, args))
        for ln in lines:
            bench_common.emit(ln, args.label)


if __name__ == "__main__":
    main()
