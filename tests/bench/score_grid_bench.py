#!/usr/bin/env python3
"""lsm2d_score_grid_select (a pose grid made on the device and scored coarse to fine: no upload of hypotheses, one copy down, one wait) against the same
pyramid made of existing calls -- lsm2d_score_aligner_select per level, the children made on the host -- and, for context, against the exhaustive
64 x 64 x 16 grid through lsm2d_score_aligner_select.  All routes run through the bare C ABI from one C++ program (tests/cpp/score_grid_bench.cpp, built here
with g++), alternating call by call; medians over --steps timed calls after --warmup, wall clock around calls that end in their wait, kernel timing off;
`*_kernel_ms` is lsm2d_last_kernel_ms of one more call with kernel timing on.  The program is run --runs times (default 2): the per-level route's own movement
between the runs is the yardstick's noise.

ONE scan of 1081 beams against the 100 000-point map of relocalize_bench.py, the loop detector's aligner (Cauchy 0.05, projective finder: MULTI.json:602-630)
and thresholds (500 / 0.1 / 0.8: MULTI.json:964-986; --min-inliers lowers the first).  The coarse grid is 16 x 16 x 16 cells over +-0.5 m and +-0.08 rad round
a centre a little off the truth; the pyramids are 16 x 16 x 16 -> refine (4, 4, 1), and 16 x 16 x 16 -> refine (2, 2, 1) twice; k_parents 64, k 64.
Part "pyramids": the thresholds judge every level.  Part "nobody": the coarse thresholds pass nobody -- the per-level route stops after level 0, the new call
still runs its pads: the pad cost.

Parity gate, inside every run and before any time is reported: every output of the new call equals the per-level route's byte for byte.

    python tests/bench/score_grid_bench.py [--map 100000] [--steps 20] [--warmup 2] [--runs 2] [--min-inliers N] [--parts pyramids,nobody]

Measured figures: README.md and profiles/r31/."""
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
CENTER_OFF = (0.013, -0.021, 0.004)
STEP = (1.0 / 16, 1.0 / 16, 0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--map", type=int, default=100000)
    ap.add_argument("--min-inliers", type=int, default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--parts", default="pyramids,nobody")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, HERE_ROOT)
    from srrg2_laser_slam_2d_amd import api, synth
    sel = api.SelectParams()      # the loop detector's thresholds
    if args.min_inliers is not None:
        sel.min_inliers = args.min_inliers
    with tempfile.TemporaryDirectory() as tmp:
        exe = bench_common.build("score_grid_bench.cpp", tmp)
        wl = synth.make_workload(4, args.map, seed=1)
        lo, hi = int(wl.scan_offsets[0]), int(wl.scan_offsets[1])
        scan, m = os.path.join(tmp, "scan.bin"), os.path.join(tmp, "map.bin")
        np.ascontiguousarray(wl.scan_points[lo:hi], np.float32).tofile(scan); np.ascontiguousarray(wl.map_points, np.float32).tofile(m)
        center = np.float32(wl.x0[0]) + np.float32(CENTER_OFF)
        for part in args.parts.split(","):
            runs = []
            for _ in range(args.runs):
                out = subprocess.run([exe, scan, m, str(COLS), repr(TAU)] + [bits_arg(v) for v in center] + [bits_arg(v) for v in STEP] +
                                     [str(sel.min_inliers), bits_arg(sel.max_chi_per_inlier), bits_arg(sel.min_inlier_ratio), "1" if part == "nobody" else "0", str(args.steps), str(args.warmup)],
                                     check=True, capture_output=True, text=True).stdout
                r = json.loads(out)
                assert all(p["outputs_equal"] == 1 for p in r["pyramids"]), "parity: the new call's outputs against the per-level route's"
                runs.append(r)
            for i, p0 in enumerate(runs[0]["pyramids"]):
                per_level = [r["pyramids"][i]["per_level_ms"][0] for r in runs]; grid = [r["pyramids"][i]["grid_ms"][0] for r in runs]
                line = dict(bench="score_grid", part=part, n_levels=p0["n_levels"], refine=p0["refine"], k_parents=64, k=64, steps=args.steps, runs=args.runs,
                            grid_ms=grid, per_level_ms=per_level, exhaustive_ms=[r["exhaustive_ms"][0] for r in runs],
                            per_level_movement_ms=round(max(per_level) - min(per_level), 4),
                            grid_minus_per_level_ms=[round(g - b, 4) for g, b in zip(grid, per_level)],
                            grid_ms_min_max=[r["pyramids"][i]["grid_ms"][1:] for r in runs], per_level_ms_min_max=[r["pyramids"][i]["per_level_ms"][1:] for r in runs],
                            grid_kernel_ms=[r["pyramids"][i]["grid_kernel_ms"] for r in runs], exhaustive_kernel_ms=[r["exhaustive_kernel_ms"] for r in runs],
                            level_counts=p0["level_counts"], exhaustive_accepted=runs[0]["exhaustive_accepted"],
                            best_to_exhaustive_best_m=p0["best_to_exhaustive_best_m"], best_to_exhaustive_best_rad=p0["best_to_exhaustive_best_rad"],
                            same_level0_cell=p0["same_level0_cell"], thresholds=[sel.min_inliers, sel.max_chi_per_inlier, sel.min_inlier_ratio], parity="ok")
                bench_common.emit(line, args.label)


if __name__ == "__main__":
    main()
