#!/usr/bin/env python3
"""lsm2d_occupancy_update_scans into a LOG-ODDS grid set (ABI 0.7.14: one clamped vote per scan and cell, the scans in list order) against
  (a) host    the definition's loops on ONE host core at -O2 with the grid kept on the host (tests/cpp/occupancy_scan_ref.cpp makes each scan's rays,
              tests/cpp/occupancy_logodds_ref.cpp votes), and
  (b) counts  THE SAME CALL on a counts set of the same geometry in the same process: what the once-per-scan rule costs.
All routes run through the bare C ABI from one C++ program (tests/cpp/occupancy_logodds_bench.cpp, built here with g++), alternating call by call; medians
over --steps timed calls after --warmup, wall clock round calls that end in their wait, kernel timing off.  The program is run --runs times (default 2): each
route's own movement between the runs is the yardstick's noise.  One more call of each device route with kernel timing on gives lsm2d_last_kernel_ms and the
median and the longest lifetime of the tile workgroups that had work, under both kinds of set.

Parts and variants are tests/bench/occupancy_scan_bench.py's: live (one scan into 2048 x 2048), redraw (1000 scans into 1024 x 768), fleet (256 scans into
256 grids of 512 x 512); `none` (every beam a return) and `no_return` (range_max 12 m, trace_range 10 m).

Parity gate, inside every run: the log-odds set's cells equal the host route's byte for byte after the first call of each route and after the last, and the
ray counts equal the counts call's.  There is no speed gate: `host_route_wins` says whether the host's best run beats the log-odds call's worst, and
`logodds_above_counts` whether the log-odds call's median lies above the counts call's by more than the counts call's own movement between its runs.

    python tests/bench/occupancy_logodds_bench.py [--steps 20] [--warmup 2] [--runs 2] [--parts live,redraw,fleet] [--variants none,no_return]

Measured figures: README.md, DESIGN.md section 8 and profiles/r37/."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

import bench_common
import occupancy_scan_bench as scan_bench      # (the parts, the sensor and the variants are that bench's)
from bench_common import HERE_ROOT, bits_arg as bits

LOGODDS = (85, -40, -200, 350)      # l_hit, l_miss, l_min, l_max at 0.01 log-odds per unit: p_hit 0.7, p_miss 0.4, clamps at 0.12 and 0.97


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--parts", default="live,redraw,fleet")
    ap.add_argument("--variants", default="none,no_return")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert args.steps >= 20, "medians of at least 20 timed steps"
    sys.path.insert(0, HERE_ROOT)
    from srrg2_laser_slam_2d_amd import synth
    with tempfile.TemporaryDirectory() as tmp:
        exe = bench_common.build(["occupancy_logodds_bench.cpp", "occupancy_scan_ref.cpp", "occupancy_logodds_ref.cpp"], tmp, flags=("-O2", "-ffp-contract=off"))
        for part in args.parts.split(","):
            ranges, poses, grid, n_grids, geo = scan_bench._inputs(synth, part)
            fr, fq, fg = (os.path.join(tmp, n) for n in ("ranges.bin", "poses.bin", "grid.bin"))
            np.ascontiguousarray(ranges, np.float32).tofile(fr); np.ascontiguousarray(poses, np.float32).tofile(fq)
            if grid is not None:
                grid.tofile(fg)
            for variant in args.variants.split(","):
                range_max, trace = scan_bench.VARIANTS[variant]
                share = float(np.mean(~(ranges <= np.float32(range_max))))
                runs = []
                for _ in range(args.runs):
                    p = subprocess.run([exe, fr, fq, fg if grid is not None else "-", str(n_grids), str(scan_bench.N_BEAMS), bits(scan_bench.ANGLE_MIN),
                                        bits(scan_bench.ANGLE_MAX), bits(scan_bench.RANGE_MIN), bits(range_max), bits(trace), "1", bits(geo[0]), bits(geo[1]), bits(geo[2]),
                                        str(geo[3]), str(geo[4]), str(args.steps), str(args.warmup)] + [str(v) for v in LOGODDS], capture_output=True, text=True)
                    assert p.returncode in (0, 3), p.stderr[-2000:]
                    r = json.loads(p.stdout)
                    assert r["outputs_equal"] == 1, "parity: the log-odds set's cells against the host route's, the ray counts against the counts call's"
                    runs.append(r)
                med = lambda key: [r[key][0] for r in runs]      # noqa: E731
                lo, cnt, host = med("logodds_call_ms"), med("counts_call_ms"), med("host_route_ms")
                col = lambda key: [r[key] for r in runs]      # noqa: E731
                line = dict(bench="occupancy_logodds", part=part, variant=variant, scans=runs[0]["scans"], beams=runs[0]["beams"], grids=n_grids, width=geo[3], height=geo[4],
                            resolution=geo[2], range_max=range_max, trace_range=trace, no_return_share=round(share, 4), hit_rays=runs[0]["hit_rays"],
                            clear_rays=runs[0]["clear_rays"], dropped=runs[0]["dropped"], logodds=list(LOGODDS), steps=args.steps, runs=args.runs,
                            logodds_call_ms=lo, counts_call_ms=cnt, host_route_ms=host,
                            logodds_call_movement_ms=round(max(lo) - min(lo), 4), counts_call_movement_ms=round(max(cnt) - min(cnt), 4),
                            host_route_movement_ms=round(max(host) - min(host), 4),
                            logodds_call_ms_min_max=[r["logodds_call_ms"][1:] for r in runs], counts_call_ms_min_max=[r["counts_call_ms"][1:] for r in runs],
                            host_route_ms_min_max=[r["host_route_ms"][1:] for r in runs],
                            logodds_kernel_ms=col("logodds_kernel_ms"), counts_kernel_ms=col("counts_kernel_ms"),
                            logodds_tile_workgroup_median_us=col("logodds_tile_workgroup_median_us"), logodds_tile_workgroup_longest_us=col("logodds_tile_workgroup_longest_us"),
                            counts_tile_workgroup_median_us=col("counts_tile_workgroup_median_us"), counts_tile_workgroup_longest_us=col("counts_tile_workgroup_longest_us"),
                            host_route_wins=bool(min(host) < max(lo)),
                            logodds_above_counts=bool(float(np.median(lo)) - float(np.median(cnt)) > max(cnt) - min(cnt)),
                            logodds_over_counts=round(float(np.median(lo)) / float(np.median(cnt)), 3), parity="ok")
                bench_common.emit(line, args.label)


if __name__ == "__main__":
    main()
