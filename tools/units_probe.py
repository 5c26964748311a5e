"""How long are the culled stream's unit lists, and how often are they rebuilt?  With --iterations: how many of its iterations does an alignment of the
headline workload actually EXECUTE, and which periods does the fast-forward find?  (GPU box, DIAGNOSTICS BUILD: the library must be built with
LSM2D_EXTRA_HIPCC_FLAGS=-DLSM2D_DEBUG_UNITS, which puts the list length / rebuild flag of slice 0 in place of the outlier statistics and marks every row the
fast-forward filled in for a skipped iteration with minus the period it skipped by -- and, where "fast_forward" 2 FINISHED the alignment from the ring at that
match, so that nothing runs behind the filled-in rows, with minus (the period + 0.5).  "fast_forward" 1 skips whole periods and replays the remainder: its
alignments count as "skipped and replayed", also those whose remainder happens to be empty.)
usage: LSM2D_EXTRA_HIPCC_FLAGS=-DLSM2D_DEBUG_UNITS python -m srrg2_laser_slam_2d_amd.build --force && python tools/units_probe.py [--iterations]"""
import numpy as np, math, os, sys
sys.path.insert(0, '.')
from srrg2_laser_slam_2d_amd import api, synth
ITERATIONS = "--iterations" in sys.argv
if ITERATIONS:      # configs[1] as bench.py makes it (seed 0, pose set 0): 1000 scans of 1081 beams cast against the world, a 100k-point map
    world = synth.make_world(0)
    wl = synth.make_workload(1000, 100000, seed=0, n_beams=1081, world=world, map_points=np.zeros((0, 4), np.float32))
    wl.map_points = synth.make_map(world, 100000, seed=0)
else:
    wl = synth.make_workload(64, 100000, seed=0)
ctx = api.Context(0)
ctx.set_option("align_path", 1)
for kv in filter(None, os.environ.get("LSM2D_BENCH_OPTIONS", "").split(",")):      # e.g. fast_forward=1: the rule that skips whole periods and replays the remainder
    ctx.set_option(kv.partition("=")[0].strip(), int(kv.partition("=")[2]))
proj = api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)
al = api.MultiAligner2D(ctx, max_iterations=20, min_num_inliers=10)
al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(api.CorrespondenceFinderProjective2f(ctx, proj, 0.5, 0.8), min_num_correspondences=10))
fx = api.CloudSet(ctx, wl.scan_points, wl.scan_offsets); mv = api.CloudSet(ctx, wl.map_points)
r = al.compute_batch([fx], [mv], wl.x0, want_stats=True)
u = r.stats["n_outliers"].astype(float); rb = r.stats["chi_outliers"]
if ITERATIONS:
    n = len(r.status)
    rows = np.arange(rb.shape[1])[None, :] < r.iterations[:, None]      # the iterations the alignment counts
    skipped = rows & (rb < 0)
    executed = (rows & ~skipped).sum(1)
    first = -rb[np.arange(n), skipped.argmax(1)]      # the first filled-in row's mark: the period, + 0.5 where the alignment was finished there
    period = np.where(skipped.any(1), np.floor(first), 0).astype(int)      # of the first skip (0: nothing skipped)
    finished = skipped.any(1) & (first != np.floor(first))
    replayed = skipped.any(1) & ~finished
    behind = np.arange(rb.shape[1])[None, :] > skipped.argmax(1)[:, None]
    replays = (rows & ~skipped & behind & replayed[:, None]).sum(1)      # iterations executed behind the first skip: the remainder of a period, run again
    print("fast_forward %d, %d alignments, statuses %s, iterations counted %s" % (ctx.get_option("fast_forward"), n, dict(zip(*np.unique(r.status, return_counts=True))),
                                                                                 dict(zip(*np.unique(r.iterations, return_counts=True)))))
    print("iterations executed: mean %.2f of 20 (first 160 alignments: %.2f), median %d, p90 %d, max %d; alignments that run all 20: %d"
          % (executed.mean(), executed[:160].mean(), np.median(executed), np.percentile(executed, 90), executed.max(), int((executed == 20).sum())))
    print("histogram of iterations executed (1 .. 20):", np.bincount(executed, minlength=21)[1:].tolist())
    print("alignments finished from the ring: %d; skipped and replayed: %d (%d iterations replayed behind a skip); neither -- no repeat found, or found by the last iteration: %d"
          % (int(finished.sum()), int(replayed.sum()), int(replays.sum()), int(n - finished.sum() - replayed.sum())))
    print("period of the first skip (0 = none, 1 .. 16):", np.bincount(period, minlength=17).tolist())
    # (a filled-in row carries the list length of the iteration it repeats: what the skipped iteration would have streamed)
    print("units streamed against what all counted iterations would have streamed: %.3f" % ((u * (rows & ~skipped)).sum() / max(1.0, (u * rows).sum())))
    sys.exit(0)
print("units per iteration (mean over 64 alignments):", np.round(u.mean(0)).astype(int).tolist())
print("fraction of 3584:", np.round(u.mean(0) / 3584, 3).tolist())
print("rebuild flag at end of iteration (mean):", np.round(rb.mean(0), 2).tolist())
print("overall mean fraction", u.mean() / 3584)
