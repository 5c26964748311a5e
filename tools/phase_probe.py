#!/usr/bin/env python3
"""Where a k_align workgroup's cycles go (library built with -DLSM2D_PHASE_PROBE): query / projection phase, barrier + reduction, solve + rest.
usage: LSM2D_EXTRA_HIPCC_FLAGS=-DLSM2D_PHASE_PROBE python -m srrg2_laser_slam_2d_amd.build --force && python tools/phase_probe.py <role> <finder>
With --full-length (role A, projective; LSM2D_EXTRA_HIPCC_FLAGS="-DLSM2D_PHASE_PROBE=3 -DLSM2D_DEBUG_UNITS": buckets unit lists | stream | everything else, and the
fast-forward's filled-in statistics rows marked): only the alignments of the headline batch that EXECUTE every iteration -- the ones the launch waits for behind the
fast-forward -- first inside the whole batch, then by themselves, one workgroup per otherwise empty CU: what one of their iterations costs there, stream and the rest.
Built with -DLSM2D_PHASE_PROBE=4 instead (pass --mode4: the library cannot say how it was built) the buckets are bin walk + wave sums | wave 0's stretch behind the sums'
barrier | everything else, and the lone workgroups are measured once more with want_stats=False: the launch bench.py times writes no statistics rows and no digest."""
import math, os, sys, tempfile
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
dump = tempfile.mktemp(suffix=".stamps"); os.environ["LSM2D_DUMP_STAMPS"] = dump
from srrg2_laser_slam_2d_amd import api, synth

FULL_LENGTH = "--full-length" in sys.argv
if FULL_LENGTH:
    sys.argv.remove("--full-length")
MODE4 = "--mode4" in sys.argv
if MODE4:
    sys.argv.remove("--mode4")
role, kind = (sys.argv + (["A", "projective"] if FULL_LENGTH else ["B", "distmap"]))[1:3]
ctx = api.Context(0, kernel_timing=True); ctx.set_option("clock_stride", 1)
for kv in filter(None, os.environ.get("LSM2D_BENCH_OPTIONS", "").split(",")):
    ctx.set_option(kv.partition("=")[0].strip(), int(kv.partition("=")[2]))
wl = synth.make_workload(1000, 100000, seed=0)
if kind == "projective":
    f = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0), 0.5, 0.8)
elif kind == "nn":
    f = api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.5 if role == "B" else 0.3)
else:
    f = api.CorrespondenceFinderNN2D(ctx, max_distance_m=0.5, resolution=0.05)
al = api.MultiAligner2D(ctx, max_iterations=20, min_num_inliers=10)
al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(f, min_num_correspondences=10))
scans = api.CloudSet(ctx, wl.scan_points, wl.scan_offsets); mp = api.CloudSet(ctx, wl.map_points)
x0 = wl.x0 if role == "A" else synth.invert_poses(wl.x0.astype(np.float64)).astype(np.float32)
def stamped(n):      # the last launch's stamps: [n] x (lifetime, first bucket, third bucket) in cycles -- the dump gives the second relative to its minimum: it is the remainder
    rows = [l.split() for l in open(dump) if not l.startswith("#")][-n:]
    a = np.array([[int(v) for v in r[1:3]] + [int(r[4], 16)] for r in rows], dtype=np.float64)
    return a[:, 0], a[:, 1], a[:, 2]
if FULL_LENGTH:
    its = al.param_max_iterations if hasattr(al, "param_max_iterations") else 20
    ctx.set_option("align_path", 1); ctx.set_option("zero_copy_max", 0)      # k_align, results by copies, whatever the batch size
    for _ in range(3):
        r = al.compute_batch([scans], [mp], x0, want_stats=True)
    executed = ((np.arange(r.stats.shape[1])[None, :] < r.iterations[:, None]) & ~(r.stats["chi_outliers"] < 0)).sum(1)
    full = np.flatnonzero(executed == its)
    life, lists, rest = stamped(len(x0))
    print("fast_forward %d: kernel %.3f ms; iterations executed: mean %.2f; alignments that execute all %d: %s" % (ctx.get_option("fast_forward"), r.kernel_ms, executed.mean(), its, full.tolist()))
    print("  inside the batch: lifetime of those %s kcyc (median of all %.0f, max of all %.0f)" % (np.round(life[full] / 1e3).astype(int).tolist(), np.median(life) / 1e3, life.max() / 1e3))
    if len(full):
        sub = api.CloudSet(ctx, np.concatenate([wl.scan_points[wl.scan_offsets[i]:wl.scan_offsets[i + 1]] for i in full]),
                           np.concatenate([[0], np.cumsum([wl.scan_offsets[i + 1] - wl.scan_offsets[i] for i in full])]).astype(np.int32))
        for _ in range(3):
            r1 = al.compute_batch([sub], [mp], x0[full], want_stats=True)
        assert np.array_equal(r1.pose.view(np.uint32), r.pose[full].view(np.uint32)) and np.all(r1.iterations == its)
        life, lists, rest = stamped(len(full))
        def lone_stretch(label, res, n):      # mode 4's buckets of the last launch
            life, walk, tail = stamped(n)
            other = life - walk - tail
            print("  by themselves, %s (%d workgroups, a CU each): kernel %.3f ms; lifetime %s kcyc; per iteration: %s kcyc = bin walk + wave sums %s + wave 0's stretch %s + everything else (prologue / %d included) %s"
                  % (label, n, res.kernel_ms, np.round(life / 1e3).astype(int).tolist(), np.round(life / its / 1e3, 1).tolist(), np.round(walk / its / 1e3, 2).tolist(),
                     np.round(tail / its / 1e3, 2).tolist(), its, np.round(other / its / 1e3, 1).tolist()))
        if MODE4:
            lone_stretch("statistics rows written", r1, len(full))
            for _ in range(3):
                r0 = al.compute_batch([sub], [mp], x0[full], want_stats=False)
            assert np.array_equal(r0.pose.view(np.uint32), r1.pose.view(np.uint32)) and np.all(r0.iterations == its)
            lone_stretch("want_stats=False", r0, len(full))
            os.remove(dump)
            sys.exit(0)
        stream = life - lists - rest
        print("  by themselves (%d workgroups, a CU each): kernel %.3f ms; lifetime %s kcyc; per iteration: %s kcyc = unit lists %s + stream %s + everything else (prologue / %d included) %s"
              % (len(full), r1.kernel_ms, np.round(life / 1e3).astype(int).tolist(), np.round(life / its / 1e3, 1).tolist(), np.round(lists / its / 1e3, 1).tolist(),
                 np.round(stream / its / 1e3, 1).tolist(), its, np.round(rest / its / 1e3, 1).tolist()))
    os.remove(dump)
    sys.exit(0)
for _ in range(5):
    r = al.compute_batch([scans], [mp], x0) if role == "A" else al.compute_batch([mp], [scans], x0)
rows = [l.split() for l in open(dump) if not l.startswith("#")][-1000:]
a = np.array([[int(v) for v in r[1:4]] + [int(r[4], 16)] for r in rows], dtype=np.float64)
# columns as dumped: lifetime cycles, query cycles, (reduce cycles - t0), solve cycles -- the dump subtracts the smallest third column
life, q, solve = a[:, 0], a[:, 1], a[:, 3]
red = life - q - solve          # (the dumped third column is relative to its minimum: take the remainder instead)
print("role %s / %s: kernel %.3f ms; per workgroup (median over %d): lifetime %.0f kcyc = query %.0f + barrier wait / reduction / prologue %.0f + solve and next-iteration set-up %.0f kcyc"
      % (role, kind, r.kernel_ms, len(a), np.median(life) / 1e3, np.median(q) / 1e3, np.median(red) / 1e3, np.median(solve) / 1e3))
os.remove(dump)
