#!/usr/bin/env python3
"""Where a k_align workgroup's cycles go (library built with -DLSM2D_PHASE_PROBE): query / projection phase, barrier + reduction, solve + rest.
usage: LSM2D_EXTRA_HIPCC_FLAGS=-DLSM2D_PHASE_PROBE python -m srrg2_laser_slam_2d_amd.build --force && python tools/phase_probe.py <role> <finder>
With --full-length (role A, projective; LSM2D_EXTRA_HIPCC_FLAGS="-DLSM2D_PHASE_PROBE=3 -DLSM2D_DEBUG_UNITS": buckets unit lists | stream | everything else, and the
fast-forward's filled-in statistics rows marked): only the alignments of the headline batch that EXECUTE every iteration -- the ones the launch waits for behind the
fast-forward -- first inside the whole batch, then by themselves, one workgroup per otherwise empty CU: what one of their iterations costs there, stream and the rest.
Built with -DLSM2D_PHASE_PROBE=4 instead (pass --mode4: the library cannot say how it was built) the buckets are bin walk + wave sums | wave 0's stretch behind the sums'
barrier | everything else, and the lone workgroups are measured once more with want_stats=False: the launch bench.py times writes no statistics rows and no digest.
With --lists5 / --lists6 (LSM2D_EXTRA_HIPCC_FLAGS="-DLSM2D_PHASE_PROBE=5 -DLSM2D_DEBUG_UNITS -DLSM2D_DEBUG_CAND", or =6) the same alignments get the candidate lists'
columns: cycles in the unit list's plain stream | the build iteration's stream | a list-served gather (5), in a blockers pass of its own | the collect pass | unit-list
rebuilds (6), each in all and per iteration of its kind, what is in none of them, the entries of every list built and the maybes its build queued ("cand_queue" 1; the
streamed points beside them are units x block steps x 2, an upper bound) -- inside the whole batch and alone on a CU -- and the maybes per build over the whole batch."""
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
LISTS = 0      # --lists5 / --lists6: the candidate lists' columns, library built with -DLSM2D_PHASE_PROBE=5 (or 6) -DLSM2D_DEBUG_UNITS -DLSM2D_DEBUG_CAND
for m in (5, 6):
    if "--lists%d" % m in sys.argv:
        sys.argv.remove("--lists%d" % m); LISTS = m; FULL_LENGTH = True
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
def stamped_abs(n):      # the same with all three buckets as they were stamped (the dump's header line carries what the third column is relative to)
    lines = open(dump).read().split("\n")
    t0 = [int(l.split("t0=")[1]) for l in lines if l.startswith("# launch") and "t0=" in l][-1]
    rows = [l.split() for l in lines if l and not l.startswith("#")][-n:]
    a = np.array([[int(r[1]), int(r[2]), (int(r[3]) + t0) % 2 ** 64, int(r[4], 16)] for r in rows], dtype=np.float64)      # (exact integers: the dump's difference may have wrapped)
    return a[:, 0], a[:, 1], a[:, 2], a[:, 3]
if LISTS:
    # The candidate lists' columns: per iteration of bench.py's full-length alignments, cycles of thread 0 in the unit list's stream, in the build iteration's
    # stream, in a blockers pass of its own, in the collect pass, in a list-served gather, in unit-list rebuilds and in everything else; entries per list.
    # Mode 5 stamps plain stream | build iteration's stream | gather, mode 6 blockers pass | collect pass | unit-list rebuilds: two builds, two runs.
    its = 20
    BLOCK_STEPS = 2 * ((((len(wl.map_points) + 1) // 2 + 511) // 512 + 13) // 14)      # cull_block_steps: steps of two points in a unit
    names = {5: ("plain stream", "build iteration's stream", "gather"), 6: ("blockers pass", "collect pass", "unit-list rebuilds")}[LISTS]
    ctx.set_option("align_path", 1); ctx.set_option("zero_copy_max", 0)
    def report(label, res, idx, n):
        life, b0, b1, b2 = stamped_abs(n)
        lo = res.stats["pair_digest_lo"].astype(np.int64); entries = res.stats["pair_digest_hi"].astype(np.int64)
        state = lo & 3; maybes = lo >> 2; streamed = 2 * BLOCK_STEPS * res.stats["n_outliers"].astype(np.int64)      # (of a build iteration: LSM2D_DEBUG_CAND; LSM2D_DEBUG_UNITS puts the unit list's length in place of the outliers)
        for j, i in enumerate(idx):
            ran = int(res.iterations[i]) if res.iterations[i] <= its else its
            st = state[i, :ran]
            n_plain, n_build, n_served = int((st == 0).sum()), int((st == 2).sum()), int((st == 1).sum())
            per = {5: (n_plain, n_build, n_served), 6: (n_build, n_build, ran)}[LISTS]
            cells = ["%s %.0f cyc in all, %d iterations, %.0f each" % (nm, b[i], k, b[i] / max(k, 1)) for nm, b, k in zip(names, (b0, b1, b2), per)]
            print("  %s: alignment %d: lifetime %.0f cyc over %d iterations (%d plain, %d build, %d served); %s; everything else in this mode %.0f; entries per list %s, maybes queued of at most so many streamed points per build %s (state per iteration %s)"
                  % (label, idx_names[j], life[i], ran, n_plain, n_build, n_served, "; ".join(cells), life[i] - b0[i] - b1[i] - b2[i],
                     entries[i, :ran][st == 2].tolist(), ["%d of %d" % mv for mv in zip(maybes[i, :ran][st == 2].tolist(), streamed[i, :ran][st == 2].tolist())], "".join(str(int(v)) for v in st)))
    for _ in range(3):
        r = al.compute_batch([scans], [mp], x0, want_stats=True)
    executed = ((np.arange(r.stats.shape[1])[None, :] < r.iterations[:, None]) & ~(r.stats["chi_outliers"] < 0)).sum(1)
    full = np.flatnonzero(executed == its)
    life = stamped_abs(len(x0))[0]
    print("mode %d, fast_forward %d, cand_lists %d: kernel %.3f ms; alignments that execute all %d iterations: %s; lifetime of all: median %.0f cyc, max %.0f cyc; lists built %d, iterations served %d"
          % (LISTS, ctx.get_option("fast_forward"), ctx.get_option("cand_lists"), r.kernel_ms, its, full.tolist(), np.median(life), life.max(), ctx.get_option("last_cand_builds"), ctx.get_option("last_cand_iterations")))
    # the provisional test's yield over every build of the batch: maybes / streamed points per build (rows the fast-forward filled in were not executed)
    lo_all = r.stats["pair_digest_lo"].astype(np.int64)
    ran_all = (np.arange(r.stats.shape[1])[None, :] < r.iterations[:, None]) & ~(r.stats["chi_outliers"] < 0) & ((lo_all & 3) == 2)
    mb = (lo_all >> 2)[ran_all]; sm = 2 * BLOCK_STEPS * r.stats["n_outliers"].astype(np.int64)[ran_all]; en = r.stats["pair_digest_hi"].astype(np.int64)[ran_all]
    if len(mb):
        sh = mb / np.maximum(sm, 1)
        print("  builds with statistics rows: %d; maybes per build: min %d, median %d, p90 %d, max %d, sum %d; streamed points per build (units x block: an upper bound): median %d, sum %d; share: median %.3f, p90 %.3f, max %.3f, overall %.3f; builds with more than 16384 maybes: %d; entries per list: median %d, max %d"
              % (len(mb), mb.min(), np.median(mb), np.percentile(mb, 90), mb.max(), mb.sum(), np.median(sm), sm.sum(), np.median(sh), np.percentile(sh, 90), sh.max(), mb.sum() / max(sm.sum(), 1), int((mb > 16384).sum()), np.median(en), en.max()))
    idx_names = full.tolist()
    report("inside the whole batch", r, full.tolist(), len(x0))
    sub = api.CloudSet(ctx, np.concatenate([wl.scan_points[wl.scan_offsets[i]:wl.scan_offsets[i + 1]] for i in full]),
                       np.concatenate([[0], np.cumsum([wl.scan_offsets[i + 1] - wl.scan_offsets[i] for i in full])]).astype(np.int32))
    for _ in range(3):
        r1 = al.compute_batch([sub], [mp], x0[full], want_stats=True)
    assert np.array_equal(r1.pose.view(np.uint32), r.pose[full].view(np.uint32)) and np.all(r1.iterations == its)
    report("alone, a CU each", r1, list(range(len(full))), len(full))
    os.remove(dump)
    sys.exit(0)
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
