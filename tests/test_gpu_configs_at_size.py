"""GPU parity tests, BASELINE configs at their full sizes, the loop-closure sweep (row f3), the multi-rank bench rehearsals (row e), the committed golden bits.

The HIP path (through the C ABI) against the CPU oracle on identical inputs.  Bars (BASELINE.json north_star): index work bit-exact; H / b / chi 2e-5 relative
against the fp64 oracle and BITWISE against the fp32 oracle in the launch's order; aligner pose within 1e-4 m / 1e-4 rad (gpu_helpers.POSE_TOL_*)."""
import json
import math

import numpy as np
import pytest

import fuzz_cases
from conftest import golden_path
from gpu_helpers import (_same_correspondence_sets, _assert_bitwise_equal_to_device_order_oracle, _pose_diff, _Envelope, _projector, _aligner, _nn_aligner, _ranges_in_pose_out_step, _kd_finder, _kd_aligner, _neg_eps, _oracle_slice, POSE_TOL_M, POSE_TOL_RAD)
from srrg2_laser_slam_2d_amd import api, synth

pytestmark = pytest.mark.gpu


def test_full_size_batch_properties(ctx):
    """BASELINE configs[1] at full size: 1000 scans x 100k-point map x 20 iterations.  Too slow for the
    scalar oracle in a unit test, so it is checked through size-independent properties: convergence to the
    generating pose on noise-free data, run-to-run bitwise determinism, permutation equivariance."""
    wl = synth.make_workload(1000, 100000, seed=0)
    al = _aligner(ctx)
    fixed = api.CloudSet(ctx, wl.scan_points, wl.scan_offsets); moving = api.CloudSet(ctx, wl.map_points)
    res = al.compute_batch([fixed], [moving], wl.x0)
    assert np.all(res.status == 0)
    d = np.abs(res.pose - wl.x_true)
    assert d[:, :2].max() < POSE_TOL_M and d[:, 2].max() < POSE_TOL_RAD
    perm = np.argsort(synth.Stream(9).uniform(1000)).astype(np.int32)
    res_p = al.compute_batch([fixed], [moving], wl.x0[perm], fixed_index=perm[None, :])
    assert np.array_equal(res_p.pose, res.pose[perm])


def test_loop_closure_sweep_acceptance(ctx, po):
    """Row f3: a sweep of candidate (scan, initial guess) pairs against one submap, as MultiLoopDetectorBruteForce2D does with
    relocalize_aligner (30 iterations, Cauchy 0.05, point_distance 1.414: MULTI.json:572-630,771-784), then the acceptance
    test of MULTI.json:979-985.  Good guesses must be accepted, hopeless ones rejected; decisions equal the oracle's."""
    wl = synth.make_workload(12, 60000, seed=12)
    x0 = wl.x0.copy()
    x0[8:] += np.float32([3.0, -2.0, 0.7])                      # candidates 8..11: wrong place
    proj = api.PointNormal2fProjectorPolar(721, -math.pi, math.pi, 0.3, 20.0)
    al = api.MultiAligner2D(ctx, max_iterations=30, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(
        api.CorrespondenceFinderProjective2f(ctx, proj, point_distance=1.414, normal_cos=0.8), robustifier=api.RobustifierCauchy(0.05),
        min_num_correspondences=10))
    res = al.compute_batch([api.CloudSet(ctx, wl.scan_points, wl.scan_offsets)], [api.CloudSet(ctx, wl.map_points)], x0, want_stats=True)
    acc = res.loop_closure_accept(300, 0.1, 0.8)
    osp = po.slice_params(canvas_cols=721, range_max=20.0, point_distance=1.414, robustifier=po.ROBUST_CAUCHY, chi_threshold=0.05)
    xo, _, status, last = po.align_batch(po.aligner_params(30), osp, wl.scan_points, wl.scan_offsets, wl.map_points, x0)
    want = np.array([status[i] == 0 and last[i].n_in >= 300 and last[i].chi_in / max(last[i].n_in, 1) <= 0.1 and
                     last[i].n_in / max(last[i].n_corr, 1) >= 0.8 for i in range(12)])
    assert np.array_equal(acc, want)
    assert acc[:8].all() and not acc[8:].any()


def test_configs3_full_size_loop_closure_sweep(ctx, po):
    """BASELINE configs[3] at its size on one GPU: 65 536 candidate (scan, initial guess) pairs -- 2 048 distinct scans chosen
    through the index array, as MultiLoopDetectorBruteForce2D's candidate loop would (MULTI.json:964-986) -- against one 100k-point
    submap, Cauchy tau 0.05 (MULTI.json:957-962).  Size-independent properties over the whole sweep (generating pose,
    equivariance under a permutation of the candidates, run-to-run bits, acceptance decisions) and 16 sampled candidates against
    the oracle: within the north_star tolerance of the reference-order mirror, bit-identical to the device-order mirror."""
    n_cand, n_unique, iters = 65536, 2048, 20
    world = synth.make_world(3)
    wl = synth.make_workload(n_unique, 100000, seed=3, world=world)
    scan_index = (np.arange(n_cand) % n_unique).astype(np.int32)
    st = synth.Stream(4242, salt=9)
    delta = st.uniform(3 * n_cand, -0.05, 0.05).reshape(n_cand, 3)
    x_true = wl.x_true[scan_index]
    x0 = synth.invert_poses(synth.compose_poses(synth.invert_poses(wl.x_true)[scan_index], delta)).astype(np.float32)
    proj = api.PointNormal2fProjectorPolar(1081, -math.pi, math.pi, 0.3, 30.0)
    al = api.MultiAligner2D(ctx, max_iterations=iters, min_num_inliers=10)
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(
        api.CorrespondenceFinderProjective2f(ctx, proj, point_distance=0.5, normal_cos=0.8), robustifier=api.RobustifierCauchy(0.05),
        min_num_correspondences=10))
    scans = api.CloudSet(ctx, wl.scan_points, wl.scan_offsets); submap = api.CloudSet(ctx, wl.map_points)
    res = al.compute_batch([scans], [submap], x0, fixed_index=scan_index[None, :], want_stats=True)
    assert ctx.get_option("last_align_path") == 1                      # the throughput kernel
    # (1) noise-free data: every candidate converges to the pose its scan was rendered from
    err = np.abs(res.pose - x_true); err[:, 2] = np.abs((err[:, 2] + np.pi) % (2 * np.pi) - np.pi)
    assert (res.status == 0).all() and err[:, :2].max() < 1e-4 and err[:, 2].max() < 1e-4, (err[:, :2].max(), err[:, 2].max())
    assert (res.iterations == iters).all()
    # (2) the acceptance test of the sweep's consumer (MULTI.json:979-985): all of these are true closures
    assert res.loop_closure_accept(500, 0.1, 0.8).all()
    # (3) run-to-run: the same bits
    res2 = al.compute_batch([scans], [submap], x0, fixed_index=scan_index[None, :])
    assert np.array_equal(res.pose, res2.pose) and np.array_equal(res.information, res2.information)
    # (4) a permutation of the candidates permutes the results, bit for bit (an alignment does not depend on its neighbours)
    perm = np.random.default_rng(5).permutation(n_cand)
    resp = al.compute_batch([scans], [submap], x0[perm], fixed_index=scan_index[perm][None, :])
    assert np.array_equal(resp.pose, res.pose[perm]) and np.array_equal(resp.information, res.information[perm])
    # (5) 16 sampled candidates against the oracle
    osp = po.slice_params(robustifier=po.ROBUST_CAUCHY, chi_threshold=0.05)
    for i in np.random.default_rng(6).choice(n_cand, 16, replace=False):
        sc = wl.scan_points[wl.scan_offsets[scan_index[i]]:wl.scan_offsets[scan_index[i] + 1]]
        ref = po.align(po.aligner_params(iters), [osp], [sc], [wl.map_points], x0[i])
        d = np.abs(res.pose[i] - ref["pose"])
        assert ref["status"] == 0 and d[:2].max() < 1e-4 and d[2] < 1e-4, (i, d)
        dev = po.align(po.aligner_params(iters, device_order=True), [osp], [sc], [wl.map_points], x0[i])
        assert np.array_equal(res.pose[i], dev["pose"]) and np.array_equal(res.information[i], dev["H"]), i


def test_bench_strong_scaling_leg_runs_over_rccl_on_one_gpu(tmp_path):
    """bench.py's N > 1 leg for configs[3] (shard the candidates, RCCL broadcast of the submap, all_gather of the poses, the
    cross-rank bit check) executed on hardware with a world of one rank: LSM2D_BENCH_FORCE_DIST=1 initialises the nccl (= RCCL)
    process group and takes every collective the 8-GPU run takes."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LSM2D_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", RANK="0", LOCAL_RANK="0", WORLD_SIZE="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--total-candidates", "65536", "--unique-scans", "2048",
                        "--cauchy", "0.05", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["parity_ok"] and d["ranks_seen"] == 1 and d["scaling"] == "strong" and d["config"]["alignments_per_gpu"] == 65536
    assert d["cross_rank_check"].startswith("1 of 1 ranks"), d["cross_rank_check"]
    assert d["value"] > 10000 and d["max_pose_err_m"] < 1e-4


def test_bench_four_ranks_share_the_gpu_weak_and_strong(tmp_path):
    """bench.py launched as the round-end driver launches it for N > 1 (torch.distributed.run, one process per rank) with FOUR ranks
    on THIS one GPU (the pool allows six processes on a card: this test process, the launcher and four ranks -- five ranks were killed by its process guard;
    round 4 rehearsed three): RCCL refuses two
    ranks on a device, so the transport is gloo (LSM2D_BENCH_BACKEND) -- everything else is the N-GPU
    run: per-rank scans, the submap broadcast from rank 0, sharding, barrier-bracketed timing with the maximum over ranks, the cross-rank
    bit check, every rank pinned to its own cores and keeping its own note file.  Weak scaling (the default line) and the strong-scaling sweep
    of configs[3] at a reduced size."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LSM2D_BENCH_BACKEND="gloo", LSM2D_BENCH_RANK_DIR=str(tmp_path))
    env.pop("WORLD_SIZE", None); env.pop("RANK", None); env.pop("LOCAL_RANK", None)
    NR = 4
    for extra, scaling, per_rank in ((["--scans", "300"], "weak", 300), (["--total-candidates", "3001", "--unique-scans", "256", "--cauchy", "0.05"], "strong", None)):
        # weak: through the launcher, as the driver does; strong: the PLAIN command -- bench.py finds no WORLD_SIZE and starts its three ranks itself
        # (round 3's plain `--gpus N` silently ran one rank and printed n_gpus: 1)
        launcher = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(NR), "--master-addr", "127.0.0.1", "--master-port", "29541"] if per_rank else [sys.executable]
        r = subprocess.run(launcher + [os.path.join(root, "bench.py"), "--gpus", str(NR), "--steps", "3", "--warmup", "1", "--spinup-s", "0.05", "--no-cpu-baseline"] + extra,
                           env=env, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]                      # rank 0 prints, the others stay silent
        d = json.loads(lines[0])
        assert d["n_gpus"] == NR and d["ranks_seen"] == NR and d["scaling"] == scaling and d["parity_ok"], d
        assert d["cross_rank_check"].startswith("%d of %d ranks" % (NR, NR)), d["cross_rank_check"]
        assert len(d["ms_per_step_per_rank"]) == NR and max(d["ms_per_step_per_rank"]) <= d["ms_per_step"] * 1.001      # the line's time is the slowest rank's
        # every rank's own note file reached "done" with a parity verdict; the affinity masks are disjoint (when the box has the cores) and cover what rank 0 may use
        notes = [json.load(open(tmp_path / ("bench_rank%d.json" % k))) for k in range(NR)]
        assert all(nt["stage"] == "done" and nt["parity_ok"] and nt["world"] == NR for nt in notes)
        cores = [c for nt in notes for c in nt["cpu_affinity"]]
        assert len(set(cores)) == len(cores) or len(notes[0]["cpu_affinity"]) < NR
        assert ("strong_scaling_gather" in d) == (scaling == "strong")                                                   # ... and the sweep's gather is inside it
        if per_rank:
            assert d["config"]["alignments_per_gpu"] == per_rank and abs(d["value"] * d["ms_per_step"] * 1e-3 - NR * per_rank) < 1e-6 * NR * per_rank
        else:
            assert abs(d["value"] * d["ms_per_step"] * 1e-3 - 3001) < 1e-2       # the whole sweep per step, whatever the shard sizes
            sh = d["sharding"]                                                    # sharded by estimated work: balanced to within a candidate's worth, never worse than by count
            assert sh["by"] == "work" and sum(sh["candidates_per_rank"]) == 3001 and sh["work_max_over_mean"] <= min(1.01, sh["work_max_over_mean_if_sharded_by_count"] + 1e-9)
            assert d["ms_per_step_rank_max"] == max(d["ms_per_step_per_rank"])
        assert d["max_pose_err_m"] < 1e-4


def test_gpu_reproduces_the_frozen_golden_bits(ctx):
    """tests/golden/oracle_regression.json holds the fp32 mirror's poses and per-iteration statistics in the kernels' summation order,
    frozen as hex floats (generated on the CPU by tests/golden/make_oracle_regression.py).  The device must give exactly those bits --
    no oracle call in this test: committed data against the HIP path."""
    g = json.load(open(golden_path("oracle_regression.json")))
    wl = synth.make_workload(3, 8000, seed=42, n_beams=361)
    finders = {"projective": lambda: api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(361, -math.pi, math.pi, 0.3, 30.0)),
               "nn": lambda: api.CorrespondenceFinderKDTree2D(ctx, max_distance_m=0.3, normal_cos=0.8),
               "distmap": lambda: api.CorrespondenceFinderNN2D(ctx, max_distance_m=0.5, resolution=0.1, normal_cos=0.8)}
    fixed = api.CloudSet(ctx, wl.scan_points, wl.scan_offsets); moving = api.CloudSet(ctx, wl.map_points)
    for name, mk in finders.items():
        al = api.MultiAligner2D(ctx, max_iterations=10, min_num_inliers=10)
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(mk(), min_num_correspondences=10))
        res = al.compute_batch([fixed], [moving], wl.x0, want_stats=True)
        for c in g["cases"]:
            i = c["index"]; w = c[name + "_fp32"]["device_order"]
            assert int(res.status[i]) == w["status"], (name, i)
            assert [float(v).hex() for v in res.pose[i]] == w["pose_hex"], (name, i, res.pose[i].tolist())
            k = len(w["n_corr"])
            assert res.stats[i]["n_correspondences"][:k].tolist() == w["n_corr"]
            assert [float(v).hex() for v in res.stats[i]["chi_inliers"][:k]] == w["chi_in_hex"]


def test_gpu_reproduces_the_frozen_tracker_chain(ctx):
    """tests/golden/tracker_chain.json (digests written by the oracle on the CPU box): the HIP path, fed the same raw ranges, must
    produce the same preprocessed scans, clipped scenes, poses, information matrices and local maps at every step -- committed data
    against the device, no oracle call; once with kernel timing (every call launches at once) and once without (deferred launches,
    both scans preprocessed by one launch)."""
    import tracker_chain
    g = json.load(open(golden_path("tracker_chain.json")))
    assert tracker_chain.run_device(api, ctx, len(g["steps"])) == g["steps"]
    quiet = api.Context(0, kernel_timing=False)
    try:
        assert tracker_chain.run_device(api, quiet, len(g["steps"])) == g["steps"]
    finally:
        quiet.close()


# ---- BASELINE configs[2] and configs[4] at their stated sizes ---------------------------------------------------------------------------
def test_configs2_full_replay_1000_steps_against_committed_digests(ctx):
    """BASELINE configs[2] at its size (usage contract apps/visual_test_tracker_2d.cpp:167-183): 1 000 tracker steps with the
    MULTI parameters -- 721-column projectors, 10 iterations, two WithSensor laser slices (Cauchy 0.01 / none) plus the odometry prior,
    raw ranges in, preprocess, clip, align, merge, everything chained on the DEVICE's own state (asynchronous clip / merge: one
    synchronisation per step, for the pose).  tests/golden/tracker_replay_1000.json holds the oracle's digests of every 50th step (scans,
    clipped scene, pose bits, information matrix, local map), written on the CPU box by tests/golden/make_tracker_chain.py and re-checked
    against the oracle by tests/test_oracle.py: a single flipped bit anywhere in the 1 000 steps changes every later digest."""
    import time
    import tracker_chain
    g = json.load(open(golden_path("tracker_replay_1000.json")))
    assert g["steps_total"] == 1000 and g["record_every"] == 50 and len(g["steps"]) == 20
    quiet = api.Context(0, kernel_timing=False)
    try:
        t0 = time.perf_counter()
        got = tracker_chain.run_device(api, quiet, 1000, record_every=50, map_capacity=60000)
        dt = time.perf_counter() - t0
    finally:
        quiet.close()
    assert [r["step"] for r in got] == [r["step"] for r in g["steps"]]
    for a, b in zip(got, g["steps"]):
        assert a == b, (a["step"], {k: (a[k], b[k]) for k in b if a[k] != b[k]})
    assert all(r["status"] == 0 for r in got) and got[-1]["map_points"] > 4000
    print("configs[2] replay: 1000 steps in %.2f s (Python driver, ranges in -> pose out, %.3f ms per step incl. the digests' downloads)" % (dt, dt))


def test_configs4_full_size_properties_1000_scans_vs_1m_map(ctx, po):
    """BASELINE configs[4] at its size: 1 000 scans x 1M-point map x 20 iterations -- too slow for the scalar oracle as a unit test beyond a
    few alignments, so: convergence to the generating pose on noise-free data (1e-4 m / 1e-4 rad), run-to-run bitwise determinism,
    permutation equivariance through the index array, the culled and the un-culled stream bit for bit, and three sampled alignments
    bitwise against the device-order oracle."""
    wl = synth.make_workload(1000, 1000000, seed=4)
    al = _aligner(ctx)
    fixed = api.CloudSet(ctx, wl.scan_points, wl.scan_offsets); moving = api.CloudSet(ctx, wl.map_points)
    res = al.compute_batch([fixed], [moving], wl.x0)
    assert np.all(res.status == 0)
    d = np.abs(res.pose - wl.x_true)
    assert d[:, :2].max() < POSE_TOL_M and d[:, 2].max() < POSE_TOL_RAD
    again = al.compute_batch([fixed], [moving], wl.x0)
    assert np.array_equal(again.pose, res.pose) and np.array_equal(again.information, res.information)
    perm = np.argsort(synth.Stream(11).uniform(1000)).astype(np.int32)
    res_p = al.compute_batch([fixed], [moving], wl.x0[perm], fixed_index=perm[None, :])
    assert np.array_equal(res_p.pose, res.pose[perm]) and np.array_equal(res_p.information, res.information[perm])
    ctx.set_option("cull", 0)
    try:
        plain = al.compute_batch([fixed], [moving], wl.x0)
    finally:
        ctx.set_option("cull", 1)
    assert np.array_equal(plain.pose, res.pose) and np.array_equal(plain.information, res.information) and np.array_equal(plain.iterations, res.iterations)
    for i in (0, 499, 999):
        sc = wl.scan_points[wl.scan_offsets[i]:wl.scan_offsets[i + 1]]
        rt = po.align(po.aligner_params(20, device_order=True), [po.slice_params()], [sc], [wl.map_points], wl.x0[i])
        assert np.array_equal(res.pose[i], rt["pose"]) and np.array_equal(res.information[i], rt["H"]), i
