"""Mixed batches for the launch-form tests, as DATA: a deterministic generator of loop-closure-like batches in which alignments that converge, alignments
that need more iterations, light ones and ones that fail or stop early sit side by side -- what a packed workgroup (two alignments, one after the other) and
the placement that pairs the lightest alignments meet in a real candidate sweep.  tests/test_gpu_launch_forms.py runs them in every launch form;
tests/test_mixed_batches_cpu.py holds the generator to the statuses it claims, on the CPU alone.

Alignment i of a setting is the same whatever the batch size: everything is drawn for NMAX alignments and a batch of n takes the first n, so a smaller
batch is a prefix of a larger one.  Nothing here touches the GPU; the api classes are used only as parameter holders."""
from __future__ import annotations

import math

import numpy as np

from fuzz_cases import oracle_slice
from srrg2_laser_slam_2d_amd import api, synth

NMAX = 4096

# the kinds, and the statuses each one may end with under every setting and both oracles (None: no claim -- the test checks what it needs itself)
#   converge     full scan, start near the truth
#   slow         full scan, a larger start error: more iterations (under S2 it stops later than `converge`)
#   light        a narrow field of view, 60-200 points: converges, or -- one wall in view -- stops with SingularH
#   far          a hopeless start (+80 m): NotEnoughCorrespondences at iteration 1
#   empty        a zero-length fixed cloud: NotEnoughCorrespondences at iteration 1
#   few_inliers  a handful of points: correspondences enough, inliers never reach min_num_inliers
#   drift        a short, narrow scan from a poor start: its pairs thin out or line up -- it fails at iteration 1, 2 or 3 (any status), or converges
#   nan, inf     a start pose that is not a number: a failure status; the oracle has no defined answer to compare with
# (SingularH needs no kind of its own: light and drift alignments that see one wall end with it, in every setting.)
KINDS = ("converge", "slow", "light", "far", "empty", "few_inliers", "drift", "nan", "inf")
CLAIMED_STATUS = dict(converge=(0,), slow=(0,), light=(0, 3), far=(1,), empty=(1,), few_inliers=(2,), drift=None, nan=None, inf=None)
NON_FINITE = ("nan", "inf")
# one block of 40 alignments holds every kind this often; each block is shuffled on its own, so the kinds are spread through the batch, never in runs
_BLOCK = dict(converge=18, slow=6, light=5, far=2, empty=2, few_inliers=3, drift=2, nan=1, inf=1)
SETTINGS = ("S1", "S2", "S3")
N_POSES = 24


def _world():
    world = synth.make_world(5)
    return world, synth.make_map(world, 20000, noise_sigma=0.003, seed=8), synth.sample_poses(world, N_POSES, seed=29)


def _kinds(rng):
    block = np.array([k for k in KINDS for _ in range(_BLOCK[k])])
    return np.concatenate([block[rng.permutation(len(block))] for _ in range((NMAX + len(block) - 1) // len(block))])[:NMAX]


def _slice_clouds(world, robots, S, beams, fov, few, seed):
    """the fixed clouds of one slice, from the sensor at robot o S: N_POSES full scans, N_POSES light ones, N_POSES with a few points, N_POSES short ones for
    `drift`, and one empty cloud (the last).  Returns (points, offsets, {kind: first cloud index})."""
    sensors = synth.compose_poses(robots, np.tile(np.asarray(S, np.float64)[None, :], (len(robots), 1)))
    parts, counts, first = [], [], {}
    def add(kind, pts, offs):
        first[kind] = len(counts)
        for c in range(len(offs) - 1):
            parts.append(pts[offs[c]:offs[c + 1]]); counts.append(offs[c + 1] - offs[c])
    add("full", *synth.make_scans(world, sensors, n_beams=beams, fov_deg=fov, noise_sigma=0.003, seed=seed))
    add("light", *synth.make_scans(world, sensors, n_beams=180, fov_deg=120.0, noise_sigma=0.003, seed=seed + 1))
    add("few", *synth.make_scans(world, sensors, n_beams=few, fov_deg=270.0, noise_sigma=0.003, seed=seed + 2))
    add("short", *synth.make_scans(world, sensors, n_beams=40, fov_deg=40.0, noise_sigma=0.003, seed=seed + 3))
    first["empty"] = len(counts); parts.append(np.zeros((0, 4), np.float32)); counts.append(0)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(parts, 0), np.float32), offs, first


def batch(seed: int, n: int, setting: str, damping: float = 0.0, full_omega: bool = False):
    """The first n alignments of a setting's mixed batch.  Returns a dict: kinds [n] (str), x0 float32 [n, 3], priors (list of (z, omega) or None),
    fixed_index int32 [ns, n], map (the one moving cloud, float32 [20000, 4]), slices (per slice: cols, cauchy, tau, S, min_corr, pts, offs), aligner
    parameters (max_iterations, min_num_inliers, termination_chi_epsilon, inlier_only, keep_only_inlier, damping).
    damping: the Gauss-Newton damping aligner() and oracle_align() pass on.  full_omega (settings with priors): every prior's information matrix is a full
    symmetric positive definite L L^T instead of a diagonal, and its mean is turned by a further rotation, so that the prior's own rotation is not the
    identity at the start.  Neither touches a draw of the batch itself: what full_omega needs comes from a generator of its own."""
    assert setting in SETTINGS and 0 < n <= NMAX, (setting, n)
    assert not full_omega or setting in ("S2", "S3"), setting
    rng = np.random.default_rng([seed, SETTINGS.index(setting)])
    world, m, robots = _world()
    kinds = _kinds(rng)
    robot = rng.integers(0, N_POSES, NMAX)
    # start errors (robot frame), per kind
    scale = np.where(kinds == "slow", 0.12, np.where(kinds == "drift", 0.12, 0.02))
    delta = rng.uniform(-1.0, 1.0, (NMAX, 3)) * scale[:, None]
    delta[:, 2] *= np.where(kinds == "slow", 0.6, 1.0)
    x0 = synth.invert_poses(synth.compose_poses(robots[robot], delta)).astype(np.float32)
    x0[kinds == "far"] += np.float32([80.0, 80.0, 0.0])
    comp = rng.integers(0, 3, NMAX)
    for i in np.flatnonzero(kinds == "nan"):
        x0[i, comp[i]] = np.nan
    for i in np.flatnonzero(kinds == "inf"):
        x0[i, comp[i]] = np.inf if comp[i] != 1 else -np.inf
    if setting == "S3":
        slice_defs = [dict(cols=721, cauchy=True, tau=0.02, S=(0.0, 0.0, 0.0), beams=721, fov=270.0),
                      dict(cols=541, cauchy=False, tau=0.0, S=(0.12, -0.08, 0.4), beams=541, fov=240.0)]
    else:
        slice_defs = [dict(cols=1081, cauchy=True, tau=0.02, S=(0.0, 0.0, 0.0), beams=1081, fov=270.0)]
    slices, fixed_index = [], []
    for s, d in enumerate(slice_defs):
        pts, offs, first = _slice_clouds(world, robots, d["S"], d["beams"], d["fov"], 19 if len(slice_defs) > 1 else 32, seed=31 + 10 * s)
        cloud = np.select([kinds == "light", kinds == "few_inliers", kinds == "drift", kinds == "empty"],
                          [first["light"] + robot, first["few"] + robot, first["short"] + robot, np.full(NMAX, first["empty"])], first["full"] + robot)
        fixed_index.append(cloud.astype(np.int32))
        slices.append(dict(cols=d["cols"], cauchy=d["cauchy"], tau=d["tau"], S=np.float32(d["S"]), min_corr=10, pts=pts, offs=offs))
    params = dict(max_iterations=8, min_num_inliers=40, termination_chi_epsilon=0.0, inlier_only=False, keep_only_inlier=False)
    priors = None
    if setting in ("S2", "S3"):
        # a prior near the truth on some alignments, a zero information matrix on the others (the batch carries priors for all or for none)
        z = synth.invert_poses(synth.compose_poses(robots[robot], rng.uniform(-0.01, 0.01, (NMAX, 3)))).astype(np.float32)
        w = (rng.uniform(5.0, 60.0, (NMAX, 3)) * (rng.random(NMAX) < 0.5)[:, None]).astype(np.float32)
        priors = [(z[i], np.diag(w[i])) for i in range(n)]
        if full_omega:
            rng_f = np.random.default_rng([seed, SETTINGS.index(setting), 1])
            diag = rng_f.uniform(3.0, 8.0, (NMAX, 3)); low = rng_f.uniform(-3.0, 3.0, (NMAX, 3)); turn = rng_f.uniform(-0.4, 0.4, NMAX)
            z[:, 2] = ((z[:, 2].astype(np.float64) + turn + math.pi) % (2.0 * math.pi) - math.pi).astype(np.float32)
            priors = []
            for i in range(n):
                L = np.array([[diag[i, 0], 0.0, 0.0], [low[i, 0], diag[i, 1], 0.0], [low[i, 1], low[i, 2], diag[i, 2]]])
                priors.append((z[i], (L @ L.T).astype(np.float32)))
    if setting == "S2":
        params.update(termination_chi_epsilon=1e-3, inlier_only=True, keep_only_inlier=True)
    params["damping"] = float(damping)
    return dict(setting=setting, seed=seed, n=n, ns=len(slices), kinds=kinds[:n], x0=x0[:n].copy(), priors=priors,
                fixed_index=np.ascontiguousarray(np.stack(fixed_index)[:, :n]), map=m, slices=slices, **params)


def aligner(ctx, spec):
    """the api aligner of a batch (ctx may be None: parameters only)"""
    al = api.MultiAligner2D(ctx, max_iterations=spec["max_iterations"], min_num_inliers=spec["min_num_inliers"], damping=spec["damping"],
                            termination_chi_epsilon=spec["termination_chi_epsilon"])
    al.param_enable_inlier_only_runs = spec["inlier_only"]
    al.param_keep_only_inlier_correspondences = spec["keep_only_inlier"]
    for sl in spec["slices"]:
        f = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(sl["cols"], -math.pi, math.pi, 0.3, 30.0))
        rob = api.RobustifierCauchy(sl["tau"]) if sl["cauchy"] else None
        if sl["S"].any():
            al.param_slice_processors.append(api.AlignerSliceProcessorLaser2DWithSensor(f, sensor_in_robot=sl["S"], robustifier=rob, min_num_correspondences=sl["min_corr"]))
        else:
            al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(f, robustifier=rob, min_num_correspondences=sl["min_corr"]))
    return al


def oracle_align(po, spec, i, device_order=False, want_pairs=False, double=False):
    """po.align of alignment i: the device-order fp32 oracle (device_order=True, the tree order) or the sequential one (the reference's order); double: the
    fp64 oracle"""
    kw = dict(prior_z=spec["priors"][i][0], prior_omega=spec["priors"][i][1]) if spec["priors"] is not None else {}
    ap = po.aligner_params(spec["max_iterations"], min_num_inliers=spec["min_num_inliers"], damping=spec["damping"], device_order=device_order,
                           termination_chi_epsilon=spec["termination_chi_epsilon"], enable_inlier_only_runs=spec["inlier_only"],
                           keep_only_inlier_correspondences=spec["keep_only_inlier"], **kw)
    osl = [oracle_slice(po, p.slice_params()) for p in aligner(None, spec).param_slice_processors]      # the values the api hands the library
    fixed = []
    for s, sl in enumerate(spec["slices"]):
        c = int(spec["fixed_index"][s, i])
        fixed.append(sl["pts"][sl["offs"][c]:sl["offs"][c + 1]])
    return po.align(ap, osl, fixed, [spec["map"]] * spec["ns"], spec["x0"][i], want_pairs=want_pairs, double=double)


# ---- what tests/test_damping_and_prior_cpu.py measures on the oracle and tests/test_gpu_damping_and_prior.py asserts on the device -------------------------
DAMPING_SEED, DAMPING_N, DAMPING = 2024, 120, 50.0
MIN_DIFFERENT = 95      # of the 114 finite alignments among the first 120 (the device-order oracle with diagonal priors: S1 98, S3 99 differ from damping 0)


def wall_cloud():
    """test_oracle.py::test_aligner_status_logic's wall: 400 points on y = 2, normals (0, -1) -- nothing observes the translation along it"""
    return np.stack([np.linspace(-3, 3, 400), np.full(400, 2.0), np.zeros(400), -np.ones(400)], 1).astype(np.float32)


# (start, damping, status, iterations), 8 iterations, min_num_correspondences 0: identity start -- b is zero, so every successful step is zero and the pose stays exactly zero
WALL_ROWS = [((0.0, 0.0, 0.0), 0.0, 3, 1)]
WALL_ROWS += [((0.0, 0.0, 0.0), lam, 0, 8) for lam in (1e-6, 1e-3, 1.0, 100.0)]
WALL_ROWS += [((0.0, 0.0, 0.0), lam, 3, 1) for lam in (-1.0, float("nan"), float("inf"))]
WALL_OFFSET_START = (0.01, 0.02, 0.003)      # with damping 1 the direction nothing observes is held, the other two converge: Success after 8 iterations
WALL_OFFSET_TOL = 1e-6                       # the oracle ends within 3.5e-8 of (0.01, 0, 0) in both orders


def prior_variants(spec):
    """the latency-kernel cases: no prior, the batch's (full) matrices, each made asymmetric ([0,1] += 4, [2,0] -= 3), and those transposed"""
    asym = []
    for z, om in spec["priors"]:
        a = om.copy(); a[0, 1] += 4.0; a[2, 0] -= 3.0
        asym.append((z, a))
    return dict(none=None, full=spec["priors"], asymmetric=asym, transposed=[(z, a.T.copy()) for z, a in asym])


def with_slices(spec, ns, **changes):
    """the batch with its first ns slices only (and whatever else is to change)"""
    return dict(spec, ns=ns, slices=spec["slices"][:ns], fixed_index=np.ascontiguousarray(spec["fixed_index"][:ns]), **changes)
