"""The oracle's aligner (po.align) pinned for the two inputs of the Gauss-Newton step that tests/test_gpu_damping_and_prior.py holds the device to it for:
a non-zero damping and a prior whose information matrix is full (and not even symmetric), with a mean that is not the start pose.  CPU alone.

  * one iteration restated in numpy float64, independently of the oracle's aligner loop, against po.align(..., double=True);
  * a single wall (H singular along it): what damping does to the status, in both summation orders;
  * the mixed batches (tests/mixed_batches.py) with damping and with full prior matrices: the counts the GPU test relies on."""
import collections
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mixed_batches as mb
from gpu_helpers import POSE_TOL_M, POSE_TOL_RAD, _pose_diff
from mixed_batches import WALL_OFFSET_START, WALL_OFFSET_TOL, WALL_ROWS, wall_cloud
from srrg2_laser_slam_2d_amd import synth

# ---- one iteration, restated ---------------------------------------------------------------------------------------------------------------------
L_FULL = np.array([[6.0, 0.0, 0.0], [2.5, 5.0, 0.0], [-3.0, 1.5, 4.0]])
OMEGA_FULL = L_FULL @ L_FULL.T                                  # full, symmetric, positive definite; every entry exact in fp32
OMEGA_ASYM = OMEGA_FULL.copy(); OMEGA_ASYM[0, 1] += 4.0; OMEGA_ASYM[2, 0] -= 3.0      # taken as given, row-major: not symmetrised anywhere
PRIOR_OFFSET = (0.05, -0.03, 0.4)                                # z = x0 o PRIOR_OFFSET: the prior's rotation is 0.4 rad away from the identity at the start
RESTATEMENT_POSE_TOL = 1e-12      # absolute: fp64 round-off of a 3x3 solve (measured 1.8e-15)
RESTATEMENT_H_TOL = 1e-12         # relative to max |H| (measured 1.3e-19)


def _v2t(v):
    c, s = math.cos(v[2]), math.sin(v[2])
    return np.array([[c, -s, v[0]], [s, c, v[1]], [0.0, 0.0, 1.0]])


def _t2v(T):
    return np.array([T[0, 2], T[1, 2], math.atan2(T[1, 0], T[0, 0])])


def _one_iteration_fp64(po, sp, fixed, moving, x0, z, omega, damping):
    """pairs and the slice's H, b from the oracle's finder and factor; the prior, the damped solve and the update by hand.  Returns (pose, H: all nine
    entries as summed, without the damping)."""
    x0 = np.asarray(x0, np.float64)
    pairs = po.find(sp, fixed, moving, x0, double=True)
    assert len(pairs) > sp.min_num_correspondences
    H, b, _ = po.linearize(sp, fixed, moving, pairs, x0, double=True)
    H = H.copy(); b = b.copy()
    e = _t2v(np.linalg.inv(_v2t(z)) @ _v2t(x0))
    c, s = math.cos(e[2]), math.sin(e[2])
    J = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    H += J.T @ omega @ J
    b += J.T @ omega @ e
    A = np.triu(H) + np.triu(H, 1).T + damping * np.eye(3)      # the solve reads H's upper triangle
    dx = np.linalg.solve(A, -b)
    return _t2v(_v2t(x0) @ _v2t(dx)), H


@pytest.mark.parametrize("damping", [0.0, 25.0])
@pytest.mark.parametrize("omega_name", ["full", "asymmetric"])
def test_one_iteration_restated_in_fp64(po, omega_name, damping):
    wl = synth.make_workload(4, 5000, seed=0)
    fixed = wl.scan_points[wl.scan_offsets[0]:wl.scan_offsets[1]]
    x0 = wl.x0[0]
    z = synth.compose_poses(x0[None, :].astype(np.float64), np.array([PRIOR_OFFSET]))[0].astype(np.float32)      # (the oracle's parameters hold z and Omega in fp32)
    omega = (OMEGA_FULL if omega_name == "full" else OMEGA_ASYM).astype(np.float32)
    assert np.array_equal(omega.astype(np.float64), OMEGA_FULL if omega_name == "full" else OMEGA_ASYM)
    sp = po.slice_params()
    r = po.align(po.aligner_params(1, damping=damping, prior_z=z, prior_omega=omega), [sp], [fixed], [wl.map_points], x0, double=True)
    assert r["status"] == po.SUCCESS and r["iterations"] == 1
    pose, H = _one_iteration_fp64(po, sp, fixed, wl.map_points, x0, z.astype(np.float64), omega.astype(np.float64), damping)
    d_pose = np.abs(r["pose"] - pose); d_pose[2] = abs((d_pose[2] + math.pi) % (2 * math.pi) - math.pi)
    d_H = np.abs(r["H"] - H).max() / np.abs(H).max()
    print("restated iteration: Omega %s, damping %g: pose differs by %.2e, H by %.2e relative; H[1,0] - H[0,1] = %.3g" % (omega_name, damping, d_pose.max(), d_H, H[1, 0] - H[0, 1]))
    assert d_pose.max() <= RESTATEMENT_POSE_TOL, (d_pose, r["pose"], pose)
    assert d_H <= RESTATEMENT_H_TOL, (d_H, r["H"], H)
    # the information matrix handed back is H WITHOUT the damping ...
    H0 = po.align(po.aligner_params(1, damping=0.0, prior_z=z, prior_omega=omega), [sp], [fixed], [wl.map_points], x0, double=True)["H"]
    assert np.array_equal(r["H"], H0)
    # ... with all nine entries as computed, not mirrored: an asymmetric Omega leaves it asymmetric by J^T (Omega - Omega^T) J, here of the order of the 4 and the 3
    if omega_name == "asymmetric":
        assert abs(r["H"][0, 1] - r["H"][1, 0]) > 1.0 and abs(r["H"][0, 2] - r["H"][2, 0]) > 1.0, r["H"]
        rt = po.align(po.aligner_params(1, damping=damping, prior_z=z, prior_omega=omega.T.copy()), [sp], [fixed], [wl.map_points], x0, double=True)
        assert np.abs(rt["H"] - r["H"]).max() > 1.0 and np.abs(rt["pose"] - r["pose"]).max() > 1e-4, (rt["H"] - r["H"], rt["pose"] - r["pose"])
    # ... and the damping reaches the step
    if damping:
        r0 = po.align(po.aligner_params(1, damping=0.0, prior_z=z, prior_omega=omega), [sp], [fixed], [wl.map_points], x0, double=True)
        assert np.abs(r0["pose"] - r["pose"]).max() > 1e-6, (r0["pose"], r["pose"])


def test_fp32_information_matrix_is_not_mirrored(po):
    """the fp32 oracles, full SYMMETRIC Omega: (1,0) and (0,1) of the prior's J^T Omega J are summed in different orders and differ in the last bits -- a device
    path that mirrored one triangle from the other could not give both"""
    wl = synth.make_workload(4, 5000, seed=0)
    fixed = wl.scan_points[wl.scan_offsets[0]:wl.scan_offsets[1]]
    z = synth.compose_poses(wl.x0[:1].astype(np.float64), np.array([PRIOR_OFFSET]))[0].astype(np.float32)
    differs = 0
    for device_order in (False, True):
        r = po.align(po.aligner_params(8, damping=25.0, prior_z=z, prior_omega=OMEGA_FULL.astype(np.float32), device_order=device_order), [po.slice_params()], [fixed],
                     [wl.map_points], wl.x0[0])
        assert r["status"] == po.SUCCESS
        differs += int(not np.array_equal(r["H"], r["H"].T))
    assert differs == 2


# ---- the wall ------------------------------------------------------------------------------------------------------------------------------------
def wall_align(po, start, damping, device_order):
    w = wall_cloud()
    return po.align(po.aligner_params(8, damping=damping, device_order=device_order), [po.slice_params(min_num_correspondences=0)], [w], [w], np.float32(start))


@pytest.mark.parametrize("device_order", [False, True])
def test_wall_damping_decides_the_status(po, device_order):
    for start, lam, status, its in WALL_ROWS:
        r = wall_align(po, start, lam, device_order)
        assert (r["status"], r["iterations"]) == (status, its), (lam, r["status"], r["iterations"])
        assert r["pose"].tobytes() == np.float32(start).tobytes() or (status == 0 and np.all(r["pose"] == 0.0)), (lam, r["pose"])
        if status == 3:
            assert r["pose"].tobytes() == np.float32(start).tobytes(), (lam, r["pose"])      # the failed step is discarded: the start pose's bits
    # away from the identity, damping 1: the direction nothing observes is held, the other two converge
    r = wall_align(po, WALL_OFFSET_START, 1.0, device_order)
    assert r["status"] == po.SUCCESS and r["iterations"] == 8
    d = np.abs(r["pose"].astype(np.float64) - [WALL_OFFSET_START[0], 0.0, 0.0])
    print("wall, offset start, damping 1, device_order %d: |pose - (0.01, 0, 0)| = %s" % (device_order, d.tolist()))
    assert d.max() <= WALL_OFFSET_TOL, (r["pose"], d)


# ---- the mixed batches ---------------------------------------------------------------------------------------------------------------------------
MIXED_SEED, MIXED_N, MIXED_DAMPING, MIXED_MIN_DIFFERENT = mb.DAMPING_SEED, mb.DAMPING_N, mb.DAMPING, mb.MIN_DIFFERENT


def mixed_oracle(po, spec, device_order=True):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda i: None if spec["kinds"][i] in mb.NON_FINITE else mb.oracle_align(po, spec, i, device_order=device_order), range(spec["n"])))


def count_different(a, b):
    """alignments (finite starts) whose pose bits or status differ between two runs of the same batch; the number compared"""
    both = [(x, y) for x, y in zip(a, b) if x is not None]
    return sum(int(x["status"] != y["status"] or x["pose"].tobytes() != y["pose"].tobytes()) for x, y in both), len(both)


@pytest.mark.parametrize("device_order", [True, False], ids=["device-order", "sequential"])
@pytest.mark.parametrize("setting", ["S1", "S3"])
def test_mixed_batches_with_damping_and_full_priors(po, setting, device_order):
    """(the counts in the comments are the device-order oracle's; the sequential one, which the device is held to with "sum_order" 1, meets the same conditions)"""
    plain = mixed_oracle(po, mb.batch(MIXED_SEED, MIXED_N, setting), device_order)
    damped = mixed_oracle(po, mb.batch(MIXED_SEED, MIXED_N, setting, damping=MIXED_DAMPING), device_order)
    h0 = collections.Counter(r["status"] for r in plain if r is not None); h1 = collections.Counter(r["status"] for r in damped if r is not None)
    diff, n = count_different(plain, damped)
    print("mixed batch %s, %s oracle: statuses without damping %s, with damping %g %s; %d of %d finite alignments differ" % (setting, "device-order" if device_order else "sequential", dict(sorted(h0.items())), MIXED_DAMPING,
                                                                                                                   dict(sorted(h1.items())), diff, n))
    assert n == 114
    assert h0[3] >= 1 and h1[3] == 0, (h0, h1)      # damping lifts every singular H of this batch
    assert diff >= MIXED_MIN_DIFFERENT, diff
    if setting == "S3":
        spec_f = mb.batch(MIXED_SEED, MIXED_N, setting, damping=MIXED_DAMPING, full_omega=True)
        assert all(np.count_nonzero(om) == 9 and np.array_equal(om, om.T) and np.linalg.eigvalsh(om.astype(np.float64)).min() > 0 for _, om in spec_f["priors"])
        full = mixed_oracle(po, spec_f, device_order)
        diff_f, n_f = count_different(damped, full)
        print("mixed batch S3, damping %g: %d of %d finite alignments differ between diagonal and full prior matrices; statuses %s"
              % (MIXED_DAMPING, diff_f, n_f, dict(sorted(collections.Counter(r["status"] for r in full if r is not None).items()))))
        assert n_f == 114 and diff_f >= MIXED_MIN_DIFFERENT, diff_f


def test_mixed_batch_keywords_leave_every_draw_untouched():
    for setting in ("S1", "S3"):
        a, b = mb.batch(7, 80, setting), mb.batch(7, 80, setting, damping=3.0, full_omega=setting == "S3")
        assert a["damping"] == 0.0 and b["damping"] == 3.0
        assert a["x0"].tobytes() == b["x0"].tobytes() and np.array_equal(a["fixed_index"], b["fixed_index"]) and np.array_equal(a["kinds"], b["kinds"])
        if setting == "S3":
            c = mb.batch(7, 200, setting, full_omega=True)      # a prefix, too
            for (za, oa), (zb, ob), (zc, oc) in zip(a["priors"], b["priors"], c["priors"]):
                assert np.array_equal(za[:2], zb[:2]) and za[2] != zb[2] and abs((float(za[2]) - float(zb[2]) + math.pi) % (2 * math.pi) - math.pi) <= 0.4 + 1e-6
                assert np.array_equal(zb, zc) and np.array_equal(ob, oc)
                assert np.count_nonzero(oa - np.diag(np.diag(oa))) == 0


def test_small_contrasts_the_gpu_tests_rely_on(po):
    """what tests/test_gpu_damping_and_prior.py asserts on a handful of alignments, measured here on the oracles (seed 2024, S3, damping 50, full prior matrices):
    the split-path test's first 8 alignments, the latency-kernel test's eight (prior, damping) combinations, the fp64 test's strict class"""
    full = mb.batch(MIXED_SEED, MIXED_N, "S3", damping=MIXED_DAMPING, full_omega=True)
    diag = mb.batch(MIXED_SEED, MIXED_N, "S3", damping=MIXED_DAMPING); plain = mb.batch(MIXED_SEED, MIXED_N, "S3", damping=0.0, full_omega=True)
    for device_order in (True, False):
        # the first 8: five succeed; all five differ from their diagonal-matrix result, four from their undamped one (the fifth has converged to the same bits)
        rows = [i for i in range(8) if full["kinds"][i] not in mb.NON_FINITE]
        a, b, c = ([mb.oracle_align(po, s, i, device_order=device_order) for i in rows] for s in (full, diag, plain))
        ok = [k for k in range(len(rows)) if a[k]["status"] == 0]
        assert len(ok) == 5
        assert sum(a[k]["pose"].tobytes() != b[k]["pose"].tobytes() for k in ok) == 5 and sum(a[k]["pose"].tobytes() != c[k]["pose"].tobytes() for k in ok) == 4
        # the first `converge` alignment, one slice and two: the eight combinations end with eight different (pose, information matrix) -- after 8 iterations the
        # poses alone need not differ (a converged run forgets its damping), the information matrices of Omega and its transpose do
        i0 = int(np.flatnonzero(full["kinds"][:8] == "converge")[0])
        for ns in (1, 2):
            seen = set()
            for name, priors in mb.prior_variants(full).items():
                for lam in (0.0, MIXED_DAMPING):
                    r = mb.oracle_align(po, mb.with_slices(full, ns, priors=priors, damping=lam), i0, device_order=device_order)
                    assert r["status"] == 0, (ns, name, lam)
                    seen.add(r["pose"].tobytes() + r["H"].tobytes())
            assert len(seen) == 8, (device_order, ns, len(seen))
    # the `converge` alignments: with the device-order oracle standing in for the device (the GPU test holds the device to its bits), 49 of 54 use the sequential
    # oracle's pairs in every iteration and lie within 2.9e-5 of the fp64 oracle; the other five within 1.2e-6
    rows = [int(i) for i in np.flatnonzero(full["kinds"] == "converge")]
    with ThreadPoolExecutor(16) as ex:
        dev, seq, dbl = (list(ex.map(lambda i: mb.oracle_align(po, full, i, **kw), rows)) for kw in (dict(device_order=True), dict(), dict(double=True)))
    strict = 0
    for d, r, rd in zip(dev, seq, dbl):
        assert d["status"] == rd["status"] == 0
        dm, dr = _pose_diff(d["pose"], rd["pose"])
        assert dm <= POSE_TOL_M and dr <= POSE_TOL_RAD, (dm, dr)
        strict += int(d["iterations"] == r["iterations"] and all(x.n_corr == y.n_corr and x.pair_digest == y.pair_digest for x, y in zip(d["stats"], r["stats"])))
    assert len(rows) == 54 and strict == 49, (len(rows), strict)
