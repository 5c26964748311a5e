"""The fast-forward of align_body (csrc/lsm2d_k_align.h; option "fast_forward", default 1): once the pose after an iteration equals, bit for bit, the pose one
of the last eight iterations started at, whole periods of the cycle are skipped.  Nothing a caller can see may change: on the workload of
tests/fast_forward_cases.py (96 alignments whose pose sequences repeat with periods 1, 2, 3, 4 and 7, first at iterations 1 .. 16:
tests/test_fast_forward_cpu.py), tiled to the batch sizes that reach every launch form of the body, "fast_forward" 1 and 0 give the same pose, information
matrix, status, iteration count and statistics rows (digest included) at max_iterations 3, 7, 20 and 21; the tiles agree with each other; and the 96
distinct alignments equal the oracle -- the device-order one in the tree order, the sequential one with "sum_order" 1.  All comparisons are bitwise.
(That iterations ARE skipped is not visible here by construction: tools/units_probe.py --iterations shows it on the diagnostics build.)"""
import math
import time

import numpy as np
import pytest

import fast_forward_cases as ffc
from gpu_helpers import _assert_bitwise_equal_to_device_order_oracle, _oracle_slice, assert_same_bits, result_bits
from srrg2_laser_slam_2d_amd import api, synth

pytestmark = pytest.mark.gpu

# (alignments, sum_order, forced options, last_align_width of the form)
FORMS = {"k_align": (288, 0, dict(align_path=1), 512), "k_align_two": (1025, 0, dict(align_width=1024), 1024), "k_align_narrow": (1100, 0, dict(align_width=256), 256),
         "k_align_seq": (288, 1, dict(align_path=1), 512), "k_align_seq_two": (1025, 1, dict(align_width=1024), 1024)}
_DEVICE = {}


def _sets(ctx):
    if "sets" not in _DEVICE:
        m, wl = ffc.workload()
        _DEVICE["sets"] = (api.CloudSet(ctx, wl.scan_points, wl.scan_offsets), api.CloudSet(ctx, m))
    return _DEVICE["sets"]


def _aligner(ctx, its, cols=(ffc.COLS,), cauchy=None, **kw):
    al = api.MultiAligner2D(ctx, max_iterations=its, min_num_inliers=10, **kw)
    for c in cols:
        finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(c, -math.pi, math.pi, 0.3, 30.0))
        al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, robustifier=None if cauchy is None else api.RobustifierCauchy(cauchy), min_num_correspondences=10))
    return al


def _run(ctx, al, n, fast_forward, sum_order=0, priors=None, **opts):
    fixed, moving = _sets(ctx)
    _, wl = ffc.workload()
    ns = len(al.param_slice_processors)
    idx = np.arange(n) % ffc.N
    opts = dict(opts, fast_forward=fast_forward, sum_order=sum_order)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        r = al.compute_batch([fixed] * ns, [moving] * ns, wl.x0[idx], priors=None if priors is None else [priors[i] for i in idx],
                             fixed_index=np.tile(idx.astype(np.int32), (ns, 1)), want_stats=True)
        return r, ctx.get_option("last_align_path"), ctx.get_option("last_align_width")
    finally:
        for k in opts:
            ctx.set_option(k, 1 if k == "fast_forward" else 0)


def _assert_option_changes_nothing_and_tiles_agree(on, off, tag):
    a = result_bits(on)
    assert_same_bits(a, result_bits(off), (tag, "fast_forward 1 against 0"))
    assert_same_bits(a, a, (tag, "tiles differ"), rows=np.arange(len(on.status)) % ffc.N)


def _assert_oracle(res, want, tag):
    for i in range(ffc.N):
        _assert_bitwise_equal_to_device_order_oracle(res, i, want[i], (tag, i))


@pytest.mark.parametrize("its", [3, 7, 20, 21])
@pytest.mark.parametrize("form", list(FORMS))
def test_launch_forms(ctx, po, form, its):
    t0 = time.time()
    n, sum_order, opts, width = FORMS[form]
    al = _aligner(ctx, its)
    on, path, w = _run(ctx, al, n, 1, sum_order, **opts)
    assert path == 1 and w == width, (form, path, w)
    off, path, w = _run(ctx, al, n, 0, sum_order, **opts)
    assert path == 1 and w == width, (form, path, w)
    _assert_option_changes_nothing_and_tiles_agree(on, off, (form, its))
    _assert_oracle(on, ffc.oracle_runs(po, its, device_order=not sum_order), (form, its))
    assert np.all(on.iterations == its), sorted(set(on.iterations.tolist()))      # (skipped iterations count: nobody ends by itself on this workload)
    print("fast-forward, %s, n %d, max_iterations %d: option on = off = oracle, bit for bit; %.1f s" % (form, n, its, time.time() - t0))


def _variant(ctx, po, key, al, ap_kw=None, priors=None, its=20):
    """288 alignments on k_align: option on = off, tiles agree, the 96 equal the device-order oracle of the same aligner"""
    m, wl = ffc.workload()
    osl = [_oracle_slice(po, s.slice_params()) for s in al.param_slice_processors]

    def one(i):
        kw = dict(ap_kw or {})
        if priors is not None:
            kw.update(prior_z=priors[i][0], prior_omega=priors[i][1])
        return po.align(po.aligner_params(its, device_order=True, **kw), osl, [ffc.scan(wl, i)] * len(osl), [m] * len(osl), wl.x0[i])
    on, path, w = _run(ctx, al, 288, 1, priors=priors, align_path=1)
    assert path == 1 and w == 512, (key, path, w)
    off, _, _ = _run(ctx, al, 288, 0, priors=priors, align_path=1)
    _assert_option_changes_nothing_and_tiles_agree(on, off, key)
    want = ffc.oracle_runs(po, its, True, key=key, one=one)
    _assert_oracle(on, want, key)
    return on, want


def test_prior_and_damping(ctx, po):
    _, wl = ffc.workload()
    rng = np.random.default_rng(5)
    priors = []
    for i in range(ffc.N):      # means a little off the start pose, full information matrices
        L = np.tril(rng.uniform(-3.0, 3.0, (3, 3)), -1) + np.diag(rng.uniform(3.0, 8.0, 3))
        z = synth.compose_poses(wl.x0[i:i + 1].astype(np.float64), np.array([[0.02, -0.01, 0.01]]))[0].astype(np.float32)
        priors.append((z, (L @ L.T).astype(np.float32)))
    on, _ = _variant(ctx, po, "prior+damping", _aligner(ctx, 20, damping=1.0), ap_kw=dict(damping=1.0), priors=priors)
    plain = _run(ctx, _aligner(ctx, 20), 288, 1, align_path=1)[0]
    assert np.any(on.pose.view(np.uint32) != plain.pose.view(np.uint32))      # (the inputs are seen)


def test_cauchy(ctx, po):
    _variant(ctx, po, "cauchy", _aligner(ctx, 20, cauchy=0.05))


def test_two_slices(ctx, po):
    _variant(ctx, po, "two slices", _aligner(ctx, 20, cols=(ffc.COLS, 181)))


def test_termination_epsilon_switches_it_off(ctx, po):
    on, want = _variant(ctx, po, "chi epsilon", _aligner(ctx, 20, termination_chi_epsilon=1e-3), ap_kw=dict(termination_chi_epsilon=1e-3))
    assert np.any(on.iterations < 20)      # (the criterion ends some of them early: it is at work)


def test_inlier_only_runs_switch_it_off(ctx, po):
    al = _aligner(ctx, 20)
    al.param_enable_inlier_only_runs = True
    on, _ = _variant(ctx, po, "inlier runs", al, ap_kw=dict(enable_inlier_only_runs=True))
    assert np.any(on.iterations > 20)      # (a second phase ran)
