"""Finishing a found cycle from the ring (align_body, csrc/lsm2d_k_align.h; option "fast_forward" 2, the default): once the pose after an iteration equals,
bit for bit, the pose one of the last sixteen iterations started at, nothing more runs -- pose, information matrix, inlier count and last start pose are
those of the last iteration's twin one lap back.  Nothing a caller can see may change.  On the 512 alignments of tests/ff_finish_cases.py (periods 1 .. 7,
10 and 13; the rule itself and the classes: tests/test_ff_finish_cpu.py), tiled to the batch sizes that reach every launch form of the body, "fast_forward"
2, 1 and 0 give the same pose, information matrix, status, iteration count and statistics rows (digest included) at max_iterations 12, 13, 20, 21, 22 and
23 -- for the alignment that finds period 10 after 12 iterations that is 0, 1, 8, p - 1, p and p + 1 iterations left; the tiles agree with each other; and
the 512 distinct alignments equal the oracle -- the device-order one in the tree order, the sequential one with "sum_order" 1.  All comparisons are bitwise.
(That iterations ARE left out is not visible here by construction: tools/units_probe.py --iterations shows it on the diagnostics build.)"""
import math
import time

import numpy as np
import pytest

import ff_finish_cases as fc
from gpu_helpers import _oracle_slice, assert_same_bits, result_bits
from srrg2_laser_slam_2d_amd import api, synth

pytestmark = pytest.mark.gpu

# (alignments, sum_order, forced options, last_align_width of the form)
FORMS = {"k_align": (512, 0, dict(align_path=1), 512), "k_align_two": (1040, 0, dict(align_width=1024), 1024), "k_align_narrow": (1100, 0, dict(align_width=256), 256),
         "k_align_seq": (512, 1, dict(align_path=1), 512), "k_align_seq_two": (1040, 1, dict(align_width=1024), 1024)}
_DEVICE = {}


def _sets(ctx):
    if "sets" not in _DEVICE:
        m, wl = fc.workload()
        _DEVICE["sets"] = (api.CloudSet(ctx, wl.scan_points, wl.scan_offsets), api.CloudSet(ctx, m))
    return _DEVICE["sets"]


def _aligner(ctx, its, cauchy=None, **kw):
    al = api.MultiAligner2D(ctx, max_iterations=its, min_num_inliers=10, **kw)
    finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(fc.COLS, -math.pi, math.pi, 0.3, 30.0))
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, robustifier=None if cauchy is None else api.RobustifierCauchy(cauchy), min_num_correspondences=10))
    return al


def _run(ctx, al, n, fast_forward, sum_order=0, priors=None, **opts):
    fixed, moving = _sets(ctx)
    _, wl = fc.workload()
    idx = np.arange(n) % fc.N
    opts = dict(opts, fast_forward=fast_forward, sum_order=sum_order)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        r = al.compute_batch([fixed], [moving], wl.x0[idx], priors=None if priors is None else [priors[i] for i in idx], fixed_index=idx.astype(np.int32)[None, :], want_stats=True)
        assert ctx.get_option("fast_forward") == fast_forward
        return r, ctx.get_option("last_align_path"), ctx.get_option("last_align_width")
    finally:
        for k in opts:
            ctx.set_option(k, 2 if k == "fast_forward" else 0)      # (the library's defaults)


def _three_ways(ctx, al, n, tag, want, sum_order=0, width=512, priors=None, **opts):
    """"fast_forward" 2, 1 and 0 on the same batch: equal to each other, every tile equal to the first, the first 512 equal to the oracle's arrays `want`"""
    res = {}
    for ff in (2, 1, 0):
        r, path, w = _run(ctx, al, n, ff, sum_order, priors=priors, **opts)
        assert path == 1 and w == width, (tag, ff, path, w)
        res[ff] = result_bits(r)
    assert_same_bits(res[2], res[0], (tag, "fast_forward 2 against 0"))
    assert_same_bits(res[1], res[0], (tag, "fast_forward 1 against 0"))
    assert_same_bits(res[2], res[2], (tag, "tiles differ"), rows=np.arange(n) % fc.N)
    assert_same_bits({k: v[:fc.N] for k, v in res[2].items()}, want, (tag, "fast_forward 2 against the oracle"))
    return res[2]


@pytest.mark.parametrize("its", fc.ITS_GPU)
@pytest.mark.parametrize("form", list(FORMS))
def test_launch_forms(ctx, po, form, its):
    t0 = time.time()
    n, sum_order, opts, width = FORMS[form]
    want = fc.oracle_arrays(po, its, device_order=not sum_order)
    t1 = time.time()
    got = _three_ways(ctx, _aligner(ctx, its), n, (form, its), want, sum_order, width, **opts)
    assert np.all(got["iterations"] == its), sorted(set(got["iterations"].tolist()))      # (left-out iterations count: nobody ends by itself on this workload)
    print("finish from the ring, %s, n %d, max_iterations %d: fast_forward 2 = 1 = 0 = oracle, bit for bit; oracle %.1f s, device %.1f s" % (form, n, its, t1 - t0, time.time() - t1))


def _variant(ctx, po, key, al, ap_kw=None, priors=None, its=20):
    """512 alignments on k_align with another aligner: the three values agree and equal the device-order oracle of the same aligner"""
    m, wl = fc.workload()
    osl = [_oracle_slice(po, s.slice_params()) for s in al.param_slice_processors]

    def one(i):
        kw = dict(ap_kw or {})
        if priors is not None:
            kw.update(prior_z=priors[i][0], prior_omega=priors[i][1])
        return po.align(po.aligner_params(its, device_order=True, **kw), osl, [fc.scan(wl, i)], [m], wl.x0[i])
    want = fc.oracle_arrays(po, its, True, key=key, one=one)
    return _three_ways(ctx, al, fc.N, key, want, priors=priors, align_path=1)


def test_full_prior_matrix_and_damping(ctx, po):
    _, wl = fc.workload()
    rng = np.random.default_rng(5)
    priors = []
    for i in range(fc.N):      # means a little off the start pose, full information matrices
        L = np.tril(rng.uniform(-3.0, 3.0, (3, 3)), -1) + np.diag(rng.uniform(3.0, 8.0, 3))
        z = synth.compose_poses(wl.x0[i:i + 1].astype(np.float64), np.array([[0.02, -0.01, 0.01]]))[0].astype(np.float32)
        priors.append((z, (L @ L.T).astype(np.float32)))
    got = _variant(ctx, po, "prior+damping", _aligner(ctx, 20, damping=1.0), ap_kw=dict(damping=1.0), priors=priors)
    plain = fc.oracle_arrays(po, 20, True)
    assert np.any(got["pose"] != plain["pose"]) and np.any(got["information"] != plain["information"])      # (the inputs are seen)


def test_cauchy(ctx, po):
    got = _variant(ctx, po, "cauchy", _aligner(ctx, 20, cauchy=0.05))
    assert np.any(got["pose"] != fc.oracle_arrays(po, 20, True)["pose"])
