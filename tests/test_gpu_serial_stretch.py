"""The stretch between an iteration's sums and its closing barrier (align_body, csrc/lsm2d_k_align.h) runs as a vector over wave 0: the solve without early
exits (solve_flat: a failed pivot is a flag tested at the end), the ring compared by sixteen lanes at once, rows and poses stored by several lanes.  Nothing a
caller can see may change, on any launch form of the body (FORMS, as in tests/test_gpu_ff_finish.py) and with "fast_forward" 2 and 0:
  1. the failure verdicts of the flag-based solve in the first and in a later iteration -- a straight wall gives a singular H (nothing constrains y), a little
     damping makes it regular -- against the oracle (device order for "sum_order" 0, sequential for "sum_order" 1);
  2. want_stats=False, the path bench.py times, gives what want_stats=True gives (no statistics rows, no digest: other stores, other lanes);
  3. alignments that fail next to alignments that succeed in one launch: every eighth start pose of tests/ff_finish_cases.py moved 500 m away.
All comparisons are bitwise."""
import math

import numpy as np
import pytest

import ff_finish_cases as fc
from gpu_helpers import assert_same_bits, result_bits
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu

# (alignments, sum_order, forced options, last_align_width of the form)
FORMS = {"k_align": (512, 0, dict(align_path=1), 512), "k_align_two": (1040, 0, dict(align_width=1024), 1024), "k_align_narrow": (1100, 0, dict(align_width=256), 256),
         "k_align_seq": (512, 1, dict(align_path=1), 512), "k_align_seq_two": (1040, 1, dict(align_width=1024), 1024)}
SUCCESS, NOT_ENOUGH_CORRESPONDENCES, SINGULAR_H = 0, 1, 3
_CACHE = {}


def _aligner(ctx, its, **kw):
    al = api.MultiAligner2D(ctx, max_iterations=its, min_num_inliers=10, **kw)
    finder = api.CorrespondenceFinderProjective2f(ctx, api.PointNormal2fProjectorPolar(fc.COLS, -math.pi, math.pi, 0.3, 30.0))
    al.param_slice_processors.append(api.AlignerSliceProcessorLaser2D(finder, min_num_correspondences=10))
    return al


def _run(ctx, al, fixed, moving, x0, fast_forward, sum_order, width, want_stats=True, fixed_index=None, **opts):
    opts = dict(opts, fast_forward=fast_forward, sum_order=sum_order)
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        r = al.compute_batch([fixed], [moving], x0, fixed_index=fixed_index, want_stats=want_stats)
        assert ctx.get_option("fast_forward") == fast_forward
        assert (ctx.get_option("last_align_path"), ctx.get_option("last_align_width")) == (1, width), (ctx.get_option("last_align_path"), ctx.get_option("last_align_width"))
        return r
    finally:
        for k in opts:
            ctx.set_option(k, 2 if k == "fast_forward" else 0)      # (the library's defaults)


# ---- 1. the verdicts of the flag-based solve ----------------------------------------------------------------------------------------------------------------
WALL_ITS = 20
WALL_X0 = np.array([(0.0, 0.0, 0.0), (0.01, 0.02, 0.003), (0.02, -0.03, -0.004), (-0.01, 0.05, 0.002)], np.float32)
WALL_VERDICTS = [(SINGULAR_H, 1), (SINGULAR_H, 2), (NOT_ENOUGH_CORRESPONDENCES, 2), (SINGULAR_H, 1)]      # the device-order oracle's (status, iterations), undamped


def _wall(n):
    y = np.linspace(-1.0, 1.0, n)
    return np.stack([np.full(n, 2.0), y, np.full(n, -1.0), np.zeros(n)], 1).astype(np.float32)


def _wall_oracle(po, device_order, damping):
    k = ("wall", bool(device_order), float(damping))
    if k not in _CACHE:
        runs = [po.align(po.aligner_params(WALL_ITS, device_order=device_order, damping=damping), [po.slice_params(canvas_cols=fc.COLS)], [_wall(300)], [_wall(10000)], x)
                for x in WALL_X0]
        _CACHE[k] = (runs, fc.as_arrays(runs, WALL_ITS))
    return _CACHE[k]


def _wall_sets(ctx):
    if "wall_sets" not in _CACHE:
        _CACHE["wall_sets"] = (api.CloudSet(ctx, _wall(300)), api.CloudSet(ctx, _wall(10000)))
    return _CACHE["wall_sets"]


@pytest.mark.parametrize("damping", [0.0, 1.0])
@pytest.mark.parametrize("form", list(FORMS))
def test_failure_verdicts(ctx, po, form, damping):
    n, sum_order, opts, width = FORMS[form]
    runs, _ = _wall_oracle(po, True, damping)      # the inputs keep meaning what they are for
    got_verdicts = [(r["status"], r["iterations"]) for r in runs]
    assert got_verdicts == (WALL_VERDICTS if damping == 0.0 else [(SUCCESS, WALL_ITS)] * 4), got_verdicts
    _, want = _wall_oracle(po, not sum_order, damping)
    fixed, moving = _wall_sets(ctx)
    rows = np.arange(n) % len(WALL_X0)
    for ff in (2, 0):
        r = _run(ctx, _aligner(ctx, WALL_ITS, damping=damping), fixed, moving, WALL_X0[rows], ff, sum_order, width, **opts)
        assert_same_bits(result_bits(r), want, (form, damping, ff, "against the oracle"), rows=rows)


# ---- 2. and 3. on the 512 alignments of ff_finish_cases -----------------------------------------------------------------------------------------------------
def _ff_sets(ctx):
    if "ff_sets" not in _CACHE:
        m, wl = fc.workload()
        _CACHE["ff_sets"] = (api.CloudSet(ctx, wl.scan_points, wl.scan_offsets), api.CloudSet(ctx, m))
    return _CACHE["ff_sets"]


@pytest.mark.parametrize("its", [20, 23])
@pytest.mark.parametrize("form", list(FORMS))
def test_stats_off_equals_stats_on(ctx, form, its):
    n, sum_order, opts, width = FORMS[form]
    fixed, moving = _ff_sets(ctx)
    _, wl = fc.workload()
    idx = np.arange(n) % fc.N
    res = {}
    for want_stats in (True, False):
        r = _run(ctx, _aligner(ctx, its), fixed, moving, wl.x0[idx], 2, sum_order, width, want_stats=want_stats, fixed_index=idx.astype(np.int32)[None, :], **opts)
        res[want_stats] = result_bits(r, stats=False)
    assert np.all(res[True]["iterations"] == its)
    assert_same_bits(res[False], res[True], (form, its, "want_stats=False against want_stats=True"))


MOVED_ITS = 20


def _moved_oracle(po, device_order):
    """every eighth alignment's start pose 500 m off in x: its oracle result; the others are ff_finish_cases' cached arrays"""
    k = ("moved", bool(device_order))
    if k not in _CACHE:
        m, wl = fc.workload()
        plain = fc.oracle_arrays(po, MOVED_ITS, device_order)
        moved = np.arange(0, fc.N, 8)
        runs = [po.align(po.aligner_params(MOVED_ITS, device_order=device_order), [po.slice_params(canvas_cols=fc.COLS)], [fc.scan(wl, i)], [m],
                         wl.x0[i] + np.array([500.0, 0.0, 0.0], np.float32)) for i in moved]
        far = fc.as_arrays(runs, MOVED_ITS)
        want = {key: v.copy() for key, v in plain.items()}
        for key in want:
            want[key][moved] = far[key]
        _CACHE[k] = (runs, want)
    return _CACHE[k]


@pytest.mark.parametrize("form", list(FORMS))
def test_failures_next_to_successes(ctx, po, form):
    n, sum_order, opts, width = FORMS[form]
    runs, want = _moved_oracle(po, not sum_order)
    assert all((r["status"], r["iterations"]) == (NOT_ENOUGH_CORRESPONDENCES, 1) for r in runs)
    fixed, moving = _ff_sets(ctx)
    _, wl = fc.workload()
    idx = np.arange(n) % fc.N
    x0 = wl.x0[idx].copy()
    x0[idx % 8 == 0, 0] += np.float32(500.0)
    res = {}
    for ff in (2, 0):
        r = _run(ctx, _aligner(ctx, MOVED_ITS), fixed, moving, x0, ff, sum_order, width, fixed_index=idx.astype(np.int32)[None, :], **opts)
        res[ff] = result_bits(r)
        assert_same_bits(res[ff], want, (form, ff, "against the oracle"), rows=idx)
    assert_same_bits(res[2], res[0], (form, "fast_forward 2 against 0"))
