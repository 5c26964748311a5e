"""The finish rule of align_body (csrc/lsm2d_k_align.h; option "fast_forward" 2) on the CPU.  When the pose after an iteration equals the start pose of
one of the last sixteen iterations, the kernel runs nothing more: it takes pose, information matrix, inlier count and status from the twin of the last
iteration, one lap back.  Here the rule is restated in numpy (tests/ff_finish_cases.py: finish) on the device-order oracle's runs at max_iterations 1 .. 23
of the 512 alignments, and what it picks must equal, bit for bit, what the oracle leaves when it runs all the iterations -- at every iteration count the
GPU tests use.  The workload must hold the cases the GPU tests rely on, or all of this passes on nothing."""
import collections
import time

import numpy as np

import ff_finish_cases as fc

ITS_MAX = max(fc.ITS_GPU)


def _runs_by_alignment(po):
    _, wl = fc.workload()
    per_its = [None] + [fc.oracle_runs(po, k, device_order=True) for k in range(1, ITS_MAX + 1)]
    return [[dict(pose=wl.x0[i])] + [per_its[k][i] for k in range(1, ITS_MAX + 1)] for i in range(fc.N)]


def test_finish_rule_reproduces_the_full_run_and_the_workload_holds_the_cases(po):
    t0 = time.time()
    runs = _runs_by_alignment(po)
    reps = [fc.first_repeat(r, 20) for r in runs]
    periods = collections.Counter(r[1] for r in reps if r is not None)
    print("first repeats within 20 iterations: periods %s among %d alignments, %d without; oracle runs %.1f s" % (dict(sorted(periods.items())), fc.N, sum(r is None for r in reps), time.time() - t0))
    # the workload: short periods, periods only the ring of sixteen sees (found with iterations left to finish), and one found with exactly one left
    assert all(periods[p] >= 1 for p in range(1, 8)), periods
    long_ones = [(i, r) for i, r in enumerate(reps) if r is not None and 9 <= r[1] <= 16 and r[0] <= 19]
    assert len(long_ones) >= 2, long_ones
    assert any(r[0] == 19 for _, r in long_ones), long_ones
    # one alignment whose remainders R over the GPU tests' iteration counts are 0, 1, p - 1, p and p + 1
    assert any(r is not None and {0, 1, r[1] - 1, r[1], r[1] + 1} <= {its - r[0] for its in fc.ITS_GPU} for r in reps), [r for r in reps if r is not None and r[1] >= 9]
    for its in fc.ITS_GPU:
        full = fc.oracle_runs(po, its, device_order=True)
        finished = 0
        for i in range(fc.N):
            (pose, H, status, n_in), how = fc.finish(runs[i], its)
            f = full[i]
            want_n_in = f["stats"][f["iterations"] - 1].n_in if f["iterations"] > 0 else 0
            assert np.array_equal(pose, np.asarray(f["pose"], np.float32).view(np.uint32)), (its, i, how, "pose")
            assert np.array_equal(H, np.asarray(f["H"], np.float32).view(np.uint32).reshape(9)), (its, i, how, "H")
            assert status == f["status"] and n_in == want_n_in, (its, i, how, status, f["status"], n_in, want_n_in)
            finished += how is not None
        print("max_iterations %d: %d of %d alignments finished from the ring, all equal to the full run" % (its, finished, fc.N))
        assert finished > fc.N // 2      # (the rule is at work: most alignments repeat a pose early)
