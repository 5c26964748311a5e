"""The fast-forward of align_body (csrc/lsm2d_k_align.h; option "fast_forward") on the CPU: the device-order oracle's pose sequences on the workload of
tests/fast_forward_cases.py hold every class the GPU tests rely on, and the skip rule, restated in numpy and applied to those sequences, lands on the pose
the oracle reaches by running all twenty iterations -- for every one of the 96 alignments."""
import collections
import time

import numpy as np

import fast_forward_cases as ffc

ITS = 20


def test_recipe_holds_every_class_and_the_skip_rule_reproduces_the_full_run(po):
    t0 = time.time()
    seqs = ffc.pose_sequences(po, ITS, device_order=True)
    reps = [ffc.first_repeat(s) for s in seqs]
    periods = collections.Counter(r[1] for r in reps if r is not None)
    found_at = sorted(set(r[0] - 1 for r in reps if r is not None))      # the iteration whose solve produced the repeated pose
    print("first-repeat periods %s among %d alignments (%d without a repeat in %d iterations), found at iterations %s; %.1f s"
          % (dict(sorted(periods.items())), len(seqs), sum(r is None for r in reps), ITS, found_at, time.time() - t0))
    assert periods[1] >= 1 and periods[2] >= 1 and sum(n for p, n in periods.items() if p >= 3) >= 1, periods
    # max_iterations = 3: somebody has not repeated a pose yet (the GPU test's shortest run must hold alignments that skip nothing)
    assert any(ffc.first_repeat(s[:4]) is None for s in seqs)
    full = ffc.oracle_runs(po, ITS, device_order=True)
    for i, s in enumerate(seqs):
        assert len(s) == ITS + 1, (i, len(s))      # nobody stops by itself on this workload: the sequences are whole
        got = ffc.fast_forward_pose(s, ITS)
        assert np.array_equal(got.view(np.uint32), np.array(full[i]["pose"], np.float32).view(np.uint32)), (i, reps[i], got.tolist(), full[i]["pose"].tolist())
    # ... and at the other iteration counts the GPU tests run (a remainder of the period is left over at some of them)
    for its in (3, 7):
        run = ffc.oracle_runs(po, its, device_order=True)
        for i, s in enumerate(seqs):
            assert np.array_equal(ffc.fast_forward_pose(s, its).view(np.uint32), np.array(run[i]["pose"], np.float32).view(np.uint32)), (its, i, reps[i])
