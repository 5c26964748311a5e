"""CPU checks of lsm2d_align_select's ABI and of its restatement api.align_rank: the two symbols are declared by include/lsm2d.h, bound by the Python mirror
and exported by the gfx950 build; the pack kernel and the selection's kernels for the aligned row are in the library's code object; the C++ mirror has its
entries and compiles; align_rank equals a plain Python loop over the oracle's results; and the workload the GPU tests select from exercises every term of the
verdict (the oracle's results, no GPU) -- so that the GPU tests cannot pass vacuously.

One condition of the issue cannot hold as it is worded.  "With the middle thresholds of the Success candidates' last rows ... at least one non-Success
candidate passes the thresholds alone": a candidate ends NotEnoughInliers exactly when its last row has fewer inliers than min_num_inliers, every Success
candidate has at least that many, and a NotEnoughCorrespondences candidate has none -- a min_inliers threshold that is a Success candidate's own count rejects
every one of them.  The condition is therefore checked (and the GPU tests run) with a SECOND set of thresholds as well, align_select_cases.status_thresholds,
taken from the rows of all candidates: under those the status term alone rejects dozens of candidates."""
import numpy as np
import pytest

import abi_checks
import align_select_cases as cases
import cpp_build

NAMES = {"lsm2d_align_select": 13, "lsm2d_sweep_align_select": 16}


def test_align_select_symbols_declared_bound_and_exported():
    for name, n_args in NAMES.items():
        abi_checks.assert_declared_bound_exported(name, n_args)
    assert "0.7.7" in abi_checks.header()


def test_align_select_kernels_are_in_the_code_object():
    abi_checks.assert_kernels_in_code_object((b"k_align_rows", b"k_select_keysINS_8AlignRow", b"k_select_gatherINS_8AlignRow", b"k_select_tile_oneINS_8AlignRow"))


def test_mirrors_have_align_select():
    from srrg2_laser_slam_2d_amd import api
    abi_checks.assert_mirrors_have(("align_select", "align_rank", "last_stats_rows"), ("alignSelect(", "computeSelect(", "lsm2d_align_select(", "lsm2d_sweep_align_select("))
    fields = [f.name for f in __import__("dataclasses").fields(api.AlignSelectResult)]
    assert fields[:7] == ["index", "pose", "information", "iterations", "last_stats", "n_accepted", "n_success"]


@pytest.mark.parametrize("source", ["align_select_driver.cpp", "align_select_bench.cpp"])
def test_cpp_sources_compile(source):
    r = cpp_build.syntax_only(source)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- api.align_rank on hand-made results ---------------------------------------------------------------------------------------------------------------------
def test_align_rank_status_iterations_and_last_row():
    from srrg2_laser_slam_2d_amd import api
    st = np.zeros((6, 3), api.STATS_DTYPE)
    row = lambda n_in, n_out, chi: (n_in + n_out, n_in, n_out, chi, 0.0, 0, 0)
    st[0, 0] = row(9, 0, 1.0); st[0, 1] = row(5, 0, 1.0)            # the LAST started row counts (5 inliers), not the best one
    st[1, 0] = row(7, 0, 2.0)                                       # one iteration
    st[2, 2] = row(9, 0, 0.5)                                       # best of all, but NotEnoughInliers
    st[3, 0] = row(9, 0, 0.1)                                       # Success without an iteration: its row 0 must not be read
    st[4, 0] = row(7, 0, 2.0)                                       # ties with 1: by index
    st[5, 1] = row(7, 1, 1.5)
    status = np.int32([0, 0, 2, 0, 0, 0]); its = np.int32([2, 1, 3, 0, 1, 2])
    everything = api.SelectParams(0, float("inf"), 0.0)
    idx, n_acc, n_suc = api.align_rank(status, its, st, everything, 8)
    assert idx.dtype == np.int32 and idx.tolist() == [5, 1, 4, 0] and (n_acc, n_suc) == (4, 5)
    assert api.align_rank(status, its, st, everything, 2)[0].tolist() == [5, 1]
    assert api.align_rank(status, its, st, api.SelectParams(6, float("inf"), 0.0), 8)[:2][1] == 3
    last = api.last_stats_rows(its, st)      # the one-dimensional form: the last rows themselves
    assert last["n_inliers"].tolist() == [5, 7, 9, 0, 7, 7] and api.align_rank(status, its, last, everything, 8)[0].tolist() == [5, 1, 4, 0]
    empty = api.align_rank(status[:0], its[:0], st[:0], everything, 3)
    assert len(empty[0]) == 0 and empty[1:] == (0, 0)
    with pytest.raises(ValueError):
        api.align_rank(status, its, st, everything, 0)


# ---- the GPU tests' workload, on the CPU ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_order", [0, 1], ids=["reference", "tree"])
@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_workload_exercises_every_term(po, kind, device_order):
    from srrg2_laser_slam_2d_amd import api
    c = cases.make_cases()
    M = cases.middle_min_inliers(po, c, kind, po.ROBUST_CAUCHY, device_order)
    r = cases.oracle_results(po, c, kind, po.ROBUST_CAUCHY, device_order, M)
    last = r.last(); ok = r.status == 0
    assert all(np.any(r.status == s) for s in (0, 1, 2)), np.bincount(r.status)      # Success, NotEnoughCorrespondences, NotEnoughInliers
    assert np.all(r.iterations >= 1) and r.iterations[1] == 1 and r.status[1] == 1
    # the middle thresholds of the Success candidates' last rows
    mid = cases.middle_thresholds(last[ok])
    passes = np.all(cases.conditions(last, mid), axis=0)
    idx, n_acc, n_suc = api.align_rank(r.status, r.iterations, r.stats, mid, 1024)
    assert n_suc == int(ok.sum()) and 0 < n_acc < n_suc and n_acc == int((ok & passes).sum())
    assert np.any(ok & ~passes)                                            # a Success candidate the thresholds reject
    n_in = last["n_inliers"][idx]
    assert len(np.unique(n_in)) < len(n_in)                                # two accepted candidates share n_inliers: chi^2 decides
    for a, b in cases.DUPLICATES:                                          # the duplicates are accepted, side by side in the ranking: the index decides
        assert np.array_equal(c.poses[a], c.poses[b]) and last[a].tobytes() == last[b].tobytes()
        pa, pb = idx.tolist().index(a), idx.tolist().index(b)
        assert pa < pb and set(idx[pa:pb + 1].tolist()) <= {x for pair in cases.DUPLICATES for x in pair}
    # ... and the thresholds under which the status term decides (see the module's docstring)
    low = cases.status_thresholds(last[r.iterations >= 1])
    passes_low = np.all(cases.conditions(last, low), axis=0)
    assert np.any(~ok & passes_low) and np.any(ok & ~passes_low)           # non-Success candidates that pass the thresholds alone
    idx_low, n_acc_low, _ = api.align_rank(r.status, r.iterations, r.stats, low, 1024)
    assert 0 < n_acc_low == int((ok & passes_low).sum()) < int(passes_low.sum()) and not np.any(~ok[idx_low])
    # the restatement against a plain loop, for both sets and a k that cuts
    for sel in (mid, low, api.SelectParams(0, float("inf"), 0.0)):
        for k in (1024, 7):
            want = cases.plain_loop_rank(r.status, r.iterations, r.stats, sel, k)
            got = api.align_rank(r.status, r.iterations, r.stats, sel, k)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (sel, k)
