"""CPU checks of the grouped select calls (lsm2d_score_select_grouped, lsm2d_score_aligner_select_grouped, lsm2d_align_select_grouped): the three symbols are
declared by include/lsm2d.h, bound by the Python mirror and exported by the gfx950 build; the grouped kernels for the three row formats are in the library's
code object; the Python and C++ mirrors have their entries and the C++ sources compile; the restatements api.score_rank_grouped / api.align_rank_grouped
equal a hand loop on hand-made rows; and the group tables the GPU tests use contain every kind of group on the oracle's rows (no GPU), so that the GPU tests
cannot pass vacuously.  Every comparison is on integers."""
import numpy as np
import pytest

import abi_checks
import align_select_cases as acases
import cpp_build
import score_select_cases as scases
import select_grouped_cases as gc

NAMES = {"lsm2d_score_select_grouped": 18, "lsm2d_score_aligner_select_grouped": 13, "lsm2d_align_select_grouped": 15}


def test_grouped_symbols_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi
    for name, n_args in NAMES.items():
        abi_checks.assert_declared_bound_exported(name, n_args)
    header = abi_checks.header()
    assert "0.7.7" in header and "0.7.8" in header
    assert "#define LSM2D_SELECT_MAX_GROUP_ROWS (1 << 18)" in header and _capi.SELECT_MAX_GROUP_ROWS == 1 << 18


def test_grouped_kernels_are_in_the_code_object():
    abi_checks.assert_kernels_in_code_object([k + row for row in (b"INS_8ScoreRow", b"INS_7CombRow", b"INS_8AlignRow")
                                              for k in (b"k_select_group_one", b"k_select_keys_seg", b"k_select_gather_group")] + [b"k_select_tile_seg"])


def test_mirrors_have_the_grouped_calls():
    from srrg2_laser_slam_2d_amd import api
    abi_checks.assert_mirrors_have(("score_select_grouped", "score_aligner_select_grouped", "align_select_grouped", "score_rank_grouped", "align_rank_grouped"),
                                   ('#include "lsm2d.hpp"', "scoreSelectGrouped(", "scoreAlignerSelectGrouped(", "alignSelectGrouped(") + tuple(n + "(" for n in NAMES),
                                   "lsm2d_grouped.hpp")
    fields = [f.name for f in __import__("dataclasses").fields(api.AlignSelectGroupedResult)]
    assert fields[:7] == ["index", "pose", "information", "iterations", "last_stats", "n_accepted", "n_success"]
    assert "_select_grouped" not in abi_checks.assert_mirrors_have((), ())      # the first header's set of C calls stays what its stand-in defines


@pytest.mark.parametrize("source", ["select_grouped_driver.cpp", "select_grouped_bench.cpp"])
def test_cpp_sources_compile(source):
    r = cpp_build.syntax_only(source)      # (the driver includes lsm2d_grouped.hpp; the bench is the bare C ABI)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the restatements on hand-made rows ------------------------------------------------------------------------------------------------------------------------
def _rows():
    from srrg2_laser_slam_2d_amd import api
    row = lambda n_in, n_out, chi: (n_in + n_out, n_in, n_out, chi, 0.0, 0, 0)
    st = np.zeros(12, api.STATS_DTYPE)
    st[0] = row(7, 0, 2.0)
    st[1] = row(9, 0, 1.0); st[2] = row(9, 0, 1.0)       # equal rows on both sides of the boundary between groups 2 and 3 (items 2 | 3 below)
    st[3] = row(9, 0, 1.0); st[4] = row(9, 0, 0.5)
    st[5] = row(5, 0, float("nan"))                      # a NaN row: rejected
    st[6] = row(8, 1, 1.0); st[7] = row(8, 0, 1.0); st[8] = row(3, 0, 0.1)
    st[9] = row(9, 0, 1.0); st[10] = row(9, 0, 1.0); st[11] = row(6, 0, 0.0)
    #        empty | one | 1, 2 | 3, 4, 5 | empty | 6 .. 10 | 11 | empty
    sizes = [0, 1, 2, 3, 0, 5, 1, 0]
    return st, gc.offsets(sizes), sizes


def test_score_rank_grouped_on_hand_made_rows():
    from srrg2_laser_slam_2d_amd import api
    st, off, sizes = _rows()
    everything = api.SelectParams(0, float("inf"), 0.0)
    idx, n_acc = api.score_rank_grouped(st, off, everything, 2)
    assert n_acc.dtype == np.int32 and n_acc.tolist() == [0, 1, 2, 2, 0, 5, 1, 0]
    # the tie between items 2 and 3 is never seen: each stays in its group; inside group 5 items 9 and 10 tie and come out by index; k = 2 cuts group 5 only
    assert [i.tolist() for i in idx] == [[], [0], [1, 2], [4, 3], [], [9, 10], [11], []]
    for k in (1, 2, 3, 1024):      # k larger than every group
        for sel in (everything, api.SelectParams(8, 0.2, 0.9), api.SelectParams(10 ** 9, 0.0, 2.0)):
            got = api.score_rank_grouped(st, off, sel, k); want = gc.hand_loop_score(st, off, sel, k)
            assert gc.same_lists(got[0], want[0]) and np.array_equal(got[1], want[1]), (k, sel)
    active = np.int32([1, 1, 0, 1, 0, 1, 1, 1, 1, 0, 1, 0])      # active == 0 rejects whatever the thresholds are: item 4 was group 3's winner
    got = api.score_rank_grouped(st, off, everything, 2, active=active); want = gc.hand_loop_score(st, off, everything, 2, active=active)
    assert gc.same_lists(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert [i.tolist() for i in got[0]] == [[], [0], [1], [3], [], [10, 6], [], []] and got[1].tolist() == [0, 1, 1, 1, 0, 4, 0, 0]
    one = api.score_rank_grouped(st, [0, len(st)], everything, 4)      # one group: score_rank itself
    assert np.array_equal(one[0][0], api.score_rank(st, everything, 4)[0]) and one[1].tolist() == [api.score_rank(st, everything, 4)[1]]
    with pytest.raises(ValueError):
        api.score_rank_grouped(st, off, everything, 0)


def test_align_rank_grouped_on_hand_made_rows():
    from srrg2_laser_slam_2d_amd import api
    st1, off, sizes = _rows()
    st = np.zeros((12, 2), api.STATS_DTYPE)
    its = np.int32([1, 2, 1, 1, 2, 1, 1, 0, 1, 2, 1, 1])
    for i in range(12):
        st[i, max(its[i] - 1, 0)] = st1[i]
        if its[i] == 2:
            st[i, 0] = (20, 20, 0, 0.01, 0.0, 0, 0)      # a better EARLIER row: must not be read
    status = np.int32([0, 0, 0, 2, 0, 0, 0, 0, 1, 0, 0, 0])      # item 7: Success without an iteration
    everything = api.SelectParams(0, float("inf"), 0.0)
    idx, n_acc, n_suc = api.align_rank_grouped(status, its, st, off, everything, 2)
    assert [i.tolist() for i in idx] == [[], [0], [1, 2], [4], [], [9, 10], [11], []]
    assert n_acc.tolist() == [0, 1, 2, 1, 0, 3, 1, 0] and n_suc.tolist() == [0, 1, 2, 2, 0, 4, 1, 0]
    for k in (1, 2, 1024):
        for sel in (everything, api.SelectParams(8, 0.2, 0.9)):
            got = api.align_rank_grouped(status, its, st, off, sel, k); want = gc.hand_loop_align(status, its, st, off, sel, k)
            assert gc.same_lists(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (k, sel)


# ---- the GPU tests' group tables on the oracle's rows: every kind of group is there -------------------------------------------------------------------------------
def _every_kind(n_acc, sizes, k, winners, global_winner, tag):
    kd = gc.kinds(n_acc, sizes, k)
    assert all(len(v) > 0 for v in kd.values()), (tag, kd, n_acc.tolist())
    firsts = [int(w[0]) for w in winners if len(w)]
    assert any(w != int(global_winner) for w in firsts), tag      # a group's winner that the one pool would not have named


@pytest.mark.parametrize("order", [0, 1], ids=["tree", "reference"])
@pytest.mark.parametrize("kind", scases.KINDS)
def test_score_workload_has_every_kind_of_group(po, kind, order):
    from srrg2_laser_slam_2d_amd import api
    c = scases.make_cases()
    pairs = scases.oracle_pairs(po, c, kind)
    for robust in (po.ROBUST_NONE, po.ROBUST_CAUCHY):
        _, _, st = scases.oracle_rows(po, c, kind, robust, order, pairs)
        sel = scases.middle_thresholds(st)
        off = gc.offsets(gc.SIZES_MIXED)
        idx, n_acc = api.score_rank_grouped(st, off, sel, gc.K_MIXED)
        want = gc.hand_loop_score(st, off, sel, gc.K_MIXED)
        assert gc.same_lists(idx, want[0]) and np.array_equal(n_acc, want[1])
        _every_kind(n_acc, gc.SIZES_MIXED, gc.K_MIXED, idx, api.score_rank(st, sel, 1)[0][0], (kind, robust, order))
        assert int(n_acc.sum()) == api.score_rank(st, sel, 1)[1]


@pytest.mark.parametrize("device_order", [0, 1], ids=["reference", "tree"])
@pytest.mark.parametrize("kind", ["proj", "nn"])
def test_align_workload_has_every_kind_of_group(po, kind, device_order):
    from srrg2_laser_slam_2d_amd import api
    c = acases.make_cases()
    M = acases.middle_min_inliers(po, c, kind, po.ROBUST_CAUCHY, device_order)
    r = acases.oracle_results(po, c, kind, po.ROBUST_CAUCHY, device_order, M)
    last = r.last(); ok = r.status == 0
    off = gc.offsets(gc.SIZES_MIXED)
    for sel in (acases.middle_thresholds(last[ok]), acases.status_thresholds(last[r.iterations >= 1])):
        idx, n_acc, n_suc = api.align_rank_grouped(r.status, r.iterations, r.stats, off, sel, gc.K_MIXED)
        want = gc.hand_loop_align(r.status, r.iterations, r.stats, off, sel, gc.K_MIXED)
        assert gc.same_lists(idx, want[0]) and np.array_equal(n_acc, want[1]) and np.array_equal(n_suc, want[2])
        _every_kind(n_acc, gc.SIZES_MIXED, gc.K_MIXED, idx, api.align_rank(r.status, r.iterations, r.stats, sel, 1)[0][0], (kind, device_order, sel))
        assert int(n_suc.sum()) == int(ok.sum()) and np.all(n_acc <= n_suc)
