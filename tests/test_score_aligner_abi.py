"""CPU checks of the aligner-scoring calls: lsm2d_score_aligner_batch / lsm2d_score_aligner_select are declared by include/lsm2d.h, bound by the Python
mirror and exported by the gfx950 build, their kernels are in the code object, both mirrors have their entries; and the yardstick of the GPU tests --
score_aligner_cases.combine, a scored item restated in numpy float32 from per-slice rows -- equals the sequential oracle's align(max_iterations=1) bit for
bit on the inputs the GPU tests use: H, the first statistics row, the digest, the NotEnoughCorrespondences status, and through po.solve_update the pose.
No tolerance appears in this file."""
import ctypes as C

import numpy as np
import pytest

import abi_checks
import score_aligner_cases as cases

NAMES = {"lsm2d_score_aligner_batch": 6, "lsm2d_score_aligner_select": 11}


def test_symbols_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi
    bound = {name: abi_checks.assert_declared_bound_exported(name, n_args) for name, n_args in NAMES.items()}
    assert all(b[1] is C.c_int for b in bound.values())
    assert bound["lsm2d_score_aligner_batch"][2][1] == C.POINTER(_capi.Batch)
    assert bound["lsm2d_score_aligner_select"][2][1] == C.POINTER(_capi.Batch) and bound["lsm2d_score_aligner_select"][2][2] == C.POINTER(_capi.SelectParamsC)


def test_struct_layout():
    """the descriptor the calls take is lsm2d_batch as the aligner takes it; a prior is 12 floats; a statistics row 28 bytes"""
    from srrg2_laser_slam_2d_amd import _capi, api
    assert [f[0] for f in _capi.Batch._fields_] == ["n_alignments", "n_slices", "slices", "fixed", "moving", "fixed_index", "moving_index", "init_pose", "prior"]
    assert _capi.Batch.prior.offset == 8 + 6 * C.sizeof(C.c_void_p) and C.sizeof(_capi.Batch) == 8 + 7 * C.sizeof(C.c_void_p)
    assert C.sizeof(_capi.Prior) == 48 and C.sizeof(_capi.IterationStats) == 28 == api.STATS_DTYPE.itemsize
    assert C.sizeof(_capi.SelectParamsC) == 12


def test_kernels_are_in_the_code_object():
    abi_checks.assert_kernels_in_code_object((b"k_score_aligner_items", b"k_score_combine", b"k_select_tile_one", b"k_select_keys", b"k_select_gather", b"k_score_partial_batch"))


def test_mirrors_have_the_entries():
    abi_checks.assert_mirrors_have(("score_aligner", "score_aligner_select"), ("scoreAligner(", "scoreAlignerSelect(", "lsm2d_score_aligner_batch(", "lsm2d_score_aligner_select("))


def test_score_rank_active_rejects_items_without_a_contributing_slice():
    from srrg2_laser_slam_2d_amd import api
    st = np.zeros(4, api.STATS_DTYPE)
    st["n_inliers"] = [5, 9, 9, 7]; st["n_correspondences"] = [9, 9, 9, 9]; st["chi_inliers"] = [0.1, 0.2, 0.1, 0.3]
    every = api.SelectParams(0, float("inf"), 0.0)
    assert api.score_rank(st, every, 8)[0].tolist() == [2, 1, 3, 0]
    idx, n_acc = api.score_rank(st, every, 8, active=np.array([1, 2, 0, 1], np.int32))
    assert idx.tolist() == [1, 3, 0] and n_acc == 3
    assert api.score_rank(st, every, 8, active=np.ones(4, np.int32))[0].tolist() == [2, 1, 3, 0]


# ---- the yardstick itself: the numpy combination against the sequential oracle's first iteration ---------------------------------------------------------------
@pytest.fixture(scope="module")
def inputs():
    return cases.make_inputs()


def _item(po, c, i, ns, min_corr, prior):
    """the numpy restatement of item i over the first ns slices ("sum_order" 1 rows) and what po.align(max_iterations=1) says"""
    sl = cases.oracle_slices(po, min_corr)[:ns]
    X = c.poses[i]
    rows = []
    for s in range(ns):
        Xe = cases.effective_pose(po, cases.S_OFF[s], X)
        rows.append(cases.oracle_row(po, sl[s], s, c.fixed[s][i], c.moving[s], Xe, 1))
    mc = [sp.min_num_correspondences for sp in sl]
    got = cases.combine(po, rows, mc, X, prior)
    ap = po.aligner_params(1, prior_z=None if prior is None else prior[0], prior_omega=None if prior is None else prior[1])
    want = po.align(ap, sl, [c.fixed[s][i] for s in range(ns)], [c.moving[s] for s in range(ns)], X)
    return got, want, rows


def _assert_item_is_the_oracles(po, got, want, X, tag):
    st = want["stats"][0]
    print(tag, "pairs", got["n_corr"], "inliers", got["n_in"], "active", got["active"], "status", want["status"])
    assert want["iterations"] == 1
    assert (got["n_corr"], got["n_in"], got["n_out"]) == (st.n_corr, st.n_in, st.n_out), tag
    assert cases.u32(got["chi_in"]) == cases.u32(st.chi_in) and cases.u32(got["chi_out"]) == cases.u32(st.chi_out), tag
    assert got["digest"] == st.pair_digest, tag
    if got["active"] == 0:
        assert want["status"] == po.NOT_ENOUGH_CORRESPONDENCES and not got["H"].any() and not got["b"].any() and not want["H"].any(), tag
        return
    assert np.array_equal(cases.u32(got["H"]), cases.u32(want["H"])), (tag, got["H"], want["H"])
    rc, pose, _ = po.solve_update(got["H"], got["b"], X, 0.0)
    assert want["status"] in (po.SUCCESS, po.NOT_ENOUGH_INLIERS)
    assert np.array_equal(cases.u32(pose), cases.u32(want["pose"])), (tag, pose, want["pose"])


@pytest.mark.parametrize("ns", [1, 2, 3, 4])
def test_combination_is_the_sequential_oracles_first_iteration(po, inputs, ns):
    for i in range(inputs.n):
        got, want, rows = _item(po, inputs, i, ns, None, None)
        # (the three slices of the issue give 300 .. 630 pairs each; the fourth, of this file's choosing, more than two workgroups' 512)
        assert got["active"] == ns and want["status"] == 0 and all(300 <= r[2] <= 630 for r in rows[:3]) and all(r[2] > 512 for r in rows[3:]), [r[2] for r in rows]
        _assert_item_is_the_oracles(po, got, want, inputs.poses[i], ("slices", ns, "scan", i))


def test_combination_with_the_prior(po, inputs):
    for i in range(inputs.n):
        prior = cases.asym_prior(inputs.poses[i], seed=i)
        assert prior[1][0, 2] != prior[1][2, 0]
        got, want, _ = _item(po, inputs, i, 3, None, prior)
        plain, _, _ = _item(po, inputs, i, 3, None, None)
        assert not np.array_equal(got["H"], plain["H"]) and not np.array_equal(got["H"], got["H"].T)      # the prior is in, asymmetric as given
        _assert_item_is_the_oracles(po, got, want, inputs.poses[i], ("prior", i))


def test_combination_skip_rule(po, inputs):
    i = 1
    _, _, rows = _item(po, inputs, i, 3, None, None)
    counts = [r[2] for r in rows]
    prior = cases.asym_prior(inputs.poses[i])
    # a threshold equal to a slice's own pair count skips it -- its pairs stay in n_correspondences and the digest; one less keeps it
    for s in range(3):
        mc = [cases.MIN_CORR] * 4; mc[s] = counts[s]
        got, want, _ = _item(po, inputs, i, 3, mc, prior)
        assert got["active"] == 2 and got["n_corr"] == sum(counts)
        _assert_item_is_the_oracles(po, got, want, inputs.poses[i], ("skipped", s))
        mc[s] = counts[s] - 1
        got, want, _ = _item(po, inputs, i, 3, mc, prior)
        assert got["active"] == 3
        _assert_item_is_the_oracles(po, got, want, inputs.poses[i], ("kept", s))
    # all slices skipped: zeros, no prior, counts and digest reported
    got, want, _ = _item(po, inputs, i, 3, counts + [0], prior)
    assert got["active"] == 0 and got["n_corr"] == sum(counts) and got["digest"] != 0
    _assert_item_is_the_oracles(po, got, want, inputs.poses[i], ("all skipped",))
