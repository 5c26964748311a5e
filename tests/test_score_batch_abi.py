"""CPU checks of the fused finder + factor call's ABI: lsm2d_score_batch is declared by include/lsm2d.h, bound by the Python mirror with its eleven arguments
and exported by the gfx950 build; the three k_score_* kernels are in the library's code object; the Python and the C++ mirror have their entries."""
import abi_checks


def test_score_batch_symbol_declared_bound_and_exported():
    abi_checks.assert_declared_bound_exported("lsm2d_score_batch", 11)


def test_score_batch_kernels_are_in_the_code_object():
    abi_checks.assert_kernels_in_code_object((b"k_score_partial_batch", b"k_score_final_batch", b"k_score_seq_batch"))


def test_mirrors_have_score_batch():
    abi_checks.assert_mirrors_have("score_batch", ("scoreBatch(", "lsm2d_score_batch("))


def test_score_accept_applies_the_loop_detectors_three_tests():
    from srrg2_laser_slam_2d_amd import api
    from srrg2_laser_slam_2d_amd._capi import IterationStats

    def st(n_in, n_out, chi_in):
        s = IterationStats(); s.n_inliers, s.n_outliers, s.n_correspondences, s.chi_inliers = n_in, n_out, n_in + n_out, chi_in
        return s

    stats = [st(600, 100, 30.0), st(499, 0, 1.0), st(600, 100, 61.0), st(600, 151, 30.0), st(0, 0, 0.0)]
    assert api.score_accept(stats).tolist() == [True, False, False, False, False]      # too few inliers, chi per inlier, inlier ratio, nothing found
    assert api.score_accept(stats, 400, 0.2, 0.75).tolist() == [True, True, True, True, False]
