"""CPU checks of the fused finder + factor call's ABI: lsm2d_score_batch is declared by include/lsm2d.h, bound by the Python mirror with its eleven arguments
and exported by the gfx950 build; the three k_score_* kernels are in the library's code object; the Python and the C++ mirror have their entries."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

NAME = "lsm2d_score_batch"


def test_score_batch_symbol_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi, build
    header = open(os.path.join(ROOT, "include", "lsm2d.h")).read()
    bound = {s[0]: s for s in _capi.SYMBOLS}
    lib = C.CDLL(build.build())
    assert NAME + "(" in header
    assert NAME in bound
    assert len(bound[NAME][2]) == 11
    assert hasattr(lib, NAME)
    assert "LSM2D_VERSION 160" in header      # an addition only: the number stays


def test_score_batch_kernels_are_in_the_code_object():
    from srrg2_laser_slam_2d_amd import build
    path = build.build()
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump" if os.path.exists("/opt/rocm/llvm/bin/llvm-objdump") else "objdump", "-h", path],
                         capture_output=True, text=True).stdout
    assert ".hip_fatbin" in out
    blob = open(path, "rb").read()
    for k in (b"k_score_partial_batch", b"k_score_final_batch", b"k_score_seq_batch"):
        assert k in blob, k


def test_mirrors_have_score_batch():
    from srrg2_laser_slam_2d_amd import api
    assert callable(api.score_batch)
    hpp = open(os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "host", "lsm2d.hpp")).read()
    assert "scoreBatch(" in hpp
    assert "lsm2d_score_batch(" in hpp


def test_score_accept_applies_the_loop_detectors_three_tests():
    from srrg2_laser_slam_2d_amd import api
    from srrg2_laser_slam_2d_amd._capi import IterationStats

    def st(n_in, n_out, chi_in):
        s = IterationStats(); s.n_inliers, s.n_outliers, s.n_correspondences, s.chi_inliers = n_in, n_out, n_in + n_out, chi_in
        return s

    stats = [st(600, 100, 30.0), st(499, 0, 1.0), st(600, 100, 61.0), st(600, 151, 30.0), st(0, 0, 0.0)]
    assert api.score_accept(stats).tolist() == [True, False, False, False, False]      # too few inliers, chi per inlier, inlier ratio, nothing found
    assert api.score_accept(stats, 400, 0.2, 0.75).tolist() == [True, True, True, True, False]
