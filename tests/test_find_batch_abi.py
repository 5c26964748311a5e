"""CPU checks of the batched finder's ABI: lsm2d_find_correspondences_batch is declared by include/lsm2d.h, bound by the Python mirror with its eleven
arguments and exported by the gfx950 build; the two batched finder kernels are in the library's code object."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

NAME = "lsm2d_find_correspondences_batch"


def test_find_batch_symbol_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi, build
    header = open(os.path.join(ROOT, "include", "lsm2d.h")).read()
    bound = {s[0]: s for s in _capi.SYMBOLS}
    lib = C.CDLL(build.build())
    assert NAME + "(" in header
    assert NAME in bound
    assert len(bound[NAME][2]) == 11
    assert hasattr(lib, NAME)
    assert "LSM2D_VERSION 160" in header      # an addition only: the number stays


def test_find_batch_kernels_are_in_the_code_object():
    from srrg2_laser_slam_2d_amd import build
    path = build.build()
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump" if os.path.exists("/opt/rocm/llvm/bin/llvm-objdump") else "objdump", "-h", path],
                         capture_output=True, text=True).stdout
    assert ".hip_fatbin" in out
    blob = open(path, "rb").read()
    for k in (b"k_find_projective_batch", b"k_find_nn_batch"):
        assert k in blob, k


def test_finder_classes_have_compute_batch():
    from srrg2_laser_slam_2d_amd import api
    for cls in (api.CorrespondenceFinderProjective2f, api.CorrespondenceFinderKDTree2D, api.CorrespondenceFinderNN2D):
        assert callable(getattr(cls, "compute_batch"))
    hpp = open(os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "host", "lsm2d.hpp")).read()
    assert hpp.count("computeBatch(") == 2
