"""CPU checks of the batched voxelising clipper's ABI: lsm2d_clip_scene_voxelized_batch is declared by include/lsm2d.h, bound by the Python
mirror with its 10 arguments and exported by the gfx950 build; k_clip_vox_batch is in the library's code object."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

NAME = "lsm2d_clip_scene_voxelized_batch"


def test_symbol_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi, build
    header = open(os.path.join(ROOT, "include", "lsm2d.h")).read()
    assert "LSM2D_VERSION 160" in header      # an addition only: the number stays
    assert NAME + "(" in header
    assert "scene_clipper_projective_2d.cpp:36-48" in header[header.index("/* lsm2d_clip_scene_voxelized for n_trackers"):header.index(NAME + "(")]
    bound = {s[0]: s for s in _capi.SYMBOLS}
    assert NAME in bound and len(bound[NAME][2]) == 10
    assert bound[NAME][2][7] is C.c_float      # voxelize_resolution, by value
    lib = C.CDLL(build.build())
    assert hasattr(lib, NAME)


def test_kernel_is_in_the_code_object():
    from srrg2_laser_slam_2d_amd import build
    path = build.build()
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump" if os.path.exists("/opt/rocm/llvm/bin/llvm-objdump") else "objdump", "-h", path],
                         capture_output=True, text=True).stdout
    assert ".hip_fatbin" in out
    assert b"k_clip_vox_batch" in open(path, "rb").read()
