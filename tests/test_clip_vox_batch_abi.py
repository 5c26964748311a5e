"""CPU checks of the batched voxelising clipper's ABI: lsm2d_clip_scene_voxelized_batch is declared by include/lsm2d.h, bound by the Python
mirror with its 10 arguments and exported by the gfx950 build; k_clip_vox_batch is in the library's code object."""
import ctypes as C

import abi_checks

NAME = "lsm2d_clip_scene_voxelized_batch"


def test_symbol_declared_bound_and_exported():
    binding = abi_checks.assert_declared_bound_exported(NAME, 10)
    assert binding[2][7] is C.c_float      # voxelize_resolution, by value
    header = abi_checks.header()
    assert "scene_clipper_projective_2d.cpp:36-48" in header[header.index("/* lsm2d_clip_scene_voxelized for n_trackers"):header.index(NAME + "(")]


def test_kernel_is_in_the_code_object():
    abi_checks.assert_kernels_in_code_object((b"k_clip_vox_batch",))
