"""CPU checks of the batched-tracker ABI: the four entry points of N independent trackers per call are declared by include/lsm2d.h, bound
by the Python mirror and exported by the gfx950 build; the batched kernels are in the library's code object."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

NEW = ["lsm2d_cloudset_create_reserved_many", "lsm2d_cloudset_clear_clouds", "lsm2d_clip_scene_batch", "lsm2d_merge_scene_batch"]


def test_batch_symbols_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi, build
    header = open(os.path.join(ROOT, "include", "lsm2d.h")).read()
    bound = {s[0]: s for s in _capi.SYMBOLS}
    lib = C.CDLL(build.build())
    for name in NEW:
        assert name + "(" in header, name
        assert name in bound, name
        assert hasattr(lib, name), name
    assert len(bound["lsm2d_clip_scene_batch"][2]) == 9 and len(bound["lsm2d_merge_scene_batch"][2]) == 12


def test_batch_kernels_are_in_the_code_object():
    from srrg2_laser_slam_2d_amd import build
    path = build.build()
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump" if os.path.exists("/opt/rocm/llvm/bin/llvm-objdump") else "objdump", "-h", path],
                         capture_output=True, text=True).stdout
    assert ".hip_fatbin" in out
    blob = open(path, "rb").read()
    for k in (b"k_clip_batch", b"k_merge_batch"):
        assert k in blob, k
