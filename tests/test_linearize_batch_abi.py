"""CPU checks of the batched factor's ABI: lsm2d_linearize_batch is declared by include/lsm2d.h, bound by the Python mirror with its fourteen arguments and
exported by the gfx950 build; the three batch kernels are in the library's code object; the Python and the C++ mirror have their entries."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

NAME = "lsm2d_linearize_batch"


def test_linearize_batch_symbol_declared_bound_and_exported():
    from srrg2_laser_slam_2d_amd import _capi, build
    header = open(os.path.join(ROOT, "include", "lsm2d.h")).read()
    bound = {s[0]: s for s in _capi.SYMBOLS}
    lib = C.CDLL(build.build())
    assert NAME + "(" in header
    assert NAME in bound
    assert len(bound[NAME][2]) == 14
    assert hasattr(lib, NAME)
    assert "LSM2D_VERSION 160" in header      # an addition only: the number stays


def test_linearize_batch_kernels_are_in_the_code_object():
    from srrg2_laser_slam_2d_amd import build
    path = build.build()
    out = subprocess.run(["/opt/rocm/llvm/bin/llvm-objdump" if os.path.exists("/opt/rocm/llvm/bin/llvm-objdump") else "objdump", "-h", path],
                         capture_output=True, text=True).stdout
    assert ".hip_fatbin" in out
    blob = open(path, "rb").read()
    for k in (b"k_linearize_partial_batch", b"k_linearize_final_batch", b"k_linearize_seq_batch"):
        assert k in blob, k


def test_mirrors_have_linearize_batch():
    from srrg2_laser_slam_2d_amd import api
    assert callable(api.linearize_batch)
    hpp = open(os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "host", "lsm2d.hpp")).read()
    assert "linearizeBatch(" in hpp and "linearize(" in hpp
    assert "lsm2d_linearize_batch(" in hpp
