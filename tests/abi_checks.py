"""What every tests/test_*_abi.py asks of a new entry point, stated once: declared by include/lsm2d.h, bound by the Python mirror with as many arguments,
exported by the gfx950 build, the version number unchanged; its kernels in the library's code object; its entries in the Python and the C++ mirror."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

HOST = os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "host")


def header(name="lsm2d.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def bound_symbols(table="SYMBOLS"):
    """name -> (name, restype, argtypes) of the Python mirror's binding table (LOGODDS_SYMBOLS: the extension header's)"""
    from srrg2_laser_slam_2d_amd import _capi
    return {s[0]: s for s in getattr(_capi, table)}


def assert_declared_bound_exported(name, n_args=None, header_name="lsm2d.h", table="SYMBOLS"):
    """`name` is declared in include/<header_name>, bound in _capi.<table> and exported by the build -- with n_args parameters in the declaration and in the
    binding, if given -- and lsm2d.h still says LSM2D_VERSION 160 (entry points are additions).  Returns the binding for further checks."""
    from srrg2_laser_slam_2d_amd import build
    text = header()
    plain = re.sub(r"/\*.*?\*/", "", header(header_name), flags=re.S)
    bound = bound_symbols(table)
    assert name + "(" in plain, name
    assert name in bound, name
    assert hasattr(C.CDLL(build.build()), name), name
    if n_args is not None:
        decl = plain[plain.index(name + "("):]
        assert decl[:decl.index(");")].count(",") + 1 == n_args, name
        assert len(bound[name][2]) == n_args, name
    assert "LSM2D_VERSION 160" in text
    return bound[name]


def assert_kernels_in_code_object(names):
    """The built library carries a HIP code object, and every name (bytes) occurs in it."""
    from srrg2_laser_slam_2d_amd import build
    path = build.build()
    objdump = "/opt/rocm/llvm/bin/llvm-objdump" if os.path.exists("/opt/rocm/llvm/bin/llvm-objdump") else "objdump"
    assert ".hip_fatbin" in subprocess.run([objdump, "-h", path], capture_output=True, text=True).stdout
    blob = open(path, "rb").read()
    for k in names:
        assert k in blob, k


def assert_mirrors_have(api_names, hpp_needles, hpp="lsm2d.hpp"):
    """The Python mirror has the callables `api_names`; the C++ mirror's header `hpp` contains every needle.  Returns the header's text."""
    from srrg2_laser_slam_2d_amd import api
    for name in [api_names] if isinstance(api_names, str) else api_names:
        assert callable(getattr(api, name)), name
    text = open(os.path.join(HOST, hpp)).read()
    for needle in hpp_needles:
        assert needle in text, needle
    return text
