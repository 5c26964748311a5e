"""Every C++ program under tests/cpp/ -- the mirror drivers, the bare-ABI benches, the CPU references and the stand-ins -- passes g++ -std=c++17 -fsyntax-only
-Wall -Wextra without a diagnostic.  The bench programs are otherwise compiled only when somebody runs their script on a GPU machine: a header or mirror change
that breaks one is found here instead.  (placement_deal_driver.hip needs hipcc and is compiled by test_placement_model_cpu.py.)"""
import glob
import os

import pytest

import cpp_build

ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")
ADAPTER_DIRS = (os.path.join(cpp_build.ROOT, "adapters", "srrg"), os.path.join(cpp_build.CPP, "adapter_shim"))
# the four programs that include more than include/, the host mirror and tests/cpp/
INCLUDE_DIRS = {"adapter_driver.cpp": ADAPTER_DIRS, "adapter_sum_order_driver.cpp": ADAPTER_DIRS,
                "capi_own_driver.cpp": (os.path.join(cpp_build.ROOT, "srrg2_laser_slam_2d_amd", "csrc"), ROCM_INCLUDE),
                "stream_step_bench.cpp": (ROCM_INCLUDE,)}
FLAGS = {"capi_own_driver.cpp": ("-D__HIP_PLATFORM_AMD__",), "stream_step_bench.cpp": ("-D__HIP_PLATFORM_AMD__",)}
PROGRAMS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(cpp_build.CPP, "*.cpp")))


def test_there_are_programs_to_check():
    assert len(PROGRAMS) >= 39 and set(INCLUDE_DIRS) <= set(PROGRAMS)


@pytest.mark.parametrize("source", PROGRAMS)
def test_program_compiles_without_a_diagnostic(source):
    r = cpp_build.syntax_only(source, flags=("-Wall", "-Wextra") + FLAGS.get(source, ()), include_dirs=INCLUDE_DIRS.get(source, ()))
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
