"""The owners of srrg2_laser_slam_2d_amd/csrc/lsm2d_capi_own.h (DevBuf, PinnedBuf, Event, Stream, the grow-on-demand pair and the live-handle count), checked
without a GPU: tests/cpp/capi_own_driver.cpp is a stand-alone program that defines the HIP functions the header calls on top of malloc / free, compiled with
the address and undefined-behaviour sanitizers and run.  It walks moves, self-moves, double resets, moved-from owners, caches in a reallocating vector, the
grow pair's three outcomes, the pinned buffer's device address and the borrowed stream, comparing the header's live count with the stand-ins' count at every
step.  A sanitizer report or a failed check is a non-zero exit status."""
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpp_build      # noqa: E402

CSRC = os.path.join(cpp_build.ROOT, "srrg2_laser_slam_2d_amd", "csrc")
ROCM_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_the_owners_release_once_and_count_what_lives(tmp_path):
    exe = cpp_build.build("capi_own_driver.cpp", tmp_path, flags=("-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                                  "-D__HIP_PLATFORM_AMD__"), include_dirs=(CSRC, ROCM_INCLUDE), link=False)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "owners ok" in r.stdout and "none left" in r.stdout, r.stdout


def test_the_header_stands_alone():
    """Host only: the runtime's API header, <atomic> and <utility>; no kernels and nothing of lsm2d.h."""
    text = open(os.path.join(CSRC, "lsm2d_capi_own.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ["<hip/hip_runtime_api.h>", "<atomic>", "<utility>"], includes
    assert "__global__" not in text and "lsm2d.h\"" not in text
