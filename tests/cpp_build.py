"""The one place the tests and tests/bench/ compile a C++ driver with plain g++ against the C ABI (include/lsm2d.h), the host mirror
(srrg2_laser_slam_2d_amd/host/lsm2d.hpp) and, when asked, liblsm2d_hip.so.  Every caller passes the flags it always passed; only the line itself lives here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HOST = os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "host")
LIB = os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "lib")
CPP = os.path.join(ROOT, "tests", "cpp")


def _sources(source):
    names = [source] if isinstance(source, (str, os.PathLike)) else list(source)
    return [str(s) if os.path.isabs(str(s)) else os.path.join(CPP, str(s)) for s in names]


def _command(sources, flags, include_dirs):
    return ["g++", "-std=c++17", *flags, "-I" + INCLUDE, "-I" + HOST, "-I" + CPP, *("-I" + str(d) for d in include_dirs), *sources]


def build(source, out_dir, flags=("-O2",), include_dirs=(), link=True, link_flags=()):
    """Compiles `source` (a file of tests/cpp/ by name, an absolute path, or a list of either) into `out_dir` and returns the executable's path.  link: against
    liblsm2d_hip.so (True) or the library of that name (a string), with its directory as the run path; link_flags: what has to stand behind the sources."""
    sources = _sources(source)
    exe = os.path.join(str(out_dir), os.path.splitext(os.path.basename(sources[0]))[0])
    tail = ["-L" + LIB, "-l" + (link if isinstance(link, str) else "lsm2d_hip"), "-Wl,-rpath," + LIB] if link else []
    subprocess.run(_command(sources, flags, include_dirs) + tail + list(link_flags) + ["-o", exe], check=True)
    return exe


def syntax_only(source, flags=("-Wall", "-Wextra"), include_dirs=()):
    """g++ -fsyntax-only over `source`; returns the finished process (returncode, stderr) for the caller to assert on."""
    return subprocess.run(_command(_sources(source), list(flags) + ["-fsyntax-only"], include_dirs), capture_output=True, text=True)
