"""The C ABI calls the C++ host mirror (srrg2_laser_slam_2d_amd/host/lsm2d.hpp) makes, checked without a GPU -- tests/test_api_calls_cpu.py applied to C++:
tests/cpp/mirror_trace_driver.cpp runs one script over every public function and class method of the header, then every refusal a caller can reach without a
device, linked against tests/cpp/lsm2d_standin.cpp, which records every call -- the symbol and every argument -- and what the driver got back.  The record
is compared with the stored one (tests/golden/cpp_mirror_call_trace.json, taken from lsm2d.hpp as it stood BEFORE it was rewritten to state each thing once;
``python tests/test_cpp_mirror_calls_cpu.py --write`` writes the file from the header it runs on: only ever do that on a commit whose header is trusted, never
to make a failing comparison pass).

The stand-in also follows every handle: one that arrives in a call after its destroy, or is destroyed twice, ends the run (exit status 3), and after every
scene whatever was made and not destroyed is reported (exit status 4).  The header the stored record was taken from leaked in two scenes -- the second create
of TrackerBatch's constructor failing, the second lsm2d_preprocess_scans of TrackerBatch::reset failing -- and the record does not hold the leak check's
verdict, so that this one difference could be mended."""
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpp_build      # noqa: E402

GOLDEN = os.path.join(cpp_build.ROOT, "tests", "golden", "cpp_mirror_call_trace.json")


def _run(out_dir):
    exe = cpp_build.build(["mirror_trace_driver.cpp", "lsm2d_standin.cpp"], out_dir, flags=("-O1", "-Wall", "-Wextra"), link=False)
    return subprocess.run([exe], capture_output=True, text=True)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    return _run(tmp_path_factory.mktemp("mirror_trace"))


def test_the_calls_are_the_recorded_ones(run):
    want = json.load(open(GOLDEN))
    got = run.stdout.splitlines()
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "line %d" % i
    assert len(got) == len(want)


def test_the_header_references_the_symbols_the_stand_in_defines():
    import re
    used = set(re.findall(r"\b(lsm2d_[a-z0-9_]+)\(", open(os.path.join(cpp_build.HOST, "lsm2d.hpp")).read()))
    defined = set(re.findall(r"^(?:[a-z0-9_]+\*? )+\*?(lsm2d_[a-z0-9_]+)\(", open(os.path.join(cpp_build.CPP, "lsm2d_standin.cpp")).read(), re.M))
    assert used == defined


def test_no_handle_is_used_after_its_destroy_and_none_leaks(run):
    assert run.returncode == 0 and run.stderr == "", run.stderr


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_cpp_mirror_calls_cpu.py --write      (writes %s from the lsm2d.hpp it runs on)" % GOLDEN)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        r = _run(d)
    sys.stderr.write(r.stderr)
    if r.returncode not in (0, 4):
        sys.exit("the driver ended with status %d" % r.returncode)
    lines = r.stdout.splitlines()
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(line) for line in lines) + "\n]\n")
    print("%d lines, %d bytes, driver status %d" % (len(lines), os.path.getsize(GOLDEN), r.returncode))
