"""Generates tests/golden/reference_params.json: what tests/test_abi.py checks the adapters, the compile shim and the Python mirror against,
read out of the reference project's headers and sources once (data only, no source text):
  params      -- every PARAM (property type, numeric default or "expr") of the six reference classes the adapters replace or recognise
  member_ids  -- every underscore identifier (`_fixed`, `_meas`, ...) the reference's .h / .hpp / .cpp files use

    python tests/golden/make_reference_params.py PATH/TO/srrg2_laser_slam_2d
"""
import glob
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_abi import REFERENCE_CLASSES, _params_of      # noqa: E402

if __name__ == "__main__":
    ref = os.path.abspath(sys.argv[1])
    src = os.path.join(ref, "src", "srrg2_laser_slam_2d")
    params = {}
    for header, cls in REFERENCE_CLASSES:
        got = _params_of(open(os.path.join(src, header)).read(), cls)
        assert got, (header, cls)
        params[cls] = {"header": header, "params": {name: [typ, default] for name, (typ, default) in got.items()}}
    ids = set()
    for p in glob.glob(ref + "/**/*", recursive=True):
        if os.path.isfile(p) and p.endswith((".h", ".hpp", ".cpp")):
            ids |= set(re.findall(r"\b_[a-z][a-zA-Z_0-9]*\b", open(p, errors="ignore").read()))
    out = {"note": "read out of the reference project's headers and sources by tests/golden/make_reference_params.py", "params": params,
           "member_ids": sorted(ids)}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_params.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path, "(%d classes, %d member names)" % (len(params), len(ids)))
