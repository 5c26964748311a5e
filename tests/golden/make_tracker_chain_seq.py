"""Generates tests/golden/tracker_chain_seq.json and tracker_replay_seq_1000.json: ORACLE-GENERATED digests (NOT reference outputs) of the
live-tracker chain of tests/tracker_chain.py with the aligner in the reference's order of summation -- the sequential fp32 oracle
(device_order = 0), which the library equals bit for bit with the option "sum_order" 1 (tests/tracker_chain_seq.py).
tests/test_sum_order_chain_cpu.py holds the oracle to both files on the CPU box, tests/test_gpu_sum_order_latency.py the HIP path on the MI355X.

    python tests/golden/make_tracker_chain_seq.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as po          # noqa: E402
import tracker_chain_seq                   # noqa: E402

NOTE = "oracle-generated digests (sha256[:20] of the float32 arrays), not reference outputs; aligner in the reference's order (sequential fp32 oracle)"

if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    out = {"note": NOTE, "scenario": "tests/tracker_chain.py scenario(8)", "steps": tracker_chain_seq.run_oracle(po, 8)}
    path = os.path.join(here, "tracker_chain_seq.json")
    json.dump(out, open(path, "w"), indent=1)
    print("wrote", path, "final map", out["steps"][-1]["map_points"], "points")
    out = {"note": NOTE, "scenario": "tests/tracker_chain.py scenario(1000)", "steps_total": 1000, "record_every": 50,
           "steps": tracker_chain_seq.run_oracle(po, 1000, record_every=50)}
    path = os.path.join(here, "tracker_replay_seq_1000.json")
    json.dump(out, open(path, "w"), indent=1)
    print("wrote", path, "final map", out["steps"][-1]["map_points"], "points")
