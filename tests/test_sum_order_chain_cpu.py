"""CPU tests of the tracker chain in the reference's order of summation: the sequential fp32 oracle (device_order = 0, what the library computes with
"sum_order" 1) reproduces the committed goldens tests/golden/tracker_chain_seq.json and tracker_replay_seq_1000.json bit for bit
(tests/golden/make_tracker_chain_seq.py; tests/test_gpu_sum_order_latency.py holds the device to the same files)."""
import json

from conftest import golden_path


def test_tracker_chain_seq_digests(po):
    import tracker_chain_seq
    g = json.load(open(golden_path("tracker_chain_seq.json")))
    got = tracker_chain_seq.run_oracle(po, len(g["steps"]))
    assert got == g["steps"]
    assert all(st["status"] == 0 for st in got) and got[-1]["map_points"] > got[0]["map_points"]


def test_tracker_replay_seq_1000_digests(po):
    import tracker_chain_seq
    g = json.load(open(golden_path("tracker_replay_seq_1000.json")))
    got = tracker_chain_seq.run_oracle(po, g["steps_total"], record_every=g["record_every"])
    assert got == g["steps"]
    assert len(got) == 20 and all(st["status"] == 0 for st in got)


def test_the_two_orders_give_different_chains():
    """the goldens pin the reference's order, not the device's tree order again: the poses of the two chains differ"""
    for a, b in (("tracker_chain.json", "tracker_chain_seq.json"), ("tracker_replay_1000.json", "tracker_replay_seq_1000.json")):
        x, y = json.load(open(golden_path(a)))["steps"], json.load(open(golden_path(b)))["steps"]
        assert [s["step"] for s in x] == [s["step"] for s in y]
        assert any(s["pose_hex"] != t["pose_hex"] for s, t in zip(x, y))
