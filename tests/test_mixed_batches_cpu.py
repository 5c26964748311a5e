"""The mixed-batch generator (tests/mixed_batches.py) held to what it claims, on the CPU alone: a generator that drifted into batches where everything
converges would let tests/test_gpu_launch_forms.py pass without meeting the packed workgroups' hard cases.  Both fp32 oracles: the sequential one (the
reference's order) and the device-order one (the tree order)."""
import collections
import math

import numpy as np
import pytest

import mixed_batches as mb

SAMPLE = 400      # ten blocks of 40: every kind at least ten times


@pytest.mark.parametrize("setting", mb.SETTINGS)
def test_mixed_batch_kinds_give_their_statuses(po, setting):
    spec = mb.batch(2024, SAMPLE, setting)
    assert set(spec["kinds"]) == set(mb.KINDS)
    for device_order in (False, True):
        statuses, its, early = collections.Counter(), set(), 0
        for i in range(SAMPLE):
            k = spec["kinds"][i]
            r = mb.oracle_align(po, spec, i, device_order=device_order)
            want = mb.CLAIMED_STATUS[k]
            if want is not None:
                assert r["status"] in want, (setting, device_order, i, k, r["status"], r["iterations"])
            if k in ("far", "empty"):
                assert r["iterations"] == 1, (setting, device_order, i, k, r["iterations"])
            if k in mb.NON_FINITE:
                assert r["status"] != 0, (setting, device_order, i, k)
            statuses[r["status"]] += 1; its.add(r["iterations"])
            early += int(r["status"] == 0 and r["iterations"] < spec["max_iterations"])
        print(setting, "device order" if device_order else "sequential", "statuses", dict(statuses), "iteration counts", sorted(its), "early stops", early)
        assert statuses[0] and statuses[1] and statuses[2], (setting, device_order, statuses)
        assert len(its) >= 3, (setting, device_order, its)
        if setting == "S2":      # the termination criterion ends some successful runs before max_iterations
            assert early > 0, (setting, device_order)


def test_mixed_batch_is_deterministic_and_a_prefix():
    for setting in mb.SETTINGS:
        a, b, c = mb.batch(5, 300, setting), mb.batch(5, 300, setting), mb.batch(5, 1040, setting)
        assert np.array_equal(a["kinds"], b["kinds"]) and np.array_equal(a["fixed_index"], b["fixed_index"])
        assert a["x0"].tobytes() == b["x0"].tobytes() and a["x0"].tobytes() == c["x0"][:300].tobytes()      # (bytes: NaN starts compare too)
        assert np.array_equal(a["fixed_index"], c["fixed_index"][:, :300]) and np.array_equal(a["kinds"], c["kinds"][:300])
        for sa, sb in zip(a["slices"], b["slices"]):
            assert np.array_equal(sa["pts"], sb["pts"]) and np.array_equal(sa["offs"], sb["offs"])
        if a["priors"] is not None:
            assert all(np.array_equal(p[0], q[0]) and np.array_equal(p[1], q[1]) for p, q in zip(a["priors"], c["priors"][:300]))
        # the kinds are spread through the batch: every block of 40 holds each of them
        for lo in range(0, 1040 - 40, 40):
            assert set(c["kinds"][lo:lo + 40]) == set(mb.KINDS), (setting, lo)
    assert not np.array_equal(mb.batch(5, 300, "S1")["x0"][:, :2], mb.batch(6, 300, "S1")["x0"][:, :2])
