"""The live-tracker chain of tests/tracker_chain.py with the aligner in the REFERENCE'S order of summation: the sequential fp32 oracle
(lsmo_align_f with device_order = 0, what the library computes with "sum_order" 1) instead of the device-order mirror.  Same scenario,
parameters and digest fields; the goldens are tests/golden/tracker_chain_seq.json and tracker_replay_seq_1000.json
(tests/golden/make_tracker_chain_seq.py).  The device side is tracker_chain.run_device on a context with "sum_order" 1.
"""
import tracker_chain


class _SequentialOracle:
    """the oracle module with aligner_params forced to device_order = False; everything else passes through"""

    def __init__(self, po):
        self._po = po

    def aligner_params(self, *args, **kw):
        kw["device_order"] = False
        return self._po.aligner_params(*args, **kw)

    def __getattr__(self, name):
        return getattr(self._po, name)


def run_oracle(po, steps: int = 8, record_every: int = 1):
    """tracker_chain.run_oracle, aligned in the reference's order (record_every as there)"""
    return tracker_chain.run_oracle(_SequentialOracle(po), steps, record_every=record_every)
