"""The placement deal on the device: balance_order (csrc/lsm2d_k_placement.h) alone, on chosen work counts and chosen notes.

Through the library the deal's inputs are the dispatcher's and the workload's: no aligner call on this chip puts nine workgroups on a CU or forms more than 512
groups, and the suite's batches carry twelve distinct counts.  tests/cpp/placement_deal_driver.hip calls the function as k_cull_estimate's last workgroup does,
one workgroup per case of tests/placement_cases.py, and every order block that comes back is held to what the header's comments promise (placement_cases.check:
nothing written astray, every alignment exactly once, heaviest first beyond the first round, the pairing rule of packed batches, the level-by-level deal, the
plain order where the notes cannot be used).  Which alignment of equal count lands where is the atomics' business: two runs of the same cases need not agree, and
both must pass.  One test goes through the library: what the deal hands k_align and k_align_two is run, every alignment once."""
import subprocess

import numpy as np
import pytest

import placement_cases as pc
from gpu_helpers import _aligner
from srrg2_laser_slam_2d_amd import api, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def deal_driver(tmp_path_factory):
    """the driver, built once with the library's flags, and the case file"""
    d = tmp_path_factory.mktemp("placement_deal")
    exe, case_file = str(d / "placement_deal_driver"), str(d / "cases.bin")
    subprocess.run(pc.driver_command(exe), check=True, timeout=300)
    pc.write_cases(case_file, pc.cases())
    return exe, case_file, d


def _run(deal_driver, name):
    exe, case_file, d = deal_driver
    out = str(d / name)
    r = subprocess.run(["timeout", "-k", "10", "120", exe, case_file, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    return pc.read_blocks(out, len(pc.cases()))


def _check_all(blocks):
    failed = []
    for c, b in zip(pc.cases(), blocks):
        try:
            pc.check(c, b)
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, "%d of %d cases:\n%s" % (len(failed), len(blocks), "\n".join(failed[:20]))


def test_the_deal_keeps_its_promises_on_chosen_inputs(deal_driver):
    t = pc.tally(pc.cases())
    print("placement deal: %(cases)d cases; the deal %(deal)d (packed %(packed_deal)d), packed %(packed)d, fallback for more than 8 on a key %(fallback_over_eight)d, "
          "fallback for more than 512 groups %(fallback_too_many_groups)d (packed fallbacks %(packed_fallback)d); exactly 8 on a key %(eight_on_a_key)d, exactly 512 groups %(groups_512)d" % t)
    assert all(v > 0 for v in t.values()), t
    _check_all(_run(deal_driver, "blocks_0.bin"))


def test_the_promises_do_not_depend_on_the_order_of_the_atomics(deal_driver):
    a, b = _run(deal_driver, "blocks_1.bin"), _run(deal_driver, "blocks_2.bin")
    print("placement deal: %d of %d cases came out word for word the same in two runs" % (sum(np.array_equal(x, y) for x, y in zip(a, b)), len(a)))
    _check_all(a)
    _check_all(b)


def test_what_the_deal_hands_the_aligner_kernels_is_run_once_each(ctx):
    """The hand-over: order / order2 as k_align and k_align_two read them.  A placed batch -- by the round-3 assumption, then by the first launch's notes -- equals the
    batch run with workgroup i on alignment i in every bit, and no status is the word the host fills the statuses with before the launch: an alignment
    nobody ran fails here by itself, not by comparison (257: one round and one workgroup; 1025 and 2049: packed, one and two whole rounds with one pair)."""
    wl = synth.make_workload(12, 60000, seed=31, map_noise=0.004, scan_noise=0.004)
    fixed = api.CloudSet(ctx, wl.scan_points, wl.scan_offsets); moving = api.CloudSet(ctx, wl.map_points)
    al = _aligner(ctx)
    not_written = np.int32(-1)      # kStatusNotWritten: the 0xFF bytes of lsm2d_capi_aligner.inc's memset
    was = ctx.get_option("balance")
    try:
        for n in (257, 1025, 2049):
            fb = (np.arange(n, dtype=np.int32) % 12).reshape(1, n)
            runs = []
            for k, balance in enumerate((1, 1, 0)):
                ctx.set_option("balance", balance)
                runs.append(al.compute_batch([fixed], [moving], wl.x0[fb[0]], fixed_index=fb, want_stats=True))
                if k == 0:
                    assert ctx.get_option("last_cull_estimate") == 1, n
                if balance == 1 and n > 1024:      # (the packed form: k_align_two reads order2)
                    assert ctx.get_option("last_align_width") == 1024, (n, k, ctx.get_option("last_align_width"))
                if balance == 0:
                    assert ctx.get_option("last_cull_estimate") == 0, n
            plain = runs[-1]
            for k, r in enumerate(runs):
                assert r.status.shape == (n,) and not np.any(r.status.astype(np.int32) == not_written), (n, k, np.flatnonzero(r.status.astype(np.int32) == not_written)[:8])
            assert np.any(plain.status == 0)
            for k, r in enumerate(runs[:-1]):
                for field in ("pose", "information", "status", "iterations", "stats"):
                    got, want = np.ascontiguousarray(getattr(r, field)), np.ascontiguousarray(getattr(plain, field))
                    assert got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes(), (n, k, field)
    finally:
        ctx.set_option("balance", was)
