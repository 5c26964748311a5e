"""The placement deal's test harness, without a GPU: the sequential restatement of balance_order satisfies every property the checker states, under any
order of ties; the checker rejects each kind of wrong deal; `expect` reads a batch as the host does; and the device driver still compiles against the
library's headers (tests/placement_cases.py, tests/cpp/placement_deal_driver.hip; the device run is tests/test_gpu_placement_deal.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import placement_cases as pc
from conftest import ROOT

CSRC = os.path.join(ROOT, "srrg2_laser_slam_2d_amd", "csrc")


def test_constants_are_the_headers():
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("lsm2d_kernels.h", "lsm2d_k_align_args.h", "lsm2d_k_placement.h"))

    def const(name):
        m = re.search(r"\b%s = ([0-9+* ()a-zA-Z]+?)[,;]" % name, text)
        assert m, name
        return eval(m.group(1), {"kPackMaxRounds": 3})
    assert (const("kAlignBlock"), const("kPlaceKeys")) == (pc.ALIGN_BLOCK, pc.PLACE_KEYS)
    assert (const("kBalMaxFirst"), const("kBalMaxLevels"), const("kBalMaxGroups")) == (pc.MAX_FIRST, pc.MAX_LEVELS, pc.MAX_GROUPS)
    assert (const("kPackConst"), const("kPackMaxRounds")) == (pc.PACK_CONST, pc.PACK_MAX_ROUNDS)
    assert (const("kOrderInts"), const("kPackOrder2At"), const("kPackSecondsAt")) == (pc.ORDER_INTS, pc.ORDER2_AT, pc.SECONDS_AT)
    assert re.search(r"balance_order\(\*reinterpret_cast<BalanceLds\*>\(smem\), work, \(int\) gridDim\.x, n_cu, 4, order, place, tid, kAlignBlock, order2\)", text)      # PER_CU and nt


def test_cases_cover_the_grid_and_every_form():
    cases = pc.cases()
    assert 200 <= len(cases) <= 500
    assert {(c["n_cu"], c["n"]) for c in cases} >= {(u, n) for u in pc.N_CUS for n in pc.SIZES}
    assert {c["counts_kind"] for c in cases} == set(pc.COUNT_KINDS) and {c["notes_kind"] for c in cases} == set(pc.NOTE_KINDS)
    for c in cases:      # the contract the host guarantees
        assert 1 <= c["n"] <= 4096 and c["n_cu"] >= 1 and c["work"].dtype == np.int32 and c["work"].min() >= 0 and c["work"].max() <= pc.ALIGN_BLOCK
        assert c["place"] is None or (c["place"].dtype == np.int32 and c["place"].size >= pc.first_round(c["n"], c["n_cu"]))
    t = pc.tally(cases)
    assert all(v > 0 for v in t.values()), t
    again = pc.make_case(1025, 256, "uniform", "mixed", True, np.random.default_rng(5))
    same = pc.make_case(1025, 256, "uniform", "mixed", True, np.random.default_rng(5))
    assert np.array_equal(again["work"], same["work"]) and np.array_equal(again["place"], same["place"])


@pytest.mark.parametrize("tie_seed", [0, 1, 2])
def test_the_restated_function_passes_every_check(tie_seed):
    rng = np.random.default_rng(1000 + tie_seed)
    for c in pc.cases():
        pc.check(c, pc.model(c, rng))


def _case(n, n_cu, counts, notes, order2, seed=7):
    c = pc.make_case(n, n_cu, counts, notes, order2, np.random.default_rng(seed))
    b = pc.model(c, np.random.default_rng(seed + 1))
    pc.check(c, b)
    return c, b, pc.expect(c)


def test_checker_rejects_a_duplicated_entry():
    for args in ((1000, 256, "uniform", "four", False), (1025, 256, "uniform", "four", True), (2049, 256, "uniform", "nine", False)):
        c, b, e = _case(*args)
        for dst, src in ((3, 5), (e["n_wg"] - 1, 0)):
            bad = b.copy(); bad[dst] = bad[src]
            with pytest.raises(AssertionError, match="check 2"):
                pc.check(c, bad)
    c, b, e = _case(1025, 256, "uniform", "four", True)
    bad = b.copy(); b2 = int(np.flatnonzero(bad[pc.ORDER2_AT:pc.ORDER2_AT + 1024] >= 0)[0]); bad[pc.ORDER2_AT + b2] = bad[7]      # a second that some workgroup runs as its first
    with pytest.raises(AssertionError, match="check 2"):
        pc.check(c, bad)
    bad = b.copy(); bad[11] = c["n"]                                                                                          # an alignment that does not exist
    with pytest.raises(AssertionError, match="check 2"):
        pc.check(c, bad)


def test_checker_rejects_a_tail_out_of_order():
    for args in ((2100, 256, "uniform", "four", False), (2100, 256, "uniform", "one_key", False), (1100, 304, "uniform", "none", True)):
        c, b, e = _case(*args)
        assert not e["packed"]
        w = c["work"][b[:c["n"]]]
        r = e["first"] + int(np.flatnonzero(w[e["first"] + 1:] != w[e["first"]:-1])[0])      # two neighbours of unequal count beyond the first round
        bad = b.copy(); bad[[r, r + 1]] = bad[[r + 1, r]]
        with pytest.raises(AssertionError, match="check 3"):
            pc.check(c, bad)
        # ... and the lightest of the first round against the heaviest behind it
        f = int(np.argmin(w[:e["first"]]))
        assert w[f] > w[-1]
        bad = b.copy(); bad[[f, c["n"] - 1]] = bad[[c["n"] - 1, f]]
        with pytest.raises(AssertionError, match="check 3"):
            pc.check(c, bad)


def test_checker_rejects_a_second_swapped_with_a_heavier_single():
    for args in ((1048, 256, "uniform", "four", True), (1100, 128, "uniform", "mixed", True), (3080, 256, "uniform", "distinct", True)):
        c, b, e = _case(*args)
        assert e["packed"]
        o2 = b[pc.ORDER2_AT:pc.ORDER2_AT + e["n_bins"]]
        w1 = c["work"][b[:e["n_bins"]]]
        single = int(np.argmax(np.where(o2 < 0, w1, -1)))                       # the heaviest single: heavier than every paired alignment
        pair = int(np.flatnonzero(o2 >= 0)[0])
        assert w1[single] > np.sort(c["work"])[2 * e["pairs"] - 1]
        bad = b.copy(); bad[single], bad[pc.ORDER2_AT + pair] = b[pc.ORDER2_AT + pair], b[single]
        with pytest.raises(AssertionError, match="check 4"):
            pc.check(c, bad)
    # two pairs' seconds exchanged: the same alignments paired, the pairing rule broken
    c, b, e = _case(1100, 256, "uniform", "four", True)
    o2 = b[pc.ORDER2_AT:pc.ORDER2_AT + e["n_bins"]]
    ws = np.where(o2 >= 0, c["work"][np.maximum(o2, 0)], -1)
    lo, hi = int(np.argmax(np.where(o2 >= 0, -ws, -10 ** 6))), int(np.argmax(ws))
    assert ws[lo] < ws[hi] and c["work"][b[lo]] != c["work"][b[hi]]
    bad = b.copy(); bad[pc.ORDER2_AT + lo], bad[pc.ORDER2_AT + hi] = b[pc.ORDER2_AT + hi], b[pc.ORDER2_AT + lo]
    with pytest.raises(AssertionError, match="check 4"):
        pc.check(c, bad)


def test_checker_rejects_the_heavier_group_holding_the_heavier_item():
    n_checked = 0
    for args in ((1000, 256, "uniform", "four", False), (1024, 304, "uniform", "none", False), (1024, 256, "tail", "mixed", True), (600, 100, "uniform", "high_bits", False)):
        c, b, e = _case(*args)
        assert not e["fallback"] and not e["packed"]
        first = e["first"]
        keys, w = pc.keys_of(c, first), c["work"][b[:first]].astype(np.int64)
        # per group: its workgroup ids, heaviest alignment first -- the id at position k holds the group's level-k item
        groups = {}
        for wg in np.lexsort((-w, keys)):
            groups.setdefault(int(keys[wg]), []).append(int(wg))
        for k in (1, 2):
            at = [(sum(w[m[:k]]), w[m[k]], m[k]) for m in groups.values() if len(m) > k]
            at.sort()
            (s_lo, c_lo, wg_lo), (s_hi, c_hi, wg_hi) = at[0], at[-1]                # the group that carries least so far, and the one that carries most
            assert s_lo < s_hi and c_lo > c_hi, (args, k)
            bad = b.copy(); bad[[wg_lo, wg_hi]] = bad[[wg_hi, wg_lo]]
            with pytest.raises(AssertionError, match="check 5: level %d: a group carrying" % k):
                pc.check(c, bad)
            n_checked += 1
        # an item moved to another level altogether: a level-0 item with a lighter level-1 item of another group
        m0, m1 = list(groups.values())[0], [m for m in groups.values() if len(m) > 1][-1]
        if w[m0[0]] != w[m1[1]] and m0 is not m1:
            bad = b.copy(); bad[[m0[0], m1[1]]] = bad[[m1[1], m0[0]]]
            with pytest.raises(AssertionError, match="check 5"):
                pc.check(c, bad)
    assert n_checked == 8
    # equal groups whose sums lie too far apart: every group's items in place, the first round a set of counts the deal would not have spread like this
    c, b, e = _case(1024, 256, "uniform", "four", False)
    keys, w = pc.keys_of(c, 1024), c["work"][b[:1024]]
    by_key = np.argsort(keys, kind="stable")                                         # four ids per key, side by side
    bad = b.copy(); bad[by_key] = b[:1024][np.argsort(-w, kind="stable")]             # ... get four NEIGHBOURS of the descending order: the first group the four heaviest
    with pytest.raises(AssertionError, match="check 5"):
        pc.check(c, bad)


def test_checker_rejects_a_stray_word_and_a_second_beyond_the_first_round():
    for args, packed in (((1000, 256, "uniform", "four", False), False), ((1025, 256, "uniform", "four", True), True), ((2049, 256, "uniform", "four", False), False),
                         ((2049, 256, "uniform", "nine", True), True), ((1, 256, "equal", "none", True), False)):
        c, b, e = _case(*args)
        assert e["packed"] == packed
        edges = [e["n_wg"], pc.ORDER2_AT - 1, pc.ORDER_INTS - 1, pc.SECONDS_AT + e["pairs"]]
        edges += [pc.ORDER2_AT + e["n_bins"], pc.SECONDS_AT - 1] if packed else [pc.ORDER2_AT, pc.SECONDS_AT]
        for at in edges:
            if at >= pc.ORDER_INTS:
                continue
            assert b[at] == pc.SENTINEL, (args, at)
            for value in (0, -1):
                bad = b.copy(); bad[at] = value
                with pytest.raises(AssertionError, match="check 1"):
                    pc.check(c, bad)
    # a pair moved to a workgroup of the second round: still every alignment once, still E pairs
    for args in ((2049, 256, "uniform", "four", True), (3080, 256, "tail", "one_key", True)):
        c, b, e = _case(*args)
        o2 = b[pc.ORDER2_AT:pc.ORDER2_AT + e["n_bins"]]
        src, dst = int(np.flatnonzero(o2 >= 0)[0]), e["first"] + 3
        bad = b.copy(); bad[pc.ORDER2_AT + dst], bad[pc.ORDER2_AT + src] = b[pc.ORDER2_AT + src], -1
        with pytest.raises(AssertionError, match="check 4: workgroup %d, beyond the first round" % dst):
            pc.check(c, bad)
        bad = b.copy(); bad[pc.ORDER2_AT + e["n_bins"] - 1] = pc.SENTINEL                 # ... and an order2 word nobody wrote
        with pytest.raises(AssertionError, match="check 4"):
            pc.check(c, bad)


def test_checker_rejects_a_fallback_that_is_not_heaviest_first():
    for args in ((1000, 256, "uniform", "nine", False), (1024, 1024, "uniform", "none", False), (1048, 256, "uniform", "one_key", True)):
        c, b, e = _case(*args)
        assert e["fallback"]
        w = c["work"][b[:e["first"]]]
        r = e["pairs"] + int(np.flatnonzero(w[e["pairs"] + 1:] != w[e["pairs"]:-1])[0])
        bad = b.copy(); bad[[r, r + 1]] = bad[[r + 1, r]]
        with pytest.raises(AssertionError, match="check 6"):
            pc.check(c, bad)


def test_expect_reads_a_batch_as_the_host_does():
    """pack_two_for (lsm2d_capi_aligner.inc) packs, on the 256-CU part, the sizes test_gpu_aligner_paths.py's width rule lists with 1024 workgroups; the kernel
    must then read the batch as packed too -- and never a batch of whole rounds, or one without order2."""
    rng = np.random.default_rng(0)
    for n in (1025, 1040, 1048, 1537, 1700, 2047, 2049, 2064, 3073, 3080):
        e = pc.expect(pc.make_case(n, 256, "uniform", "four", True, rng))
        assert e["packed"] and e["first"] == 1024 and e["n_wg"] == (n // 1024) * 1024 and e["pairs"] == n % 1024, n
        assert not pc.expect(pc.make_case(n, 256, "uniform", "four", False, rng))["packed"], n
    for n in (1024, 2048, 3072, 4096, 1000, 257):
        assert not pc.expect(pc.make_case(n, 256, "uniform", "four", True, rng))["packed"], n
    e = pc.expect(pc.make_case(4095, 256, "uniform", "four", True, rng))
    assert e["packed"] and e["pairs"] == 1023 and not e["fallback"]
    for notes, fallback in (("nine", True), ("one_key", True), ("distinct", True), ("max_groups", False), ("mixed", False), ("high_bits", False), ("none", False)):
        assert pc.expect(pc.make_case(1024, 256, "uniform", notes, False, rng))["fallback"] == fallback, notes
    assert pc.expect(pc.make_case(4096, 1024, "uniform", "none", False, rng))["too_many_groups"]      # the round-3 assumption on a part of more than 512 CUs


def test_case_file_round_trip(tmp_path):
    cases = pc.cases()[:7]
    path = str(tmp_path / "cases.bin")
    pc.write_cases(path, cases)
    raw = np.fromfile(path, "<i4")
    assert raw[0:1].tobytes() == pc.MAGIC and raw[1] == 7
    at = 2
    for c in cases:
        n, n_cu, n_place, o2 = raw[at:at + 4]
        assert (n, n_cu, bool(o2)) == (c["n"], c["n_cu"], c["order2"]) and n_place == (0 if c["place"] is None else c["place"].size)
        assert np.array_equal(raw[at + 4:at + 4 + n], c["work"])
        at += 4 + n + n_place
    assert at == raw.size
    with pytest.raises(AssertionError):      # the contract holds for the file, too
        bad = dict(cases[0], work=cases[0]["work"] + pc.ALIGN_BLOCK + 1)
        pc.write_cases(path, [bad])


def test_the_driver_compiles_for_gfx950(tmp_path):
    """A compile only: a change to lsm2d_k_placement.h that breaks the harness shows without a GPU."""
    exe = str(tmp_path / "placement_deal_driver")
    r = subprocess.run(pc.driver_command(exe),capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and os.path.exists(exe), r.stdout + r.stderr
