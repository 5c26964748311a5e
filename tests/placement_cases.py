"""The placement deal (balance_order, csrc/lsm2d_k_placement.h) on chosen inputs: the cases, what the header promises for each, the function restated
sequentially, and the checker the CPU and GPU tests share.

A case is what k_cull_estimate's last workgroup hands the function: n work counts in [0, kAlignBlock], the chip's n_cu, the previous launch's notes (or none)
and whether the batch may be packed (order2 given).  tests/cpp/placement_deal_driver.hip runs the function alone on the device, one workgroup per case, and
returns the whole order block -- kOrderInts words that were SENTINEL before the launch.

`expect` states from the header's comments which form a case takes (packed or not, the deal or the plain heaviest-first order); `check` holds a block to the
properties those comments promise, from the block alone: WHICH alignment of equal count lands where, and which group gets which dense id, is settled by LDS
atomics on the device, so counts are compared, never alignment numbers against `model`.  `model` is the function as sequential Python with ties and group ids
in an order drawn from a generator: tests/test_placement_model_cpu.py holds it to `check` (the properties are the function's, not an accident of one tie
order) and shows that `check` rejects each kind of wrong deal."""
import itertools
import os

import numpy as np

from srrg2_laser_slam_2d_amd import build

# csrc/lsm2d_kernels.h, lsm2d_k_align_args.h, lsm2d_k_placement.h (test_placement_model_cpu.py reads them back from the headers)
ALIGN_BLOCK = 512
PLACE_KEYS = 4096
MAX_FIRST, MAX_LEVELS, MAX_GROUPS = 1024, 8, 512
PACK_CONST, PACK_MAX_ROUNDS = 150, 3
ORDER_INTS, ORDER2_AT, SECONDS_AT = 8192, 4096, 4096 + 3 * 1024
PER_CU = 4            # what k_cull_estimate passes
SENTINEL = -7
MAGIC = b"PDC1"

N_CUS = (256, 64, 100, 128, 304, 1024)
SIZES = (1, 2, 255, 256, 257, 600, 1000, 1023, 1024, 1025, 1048, 1100, 1536, 2047, 2048, 2049, 2100, 3071, 3072, 3073, 4000, 4095, 4096)
COUNT_KINDS = ("uniform", "equal", "two", "ends", "tail", "distinct")
NOTE_KINDS = ("none", "four", "mixed", "nine", "one_key", "distinct", "max_groups", "high_bits")


def first_round(n, n_cu):
    return min(n, PER_CU * n_cu, MAX_FIRST)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _counts(kind, n, rng):
    if kind == "distinct" and n > ALIGN_BLOCK + 1:
        kind = "uniform"
    if kind == "uniform":
        w = rng.integers(0, ALIGN_BLOCK + 1, n)
    elif kind == "equal":
        w = np.full(n, rng.integers(0, ALIGN_BLOCK + 1))
    elif kind == "two":
        w = rng.choice([5, ALIGN_BLOCK], n)
    elif kind == "ends":
        w = rng.choice([0, 1, ALIGN_BLOCK - 1, ALIGN_BLOCK], n)
    elif kind == "tail":      # most alignments light, a few up against the clip
        w = np.minimum(ALIGN_BLOCK, np.floor(12.0 * (1.0 + rng.pareto(0.9, n))))
    else:
        w = rng.permutation(ALIGN_BLOCK + 1)[:n]
    return kind, np.ascontiguousarray(w, np.int32)


def _four_per_key(first, rng):
    keys = rng.choice(PLACE_KEYS, (first + 3) // 4, replace=False)
    return rng.permutation(np.repeat(keys, 4)[:first])


def _notes(kind, first, rng):
    """-> (kind used, keys of the first round's workgroup ids or None)"""
    if (kind in ("mixed", "nine") and first < 9) or (kind == "max_groups" and first != MAX_FIRST):
        kind = "four"
    if kind == "none":
        return kind, None
    if kind == "four":                # the shape of a 256-CU part
        k = _four_per_key(first, rng)
    elif kind == "mixed":             # 1 .. 8 workgroups on a key, one key with exactly 8
        sizes = [MAX_LEVELS]
        while sum(sizes) < first:
            sizes.append(min(int(rng.integers(1, MAX_LEVELS + 1)), first - sum(sizes)))
        keys = rng.choice(PLACE_KEYS, len(sizes), replace=False)
        k = rng.permutation(np.repeat(keys, sizes))
    elif kind == "nine":              # one key too many on one CU
        sizes = [MAX_LEVELS + 1] + [4] * ((first - 9) // 4) + ([(first - 9) % 4] if (first - 9) % 4 else [])
        keys = rng.choice(PLACE_KEYS, len(sizes), replace=False)
        k = rng.permutation(np.repeat(keys, sizes))
    elif kind == "one_key":           # (the key's byte counter overflows)
        k = np.full(first, rng.integers(0, PLACE_KEYS))
    elif kind == "distinct":
        k = rng.choice(PLACE_KEYS, first, replace=False)
    elif kind == "max_groups":        # the largest legal number of groups
        k = rng.permutation(np.repeat(rng.choice(PLACE_KEYS, MAX_GROUPS, replace=False), 2))
    else:                             # high_bits: only the low 12 bits are the key
        k = _four_per_key(first, rng).astype(np.int64) | (rng.integers(0, 1 << 19, first) << 12)
        k[::2] |= 1 << 31
        k = k.astype(np.uint32).view(np.int32)
    return kind, np.ascontiguousarray(k, np.int32)


def make_case(n, n_cu, counts, notes, order2, rng, pad_notes=False):
    first = first_round(n, n_cu)
    counts, work = _counts(counts, n, rng)
    notes, place = _notes(notes, first, rng)
    if place is not None and pad_notes:      # the library's buffer holds 1024 notes whatever the batch: the ones beyond the first round are nobody's
        place = np.concatenate([place, rng.integers(-2 ** 31, 2 ** 31, MAX_FIRST - first).astype(np.int32)])
    return dict(name="n=%d n_cu=%d counts=%s notes=%s%s order2=%d" % (n, n_cu, counts, notes, "+pad" if place is not None and pad_notes else "", int(order2)),
                n=int(n), n_cu=int(n_cu), work=work, place=place, order2=bool(order2), counts_kind=counts, notes_kind=notes)


def _packable(n, n_cu):
    first = first_round(n, n_cu)
    return first == PER_CU * n_cu and n % first != 0 and n // first <= PACK_MAX_ROUNDS and n < 4096


_cases = None


def cases():
    """Every (n_cu, n) of the grid; count kinds x note kinds dealt over them in a shuffled cycle (each combination comes up six times or more); order2
    given twice and withheld once where the batch can be packed, alternating elsewhere (there it must stay untouched); then the combinations the
    cycle cannot be relied on for, by name."""
    global _cases
    if _cases is not None:
        return _cases
    rng = np.random.default_rng(39)
    combos = [(c, k) for c in COUNT_KINDS for k in NOTE_KINDS]
    rng.shuffle(combos)
    cyc = itertools.cycle(combos)
    out, i = [], 0
    for n_cu in N_CUS:
        for n in SIZES:
            for o2 in ((True, True, False) if _packable(n, n_cu) else (bool(i & 1), not (i & 1))):
                c, k = next(cyc)
                out.append(make_case(n, n_cu, c, k, o2, rng, pad_notes=bool(i % 3 == 0)))
                i += 1
    for n, n_cu, c, k, o2 in (
            (1024, 256, "uniform", "max_groups", False), (1025, 256, "uniform", "max_groups", True), (4096, 1024, "tail", "max_groups", False),
            (2049, 304, "two", "max_groups", True), (2047, 256, "ends", "max_groups", True),
            (1025, 256, "uniform", "nine", True), (2049, 256, "tail", "one_key", True), (3073, 256, "uniform", "distinct", True), (600, 128, "ends", "nine", True),
            (257, 64, "uniform", "one_key", True), (1100, 100, "two", "one_key", True), (4095, 256, "equal", "distinct", True),
            (1000, 256, "uniform", "mixed", False), (1024, 256, "tail", "mixed", True), (1048, 256, "uniform", "mixed", True), (1100, 128, "two", "mixed", True),
            (513, 256, "distinct", "four", False), (513, 128, "distinct", "mixed", True), (1024, 256, "equal", "high_bits", False), (3071, 256, "ends", "high_bits", True),
            (9, 256, "distinct", "nine", False), (8, 256, "distinct", "one_key", False), (512, 1024, "uniform", "distinct", False), (513, 1024, "uniform", "distinct", True)):
        out.append(make_case(n, n_cu, c, k, o2, rng))
    _cases = out
    return out


# ---- what the header promises -----------------------------------------------------------------------------------------------------------
def keys_of(case, first):
    """the place key of workgroup ids 0 .. first - 1: the previous launch's notes, or the round-3 assumption"""
    if case["place"] is None:
        return np.arange(first, dtype=np.int64) % case["n_cu"]
    return (case["place"][:first].astype(np.int64)) & (PLACE_KEYS - 1)


def expect(case):
    n, n_cu = case["n"], case["n_cu"]
    first = first_round(n, n_cu)
    n_bins = (n // first) * first
    packed = bool(case["order2"] and first == PER_CU * n_cu and n > n_bins and n_bins <= PACK_MAX_ROUNDS * first and n - n_bins <= first and n < 4096)
    per_key = np.bincount(keys_of(case, first), minlength=PLACE_KEYS)
    max_on_key, n_groups = int(per_key.max()), int(np.count_nonzero(per_key))
    over, many = max_on_key > MAX_LEVELS, n_groups > MAX_GROUPS
    return dict(first=first, n_bins=n_bins, packed=packed, pairs=n - n_bins if packed else 0, n_wg=n_bins if packed else n,
                fallback=over or many, over_eight=over, too_many_groups=many, max_on_key=max_on_key, n_groups=n_groups)


def tally(case_list):
    """how many cases take each form -- the GPU test's log, and what both suites require to be there at all"""
    t = dict(cases=len(case_list), deal=0, packed=0, packed_deal=0, packed_fallback=0, fallback_over_eight=0, fallback_too_many_groups=0, eight_on_a_key=0, groups_512=0)
    for c in case_list:
        e = expect(c)
        t["deal"] += not e["fallback"]
        t["packed"] += e["packed"]
        t["packed_deal"] += e["packed"] and not e["fallback"]
        t["packed_fallback"] += e["packed"] and e["fallback"]
        t["fallback_over_eight"] += e["over_eight"]
        t["fallback_too_many_groups"] += e["too_many_groups"] and not e["over_eight"]
        t["eight_on_a_key"] += (not e["fallback"]) and e["max_on_key"] == MAX_LEVELS
        t["groups_512"] += (not e["fallback"]) and e["n_groups"] == MAX_GROUPS
    return {k: int(v) for k, v in t.items()}


# ---- the function, sequentially -----------------------------------------------------------------------------------------------------------
def model(case, rng):
    """balance_order restated: the same steps in the same order, one after the other; wherever the device lets atomics decide (the rank among equal
    counts, a workgroup id's slot on its key, a key's dense group id) the order is drawn from `rng`.  -> the block of ORDER_INTS words."""
    n, n_cu, work = case["n"], case["n_cu"], case["work"].astype(np.int64)
    block = np.full(ORDER_INTS, SENTINEL, np.int64)
    order, order2, seconds = block[:ORDER2_AT], (block[ORDER2_AT:] if case["order2"] else None), block[SECONDS_AT:]
    first = min(n, n_cu * PER_CU)
    first = min(first, MAX_FIRST)
    n_bins = (n // first) * first
    packed = order2 is not None and first == n_cu * PER_CU and n > n_bins and n_bins >= first and n_bins <= PACK_MAX_ROUNDS * first and n - n_bins <= first and n < 4096
    n_pairs = n - n_bins if packed else 0
    n_singles = n_bins - n_pairs
    by_rank = np.lexsort((rng.permutation(n), -work))      # the alignment of rank r: heaviest first, ties in any order
    sorted_ = np.zeros(first, np.int64)
    sw = np.zeros(first, np.int64)
    if packed:
        for r in range(n):
            a = by_rank[r]; w = work[a]
            if r < n_singles:
                item = n_pairs + r
                if item < first:
                    sorted_[item] = a; sw[item] = w + PACK_CONST
                else:
                    order[item] = a
            elif r < n_bins:
                sorted_[r - n_singles] = a; sw[r - n_singles] = w + PACK_CONST
            else:
                seconds[n - 1 - r] = a | (w << 16)
        for j in range(n_pairs):
            sw[j] += (seconds[j] >> 16) + PACK_CONST
        order2[first:n_bins] = -1
    else:
        sorted_[:] = by_rank[:first]; sw[:] = work[sorted_]
        order[first:n] = by_rank[first:]
    keys = keys_of(case, first)
    members, slot, bad = {}, np.zeros(first, np.int64), False
    for b in rng.permutation(first):
        slot[b] = members.get(keys[b], 0)
        members[keys[b]] = slot[b] + 1
        bad = bad or slot[b] >= MAX_LEVELS
    gid, gsize = {}, []
    if not bad:
        distinct = list(members)
        for i in rng.permutation(len(distinct)):
            gid[distinct[i]] = len(gsize); gsize.append(members[distinct[i]])
    G = len(gsize)
    if bad or G > MAX_GROUPS:
        order[:first] = sorted_
        if packed:
            order2[:first] = -1
            order2[:n_pairs] = seconds[:n_pairs] & 0xFFFF
        return block.astype(np.int32)
    gsize = np.array(gsize, np.int64)
    gload = np.zeros(G, np.int64)
    assign = np.zeros((G, MAX_LEVELS), np.int64)
    base = 0
    for k in range(MAX_LEVELS):
        part = np.flatnonzero(gsize > k)
        m = len(part)
        if m == 0:
            break
        by_load = part[np.argsort(-(gload[part] * MAX_GROUPS + (MAX_GROUPS - 1 - part)), kind="stable")]      # the group that carries most first; ties: the lower id
        for rank, g in enumerate(by_load):
            r = base + (m - 1 - rank)                  # ... takes the lightest of the block
            assign[g, k] = r; gload[g] += sw[r]
        base += m
    for b in range(first):
        item = assign[gid[keys[b]], slot[b]]
        order[b] = sorted_[item]
        if packed:
            order2[b] = (seconds[item] & 0xFFFF) if item < n_pairs else -1
    return block.astype(np.int32)


# ---- the checker ------------------------------------------------------------------------------------------------------------------------
def _non_increasing(v):
    return bool(np.all(v[1:] <= v[:-1]))


def check(case, block):
    """Hold one order block to what lsm2d_k_placement.h promises for this case; raises AssertionError naming the case and the property."""
    e = expect(case)
    n, work = case["n"], case["work"].astype(np.int64)
    first, n_bins, packed, E, n_wg = e["first"], e["n_bins"], e["packed"], e["pairs"], e["n_wg"]

    def fail(k, what):
        raise AssertionError("%s [%s]: check %d: %s" % (case["name"], "packed" if packed else "plain", k, what))

    block = np.asarray(block)
    assert block.shape == (ORDER_INTS,) and block.dtype == np.int32, (block.shape, block.dtype)
    block = block.astype(np.int64)
    # 1. nothing stray
    mine = np.zeros(ORDER_INTS, bool)
    mine[:n_wg] = True
    if packed:
        mine[ORDER2_AT:ORDER2_AT + n_bins] = True
        mine[SECONDS_AT:SECONDS_AT + E] = True
    stray = np.flatnonzero(~mine & (block != SENTINEL))
    if stray.size:
        fail(1, "%d words written outside the case's ranges, the first at %d (= %d)" % (stray.size, stray[0], block[stray[0]]))
    order = block[:n_wg]
    order2 = block[ORDER2_AT:ORDER2_AT + n_bins] if packed else np.zeros(0, np.int64)
    # 2. every alignment exactly once
    ids = np.concatenate([order, order2[order2 >= 0]])
    if ids.size != n or ids.min() < 0 or ids.max() >= n:
        fail(2, "%d entries for %d alignments, values %d .. %d" % (ids.size, n, ids.min(), ids.max()))
    times = np.bincount(ids, minlength=n)
    if np.any(times != 1):
        a = int(np.flatnonzero(times != 1)[0])
        fail(2, "alignment %d is run %d times (%d alignments not exactly once)" % (a, times[a], np.count_nonzero(times != 1)))
    w1 = work[order]                                   # workgroup b's (first) alignment's count
    if not packed:
        # 3. beyond the first round: the heaviest go first, and nothing there is heavier than anything in the first round
        tail = w1[first:]
        if not _non_increasing(tail):
            fail(3, "counts beyond the first round rise at rank %d" % (first + 1 + int(np.flatnonzero(tail[1:] > tail[:-1])[0])))
        if tail.size and tail.max() > w1[:first].min():
            fail(3, "a count of %d beyond the first round, %d within it" % (tail.max(), w1[:first].min()))
    else:
        # 4. the pairs
        has2 = order2 >= 0
        if np.any(has2[first:]):
            fail(4, "workgroup %d, beyond the first round, has a second alignment" % (first + int(np.flatnonzero(has2[first:])[0])))
        if np.count_nonzero(has2) != E:
            fail(4, "%d workgroups with a second alignment, %d expected" % (np.count_nonzero(has2), E))
        if np.any(order2[~has2] != -1):
            fail(4, "order2[%d] = %d: neither an alignment nor -1" % (int(np.flatnonzero(~has2 & (order2 != -1))[0]), order2[~has2 & (order2 != -1)][0]))
        asc = np.sort(work)
        fw, sw = w1[has2], work[order2[has2]]
        if not np.array_equal(np.sort(np.concatenate([fw, sw])), asc[:2 * E]):
            fail(4, "the paired alignments do not carry the %d smallest counts" % (2 * E))
        if np.any(fw < sw):
            fail(4, "a pair's first alignment (%d) is lighter than its second (%d)" % (fw[fw < sw][0], sw[fw < sw][0]))
        got = np.stack([fw, sw], 1); got = got[np.lexsort((got[:, 1], got[:, 0]))]
        want = np.stack([asc[E:2 * E][::-1], asc[:E]], 1); want = want[np.lexsort((want[:, 1], want[:, 0]))]
        if not np.array_equal(got, want):
            fail(4, "the pairs are not heaviest-of-the-light with lightest: first difference got %s, want %s" % (got[np.any(got != want, 1)][0], want[np.any(got != want, 1)][0]))
        tail, singles = w1[first:], w1[:first][~has2[:first]]
        if not _non_increasing(tail):
            fail(4, "the singles beyond the first round rise at workgroup %d" % (first + 1 + int(np.flatnonzero(tail[1:] > tail[:-1])[0])))
        if tail.size and singles.size and tail.max() > singles.min():
            fail(4, "a single of %d beyond the first round, one of %d within it" % (tail.max(), singles.min()))
    if e["fallback"]:
        # 6. notes the deal cannot use: the plain heaviest-first order
        if not packed:
            if not _non_increasing(w1[:first]):
                fail(6, "fallback: the first round's counts rise at rank %d" % (1 + int(np.flatnonzero(w1[1:first] > w1[:first - 1])[0])))
        else:
            if not np.array_equal(order2 >= 0, np.arange(n_bins) < E):
                fail(6, "fallback: the pairs are not workgroups 0 .. %d" % (E - 1))
            if not _non_increasing(w1[:E]) or not _non_increasing(-work[order2[:E]]) or not _non_increasing(w1[E:]):
                fail(6, "fallback: firsts non-increasing %s, seconds non-decreasing %s, singles non-increasing %s" % (_non_increasing(w1[:E]), _non_increasing(-work[order2[:E]]), _non_increasing(w1[E:])))
    elif not packed:
        # 5. the deal: level k = the k-th heaviest of every group = the next block of the first round's counts; within a level the group that carries more holds no more
        keys, c = keys_of(case, first), w1[:first]
        by = np.lexsort((-c, keys))
        ks, cs = keys[by], c[by]
        start = np.r_[True, ks[1:] != ks[:-1]]
        g = np.cumsum(start) - 1
        level = np.arange(first) - np.flatnonzero(start)[g]
        csum = np.cumsum(cs) - cs
        before = csum - csum[np.flatnonzero(start)][g]      # the group's sum over the levels above this one
        desc = np.sort(c)[::-1]
        base = 0
        for k in range(int(level.max()) + 1):
            at = level == k
            m = int(np.count_nonzero(at))
            if not np.array_equal(np.sort(cs[at])[::-1], desc[base:base + m]):
                fail(5, "level %d (%d groups) does not hold the first round's counts of ranks %d .. %d" % (k, m, base, base + m - 1))
            s, v = before[at], cs[at]
            wrong = (s[:, None] > s[None, :]) & (v[:, None] > v[None, :])
            if np.any(wrong):
                i, j = np.argwhere(wrong)[0]
                fail(5, "level %d: a group carrying %d holds a count of %d, one carrying %d a count of %d" % (k, s[i], v[i], s[j], v[j]))
            base += m
        sizes = np.bincount(g)
        if np.all(sizes == sizes[0]):
            sums = np.bincount(g, weights=cs)
            if sums.max() - sums.min() > c.max() - c.min():
                fail(5, "groups of %d: sums %d .. %d, further apart than the counts %d .. %d" % (sizes[0], sums.min(), sums.max(), c.min(), c.max()))


# ---- the driver and its files -------------------------------------------------------------------------------------------------------------
def driver_command(exe):
    """tests/cpp/placement_deal_driver.hip with the library's own flags (a program, no shared object)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    flags = [f for f in build.HIPCC_FLAGS if f not in ("-fPIC", "-shared")]
    return [build.hipcc(), *flags, "-I" + os.path.join(root, "include"), "-I" + os.path.join(root, "srrg2_laser_slam_2d_amd", "csrc"), "-o", exe,
            os.path.join(root, "tests", "cpp", "placement_deal_driver.hip")]


def write_cases(path, case_list):
    with open(path, "wb") as f:
        f.write(MAGIC + np.array([len(case_list)], "<i4").tobytes())
        for c in case_list:
            first = first_round(c["n"], c["n_cu"])
            assert 1 <= c["n"] <= 4096 and c["n_cu"] >= 1 and c["work"].shape == (c["n"],) and c["work"].min() >= 0 and c["work"].max() <= ALIGN_BLOCK, c["name"]
            assert c["place"] is None or first <= c["place"].size <= MAX_FIRST, c["name"]
            f.write(np.array([c["n"], c["n_cu"], 0 if c["place"] is None else c["place"].size, int(c["order2"])], "<i4").tobytes())
            f.write(c["work"].astype("<i4").tobytes())
            if c["place"] is not None:
                f.write(c["place"].astype("<i4").tobytes())


def read_blocks(path, n_cases):
    blocks = np.fromfile(path, "<i4")
    assert blocks.size == n_cases * ORDER_INTS, (blocks.size, n_cases)
    return blocks.reshape(n_cases, ORDER_INTS).astype(np.int32)
