"""The aligner's launch forms (wide k_align / k_align_seq, narrow k_align_narrow<256>, packed k_align_two / k_align_seq_two) against the oracle on MIXED
batches (tests/mixed_batches.py): converging, slow, light, failing, early-stopping and not-a-number alignments side by side -- in a packed workgroup the
lightest alignments, i.e. the failing ones, run two to a workgroup, one after the other, and the second must not see anything of the first.

Every case: the automatic call takes the intended form; forced widths, culling and balancing off, a permuted batch, a prepared batch run three times,
asynchronous begin / wait alone and beside a second batch all give its bits; and its alignments equal the fp32 oracle bit for bit (the device-order
oracle in the tree order, the sequential one with "sum_order" 1)."""
import collections
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import mixed_batches as mb
from gpu_helpers import _assert_bitwise_equal_to_device_order_oracle, assert_same_bits, result_bits
from srrg2_laser_slam_2d_amd import api

pytestmark = pytest.mark.gpu

SEED = 2024
# (sum_order, n, setting, the form the automatic call takes: last_align_width)
CASES = [(0, n, s, w) for n, w in ((300, 512), (1025, 1024), (1040, 1024), (1100, 256), (1537, 1024), (2049, 1024), (3073, 1024)) for s in ("S1", "S2")]
CASES += [(0, 1040, "S3", 1024), (0, 1537, "S3", 1024)]      # (two slices: the canvases' LDS leaves room for five narrow workgroups per CU -- 1280 -- so 1537 packs)
CASES += [(1, n, s, 1024) for n in (1040, 1537, 2049) for s in ("S1", "S3")]      # (no narrow form in the reference's order: packed up to 1600, and 2049)
_ORACLE = {}      # (sum_order, setting, i) -> result: alignment i is the same in every batch size of a setting (mixed_batches: a batch is a prefix of a larger one)


def _run(ctx, al, spec, x0=None, want_pairs=False, **opts):
    fixed = spec["_fixed"]
    for k, v in opts.items():
        ctx.set_option(k, v)
    try:
        r = al.compute_batch(fixed, [spec["_moving"]] * spec["ns"], spec["x0"] if x0 is None else x0, priors=spec["priors"], fixed_index=spec["fixed_index"],
                             want_stats=True, want_pairs=want_pairs)
        return r, ctx.get_option("last_align_path"), ctx.get_option("last_align_width")
    finally:
        for k in opts:
            ctx.set_option(k, 1 if k in ("cull", "balance") else 0)


@pytest.mark.parametrize("sum_order,n,setting,form", CASES)
def test_launch_forms_on_mixed_batches(ctx, po, sum_order, n, setting, form):
    t0 = time.time()
    spec = mb.batch(SEED, n, setting)
    kinds = spec["kinds"]
    spec["_fixed"] = [api.CloudSet(ctx, sl["pts"], sl["offs"]) for sl in spec["slices"]]
    spec["_moving"] = api.CloudSet(ctx, spec["map"])
    al = mb.aligner(ctx, spec)
    ctx.set_option("sum_order", sum_order)
    try:
        ref, path, width = _run(ctx, al, spec)
        assert path == 1, (n, setting, path)      # (first: last_align_width is not updated by split or latency-kernel launches)
        assert width == form, (n, setting, sum_order, width, form)
        want = result_bits(ref)
        # ---- the variants: every one must give the automatic call's bits, every alignment
        widths = [512, 256] + ([1024] if n > 1024 and n % 1024 else [])
        for w in widths:
            r, path, got_w = _run(ctx, al, spec, align_width=w)
            assert path == 1 and got_w == (512 if (sum_order and w == 256) else w), (n, setting, sum_order, w, got_w)      # (no narrow reference-order kernel: 256 launches 512)
            assert_same_bits(result_bits(r), want, labels=kinds, tag=("align_width", w))
        r, _, _ = _run(ctx, al, spec, cull=0, balance=0)
        assert_same_bits(result_bits(r), want, labels=kinds, tag="cull 0, balance 0")
        perm = np.random.default_rng(n).permutation(n)
        sp = dict(spec, x0=spec["x0"][perm], fixed_index=np.ascontiguousarray(spec["fixed_index"][:, perm]),
                  priors=None if spec["priors"] is None else [spec["priors"][j] for j in perm])
        r, _, _ = _run(ctx, al, sp)
        assert_same_bits(result_bits(r, np.argsort(perm)), want, labels=kinds, tag="permuted")
        args = (spec["_fixed"], [spec["_moving"]] * spec["ns"], spec["x0"])
        kw = dict(priors=spec["priors"], fixed_index=spec["fixed_index"], want_stats=True)
        prep = al.prepare_batch(*args, **kw)
        for k in range(3):      # the third run: the kept placement (no estimate) where the library keeps one
            assert_same_bits(result_bits(prep.run(copy=True)), want, labels=kinds, tag=("prepared", k))
        if n <= 1024 or (form == 1024 and n < 2048):
            assert ctx.get_option("last_cull_estimate") == 0, (n, setting)
        prep.begin(); assert_same_bits(result_bits(prep.wait(copy=True)), want, labels=kinds, tag="begin / wait")
        prep2 = al.prepare_batch(spec["_fixed"], [spec["_moving"]] * spec["ns"], sp["x0"], priors=sp["priors"], fixed_index=sp["fixed_index"], want_stats=True)
        prep.begin(); prep2.begin()
        a, b = prep.wait(copy=True), prep2.wait(copy=True)
        assert_same_bits(result_bits(a), want, labels=kinds, tag="begin / wait beside a second batch")
        assert_same_bits(result_bits(b, np.argsort(perm)), want, labels=kinds, tag="the second batch in flight (permuted)")
        # ---- not-a-number starts: a failure status, and the alignments beside them as in the same batch with finite starts there instead
        bad = np.isin(kinds, mb.NON_FINITE)
        assert bad.any() and np.all(ref.status[bad] != 0), ref.status[bad]
        x_fin = spec["x0"].copy(); x_fin[bad] = spec["x0"][np.flatnonzero(kinds == "far")[0]]
        r, _, _ = _run(ctx, al, spec, x0=x_fin)
        assert_same_bits(result_bits(r, np.flatnonzero(~bad)), result_bits(ref, np.flatnonzero(~bad)), labels=kinds[~bad], tag="finite starts in place of the non-finite ones")
        pairs = None
        if setting == "S1" and n == 1040 and not sum_order:
            pairs, _, _ = _run(ctx, al, spec, want_pairs=True)
            assert_same_bits(result_bits(pairs), want, labels=kinds, tag="want_pairs")
    finally:
        ctx.set_option("sum_order", 0)
    # ---- against the oracle: every alignment up to 1100; above, every light or failing one (those are paired) and a stride sample of the others
    finite = np.flatnonzero(~bad)
    if n <= 1100:
        check = finite
    else:
        heavy = np.isin(kinds, ("converge", "slow"))
        check = np.union1d(finite[~heavy[finite]], finite[heavy[finite]][:: max(1, int(heavy.sum()) // 200)])
    todo = [int(i) for i in check if (sum_order, setting, int(i)) not in _ORACLE]
    with ThreadPoolExecutor(16) as ex:
        for i, r in zip(todo, ex.map(lambda i: mb.oracle_align(po, spec, i, device_order=not sum_order), todo)):
            _ORACLE[(sum_order, setting, i)] = r
    for i in check:
        _assert_bitwise_equal_to_device_order_oracle(ref, int(i), _ORACLE[(sum_order, setting, int(i))], (setting, n, sum_order, int(i), kinds[i]))
    if pairs is not None:
        for i in check:
            w_ = mb.oracle_align(po, spec, int(i), device_order=True, want_pairs=True)
            assert np.array_equal(pairs.pairs[i][0], w_["pairs"][0]), ("pairs", int(i), kinds[i])
    hist = collections.Counter(ref.status.tolist())
    assert hist[0] and hist[1] and hist[2], hist
    print("launch forms: sum_order %d, n %d, %s: form %d; statuses %s; iteration counts %s; %d of %d alignments checked against the oracle (%d light or failing)%s; %.1f s"
          % (sum_order, n, setting, form, dict(sorted(hist.items())), sorted(set(ref.iterations.tolist())), len(check), n,
             int(np.sum(~np.isin(kinds[check], ("converge", "slow")))), ", pairs too" if pairs is not None else "", time.time() - t0))
