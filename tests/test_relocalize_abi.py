"""CPU checks of lsm2d_relocalize_select (ABI 0.7.9): the symbol is declared by include/lsm2d.h, bound by the Python mirror with the right argument count and
exported by the gfx950 build; the two new kernels are in the library's code object; the Python and C++ mirrors exist and the C++ sources compile; and -- on
the CPU oracle, no GPU -- the workload and the thresholds the GPU tests use are such that those tests cannot pass vacuously (relocalize_cases)."""
import dataclasses

import numpy as np
import pytest

import abi_checks
import align_select_cases as ac
import cpp_build
import relocalize_cases as rc


def test_symbol_declared_bound_and_exported():
    abi_checks.assert_declared_bound_exported("lsm2d_relocalize_select", 19)
    header = abi_checks.header()
    assert "MULTI.json:749-769, :964-986" in header and "0.7.9" in header


def test_kernels_are_in_the_code_object():
    abi_checks.assert_kernels_in_code_object((b"k_reloc_items", b"k_align_rows_liveINS_8AlignRow"))


def test_mirrors_exist():
    from srrg2_laser_slam_2d_amd import api
    abi_checks.assert_mirrors_have(("relocalize_select", "relocalize"), ("relocalizeSelect(", "lsm2d_relocalize_select(", '#include "lsm2d.hpp"'), "lsm2d_relocalize.hpp")
    fields = [f.name for f in dataclasses.fields(api.RelocalizeSelectResult)]
    assert fields[:10] == ["scored_index", "scored_stats", "n_scored_accepted", "index", "pose", "information", "iterations", "last_stats", "n_accepted", "n_success"]


@pytest.mark.parametrize("source", ["relocalize_select_driver.cpp", "relocalize_bench.cpp"])
def test_cpp_sources_compile(source):
    r = cpp_build.syntax_only(source)
    assert r.returncode == 0, r.stderr[-3000:]


# ---- the GPU tests' workload and thresholds, on the oracle ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stages(po):
    c = rc.make_cases()
    rows1, active, M, full = rc.oracle_stages(po, c)
    return c, rows1, active, full, rc.threshold_cases(rows1, active, full)


def test_workload_cannot_pass_vacuously(stages):
    from srrg2_laser_slam_2d_amd import api
    c, rows1, active, full, tc = stages
    n = len(c.poses)
    assert active[1] == 0 and full.status[1] == 1 and int(active.sum()) == n - 1      # the pose that finds nothing
    seen = {}
    for name, (s1, k_score, s2) in tc.items():
        r = rc.restate(rows1, active, full, s1, k_score, s2, 1024)
        m = len(r.scored_index)
        sub_ok = full.status[r.scored_index] == 0
        print(name, "k_score", k_score, "scored accepted", r.n_scored_accepted, "m", m, "success", r.n_success, "accepted", r.n_accepted)
        seen[name] = (m, r)
        assert r.n_success == int(sub_ok.sum()) and r.n_accepted <= r.n_success <= m
    m, r = seen["some"]
    assert 0 < m < tc["some"][1] and m == r.n_scored_accepted                        # 0 < m < k_score
    assert 0 < r.n_accepted < m                                                      # beside a hypothesis the verdict accepts, one it rejects after alignment
    m, r = seen["cut"]
    assert m == tc["cut"][1] < r.n_scored_accepted                                   # m = k_score < accepted
    assert seen["none"][0] == 0 and seen["none"][1].n_accepted == 0 and seen["none"][1].n_success == 0      # m = 0
    m, r = seen["all"]
    assert m == n - 1 and 0 < r.n_accepted < m
    for a, b in ac.DUPLICATES:                                                       # a duplicate pair inside the selection: adjacent, the lower index first
        si = r.scored_index.tolist()
        assert a in si and b in si and si.index(a) < si.index(b)
        assert rows1[a].tobytes() == rows1[b].tobytes() and full.last()[a].tobytes() == full.last()[b].tobytes()
    dup = {x for pair in ac.DUPLICATES for x in pair}
    assert len(dup & set(r.index.tolist())) >= 2                                     # ... and through the second ranking, where stage-1 rank breaks the tie
    oi = r.index.tolist()
    assert oi.index(8) < oi.index(180) < oi.index(250)
    # a k that cuts the second ranking
    r7 = rc.restate(rows1, active, full, *tc["all"][:2], tc["all"][2], 7)
    assert len(r7.index) == 7 and np.array_equal(r7.index, r.index[:7])
