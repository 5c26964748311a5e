"""tools/isa_diff.py: the classifier that a "no instruction changed" refactor is held to.  Hand-written function texts, no compiler, no GPU."""
import importlib.util
import io
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def isa_diff():
    spec = importlib.util.spec_from_file_location("isa_diff", os.path.join(ROOT, "tools", "isa_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def listing(*functions):
    """an assembly file of (name, body) functions, framed the way the compiler frames them"""
    out = ["\t.text\n"]
    for name, body in functions:
        out.append("\t.globl\t%s ; -- Begin function %s\n%s:\n%s\t.end_amdhsa_kernel\n\t; -- End function\n" % (name, name, name, body))
    return "".join(out)


HEAD = "\t.amdhsa_kernel k\n\t\t.amdhsa_group_segment_fixed_size 1024\n\t\t.amdhsa_private_segment_fixed_size 0\n\t\t.amdhsa_next_free_vgpr 64\n\t\t.amdhsa_next_free_sgpr 40\n"
BASE = ("; %bb.0:\n"
        "\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n"
        "\tv_lshlrev_b32_e32 v1, 2, v0 ; scale the index\n"
        "\n"
        ".LBB0_1: ; %.lr.ph1050.i\n"
        "\tv_add_f32_e32 v2, v2, v3\n"
        "\tv_mul_f32_e32 v4, v2, v5\n"
        "\ts_cbranch_scc1 .LBB0_1\n"
        "; %bb.2: ; %._crit_edge\n"
        "\ts_endpgm\n") + HEAD
# the same instructions; the basic blocks' comments renumbered, a blank line gone, a comment line added
RENUMBERED = ("; %bb.0: ; %entry\n"
              "\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n"
              "\tv_lshlrev_b32_e32 v1, 2, v0\n"
              ".LBB0_1: ; %.lr.ph1062.i\n"
              "\t; implicit-def: $vgpr7\n"
              "\tv_add_f32_e32 v2, v2, v3\n"
              "\tv_mul_f32_e32 v4, v2, v5\n"
              "\ts_cbranch_scc1 .LBB0_1\n"
              "; %bb.3: ; %._crit_edge\n"
              "\ts_endpgm\n") + HEAD
SWAPPED = BASE.replace("\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n\tv_lshlrev_b32_e32 v1, 2, v0 ; scale the index\n",
                       "\tv_lshlrev_b32_e32 v1, 2, v0 ; scale the index\n\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n")
OPERAND = BASE.replace("v_mul_f32_e32 v4, v2, v5", "v_mul_f32_e32 v4, v2, v6").replace("next_free_vgpr 64", "next_free_vgpr 72")


def test_texts_are_what_they_claim():
    assert SWAPPED != BASE and OPERAND != BASE and RENUMBERED != BASE


def test_classes(isa_diff):
    assert isa_diff.classify(BASE, BASE) == "identical"
    assert isa_diff.classify(BASE, RENUMBERED) == "identical"      # only comments and blank lines differ
    assert isa_diff.classify(BASE, SWAPPED) == "reordered"
    assert isa_diff.classify(BASE, OPERAND) == "different"
    assert isa_diff.classify(BASE, BASE + "\ts_nop 0\n") == "different"      # one instruction more


def test_comments_do_not_hide_a_changed_instruction(isa_diff):
    assert isa_diff.classify(RENUMBERED, RENUMBERED.replace("v_add_f32_e32 v2, v2, v3", "v_add_f32_e32 v2, v2, v4")) == "different"


def run(isa_diff, tmp_path, left, right):
    a, b = tmp_path / "a.s", tmp_path / "b.s"
    a.write_text(left)
    b.write_text(right)
    return isa_diff.main(["isa_diff.py", str(a), str(b)])


def test_exit_status_and_report(isa_diff, tmp_path, capsys):
    assert run(isa_diff, tmp_path, listing(("k0", BASE), ("k1", BASE)), listing(("k0", RENUMBERED), ("k1", BASE))) == 0
    out = capsys.readouterr().out
    assert "2 identical, 0 reordered, 0 different, 0 on one side only" in out

    assert run(isa_diff, tmp_path, listing(("k0", BASE), ("k1", BASE)), listing(("k0", SWAPPED), ("k1", BASE))) == 1
    out = capsys.readouterr().out
    assert "1 identical, 1 reordered, 0 different" in out and "reordered : k0" in out and "identical : k1" in out
    assert out.count("next_free_vgpr 64 next_free_sgpr 40 private_segment_fixed_size 0 group_segment_fixed_size 1024") == 2      # both sides' budgets

    assert run(isa_diff, tmp_path, listing(("k0", BASE)), listing(("k0", OPERAND))) == 1
    out = capsys.readouterr().out
    assert "different : k0" in out and "next_free_vgpr 64 " in out and "next_free_vgpr 72 " in out


def test_a_function_on_one_side_only_fails(isa_diff, tmp_path, capsys):
    assert run(isa_diff, tmp_path, listing(("k0", BASE), ("k1", BASE)), listing(("k0", BASE))) == 1
    assert "only left : k1" in capsys.readouterr().out
    assert run(isa_diff, tmp_path, listing(("k0", BASE)), listing(("k0", BASE), ("k2", BASE))) == 1
    assert "only right: k2" in capsys.readouterr().out


def test_compare_takes_dictionaries(isa_diff):
    buf = io.StringIO()
    assert isa_diff.compare({"k": BASE}, {"k": RENUMBERED}, out=buf) == 0
    assert isa_diff.compare({"k": BASE}, {"k": SWAPPED}, out=buf) == 1
