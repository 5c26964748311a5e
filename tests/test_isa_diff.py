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


def at_ordinal(text, f):
    """`text` (a function at ordinal 0) as the compiler writes it for the f-th function of a code object"""
    return text.replace(".LBB0_", ".LBB%d_" % f).replace(".Lfunc_end0", ".Lfunc_end%d" % f)


def named(name):
    """BASE's instructions and budget as function `name`, with the lines that carry a function's own name"""
    return (BASE.replace(".amdhsa_kernel k\n", ".amdhsa_kernel %s\n" % name)
            + ".Lfunc_end0:\n\t.size\t%s, .Lfunc_end0-%s\n" % (name, name))


# two blocks, so that a branch has two labels to choose from
TWO_BLOCKS = BASE.replace("; %bb.2: ; %._crit_edge\n", ".LBB0_2:\n\tv_mov_b32_e32 v6, 0\n\ts_cbranch_vccnz .LBB0_2\n") + ".Lfunc_end0:\n"
CALLER = BASE.replace("\ts_endpgm\n", "\ts_getpc_b64 s[2:3]\n\ts_add_u32 s2, s2, _ZN1a6calleeEv@rel32@lo+4\n\ts_swappc_b64 s[30:31], s[2:3]\n\ts_endpgm\n")


def test_a_functions_place_in_the_code_object_does_not_count(isa_diff):
    assert ".LBB7_1" in at_ordinal(TWO_BLOCKS, 7) and ".Lfunc_end7" in at_ordinal(TWO_BLOCKS, 7) and ".LBB0_" not in at_ordinal(TWO_BLOCKS, 7)
    assert isa_diff.classify(TWO_BLOCKS, at_ordinal(TWO_BLOCKS, 7)) == "identical"
    assert isa_diff.instructions(TWO_BLOCKS) == isa_diff.instructions(at_ordinal(TWO_BLOCKS, 7))
    assert "\ts_cbranch_scc1 .LBB_1" in isa_diff.instructions(TWO_BLOCKS) and ".Lfunc_end:" in isa_diff.instructions(TWO_BLOCKS)      # the _<n> part stays


def test_a_retargeted_branch_is_a_difference(isa_diff):
    retargeted = TWO_BLOCKS.replace("s_cbranch_scc1 .LBB0_1", "s_cbranch_scc1 .LBB0_2")
    assert retargeted != TWO_BLOCKS and ".LBB0_1:" in retargeted and ".LBB0_2:" in retargeted
    assert isa_diff.classify(TWO_BLOCKS, retargeted) == "different"
    assert isa_diff.classify(at_ordinal(TWO_BLOCKS, 7), retargeted) == "different"


def test_two_ordinals_in_one_function_are_left_alone(isa_diff):
    mixed = TWO_BLOCKS.replace("s_cbranch_vccnz .LBB0_2", "s_cbranch_vccnz .LBB3_2")
    lines = isa_diff.instructions(mixed)
    assert "\ts_cbranch_scc1 .LBB0_1" in lines and "\ts_cbranch_vccnz .LBB3_2" in lines and ".Lfunc_end0:" in lines      # nothing of it rewritten
    assert isa_diff.classify(TWO_BLOCKS, mixed) == "different"
    assert isa_diff.classify(mixed, mixed) == "identical"
    assert isa_diff.classify(mixed, at_ordinal(mixed, 7).replace(".LBB3_", ".LBB9_")) == "different"      # it fails honestly against itself elsewhere


def test_linkage_does_not_count(isa_diff):
    comdat = BASE + "\t.section\t.text.k0,\"axG\",@progbits,k0,comdat\n.Lfunc_end0:\n"
    plain = BASE + "\t.text\n.Lfunc_end0:\n"
    assert isa_diff.classify(comdat, plain) == "identical"
    assert isa_diff.classify(comdat, plain.replace("\t.text\n", "\t.p2align\t8\n")) == "different"      # only section switches are dropped


def test_own_name_is_a_placeholder_and_a_callee_is_not(isa_diff):
    assert named("k_old") != named("k_new") and "\t.size\tk_old, .Lfunc_end0-k_old\n" in named("k_old")
    assert isa_diff.classify(named("k_old"), named("k_new")) == "different"      # unpaired texts differ by the name
    assert isa_diff.classify(named("k_old"), named("k_new"), "k_old", "k_new") == "identical"
    assert isa_diff.classify(named("k_old"), named("k_new").replace("v2, v2, v3", "v2, v2, v4"), "k_old", "k_new") == "different"
    other_callee = CALLER.replace("_ZN1a6calleeEv", "_ZN1a7callee2Ev")
    assert other_callee != CALLER
    assert isa_diff.classify(CALLER, other_callee, "k", "k") == "different"
    assert isa_diff.classify(CALLER, other_callee, "k_old", "k_new") == "different"


def run_renamed(isa_diff, tmp_path, left, right, *renames):
    a, b = tmp_path / "a.s", tmp_path / "b.s"
    a.write_text(left)
    b.write_text(right)
    return isa_diff.main(["isa_diff.py"] + [x for r in renames for x in ("--rename", r)] + [str(a), str(b)])


def test_rename_pairs_a_function_whose_name_changed(isa_diff, tmp_path, capsys):
    left = listing(("k0", BASE), ("k_old", named("k_old")), ("j_old", at_ordinal(named("j_old"), 2)))
    right = listing(("k_new", named("k_new")), ("k0", at_ordinal(BASE, 1)), ("j_new", at_ordinal(named("j_new"), 2)))
    assert run_renamed(isa_diff, tmp_path, left, right) == 1      # unpaired: two functions on each side without a partner
    assert "1 identical, 0 reordered, 0 different, 4 on one side only" in capsys.readouterr().out

    assert run_renamed(isa_diff, tmp_path, left, right, "k_old=k_new", "j_old=j_new") == 0
    out = capsys.readouterr().out
    assert "3 functions on the left, 3 on the right; 3 identical, 0 reordered, 0 different, 0 on one side only" in out
    assert "identical : k_new" in out and "identical : j_new" in out and "identical : k_old" not in out and "only left" not in out and "only right" not in out

    changed = right.replace("v_mul_f32_e32 v4, v2, v5", "v_mul_f32_e32 v4, v2, v6", 1)      # the first function on the right is k_new
    assert run_renamed(isa_diff, tmp_path, left, changed, "k_old=k_new", "j_old=j_new") == 1
    out = capsys.readouterr().out
    assert "2 identical, 0 reordered, 1 different, 0 on one side only" in out and "different : k_new" in out


def test_rename_of_a_missing_function_is_an_error(isa_diff, tmp_path, capsys):
    left, right = listing(("k_old", named("k_old"))), listing(("k_new", named("k_new")))
    assert run_renamed(isa_diff, tmp_path, left, right, "k_gone=k_new") == 2
    assert "k_gone" in capsys.readouterr().err
    assert run_renamed(isa_diff, tmp_path, left, right, "k_old=k_nowhere") == 2
    assert "k_nowhere" in capsys.readouterr().err
    assert run_renamed(isa_diff, tmp_path, left, right, "k_old=k_new") == 0


def test_compare_takes_dictionaries(isa_diff):
    buf = io.StringIO()
    assert isa_diff.compare({"k": BASE}, {"k": RENUMBERED}, out=buf) == 0
    assert isa_diff.compare({"k": BASE}, {"k": SWAPPED}, out=buf) == 1
