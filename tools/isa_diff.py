#!/usr/bin/env python3
"""Compare two ISA dumps of the library (tools/isa_dump.sh -> lsm2d.s), function by function, on the INSTRUCTIONS alone.

    OUT=/tmp/isa_parent bash <parent checkout>/tools/isa_dump.sh && OUT=/tmp/isa_tree bash tools/isa_dump.sh
    python3 tools/isa_diff.py [--rename OLD=NEW]... /tmp/isa_parent/lsm2d.s /tmp/isa_tree/lsm2d.s

A function's text is everything between its `; -- Begin function` and `; -- End function` lines.  Of every line only what stands in front of the first `;`
counts, and lines that are then empty are dropped: the compiler's comments name basic blocks (`; %.lr.ph1050.i`) by numbers that move with any edit to the
source, and the raw text of a kernel then differs although no instruction of it does.

A function is compared independent of its PLACE in the code object and of its LINKAGE, neither of which is an instruction:

    place     the compiler numbers a function's local labels by the function's ordinal in the code object (.LBB<f>_<n>, .Lfunc_end<f>, .Lfunc_begin<f>,
              .LJTI<f>_<n>, .LCPI<f>_<n>), so a kernel added, removed or moved in front of it renames every one of them.  The ordinal <f> is stripped
              (.LBB_<n>, .Lfunc_end); the _<n> part stays.  Nothing is lost: a function's labels are referenced only inside it.  A function whose lines carry
              two different ordinals for one kind of label is not what the compiler writes; its text is left as it is, and it fails honestly.
    name      every occurrence of the function's own mangled name in its text (.amdhsa_kernel, .size, ...) is replaced by a placeholder, so a function whose
              name changed (--rename OLD=NEW, repeatable; reported under NEW) compares on what it does.  Callees' names stay.
    linkage   lines that switch the section (.section ..., a bare .text) are dropped: they say comdat for a template's instantiation and .text for a plain
              kernel.

Everything else stays in the comparison: every instruction and operand, the _<n> part of every label, the other directives and the .amdhsa block.
Each function on both sides falls into one class:

    identical   the same lines in the same order
    reordered   the same multiset of lines in another order
    different   anything else

For the last two, both sides' register, scratch and LDS budgets are printed.  Exit status 0 only if every function is identical and none is missing on
either side; 2 for a wrong command line, which includes a --rename whose OLD is not on the left or whose NEW is not on the right."""
import collections
import difflib
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def functions(lines):
    """{name: raw text} of an assembly listing, given as an iterable of lines"""
    out, name, buf = {}, None, []
    for line in lines:
        m = re.search(r"; -- Begin function (\S+)", line)
        if m:
            name, buf = m.group(1), []
        elif "; -- End function" in line and name:
            out[name] = "".join(buf)
            name = None
        elif name:
            buf.append(line if line.endswith("\n") else line + "\n")
    return out


LOCAL_LABEL = re.compile(r"\.L(BB|func_end|func_begin|JTI|CPI)(\d+)")
SECTION_SWITCH = re.compile(r"\s*\.(section\s.*|text)$")
OWN_NAME = "<this function>"


def instructions(text, name=None):
    """a function's lines without comments (everything from the first `;` on), without the lines that leaves empty and without section switches; the
    function's ordinal stripped from its local labels, and its own name `name` (if given) replaced by a placeholder"""
    kept = (line.split(";", 1)[0].rstrip() for line in text.splitlines())
    kept = [line for line in kept if line.strip() and not SECTION_SWITCH.match(line)]
    ordinals = collections.defaultdict(set)
    for line in kept:
        for kind, f in LOCAL_LABEL.findall(line):
            ordinals[kind].add(f)
    if all(len(fs) == 1 for fs in ordinals.values()):
        kept = [LOCAL_LABEL.sub(r".L\1", line) for line in kept]
    if name:
        own = re.compile(r"(?<![\w$.])" + re.escape(name) + r"(?![\w$])")
        kept = [own.sub(OWN_NAME, line) for line in kept]
    return kept


def classify(a, b, name_a=None, name_b=None):
    ia, ib = instructions(a, name_a), instructions(b, name_b)
    if ia == ib:
        return "identical"
    return "reordered" if collections.Counter(ia) == collections.Counter(ib) else "different"


def resources(text):
    def value(key):
        m = re.search(r"\.amdhsa_" + key + r"\s+(\S+)", text)
        return m.group(1) if m else "?"
    return " ".join("%s %s" % (k, value(k)) for k in RESOURCES)


def compare(a, b, out=None, renames=()):
    """a, b: {name: text}; renames: (old, new) pairs of functions whose name changed from a to b.  Prints the report (to `out`, or standard output); returns
    the exit status."""
    out = out or sys.stdout
    for old, new in renames:
        if old not in a or new not in b:
            print("--rename %s=%s: no function %s on the %s" % ((old, new, old, "left") if old not in a else (old, new, new, "right")), file=sys.stderr)
            return 2
    new_name = dict(renames)
    left = {new_name.get(n, n): n for n in a}      # the name a left function is compared and reported under -> the name its own text calls it by
    a = {n: a[left[n]] for n in left}
    both = [n for n in a if n in b]
    cls = {n: classify(a[n], b[n], left[n], n) for n in both}
    count = collections.Counter(cls.values())
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    print("%d functions on the left, %d on the right; %d identical, %d reordered, %d different, %d on one side only"
          % (len(a), len(b), count["identical"], count["reordered"], count["different"], len(only_a) + len(only_b)), file=out)
    for n in only_a:
        print("only left : %s" % n, file=out)
    for n in only_b:
        print("only right: %s" % n, file=out)
    for kind in ("different", "reordered"):
        for n in sorted(both):
            if cls[n] != kind:
                continue
            ia, ib = instructions(a[n], left[n]), instructions(b[n], n)
            kept = sum(m.size for m in difflib.SequenceMatcher(None, ia, ib, autojunk=False).get_matching_blocks())      # lines both sides have in the same order
            print("%-10s: %s (%d lines against %d; %d and %d of them outside the common order)" % (kind, n, len(ia), len(ib), len(ia) - kept, len(ib) - kept), file=out)
            print("            left : %s" % resources(a[n]), file=out)
            print("            right: %s" % resources(b[n]), file=out)
    for n in sorted(both):
        if cls[n] == "identical":
            print("identical : %s%s" % (n, " (was %s)" % left[n] if left[n] != n else ""), file=out)
    return 0 if count["identical"] == len(a) == len(b) else 1


def main(argv):
    args, renames = argv[1:], []
    while len(args) >= 2 and args[0] == "--rename" and "=" in args[1]:
        renames.append(tuple(args[1].split("=", 1)))
        args = args[2:]
    if len(args) != 2 or args[0].startswith("--"):
        print(__doc__, file=sys.stderr)
        return 2
    with open(args[0], errors="replace") as fa, open(args[1], errors="replace") as fb:
        a, b = functions(fa), functions(fb)
    return compare(a, b, renames=renames)

if __name__ == "__main__":
    sys.exit(main(sys.argv))
