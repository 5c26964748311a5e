#!/usr/bin/env python3
"""Compare two ISA dumps of the library (tools/isa_dump.sh -> lsm2d.s), function by function, on the INSTRUCTIONS alone.

    OUT=/tmp/isa_parent bash <parent checkout>/tools/isa_dump.sh && OUT=/tmp/isa_tree bash tools/isa_dump.sh
    python3 tools/isa_diff.py /tmp/isa_parent/lsm2d.s /tmp/isa_tree/lsm2d.s

A function's text is everything between its `; -- Begin function` and `; -- End function` lines.  Of every line only what stands in front of the first `;`
counts, and lines that are then empty are dropped: the compiler's comments name basic blocks (`; %.lr.ph1050.i`) by numbers that move with any edit to the
source, and the raw text of a kernel then differs although no instruction of it does.  Labels, directives and the .amdhsa block stay in the comparison.
Each function on both sides falls into one class:

    identical   the same lines in the same order
    reordered   the same multiset of lines in another order
    different   anything else

For the last two, both sides' register, scratch and LDS budgets are printed.  Exit status 0 only if every function is identical and none is missing on
either side."""
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


def instructions(text):
    """a function's lines without comments (everything from the first `;` on) and without the lines that leaves empty"""
    kept = (line.split(";", 1)[0].rstrip() for line in text.splitlines())
    return [line for line in kept if line.strip()]


def classify(a, b):
    ia, ib = instructions(a), instructions(b)
    if ia == ib:
        return "identical"
    return "reordered" if collections.Counter(ia) == collections.Counter(ib) else "different"


def resources(text):
    def value(key):
        m = re.search(r"\.amdhsa_" + key + r"\s+(\S+)", text)
        return m.group(1) if m else "?"
    return " ".join("%s %s" % (k, value(k)) for k in RESOURCES)


def compare(a, b, out=None):
    """a, b: {name: text}.  Prints the report (to `out`, or standard output); returns the exit status."""
    out = out or sys.stdout
    both = [n for n in a if n in b]
    cls = {n: classify(a[n], b[n]) for n in both}
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
            ia, ib = instructions(a[n]), instructions(b[n])
            kept = sum(m.size for m in difflib.SequenceMatcher(None, ia, ib, autojunk=False).get_matching_blocks())      # lines both sides have in the same order
            print("%-10s: %s (%d lines against %d; %d and %d of them outside the common order)" % (kind, n, len(ia), len(ib), len(ia) - kept, len(ib) - kept), file=out)
            print("            left : %s" % resources(a[n]), file=out)
            print("            right: %s" % resources(b[n]), file=out)
    for n in sorted(both):
        if cls[n] == "identical":
            print("identical : %s" % n, file=out)
    return 0 if count["identical"] == len(a) == len(b) else 1


def main(argv):
    if len(argv) != 3:
        print(__doc__, file=sys.stderr)
        return 2
    with open(argv[1], errors="replace") as fa, open(argv[2], errors="replace") as fb:
        a, b = functions(fa), functions(fb)
    return compare(a, b)


if __name__ == "__main__":
    sys.exit(main(sys.argv))
