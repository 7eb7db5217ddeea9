#!/usr/bin/env python3
"""Instructions per candidate of the minikeys filter (k_mini_filter) from an ISA listing.

The kernel's per-candidate work is its one 58-trip loop (kh_kernels.hip: one row per lane, one trip
per candidate); everything before it -- the lane's digits, message words 0..4, the rounds and schedule
terms that depend on them alone -- runs once per 58 candidates.  The tool finds the function's largest
backward-branch loop and counts its instructions by kind (the rare push of a valid candidate, one trip
in 256, is inside it and counted whole, so the figure is an upper bound by a few instructions).

usage: python tools/minikeys_valu.py LISTING.s   (a listing as tools/isa_bsgs.sh makes it)
"""
import json
import re
import sys

SYMBOL = "_Z13k_mini_filter16mini_filter_args"


def body(text: str) -> list[str]:
    start = text.index("\n" + SYMBOL + ":")
    end = text.index("s_endpgm", start)
    return text[start:end].split("\n")


def main(path: str) -> None:
    lines = body(open(path).read())
    label_at = {m.group(1): i for i, l in enumerate(lines) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
    loops = []
    for i, l in enumerate(lines):
        m = re.match(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            loops.append((label_at[m.group(1)], i))
    lo, hi = max(loops, key=lambda p: p[1] - p[0])
    ins = [l.split()[0] for l in lines[lo:hi + 1] if re.match(r"^\s+[a-z]", l)]
    count = lambda pred: sum(1 for x in ins if pred(x))
    before = [l.split()[0] for l in lines[:lo] if re.match(r"^\s+[a-z]", l)]
    print(json.dumps({
        "kernel": "k_mini_filter",
        "per_candidate": {"valu": count(lambda x: x.startswith("v_")), "salu": count(lambda x: x.startswith("s_")),
                          "lds": count(lambda x: x.startswith("ds_")),
                          "alignbit": count(lambda x: x == "v_alignbit_b32"), "bitop3": count(lambda x: x == "v_bitop3_b32"),
                          "add": count(lambda x: x.startswith("v_add")), "total": len(ins)},
        "per_row_of_58": {"valu": sum(1 for x in before if x.startswith("v_")), "total": len(before)},
    }))


if __name__ == "__main__":
    main(sys.argv[1])
