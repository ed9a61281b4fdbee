#!/usr/bin/env python3
"""Static instruction count of the Burg recursion loops in the encoder's device ISA (profiles/burg_steps.txt).

  hipcc --offload-arch=gfx950 -O2 -std=c++17 -fPIC -Wno-pass-failed -DSOLO_WITH_ENCODER --cuda-device-only -S solo_amd/csrc/solo_enc_k.hip -o enc.s
  python tools/debug/burg_step_count.py enc.s

A recursion loop is recognised by the v_permlane32_swap pair of its step (b); it runs from its header label to its last back
branch.  Every instruction line in between is counted once (s_waitcnt, s_nop and branches included), which is one turn of the loop
with the division taken and no early exit.  The loops come out in source order: per kernel the two regimes of each call site
(hi = false first: the compiler puts the `rshifts <= -2` instance in front)."""
import re
import sys
from collections import Counter

CLASSES = ("VALU", "DPP/lane", "SALU", "DS", "s_waitcnt", "s_nop", "branch", "other")


def classify(op, line):
    if op.startswith("s_waitcnt"): return "s_waitcnt"
    if op == "s_nop": return "s_nop"
    if op.startswith("s_cbranch") or op == "s_branch": return "branch"
    if op.startswith("ds_"): return "DS"
    if op.startswith("v_permlane") or op.startswith("v_readlane") or op.startswith("v_readfirstlane") or op.startswith("v_writelane"): return "DPP/lane"
    if op.startswith("v_") and ("row_" in line or "quad_perm" in line or "_dpp" in op): return "DPP/lane"
    if op.startswith("v_"): return "VALU"
    if op.startswith("s_"): return "SALU"
    return "other"


def main(path):
    lines = open(path).read().split("\n")
    func, header_at, loops = None, {}, []
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", l)
        if m and not l.startswith(".L"): func = m.group(1)
        m = re.match(r"^(\.LBB\d+_\d+):.*Loop Header", l)
        if m: header_at[m.group(1)] = (i, func)
    swaps = [i for i, l in enumerate(lines) if "v_permlane32_swap" in l]
    seen = set()
    for s in swaps:
        head = max((v[0], k, v[1]) for k, v in header_at.items() if v[0] < s)
        if head[1] in seen or "burg" not in (head[2] or ""): continue
        seen.add(head[1])
        start, label, fn = head
        end = max(i for i, l in enumerate(lines) if re.search(r"s_cbranch\w*\s+" + re.escape(label) + r"\s*$", l) or re.search(r"s_branch\s+" + re.escape(label) + r"\s*$", l))
        if end < s: continue            # a loop in front of the swaps, not around them
        c, ops = Counter(), Counter()
        for l in lines[start + 1:end + 1]:
            t = l.strip()
            if not t or t.startswith(";") or t.startswith(".") or t.endswith(":") or re.match(r"^\.?\w+:", t): continue
            op = t.split()[0]
            c[classify(op, t)] += 1
            ops[op] += 1
        loops.append((fn, label, start + 1, end + 1, c, ops))
    print("%-34s %-10s %6s " % ("function", "loop", "all") + " ".join("%9s" % k for k in CLASSES) + "   ds_read ds_bperm readlane")
    for fn, label, a, b, c, ops in loops:
        print("%-34s %-10s %6d " % (fn[:34], label, sum(c.values())) + " ".join("%9d" % c[k] for k in CLASSES) +
              "   %7d %8d %8d" % (sum(v for k, v in ops.items() if k.startswith("ds_read")), ops["ds_bpermute_b32"], ops["v_readlane_b32"]))


if __name__ == "__main__":
    main(sys.argv[1])
