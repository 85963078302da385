#!/usr/bin/env python3
"""Basic blocks of one kernel in a gfx950 assembly listing (hipcc -S --offload-device-only): for every label the number
of instructions up to the next label, its share of v_mad_u64_u32, and where its branches go.  Used to count the
steady-state loop body of k_accumulate ("Bucket addition: instruction count").

    python tools/loop_count.py msm.s _ZN3lsa12k_accumulateINS_7CurveG1ELj1EE
"""
import re
import sys


def blocks(path, prefix):
    out, cur, inside = [], None, False
    for line in open(path):
        s = line.strip()
        if not inside:
            if s.startswith(prefix) and ":" in s.split(";")[0]:
                inside = True
                cur = {"label": "entry", "n": 0, "mad": 0, "br": []}
                out.append(cur)
            continue
        if s.startswith(".Lfunc_end"):
            break
        if not s or s.startswith(";") or s.startswith("."):
            m = re.match(r"(\.LBB\d+_\d+):", s)
            if m:
                cur = {"label": m.group(1), "n": 0, "mad": 0, "br": []}
                out.append(cur)
            continue
        op = s.split()[0]
        cur["n"] += 1
        if op.startswith("v_mad_u64_u32"):
            cur["mad"] += 1
        if op.startswith("s_cbranch") or op == "s_branch":
            cur["br"].append("@%d %s %s" % (cur["n"], op, s.split()[1]))      # @k: the branch is the block's k-th instruction
        if op == "s_endpgm":
            cur["br"].append("end")
    return out


if __name__ == "__main__":
    bl = blocks(sys.argv[1], sys.argv[2])
    for i, b in enumerate(bl):
        print("%3d %-12s %5d instr %5d mad  %s" % (i, b["label"], b["n"], b["mad"], ", ".join(b["br"])))
    print("total", sum(b["n"] for b in bl))
