#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the gfx950 code of two source trees.

    python tools/isa_compare.py OLD_CSRC NEW_CSRC [--files-old a.hip,b.hip] [--files-new ...]
                                [--out FILE.json]

Compiles the kernel sources of both trees to device assembly with the build's
own flags (isa_phases.compile_asm, no marks) and compares, for every kernel
symbol, the instruction text after two normalisations: the local labels
.LBBn_m are renumbered in order of appearance, and comment and directive
lines are dropped.  Prints one line per kernel: same, DIFF (with both
instruction counts), old-only or new-only; a kernel that differs or exists
on one side only also gets its VGPRs, SGPRs, LDS, scratch, spills and
occupancy.  The comparison is of text only.  Needs hipcc, no GPU.

Without --files-*, a tree's files are those of COUNT_FILES that it holds.
"""
import argparse
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_phases import body_of, compile_asm  # noqa: E402

COUNT_FILES = ["hm_kernels.hip", "hm_aggregate.hip", "hm_general.hip"]
FIGURES = ["TotalNumSgprs", "NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize"]


def normalise(body):
    names, out = {}, []
    for l in body:
        s = l.split(";")[0].strip()
        if not s or s.startswith(("//", ".")) and not s.endswith(":"):
            continue
        s = re.sub(r"\.LBB\d+_\d+", lambda m: names.setdefault(m.group(0), ".L%d" % len(names)), s)
        out.append(" ".join(s.split()))
    return out


def figures(text, sym, tail):
    f = {}
    for l in tail:
        m = re.match(r";\s*(\w+):?\s*(\d+)", l.strip())
        if m and m.group(1) in FIGURES:
            f[m.group(1)] = int(m.group(2))
    for blk in re.split(r"\n\s+- \.agpr_count", text[text.find("amdhsa.kernels"):]):
        if re.search(r"\.name:\s+%s\s" % re.escape(sym), blk):
            for key in ("sgpr_spill_count", "vgpr_spill_count"):
                m = re.search(r"\.%s:\s+(\d+)" % key, blk)
                if m:
                    f[key] = int(m.group(1))
    return f


def kernels(csrc, files):
    """-> {symbol: (file, instruction lines, figures)} over the kernel symbols of the files."""
    out = {}
    for fn in files:
        text = compile_asm(csrc, None, [], source=fn)
        for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
            body, tail = body_of(text, sym)
            ins = [l for l in normalise(body) if not l.endswith(":")]
            out[sym] = (fn, normalise(body), len(ins), figures(text, sym, tail))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--files-old", default=None)
    ap.add_argument("--files-new", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    def files(csrc, given):
        want = given.split(",") if given else COUNT_FILES
        return [f for f in want if os.path.exists(os.path.join(csrc, f))]

    old, new = kernels(a.old, files(a.old, a.files_old)), kernels(a.new, files(a.new, a.files_new))
    rows = []
    for sym in sorted(set(old) | set(new)):
        o, n = old.get(sym), new.get(sym)
        row = {"kernel": sym, "old_file": o and o[0], "new_file": n and n[0]}
        if o and n:
            row["status"] = "same" if o[1] == n[1] else "DIFF"
        else:
            row["status"] = "old-only" if o else "new-only"
        if row["status"] != "same":
            row["old"] = o and dict(instructions=o[2], **o[3])
            row["new"] = n and dict(instructions=n[2], **n[3])
        else:
            row["instructions"] = n[2]
        rows.append(row)
        print("%-8s %-72s %s" % (row["status"], sym, row.get("instructions",
              "%s -> %s" % (o and o[2], n and n[2]))))
        if row["status"] != "same":
            print("         old %s\n         new %s" % (row["old"], row["new"]))
    tally = {}
    for r in rows:
        tally[r["status"]] = tally.get(r["status"], 0) + 1
    print(tally)
    if a.out:
        with open(a.out, "w") as f:   # one line per kernel
            f.write('{"tally": %s, "kernels": [\n' % json.dumps(tally))
            f.write(",\n".join(json.dumps(r) for r in rows) + "\n]}\n")


if __name__ == "__main__":
    main()
