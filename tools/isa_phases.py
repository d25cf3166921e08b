#!/usr/bin/env python3
"""Per-phase instruction counts of one kernel, read from its gfx950 assembly.

    python tools/isa_phases.py [--mode 4] [--kernel 'k_l1_fast<uint32_t,false>'] [-D NAME=V ...] [--csrc DIR]

Compiles the source that holds the kernel (MODE_FILES: hm_kernels.hip for
modes 1 to 4, hm_aggregate.hip for 5 and 7) to assembly with the build's own
flags plus -DHM_ISA_MARKS=<mode>, which turns the HM_STAMP_M(<mode>, n) sites
of that kernel (the phase-stamp sites of tools/stamps.py) into assembly
comments, and prints for the text between consecutive marks the number of VALU, SALU, LDS,
VMEM, SMEM, s_waitcnt and branch instructions (classified by mnemonic prefix
only), then the kernel's VGPRs, SGPRs, scratch and spills.  Three counts per
phase follow serial chains: the vmcnt waits before the phase's last VMEM
load, the lgkmcnt waits before its first LDS write, and the lgkmcnt waits
before its first VMEM store.  Phases are stretches of program TEXT: a block
the compiler laid out elsewhere (a cold path) counts where it stands.

Needs hipcc only: no GPU.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

MODE_NAMES = {
    2: ["issue+lds_setup", "project(loads)", "redo+count_rank", "reserve+scan", "stage", "dbase", "copy"],
    4: ["issue+lds_setup", "project(loads)", "redo+count_rank", "reserve+scan", "stage", "copy"],
}
# the source file that holds the kernel of each stamp mode (csrc/hm_stamps.h)
MODE_FILES = {1: "hm_kernels.hip", 2: "hm_kernels.hip", 3: "hm_kernels.hip", 4: "hm_kernels.hip",
              5: "hm_aggregate.hip", 7: "hm_aggregate.hip"}
CLASSES = ["VALU", "SALU", "LDS", "VMEM", "SMEM", "waitcnt", "branch"]
VMEM_PREFIXES = ("global_", "buffer_", "flat_", "scratch_")
BRANCH_PREFIXES = ("s_cbranch", "s_branch", "s_setpc", "s_swappc", "s_call")


def classify(mn):
    if mn.startswith("s_waitcnt"):
        return "waitcnt"
    if mn.startswith(BRANCH_PREFIXES):
        return "branch"
    if mn.startswith("v_"):
        return "VALU"
    if mn.startswith("ds_"):
        return "LDS"
    if mn.startswith(VMEM_PREFIXES):
        return "VMEM"
    if mn.startswith(("s_load", "s_buffer_load", "s_memtime", "s_memrealtime")):
        return "SMEM"
    if mn.startswith("s_"):
        return "SALU"
    return None


def compile_asm(csrc, mode, defines, keep=None, source=None):
    """Device assembly of `source` (default: the file of `mode`'s kernel);
    mode None: no marks, the code as the build compiles it."""
    from heatmap_amd import build as b

    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    flags = [f for f in b.FLAGS if f != "-fPIC"]
    marks = [] if mode is None else ["-DHM_ISA_MARKS=%d" % mode]
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, *marks, *["-D" + d for d in defines], "-S",
           "--cuda-device-only", os.path.join(csrc, source or MODE_FILES[mode]), "-o", out]
    subprocess.check_call(cmd)
    text = open(out).read()
    if keep:
        os.replace(out, keep)
    else:
        os.unlink(out)
    return text


TYPE_CODES = {"uint32_t": "j", "unsigned int": "j", "uint16_t": "t", "unsigned short": "t", "int": "i",
              "uint64_t": "m", "unsigned long": "m", "true": "Lb1E", "false": "Lb0E"}


def mangled_prefix(want):
    """'name<targ, ...>' -> the Itanium prefix of its symbol (the template
    arguments the kernels here use: integer types, bools, ints)."""
    m = re.match(r"\s*(\w+)\s*(?:<(.*)>)?\s*$", want)
    name, targs = m.group(1), m.group(2)
    pre = "_Z%d%s" % (len(name), name)
    if targs is None:
        return pre
    codes = []
    for t in targs.split(","):
        t = t.strip()
        codes.append(TYPE_CODES[t] if t in TYPE_CODES else "Li%sE" % t.replace("-", "n"))
    return pre + "I" + "".join(codes) + "E"


def find_kernel(text, want):
    syms = re.findall(r"^\s*\.globl\s+(\S+)", text, re.M)
    pre = mangled_prefix(want)
    hits = [s for s in syms if s.startswith(pre) and ("<" in want or not s[len(pre):].startswith("I"))]
    if len(hits) != 1:
        sys.exit("kernel %r (%s...): %d matches among %d symbols" % (want, pre, len(hits), len(syms)))
    return hits[0], want


def body_of(text, sym):
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].lstrip().startswith(".Lfunc_end"))
    # the register summary the compiler prints after the function
    tail = lines[end:end + 60]
    return lines[start + 1:end], tail


def analyse(body):
    """-> list of phases; a phase is (label, counts, chains)."""
    phases = []
    cur = {"label": "before mark 0", "ins": []}
    for l in body:
        s = l.strip()
        m = re.match(r";\s*hm_phase_mark\s+(\d+)", s)
        if m:
            phases.append(cur)
            cur = {"label": int(m.group(1)), "ins": []}
            continue
        if not s or s.startswith((";", ".", "//")) or s.endswith(":"):
            continue
        cur["ins"].append(s.split(";")[0].split())
    phases.append(cur)
    out = []
    for p in phases:
        c = dict.fromkeys(CLASSES, 0)
        mns = [i[0] for i in p["ins"]]
        for mn in mns:
            k = classify(mn)
            if k:
                c[k] += 1
        is_load = [mn.startswith(VMEM_PREFIXES) and "_load" in mn for mn in mns]
        is_store = [mn.startswith(VMEM_PREFIXES) and "_store" in mn for mn in mns]
        is_dsw = [mn.startswith("ds_write") or mn.startswith("ds_store") for mn in mns]
        wait = [(" ".join(i[1:]) if i[0].startswith("s_waitcnt") else None) for i in p["ins"]]

        def before(idx, what):
            return sum(1 for w in wait[:idx] if w is not None and what in w)

        last_load = max((i for i, v in enumerate(is_load) if v), default=None)
        first_dsw = next((i for i, v in enumerate(is_dsw) if v), None)
        first_st = next((i for i, v in enumerate(is_store) if v), None)
        last_dsw = max((i for i, v in enumerate(is_dsw) if v), default=None)
        chains = {
            "vmcnt waits before last load": None if last_load is None else before(last_load, "vmcnt"),
            "lgkmcnt waits before first LDS write": None if first_dsw is None else before(first_dsw, "lgkmcnt"),
            "before last LDS write": None if last_dsw is None else before(last_dsw, "lgkmcnt"),
            "lgkmcnt waits before first store": None if first_st is None else before(first_st, "lgkmcnt"),
        }
        out.append((p["label"], c, chains, len(mns)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", type=int, default=4, help="the kernel's HM_STAMPS number (4: k_l1_fast)")
    ap.add_argument("--kernel", default="k_l1_fast<uint32_t,false>")
    ap.add_argument("-D", dest="defines", action="append", default=[])
    ap.add_argument("--csrc", default=os.path.join(REPO, "heatmap_amd", "csrc"))
    ap.add_argument("--keep-asm", metavar="FILE", default=None, help="keep the assembly here")
    a = ap.parse_args()
    text = compile_asm(a.csrc, a.mode, a.defines, a.keep_asm)
    sym, dem = find_kernel(text, a.kernel)
    body, tail = body_of(text, sym)
    names = MODE_NAMES.get(a.mode, [])
    print("kernel  %s" % dem)
    print("defines %s" % (" ".join(a.defines) or "(none)"))
    print("%-28s %6s %6s %6s %6s %6s %8s %7s %6s" % ("phase", *CLASSES, "all"))
    tot = dict.fromkeys(CLASSES, 0)
    rows = analyse(body)
    for label, c, chains, n in rows:
        if isinstance(label, int):
            label = "%d %s" % (label, names[label] if label < len(names) else "end")
        print("%-28s %6d %6d %6d %6d %6d %8d %7d %6d" % (label, *[c[k] for k in CLASSES], n))
        for k in CLASSES:
            tot[k] += c[k]
    print("%-28s %6d %6d %6d %6d %6d %8d %7d" % ("total", *[tot[k] for k in CLASSES]))
    print()
    for label, c, chains, n in rows:
        if isinstance(label, int):
            label = "%d %s" % (label, names[label] if label < len(names) else "end")
        got = ", ".join("%s: %d" % (k, v) for k, v in chains.items() if v is not None)
        if got:
            print("%-28s %s" % (label, got))
    print()
    for l in tail:
        m = re.match(r";\s*(TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize|codeLenInByte):?\s*(.*)", l.strip())
        if m:
            print("%-14s %s" % (m.group(1), m.group(2)))
    m = re.search(r"\.name:\s+%s\b.*?\n(?=\s+- \.|\Z)" % re.escape(sym), text, re.S)
    meta = text[text.find("amdhsa.kernels"):]
    blocks = re.split(r"\n\s+- \.agpr_count", meta)
    for blk in blocks:
        if re.search(r"\.name:\s+%s\s" % re.escape(sym), blk):
            for key in ("sgpr_spill_count", "vgpr_spill_count"):
                mm = re.search(r"\.%s:\s+(\d+)" % key, blk)
                if mm:
                    print("%-14s %s" % (key, mm.group(1)))


if __name__ == "__main__":
    main()
