#!/usr/bin/env python3
"""Compare the gfx950 code of two builds of pose2room_amd/csrc, kernel by kernel.

Both directories are built with the Makefile's own flags plus the compiler's ISA listings:
    make -C <dir> EXTRA=--save-temps
For every kernel of the named translation units (default: the users of stgcn_tile.h) the instruction stream
(comments and debug labels dropped) and the six resource values of the kernel metadata are compared.  Prints one
markdown table row per kernel; exit status 1 when any kernel differs.

    python tools/compare_isa.py <parent csrc dir> <branch csrc dir> [unit ...]
"""
import os
import re
import subprocess
import sys
from collections import Counter

UNITS = ["stgcn_gcn2", "stgcn_gcn3", "stgcn_gcn3_grad", "stgcn_gcn3h_grad", "stgcn_gcn3_dw", "stgcn_gcn3h_fwd",
         "stgcn_gcn3h_dx", "stgcn_tconv2", "stgcn_tconv3"]
META = [".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
        ".private_segment_fixed_size"]
SUFFIX = "-hip-amdgcn-amd-amdhsa-gfx950.s"


def kernels(path):
    """{kernel name: (instruction lines, {metadata key: value})} of one ISA listing."""
    text = open(path).read().split("\n")
    names = [l.split()[1] for l in text if l.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(text) if l.startswith(name + ":"))
        ins = []
        for l in text[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";")[0].strip()
            if (l and not l.startswith((".", "_"))) or re.match(r"\.LBB\d+_\d+:", l):
                ins.append(re.sub(r"\s+", " ", l))
        out[name] = [ins, {}]
    cur = None
    for l in text[text.index("amdhsa.kernels:"):]:
        l = l.strip().lstrip("- ").strip()
        k, _, v = l.partition(":")
        if k in META or k == ".name":
            cur = cur or {}
            cur[k] = v.strip()
        if l.startswith(".wavefront_size"):      # last key of a kernel's record
            out[cur.pop(".name")][1] = cur
            cur = None
    return out


def main():
    a_dir, b_dir = sys.argv[1], sys.argv[2]
    units = sys.argv[3:] or UNITS
    print("| kernel | instructions | identical | " + " | ".join(m[1:] for m in META) + " |")
    print("|---|---|---|" + "---|" * len(META))
    bad = 0
    for u in units:
        a, b = kernels(os.path.join(a_dir, u + SUFFIX)), kernels(os.path.join(b_dir, u + SUFFIX))
        for name in sorted(set(a) | set(b)):
            short = subprocess.run(["c++filt", "-p", name], capture_output=True, text=True).stdout.strip()
            short = short.replace("(anonymous namespace)::", "") or name
            if name not in a or name not in b:
                print("| %s | - | only in %s | |" % (short, "parent" if name in a else "branch"))
                bad += 1
                continue
            (ia, ma), (ib, mb) = a[name], b[name]
            same = "yes" if ia == ib and ma == mb else ("no (same mix)" if Counter(x.split()[0] for x in ia) ==
                                                        Counter(x.split()[0] for x in ib) else "no")
            bad += same != "yes"
            cells = [ma[m] if ma[m] == mb[m] else "%s -> %s" % (ma[m], mb[m]) for m in META]
            n = str(len(ia)) if len(ia) == len(ib) else "%d -> %d" % (len(ia), len(ib))
            print("| %s | %s | %s | %s |" % (short, n, same, " | ".join(cells)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
