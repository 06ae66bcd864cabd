#!/usr/bin/env python3
"""Kernel resources and instruction counts of two builds, side by side: for every kernel symbol in the assembly files of directory A
(the parent commit's) and B (this tree's) -- hipcc --cuda-device-only -S of the trace units and post_kernels.hip with the Makefile's
flags -- VGPRs, SGPRs, scratch bytes and the number of instruction lines, and whether the instruction streams differ (a branch
counts by the instruction it goes to, not by the name of its label: the names number the file's functions in the order they come out).

    tools/isa_resources.py DIR_A DIR_B        prints the table (profiles/reach/isa_resources.txt is one)
"""
import glob
import os
import re
import subprocess
import sys


LABEL = re.compile(r"\.LBB\d+_\d+")


def kernels(path):
    """{symbol: (vgprs, sgprs, scratch, [instruction lines])} of one assembly file"""
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, re.M | re.S):
        sym, desc = m.group(1), m.group(2)

        def field(name):
            return int(re.search(r"\.amdhsa_%s\s+(\d+)" % name, desc).group(1))
        start = text.index("\n" + sym + ":")
        body = text[start:text.index("s_endpgm", start)]
        ins, at = [], {}
        for ln in body.splitlines()[2:]:
            ln = ln.split(";")[0].strip()
            if ln.endswith(":"):
                at[ln[:-1]] = len(ins)
            elif ln and not ln.startswith((".", ";")):
                ins.append(ln)
        # A block label (.LBB<n>_<k>) carries the number n of its function within the file, which moves when the file's kernels come
        # out in another order: a branch is compared by the instruction it goes to, "@<index in this kernel>", not by the label's name
        ins = [LABEL.sub(lambda m: "@%d" % at[m.group(0)] if m.group(0) in at else m.group(0), ln) for ln in ins]
        out[sym] = (field("next_free_vgpr"), field("next_free_sgpr"), field("private_segment_fixed_size"), ins)
    return out


def demangle(syms):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True, check=True).stdout.split("\n")
        return {s: d.replace("void ", "").replace("(pwn_trace_params)", "").replace("(bool)", "").replace("(int)", "") for s, d in zip(syms, out)}
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in syms}


def main(a, b):
    A, B = {}, {}
    for d, into in ((a, A), (b, B)):
        for f in sorted(glob.glob(os.path.join(d, "*.s"))):
            for sym, v in kernels(f).items():
                into[(os.path.basename(f), sym)] = v
    names = demangle(sorted({s for _, s in list(A) + list(B)}))
    print("%-22s %-62s %5s %5s %7s %6s   %s" % ("unit", "kernel", "VGPRs", "SGPRs", "scratch", "instr", "against the parent"))
    same = differ = new = 0
    for key in sorted(B, key=lambda k: (k not in A, k)):
        v, s, sc, ins = B[key]
        if key in A:
            pv, ps, psc, pins = A[key]
            if (pv, ps, psc, len(pins)) == (v, s, sc, len(ins)):
                d = [(x, y) for x, y in zip(pins, ins) if x != y]
                note = "same" if not d else "same resources and count; %d instruction(s) differ: %s" % (len(d), " | ".join("-%s +%s" % p for p in d[:2]))
                same += 1
            else:
                note = "DIFFERENT: parent %d / %d / %d / %d" % (pv, ps, psc, len(pins))
                differ += 1
        else:
            note = "NEW"
            new += 1
        print("%-22s %-62s %5d %5d %7d %6d   %s" % (key[0], names[key[1]], v, s, sc, len(ins), note))
    gone = sorted(set(A) - set(B))
    print("\n%d existing kernels with equal VGPRs, SGPRs, scratch and instruction count; %d different; %d new; %d gone" % (same, differ, new, len(gone)))
    return 1 if differ or gone else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
