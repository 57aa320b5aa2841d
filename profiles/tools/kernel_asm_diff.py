"""Per-kernel comparison of two sets of gfx950 device assembly files (hipcc ... --cuda-device-only -S with the Makefile's
flags) — no GPU needed.

    python profiles/tools/kernel_asm_diff.py PARENT_DIR HEAD_DIR [--match REGEX]

Every *.s of the two directories is cut into kernels (.amdhsa_kernel symbols); comments, directives and the numbering of
block labels are dropped.  Per kernel, parent | head: instruction lines, VGPRs, SGPRs, scratch bytes, LDS bytes, occupancy
(the compiler's "Kernel info" figures), then "same" or where the texts differ: whether the body of the main loop — the
innermost loop that holds the most MFMA instructions, from its header label to its back-edge — is the parent's
instruction for instruction with only register numbers changed, or at least has the same multiset of opcodes, and how
many lines differ inside / outside it.
"""
import collections
import difflib
import glob
import os
import re
import subprocess
import sys

INFO = {"vgpr": r"; NumVgprs: (\d+)", "sgpr": r"; TotalNumSgprs: (\d+)", "scratch": r"; ScratchSize: (\d+)",
        "lds": r"; LDSByteSize: (\d+)", "occ": r"; Occupancy: (\d+)"}


def kernels(path):
    """{mangled name: (normalised instruction / label lines, info dict)}"""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, flags=re.M)
    out = {}
    for name in names:
        start = text.index("\n%s:" % name)
        end = text.index("; Kernel info:", start)
        tail = text[end:end + 1200]
        info = {k: int(re.search(p, tail).group(1)) for k, p in INFO.items()}
        lines = []
        for l in text[start:text.index(".Lfunc_end", start)].splitlines()[2:]:
            l = l.split(";")[0].strip()
            if not l or (l.startswith(".") and not l.endswith(":")):
                continue
            lines.append(re.sub(r"\.LBB\d+_\d+", ".LBB", " ".join(l.split())))
        out[name] = (lines, info)
    return out


def raw_labels(path, name):
    """the kernel's lines with their label numbers kept: the loop structure is read from these"""
    text = open(path).read()
    start = text.index("\n%s:" % name)
    lines = []
    for l in text[start:text.index(".Lfunc_end", start)].splitlines()[2:]:
        l = l.split(";")[0].strip()
        if l and not (l.startswith(".") and not l.endswith(":")):
            lines.append(" ".join(l.split()))
    return lines


def main_loop(lines):
    """(first, last) line index of the innermost loop with the most MFMAs"""
    where = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    best = None
    for i, l in enumerate(lines):
        m = re.match(r"s_c?branch\S* (\.LBB\d+_\d+)", l)
        if m and where.get(m.group(1), i) < i:
            a = where[m.group(1)]
            n = sum(1 for x in lines[a:i + 1] if x.startswith("v_mfma"))
            key = (-n, i - a)
            if best is None or key < best[0]:
                best = (key, a, i)
    return best[1], best[2]


def blank_registers(lines):
    """instructions in order, register numbers and label numbers blanked"""
    return [re.sub(r"\b([sv])\[?\d+(:\d+)?\]?", r"\1#", re.sub(r"\.LBB\d+_\d+", ".LBB", l)) for l in lines if not l.endswith(":")]


def opcodes(lines):
    return collections.Counter(l.split()[0] for l in lines if not l.endswith(":"))


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True)
    return {n: re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", d)) for n, d in zip(names, r.stdout.splitlines())}


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    match = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--match=")), ".")
    sides = []
    for d in args[:2]:
        ks = {}
        for f in sorted(glob.glob(os.path.join(d, "*.s"))):
            for name, v in kernels(f).items():
                ks[name] = v + (f,)
        sides.append(ks)
    a, b = sides
    dm = demangle(sorted(set(a) | set(b)))
    same = 0
    print("%-52s %13s %11s %9s %9s %15s %5s" % ("kernel", "lines", "VGPRs", "SGPRs", "scratch", "LDS", "occ"))
    for name in sorted(set(a) | set(b), key=lambda n: dm[n]):
        if not re.search(match, dm[name]):
            continue
        if name not in a or name not in b:
            print("%-52s only in %s" % (dm[name], "parent" if name in a else "head"))
            continue
        (la, ia, fa), (lb, ib, fb) = a[name], b[name]
        cols = "%-52s %5d | %-5d %4d | %-4d %3d | %-3d %3d | %-3d %6d | %-6d %d | %d" % (
            dm[name], len(la), len(lb), ia["vgpr"], ib["vgpr"], ia["sgpr"], ib["sgpr"], ia["scratch"], ib["scratch"],
            ia["lds"], ib["lds"], ia["occ"], ib["occ"])
        if la == lb:
            same += 1
            print(cols + "   same")
            continue
        ra, rb = raw_labels(fa, name), raw_labels(fb, name)
        (a0, a1), (b0, b1) = main_loop(ra), main_loop(rb)
        loop_same = opcodes(ra[a0:a1 + 1]) == opcodes(rb[b0:b1 + 1])
        renumbered = blank_registers(ra[a0:a1 + 1]) == blank_registers(rb[b0:b1 + 1])
        n_in = n_out = 0
        for tag, i0, i1, j0, j1 in difflib.SequenceMatcher(None, la, lb, autojunk=False).get_opcodes():
            if tag == "equal":
                continue
            n = max(i1 - i0, j1 - j0)
            if (i0 < i1 and a0 <= i0 <= a1) or (i0 == i1 and a0 < i0 <= a1):
                n_in += n
            else:
                n_out += n
        print(cols + "   main loop (%d | %d lines): %s, %d lines differ in it, %d outside" % (
            a1 - a0 + 1, b1 - b0 + 1, "the parent's instructions with registers renumbered" if renumbered else
            "opcode multiset equal" if loop_same else "opcode multiset DIFFERS", n_in, n_out))
        if not loop_same:
            d = opcodes(rb[b0:b1 + 1])
            d.subtract(opcodes(ra[a0:a1 + 1]))
            print("      head - parent: " + ", ".join("%s %+d" % kv for kv in sorted(d.items()) if kv[1]))
    print("%d kernels, %d identical" % (len([n for n in set(a) | set(b) if re.search(match, dm[n])]), same))


if __name__ == "__main__":
    main()
