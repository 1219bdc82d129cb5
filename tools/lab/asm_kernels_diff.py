#!/usr/bin/env python3
"""Same device code, kernel by kernel: compares the kernels of device assembly files (hipcc ... --cuda-device-only -S) keyed by kernel symbol.

    asm_kernels_diff.py parent.s -- new_a.s new_b.s [--twice KERNEL_NAME ...]

For a change that moves kernels between files or reorders their instantiations, where a whole-file diff cannot be empty.  Per kernel it
compares the instruction sequence, the .amdhsa_* descriptor block, the `.set <kernel>.<resource>` lines and the kernel's record in the
metadata note (register counts, scratch and LDS bytes, arguments).  What is normalised: comments, the per-function numbers of local labels
(.LBB<n>_, .Lfunc_end<n>), the kernel's own symbol, and an anonymous namespace in it (a kernel given internal linkage keeps its code).
Every kernel of the left side must appear exactly once on the right; the kernels named after --twice (demangled name up to the '(')
once in EACH right-hand file.  Exit status 0: all equal.  profiles/r15_wgrad_files.txt has a run."""
import collections
import re
import subprocess
import sys


def demangle(symbols):
    out = subprocess.run(["c++filt"], input="\n".join(symbols), capture_output=True, text=True, check=True).stdout
    return [s.replace("(anonymous namespace)::", "") for s in out.splitlines()]


def kernels(path):
    """{demangled signature: (text that must match, {resource: value})} of one assembly file"""
    lines = open(path).read().splitlines()
    symbols = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    names = dict(zip(symbols, demangle(symbols)))
    assert len(set(names.values())) == len(symbols), "two kernels of %s demangle to one name" % path
    found = {}
    for sym in symbols:
        begin = next(i for i, l in enumerate(lines) if l.startswith(sym + ":"))
        end = next(i for i in range(begin, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        text = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].strip()) for l in lines[begin + 1:end]]
        text += sorted(l.strip() for l in lines if l.startswith("\t.set " + sym + "."))
        # the metadata record: from "- .agpr_count" (its first key) to the next record, found through its .name line
        at = next(i for i, l in enumerate(lines) if l.split() == [".name:", sym])
        lo = max(i for i in range(at) if lines[i].lstrip().startswith("- .agpr_count"))
        hi = next(i for i in range(at, len(lines)) if lines[i].lstrip().startswith("- .agpr_count") or lines[i].startswith("amdhsa."))
        record = [l.strip().lstrip("- ") for l in lines[lo:hi]]
        text += record
        res = {k: int(v) for k, v in (l.rstrip().split(":") for l in record if re.match(r"\.(vgpr_count|private_segment_fixed_size|group_segment_fixed_size):", l))}
        found[names[sym]] = ([l.replace(sym, "KERNEL") for l in text if l], res)
    return found


def histogram(sides, key):
    c = collections.Counter(res[key] for k in sides for _, res in k.values())
    return ", ".join("%d x %d" % (v, n) for v, n in sorted(c.items()))


def main():
    args = sys.argv[1:]
    twice = []
    if "--twice" in args:
        twice = args[args.index("--twice") + 1:]
        args = args[:args.index("--twice")]
    left = [kernels(p) for p in args[:args.index("--")]]
    right = [kernels(p) for p in args[args.index("--") + 1:]]
    assert len(left) == 1, "one file on the left"
    bad = 0
    for name, (text, _) in sorted(left[0].items()):
        hits = [k[name][0] for k in right if name in k]
        want = len(right) if name.split("(")[0] in twice else 1
        if len(hits) != want:
            print("COUNT    %s: %d on the right, %d wanted" % (name, len(hits), want))
            bad += 1
        for h in hits:
            if h != text:
                first = next((i for i, (a, b) in enumerate(zip(text, h)) if a != b), min(len(text), len(h)))
                print("DIFFERS  %s: %d / %d lines, first at %d: %r / %r" % (name, len(text), len(h), first, text[first:first + 1], h[first:first + 1]))
                bad += 1
    extra = sorted(set(n for k in right for n in k) - set(left[0]))
    for name in extra:
        print("EXTRA    %s" % name)
    for side, ks in (("left", left), ("right", right)):
        print("%-5s kernels %d; .vgpr_count %s; .private_segment_fixed_size %s; .group_segment_fixed_size %s" % (
            side, sum(len(k) for k in ks), histogram(ks, ".vgpr_count"), histogram(ks, ".private_segment_fixed_size"),
            histogram(ks, ".group_segment_fixed_size")))
    print("%d kernels compared, %d differences, %d extra" % (len(left[0]), bad, len(extra)))
    return 1 if bad or extra else 0


if __name__ == "__main__":
    sys.exit(main())
