#!/usr/bin/env python3
"""Compare the kernel resource usage of two builds.

    make -C compression_algorithms_amd/csrc -Otarget EXTRA=-Rpass-analysis=kernel-resource-usage 2> build.log   (on each tree;
                                                                  -Otarget keeps a parallel build's remarks together per file)
    python scripts/resource_usage_diff.py parent.log tree.log [name filter ...]

Prints one line per kernel (demangled where c++filt is there): VGPRs, SGPRs, scratch, occupancy and LDS bytes of both builds;
a template instantiation that exists only in the second build is shown beside the first build's kernel of the same base name.
"""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "vgpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"),
          ("LDS Size [bytes/block]", "lds"))


def parse(path):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for key, short in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(key) + r": (\d+)", line)
            if m and cur is not None:
                cur[short] = int(m.group(1))
    return out


def demangle(names):
    try:
        res = subprocess.run(["c++filt", "-p"] + list(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: r.replace("(anonymous namespace)::", "") for n, r in zip(names, res)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    a, b = parse(sys.argv[1]), parse(sys.argv[2])
    filt = sys.argv[3:]
    names = demangle(sorted(set(a) | set(b)))
    base = lambda d: re.sub(r"<.*", "", d)
    by_base = {}
    for n in a:
        by_base.setdefault(base(names[n]), []).append(n)
    fmt = lambda r: "vgpr %3d sgpr %3d scratch %3d occ %d lds %6d" % tuple(r.get(s, -1) for _, s in FIELDS) if r else "(absent)"
    for n in sorted(set(a) | set(b), key=lambda n: names[n]):
        d = names[n]
        if filt and not any(f in d for f in filt):
            continue
        left = a.get(n)
        note = ""
        if left is None:                                   # a new instantiation: beside the parent's kernel of that name
            sib = [m for m in by_base.get(base(d), []) if re.sub(r"\btrue\b", "false", d) in (names[m], names[m] + "<false>")] or by_base.get(base(d), [])
            if sib:
                left, note = a[sib[0]], "   [parent: " + names[sib[0]] + "]"
        same = left is not None and b.get(n) is not None and all(left.get(s) == b[n].get(s) for _, s in FIELDS if s != "sgpr")
        print("%-44s parent %s | tree %s%s%s" % (d, fmt(left), fmt(b.get(n)), "" if n not in b or left is None else ("  same" if same else "  DIFFERS"), note))


if __name__ == "__main__":
    main()
