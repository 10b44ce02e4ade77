#!/usr/bin/env python
"""Are the kernels of one gfx950 assembly file (hipcc -save-temps / -S output) the same code in another build of it?

    python tools/isa_same.py before.s after.s [name-filter]

Compares, for every kernel of before.s whose demangled name contains the filter, the body (label numbers normalised, comments dropped) and the
.amdhsa_ resource block with the kernel of the same name in after.s. Prints one line a kernel and a summary; exits 1 on any difference or
any kernel missing from after.s. Kernels only after.s has are listed as new."""
from __future__ import annotations

import re
import sys

from isa_report import demangle


def kernels(path):
    text = open(path, errors="replace").read()
    out = {}
    for m in re.finditer(r"^(_Z\w+|\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = []
        for ln in m.group(2).split("\n"):
            ln = ln.split(";")[0].rstrip()
            if ln.strip():
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", ln))
        out[m.group(1)] = ["\n".join(body), ""]
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
        if m.group(1) in out:
            out[m.group(1)][1] = m.group(2)
    return {k: v for k, v in out.items() if v[1]}


def main():
    if len(sys.argv) < 3:
        print(__doc__)
        return 2
    before, after = kernels(sys.argv[1]), kernels(sys.argv[2])
    filt = sys.argv[3] if len(sys.argv) > 3 else ""
    names = sorted(before)
    pretty = dict(zip(names, demangle(names)))
    bad = same = 0
    for name in names:
        if filt not in pretty[name]:
            continue
        if name not in after:
            print(f"MISSING    {pretty[name]}")
            bad += 1
        elif before[name] != after[name]:
            print(f"DIFFERENT  {pretty[name]}")
            bad += 1
        else:
            n = before[name][0].count("\n") + 1
            print(f"identical  {pretty[name]}  ({n} lines)")
            same += 1
    new = sorted(set(after) - set(before))
    for name, label in zip(new, demangle(new)):
        print(f"new        {label}")
    print(f"{same} kernels identical, {bad} different or missing, {len(new)} new")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
