#!/usr/bin/env python3
"""Has a change moved the generated code of kernels it did not mean to touch?  Compares two `hipcc -S` outputs of
csrc/hydro_kernels.hip (build.device_flags() + --cuda-device-only -S), restricted to the kernels whose mangled name
contains one of the needles: the function text from its label to its end marker and its .amdhsa_kernel descriptor.
The per-function numbering of local labels (.LBB<fn>_<block>, .Lfunc_end<fn>) depends on how many functions precede it in
the file, not on its code, and is normalised away.

  python scripts/asm_symbols.py before.s after.s step_fused_multi_tiled_kernelI [more needles]
exit status 0 and "identical" per kernel, or 1 and the first differing lines."""
import difflib
import re
import sys


def kernels(asm: str, needles) -> dict:
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        name = m.group(1)
        if any(n in name for n in needles):
            text = re.sub(r"\.LBB\d+_", ".LBB_", m.group(2))
            lines = [l.split(";")[0].rstrip() for l in text.splitlines()]            # (comments name basic blocks by function number too)
            out[name] = [l for l in lines if l]
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        if m.group(1) in out:
            out[m.group(1)] += ["<descriptor>"] + m.group(2).splitlines()
    return out


def main(before: str, after: str, needles) -> int:
    a, b = kernels(open(before).read(), needles), kernels(open(after).read(), needles)
    bad = 0
    for name in sorted(set(a) | set(b)):
        if a.get(name) == b.get(name):
            continue
        bad += 1
        print("DIFFERS", name)
        for line in list(difflib.unified_diff(a.get(name, []), b.get(name, []), "before", "after", lineterm="", n=1))[:40]:
            print("   ", line)
    print(f"{len(a)} kernels before, {len(b)} after, {'identical' if not bad else str(bad) + ' differ'}")
    return 1 if bad or not a else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
