#!/usr/bin/env python3
"""Has a change moved the generated code of kernels it did not mean to touch?  Compares two `hipcc -S` outputs of
csrc/hydro_kernels.hip (build.device_flags() + --cuda-device-only -S), restricted to the kernels whose mangled name
contains one of the needles: the function text from its label to its end marker and its .amdhsa_kernel descriptor.
The per-function numbering of local labels (.LBB<fn>_<block>, .Lfunc_end<fn>) depends on how many functions precede it in
the file, not on its code, and is normalised away.

  python scripts/asm_symbols.py [--commutative] before.s after.s step_fused_multi_tiled_kernelI [more needles]
exit status 0 and "identical" per kernel, or 1 and the first differing lines.

--commutative: moving a kernel body into an inlined function can make the compiler exchange the two sources of a
commutative instruction (`v_mul_f64 v[24:25], v[2:3], v[4:5]` -> `... v[4:5], v[2:3]`): same opcodes in the same order,
same registers, same arithmetic.  With the option the first two source operands of the instructions in COMMUTATIVE - and
of nothing else - are put in sorted order before the texts are compared; an operand's modifiers (-v3, |v3|) travel with
it.  Never in the list: subtractions, compares, selects, shifts, divisions, anything with carry."""
import difflib
import re
import sys

COMMUTATIVE = re.compile(r"(v_(add|mul|max|min)_(f16|f32|f64)|v_mul_legacy_f32|v_fma_(f32|f64)|v_(and|or|xor)_b32|v_add_u32|"
                         r"v_mul_(lo|hi)_u32|v_pk_(add|mul|fma)_f32|s_(and|or|xor)_b(32|64)|s_mul_i32|s_add_i32)(_e32|_e64)?")
# modifiers that address the sources by position: a line that carries one is compared as it stands
POSITIONAL = ("op_sel", "neg_lo", "neg_hi")


def sort_sources(line: str) -> str:
    """`line` with its first two source operands in sorted order, if its instruction is commutative in them."""
    head = line.split(None, 1)
    if len(head) < 2 or not COMMUTATIVE.fullmatch(head[0]) or any(p in head[1] for p in POSITIONAL):
        return line
    ops = [o.strip() for o in head[1].split(",")]
    if len(ops) < 3:
        return line
    last, _, modifiers = ops[-1].partition(" ")          # (the instruction's own modifiers follow the last operand: clamp, mul:2)
    ops[-1] = last
    ops[1:3] = sorted(ops[1:3])
    return line[:len(line) - len(line.lstrip())] + head[0] + " " + ", ".join(ops) + (" " + modifiers if modifiers else "")


def kernels(asm: str, needles, commutative: bool = False) -> dict:
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.S | re.M):
        name = m.group(1)
        if any(n in name for n in needles):
            text = re.sub(r"\.LBB\d+_", ".LBB_", m.group(2))
            lines = [l.split(";")[0].rstrip() for l in text.splitlines()]            # (comments name basic blocks by function number too)
            out[name] = [sort_sources(l) if commutative else l for l in lines if l]
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", asm, re.S):
        if m.group(1) in out:
            out[m.group(1)] += ["<descriptor>"] + m.group(2).splitlines()
    return out


def main(before: str, after: str, needles, commutative: bool = False) -> int:
    a, b = kernels(open(before).read(), needles, commutative), kernels(open(after).read(), needles, commutative)
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
    args = [x for x in sys.argv[1:] if x != "--commutative"]
    sys.exit(main(args[0], args[1], args[2:], "--commutative" in sys.argv[1:]))
