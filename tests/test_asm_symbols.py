"""scripts/asm_symbols.py decides whether a refactor left the device code alone, so what it calls "identical" is pinned
here on hand-written kernel texts (no compiler needed): exchanged sources of a listed commutative instruction compare equal
with --commutative and only with it; anything else - exchanged sources of a subtraction, a register, an opcode, a descriptor
field - differs either way."""
import pytest

from scripts import asm_symbols

KERNEL = """\t.text
\t.globl\t_Z6kernelILb0EEvPf
_Z6kernelILb0EEvPf:                     ; @_Z6kernelILb0EEvPf
; %bb.0:
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mul_f64 v[24:25], v[2:3], v[4:5]
\tv_add_f64 v[6:7], v[24:25], -v[8:9]
\tv_sub_f64 v[10:11], v[6:7], v[2:3]
\tv_fma_f32 v12, v1, |v0|, v13
\tv_cmp_lt_f32_e32 vcc, v12, v1
\ts_cbranch_vccz .LBB7_2
; %bb.1:
\tv_add_f32_e64 v12, v12, s2 clamp
.LBB7_2:
\tglobal_store_dword v14, v12, s[0:1]
\ts_endpgm
.Lfunc_end7:
\t.amdhsa_kernel _Z6kernelILb0EEvPf
\t\t.amdhsa_next_free_vgpr 26
\t\t.amdhsa_next_free_sgpr 6
\t.end_amdhsa_kernel
"""


def compare(tmp_path, before, after, commutative):
    a, b = tmp_path / "before.s", tmp_path / "after.s"
    a.write_text(before)
    b.write_text(after)
    return asm_symbols.main(str(a), str(b), ["_Z"], commutative)


def changed(old, new):
    assert KERNEL.count(old) == 1
    return KERNEL.replace(old, new)


def test_same_text_and_renumbered_labels_are_identical(tmp_path):
    moved = KERNEL.replace(".LBB7_", ".LBB31_").replace(".Lfunc_end7", ".Lfunc_end31")
    assert compare(tmp_path, KERNEL, moved, False) == 0
    assert compare(tmp_path, KERNEL, moved, True) == 0


@pytest.mark.parametrize("old, new", [
    ("v_add_f64 v[6:7], v[24:25], -v[8:9]", "v_add_f64 v[6:7], -v[8:9], v[24:25]"),        # the modifier travels with its operand
    ("v_mul_f64 v[24:25], v[2:3], v[4:5]", "v_mul_f64 v[24:25], v[4:5], v[2:3]"),
    ("v_fma_f32 v12, v1, |v0|, v13", "v_fma_f32 v12, |v0|, v1, v13"),                      # the two factors, not the addend
    ("v_add_f32_e64 v12, v12, s2 clamp", "v_add_f32_e64 v12, s2, v12 clamp"),
])
def test_exchanged_sources_of_a_commutative_instruction(tmp_path, old, new):
    assert compare(tmp_path, KERNEL, changed(old, new), True) == 0
    assert compare(tmp_path, KERNEL, changed(old, new), False) == 1


@pytest.mark.parametrize("old, new", [
    ("v_sub_f64 v[10:11], v[6:7], v[2:3]", "v_sub_f64 v[10:11], v[2:3], v[6:7]"),          # a subtraction is not commutative
    ("v_cmp_lt_f32_e32 vcc, v12, v1", "v_cmp_lt_f32_e32 vcc, v1, v12"),                    # nor a compare
    ("v_fma_f32 v12, v1, |v0|, v13", "v_fma_f32 v12, v1, v13, |v0|"),                      # nor a factor and the addend
    ("v_add_f64 v[6:7], v[24:25], -v[8:9]", "v_add_f64 v[6:7], -v[24:25], v[8:9]"),        # the modifier moved to the other operand
    ("v_mul_f64 v[24:25], v[2:3], v[4:5]", "v_mul_f64 v[24:25], v[2:3], v[6:7]"),          # a register
    ("v_mul_f64 v[24:25], v[2:3], v[4:5]", "v_mul_f64 v[26:27], v[2:3], v[4:5]"),          # the destination
    ("v_mul_f64 v[24:25], v[2:3], v[4:5]", "v_add_f64 v[24:25], v[2:3], v[4:5]"),          # an opcode
    ("v_add_f32_e64 v12, v12, s2 clamp", "v_add_f32_e64 v12, v12, s2"),                    # an instruction modifier
    (".amdhsa_next_free_vgpr 26", ".amdhsa_next_free_vgpr 28"),                            # a descriptor field
])
def test_anything_else_differs_with_and_without_the_option(tmp_path, old, new):
    assert compare(tmp_path, KERNEL, changed(old, new), True) == 1
    assert compare(tmp_path, KERNEL, changed(old, new), False) == 1


def test_the_order_of_two_instructions_and_a_missing_kernel_differ(tmp_path):
    a, b = "\tv_mul_f64 v[24:25], v[2:3], v[4:5]\n", "\tv_add_f64 v[6:7], v[24:25], -v[8:9]\n"
    assert compare(tmp_path, KERNEL, changed(a + b, b + a), True) == 1
    assert compare(tmp_path, KERNEL, KERNEL.replace("_Z6kernelILb0EEvPf", "_Z6kernelILb1EEvPf"), True) == 1
    assert compare(tmp_path, KERNEL, "\t.text\n", True) == 1
