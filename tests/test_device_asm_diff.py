"""tools/device_asm_diff.py: the splitter and the normaliser on hand-written assembly (no compilation).  Two dumps of the same kernel
that differ only in the function index of their labels (and in comments) compare equal; one changed operand does not."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("device_asm_diff", os.path.join(ROOT, "tools", "device_asm_diff.py"))
dad = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dad)

ASM = """\
	.text
	.protected	_Z3k_aPf
	.globl	_Z3k_aPf
	.type	_Z3k_aPf,@function
_Z3k_aPf:                               ; @_Z3k_aPf
; %bb.{bb}:
	s_load_dwordx2 s[0:1], s[0:1], 0x0
	s_branch .LBB{fn}_0
	.p2align	8
.LBB{fn}_0:
	v_mov_b32_e32 v1, {imm}
	s_cbranch_execz .LBB{fn}_2
; %bb.{bb}:
	global_store_dword v0, v1, s[0:1]
.LBB{fn}_2:                                ; %exit
	s_endpgm
	.section	.rodata,"a",@progbits
	.amdhsa_kernel _Z3k_aPf
		.amdhsa_group_segment_fixed_size {lds}
		.amdhsa_next_free_vgpr 2
	.end_amdhsa_kernel
	.text
.Lfunc_end{fn}:
	.size	_Z3k_aPf, .Lfunc_end{fn}-_Z3k_aPf
                                        ; -- End function
	.set _Z3k_aPf.num_vgpr, 2
; NumVgprs: 2
	.type	_ZL5table,@object
	.section	.rodata,"a",@progbits
_ZL5table:
	.long	{tab}
	.asciz	"a;b"                   ; a quoted semicolon
	.size	_ZL5table, 4
	.type	_Z3k_bv,@function
_Z3k_bv:
	s_endpgm
.Lfunc_end{fn2}:
	.size	_Z3k_bv, .Lfunc_end{fn2}-_Z3k_bv
	.ident	"{ident}"
	.amdgpu_metadata
    .name:           _Z3k_aPf
	.end_amdgpu_metadata
"""


def _asm(fn=0, bb=0, imm="0x3f800000", lds=0, tab=7, ident="clang"):
    return ASM.format(fn=fn, fn2=fn + 1, bb=bb, imm=imm, lds=lds, tab=tab, ident=ident)


def test_normalise_split_compare():
    assert dad.normalise("\ts_cbranch_execz .LBB12_3   ; comment") == "\ts_cbranch_execz .LBB_3"
    assert dad.normalise(".Lfunc_end7:") == ".Lfunc_end:"
    assert dad.normalise("\t.size	k, .Lfunc_end7-k") == "\t.size	k, .Lfunc_end-k"
    assert dad.normalise("; %bb.4:") == ""
    assert dad.normalise("\tv_mov_b32_e32 v12, v3") == "\tv_mov_b32_e32 v12, v3"      # registers and immediates keep their digits

    assert dad.normalise('\t.asciz\t"a;b"   ; c') == '\t.asciz\t"a;b"'                     # a ';' inside a string is no comment
    assert dad.normalise("__hip_cuid_ae7fd0574bafc11f:") == "__hip_cuid:"

    a, fa, na = dad.split_symbols(_asm(fn=0, bb=0))
    b, fb, nb = dad.split_symbols(_asm(fn=41, bb=332))
    assert sorted(a) == sorted(["_Z3k_aPf", "_Z3k_bv", "_ZL5table", dad.REST]) and (fa, fb, na, nb) == (2, 2, 1, 1)
    assert '\t.asciz\t"a;b"' in a["_ZL5table"] and any(".ident" in l for l in a[dad.REST])
    assert sum(dad.is_instruction(l) for l in a["_Z3k_aPf"]) == 6 and sum(dad.is_instruction(l) for l in a["_Z3k_bv"]) == 1
    assert any(".amdhsa_group_segment_fixed_size" in l for l in a["_Z3k_aPf"])      # the descriptor and the resource lines belong to the symbol
    assert any(".num_vgpr" in l for l in a["_Z3k_aPf"]) and not any("metadata" in l or ".name" in l for l in a["_Z3k_bv"])
    assert dad.compare(a, b) == []                                                   # the label index alone: equal

    c = dad.split_symbols(_asm(fn=0, bb=0, imm="0x3f000000"))[0]                    # one operand
    d = dad.compare(a, c)
    assert [n for n, _ in d] == ["_Z3k_aPf"] and "0x3f000000" in d[0][1]
    assert [n for n, _ in dad.compare(a, dad.split_symbols(_asm(tab=8))[0])] == ["_ZL5table"]             # a constant table
    assert [n for n, _ in dad.compare(a, dad.split_symbols(_asm(ident="other"))[0])] == [dad.REST]       # a directive outside every symbol
    e = dad.split_symbols(_asm(lds=4096))[0]                                         # the descriptor alone (LDS size)
    assert [n for n, _ in dad.compare(a, e)] == ["_Z3k_aPf"]
    del e["_Z3k_bv"]
    assert ("_Z3k_bv", "only in A") in dad.compare(a, e)
