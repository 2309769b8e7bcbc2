"""tools/isa_diff.py: the kernel-by-kernel comparison of two device assemblies (CPU only, no compiler: hand-written text)."""
import importlib.util
import os

_TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "isa_diff.py")
_spec = importlib.util.spec_from_file_location("isa_diff", _TOOL)
isa_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_diff)


def _kernel(name, fn, labels, vreg="v1", comment="", lds=0):
    a, b = labels
    return """\t.protected\t{name}
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:
{comment}\ts_load_dwordx2 s[2:3], s[0:1], 0x0
\tv_mov_b32_e32 {vreg}, 0
\ts_cbranch_scc1 .LBB{fn}_{b}
.LBB{fn}_{a}:                                 ; =>This Inner Loop Header: Depth=1
\ts_sleep 2
\ts_cbranch_vccnz .LBB{fn}_{a}
.LBB{fn}_{b}:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size {lds}
\t\t.amdhsa_next_free_vgpr 2
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{fn}:
\t.size\t{name}, .Lfunc_end{fn}-{name}
; NumVgprs: 2
""".format(name=name, fn=fn, a=a, b=b, vreg=vreg, comment=comment, lds=lds)


def _meta(names, vgprs=2):
    out = "\t.amdgpu_metadata\n---\namdhsa.kernels:\n"
    for n in names:
        out += "  - .args:\n      - .offset:         0\n        .size:           8\n    .name:           %s\n" \
               "    .sgpr_count:     8\n    .vgpr_count:     %d\n    .wavefront_size: 64\n" % (n, vgprs)
    return out + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n"


_A = "\t.text\n" + _kernel("k_one", 0, (1, 2)) + _kernel("k_two", 1, (4, 7)) + _meta(["k_one", "k_two"])


def _names(text_a, text_b):
    a, b, only_a, only_b, differ = isa_diff.compare(text_a, text_b)
    return len(a), len(b), only_a, only_b, differ


def test_labels_comments_and_order_do_not_count():
    other = "\t.text\n" + _kernel("k_two", 0, (3, 9), comment="; kpr_lds_fence W\n\t; a comment line\n") + \
            _kernel("k_one", 1, (12, 5)) + _meta(["k_two", "k_one"])
    assert _names(_A, other) == (2, 2, [], [], [])


def test_a_changed_register_is_reported():
    other = "\t.text\n" + _kernel("k_one", 0, (1, 2)) + _kernel("k_two", 1, (4, 7), vreg="v3") + _meta(["k_one", "k_two"])
    assert _names(_A, other) == (2, 2, [], [], ["k_two"])


def test_a_swapped_branch_target_is_reported():
    # the renaming is by order of appearance: a branch to the OTHER label is a difference, not a renumbering
    other = _A.replace("s_cbranch_vccnz .LBB0_1", "s_cbranch_vccnz .LBB0_2")
    assert _names(_A, other) == (2, 2, [], [], ["k_one"])


def test_a_changed_descriptor_field_is_reported():
    other = "\t.text\n" + _kernel("k_one", 0, (1, 2), lds=4096) + _kernel("k_two", 1, (4, 7)) + _meta(["k_one", "k_two"])
    assert _names(_A, other) == (2, 2, [], [], ["k_one"])
    other = "\t.text\n" + _kernel("k_one", 0, (1, 2)) + _kernel("k_two", 1, (4, 7)) + _meta(["k_one", "k_two"], vgprs=3)
    assert _names(_A, other) == (2, 2, [], [], ["k_one", "k_two"])


def test_missing_and_extra_symbols_and_exit_status(tmp_path, capsys):
    other = "\t.text\n" + _kernel("k_one", 0, (1, 2)) + _kernel("k_three", 1, (4, 7)) + _meta(["k_one", "k_three"])
    assert _names(_A, other) == (2, 2, ["k_two"], ["k_three"], [])
    pa, pb = tmp_path / "a.s", tmp_path / "b.s"
    pa.write_text(_A)
    pb.write_text(other)
    assert isa_diff.main([str(pa), str(pa)]) == 0
    assert isa_diff.main([str(pa), str(pb)]) == 1
    out = capsys.readouterr().out
    assert "k_two" in out and "k_three" in out and "kernels: 2 in" in out
    pb.write_text(_A.replace("v_mov_b32_e32 v1, 0", "v_mov_b32_e32 v1, 1"))
    assert isa_diff.main([str(pa), str(pb), "--show", "k_one"]) == 1
    out = capsys.readouterr().out
    assert "-\tv_mov_b32_e32 v1, 0" in out and "+\tv_mov_b32_e32 v1, 1" in out
