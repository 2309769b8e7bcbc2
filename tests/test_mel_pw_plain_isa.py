"""ISA budget of the plain-output instance k_mel_plain_pw<1024,16,2,1> against the general instance k_mel_pw<1024,16,false> it
specialises (CPU test: hipcc cross-compiles gfx950 once; both symbols come from the same listing).

Frame loop = the blocks of the depth-1 loop behind the prologue barrier: from the first block that names the loop's header to the
end of the last one, counted statically in layout order as profiles/mel_pw_geometry_isa.md counts its spans (branches that one
frame does not take included: both kernels carry the same edge-frame and no-ticket fetch paths).  profiles/mel_pw_plain.md has the
table; MIN_VALU_SAVED is the figure it states."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GENERAL = "_ZN3kpr8k_mel_pwILi1024ELi16ELb0EEEvPKfNS_4GeomES2_PK15HIP_vector_typeIfLj2EENS_6PwPlanENS_5DbDevEPjPfiiPx"
PLAIN = "_ZN3kpr14k_mel_plain_pwILi1024ELi16ELi2ELi1EEEvPKfNS_4GeomES2_PK15HIP_vector_typeIfLj2EENS_6PwPlanEPfiiPx"
MIN_VALU_SAVED = 120                   # profiles/mel_pw_plain.md section 1: 958 -> 825 vector instructions in the frame loop


@pytest.fixture(scope="module")
def asm():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    with tempfile.TemporaryDirectory() as td:
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-pass-failed",
                        "-DKPR_RING_DEPTH=3", "--cuda-device-only", "-S",
                        os.path.join(REPO, "kapre_amd", "csrc", "kapre_hip.hip"), "-o", "k.s"],
                       cwd=td, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(os.path.join(td, "k.s")).read()


def _metadata(asm_text, kernel):
    m = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                  r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % kernel, asm_text)
    assert m, "metadata of %s" % kernel
    return dict(zip(("scratch", "sgpr_spills", "vgprs", "vgpr_spills"), (int(g) for g in m.groups())))


def frame_loop(asm_text, kernel):
    """instructions (mnemonic, operands) of the kernel's frame loop, in layout order"""
    i = asm_text.index("\n" + kernel + ":")
    lines = asm_text[i:asm_text.index(".end_amdhsa_kernel", i)].splitlines()
    bar = next(k for k, l in enumerate(lines) if l.strip().startswith("s_barrier"))
    head = next(k for k in range(bar, len(lines)) if "Loop Header: Depth=1" in lines[k])
    tag = re.match(r"\.L(BB\d+_\d+):", lines[head].strip()).group(1)
    starts = [k for k, l in enumerate(lines) if re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)", l.strip())]
    mine = [k for k in starts if k == head or re.search(r"\b%s\b" % tag, lines[k])]
    end = next((k for k in starts if k > max(mine)), len(lines))
    out = []
    for line in lines[min(mine):end]:
        s = line.strip()
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        out.append(s.split(None, 1))
    return out


def counts(ins):
    op = [p[0] for p in ins]
    return {"valu": sum(o.startswith("v_") for o in op),
            "salu": sum(o.startswith("s_") and not o.startswith(("s_waitcnt", "s_nop", "s_load", "s_buffer_load")) for o in op),
            "lds": sum(o.startswith("ds_") for o in op),
            "lgkm_waits": sum(1 for p in ins if p[0] == "s_waitcnt" and len(p) > 1 and "lgkmcnt" in p[1]),
            "total": len(op)}


def test_registers_and_spills(asm):
    gen, plain = _metadata(asm, GENERAL), _metadata(asm, PLAIN)
    assert plain["scratch"] == 0 and plain["vgpr_spills"] == 0
    assert plain["vgprs"] <= 128
    assert plain["sgpr_spills"] <= gen["sgpr_spills"], (plain, gen)


def test_frame_loop_has_fewer_vector_instructions(asm):
    gen, plain = counts(frame_loop(asm, GENERAL)), counts(frame_loop(asm, PLAIN))
    print("general", gen, "plain", plain)
    assert gen["valu"] > 600 and plain["valu"] > 600             # both spans hold the FFT
    assert plain["valu"] <= gen["valu"] - MIN_VALU_SAVED, (gen, plain)
    assert plain["lgkm_waits"] < gen["lgkm_waits"] and plain["salu"] < gen["salu"], (gen, plain)


def test_one_lane_draw_and_scalar_row_base(asm):
    """the ticket is drawn with one LDS instruction (no wave-aggregated add), and every output store takes the frame's row from
    an SGPR pair"""
    ins = frame_loop(asm, PLAIN)
    ops = [p[0] for p in ins]
    assert ops.count("ds_inc_rtn_u32") == 1 and not any(o.startswith(("ds_add_rtn", "s_bcnt1")) for o in ops)
    stores = [p for p in ins if p[0].startswith("global_store")]
    assert stores and all(re.search(r", s\[\d+:\d+\]", p[1]) for p in stores), stores
    assert not any(o.startswith("flat_") for o in ops)
