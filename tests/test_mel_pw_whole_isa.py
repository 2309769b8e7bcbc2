"""ISA budget of the whole-frames instance k_mel_whole_pw<1024,16,2,1> against the plain instance k_mel_plain_pw<1024,16,2,1> it
specialises (CPU test: hipcc cross-compiles gfx950 once; both symbols come from the same listing).

Frame loop = the blocks of the depth-1 loop behind the prologue barrier, counted statically in layout order exactly as
tests/test_mel_pw_plain_isa.py counts them (the helpers are copies of that file's).  The plain loop holds the zero-filling edge
fetch and the per-store tests; the whole-frames loop must not.  profiles/mel_pw_whole.md has the table; MIN_VALU_SAVED is the
figure it states."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PLAIN = "_ZN3kpr14k_mel_plain_pwILi1024ELi16ELi2ELi1EEEvPKfNS_4GeomES2_PK15HIP_vector_typeIfLj2EENS_6PwPlanEPfiiPx"
WHOLE = "_ZN3kpr14k_mel_whole_pwILi1024ELi16ELi2ELi1EEEvPKfNS_4GeomES2_PK15HIP_vector_typeIfLj2EENS_6PwPlanEPfiiPx"
MIN_VALU_SAVED = 200                   # profiles/mel_pw_whole.md section 1: 825 -> 620 vector instructions in the frame loop


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
    plain, whole = _metadata(asm, PLAIN), _metadata(asm, WHOLE)
    assert whole["scratch"] == 0 and whole["vgpr_spills"] == 0
    assert whole["vgprs"] <= 128
    assert whole["sgpr_spills"] <= plain["sgpr_spills"], (whole, plain)


def test_frame_loop_has_no_edge_fetch(asm):
    """no flat access, and none of the zero-filling fetch's per-sample dword loads (the whole-frame fetch is sixteen dwordx2)"""
    plain, whole = frame_loop(asm, PLAIN), frame_loop(asm, WHOLE)
    assert not any(p[0].startswith("flat_") for p in whole)
    n_plain, n_whole = (sum(p[0] == "global_load_dword" for p in ins) for ins in (plain, whole))
    print("global_load_dword: plain", n_plain, "whole", n_whole)
    assert n_plain > 0 and n_whole < n_plain
    assert sum(p[0] == "global_load_dwordx2" for p in whole) == 16


def test_frame_loop_has_fewer_vector_and_scalar_instructions(asm):
    plain, whole = counts(frame_loop(asm, PLAIN)), counts(frame_loop(asm, WHOLE))
    print("plain", plain, "whole", whole)
    assert plain["valu"] > 500 and whole["valu"] > 500           # both spans hold the FFT
    assert whole["valu"] <= plain["valu"] - MIN_VALU_SAVED, (plain, whole)
    assert whole["salu"] < plain["salu"], (plain, whole)
