"""ISA budget of the headline instance k_mel_pw<1024,16,false> in front of its first sample request (CPU test: hipcc
cross-compiles gfx950).  One frame per ticket on contiguous rows has wave-uniform geometry: the frame's start is computed
on the scalar unit and the samples are requested from two SGPR bases.
Span (a) of profiles/mel_pw_geometry_isa.md: kernel entry .. the first sample global_load (layout order)."""
import os
import re
import subprocess
import tempfile

import pytest

from conftest import REPO

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KERNEL = "_ZN3kpr8k_mel_pwILi1024ELi16ELb0EEEvPKfNS_4GeomES2_PK15HIP_vector_typeIfLj2EENS_6PwPlanENS_5DbDevEPjPfiiPx"
MAX_VALU_BEFORE_FIRST_REQUEST = 40     # 58 before the scalar fast path (span (a): 166 instructions -> 122)
MAX_SGPR_SPILLS = 23                   # no new spills (23 before the scalar fast path, 22 with it)


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


def _instrs(asm_text):
    i = asm_text.index("\n" + KERNEL + ":")
    body = asm_text[i:asm_text.index(".end_amdhsa_kernel", i)]
    out = []
    for line in body.splitlines()[1:]:
        s = line.strip()
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        out.append(s.split(None, 1))
    return out


def test_valu_before_first_sample_request(asm):
    ins = _instrs(asm)
    first = next(i for i, p in enumerate(ins) if p[0].startswith("global_load"))
    assert re.search(r", s\[\d+:\d+\]", ins[first][1]), "first request not from an SGPR base: %s" % " ".join(ins[first])
    assert not any(p[0].startswith("flat_") for p in ins[:first + 1])
    valu = sum(1 for p in ins[:first] if p[0].startswith("v_"))
    assert valu <= MAX_VALU_BEFORE_FIRST_REQUEST, "%d VALU instructions before the first sample request" % valu


def test_no_new_spills_no_scratch(asm):
    m = re.search(r"\.name:\s+%s\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_spill_count:\s+(\d+)\n"
                  r"(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)" % KERNEL, asm)
    assert m, "metadata of %s" % KERNEL
    scratch, sspill, vgpr, vspill = (int(g) for g in m.groups())
    assert scratch == 0 and vspill == 0
    assert sspill <= MAX_SGPR_SPILLS
    assert vgpr <= 128
