"""Compiler-output contract of csrc/post_fsr.hip (hipcc cross-compiles gfx950 without a GPU), read from the kernel descriptors alone:
the file holds the eight instances of the fused FSR upscale -- f16 / f32 input, plain / PQ, RCAS off / on -- and nothing else; each
runs without scratch (a private segment of zero bytes, no dynamic stack) and in LDS small enough for three workgroups per CU; the
RCAS-off instances hold the u16 codes tile and nothing more.  The ISA is obtained the way tests/test_isa_post_scale_cas.py obtains
post_scale_cas.hip's, with the -ffp-contract=off the Makefile builds this file with."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

TH, TW = 32, 64                                           # PS_TH x PS_TW output pixels per workgroup
CODES_OFF = 3 * (TH + 3) * (TW + 3 + 1) * 2               # one source pixel before and two after on each axis, rows padded by one code
CODES_ON = 3 * (TH + 2 + 3) * (TW + 2 + 3 + 1) * 2        # the same around the tile and its one-pixel ring
EASU_ON = 3 * (TH + 2) * (TW + 2) * 4                     # the float32 EASU tile with its ring


def test_post_fsr_kernels_use_no_scratch_and_leave_room_for_three_workgroups(tmp_path):
    out = tmp_path / "post_fsr.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize",
                    "-fno-vectorize", "-ffp-contract=off", "-DHDRTV_AB", "-S", "--cuda-device-only", os.path.join(CSRC, "post_fsr.hip"),
                    "-o", str(out)], check=True, capture_output=True)
    text = out.read_text()
    descriptors = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    names = sorted(descriptors)
    # <T, PQ, RCAS> over f16 / float and both values of either switch
    assert len(names) == 8 and all("post_fsr_kernel" in n for n in names), names
    assert sum("DF16_" in n for n in names) == 4 and sum("IfLb" in n for n in names) == 4, names
    for tag in ("Lb0ELb0E", "Lb0ELb1E", "Lb1ELb0E", "Lb1ELb1E"):
        assert sum(tag in n for n in names) == 2, (tag, names)
    for n in names:
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", descriptors[n])
        assert m and int(m.group(1)) == 0, (n, m and m.group(1))
        dyn = re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", descriptors[n])
        assert not dyn or int(dyn.group(1)) == 0, n
        lds = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", descriptors[n])
        assert lds and int(lds.group(1)) <= 160 * 1024 // 3 == 54613, (n, lds and lds.group(1))
        rcas = "ELb1EEEv" in n                            # the last template argument
        assert int(lds.group(1)) == (CODES_ON + EASU_ON if rcas else CODES_OFF), (n, lds.group(1))
    assert CODES_OFF == 14280 and CODES_ON + EASU_ON == 42468
