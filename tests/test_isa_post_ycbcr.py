"""Compiler-output contract of csrc/post_ycbcr.hip (hipcc cross-compiles gfx950 without a GPU): every kernel instance -- the fused
kernel for f16 / f32 input, plain / PQ, P010 / yuv420p10 / yuv422p10, and the RGB48-codes kernel for the three layouts -- runs
without scratch: a private segment of zero bytes and no scratch instruction.  The ISA is obtained the way
tests/test_isa_contracts.py obtains it (the library's flags, -S --cuda-device-only)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def test_post_ycbcr_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "post_ycbcr.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize",
                    "-fno-vectorize", "-DHDRTV_AB", "-S", "--cuda-device-only", os.path.join(CSRC, "post_ycbcr.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)}
    descriptors = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    fused = sorted(n for n in descriptors if "post_ycbcr10_kernel" in n)
    codes = sorted(n for n in descriptors if "rgb48_ycbcr10_kernel" in n)
    # <f16 | float, false | true, 0 | 1 | 2> and <0 | 1 | 2>
    assert len(fused) == 12 and sum("DF16_" in n for n in fused) == 6 and sum("Lb1E" in n for n in fused) == 6, fused
    assert all(sum("Li%dE" % f in n for n in fused) == 4 for f in range(3)), fused
    assert len(codes) == 3, codes
    for n in fused + codes:
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", descriptors[n])
        assert m and int(m.group(1)) == 0, (n, m and m.group(1))
        dyn = re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", descriptors[n])
        assert not dyn or int(dyn.group(1)) == 0, n
        assert n in bodies and "scratch_" not in bodies[n], n
