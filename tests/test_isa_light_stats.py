"""Compiler-output contract of csrc/light_stats.hip (hipcc cross-compiles gfx950 without a GPU), read from the kernel descriptors
only: every instance -- the tensor kernel for f16 / f32 input, plain / PQ, and the RGB48-codes kernel -- has a private segment of
zero bytes and no dynamic stack (no scratch), at most 64 VGPRs (eight waves per SIMD: eight 256-lane workgroups per CU) and a static
LDS size of at most 20 KiB (the 16 KiB histogram plus the reduction words; eight workgroups fit a CU's 160 KiB).  The assembly is
obtained the way tests/test_isa_contracts.py obtains it (the library's flags, -S --cuda-device-only)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _field(desc, name):
    m = re.search(r"\.amdhsa_%s (\d+)" % name, desc)
    return None if m is None else int(m.group(1))


def test_light_stats_kernels_fit_eight_workgroups_per_cu_without_scratch(tmp_path):
    out = tmp_path / "light_stats.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize",
                    "-fno-vectorize", "-S", "--cuda-device-only", os.path.join(CSRC, "light_stats.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    descriptors = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    tensor = sorted(n for n in descriptors if "18light_stats_kernel" in n)
    codes = sorted(n for n in descriptors if "rgb48_light_stats_kernel" in n)
    # <f16 | float, false | true> and the RGB48 source; nothing else is a kernel of this file
    assert len(tensor) == 4 and sum("DF16_" in n for n in tensor) == 2 and sum("IfLb" in n for n in tensor) == 2, tensor
    assert sum("Lb1E" in n for n in tensor) == 2 and sum("Lb0E" in n for n in tensor) == 2, tensor
    assert len(codes) == 1 and len(descriptors) == 5, sorted(descriptors)
    for n in tensor + codes:
        d = descriptors[n]
        assert _field(d, "private_segment_fixed_size") == 0, (n, _field(d, "private_segment_fixed_size"))
        assert _field(d, "uses_dynamic_stack") in (None, 0), n
        vgprs = _field(d, "next_free_vgpr")
        assert vgprs is not None and vgprs <= 64, (n, vgprs)
        lds = _field(d, "group_segment_fixed_size")
        assert lds is not None and 16 * 1024 <= lds <= 20 * 1024, (n, lds)
