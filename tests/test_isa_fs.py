"""Compiler-output contract of csrc/post_ycbcr_fs.hip (hipcc cross-compiles gfx950 without a GPU), read from the kernel descriptors
alone: the diffusion kernel and every instance of the samples pass run without scratch (a private segment of zero bytes), the
diffusion kernel's LDS is the size the file's header comment derives -- two staging buffers of FS_ROWS x (FS_CHUNK + 1) int32 and
one hand-over row of FS_CHUNK int32 per wave --, and the samples pass keeps the tile code's LDS.  The ISA is obtained the way
tests/test_isa_post_ycbcr.py obtains it (the library's flags, -S --cuda-device-only)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _field(descriptor, name):
    m = re.search(r"\.amdhsa_%s (\d+)" % name, descriptor)
    return int(m.group(1)) if m else None


def test_fs_kernels_use_no_scratch_and_the_derived_lds(tmp_path):
    from hdrtv_mi355x import lib as L
    out = tmp_path / "post_ycbcr_fs.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize",
                    "-fno-vectorize", "-S", "--cuda-device-only", os.path.join(CSRC, "post_ycbcr_fs.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    descriptors = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", out.read_text(), re.S)}
    diffuse = [n for n in descriptors if "fs_diffuse_kernel" in n]
    fused = [n for n in descriptors if "post_ycc10_fs_samples_kernel" in n]
    codes = [n for n in descriptors if "rgb48_ycc10_fs_samples_kernel" in n]
    # one diffusion kernel; samples: <f16 | float, plain | PQ, 4:2:0 | 4:2:2> and <4:2:0 | 4:2:2> (P010 shares the 4:2:0 instances)
    assert len(descriptors) == 11 and len(diffuse) == 1 and len(fused) == 8 and len(codes) == 2, sorted(descriptors)
    for n, d in descriptors.items():
        assert _field(d, "private_segment_fixed_size") == 0, n
        assert not _field(d, "uses_dynamic_stack"), n
    lds = 2 * L.FS_ROWS * (L.FS_CHUNK + 1) * 4 + (L.FS_ROWS // 64) * L.FS_CHUNK * 4
    assert lds == 68096 and _field(descriptors[diffuse[0]], "group_segment_fixed_size") == lds
    for n in fused + codes:
        assert _field(descriptors[n], "group_segment_fixed_size") == 3 * 17 * 136 * 2, n        # post_ycbcr.hip's codes[3][17][136] u16
