"""Compiler-output contract of csrc/post_ycbcr_dither.hip and csrc/post_deband.hip (hipcc cross-compiles gfx950 without a GPU): every
kernel instance -- the dithered fused kernel for f16 / f32 input, plain / PQ, P010 / yuv420p10 / yuv422p10, the dithered RGB48-codes
kernel for the three layouts, and the deband kernel -- runs without scratch: a private segment of zero bytes and no scratch
instruction.  The new instances carry their own names, so that tests/test_isa_post_ycbcr.py still counts post_ycbcr.hip's fifteen.
The ISA is obtained the way tests/test_isa_post_ycbcr.py obtains it (the library's flags, -S --cuda-device-only)."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "hdr-realtime-video-pipeline_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


def _kernels(tmp_path, name):
    """-> ({kernel: descriptor text}, {function: body text}) of csrc/<name>."""
    out = tmp_path / (name + ".s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize",
                    "-fno-vectorize", "-DHDRTV_AB", "-S", "--cuda-device-only", os.path.join(CSRC, name), "-o", str(out)],
                   check=True, capture_output=True)
    text = out.read_text()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M)}
    descriptors = {m.group(1): m.group(2) for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}
    return descriptors, bodies


def _assert_no_scratch(descriptors, bodies, names):
    for n in names:
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", descriptors[n])
        assert m and int(m.group(1)) == 0, (n, m and m.group(1))
        dyn = re.search(r"\.amdhsa_uses_dynamic_stack (\d+)", descriptors[n])
        assert not dyn or int(dyn.group(1)) == 0, n
        assert n in bodies and "scratch_" not in bodies[n], n


def test_dithered_conversions_use_no_scratch(tmp_path):
    descriptors, bodies = _kernels(tmp_path, "post_ycbcr_dither.hip")
    fused = sorted(n for n in descriptors if "post_ycc10_dither_kernel" in n)
    codes = sorted(n for n in descriptors if "rgb48_ycc10_dither_kernel" in n)
    assert len(descriptors) == 15 and len(fused) == 12 and len(codes) == 3, sorted(descriptors)
    # <f16 | float, false | true, 0 | 1 | 2> and <0 | 1 | 2>
    assert sum("DF16_" in n for n in fused) == 6 and sum("Lb1E" in n for n in fused) == 6, fused
    assert all(sum("Li%dE" % f in n for n in fused) == 4 for f in range(3)), fused
    assert all(sum("Li%dE" % f in n for n in codes) == 1 for f in range(3)), codes
    # none of them can be mistaken for an instance of post_ycbcr.hip
    assert not any("post_ycbcr10_kernel" in n or "rgb48_ycbcr10_kernel" in n for n in descriptors)
    _assert_no_scratch(descriptors, bodies, fused + codes)


def test_deband_kernel_uses_no_scratch_and_one_tile_of_lds(tmp_path):
    descriptors, bodies = _kernels(tmp_path, "post_deband.hip")
    assert sorted(descriptors) == [n for n in descriptors if "rgb48_deband_kernel" in n] and len(descriptors) == 1, sorted(descriptors)
    _assert_no_scratch(descriptors, bodies, list(descriptors))
    (n, d), = descriptors.items()
    lds = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", d)
    assert lds and int(lds.group(1)) == 64 * 160 * 3 * 2, lds and lds.group(1)      # (32 + 2 * 16) x (128 + 2 * 16) pixels of 6 bytes: two per CU
