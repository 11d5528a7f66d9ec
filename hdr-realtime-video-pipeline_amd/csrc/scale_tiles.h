// scale_tiles.h -- the tile extents of the RGB48 scalers' kernels that the host needs too: plain C++, no HIP header, so that
// scale_tables.h (and a host-only test program) can include it.  common.h includes it for the kernels and their launchers.
#pragma once

// post_scale*.hip and post_fsr.hip: output pixels per workgroup
constexpr int PS_TW = 64, PS_TH = 32;
// post_down.hip: a workgroup owns DN_TH2 x DN_TW output pixels up to a ratio of 2 on both axes, DN_TH4 x DN_TW up to 4
constexpr int DN_TW = 32, DN_TH2 = 16, DN_TH4 = 8;
// post_ssimsr.hip: a workgroup owns SR_TH x SR_TW output pixels, SR_NT weights per source index; the extents of the regions it keeps
// in LDS (post_ssimsr.hip's header derives them): low-resolution positions, spline36 codes and source codes, with stage B / without
constexpr int SR_TW = 32, SR_TH = 16, SR_NT = 9;
constexpr int sr_nl(int t) { return t + 4; }                                  // low-resolution pixels: Lr
constexpr int sr_np(bool ssim, int t) { return ssim ? t + 18 : t; }           // spline36 codes
constexpr int sr_nc(bool ssim, int t) { return ssim ? t + 14 : t + 5; }       // source codes
