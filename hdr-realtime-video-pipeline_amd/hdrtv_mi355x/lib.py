"""ctypes binding of libhdrtv_mi355x.so (C ABI: include/hdrtv_mi355x.h).

There is no CPU fallback: if the shared library is missing, or the device is not
gfx950, construction raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C hdr-realtime-video-pipeline_amd/csrc``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import NamedTuple

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_PKG), "lib", "libhdrtv_mi355x.so")
# the A/B build (make AB=1): the same sources plus superseded kernels, for the GPU bit-identity tests only
LIB_PATH_AB = os.path.join(os.path.dirname(_PKG), "lib", "libhdrtv_mi355x_ab.so")

OK, EINVAL, EWEIGHTS, EHIP, ENOMEM, ESTATE = 0, -1, -2, -3, -4, -5
F16, F32 = 0, 1
PREC_F16, PREC_F32 = 0, 1
YUV_I420, YUV_NV12 = 0, 1                  # hdrtv_yuv420_to_bgr_u8 / hdrtv_preprocess_yuv420 layouts
YCC_P010, YCC_YUV420P10, YCC_YUV422P10 = 0, 1, 2   # hdrtv_post_ycbcr10 / hdrtv_rgb48_to_ycbcr10 / hdrtv_preprocess_ycbcr10 layouts
SITING_LEFT, SITING_TOPLEFT = 0, 1
DITHER_NONE, DITHER_ORDERED = 0, 1         # hdrtv_post_ycbcr10_ex / hdrtv_rgb48_to_ycbcr10_ex
DITHER_FS = 2                              # Floyd-Steinberg error diffusion: never an argument of the _ex entry points (hdrtv_*_fs instead)
FS_ROWS, FS_CHUNK = 256, 32                # csrc/common.h: the rows the diffusion kernel keeps in flight, its staging chunk in columns
DEBAND_RANGE_MAX, DEBAND_RANGE, DEBAND_THRESHOLD = 16, 16, 1311     # hdrtv_rgb48_deband: the largest range and the defaults
LIGHT_BINS, LIGHT_WORDS = 4096, 4104       # hdrtv_light_stats / hdrtv_rgb48_light_stats: the record, u32 words (lightlevel.py reads it)
FR_CROP, FR_NORMALIZED = 1, 2              # hdrtv_full_reference_metrics flags
FR_MAX_SIDE, FR_MAX_SHRINK = 512, 16       # the reference's evaluation size (_OBJECTIVE_METRIC_MAX_SIDE); the area reduction's largest ratio
# _compute_full_reference_metrics' obj_note (gui_objective_metrics.py:659-664), without / with its crop suffix
FR_NOTE = ("Computed (raw + normalized; PSNR/SSIM linear, DeltaEITP/HDR-VDP3 color-managed; DeltaEITP-N normalized pre-PQ{})")
FR_NOTE_CROPPED = "; shared black borders cropped"

# every symbol include/hdrtv_mi355x.h declares: (name, restype, argtypes)
_VP, _I, _SZ = C.c_void_p, C.c_int, C.c_size_t
SYMBOLS = [
    ("hdrtv_version", C.c_char_p, []),
    ("hdrtv_create", _I, [_VP, _SZ, _VP, _SZ, _I, C.POINTER(_VP)]),
    ("hdrtv_create_ex", _I, [_VP, _SZ, _VP, _SZ, _I, _I, C.POINTER(_VP)]),
    ("hdrtv_destroy", _I, [_VP]),
    ("hdrtv_has_hg", _I, [_VP]),
    ("hdrtv_set_hg_mask_r", _I, [_VP, C.c_float]),
    ("hdrtv_set_cond_mode", _I, [_VP, _I]),
    ("hdrtv_reserve", _I, [_VP, _I, _I]),
    ("hdrtv_preprocess", _I, [_VP, _VP, _VP, _I, _I, _VP, _VP]),
    ("hdrtv_infer", _I, [_VP, _VP, _VP, _VP, _I, _I, _VP, _I, _VP]),
    ("hdrtv_set_lanes", _I, [_VP, _I]),
    ("hdrtv_get_lanes", _I, [_VP]),
    ("hdrtv_infer_lane", _I, [_VP, _I, _VP, _VP, _VP, _I, _I, _VP, _I, _VP]),
    ("hdrtv_post_u8", _I, [_VP, _VP, _VP, _I, _I, _I, _VP]),
    ("hdrtv_post_rgb48", _I, [_VP, _VP, _VP, _I, _I, _I, _VP]),
    ("hdrtv_post_pq_rgb48", _I, [_VP, _VP, _VP, _I, _I, _I, C.c_float, _VP]),
    ("hdrtv_post_rgb48_scaled", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, _I, _I]),
    ("hdrtv_post_rgb48_scaled_ex", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, _I, _I, _I]),
    ("hdrtv_post_rgb48_scaled_cas", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, _I, _I, _I, _I]),
    ("hdrtv_post_rgb48_fsr", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, _I, _I, _I, C.c_float]),
    ("hdrtv_post_rgb48_down", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, _I, _I, _I, _I]),
    ("hdrtv_post_rgb48_ssimsr", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, _I, _I, _I]),
    ("hdrtv_film_grain_seed", C.c_float, [C.c_uint32, C.c_uint32]),
    ("hdrtv_rgb48_film_grain", _I, [_VP, _VP, _VP, _I, _I, C.c_float, C.c_float, _VP]),
    ("hdrtv_post_rgb48_grain", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, C.c_float, C.c_float]),
    ("hdrtv_post_rgb48_scaled_grain", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, _I, _I, _I, _I, C.c_float, C.c_float]),
    ("hdrtv_post_rgb48_fsr_grain", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, _I, _I, _I, C.c_float, C.c_float, C.c_float]),
    ("hdrtv_pq_eotf_table", _I, [_VP]),
    ("hdrtv_rgb48_tonemap", _I, [_VP, _VP, _VP, _I, _I, _VP, _VP]),
    ("hdrtv_post_rgb48_tonemap", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _VP, _VP]),
    ("hdrtv_post_ycbcr10", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _I, _I, _VP, _I, _VP, _VP, _I]),
    ("hdrtv_rgb48_to_ycbcr10", _I, [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _I, _VP, _VP, _I]),
    ("hdrtv_ycbcr10_bytes", C.c_int64, [_I, _I, _I]),
    ("hdrtv_rgb48_deband", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_uint32, _VP]),
    ("hdrtv_post_ycbcr10_ex", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _I, _I, _VP, _I, _VP, _VP, _I, _I]),
    ("hdrtv_rgb48_to_ycbcr10_ex", _I, [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _I, _VP, _VP, _I, _I]),
    ("hdrtv_ycbcr10_fs_scratch_bytes", C.c_int64, [_I, _I, _I]),
    ("hdrtv_post_ycbcr10_fs", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _I, _I, _VP, _I, _VP, _VP, _I, _VP]),
    ("hdrtv_rgb48_to_ycbcr10_fs", _I, [_VP, _VP, _VP, _I, _I, _I, _I, _VP, _I, _VP, _VP, _I, _VP]),
    ("hdrtv_light_stats", _I, [_VP, _VP, _VP, _I, _I, _I, _I, C.c_float, _I, _I, _I, _I, _VP]),
    ("hdrtv_rgb48_light_stats", _I, [_VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP]),
    ("hdrtv_letterbox_u8", _I, [_VP, _VP, _VP, _I, _I, _VP, _I, _I]),
    ("hdrtv_yuv420_to_bgr_u8", _I, [_VP, _VP, _VP, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP]),
    ("hdrtv_preprocess_yuv420", _I, [_VP, _VP, _VP, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP]),
    ("hdrtv_ycbcr10_to_rgb10", _I, [_VP, _VP, _VP, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP]),
    ("hdrtv_preprocess_ycbcr10", _I, [_VP, _VP, _VP, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _VP]),
    ("hdrtv_letterbox_ycbcr10", _I, [_VP, _VP, _VP, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _I, _I]),
    ("hdrtv_preprocess_ycbcr10_letterboxed", _I, [_VP, _VP, _VP, _I, _VP, _VP, _I, _I, _I, _I, _I, _I, _I, _I, _VP, _VP]),
    ("hdrtv_metrics", _I, [_VP, _VP, _VP, _VP, _I, _I, _I, C.c_float, C.POINTER(C.c_double)]),
    ("hdrtv_full_reference_metrics", _I, [_VP, _VP, _VP, _VP, _I, _I, _I, C.c_float, _I, C.POINTER(C.c_double), C.POINTER(_I)]),
    ("hdrtv_rgb48_border_counts", _I, [_VP, _VP, _VP, _VP, _I, _I, _VP]),
    ("hdrtv_rgb48_area_reduce", _I, [_VP, _VP, _VP, _I, _I, _I, _I, _I, _I, _VP, _I, _I]),
    ("hdrtv_rgb48_grade_match", _I, [_VP, _VP, _VP, _VP, _I, _I, C.c_float, C.POINTER(C.c_float)]),
    ("hdrtv_ring_create", _I, [_VP, _I, _I, _I]),
    ("hdrtv_ring_acquire", _I, [_VP, _I, C.POINTER(_VP), C.POINTER(_VP)]),
    ("hdrtv_ring_commit", _I, [_VP, _I, _VP]),
    ("hdrtv_ring_commit_bytes", _I, [_VP, _I, _VP, _SZ]),
    ("hdrtv_ring_wait", _I, [_VP, _I]),
    ("hdrtv_ring_release", _I, [_VP, _I]),
    ("hdrtv_ring_destroy", _I, [_VP]),
    ("hdrtv_get_tap", _I, [_VP, C.c_char_p, C.POINTER(_VP), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    ("hdrtv_infer_stats", _I, [_VP, C.POINTER(_I), C.POINTER(C.c_double)]),
    ("hdrtv_profile_enable", _I, [_VP, _I]),
    ("hdrtv_profile_get", _I, [_VP, _I, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_float),
                               C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    ("hdrtv_profile_tiles", _I, [_VP, _I, C.POINTER(_I), C.POINTER(_I)]),
    ("hdrtv_set_variant", _I, [_VP, C.c_char_p, _I]),
    ("hdrtv_get_variant", _I, [_VP, C.c_char_p, C.POINTER(_I)]),
    ("hdrtv_last_error", C.c_char_p, [_VP]),
]

# output pixel formats of the frame path: "rgb48le" (6 bytes per pixel, the default) and the 10-bit Y'CbCr layouts
YCC_FORMATS = {"p010le": YCC_P010, "yuv420p10le": YCC_YUV420P10, "yuv422p10le": YCC_YUV422P10}
YCC_SITINGS = {"left": SITING_LEFT, "topleft": SITING_TOPLEFT}
OUT_PIX_FMTS = ("rgb48le",) + tuple(YCC_FORMATS)


def check_out_format(pix_fmt, siting="left"):
    """Validates an output format / chroma siting pair; returns them lower-cased."""
    pix_fmt, siting = str(pix_fmt).lower(), str(siting).lower()
    if pix_fmt not in OUT_PIX_FMTS:
        raise ValueError(f"out_pix_fmt must be one of {list(OUT_PIX_FMTS)}")
    if siting not in YCC_SITINGS:
        raise ValueError(f"out_siting must be one of {sorted(YCC_SITINGS)}")
    if pix_fmt == "yuv422p10le" and siting != "left":
        raise ValueError("4:2:2 chroma is horizontally co-sited: out_siting must be 'left'")
    return pix_fmt, siting


class OutputFormat(NamedTuple):
    """What a sink receives per frame: the pixel format, the 4:2:0 chroma siting and the size the frame is delivered at.  Built by
    ``output_format`` (which validates); a plain tuple, so it crosses into the dispatcher's worker processes as it is."""
    pix_fmt: str
    siting: str
    h: int
    w: int

    @property
    def is_rgb48(self):
        return self.pix_fmt == "rgb48le"

    @property
    def nbytes(self):
        """Bytes of one contiguous frame: H * W * 6 for rgb48le, hdrtv_ycbcr10_bytes' formula for the Y'CbCr layouts (3 H W for
        the two 4:2:0 layouts, 4 H W for 4:2:2)."""
        return self.h * self.w * (6 if self.is_rgb48 else 4 if self.pix_fmt == "yuv422p10le" else 3)

    @property
    def shape(self):
        """The frame as a u16 array: RGB48 (h, w, 3), or the 10-bit Y'CbCr planes back to back, 1-D."""
        return (self.h, self.w, 3) if self.is_rgb48 else (self.nbytes // 2,)

    def at(self, h, w):
        """The same format at another size."""
        return self if (h, w) == (self.h, self.w) else output_format(self.pix_fmt, self.siting, h, w)

    def planes(self, ptr):
        """The trailing arguments of hdrtv_post_ycbcr10 / hdrtv_rgb48_to_ycbcr10 for a frame whose planes lie back to back at
        device address ``ptr`` at their minimum pitches: (fmt, siting, dst_y, y_pitch, dst_u, dst_v, c_pitch)."""
        if self.is_rgb48:
            raise ValueError("rgb48le has no Y'CbCr planes")
        fmt, sit, h, w = YCC_FORMATS[self.pix_fmt], YCC_SITINGS[self.siting], self.h, self.w
        u = ptr + h * w * 2
        if fmt == YCC_P010:
            return fmt, sit, ptr, 2 * w, u, None, 2 * w
        ch = h if fmt == YCC_YUV422P10 else h // 2
        return fmt, sit, ptr, 2 * w, u, u + ch * w, w


def output_format(pix_fmt, siting, h, w):
    """The one constructor of ``OutputFormat``: known names, 4:2:2 only with ``left`` (``check_out_format``), and W even, H even
    for 4:2:0, for the Y'CbCr layouts."""
    pix_fmt, siting = check_out_format(pix_fmt, siting)
    h, w = int(h), int(w)
    if pix_fmt != "rgb48le" and (h <= 0 or w <= 0 or w % 2 or (pix_fmt != "yuv422p10le" and h % 2)):
        raise ValueError(f"{pix_fmt} needs an even width{'' if pix_fmt == 'yuv422p10le' else ' and height'} (got {w}x{h})")
    return OutputFormat(pix_fmt, siting, h, w)


YCBCR10_IN_FORMATS = dict(YCC_FORMATS)      # the 10-bit input pixel formats: the names and codes of the output side
YUV_LAYOUTS = {"i420": YUV_I420, "yuv420p": YUV_I420, "nv12": YUV_NV12}      # the 8-bit 4:2:0 input formats ("i420" = "yuv420p")
IN_PIX_FMTS = ("bgr24",) + tuple(YUV_LAYOUTS) + tuple(YCBCR10_IN_FORMATS)


class InputFormat(NamedTuple):
    """What a source delivers per frame, the twin of ``OutputFormat``: the pixel format and, for Y'CbCr, the matrix (601 / 709 /
    2020) and range it converts with.  Built by ``input_format`` (which validates); a plain tuple, so it crosses into the
    dispatcher's worker processes as it is.  It knows its family -- ``bgr24``, ``yuv420`` (8-bit 4:2:0: i420 / yuv420p / nv12) or
    ``ycbcr10`` (p010le / yuv420p10le / yuv422p10le) --, the array a frame is held as, and the C entry point that reads it."""
    pix_fmt: str
    matrix: int = 709
    full_range: bool = False

    @property
    def family(self):
        return "bgr24" if self.pix_fmt == "bgr24" else "yuv420" if self.pix_fmt in YUV_LAYOUTS else "ycbcr10"

    @property
    def dtype(self):
        """u16 samples for the 10-bit formats, bytes for the others."""
        return np.uint16 if self.family == "ycbcr10" else np.uint8

    @property
    def entry(self):
        """The C preprocess entry point that serves the format (its ``_letterboxed`` form, where there is one, adds the suffix)."""
        return {"bgr24": "hdrtv_preprocess", "yuv420": "hdrtv_preprocess_yuv420", "ycbcr10": "hdrtv_preprocess_ycbcr10"}[self.family]

    @property
    def kwargs(self):
        """The keyword arguments of the family's public processor methods (``preprocess_yuv420(frame, layout=...)``,
        ``preprocess_ycbcr10(frame, pix_fmt=...)``)."""
        name = {"yuv420": "layout", "ycbcr10": "pix_fmt"}[self.family]
        return {name: self.pix_fmt, "matrix": self.matrix, "full_range": self.full_range}

    def _what(self):
        c422 = self.pix_fmt == "yuv422p10le"
        return f"a {self.pix_fmt} frame must be {np.dtype(self.dtype).name} " + \
            ("[H, W, 3]" if self.family == "bgr24" else f"[{'2*H' if c422 else 'H*3//2'}, W]")

    def frame_shape(self, h, w):
        """The array shape of an ``h`` x ``w`` frame: BGR ``(h, w, 3)``, or the planes back to back at minimum pitch, ``(h*3//2, w)``
        for 4:2:0 and ``(2*h, w)`` for ``yuv422p10le``.  Y'CbCr: W even; H even for 4:2:0."""
        h, w = int(h), int(w)
        if self.family == "bgr24":
            return (h, w, 3)
        c422 = self.pix_fmt == "yuv422p10le"
        if h <= 0 or w <= 0 or w % 2 or (not c422 and h % 2):
            raise ValueError(f"{self.pix_fmt} needs an even width{'' if c422 else ' and height'} (got {w}x{h})")
        return (2 * h, w) if c422 else (h * 3 // 2, w)

    def frame_hw(self, frame):
        """(H, W) of a frame held as the array of ``frame_shape``."""
        nd = 3 if self.family == "bgr24" else 2
        if getattr(frame, "ndim", 0) != nd or str(frame.dtype) != np.dtype(self.dtype).name:
            raise ValueError(self._what())
        rows, w = frame.shape[0], frame.shape[1]
        h = rows if nd == 3 else rows // 2 if self.pix_fmt == "yuv422p10le" else rows // 3 * 2
        if tuple(frame.shape) != self.frame_shape(h, w):
            raise ValueError(self._what())
        return h, w

    def planes(self, ptr, h, w):
        """The leading arguments of the C entry points for a frame whose planes lie back to back at device address ``ptr`` at their
        minimum pitches: ``(ptr,)`` for BGR, else (y, y_pitch, u, v, c_pitch, layout, matrix, full_range)."""
        self.frame_shape(h, w)                                 # raises for a size the format does not have
        h, w = int(h), int(w)
        if self.family == "bgr24":
            return (ptr,)
        b = np.dtype(self.dtype).itemsize
        code = YUV_LAYOUTS[self.pix_fmt] if b == 1 else YCBCR10_IN_FORMATS[self.pix_fmt]
        u, tail = ptr + h * w * b, (code, self.matrix, int(self.full_range))
        if self.pix_fmt in ("nv12", "p010le"):                 # CbCr interleaved in one plane
            return (ptr, w * b, u, None, w * b) + tail
        ch = h if self.pix_fmt == "yuv422p10le" else h // 2
        return (ptr, w * b, u, u + ch * (w // 2) * b, (w // 2) * b) + tail


def input_format(pix_fmt, matrix=709, full_range=False):
    """The one constructor of ``InputFormat``: a known name and a known matrix."""
    pix_fmt = str(pix_fmt).lower()
    if pix_fmt not in IN_PIX_FMTS:
        raise ValueError(f"pix_fmt must be one of {list(IN_PIX_FMTS)}")
    if int(matrix) not in (601, 709, 2020):
        raise ValueError("matrix must be 601, 709 or 2020")
    return InputFormat(pix_fmt, int(matrix), bool(full_range))


def ycbcr10_frame_shape(pix_fmt, h, w):
    """``InputFormat.frame_shape`` of a 10-bit ``pix_fmt``."""
    if pix_fmt not in YCBCR10_IN_FORMATS:
        raise ValueError(f"pix_fmt must be one of {sorted(YCBCR10_IN_FORMATS)}")
    return InputFormat(pix_fmt).frame_shape(h, w)


def ycbcr10_frame_hw(frame, pix_fmt):
    """``InputFormat.frame_hw`` of a 10-bit ``pix_fmt``."""
    if pix_fmt not in YCBCR10_IN_FORMATS:
        raise ValueError(f"pix_fmt must be one of {sorted(YCBCR10_IN_FORMATS)}")
    return InputFormat(pix_fmt).frame_hw(frame)


def out_frame_bytes(pix_fmt, h, w):
    """``OutputFormat.nbytes`` of a ``pix_fmt`` frame of ``h`` x ``w``."""
    return output_format(pix_fmt, "left", h, w).nbytes


def ycbcr10_planes(ptr, h, w, pix_fmt, siting="left"):
    """``OutputFormat.planes`` of a ``pix_fmt`` / ``siting`` frame of ``h`` x ``w`` at device address ``ptr``."""
    return output_format(pix_fmt, siting, h, w).planes(ptr)


DITHERS = {"none": DITHER_NONE, "ordered": DITHER_ORDERED, "floyd_steinberg": DITHER_FS}


class OutputCleanup(NamedTuple):
    """The picture-quality steps of the output stage, off by default: debanding of the RGB48 codes
    (``hdrtv_rgb48_deband`` with ``deband_range`` / ``deband_threshold``) and the dither of the 10-bit Y'CbCr conversion (``"none"``,
    ``"ordered"`` or ``"floyd_steinberg"``).  Built by ``output_cleanup`` (which validates); it travels beside ``OutputFormat``, a plain tuple that
    crosses into the dispatcher's worker processes as it is."""
    deband: bool
    deband_range: int
    deband_threshold: int
    dither: str

    @property
    def active(self):
        return self.deband or self.dither != "none"

    @property
    def dither_code(self):
        return DITHERS[self.dither]

    @property
    def error_diffusion(self):
        """The dither is Floyd-Steinberg error diffusion: the ``hdrtv_*_fs`` entry points and their scratch, not the ``_ex`` ones."""
        return self.dither == "floyd_steinberg"


def _int_in(name, v, lo, hi):
    if isinstance(v, bool) or not hasattr(v, "__index__"):          # an integer type (numpy's included), not a float or a string
        raise ValueError(f"{name} must be an integer in {lo} .. {hi} (got {v!r})")
    v = int(v)
    if not lo <= v <= hi:
        raise ValueError(f"{name} must be in {lo} .. {hi} (got {v})")
    return v


def output_cleanup(deband=False, deband_range=DEBAND_RANGE, deband_threshold=DEBAND_THRESHOLD, dither="none", pix_fmt=None):
    """The one constructor of ``OutputCleanup``: ``deband_range`` 1 .. 16 pixels, ``deband_threshold`` 1 .. 65535 u16 code units,
    ``dither`` ``"none"``, ``"ordered"`` (a 16 x 16 Bayer threshold) or ``"floyd_steinberg"`` (error diffusion).  ``pix_fmt`` (when
    given): the output format the cleanup goes with -- 16-bit codes are not dithered, so a dither with ``rgb48le`` is refused."""
    if not isinstance(deband, (bool, int)) or deband not in (0, 1):
        raise ValueError(f"deband must be True or False (got {deband!r})")
    dither = str(dither).lower() if isinstance(dither, str) else dither
    if dither not in DITHERS:
        raise ValueError(f"dither must be one of {sorted(DITHERS)} (got {dither!r})")
    if pix_fmt is not None and dither != "none" and str(pix_fmt).lower() == "rgb48le":
        raise ValueError("dither applies to the 10-bit Y'CbCr formats: rgb48le (16-bit codes) is not dithered")
    return OutputCleanup(bool(deband), _int_in("deband_range", deband_range, 1, DEBAND_RANGE_MAX),
                         _int_in("deband_threshold", deband_threshold, 1, 65535), dither)


ANTIRING_ONE = 256                         # hdrtv_post_rgb48_scaled_ex: the code of full strength


def antiring_code(value):
    """The ``antiring`` argument of ``hdrtv_post_rgb48_scaled_ex`` for a strength in [0, 1]: ``floor(value * 256 + 0.5)``, 0 .. 256.
    ``ValueError`` for anything that is not such a number (a bool, a string -- ``"auto"`` is resolved by ``resolve_antiring``
    where the two sizes are known --, None, NaN, a value outside the range)."""
    if isinstance(value, (bool, str, bytes)) or value is None:
        raise ValueError(f"antiring must be a number in [0, 1] (got {value!r})")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"antiring must be a number in [0, 1] (got {value!r})") from None
    if not 0.0 <= v <= 1.0:                  # NaN fails both comparisons
        raise ValueError(f"antiring must be in [0, 1] (got {value!r})")
    return int(v * ANTIRING_ONE + 0.5)


def check_antiring(value):
    """An ``antiring`` option as the worker, the dispatcher and the command line take it: ``"auto"`` (any case) -> ``"auto"``, a
    strength in [0, 1] -> that float; ``ValueError`` otherwise."""
    if isinstance(value, str) and value.lower() == "auto":
        return "auto"
    antiring_code(value)
    return float(value)


def scale_antiring(proc_w, proc_h, out_w, out_h):
    """The reference's anti-ringing strength for a separable Lanczos kernel (gui_scaling.py:82-111, 150-162: what it hands mpv as
    ``scale-antiring`` in its lower-resolution processing mode): 0.0 unless both axes are enlarged, else 0.30 for a processing
    size of at most 960x540 (either extent), 0.22 up to 1280x720, 0.10 above."""
    proc_w, proc_h, out_w, out_h = int(proc_w), int(proc_h), int(out_w), int(out_h)
    if not (out_w > proc_w and out_h > proc_h):
        return 0.0
    if proc_h <= 540 or proc_w <= 960:
        return 0.30
    if proc_h <= 720 or proc_w <= 1280:
        return 0.22
    return 0.10


def resolve_antiring(value, proc_w, proc_h, out_w, out_h):
    """``check_antiring``'s result for a frame of known sizes -> a strength in [0, 1]: ``"auto"`` through ``scale_antiring``."""
    value = check_antiring(value)
    return scale_antiring(proc_w, proc_h, out_w, out_h) if value == "auto" else value


CAS_CODE_MIN, CAS_CODE_MAX = 1032, 4096    # hdrtv_post_rgb48_scaled_cas: the CAS codes it takes beside 0 = off


def cas_code(value):
    """The ``cas`` argument of ``hdrtv_post_rgb48_scaled_cas`` for a sharpening strength in [0, 1] (ffmpeg's ``cas=<strength>``):
    with ``c = floor(value * 256 + 0.5)``, 0 (off) for ``c == 0``, else ``K = 4096 - ((c * 3064 + 128) >> 8)``, 1032 .. 4084 --
    ``K / 256`` is the filter's ``lerp(16, 4.03, strength)``.  The reference's 0.22 / 0.20 / 0.16 are 3426 / 3486 / 3605.
    ``ValueError`` for anything that is not such a number (a bool, a string -- ``"auto"`` is resolved by ``resolve_cas`` where
    the two sizes are known --, None, NaN, a value outside the range)."""
    if isinstance(value, (bool, str, bytes)) or value is None:
        raise ValueError(f"cas must be a number in [0, 1] (got {value!r})")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"cas must be a number in [0, 1] (got {value!r})") from None
    if not 0.0 <= v <= 1.0:                  # NaN fails both comparisons
        raise ValueError(f"cas must be in [0, 1] (got {value!r})")
    c = int(v * 256 + 0.5)
    return 0 if c == 0 else 4096 - ((c * 3064 + 128) >> 8)


def check_cas(value):
    """A ``cas`` option as the worker, the dispatcher and the command line take it: ``"auto"`` (any case) -> ``"auto"``, a
    strength in [0, 1] -> that float; ``ValueError`` otherwise."""
    if isinstance(value, str) and value.lower() == "auto":
        return "auto"
    cas_code(value)
    return float(value)


def scale_cas(proc_w, proc_h, out_w, out_h):
    """The reference's sharpening strength for a separable Lanczos kernel (``_select_mpv_cas_strength``, gui_scaling.py:114-138: what
    it appends as ``cas=`` to the filter chain of its HDR frames when it upscales without its FSR shader): 0.0 unless both axes are
    enlarged, else 0.22 for a processing size of at most 960x540 (either extent), 0.20 up to 1280x720, 0.16 above."""
    proc_w, proc_h, out_w, out_h = int(proc_w), int(proc_h), int(out_w), int(out_h)
    if not (out_w > proc_w and out_h > proc_h):
        return 0.0
    if proc_h <= 540 or proc_w <= 960:
        return 0.22
    if proc_h <= 720 or proc_w <= 1280:
        return 0.20
    return 0.16


def resolve_cas(value, proc_w, proc_h, out_w, out_h):
    """``check_cas``'s result for a frame of known sizes -> a strength in [0, 1]: ``"auto"`` through ``scale_cas``."""
    value = check_cas(value)
    return scale_cas(proc_w, proc_h, out_w, out_h) if value == "auto" else value


SCALERS = ("lanczos", "fsr")               # what enlarges a frame to the delivered size: the fused Lanczos passes, or hdrtv_post_rgb48_fsr
FSR_MAX_RATIO = 2                          # hdrtv_post_rgb48_fsr: the largest ratio per axis (the shader's EASU stage stops there)
FSR_SHARPNESS = 0.2                        # the reference's RCAS sharpness (0 = the sharpest, 2 = the mildest)
# every enlarging choice: the two above, and hdrtv_post_rgb48_ssimsr without ("spline36") / with ("ssim_superres", the reference's
# third upscaler) its SSimSuperRes stage
UPSCALERS = SCALERS + ("spline36", "ssim_superres")
SSIMSR_SCALERS = UPSCALERS[len(SCALERS):]
SSIMSR_MAX_RATIO = 2                       # hdrtv_post_rgb48_ssimsr: the largest ratio per axis


def check_scaler(value="lanczos"):
    """A ``scaler`` option as the processor, the worker, the dispatcher and the command line take it: ``"lanczos"`` (the default: the
    fused Lanczos upscale with its ``antiring`` and ``cas``), ``"fsr"`` (``hdrtv_post_rgb48_fsr``, the reference's default),
    ``"spline36"`` or ``"ssim_superres"`` (``hdrtv_post_rgb48_ssimsr`` with ``ssim`` 0 / 1), any case; ``ValueError`` otherwise."""
    if not isinstance(value, str) or value.lower() not in UPSCALERS:
        raise ValueError(f"scaler must be one of {list(UPSCALERS)} (got {value!r})")
    return value.lower()


def check_fsr_sharpness(value):
    """An ``fsr_sharpness`` option: ``None`` = EASU alone (``rcas = 0``), else the RCAS sharpness, a float in [0, 2] (0 = the
    sharpest; the reference's 0.2).  ``ValueError`` for anything else (a bool, a string, NaN, a value outside the range)."""
    if value is None:
        return None
    if isinstance(value, (bool, str, bytes)):
        raise ValueError(f"fsr_sharpness must be None or a number in [0, 2] (got {value!r})")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"fsr_sharpness must be None or a number in [0, 2] (got {value!r})") from None
    if not 0.0 <= v <= 2.0:                  # NaN fails both comparisons
        raise ValueError(f"fsr_sharpness must be in [0, 2] (got {value!r})")
    return v


def check_fsr_size(proc_w, proc_h, out_w, out_h):
    """``ValueError`` unless ``hdrtv_post_rgb48_fsr`` takes the two sizes: not below the processing size and at most
    ``FSR_MAX_RATIO`` times it on either axis."""
    proc_w, proc_h, out_w, out_h = int(proc_w), int(proc_h), int(out_w), int(out_h)
    if out_w < proc_w or out_h < proc_h:
        raise ValueError(f"output size {out_w}x{out_h} is below the processing size {proc_w}x{proc_h} (enlarging only)")
    if out_w > FSR_MAX_RATIO * proc_w or out_h > FSR_MAX_RATIO * proc_h:
        raise ValueError(f"scaler 'fsr' enlarges by at most {FSR_MAX_RATIO}x per axis: {proc_w}x{proc_h} -> {out_w}x{out_h} is more "
                         f"(the limit is {FSR_MAX_RATIO * proc_w}x{FSR_MAX_RATIO * proc_h})")


def check_ssimsr_size(proc_w, proc_h, out_w, out_h):
    """``ValueError`` unless ``hdrtv_post_rgb48_ssimsr`` takes the two sizes: equal to the processing size (nothing is enlarged), or
    above it on BOTH axes and at most ``SSIMSR_MAX_RATIO`` times it on either."""
    proc_w, proc_h, out_w, out_h = int(proc_w), int(proc_h), int(out_w), int(out_h)
    if out_w < proc_w or out_h < proc_h:
        raise ValueError(f"output size {out_w}x{out_h} is below the processing size {proc_w}x{proc_h} (enlarging only)")
    if out_w > SSIMSR_MAX_RATIO * proc_w or out_h > SSIMSR_MAX_RATIO * proc_h:
        raise ValueError(f"scalers 'spline36' and 'ssim_superres' enlarge by at most {SSIMSR_MAX_RATIO}x per axis: {proc_w}x{proc_h} -> "
                         f"{out_w}x{out_h} is more (the limit is {SSIMSR_MAX_RATIO * proc_w}x{SSIMSR_MAX_RATIO * proc_h})")
    if (out_w == proc_w) != (out_h == proc_h):
        raise ValueError(f"scalers 'spline36' and 'ssim_superres' enlarge both axes: {proc_w}x{proc_h} -> {out_w}x{out_h} leaves one "
                         f"at identity (the limit is {SSIMSR_MAX_RATIO}x per axis)")


def scaler_options(scaler, antiring=0.0, cas=0.0):
    """``antiring`` and ``cas`` as they hold under ``scaler`` -> ``(antiring, cas)``, each checked.  ``"lanczos"``: unchanged.
    ``"fsr"``: the reference's schedules give 0 for both when its FSR shader does the enlargement (up to 2x), so ``"auto"`` resolves to
    0.0 here; an explicit nonzero value belongs to the Lanczos scaler and is a ``ValueError``.  ``"spline36"`` and
    ``"ssim_superres"`` likewise: the reference sets scale-antiring = 0 and cas = 0 beside its SSimSuperRes shader."""
    scaler, antiring, cas = check_scaler(scaler), check_antiring(antiring), check_cas(cas)
    if scaler == "lanczos":
        return antiring, cas
    for name, v in (("antiring", antiring), ("cas", cas)):
        if v != "auto" and v != 0:
            raise ValueError(f"{name}={v!r} belongs to scaler 'lanczos': scaler {scaler!r} takes 0 or 'auto' (which is 0)")
    return 0.0, 0.0


DOWNSCALERS = ("mitchell", "ssim")         # what shrinks a frame to the delivered size: hdrtv_post_rgb48_down without / with its SSimDownscaler stage
DOWN_MAX_RATIO = 4                         # hdrtv_post_rgb48_down: the largest ratio per axis
DOWN_ANTIRING = 0.20                       # the reference's dscale-antiring (gui_mpv_widget.py _mpv_downscale_antiring)


def check_downscaler(value=None):
    """A ``downscaler`` option as the processor, the worker, the dispatcher and the command line take it: ``None`` (the default: a
    delivered size below the processing size stays a ``ValueError``), ``"mitchell"`` (``hdrtv_post_rgb48_down`` with ``ssim = 0``) or
    ``"ssim"`` (the reference's chain: Mitchell, then its SSimDownscaler shader), any case; ``ValueError`` otherwise."""
    if value is None:
        return None
    if not isinstance(value, str) or value.lower() not in DOWNSCALERS:
        raise ValueError(f"downscaler must be None or one of {list(DOWNSCALERS)} (got {value!r})")
    return value.lower()


def check_down_antiring(value=0.0):
    """A ``down_antiring`` option: ``"auto"`` (any case) -> the reference's ``DOWN_ANTIRING``, a strength in [0, 1] -> that float;
    ``ValueError`` otherwise.  Unlike the enlarging ``antiring`` the reference's value does not depend on the sizes."""
    value = check_antiring(value)
    return DOWN_ANTIRING if value == "auto" else value


def check_down_size(proc_w, proc_h, out_w, out_h):
    """``ValueError`` unless ``hdrtv_post_rgb48_down`` has something to do with the two sizes: no axis above the processing size (a
    mixed request, one axis up and one down, included), none below a ``DOWN_MAX_RATIO``-th of it, and at least one axis below it."""
    proc_w, proc_h, out_w, out_h = int(proc_w), int(proc_h), int(out_w), int(out_h)
    if out_w < 1 or out_h < 1:
        raise ValueError(f"output size {out_w}x{out_h} is not positive")
    if out_w > proc_w or out_h > proc_h:
        what = "one axis up and one down" if out_w < proc_w or out_h < proc_h else "enlarging"
        raise ValueError(f"a downscaler shrinks: {proc_w}x{proc_h} -> {out_w}x{out_h} is {what}")
    if DOWN_MAX_RATIO * out_w < proc_w or DOWN_MAX_RATIO * out_h < proc_h:
        raise ValueError(f"a downscaler shrinks by at most {DOWN_MAX_RATIO}x per axis: {proc_w}x{proc_h} -> {out_w}x{out_h} is more")
    if out_w == proc_w and out_h == proc_h:
        raise ValueError(f"a downscaler applies to a shrunk frame: the output size equals the processing size {proc_w}x{proc_h}")


def down_options(downscaler, down_antiring, proc_w, proc_h, out_w, out_h, scaler="lanczos", antiring=0.0, cas=0.0):
    """The ``downscaler`` / ``down_antiring`` options of a frame of known sizes -> None (no downscaler: everything as before, a
    smaller output size refused where it was), or ``(antiring code, ssim)`` as ``hdrtv_post_rgb48_down`` takes them, after the
    checks: the sizes (``check_down_size``), and that nothing of the enlarging path came along -- ``scaler`` must be ``"lanczos"``
    and ``antiring`` / ``cas`` 0 or ``"auto"`` (which is 0 unless both axes are enlarged).  An explicit nonzero ``down_antiring``
    without a downscaler is a ``ValueError`` too."""
    downscaler, strength = check_downscaler(downscaler), check_down_antiring(down_antiring)
    if downscaler is None:
        if strength != 0 and not (isinstance(down_antiring, str) and down_antiring.lower() == "auto"):
            raise ValueError(f"down_antiring={down_antiring!r} needs a downscaler")
        return None
    check_down_size(proc_w, proc_h, out_w, out_h)
    if check_scaler(scaler) != "lanczos":
        raise ValueError(f"scaler {scaler!r} enlarges: it does not go with downscaler {downscaler!r}")
    for name, v in (("antiring", check_antiring(antiring)), ("cas", check_cas(cas))):
        if v != "auto" and v != 0:
            raise ValueError(f"{name}={v!r} belongs to enlarging: downscaler {downscaler!r} takes down_antiring")
    return antiring_code(strength), 1 if downscaler == "ssim" else 0


FILM_GRAIN_INTENSITY = 0.01                # the reference's INTENSITY (assets/shaders/filmgrain.glsl)
FILM_GRAIN_MAX = 0.1                       # the largest intensity the ``_grain`` entry points take


def check_film_grain(value=False):
    """A ``film_grain`` option as the processor, the worker, the dispatcher and the command line take it -> the intensity as a float:
    ``False`` / ``0`` -> 0.0 (off), ``True`` -> the reference's ``FILM_GRAIN_INTENSITY``, a float in [0, ``FILM_GRAIN_MAX``] -> itself;
    ``ValueError`` for anything else (a string, None, NaN, a value outside the range)."""
    if isinstance(value, (bool, np.bool_)):
        return FILM_GRAIN_INTENSITY if value else 0.0
    if isinstance(value, (str, bytes)) or value is None:
        raise ValueError(f"film_grain must be True, False or an intensity in [0, {FILM_GRAIN_MAX}] (got {value!r})")
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"film_grain must be True, False or an intensity in [0, {FILM_GRAIN_MAX}] (got {value!r})") from None
    if not 0.0 <= v <= FILM_GRAIN_MAX:        # NaN fails both comparisons
        raise ValueError(f"film_grain must be in [0, {FILM_GRAIN_MAX}] (got {value!r})")
    return v


def check_grain_seed(value=0.0):
    """A per-frame ``grain_seed`` (``film_grain_seed`` of the stream's seed and the frame index) -> a float in [0, 1)."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"grain_seed must be a number in [0, 1) (got {value!r})") from None
    if isinstance(value, bool) or not 0.0 <= v < 1.0:
        raise ValueError(f"grain_seed must be in [0, 1) (got {value!r})")
    return v


def check_grain_stream_seed(value=0):
    """A ``grain_stream_seed`` option: an integer in 0 .. 2^32 - 1 (``film_grain_seed`` hashes it with the frame index)."""
    return _int_in("grain_stream_seed", value, 0, 0xFFFFFFFF)


def film_grain_seed(stream_seed, frame_index):
    """The seed of frame ``frame_index`` (taken mod 2^32) of the stream ``stream_seed``: ``hdrtv_film_grain_seed``, the integer hash
    of include/hdrtv_mi355x.h -- a function of the frame index, not of the order frames complete in, so two lanes or two devices
    give a frame the grain one lane would.  Host only: needs the built library, no device."""
    return float(load().hdrtv_film_grain_seed(check_grain_stream_seed(stream_seed), int(frame_index) & 0xFFFFFFFF))


def check_grain_chain(film_grain, scaler="lanczos", downscaler=None, deband=False):
    """``ValueError`` for the chains the film grain is not provided in, whatever the sizes: ``scaler``
    ``"spline36"`` / ``"ssim_superres"`` and any ``downscaler`` -- in the reference the grain sits in front of those scalers, inside
    kernels that do not take it --, and ``deband``, which behind the grain would average it away.  Returns the intensity."""
    intensity = check_film_grain(film_grain)
    if intensity == 0:
        return 0.0
    if downscaler is not None:
        raise ValueError(f"film_grain does not go with downscaler {downscaler!r}: the grain in front of the shrinking chain is not provided")
    if scaler in SSIMSR_SCALERS:
        raise ValueError(f"film_grain does not go with scaler {scaler!r}: the grain in front of spline36 / SSimSuperRes is not provided "
                         f"(scalers {list(SCALERS)} take it)")
    if deband:
        raise ValueError("film_grain does not go with deband: a deband behind the grain would average the grain away")
    return intensity


TONE_CURVES = ("spline", "bt.2390", "clip")          # tonemap.KINDS; "spline" is the reference's (mpv tone-mapping=spline)
TONE_SOURCE_PEAK = 1000.0                  # the reference's expectation of the model's output, in nits


class ToneMapping(NamedTuple):
    """The tone map of the delivered frames: the arguments of ``tonemap.tone_curve``, validated.  Built by
    ``tone_mapping``; a plain tuple that crosses into the dispatcher's worker processes as it is, like ``OutputCleanup``, and the
    key under which a processor keeps the curve's device gain table."""
    kind: str
    target_peak: float
    source_peak: float
    target_min: float
    source_min: float
    source_avg: object
    param: object

    def curve(self):
        from . import tonemap
        return tonemap.tone_curve(*self)

    def gain_table(self):
        """The curve's ``gain[65536]`` as float32 (``hdrtv_rgb48_tonemap``'s ``dev_gain``, once uploaded)."""
        return self.curve().gain_table()


def tone_mapping(kind=None, target_peak=None, source_peak=TONE_SOURCE_PEAK, target_min=0.0, source_min=0.0, source_avg=None, param=None):
    """The one constructor of ``ToneMapping``, as the processor, the worker, the dispatcher and the command line take the option:
    ``kind`` None / ``"none"`` -> None (off: nothing else is looked at); one of ``TONE_CURVES`` with a ``target_peak`` in nits ->
    the record, or None when ``target_peak >= source_peak`` (nothing to roll off; mpv does not tone-map then either).
    ``ValueError`` for everything ``tonemap.tone_curve`` refuses and for a curve without ``target_peak``."""
    if kind is None or (isinstance(kind, str) and kind.lower() == "none"):
        return None
    if target_peak is None:
        raise ValueError(f"tone mapping {kind!r} needs target_peak, the sink's peak in nits")
    from . import tonemap
    c = tonemap.tone_curve(kind, target_peak, source_peak, target_min, source_min, source_avg, param)
    return None if c.off else ToneMapping(c.kind, c.target_peak, c.source_peak, c.target_min, c.source_min, c.source_avg, c.param)


def pq_eotf_table():
    """``hdrtv_pq_eotf_table``: the tone map's ``lin[65536]`` as float32 -- the level (1.0 = 10000 nits) of every u16 PQ code, with
    ``code(lin[c]) == c``.  Host only: needs the built library, no device."""
    lin = np.empty(65536, dtype=np.float32)
    rc = load().hdrtv_pq_eotf_table(lin.ctypes.data)
    if rc != OK:
        raise RuntimeError(f"hdrtv_pq_eotf_table failed ({rc})")
    return lin


class ScalePlan(NamedTuple):
    """How one frame geometry is resized: ``entry``, the C symbol (one of the six ``hdrtv_post_rgb48_scaled*`` / ``_fsr`` / ``_down`` /
    ``_ssimsr``, or with film grain ``hdrtv_post_rgb48_scaled_grain`` / ``_fsr_grain``), and ``args``, the tuple that follows
    ``dH, dW`` in its signature."""
    entry: str
    args: tuple


class ScaleOptions(NamedTuple):
    """The six options of a frame delivered at another size than the processing size, checked
    (``scale_options`` builds one); the processor, the worker, the dispatcher and the command line all take them by these names.

    ``scaler``: what enlarges.  ``"lanczos"`` (the default): the fused Lanczos passes, ``hdrtv_post_rgb48_scaled``, with
    ``antiring``, the anti-ringing strength 0 .. 1 or ``"auto"`` = ``scale_antiring`` of the two sizes (nonzero:
    ``hdrtv_post_rgb48_scaled_ex``), and ``cas``, the strength of the contrast-adaptive sharpening in front of the upscale, 0 .. 1
    or ``"auto"`` = ``scale_cas`` of the two sizes (nonzero: ``hdrtv_post_rgb48_scaled_cas``).  ``"fsr"``: ``hdrtv_post_rgb48_fsr``,
    the reference's default upscaler, at most 2x per axis, with RCAS at ``fsr_sharpness`` (0 .. 2, 0 = the sharpest; the reference's
    0.2) or, with None, EASU alone.  ``"spline36"`` / ``"ssim_superres"``: ``hdrtv_post_rgb48_ssimsr`` without / with the
    reference's SSimSuperRes shader stage, both axes enlarged, by at most 2x.  Under the last three ``antiring`` and ``cas`` are 0:
    ``"auto"`` resolves to 0, as the reference's schedules do, and an explicit nonzero value is a ``ValueError``.
    ``downscaler``: what shrinks a frame delivered BELOW the processing size.  None (the default): such a size is a
    ``ValueError``.  ``"mitchell"`` / ``"ssim"``: ``hdrtv_post_rgb48_down`` without / with the reference's SSimDownscaler stage, at
    most 4x per axis, with the anti-ringing strength ``down_antiring`` (0 .. 1; ``"auto"`` = the reference's 0.20, resolved in the
    record); ``down_options`` has the refusals (a mixed or enlarging request, an enlarging ``scaler``, a nonzero ``antiring`` /
    ``cas``, nothing to shrink).  A frame delivered at the processing size is untouched by all of them."""
    antiring: object
    cas: object
    scaler: str
    fsr_sharpness: object
    downscaler: object
    down_antiring: float

    def plan(self, proc_w, proc_h, out_w, out_h, film_grain=0.0, grain_seed=0.0):
        """The ``ScalePlan`` of a frame processed at ``proc_w`` x ``proc_h`` and delivered at ``out_w`` x ``out_h``, or None when
        nothing is scaled; everything that depends on the sizes is checked (``ValueError``) and ``"auto"`` resolved here.
        ``film_grain`` (``check_film_grain``) nonzero: the plan's entry is the scaler's ``_grain`` form -- ``"lanczos"``:
        ``hdrtv_post_rgb48_scaled_grain`` with ``(antiring, cas, intensity, seed)``, ``"fsr"``: ``hdrtv_post_rgb48_fsr_grain`` with
        ``(rcas, sharpness, intensity, seed)`` --, ``grain_seed`` the frame's seed; the chains without grain are refused
        (``check_grain_chain``).  At 0 the plan is the one of before."""
        intensity = check_grain_chain(film_grain, self.scaler, self.downscaler) if film_grain else 0.0
        grain = (intensity, check_grain_seed(grain_seed)) if intensity else None
        if self.downscaler is not None:
            return ScalePlan("hdrtv_post_rgb48_down", down_options(self.downscaler, self.down_antiring, proc_w, proc_h, out_w, out_h,
                                                                   self.scaler, self.antiring, self.cas))
        if out_w == proc_w and out_h == proc_h:
            return None
        if out_w < proc_w or out_h < proc_h:
            raise ValueError(f"output size {out_w}x{out_h} is below the processing size {proc_w}x{proc_h} (enlarging only)")
        if self.scaler == "fsr":
            check_fsr_size(proc_w, proc_h, out_w, out_h)
            args = (0, 0.0) if self.fsr_sharpness is None else (1, self.fsr_sharpness)
            return ScalePlan("hdrtv_post_rgb48_fsr_grain", args + grain) if grain else ScalePlan("hdrtv_post_rgb48_fsr", args)
        if self.scaler in SSIMSR_SCALERS:
            check_ssimsr_size(proc_w, proc_h, out_w, out_h)
            return ScalePlan("hdrtv_post_rgb48_ssimsr", (1 if self.scaler == "ssim_superres" else 0,))
        antiring = antiring_code(resolve_antiring(self.antiring, proc_w, proc_h, out_w, out_h))
        cas = cas_code(resolve_cas(self.cas, proc_w, proc_h, out_w, out_h))
        if grain:
            return ScalePlan("hdrtv_post_rgb48_scaled_grain", (antiring, cas) + grain)
        if cas:
            return ScalePlan("hdrtv_post_rgb48_scaled_cas", (antiring, cas))
        return ScalePlan("hdrtv_post_rgb48_scaled_ex", (antiring,)) if antiring else ScalePlan("hdrtv_post_rgb48_scaled", ())


def scale_options(antiring=0.0, cas=0.0, scaler="lanczos", fsr_sharpness=FSR_SHARPNESS, downscaler=None, down_antiring=0.0):
    """The six options -> a ``ScaleOptions``, after every check that does not depend on the sizes (``ValueError``)."""
    scaler = check_scaler(scaler)
    antiring, cas = scaler_options(scaler, antiring, cas)
    fsr_sharpness = check_fsr_sharpness(fsr_sharpness)
    downscaler, strength = check_downscaler(downscaler), check_down_antiring(down_antiring)
    if downscaler is None:
        if strength != 0:
            down_options(None, down_antiring, 0, 0, 0, 0)        # an explicit strength without a downscaler is refused there
    else:                                                        # nothing is enlarged: "auto" is 0 (an explicit value: down_options)
        antiring, cas = (0.0 if v == "auto" else v for v in (antiring, cas))
    return ScaleOptions(antiring, cas, scaler, fsr_sharpness, downscaler, strength)


SCALE_OFF = scale_options()                # the defaults: a frame at the processing size, or plain Lanczos to a larger one


_libs = {}


def load(ab=False):
    """Load the shared library (once).  Raises RuntimeError when it has not been built.  ``ab=True``: the A/B library."""
    path = LIB_PATH_AB if ab else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} not found: the MI355X HIP extension is not built and there is no "
            "fallback path (run __graft_entry__.build())")
    # PyTorch ships its own HIP runtime (libamdhip64 with the system library's SONAME).  Whichever copy a process loads
    # first serves both users, and torch on the system copy finds no device: make torch's the first.
    import torch  # noqa: F401
    lib = C.CDLL(path)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)      # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    _libs[path] = lib
    return lib


def build_id(ab=False):
    """The library's build id: the hash over its sources that csrc/Makefile stamps into hdrtv_version() ("... build <id>")."""
    v = load(ab).hdrtv_version().decode()
    return v.rsplit(" build ", 1)[1] if " build " in v else "unstamped"


def source_hash(name):
    """First 12 hex digits of the SHA-1 of csrc/<name>: what tools/pmc_to_json.py records per source file."""
    import hashlib
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "csrc", name), "rb") as f:
        return hashlib.sha1(f.read()).hexdigest()[:12]


class HdrtvError(RuntimeError):
    pass


def check(lib, ctx, rc, what):
    if rc < 0:
        msg = lib.hdrtv_last_error(ctx)
        raise HdrtvError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
    return rc
