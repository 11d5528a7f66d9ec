"""HDRTVNetMI355X -- drop-in processor for the reference's ``HDRTVNetTorch``.

Mirrors the call surface of ``src/models/hdrtvnet_torch.py:1513-2472`` (constructor
arguments, ``preprocess`` / ``infer`` / ``postprocess`` / ``process`` /
``process_timed`` / ``warmup_compile`` / ``end_profiling`` and the attributes callers
read: ``gui_pipeline_worker_model.py:52,238,242,274``, ``main.py:68,96,104,487``,
``compile_kernels.py:332-345``), the same way the reference's own
``HDRTVNetTensorRT(HDRTVNetTorch)`` is a second backend behind that surface.

All arithmetic runs in ``libhdrtv_mi355x.so`` (hand-written gfx950 HIP kernels) through
the C ABI in ``include/hdrtv_mi355x.h``.  torch is used for device buffers, pinned host
buffers and streams only.  There is no CPU path and no eager fallback: a missing
library, a non-gfx950 device or ``device="cpu"`` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np
import torch

from . import lib as _L
from . import weights as _W


def _split_composite(state):
    """An ``HG_Composite`` checkpoint (keys ``base.AGCM.* / base.LE.* / hg.*``, hdrtvnet_torch.py:1797-1830 and
    HG_Composite_arch.py:30-76) -> (HR state, HG state or None); any other state passes through as (state, None)."""
    if not any(k.startswith("base.") for k in state):
        return state, None
    hr = {k[5:]: v for k, v in state.items() if k.startswith("base.")}
    hg = {k[3:]: v for k, v in state.items() if k.startswith("hg.")}
    return hr, (hg or None)


def _load_state(path_or_state, what):
    """Accepts a mapping, an ``.hdrw`` pack, or a torch checkpoint (raw state_dict or the
    reference's ``{"state_dict":..., "architecture":...}`` wrapper, hdrtvnet_torch.py:1491)."""
    if isinstance(path_or_state, dict):
        return path_or_state
    path = str(path_or_state)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{what} not found: {path}")
    if path.endswith(".hdrw"):
        return _W.load_pack(path)
    payload = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(payload, dict) and "state_dict" in payload:
        payload = payload["state_dict"] or {}
    if not isinstance(payload, dict):
        raise ValueError(f"{what}: unsupported checkpoint payload in {path}")
    return {(k[7:] if k.startswith("module.") else k): v for k, v in payload.items()}


def _dtype_code(t):
    """The C ABI's dtype code of an f16 / f32 tensor."""
    return _L.F32 if t.dtype == torch.float32 else _L.F16


def kernel_arithmetic(tag):
    """The arithmetic class of a launch by its profile tag (csrc/api_graph.hip writes the tags): 'int8' = v_mfma_i32_*_i8,
    'fq-f16' = activation quantiser in registers + fp16 MFMA on dequantised weights, 'fq-f32' = fp32 fake-quant, 'f16'."""
    t = tag.lower()
    if "rows<fq>" in t:
        return "fq-f16"
    if t.startswith("cls_block<fq>"):
        return "fq-f32"
    if "_i8" in t or ",i8" in t or "<i8" in t or "q8" in t or "-i8" in t:
        return "int8"
    return "f16"


def summarize_profile(profile):
    """{class: {"launches", "gmac", "ms", "kernels"}} + "text": one sentence for a bench label, taken from what ran."""
    out = {k: {"launches": 0, "gmac": 0.0, "ms": 0.0, "kernels": set()} for k in ("int8", "fq-f16", "fq-f32", "f16")}
    for _layer, kern, ms, macs, _bytes in profile:
        c = out[kernel_arithmetic(kern)]
        c["launches"] += 1
        c["gmac"] += macs / 1e9
        c["ms"] += ms
        c["kernels"].add(kern.split("<")[0])
    total = sum(c["gmac"] for c in out.values()) or 1.0
    names = {"int8": "on int8 MFMA", "fq-f16": "as fake-quant on fp16 MFMA inside the fused LE row kernels",
             "fq-f32": "as fp32 fake-quant", "f16": "on fp16 MFMA / vector units"}
    parts = [f"{100 * c['gmac'] / total:.1f} % of the MACs in {c['launches']} launches {names[k]}" for k, c in out.items() if c["launches"]]
    res = {k: {"launches": c["launches"], "gmac": round(c["gmac"], 2), "ms": round(c["ms"], 3), "kernels": sorted(c["kernels"])}
           for k, c in out.items()}
    res["text"] = "; ".join(parts)
    return res


class HDRTVNetMI355X:
    """MI355X-native backend with the ``HDRTVNetTorch`` surface.

    ``model_path``: HR checkpoint (``HR.pt``, an ``.hdrw`` pack, or a state mapping).
    ``hg_weights``: HG checkpoint path / mapping, or ``"seeded:<int>"`` for the deterministic
    stand-in of the un-shipped ``HG.pt`` (weights.seeded_hg_state); ``"seeded-w8a8:<int>"`` is that
    stand-in as a W8A8 checkpoint (weights.seeded_hg_w8a8_state).  An HG checkpoint that carries
    ``weight_int8`` / ``x_scale`` / ``x_zero`` tensors in the layout of weights.HG_W8A8_GROUPS runs its
    18 quantised layers on int8 MFMA (BASELINE configs[4]); any other layout is rejected.  As in the reference
    (hdrtvnet_torch.py:2065-2086): an explicit but missing path raises ``FileNotFoundError``;
    with no path given and ``use_hg=True`` the model silently continues without HG.
    An ``HG_Composite`` checkpoint (``base.*`` + ``hg.*`` keys, the layout of the reference's
    ``pytorch_int8/hg/HR_HG_*.pt``) is split into its two halves; with ``use_hg=True`` and no HG tensors anywhere the
    reference's search order applies (``_resolve_hg_weights``, 2016-2042: explicit path, ``HG.pt`` next to the model,
    ``<cwd>/src/models/weights/original/HG.pt``).
    ``compile_*`` and ``force_channels_last`` are accepted and ignored: there is nothing to JIT (kernels are precompiled
    for gfx950).  ``predequantize``: "auto" / True run an INT8 checkpoint as fp16 convs of the dequantised weights (the
    reference's ROCm behaviour), "off" / False keep its W8A8 layers and run them on int8 MFMA.
    ``use_cuda_graphs=True`` replays ``infer`` from a captured hipGraph (2306-2331).  ``fast_condition_resize=True`` (or
    ``HDRTVNET_FAST_COND_RESIZE=1``) derives the condition map with the bilinear 0.25x resize, ``HDRTVNET_ZERO_COND=1``
    zeroes it (1539-1543, 2262-2276).
    ``lanes`` (no reference counterpart; 1 or 2, default 1): frames in flight on the device.  Each lane has its own activation
    workspace, boundary tensors and HIP stream (``enqueue_frame``; the fp32 preset takes one lane only); the reference-shaped calls (``process`` / ``preprocess`` /
    ``infer`` / ``postprocess``) always run on lane 0 and the caller's current stream.
    """

    def __init__(self, model_path, device="auto", precision="auto",
                 compile_model=True, force_compile=False, compile_mode="auto",
                 use_cuda_graphs=False, force_channels_last=False,
                 predequantize="auto", hg_weights=None, use_hg=True,
                 warmup_passes=3, fast_condition_resize=False, lanes=1, _ab_library=False):
        self.model_path = model_path
        self._lanes = int(lanes)
        if not 1 <= self._lanes <= (4 if os.environ.get("HDRTV_LANES_ANY") == "1" else 2):
            raise ValueError("lanes must be 1 or 2")
        self._warmup_passes = int(warmup_passes)
        env_true = lambda n: str(os.environ.get(n, "")).strip().lower() in ("1", "true", "yes", "on")   # noqa: E731
        self._fast_condition_resize = bool(fast_condition_resize) or env_true("HDRTVNET_FAST_COND_RESIZE")
        self._fast_zero_condition = env_true("HDRTVNET_ZERO_COND")
        self._use_cuda_graphs = bool(use_cuda_graphs)
        self._graphs = {}
        self._profiling = False
        self.device = self._resolve_device(device)
        self.precision = self._resolve_precision(precision)
        self._use_cuda = True
        # fp32: the reference's maximum-precision preset -- the same graph on fp32 tensors (csrc/fp32_ops.hip, fp32_graph.hip)
        self._fp32 = self.precision == "fp32"
        self._dtype = torch.float32 if self._fp32 else torch.float16
        self._compiled = False          # nothing is JIT-compiled; warmup_compile() is a no-op
        self._compile_mode = None
        self._trt_engine = None
        self._is_w8_model = False
        self._memory_format_name = "nhwc-internal"
        self.engine_path = _L.LIB_PATH
        self.model = None               # no nn.Module exists; callers treat None as "0 MB"
        self._lib = _L.load(ab=bool(_ab_library))     # _ab_library: tests only (superseded kernels as bit-identity yardsticks)
        self._ctx = C.c_void_p()

        hr_state, hg_from_ckpt = _split_composite(_load_state(model_path, "model weights"))
        if self.precision.startswith("int8"):
            # hdrtvnet_torch.py:1748-1963: an INT8 runtime checkpoint.  On ROCm the reference
            # pre-dequantizes it to native fp16 convs at load time ("auto", 1893-1899): INT8 is
            # compressed storage, compute is fp16 -- exactly what is done here.
            if not _W.is_int8_state(hr_state):
                raise ValueError(f"precision '{self.precision}' needs an INT8 checkpoint (weight_int8 tensors)")
            if str(predequantize).lower() in ("off", "false", "0", "no"):
                # the quantised layers stay in place (hdrtvnet_torch.py:1893-1917 with predequantize off): W8A8 layers run
                # on int8 MFMA with the reference's activation quantisers, W8 (weight-only) layers as fp16 convs of the
                # dequantised weights, exactly what W8Conv2d.forward computes.  hdrtv_create rejects a checkpoint with a
                # W8A8 layer it has no int8 kernel for.
                hr_state = _W.normalize_int8_state(hr_state)
                self._is_w8_model = True
            else:
                hr_state = _W.dequantize_int8_state(hr_state, "fp16")
                self._is_w8_model = False          # as the reference after pre-dequantization (1919)
        elif _W.is_int8_state(hr_state):
            raise ValueError("INT8 checkpoint given with a floating-point precision; use precision='int8-full'/'int8-mixed'")
        try:
            _W.check_hr_state(hr_state)
        except ValueError as exc:
            raise ValueError(f"Unsupported checkpoint for the MI355X backend: {exc}") from exc
        hg_state = None
        self._use_hg = bool(use_hg)
        if self._use_hg:
            if isinstance(hg_weights, str) and hg_weights.startswith("seeded:"):
                hg_state = _W.seeded_hg_state(int(hg_weights.split(":", 1)[1]))
            elif isinstance(hg_weights, str) and hg_weights.startswith("seeded-w8a8:"):
                hg_state = _W.seeded_hg_w8a8_state(int(hg_weights.split(":", 1)[1]))
            elif isinstance(hg_weights, str) and hg_weights.startswith("seeded-w8a8-minmax:"):
                # the same stand-in calibrated the reference's way (x_zero = running minimum: float zero points)
                hg_state = _W.seeded_hg_w8a8_state(int(hg_weights.split(":", 1)[1]), integer_zero=False)
            elif hg_weights is not None:
                hg_state = _split_composite(_load_state(hg_weights, "HG weights"))     # FileNotFoundError if missing
                hg_state = hg_state[1] if hg_state[1] is not None else hg_state[0]
            elif hg_from_ckpt is not None:
                hg_state = hg_from_ckpt                                # HG_Composite checkpoint: its own hg.* half
            else:
                found, searched = self._resolve_hg_weights(model_path)
                if found:
                    hg_state = _load_state(found, "HG weights")
                    hg_weights = found
                elif self.precision.startswith("int8"):
                    # hdrtvnet_torch.py:1928-1937: an INT8 no-HG checkpoint with HG requested needs split HG weights
                    raise FileNotFoundError("INT8 HG weights were requested but not found.\n  Searched paths:\n" +
                                            "\n".join(f"  - {p}" for p in searched) + "\n  Pass hg_weights or disable HG.")
                else:
                    print("WARNING: HG weights not found; continuing with no-HG model.\n  Searched paths:\n" +
                          "\n".join(f"  - {p}" for p in searched))
                    self._use_hg = False
            if hg_state is not None and _W.is_int8_state(hg_state) and not self._is_w8_model and self.precision.startswith("int8") \
                    and not _W.is_hg_w8a8_layout(hg_state):
                # a quantised HG half in a layout the int8 HG kernels do not serve, with predequantize on: fp16 convs
                hg_state = _W.dequantize_int8_state(hg_state, "fp16")
        self._hg_weights = hg_weights if self._use_hg else None
        self._hg_int8 = hg_state is not None and _W.is_int8_state(hg_state)
        self._hg_state_fp = hg_state if (hg_state is not None and not self._hg_int8) else None
        hr_blob = _W.pack_state(hr_state if self._is_w8_model else {k: hr_state[k] for k, _ in _arch_hr()})
        hg_blob = _W.pack_state({k: v for k, v in hg_state.items()
                                 if not k.endswith("num_batches_tracked")}) if hg_state is not None else b""
        rc = self._lib.hdrtv_create_ex(hr_blob, len(hr_blob), hg_blob if hg_blob else None, len(hg_blob),
                                       self.device.index or 0, _L.PREC_F32 if self._fp32 else _L.PREC_F16, C.byref(self._ctx))
        if rc < 0:
            msg = self._lib.hdrtv_last_error(self._ctx).decode() if self._ctx else "allocation failed"
            self._lib.hdrtv_destroy(self._ctx)
            self._ctx = C.c_void_p()
            if rc == _L.EWEIGHTS:
                raise ValueError(f"model backend failed - {msg}")
            raise RuntimeError(f"model backend failed - {msg}")

        if self._lanes > 1:
            # (HDRTV_EINVAL for the fp32 preset: one lane only there, include/hdrtv_mi355x.h)
            try:
                self._chk(self._lib.hdrtv_set_lanes(self._ctx, self._lanes), "hdrtv_set_lanes")
            except Exception:
                self._lib.hdrtv_destroy(self._ctx)
                self._ctx = C.c_void_p()
                raise
        self._lane_bufs, self._lane_streams = [], []
        self._tone_tables = {}                 # _tone_gain: lib.ToneMapping -> its device gain table, at most TONE_TABLES_MAX of them
        self._ycc_scratch = {}                 # _post_out: RGB48 at the output size per lane / caller (the two-launch Y'CbCr path)
        if self._fast_zero_condition or self._fast_condition_resize:
            self._chk(self._lib.hdrtv_set_cond_mode(self._ctx, 2 if self._fast_zero_condition else 1), "hdrtv_set_cond_mode")
        self._buf_hw = None
        self._gpu_input = self._gpu_cond = self._gpu_raw = None
        self._pin_input = self._pin_output = None
        self._staging = {}                     # _upload: [pinned slot, device buffer, event behind the last upload] per input path
        self._gpu_out = self._gpu_agcm = self._gpu_u8 = None
        print(f"MI355X device : {self.device}")
        # which arithmetic a W8A8 layer runs in depends on the kernel the launch sequence picks for it per resolution
        # (int8 MFMA, or the fake-quant form inside a fused LE row kernel): `execution_summary()` reports it from a profile
        print(f"MI355X precision: {self.precision}{' (W8A8 layers kept quantised: predequantize off)' if self._is_w8_model else ''}  "
              f"(HG {('W8A8 on int8 MFMA' if self._hg_int8 else 'on') if self._use_hg else 'off'})")
        if self._warmup_passes > 0:
            self._warmup()

    # ------------------------------------------------------------------ helpers
    def _resolve_device(self, device):
        mode = str(device).lower()
        if mode not in ("auto", "cuda", "cpu") and not mode.startswith("cuda:"):
            raise ValueError("device must be one of: auto, cuda, cpu")
        if mode == "cpu":
            raise RuntimeError("the MI355X backend has no CPU path; use the reference's HDRTVNetTorch for device='cpu'")
        if not torch.cuda.is_available():
            raise RuntimeError("CUDA/ROCm device not available for the MI355X backend.")
        if mode.startswith("cuda:"):
            return torch.device(mode)
        return torch.device("cuda", torch.cuda.current_device())

    def _resolve_precision(self, precision):
        p = str(precision).lower()
        if p not in {"auto", "fp16", "fp32", "int8-full", "int8-mixed"}:
            raise ValueError("precision must be one of: auto, fp16, fp32, int8-full, int8-mixed")
        if p in ("auto", "fp16"):
            return "fp16"
        return p              # int8-*: INT8 storage, fp16 compute (the reference's own ROCm behaviour); fp32: the fp32 graph

    def _resolve_hg_weights(self, model_path):
        """hdrtvnet_torch.py:2016-2042 (the user override is handled by the caller): HG.pt next to the checkpoint, then
        the repo-default location relative to the working directory; ``.hdrw`` packs are accepted beside ``.pt``."""
        cands = []
        if not isinstance(model_path, dict):
            d = os.path.dirname(os.path.abspath(str(model_path)))
            cands += [os.path.join(d, "HG.pt"), os.path.join(d, "HG.hdrw")]
        cands.append(os.path.join(os.getcwd(), "src", "models", "weights", "original", "HG.pt"))
        for p in cands:
            if os.path.isfile(p):
                return p, cands
        return None, cands

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _chk(self, rc, what):
        return _L.check(self._lib, self._ctx, rc, what)

    @property
    def _out_dt(self):
        """The dtype code of the model's output tensor: f32 from the HG tail and the fp32 preset, f16 otherwise."""
        return _L.F32 if (self._use_hg or self._fp32) else _L.F16

    def _warmup(self):
        h, w = 1080, 1920
        dummy = np.zeros((h, w, 3), dtype=np.uint8)
        for _ in range(self._warmup_passes):
            self.process(dummy)
        torch.cuda.synchronize(self.device)

    # ------------------------------------------------------------------ buffers
    def _ensure_buffers(self, h, w):
        """hdrtvnet_torch.py:2198-2233."""
        if self._buf_hw == (h, w):
            return
        self._graphs.clear()                      # captured graphs point into the buffers replaced below
        with torch.cuda.device(self.device):
            self._chk(self._lib.hdrtv_reserve(self._ctx, h, w), "hdrtv_reserve")
            ch, cw = max(1, h // 4), max(1, w // 4)
            dev = self.device
            self._gpu_input = torch.empty((1, 3, h, w), dtype=self._dtype, device=dev)
            self._gpu_cond = torch.empty((1, 3, ch, cw), dtype=self._dtype, device=dev)
            self._gpu_raw = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
            self._gpu_u8 = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
            self._gpu_out = torch.empty((1, 3, h, w), dtype=torch.float32 if self._out_dt == _L.F32 else torch.float16, device=dev)
            self._gpu_agcm = torch.empty((1, 3, h, w), dtype=self._dtype, device=dev)
            self._pin_input = torch.empty((h, w, 3), dtype=torch.uint8, pin_memory=True)
            self._staging["bgr"] = [self._pin_input, self._gpu_raw, None]
            self._pin_output = torch.empty((h, w, 3), dtype=torch.uint8, pin_memory=True)
            # lane l > 0: its own boundary tensors (input, cond, out, agcm) and stream; lane 0 is the set above
            self._lane_bufs = [(self._gpu_input, self._gpu_cond, self._gpu_out, self._gpu_agcm)]
            for _ in range(1, self._lanes):
                self._lane_bufs.append((torch.empty_like(self._gpu_input), torch.empty_like(self._gpu_cond),
                                        torch.empty_like(self._gpu_out), torch.empty_like(self._gpu_agcm)))
            if len(self._lane_streams) != self._lanes:
                self._lane_streams = [torch.cuda.Stream(dev) for _ in range(self._lanes)]
        self._buf_hw = (h, w)

    # ------------------------------------------------------------------ lanes
    @property
    def lanes(self):
        return self._lanes

    def lane_stream(self, lane):
        """The HIP stream lane ``lane``'s frames are enqueued on (a ``torch.cuda.Stream``; valid after the first
        ``_ensure_buffers``)."""
        return self._lane_streams[lane]

    def _scratch(self, key, out, nbytes=None):
        """The RGB48 scratch at the output size kept per ``key``; with ``nbytes``, a scratch of that many bytes instead."""
        shape, dtype = ((out.h, out.w, 3), torch.uint16) if nbytes is None else ((int(nbytes),), torch.uint8)
        scratch = self._ycc_scratch.get(key)
        if scratch is None or tuple(scratch.shape) != shape or scratch.dtype != dtype:
            scratch = self._ycc_scratch[key] = torch.empty(shape, dtype=dtype, device=self.device)
        return scratch.data_ptr()

    def _fs_scratch(self, key, out):
        """The scratch of the error-diffusion conversions (``hdrtv_ycbcr10_fs_scratch_bytes``) for ``out``, kept per ``key``: one
        per lane / caller, so that two lanes never share one."""
        nbytes = self._lib.hdrtv_ycbcr10_fs_scratch_bytes(_L.YCC_FORMATS[out.pix_fmt], out.h, out.w)
        if nbytes < 0:
            raise ValueError(f"no error-diffusion scratch for {out.pix_fmt} at {out.w}x{out.h}")
        return self._scratch((key, "fs"), out, nbytes)

    def _post_out(self, st, src_ptr, dt, h, w, dst_ptr, out, scratch_key, light_ptr=None, light_rect=None, cleanup=None, scale=None,
                  film_grain=0.0, grain_seed=0.0, tone=None):
        """The output conversion of a frame whose planar tensor lies at ``src_ptr``, to the ``lib.OutputFormat`` ``out`` at
        ``dst_ptr``: ``rgb48le`` at the processing size (``hdrtv_post_rgb48``) or enlarged to ``out.h`` x ``out.w``
        (``hdrtv_post_rgb48_scaled``); a 10-bit Y'CbCr layout in one kernel at the processing size (``hdrtv_post_ycbcr10``), or,
        enlarged, in two launches through an RGB48 scratch kept per ``scratch_key`` (``hdrtv_post_rgb48_scaled`` +
        ``hdrtv_rgb48_to_ycbcr10``).  ``light_ptr``: device address of a ``lib.LIGHT_WORDS`` u32 record that receives the
        delivered frame's content light level over ``light_rect = (x0, y0, rw, rh)`` in delivered-frame
        coordinates (default: the whole frame): ``hdrtv_light_stats`` on the tensor for an unscaled frame, ``hdrtv_rgb48_light_stats``
        on the scaled frame's RGB48 codes (the destination, or the Y'CbCr scratch) otherwise.  None: nothing more is launched.
        ``cleanup``: a ``lib.OutputCleanup`` (None or inactive: the launches above, nothing more allocated).
        Deband: tensor -> ``hdrtv_post_rgb48`` / ``hdrtv_post_rgb48_scaled`` into a scratch -> ``hdrtv_rgb48_deband`` -> ``dst``
        (``rgb48le``), or into a second scratch and through the conversion from codes; the light level record is then taken from
        the debanded codes, which are what is delivered.  Dither alone: ``hdrtv_post_ycbcr10_ex`` at the processing size, the
        ``_ex`` conversion behind the scaled codes otherwise; it does not enter the record, which is defined on RGB48 codes.
        ``dither="floyd_steinberg"`` takes the same two places through ``hdrtv_post_ycbcr10_fs`` / ``hdrtv_rgb48_to_ycbcr10_fs``
        and a scratch of ``hdrtv_ycbcr10_fs_scratch_bytes`` bytes kept per ``scratch_key``; the ``_ex`` entry points never see its code.
        ``scale``: the ``lib.ScalePlan`` of a frame delivered at another size (``lib.ScaleOptions.plan`` of the two sizes, which is
        the one place that chooses among the six entry points): its entry point replaces
        ``hdrtv_post_rgb48_scaled``, and everything behind it -- deband, the conversion from codes, the record -- sees its codes.
        A frame delivered at the processing size has none.
        ``film_grain`` (an intensity, ``lib.check_film_grain``; 0: every path above as it is, no new launch, no new scratch) with
        the frame's ``grain_seed``: the frame passes through RGB48 codes -- ``hdrtv_post_rgb48_grain`` at the processing size, the
        ``_grain`` entry of ``scale`` (``lib.ScaleOptions.plan(..., film_grain, grain_seed)``) otherwise --, a Y'CbCr layout is
        converted from those codes through the scratch, and the light level record is taken from the grained codes, which are
        what the sink receives.  Deband with grain is a ``ValueError`` (``lib.check_grain_chain``).
        ``tone`` (a ``lib.ToneMapping``; None: every path above as it is, no new launch, no new scratch): the frame is rolled off to
        the sink's peak behind scale, grain and deband and in front of the record and the conversion from
        codes.  A frame at the processing size without grain and deband takes ``hdrtv_post_rgb48_tonemap`` in place of
        ``hdrtv_post_rgb48`` (a Y'CbCr layout into the codes scratch it is then converted from); every other path runs
        ``hdrtv_rgb48_tonemap`` in place on the RGB48 codes it already holds.  The record is always taken from the tone-mapped
        codes (``hdrtv_rgb48_light_stats``), so MaxCLL describes what is delivered."""
        scaled = (out.h, out.w) != (h, w)
        grain = film_grain != 0
        gain_ptr = None if tone is None else self._tone_gain(tone)
        rect = (0, 0, out.w, out.h) if light_rect is None else tuple(int(v) for v in light_rect)
        active = cleanup is not None and cleanup.active
        deband, dither = active and cleanup.deband, active and cleanup.dither != "none"
        if dither and out.is_rgb48:
            raise ValueError("dither applies to the 10-bit Y'CbCr formats: rgb48le (16-bit codes) is not dithered")
        if grain:
            _L.check_grain_chain(film_grain, deband=deband)
            if scaled and not scale.entry.endswith("_grain"):
                raise ValueError(f"film_grain needs the _grain form of {scale.entry} (lib.ScaleOptions.plan(..., film_grain, grain_seed))")
        codes = scaled or deband or grain or gain_ptr is not None      # the frame passes through RGB48 codes in device memory
        if light_ptr is not None and not codes:
            self._chk(self._lib.hdrtv_light_stats(self._ctx, st, src_ptr, dt, h, w, 0, 0.0, *rect, light_ptr), "hdrtv_light_stats")
        if not out.is_rgb48 and not codes:
            if dither and cleanup.error_diffusion:
                self._chk(self._lib.hdrtv_post_ycbcr10_fs(self._ctx, st, src_ptr, dt, h, w, 0, 0.0, *out.planes(dst_ptr),
                                                          self._fs_scratch(scratch_key, out)), "hdrtv_post_ycbcr10_fs")
            elif dither:
                self._chk(self._lib.hdrtv_post_ycbcr10_ex(self._ctx, st, src_ptr, dt, h, w, 0, 0.0, *out.planes(dst_ptr), cleanup.dither_code),
                          "hdrtv_post_ycbcr10_ex")
            else:
                self._chk(self._lib.hdrtv_post_ycbcr10(self._ctx, st, src_ptr, dt, h, w, 0, 0.0, *out.planes(dst_ptr)), "hdrtv_post_ycbcr10")
            return
        rgb_ptr = dst_ptr if out.is_rgb48 else self._scratch(scratch_key, out)
        raw_ptr = self._scratch((scratch_key, "raw"), out) if deband else rgb_ptr       # deband never works in place
        if scaled:
            self._chk(getattr(self._lib, scale.entry)(self._ctx, st, src_ptr, dt, h, w, 0, 0.0, raw_ptr, out.h, out.w, *scale.args), scale.entry)
        elif grain:
            self._chk(self._lib.hdrtv_post_rgb48_grain(self._ctx, st, src_ptr, dt, h, w, 0, 0.0, raw_ptr, film_grain, grain_seed),
                      "hdrtv_post_rgb48_grain")
        elif gain_ptr is not None and not deband:
            self._chk(self._lib.hdrtv_post_rgb48_tonemap(self._ctx, st, src_ptr, dt, h, w, 0, 0.0, gain_ptr, rgb_ptr), "hdrtv_post_rgb48_tonemap")
            gain_ptr = None                          # done
        else:
            self._chk(self._lib.hdrtv_post_rgb48(self._ctx, st, src_ptr, dt, h, w, raw_ptr), "hdrtv_post_rgb48")
        if deband:
            self._chk(self._lib.hdrtv_rgb48_deband(self._ctx, st, raw_ptr, out.h, out.w, cleanup.deband_range, cleanup.deband_threshold, 0,
                                                   rgb_ptr), "hdrtv_rgb48_deband")
        if gain_ptr is not None:
            self._chk(self._lib.hdrtv_rgb48_tonemap(self._ctx, st, rgb_ptr, out.h, out.w, gain_ptr, rgb_ptr), "hdrtv_rgb48_tonemap")
        if light_ptr is not None and codes:
            self._chk(self._lib.hdrtv_rgb48_light_stats(self._ctx, st, rgb_ptr, out.h, out.w, *rect, light_ptr), "hdrtv_rgb48_light_stats")
        if out.is_rgb48:
            return
        if dither and cleanup.error_diffusion:
            self._chk(self._lib.hdrtv_rgb48_to_ycbcr10_fs(self._ctx, st, rgb_ptr, out.h, out.w, *out.planes(dst_ptr),
                                                          self._fs_scratch(scratch_key, out)), "hdrtv_rgb48_to_ycbcr10_fs")
        elif dither:
            self._chk(self._lib.hdrtv_rgb48_to_ycbcr10_ex(self._ctx, st, rgb_ptr, out.h, out.w, *out.planes(dst_ptr), cleanup.dither_code),
                      "hdrtv_rgb48_to_ycbcr10_ex")
        else:
            self._chk(self._lib.hdrtv_rgb48_to_ycbcr10(self._ctx, st, rgb_ptr, out.h, out.w, *out.planes(dst_ptr)), "hdrtv_rgb48_to_ycbcr10")

    TONE_TABLES_MAX = 16                       # gain tables a processor keeps (256 KiB each): one per lib.ToneMapping it has been given

    def _tone_gain(self, tone):
        """Device address of the float32 ``gain[65536]`` of the ``lib.ToneMapping`` ``tone``: built (``tonemap.py``, on the host) and
        uploaded on first use, then kept for as long as the processor lives -- frames in flight on any lane may read it, so no
        entry is ever replaced.  The cache is bounded instead: a processor serves a few sinks, and record number
        ``TONE_TABLES_MAX`` + 1 is a ``ValueError``."""
        if not isinstance(tone, _L.ToneMapping):
            raise ValueError("tone must be a lib.ToneMapping (lib.tone_mapping builds one) or None")
        table = self._tone_tables.get(tone)
        if table is None:
            if len(self._tone_tables) >= self.TONE_TABLES_MAX:
                raise ValueError(f"this processor already keeps {self.TONE_TABLES_MAX} tone curves (their tables live as long as it does)")
            tone = _L.tone_mapping(*tone)          # validated again: the record may have crossed a process boundary
            if tone is None:
                raise ValueError("tone resolves to off (target_peak >= source_peak): pass None")
            with torch.cuda.device(self.device):
                table = torch.from_numpy(tone.gain_table()).to(self.device)
                torch.cuda.current_stream().synchronize()      # uploaded before any lane's stream reads it
            self._tone_tables[tone] = table
        return table.data_ptr()

    def light_stats(self, tensor, rect=None):
        """The content light level record (``lib.LIGHT_WORDS`` u32, a device tensor; ``lightlevel.FrameLight.from_record`` reads
        its host copy) of the model's output ``tensor`` ``[1, 3, H, W]`` or ``[3, H, W]``: of the RGB48 codes ``hdrtv_post_rgb48``
        writes for it, over ``rect = (x0, y0, rw, rh)`` (default: the whole frame).  Enqueued on the current stream."""
        t = (tensor[0] if isinstance(tensor, (tuple, list)) else tensor).contiguous()
        h, w = int(t.shape[-2]), int(t.shape[-1])
        rec = torch.empty(_L.LIGHT_WORDS, dtype=torch.uint32, device=t.device)
        rect = (0, 0, w, h) if rect is None else tuple(int(v) for v in rect)
        with torch.cuda.device(self.device):
            self._chk(self._lib.hdrtv_light_stats(self._ctx, self._stream(), t.data_ptr(), _dtype_code(t), h, w, 0, 0.0, *rect, rec.data_ptr()),
                      "hdrtv_light_stats")
        return rec

    def _frame_out(self, lane, h, w, out_hw, out_pix_fmt, out_siting):
        """The argument checks ``enqueue_frame*`` share -> the ``lib.OutputFormat`` of the frame."""
        if not 0 <= lane < self._lanes:
            raise ValueError(f"lane {lane} of {self._lanes}")
        return _L.output_format(out_pix_fmt, out_siting, *((h, w) if out_hw is None else out_hw))

    @staticmethod
    def _cleanup_for(cleanup, out):
        """The ``cleanup`` argument of ``enqueue_frame*`` checked against the frame's format -> a ``lib.OutputCleanup`` or None."""
        if cleanup is None:
            return None
        if not isinstance(cleanup, _L.OutputCleanup):
            raise ValueError("cleanup must be a lib.OutputCleanup (lib.output_cleanup builds one) or None")
        return _L.output_cleanup(*cleanup, pix_fmt=out.pix_fmt)

    @staticmethod
    def _plan_for(h, w, out, antiring, cas, scaler, fsr_sharpness, downscaler, down_antiring, film_grain=0.0, grain_seed=0.0):
        """The six scaler arguments of ``enqueue_frame*`` (``lib.ScaleOptions``) and the film grain's two -> the ``lib.ScalePlan`` of
        the frame, or None."""
        def off(v):
            return type(v) in (float, int) and v == 0
        if scaler == "lanczos" and downscaler is None and off(antiring) and off(cas) and off(down_antiring):
            opts = _L.SCALE_OFF                                       # the default: nothing to check on the hot path
        else:
            opts = _L.scale_options(antiring, cas, scaler, fsr_sharpness, downscaler, down_antiring)
        return opts.plan(w, h, out.w, out.h, film_grain, grain_seed) if film_grain else opts.plan(w, h, out.w, out.h)

    def _enqueue_planes(self, fmt, lane, src_ptr, h, w, dst_ptr, stream=None, out_hw=None, out_pix_fmt="rgb48le", out_siting="left",
                        light_ptr=None, light_rect=None, cleanup=None, antiring=0.0, cas=0.0, scaler="lanczos",
                        fsr_sharpness=_L.FSR_SHARPNESS, downscaler=None, down_antiring=0.0, film_grain=0.0, grain_seed=0.0, tone=None):
        """The body of ``enqueue_frame*`` (whose arguments these are): the argument checks, then the preprocess entry point of the
        ``lib.InputFormat`` ``fmt`` on the frame at ``src_ptr``, ``hdrtv_infer_lane`` and ``_post_out``, all on the lane's buffers
        and ``stream`` (default: the lane's own)."""
        out = self._frame_out(lane, h, w, out_hw, out_pix_fmt, out_siting)
        src = fmt.planes(src_ptr, h, w)
        if film_grain:                         # 0.0 / False: the path of before, nothing checked
            film_grain, grain_seed = _L.check_grain_chain(film_grain, scaler, downscaler), _L.check_grain_seed(grain_seed)
        cleanup = self._cleanup_for(cleanup, out)
        plan = self._plan_for(h, w, out, antiring, cas, scaler, fsr_sharpness, downscaler, down_antiring, film_grain, grain_seed)
        self._ensure_buffers(h, w)
        st = C.c_void_p((stream if stream is not None else self._lane_streams[lane]).cuda_stream)
        tin, tcond, tout, tagcm = self._lane_bufs[lane]
        self._chk(getattr(self._lib, fmt.entry)(self._ctx, st, *src, h, w, tin.data_ptr(), tcond.data_ptr()), fmt.entry)
        self._chk(self._lib.hdrtv_infer_lane(self._ctx, lane, st, tin.data_ptr(), tcond.data_ptr(), h, w, tout.data_ptr(), self._out_dt,
                                             tagcm.data_ptr()), "hdrtv_infer_lane")
        self._post_out(st, tout.data_ptr(), self._out_dt, h, w, dst_ptr, out, ("lane", lane), light_ptr, light_rect, cleanup, plan,
                       film_grain, grain_seed, tone)

    def enqueue_frame(self, lane, src_bgr_ptr, h, w, dst_rgb48_ptr, stream=None, out_hw=None, out_pix_fmt="rgb48le",
                      out_siting="left", light_ptr=None, light_rect=None, cleanup=None, antiring=0.0, cas=0.0,
                      scaler="lanczos", fsr_sharpness=_L.FSR_SHARPNESS, downscaler=None, down_antiring=0.0, film_grain=0.0,
                      grain_seed=0.0, tone=None):
        """One frame of the hot path on lane ``lane``, stream-ordered and without any host synchronisation: u8 BGR frame in
        device memory at ``src_bgr_ptr`` -> hdrtv_preprocess -> hdrtv_infer_lane -> hdrtv_post_rgb48 -> u16 RGB48 at the device
        address ``dst_rgb48_ptr``.  ``stream``: a ``torch.cuda.Stream`` (default: the lane's own).  Frames enqueued on different
        lanes may overlap on the device; the bytes written do not depend on the lane (tests/test_gpu_lanes.py).  The caller
        orders the use of ``src`` / ``dst`` against the stream (events), as with any asynchronous launch.  ``out_hw = (out_h,
        out_w)``: the frame is delivered at that size (``hdrtv_post_rgb48_scaled``; ``dst`` holds out_h * out_w * 3 u16).
        ``out_pix_fmt`` ``p010le`` / ``yuv420p10le`` / ``yuv422p10le`` (``out_siting`` ``left`` / ``topleft``): ``dst`` receives the
        10-bit Y'CbCr planes back to back instead (``lib.out_frame_bytes`` bytes) -- ``hdrtv_post_ycbcr10`` at
        the processing size, with ``out_hw`` two launches through a per-lane RGB48 scratch.  ``light_ptr`` / ``light_rect``: the
        delivered frame's content light level record, behind the frame on the same stream (``_post_out``).
        ``cleanup``: a ``lib.OutputCleanup`` (``lib.output_cleanup``): deband and / or ordered dither of the delivered frame
        (``_post_out``); None: neither, and the bytes of before.  ``antiring``, ``cas``, ``scaler``,
        ``fsr_sharpness``, ``downscaler``, ``down_antiring``: how a frame with an ``out_hw`` other than the processing size is resized
        (``lib.ScaleOptions`` describes the six).  The defaults: plain Lanczos to a larger size, a smaller one is a
        ``ValueError``, and a frame at the processing size is touched by none of them.  ``film_grain`` (``lib.check_film_grain``:
        True = the reference's 0.01, or an intensity up to 0.1) with ``grain_seed`` = ``lib.film_grain_seed(stream_seed, frame
        index)``: the reference's film grain on the delivered frame, placed as its shader chain places it (``_post_out``;
        INTEGRATION.md 5c); 0: every path exactly as before.  ``tone`` (a ``lib.ToneMapping``, ``lib.tone_mapping``): the delivered
        frame rolled off to the sink's peak, behind scale, grain and deband and in front of the record (``_post_out``;
        INTEGRATION.md 5i); None: every path exactly as before."""
        self._enqueue_planes(_BGR24, lane, src_bgr_ptr, h, w, dst_rgb48_ptr, stream, out_hw, out_pix_fmt, out_siting,
                             light_ptr, light_rect, cleanup, antiring, cas, scaler, fsr_sharpness, downscaler, down_antiring,
                             film_grain, grain_seed, tone)

    def enqueue_frame_yuv420(self, lane, src_ptr, h, w, dst_rgb48_ptr, *, layout="i420", matrix=709, full_range=False, stream=None,
                             out_hw=None, out_pix_fmt="rgb48le", out_siting="left", light_ptr=None, light_rect=None, cleanup=None,
                             antiring=0.0, cas=0.0, scaler="lanczos", fsr_sharpness=_L.FSR_SHARPNESS, downscaler=None, down_antiring=0.0,
                             film_grain=0.0, grain_seed=0.0, tone=None):
        """``enqueue_frame`` of an 8-bit 4:2:0 frame: the planes lie back to back at the device address ``src_ptr`` (the
        ``(h*3//2, w)`` u8 array ``preprocess_yuv420`` takes) and ``hdrtv_preprocess_yuv420`` replaces ``hdrtv_preprocess``."""
        self._enqueue_planes(_in_format("yuv420", layout, matrix, full_range), lane, src_ptr, h, w, dst_rgb48_ptr, stream, out_hw, out_pix_fmt,
                             out_siting, light_ptr, light_rect, cleanup, antiring, cas, scaler, fsr_sharpness, downscaler, down_antiring,
                             film_grain, grain_seed, tone)

    def enqueue_frame_ycbcr10(self, lane, src_ptr, h, w, dst_ptr, *, pix_fmt, matrix=709, full_range=False, stream=None, out_hw=None,
                              out_pix_fmt="rgb48le", out_siting="left", cleanup=None, antiring=0.0, cas=0.0, scaler="lanczos",
                              fsr_sharpness=_L.FSR_SHARPNESS, downscaler=None, down_antiring=0.0, film_grain=0.0, grain_seed=0.0,
                              tone=None):
        """``enqueue_frame`` of a 10-bit Y'CbCr frame (``pix_fmt`` ``p010le`` / ``yuv420p10le`` / ``yuv422p10le``): the planes lie
        back to back at the device address ``src_ptr`` (the u16 array ``preprocess_ycbcr10`` takes) and
        ``hdrtv_preprocess_ycbcr10`` replaces ``hdrtv_preprocess``."""
        self._enqueue_planes(_in_format("ycbcr10", pix_fmt, matrix, full_range), lane, src_ptr, h, w, dst_ptr, stream, out_hw, out_pix_fmt,
                             out_siting, None, None, cleanup, antiring, cas, scaler, fsr_sharpness, downscaler, down_antiring,
                             film_grain, grain_seed, tone)

    def _upload(self, key, src, staged=None):
        """Device pointer of the host u8 array ``src``, uploaded through the staging slot kept per ``key`` in ``_staging``: a
        pinned slot, its device buffer and the event behind the last upload out of the slot (allocated on first use and on a shape
        change; the BGR path's are ``_ensure_buffers``').  A plain memcpy into the pinned slot (GIL released), not tensor.copy_:
        ATen parallelises a 25 MB copy over every OpenMP thread, whose spin-wait afterwards starves the HIP runtime's completion
        handling (measured on the GPU box: every third 4K frame stalled ~55 ms behind a 128-thread copy).  ``staged``: the frame
        already lives in page-locked memory (playback.PinnedPrefetch filled it on its own thread while the previous frame was on
        the GPU) and is uploaded as it is."""
        slot = self._staging.get(key)
        if slot is None or tuple(slot[0].shape) != tuple(src.shape):
            slot = self._staging[key] = [torch.empty(src.shape, dtype=torch.uint8, pin_memory=True),
                                         torch.empty(src.shape, dtype=torch.uint8, device=self.device), None]
        pin, dev, uploaded = slot
        if staged is not None and staged.is_pinned() and tuple(staged.shape) == tuple(src.shape):
            dev.copy_(staged, non_blocking=True)
            return dev.data_ptr()
        src = np.ascontiguousarray(src)
        # the slot is reused: the last frame's upload out of it is asynchronous and must have been read before the host
        # overwrites it (two calls without a synchronisation in between uploaded the second frame twice)
        if uploaded is None:
            uploaded = slot[2] = torch.cuda.Event()
        else:
            uploaded.synchronize()
        C.memmove(pin.data_ptr(), src.ctypes.data, src.nbytes)
        dev.copy_(pin, non_blocking=True)
        uploaded.record(torch.cuda.current_stream(self.device))
        return dev.data_ptr()

    # ------------------------------------------------------------------ API
    @torch.inference_mode()
    def preprocess(self, frame_bgr):
        """hdrtvnet_torch.py:2238-2296.  Returns processor-owned persistent tensors."""
        if frame_bgr.ndim != 3 or frame_bgr.shape[2] != 3 or frame_bgr.dtype != np.uint8:
            raise ValueError("frame_bgr must be uint8 [H,W,3]")
        h, w = frame_bgr.shape[:2]
        self._ensure_buffers(h, w)
        dev_copy, ready = getattr(frame_bgr, "device_tensor", None), getattr(frame_bgr, "ready_event", None)
        if dev_copy is not None and ready is not None and dev_copy.device == self.device and tuple(dev_copy.shape) == (h, w, 3):
            # already uploaded by the prefetcher on its own stream (hipMemcpyAsync + hipEvent handoff): wait for that
            # event in stream order and unpack straight from its buffer
            torch.cuda.current_stream(self.device).wait_event(ready)
            raw = dev_copy.data_ptr()
        else:
            raw = self._upload("bgr", frame_bgr, getattr(frame_bgr, "pinned_tensor", None))
        self._chk(self._lib.hdrtv_preprocess(self._ctx, self._stream(), raw, h, w,
                                             self._gpu_input.data_ptr(), self._gpu_cond.data_ptr()), "hdrtv_preprocess")
        return self._gpu_input, self._gpu_cond

    @torch.inference_mode()
    def preprocess_letterboxed(self, frame_bgr, out_w, out_h):
        """``preprocess(_letterbox_bgr(frame, out_w, out_h))`` (gui_scaling.py:228-244 followed by
        hdrtvnet_torch.py:2238-2296) with the resize on the device: the source frame is uploaded at ITS size and
        ``hdrtv_letterbox_u8`` writes the letterboxed u8 frame the ordinary unpack/condition kernels read.  The resize
        arithmetic is oracle/letterbox_oracle.py's restatement of OpenCV (parity with cv2 unpinned)."""
        if frame_bgr.ndim != 3 or frame_bgr.shape[2] != 3 or frame_bgr.dtype != np.uint8:
            raise ValueError("frame_bgr must be uint8 [H,W,3]")
        sh, sw = frame_bgr.shape[:2]
        out_w, out_h = int(out_w), int(out_h)
        if (sw, sh) == (out_w, out_h):
            return self.preprocess(frame_bgr)
        self._ensure_buffers(out_h, out_w)
        self._chk(self._lib.hdrtv_letterbox_u8(self._ctx, self._stream(), self._upload("letterbox", frame_bgr), sh, sw,
                                               self._gpu_raw.data_ptr(), out_h, out_w), "hdrtv_letterbox_u8")
        self._chk(self._lib.hdrtv_preprocess(self._ctx, self._stream(), self._gpu_raw.data_ptr(), out_h, out_w,
                                             self._gpu_input.data_ptr(), self._gpu_cond.data_ptr()), "hdrtv_preprocess")
        return self._gpu_input, self._gpu_cond

    def _upload_planes(self, fmt, frame):
        """Device pointer of a Y'CbCr frame (the array of ``fmt.frame_shape``), uploaded through the staging slot of its family
        (``_upload``: the BGR path's buffers stay as they are), or, for an 8-bit frame, the prefetcher's own upload / pinned buffer
        as ``preprocess`` uses them."""
        if fmt.family == "ycbcr10":             # the upload path moves bytes: a u16 frame goes through it as the u8 view of its samples
            return self._upload("ycbcr10", np.ascontiguousarray(frame).view(np.uint8))
        dev_copy, ready = getattr(frame, "device_tensor", None), getattr(frame, "ready_event", None)
        if dev_copy is not None and ready is not None and dev_copy.device == self.device and tuple(dev_copy.shape) == tuple(frame.shape):
            torch.cuda.current_stream(self.device).wait_event(ready)
            return dev_copy.data_ptr()
        return self._upload("yuv", frame, getattr(frame, "pinned_tensor", None))

    @torch.inference_mode()
    def _preprocess_planes(self, fmt, frame, letterbox_to=None):
        """``preprocess`` of a Y'CbCr frame of the ``lib.InputFormat`` ``fmt``, through its C entry point; with ``letterbox_to =
        (out_w, out_h)`` other than the frame's size, letterboxed to that size on the device: at ten bits in one launch
        (``hdrtv_preprocess_ycbcr10_letterboxed``), at eight through BGR at the source size (``hdrtv_yuv420_to_bgr_u8``,
        ``hdrtv_letterbox_u8``, ``hdrtv_preprocess``)."""
        sh, sw = fmt.frame_hw(frame)
        out_w, out_h = (sw, sh) if letterbox_to is None else (int(letterbox_to[0]), int(letterbox_to[1]))
        planes = fmt.planes(self._upload_planes(fmt, frame), sh, sw)
        self._ensure_buffers(out_h, out_w)
        st, dst = self._stream(), (self._gpu_input.data_ptr(), self._gpu_cond.data_ptr())
        if (sw, sh) == (out_w, out_h):
            self._chk(getattr(self._lib, fmt.entry)(self._ctx, st, *planes, sh, sw, *dst), fmt.entry)
        elif fmt.family == "ycbcr10":
            self._chk(self._lib.hdrtv_preprocess_ycbcr10_letterboxed(self._ctx, st, *planes, sh, sw, out_h, out_w, *dst),
                      "hdrtv_preprocess_ycbcr10_letterboxed")
        else:
            if getattr(self, "_yuv_bgr_shape", None) != (sh, sw):
                self._yuv_bgr = torch.empty((sh, sw, 3), dtype=torch.uint8, device=self.device)
                self._yuv_bgr_shape = (sh, sw)
            self._chk(self._lib.hdrtv_yuv420_to_bgr_u8(self._ctx, st, *planes, sh, sw, self._yuv_bgr.data_ptr()), "hdrtv_yuv420_to_bgr_u8")
            self._chk(self._lib.hdrtv_letterbox_u8(self._ctx, st, self._yuv_bgr.data_ptr(), sh, sw, self._gpu_raw.data_ptr(), out_h, out_w),
                      "hdrtv_letterbox_u8")
            self._chk(self._lib.hdrtv_preprocess(self._ctx, st, self._gpu_raw.data_ptr(), out_h, out_w, *dst), "hdrtv_preprocess")
        return self._gpu_input, self._gpu_cond

    def preprocess_yuv420(self, frame, *, layout="i420", matrix=709, full_range=False):
        """``preprocess`` of an 8-bit 4:2:0 frame: ``frame`` is u8 ``(H*3//2, W)``, the planes back to back as ``ffmpeg -f
        rawvideo -pix_fmt yuv420p`` (``layout="i420"``) or ``nv12`` writes them.  The conversion to RGB (include/hdrtv_mi355x.h:
        ``matrix`` 601 / 709 / 2020, limited or ``full_range``) runs inside the preprocess kernel; the result equals
        ``preprocess`` of the converted BGR frame bit for bit.  Returns the same processor-owned ``(tensor, cond)``."""
        return self._preprocess_planes(_in_format("yuv420", layout, matrix, full_range), frame)

    def preprocess_yuv420_letterboxed(self, frame, out_w, out_h, *, layout="i420", matrix=709, full_range=False):
        """``preprocess_letterboxed`` of an 8-bit 4:2:0 frame: converted to BGR on the device at the source size
        (``hdrtv_yuv420_to_bgr_u8``), then ``hdrtv_letterbox_u8`` and ``hdrtv_preprocess``.  Equal sizes: ``preprocess_yuv420``."""
        return self._preprocess_planes(_in_format("yuv420", layout, matrix, full_range), frame, (out_w, out_h))

    def preprocess_ycbcr10(self, frame, *, pix_fmt, matrix=709, full_range=False):
        """``preprocess`` of a 10-bit Y'CbCr frame: ``frame`` is u16, the planes back to back at their minimum pitches as ``ffmpeg
        -f rawvideo -pix_fmt <pix_fmt>`` writes them -- ``(H*3//2, W)`` for ``p010le`` and ``yuv420p10le``, ``(2*H, W)`` for
        ``yuv422p10le``.  The conversion to RGB (include/hdrtv_mi355x.h: ``matrix`` 601 / 709 / 2020, limited or ``full_range``)
        runs inside the preprocess kernel and keeps the ten bits: the tensor holds ``fp16(code / 1023)``.  Returns the same
        processor-owned ``(tensor, cond)``."""
        return self._preprocess_planes(_in_format("ycbcr10", pix_fmt, matrix, full_range), frame)

    def preprocess_ycbcr10_letterboxed(self, frame, out_w, out_h, *, pix_fmt, matrix=709, full_range=False):
        """``preprocess_letterboxed`` of a 10-bit Y'CbCr frame, at ten bits: the planes are uploaded at THEIR size and one kernel
        (``hdrtv_preprocess_ycbcr10_letterboxed``) converts, resizes and pastes them into the ``out_h x out_w`` tensor, which holds
        ``fp16(code / 1023)`` of the letterboxed codes (include/hdrtv_mi355x.h states the rule; a shrink beyond 4x on an axis is
        refused).  Equal sizes: ``preprocess_ycbcr10``."""
        return self._preprocess_planes(_in_format("ycbcr10", pix_fmt, matrix, full_range), frame, (out_w, out_h))

    @torch.inference_mode()
    def infer(self, input_cond):
        """hdrtvnet_torch.py:2301-2346.  Returns ``(out, agcm_out)`` like the eager model; both are
        processor-owned and overwritten by the next call (as HDRTVNetTensorRT's output is)."""
        tensor, cond = input_cond
        if tensor.dtype != self._dtype or cond.dtype != self._dtype or not tensor.is_cuda:
            raise ValueError(f"infer expects the {self.precision if self._fp32 else 'fp16'} CUDA tensors returned by preprocess()")
        h, w = int(tensor.shape[2]), int(tensor.shape[3])
        self._ensure_buffers(h, w)
        tensor = tensor.contiguous()
        cond = cond.contiguous()
        if tuple(cond.shape[2:]) != (max(1, h // 4), max(1, w // 4)):
            raise ValueError("cond must be [1,3,H//4,W//4]")
        if self._use_cuda_graphs and not self._profiling:
            return self._infer_graph(tensor, cond, h, w)
        self._chk(self._lib.hdrtv_infer(self._ctx, self._stream(), tensor.data_ptr(), cond.data_ptr(), h, w,
                                        self._gpu_out.data_ptr(), self._out_dt,
                                        self._gpu_agcm.data_ptr()), "hdrtv_infer")
        return self._gpu_out, self._gpu_agcm

    def _infer_graph(self, tensor, cond, h, w):
        """hdrtvnet_torch.py:2306-2331: static input buffers, one capture per shape, replay afterwards.  The ~66 launches of
        hdrtv_infer are captured into a hipGraph on torch's capture stream (the C ABI is stream-ordered and allocation-free
        after hdrtv_reserve); a capture failure falls back to eager launches as the reference does."""
        if tensor.data_ptr() != self._gpu_input.data_ptr():
            self._gpu_input.copy_(tensor)
        if cond.data_ptr() != self._gpu_cond.data_ptr():
            self._gpu_cond.copy_(cond)

        def launch():
            self._chk(self._lib.hdrtv_infer(self._ctx, self._stream(), self._gpu_input.data_ptr(), self._gpu_cond.data_ptr(), h, w,
                                            self._gpu_out.data_ptr(), self._out_dt,
                                            self._gpu_agcm.data_ptr()), "hdrtv_infer")

        g = self._graphs.get((h, w))
        if g is None:
            launch()                                   # eager once: one-time kernel attributes are set outside the capture
            torch.cuda.synchronize(self.device)
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    launch()
            except Exception as exc:  # noqa: BLE001
                print(f"WARNING: hipGraph capture failed ({exc}); continuing with eager launches.")
                self._use_cuda_graphs = False
                launch()
                return self._gpu_out, self._gpu_agcm
            self._graphs[(h, w)] = g
        g.replay()
        return self._gpu_out, self._gpu_agcm

    @torch.inference_mode()
    def objective_metrics(self, pred, ref, peak_nits=1000.0):
        """PSNR / SSIM / dE-ITP between two ``[1,3,H,W]`` (or ``[3,H,W]``) CUDA tensors in unit range, as the reference's
        ``_psnr_bgr`` / ``_ssim_bgr`` / ``_delta_e_itp_bgr`` compute them (gui_objective_metrics.py:438-528) -> a dict
        with the reference's metric keys (``psnr_db``, ``sssim``, ``delta_e_itp``).  Parity unpinned (cv2 module)."""
        a = pred[0] if isinstance(pred, (tuple, list)) else pred
        b = ref[0] if isinstance(ref, (tuple, list)) else ref
        if a.shape != b.shape or a.shape[-3] != 3:
            raise ValueError("objective_metrics expects two tensors of the same [.., 3, H, W] shape")
        dt = torch.float32 if (a.dtype == torch.float32 or b.dtype == torch.float32) else torch.float16
        a = a.to(device=self.device, dtype=dt).contiguous()
        b = b.to(device=self.device, dtype=dt).contiguous()
        h, w = int(a.shape[-2]), int(a.shape[-1])
        out = (C.c_double * 3)()
        self._chk(self._lib.hdrtv_metrics(self._ctx, self._stream(), a.data_ptr(), b.data_ptr(),
                                          _dtype_code(a), h, w, float(peak_nits), out),
                  "hdrtv_metrics")
        return {"psnr_db": float(out[0]), "sssim": float(out[1]), "delta_e_itp": float(out[2])}

    def _rgb48_on_device(self, frame, what):
        """A u16 ``(H, W, 3)`` RGB48 frame (device tensor, host tensor or numpy array) as a contiguous device tensor."""
        if not isinstance(frame, torch.Tensor):
            frame = torch.from_numpy(np.ascontiguousarray(frame))
        if frame.dtype != torch.uint16 or frame.ndim != 3 or frame.shape[2] != 3 or frame.shape[0] < 1 or frame.shape[1] < 1:
            raise ValueError(f"{what} expects uint16 (H, W, 3) frames of RGB48 codes")
        return frame.to(self.device).contiguous()

    @torch.inference_mode()
    def full_reference_metrics(self, pred_u16, ref_u16, max_side=_L.FR_MAX_SIDE, peak_nits=1000.0, crop=True, normalized=True):
        """The metrics the reference's compare dialog, session log and quality benchmark report (``_compute_full_reference_metrics``,
        gui_objective_metrics.py:617-677), between two RGB48 frames u16 ``(H, W, 3)`` of the same size -- the delivered codes and a
        ground truth the caller has brought to that size: shared black borders cropped (``crop``), both frames reduced with
        INTER_AREA until the longer side is ``max_side``, the three metrics on the u16 codes, and (``normalized``) the three again
        after the prediction's per-channel mean and standard deviation are matched to the ground truth's.  All of it on the device
        (``hdrtv_full_reference_metrics``; include/hdrtv_mi355x.h states the rules).  ``crop=False, normalized=False`` is the
        reference's live path (gui_pipeline_worker_objective.py:60-73).  Returns a dict with the reference's keys (``psnr_db``,
        ``sssim``, ``delta_e_itp``, ``psnr_norm_db``, ``sssim_norm``, ``delta_e_itp_norm``: the last three ``None`` without
        ``normalized``), its ``obj_note``, and ``crop_rect`` = (top, bottom, left, right) and ``eval_size`` = (h, w).
        Synchronises the current stream."""
        a = self._rgb48_on_device(pred_u16, "full_reference_metrics")
        b = self._rgb48_on_device(ref_u16, "full_reference_metrics")
        if a.shape != b.shape:
            raise ValueError("full_reference_metrics expects two frames of the same size")
        h, w = int(a.shape[0]), int(a.shape[1])
        flags = (_L.FR_CROP if crop else 0) | (_L.FR_NORMALIZED if normalized else 0)
        out, info = (C.c_double * 6)(), (C.c_int * 6)()
        self._chk(self._lib.hdrtv_full_reference_metrics(self._ctx, self._stream(), a.data_ptr(), b.data_ptr(), h, w, int(max_side),
                                                         float(peak_nits), flags, out, info), "hdrtv_full_reference_metrics")
        rect = tuple(int(v) for v in info[:4])
        norm = [float(v) for v in out[3:6]] if normalized else [None] * 3
        return {"psnr_db": float(out[0]), "sssim": float(out[1]), "delta_e_itp": float(out[2]),
                "psnr_norm_db": norm[0], "sssim_norm": norm[1], "delta_e_itp_norm": norm[2],
                "obj_note": _L.FR_NOTE.format(_L.FR_NOTE_CROPPED if rect != (0, h, 0, w) else ""),
                "crop_rect": rect, "eval_size": (int(info[4]), int(info[5]))}

    @torch.inference_mode()
    def rgb48_border_counts(self, pred_u16, ref_u16):
        """``hdrtv_rgb48_border_counts``: a device u32-as-int32 ``(2, H + W)`` tensor, per frame the signal pixels (max(R, G, B) >= 132)
        of each row, then of each column.  Stream-ordered, no synchronisation."""
        a, b = self._rgb48_on_device(pred_u16, "rgb48_border_counts"), self._rgb48_on_device(ref_u16, "rgb48_border_counts")
        if a.shape != b.shape:
            raise ValueError("rgb48_border_counts expects two frames of the same size")
        h, w = int(a.shape[0]), int(a.shape[1])
        counts = torch.empty((2, h + w), dtype=torch.int32, device=self.device)
        self._chk(self._lib.hdrtv_rgb48_border_counts(self._ctx, self._stream(), a.data_ptr(), b.data_ptr(), h, w, counts.data_ptr()),
                  "hdrtv_rgb48_border_counts")
        return counts

    @torch.inference_mode()
    def rgb48_area_reduce(self, src_u16, out_w, out_h, rect=None):
        """``hdrtv_rgb48_area_reduce``: the rows [top, bottom) and columns [left, right) of ``rect`` (default: the whole frame) of a
        u16 ``(H, W, 3)`` frame reduced to ``out_h`` x ``out_w`` with the 16-bit INTER_AREA rule, at most 16x per axis.  Returns a
        new device u16 tensor; stream-ordered, no synchronisation."""
        src = self._rgb48_on_device(src_u16, "rgb48_area_reduce")
        h, w = int(src.shape[0]), int(src.shape[1])
        top, bottom, left, right = (0, h, 0, w) if rect is None else (int(v) for v in rect)
        out_w, out_h = int(out_w), int(out_h)
        dst = torch.empty((max(out_h, 1), max(out_w, 1), 3), dtype=torch.uint16, device=self.device)
        self._chk(self._lib.hdrtv_rgb48_area_reduce(self._ctx, self._stream(), src.data_ptr(), h, w, left, top, right - left, bottom - top,
                                                    dst.data_ptr(), out_h, out_w), "hdrtv_rgb48_area_reduce")
        return dst

    @torch.inference_mode()
    def rgb48_grade_match(self, pred_u16, ref_u16, peak_nits=1000.0):
        """``hdrtv_rgb48_grade_match``: the gains and biases that match the prediction's per-channel mean and standard deviation to the
        ground truth's, from exact histograms -> a float32 numpy array [12]: gain[3], bias[3] on the codes, gain[3], bias[3] on
        absolute RGB.  Synchronises the current stream."""
        a, b = self._rgb48_on_device(pred_u16, "rgb48_grade_match"), self._rgb48_on_device(ref_u16, "rgb48_grade_match")
        if a.shape != b.shape:
            raise ValueError("rgb48_grade_match expects two frames of the same size")
        out = (C.c_float * 12)()
        self._chk(self._lib.hdrtv_rgb48_grade_match(self._ctx, self._stream(), a.data_ptr(), b.data_ptr(), int(a.shape[0]), int(a.shape[1]),
                                                    float(peak_nits), out), "hdrtv_rgb48_grade_match")
        return np.array(list(out), dtype=np.float32)

    @torch.inference_mode()
    def postprocess(self, output):
        """hdrtvnet_torch.py:2351-2368.  Returns a zero-copy view of processor-owned pinned memory."""
        if isinstance(output, (tuple, list)):
            output = output[0]
        h, w = int(output.shape[-2]), int(output.shape[-1])
        self._ensure_buffers(h, w)
        output = output.contiguous()
        if output.dtype not in (torch.float16, torch.float32):
            raise ValueError("postprocess expects an fp16 or fp32 tensor")
        self._chk(self._lib.hdrtv_post_u8(self._ctx, self._stream(), output.data_ptr(), _dtype_code(output), h, w,
                                          self._gpu_u8.data_ptr()), "hdrtv_post_u8")
        self._pin_output.copy_(self._gpu_u8, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self._pin_output.numpy()

    @torch.inference_mode()
    def postprocess_rgb48_scaled(self, output, out_w, out_h, pq=False, peak_nits=1000.0, antiring=0.0, cas=0.0, scaler="lanczos",
                                 fsr_sharpness=_L.FSR_SHARPNESS, downscaler=None, down_antiring=0.0, film_grain=0.0, grain_seed=0.0):
        """RGB48 at the display size: the u16 codes of ``hdrtv_post_rgb48`` (``pq=True``: of
        ``hdrtv_post_pq_rgb48`` at ``peak_nits``) upscaled to ``out_h`` x ``out_w`` by ``hdrtv_post_rgb48_scaled`` in one kernel.
        The six options after ``peak_nits`` choose another scaler, or one for a size below the processing size (``lib.ScaleOptions``
        describes them; its ``plan`` has the refusals, each a ``ValueError``).  ``film_grain`` / ``grain_seed``: the reference's film
        grain in the chain (``lib.check_film_grain``, ``lib.film_grain_seed``; the ``_grain`` entry points, ``hdrtv_post_rgb48_grain``
        at equal sizes).  Returns a new device u16 ``(out_h, out_w, 3)`` tensor; stream-ordered on the current stream, no
        synchronisation."""
        if isinstance(output, (tuple, list)):
            output = output[0]
        if output.dtype not in (torch.float16, torch.float32):
            raise ValueError("postprocess_rgb48_scaled expects an fp16 or fp32 tensor")
        h, w = int(output.shape[-2]), int(output.shape[-1])
        out_w, out_h = int(out_w), int(out_h)
        opts = _L.scale_options(antiring, cas, scaler, fsr_sharpness, downscaler, down_antiring)
        # equal sizes: the entry point itself writes the unscaled kernel's bytes (and takes pq, which hdrtv_post_rgb48 does not)
        intensity = _L.check_grain_chain(film_grain, opts.scaler, opts.downscaler)
        if intensity:
            seed = _L.check_grain_seed(grain_seed)
            plan = opts.plan(w, h, out_w, out_h, intensity, seed) or _L.ScalePlan("hdrtv_post_rgb48_scaled_grain", (0, 0, intensity, seed))
        else:
            plan = opts.plan(w, h, out_w, out_h) or _L.ScalePlan("hdrtv_post_rgb48_scaled", ())
        output = output.contiguous()
        dst = torch.empty((out_h, out_w, 3), dtype=torch.uint16, device=self.device)
        self._chk(getattr(self._lib, plan.entry)(self._ctx, self._stream(), output.data_ptr(), _dtype_code(output), h, w, 1 if pq else 0,
                                                 float(peak_nits), dst.data_ptr(), out_h, out_w, *plan.args), plan.entry)
        return dst

    @torch.inference_mode()
    def postprocess_film_grain(self, rgb48, intensity=_L.FILM_GRAIN_INTENSITY, seed=0.0):
        """Grained RGB48 codes: ``hdrtv_rgb48_film_grain`` on a device u16 ``(H, W, 3)`` tensor of codes (what
        ``hdrtv_post_rgb48`` / ``postprocess_rgb48_scaled`` write), grain positions over its ``H`` x ``W``, ``seed`` =
        ``lib.film_grain_seed(stream_seed, frame_index)``.  Returns a new device tensor of the same shape; the source is not
        touched.  Stream-ordered on the current stream, no synchronisation."""
        if not isinstance(rgb48, torch.Tensor) or rgb48.dtype != torch.uint16 or rgb48.ndim != 3 or rgb48.shape[2] != 3 or not rgb48.is_cuda:
            raise ValueError("postprocess_film_grain expects a device uint16 (H, W, 3) tensor of RGB48 codes")
        if rgb48.shape[0] < 1 or rgb48.shape[1] < 1:
            raise ValueError("postprocess_film_grain expects a non-empty frame")
        intensity, seed = _L.check_film_grain(intensity), _L.check_grain_seed(seed)
        src = rgb48.contiguous()
        dst = torch.empty_like(src)
        self._chk(self._lib.hdrtv_rgb48_film_grain(self._ctx, self._stream(), src.data_ptr(), int(src.shape[0]), int(src.shape[1]),
                                                   intensity, seed, dst.data_ptr()), "hdrtv_rgb48_film_grain")
        return dst

    @torch.inference_mode()
    def postprocess_tonemap(self, rgb48, tone):
        """Tone-mapped RGB48 codes: ``hdrtv_rgb48_tonemap`` on a device u16 ``(H, W, 3)`` tensor of BT.2020 PQ
        codes (what ``hdrtv_post_rgb48`` / ``postprocess_rgb48_scaled`` write for the model's output) with the curve of the
        ``lib.ToneMapping`` ``tone`` (``lib.tone_mapping``; None: a copy of the codes).  Returns a new device tensor of the same
        shape; the source is not touched.  Stream-ordered on the current stream; the first use of a curve uploads its table and
        waits for that, later calls do not synchronise."""
        if not isinstance(rgb48, torch.Tensor) or rgb48.dtype != torch.uint16 or rgb48.ndim != 3 or rgb48.shape[2] != 3 or not rgb48.is_cuda:
            raise ValueError("postprocess_tonemap expects a device uint16 (H, W, 3) tensor of RGB48 codes")
        if rgb48.shape[0] < 1 or rgb48.shape[1] < 1:
            raise ValueError("postprocess_tonemap expects a non-empty frame")
        src = rgb48.contiguous()
        if tone is None:
            return src.clone()
        gain = self._tone_gain(tone)
        dst = torch.empty_like(src)
        with torch.cuda.device(self.device):
            self._chk(self._lib.hdrtv_rgb48_tonemap(self._ctx, self._stream(), src.data_ptr(), int(src.shape[0]), int(src.shape[1]), gain,
                                                    dst.data_ptr()), "hdrtv_rgb48_tonemap")
        return dst

    @torch.inference_mode()
    def postprocess_deband(self, rgb48, deband_range=_L.DEBAND_RANGE, deband_threshold=_L.DEBAND_THRESHOLD, seed=0):
        """Debanded RGB48 codes: ``hdrtv_rgb48_deband`` on a device u16 ``(H, W, 3)`` tensor of codes (what
        ``hdrtv_post_rgb48`` / ``postprocess_rgb48_scaled`` write).  Returns a new device tensor of the same shape; the source is
        not touched.  Stream-ordered on the current stream, no synchronisation."""
        if not isinstance(rgb48, torch.Tensor) or rgb48.dtype != torch.uint16 or rgb48.ndim != 3 or rgb48.shape[2] != 3 or not rgb48.is_cuda:
            raise ValueError("postprocess_deband expects a device uint16 (H, W, 3) tensor of RGB48 codes")
        if rgb48.shape[0] < 1 or rgb48.shape[1] < 1:
            raise ValueError("postprocess_deband expects a non-empty frame")
        c = _L.output_cleanup(True, deband_range, deband_threshold)
        seed = int(seed)
        if not 0 <= seed <= 0xFFFFFFFF:
            raise ValueError("seed must be a u32")
        src = rgb48.contiguous()
        dst = torch.empty_like(src)
        self._chk(self._lib.hdrtv_rgb48_deband(self._ctx, self._stream(), src.data_ptr(), int(src.shape[0]), int(src.shape[1]),
                                               c.deband_range, c.deband_threshold, seed, dst.data_ptr()), "hdrtv_rgb48_deband")
        return dst

    @torch.inference_mode()
    def postprocess_ycbcr10(self, output, pix_fmt="p010le", siting="left", pq=False, peak_nits=1000.0, dither="none"):
        """10-bit limited-range BT.2020nc Y'CbCr for an encoder: ``hdrtv_post_ycbcr10`` converts the u16 codes
        of ``hdrtv_post_rgb48`` (``pq=True``: of ``hdrtv_post_pq_rgb48`` at ``peak_nits``) in one kernel, without an RGB48
        intermediate.  ``pix_fmt`` ``p010le`` / ``yuv420p10le`` / ``yuv422p10le``; ``siting`` of 4:2:0 chroma ``left`` (MPEG-2 /
        H.264, ffmpeg's default) or ``topleft`` (BT.2100 / HDR10).  Returns a new contiguous 1-D device u16 tensor, the planes back
        to back (``lib.out_frame_bytes`` bytes); stream-ordered on the current stream, no synchronisation.  ``dither="ordered"``:
        the ordered dither of INTEGRATION.md 5f (``hdrtv_post_ycbcr10_ex``); ``"floyd_steinberg"``: its error diffusion
        (``hdrtv_post_ycbcr10_fs``, through a scratch kept by the processor); ``"none"``: the bytes of before."""
        if isinstance(output, (tuple, list)):
            output = output[0]
        if output.dtype not in (torch.float16, torch.float32):
            raise ValueError("postprocess_ycbcr10 expects an fp16 or fp32 tensor")
        cleanup = _L.output_cleanup(dither=dither)
        out = _L.output_format(pix_fmt, siting, int(output.shape[-2]), int(output.shape[-1]))
        if out.is_rgb48:
            raise ValueError("postprocess_ycbcr10 writes p010le, yuv420p10le or yuv422p10le")
        output = output.contiguous()
        dst = torch.empty(out.shape, dtype=torch.uint16, device=self.device)
        args = (self._ctx, self._stream(), output.data_ptr(), _dtype_code(output), out.h, out.w, 1 if pq else 0, float(peak_nits),
                *out.planes(dst.data_ptr()))
        if cleanup.error_diffusion:
            self._chk(self._lib.hdrtv_post_ycbcr10_fs(*args, self._fs_scratch("postprocess_ycbcr10", out)), "hdrtv_post_ycbcr10_fs")
        else:
            self._chk(self._lib.hdrtv_post_ycbcr10_ex(*args, cleanup.dither_code), "hdrtv_post_ycbcr10_ex")
        return dst

    @torch.inference_mode()
    def process(self, frame_bgr):
        tensor, cond = self.preprocess(frame_bgr)
        return self.postprocess(self.infer((tensor, cond)))

    @torch.inference_mode()
    def process_yuv420(self, frame, *, layout="i420", matrix=709, full_range=False):
        """``process`` of an 8-bit 4:2:0 frame (``preprocess_yuv420``): u8 BGR out, as ``process``."""
        tensor, cond = self.preprocess_yuv420(frame, layout=layout, matrix=matrix, full_range=full_range)
        return self.postprocess(self.infer((tensor, cond)))

    @torch.inference_mode()
    def process_ycbcr10(self, frame, *, pix_fmt, matrix=709, full_range=False):
        """``process`` of a 10-bit Y'CbCr frame (``preprocess_ycbcr10``): u8 BGR out, as ``process``."""
        tensor, cond = self.preprocess_ycbcr10(frame, pix_fmt=pix_fmt, matrix=matrix, full_range=full_range)
        return self.postprocess(self.infer((tensor, cond)))

    @torch.inference_mode()
    def process_timed(self, frame_bgr):
        """hdrtvnet_torch.py:2379-2395 -> (output, pre_ms, run_ms, post_ms)."""
        t0 = time.perf_counter()
        tensor, cond = self.preprocess(frame_bgr)
        torch.cuda.synchronize(self.device)
        t1 = time.perf_counter()
        out = self.infer((tensor, cond))
        torch.cuda.synchronize(self.device)
        t2 = time.perf_counter()
        output = self.postprocess(out)
        t3 = time.perf_counter()
        return output, (t1 - t0) * 1000.0, (t2 - t1) * 1000.0, (t3 - t2) * 1000.0

    def warmup_compile(self, width=1920, height=1080):
        """hdrtvnet_torch.py:2400-2469: only meaningful when torch.compile is active; never here."""
        return None

    def end_profiling(self):
        return None

    # ------------------------------------------------------------------ extras (tests / bench)
    def tap(self, name):
        """Internal activation by name (after infer) as a torch tensor copy: NHWC taps come back
        as [C,H,W] float32 for direct comparison with the oracle."""
        p, c, h, w, lay = C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._chk(self._lib.hdrtv_get_tap(self._ctx, name.encode(), C.byref(p), C.byref(c), C.byref(h), C.byref(w),
                                          C.byref(lay)), "hdrtv_get_tap")
        n = c.value * h.value * w.value
        torch.cuda.synchronize(self.device)
        if lay.value in (0, 1):
            buf = torch.empty(n, dtype=torch.float16, device=self.device)
        elif lay.value == 4:
            buf = torch.empty(n, dtype=torch.uint8, device=self.device)
        elif lay.value == 5:
            buf = torch.empty(n, dtype=torch.int8, device=self.device)
        else:
            buf = torch.empty(n, dtype=torch.float32, device=self.device)
        _hip_memcpy_d2d(buf.data_ptr(), p.value, buf.numel() * buf.element_size())
        torch.cuda.synchronize(self.device)
        if lay.value in (0, 5):          # NHWC; int8 taps are codes q - 128 of the reading layer's quantiser
            return buf.view(h.value, w.value, c.value).permute(2, 0, 1).float().cpu()
        return buf.view(c.value, h.value, w.value).float().cpu()

    def _tap_device(self, name):
        """Flat device copy of an internal activation (no layout conversion)."""
        p, c, h, w, lay = C.c_void_p(), C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._chk(self._lib.hdrtv_get_tap(self._ctx, name.encode(), C.byref(p), C.byref(c), C.byref(h), C.byref(w),
                                          C.byref(lay)), "hdrtv_get_tap")
        dt = {0: torch.float16, 1: torch.float16, 4: torch.uint8, 5: torch.int8}.get(lay.value, torch.float32)
        buf = torch.empty(c.value * h.value * w.value, dtype=dt, device=self.device)
        torch.cuda.synchronize(self.device)
        _hip_memcpy_d2d(buf.data_ptr(), p.value, buf.numel() * buf.element_size())
        torch.cuda.synchronize(self.device)
        return buf

    @torch.inference_mode()
    def calibrate_hg_w8a8(self, frames):
        """Activation ranges for a W8A8 HG checkpoint, the reference's ``calibrate_w8a8(method="max")``
        (hdrtvnet_torch.py:1001-1099: running min / max of every quantised layer's input over the calibration set),
        taken from this fp16 model's own activations on ``frames`` (u8 BGR).  Returns ``{group: (lo, hi)}`` for
        ``weights.hg_w8a8_state`` / ``hg_w8a8_checkpoint``; layers that read one tensor or a concatenation share a range."""
        if self._hg_state_fp is None:
            raise RuntimeError("calibrate_hg_w8a8 needs a model loaded with floating-point HG weights")
        members = {"p1": ("hg.p1",), "conv2+up4": ("hg.conv2", "hg.up4"), "p3": ("hg.p3",), "conv3_2+up3": ("hg.conv3_2", "hg.up3"), "p4": ("hg.p4",),
                   "conv4_2+up2": ("hg.conv4_2", "hg.up2"), "p5": ("hg.p5",), "conv5_2+up1": ("hg.conv5_2", "hg.up1"),
                   "pc": ("hg.pc",), "conv_code2": ("hg.conv_code2",), "conv6": ("hg.conv6",), "conv7": ("hg.conv7",),
                   "conv8": ("hg.conv8",), "conv9": ("hg.conv9",)}
        assert list(members) == list(_W.HG_W8A8_GROUPS)
        ranges = {g: [0.0, 0.0] for g in members}
        for f in frames:
            self.infer(self.preprocess(f))
            for g, taps in members.items():
                for t in taps:
                    v = self._tap_device(t)
                    ranges[g][0] = min(ranges[g][0], float(v.amin()))
                    ranges[g][1] = max(ranges[g][1], float(v.amax()))
        return {g: (lo, hi) for g, (lo, hi) in ranges.items()}

    def hg_w8a8_checkpoint(self, ranges):
        """This model's HG weights as a W8A8 state (reference key layout) for ``hg_weights=``; see calibrate_hg_w8a8."""
        if self._hg_state_fp is None:
            raise RuntimeError("hg_w8a8_checkpoint needs a model loaded with floating-point HG weights")
        return _W.hg_w8a8_state(self._hg_state_fp, ranges)

    def set_hg_mask_r(self, r=0.75):
        """``HG_Composite(mask_r=...)`` (HG_Composite_arch.py:21): threshold base of the highlight mask."""
        self._chk(self._lib.hdrtv_set_hg_mask_r(self._ctx, float(r)), "hdrtv_set_hg_mask_r")
        self._graphs.clear()          # a captured hipGraph has the old threshold baked into its kernel arguments

    def set_variant(self, name, value):
        """Developer / test switch (``hdrtv_set_variant``): which of several equivalent kernels a layer runs on."""
        self._chk(self._lib.hdrtv_set_variant(self._ctx, name.encode(), int(value)), "hdrtv_set_variant")
        self._graphs.clear()          # a captured hipGraph replays the launches it was captured with

    def get_variant(self, name):
        v = C.c_int()
        self._chk(self._lib.hdrtv_get_variant(self._ctx, name.encode(), C.byref(v)), "hdrtv_get_variant")
        return v.value

    def profile_enable(self, on=True):
        """Per-launch HIP-event timing of subsequent infer() calls (bench.py roofline).  While it is on, infer() launches
        eagerly even with ``use_cuda_graphs``: a graph replay records no events, and a graph captured with profiling on
        would carry the event records."""
        self._chk(self._lib.hdrtv_profile_enable(self._ctx, 1 if on else 0), "hdrtv_profile_enable")
        self._profiling = bool(on)

    def profile_read(self):
        """[(layer, kernel, ms, macs, bytes)] of the last infer(); synchronises on its events."""
        n = self._lib.hdrtv_profile_get(self._ctx, -1, None, None, None, None, None)
        out = []
        for i in range(max(n, 0)):
            layer, kern, ms, macs, nbytes = C.c_char_p(), C.c_char_p(), C.c_float(), C.c_double(), C.c_double()
            self._chk(self._lib.hdrtv_profile_get(self._ctx, i, C.byref(layer), C.byref(kern), C.byref(ms),
                                                  C.byref(macs), C.byref(nbytes)), "hdrtv_profile_get")
            out.append((layer.value.decode(), kern.value.decode(), ms.value, macs.value, nbytes.value))
        return out

    def profile_tiles(self):
        """[(layer, kernel, executed, total)] of the last profiled infer(): the tiles a launch that walked an HG need list
        computed, and the tiles of a dense launch; total = 0 for a launch without a list (or whose list was dropped)."""
        n = self._lib.hdrtv_profile_get(self._ctx, -1, None, None, None, None, None)
        out = []
        for i in range(max(n, 0)):
            layer, kern, done, total = C.c_char_p(), C.c_char_p(), C.c_int(), C.c_int()
            self._chk(self._lib.hdrtv_profile_get(self._ctx, i, C.byref(layer), C.byref(kern), None, None, None), "hdrtv_profile_get")
            self._chk(self._lib.hdrtv_profile_tiles(self._ctx, i, C.byref(done), C.byref(total)), "hdrtv_profile_tiles")
            out.append((layer.value.decode(), kern.value.decode(), done.value, total.value))
        return out

    def execution_summary(self, profile=None):
        """What the last profiled ``infer()`` ran on, by kernel tag: MACs (and launches) on int8 MFMA, as fake-quant on fp16 MFMA
        (W8A8 layers inside ``le_*_rows<fq>``), as fp32 fake-quant (the AGCM classifier of a full-QAT checkpoint) and on fp16
        MFMA.  ``profile`` = ``profile_read()`` of a run with profiling enabled (read here when omitted)."""
        return summarize_profile(profile if profile is not None else self.profile_read())

    def infer_stats(self):
        n, m = C.c_int(), C.c_double()
        self._lib.hdrtv_infer_stats(self._ctx, C.byref(n), C.byref(m))
        return n.value, m.value

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.hdrtv_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _arch_hr():
    from . import arch
    return arch.hr_params()


_hip = None


YUV_LAYOUTS, YCBCR10_IN_FORMATS, ycbcr10_frame_shape, ycbcr10_frame_hw = _L.YUV_LAYOUTS, _L.YCBCR10_IN_FORMATS, _L.ycbcr10_frame_shape, _L.ycbcr10_frame_hw

_BGR24 = _L.input_format("bgr24")


def _in_format(family, name, matrix, full_range):
    """The ``lib.InputFormat`` behind the ``layout=`` / ``pix_fmt=`` argument of the ``*_yuv420`` / ``*_ycbcr10`` methods."""
    names = YUV_LAYOUTS if family == "yuv420" else YCBCR10_IN_FORMATS
    if str(name).lower() not in names:
        raise ValueError(f"{'layout' if family == 'yuv420' else 'pix_fmt'} must be one of {sorted(names)}")
    return _L.input_format(name, matrix, full_range)


def _hip_memcpy_d2d(dst, src, nbytes):
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpy.restype = C.c_int
    rc = _hip.hipMemcpy(dst, src, nbytes, 3)   # hipMemcpyDeviceToDevice
    if rc != 0:
        raise RuntimeError(f"hipMemcpy failed: {rc}")
