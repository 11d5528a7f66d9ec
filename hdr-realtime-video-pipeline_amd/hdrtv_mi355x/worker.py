"""Headless counterparts of the reference's pipeline-worker mixins for the hot path.

  _load_model / _silent_warmup   src/gui_pipeline_worker_model.py:39-257   (AMD branch 202-228)
  _process_frame                 src/gui_pipeline_worker_frame_processing.py:168-331
  _stage_hdr_display_tensor      src/gui_pipeline_worker_frame_processing.py:118-156
  _tensor_to_rgb48_bytes + ring  src/gui_pipeline_worker_feeders.py:38-70, 125-249
  _hdr_feeder_fn (core)          src/gui_pipeline_worker_feeders.py:440-496

Same names, argument meaning and error behaviour (``_load_model`` swallows backend exceptions
into a status message and returns False), without PyQt/cv2/mpv: status messages go to a list
or callback, the display sink is any callable taking a ``PinnedFrame``.  Frames that are not at
the processing size are letterboxed on the device (``preprocess_letterboxed``; 10-bit Y'CbCr frames
where ``set_input_format(..., letterbox=True)`` asked for it).
"""
from __future__ import annotations

import ctypes as C
import os
import queue as _queue
import sys
import threading
import time

import numpy as np
import torch

from . import lib as _L
from .lightlevel import ContentLightLevel
from .lib import YCBCR10_IN_FORMATS, input_format
from .processor import HDRTVNetMI355X, _dtype_code

_RING_FRAMES = max(2, min(8, int(os.environ.get("HDRTVNET_FEEDER_GPU_RGB48_RING_FRAMES", "3") or 3)))

# preset table: the subset of gui_config.PRECISIONS (src/gui_config.py:19-160) this backend serves
def _int8_preset(recipe, suffix):
    return {"precision": f"int8-{recipe}", "model": f"original/pytorch_int8/hg/HR_HG_original_int8_{recipe}{suffix}.pt",
            "model_nohg": f"original/pytorch_int8/hr/HR_original_int8_{recipe}{suffix}.pt"}


PRECISIONS = {
    "FP16": {"precision": "fp16", "model": "original/HR.pt", "model_nohg": "original/HR.pt",
             "hg_weights": "original/HG.pt"},
    "FP32": {"precision": "fp32", "model": "original/HR.pt", "model_nohg": "original/HR.pt",
             "hg_weights": "original/HG.pt"},
    # the six INT8 presets (all of gui_config.py's); the TensorRT-only FP8 presets are not served by this backend
    "INT8 Mixed (PTQ)": _int8_preset("mixed", ""),
    "INT8 Mixed (QAT)": _int8_preset("mixed", "_qat"),
    "INT8 Mixed (QAT) (Film)": _int8_preset("mixed", "_qat_film"),
    "INT8 Full (PTQ)": _int8_preset("full", ""),
    "INT8 Full (QAT)": _int8_preset("full", "_qat"),
    "INT8 Full (QAT) (Film)": _int8_preset("full", "_qat_film"),
}


class PinnedFrame:
    """_PinnedMpvFrame (feeders.py:38-70): a pinned host RGB48 frame whose ring slot is released
    after the sink has consumed it."""

    def __init__(self, worker, slot, host_ptr, shape, light_host=None):
        self._w, self._slot, self._host, self._shape = worker, slot, host_ptr, shape
        self._light_host = light_host      # the slot's pinned light level record (numpy u32 view), filled in front of the slot's commit
        self._ready_waited = self._released = False

    def wait_ready(self):
        if not self._ready_waited:
            p = self._w._processor
            p._chk(p._lib.hdrtv_ring_wait(p._ctx, self._slot), "hdrtv_ring_wait")
            self._ready_waited = True

    def buffer_view(self):
        self.wait_ready()
        n = int(np.prod(self._shape))
        return memoryview((C.c_uint16 * n).from_address(self._host)).cast("B")

    def numpy(self):
        self.wait_ready()
        n = int(np.prod(self._shape))
        return np.ctypeslib.as_array((C.c_uint16 * n).from_address(self._host)).reshape(self._shape)

    @property
    def light(self):
        """The frame's content light level record (``lib.LIGHT_WORDS`` u32; ``lightlevel.FrameLight.from_record``), a private
        copy taken once the slot is complete -- read it before ``release``; None when the worker does not measure it."""
        if self._light_host is None:
            return None
        self.wait_ready()
        return self._light_host.copy()

    def release(self):
        if self._released:
            return
        self._released = True
        try:
            self.wait_ready()
        finally:
            p = self._w._processor
            if p is not None:
                p._lib.hdrtv_ring_release(p._ctx, self._slot)


class HostFrame:
    """What ``_tensor_to_rgb48_bytes`` returns when no ring slot frees up within 250 ms (feeders.py:209-235): the frame
    in the single blocking pinned buffer, already complete; same surface as ``PinnedFrame`` (the reference returns
    ``bytes`` there, which its sink treats like a released frame)."""

    def __init__(self, array, light=None):
        self._a = array
        self.light = light                 # the frame's content light level record (a private copy), or None

    def wait_ready(self):
        return None

    def buffer_view(self):
        return memoryview(self._a).cast("B")

    def numpy(self):
        return self._a

    def release(self):
        return None


class HeadlessPipelineWorker:
    # the six checked scaler options, read from the record they are kept in
    _antiring, _cas, _scaler, _fsr_sharpness, _downscaler, _down_antiring = (
        property(lambda self, name=name: getattr(self._scale, name)) for name in _L.ScaleOptions._fields)

    def __init__(self, weights_dir, use_hg=True, proc_w=1920, proc_h=1080, hg_weights=None,
                 status_cb=None, buffer_frames=1, out_w=None, out_h=None, out_pix_fmt="rgb48le", out_siting="left",
                 light_stats=False, light_rect=None, deband=False, deband_range=_L.DEBAND_RANGE,
                 deband_threshold=_L.DEBAND_THRESHOLD, dither="none", antiring=0.0, cas=0.0, scaler="lanczos",
                 fsr_sharpness=_L.FSR_SHARPNESS, downscaler=None, down_antiring=0.0, film_grain=False, grain_stream_seed=0,
                 tone_mapping=None, target_peak=None, source_peak=_L.TONE_SOURCE_PEAK, tone_param=None):
        self._weights_dir = weights_dir
        self._use_hg = bool(use_hg)
        self._hg_override = hg_weights
        self._proc_w, self._proc_h = int(proc_w), int(proc_h)
        # the size frames are delivered at; None = the processing size.  It belongs to the sink, not to the
        # model: a hot-swap of the processing resolution keeps it.
        self._out_w, self._out_h = (int(out_w) if out_w else None), (int(out_h) if out_h else None)
        # what the sink receives, one lib.OutputFormat: "rgb48le", or 10-bit Y'CbCr ("p010le", "yuv420p10le",
        # "yuv422p10le") with the 4:2:0 chroma siting "left" / "topleft"; then a frame is a 1-D u16 view of its planes, back to back
        self._out = _L.output_format(out_pix_fmt, out_siting, self._out_h or self._proc_h, self._out_w or self._proc_w)
        # deband / dither (ordered or error diffusion) of the delivered frames, one lib.OutputCleanup; off: nothing more is launched
        # or allocated and the bytes are those of before.  With light_stats the record describes the debanded codes.
        self._cleanup = _L.output_cleanup(deband, deband_range, deband_threshold, dither, pix_fmt=self._out.pix_fmt)
        # how a frame delivered at another size than the processing size is resized: one lib.ScaleOptions, which
        # describes the six options.  "auto" strengths are resolved per frame from its two sizes (_tensor_to_rgb48_bytes), so a
        # hot-swap of the processing resolution changes them.  The limits of a scaler or downscaler are checked here against the
        # sizes known now; plain Lanczos has none, and a size below the processing size without a downscaler is refused per frame.
        self._scale = _L.scale_options(antiring, cas, scaler, fsr_sharpness, downscaler, down_antiring)
        if self._scale.scaler != "lanczos" or self._scale.downscaler is not None:
            self._scale.plan(self._proc_w, self._proc_h, self._out.w, self._out.h)
        # the reference's film grain on the delivered frames, placed as its shader chain places it: True = its
        # 0.01, or an intensity up to 0.1; off: nothing more is launched and the bytes are those of before.  Frame n of the stream
        # gets lib.film_grain_seed(grain_stream_seed, n), n = the frame_idx of _process_frame: a function of the index, so another
        # sink of the same stream (a second worker, the dispatcher's lanes) gives the frame the same grain.  With light_stats the
        # record describes the grained codes.  The chains without grain are refused here (lib.check_grain_chain).
        self._film_grain = _L.check_grain_chain(film_grain, self._scale.scaler, self._scale.downscaler, self._cleanup.deband)
        self._grain_stream_seed = _L.check_grain_stream_seed(grain_stream_seed)
        # the delivered frames rolled off to the sink's peak, one lib.ToneMapping or None: tone_mapping "spline"
        # (the reference's mpv setting; tone_param = its contrast, default 0.45), "bt.2390" or "clip" from source_peak (the model's
        # 1000 nits) to target_peak nits, behind scale, grain and deband.  None / "none", or a target_peak at or above source_peak:
        # nothing more is launched and the bytes are those of before.  With light_stats the record describes the tone-mapped codes.
        self._tone = _L.tone_mapping(tone_mapping, target_peak, source_peak, param=tone_param)
        # HDR10 content light level: every delivered frame carries its record (``.light``), measured on the
        # device from the codes the sink receives over ``light_rect = (x0, y0, rw, rh)`` in delivered-frame coordinates (None: the
        # whole frame), and ``content_light`` accumulates MaxCLL / MaxFALL in delivery order.  Off: nothing is launched or allocated.
        self._light = bool(light_stats)
        self._light_rect = None if light_rect is None else tuple(int(v) for v in light_rect)
        if self._light_rect is not None:
            x0, y0, rw, rh = self._light_rect
            if rw <= 0 or rh <= 0 or x0 < 0 or y0 < 0 or x0 + rw > self._out.w or y0 + rh > self._out.h:
                raise ValueError(f"light_rect {self._light_rect} is empty or leaves the {self._out.w}x{self._out.h} frame")
        self.content_light = ContentLightLevel() if self._light else None
        self._light_bufs = {}              # ring slot (or "fallback") -> (device u32 record, pinned host u32 record)
        self._processor = None
        self._precision_key = None
        self.status_messages = []
        self._status_cb = status_cb
        self._video_playback_buffer_frames = int(buffer_frames)
        self._pool, self._pool_key, self._pool_idx = None, None, 0
        self._timing_events = None
        self._hdr_queue = None
        self._hdr_thread = None
        self._hdr_stop = threading.Event()
        self._ring_shape = None
        self._hdr_sink = None              # remembered so that a hot-swap (_load_model) can restart the feeder
        self._hdr_error = None             # exception that ended the feeder thread, re-raised by _process_frame
        self._fallback = None              # (pinned host u16 tensor, device u16 tensor) of the ring-exhaustion fallback
        self.ring_fallbacks = 0
        self._input_format = input_format("i420")      # the lib.InputFormat of 2-D (Y'CbCr) frames: set_input_format
        self._letterbox10 = False          # set_input_format(letterbox=True): 10-bit frames of another size are letterboxed on the device

    def set_input_format(self, pix_fmt, yuv_matrix=709, yuv_full_range=False, *, letterbox=False):
        """How ``_process_frame`` reads a 2-D frame: u8 ``(H*3//2, W)`` with ``pix_fmt`` ``yuv420p`` or ``nv12``
        (``HDRTVNetMI355X.preprocess_yuv420``), or u16 with ``p010le`` / ``yuv420p10le`` / ``yuv422p10le`` (``preprocess_ycbcr10``),
        and its matrix and range.  A 10-bit frame is taken at the processing size only unless ``letterbox=True``: then a frame of
        another size is letterboxed to the processing size on the device, at ten bits (``preprocess_ycbcr10_letterboxed``; 8-bit
        frames are letterboxed whatever the flag says).  3-D frames are BGR whatever is set here."""
        self._letterbox10 = bool(letterbox)
        if pix_fmt not in ("yuv420p", "nv12") + tuple(YCBCR10_IN_FORMATS):
            raise ValueError(f"pix_fmt must be yuv420p, nv12 or one of {sorted(YCBCR10_IN_FORMATS)}")
        self._input_format = input_format(pix_fmt, yuv_matrix, yuv_full_range)

    @property
    def _yuv_format(self):
        """The input format as the keyword arguments of the processor's ``preprocess_yuv420`` / ``preprocess_ycbcr10`` methods."""
        return self._input_format.kwargs

    # ---------------------------------------------------------------- status
    def _emit(self, msg):
        self.status_messages.append(msg)
        if self._status_cb:
            self._status_cb(msg)

    # ---------------------------------------------------------------- model load / swap
    @staticmethod
    def _silent_warmup(processor, w, h):
        """model.py:39-70: prime the runtime once (no compiled graph exists here)."""
        if getattr(processor, "_compiled", False):
            processor.warmup_compile(w, h)
        else:
            processor.process(np.zeros((max(1, int(h)), max(1, int(w)), 3), dtype=np.uint8))
            torch.cuda.synchronize()

    def _load_model(self, key, announce_ready=True, *, compile_model=None, force_compile=False,
                    compile_mode=None, warmup=True):
        """model.py:72-257.  Returns True on success; on any backend failure emits
        ``ERROR: model backend failed - ...`` and returns False (model.py:229-235)."""
        cfg = PRECISIONS.get(key, {})
        if not cfg:
            self._emit(f"ERROR: precision preset is not defined - {key}")
            return False
        path = cfg["model"] if self._use_hg else cfg["model_nohg"]
        if not (isinstance(path, dict) or os.path.isabs(str(path))):
            path = os.path.join(self._weights_dir, path)
        if not isinstance(path, dict):
            if not os.path.isfile(path) and os.path.isfile(os.path.splitext(path)[0] + ".hdrw"):
                path = os.path.splitext(path)[0] + ".hdrw"
            if not os.path.isfile(path):
                self._emit(f"ERROR: weights not found - {path}")
                return False
        cw, ch = self._proc_w, self._proc_h
        if announce_ready:
            self._emit(f"Loading model: {key} ...")
        sink = self._hdr_sink                  # a running feeder is restarted on the new processor (hot-swap)
        if self._processor is not None:
            if not self._stop_hdr_feeder(keep_sink=True):
                self._emit("ERROR: HDR feeder did not stop; keeping the current model")
                return False
            self._processor.close()
            self._processor = None
            self._ring_shape = None            # the pinned ring lived in the closed context
            self._fallback = None
            self._light_bufs = {}
            torch.cuda.empty_cache()
        try:
            hg = self._hg_override
            if hg is None and self._use_hg:
                cand = os.path.join(self._weights_dir, cfg.get("hg_weights", ""))
                hg = cand if os.path.isfile(cand) else None        # missing -> no-HG, as model.py:208-209
            self._processor = HDRTVNetMI355X(
                path, device="auto", precision=cfg["precision"], compile_model=bool(compile_model),
                force_compile=bool(force_compile), compile_mode=compile_mode or "default",
                hg_weights=hg, use_hg=self._use_hg, warmup_passes=0)
        except Exception as exc:  # noqa: BLE001  (the reference catches everything here)
            self._processor = None
            self._emit(f"ERROR: model backend failed - {exc}")
            print(f"ERROR: model backend failed: {exc}", file=sys.stderr)
            torch.cuda.empty_cache()
            return False
        if announce_ready and warmup:
            self._emit(f"Priming model for {cw}x{ch} ({key}) ...")
        if warmup:
            self._silent_warmup(self._processor, cw, ch)
        self._precision_key = key
        if sink is not None:
            self._start_hdr_feeder(sink)
        if announce_ready:
            self._emit(f"Ready - {key} [MI355X]")
        return True

    # ---------------------------------------------------------------- per-frame
    def _prepare_hdr_output_tensor(self, raw_out, lower_res_processing=False):
        return raw_out[0] if isinstance(raw_out, (tuple, list)) else raw_out

    def _stage_hdr_display_tensor(self, prepared_out, use_cuda=True):
        """frame_processing.py:118-156: copy the backend-owned output into a rotating pool so the
        feeder never reads a tensor the next infer() overwrites."""
        pool_size = max(2, min(16, self._video_playback_buffer_frames + 2))
        key = (tuple(prepared_out.shape), str(prepared_out.device), str(prepared_out.dtype), pool_size)
        if self._pool_key != key or not self._pool:
            self._pool = [torch.empty_like(prepared_out) for _ in range(pool_size)]
            self._pool_key, self._pool_idx = key, 0
        staged = self._pool[self._pool_idx % len(self._pool)]
        self._pool_idx = (self._pool_idx + 1) % len(self._pool)
        staged.copy_(prepared_out, non_blocking=True)
        return staged

    def _cuda_timing_events(self):
        if self._timing_events is None:
            self._timing_events = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        return self._timing_events

    def _process_frame(self, *, frame, frame_idx, present_t=None, out_w=None, out_h=None, proc_w=None, proc_h=None,
                       lower_res_processing=False, mpv_w=True, use_cuda=True, need_compare_frame=False):
        """frame_processing.py:168-331 (SDR->HDR branch).  Returns the reference's 5-tuple
        ``(display_frame, output, prepared_out, need_hdr_cpu, model_latency_ms)``; with a sink
        attached (``mpv_w`` truthy and the HDR feeder running) the staged tensor and its ready
        event are queued as ``(present_t, tensor, event, out_hw)``.  ``out_w`` / ``out_h`` (default: the worker's own): the size
        the sink receives the frame at, each >= the processing size; the upscale is part of the RGB48 conversion
        (``hdrtv_post_rgb48_scaled``) whether or not ``lower_res_processing`` is set."""
        if self._processor is None:
            raise RuntimeError("no model loaded")
        if self._hdr_error is not None:        # the feeder thread died: surface it instead of silently dropping frames
            err, self._hdr_error = self._hdr_error, None
            raise RuntimeError(f"HDR feeder failed: {err!r}") from err
        start, end = self._cuda_timing_events()
        start.record(torch.cuda.current_stream())
        pw, ph = int(proc_w or self._proc_w), int(proc_h or self._proc_h)
        ow, oh = int(out_w or self._out_w or pw), int(out_h or self._out_h or ph)
        if self._downscaler is None and (ow < pw or oh < ph):
            raise ValueError(f"output size {ow}x{oh} is below the processing size {pw}x{ph} (enlarging only)")
        with torch.inference_mode():
            if frame.ndim == 2 and frame.dtype == np.uint16:
                # 10-bit Y'CbCr planes (set_input_format): converted inside the preprocess kernel; letterboxed there, at ten bits,
                # only where set_input_format(letterbox=True) asked for it
                if self._input_format.family != "ycbcr10":
                    raise ValueError("a uint16 frame needs set_input_format('p010le' | 'yuv420p10le' | 'yuv422p10le')")
                fh, fw = self._input_format.frame_hw(frame)
                if fw == pw and fh == ph:
                    tensor, cond = self._processor.preprocess_ycbcr10(frame, **self._yuv_format)
                elif self._letterbox10:
                    tensor, cond = self._processor.preprocess_ycbcr10_letterboxed(frame, pw, ph, **self._yuv_format)
                else:
                    raise ValueError(f"a {self._input_format.pix_fmt} source of {fw}x{fh} differs from the processing size {pw}x{ph}: "
                                     "the 10-bit letterbox is off, ask for it with set_input_format(..., letterbox=True) or feed the "
                                     "frame at the processing size")
            elif frame.ndim == 2:
                # 8-bit 4:2:0 planes: converted on the device (set_input_format), letterboxed there when the sizes differ
                fh = frame.shape[0] // 3 * 2
                if frame.shape[1] != pw or fh != ph:
                    tensor, cond = self._processor.preprocess_yuv420_letterboxed(frame, pw, ph, **self._yuv_format)
                else:
                    tensor, cond = self._processor.preprocess_yuv420(frame, **self._yuv_format)
            elif frame.shape[1] != pw or frame.shape[0] != ph:
                # the reference letterboxes on the host with cv2 before preprocess (gui_export.py:1080,
                # gui_scaling.py:228-244); here the resize runs on the device
                tensor, cond = self._processor.preprocess_letterboxed(frame, pw, ph)
            else:
                tensor, cond = self._processor.preprocess(frame)
            raw_out = self._processor.infer((tensor, cond))
        end.record(torch.cuda.current_stream())
        end.synchronize()
        model_latency_ms = max(0.0, float(start.elapsed_time(end)))
        prepared_out = self._prepare_hdr_output_tensor(raw_out, lower_res_processing)
        if mpv_w and self._hdr_queue is not None:
            staged = self._stage_hdr_display_tensor(prepared_out, use_cuda)
            ready = torch.cuda.Event(enable_timing=False)
            ready.record(torch.cuda.current_stream())
            self._queue_display_item(self._hdr_queue, (present_t, staged, ready, (oh, ow), int(frame_idx)))
        need_hdr_cpu = not mpv_w
        output = self._processor.postprocess(prepared_out) if need_hdr_cpu else frame
        return None, output, prepared_out, need_hdr_cpu, model_latency_ms

    @staticmethod
    def _queue_display_item(q, item):
        try:
            q.put(item, timeout=0.25)
        except _queue.Full:
            try:
                q.get_nowait()          # drop the oldest frame rather than stall inference
            except _queue.Empty:
                pass
            q.put_nowait(item)

    # ---------------------------------------------------------------- RGB48 ring + feeder
    def _tensor_to_rgb48_bytes(self, tensor, stream=None, out_hw=None, frame_idx=0):
        """feeders.py:193-249, GPU branch: quantise to RGB48 directly into a pinned ring slot and
        return a ``PinnedFrame`` guarded by the slot's ready event.  Ring exhaustion (no slot free
        within 250 ms, feeders.py:166-167) falls back to one blocking pinned buffer as the reference
        does (209-235): convert, copy, synchronise the stream, hand the finished frame over.  ``out_hw = (out_h, out_w)``: the
        ring, the fallback buffer and the frame are at that size and the conversion is the ``lib.ScalePlan`` of the worker's scaler
        options for the tensor's and the delivered size (``hdrtv_post_rgb48_scaled`` by default).  With a
        Y'CbCr ``out_pix_fmt`` the slot (an RGB48 slot holds any of the layouts) receives the planes, only the frame's bytes are
        committed (``hdrtv_ring_commit_bytes``) and the frame is a 1-D u16 view of them.  ``frame_idx``: the frame's index in the
        stream, which with ``film_grain`` on gives its grain seed (``lib.film_grain_seed``)."""
        p = self._processor
        t = tensor[0] if isinstance(tensor, (tuple, list)) else tensor
        th, tw = int(t.shape[-2]), int(t.shape[-1])
        h, w = (int(out_hw[0]), int(out_hw[1])) if out_hw is not None else (th, tw)
        if self._downscaler is None and (h < th or w < tw):
            raise ValueError(f"output size {w}x{h} is below the tensor's {tw}x{th} (enlarging only)")
        if self._ring_shape != (h, w):
            p._chk(p._lib.hdrtv_ring_create(p._ctx, _RING_FRAMES, h, w), "hdrtv_ring_create")
            self._ring_shape = (h, w)

        out = self._out.at(h, w)
        shape = out.shape
        # a hot-swap of the processing resolution may have moved the ratio past a scaler's limit: checked again here
        grain = self._film_grain
        seed = _L.film_grain_seed(self._grain_stream_seed, frame_idx) if grain else 0.0
        scale = self._scale.plan(tw, th, w, h, grain, seed) if (h, w) != (th, tw) else None

        def convert(dst, key):
            """The frame into ``dst`` and, when measured, its light level record into the pinned record kept per ``key``, all on
            ``st``: whatever is recorded on ``st`` afterwards (the slot's ready event) covers both.  Returns that record."""
            if not self._light:
                p._post_out(sp, t.contiguous().data_ptr(), _dtype_code(t), th, tw, dst, out, "worker", cleanup=self._cleanup, scale=scale,
                            film_grain=grain, grain_seed=seed, tone=self._tone)
                return None
            bufs = self._light_bufs.get(key)
            if bufs is None:
                bufs = self._light_bufs[key] = (torch.empty(_L.LIGHT_WORDS, dtype=torch.uint32, device=p.device),
                                                torch.empty(_L.LIGHT_WORDS, dtype=torch.uint32, pin_memory=True))
            p._post_out(sp, t.contiguous().data_ptr(), _dtype_code(t), th, tw, dst, out, "worker", bufs[0].data_ptr(), self._light_rect,
                        self._cleanup, scale, grain, seed, self._tone)
            with torch.cuda.stream(st):
                bufs[1].copy_(bufs[0], non_blocking=True)
            return bufs[1].numpy()
        host, dev = C.c_void_p(), C.c_void_p()
        st = stream or torch.cuda.current_stream(p.device)
        sp = C.c_void_p(st.cuda_stream)
        slot = p._lib.hdrtv_ring_acquire(p._ctx, 250, C.byref(host), C.byref(dev))
        if slot == _L.ESTATE:
            self.ring_fallbacks += 1
            if self._fallback is None or tuple(self._fallback[0].shape) != shape:
                self._fallback = (torch.empty(shape, dtype=torch.uint16, pin_memory=True),
                                  torch.empty(shape, dtype=torch.uint16, device=p.device))
            fb_host, fb_dev = self._fallback
            light = convert(fb_dev.data_ptr(), "fallback")
            with torch.cuda.stream(st):
                fb_host.copy_(fb_dev, non_blocking=True)
            st.synchronize()
            # the reference's host_np.tobytes(): a private copy
            return HostFrame(fb_host.numpy().copy(), None if light is None else light.copy())
        p._chk(slot, "hdrtv_ring_acquire")
        light = convert(dev.value, slot)
        p._chk(p._lib.hdrtv_ring_commit_bytes(p._ctx, slot, sp, out.nbytes), "hdrtv_ring_commit_bytes")
        return PinnedFrame(self, slot, host.value, shape, light)

    def _start_hdr_feeder(self, sink):
        """feeders.py:632-657 + 440-496: a thread that waits for each frame's ready event,
        converts on a side stream into the pinned ring and hands the frame to ``sink``."""
        self._stop_hdr_feeder()
        self._hdr_sink = sink
        self._hdr_error = None
        ring_hw = (self._out.h, self._out.w)                                         # the size frames are delivered at
        if self._processor is not None and self._ring_shape != ring_hw:
            # pin the ring now (3 x 50 MB at 4K takes tens of ms) rather than inside the first frame's deadline
            p = self._processor
            p._chk(p._lib.hdrtv_ring_create(p._ctx, _RING_FRAMES, ring_hw[0], ring_hw[1]), "hdrtv_ring_create")
            self._ring_shape = ring_hw
        # feeders.py:634-644: queue depth = buffer_frames (1..3).  With the staging pool of buffer_frames + 2
        # (_stage_hdr_display_tensor) that is exactly enough: queued + the one in the feeder's hands + the one
        # being staged; one more queued frame and the main stream overwrites a tensor the side stream still reads.
        self._hdr_queue = _queue.Queue(maxsize=min(3, max(1, self._video_playback_buffer_frames)))
        self._hdr_stop.clear()
        dev = self._processor.device

        hq = self._hdr_queue

        def run():
            try:
                side = torch.cuda.Stream(device=dev)
                while not self._hdr_stop.is_set():
                    try:
                        item = hq.get(timeout=0.05)
                    except _queue.Empty:
                        continue
                    if item is None:
                        break
                    present_t, tensor, ready, out_hw, frame_idx = item
                    ready.synchronize()                      # cross-thread device sync (feeders.py:469-473)
                    with torch.cuda.stream(side):
                        payload = self._tensor_to_rgb48_bytes(tensor, side, out_hw, frame_idx)
                    if present_t is not None:
                        delay = present_t - time.perf_counter()
                        if delay > 0:
                            time.sleep(delay)
                    if self.content_light is not None:
                        self.content_light.update(payload.light)
                    sink(payload)
            except BaseException as exc:  # noqa: BLE001  (a dead daemon thread must not be silent: _process_frame re-raises)
                self._hdr_error = exc

        self._hdr_thread = threading.Thread(target=run, name="hdr-feeder", daemon=True)
        self._hdr_thread.start()

    def _stop_hdr_feeder(self, keep_sink=False):
        """Stops the feeder thread.  Returns False (and leaves everything in place) if the thread is still running after
        10 s: the processor must not be closed under a thread that may be inside the C library."""
        if self._hdr_thread is not None:
            self._hdr_stop.set()
            try:
                self._hdr_queue.put_nowait(None)
            except Exception:  # noqa: BLE001
                pass
            self._hdr_thread.join(timeout=10.0)
            if self._hdr_thread.is_alive():
                # the stop flag and the sentinel are already set: the thread exits as soon as it unblocks and nothing will
                # drain the queue afterwards -- make the next _process_frame raise instead of queueing into the void
                self._hdr_error = RuntimeError("HDR feeder did not stop within 10 s; frames are no longer being delivered")
                return False
        self._hdr_thread, self._hdr_queue = None, None
        if not keep_sink:
            self._hdr_sink = None
        return True

    def close(self):
        if not self._stop_hdr_feeder():
            raise RuntimeError("HDR feeder thread did not stop; not destroying the processor under it")
        if self._processor is not None:
            self._processor.close()
            self._processor = None


def shard_frames(n_frames: int, rank: int, world_size: int):
    """Frame-parallel partition of BASELINE.json configs[3]: frame i -> GPU (rank) i mod N.
    No data-path collective; order is restored on the host by frame index."""
    return list(range(rank, n_frames, world_size))
