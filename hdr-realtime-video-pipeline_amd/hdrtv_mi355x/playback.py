"""Headless realtime playback around ``HeadlessPipelineWorker``.

  pacing loop, catch-up drop, fps limiter   src/gui_pipeline_worker.py:860-936, 1024-1029 (constants 38-40)
  hot-swap of precision / resolution        src/gui_pipeline_worker.py:737-759
  display prebuffer                         src/gui_pipeline_worker.py:516-530, 1082-1088
  live metrics dict                         src/gui_pipeline_worker_runtime_metrics.py:16-26, 120-199
  CSV schema, 1 % low fps                   src/cli_playback_benchmark.py:278-313, 1123-1129
  rawvideo rgb48le wire format              src/gui_mpv_widget.py:950-960, 998 ; src/gui_export.py:940-1015

No PyQt / cv2 / mpv: Qt signals become plain callbacks, the frame source is any object with
``read() -> (ok, frame_bgr_u8)`` and ``fps``, the HDR sink any callable taking a ``PinnedFrame``.
The clock and sleep functions are injectable so the scheduling logic is testable without a GPU.
"""
from __future__ import annotations

import csv
import os
import queue
import threading
import time

import numpy as np

from . import lib as _lib
from .weights import synthetic_frame

# gui_pipeline_worker.py:38-40
_REALTIME_CATCHUP_ENABLED = True
_REALTIME_SKIP_LAG_FRAMES = 1.1
_REALTIME_MAX_CATCHUP_SKIP = 6

# cli_playback_benchmark.py:278-313
CSV_FIELDS = [
    "elapsed_s", "logged_at_local", "fps", "latency_ms", "model_latency_ms", "live_video_latency_ms", "frame",
    "cpu_mb", "gpu_mb", "model_mb", "model_size_label", "precision", "proc_res", "psnr_db", "sssim", "delta_e_itp",
    "hdr_vdp3", "objective_enabled", "objective_note", "hdr_vdp3_note", "is_live_capture", "decode_ms", "resize_ms",
    "infer_ms", "pre_ms", "run_ms", "post_ms", "render_ms", "fps_1p_low", "dropped_frames", "catchup_dropped_frames",
    "fps_limiter_dropped_frames", "source_loops", "playback_mode",
]


# ------------------------------------------------------------------------------- sources
class SyntheticSource:
    """Seeded u8 BGR frames (a small pool cycled, so decode cost stays out of the loop)."""

    def __init__(self, width, height, fps=60.0, n_frames=120, seed=1234, pool=4, kind="gradient"):
        self.width, self.height, self.fps, self.frame_count = int(width), int(height), float(fps), int(n_frames)
        self._pool = [synthetic_frame(self.height, self.width, seed + i, kind) for i in range(max(1, pool))]
        self._i = 0

    def read(self):
        if self._i >= self.frame_count:
            return False, None
        f = self._pool[self._i % len(self._pool)]
        self._i += 1
        return True, f

    def release(self):
        pass


class PinnedFrame(np.ndarray):
    """A u8 BGR (or 4:2:0, ``(H*3//2, W)``) frame that lives in page-locked memory; ``pinned_tensor`` is the torch tensor sharing it
    (HDRTVNetMI355X.preprocess uploads such a frame without the host-side copy into its own pinned slot).  When the
    prefetcher has already uploaded it, ``device_tensor`` is the device copy and ``ready_event`` the event recorded
    behind that upload on the prefetcher's stream."""
    pinned_tensor = None
    device_tensor = None
    ready_event = None


class PinnedPrefetch:
    """Source wrapper: a reader thread pulls frames from ``source`` and copies them into a small pool of page-locked
    buffers while the previous frame is on the GPU, so the 25 MB host copy of a 4K frame (2-3 ms) leaves the
    per-frame critical path.  The reference copies into its pinned slot inside preprocess, on the caller's thread
    (hdrtvnet_torch.py:2262-2266); here the HIP path hands the buffer over by hipMemcpyAsync + the stream order.
    At most one frame is queued and one is being filled, so a pool of three is never overwritten while in use
    (``_process_frame`` returns only after the frame's work has completed)."""

    def __init__(self, source, pool=3, upload=True):
        self._src = source
        self._upload = bool(upload)       # also hipMemcpyAsync the frame to the device on a side stream (+ hipEvent)
        self._dev = {}
        self._stream = None
        self._error = None
        self.width, self.height, self.fps = source.width, source.height, source.fps
        self.frame_count = getattr(source, "frame_count", 0)
        self.pix_fmt = getattr(source, "pix_fmt", "bgr24")
        self.yuv_matrix, self.yuv_full_range = getattr(source, "yuv_matrix", 709), getattr(source, "yuv_full_range", False)
        self._pool_n = max(3, int(pool))
        self._bufs = {}
        self._q = queue.Queue(maxsize=1)
        self._stop = threading.Event()
        self._t = threading.Thread(target=self._run, name="hdrtv-pinned-prefetch", daemon=True)
        self._t.start()

    def _stage(self, frame, i):
        import ctypes
        import torch
        key = frame.shape
        pool = self._bufs.get(key)
        if pool is None:
            try:
                pool = [torch.empty(key, dtype=torch.uint8, pin_memory=True) for _ in range(self._pool_n)]
            except RuntimeError:          # no HIP runtime in this process (CPU-only host): frames pass through unstaged
                pool = []
            self._bufs[key] = pool
        if not pool:
            return frame
        t = pool[i % self._pool_n]
        src = np.ascontiguousarray(frame)
        ctypes.memmove(t.data_ptr(), src.ctypes.data, src.nbytes)      # plain memcpy, GIL released
        out = t.numpy().view(PinnedFrame)
        out.pinned_tensor = t
        if self._upload and torch.cuda.is_available():
            dpool = self._dev.get(key)
            if dpool is None:
                dpool = self._dev[key] = [torch.empty(key, dtype=torch.uint8, device="cuda") for _ in range(self._pool_n)]
                self._stream = self._stream or torch.cuda.Stream()
            d = dpool[i % self._pool_n]
            with torch.cuda.stream(self._stream):
                d.copy_(t, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self._stream)
            out.device_tensor, out.ready_event = d, ev
        return out

    def _run(self):
        try:
            self._loop()
        except BaseException as exc:  # noqa: BLE001  (handed to the consumer: read() re-raises it)
            self._error = exc

    def _loop(self):
        i = 0
        while not self._stop.is_set():
            ret, frame = self._src.read()
            item = (False, None)
            if ret and frame is not None and frame.dtype == np.uint8 and frame.ndim in (2, 3):      # BGR or 4:2:0 planes
                item = (True, self._stage(frame, i))
                i += 1
            elif ret:
                item = (ret, frame)
            while not self._stop.is_set():
                try:
                    self._q.put(item, timeout=0.1)
                    break
                except queue.Full:
                    continue
            if not item[0]:
                return

    def read(self):
        while True:
            try:
                return self._q.get(timeout=0.05 if not self._t.is_alive() else 0.5)
            except queue.Empty:
                if not self._t.is_alive() and self._q.empty():
                    if self._error is not None:
                        err, self._error = self._error, None
                        raise RuntimeError("frame source failed in the prefetch thread") from err
                    return False, None

    def release(self):
        self._stop.set()
        self._t.join(timeout=2.0)
        self._src.release()


class RawVideoSource:
    """Headerless rawvideo file (what ``ffmpeg -f rawvideo -pix_fmt <pix_fmt>`` writes), memory-mapped.  ``pix_fmt``:
    ``bgr24`` frames are u8 ``(H, W, 3)``; ``yuv420p`` (I420) and ``nv12`` frames are u8 ``(H*3//2, W)``, the planes back to back
    (``HDRTVNetMI355X.preprocess_yuv420``), even sizes only; ``p010le`` / ``yuv420p10le`` / ``yuv422p10le`` frames are little-endian
    u16 ``(H*3//2, W)``, or ``(2*H, W)`` for 4:2:2 (``HDRTVNetMI355X.preprocess_ycbcr10``; a size other than the processing size needs
    the worker's 10-bit letterbox, ``RealtimePlayback(letterbox=True)``).  ``yuv_matrix`` (601 / 709 / 2020) and ``yuv_full_range`` say how
    the 4:2:0 frames convert to RGB (the stream's ``color_space`` / ``color_range``)."""

    PIX_FMTS = ("bgr24", "yuv420p", "nv12") + tuple(_lib.YCBCR10_IN_FORMATS)

    def __init__(self, path, width, height, fps, pix_fmt="bgr24", yuv_matrix=709, yuv_full_range=False):
        self.width, self.height, self.fps = int(width), int(height), float(fps)
        if pix_fmt not in self.PIX_FMTS:
            raise ValueError(f"pix_fmt must be one of {self.PIX_FMTS}")
        fmt = _lib.input_format(pix_fmt, yuv_matrix, yuv_full_range)
        self.pix_fmt, self.yuv_matrix, self.yuv_full_range = fmt
        shape, dtype = fmt.frame_shape(self.height, self.width), np.dtype(fmt.dtype).newbyteorder("<")
        fb = int(np.prod(shape)) * np.dtype(dtype).itemsize
        size = os.path.getsize(path)
        if size < fb or size % fb:
            raise ValueError(f"{path}: size {size} is not a whole number of {self.width}x{self.height} {pix_fmt} frames")
        self.frame_count = size // fb
        self._mm = np.memmap(path, dtype=dtype, mode="r", shape=(self.frame_count,) + shape)
        self._i = 0

    def read(self):
        if self._i >= self.frame_count:
            return False, None
        f = np.ascontiguousarray(self._mm[self._i])
        self._i += 1
        return True, f

    def release(self):
        self._mm = None


# ------------------------------------------------------------------------------- rgb48le sink
class Rgb48leSink:
    """Writes each RGB48 frame as headerless little-endian ``rgb48le`` rawvideo -- the byte stream the
    reference pipes into mpv (gui_mpv_widget.py:950-960) and into ffmpeg on export (gui_export.py:957-975)
    -- to a file object / path / pipe, then releases the frame's ring slot (gui_mpv_widget.py:663-668)."""

    def __init__(self, target, width, height, fps):
        self.width, self.height, self.fps = int(width), int(height), float(fps)
        self._own = isinstance(target, (str, os.PathLike))
        self._f = open(target, "wb") if self._own else target
        self.frames = 0
        self.bytes = 0

    def __call__(self, payload):
        try:
            view = payload.buffer_view()
            if len(view) != self.width * self.height * 6:
                raise ValueError(f"frame of {len(view)} bytes does not match {self.width}x{self.height} rgb48le")
            self._f.write(view)
            self.frames += 1
            self.bytes += len(view)
        finally:
            payload.release()

    def close(self):
        if self._f is not None:
            self._f.flush()
            if self._own:
                self._f.close()
            self._f = None

    def mpv_args(self):
        """Command-line form of the demuxer options of gui_mpv_widget.py:955-960 and the HDR tag of 998."""
        return ["--demuxer=rawvideo", f"--demuxer-rawvideo-w={self.width}", f"--demuxer-rawvideo-h={self.height}",
                "--demuxer-rawvideo-mp-format=rgb48le", f"--demuxer-rawvideo-fps={self.fps:g}",
                "--vf=format=colorlevels=full:primaries=bt.2020:gamma=pq"]

    def ffmpeg_input_args(self):
        """Input half of the export command (gui_export.py:957-977): full-range BT.2020 / PQ rgb48le on stdin."""
        return ["-f", "rawvideo", "-pix_fmt", "rgb48le", "-s:v", f"{self.width}x{self.height}", "-r", f"{self.fps:.6f}",
                "-color_range", "pc", "-colorspace", "bt2020nc", "-color_trc", "smpte2084", "-color_primaries", "bt2020",
                "-i", "-"]


class RawVideoSink(Rgb48leSink):
    """``Rgb48leSink`` for any output pixel format of the worker: ``rgb48le``, or the 10-bit limited-range BT.2020nc Y'CbCr
    layouts ``p010le`` / ``yuv420p10le`` / ``yuv422p10le`` an encoder takes, written as headerless rawvideo
    with the planes back to back.  ``siting``: where the 4:2:0 chroma samples sit (``left``, ffmpeg's default, or ``topleft``)."""

    def __init__(self, target, width, height, fps, pix_fmt="rgb48le", siting="left"):
        super().__init__(target, width, height, fps)
        self.format = _lib.output_format(pix_fmt, siting, self.height, self.width)
        self.pix_fmt, self.siting = self.format.pix_fmt, self.format.siting

    def __call__(self, payload):
        try:
            view = payload.buffer_view()
            if len(view) != self.format.nbytes:
                raise ValueError(f"frame of {len(view)} bytes does not match {self.width}x{self.height} {self.pix_fmt}")
            self._f.write(view)
            self.frames += 1
            self.bytes += len(view)
        finally:
            payload.release()

    @staticmethod
    def x265_params(cll):
        """``max-cll=<MaxCLL>,<MaxFALL>`` for the encode command's ``-x265-params`` from the worker's ``content_light``
        (``lightlevel.ContentLightLevel``) at the end of the stream."""
        return cll.x265_params()

    def mpv_args(self):
        if self.pix_fmt == "rgb48le":
            return super().mpv_args()
        return ["--demuxer=rawvideo", f"--demuxer-rawvideo-w={self.width}", f"--demuxer-rawvideo-h={self.height}",
                f"--demuxer-rawvideo-mp-format={self.pix_fmt[:-2]}", f"--demuxer-rawvideo-fps={self.fps:g}",
                "--vf=format=colorlevels=limited:colormatrix=bt.2020-ncl:primaries=bt.2020:gamma=pq"]

    def ffmpeg_input_args(self):
        """Input half of an encode command: limited-range BT.2020nc / PQ 10-bit Y'CbCr on stdin.  ``-chroma_sample_location`` is
        given only where ffmpeg needs it: ``left`` is what it assumes for 4:2:0 when nothing is said, and 4:2:2 has no choice."""
        if self.pix_fmt == "rgb48le":
            return super().ffmpeg_input_args()
        args = ["-f", "rawvideo", "-pix_fmt", self.pix_fmt, "-s:v", f"{self.width}x{self.height}", "-r", f"{self.fps:.6f}",
                "-color_range", "tv", "-colorspace", "bt2020nc", "-color_trc", "smpte2084", "-color_primaries", "bt2020"]
        if self.siting == "topleft":
            args += ["-chroma_sample_location", "topleft"]
        return args + ["-i", "-"]


# ------------------------------------------------------------------------------- metrics
def trimmed_latency_average(values) -> float:
    """runtime_metrics.py:16-26."""
    vals = [float(v) for v in values if float(v) > 0.0]
    if not vals:
        return 0.0
    if len(vals) < 8:
        return sum(vals) / len(vals)
    vals.sort()
    trim = max(1, len(vals) // 10)
    kept = vals[trim:-trim] if len(vals) > (trim * 2) else vals
    return sum(kept) / len(kept)


def one_percent_low(fps_samples, avg_fps):
    """cli_playback_benchmark.py:1123-1129."""
    s = sorted(fps_samples)
    if not s:
        return avg_fps
    k = max(1, int(len(s) * 0.01))
    return sum(s[:k]) / k


class CsvLogger:
    def __init__(self, path):
        self._f = open(path, "w", newline="")
        self._w = csv.DictWriter(self._f, fieldnames=CSV_FIELDS, extrasaction="ignore")
        self._w.writeheader()
        self._t0 = time.perf_counter()

    def log(self, metrics):
        row = {k: metrics.get(k, "") for k in CSV_FIELDS}
        row["elapsed_s"] = f"{time.perf_counter() - self._t0:.3f}"
        row["logged_at_local"] = time.strftime("%Y-%m-%d %H:%M:%S")
        self._w.writerow(row)

    def close(self):
        self._f.close()


# ------------------------------------------------------------------------------- the loop
OBJECTIVE_MODES = ("tensor", "reference")


class Rgb48leSource:
    """Ground-truth frames for ``RealtimePlayback(objective_mode="reference")``: a headerless little-endian ``rgb48le`` rawvideo file
    at the delivered size, memory-mapped; ``read()`` yields u16 ``(H, W, 3)`` frames."""

    def __init__(self, path, width, height):
        self.width, self.height = int(width), int(height)
        fb = self.width * self.height * 6
        size = os.path.getsize(path)
        if fb <= 0 or size < fb or size % fb:
            raise ValueError(f"{path}: size {size} is not a whole number of {self.width}x{self.height} rgb48le frames")
        self.frame_count = size // fb
        self._mm = np.memmap(path, dtype=np.dtype("<u2"), mode="r", shape=(self.frame_count, self.height, self.width, 3))
        self._i = 0

    def read(self):
        if self._i >= self.frame_count:
            return False, None
        f = np.ascontiguousarray(self._mm[self._i]).astype(np.uint16, copy=False)
        self._i += 1
        return True, f


class RealtimePlayback:
    """The worker's ``run()`` loop for a file-like source (not live capture), headless.

    ``worker`` needs ``_process_frame(frame=, frame_idx=, present_t=, proc_w=, proc_h=, mpv_w=)`` returning the
    reference's 5-tuple, ``_load_model(key)``, ``_silent_warmup(processor, w, h)``, ``_processor``, ``_precision_key``,
    ``_proc_w/_proc_h`` -- i.e. a ``HeadlessPipelineWorker`` (or a stand-in in tests)."""

    def __init__(self, worker, source, *, sink=True, frame_stride=1, realtime=True, metrics_cb=None, csv_path=None,
                 metrics_interval_s=0.20, metrics_window=120, clock=time.perf_counter, sleep=None, status_cb=None,
                 gt_source=None, objective_every=10, letterbox=False, objective_mode="tensor"):
        self.w, self.source = worker, source
        self.sink = sink
        self.frame_stride = max(1, int(frame_stride))
        self.realtime = bool(realtime)
        self.metrics_cb, self.status_cb = metrics_cb, status_cb
        self._csv = CsvLogger(csv_path) if csv_path else None
        self._metrics_interval_s = max(0.05, float(metrics_interval_s))
        self._window = int(metrics_window)
        self._clock = clock
        self._sleep = sleep or self._sleep_until_default
        # optional ground-truth HDR frames ([3,H,W] or [1,3,H,W] unit-range tensors from ``gt_source.read()``): every
        # ``objective_every``-th processed frame is scored on the device (gui_pipeline_worker_objective.py role)
        self.gt_source, self.objective_every = gt_source, max(1, int(objective_every))
        # ``objective_mode``: "tensor" scores the model's float tensor at the processing size (``objective_metrics``); "reference"
        # scores what the reference's live path scores (gui_pipeline_worker_objective.py:60-73): the delivered RGB48 codes against
        # u16 ``(H, W, 3)`` ground-truth frames at the delivered size, both area-reduced to 512 on the longer side
        # (``full_reference_metrics(crop=False, normalized=False)``)
        if objective_mode not in OBJECTIVE_MODES:
            raise ValueError(f"objective_mode must be one of {list(OBJECTIVE_MODES)} (got {objective_mode!r})")
        self.objective_mode = objective_mode
        # a 4:2:0 source (RawVideoSource pix_fmt yuv420p / nv12): the worker converts its 2-D frames on the device.  ``letterbox``: a
        # 10-bit source of another size than the processing size is letterboxed there too (the worker's opt-in; bgr24, yuv420p and
        # nv12 frames are letterboxed without it)
        if getattr(source, "pix_fmt", "bgr24") != "bgr24" and hasattr(worker, "set_input_format"):
            fmt = (source.pix_fmt, getattr(source, "yuv_matrix", 709), getattr(source, "yuv_full_range", False))
            if letterbox and source.pix_fmt in _lib.YCBCR10_IN_FORMATS:
                worker.set_input_format(*fmt, letterbox=True)
            else:
                worker.set_input_format(*fmt)
        self._objective = {"psnr_db": None, "sssim": None, "delta_e_itp": None}
        self._pending_precision = None
        self._pending_resolution = None
        self._display_prebuffer_target = 0
        self._display_prebuffer_count = 0
        self.prebuffer_ready = None          # callback(frame_idx, buffered)
        self._stop = False
        # counters (CSV columns)
        self.realtime_drop_frames = 0
        self.fps_limiter_dropped_frames = 0
        self.frames_processed = 0
        self.last_metrics = None

    # -- control surface (gui_pipeline_worker.py:516-530 and the pending_* slots)
    def request_precision(self, key):
        self._pending_precision = key

    def request_resolution(self, w, h):
        self._pending_resolution = (int(w), int(h))

    def request_display_prebuffer(self, frames):
        self._display_prebuffer_target = max(0, int(frames))
        self._display_prebuffer_count = 0

    def cancel_display_prebuffer(self):
        self._display_prebuffer_target = 0
        self._display_prebuffer_count = 0

    def stop(self):
        self._stop = True

    def _sleep_until_default(self, t):
        while True:
            d = t - self._clock()
            if d <= 0:
                return
            time.sleep(min(d, 0.002) if d < 0.004 else d - 0.002)

    def _status(self, msg):
        if self.status_cb:
            self.status_cb(msg)

    # -- the loop
    def run(self, max_frames=None):
        w = self.w
        frame_interval_s = 1.0 / max(1e-6, float(self.source.fps))
        proc_w, proc_h = int(w._proc_w), int(w._proc_h)
        frame_idx = 0
        frame_times, model_times, presented_times, fps_samples = [], [], [], []
        next_frame_t = self._clock()
        t_start = next_frame_t
        last_emit_t = 0.0
        while not self._stop:
            # hot-swap precision / processing resolution between frames (737-759)
            pending = self._pending_precision
            if pending and pending != w._precision_key:
                self._pending_precision = None
                if not w._load_model(pending):
                    continue
            elif pending:
                self._pending_precision = None
            if self._pending_resolution is not None:
                new_pw, new_ph = self._pending_resolution
                self._pending_resolution = None
                if (new_pw, new_ph) != (proc_w, proc_h):
                    self._status(f"Switching to {new_pw}x{new_ph} ...")
                    w._proc_w, w._proc_h = new_pw, new_ph
                    proc_w, proc_h = new_pw, new_ph
                    w._silent_warmup(w._processor, proc_w, proc_h)
                    self._status(f"Ready - {w._precision_key} @ {proc_w}x{proc_h}")

            now = self._clock()
            lag_s = 0.0
            if self.realtime:
                if now < next_frame_t:
                    self._sleep(next_frame_t)
                    now = self._clock()
                else:
                    lag_s = now - next_frame_t

            ret, frame = self.source.read()
            if not ret:
                break
            frame_idx += 1

            # real-time catch-up: behind the wall clock -> drop decoded frames, process the newest (899-936)
            if self.realtime and _REALTIME_CATCHUP_ENABLED and lag_s > frame_interval_s * _REALTIME_SKIP_LAG_FRAMES:
                skip_n = min(_REALTIME_MAX_CATCHUP_SKIP, max(0, int(lag_s / frame_interval_s)))
                while skip_n > 0:
                    ret_skip, frame_skip = self.source.read()
                    if not ret_skip:
                        ret = False
                        break
                    frame = frame_skip
                    frame_idx += 1
                    self.realtime_drop_frames += 1
                    next_frame_t += frame_interval_s
                    skip_n -= 1
                if not ret:
                    break

            # fps limiter via frame skipping (keeps wall-clock speed)
            if self.frame_stride > 1 and (frame_idx % self.frame_stride) != 0:
                next_frame_t += frame_interval_s
                self.fps_limiter_dropped_frames += 1
                continue

            present_t = max(next_frame_t, self._clock()) if self.realtime else None
            t0 = self._clock()
            _, _, prepared, _, model_latency_ms = w._process_frame(frame=frame, frame_idx=frame_idx, present_t=present_t,
                                                                    proc_w=proc_w, proc_h=proc_h, mpv_w=self.sink)
            if self.gt_source is not None:
                ok_gt, gt = self.gt_source.read()
                if ok_gt and prepared is not None and (self.frames_processed % self.objective_every) == 0:
                    if self.objective_mode == "reference":
                        self._objective = w._processor.full_reference_metrics(self._delivered_rgb48(prepared), gt, crop=False,
                                                                              normalized=False)
                    else:
                        self._objective = w._processor.objective_metrics(prepared, gt)
            t1 = self._clock()
            next_frame_t += frame_interval_s
            frame_ms = (t1 - t0) * 1000.0
            frame_times.append(frame_ms)
            if frame_ms > 0:
                fps_samples.append(1000.0 / frame_ms)
            if model_latency_ms > 0.0:
                model_times.append(float(model_latency_ms))
            presented_times.append(max(t1, present_t) if present_t is not None else t1)
            for lst in (frame_times, model_times, presented_times):
                if len(lst) > self._window:
                    del lst[: len(lst) - self._window]
            self.frames_processed += 1

            if self._display_prebuffer_target > 0:
                self._display_prebuffer_count += 1
                if self._display_prebuffer_count >= self._display_prebuffer_target:
                    buffered = int(self._display_prebuffer_count)
                    self._display_prebuffer_target = 0
                    self._display_prebuffer_count = 0
                    if self.prebuffer_ready:
                        self.prebuffer_ready(frame_idx, buffered)

            now_t = self._clock()
            if last_emit_t <= 0.0 or (now_t - last_emit_t) >= self._metrics_interval_s:
                last_emit_t = now_t
                self._emit_metrics(frame_idx, frame_times, model_times, presented_times, fps_samples, proc_w, proc_h)
            if max_frames is not None and self.frames_processed >= max_frames:
                break
        if frame_times:
            self._emit_metrics(frame_idx, frame_times, model_times, presented_times, fps_samples, proc_w, proc_h)
        if self._csv:
            self._csv.close()
            self._csv = None
        elapsed = self._clock() - t_start
        return {"frames_processed": self.frames_processed, "frames_read": frame_idx, "elapsed_s": elapsed,
                "catchup_dropped_frames": self.realtime_drop_frames,
                "fps_limiter_dropped_frames": self.fps_limiter_dropped_frames,
                "fps": (self.frames_processed / elapsed) if elapsed > 0 else 0.0, "last_metrics": self.last_metrics}

    def _delivered_rgb48(self, prepared):
        """The RGB48 codes the sink receives for ``prepared``, as a device tensor: the worker's delivered size and scaler options
        through the processor's own conversion (the bytes the feeder's ring slot gets, before any deband).  A worker delivering
        10-bit Y'CbCr has no RGB48 frame to score."""
        t = prepared[0] if isinstance(prepared, (tuple, list)) else prepared
        out = getattr(self.w, "_out", None)
        if out is not None and not out.is_rgb48:
            raise ValueError(f"objective_mode='reference' scores RGB48 codes: the worker delivers {out.pix_fmt}")
        oh, ow = (out.h, out.w) if out is not None else (int(t.shape[-2]), int(t.shape[-1]))
        opts = getattr(self.w, "_scale", _lib.SCALE_OFF)
        return self.w._processor.postprocess_rgb48_scaled(t, ow, oh, **opts._asdict())

    def _emit_metrics(self, frame_idx, frame_times, model_times, presented_times, fps_samples, proc_w, proc_h):
        avg = sum(frame_times) / len(frame_times)
        model_avg = (sum(model_times) / len(model_times)) if model_times else 0.0
        if len(presented_times) >= 2:
            dt = presented_times[-1] - presented_times[0]
            fps = ((len(presented_times) - 1) / dt) if dt > 0 else 0.0
        else:
            fps = 1000.0 / avg if avg > 0 else 0.0
        cpu_mb = gpu_mb = 0.0
        try:
            import psutil
            cpu_mb = psutil.Process().memory_info().rss / (1024 * 1024)
        except Exception:  # noqa: BLE001
            pass
        try:
            import torch
            if torch.cuda.is_available():
                gpu_mb = float(torch.cuda.memory_reserved() / (1024 * 1024)) or float(torch.cuda.memory_allocated() / (1024 * 1024))
        except Exception:  # noqa: BLE001
            pass
        m = {
            "fps": fps, "latency_ms": avg, "model_latency_ms": float(model_avg),
            "model_latency_display_ms": float(trimmed_latency_average(model_times)), "live_video_latency_ms": 0.0,
            "is_live_capture": False, "frame": frame_idx, "cpu_mb": cpu_mb, "gpu_mb": gpu_mb,
            "model_mb": float(getattr(self.w, "_model_mb", 0.0) or 0.0), "model_size_label": "Checkpoint",
            "precision": self.w._precision_key, "proc_res": f"{proc_w}x{proc_h}",
            "psnr_db": self._objective["psnr_db"], "sssim": self._objective["sssim"],
            "delta_e_itp": self._objective["delta_e_itp"], "hdr_vdp3": None, "objective_enabled": self.gt_source is not None,
            "objective_note": "", "hdr_vdp3_note": "",
            # CSV-only columns (cli_playback_benchmark.py)
            "infer_ms": float(model_avg), "fps_1p_low": one_percent_low(fps_samples, fps),
            "dropped_frames": self.realtime_drop_frames + self.fps_limiter_dropped_frames,
            "catchup_dropped_frames": self.realtime_drop_frames,
            "fps_limiter_dropped_frames": self.fps_limiter_dropped_frames, "source_loops": 0,
            "playback_mode": "realtime" if self.realtime else "max-throughput",
        }
        self.last_metrics = m
        if self.metrics_cb:
            self.metrics_cb(m)
        if self._csv:
            self._csv.log(m)


def parse_args(argv=None):
    """The command line of ``main`` -> the argparse namespace, checked (a bad value ends in ``ap.error``): ``.proc_wh``, ``.out_wh`` and
    ``.src_wh`` hold the three sizes as ``(w, h)``, ``.cleanup`` the ``lib.OutputCleanup`` of --deband / --dither, ``.antiring`` and ``.cas`` ``"auto"`` or the
    strength as a float (0.0: off; both 0.0 under any ``--scaler`` but lanczos), ``.scaler`` one of ``lib.UPSCALERS``, ``.fsr_sharpness`` the RCAS
    sharpness as a float or None (EASU alone), ``.downscaler`` None, ``"mitchell"`` or ``"ssim"``, ``.down_antiring`` its anti-ringing
    strength as a float (``auto`` resolved to the reference's 0.20), ``.film_grain`` the film grain's intensity as a float (0.0: off)
    and ``.film_grain_seed`` the stream's seed, ``.tone`` the ``lib.ToneMapping`` of --tone-mapping / --target-peak / --source-peak /
    --tone-mapping-param, or None when off."""
    import argparse

    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--weights-dir", required=True, help="directory holding original/HR.pt (or .hdrw) [and original/HG.pt]")
    ap.add_argument("--precision", default="FP16")
    ap.add_argument("--size", default="3840x2160", help="processing size WxH: the size the network runs at")
    ap.add_argument("--out-size", default=None, help="size WxH the sink receives frames at (default: --size; not below it on either "
                    "axis unless --downscaler is given): the RGB48 conversion upscales on the device (hdrtv_post_rgb48_scaled)")
    ap.add_argument("--src-size", default=None, help="size WxH of the source frames (default: --size): a source of another size is "
                    "letterboxed to --size on the device, 10-bit formats at ten bits (hdrtv_preprocess_ycbcr10_letterboxed: a shrink "
                    "of at most 4x per axis)")
    ap.add_argument("--fps", type=float, default=60.0)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--input", help="rawvideo file at --src-size in --pix-fmt (default: synthetic frames)")
    ap.add_argument("--pix-fmt", choices=RawVideoSource.PIX_FMTS, default="bgr24", help="pixel format of --input")
    ap.add_argument("--yuv-matrix", type=int, choices=(601, 709, 2020), default=709, help="Y'CbCr matrix of a yuv420p / nv12 / 10-bit input")
    ap.add_argument("--yuv-range", choices=("limited", "full"), default="limited", help="Y'CbCr range of a yuv420p / nv12 / 10-bit input")
    ap.add_argument("--out", help="rawvideo output in --out-pix-fmt (file or fifo); omit to run without a display sink")
    ap.add_argument("--out-pix-fmt", choices=_lib.OUT_PIX_FMTS, default="rgb48le", help="what the sink receives: full-range RGB48, or "
                    "10-bit limited-range BT.2020nc Y'CbCr for an encoder, converted on the device (hdrtv_post_ycbcr10)")
    ap.add_argument("--out-siting", choices=sorted(_lib.YCC_SITINGS), default="left", help="chroma siting of a 4:2:0 --out-pix-fmt: left "
                    "(MPEG-2 / H.264, ffmpeg's default) or topleft (BT.2100 / HDR10)")
    ap.add_argument("--light-level", action="store_true", help="measure the HDR10 content light level of the delivered frames on the "
                    "device (hdrtv_light_stats): the result line gains max_cll / max_fall / light_frames")
    ap.add_argument("--light-level-json", metavar="PATH", help="also write MaxCLL / MaxFALL and the max-cll= string for the encoder "
                    "to PATH (implies --light-level)")
    ap.add_argument("--deband", action="store_true", help="deband the RGB48 codes of the delivered frames on the device "
                    "(hdrtv_rgb48_deband; INTEGRATION.md 5f)")
    ap.add_argument("--deband-range", type=int, default=_lib.DEBAND_RANGE, help="reach of the deband references in pixels, 1 .. 16")
    ap.add_argument("--deband-threshold", type=int, default=_lib.DEBAND_THRESHOLD, help="largest difference a deband reference may "
                    "have, in u16 code units, 1 .. 65535 (1311 = 2 %% of the range)")
    ap.add_argument("--dither", choices=sorted(_lib.DITHERS), default="none", help="dither of the 16 -> 10 bit rounding of a Y'CbCr "
                    "--out-pix-fmt: ordered = a 16x16 Bayer threshold (hdrtv_post_ycbcr10_ex), floyd_steinberg = error diffusion "
                    "(hdrtv_post_ycbcr10_fs; INTEGRATION.md 5f); not for rgb48le")
    ap.add_argument("--antiring", default=None, metavar="{auto|0..1}", help="anti-ringing of the --out-size upscale "
                    "(hdrtv_post_rgb48_scaled_ex; INTEGRATION.md 5c): a strength in 0 .. 1, or auto = the reference's schedule by "
                    "processing size (0.30 up to 960x540, 0.22 up to 1280x720, 0.10 above); default: off")
    ap.add_argument("--cas", default=None, metavar="{auto|0..1}", help="contrast-adaptive sharpening in front of the --out-size "
                    "upscale (hdrtv_post_rgb48_scaled_cas; INTEGRATION.md 5c): a strength in 0 .. 1 as ffmpeg's cas filter takes it, "
                    "or auto = the reference's schedule by processing size (0.22 up to 960x540, 0.20 up to 1280x720, 0.16 above); "
                    "default: off")
    ap.add_argument("--scaler", choices=_lib.UPSCALERS, default="lanczos", help="what enlarges to --out-size: lanczos (the fused Lanczos "
                    "upscale with --antiring / --cas), fsr (hdrtv_post_rgb48_fsr, the reference's default upscaler: EASU + RCAS; at "
                    "most 2x per axis), spline36 or ssim_superres (hdrtv_post_rgb48_ssimsr without / with the reference's SSimSuperRes "
                    "shader stage; both axes enlarged, at most 2x); --antiring and --cas are 0 under all but lanczos; INTEGRATION.md 5c")
    ap.add_argument("--fsr-sharpness", default=None, metavar="{none|0..2}", help="RCAS sharpness of --scaler fsr: 0 (the sharpest) .. 2, "
                    "or none = EASU alone; default: the reference's 0.2")
    ap.add_argument("--downscaler", choices=_lib.DOWNSCALERS, default=None, help="what shrinks to an --out-size below --size, by at "
                    "most 4x per axis (hdrtv_post_rgb48_down; INTEGRATION.md 5c): mitchell, or ssim = the reference's chain, Mitchell "
                    "and its SSimDownscaler shader; default: none, a smaller --out-size is refused")
    ap.add_argument("--down-antiring", default=None, metavar="{auto|0..1}", help="anti-ringing of --downscaler: a strength in 0 .. 1, or "
                    "auto = the reference's 0.20; default: off")
    ap.add_argument("--film-grain", type=int, choices=(0, 1), default=0, help="the reference's flag: 1 = its film grain shader on the "
                    "delivered frames at its intensity 0.01, on the device and placed as its shader chain places it (hdrtv_post_rgb48_grain "
                    "and the _grain scalers; INTEGRATION.md 5c); with --scaler lanczos or fsr, without --downscaler and --deband")
    ap.add_argument("--film-grain-intensity", type=float, default=None, metavar="{0..0.1}", help="intensity of --film-grain 1 instead of "
                    "the reference's 0.01")
    ap.add_argument("--film-grain-seed", type=int, default=0, help="the stream's grain seed, 0 .. 2^32 - 1: frame n is grained with "
                    "hdrtv_film_grain_seed(seed, n)")
    ap.add_argument("--tone-mapping", choices=("none",) + tuple(_lib.TONE_CURVES), default="none", help="roll the delivered frames off to "
                    "--target-peak on the device (hdrtv_rgb48_tonemap / hdrtv_post_rgb48_tonemap; INTEGRATION.md 5i): spline = the "
                    "reference's mpv setting (this library's restatement of it), bt.2390 = the Report's EETF, clip; default: none")
    ap.add_argument("--target-peak", type=float, default=None, metavar="NITS", help="the sink's peak in nits, needed with --tone-mapping; at "
                    "or above --source-peak nothing is tone-mapped")
    ap.add_argument("--source-peak", type=float, default=_lib.TONE_SOURCE_PEAK, metavar="NITS", help="the peak the frames are mastered at; "
                    "default: the model's 1000 nits")
    ap.add_argument("--tone-mapping-param", type=float, default=None, metavar="{0..1}", help="contrast of --tone-mapping spline; default: "
                    "the reference's 0.45")
    ap.add_argument("--no-hg", action="store_true")
    ap.add_argument("--hg-weights", default=None, help="HG weight file, or seeded:<n>")
    ap.add_argument("--max-throughput", action="store_true", help="do not pace to the source clock")
    ap.add_argument("--no-prefetch", action="store_true", help="copy each frame into pinned memory on the processing thread, as the reference does")
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--csv")
    ap.add_argument("--gt", metavar="PATH", help="ground-truth frames for --objective-mode reference: rgb48le rawvideo at the delivered "
                    "size (--out-size), one frame per source frame")
    ap.add_argument("--objective-every", type=int, default=6, help="score every N-th processed frame against --gt (the reference "
                    "samples every sixth)")
    ap.add_argument("--objective-mode", choices=OBJECTIVE_MODES, default="tensor", help="what the objective metrics score: tensor (the "
                    "model's float tensor at the processing size) or reference (the delivered RGB48 codes against --gt, both "
                    "area-reduced to 512 on the longer side, as the reference's live path reports them)")
    a = ap.parse_args(argv)
    if a.objective_mode == "reference" and not a.gt:
        ap.error("--objective-mode reference needs --gt")
    if a.gt and a.objective_mode != "reference":
        ap.error("--gt holds RGB48 frames: it goes with --objective-mode reference")
    if a.gt and a.out_pix_fmt != "rgb48le":
        ap.error("--objective-mode reference scores RGB48 codes: --out-pix-fmt must be rgb48le")
    if a.objective_every < 1:
        ap.error("--objective-every must be at least 1")
    wd, ht = (int(v) for v in a.size.lower().split("x", 1))
    owd, oht = (int(v) for v in a.out_size.lower().split("x", 1)) if a.out_size else (wd, ht)
    try:
        swd, sht = (int(v) for v in a.src_size.lower().split("x", 1)) if a.src_size else (wd, ht)
    except ValueError:
        ap.error(f"--src-size {a.src_size}: expected WxH")
    if swd <= 0 or sht <= 0:
        ap.error(f"--src-size {swd}x{sht} is not positive")
    if a.downscaler is None and (owd < wd or oht < ht):
        ap.error(f"--out-size {owd}x{oht} is below --size {wd}x{ht}: the output stage only enlarges unless --downscaler is given")
    if a.down_antiring is not None and a.downscaler is None:
        ap.error("--down-antiring applies to --downscaler")
    if not a.input and a.pix_fmt != "bgr24":
        ap.error("--pix-fmt applies to an --input file")
    try:
        a.cleanup = _lib.output_cleanup(a.deband, a.deband_range, a.deband_threshold, a.dither, pix_fmt=a.out_pix_fmt)
    except ValueError as exc:
        ap.error(str(exc))
    if a.antiring is None:
        a.antiring = 0.0
    else:
        if (owd, oht) == (wd, ht):
            ap.error("--antiring applies to an upscale: --out-size equals --size")
        try:
            a.antiring = _lib.check_antiring(a.antiring if a.antiring.lower() == "auto" else float(a.antiring))
        except ValueError as exc:
            ap.error(f"--antiring: {exc}")
    if a.cas is None:
        a.cas = 0.0
    else:
        if (owd, oht) == (wd, ht):
            ap.error("--cas applies to an upscale: --out-size equals --size")
        try:
            a.cas = _lib.check_cas(a.cas if a.cas.lower() == "auto" else float(a.cas))
        except ValueError as exc:
            ap.error(f"--cas: {exc}")
    if a.fsr_sharpness is not None and a.scaler != "fsr":
        ap.error("--fsr-sharpness applies to --scaler fsr")
    try:
        if a.fsr_sharpness is None:
            a.fsr_sharpness = _lib.FSR_SHARPNESS
        else:
            a.fsr_sharpness = _lib.check_fsr_sharpness(None if a.fsr_sharpness.lower() == "none" else float(a.fsr_sharpness))
    except ValueError as exc:
        ap.error(f"--fsr-sharpness: {exc}")
    if a.scaler == "fsr":
        if (owd, oht) == (wd, ht):
            ap.error("--scaler fsr applies to an upscale: --out-size equals --size")
        try:
            _lib.check_fsr_size(wd, ht, owd, oht)
            a.antiring, a.cas = _lib.scaler_options("fsr", a.antiring, a.cas)
        except ValueError as exc:
            ap.error(f"--scaler fsr: {exc}")
    if a.scaler in _lib.SSIMSR_SCALERS:
        if (owd, oht) == (wd, ht):
            ap.error(f"--scaler {a.scaler} applies to an upscale: --out-size equals --size")
        try:
            _lib.check_ssimsr_size(wd, ht, owd, oht)
            a.antiring, a.cas = _lib.scaler_options(a.scaler, a.antiring, a.cas)
        except ValueError as exc:
            ap.error(f"--scaler {a.scaler}: {exc}")
    try:
        a.down_antiring = 0.0 if a.down_antiring is None else _lib.check_down_antiring(
            a.down_antiring if a.down_antiring.lower() == "auto" else float(a.down_antiring))
        _lib.down_options(a.downscaler, a.down_antiring, wd, ht, owd, oht, a.scaler, a.antiring, a.cas)
    except ValueError as exc:
        ap.error(f"--downscaler: {exc}")
    if a.film_grain_intensity is not None and not a.film_grain:
        ap.error("--film-grain-intensity applies to --film-grain 1")
    try:
        # a bool is the flag itself; an intensity is a float (never True / False, which check_film_grain reads as the flag)
        a.film_grain = _lib.check_grain_chain(bool(a.film_grain) if a.film_grain_intensity is None else float(a.film_grain_intensity),
                                              a.scaler, a.downscaler, a.cleanup.deband)
        a.film_grain_seed = _lib.check_grain_stream_seed(a.film_grain_seed)
    except ValueError as exc:
        ap.error(f"--film-grain: {exc}")
    if a.tone_mapping == "none" and (a.target_peak is not None or a.tone_mapping_param is not None):
        ap.error("--target-peak and --tone-mapping-param apply to --tone-mapping spline, bt.2390 or clip")
    try:
        a.tone = _lib.tone_mapping(a.tone_mapping, a.target_peak, a.source_peak, param=a.tone_mapping_param)
    except ValueError as exc:
        ap.error(f"--tone-mapping: {exc}")
    a.proc_wh, a.out_wh, a.src_wh = (wd, ht), (owd, oht), (swd, sht)
    return a


def main(argv=None):
    """``python -m hdrtv_mi355x.playback``: synthetic (or bgr24 / yuv420p / nv12 / 10-bit Y'CbCr rawvideo) source -> worker -> rgb48le sink."""
    import json

    from .worker import HeadlessPipelineWorker

    a = parse_args(argv)
    (wd, ht), (owd, oht), (swd, sht) = a.proc_wh, a.out_wh, a.src_wh
    if a.input:
        src = RawVideoSource(a.input, swd, sht, a.fps, pix_fmt=a.pix_fmt, yuv_matrix=a.yuv_matrix, yuv_full_range=a.yuv_range == "full")
    else:
        src = SyntheticSource(swd, sht, a.fps, a.frames)
    if not a.no_prefetch:
        src = PinnedPrefetch(src)
    worker = HeadlessPipelineWorker(a.weights_dir, use_hg=not a.no_hg, proc_w=wd, proc_h=ht, hg_weights=a.hg_weights,
                                    status_cb=lambda m: print(m, flush=True), out_w=owd, out_h=oht, out_pix_fmt=a.out_pix_fmt,
                                    out_siting=a.out_siting, light_stats=bool(a.light_level or a.light_level_json),
                                    deband=a.cleanup.deband, deband_range=a.cleanup.deband_range,
                                    deband_threshold=a.cleanup.deband_threshold, dither=a.cleanup.dither, antiring=a.antiring,
                                    cas=a.cas, scaler=a.scaler, fsr_sharpness=a.fsr_sharpness, downscaler=a.downscaler,
                                    down_antiring=a.down_antiring, film_grain=a.film_grain, grain_stream_seed=a.film_grain_seed,
                                    tone_mapping=a.tone_mapping, target_peak=a.target_peak, source_peak=a.source_peak,
                                    tone_param=a.tone_mapping_param)
    if not worker._load_model(a.precision):
        return 1
    sink = None
    if a.out:
        sink = RawVideoSink(a.out, owd, oht, a.fps, a.out_pix_fmt, a.out_siting)      # the sink, mpv_args() and ffmpeg_input_args() speak of the output size
        worker._start_hdr_feeder(sink)
    pb = RealtimePlayback(worker, src, sink=bool(sink), frame_stride=a.stride, realtime=not a.max_throughput, csv_path=a.csv,
                          letterbox=a.src_wh != a.proc_wh, gt_source=Rgb48leSource(a.gt, owd, oht) if a.gt else None,
                          objective_every=a.objective_every, objective_mode=a.objective_mode)
    res = pb.run(max_frames=a.frames)
    if sink:
        deadline = time.perf_counter() + 5.0
        while sink.frames < res["frames_processed"] and time.perf_counter() < deadline:
            time.sleep(0.01)
        worker._stop_hdr_feeder()
        sink.close()
        res["sink_frames"], res["sink_bytes"] = sink.frames, sink.bytes
    cll = worker.content_light             # fed by the feeder, frame by frame, from what the sink received
    worker.close()
    lm = res.pop("last_metrics") or {}
    res.update({k: lm.get(k) for k in ("latency_ms", "model_latency_ms", "fps_1p_low", "proc_res", "precision")})
    if a.gt:
        res.update({k: lm.get(k) for k in ("psnr_db", "sssim", "delta_e_itp")})
    if a.src_wh != a.proc_wh:
        res["src_res"] = f"{swd}x{sht}"
    if a.out_size:
        res["out_res"] = f"{owd}x{oht}"
    if a.out_pix_fmt != "rgb48le":
        res["out_pix_fmt"] = a.out_pix_fmt
    if a.cleanup.active:
        res["deband"], res["dither"] = a.cleanup.deband, a.cleanup.dither
    if a.antiring:
        res["antiring"] = _lib.resolve_antiring(a.antiring, wd, ht, owd, oht)
    if a.cas:
        res["cas"] = _lib.resolve_cas(a.cas, wd, ht, owd, oht)
    if a.scaler != "lanczos":
        res["scaler"], res["fsr_sharpness"] = a.scaler, a.fsr_sharpness
    if a.downscaler is not None:
        res["downscaler"], res["down_antiring"] = a.downscaler, a.down_antiring
    if a.film_grain:
        res["film_grain"], res["film_grain_seed"] = a.film_grain, a.film_grain_seed
    if a.tone is not None:
        res["tone_mapping"], res["target_peak"], res["source_peak"] = a.tone.kind, a.tone.target_peak, a.tone.source_peak
    if cll is not None:
        res["max_cll"], res["max_fall"], res["light_frames"] = cll.max_cll, cll.max_fall, cll.frames
        if a.light_level_json:
            with open(a.light_level_json, "w") as f:
                json.dump(cll.as_dict(), f, indent=1)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
