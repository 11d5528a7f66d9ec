"""Parity of the HIP path (through the C ABI) against the oracle and the committed golden
vectors.  All tests here need a real MI355X: ``pytest -m gpu``.

Tolerances (stated once, used below):
  * pre/post quantisers, given identical float inputs: EXACT integers.
  * network floats: the product computes in fp16 storage / fp32 accumulate, the oracle and
    the goldens are the reference's CPU fp32 path.  Every bar below is 1.5 x the worst value the round-5 build
    prints over all tests of this file (gpurun_out/r5_gputest_b.log; values on O(1) tensors): AGCM out max_abs
    9.0e-4 -> 1.35e-3; LE / final out max_abs 2.46e-3 -> 3.7e-3, mean_abs 1.66e-4 -> 2.5e-4; u8 max 1 -> 2 LSB,
    mean 0.055 -> 0.09 LSB; per-tap bars next to their tests.  (The reference's own bar for a re-quantised graph
    is float MAE <= 0.02 and u8 MAE <= 5, scripts/validate_tensorrt_sources.py:598-609.)
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

AGCM_MAX = 1.35e-3
OUT_MAX, OUT_MEAN = 3.7e-3, 2.5e-4
U8_MAX, U8_MEAN = 2, 0.09
# HG taps against the oracle on the device's own LE output: (max_abs, mean_abs), measured 3.3e-3 / 1.4e-4, 8.8e-3 / 4.7e-4 (conv5_2),
# 2.1e-3 / 2.1e-4 (conv9) at 96x128 .. 2176x3840
HG_TAP = {"hg.conv2": (4.9e-3, 2.2e-4), "hg.conv5_2": (1.32e-2, 7.0e-4), "hg.conv9": (3.1e-3, 3.2e-4)}
HG_OUT_MAX = 1.4e-3                  # final HG output vs the oracle on our base: measured 9.4e-4


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def proc_hr(torch_cuda, golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0)
    yield p
    p.close()


@pytest.fixture(scope="module")
def proc_hg(torch_cuda, golden_dir):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234",
                       warmup_passes=0)
    yield p
    p.close()


def _stats(name, got, want):
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    print(f"  {name}: max_abs={d.max():.3e} mean_abs={d.mean():.3e} ref_absmean={np.abs(want).mean():.3e}")
    return d.max(), d.mean()


def test_library_is_native(proc_hr):
    from hdrtv_mi355x import lib
    assert os.path.exists(lib.LIB_PATH)
    assert b"gfx950" in lib.load().hdrtv_version()


def test_pre_exact_and_cond(proc_hr, golden_dir, torch_cuda):
    from oracle import hdrtvnet_oracle as O
    d = np.load(os.path.join(golden_dir, "scalar_tables.npz"))
    frame = np.zeros((16, 256, 3), np.uint8)
    frame[:, :, 0] = d["u8"][None]          # B
    frame[:, :, 1] = d["u8"][None, ::-1]    # G
    frame[:, :, 2] = ((d["u8"][None].astype(np.int32) * 7) % 256).astype(np.uint8)
    # 16 rows is below the classifier's minimum, but preprocess alone has no such limit -> use 80 rows
    frame = np.ascontiguousarray(np.tile(frame, (5, 1, 1)))
    t, c = proc_hr.preprocess(frame)
    t = t.float().cpu().numpy()[0]
    assert np.array_equal(t[2, 0].astype(np.float16), d["pre_f16"])
    assert np.array_equal(t[1, 0].astype(np.float16), d["pre_f16"][::-1])
    g = np.load(os.path.join(golden_dir, "hr_64x96_noise_s0.npz"))
    t, c = proc_hr.preprocess(g["frame"])
    assert np.array_equal(t.float().cpu().numpy()[0], g["tensor"].astype(np.float16).astype(np.float32))
    mx, _ = _stats("cond", c.float().cpu().numpy()[0], g["cond"])
    assert mx <= 1.2e-3        # fp16 input rounding (2.4e-4) + fp16 output rounding (4.9e-4 at 1.0)
    # exactness against the oracle fed the SAME fp16-rounded input
    ref = O.bicubic_aa_quarter(g["tensor"].astype(np.float16).astype(np.float32)).astype(np.float16)
    assert np.abs(c.cpu().numpy()[0].astype(np.float32) - ref.astype(np.float32)).max() <= 1e-3


@pytest.mark.parametrize("hw", [(64, 96), (61, 103), (1080, 1920), (2160, 3840)])
def test_post_quantisers_exact(proc_hr, torch_cuda, golden_dir, hw):
    """fp32 and fp16 inputs through post_u8 / post_rgb48 vs the oracle: exact integers."""
    import ctypes as C
    from hdrtv_mi355x import lib as L
    from oracle import hdrtvnet_oracle as O
    torch = torch_cuda
    h, w = hw
    rng = np.random.default_rng(h * 1000 + w)
    x = rng.uniform(-0.05, 1.05, (3, h, w)).astype(np.float32)
    tab = np.load(os.path.join(golden_dir, "scalar_tables.npz"))["post_in"]
    x.reshape(-1)[: tab.size] = tab
    lib = L.load()
    for dt, tdt in ((L.F32, torch.float32), (L.F16, torch.float16)):
        xin = torch.from_numpy(x).to("cuda").to(tdt).contiguous()
        xf = xin.float().cpu().numpy()
        u8 = torch.empty((h, w, 3), dtype=torch.uint8, device="cuda")
        u16 = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.hdrtv_post_u8(proc_hr._ctx, st, xin.data_ptr(), dt, h, w, u8.data_ptr()) == 0
        assert lib.hdrtv_post_rgb48(proc_hr._ctx, st, xin.data_ptr(), dt, h, w, u16.data_ptr()) == 0
        torch.cuda.synchronize()
        assert np.array_equal(u16.cpu().numpy(), O.post_rgb48(xf))      # feeder always upcasts to fp32
        if dt == L.F32:
            assert np.array_equal(u8.cpu().numpy(), O.postprocess_u8(xf))
        else:
            # reference fp16 tensors quantise in fp16: clamp, *255 (round), +0.5 (round), trunc
            c = np.clip(xf, 0, 1).astype(np.float16)
            m = (c.astype(np.float32) * np.float32(255)).astype(np.float16)
            a = (m.astype(np.float32) + np.float32(0.5)).astype(np.float16)
            want = a.astype(np.float32).astype(np.uint8)[::-1].transpose(1, 2, 0)
            assert np.array_equal(u8.cpu().numpy(), want)


def test_post_pq_matches_oracle(proc_hr, torch_cuda):
    """BT.709 -> BT.2020 + ST.2084 PQ -> u16: EXACT integers.  The code is defined as floor(pq(y) * 65535 + 0.5) with the OETF
    in double precision for the fp32 argument y (oracle: orc_pq_code); the device reaches it through a table of the 65535
    code boundaries, so no math-library rounding is involved on either side.  1080 x 1920 random values + a dense sweep."""
    import ctypes as C
    from hdrtv_mi355x import lib as L
    from oracle import hdrtvnet_oracle as O
    torch = torch_cuda
    h, w = 1080, 1920
    x = np.random.default_rng(3).uniform(-0.05, 1.05, (3, h, w)).astype(np.float32)
    x[:, 1, :] = np.linspace(0.0, 1.0, w, dtype=np.float32)[None]              # grey ramp: every channel sweeps the curve
    x[:, 2, :] = (np.linspace(0.0, 1.0, w, dtype=np.float32) ** 4)[None]       # dense near black, where the curve is steep
    x[:, 0, :4] = np.array([0.0, 0.1, 1.0, 0.5])[None]
    xin = torch.from_numpy(x).cuda()
    u16 = torch.empty((h, w, 3), dtype=torch.uint16, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.load().hdrtv_post_pq_rgb48(proc_hr._ctx, st, xin.data_ptr(), L.F32, h, w, C.c_float(1000.0), u16.data_ptr()) == 0
    torch.cuda.synchronize()
    got = u16.cpu().numpy().astype(int)
    want = O.post_pq_rgb48(x, 1000.0).astype(int)
    assert np.array_equal(got, want)
    assert got[0, 2].tolist() == [49271, 49271, 49271] and got[0, 0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("hw", [(5, 7), (1, 7), (61, 103)])
def test_post_pq_ragged_tail_matches_oracle(proc_hr, torch_cuda, hw):
    """Pixel counts that are no multiple of eight: the last npix % 8 pixels leave post_rgb48_kernel<T, true> through its one-pixel
    tail (35 = four groups + 3, 7 = the tail alone, 6283 = several blocks + 3).  Exact integers from f32 and f16 input, and nothing
    written past the frame."""
    import ctypes as C
    from hdrtv_mi355x import lib as L
    from oracle import hdrtvnet_oracle as O
    torch = torch_cuda
    h, w = hw
    x = np.random.default_rng(100 * h + w).uniform(-0.05, 1.05, (3, h, w)).astype(np.float32)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for dt, tdt in ((L.F32, torch.float32), (L.F16, torch.float16)):
        xin = torch.from_numpy(x).to("cuda").to(tdt).contiguous()
        u16 = torch.full((h * w * 3 + 8,), 0xA5A5, dtype=torch.uint16, device="cuda")
        assert L.load().hdrtv_post_pq_rgb48(proc_hr._ctx, st, xin.data_ptr(), dt, h, w, C.c_float(1000.0), u16.data_ptr()) == 0
        torch.cuda.synchronize()
        got = u16.cpu().numpy()
        assert (got[h * w * 3:] == 0xA5A5).all()
        assert np.array_equal(got[:h * w * 3].reshape(h, w, 3), O.post_pq_rgb48(xin.float().cpu().numpy(), 1000.0)), dt


@pytest.mark.parametrize("name", ["hr_64x96_noise_s0", "hr_60x100_noise_s2", "hr_52x76_gradient_s5",
                                  "hr_32x96_gradient_s1_taps"])
def test_hr_golden(proc_hr, golden_dir, hr_state, name):
    from oracle import hdrtvnet_oracle as O
    d = np.load(os.path.join(golden_dir, name + ".npz"))
    t, c = proc_hr.preprocess(d["frame"])
    out, agcm = proc_hr.infer((t, c))
    out_np, agcm_np = out.float().cpu().numpy()[0], agcm.float().cpu().numpy()[0]
    bias = proc_hr.tap("agcm.bias").numpy().ravel()
    if "fea6" in d.files:
        mx, _ = _stats("fea6", bias[160:166], d["fea6"])
        assert mx <= 1e-6            # fp32 on both sides (measured 1.3e-8)
    mx, _ = _stats("agcm_out", agcm_np, d["agcm_out"])
    assert mx <= AGCM_MAX
    # LE stage taps against the oracle evaluated on OUR agcm output (isolates LE from AGCM error)
    taps = {}
    O.le(hr_state, agcm_np, taps)
    # 1.5 x measured (7.5e-4, 7.8e-4, 1.23e-3, 2.1e-3, 4.8e-3 on values ~1.5, 1.2e-3, 1.6e-3, 3.8e-3)
    for ours, theirs, tol in (("le.cond", "LE.cond_first", 1.2e-3), ("le.cond1", "LE.CondNet1", 1.2e-3),
                              ("le.cond2", "LE.CondNet2", 1.9e-3), ("le.cond3", "LE.CondNet3", 3.2e-3),
                              ("le.cond4", "LE.CondNet4", 7.2e-3), ("le.fea0", None, 1.8e-3),
                              ("le.fea1", "LE.recon_trunk1", 2.5e-3), ("le.fea2", "LE.recon_trunk2", 5.8e-3)):
        got = proc_hr.tap(ours).numpy()
        if theirs is None:
            want = np.maximum(taps["LE.HR_conv1"], 0)
        else:
            want = taps[theirs]
        mx, _ = _stats(ours, got, want)
        assert mx <= tol, ours
    mx, mean = _stats("out", out_np, d["out"])
    assert mx <= OUT_MAX and mean <= OUT_MEAN
    u8 = proc_hr.postprocess((out, agcm)).astype(int)
    du8 = np.abs(u8 - d["u8_bgr"].astype(int))
    print(f"  u8: max={du8.max()} mean={du8.mean():.3f}")
    assert du8.max() <= U8_MAX and du8.mean() <= U8_MEAN


@pytest.mark.parametrize("name", ["hg_96x128_gradient_s3", "hg_80x112_gradient_s4"])
def test_hg_golden(proc_hg, golden_dir, hr_state, hg_state, name):
    from oracle import hdrtvnet_oracle as O
    d = np.load(os.path.join(golden_dir, name + ".npz"))
    t, c = proc_hg.preprocess(d["frame"])
    out, agcm = proc_hg.infer((t, c))
    assert out.dtype.is_floating_point and out.element_size() == 4      # fp32, as the reference's mask promotion gives
    out_np = out.cpu().numpy()[0]
    base = proc_hg.tap("le.out").numpy()
    mx, _ = _stats("base", base, d["tap:base"])
    assert mx <= OUT_MAX
    # HG evaluated by the oracle on OUR base (isolates HG; the highlight mask is a hard threshold)
    mask = O.hg_mask(base)
    h, w = base.shape[1:]
    ph, pw = (32 - h % 32) % 32, (32 - w % 32) % 32
    taps = {}
    ref = O.hg_generator(hg_state, np.pad(base, ((0, 0), (0, ph), (0, pw)), mode="reflect"),
                         np.pad(mask, ((0, 0), (0, ph), (0, pw)), mode="reflect"), taps)[:, :h, :w]
    assert np.array_equal(proc_hg.tap("hg.mask").numpy()[:, :h, :w], mask)
    # 1.5 x measured (2.9e-3, 4.2e-3, 7.6e-3, 8.2e-3, 6.7e-3, 3.3e-3, 3.0e-3, 2.2e-3, 1.9e-3)
    for ours, tol in (("hg.conv2", 4.5e-3), ("hg.conv3_2", 6.4e-3), ("hg.conv4_2", 1.15e-2), ("hg.conv5_2", 1.25e-2),
                      ("hg.conv_code2", 1.0e-2), ("hg.conv6", 5e-3), ("hg.conv7", 4.6e-3), ("hg.conv8", 3.4e-3),
                      ("hg.conv9", 2.9e-3)):
        mx, _ = _stats(ours, proc_hg.tap(ours).numpy(), taps[ours])
        assert mx <= tol, ours
    mx, mean = _stats("hg_out vs oracle(our base)", out_np, ref)
    assert mx <= HG_OUT_MAX and mean <= 2.1e-5               # measured 7.2e-4 / 1.4e-5
    # against the reference's golden output, away from pixels whose mask bit flipped under fp16
    same = (mask == d["mask"])[0]
    print(f"  mask flips vs golden: {int((~same).sum())} of {same.size}")
    assert (~same).mean() <= 0.002
    dd = np.abs(out_np - d["out"])[:, same]
    print(f"  hg_out vs golden: max_abs={dd.max():.3e} mean_abs={dd.mean():.3e}")
    assert dd.max() <= 3.5e-3 and dd.mean() <= 2.6e-4        # measured 2.3e-3 / 1.7e-4


def test_mid_size_vs_oracle(proc_hg, hr_state, hg_state):
    """272x480 (oracle finishes in seconds): full AGCM+LE+HG, gradient+highlight frame."""
    from hdrtv_mi355x import weights as W
    from oracle import hdrtvnet_oracle as O
    f = W.synthetic_frame(272, 480, seed=11, kind="gradient")
    t, c = proc_hg.preprocess(f)
    out, agcm = proc_hg.infer((t, c))
    base = proc_hg.tap("le.out").numpy()
    rt, rc = O.preprocess(f)
    rbase, ragcm = O.hr_forward(hr_state, rt, rc)
    mx, mean = _stats("base 272x480", base, rbase)
    assert mx <= OUT_MAX and mean <= OUT_MEAN
    mask = O.hg_mask(base)
    ph, pw = (32 - 272 % 32) % 32, 0
    ref = O.hg_generator(hg_state, np.pad(base, ((0, 0), (0, ph), (0, pw)), mode="reflect"),
                         np.pad(mask, ((0, 0), (0, ph), (0, pw)), mode="reflect"))[:, :272, :480]
    mx, mean = _stats("hg 272x480", out.cpu().numpy()[0], ref)
    assert mx <= HG_OUT_MAX and mean <= 4e-6                 # measured 7.6e-4 / 2.2e-6 (the mask is sparse)


@pytest.mark.parametrize("hw", [(1080, 1920), (2160, 3840)])
def test_full_size_properties(proc_hr, torch_cuda, hw):
    """BASELINE.json sizes: exact pre/post identities, determinism, and locality (a change in one
    corner cannot move LE outputs far away -- catches tile-seam / block-remap indexing errors)."""
    from hdrtv_mi355x import weights as W
    torch = torch_cuda
    h, w = hw
    f = W.synthetic_frame(h, w, seed=1234, kind="noise")
    t, c = proc_hr.preprocess(f)
    # pre -> post_u8 is the identity on u8
    assert np.array_equal(proc_hr.postprocess(t), f)
    tn = t.float().cpu().numpy()[0]
    assert np.array_equal(tn, ((f[:, :, ::-1].astype(np.float32) * np.float32(1 / 255.0)).astype(np.float16)
                               .astype(np.float32)).transpose(2, 0, 1))
    t0, c0 = t.clone(), c.clone()
    out1 = proc_hr.infer((t0, c0))[0].clone()
    out2 = proc_hr.infer((t0, c0))[0].clone()
    assert torch.equal(out1, out2)                      # no atomics anywhere: bit-reproducible
    assert torch.isfinite(out1).all()
    t1 = t0.clone()
    t1[:, :, :32, :32] = 1.0 - t1[:, :, :32, :32]
    out3 = proc_hr.infer((t1, c0))[0]
    assert not torch.equal(out3[:, :, :64, :64], out1[:, :, :64, :64])
    assert torch.equal(out3[:, :, 400:, :], out1[:, :, 400:, :])
    assert torch.equal(out3[:, :, :, 400:], out1[:, :, :, 400:])


def test_process_api_and_errors(proc_hr, golden_dir, torch_cuda):
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    d = np.load(os.path.join(golden_dir, "hr_64x96_noise_s0.npz"))
    out, pre, run, post = proc_hr.process_timed(d["frame"])
    assert out.shape == (64, 96, 3) and out.dtype == np.uint8 and min(pre, run, post) >= 0
    assert np.abs(out.astype(int) - d["u8_bgr"].astype(int)).max() <= U8_MAX
    assert proc_hr.warmup_compile(96, 64) is None and proc_hr._compiled is False
    with pytest.raises(ValueError):
        HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), precision="bf16")
    with pytest.raises(FileNotFoundError):
        HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), hg_weights="/nonexistent/HG.pt")
    with pytest.raises(RuntimeError):
        HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), device="cpu")
    with pytest.raises(Exception):
        proc_hr.process(np.zeros((16, 16, 3), np.uint8))        # too small for the classifier's InstanceNorm


@pytest.mark.parametrize("tag,prec", [("full_qat", "int8-full"), ("mixed_qat", "int8-mixed")])
def test_int8_checkpoint_storage(golden_dir, torch_cuda, tag, prec):
    """precision='int8-*': INT8 storage, fp16 compute -- the reference's own behaviour on ROCm
    (pre-dequantize at load).  Bars: the fp16 tolerances above (its quantised-graph bar is u8 MAE <= 5)."""
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    p = HDRTVNetMI355X(os.path.join(golden_dir, f"hr_int8_{tag}.hdrw"), precision=prec, use_hg=False, warmup_passes=0)
    try:
        assert p.precision == prec and p._is_w8_model is False
        d = np.load(os.path.join(golden_dir, f"int8_{tag}_64x96_gradient_s6.npz"))
        t, c = p.preprocess(d["frame"])
        out, agcm = p.infer((t, c))
        mx, mean = _stats(f"int8 {tag} out", out.float().cpu().numpy()[0], d["out"])
        assert mx <= OUT_MAX and mean <= OUT_MEAN
        du8 = np.abs(p.postprocess(out).astype(int) - d["u8_bgr"].astype(int))
        assert du8.max() <= U8_MAX and du8.mean() <= U8_MEAN
        with pytest.raises(ValueError):
            HDRTVNetMI355X(os.path.join(golden_dir, f"hr_int8_{tag}.hdrw"), precision="fp16", use_hg=False)
        with pytest.raises(ValueError):
            HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), precision=prec, use_hg=False)
    finally:
        p.close()


def test_persistent_schedules_do_not_change_results(torch_cuda, golden_dir, monkeypatch):
    """Every conv kernel is persistent (a workgroup walks a run of tiles with cross-tile DMA prefetch and
    hand-counted vmcnt waits), but the small goldens give each workgroup a single tile.  At 3840x2160 with HG,
    the real schedule must reproduce, bit for bit, the one-tile-per-workgroup schedule (variant force_ncu) that
    the goldens validate: per-tile arithmetic does not depend on which workgroup runs the tile or in what order."""
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    torch = torch_cuda
    path = os.path.join(golden_dir, "hr_weights.hdrw")
    f = W.synthetic_frame(2160, 3840, seed=21, kind="gradient")
    outs = []
    for force in (None, "4000000"):
        if force:
            monkeypatch.setenv("HDRTV_VARIANTS", "force_ncu=" + force)      # read once, by hdrtv_create
        else:
            monkeypatch.delenv("HDRTV_VARIANTS", raising=False)
        p = HDRTVNetMI355X(path, use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
        out, agcm = p.infer(p.preprocess(f))
        outs.append((out.clone(), agcm.clone(), p.tap("le.out").clone(), p.tap("hg.conv9").clone()))
        p.close()
    for a, b in zip(*outs):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


def test_full_hd_hg_vs_oracle(proc_hg, hr_state, hg_state):
    """BASELINE.json configs[1] size (1920x1080, padded to 1088 rows for HG), where every persistent kernel runs
    several tiles per workgroup: the HG head against the oracle evaluated on our LE output.  The highlight mask
    is sparse on synthetic frames (the LE output rarely exceeds 0.775), so the U-Net body is checked at its last
    full-width tensor (conv9, input of Up_conv5) as well as at the masked output.  ~10 s of oracle CPU time."""
    from hdrtv_mi355x import weights as W
    from oracle import hdrtvnet_oracle as O
    h, w = 1080, 1920
    f = W.synthetic_frame(h, w, seed=31, kind="gradient")
    out, agcm = proc_hg.infer(proc_hg.preprocess(f))
    base = proc_hg.tap("le.out").numpy()
    mask = O.hg_mask(base)
    print(f"  highlight mask fraction: {mask.mean():.5f}")
    ph = (32 - h % 32) % 32
    taps = {}
    ref = O.hg_generator(hg_state, np.pad(base, ((0, 0), (0, ph), (0, 0)), mode="reflect"),
                         np.pad(mask, ((0, 0), (0, ph), (0, 0)), mode="reflect"), taps)[:, :h, :w]
    for name, (tol, tol_mean) in HG_TAP.items():
        mx, mean = _stats(name + " 1088x1920", proc_hg.tap(name).numpy(), taps[name])
        assert mx <= tol and mean <= tol_mean, name
    mx, mean = _stats("hg out 1080x1920", out.cpu().numpy()[0], ref)
    assert mx <= HG_OUT_MAX and mean <= 1e-6                 # measured 7.1e-4 / 3.3e-8 (0.02 % of the pixels are masked in)
    # LE itself at this size (multi-tile persistent schedule of every LE kernel) against the oracle's whole HR forward
    rt, rc = O.preprocess(f)
    rbase, ragcm = O.hr_forward(hr_state, rt, rc)
    mx, mean = _stats("le.out 1080x1920 vs O.hr_forward", base, rbase)
    assert mx <= OUT_MAX and mean <= OUT_MEAN
    mx, _ = _stats("agcm 1080x1920", agcm.float().cpu().numpy()[0], ragcm)
    assert mx <= AGCM_MAX


def test_full_hd_hg_tail_dense_mask(proc_hg, hr_state, hg_state):
    """The HG tail -- Up_conv5's fused pixel-shuffle + 64->3 dot-product epilogue (conv_pglds<ps_dot3>) and
    hg_final_fused -- reaches the output only through the highlight mask, which is on for ~0.02 % of the pixels of a
    synthetic frame at the reference's mask_r = 0.75.  HG_Composite takes mask_r as a constructor argument
    (HG_Composite_arch.py:21): with mask_r = 0.3 more than half of the 1080x1920 frame is masked in, so the whole tail is
    compared with the oracle over the whole frame, and its partial sums (hg.part) over all 1088x1920 padded pixels."""
    from hdrtv_mi355x import weights as W
    from oracle import hdrtvnet_oracle as O
    h, w = 1080, 1920
    f = W.synthetic_frame(h, w, seed=32, kind="gradient")
    proc_hg.set_hg_mask_r(0.3)
    try:
        out, agcm = proc_hg.infer(proc_hg.preprocess(f))
        out_np = out.cpu().numpy()[0]
        base = proc_hg.tap("le.out").numpy()
        part = proc_hg.tap("hg.part").numpy().reshape(-1).reshape(1088, w, 4)[:, :, :3].transpose(2, 0, 1)
        dev_mask = proc_hg.tap("hg.mask").numpy()[:, :h, :w]
    finally:
        proc_hg.set_hg_mask_r(0.75)
    mask = O.hg_mask(base, r=0.3)
    frac = float(mask.mean())
    print(f"  highlight mask fraction at mask_r=0.3: {frac:.3f}")
    assert frac >= 0.2
    assert np.array_equal(dev_mask, mask)
    ph = (32 - h % 32) % 32
    taps = {}
    ref = O.hg_generator(hg_state, np.pad(base, ((0, 0), (0, ph), (0, 0)), mode="reflect"),
                         np.pad(mask, ((0, 0), (0, ph), (0, 0)), mode="reflect"), taps)[:, :h, :w]
    # first half of conv10 (Hallucination_arch.py:131-133) over Up_conv5's 64 channels, bias excluded
    w10 = np.asarray(hg_state["conv10.weight"], np.float32).reshape(3, 128)[:, :64]
    want_part = np.einsum("ok,khw->ohw", w10, taps["hg.up5"]).astype(np.float32)
    mx, mean = _stats("hg.part (ps_dot3 epilogue) 1088x1920", part, want_part)
    assert mx <= 1.5e-3 and mean <= 1.5e-4                   # measured 9.7e-4 / 9.6e-5
    mx, mean = _stats("hg out, dense mask", out_np, ref)
    assert mx <= HG_OUT_MAX and mean <= 1e-4                 # measured 9.3e-4 / 6.5e-5
    inside = mask[0] > 0
    dd = np.abs(out_np - ref)[:, inside]
    print(f"  masked-in pixels only ({int(inside.sum())}): max_abs={dd.max():.3e} mean_abs={dd.mean():.3e}")
    assert dd.max() <= HG_OUT_MAX


def test_uhd_le_vs_oracle(proc_hr, hr_state):
    """BASELINE.json configs[2] size: AGCM + LE at 3840x2160 against the oracle's HR forward (~40 s of CPU)."""
    from hdrtv_mi355x import weights as W
    from oracle import hdrtvnet_oracle as O
    O.set_threads(min(16, os.cpu_count() or 1))
    f = W.synthetic_frame(2160, 3840, seed=41, kind="gradient")
    out, agcm = proc_hr.infer(proc_hr.preprocess(f))
    rt, rc = O.preprocess(f)
    rbase, ragcm = O.hr_forward(hr_state, rt, rc)
    mx, mean = _stats("le.out 2160x3840 vs O.hr_forward", out.float().cpu().numpy()[0], rbase)
    assert mx <= OUT_MAX and mean <= OUT_MEAN
    mx, _ = _stats("agcm 2160x3840", agcm.float().cpu().numpy()[0], ragcm)
    assert mx <= AGCM_MAX


@pytest.mark.parametrize("variant", ["fp16", "int8-full", "int8-mixed"])
def test_one_barrier_conv32_schedule_is_bit_identical(torch_cuda, golden_dir, monkeypatch, variant):
    """conv32s.hip (one barrier per tile, wave-private epilogue, counted vmcnt waits) against conv32p.hip's single-pass
    kernels it replaces (variant conv32_old = 1): same tiles, same per-element arithmetic, so the LE output and every
    intermediate must agree bit for bit -- at 4K (126 tiles per workgroup: the steady state of the three-buffer
    pipeline), at 1080p and at sizes with ragged right / bottom tiles (masked lanes store to the trash line)."""
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    torch = torch_cuda
    if variant == "fp16":
        p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=False, warmup_passes=0, _ab_library=True)
    else:
        tag = variant.split("-")[1]
        p = HDRTVNetMI355X(os.path.join(golden_dir, f"hr_int8_{tag}_qat.hdrw"), precision=variant, predequantize="off",
                           use_hg=False, warmup_passes=0, _ab_library=True)
    taps = ("le.fea0", "le.fea1", "le.fea3", "le.up1", "le.up3", "le.out")
    try:
        for (h, w), seed in (((2160, 3840), 41), ((1080, 1920), 42), ((270, 486), 43), ((61, 103), 44)):
            f = W.synthetic_frame(h, w, seed=seed, kind="gradient" if seed % 2 else "noise")
            res = []
            # old schedule (conv_first as its own launch) | new schedule, conv_first unfused | new schedule with conv_first
            # computed inside HR_conv1's kernel (the default for fp16 HR_conv1 among the per-layer kernels)
            # (int8-full: no_c3q8 = the generic planar3_to_q8 + conv_q8 form of the W8A8 conv_first against conv_c3_q8)
            # conv32_nosplit: every wave convolves and prepares (conv32s's first form) against the role split
            # le_rows = 0 throughout: the fused row-streaming kernels (tests/test_gpu_le_rows.py) would bypass these layers
            switches = ("conv32_old", "no_c3fuse", "no_c3q8", "conv32_nosplit")
            p.set_variant("le_rows", 0)
            for env in ({"conv32_old": 1, "no_c3q8": 1}, {"no_c3fuse": 1, "conv32_nosplit": 1}, {"conv32_nosplit": 1}, {"no_c3fuse": 1}, {}):
                for k in switches:
                    p.set_variant(k, env.get(k, 0))
                out, _ = p.infer(p.preprocess(f))
                res.append([out.clone()] + [p.tap(t).clone() for t in taps])
            for other in res[1:]:
                for name, a, b in zip(("out",) + taps, res[0], other):
                    assert torch.isfinite(a).all(), (h, w, name)
                    assert torch.equal(a, b), (h, w, name)
    finally:
        p.close()


def test_smallest_frames_and_rejections(torch_cuda, golden_dir, hr_state):
    """Edge sizes.  The reference accepts any frame whose condition map keeps more than one spatial element up to the
    4th InstanceNorm of the classifier (torch's instance_norm raises below that; hdrtv_reserve mirrors it) and, with HG,
    whose reflect padding to a multiple of 32 is smaller than the frame (F.pad reflect raises otherwise).  The smallest
    frames that pass -- strips 8 pixels wide or high, single-tile everywhere, most lanes of every kernel masked -- against
    the oracle (u8, +-1 as the f16 path allows), and the rejections as errors, not garbage."""
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.lib import HdrtvError
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    from oracle import hdrtvnet_oracle as O
    path = os.path.join(golden_dir, "hr_weights.hdrw")
    p = HDRTVNetMI355X(path, use_hg=False, warmup_passes=0)
    try:
        for (h, w) in ((68, 8), (8, 68), (68, 12), (9, 70), (40, 72), (33, 130)):
            f = W.synthetic_frame(h, w, seed=3, kind="noise")
            d = np.abs(p.process(f).astype(int) - O.process(hr_state, f).astype(int))
            assert d.max() <= 1 and d.mean() < 0.1, (h, w, d.max(), d.mean())
        for (h, w), what in (((4, 4), "unsupported frame size"), ((65, 9), "AGCM classifier"), ((47, 33), "AGCM classifier")):
            with pytest.raises(HdrtvError, match=what):
                p.process(W.synthetic_frame(h, w, seed=3, kind="noise"))
        with pytest.raises(HdrtvError, match="16.7 Mpixel"):          # 32-bit LDS-DMA offsets: refused, not wrapped around
            p.process(np.zeros((4400, 7800, 3), np.uint8))
        assert p.process(W.synthetic_frame(68, 8, seed=4, kind="noise")).shape == (68, 8, 3)     # still usable after a refusal
    finally:
        p.close()
    ph = HDRTVNetMI355X(path, use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    try:
        with pytest.raises(HdrtvError, match="reflect padding"):
            ph.process(W.synthetic_frame(68, 8, seed=3, kind="gradient"))
        for (h, w) in ((33, 130), (68, 40)):
            out = ph.process(W.synthetic_frame(h, w, seed=3, kind="gradient"))
            assert out.shape == (h, w, 3)
    finally:
        ph.close()


def test_persistent_1x1_matches_tile_kernel(torch_cuda, golden_dir, monkeypatch):
    """conv_glds1p (the HG fuse convs conv6..conv9 as one persistent stream of (tile, chunk) iterations, wave-private
    epilogue strips, counted vmcnt waits across tile boundaries) against the one-tile-per-workgroup kernel it replaces
    (variant glds1_old = 1): same accumulation order, so every tap must agree bit for bit -- at 1080p (32 tiles per workgroup
    on conv9) and at a size with ragged tiles."""
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    torch = torch_cuda
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0, _ab_library=True)
    try:
        for (h, w), seed in (((1080, 1920), 51), ((270, 486), 52)):
            f = W.synthetic_frame(h, w, seed=seed, kind="gradient")
            res = []
            for old in (1, 0):
                p.set_variant("glds1_old", old)
                out, _ = p.infer(p.preprocess(f))
                res.append([out.clone()] + [p.tap(t).clone() for t in ("hg.conv6", "hg.conv7", "hg.conv8", "hg.conv9")])
            for name, a, b in zip(("out", "conv6", "conv7", "conv8", "conv9"), res[0], res[1]):
                assert torch.isfinite(a).all(), (h, w, name)
                assert torch.equal(a, b), (h, w, name)
    finally:
        p.close()


def test_private_weight_conv_schedule_is_bit_identical(torch_cuda, golden_dir, monkeypatch):
    """conv_prw (csrc/conv3x3_prw.hip: 256 output channels per workgroup, a wave owns 32 of them for the whole 16x16 tile
    and keeps its weight rows in a private LDS ring; one barrier per 64-channel chunk) against conv_pglds (variant prw = 0):
    same accumulation order per output element, so every HG tensor and the final output agree bit for bit -- at 4K (the
    steady state of the cross-tile software pipeline), at 1080p, and at sizes with ragged right / bottom tiles and with
    fewer tiles than workgroups.  prw = 2 forces the new schedule onto every layer it can run (the default, 1, leaves
    the low-resolution layers on conv_pglds)."""
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    torch = torch_cuda
    taps = ("hg.conv2", "hg.conv3_2", "hg.conv4_2", "hg.conv5_2", "hg.conv_code2", "hg.conv6", "hg.conv7", "hg.conv8", "hg.conv9")
    p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights="seeded:1234", warmup_passes=0)
    try:
        for (h, w), seed in (((2160, 3840), 71), ((1080, 1920), 72), ((270, 486), 73), ((97, 131), 74)):
            f = W.synthetic_frame(h, w, seed=seed, kind="gradient")
            res = []
            for mode in ("0", "1", "2"):
                p.set_variant("prw", int(mode))
                out, _ = p.infer(p.preprocess(f))
                res.append([out.clone()] + [p._tap_device(t).clone() for t in taps] + [p._tap_device("hg.part").clone()])
                if mode != "0":
                    p.profile_enable(True)
                    p.infer(p.preprocess(f))
                    kern = [k for _, k, _, _, _ in p.profile_read()]
                    p.profile_enable(False)
                    assert (sum("conv_prw" in k for k in kern) >= 7) if (mode == "2" or h >= 1080) else True
            for other in res[1:]:
                for name, a, b in zip(("out",) + taps + ("hg.part",), res[0], other):
                    assert torch.isfinite(a.float()).all(), (h, w, name)
                    # Up_conv5's fused 64 -> 3 dot products included: both kernels form them per 32-channel half on the matrix
                    # pipe from one table and add the halves (conv_prw across a wave pair, conv_pglds inside a wave)
                    assert torch.equal(a, b), (h, w, name, int((a != b).sum()))
            assert torch.equal(res[1][0], res[2][0]) and torch.equal(res[1][-1], res[2][-1])      # both conv_prw runs agree exactly
    finally:
        p.close()


@pytest.mark.gpu
def test_hg_tail_variants_are_bit_identical(torch_cuda, golden_dir, monkeypatch):
    """The HG tail (conv10's second half over conv1, conv_last, mask blend; Hallucination_arch.py:130-137): by default conv1's
    kernel leaves the 64 -> 3 sums per pixel (conv_c3<64,dot3>) and a per-pixel kernel finishes (hg_final_light);
    variant final_recompute = 1 recomputes conv1 inside the tail (hg_final_fused).  Same fragments, same expressions in the same order:
    the outputs agree bit for bit -- at 4K, at 1080p, at a width that is not a multiple of 4 (scalar stores) and at a size with
    fewer tiles than workgroups; fp16 and W8A8 HG heads."""
    from hdrtv_mi355x import weights as W
    from hdrtv_mi355x.processor import HDRTVNetMI355X
    torch = torch_cuda
    for hgw in ("seeded:1234", "seeded-w8a8:1234"):
        p = HDRTVNetMI355X(os.path.join(golden_dir, "hr_weights.hdrw"), use_hg=True, hg_weights=hgw, warmup_passes=0, _ab_library=True)
        try:
            for (h, w), seed in (((2160, 3840), 81), ((1080, 1920), 82), ((97, 131), 83), ((64, 96), 84)):
                f = W.synthetic_frame(h, w, seed=seed, kind="gradient")
                res = {}
                for mode in ("1", "0"):
                    p.set_variant("final_recompute", int(mode))
                    out, _ = p.infer(p.preprocess(f))
                    p.profile_enable(True)
                    p.infer(p.preprocess(f))
                    kern = [k for _, k, _, _, _ in p.profile_read()]
                    p.profile_enable(False)
                    assert ("hg_final_fused" in kern) == (mode == "1") and ("hg_final_light" in kern) == (mode == "0"), kern
                    assert ("conv_c3<64,dot3>" in kern) == (mode == "0"), kern
                    res[mode] = (out.clone(), p._tap_device("hg.p1" if "w8a8" not in hgw else "hg8.p1").clone())
                assert torch.isfinite(res["0"][0]).all()
                assert torch.equal(res["0"][0], res["1"][0]), (hgw, h, w, (res["0"][0] - res["1"][0]).abs().max().item())
                assert torch.equal(res["0"][1], res["1"][1]), (hgw, h, w)
        finally:
            p.close()
