"""The FSR rule of hdrtv_post_rgb48_fsr (include/hdrtv_mi355x.h), restated in plain NumPy: EASU (edge-adaptive spatial upsampling)
of the u16 codes, then, optionally, RCAS (robust contrast-adaptive sharpening) of the float32 EASU image, then quant_u16.  Every
float operation is a float32 operation of its own -- NumPy rounds each elementwise multiply, add and divide separately and fuses
nothing -- so the arrays below ARE the rule, op by op; denormals are kept.  The arithmetic is that of the reference's display shader
for its default upscaler (FidelityFX FSR 1.0.2 on RGB: de-ringing on, full analysis, no early exit, RCAS with denoise), written
out from its operations.  Orders the shader leaves open are fixed here:
  luma        (0.2126 r + 0.7152 g) + 0.0722 b
  len         len + ((w * lenX) + (w * lenY))
  min / max   any order: no NaN and no negative zero reaches them
  RCAS sum    (((lobe b + lobe d) + lobe h) + lobe f) + e;  the denoise mean 0.25 * (((b + d) + f) + h)
"""
import numpy as np

F = np.float32
RCP_MAGIC, RSQ_MAGIC = 0x7EF07EBB, 0x5F347D74
LUMA_R, LUMA_G, LUMA_B = F(0.2126), F(0.7152), F(0.0722)
LOB_K = F((0.25 - 0.04) - 0.5)              # -0.29 as a float32
W_B = F(2.0 / 5.0)
RCAS_LIMIT = F(0.25 - 1.0 / 16.0)
EPS = F(1e-6)
MAX_RATIO = 2


def positions(n, m):
    """Per destination index d of an axis with n source and m destination samples: fp[d] = floor(p) (int32) and
    pp[d] = float32(p - fp[d]) with p = (d + 0.5) * n / m - 0.5 in double."""
    d = np.arange(m, dtype=np.float64)
    p = (d + 0.5) * n / m - 0.5
    fp = np.floor(p)
    return fp.astype(np.int32), (p - fp).astype(F)


def aprx_rcp(a):
    """The low-precision reciprocal: an integer subtraction on the u32 pattern of the float32."""
    return (np.uint32(RCP_MAGIC) - np.asarray(a, F).view(np.uint32)).view(F)


def aprx_rsq(a):
    """The low-precision reciprocal square root, likewise."""
    return (np.uint32(RSQ_MAGIC) - (np.asarray(a, F).view(np.uint32) >> np.uint32(1))).view(F)


def samples(codes):
    """u16 codes -> float32 samples: one correctly rounded division (a unorm16 texture fetch)."""
    return np.asarray(codes).astype(F) / F(65535)


def _luma(c):
    return (LUMA_R * c[..., 0] + LUMA_G * c[..., 1]) + LUMA_B * c[..., 2]


def _clamp01(x):
    return np.minimum(np.maximum(x, F(0)), F(1))


def easu(codes, dh, dw, with_weight=False):
    """(H, W, 3) u16 codes -> the float32 EASU image (dh, dw, 3); with_weight: also the weight sums aW (dh, dw)."""
    s = samples(codes)
    h, w = s.shape[:2]
    fy, py = positions(h, dh)
    fx, px = positions(w, dw)
    ppx, ppy = np.broadcast_to(px[None, :], (dh, dw)), np.broadcast_to(py[:, None], (dh, dw))

    def tap(ox, oy):
        return s[np.clip(fy + oy, 0, h - 1)[:, None], np.clip(fx + ox, 0, w - 1)[None, :]]

    offs = {"b": (0, -1), "c": (1, -1), "e": (-1, 0), "f": (0, 0), "g": (1, 0), "h": (2, 0), "i": (-1, 1), "j": (0, 1), "k": (1, 1),
            "l": (2, 1), "n": (0, 2), "o": (1, 2)}
    col = {k: tap(*v) for k, v in offs.items()}
    lum = {k: _luma(v) for k, v in col.items()}
    one = F(1)
    wgt = {"s": (one - ppx) * (one - ppy), "t": ppx * (one - ppy), "u": (one - ppx) * ppy, "v": ppx * ppy}
    dirx = np.zeros((dh, dw), F)
    diry = np.zeros((dh, dw), F)
    ln = np.zeros((dh, dw), F)
    for key, (la, lb, lc, ld, le) in (("s", "befgj"), ("t", "cfghk"), ("u", "fijkn"), ("v", "gjklo")):
        wt = wgt[key]
        la, lb, lc, ld, le = lum[la], lum[lb], lum[lc], lum[ld], lum[le]
        dc, cb = ld - lc, lc - lb
        lenx = aprx_rcp(np.maximum(np.abs(dc), np.abs(cb)))
        dx = ld - lb
        lenx = _clamp01(np.abs(dx) * lenx)
        lenx = lenx * lenx
        ec, ca = le - lc, lc - la
        leny = aprx_rcp(np.maximum(np.abs(ec), np.abs(ca)))
        dy = le - la
        leny = _clamp01(np.abs(dy) * leny)
        leny = leny * leny
        dirx = dirx + dx * wt
        diry = diry + dy * wt
        ln = ln + ((wt * lenx) + (wt * leny))
    dirr = dirx * dirx + diry * diry
    zro = dirr < F(1.0 / 32768.0)
    dirr = np.where(zro, one, aprx_rsq(dirr))
    dirx = np.where(zro, one, dirx)
    dirx = dirx * dirr
    diry = diry * dirr
    ln = ln * F(0.5)
    ln = ln * ln
    stretch = (dirx * dirx + diry * diry) * aprx_rcp(np.maximum(np.abs(dirx), np.abs(diry)))
    len2x = one + (stretch - one) * ln
    len2y = one + F(-0.5) * ln
    lob = F(0.5) + LOB_K * ln
    clp = aprx_rcp(lob)
    ac = np.zeros((dh, dw, 3), F)
    aw = np.zeros((dh, dw), F)
    for k in "bcijfeklhgon":
        ox, oy = offs[k]
        offx, offy = F(ox) - ppx, F(oy) - ppy
        vx = (offx * dirx) + (offy * diry)
        vy = (offx * -diry) + (offy * dirx)
        vx = vx * len2x
        vy = vy * len2y
        d2 = np.minimum(vx * vx + vy * vy, clp)
        wb = W_B * d2 + F(-1)
        wa = lob * d2 + F(-1)
        wb = wb * wb
        wa = wa * wa
        wb = F(25.0 / 16.0) * wb + F(-(25.0 / 16.0 - 1.0))
        wk = wb * wa
        ac = ac + col[k] * wk[..., None]
        aw = aw + wk
    pix = ac / aw[..., None]
    mn = np.minimum(np.minimum(col["f"], np.minimum(col["g"], col["j"])), col["k"])
    mx = np.maximum(np.maximum(col["f"], np.maximum(col["g"], col["j"])), col["k"])
    pix = _clamp01(np.minimum(np.maximum(pix, mn), mx))
    return (pix, aw) if with_weight else pix


def sharp_factor(sharpness):
    """float32(2^-sharpness), computed in double from the float32 the C entry point receives."""
    return F(2.0 ** -float(F(sharpness)))


def rcas(img, sharpness):
    """The float32 EASU image -> the float32 RCAS image of the same size; sharpness in [0, 2] (0 = sharpest)."""
    e = np.asarray(img, F)
    pad = np.pad(e, ((1, 1), (1, 1), (0, 0)), mode="edge")
    b, d, f, h = pad[:-2, 1:-1], pad[1:-1, :-2], pad[1:-1, 2:], pad[2:, 1:-1]
    mn1 = np.minimum(np.minimum(b, np.minimum(d, f)), h)
    mx1 = np.maximum(np.maximum(b, np.maximum(d, f)), h)
    hit_min = np.minimum(mn1, e) / np.maximum(F(4) * mx1, EPS)
    hit_max = (F(1) - np.maximum(mx1, e)) / np.minimum(F(4) * mn1 - F(4), -EPS)
    lobe = np.maximum(-RCAS_LIMIT, np.minimum(np.maximum(-hit_min, hit_max), F(0))) * sharp_factor(sharpness)
    rng = np.maximum(mx1, e) - np.minimum(mn1, e)
    nz = np.abs(F(0.25) * (((b + d) + f) + h) - e) / np.maximum(rng, EPS)
    nzmax = _clamp01(np.maximum(nz[..., 0], np.maximum(nz[..., 1], nz[..., 2])))
    lobe = lobe * (F(-0.5) * nzmax + F(1))[..., None]
    rcp = F(1) / (F(4) * lobe + F(1))
    pix = ((((lobe * b + lobe * d) + lobe * h) + lobe * f) + e) * rcp
    return _clamp01(pix)


def quant(img):
    """quant_u16 of csrc/post_quant.h on values in [0, 1]: (int)(x * 65535 + 0.5), both operations float32."""
    return (np.asarray(img, F) * F(65535) + F(0.5)).astype(np.int32).astype(np.uint16)


def scale(codes, dh, dw, sharpness=None):
    """hdrtv_post_rgb48_fsr on (H, W, 3) u16 codes: sharpness None = rcas 0 (EASU alone), else rcas 1 with that sharpness.
    Equal sizes return the codes; more than 2x on an axis, or shrinking, is refused."""
    codes = np.asarray(codes)
    h, w = codes.shape[:2]
    if not (h <= dh <= MAX_RATIO * h and w <= dw <= MAX_RATIO * w):
        raise ValueError("FSR scales by 1 .. 2 per axis")
    if (dh, dw) == (h, w):
        return codes.astype(np.uint16)
    img = easu(codes, dh, dw)
    if sharpness is not None:
        img = rcas(img, sharpness)
    return quant(img)
