"""NumPy restatement of the film grain rule of include/hdrtv_mi355x.h (hdrtv_rgb48_film_grain and the ``_grain`` entry points): the
reference's last display shader, gaussian film grain, as a rule on u16 RGB48 codes.  Every operation is one float32 operation,
rounded on its own: no fused multiply-add, divisions are divisions (GLSL parses ``x * 1.0/289.0`` as ``(x * 1.0) / 289.0``), and
``fract(v) = v - floor(v)``.  The device kernels (csrc/film_grain.h) are held to these integers bit for bit.

``grain(H, W, seed)``: the float32 grain value of every position of an H x W frame, the same for the three channels.
``apply(codes, H, W, seed, intensity)``: the grained codes of a u16 ``(H, W, 3)`` frame.
``seed(stream_seed, frame_index)``: the per-frame seed in [0, 1), an integer hash, so that two sinks agree on a frame's grain."""
import numpy as np

F = np.float32
INTENSITY = 0.01                            # the reference's INTENSITY
# the shader's rational approximation of the inverse normal distribution, each constant rounded once to float32
A0, A1, A2 = F(0.151015505647689), F(-0.5303572634357367), F(1.365020122861334)
B0, B1 = F(0.132089632343748), F(-0.7607324991323768)
NORM = F(0.255121822830526)


def _fract(v):
    return v - np.floor(v)


def _permute(v):
    t = (F(34.0) * v + F(1.0)) * v
    return _fract(t / F(289.0)) * F(289.0)


def grain(H, W, seed):
    """float32 (H, W): g of the rule, for the per-frame ``seed`` (a float32 in [0, 1))."""
    H, W = int(H), int(W)
    px = (np.arange(W, dtype=F) + F(0.5)) / F(W)
    py = (np.arange(H, dtype=F) + F(0.5)) / F(H)
    mx = np.broadcast_to((px + F(1.0))[None, :], (H, W))
    my = np.broadcast_to((py + F(1.0))[:, None], (H, W))
    mz = F(seed) + F(1.0)
    state = _permute(_permute(mx) + my) + mz
    state = _permute(state)
    rnd = _fract(state / F(41.0))
    p = F(0.95) * rnd + F(0.025)
    q = p - F(0.5)
    r = q * q
    num = A1 * r + A0
    den = (r * r + B1 * r) + B0
    g = q * (A2 + num / den)
    g = g * NORM
    assert g.dtype == F
    return g


def apply(codes, H, W, seed, intensity):
    """The grained codes of ``codes`` (u16, (H, W, 3)): s = c / 65535, v = sat(s + I * g), G = (int)(v * 65535 + 0.5)."""
    codes = np.asarray(codes)
    assert codes.dtype == np.uint16 and codes.shape == (H, W, 3), (codes.dtype, codes.shape)
    ig = (F(intensity) * grain(H, W, seed))[:, :, None]
    s = codes.astype(F) / F(65535.0)
    v = np.minimum(np.maximum(s + ig, F(0.0)), F(1.0))
    out = (v * F(65535.0) + F(0.5)).astype(np.int32)
    return out.astype(np.uint16)


def seed_hash(stream_seed, frame_index):
    """The u32 hash h of the rule."""
    m = 0xFFFFFFFF
    h = ((int(frame_index) & m) * 0x9E3779B1 + (int(stream_seed) & m) * 0x85EBCA77) & m
    h ^= h >> 16
    h = (h * 0x21F0AAAD) & m
    h ^= h >> 15
    h = (h * 0x735A2D97) & m
    h ^= h >> 15
    return h


def seed(stream_seed, frame_index):
    """float32((h >> 8) * 2^-24): 24 bits, exact in float32, in [0, 1)."""
    return F((seed_hash(stream_seed, frame_index) >> 8) * 2.0 ** -24)
