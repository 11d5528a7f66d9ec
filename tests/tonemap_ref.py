"""NumPy restatement of the tone-map pixel rule of include/hdrtv_mi355x.h (hdrtv_rgb48_tonemap / hdrtv_post_rgb48_tonemap): the
yardstick the GPU tests hold the kernels to bit for bit.  On u16 RGB48 codes of BT.2020 PQ, with the curve as ``gain[65536]``:

    m = max(R, G, B);  g = gain[m];  per channel c:  y = lin[c] * g (ONE float32 multiply);  y = min(max(y, 0), 1);  out = code(y)

``lin`` is read from the library (``hdrtv_pq_eotf_table``, host only) and ``code`` is the oracle's ``orc_pq_code`` (the ST.2084 OETF
in double precision, ``floor(pq(y) * 65535 + 0.5)``), so nothing here is derived with a second math library.  The curves that fill
``gain`` live in the product (hdrtv_mi355x/tonemap.py) and are not used here: a table is an input."""
import ctypes

import numpy as np

F = np.float32
_ORC = None


def _orc_pq_code():
    global _ORC
    if _ORC is None:
        from oracle import hdrtvnet_oracle as O
        so = ctypes.CDLL(O._lib()._name)              # a handle of our own: the oracle's prototypes stay as they are
        so.orc_pq_code.restype = ctypes.c_uint16
        so.orc_pq_code.argtypes = [ctypes.c_float]
        _ORC = so.orc_pq_code
    return _ORC


def lin_table():
    """The rule's ``lin[65536]`` (float32): the level, 1.0 = 10000 nits, of every code."""
    from hdrtv_mi355x import lib as L
    return L.pq_eotf_table()


def code(y):
    """``orc_pq_code`` of every element of the float32 array ``y`` (values in [0, 1]) -> int64 codes."""
    y = np.ascontiguousarray(y, dtype=F)
    f = _orc_pq_code()
    vals, inv = np.unique(y.reshape(-1), return_inverse=True)
    codes = np.fromiter((f(float(v)) for v in vals), dtype=np.int64, count=vals.size)
    return codes[inv].reshape(y.shape)


def apply(codes, gain, lin=None):
    """The tone-mapped codes of a u16 ``(H, W, 3)`` frame under the float32 table ``gain[65536]``."""
    c = np.asarray(codes)
    gain = np.asarray(gain)
    assert c.dtype == np.uint16 and c.ndim == 3 and c.shape[2] == 3 and gain.dtype == F and gain.shape == (65536,)
    lin = lin_table() if lin is None else lin
    assert lin.dtype == F and lin.shape == (65536,)
    g = gain[c.max(axis=2)][:, :, None]
    y = lin[c] * g                                    # float32 * float32 -> float32, rounded to nearest: the rule's one multiply
    assert y.dtype == F
    y = np.minimum(np.maximum(y, F(0)), F(1))
    return code(y).astype(np.uint16)
