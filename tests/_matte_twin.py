"""Reference of the stage stack with a matte plane scaling the strength per pixel -- TEST INFRASTRUCTURE ONLY.

`tests._mix_twin` with the strength of a pixel formed from its frame's strength and its matte sample, in the five operations of
the contract with `np.float32` intermediates: the integer clamp, the integer inversion, the normalisation (one rounded product
with rcp = 1.0f / (float)Mm), the scaling (one rounded product) and the mix (product, sum, sum of the rounding).  A still matte
([rows, cols] or [1, rows, cols]) broadcasts over the frames; a per-frame strength broadcasts over [nf, rows, cols].
"""
from __future__ import annotations

import numpy as np

from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
from tests import _mix_twin as mix
from tests import _stack_twin as st

F = np.float32
LAYOUTS = st.LAYOUTS
consts = st.consts
clamp = mix.clamp


def rcp(depth):
    """1.0f / (float)Mm, formed once."""
    return (F(1.0) / F((1 << depth) - 1)).astype(F)


def matte_t(a, depth, invert=False):
    """t = (float)a'' * rcp: a' = min(a, Mm) and a'' = invert ? Mm - a' : a' on integers."""
    mm = (1 << depth) - 1
    a = np.minimum(np.asarray(a).astype(np.int64), mm)
    if invert:
        a = mm - a
    return (a.astype(F) * rcp(depth)).astype(F)


def weight(strength, a, depth, invert=False):
    """w = s' * t, one rounded product.  `strength` a scalar, or one per frame for a = [nf, rows, cols]."""
    t = matte_t(a, depth, invert)
    s = clamp(strength)
    sb = s.reshape(s.shape + (1,) * (t.ndim - s.ndim)) if s.ndim else s
    return (sb * t).astype(F)


def mix_codes(w, q0, q1):
    """q_c = (int)((q0_c + w * (q1_c - q0_c)) + 0.5f) per channel, w an array of the planes' shape (already in [0, 1])."""
    out = []
    for a, b in zip(q0, q1):
        a, b = np.asarray(a).astype(F), np.asarray(b).astype(F)
        d = (b - a).astype(F)                                   # exact: both are integers below 2^16
        p = (w * d).astype(F)
        t = (a + p).astype(F)
        out.append((t + F(0.5)).astype(F).astype(np.int64))
    return tuple(out)


def apply(stages, strength, matte, depth, invert, k, dl, dout, icsx, icsy, ocsx, ocsy, planes, **res):
    """The contract: (Y, Cb, Cr) at the output depth and layout.  `planes` [rows, cols] or [nf, rows, cols]; `matte` [rows, cols]
    of the luma plane's size, [1, rows, cols] or [nf, rows, cols]; `strength` a scalar or one per frame."""
    single = np.asarray(planes[0]).ndim == 2
    if single:
        planes = [np.asarray(p)[None] for p in planes]
    nf = planes[0].shape[0]
    matte = np.asarray(matte)
    m = np.broadcast_to(matte if matte.ndim == 3 else matte[None], (nf,) + planes[0].shape[1:])
    per_frame = np.broadcast_to(np.asarray(strength, dtype=F), (nf,))
    out = []
    for f in range(nf):
        frame = [p[f] for p in planes]
        q0 = tuple(np.asarray(v).astype(np.int64) for v in yuv_to_rgb_codes(k, icsx, icsy, frame))
        q1 = st.rgb_out(stages, k, dl, icsx, icsy, frame, **res)
        q = mix_codes(weight(per_frame[f], m[f], depth, invert), q0, q1)
        out.append(rgb_codes_to_yuv(k, dout, ocsx, ocsy, q))
    if single:
        return out[0]
    return [np.stack([f[i] for f in out]) for i in range(3)]
