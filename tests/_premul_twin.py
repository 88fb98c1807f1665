"""Reference of premultiplied alpha: unpremultiply, lut3d, premultiply -- TEST INFRASTRUCTURE ONLY.

A composition of pieces that exist: stage 1 of the YUV contract (`oracle.lut3d_numpy.yuv_to_rgb_codes`), the two integer steps
below in int64, the C oracle's lut3d on the integer RGB (`oracle.binding.apply_rgb`: all five modes and the .csp prelut), and
stage 3 at the output layout (`oracle.lut3d_numpy.rgb_codes_to_yuv`) with the constants of `tests._xsub_twin.consts`.  The float
side is built on `tests._rgbf_twin` (`sanitize`, `apply_float`).
"""
from __future__ import annotations

import numpy as np

from oracle import binding as orc
from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
from tests import _rgbf_twin as rf
from tests import _xsub_twin as xs

F = np.float32
LAYOUTS = xs.LAYOUTS
consts = xs.consts


# ------------------------------------------------------------------ the two integer steps
def unpremul(c, a, ma, ml):
    """S = min(Ml, floor((C * Ma + floor(a / 2)) / a)) for a > 0, C for a == 0 (int64)."""
    c, a = np.asarray(c, dtype=np.int64), np.asarray(a, dtype=np.int64)
    a1 = np.maximum(a, 1)
    s = np.minimum((c * ma + a // 2) // a1, ml)
    return np.where(a > 0, s, c)


def premul(c, a, ma):
    """P = floor((C * a + floor(Ma / 2)) / Ma) (int64)."""
    c, a = np.asarray(c, dtype=np.int64), np.asarray(a, dtype=np.int64)
    return (c * a + ma // 2) // ma


def numerator_max(ma, ml):
    """The largest numerator either step forms with C <= Ml and a <= Ma: C * Ma + floor(a / 2) and C * a + floor(Ma / 2)."""
    return ml * ma + ma // 2


# ------------------------------------------------------------------ integer YUV
def apply(table, scale, interp, k, din, dl, dout, icsx, icsy, ocsx, ocsy, planes, alpha, prelut=None):
    """The contract: (Y, Cb, Cr) at the output depth and layout from the source's (Y, Cb, Cr) and its alpha plane (codes at
    `din` bits; a code above Ma counts as Ma, as lutr_alpha_plane reads it)."""
    ma, ml = (1 << din) - 1, (1 << dl) - 1
    a = np.minimum(np.asarray(alpha).astype(np.int64), ma)
    r, g, b = [np.asarray(p).astype(np.int64) for p in yuv_to_rgb_codes(k, icsx, icsy, planes)]
    dt = np.uint8 if dl <= 8 else np.uint16
    sr, sg, sb = [unpremul(c, a, ma, ml).astype(dt) for c in (r, g, b)]
    go, bo, ro = orc.apply_rgb(table, scale, dl, interp, (sg, sb, sr), prelut=prelut)
    p = [premul(c, a, ma) for c in (ro, go, bo)]
    return rgb_codes_to_yuv(k, dout, ocsx, ocsy, p)


# ------------------------------------------------------------------ float RGB
def alpha_t(a):
    """t = clamp(a, 0, 1); NaN -> 0 on the bit pattern, -0 and everything below -> +0."""
    a = np.ascontiguousarray(a, dtype=F)
    nan = (a.view(np.uint32) & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    with np.errstate(invalid="ignore"):
        t = np.where(a > 0, np.minimum(a, F(1)), F(0)).astype(F)
    t[nan] = F(0)
    return t


def unpremul_float(c, t):
    """S1 = sanitize(sanitize(C) / t) for t > 0, sanitize(C) for t == 0: one fp32 division, round to nearest even."""
    c1 = rf.sanitize(c)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore", under="ignore"):
        q = np.divide(c1, np.where(t > 0, t, F(1)).astype(F), dtype=F)
    return rf.sanitize(np.where(t > 0, q, c1).astype(F))


def apply_float(table, scale, interp, src, prelut=None):
    """gbrapf32le in, gbrapf32le out: (G, B, R, A) float32 planes; the alpha plane comes back as it is."""
    g, b, r, a = [np.ascontiguousarray(p, dtype=F) for p in src]
    t = alpha_t(a)
    s = [unpremul_float(c, t) for c in (g, b, r)]
    lut = rf.apply_float(table, scale, interp, s, prelut=prelut)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        out = [np.multiply(p, t, dtype=F) for p in lut]
    return out + [a.copy()]
