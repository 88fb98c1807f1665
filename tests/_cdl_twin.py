"""Reference of the ASC CDL pass -- TEST INFRASTRUCTURE ONLY.

A composition of what exists plus the three lines of the CDL itself: stage 1 of the YUV contract at the INPUT layout
(`oracle.lut3d_numpy.yuv_to_rgb_codes`), stage A in NumPy float64 rounded to float32 (`table`), stage B in float32 step by step
(`saturate`), `oracle.lut3d_numpy._interp` on the clipped coordinates as `tests._rgbf_twin.lattice_rgb` forms them, lut3d's
truncation and clip, and stage 3 at the OUTPUT layout (`oracle.lut3d_numpy.rgb_codes_to_yuv` with `tests._xsub_twin.consts`).
tests/test_cdl.py pins it to the C oracle: with the identity CDL it is `tests._xsub_twin.apply`.
"""
from __future__ import annotations

import numpy as np

from oracle.lut3d_numpy import _interp, rgb_codes_to_yuv, yuv_to_rgb_codes
from tests import _xsub_twin as xs

F = np.float32
LAYOUTS = xs.LAYOUTS
consts = xs.consts
#: Rec.709 luma weights of ASC CDL v1.2, as the float32 constants the kernel holds
WR, WG, WB = F(0.2126), F(0.7152), F(0.0722)


def table(cdl, depth):
    """Stage A: float32 [3, 2^depth], the value of every integer code after slope, offset, clamp and power.  The CDL's numbers are
    taken as the float32 the C-ABI carries; the arithmetic is double (the product of two float32 is exact there)."""
    m = (1 << depth) - 1
    x = (np.arange(m + 1, dtype=F) * (F(1.0) / F(m))).astype(F).astype(np.float64)
    out = np.empty((3, m + 1), dtype=F)
    for c in range(3):
        s, o, p = float(F(cdl.slope[c])), float(F(cdl.offset[c])), float(F(cdl.power[c]))
        t = np.clip(x * s + o, 0.0, 1.0)
        out[c] = (t if p == 1.0 else np.power(t, p)).astype(F)
    return out


def luma(t):
    """l of stage B: every product and sum rounded to float32 on its own."""
    tr, tg, tb = t
    return (((WR * tr).astype(F) + (WG * tg).astype(F)).astype(F) + (WB * tb).astype(F)).astype(F)


def saturate(sat, t):
    """Stage B on float32 (T_R, T_G, T_B); nothing at all when sat == 1."""
    sat = F(sat)
    if sat == F(1.0):
        return list(t)
    lum = luma(t)
    return [np.clip((lum + (sat * (v - lum).astype(F)).astype(F)).astype(F), F(0), F(1)).astype(F) for v in t]


def lattice_codes(lut, interp, dl, unit):
    """Stage C up to lut3d's store: integer (R, G, B) codes at depth dl from unit floats (o_R, o_G, o_B)."""
    tab3 = np.asarray(lut.table, dtype=F)
    lut_max = F(tab3.shape[0] - 1)
    s = [np.clip((v * (F(sc) * lut_max)).astype(F), F(0), lut_max).astype(F) for v, sc in zip(unit, lut.scale)]
    v = _interp(tab3, interp, s)
    m = (1 << dl) - 1
    q = np.clip(np.trunc((v * F(m)).astype(F).astype(np.float64)), 0, m).astype(np.int64)
    return q[..., 0], q[..., 1], q[..., 2]


def unit_rgb(cdl, k, dl, icsx, icsy, planes, tab=None):
    """Stages 1, A and B: the float32 (o_R, o_G, o_B) the lattice is fed.  `tab`: stage A's table when it comes from elsewhere
    (the product's own lutr_cdl_table, so that a last-bit difference between two pows cannot fail a kernel test)."""
    tab = table(cdl, dl) if tab is None else np.asarray(tab, dtype=F)
    r, g, b = yuv_to_rgb_codes(k, icsx, icsy, planes)
    return saturate(cdl.saturation, [tab[0][r], tab[1][g], tab[2][b]])


def apply(lut, cdl, interp, k, dl, dout, icsx, icsy, ocsx, ocsy, planes, tab=None):
    """The contract: (Y, Cb, Cr) at the output depth and layout.  interp: nearest | trilinear | tetrahedral."""
    return rgb_codes_to_yuv(k, dout, ocsx, ocsy, lattice_codes(lut, interp, dl, unit_rgb(cdl, k, dl, icsx, icsy, planes, tab)))
