"""Reference of the 1D LUT pass -- TEST INFRASTRUCTURE ONLY.

Two parts.  `table`: the per-code table formulas of the section in NumPy float32, written from the section's text and independent
of csrc/cube_parse.cpp (every operation is rounded to float32 with an explicit astype; NumPy never contracts).  `apply`: the pixel
contract as a composition of what exists, like `tests._xsub_twin`: stage 1 at the INPUT layout
(`oracle.lut3d_numpy.yuv_to_rgb_codes`), the lookup, the C oracle's lut3d on the codes (`oracle.binding.apply_rgb`, every mode and
the .csp prelut) or nothing, and stage 3 at the OUTPUT layout (`rgb_codes_to_yuv` with `tests._xsub_twin.consts`).
"""
from __future__ import annotations

import numpy as np

from oracle import binding as orc
from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
from tests import _xsub_twin as xs

F = np.float32
LAYOUTS = xs.LAYOUTS
consts = xs.consts
MODES = ("nearest", "linear", "cosine", "cubic", "spline")


def table(lut, scale, interp1d, depth):
    """uint16 [3, 2^depth]: T_c[k] for every integer code.  lut: float32 [3, n]; scale: the three floats of the reader."""
    lut = np.asarray(lut, dtype=F)
    n = lut.shape[1]
    m = (1 << depth) - 1
    factor = F(m)
    k = np.arange(m + 1, dtype=F)
    out = np.empty((3, m + 1), np.uint16)
    for c in range(3):
        row = lut[c]
        sc = F(F(F(scale[c]) / factor) * F(n - 1))
        s = (k * sc).astype(F)
        prev = s.astype(np.int64)                                  # truncation; s >= 0
        nxt = np.minimum(prev + 1, n - 1)
        mu = (s - prev.astype(F)).astype(F)
        p, q = row[prev], row[nxt]
        if interp1d == "nearest":
            v = row[(s.astype(np.float64) + 0.5).astype(np.int64)]
        elif interp1d == "linear":
            v = (p + ((q - p).astype(F) * mu).astype(F)).astype(F)
        elif interp1d == "cosine":
            a = (mu.astype(np.float64) * np.pi).astype(F)
            w = ((F(1.0) - np.cos(a).astype(F)).astype(F) * F(0.5)).astype(F)
            v = (p + ((q - p).astype(F) * w).astype(F)).astype(F)
        else:
            y0, y1, y2, y3 = row[np.maximum(prev - 1, 0)], p, q, row[np.minimum(nxt + 1, n - 1)]
            if interp1d == "cubic":
                mu2 = (mu * mu).astype(F)
                a0 = (((y3 - y2).astype(F) - y0).astype(F) + y1).astype(F)
                a1 = ((y0 - y1).astype(F) - a0).astype(F)
                a2 = (y2 - y0).astype(F)
                t0 = ((a0 * mu).astype(F) * mu2).astype(F)
                v = (((t0 + (a1 * mu2).astype(F)).astype(F) + (a2 * mu).astype(F)).astype(F) + y1).astype(F)
            elif interp1d == "spline":
                c1 = (F(0.5) * (y2 - y0).astype(F)).astype(F)
                c2 = (((y0 - (F(2.5) * y1).astype(F)).astype(F) + (F(2.0) * y2).astype(F)).astype(F) - (F(0.5) * y3).astype(F)).astype(F)
                c3 = ((F(0.5) * (y3 - y0).astype(F)).astype(F) + (F(1.5) * (y1 - y2).astype(F)).astype(F)).astype(F)
                v = (((((((c3 * mu).astype(F) + c2).astype(F) * mu).astype(F) + c1).astype(F) * mu).astype(F)) + y1).astype(F)
            else:
                raise ValueError(interp1d)
        x = np.clip((v * factor).astype(F), F(0), factor)
        out[c] = x.astype(np.int64).astype(np.uint16)               # truncation of a value in [0, M]
    return out


def lookup(tab, rgb):
    """q'_c = T_c[q_c] on integer (R, G, B) arrays."""
    r, g, b = rgb
    return tab[0][r].astype(np.int64), tab[1][g].astype(np.int64), tab[2][b].astype(np.int64)


def rgb_codes(tab, k, icsx, icsy, planes):
    """Stage 1 and the lookup: the integer (R, G, B) between the two filters."""
    return lookup(tab, yuv_to_rgb_codes(k, icsx, icsy, planes))


def lut3d_codes(lut, interp, dl, rgb, prelut=None):
    """The C oracle's lut3d on integer (R, G, B) at depth dl."""
    r, g, b = rgb
    dt = np.uint8 if dl <= 8 else np.uint16
    go, bo, ro = orc.apply_rgb(lut.table, lut.scale, dl, interp, (g.astype(dt), b.astype(dt), r.astype(dt)), prelut=prelut)
    return ro, go, bo


def apply(tab, lut, interp, k, dl, dout, icsx, icsy, ocsx, ocsy, planes, prelut=None):
    """The contract: (Y, Cb, Cr) at the output depth and layout.  interp None: lut1d alone (lut is not read)."""
    rgb = rgb_codes(tab, k, icsx, icsy, planes)
    if interp is not None:
        rgb = lut3d_codes(lut, interp, dl, rgb, prelut)
    return rgb_codes_to_yuv(k, dout, ocsx, ocsy, rgb)


def apply_rgb(tab, depth, planes):
    """Planar RGB (gbrp order G, B, R) at `depth`: out_c = T_c[min(code_c, M)]."""
    m = (1 << depth) - 1
    g, b, r = [np.minimum(np.asarray(p).astype(np.int64) & 0xffff, m) for p in planes]
    dt = np.uint8 if depth <= 8 else np.uint16
    return tab[1][g].astype(dt), tab[2][b].astype(dt), tab[0][r].astype(dt)
