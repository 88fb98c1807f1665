"""Reference of the blue-noise dither in the output stage -- TEST INFRASTRUCTURE ONLY.

Stages 1 and 2 are those of the existing twins (`tests/_xsub_twin.lut_rgb` for YUV sources, `tests/_rgb2yuv_twin.lut_rgb` and
`tests/_rgbf_twin.codes_rgb` for RGB and float ones).  Stage 3 is `_xsub_twin.unquantised` without its `- 0.5`: c, the float32 value
the output stage floors without dither.  Then q = clip(floor(c + d), 0, max_o) in float32, d = (2 rank - 4095) / 8192 from the
mask `lutr_dither_mask` returns, by the sample's position in its own plane.
"""
from __future__ import annotations

import numpy as np

from lut_renderer_amd import _native
from oracle.lut3d_numpy import _fma
from tests import _rgb2yuv_twin as r2y
from tests import _rgbf_twin as rgbf
from tests import _xsub_twin as xs

F = np.float32
#: the shift of the mask per output plane (Y, Cb, Cr)
OX = (0, 24, 40)
OY = (0, 37, 11)

_offsets = None


def offsets() -> np.ndarray:
    """d for every cell of the mask: float32 [64, 64], exact."""
    global _offsets
    if _offsets is None:
        rank = _native.dither_mask().astype(np.int64)
        _offsets = ((2 * rank - 4095) / 8192.0).astype(F)
    return _offsets


def plane_offsets(plane: int, h: int, w: int, d=None) -> np.ndarray:
    """d for the samples of a whole output plane of h x w samples, (0, 0) at the frame's top-left."""
    d = offsets() if d is None else d
    y = (np.arange(h) + OY[plane]) & 63
    x = (np.arange(w) + OX[plane]) & 63
    return d[np.ix_(y, x)]


def unrounded(k, ocsx, ocsy, rgb):
    """Stage 3 up to the value handed to clip_floor: `_xsub_twin.unquantised` without its - 0.5, as float32 planes."""
    ro, go, bo = [np.asarray(a).astype(F) for a in rgb]
    h, w = ro.shape
    y = _fma(F(k.cyr), ro, _fma(F(k.cyg), go, _fma(F(k.cyb), bo, F(k.yob)))).astype(F)
    bh, bw = 1 << ocsy, 1 << ocsx
    ch, cw = (h + bh - 1) >> ocsy, (w + bw - 1) >> ocsx

    def block_sum(a):
        pad = np.pad(a, ((0, ch * bh - h), (0, cw * bw - w)), mode="edge")
        return pad.reshape(ch, bh, cw, bw).sum(axis=(1, 3)).astype(F)

    rs, gs, bs = block_sum(ro), block_sum(go), block_sum(bo)
    cb = _fma(F(k.cbr), rs, _fma(F(k.cbg), gs, _fma(F(k.cbb), bs, F(k.cob)))).astype(F)
    cr = _fma(F(k.crr), rs, _fma(F(k.crg), gs, _fma(F(k.crb), bs, F(k.cob)))).astype(F)
    return y, cb, cr


def quantise_plane(c, plane: int, max_o: float, wide: bool, d=None) -> np.ndarray:
    """q = clip(floor(c + d), 0, max_o): one float32 add, rounded once.  d = a [64, 64] table (default: the mask's offsets)."""
    c = np.asarray(c, dtype=F)
    s = (c + plane_offsets(plane, c.shape[0], c.shape[1], d)).astype(F)
    return np.clip(np.floor(s), F(0), F(max_o)).astype(np.uint16 if wide else np.uint8)


def quantise(k, dout, ocsx, ocsy, rgb):
    """(Y, Cb, Cr) at the output depth and layout from the LUT's integer (R, G, B)."""
    return [quantise_plane(c, p, float(k.max_o), dout > 8) for p, c in enumerate(unrounded(k, ocsx, ocsy, rgb))]


def apply(table, scale, interp, k, dl, dout, icsx, icsy, ocsx, ocsy, planes, prelut=None):
    """A YUV source: `_xsub_twin.apply` with the dithered quantisation (any pair of layouts, the equal ones included)."""
    return quantise(k, dout, ocsx, ocsy, xs.lut_rgb(table, scale, interp, k, dl, icsx, icsy, planes, prelut))


def apply_rgb(table, scale, interp, k, pix_fmt, dout, ocsx, ocsy, src, prelut=None):
    """An integer RGB source (`_rgb2yuv_twin.apply`)."""
    return quantise(k, dout, ocsx, ocsy, r2y.lut_rgb(table, scale, interp, pix_fmt, src, prelut))


def apply_rgbf(table, scale, interp, k, dout, ocsx, ocsy, src, prelut=None):
    """A float RGB source (`_rgbf_twin.apply_yuv`)."""
    return quantise(k, dout, ocsx, ocsy, rgbf.codes_rgb(table, scale, interp, src, prelut))
