"""Reference of the RGB source -> YUV output pass -- TEST INFRASTRUCTURE ONLY.

The contract is a composition of existing oracle pieces, like tests/_xsub_twin.py: the C oracle's lut3d on the integer RGB at
the source's depth (`oracle.binding.apply_rgb` / `apply_packed`: every interpolation mode, the .csp prelut), then stage 3 of
the YUV contract at the OUTPUT layout (`oracle.lut3d_numpy.rgb_codes_to_yuv`: block mean over the output block, a partial block
padded with its edge) with the oracle's constants at the output block's n (`oracle.binding.yuv_constants(chroma_n=...)`).
"""
from __future__ import annotations

import numpy as np

from oracle import binding as orc
from oracle.lut3d_numpy import rgb_codes_to_yuv
from tests import _xsub_twin as xs

LAYOUTS = xs.LAYOUTS
PACKED = orc.PACKED


def source_depth(pix_fmt: str) -> int:
    """The depth lut3d runs at: the source's."""
    if pix_fmt in PACKED:
        return PACKED[pix_fmt][0]
    d = pix_fmt[4:].replace("le", "")
    return int(d) if d else 8


def consts(matrix_out="smpte170m", range_out="tv", dl=10, dout=None, ocsx=1, ocsy=1):
    """The oracle's constant block: only its output side is used (the input side is given the same matrix and range)."""
    return orc.yuv_constants(matrix_out, range_out, matrix_out, range_out, din=dl, dl=dl, dout=dl if dout is None else dout,
                             chroma_n=1 << (ocsx + ocsy))


def source_rgb(pix_fmt: str, src):
    """(R, G, B) integer planes of a source: gbrp planes (G, B, R) or one packed image [H,W,C]; a fourth component is dropped."""
    if pix_fmt in PACKED:
        _bits, _nc, ro, go, bo = PACKED[pix_fmt]
        img = np.asarray(src)
        return img[..., ro], img[..., go], img[..., bo]
    g, b, r = src
    return r, g, b


def lut_rgb(table, scale, interp, pix_fmt, src, prelut=None):
    """lut3d on the source at its own depth: integer (R, G, B) at luma resolution."""
    dl = source_depth(pix_fmt)
    if pix_fmt in PACKED and prelut is None:
        _bits, _nc, ro, go, bo = PACKED[pix_fmt]
        out = orc.apply_packed(table, scale, pix_fmt, interp, np.asarray(src))
        return out[..., ro], out[..., go], out[..., bo]
    r, g, b = source_rgb(pix_fmt, src)          # (apply_packed is apply_rgb on the image's components; it has no prelut argument)
    go, bo, ro = orc.apply_rgb(table, scale, dl, interp, (g, b, r), prelut=prelut)
    return ro, go, bo


def apply(table, scale, interp, k, pix_fmt, dout, ocsx, ocsy, src, prelut=None, lut=True):
    """The contract: (Y, Cb, Cr) at the output depth and layout.  lut=False: the source codes go straight to the output stage."""
    rgb = lut_rgb(table, scale, interp, pix_fmt, src, prelut) if lut else source_rgb(pix_fmt, src)
    return rgb_codes_to_yuv(k, dout, ocsx, ocsy, rgb)


def apply_dither(table, scale, interp, k, pix_fmt, dout, ocsx, ocsy, src, prelut=None):
    """The contract with error-diffusion dither: the unquantised planes through the oracle's Floyd-Steinberg."""
    x = xs.unquantised(k, ocsx, ocsy, lut_rgb(table, scale, interp, pix_fmt, src, prelut))
    return [orc.dither_plane(p, float(k.max_o), dout > 8) for p in x]


def apply_full_range(table, scale, interp, pix_fmt, src, mid_layout, prologue_out_range, matrix, dout, out_layout, prelut=None):
    """3.9 point 6, a source flagged full range: RGB -> 8-bit YUV (`mid_layout`, range R, no LUT), then the YUV contract from
    that frame (range_src = range_in = R, lut_depth 8) to the output at range tv."""
    dl = source_depth(pix_fmt)
    m = matrix or "smpte170m"
    (mx, my), (ox, oy) = LAYOUTS[mid_layout], LAYOUTS[out_layout]
    mid = apply(None, None, None, consts(m, prologue_out_range, dl, 8, mx, my), pix_fmt, 8, mx, my, src, lut=False)
    k = orc.yuv_constants(m, prologue_out_range, m, "tv", 8, 8, dout, chroma_n=1 << (ox + oy))
    if (mx, my) == (ox, oy):
        return orc.apply_yuv(table, scale, interp, k, 8, 8, dout, ox, oy, mid, prelut=prelut)
    return xs.apply(table, scale, interp, k, 8, dout, mx, my, ox, oy, mid, prelut=prelut)
