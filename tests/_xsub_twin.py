"""Reference of the chroma subsampling change -- TEST INFRASTRUCTURE ONLY.

The contract is a composition of existing pieces: stage 1 of the YUV contract at the INPUT layout
(`oracle.lut3d_numpy.yuv_to_rgb_codes`: chroma replicated over its input block), the C oracle's lut3d on the integer RGB
(`oracle.binding.apply_rgb`: every interpolation mode and the .csp prelut), and stage 3 at the OUTPUT layout
(`oracle.lut3d_numpy.rgb_codes_to_yuv`: block mean over the output block, a partial block padded with its edge), with the
oracle's constants at the output block's n (`oracle.binding.yuv_constants(chroma_n=...)`).
"""
from __future__ import annotations

import numpy as np

from oracle import binding as orc
from oracle.lut3d_numpy import _fma, rgb_codes_to_yuv, yuv_to_rgb_codes

F = np.float32
#: (csx, csy) of the layouts the engine takes on either side
LAYOUTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
#: the six ordered pairs of different layouts
CROSS_PAIRS = [(a, b) for a in LAYOUTS for b in LAYOUTS if a != b]


def consts(matrix_in="bt709", range_in="tv", matrix_out=None, range_out="tv", din=10, dl=None, dout=None, ocsx=1, ocsy=1,
           prologue=False):
    """The oracle's constant block with the OUTPUT block's n = 2^(ocsx + ocsy)."""
    return orc.yuv_constants(matrix_in, range_in, matrix_out, range_out, din, dl, dout, chroma_n=1 << (ocsx + ocsy),
                             prologue=prologue)


def lut_rgb(table, scale, interp, k, dl, icsx, icsy, planes, prelut=None):
    """Stages 1 and 2: integer (R, G, B) at luma resolution after lut3d."""
    r, g, b = yuv_to_rgb_codes(k, icsx, icsy, planes)
    dt = np.uint8 if dl <= 8 else np.uint16
    go, bo, ro = orc.apply_rgb(table, scale, dl, interp, (g.astype(dt), b.astype(dt), r.astype(dt)), prelut=prelut)
    return ro, go, bo


def apply(table, scale, interp, k, dl, dout, icsx, icsy, ocsx, ocsy, planes, prelut=None):
    """The contract: (Y, Cb, Cr) at the output depth and layout."""
    return rgb_codes_to_yuv(k, dout, ocsx, ocsy, lut_rgb(table, scale, interp, k, dl, icsx, icsy, planes, prelut))


def unquantised(k, ocsx, ocsy, rgb):
    """Stage 3 without its rounding (lutr_dither.hip's pass 1: the fma chain, then - 0.5), as float32 planes."""
    ro, go, bo = [np.asarray(a).astype(F) for a in rgb]
    h, w = ro.shape
    y = (_fma(F(k.cyr), ro, _fma(F(k.cyg), go, _fma(F(k.cyb), bo, F(k.yob)))) - F(0.5)).astype(F)
    bh, bw = 1 << ocsy, 1 << ocsx
    ch, cw = (h + bh - 1) >> ocsy, (w + bw - 1) >> ocsx

    def block_sum(a):
        pad = np.pad(a, ((0, ch * bh - h), (0, cw * bw - w)), mode="edge")
        return pad.reshape(ch, bh, cw, bw).sum(axis=(1, 3)).astype(F)

    rs, gs, bs = block_sum(ro), block_sum(go), block_sum(bo)
    cb = (_fma(F(k.cbr), rs, _fma(F(k.cbg), gs, _fma(F(k.cbb), bs, F(k.cob)))) - F(0.5)).astype(F)
    cr = (_fma(F(k.crr), rs, _fma(F(k.crg), gs, _fma(F(k.crb), bs, F(k.cob)))) - F(0.5)).astype(F)
    return y, cb, cr


def apply_dither(table, scale, interp, k, dl, dout, icsx, icsy, ocsx, ocsy, planes, prelut=None):
    """The contract with error-diffusion dither: the unquantised planes through the oracle's Floyd-Steinberg."""
    x = unquantised(k, ocsx, ocsy, lut_rgb(table, scale, interp, k, dl, icsx, icsy, planes, prelut))
    return [orc.dither_plane(p, float(k.max_o), dout > 8) for p in x]
