"""NumPy twin of the sited chroma contract -- TEST INFRASTRUCTURE ONLY.

Stage 1 (chroma up-sampling, then YUV -> integer RGB) and stage 3 (integer RGB -> YUV with the sited chroma
down-sampling) are written out here; the lut3d stage between them is the C oracle's (`oracle.binding.apply_rgb`, every
interpolation mode and the .csp prelut) and the constants are the oracle's (`oracle.binding.yuv_constants` at 4:4:4, scaled
by the down-sampling's 1/n).  The fp32 helpers come from `oracle.lut3d_numpy`.
"""
from __future__ import annotations

import numpy as np

from oracle import binding as orc
from oracle.lut3d_numpy import _clip_floor, _fma

F = np.float32
LOCS = ("left", "center", "topleft")
#: (horizontally co-sited, vertically co-sited) of each siting
COSITED = {"left": (True, False), "center": (False, False), "topleft": (True, True)}


def up_taps(n_luma: int, n_chroma: int, subsampled: bool, cosited: bool):
    """Up-sampling taps of one axis: [(chroma index array, weight array)] per luma index; weights sum to 4 (or 1)."""
    x = np.arange(n_luma)
    if not subsampled:
        return [(x, np.ones(n_luma, np.int64))]
    k = x >> 1
    odd = (x & 1).astype(bool)
    kp, km = np.minimum(k + 1, n_chroma - 1), np.maximum(k - 1, 0)
    if cosited:           # even 2k: 4 C[k]; odd 2k+1: 2 C[k] + 2 C[k+1]
        return [(k, np.where(odd, 2, 4)), (kp, np.where(odd, 2, 0))]
    # interstitial: even 1 C[k-1] + 3 C[k]; odd 3 C[k] + 1 C[k+1]
    return [(np.where(odd, k, km), np.where(odd, 3, 1)), (np.where(odd, kp, k), np.where(odd, 1, 3))]


def down_taps(n_chroma: int, n_luma: int, subsampled: bool, cosited: bool):
    """Down-sampling taps of one axis: [(luma index array, weight)] per chroma index, and their sum."""
    i = np.arange(n_chroma)
    if not subsampled:
        return [(i, 1)], 1
    clamp = lambda v: np.clip(v, 0, n_luma - 1)  # noqa: E731
    if cosited:
        return [(clamp(2 * i - 1), 1), (clamp(2 * i), 2), (clamp(2 * i + 1), 1)], 4
    return [(clamp(2 * i), 1), (clamp(2 * i + 1), 1)], 2


def down_n(loc: str, csx: int, csy: int) -> int:
    cx, cy = COSITED[loc]
    return (1 if not csx else 4 if cx else 2) * (1 if not csy else 4 if cy else 2)


def upsample(plane, h: int, w: int, csx: int, csy: int, loc: str):
    """Integer weighted sums S of a chroma plane at every luma pixel, and Wsum."""
    cx, cy = COSITED[loc]
    c = np.asarray(plane, dtype=np.int64)
    ch, cw = c.shape
    ty, tx = up_taps(h, ch, bool(csy), cy), up_taps(w, cw, bool(csx), cx)
    s = np.zeros((h, w), np.int64)
    for iy, wy in ty:
        for ix, wx in tx:
            s += wy[:, None] * wx[None, :] * c[iy[:, None], ix[None, :]]
    return s, (4 if csx else 1) * (4 if csy else 1)


def downsample(plane, csx: int, csy: int, loc: str):
    """Integer weighted sums of a luma-resolution plane at every chroma sample (1/n is in the constants)."""
    cx, cy = COSITED[loc]
    a = np.asarray(plane, dtype=np.int64)
    h, w = a.shape
    ch, cw = (h + (1 << csy) - 1) >> csy, (w + (1 << csx) - 1) >> csx
    ty, _ = down_taps(ch, h, bool(csy), cy)
    tx, _ = down_taps(cw, w, bool(csx), cx)
    s = np.zeros((ch, cw), np.int64)
    for iy, wy in ty:
        for ix, wx in tx:
            s += wy * wx * a[iy[:, None], ix[None, :]]
    return s


def consts(matrix_in, range_in, matrix_out, range_out, din, dl, dout, csx, csy, loc, prologue=False):
    """The oracle's constant block with the down-sampling's 1/n folded in (4:4:4 / replicate: the plain block)."""
    if loc is None or not (csx or csy):
        return orc.yuv_constants(matrix_in, range_in, matrix_out, range_out, din, dl, dout, 1 << (csx + csy), prologue=prologue)
    # the oracle divides by chroma_n in double for n <= 4; n is a power of two, so scaling its 4:4:4 floats by 1/n is the
    # same rounding for n = 8 and 16 too
    k = orc.yuv_constants(matrix_in, range_in, matrix_out, range_out, din, dl, dout, 1, prologue=prologue)
    inv = F(1.0 / down_n(loc, csx, csy))
    for name in ("cbr", "cbg", "cbb", "crr", "crg", "crb"):
        setattr(k, name, float(F(getattr(k, name)) * inv))
    return k


def stage1(k, csx: int, csy: int, loc: str, planes):
    """YUV codes -> integer RGB at the LUT depth: C' per chroma sample, sited up-sampling, then today's chroma terms."""
    y, cb, cr = [np.asarray(p).astype(F) for p in planes]
    h, w = y.shape
    if k.pre:
        y = _clip_floor(_fma(F(k.py), y, F(k.pyb)), k.pre_max)
        cb = _clip_floor(_fma(F(k.pc), cb, F(k.pcb)), k.pre_max)
        cr = _clip_floor(_fma(F(k.pc), cr, F(k.pcb)), k.pre_max)
    sb, wsum = upsample(cb.astype(np.int64), h, w, csx, csy, loc)
    sr, _ = upsample(cr.astype(np.int64), h, w, csx, csy, loc)
    inv = F(1.0 / wsum)
    cbd = ((sb.astype(F) * inv).astype(F) - F(k.coff)).astype(F)
    crd = ((sr.astype(F) * inv).astype(F) - F(k.coff)).astype(F)
    rv = (F(k.krv) * crd).astype(F)
    gv = _fma(F(k.kgu), cbd, (F(k.kgv) * crd).astype(F))
    bu = (F(k.kbu) * cbd).astype(F)
    yy = _fma(F(k.ky), y, F(k.yb))
    rq = _clip_floor((yy + rv).astype(F), k.max_l)
    gq = _clip_floor((yy + gv).astype(F), k.max_l)
    bq = _clip_floor((yy + bu).astype(F), k.max_l)
    return rq.astype(np.int64), gq.astype(np.int64), bq.astype(np.int64)


def stage3(k, dout: int, csx: int, csy: int, loc: str, rgb):
    """Integer RGB -> YUV at the output depth: Y per pixel as today, chroma from the sited weighted sums."""
    ro, go, bo = [np.asarray(a).astype(F) for a in rgb]
    yo = _clip_floor(_fma(F(k.cyr), ro, _fma(F(k.cyg), go, _fma(F(k.cyb), bo, F(k.yob)))), k.max_o)
    rs, gs, bs = [downsample(np.asarray(a, dtype=np.int64), csx, csy, loc).astype(F) for a in rgb]
    cbo = _clip_floor(_fma(F(k.cbr), rs, _fma(F(k.cbg), gs, _fma(F(k.cbb), bs, F(k.cob)))), k.max_o)
    cro = _clip_floor(_fma(F(k.crr), rs, _fma(F(k.crg), gs, _fma(F(k.crb), bs, F(k.cob)))), k.max_o)
    odt = np.uint8 if dout <= 8 else np.uint16
    return [yo.astype(odt), cbo.astype(odt), cro.astype(odt)]


def apply_yuv(table, scale, mode, k, din, dl, dout, csx, csy, loc, planes, prelut=None):
    """One frame (Y, Cb, Cr) through the sited contract; `k` from `consts(...)` for the same loc.  loc None or 4:4:4:
    the oracle's replicate contract."""
    if loc is None or not (csx or csy):
        return orc.apply_yuv(table, scale, mode, k, din, dl, dout, csx, csy, planes, prelut=prelut)
    rq, gq, bq = stage1(k, csx, csy, loc, planes)
    ldt = np.uint8 if dl <= 8 else np.uint16
    g, b, r = orc.apply_rgb(table, scale, dl, mode, (gq.astype(ldt), bq.astype(ldt), rq.astype(ldt)), prelut=prelut)
    return stage3(k, dout, csx, csy, loc, (r, g, b))
