"""Reference of the stage stack on RGB sources -- TEST INFRASTRUCTURE ONLY.

A composition of what exists, with no arithmetic of its own: the source's codes (`tests._rgb2yuv_twin.source_rgb`, a word above
M taken as M), then `tests._matrix_twin`'s list walk stage by stage -- `tests._lut1d_twin.lookup`, `tests._cdl_twin.table` /
`saturate` / `lattice_codes`, `tests._lut1d_twin.lut3d_codes`, `tests._matrix_twin.unit_of_codes` / `matrix_unit`,
`tests._stack_twin.round_codes` -- and either the codes themselves (a gbrp destination) or stage 3 of the YUV contract at the
output layout (`oracle.lut3d_numpy.rgb_codes_to_yuv` with `tests._rgb2yuv_twin.consts`).
"""
from __future__ import annotations

import numpy as np

from oracle.lut3d_numpy import rgb_codes_to_yuv
from tests import _cdl_twin as cdlt
from tests import _lut1d_twin as l1t
from tests import _matrix_twin as mxt
from tests import _rgb2yuv_twin as r2y
from tests import _stack_twin as skt

F = np.float32
LAYOUTS = r2y.LAYOUTS
consts = r2y.consts
source_depth = r2y.source_depth


def source_codes(pix_fmt, src, dl=None):
    """Integer (R, G, B) of a source as the list takes them: unsigned words, one above M = 2^dl - 1 taken as M."""
    dl = source_depth(pix_fmt) if dl is None else dl
    m = (1 << dl) - 1
    return tuple(np.minimum(np.asarray(v).astype(np.int64) & 0xffff, m) for v in r2y.source_rgb(pix_fmt, src))


def walk(stages, dl, codes, *, lut=None, prelut=None, lut2=None, l1d_tab=None, cdl=None, cdl_tab=None, mtx=None):
    """The list on integer (R, G, B) codes at depth dl: the final integer codes.  The resources are `tests._matrix_twin.rgb_out`'s."""
    px, unit = tuple(np.asarray(v).astype(np.int64) for v in codes), False
    for kind, mode in mxt.normalise(stages):
        if kind == "lut1d":
            if unit:
                px, unit = skt.round_codes(px, dl), False
            px = l1t.lookup(l1d_tab, px)
        elif kind == "cdl":
            if unit:
                px, unit = skt.round_codes(px, dl), False
            tab = cdlt.table(cdl, dl) if cdl_tab is None else np.asarray(cdl_tab, dtype=F)
            r, g, b = px
            px, unit = cdlt.saturate(cdl.saturation, [tab[0][r], tab[1][g], tab[2][b]]), True
        elif kind == "matrix":
            px, unit = mxt.matrix_unit(mtx, px if unit else mxt.unit_of_codes(px, dl)), True
        else:
            which = lut if kind == "lut3d" else lut2
            if unit:
                assert not (kind == "lut3d" and prelut is not None), "a prelut lattice directly behind cdl / matrix is refused"
                px, unit = cdlt.lattice_codes(which, mode, dl, px), False
            else:
                px = l1t.lut3d_codes(which, mode, dl, px, prelut if kind == "lut3d" else None)
    if unit:
        px = skt.round_codes(px, dl)
    return tuple(np.asarray(v).astype(np.int64) for v in px)


def apply_rgb(stages, pix_fmt, src, **res):
    """The contract into gbrp* at the source's depth: planes (G, B, R) of the final codes."""
    dl = source_depth(pix_fmt)
    r, g, b = walk(stages, dl, source_codes(pix_fmt, src), **res)
    dt = np.uint8 if dl <= 8 else np.uint16
    return g.astype(dt), b.astype(dt), r.astype(dt)


def apply_yuv(stages, k, pix_fmt, dout, ocsx, ocsy, src, **res):
    """The contract into planar YUV: (Y, Cb, Cr) at the output depth and layout; k = `consts(matrix_out, range_out, dl, dout, ocsx,
    ocsy)`."""
    dl = source_depth(pix_fmt)
    return rgb_codes_to_yuv(k, dout, ocsx, ocsy, walk(stages, dl, source_codes(pix_fmt, src), **res))
