"""Reference of the stage stack with an RGB matrix stage -- TEST INFRASTRUCTURE ONLY.

`tests._stack_twin`'s list walk with one more kind, `matrix`, in NumPy float32 with one operation per statement (`matrix_unit`);
everything else is what that twin composes: stage 1 and stage 3 of the YUV contract, `tests._lut1d_twin.lookup`,
`tests._cdl_twin`'s table lookup, `saturate` and `lattice_codes`, `tests._lut1d_twin.lut3d_codes` and
`tests._stack_twin.round_codes`.  A pixel is codes or unit floats; the matrix takes either and gives unit floats, and a unit
pixel is rounded to codes ahead of lut1d, ahead of cdl (whose table is per code) and at the end of the list.
"""
from __future__ import annotations

import numpy as np

from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
from tests import _cdl_twin as cdlt
from tests import _lut1d_twin as l1t
from tests import _stack_twin as skt

F = np.float32
LAYOUTS = skt.LAYOUTS
consts = skt.consts
round_codes = skt.round_codes
KINDS = skt.KINDS + ("matrix",)


def normalise(stages):
    """((kind, mode), ...) from names and (name, mode) pairs; a lut3d stage without a mode is tetrahedral."""
    out = []
    for s in stages:
        kind, mode = (s, None) if isinstance(s, str) else s
        assert kind in KINDS, kind
        out.append((kind, (mode or "tetrahedral") if kind in ("lut3d", "lut3d2") else None))
    return out


def unit_of_codes(px, dl):
    """u_c = fl(q_c * fl(1 / M)): the float the identity CDL's table holds for code q_c."""
    rcp = F(1.0) / F((1 << dl) - 1)
    return [(np.asarray(v).astype(F) * rcp).astype(F) for v in px]


def matrix_unit(mtx, u):
    """The matrix line on unit floats (u_r, u_g, u_b): per row two products summed, the third product added, the offset added, every
    one of them rounded to float32 on its own; then the clamp to [0, 1].  `mtx`: anything with .m (nine, row-major) and .offset."""
    ur, ug, ub = (np.asarray(v, dtype=F) for v in u)
    out = []
    for row in range(3):
        m0, m1, m2, off = F(mtx.m[3 * row]), F(mtx.m[3 * row + 1]), F(mtx.m[3 * row + 2]), F(mtx.offset[row])
        p0 = (m0 * ur).astype(F)
        p1 = (m1 * ug).astype(F)
        p2 = (m2 * ub).astype(F)
        s01 = (p0 + p1).astype(F)
        s012 = (s01 + p2).astype(F)
        t = (s012 + off).astype(F)
        lo = np.maximum(t, F(0))
        out.append(np.minimum(lo, F(1)).astype(F))
    return out


def rgb_out(stages, k, dl, icsx, icsy, planes, *, lut=None, prelut=None, lut2=None, l1d_tab=None, cdl=None, cdl_tab=None, mtx=None):
    """Stage 1 and the stack: integer (R, G, B) at luma resolution, as stage 3 takes them.  The resources are
    `tests._stack_twin.rgb_out`'s, and `mtx` the matrix of a matrix stage."""
    px, unit = yuv_to_rgb_codes(k, icsx, icsy, planes), False
    for kind, mode in normalise(stages):
        if kind == "lut1d":
            if unit:
                px, unit = round_codes(px, dl), False
            px = l1t.lookup(l1d_tab, px)
        elif kind == "cdl":
            if unit:
                px, unit = round_codes(px, dl), False
            tab = cdlt.table(cdl, dl) if cdl_tab is None else np.asarray(cdl_tab, dtype=F)
            r, g, b = px
            px, unit = cdlt.saturate(cdl.saturation, [tab[0][r], tab[1][g], tab[2][b]]), True
        elif kind == "matrix":
            px, unit = matrix_unit(mtx, px if unit else unit_of_codes(px, dl)), True
        else:
            which = lut if kind == "lut3d" else lut2
            if unit:
                assert not (kind == "lut3d" and prelut is not None), "a prelut lattice directly behind cdl / matrix is refused"
                px, unit = cdlt.lattice_codes(which, mode, dl, px), False
            else:
                px = l1t.lut3d_codes(which, mode, dl, px, prelut if kind == "lut3d" else None)
    if unit:
        px = round_codes(px, dl)
    return tuple(np.asarray(v).astype(np.int64) for v in px)


def apply(stages, k, dl, dout, icsx, icsy, ocsx, ocsy, planes, **res):
    """The contract: (Y, Cb, Cr) at the output depth and layout."""
    return rgb_codes_to_yuv(k, dout, ocsx, ocsy, rgb_out(stages, k, dl, icsx, icsy, planes, **res))
