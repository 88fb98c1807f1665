"""Reference of the stage-stack pass -- TEST INFRASTRUCTURE ONLY.

A composition of what exists plus the one line of the unit -> codes rounding: stage 1 of the YUV contract at the INPUT layout
(`oracle.lut3d_numpy.yuv_to_rgb_codes`), then per stage `tests._lut1d_twin.lookup` (lut1d), `tests._cdl_twin` stage A's table
lookup and `saturate` (cdl), `tests._cdl_twin.lattice_codes` (a lattice fed unit floats) or `tests._lut1d_twin.lut3d_codes` (a
lattice fed codes: the C oracle's lut3d, every mode and the first LUT's prelut), `round_codes` where a unit pixel meets lut1d or
the end of the list, and stage 3 at the OUTPUT layout (`oracle.lut3d_numpy.rgb_codes_to_yuv` with `tests._xsub_twin.consts`).
"""
from __future__ import annotations

import numpy as np

from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
from tests import _cdl_twin as cdlt
from tests import _lut1d_twin as l1t
from tests import _xsub_twin as xs

F = np.float32
LAYOUTS = xs.LAYOUTS
consts = xs.consts
KINDS = ("lut3d", "lut3d2", "lut1d", "cdl")


def round_codes(unit, dl):
    """unit -> codes: q_c = (int)(fl(fl(o_c * (float)M) + 0.5f)), the product and the sum each rounded to float32."""
    m = F((1 << dl) - 1)
    return tuple(((np.asarray(v, dtype=F) * m).astype(F) + F(0.5)).astype(F).astype(np.int64) for v in unit)


def normalise(stages):
    """((kind, mode), ...) from names and (name, mode) pairs; a lut3d stage without a mode is tetrahedral."""
    out = []
    for s in stages:
        kind, mode = (s, None) if isinstance(s, str) else s
        assert kind in KINDS, kind
        out.append((kind, (mode or "tetrahedral") if kind in ("lut3d", "lut3d2") else None))
    return out


def rgb_out(stages, k, dl, icsx, icsy, planes, *, lut=None, prelut=None, lut2=None, l1d_tab=None, cdl=None, cdl_tab=None):
    """Stage 1 and the stack: integer (R, G, B) at luma resolution, as stage 3 takes them.  lut / lut2: anything with .table and
    .scale; prelut: the first LUT's oracle prelut; l1d_tab: uint16 [3, 2^dl]; cdl: a `cdl.Cdl`, cdl_tab: its stage A table (None:
    `tests._cdl_twin.table`)."""
    px, unit = yuv_to_rgb_codes(k, icsx, icsy, planes), False
    for kind, mode in normalise(stages):
        if kind == "lut1d":
            if unit:
                px, unit = round_codes(px, dl), False
            px = l1t.lookup(l1d_tab, px)
        elif kind == "cdl":
            assert not unit
            tab = cdlt.table(cdl, dl) if cdl_tab is None else np.asarray(cdl_tab, dtype=F)
            r, g, b = px
            px, unit = cdlt.saturate(cdl.saturation, [tab[0][r], tab[1][g], tab[2][b]]), True
        else:
            which = lut if kind == "lut3d" else lut2
            if unit:
                assert not (kind == "lut3d" and prelut is not None), "a prelut lattice directly behind the CDL is refused"
                px, unit = cdlt.lattice_codes(which, mode, dl, px), False
            else:
                px = l1t.lut3d_codes(which, mode, dl, px, prelut if kind == "lut3d" else None)
    if unit:
        px = round_codes(px, dl)
    return tuple(np.asarray(v).astype(np.int64) for v in px)


def apply(stages, k, dl, dout, icsx, icsy, ocsx, ocsy, planes, **res):
    """The contract: (Y, Cb, Cr) at the output depth and layout."""
    return rgb_codes_to_yuv(k, dout, ocsx, ocsy, rgb_out(stages, k, dl, icsx, icsy, planes, **res))
