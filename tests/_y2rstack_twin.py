"""Reference of the stage stack from YUV sources into RGB frames -- TEST INFRASTRUCTURE ONLY.

A composition of what exists, with no arithmetic of its own: the constant block of the YUV -> RGB pass
(`tests._yuv2rgb_twin.consts`), stage 1 of the YUV contract and the list walk (`tests._matrix_twin.rgb_out`: chroma replicated
over its input block, YUV -> integer RGB at the destination's depth, then the list stage by stage), and the final codes arranged
as the destination holds them (`tests._yuv2rgb_twin.arrange`: G, B, R planes, or a packed image whose fourth component is Ml).
"""
from __future__ import annotations

from tests import _matrix_twin as mxt
from tests import _yuv2rgb_twin as y2r

LAYOUTS = y2r.LAYOUTS
PACKED = y2r.PACKED
dest_depth = y2r.dest_depth
consts = y2r.consts
arrange = y2r.arrange


def rgb_codes(stages, out_fmt, din, icsx, icsy, planes, matrix="bt709", range_src="tv", range_in=None, **res):
    """Integer (R, G, B) at luma resolution behind the list; the resources are `tests._matrix_twin.rgb_out`'s."""
    dl = dest_depth(out_fmt)
    k = consts(matrix, range_src, range_in, din, dl)
    return mxt.rgb_out(stages, k, dl, icsx, icsy, planes, **res)


def apply(stages, out_fmt, din, icsx, icsy, planes, matrix="bt709", range_src="tv", range_in=None, **res):
    """The contract: the destination `out_fmt` of the source `planes` (Y, Cb, Cr at `din` bits, layout icsx / icsy)."""
    return arrange(out_fmt, rgb_codes(stages, out_fmt, din, icsx, icsy, planes, matrix, range_src, range_in, **res))
