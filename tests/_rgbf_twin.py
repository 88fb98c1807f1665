"""Reference of the planar float RGB paths -- TEST INFRASTRUCTURE ONLY.

A composition of what exists: `sanitize` on the bit pattern and `prelut` (FFmpeg's prelut_interp_1d_linear) restated in NumPy,
`oracle.lut3d_numpy._interp` for the lattice (it takes float coordinates for nearest, trilinear and tetrahedral), `np.rint` for the
quantiser, `oracle.lut3d_numpy.rgb_codes_to_yuv` with the oracle's constants at lut_depth 16 for the output side, and
`oracle.binding.dither_plane` for error diffusion.  tests/test_rgbf.py pins it to the C oracle through code-valued floats:
the float frame fl(code * fl(1 / M)) through `apply_float`, then `to_codes`, is `oracle.binding.apply_rgb` on the codes -- which
is also how the GPU's pyramid and prism are checked (`_interp` has no such modes).
"""
from __future__ import annotations

import numpy as np

from lut_renderer_amd import frames
from oracle import binding as orc
from oracle.lut3d_numpy import _interp, rgb_codes_to_yuv
from tests import _xsub_twin as xs

F = np.float32
FLT_MAX = np.finfo(np.float32).max
LAYOUTS = xs.LAYOUTS


def sanitize(a):
    """vf_lut3d.c's sanitizef on the bits: NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX, everything else unchanged."""
    a = np.ascontiguousarray(a, dtype=F)
    bits = a.view(np.uint32)
    special = (bits & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
    nan = special & ((bits & np.uint32(0x007fffff)) != 0)
    neg = (bits & np.uint32(0x80000000)) != 0
    out = a.copy()
    out[special & ~nan & ~neg] = FLT_MAX
    out[special & ~nan & neg] = -FLT_MAX
    out[nan] = F(0)
    return out


def prelut(pre, c, x):
    """FFmpeg's prelut_interp_1d_linear on channel c: every operation rounds to float32."""
    size = pre.table.shape[1]
    with np.errstate(over="ignore", invalid="ignore"):
        t = np.clip(((x - F(pre.min[c])).astype(F) * F(pre.scale[c])).astype(F), F(0), F(size - 1))
    i = t.astype(np.int32)
    j = np.minimum(i + 1, size - 1)
    tab = np.asarray(pre.table[c], dtype=F)
    p, n = tab[i], tab[j]
    return (p + ((n - p).astype(F) * (t - i.astype(F)).astype(F)).astype(F)).astype(F)


def lattice_rgb(table, scale, interp, src, prelut_=None):
    """The float-to-float contract on gbrp-ordered float planes (G, B, R): float32 (R, G, B) as the lattice gives them."""
    table = np.asarray(table, dtype=F)
    g, b, r = src
    lut_max = F(table.shape[0] - 1)
    s = []
    for c, (v, sc) in enumerate(zip((r, g, b), scale)):
        x = sanitize(v)
        if prelut_ is not None:
            x = prelut(prelut_, c, x)
        with np.errstate(over="ignore"):
            s.append(np.clip((x * (F(sc) * lut_max)).astype(F), F(0), lut_max).astype(F))
    v = _interp(table, interp, s)
    return v[..., 0], v[..., 1], v[..., 2]


def apply_float(table, scale, interp, src, prelut=None):
    """gbrpf32le in, gbrpf32le out: (G, B, R) float32 planes, nothing clipped."""
    r, g, b = lattice_rgb(table, scale, interp, src, prelut)
    return [np.ascontiguousarray(p, dtype=F) for p in (g, b, r)]


def quantise(v):
    """swscale's planar-float reader: clip(rintf(v * 65535), 0, 65535), round half to even (held as float32)."""
    with np.errstate(over="ignore"):
        return np.clip(np.rint((np.asarray(v, dtype=F) * F(65535)).astype(F)), F(0), F(65535)).astype(F)


def consts(matrix_out="smpte170m", range_out="tv", dout=10, ocsx=1, ocsy=1):
    """The oracle's constant block at lut_depth 16 with the output block's n (only its output side is used)."""
    return orc.yuv_constants(matrix_out, range_out, matrix_out, range_out, din=16, dl=16, dout=dout, chroma_n=1 << (ocsx + ocsy))


def codes_rgb(table, scale, interp, src, prelut=None, lut=True):
    """The 16-bit codes (R, G, B) the output stage sees.  lut=False: sanitise and quantise only."""
    if lut:
        rgb = lattice_rgb(table, scale, interp, src, prelut)
    else:
        g, b, r = src
        rgb = [sanitize(p) for p in (r, g, b)]
    return [quantise(p) for p in rgb]


def apply_yuv(table, scale, interp, k, dout, ocsx, ocsy, src, prelut=None, lut=True):
    """gbrpf32le in, planar YUV out: (Y, Cb, Cr) at the output depth and layout."""
    return rgb_codes_to_yuv(k, dout, ocsx, ocsy, codes_rgb(table, scale, interp, src, prelut, lut))


def apply_dither(table, scale, interp, k, dout, ocsx, ocsy, src, prelut=None):
    x = xs.unquantised(k, ocsx, ocsy, codes_rgb(table, scale, interp, src, prelut))
    return [orc.dither_plane(p, float(k.max_o), dout > 8) for p in x]


def apply_full_range(table, scale, interp, src, mid_layout, prologue_out_range, matrix, dout, out_layout, prelut=None):
    """A float source flagged full range (3.9 point 6): float -> 8-bit YUV without the LUT, then the YUV contract from that frame."""
    m = matrix or "smpte170m"
    (mx, my), (ox, oy) = LAYOUTS[mid_layout], LAYOUTS[out_layout]
    mid = apply_yuv(None, None, None, consts(m, prologue_out_range, 8, mx, my), 8, mx, my, src, lut=False)
    k = orc.yuv_constants(m, prologue_out_range, m, "tv", 8, 8, dout, chroma_n=1 << (ox + oy))
    if (mx, my) == (ox, oy):
        return orc.apply_yuv(table, scale, interp, k, 8, 8, dout, ox, oy, mid, prelut=prelut)
    return xs.apply(table, scale, interp, k, 8, dout, mx, my, ox, oy, mid, prelut=prelut)


# ------------------------------------------------------------------ code-valued floats (the link to the C oracle)
def code_frame(planes, depth):
    """Integer planes at `depth` as the floats lut3d's integer path makes of them: fl(code * fl(1 / M))."""
    m = F((1 << depth) - 1)
    return [(np.asarray(p).astype(F) * (F(1.0) / m)).astype(F) for p in planes]


def to_codes(planes, depth):
    """lut3d's integer store on float planes: clip(trunc(fl(v * M)), 0, M)."""
    m = (1 << depth) - 1
    dt = np.uint8 if depth <= 8 else np.uint16
    return [np.clip(np.trunc((np.asarray(p, dtype=F) * F(m)).astype(F).astype(np.float64)), 0, m).astype(dt) for p in planes]


# ------------------------------------------------------------------ sources
def make_float(dist, w, h, k=0):
    """A gbrpf32le frame (G, B, R): "natural" / "uniform" in [0, 1] off the code grid, "hdr" uniform in [-0.5, 8], "nonfinite" a
    natural frame seeded with NaN (both signs, several payloads), +inf and -inf."""
    rng = np.random.default_rng(4000 + k)
    if dist == "hdr":
        return [rng.uniform(-0.5, 8.0, size=(h, w)).astype(F) for _ in range(3)]
    base = frames.make_rgb("natural" if dist == "nonfinite" else dist, w, h, 16, k=k)
    out = [((p.astype(np.float64) + rng.uniform(-0.5, 0.5, size=p.shape)) / 65535.0).astype(F) for p in base]
    if dist == "nonfinite":
        specials = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff812345, 0x7f800000, 0xff800000], np.uint32).view(F)
        for p in out:
            idx = rng.choice(p.size, size=max(6, p.size // 16), replace=False)
            p.reshape(-1)[idx] = specials[rng.integers(0, len(specials), size=idx.size)]
    return out
