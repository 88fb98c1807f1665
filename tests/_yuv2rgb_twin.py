"""Reference of the YUV source -> RGB output pass -- TEST INFRASTRUCTURE ONLY.

No new pixel arithmetic: the contract is a composition of existing oracle pieces.  Stage 1 of the YUV contract
(`oracle.lut3d_numpy.yuv_to_rgb_codes`: the optional prologue, chroma replicated over its input block, YUV -> integer RGB at the
LUT depth), then the C oracle's lut3d on that RGB at the LUT depth (`oracle.binding.apply_rgb`: every mode, the .csp prelut), and
the result arranged as the destination holds it: G, B, R planes, or a packed image whose fourth component is Ml.

The constants are the oracle's at din = dl; for a source of another depth (without a prologue) the input-side fields are
overwritten from the formula of the contract, evaluated here in float64 NumPy, independently of the library.
"""
from __future__ import annotations

import numpy as np

from oracle import binding as orc
from oracle.lut3d_numpy import yuv_to_rgb_codes
from tests import _xsub_twin as xs

LAYOUTS = xs.LAYOUTS
PACKED = orc.PACKED
KR_KB = {"bt709": (0.2126, 0.0722), "smpte170m": (0.299, 0.114), "bt2020nc": (0.2627, 0.0593)}
INPUT_FIELDS = ("ky", "yb", "coff", "krv", "kgu", "kgv", "kbu", "max_l")


def dest_depth(out_fmt: str) -> int:
    """The depth of an RGB destination: where lut3d runs."""
    if out_fmt in PACKED:
        return PACKED[out_fmt][0]
    d = out_fmt.replace("gbrap", "").replace("gbrp", "").replace("le", "")
    return int(d) if d else 8


def input_fields(matrix: str, rng: str, din: int, dl: int) -> dict:
    """The input-side entries of the contract's block for a source at `din` bits converted straight to RGB at `dl` bits: every
    entry formed in float64 and rounded once to float32."""
    kr, kb = (np.float64(v) for v in KR_KB[matrix])
    kg = np.float64(1.0) - kr - kb
    s = np.float64(1 << (din - 8))
    mi, ml = np.float64((1 << din) - 1), np.float64((1 << dl) - 1)
    if rng == "tv":
        ky, yoff, kc = ml / (np.float64(219.0) * s), np.float64(16.0) * s, ml / (np.float64(224.0) * s)
    else:
        ky, yoff, kc = ml / mi, np.float64(0.0), ml / mi
    two = np.float64(2.0)
    return {"ky": np.float32(ky), "yb": np.float32(-ky * yoff + np.float64(0.5)), "coff": np.float32(np.float64(128.0) * s),
            "krv": np.float32(two * (1.0 - kr) * kc), "kbu": np.float32(two * (1.0 - kb) * kc),
            "kgu": np.float32(-two * kb * (1.0 - kb) / kg * kc), "kgv": np.float32(-two * kr * (1.0 - kr) / kg * kc),
            "max_l": np.float32(ml)}


def consts(matrix="bt709", range_src="tv", range_in=None, din=10, dl=10):
    """The constant block of a call.  range_src != range_in: the oracle's prologue block, unchanged.  Otherwise the oracle's block
    at din = dl; for din != dl its input-side fields are overwritten from `input_fields`."""
    range_in = range_in or range_src
    if range_src != range_in:
        return orc.yuv_constants(matrix, range_in, matrix, range_in, din, dl, dl, chroma_n=1, prologue=True)
    k = orc.yuv_constants(matrix, range_in, matrix, range_in, din=dl, dl=dl, dout=dl, chroma_n=1)
    if din != dl:
        for name, v in input_fields(matrix, range_in, din, dl).items():
            setattr(k, name, float(v))
    return k


def rgb_codes(table, scale, interp, k, dl, icsx, icsy, planes, prelut=None, lut=True):
    """Integer (R, G, B) at luma resolution behind the LUT (lut=False: behind the YUV -> RGB stage)."""
    r, g, b = yuv_to_rgb_codes(k, icsx, icsy, planes)
    if not lut:
        return r, g, b
    dt = np.uint8 if dl <= 8 else np.uint16
    go, bo, ro = orc.apply_rgb(table, scale, dl, interp, (g.astype(dt), b.astype(dt), r.astype(dt)), prelut=prelut)
    return ro, go, bo


def arrange(out_fmt: str, rgb):
    """(R, G, B) as the destination `out_fmt` holds them: [G, B, R] planes (gbrap*: a fourth, opaque plane -- the caller replaces it
    when the source carries alpha), or one [H,W,C] image with A = Ml."""
    dl = dest_depth(out_fmt)
    dt = np.uint8 if dl <= 8 else np.uint16
    r, g, b = (np.asarray(a).astype(dt) for a in rgb)
    if out_fmt in PACKED:
        _bits, nc, ro, go, bo = PACKED[out_fmt]
        img = np.full(r.shape + (nc,), (1 << dl) - 1, dtype=dt)
        img[..., ro], img[..., go], img[..., bo] = r, g, b
        return img
    planes = [g, b, r]
    if out_fmt.startswith("gbrap"):
        planes.append(np.full(r.shape, (1 << dl) - 1, dtype=dt))
    return planes


def apply(table, scale, interp, out_fmt, din, icsx, icsy, planes, matrix="bt709", range_src="tv", range_in=None, prelut=None,
          lut=True):
    """The contract: the destination `out_fmt` of the source `planes` (Y, Cb, Cr at `din` bits, layout icsx / icsy)."""
    dl = dest_depth(out_fmt)
    k = consts(matrix, range_src, range_in, din, dl)
    return arrange(out_fmt, rgb_codes(table, scale, interp, k, dl, icsx, icsy, planes, prelut=prelut, lut=lut))
