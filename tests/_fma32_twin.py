"""NumPy twin of the FMA32 precision (include/lutr.h LUTR_PRECISION_FMA32, csrc/lutr_tile2.hip V_FMA32).

Everything but the lut3d blend is strict's and comes from oracle/lut3d_numpy.py: the YUV -> RGB stage, the RGB -> YUV stage
and the coordinate arithmetic.  The blend reads nodes pre-multiplied by M = 2^depth - 1 in fp32 (one rounding each) and
rounds once per step:
  tetrahedral  fma(w3, c111, fma(w2, cB, fma(w1, cA, w0 * c000)))   in FFmpeg's branch form (a zero-weight tap adds an
               exact +0, so the kernels' sorted form gives the same bits)
  trilinear    fma(v1 - v0, f, v0) for each of FFmpeg's seven lerps
  nearest      the node times M: identical to strict
then truncation, as strict.
"""
from __future__ import annotations

import numpy as np

from oracle.lut3d_numpy import _fma, rgb_codes_to_yuv, yuv_to_rgb_codes

F = np.float32


def fma(a, b, c):
    """fp32 fused multiply-add: a * b + c with one rounding."""
    return _fma(a, b, c)


def premultiplied(table, depth):
    """The fma32 lattice: every node times 2^depth - 1, one fp32 rounding (lutr_lat16.hip k_make_latm)."""
    return (np.asarray(table, dtype=F) * F((1 << depth) - 1)).astype(F)


def _blend(tm, mode, s):
    n = tm.shape[0]
    sr, sg, sb = s
    if mode == "nearest":
        i = [(v.astype(np.float64) + 0.5).astype(np.int32) for v in (sr, sg, sb)]
        return tm[i[0], i[1], i[2]]
    p = [v.astype(np.int32) for v in (sr, sg, sb)]
    x = [np.minimum(v + 1, n - 1) for v in p]
    d = [(v - q.astype(F)).astype(F) for v, q in zip((sr, sg, sb), p)]

    def c(i, j, k):
        return tm[(x[0] if i else p[0]), (x[1] if j else p[1]), (x[2] if k else p[2])]

    if mode == "trilinear":
        def lerp(a, b, f):
            return fma((b - a).astype(F), f[..., None], a)
        c00, c10 = lerp(c(0, 0, 0), c(1, 0, 0), d[0]), lerp(c(0, 1, 0), c(1, 1, 0), d[0])
        c01, c11 = lerp(c(0, 0, 1), c(1, 0, 1), d[0]), lerp(c(0, 1, 1), c(1, 1, 1), d[0])
        return lerp(lerp(c00, c10, d[1]), lerp(c01, c11, d[1]), d[2])
    if mode != "tetrahedral":
        raise ValueError(mode)
    dr, dg, db = d
    one = F(1)

    def blend(w0, w1, v1, w2, v2, w3):
        w = [np.asarray(q, dtype=F)[..., None] for q in (w0, w1, w2, w3)]
        acc = (w[0] * c(0, 0, 0)).astype(F)
        return fma(w[3], c(1, 1, 1), fma(w[2], v2, fma(w[1], v1, acc)))

    cases = [
        ((dr > dg) & (dg > db), lambda: blend(one - dr, dr - dg, c(1, 0, 0), dg - db, c(1, 1, 0), db)),
        ((dr > dg) & ~(dg > db) & (dr > db), lambda: blend(one - dr, dr - db, c(1, 0, 0), db - dg, c(1, 0, 1), dg)),
        ((dr > dg) & ~(dg > db) & ~(dr > db), lambda: blend(one - db, db - dr, c(0, 0, 1), dr - dg, c(1, 0, 1), dg)),
        (~(dr > dg) & (db > dg), lambda: blend(one - db, db - dg, c(0, 0, 1), dg - dr, c(0, 1, 1), dr)),
        (~(dr > dg) & ~(db > dg) & (db > dr), lambda: blend(one - dg, dg - db, c(0, 1, 0), db - dr, c(0, 1, 1), dr)),
        (~(dr > dg) & ~(db > dg) & ~(db > dr), lambda: blend(one - dg, dg - dr, c(0, 1, 0), dr - db, c(1, 1, 0), db)),
    ]
    out = np.zeros(dr.shape + (3,), dtype=F)
    for m, v in cases:
        out[m] = v()[m]
    return out


def lut3d_codes(table, scale, depth, mode, r, g, b):
    """lut3d on integer code arrays under fma32; returns integer code arrays (r, g, b)."""
    n = table.shape[0]
    m = (1 << depth) - 1
    scale_f = F(1.0) / F(m)
    lut_max = F(n - 1)
    s = []
    for v, sc in zip((r, g, b), scale):
        x = (v.astype(F) * scale_f).astype(F)
        s.append(np.clip((x * (F(sc) * lut_max)).astype(F), F(0), lut_max).astype(F))
    v = _blend(premultiplied(table, depth), mode, s)
    q = np.clip(np.trunc(v.astype(np.float64)), 0, m).astype(np.int64)
    return q[..., 0], q[..., 1], q[..., 2]


def apply_yuv(table, scale, mode, k, din, dl, dout, csx, csy, planes):
    """The fused YUV path under fma32; arguments as oracle.binding.apply_yuv (k: its YuvConsts)."""
    rq, gq, bq = yuv_to_rgb_codes(k, csx, csy, planes)
    return rgb_codes_to_yuv(k, dout, csx, csy, lut3d_codes(table, np.asarray(scale, dtype=F), dl, mode, rq, gq, bq))
