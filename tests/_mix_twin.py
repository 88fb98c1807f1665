"""Reference of the stage stack with a strength behind it -- TEST INFRASTRUCTURE ONLY.

`tests._stack_twin.rgb_out` gives q1, `oracle.lut3d_numpy.yuv_to_rgb_codes` gives q0, then the three fp32 operations of the
contract with `np.float32` intermediates -- the product, the sum and the sum of the rounding each rounded on their own -- and
stage 3 at the OUTPUT layout (`oracle.lut3d_numpy.rgb_codes_to_yuv`).  A per-frame strength broadcasts over [nf, rows, cols].
"""
from __future__ import annotations

import numpy as np

from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
from tests import _stack_twin as st

F = np.float32
LAYOUTS = st.LAYOUTS
consts = st.consts


def clamp(strength):
    """s' = fminf(fmaxf(s, 0), 1) in float32: np.fmax / np.fmin return the other operand for a NaN, so a NaN is 0."""
    s = np.asarray(strength, dtype=F)
    return np.fmin(np.fmax(s, F(0.0)), F(1.0)).astype(F)


def mix_codes(strength, q0, q1):
    """q_c = (int)((q0_c + s' * (q1_c - q0_c)) + 0.5f) per channel.  q0 / q1: (R, G, B) integer arrays of one shape, [rows, cols] or
    [nf, rows, cols]; `strength` a scalar or, for [nf, rows, cols], one value per frame."""
    s = clamp(strength)
    out = []
    for a, b in zip(q0, q1):
        a, b = np.asarray(a).astype(F), np.asarray(b).astype(F)
        sb = s.reshape(s.shape + (1,) * (a.ndim - s.ndim)) if s.ndim else s
        d = (b - a).astype(F)                                   # exact: both are integers below 2^16
        p = (sb * d).astype(F)
        t = (a + p).astype(F)
        out.append((t + F(0.5)).astype(F).astype(np.int64))
    return tuple(out)


def rgb_out(stages, strength, k, dl, icsx, icsy, planes, **res):
    """Stage 1, the stack and the mix on one frame ([rows, cols] planes): integer (R, G, B) as stage 3 takes them."""
    q0 = tuple(np.asarray(v).astype(np.int64) for v in yuv_to_rgb_codes(k, icsx, icsy, planes))
    q1 = st.rgb_out(stages, k, dl, icsx, icsy, planes, **res)
    return mix_codes(strength, q0, q1)


def apply(stages, strength, k, dl, dout, icsx, icsy, ocsx, ocsy, planes, **res):
    """The contract: (Y, Cb, Cr) at the output depth and layout.  `planes` [rows, cols] with a scalar strength, or [nf, rows, cols]
    with a scalar or one strength per frame."""
    if np.asarray(planes[0]).ndim == 2:
        return rgb_codes_to_yuv(k, dout, ocsx, ocsy, rgb_out(stages, strength, k, dl, icsx, icsy, planes, **res))
    nf = planes[0].shape[0]
    per_frame = np.broadcast_to(np.asarray(strength, dtype=F), (nf,))
    q0, q1 = [], []
    for f in range(nf):
        frame = [p[f] for p in planes]
        q0.append(tuple(np.asarray(v).astype(np.int64) for v in yuv_to_rgb_codes(k, icsx, icsy, frame)))
        q1.append(st.rgb_out(stages, k, dl, icsx, icsy, frame, **res))
    q = mix_codes(per_frame, [np.stack([f[c] for f in q0]) for c in range(3)], [np.stack([f[c] for f in q1]) for c in range(3)])
    per = [rgb_codes_to_yuv(k, dout, ocsx, ocsy, tuple(c[f] for c in q)) for f in range(nf)]
    return [np.stack([f[i] for f in per]) for i in range(3)]
