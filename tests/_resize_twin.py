"""NumPy twin of the output resize contract, written from the formula and independent of liblutr.

Tables: the bicubic B = 0, C = 0.6, per axis and plane, in double, then Q14 with the residue on the largest tap.  Pixels: the
integer separable pass (horizontal into an int intermediate, vertical, rounding shift, clamp), computed in int64 so that a
test can also check that every intermediate fits int32."""
import math

import numpy as np

Q = 16384
#: chroma_loc -> (x co-sited, y co-sited); None = interstitial on every subsampled axis
COSITED = {None: (False, False), "left": (True, False), "center": (False, False), "topleft": (True, True)}


def k(t: float) -> float:
    """The bicubic kernel, in the operation order of the library (the tables must agree to the bit)."""
    a = abs(t)
    if a < 1.0:
        return 1.4 * a * a * a - 2.4 * a * a + 1.0
    if a < 2.0:
        return -0.6 * a * a * a + 3.0 * a * a - 4.8 * a + 2.4
    return 0.0


def in_limits(src: int, dst: int) -> bool:
    return dst * 8 >= src and dst <= 16 * src


def table(src: int, dst: int, cs: int = 0, cosited: bool = False):
    """(start [n_out] int64 unclamped, weights [n_out, taps] int64) for luma sizes src -> dst on an axis subsampled by 2^cs."""
    if not in_limits(src, dst):
        raise ValueError(f"{src} -> {dst} outside 1/8 <= dst/src <= 16")
    f = src / dst
    stretch = f if f > 1.0 else 1.0
    n = 2 * math.ceil(2.0 * stretch)
    step = float(1 << cs)
    o = 0.0 if cosited else (step - 1.0) / 2.0
    n_out = (dst + (1 << cs) - 1) >> cs
    start = np.zeros(n_out, np.int64)
    w = np.zeros((n_out, n), np.int64)
    for j in range(n_out):
        X = (step * j + o + 0.5) * f - 0.5
        x = (X - o) / step
        first = math.floor(x) - n // 2 + 1
        wd = [k((first + i - x) / stretch) for i in range(n)]
        s = 0.0
        for v in wd:
            s += v
        q = [math.floor(v / s * 16384.0 + 0.5) for v in wd]
        big = int(np.argmax(q))
        q[big] += Q - sum(q)
        start[j] = first
        w[j] = q
    return start, w


def position(src: int, dst: int, cs: int, cosited: bool, j: int) -> float:
    """Source coordinate (in this plane's samples) that output sample j is centred on."""
    f = src / dst
    step = float(1 << cs)
    o = 0.0 if cosited else (step - 1.0) / 2.0
    return ((step * j + o + 0.5) * f - 0.5 - o) / step


def _pass(a: np.ndarray, start, w, axis: int) -> np.ndarray:
    """sum_k w[j, k] * a[clamp(start[j] + k)] along `axis` (int64)."""
    n_in = a.shape[axis]
    idx = np.clip(start[:, None] + np.arange(w.shape[1])[None, :], 0, n_in - 1)      # [n_out, taps]
    a = np.moveaxis(a.astype(np.int64), axis, -1)
    out = (a[..., idx] * w).sum(-1)
    return np.moveaxis(out, -1, axis)


def resize_plane(p: np.ndarray, depth: int, tx, ty, check_int32: bool = True) -> np.ndarray:
    """One plane [..., H, W] through the contract's integer pass, with the tables (start, weights) of x and y."""
    t = (_pass(p, *tx, axis=-1) + (1 << (depth - 3))) >> (depth - 2)
    if check_int32:
        assert np.abs(t).max(initial=0) < 2 ** 31
    v = _pass(t, *ty, axis=-2)
    if check_int32:
        assert np.abs(v).max(initial=0) + (1 << (29 - depth)) < 2 ** 31
    out = np.clip((v + (1 << (29 - depth))) >> (30 - depth), 0, (1 << depth) - 1)
    return out.astype(np.uint8 if depth <= 8 else np.uint16)


def resize(planes, depth: int, csx: int, csy: int, size_in, size_out, chroma_loc=None):
    """Three planes (Y, Cb, Cr or G, B, R), each [H, W] or [F, H, W], from size_in = (w, h) to size_out = (w, h)."""
    (sw, sh), (dw, dh) = size_in, size_out
    cox, coy = COSITED[chroma_loc]
    out = []
    for i, p in enumerate(planes):
        cx, cy = (csx, csy) if i else (0, 0)
        tx = table(sw, dw, cx, cox and cx > 0)
        ty = table(sh, dh, cy, coy and cy > 0)
        out.append(resize_plane(np.asarray(p), depth, tx, ty))
    return out
