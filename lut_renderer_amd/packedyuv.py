"""Planar <-> packed 4:2:2 containers of the same YUV samples.

`to_packed((y, cb, cr), "y210le")` -> one buffer of groups `Y0 Cb Y1 Cr`, each code `<< 6`; `to_planar(buf, "y210le", w)` ->
`[y, cb, cr]` as codes.  Both take NumPy arrays or torch tensors (any device) of shape [..., rows, columns]; a packed buffer is
[..., rows, 4 * ceil(w / 2)].  Odd width: `to_packed` writes the second luma sample of the last group as a copy of the last real
one, `to_planar` ignores it.  This is container shuffling for tests and for callers that hold planar frames -- the engine itself
reads and writes packed frames directly (`LutEngine.apply_yuv(pix_fmt="uyvy422")`).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from .formats import PackedYuvFmt, parse_packed_yuv_fmt
from .semiplanar import _is_np, _shl, _shr

#: position of (Y0, Y1, Cb, Cr) inside a group, by `PackedYuvFmt.order`
_SLOTS = {0: (0, 2, 1, 3), 1: (1, 3, 0, 2), 2: (0, 2, 3, 1)}


def _fmt(name: str) -> PackedYuvFmt:
    fmt = parse_packed_yuv_fmt(name)
    if fmt is None:
        raise ValueError(f"'{name}' is not a packed 4:2:2 format the engine takes")
    return fmt


def to_packed(planes: Sequence, name: str):
    """(y, cb, cr) codes of a 4:2:2 frame -> the one buffer of the container `name`: groups in its order, codes moved to the high
    bits of their words for y210le / y212le (low bits zero)."""
    fmt = _fmt(name)
    y, cb, cr = planes
    w, g = y.shape[-1], cb.shape[-1]
    if tuple(cb.shape) != tuple(cr.shape) or g != (w + 1) >> 1 or tuple(cb.shape[:-1]) != tuple(y.shape[:-1]):
        raise ValueError("not the planes of one 4:2:2 frame")
    if w % 2:                                                  # the last group's second luma sample: the last real one again
        if _is_np(y):
            y = np.concatenate([y, y[..., -1:]], axis=-1)
        else:
            import torch
            y = torch.cat([y, y[..., -1:]], dim=-1)
    pairs = y.reshape(tuple(y.shape[:-1]) + (g, 2))
    parts = [None] * 4
    y0, y1, b, r = _SLOTS[fmt.order]
    parts[y0], parts[y1], parts[b], parts[r] = pairs[..., 0], pairs[..., 1], cb, cr
    if _is_np(y):
        buf = np.stack(parts, axis=-1)
    else:
        import torch
        buf = torch.stack(parts, dim=-1)
    return _shl(buf.reshape(tuple(cb.shape[:-1]) + (4 * g,)), fmt.shift)


def to_planar(buf, name: str, w: Optional[int] = None) -> List:
    """The one buffer of the container `name` -> [y, cb, cr] codes of a frame `w` wide (default: two per group); `word >> shift`:
    whatever the low bits hold is dropped, and so is the second luma sample of the last group of an odd width."""
    fmt = _fmt(name)
    if buf.shape[-1] % 4:
        raise ValueError("a packed row holds whole groups of four samples")
    g = buf.shape[-1] // 4
    w = 2 * g if w is None else int(w)
    if (w + 1) >> 1 != g:
        raise ValueError(f"width {w} does not match rows of {g} groups")
    q = _shr(buf, fmt.shift).reshape(tuple(buf.shape[:-1]) + (g, 4))
    y0, y1, b, r = _SLOTS[fmt.order]
    if _is_np(q):
        y = np.stack([q[..., y0], q[..., y1]], axis=-1).reshape(tuple(buf.shape[:-1]) + (2 * g,))[..., :w]
        return [np.ascontiguousarray(y), np.ascontiguousarray(q[..., b]), np.ascontiguousarray(q[..., r])]
    import torch
    y = torch.stack([q[..., y0], q[..., y1]], dim=-1).reshape(tuple(buf.shape[:-1]) + (2 * g,))[..., :w]
    return [y.contiguous(), q[..., b].contiguous(), q[..., r].contiguous()]
