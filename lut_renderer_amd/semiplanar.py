"""Planar <-> semi-planar containers of the same YUV samples.

`to_semi((y, cb, cr), "p010le")` -> `[y << 6, cbcr << 6]`, `to_planar((y, cbcr), "p010le")` -> `[y, cb, cr]` as codes.  Both
take NumPy arrays or torch tensors (any device) of shape [..., rows, columns]; the chroma plane of a semi-planar frame is
[..., chroma rows, 2 * pairs per row].  This is container shuffling for tests and for callers that hold planar frames -- the engine
itself reads and writes semi-planar frames directly (`LutEngine.apply_yuv(pix_fmt="nv12")`).
"""
from __future__ import annotations

from typing import List, Sequence

import numpy as np

from .formats import SemiFmt, parse_semi_fmt


def _fmt(name: str) -> SemiFmt:
    fmt = parse_semi_fmt(name)
    if fmt is None:
        raise ValueError(f"'{name}' is not a semi-planar format the engine takes")
    return fmt


def _is_np(a) -> bool:
    return isinstance(a, np.ndarray)


def _shl(a, shift: int):
    if shift == 0:
        return a
    if _is_np(a):
        return (a.astype(np.uint32) << shift).astype(a.dtype)
    import torch
    return ((a.to(torch.int32) & 0xffff) << shift).to(a.dtype)       # (int16 planes hold uint16 bits: the cast wraps)


def _shr(a, shift: int):
    if shift == 0:
        return a
    if _is_np(a):
        return (a.astype(np.uint32) >> shift).astype(a.dtype)
    import torch
    return ((a.to(torch.int32) & 0xffff) >> shift).to(a.dtype)


def to_semi(planes: Sequence, name: str) -> List:
    """(y, cb, cr) codes -> [y, cbcr] in the container `name`: pairs interleaved (Cr first for nv21), codes moved to the high bits
    of their words for the p0xx / p2xx formats (low bits zero)."""
    fmt = _fmt(name)
    y, cb, cr = planes
    if tuple(cb.shape) != tuple(cr.shape):
        raise ValueError("Cb and Cr planes differ in shape")
    a, b = (cr, cb) if fmt.swap else (cb, cr)
    if _is_np(a):
        pairs = np.stack([a, b], axis=-1)
    else:
        import torch
        pairs = torch.stack([a, b], dim=-1)
    pairs = pairs.reshape(tuple(a.shape[:-1]) + (2 * a.shape[-1],))
    return [_shl(y, fmt.shift), _shl(pairs, fmt.shift)]


def to_planar(planes: Sequence, name: str) -> List:
    """[y, cbcr] in the container `name` -> [y, cb, cr] codes (`word >> shift`: whatever the low bits hold is dropped)."""
    fmt = _fmt(name)
    y, pairs = planes
    if pairs.shape[-1] % 2:
        raise ValueError("the chroma plane holds whole pairs: an even number of samples per row")
    p = pairs.reshape(tuple(pairs.shape[:-1]) + (pairs.shape[-1] // 2, 2))
    first, second = p[..., 0], p[..., 1]
    cb, cr = (second, first) if fmt.swap else (first, second)
    if _is_np(cb):
        cb, cr = np.ascontiguousarray(cb), np.ascontiguousarray(cr)
    else:
        cb, cr = cb.contiguous(), cr.contiguous()
    return [_shr(y, fmt.shift), _shr(cb, fmt.shift), _shr(cr, fmt.shift)]
