"""Planar yuv422p10le <-> v210, the same YUV codes in the container of 10-bit SDI capture and play-out cards.

A v210 row is ceil(w / 6) groups of four little-endian 32-bit words; a word holds three 10-bit codes -- slot a in bits 0-9, b in
bits 10-19, c in bits 20-29, bits 30-31 zero:

    word 0: Cb0 Y0 Cr0    word 1: Y1 Cb1 Y2    word 2: Cr1 Y3 Cb2    word 3: Y4 Cr2 Y5

and pair k (Cbk, Crk) belongs to luma samples 2k and 2k + 1 of the group.  Rows are padded to 128 bytes: the default stride is
128 * ceil(w / 48).

`to_v210((y, cb, cr), w)` -> one buffer of words [..., rows, stride / 4]; `to_planar(buf, w)` -> `[y, cb, cr]` as codes.  Both take
NumPy arrays (words as uint32, codes as uint16) or torch tensors on any device (words as int32, codes as int16).  `to_v210` fills
a luma slot beyond the frame with the last real luma sample of the row and a chroma pair beyond it with the last real pair (an
FFmpeg encoder writes zeros there; decoders ignore the slots), and leaves the words of a row past its last group zero;
`to_planar` reads a code as its 10 bits whatever bits 30-31 hold and ignores every slot beyond the frame.  This is container
shuffling for tests and for callers that hold planar frames -- the engine itself reads and writes v210 frames directly
(`LutEngine.apply_yuv(pix_fmt="v210", width=w)`).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np

from .formats import V210Fmt
from .semiplanar import _is_np

#: slot of a group -> (word, bit offset): luma samples 0..5, Cb of pairs 0..2, Cr of pairs 0..2
LUMA_SLOTS = ((0, 10), (1, 0), (1, 20), (2, 10), (3, 0), (3, 20))
CB_SLOTS = ((0, 0), (1, 10), (2, 20))
CR_SLOTS = ((0, 20), (2, 0), (3, 10))


def row_bytes(w: int) -> int:
    """The default stride of a v210 row of `w` luma samples."""
    return V210Fmt.row_bytes(w)


def min_row_bytes(w: int) -> int:
    """The bytes of a row that hold groups: the smallest stride a caller may give."""
    return 16 * V210Fmt.groups(w)


def frame_bytes(w: int, h: int) -> int:
    """Bytes of one frame at the default stride."""
    return row_bytes(w) * h


def _pad_edge(a, n: int):
    """`a` grown to `n` columns with copies of its last one."""
    extra = n - a.shape[-1]
    if extra <= 0:
        return a
    if _is_np(a):
        return np.concatenate([a] + [a[..., -1:]] * extra, axis=-1)
    import torch
    return torch.cat([a] + [a[..., -1:]] * extra, dim=-1)


def to_v210(planes: Sequence, w: Optional[int] = None, stride: Optional[int] = None):
    """(y, cb, cr) codes of a 10-bit 4:2:2 frame `w` wide -> the buffer of words, rows `stride` bytes apart (default: padded to
    128 bytes; any multiple of 4 of at least 16 * ceil(w / 6))."""
    y, cb, cr = planes
    w = y.shape[-1] if w is None else int(w)
    if y.shape[-1] != w or tuple(cb.shape) != tuple(cr.shape) or cb.shape[-1] != (w + 1) >> 1 or \
            tuple(cb.shape[:-1]) != tuple(y.shape[:-1]) or w < 1:
        raise ValueError("not the planes of one 4:2:2 frame of that width")
    g = V210Fmt.groups(w)
    stride = row_bytes(w) if stride is None else int(stride)
    if stride % 4 or stride < 16 * g:
        raise ValueError(f"a v210 row of {w} samples takes a stride that is a multiple of 4 and at least {16 * g}, not {stride}")
    lead = tuple(y.shape[:-1])
    if _is_np(y):
        wide = lambda a: a.astype(np.uint32) & np.uint32(0x3ff)   # noqa: E731
    else:
        import torch
        wide = lambda a: a.to(torch.int32) & 0x3ff                # noqa: E731
    yy = wide(_pad_edge(y, 6 * g)).reshape(lead + (g, 6))
    bb = wide(_pad_edge(cb, 3 * g)).reshape(lead + (g, 3))
    rr = wide(_pad_edge(cr, 3 * g)).reshape(lead + (g, 3))
    words = [None] * 4
    for slots, src in ((LUMA_SLOTS, yy), (CB_SLOTS, bb), (CR_SLOTS, rr)):
        for i, (word, off) in enumerate(slots):
            v = src[..., i] << off
            words[word] = v if words[word] is None else words[word] | v
    if _is_np(y):
        out = np.zeros(lead + (stride // 4,), np.uint32)
        out[..., :4 * g] = np.stack(words, axis=-1).reshape(lead + (4 * g,))
        return out
    import torch
    out = torch.zeros(lead + (stride // 4,), dtype=torch.int32, device=y.device)
    out[..., :4 * g] = torch.stack(words, dim=-1).reshape(lead + (4 * g,))
    return out


def to_planar(buf, w: int) -> List:
    """The buffer of words [..., rows, words a row] -> [y, cb, cr] codes of a frame `w` wide.  Bits 30-31, slots beyond the frame
    and words past the last group are ignored."""
    w = int(w)
    g = V210Fmt.groups(w)
    if w < 1 or buf.shape[-1] < 4 * g:
        raise ValueError(f"rows of {buf.shape[-1]} words do not hold {w} samples ({4 * g} words)")
    lead = tuple(buf.shape[:-1])
    if _is_np(buf):
        if buf.dtype.itemsize != 4 or buf.dtype.kind not in "iu":
            raise ValueError("a v210 buffer holds 32-bit words")
        q = buf[..., :4 * g].view(np.uint32).reshape(lead + (g, 4)) if buf[..., :4 * g].flags.c_contiguous else \
            np.ascontiguousarray(buf[..., :4 * g]).view(np.uint32).reshape(lead + (g, 4))
        code = lambda word, off: ((q[..., word] >> np.uint32(off)) & np.uint32(0x3ff)).astype(np.uint16)   # noqa: E731
        stack = lambda parts: np.stack(parts, axis=-1)            # noqa: E731
        done = np.ascontiguousarray
    else:
        import torch
        if buf.dtype != torch.int32:
            raise ValueError("a v210 buffer holds 32-bit words (torch.int32)")
        q = buf[..., :4 * g].reshape(lead + (g, 4))
        code = lambda word, off: ((q[..., word] >> off) & 0x3ff).to(torch.int16)                            # noqa: E731
        stack = lambda parts: torch.stack(parts, dim=-1)          # noqa: E731
        done = lambda a: a.contiguous()                           # noqa: E731
    cw = (w + 1) >> 1
    out = []
    for slots, n in ((LUMA_SLOTS, w), (CB_SLOTS, cw), (CR_SLOTS, cw)):
        plane = stack([code(word, off) for word, off in slots]).reshape(lead + (len(slots) * g,))
        out.append(done(plane[..., :n]))
    return out
