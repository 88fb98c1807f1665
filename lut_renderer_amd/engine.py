"""Python host of the LUT engine: a thin wrapper over the C-ABI (include/lutr.h).

PyTorch is used only as plumbing: device memory (tensors), streams and
torch.distributed (RCCL) for the one collective this path has, the broadcast of the
lattice at LUT load.  All pixel work happens in liblutr's HIP kernels; nothing here
computes pixels, and nothing falls back to the CPU.

Replaces: the `ffmpeg` child process the reference starts per task
(`/root/reference/src/lut_renderer/task_manager.py:145-151`) for the filters built at
`/root/reference/src/lut_renderer/ffmpeg.py:195-247` and `:304-310`.
"""
from __future__ import annotations

import ctypes as C
import re
import threading
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .cube import CubeLut, read_cube, read_lut

_PIXFMT_RE = re.compile(r"^(yuvj?|yuva|gbra?)(420|422|444)?p(\d+)?(le)?$")


class _YuvSide:
    """What the three format classes share: one side of a YUV call, from the `depth`, `csx`, `csy` of its container."""

    @property
    def code(self) -> int:
        return _native.fmt_code(self.depth, self.csx, self.csy)

    @property
    def np_dtype(self):
        return np.uint8 if self.depth <= 8 else np.uint16

    def layout(self) -> _native.YuvLayout:
        """This side as lutr_apply_yuv_semi takes it (here: three planes)."""
        return _native.YuvLayout(0, 0, 0)

    def packing(self) -> _native.YuvPacking:
        """This side as lutr_apply_yuv_packed takes it (here: three planes)."""
        return _native.YuvPacking(0, 0, 0)


class _YuvContainer(_YuvSide):
    """A YUV container that is not three planes: always YUV, never yuvj*, and with a planar twin."""
    family = "yuv"
    full_range = False

    @property
    def planar(self) -> str:
        """The planar format that holds the same samples (nv12 -> yuv420p, p210le -> yuv422p10le, uyvy422 -> yuv422p)."""
        return f"yuv{'420' if self.csy else '422'}p" + ("" if self.depth == 8 else f"{self.depth}le")


@dataclass(frozen=True)
class PixFmt(_YuvSide):
    """Parsed FFmpeg planar pixel-format name (the ones this path can meet)."""
    name: str
    family: str      # "yuv" or "gbr"
    depth: int
    csx: int
    csy: int
    full_range: bool  # yuvj* (legacy full-range marker, media_info.py:145-147)
    alpha: bool = False  # yuva* / gbrap*: a fourth, luma-sized plane at the same depth

    @property
    def nplanes(self) -> int:
        return 4 if self.alpha else 3

    @property
    def colour(self) -> "PixFmt":
        """The three-plane format of the same colour planes (yuva420p10le -> yuv420p10le, gbrap -> gbrp); itself without alpha."""
        if not self.alpha:
            return self
        return parse_pix_fmt(self.name.replace("yuva", "yuv", 1).replace("gbrap", "gbrp", 1))

    def plane_shape(self, plane: int, w: int, h: int) -> Tuple[int, int]:
        if self.family == "gbr" or plane in (0, 3):
            return h, w
        return (h + (1 << self.csy) - 1) >> self.csy, (w + (1 << self.csx) - 1) >> self.csx


@dataclass(frozen=True)
class SemiFmt(_YuvContainer):
    """A semi-planar YUV format: a luma plane and one plane of interleaved chroma pairs."""
    name: str
    depth: int
    csx: int
    csy: int
    swap: int         # 1: Cr comes first in a pair (nv21)
    shift: int        # left shift of the code inside its 16-bit container (p010le: 6)

    nplanes = 2

    def layout(self) -> _native.YuvLayout:
        return _native.YuvLayout(1, self.swap, self.shift)

    def plane_shape(self, plane: int, w: int, h: int) -> Tuple[int, int]:
        """Plane 0: (h, w) luma samples; plane 1: (chroma rows, 2 * pairs per row) chroma samples."""
        if plane == 0:
            return h, w
        return (h + (1 << self.csy) - 1) >> self.csy, 2 * ((w + 1) >> 1)


@dataclass(frozen=True)
class PackedYuvFmt(_YuvContainer):
    """A packed 4:2:2 YUV format: one buffer, rows of ceil(w / 2) groups of four samples."""
    name: str
    depth: int
    order: int        # the samples of a group in memory: 0 Y0 Cb Y1 Cr, 1 Cb Y0 Cr Y1 (uyvy422), 2 Y0 Cr Y1 Cb (yvyu422)
    shift: int        # left shift of the code inside its 16-bit container (y210le: 6)

    nplanes = 1
    csx, csy = 1, 0

    def packing(self) -> _native.YuvPacking:
        return _native.YuvPacking(1, self.order, self.shift)

    def plane_shape(self, plane: int, w: int, h: int) -> Tuple[int, int]:
        """The one buffer: (h, 4 * groups per row) samples."""
        return h, 4 * ((w + 1) >> 1)


@dataclass(frozen=True)
class V210Fmt(_YuvContainer):
    """v210: one buffer of 32-bit words, rows of ceil(w / 6) groups of four words, three 10-bit codes a word."""
    name: str
    depth: int

    nplanes = 1
    csx, csy = 1, 0
    itemsize = 4      # the buffer's elements are the words (torch.int32)

    @staticmethod
    def groups(w: int) -> int:
        """Groups of six luma samples in a row."""
        return (w + 5) // 6

    @staticmethod
    def row_bytes(w: int) -> int:
        """The default row stride: rows are padded to whole blocks of 128 bytes (48 luma samples)."""
        return 128 * ((w + 47) // 48)

    def plane_shape(self, plane: int, w: int, h: int) -> Tuple[int, int]:
        """The one buffer at the default stride: (h, 32 * ceil(w / 48)) words."""
        return h, self.row_bytes(w) // 4


def parse_v210_fmt(name: Optional[str]) -> Optional[V210Fmt]:
    """The `V210Fmt` of a name of `_native.V210_FORMATS` ("v210"), or None for any other name -- `parse_pix_fmt` rejects the name
    and `parse_semi_fmt` / `parse_packed_yuv_fmt` return None for it."""
    if name not in _native.V210_FORMATS:
        return None
    return V210Fmt(name, *_native.V210_FORMATS[name])


def parse_packed_yuv_fmt(name: Optional[str]) -> Optional[PackedYuvFmt]:
    """The packed 4:2:2 format `name` stands for (a name of `_native.PACKED_YUV_FORMATS`), or None for any other name --
    `parse_pix_fmt` keeps rejecting these and `parse_semi_fmt` keeps returning None for them."""
    if name not in _native.PACKED_YUV_FORMATS:
        return None
    return PackedYuvFmt(name, *_native.PACKED_YUV_FORMATS[name])


def parse_semi_fmt(name: Optional[str]) -> Optional[SemiFmt]:
    """The semi-planar format `name` stands for (a name of `_native.SEMI_FORMATS`), or None for any other name --
    `parse_pix_fmt` keeps rejecting these: it describes three-plane frames."""
    if name not in _native.SEMI_FORMATS:
        return None
    return SemiFmt(name, *_native.SEMI_FORMATS[name])


def yuv_side(name: str):
    """One side of `apply_yuv`: the `SemiFmt`, `PackedYuvFmt`, `V210Fmt` or planar `PixFmt` of a YUV format name (yuvj* read as
    yuv*)."""
    return parse_semi_fmt(name) or parse_packed_yuv_fmt(name) or parse_v210_fmt(name) or \
        parse_pix_fmt((name or "").replace("yuvj", "yuv"))


#: packed YUV names FFmpeg has that this path does not take: 4:4:4 packings and big-endian containers
_PACKED_YUV_UNSUPPORTED = ("vuyx", "vuya", "ayuv", "uyva", "xv30le", "xv36le", "xv48le", "ayuv64le", "v30xle", "y210be", "y212be",
                           "y216be", "xv30be", "xv36be", "xv48be", "ayuv64be")


#: container kind -> (its parser, what the RGB refusal calls it, what every other refusal calls it)
_CONTAINER_KINDS = {"v210": (parse_v210_fmt, "v210", "v210"),
                    "packed": (parse_packed_yuv_fmt, "packed", "packed 4:2:2"),
                    "semi": (parse_semi_fmt, "semi-planar", "semi-planar")}

#: v210's relatives FFmpeg knows as codecs, which this path does not take
_V210_UNSUPPORTED = ("v210x", "v410", "v308", "v408", "r210", "r10k")


def source_bit_depth(name: Optional[str]) -> Optional[int]:
    """`params.infer_bit_depth` for a source name that may be a container: p010le and y210le say their depth themselves (the
    digits are not a depth after a 'p')."""
    from .params import infer_bit_depth
    side = parse_semi_fmt(name) or parse_packed_yuv_fmt(name) or parse_v210_fmt(name)
    return side.depth if side else infer_bit_depth(name)


def check_container_options(pix_fmt: str, out_pix_fmt: Optional[str], dither: str = "none", chroma_loc: Optional[str] = None,
                            out_size=None, kinds=("v210", "packed", "semi"), width: Optional[int] = None) -> Optional[str]:
    """The checks `apply_yuv` makes before any GPU work when a side is not three planes: "v210" when a side is v210 (DESIGN.md
    3.14), "packed" when a side is packed 4:2:2, "semi" when one is semi-planar, None when both
    are planar (nothing checked but the packed names this path does not take).  Refused: an RGB side, two kinds of container in
    one call, a subsampling change (packed and v210: only a source that is not 4:2:2), chroma_loc, error-diffusion dither,
    out_size, and a `width` (`apply_yuv`'s, for rows that cannot tell it) when no side is packed or v210."""
    out_name = out_pix_fmt or pix_fmt
    for kind in kinds:
        parse, short, noun = _CONTAINER_KINDS[kind]
        packed, v210 = kind == "packed", kind == "v210"
        if kind == "semi" and width is not None:
            raise ValueError("width is for a packed 4:2:2 side; planar and semi-planar frames tell their own")
        for name in (pix_fmt, out_name) if packed else ():
            if name in _PACKED_YUV_UNSUPPORTED:
                raise ValueError(f"'{name}' is not supported: packed YUV frames are taken as little-endian 4:2:2 "
                                 f"({', '.join(_native.PACKED_YUV_FORMATS)})")
        for name in (pix_fmt, out_name) if v210 else ():
            if name in _V210_UNSUPPORTED:
                raise ValueError(f"'{name}' is not supported: of this family only v210 is taken")
        if parse(pix_fmt) is None and parse(out_name) is None:
            continue
        if parse_rgb_source(pix_fmt) is not None:
            raise ValueError(f"an RGB source ('{pix_fmt}') takes a planar YUV out_pix_fmt, not the {short} '{out_pix_fmt}'")
        if v210:
            if parse_rgb_source(out_name) is not None:
                raise ValueError(f"v210 frames go with YUV formats on both sides ('{pix_fmt}' -> '{out_name}')")
            for other, what in ((parse_semi_fmt, "semi-planar"), (parse_packed_yuv_fmt, "packed 4:2:2")):
                if other(pix_fmt) is not None or other(out_name) is not None:
                    raise ValueError(f"a {what} side together with a v210 side is not supported ('{pix_fmt}' -> '{out_name}')")
        if packed and (parse_semi_fmt(pix_fmt) is not None or parse_semi_fmt(out_name) is not None):
            raise ValueError(f"a semi-planar side together with a packed side is not supported ('{pix_fmt}' -> '{out_name}')")
        a, b = yuv_side(pix_fmt), yuv_side(out_name)
        if getattr(a, "alpha", False) or getattr(b, "alpha", False):
            raise ValueError(f"alpha is carried between planar sides only, not with a {noun} side ('{pix_fmt}' -> '{out_name}')")
        if a.family != "yuv" or b.family != "yuv":
            raise ValueError(f"{noun} frames go with YUV formats on both sides "
                             f"('{pix_fmt}' -> '{out_name if packed or v210 else out_pix_fmt}')")
        if (packed or v210) and (a.csx, a.csy) != (1, 0):
            raise ValueError(f"a {short} destination takes a 4:2:2 source: no chroma subsampling change into '{out_name}' "
                             f"('{pix_fmt}' -> '{out_name}')")
        if kind == "semi" and (a.csx, a.csy) != (b.csx, b.csy):
            raise ValueError(f"a chroma subsampling change is not supported with a semi-planar side "
                             f"('{pix_fmt}' -> '{out_pix_fmt}')")
        if chroma_loc is not None:
            raise ValueError(f"sited chroma resampling (chroma_loc) is not supported with a {noun} side")
        if dither != "none":
            raise ValueError(f"error-diffusion dither is not supported with a {noun} side")
        if out_size is not None:
            raise ValueError(f"a resize (out_size) is not supported with a {noun} side")
        return kind
    return None


def check_packed_options(pix_fmt: str, out_pix_fmt: Optional[str], dither: str = "none", chroma_loc: Optional[str] = None,
                         out_size=None) -> bool:
    """`check_container_options` for the packed 4:2:2 kind alone: False when neither side is packed, True otherwise."""
    return check_container_options(pix_fmt, out_pix_fmt, dither, chroma_loc, out_size, ("packed",)) is not None


def check_semi_options(pix_fmt: str, out_pix_fmt: Optional[str], dither: str = "none", chroma_loc: Optional[str] = None,
                       out_size=None) -> bool:
    """`check_container_options` for the semi-planar kind alone (a packed side is not looked at): False when neither side is
    semi-planar, True otherwise."""
    return check_container_options(pix_fmt, out_pix_fmt, dither, chroma_loc, out_size, ("semi",)) is not None


def packed_frame_width(fmt, planes, width: Optional[int] = None) -> int:
    """The frame width of one side's planes: a packed buffer holds 4 * ceil(w / 2) samples per row, so an odd width has to be
    named (`width`); every other side tells it itself."""
    first = planes if isinstance(planes, torch.Tensor) else planes[0]
    if fmt.nplanes != 1:
        w = first.shape[-1]
    else:
        if first.shape[-1] % 4:
            raise ValueError(f"'{fmt.name}' rows hold whole groups of four samples, got {first.shape[-1]} samples")
        w = first.shape[-1] // 2 if width is None else int(width)
        if 4 * ((w + 1) >> 1) != first.shape[-1]:
            raise ValueError(f"width {w} does not match '{fmt.name}' rows of {first.shape[-1]} samples")
    if width is not None and int(width) != w:
        raise ValueError(f"width {width} does not match the planes ({w})")
    return w


def v210_frame_width(fin, fout, src, dst, width: Optional[int] = None) -> int:
    """The frame width of a call with a v210 side: a planar side tells it (the source's planes, else the destination's when
    given); v210 rows are padded, so with none `width` is required.  Either way the v210 rows must hold it."""
    told = None
    if fin.nplanes == 3:
        told = src[0].shape[-1]
    elif fout.nplanes == 3 and dst is not None:
        told = dst[0].shape[-1]
    if told is None and width is None:
        raise ValueError("width is required with v210 frames when no planar side tells it: v210 rows are padded")
    if told is not None and width is not None and int(width) != told:
        raise ValueError(f"width {width} does not match the planes ({told})")
    w = told if told is not None else int(width)
    if w < 1:
        raise ValueError(f"bad width {w}")
    return w


def parse_pix_fmt(name: str) -> PixFmt:
    m = _PIXFMT_RE.match(name or "")
    if not m:
        raise ValueError(f"unsupported pixel format '{name}'")
    fam, sub, depth, _le = m.groups()
    depth_i = int(depth) if depth else 8
    if not 8 <= depth_i <= 16:
        raise ValueError(f"unsupported bit depth in '{name}'")
    if fam in ("gbr", "gbra"):
        if sub:
            raise ValueError(f"unsupported pixel format '{name}'")
        return PixFmt(name, "gbr", depth_i, 0, 0, True, fam == "gbra")
    if not sub:
        raise ValueError(f"unsupported pixel format '{name}'")
    csx, csy = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[sub]
    return PixFmt(name, "yuv", depth_i, csx, csy, fam == "yuvj", fam == "yuva")


@dataclass(frozen=True)
class RgbSource:
    """An RGB source format of `LutEngine.apply_rgb_to_yuv`: planar `gbrp*`, a packed name of `_native.PACKED_FORMATS`, or a
    planar float name of `_native.FLOAT_FORMATS`."""
    name: str
    packed: bool
    depth: int        # the depth lut3d runs at: the source's (packed: 8 or 16); float: 16, the depth of the output stage's codes
    ncomp: int        # components per pixel of a packed image; 1 for planar
    code: int         # src_kind of lutr_apply_rgb_to_yuv: 0 planar, else LUTR_PACKED(...)
    floating: bool = False   # 32-bit float planes: lutr_apply_planar_rgb_f32 / lutr_apply_rgbf_to_yuv
    nplanes: int = 3         # planes per frame of a planar source (gbrap*, gbrapf32le: 4, the last one alpha)

    @property
    def alpha_slot(self) -> Optional[int]:
        """The component index of a packed format's real alpha (rgba: 3, argb: 0), None for every other format -- rgb0's pad byte
        is not alpha."""
        return _native.PACKED_ALPHA.get(self.name) if self.packed else None

    @property
    def itemsize(self) -> int:
        return 4 if self.floating else 1 if self.depth <= 8 else 2

    def frame_bytes(self, w: int, h: int) -> int:
        return h * w * (self.ncomp if self.packed else self.nplanes) * self.itemsize


def parse_rgb_source(name: Optional[str]) -> Optional[RgbSource]:
    """The RGB source `name` stands for, or None when it is not an RGB format the engine takes (`parse_pix_fmt` keeps rejecting
    packed names: it describes planar frames)."""
    if name in _native.PACKED_FORMATS:
        bits, nc, ro, go, bo = _native.PACKED_FORMATS[name]
        return RgbSource(name, True, bits, nc, _native.packed_code(bits, nc, ro, go, bo))
    if name in _native.FLOAT_FORMATS:
        return RgbSource(name, False, 16, 1, 0, True, _native.FLOAT_FORMATS[name])
    try:
        fmt = parse_pix_fmt(name)
    except ValueError:
        return None
    return RgbSource(name, False, fmt.depth, 1, 0, False, fmt.nplanes) if fmt.family == "gbr" else None


def chroma_loc_code(chroma_loc: Optional[str]) -> int:
    """enum lutr_chroma_loc for a chroma_location name (None = replicate); ValueError for any other name."""
    if chroma_loc is None:
        return _native.CHROMA_REPLICATE
    if chroma_loc not in _native.CHROMA_LOC:
        raise ValueError(f"unknown chroma location '{chroma_loc}' (None | {' | '.join(_native.CHROMA_LOC)})")
    return _native.CHROMA_LOC[chroma_loc]


def check_chroma_loc(chroma_loc: Optional[str], dither: str = "none", pix_fmt: Optional[str] = None,
                     out_pix_fmt: Optional[str] = None) -> None:
    """The checks `apply_yuv` makes of `chroma_loc` before any GPU work: a known name, no error-diffusion dither with it, and
    (given the two pixel formats) no chroma subsampling change with it -- sited resampling across layouts is not defined."""
    chroma_loc_code(chroma_loc)
    if chroma_loc is not None and dither != "none":
        raise ValueError("error-diffusion dither is not defined with sited chroma resampling (chroma_loc)")
    if chroma_loc is not None and pix_fmt and out_pix_fmt and changes_subsampling(pix_fmt, out_pix_fmt):
        raise ValueError(f"sited chroma resampling (chroma_loc) is not defined with a chroma subsampling change "
                         f"('{pix_fmt}' -> '{out_pix_fmt}'); drop chroma_loc to replicate / average over the chroma blocks")


def changes_subsampling(pix_fmt: str, out_pix_fmt: Optional[str]) -> bool:
    """True when the two planar YUV formats differ in chroma subsampling."""
    if not out_pix_fmt:
        return False
    a, b = parse_pix_fmt(pix_fmt.replace("yuvj", "yuv")), parse_pix_fmt(out_pix_fmt.replace("yuvj", "yuv"))
    return (a.csx, a.csy) != (b.csx, b.csy)


#: keywords of `apply_yuv` that the two-output pass does not take
_DUAL_NOT_TAKEN = {"dither": "error-diffusion dither", "chroma_loc": "sited chroma resampling (chroma_loc)",
                   "out_size": "a resize (out_size)", "resize_chunk": "a resize (out_size)",
                   "width": "a packed side (width)"}


def dual_side(name: Optional[str], what: str) -> PixFmt:
    """One side of `apply_yuv_dual`, a planar YUV format (yuvj* read as yuv*); ValueError for RGB, float, semi-planar and packed
    names.  `what` names the argument in the message."""
    if not name:
        raise ValueError(f"the two-output pass needs {what}")
    if parse_semi_fmt(name) is not None or parse_packed_yuv_fmt(name) is not None or name in _PACKED_YUV_UNSUPPORTED:
        raise ValueError(f"the two-output pass takes planar YUV on every side: {what} '{name}' is a semi-planar or packed container")
    if parse_v210_fmt(name) is not None:
        raise ValueError(f"the two-output pass takes planar YUV on every side: {what} '{name}' is a v210 container")
    if parse_rgb_source(name) is not None:
        raise ValueError(f"the two-output pass takes planar YUV on every side: {what} '{name}' is an RGB format")
    fmt = parse_pix_fmt(name.replace("yuvj", "yuv"))
    if fmt.family != "yuv":
        raise ValueError(f"the two-output pass takes planar YUV on every side: {what} '{name}' is an RGB format")
    return fmt


def check_dual_options(pix_fmt: str, out_pix_fmt: Optional[str], out2_pix_fmt: Optional[str], dither: str = "none",
                       chroma_loc: Optional[str] = None, out_size=None) -> Tuple[PixFmt, PixFmt, PixFmt]:
    """The checks `apply_yuv_dual` makes of its formats and options before any GPU work: three planar YUV
    sides, no dither, chroma_loc or out_size.  Returns the three parsed formats (source, first output, second output)."""
    fin = dual_side(pix_fmt, "pix_fmt")
    f1 = dual_side(out_pix_fmt or pix_fmt, "out_pix_fmt")
    f2 = dual_side(out2_pix_fmt, "out2_pix_fmt")
    if dither != "none":
        raise ValueError("error-diffusion dither is not supported with a second output")
    if chroma_loc is not None:
        raise ValueError("sited chroma resampling (chroma_loc) is not supported with a second output")
    if out_size is not None:
        raise ValueError("a resize (out_size) is not supported with a second output")
    return fin, f1, f2


def refuse_dual_keywords(kw: dict) -> None:
    """ValueError when `kw` holds a keyword of `apply_yuv` that the two-output pass does not take, whatever its value."""
    for k, what in _DUAL_NOT_TAKEN.items():
        if k in kw:
            raise ValueError(f"{what} is not supported with a second output: apply_yuv_dual takes no '{k}'")


def dual_args(src, dst, dst2, pix_fmt, out_pix_fmt, out2_pix_fmt):
    """What `apply_yuv_dual` checks of its formats and planes before it touches the engine: the three formats, and the shapes
    and dtypes of the planes given.  Returns (fin, f1, f2, w, h)."""
    fin, f1, f2 = check_dual_options(pix_fmt, out_pix_fmt, out2_pix_fmt)
    if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
        raise ValueError(_PLANE_COUNT[fin.nplanes].format(fin.name))
    if not isinstance(src[0], torch.Tensor):
        raise TypeError("planes must be torch tensors resident on the engine's GPU")
    h, w = src[0].shape[-2], src[0].shape[-1]
    _check_planes(src, fin, w, h, "source")
    if dst is not None:
        _check_planes(dst, f1, w, h, "destination")
    if dst2 is not None:
        _check_planes(dst2, f2, w, h, "second destination")
    return fin, f1, f2, w, h


#: keywords of `apply_yuv` that the two-LUT pass does not take
_CHAIN_NOT_TAKEN = {"dither": "dither", "chroma_loc": "sited chroma resampling (chroma_loc)", "out_size": "a resize (out_size)",
                    "resize_chunk": "a resize (out_size)", "width": "a packed side (width)",
                    "out2_pix_fmt": "a second output (out2_pix_fmt)", "dst2": "a second output (dst2)"}


def chain_side(name: Optional[str], what: str) -> PixFmt:
    """One side of `apply_yuv_chain`, a planar YUV format without alpha (yuvj* read as yuv*); ValueError for alpha, RGB, float,
    semi-planar, packed and v210 names.  `what` names the argument in the message."""
    head = f"the two-LUT pass takes planar YUV on both sides: {what} '{name}'"
    if not name:
        raise ValueError(f"the two-LUT pass needs {what}")
    if parse_semi_fmt(name) is not None:
        raise ValueError(f"{head} is a semi-planar container")
    if parse_packed_yuv_fmt(name) is not None or name in _PACKED_YUV_UNSUPPORTED:
        raise ValueError(f"{head} is a packed container")
    if parse_v210_fmt(name) is not None or name in _V210_UNSUPPORTED:
        raise ValueError(f"{head} is a v210 container")
    rgb = parse_rgb_source(name)
    if rgb is not None:
        raise ValueError(f"{head} is a float RGB format" if rgb.floating else f"{head} is an RGB format")
    fmt = parse_pix_fmt(name.replace("yuvj", "yuv"))
    if fmt.alpha:
        raise ValueError(f"{head} carries alpha")
    return fmt


def check_chain_options(pix_fmt: str, out_pix_fmt: Optional[str], dither: str = "none", chroma_loc: Optional[str] = None,
                        out_size=None, second_pix_fmt: Optional[str] = None) -> Tuple[PixFmt, PixFmt]:
    """The checks `apply_yuv_chain` makes of its formats and options before any GPU work: two planar YUV sides
    without alpha, no dither, chroma_loc, out_size or second output.  Returns the two parsed formats."""
    fin = chain_side(pix_fmt, "pix_fmt")
    fout = chain_side(out_pix_fmt or pix_fmt, "out_pix_fmt")
    if dither != "none":
        raise ValueError("dither is not supported with a second LUT")
    if chroma_loc is not None:
        raise ValueError("sited chroma resampling (chroma_loc) is not supported with a second LUT")
    if out_size is not None:
        raise ValueError("a resize (out_size) is not supported with a second LUT")
    if second_pix_fmt is not None:
        raise ValueError("a second output is not supported with a second LUT")
    return fin, fout


def refuse_chain_keywords(kw: dict) -> None:
    """ValueError when `kw` holds a keyword of `apply_yuv` / `apply_yuv_dual` that the two-LUT pass does not take, whatever its
    value."""
    for k, what in _CHAIN_NOT_TAKEN.items():
        if k in kw:
            raise ValueError(f"{what} is not supported with a second LUT: apply_yuv_chain takes no '{k}'")


def check_lut2(lut) -> None:
    """ValueError for a second LUT that carries a prelut (a .csp shaper): lut3d's prelut is only taken on the first LUT."""
    if lut is not None and getattr(lut, "prelut", None) is not None:
        raise ValueError("the second LUT carries a prelut (a .csp shaper): a prelut is only supported on the first LUT")


def chain_interp(interp: str, interp2: Optional[str]) -> Tuple[int, int]:
    """The two mode codes of `apply_yuv_chain` (`interp2` None = `interp`); ValueError for a name lut3d does not have."""
    for name in (interp, interp2):
        if name is not None and name not in _native.INTERP:
            raise ValueError(f"lut3d has no interpolation mode '{name}'")
    return _native.INTERP[interp], _native.INTERP[interp if interp2 is None else interp2]


def chain_args(src, dst, pix_fmt, out_pix_fmt, interp, interp2):
    """What `apply_yuv_chain` checks of its formats, modes and planes before it touches the engine.  Returns (fin, fout, w, h,
    mode, mode2)."""
    fin, fout = check_chain_options(pix_fmt, out_pix_fmt)
    mode, mode2 = chain_interp(interp, interp2)
    if isinstance(src, torch.Tensor) or len(src) != 3:
        raise ValueError(_PLANE_COUNT[3])
    if not isinstance(src[0], torch.Tensor):
        raise TypeError("planes must be torch tensors resident on the engine's GPU")
    h, w = src[0].shape[-2], src[0].shape[-1]
    _check_planes(src, fin, w, h, "source")
    if dst is not None:
        _check_planes(dst, fout, w, h, "destination")
    return fin, fout, w, h, mode, mode2


#: frames per LUT launch when apply_yuv / apply_rgb resize (`out_size`): the LUT writes a chunk into the engine's scratch at the
#: source size and the resize reads it back while it is still in the Infinity Cache.  LUTR_RESIZE_CHUNK overrides.
RESIZE_CHUNK = 16


#: how the colour planes of an alpha-carrying source stand to their alpha
ALPHA_MODES = ("straight", "premultiplied")


def check_alpha_mode(alpha_mode) -> bool:
    """True for "premultiplied", False for "straight" (the default everywhere: today's paths, bit for bit); ValueError for any
    other value."""
    if alpha_mode not in ALPHA_MODES:
        raise ValueError(f"unknown alpha_mode '{alpha_mode}' ({' | '.join(ALPHA_MODES)})")
    return alpha_mode == "premultiplied"


def check_premul_options(pix_fmt: Optional[str], out_pix_fmt: Optional[str] = None, *, dither: str = "none",
                         chroma_loc: Optional[str] = None, out_size=None, range_src: str = "tv", range_in: Optional[str] = None,
                         lut_depth: Optional[int] = None, out2_pix_fmt: Optional[str] = None, lut2: bool = False,
                         to_yuv: bool = False) -> str:
    """The checks every layer makes of alpha_mode="premultiplied" before any GPU work: "yuv" for a planar yuva*
    source with a planar YUV output, "float" for gbrapf32le in and out; ValueError for everything the contract does not define.
    `to_yuv`: the call is `apply_rgb_to_yuv`'s; `lut2`: a second LUT is set for the call; `out2_pix_fmt`: a second output."""
    head = "alpha_mode='premultiplied'"
    src = parse_rgb_source(pix_fmt)
    if src is not None and not src.floating:
        raise ValueError(f"{head} is not defined for the integer RGB source '{pix_fmt}': PNG / TIFF alpha is straight by "
                         f"specification")
    if src is not None:
        if src.nplanes != 4:
            raise ValueError(f"{head} needs a source that carries alpha: '{pix_fmt}' has none")
    else:
        try:
            side = yuv_side(pix_fmt)
        except ValueError:
            raise ValueError(f"{head} needs a source that carries alpha: '{pix_fmt}' is not one the engine takes") from None
        if not getattr(side, "alpha", False):
            raise ValueError(f"{head} needs a source that carries alpha: '{pix_fmt}' has none")
    if out2_pix_fmt is not None:
        raise ValueError(f"{head} is not supported with the two-output pass (out2_pix_fmt)")
    if lut2:
        raise ValueError(f"{head} is not supported with the two-LUT chain (a second LUT)")
    if dither != "none":
        raise ValueError(f"{head} is not supported with dither ('{dither}')")
    if chroma_loc is not None:
        raise ValueError(f"{head} is not supported with sited chroma resampling (chroma_loc)")
    if out_size is not None:
        raise ValueError(f"{head} is not supported with a resize (out_size / resolution)")
    out_name = out_pix_fmt or pix_fmt
    if src is not None:
        if to_yuv or out_name != pix_fmt:
            raise ValueError(f"{head}: a float source with an integer or YUV output ('{pix_fmt}' -> '{out_name}') is not "
                             f"supported; '{pix_fmt}' in and out is")
        return "float"
    if to_yuv:
        raise ValueError(f"{head} is not supported from an RGB source into YUV (apply_rgb_to_yuv)")
    try:
        out = yuv_side(out_name)
    except ValueError:
        out = None
    if not isinstance(out, PixFmt) or out.family != "yuv":
        raise ValueError(f"{head} takes a planar YUV output (yuv* / yuva*), not '{out_name}'")
    if (range_in or range_src) != range_src or (lut_depth is not None and int(lut_depth) != side.depth):
        raise ValueError(f"{head} is not defined for a call with a prologue (range_src != range_in, or lut_depth other than the "
                         f"source's depth {side.depth}): such a call has no alpha to carry")
    return "yuv"


def alpha_src_struct(t: torch.Tensor, depth: int, device: torch.device) -> _native.AlphaSrc:
    """struct lutr_alpha_src for the alpha plane `t` ([H,W] / [F,H,W]) of a premultiplied call: integer at `depth` bits, or float32."""
    if not isinstance(t, torch.Tensor):
        raise TypeError("planes must be torch tensors resident on the engine's GPU")
    if t.device != device:
        raise ValueError(f"the alpha plane is on {t.device}, engine is on {device}")
    if t.stride(-1) != 1:
        raise ValueError("planes must be dense along the row")
    a = _native.AlphaSrc()
    a.kind = _native.ALPHA_FLOAT if t.dtype == torch.float32 else _native.ALPHA_INT
    a.depth = 0 if a.kind == _native.ALPHA_FLOAT else depth
    a.data = t.data_ptr()
    a.stride = t.stride(-2) * t.element_size()
    a.frame_stride = t.stride(0) * t.element_size() if t.dim() == 3 else 0
    a.step, a.offset = 1, 0
    return a


_PREMUL_IN_PLACE = ("the premultiplied-alpha pass cannot run in place: destination planes must not overlap the source planes or "
                    "the alpha source")


def resize_chunk_default() -> int:
    import os
    v = os.environ.get("LUTR_RESIZE_CHUNK")
    return max(1, int(v)) if v else RESIZE_CHUNK


def parse_size(size) -> Tuple[int, int]:
    """(w, h) from a (w, h) pair or a "WxH" string as ffmpeg's -s takes it; ValueError for anything else."""
    if isinstance(size, str):
        m = re.fullmatch(r"([1-9][0-9]*)x([1-9][0-9]*)", size)
        if not m:
            raise ValueError(f"bad size '{size}' (expected WxH, e.g. 1920x1080)")
        return int(m.group(1)), int(m.group(2))
    try:
        w, h = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"bad size {size!r} (expected (w, h) or 'WxH')") from None
    if w < 1 or h < 1:
        raise ValueError(f"bad size {size!r}")
    return w, h


def _byte_range(t: torch.Tensor) -> Tuple[int, int]:
    lo = hi = t.data_ptr()
    for n, st in zip(t.shape, t.stride()):
        if st >= 0:
            hi += (n - 1) * st * t.element_size()
        else:
            lo += (n - 1) * st * t.element_size()
    return lo, hi + t.element_size()


_RESIZE_IN_PLACE = "a resize cannot run in place: destination planes must not overlap the source planes"
_RGB2YUV_IN_PLACE = "RGB -> YUV cannot run in place: destination planes must not overlap the source"


def _check_not_in_place(src: Sequence[torch.Tensor], dst: Sequence[torch.Tensor], message: str) -> None:
    for a in src:
        alo, ahi = _byte_range(a)
        for b in dst:
            blo, bhi = _byte_range(b)
            if alo < bhi and blo < ahi:
                raise ValueError(message)


_ALPHA_OVERLAP = ("the alpha source overlaps {}: alpha may run in place only as the same plane at the same depth, and must not "
                  "share memory with any other destination plane")


def _check_alpha_overlap(a_src: Optional[torch.Tensor], din: int, dst: Sequence[torch.Tensor], dout: int) -> None:
    """What lutr_alpha_plane would refuse, found before the colour pass is launched: the alpha source (a plane,
    or the packed image that holds it; None = fill) against the alpha destination `dst[3]` -- the same plane at the same depth
    is the no-op, any other overlap of the byte ranges is refused -- and against the colour destinations `dst[:3]`, which the
    colour pass would overwrite before alpha is read."""
    if a_src is None:
        return
    alo, ahi = _byte_range(a_src)
    for i, d in enumerate(dst):
        blo, bhi = _byte_range(d)
        if not (alo < bhi and blo < ahi):
            continue
        same = (i == 3 and din == dout and a_src.dtype == d.dtype and a_src.data_ptr() == d.data_ptr() and a_src.shape == d.shape
                and a_src.stride() == d.stride())
        if not same:
            raise ValueError(_ALPHA_OVERLAP.format("the alpha destination" if i == 3 else f"destination plane {i}"))


def _frames3(planes: Sequence[torch.Tensor]) -> list:
    return [t if t.dim() == 3 else t.unsqueeze(0) for t in planes]


#: what a planar side with the wrong number of planes is told
_PLANE_COUNT = {3: "expected three planes", 4: "'{}' takes four planes: the three colour planes and alpha"}
_ALPHA_RESIZE = "a resize (out_size) is not supported with an alpha-carrying output ('{}'): the resize takes three planes"


def refuse_alpha_resize(out_pix_fmt: Optional[str], out_size) -> None:
    """ValueError for a resize (`out_size` / `resolution`) into an alpha-carrying planar output; any other name
    passes, whatever it is."""
    if out_size is None or not out_pix_fmt:
        return
    try:
        fmt = parse_pix_fmt(out_pix_fmt)
    except ValueError:
        return
    if fmt.alpha:
        raise ValueError(_ALPHA_RESIZE.format(out_pix_fmt))


def _check_planes(planes: Sequence[torch.Tensor], fmt: PixFmt, w: int, h: int, what: str) -> None:
    """The C-ABI takes bare pointers and cannot know buffer sizes: every plane must have exactly the shape and the
    element size `fmt` implies for a w x h frame, or the kernels would read or write outside it."""
    if fmt.nplanes == 2:
        if isinstance(planes, torch.Tensor) or len(planes) != 2:
            raise ValueError(f"'{fmt.name}' takes two planes: luma and the interleaved chroma pairs")
    elif fmt.nplanes == 1:
        if isinstance(planes, torch.Tensor) or len(planes) != 1:
            raise ValueError(f"'{fmt.name}' takes one buffer of packed groups")
    elif len(planes) != fmt.nplanes:
        raise ValueError(_PLANE_COUNT[fmt.nplanes].format(fmt.name))
    esize = getattr(fmt, "itemsize", 1 if fmt.depth <= 8 else 2)
    for i, t in enumerate(planes):
        if not isinstance(t, torch.Tensor):
            raise TypeError("planes must be torch tensors resident on the engine's GPU")
        if t.dim() not in (2, 3):
            raise ValueError("planes must be [H,W] or [F,H,W]")
        if t.is_floating_point() or t.element_size() != esize:
            raise ValueError(f"{what} plane {i}: '{fmt.name}' takes {8 * esize}-bit integer samples, got {t.dtype}")
        if i == 3 and t.stride(-1) != 1:                       # (the colour planes: _planes_struct; alpha goes its own way)
            raise ValueError("planes must be dense along the row")
        want = fmt.plane_shape(i, w, h)
        if isinstance(fmt, V210Fmt):                           # any row that holds the groups (FFmpeg's custom_stride)
            if t.shape[-2] != h or t.shape[-1] < 4 * fmt.groups(w):
                raise ValueError(f"{what} plane {i} is {tuple(t.shape[-2:])}, '{fmt.name}' at {w}x{h} needs {want} words "
                                 f"(at least {4 * fmt.groups(w)} a row)")
        elif tuple(t.shape[-2:]) != want:
            raise ValueError(f"{what} plane {i} is {tuple(t.shape[-2:])}, '{fmt.name}' at {w}x{h} needs {want}")


def _check_float_planes(planes: Sequence[torch.Tensor], fmt: RgbSource, w: int, h: int, what: str) -> None:
    """`_check_planes` for a float format: `fmt.nplanes` float32 planes of h x w (a three-plane list is taken for gbrapf32le too:
    the alpha plane never reaches the kernels)."""
    if isinstance(planes, torch.Tensor) or len(planes) not in (3, fmt.nplanes):
        raise ValueError(f"'{fmt.name}' takes {fmt.nplanes} planes (G, B, R{', A' if fmt.nplanes == 4 else ''})")
    for i, t in enumerate(planes):
        if not isinstance(t, torch.Tensor):
            raise TypeError("planes must be torch tensors resident on the engine's GPU")
        if t.dim() not in (2, 3):
            raise ValueError("planes must be [H,W] or [F,H,W]")
        if t.dtype != torch.float32:
            raise ValueError(f"{what} plane {i}: '{fmt.name}' takes float32 samples, got {t.dtype}")
        if tuple(t.shape[-2:]) != (h, w):
            raise ValueError(f"{what} plane {i} is {tuple(t.shape[-2:])}, '{fmt.name}' at {w}x{h} needs {(h, w)}")
        if i == 3 and t.stride(-1) != 1:                       # (the colour planes: _planes_struct; alpha goes its own way)
            raise ValueError("planes must be dense along the row")


def _planes_struct(planes: Sequence[torch.Tensor], device: torch.device, nplanes: int = 3) -> Tuple[_native.Planes, int]:
    """Describe three [H,W] or [F,H,W] tensors as struct lutr_planes; returns (struct, nframes).  nplanes = 2: a semi-planar
    side (luma, chroma pairs); slot 2 stays NULL.  nplanes = 1: a packed 4:2:2 side; slots 1 and 2 stay NULL."""
    if len(planes) != nplanes:
        raise ValueError(f"expected {('one plane', 'two planes', 'three planes')[nplanes - 1]}")
    st = _native.Planes()
    nframes = None
    for i, t in enumerate(planes):
        if not isinstance(t, torch.Tensor):
            raise TypeError("planes must be torch tensors resident on the engine's GPU")
        if t.device != device:
            raise ValueError(f"plane {i} is on {t.device}, engine is on {device}")
        if t.dim() == 2:
            f, fs = 1, 0
        elif t.dim() == 3:
            f, fs = t.shape[0], t.stride(0) * t.element_size()
        else:
            raise ValueError("planes must be [H,W] or [F,H,W]")
        if t.stride(-1) != 1:
            raise ValueError("planes must be dense along the row")
        if nframes is None:
            nframes = f
        elif nframes != f:
            raise ValueError("planes disagree on the number of frames")
        st.data[i] = t.data_ptr()
        st.stride[i] = t.stride(-2) * t.element_size()
        st.frame_stride[i] = fs
    return st, nframes


def _plane_pair(src: Sequence[torch.Tensor], dst: Sequence[torch.Tensor], device: torch.device):
    """(struct of src, struct of dst, nframes) for a source and a destination that must agree on the number of frames."""
    s, nf = _planes_struct(src, device)
    d, nfd = _planes_struct(dst, device)
    if nf != nfd:
        raise ValueError("src and dst disagree on the number of frames")
    return s, d, nf


def _packed_struct(t, name: str, nc: int, bits: int, device: torch.device, integers_only: bool) -> _native.Packed:
    """Describe one [H,W,C] or [F,H,W,C] packed image as struct lutr_packed.  integers_only: a floating-point tensor of the right
    element size is refused too (apply_packed has always taken one as raw bits)."""
    if not isinstance(t, torch.Tensor) or t.device != device:
        raise ValueError("packed images must be torch tensors resident on the engine's GPU")
    if (t.dim() not in (3, 4) or t.shape[-1] != nc or (integers_only and t.is_floating_point())
            or t.element_size() * 8 != bits):
        raise ValueError(f"'{name}' takes [H,W,{nc}] or [F,H,W,{nc}] tensors of {bits}-bit elements")
    if t.stride(-1) != 1 or t.stride(-2) != nc:
        raise ValueError("pixels must be dense along the row")
    st = _native.Packed()
    st.data = t.data_ptr()
    st.stride = t.stride(-3) * t.element_size()
    st.frame_stride = t.stride(0) * t.element_size() if t.dim() == 4 else 0
    return st


def _yuv_params(fmt_in: int, fmt_out: int, lut_depth: int, matrix_in: str, matrix_out: str, range_src: str, range_in: str,
                range_out: str) -> _native.YuvParams:
    p = _native.YuvParams()
    p.fmt_in, p.fmt_out, p.lut_depth = fmt_in, fmt_out, lut_depth
    p.matrix_in, p.matrix_out = _native.MATRIX[matrix_in], _native.MATRIX[matrix_out]
    p.range_src, p.range_in, p.range_out = _native.RANGE[range_src], _native.RANGE[range_in], _native.RANGE[range_out]
    return p


def _yuv_out_dtype(depth: int, inherit: Optional[torch.dtype]) -> torch.dtype:
    """dtype of freshly allocated YUV output planes: uint8 up to 8 bit; deeper outputs inherit a 16-bit source dtype, else (a
    narrower source, or None: an RGB source) int16."""
    return torch.uint8 if depth <= 8 else inherit if inherit is not None and inherit.itemsize == 2 else torch.int16


def _new_planes(fmt, w: int, h: int, lead: tuple, dtype, device) -> list:
    """Fresh planes of one side: `fmt.nplanes` tensors of `lead + fmt.plane_shape(i, w, h)`."""
    return [torch.empty(lead + fmt.plane_shape(i, w, h), dtype=dtype, device=device) for i in range(fmt.nplanes)]


class LutEngine:
    """One GPU context: a device lattice plus the stream its kernels run on."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        if not torch.cuda.is_available():
            raise RuntimeError("LutEngine needs a HIP GPU; there is no CPU fallback")
        self._lib = _native.load()
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        handle = C.c_void_p()
        _native.check(self._lib.lutr_ctx_create(self.device_index, C.byref(handle)))
        self._ctx = handle
        self.n = 0
        self.scale = None
        self.use_torch_stream = use_torch_stream
        # One context = one stream, one lattice, one work queue (include/lutr.h: thread-safe per context, contexts are not
        # shared between threads).  The reference runs up to 16 tasks on a thread pool (task_manager.py:229-235) and ctypes
        # releases the GIL, so every call that touches the context takes this lock; `api.apply_lut` holds it across
        # set_lut + apply so that a cached engine cannot render one task with another task's lattice.
        self._lock = threading.RLock()
        self.precision = "strict"
        self._applied_lut = None          # the CubeLut object apply_lut uploaded last (its upload-skipping shortcut)
        self._applied_lut2 = None         # ... and the second LUT of apply_lut(cube2=)
        self.n2 = 0
        # grow-only plane caches of _scratch, (key, [3 planes]) per slot: "rz" = the source-size output of the LUT ahead of a
        # resize, "fr" = the 8-bit YUV frames between the two stages of a full-range RGB source
        self._scratch_slots = {}
        # (raw name of the last alpha kernel, the joined name `last_kernel` reports for it) after an alpha-carrying call, else None
        self._alpha_kernels = None

    # -- lifetime ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.lutr_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- lattice ----------------------------------------------------------
    def set_lut(self, lut: CubeLut) -> None:
        table = np.ascontiguousarray(lut.table, dtype=np.float32)
        scale = (C.c_float * 3)(*[float(v) for v in lut.scale])
        with self._lock:
            self._applied_lut = None      # any direct upload invalidates apply_lut's "same LUT as last time" shortcut
            _native.check(self._lib.lutr_ctx_set_lut(
                self._ctx, table.ctypes.data_as(C.POINTER(C.c_float)), int(lut.n), scale))
            self.n, self.scale = int(lut.n), np.array(lut.scale, dtype=np.float32)
            self.set_prelut(getattr(lut, "prelut", None))

    def set_prelut(self, pre) -> None:
        """lut3d's prelut (a cineSpace shaper, `cube.Prelut`) for the lattice just set, or None to remove it.  Uploading a
        lattice drops the prelut of the previous one."""
        if pre is None:
            _native.check(self._lib.lutr_ctx_set_prelut(self._ctx, None, 0, None, None))
            return
        table = np.ascontiguousarray(pre.table, dtype=np.float32)
        pmin = (C.c_float * 3)(*[float(v) for v in pre.min])
        pscale = (C.c_float * 3)(*[float(v) for v in pre.scale])
        _native.check(self._lib.lutr_ctx_set_prelut(
            self._ctx, table.ctypes.data_as(C.POINTER(C.c_float)), int(table.shape[1]), pmin, pscale))

    def load_cube(self, path) -> CubeLut:
        lut = read_lut(path)
        self.set_lut(lut)
        return lut

    def set_lut2(self, lut: Optional[CubeLut]) -> None:
        """The SECOND LUT of `apply_yuv_chain`, or None to remove it.  It lives beside the first lattice: `set_lut`
        / `load_cube` leave it alone and no other call reads it.  A LUT that carries a prelut (a .csp shaper) is a ValueError."""
        check_lut2(lut)
        with self._lock:
            self._applied_lut2 = None     # any direct upload invalidates apply_lut's "same second LUT as last time" shortcut
            if lut is None:
                _native.check(self._lib.lutr_ctx_set_lut2(self._ctx, None, 0, None))
                self.n2 = 0
                return
            table = np.ascontiguousarray(lut.table, dtype=np.float32)
            scale = (C.c_float * 3)(*[float(v) for v in lut.scale])
            _native.check(self._lib.lutr_ctx_set_lut2(
                self._ctx, table.ctypes.data_as(C.POINTER(C.c_float)), int(lut.n), scale))
            self.n2 = int(lut.n)

    def load_cube2(self, path) -> CubeLut:
        lut = read_lut(path)
        self.set_lut2(lut)
        return lut

    def lattice_tensor(self) -> torch.Tensor:
        """The device lattice viewed as a float32 tensor [(n+1)^3 * 4] (no copy)."""
        ptr, size = C.c_void_p(), C.c_size_t()
        _native.check(self._lib.lutr_ctx_lut_device(self._ctx, C.byref(ptr), C.byref(size)))
        return _tensor_from_ptr(ptr.value, size.value // 4, self.device)

    def set_lut_distributed(self, lut: Optional[CubeLut], src: int = 0, group=None) -> None:
        """Rank `src` uploads the lattice; every other rank receives it with ONE broadcast
        (RCCL over xGMI on GPUs).  No other collective exists on this path."""
        import torch.distributed as dist
        self._applied_lut = None
        rank = dist.get_rank(group)
        meta = torch.zeros(4, dtype=torch.float32, device=self.device)
        if rank == src:
            if lut is None:
                raise ValueError("the source rank must pass the LUT")
            self.set_lut(lut)
            meta = torch.tensor([float(lut.n), *[float(v) for v in lut.scale]], dtype=torch.float32,
                                device=self.device)
        dist.broadcast(meta, src=src, group=group)
        if rank != src:
            n = int(meta[0].item())
            scale = (C.c_float * 3)(*[float(v) for v in meta[1:].tolist()])
            _native.check(self._lib.lutr_ctx_lut_alloc(self._ctx, n, scale))
            self.n, self.scale = n, np.array(list(scale), dtype=np.float32)
        dist.broadcast(self.lattice_tensor(), src=src, group=group)
        if rank != src:
            torch.cuda.current_stream(self.device).synchronize()
            _native.check(self._lib.lutr_ctx_lut_seal(self._ctx))      # finiteness + value range of what arrived
        # a cineSpace prelut travels with the lattice: its size first (0 = none), then table and ranges in one tensor
        pre = getattr(lut, "prelut", None) if rank == src else None
        size = torch.tensor([0 if pre is None else int(pre.table.shape[1])], dtype=torch.int32, device=self.device)
        dist.broadcast(size, src=src, group=group)
        nsz = int(size.item())
        if nsz:
            from .cube import Prelut
            if rank == src:
                flat = np.concatenate([pre.table.reshape(-1), pre.min, pre.scale]).astype(np.float32)
                buf = torch.from_numpy(flat).to(self.device)
            else:
                buf = torch.empty(3 * nsz + 6, dtype=torch.float32, device=self.device)
            dist.broadcast(buf, src=src, group=group)
            if rank != src:
                host = buf.cpu().numpy()
                self.set_prelut(Prelut(host[:3 * nsz].reshape(3, nsz), host[3 * nsz:3 * nsz + 3], host[3 * nsz + 3:]))

    # -- control ----------------------------------------------------------
    def set_variant(self, name: str) -> None:
        _native.check(self._lib.lutr_ctx_set_variant(self._ctx, _native.VARIANT[name]))

    def set_precision(self, name: str) -> None:
        """"strict" (default): bit-exact with FFmpeg's scalar C.  "fast": allow the tolerance-bounded tile kernels
        (<= 1 code from strict at 8 and 10 bit).  "fma32": strict's fp32 lattice with a fused multiply-add blend (<= 1 code
        from strict at every depth).  include/lutr.h lutr_ctx_set_precision."""
        if name not in _native.PRECISION:
            raise ValueError(f"unknown precision '{name}' ({' | '.join(_native.PRECISION)})")
        with self._lock:
            _native.check(self._lib.lutr_ctx_set_precision(self._ctx, _native.PRECISION[name]))
            self.precision = name

    @property
    def last_kernel(self) -> str:
        """The kernel of the last call; after an alpha-carrying call "<colour kernel>+<alpha kernel>" (DESIGN.md 3.16)."""
        name = self._lib.lutr_ctx_last_kernel(self._ctx).decode()
        joined = self._alpha_kernels
        return joined[1] if joined is not None and joined[0] == name else name

    def _alpha_plane(self, src, dst: torch.Tensor, din: int, dout: int, w: int, h: int, row0: int, rows: Optional[int],
                     slot: Optional[int] = None, after: Optional[str] = None) -> None:
        """The alpha plane of an alpha-carrying call (lutr_alpha_plane), launched on the engine's stream right
        after the colour pass: `src` is the source's alpha plane ([H,W] / [F,H,W], integer at `din` bits or float32), a packed
        image whose component `slot` is alpha ([H,W,C] / [F,H,W,C]), or None (no alpha on the source: `dst` is filled).
        `after`: what `last_kernel` read before this launch; it then reads "<after>+<alpha kernel>" (None: the alpha kernel)."""
        a = _native.AlphaSrc()
        a.kind, a.depth, a.step, a.offset = _native.ALPHA_NONE, 0, 1, 0
        if src is not None:
            if not isinstance(src, torch.Tensor):
                raise TypeError("planes must be torch tensors resident on the engine's GPU")
            if src.stride(-1) != 1 or (slot is not None and src.stride(-2) != src.shape[-1]):
                raise ValueError("planes must be dense along the row")
            if src.device != self.device:
                raise ValueError("planes must be torch tensors resident on the engine's GPU")
            lead = src.dim() - (2 if slot is None else 3)
            a.kind = _native.ALPHA_FLOAT if src.dtype == torch.float32 else _native.ALPHA_INT
            a.depth = 0 if a.kind == _native.ALPHA_FLOAT else din
            a.data = src.data_ptr()
            a.stride = src.stride(lead) * src.element_size()
            a.frame_stride = src.stride(0) * src.element_size() if lead else 0
            if slot is not None:
                a.step, a.offset = src.shape[-1], slot
            if (src.shape[0] if lead else 1) != (dst.shape[0] if dst.dim() == 3 else 1):
                raise ValueError("src and dst disagree on the number of frames")
        if dst.device != self.device or dst.stride(-1) != 1:
            raise ValueError("planes must be dense along the row and resident on the engine's GPU")
        nf, dfs = (dst.shape[0], dst.stride(0) * dst.element_size()) if dst.dim() == 3 else (1, 0)
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_alpha_plane(
                self._ctx, C.byref(a), dout, C.c_void_p(dst.data_ptr()), dst.stride(-2) * dst.element_size(), dfs, w, h, nf,
                row0, rows))
            if after is not None and w and rows and nf:          # (an empty call launches nothing and names nothing)
                name = self._lib.lutr_ctx_last_kernel(self._ctx).decode()
                self._alpha_kernels = (name, f"{after}+{name}")

    def tile_stats(self, enable: bool = True) -> dict:
        """Counters of the LDS-window kernels since the previous call; (re)arms collection."""
        out = (C.c_uint64 * 8)()
        _native.check(self._lib.lutr_ctx_tile_stats(self._ctx, int(enable), out))
        return {"tiles": out[0], "misses": out[1], "global_tiles": out[2], "staged": out[3],
                "tube_tiles": out[6], "level2_tiles": out[7], "mixed_tiles": out[4]}

    def sync(self) -> None:
        _native.check(self._lib.lutr_ctx_sync(self._ctx))

    def _bind_stream(self) -> None:
        self._alpha_kernels = None        # (every launch binds first: a joined alpha name never outlives the call that made it)
        if self.use_torch_stream:
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _native.check(self._lib.lutr_ctx_set_stream(self._ctx, C.c_void_p(stream)))

    # -- apply ------------------------------------------------------------
    def apply_rgb(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *,
                  depth: int, interp: str = "tetrahedral", row0: int = 0, rows: Optional[int] = None,
                  out_size=None, resize_chunk: Optional[int] = None):
        """lut3d on planar RGB; planes in gbrp order (G, B, R), each [H,W] or [F,H,W].  A fourth plane (gbrap*'s alpha, DESIGN.md
        3.16) is copied to a fourth destination plane; no out_size then.
        out_size = (w, h) or "WxH" resizes the LUT's output to that size (whole frames, not in place)."""
        if not 8 <= int(depth) <= 16:
            raise ValueError(f"unsupported depth {depth}")
        h, w = src[0].shape[-2], src[0].shape[-1]
        if not isinstance(src, torch.Tensor) and len(src) == 4:      # gbrap*: the alpha plane is copied
            fmt = PixFmt(f"gbrap{depth}", "gbr", int(depth), 0, 0, True, True)
            if out_size is not None:
                raise ValueError(_ALPHA_RESIZE.format(fmt.name))
            if dst is None:
                dst = [torch.empty_like(t) for t in src]
            _check_planes(src, fmt, w, h, "source")
            _check_planes(dst, fmt, w, h, "destination")
            _check_alpha_overlap(src[3], int(depth), dst, int(depth))
            with self._lock:
                self.apply_rgb(src[:3], dst[:3], depth=depth, interp=interp, row0=row0, rows=rows)
                self._alpha_plane(src[3], dst[3], int(depth), int(depth), w, h, row0, rows, after=self.last_kernel)
            return dst
        fmt = PixFmt(f"gbrp{depth}", "gbr", int(depth), 0, 0, True)
        if out_size is not None:
            return self._lut_then_resize(src, dst, fmt, fmt, w, h, out_size, row0, rows, resize_chunk, None,
                                         lambda s_, d_: self.apply_rgb(s_, d_, depth=depth, interp=interp))
        if dst is None:
            dst = [torch.empty_like(t) for t in src]
        _check_planes(src, fmt, w, h, "source")
        _check_planes(dst, fmt, w, h, "destination")
        s, d, nf = _plane_pair(src, dst, self.device)
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_planar_rgb(
                self._ctx, depth, _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(d), row0, rows))
        return dst

    def apply_rgb_float(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *,
                        interp: str = "tetrahedral", row0: int = 0, rows: Optional[int] = None, alpha_mode: str = "straight"):
        """lut3d on planar float RGB (gbrpf32le): float32 planes in gbrp order (G, B, R), each [H,W] or [F,H,W];
        float in, float out, nothing clipped.  Input NaN -> 0 and +-inf -> +-FLT_MAX; a .csp prelut is applied per pixel; always
        strict arithmetic.  `dst` may be `src` (in place).  A fourth plane (gbrapf32le's alpha) is copied through unchanged.
        alpha_mode="premultiplied" (four planes only) divides the colour by t = clamp(alpha, 0, 1) in front of
        lut3d and multiplies by it behind, in the same kernel; t == 1 gives the bits of the straight call."""
        premul = check_alpha_mode(alpha_mode)
        if premul and len(src) != 4:
            raise ValueError("alpha_mode='premultiplied' needs a source that carries alpha: 'gbrpf32le' has none")
        fmt = parse_rgb_source("gbrapf32le" if len(src) == 4 else "gbrpf32le")
        h, w = src[0].shape[-2], src[0].shape[-1]
        if dst is None:
            dst = [torch.empty_like(t) for t in src]
        _check_float_planes(src, fmt, w, h, "source")
        _check_float_planes(dst, fmt, w, h, "destination")
        if len(dst) != len(src):
            raise ValueError("src and dst disagree on the number of planes")
        s, d, nf = _plane_pair(src[:3], dst[:3], self.device)
        rows = h - row0 if rows is None else rows
        if premul:
            _check_alpha_overlap(src[3], 0, dst, 0)
            a = alpha_src_struct(src[3], 0, self.device)
            if (src[3].shape[0] if src[3].dim() == 3 else 1) != nf:
                raise ValueError("planes disagree on the number of frames")
        with self._lock:
            self._bind_stream()
            if premul:
                _native.check(self._lib.lutr_apply_planar_rgb_f32_premul(
                    self._ctx, _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(a), C.byref(d), row0, rows))
            else:
                _native.check(self._lib.lutr_apply_planar_rgb_f32(
                    self._ctx, _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(d), row0, rows))
            if len(src) == 4 and dst[3].data_ptr() != src[3].data_ptr():      # (torch's current stream is the one just bound)
                dst[3][..., row0:row0 + rows, :].copy_(src[3][..., row0:row0 + rows, :], non_blocking=True)
        return dst

    # -- resize -----------------------------------------------------------
    def resize(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, size,
               chroma_loc: Optional[str] = None):
        """Resize planar frames (Y, Cb, Cr or gbrp's G, B, R; each [H,W] or [F,H,W]) to `size` = (w, h) or "WxH" with the
        engine's separable bicubic (lutr_resize_planes).  `chroma_loc` sites the chroma samples (None =
        interstitial, the block centre).  Not in place; packed formats are a ValueError."""
        fmt = parse_pix_fmt(pix_fmt.replace("yuvj", "yuv"))
        loc = chroma_loc_code(chroma_loc)
        dw, dh = parse_size(size)
        sh, sw = src[0].shape[-2], src[0].shape[-1]
        if dst is None:
            dst = _new_planes(fmt, dw, dh, tuple(src[0].shape[:-2]), src[0].dtype, self.device)
        _check_planes(src, fmt, sw, sh, "source")
        _check_planes(dst, fmt, dw, dh, "destination")
        _check_not_in_place(src, dst, _RESIZE_IN_PLACE)
        s, d, nf = _plane_pair(src, dst, self.device)
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_resize_planes(
                self._ctx, _native.RESIZE_FAMILY[fmt.family], fmt.depth, fmt.csx, fmt.csy, loc, sw, sh, dw, dh, nf,
                C.byref(s), C.byref(d)))
        return dst

    def _scratch(self, slot: str, fmt: PixFmt, w: int, h: int, nframes: int, dtype) -> list:
        """Engine-owned planes of `nframes` frames at w x h in `fmt` (kept in `slot` for the next call of the same shape or smaller)."""
        key = (fmt.name, w, h, dtype)
        cur = self._scratch_slots.get(slot)
        if cur is None or cur[0] != key or cur[1][0].shape[0] < nframes:
            cur = self._scratch_slots[slot] = (key, _new_planes(fmt, w, h, (nframes,), dtype, self.device))
        return [t[:nframes] for t in cur[1]]

    def _lut_then_resize(self, src, dst, fin: Optional[PixFmt], fout: PixFmt, w: int, h: int, out_size, row0: int, rows, chunk,
                         chroma_loc, lut_call, src_frames=None):
        """The composition of DESIGN.md 3.7: the LUT into engine scratch at the source size, then the resize into dst, a chunk
        of frames at a time, both on the engine's stream with no host wait in between."""
        dw, dh = parse_size(out_size)
        if row0 != 0 or (rows is not None and rows != h):
            raise ValueError("a resize (out_size) takes whole frames: row0 / rows are not supported with it")
        if dst is None:
            lead = tuple(src_frames[0].shape[:1]) if src_frames is not None else tuple(src[0].shape[:-2])
            dst = _new_planes(fout, dw, dh, lead, _yuv_out_dtype(fout.depth, src[0].dtype), self.device)
        if src_frames is None:             # (a packed source comes checked, as a list of one [F,H,W,C] tensor, in src_frames)
            _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, dw, dh, "destination")
        _check_not_in_place(src, dst, _RESIZE_IN_PLACE)
        s3, d3 = (_frames3(src) if src_frames is None else src_frames), _frames3(dst)
        nf = s3[0].shape[0]
        if d3[0].shape[0] != nf:
            raise ValueError("src and dst disagree on the number of frames")
        chunk = resize_chunk_default() if chunk is None else max(1, int(chunk))
        with self._lock:
            tmp_all = self._scratch("rz", fout, w, h, min(chunk, nf), d3[0].dtype)
            for f0 in range(0, nf, chunk):
                n = min(chunk, nf - f0)
                tmp = [t[:n] for t in tmp_all]
                lut_call([t[f0:f0 + n] for t in s3], tmp)
                self.resize(tmp, [t[f0:f0 + n] for t in d3], pix_fmt=fout.name, size=(dw, dh), chroma_loc=chroma_loc)
        return dst

    def apply_packed(self, src: torch.Tensor, dst: Optional[torch.Tensor] = None, *, pix_fmt: str,
                     interp: str = "tetrahedral", row0: int = 0, rows: Optional[int] = None) -> torch.Tensor:
        """lut3d on packed RGB: `src` is [H,W,C] or [F,H,W,C] (C = 3 or 4, uint8, or int16/uint16 for the
        48/64-bit formats), `pix_fmt` an FFmpeg name from `_native.PACKED_FORMATS`.  The fourth component
        is carried over.  `dst` may be `src` (in place)."""
        if pix_fmt not in _native.PACKED_FORMATS:
            raise ValueError(f"unsupported packed pixel format '{pix_fmt}'")
        bits, nc, ro, go, bo = _native.PACKED_FORMATS[pix_fmt]
        if dst is None:
            dst = torch.empty_like(src)
        descs = [_packed_struct(t, pix_fmt, nc, bits, self.device, False) for t in (src, dst)]
        if src.shape != dst.shape:
            raise ValueError("src and dst shapes differ")
        h, w = src.shape[-3], src.shape[-2]
        nf = src.shape[0] if src.dim() == 4 else 1
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_packed_rgb(
                self._ctx, _native.packed_code(bits, nc, ro, go, bo), _native.INTERP[interp], w, h, nf,
                C.byref(descs[0]), C.byref(descs[1]), row0, rows))
        return dst

    def apply_yuv(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *,
                  pix_fmt: str, interp: str = "tetrahedral", matrix_in: str = "bt709",
                  matrix_out: Optional[str] = None, range_src: str = "tv", range_in: Optional[str] = None,
                  range_out: str = "tv", lut_depth: Optional[int] = None, out_pix_fmt: Optional[str] = None,
                  row0: int = 0, rows: Optional[int] = None, dither: str = "none", chroma_loc: Optional[str] = None,
                  out_size=None, resize_chunk: Optional[int] = None, width: Optional[int] = None,
                  alpha_mode: str = "straight"):
        """Fused YUV -> RGB -> lut3d -> RGB -> YUV on planar frames (Y, Cb, Cr).
        `pix_fmt` / `out_pix_fmt` may each name an alpha-carrying format (yuva420p .. yuva444p16le): that side is
        FOUR planes, the last one alpha at the luma size and the format's depth.  The colour planes are this call on the first three
        under the three-plane names, bit for bit, with every option below; alpha never meets the LUT -- it is copied, converted to
        the output depth (nearest code), dropped when the output has none (the plane is still checked), or filled opaque when
        only the output has it or the call has a prologue (range_src != range_in, or lut_depth other than the source's depth: the
        reference's 8-bit intermediate has no alpha), and is treated as straight.  The alpha source must be dense along the row and
        may overlap the destination only as the same plane at the same depth.  Planar sides only; `out_size` with an alpha-carrying output is a
        ValueError.  `last_kernel` is then "<colour kernel>+<alpha kernel>".
        alpha_mode="premultiplied" (a yuva* source, planar YUV out with or without alpha) divides the integer RGB
        by the source's alpha in front of lut3d and multiplies by it behind, inside one kernel family of its own
        (lutr_apply_yuv_premul; any layout pair, row0 / rows on the union block, strict arithmetic, not in place); the output's
        alpha plane is written as for a straight call.  Opaque pixels give the straight call's bits.  Not with a prologue, dither,
        chroma_loc or out_size.  "straight" (the default) is every path described here, unchanged.
        `pix_fmt` / `out_pix_fmt` may each name a packed 4:2:2 format (yuyv422, uyvy422, yvyu422, y210le, y212le, y216le;
        DESIGN.md 3.12): that side is ONE tensor [..., h, 4 * ceil(w / 2)] (bare or in a one-element list), uint8, or int16 as for
        planar 16-bit; `width` names an odd frame width a packed source cannot tell.  The other side may be planar 4:2:2, and a
        planar destination also 4:2:0 or 4:4:4; no dither / chroma_loc / out_size, strict arithmetic, `dst` may be `src` when
        both sides are the same packed format.  The bits are those of the planar call on the de-interleaved samples.
        `pix_fmt` / `out_pix_fmt` may each name a semi-planar format instead (nv12, nv21, nv16, p010le .. p216le; DESIGN.md
        3.11): that side is a sequence of TWO tensors, y [..., h, w] and cbcr [..., ch, 2 * cw] (the pairs of a row side by side);
        same subsampling on both sides, no dither / chroma_loc / out_size, strict arithmetic, `dst` may be `src` when the two
        formats are the same.  The bits are those of the planar call on the same samples.
        dither="error_diffusion" (the reference's `zscale_dither`) dithers the final quantisation; whole frames only.
        dither="blue_noise" (an engine setting) quantises every output sample against a 64 x 64 void-and-cluster
        mask anchored to the frame, inside the LUT pass: any layout pair, row0 / rows as without dither, strict arithmetic.
        chroma_loc ("left" | "center" | "topleft", ffprobe's chroma_location names) resamples chroma bilinearly at that
        siting instead of replicating it (strict arithmetic, not in place, no dither).  None = replicate.
        `out_pix_fmt` may change the chroma subsampling (4:2:0 / 4:2:2 / 4:4:4 either way): input chroma is
        replicated over its input block, output chroma is the mean over its output block; strict arithmetic, no chroma_loc.
        out_size = (w, h) or "WxH" resizes the output planes to that size after everything else (the reference's `-s`,
        DESIGN.md 3.7): the LUT writes `resize_chunk` frames at a time (default RESIZE_CHUNK) into engine scratch at the source
        size and the resize reads them back; whole frames only, not in place.  The resize sites chroma by `chroma_loc`."""
        if dither not in _native.DITHER:
            raise ValueError(f"unknown dither mode '{dither}'")
        premul = check_alpha_mode(alpha_mode)
        if premul:
            check_premul_options(pix_fmt, out_pix_fmt, dither=dither, chroma_loc=chroma_loc, out_size=out_size, range_src=range_src,
                                 range_in=range_in, lut_depth=lut_depth)
        kind = check_container_options(pix_fmt, out_pix_fmt, dither, chroma_loc, out_size, width=width)
        if kind == "v210":
            return self._apply_yuv_v210(src, dst, yuv_side(pix_fmt), yuv_side(out_pix_fmt or pix_fmt), interp, matrix_in, matrix_out,
                                        range_src, range_in, range_out, lut_depth, row0, rows, width)
        if kind is not None:
            return self._apply_yuv_container(kind == "packed", src, dst, yuv_side(pix_fmt), yuv_side(out_pix_fmt or pix_fmt),
                                             interp, matrix_in, matrix_out, range_src, range_in, range_out, lut_depth, row0, rows,
                                             width)
        fin = parse_pix_fmt(pix_fmt)
        fout = parse_pix_fmt(out_pix_fmt or pix_fmt)
        if fin.family != "yuv" or fout.family != "yuv":
            raise ValueError("apply_yuv takes planar YUV formats")
        if fin.alpha or fout.alpha:
            # yuva*: the colour planes through this very call under their three-plane names, then the alpha plane on the same
            # stream
            if out_size is not None and fout.alpha:
                raise ValueError(_ALPHA_RESIZE.format(fout.name))
            check_chroma_loc(chroma_loc, dither, fin.colour.name, fout.colour.name)
            if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
                raise ValueError(_PLANE_COUNT[fin.nplanes].format(fin.name))
            h, w = src[0].shape[-2], src[0].shape[-1]
            _check_planes(src, fin, w, h, "source")
            if dst is None and out_size is None:
                dst = _new_planes(fout, w, h, tuple(src[0].shape[:-2]), _yuv_out_dtype(fout.depth, src[0].dtype), self.device)
            if dst is not None and out_size is None:
                _check_planes(dst, fout, w, h, "destination")
            # a prologue call fills: the reference's 8-bit yuv4xxp intermediate has no alpha to carry
            prologue = (range_in or range_src) != range_src or (lut_depth is not None and lut_depth != fin.depth)
            a_src = src[3] if fin.alpha and not prologue else None
            if fout.alpha and dst is not None:
                _check_alpha_overlap(a_src, fin.depth, dst, fout.depth)
            if premul:
                # the colour planes through lutr_apply_yuv_premul with the source's alpha beside them, then the alpha plane exactly
                # as for a straight call
                _check_alpha_overlap(a_src, fin.depth, dst[:3], fout.depth)
                _check_not_in_place(src, dst[:3], _PREMUL_IN_PLACE)
                s, d, nf = _plane_pair(src[:3], dst[:3], self.device)
                a = alpha_src_struct(src[3], fin.depth, self.device)
                if (src[3].shape[0] if src[3].dim() == 3 else 1) != nf:
                    raise ValueError("planes disagree on the number of frames")
                p = _yuv_params(fin.colour.code, fout.colour.code, fin.depth, matrix_in, matrix_out or matrix_in, range_src,
                                range_src, range_out)
                with self._lock:
                    self._bind_stream()
                    _native.check(self._lib.lutr_apply_yuv_premul(
                        self._ctx, C.byref(p), _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(a), C.byref(d), row0,
                        h - row0 if rows is None else rows))
                    if fout.alpha:
                        self._alpha_plane(a_src, dst[3], fin.depth, fout.depth, w, h, row0, rows, after=self.last_kernel)
                return dst
            with self._lock:
                out = self.apply_yuv(src[:3], None if dst is None else dst[:3], pix_fmt=fin.colour.name, interp=interp,
                                     matrix_in=matrix_in, matrix_out=matrix_out, range_src=range_src, range_in=range_in,
                                     range_out=range_out, lut_depth=lut_depth, out_pix_fmt=fout.colour.name, row0=row0, rows=rows,
                                     dither=dither, chroma_loc=chroma_loc, out_size=out_size, resize_chunk=resize_chunk)
                if fout.alpha:
                    self._alpha_plane(a_src, dst[3], fin.depth, fout.depth, w, h, row0, rows, after=self.last_kernel)
            return out if dst is None else dst
        check_chroma_loc(chroma_loc, dither, fin.name, fout.name)
        xsub = (fin.csx, fin.csy) != (fout.csx, fout.csy)
        p = _yuv_params(fin.code, fout.code, lut_depth if lut_depth is not None else fin.depth, matrix_in, matrix_out or matrix_in,
                        range_src, range_in or range_src, range_out)
        h, w = src[0].shape[-2], src[0].shape[-1]
        if out_size is not None:
            kw = dict(pix_fmt=pix_fmt, interp=interp, matrix_in=matrix_in, matrix_out=matrix_out, range_src=range_src,
                      range_in=range_in, range_out=range_out, lut_depth=lut_depth, out_pix_fmt=out_pix_fmt, dither=dither,
                      chroma_loc=chroma_loc)
            return self._lut_then_resize(src, dst, fin, fout, w, h, out_size, row0, rows, resize_chunk, chroma_loc,
                                         lambda s_, d_: self.apply_yuv(s_, d_, **kw))
        if dst is None:
            dst = _new_planes(fout, w, h, tuple(src[0].shape[:-2]), _yuv_out_dtype(fout.depth, src[0].dtype), self.device)
        _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, w, h, "destination")
        s, d, nf = _plane_pair(src, dst, self.device)
        rows = h - row0 if rows is None else rows
        if dither == "error_diffusion" and (row0 != 0 or rows != h):
            raise ValueError("error-diffusion dither couples the rows of a frame: whole frames only")
        with self._lock:
            self._bind_stream()
            if xsub or dither == "blue_noise":
                _native.check(self._lib.lutr_apply_yuv_xsub(
                    self._ctx, C.byref(p), _native.INTERP[interp], _native.DITHER[dither], w, h, nf, C.byref(s), C.byref(d),
                    row0, rows))
            elif chroma_loc is not None:
                _native.check(self._lib.lutr_apply_yuv_sited(
                    self._ctx, C.byref(p), _native.INTERP[interp], chroma_loc_code(chroma_loc), w, h, nf, C.byref(s), C.byref(d),
                    row0, rows))
            elif dither != "none":
                _native.check(self._lib.lutr_apply_yuv_dither(
                    self._ctx, C.byref(p), _native.INTERP[interp], _native.DITHER[dither], w, h, nf, C.byref(s), C.byref(d)))
            else:
                _native.check(self._lib.lutr_apply_yuv(
                    self._ctx, C.byref(p), _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(d), row0, rows))
        return dst

    def apply_yuv_dual(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None,
                       dst2: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, out_pix_fmt: Optional[str] = None,
                       out2_pix_fmt: str, interp: str = "tetrahedral", matrix_in: str = "bt709",
                       matrix_out: Optional[str] = None, range_src: str = "tv", range_in: Optional[str] = None,
                       range_out: str = "tv", lut_depth: Optional[int] = None, row0: int = 0, rows: Optional[int] = None,
                       **other):
        """`apply_yuv` with TWO planar YUV outputs from one pass (the reference's "pro" mode: a yuv422p10le
        master and the delivery format): the source is read once and lut3d evaluated once per pixel; `out_pix_fmt` and
        `out2_pix_fmt` may differ in depth and chroma subsampling and share `matrix_out` / `range_out`.  Each output has the bits
        of `apply_yuv(..., out_pix_fmt=<its format>)` alone.  Always strict arithmetic; no dither, chroma_loc or out_size;
        nothing may overlap (not in place).  row0 / rows are multiples of the union block height of the three layouts.
        Returns (planes, planes2)."""
        refuse_dual_keywords(other)
        if other:
            raise TypeError(f"apply_yuv_dual() got an unexpected keyword argument '{next(iter(other))}'")
        fin, f1, f2, w, h = dual_args(src, dst, dst2, pix_fmt, out_pix_fmt, out2_pix_fmt)
        if fin.alpha or f1.alpha or f2.alpha:
            # each output carries, fills or drops alpha on its own; the colour planes through this very call
            lead, dt = tuple(src[0].shape[:-2]), src[0].dtype
            if dst is None:
                dst = _new_planes(f1, w, h, lead, _yuv_out_dtype(f1.depth, dt), self.device)
            if dst2 is None:
                dst2 = _new_planes(f2, w, h, lead, _yuv_out_dtype(f2.depth, dt), self.device)
            # (a prologue call fills, as in apply_yuv)
            prologue = (range_in or range_src) != range_src or (lut_depth is not None and lut_depth != fin.depth)
            a_src = src[3] if fin.alpha and not prologue else None
            for f, d in ((f1, dst), (f2, dst2)):
                _check_alpha_overlap(a_src, fin.depth, list(d[:3]) + ([d[3]] if f.alpha else []), f.depth)
            if f1.alpha and f2.alpha:
                _check_not_in_place([dst[3]], list(dst2), "the two outputs' planes must not overlap")
                _check_not_in_place([dst2[3]], list(dst), "the two outputs' planes must not overlap")
            with self._lock:
                self.apply_yuv_dual(src[:3], dst[:3], dst2[:3], pix_fmt=fin.colour.name, out_pix_fmt=f1.colour.name,
                                    out2_pix_fmt=f2.colour.name, interp=interp, matrix_in=matrix_in, matrix_out=matrix_out,
                                    range_src=range_src, range_in=range_in, range_out=range_out, lut_depth=lut_depth, row0=row0,
                                    rows=rows)
                for f, d in ((f1, dst), (f2, dst2)):
                    if f.alpha:
                        self._alpha_plane(a_src, d[3], fin.depth, f.depth, w, h, row0, rows, after=self.last_kernel)
            return dst, dst2
        p = _yuv_params(fin.code, f1.code, lut_depth if lut_depth is not None else fin.depth, matrix_in, matrix_out or matrix_in,
                        range_src, range_in or range_src, range_out)
        lead = tuple(src[0].shape[:-2])
        if dst is None:
            dst = _new_planes(f1, w, h, lead, _yuv_out_dtype(f1.depth, src[0].dtype), self.device)
        if dst2 is None:
            dst2 = _new_planes(f2, w, h, lead, _yuv_out_dtype(f2.depth, src[0].dtype), self.device)
        s, d, nf = _plane_pair(src, dst, self.device)
        d2, nf2 = _planes_struct(dst2, self.device)
        if nf != nf2:
            raise ValueError("src and dst2 disagree on the number of frames")
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_yuv_dual(
                self._ctx, C.byref(p), f2.code, _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(d), C.byref(d2), row0, rows))
        return dst, dst2

    def apply_yuv_chain(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                        out_pix_fmt: Optional[str] = None, interp: str = "tetrahedral", interp2: Optional[str] = None,
                        matrix_in: str = "bt709", matrix_out: Optional[str] = None, range_src: str = "tv",
                        range_in: Optional[str] = None, range_out: str = "tv", lut_depth: Optional[int] = None, row0: int = 0,
                        rows: Optional[int] = None, **other):
        """`apply_yuv` with TWO LUTs in one pass (ffmpeg's `lut3d=A:interp=ia,lut3d=B:interp=ib,format=...`): the
        first LUT (`set_lut`, its prelut included) in mode `interp`, then the second (`set_lut2`) in mode `interp2` (None =
        `interp`) on the first one's integer RGB at the LUT depth, then RGB -> YUV once.  Planar YUV without alpha on both
        sides, any pair of 4:2:0 / 4:2:2 / 4:4:4 at 8..16 bit.  Always strict arithmetic; no dither, chroma_loc, out_size or
        second output; not in place.  row0 / rows are multiples of the union block height of the two layouts."""
        refuse_chain_keywords(other)
        if other:
            raise TypeError(f"apply_yuv_chain() got an unexpected keyword argument '{next(iter(other))}'")
        fin, fout, w, h, mode, mode2 = chain_args(src, dst, pix_fmt, out_pix_fmt, interp, interp2)
        p = _yuv_params(fin.code, fout.code, lut_depth if lut_depth is not None else fin.depth, matrix_in, matrix_out or matrix_in,
                        range_src, range_in or range_src, range_out)
        if dst is None:
            dst = _new_planes(fout, w, h, tuple(src[0].shape[:-2]), _yuv_out_dtype(fout.depth, src[0].dtype), self.device)
        s, d, nf = _plane_pair(src, dst, self.device)
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_yuv_chain(
                self._ctx, C.byref(p), mode, mode2, w, h, nf, C.byref(s), C.byref(d), row0, rows))
        return dst

    def _apply_yuv_container(self, packed, src, dst, fin, fout, interp, matrix_in, matrix_out, range_src, range_in, range_out,
                             lut_depth, row0, rows, width):
        """apply_yuv with a semi-planar side (lutr_apply_yuv_semi) or, `packed`, a packed 4:2:2 side (lutr_apply_yuv_packed: a
        side may be a bare tensor, and `width` names an odd width); the options were checked by `check_container_options`."""
        p = _yuv_params(fin.code, fout.code, lut_depth if lut_depth is not None else fin.depth, matrix_in, matrix_out or matrix_in,
                        range_src, range_in or range_src, range_out)
        bare = packed and isinstance(dst, torch.Tensor)
        if packed and isinstance(src, torch.Tensor):
            src = [src]
        if bare:
            dst = [dst]
        if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
            raise ValueError(f"'{fin.name}' takes {fin.nplanes} plane{'s' if fin.nplanes > 1 else ''}")
        w, h = packed_frame_width(fin, src, width), src[0].shape[-2]
        if dst is None:
            dst = _new_planes(fout, w, h, tuple(src[0].shape[:-2]), _yuv_out_dtype(fout.depth, src[0].dtype), self.device)
        _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, w, h, "destination")
        s, nf = _planes_struct(src, self.device, fin.nplanes)
        d, nfd = _planes_struct(dst, self.device, fout.nplanes)
        if nf != nfd:
            raise ValueError("src and dst disagree on the number of frames")
        entry = self._lib.lutr_apply_yuv_packed if packed else self._lib.lutr_apply_yuv_semi
        sides = [f.packing() if packed else f.layout() for f in (fin, fout)]
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(entry(self._ctx, C.byref(p), _native.INTERP[interp], C.byref(sides[0]), C.byref(sides[1]), w, h, nf,
                                C.byref(s), C.byref(d), row0, rows))
        return dst[0] if bare else dst

    def _apply_yuv_v210(self, src, dst, fin, fout, interp, matrix_in, matrix_out, range_src, range_in, range_out, lut_depth, row0,
                        rows, width):
        """apply_yuv with a v210 side (lutr_apply_yuv_v210): that side is ONE int32 tensor [..., h, words] (bare
        or in a one-element list), 32 * ceil(w / 48) words a row by default; the options were checked by
        `check_container_options`."""
        p = _yuv_params(fin.code, fout.code, lut_depth if lut_depth is not None else fin.depth, matrix_in, matrix_out or matrix_in,
                        range_src, range_in or range_src, range_out)
        vi, vo = isinstance(fin, V210Fmt), isinstance(fout, V210Fmt)
        bare = vo and isinstance(dst, torch.Tensor)
        if vi and isinstance(src, torch.Tensor):
            src = [src]
        if bare:
            dst = [dst]
        if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
            raise ValueError(f"'{fin.name}' takes {fin.nplanes} plane{'s' if fin.nplanes > 1 else ''}")
        w, h = v210_frame_width(fin, fout, src, dst, width), src[0].shape[-2]
        if dst is None:
            # (a fresh v210 buffer is zeroed: the kernels never write the padding of a row)
            dst = [torch.zeros(tuple(src[0].shape[:-2]) + fout.plane_shape(0, w, h), dtype=torch.int32, device=self.device)] if vo \
                else _new_planes(fout, w, h, tuple(src[0].shape[:-2]), _yuv_out_dtype(fout.depth, src[0].dtype), self.device)
        _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, w, h, "destination")
        s, nf = _planes_struct(src, self.device, fin.nplanes)
        d, nfd = _planes_struct(dst, self.device, fout.nplanes)
        if nf != nfd:
            raise ValueError("src and dst disagree on the number of frames")
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_yuv_v210(self._ctx, C.byref(p), _native.INTERP[interp], int(vi), int(vo), w, h, nf,
                                                        C.byref(s), C.byref(d), row0, rows))
        return dst[0] if bare else dst

    # -- RGB source, YUV output --------------------------------
    def _rgb_source(self, src, fmt: RgbSource):
        """Validate an RGB source; returns (planar struct | None, packed struct | None, w, h, nframes, lead shape)."""
        if fmt.floating:
            if isinstance(src, torch.Tensor) or len(src) not in (3, fmt.nplanes):
                raise ValueError(f"'{fmt.name}' takes {fmt.nplanes} planes (G, B, R{', A' if fmt.nplanes == 4 else ''})")
            h, w = src[0].shape[-2], src[0].shape[-1]
            _check_float_planes(src, fmt, w, h, "source")
            st, nf = _planes_struct(src[:3], self.device)          # (an alpha plane is dropped for a YUV output)
            return st, None, w, h, nf, tuple(src[0].shape[:-2])
        if not fmt.packed:
            if isinstance(src, torch.Tensor) or len(src) != fmt.nplanes:
                raise ValueError(f"'{fmt.name}' takes four planes (G, B, R, A)" if fmt.nplanes == 4 else
                                 f"'{fmt.name}' takes three planes (G, B, R)")
            h, w = src[0].shape[-2], src[0].shape[-1]
            _check_planes(src, PixFmt(fmt.name, "gbr", fmt.depth, 0, 0, True, fmt.nplanes == 4), w, h, "source")
            st, nf = _planes_struct(src[:3], self.device)          # (an alpha plane goes its own way: _alpha_plane)
            return st, None, w, h, nf, tuple(src[0].shape[:-2])
        t = src
        st = _packed_struct(t, fmt.name, fmt.ncomp, fmt.depth, self.device, True)
        return None, st, t.shape[-2], t.shape[-3], (t.shape[0] if t.dim() == 4 else 1), tuple(t.shape[:-3])

    def apply_rgb_to_yuv(self, src, dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, out_pix_fmt: str,
                         interp: str = "tetrahedral", matrix_out: str = "smpte170m", range_out: str = "tv", row0: int = 0,
                         rows: Optional[int] = None, dither: str = "none", out_size=None, resize_chunk: Optional[int] = None,
                         lut: bool = True, chroma_loc: Optional[str] = None, intermediate_pix_fmt: Optional[str] = None,
                         prologue_out_range: Optional[str] = None):
        """lut3d on an RGB source, then RGB -> YUV into planar `out_pix_fmt` (4:2:0 / 4:2:2 / 4:4:4, any depth), in one pass
        (DESIGN.md 3.9).  `src` is three gbrp-ordered planes (G, B, R; `pix_fmt` = gbrp, gbrp9le .. gbrp16le) or one [F,]H,W,C
        packed tensor (`pix_fmt` a name of `_native.PACKED_FORMATS`; a fourth component is dropped).  The LUT runs at the source's
        depth; always strict arithmetic.  `pix_fmt` = gbrpf32le | gbrapf32le takes float32 planes (lut3d's float
        path, its output quantised to 16-bit codes for the output stage; an alpha plane is dropped; no `out_size`).  A yuva*
        `out_pix_fmt` takes its alpha from the fourth plane of `gbrap*` / `gbrapf32le` or from the real A of a packed
        name (rgba, bgra, argb, abgr, rgba64le, bgra64le) at the output depth; any other source, and the full-range composition,
        fill it opaque; `gbrap*` with an output without alpha drops the plane.  lut=False leaves lut3d out.  dither / out_size as for `apply_yuv`.  Not in place.
        `intermediate_pix_fmt` / `prologue_out_range` (a LutPlan's fields for a source flagged full range) select the two-stage
        composition of `apply_rgb_full_range`, with `matrix_out` as the plan's matrix."""
        if dither not in _native.DITHER:
            raise ValueError(f"unknown dither mode '{dither}'")
        if chroma_loc is not None:
            raise ValueError("chroma siting (chroma_loc) is not defined for an RGB source: it has no chroma samples to site")
        fin = parse_rgb_source(pix_fmt)
        if fin is None:
            raise ValueError(f"apply_rgb_to_yuv takes gbrp*, gbrpf32le or packed RGB sources, not '{pix_fmt}'")
        fout = parse_pix_fmt((out_pix_fmt or "").replace("yuvj", "yuv"))
        if fin.floating and out_size is not None:
            raise ValueError("a resize (out_size) is not supported with a float source")
        if fout.family != "yuv":
            raise ValueError("apply_rgb_to_yuv writes planar YUV formats; use apply_rgb / apply_packed for RGB output")
        if fout.alpha:
            # a yuva* output: the colour planes through this very call, then alpha from gbrap*'s fourth plane, a
            # packed name's real A or gbrapf32le's fourth plane -- any other source, and the full-range prologue, fill it
            if out_size is not None:
                raise ValueError(_ALPHA_RESIZE.format(fout.name))
            _, _, w, h, _, lead = self._rgb_source(src, fin)
            if dst is None:
                dst = _new_planes(fout, w, h, lead, _yuv_out_dtype(fout.depth, None), self.device)
            _check_planes(dst, fout, w, h, "destination")
            a_src, slot = None, None
            if intermediate_pix_fmt is None:
                if fin.packed and fin.alpha_slot is not None:
                    a_src, slot = src, fin.alpha_slot
                elif not fin.packed and fin.nplanes == 4 and len(src) == 4:
                    a_src = src[3]
            _check_alpha_overlap(a_src, fin.depth, dst, fout.depth)
            with self._lock:
                self.apply_rgb_to_yuv(src, dst[:3], pix_fmt=pix_fmt, out_pix_fmt=fout.colour.name, interp=interp,
                                      matrix_out=matrix_out, range_out=range_out, row0=row0, rows=rows, dither=dither, lut=lut,
                                      intermediate_pix_fmt=intermediate_pix_fmt, prologue_out_range=prologue_out_range)
                self._alpha_plane(a_src, dst[3], fin.depth, fout.depth, w, h, row0, rows, slot, after=self.last_kernel)
            return dst
        if intermediate_pix_fmt is not None:
            return self.apply_rgb_full_range(src, dst, pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt,
                                             intermediate_pix_fmt=intermediate_pix_fmt, prologue_out_range=prologue_out_range,
                                             matrix=matrix_out, interp=interp, range_out=range_out, row0=row0, rows=rows,
                                             dither=dither, out_size=out_size, resize_chunk=resize_chunk)
        planar, packed, w, h, nf, lead = self._rgb_source(src, fin)
        if out_size is not None:
            kw = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, interp=interp, matrix_out=matrix_out, range_out=range_out,
                      dither=dither, lut=lut)
            if fin.packed:
                squeeze = src.dim() == 3
                s4 = src.unsqueeze(0) if squeeze else src
                d3 = dst if dst is None or not squeeze else [t.unsqueeze(0) for t in dst]
                out = self._lut_then_resize([s4], d3, None, fout, w, h, out_size, row0, rows, resize_chunk, None,
                                            lambda s_, d_: self.apply_rgb_to_yuv(s_[0], d_, **kw), src_frames=[s4])
                return dst if dst is not None else [t[0] for t in out] if squeeze else out
            return self._lut_then_resize(src, dst, PixFmt(fin.name, "gbr", fin.depth, 0, 0, True), fout, w, h, out_size, row0,
                                         rows, resize_chunk, None, lambda s_, d_: self.apply_rgb_to_yuv(s_, d_, **kw))
        if dst is None:
            dst = _new_planes(fout, w, h, lead, _yuv_out_dtype(fout.depth, None), self.device)      # (no dtype to inherit: int16)
        _check_planes(dst, fout, w, h, "destination")
        d, nfd = _planes_struct(dst, self.device)
        if nf != nfd:
            raise ValueError("src and dst disagree on the number of frames")
        rows = h - row0 if rows is None else rows
        if dither == "error_diffusion" and (row0 != 0 or rows != h):
            raise ValueError("error-diffusion dither couples the rows of a frame: whole frames only")
        _check_not_in_place([src] if fin.packed else src[:3], dst, _RGB2YUV_IN_PLACE)
        p = _yuv_params(_native.fmt_code(fin.depth, 0, 0), fout.code, fin.depth, matrix_out, matrix_out, range_out, range_out,
                        range_out)
        mode = _native.INTERP[interp] if lut else _native.INTERP_NONE
        with self._lock:
            self._bind_stream()
            if fin.floating:
                _native.check(self._lib.lutr_apply_rgbf_to_yuv(
                    self._ctx, C.byref(p), mode, _native.DITHER[dither], w, h, nf, C.byref(planar), C.byref(d), row0, rows))
                return dst
            _native.check(self._lib.lutr_apply_rgb_to_yuv(
                self._ctx, C.byref(p), mode, _native.DITHER[dither], fin.code, w, h, nf,
                C.byref(planar) if planar is not None else None, C.byref(packed) if packed is not None else None, C.byref(d),
                row0, rows))
        return dst

    def apply_rgb_full_range(self, src, dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, out_pix_fmt: str,
                             intermediate_pix_fmt: str, prologue_out_range: Optional[str], matrix: Optional[str],
                             interp: str = "tetrahedral", range_out: str = "tv", row0: int = 0, rows: Optional[int] = None,
                             dither: str = "none", out_size=None, resize_chunk: Optional[int] = None):
        """An RGB source flagged full range (DESIGN.md 3.9 point 6).  The reference puts `scale=in_range=pc:out_range=R,
        format=<8-bit yuv>` AHEAD of lut3d for it (ffmpeg.py:212-233), so the LUT runs on an 8-bit YUV frame.  Kept by
        composition, two launches on the engine's stream with no host wait: stage 0 is `apply_rgb_to_yuv` without the LUT into
        engine-owned scratch (`intermediate_pix_fmt` at 8 bit, range R = `prologue_out_range`, matrix `matrix` or smpte170m),
        then `apply_yuv` from that frame to `out_pix_fmt`.  The three plan fields are `LutPlan.intermediate_pix_fmt`,
        `.prologue_out_range` and `.matrix`."""
        fin = parse_rgb_source(pix_fmt)
        if fin is None:
            raise ValueError(f"apply_rgb_full_range takes gbrp*, gbrpf32le or packed RGB sources, not '{pix_fmt}'")
        mid = parse_pix_fmt(intermediate_pix_fmt)
        if mid.family != "yuv" or mid.depth != 8:
            raise ValueError(f"the full-range intermediate is an 8-bit planar YUV format, not '{intermediate_pix_fmt}'")
        rng = prologue_out_range or "pc"
        if rng not in _native.RANGE:
            raise ValueError(f"unknown range '{rng}'")
        m = matrix or "smpte170m"
        _, _, w, h, nf, lead = self._rgb_source(src, fin)
        with self._lock:
            tmp = self._scratch("fr", mid, w, h, nf, torch.uint8)
            if not lead:
                tmp = [t[0] for t in tmp]
            self.apply_rgb_to_yuv(src, tmp, pix_fmt=pix_fmt, out_pix_fmt=mid.name, lut=False, matrix_out=m, range_out=rng,
                                  row0=row0, rows=rows)
            return self.apply_yuv(tmp, dst, pix_fmt=mid.name, out_pix_fmt=out_pix_fmt, interp=interp, matrix_in=m, matrix_out=m,
                                  range_src=rng, range_in=rng, range_out=range_out, lut_depth=8, row0=row0, rows=rows,
                                  dither=dither, out_size=out_size, resize_chunk=resize_chunk)


def _yuv_constants(entry: str, *extra, **kw) -> np.ndarray:
    p = _native.YuvParams()
    for k, v in kw.items():
        setattr(p, k, v)
    out = (C.c_float * 32)()
    _native.check(getattr(_native.load(), entry)(C.byref(p), *extra, out))
    return np.array(list(out), dtype=np.float32)


def yuv_constants(**kw) -> np.ndarray:
    """The 32-float constant block liblutr derives for a lutr_yuv_params (host only, no GPU)."""
    return _yuv_constants("lutr_yuv_constants", **kw)


def yuv_constants_xsub(**kw) -> np.ndarray:
    """`yuv_constants` for a chroma subsampling change (lutr_yuv_constants_xsub): the block mean's n is the output block's."""
    return _yuv_constants("lutr_yuv_constants_xsub", **kw)


def yuv_constants_rgb2yuv(**kw) -> np.ndarray:
    """The constant block of `apply_rgb_to_yuv` (lutr_yuv_constants_rgb2yuv): fmt_out, lut_depth, matrix_out and range_out count."""
    return _yuv_constants("lutr_yuv_constants_rgb2yuv", **kw)


def yuv_constants_sited(chroma_loc: Optional[str], **kw) -> np.ndarray:
    """`yuv_constants` with the sited down-sampling's 1/n folded into cbr..crb (lutr_yuv_constants_sited)."""
    return _yuv_constants("lutr_yuv_constants_sited", chroma_loc_code(chroma_loc), **kw)


def _tensor_from_ptr(ptr: int, count: int, device: torch.device) -> torch.Tensor:
    """Wrap `count` device floats at `ptr` as a tensor without copying (__cuda_array_interface__)."""

    class _Holder:
        pass

    h = _Holder()
    h.__cuda_array_interface__ = {
        "shape": (count,), "typestr": "<f4", "data": (ptr, False), "version": 2, "strides": None}
    return torch.as_tensor(h, device=device)
