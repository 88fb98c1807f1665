"""Pixel-format descriptions and the checks that look only at names and options.

Nothing here needs torch or a GPU: the argv builder (`command.py`), the numpy container helpers (`semiplanar.py`,
`packedyuv.py`, `v210.py`) and every layer above the engine read formats and refuse option combinations from this module; the
engine (`engine.py`) adds the checks that look at tensors.
"""
from __future__ import annotations

import re
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import _native

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
    first = planes if hasattr(planes, "shape") else planes[0]
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


#: keywords of `apply_yuv` that the two-output pass does not take, and what its refusals call them
_DUAL_NOT_TAKEN = {"dither": "error-diffusion dither", "chroma_loc": "sited chroma resampling (chroma_loc)",
                   "out_size": "a resize (out_size)", "resize_chunk": "a resize (out_size)",
                   "width": "a packed side (width)"}
#: ... and of `apply_yuv` / `apply_yuv_dual` that the two-LUT pass does not take
_CHAIN_NOT_TAKEN = dict(_DUAL_NOT_TAKEN, dither="dither", out2_pix_fmt="a second output (out2_pix_fmt)",
                        dst2="a second output (dst2)")


def _pass_side(name: Optional[str], what: str, noun: str, sides: str, fine: bool, alpha_ok: bool = False) -> PixFmt:
    """One side of the two-output or the two-LUT pass (`noun`), a planar YUV format (yuvj* read as yuv*); ValueError for RGB,
    float, semi-planar, packed and v210 names.  `what` names the argument in the message.  `fine`: the two-LUT pass's
    refusals -- it tells semi-planar from packed and float from integer RGB, and takes neither v210's relatives nor alpha."""
    if not name:
        raise ValueError(f"the {noun} pass needs {what}")
    head = f"the {noun} pass takes planar YUV on {sides}: {what} '{name}'"
    semi = parse_semi_fmt(name) is not None
    if semi or parse_packed_yuv_fmt(name) is not None or name in _PACKED_YUV_UNSUPPORTED:
        kind = "semi-planar or packed" if not fine else "semi-planar" if semi else "packed"
        raise ValueError(f"{head} is a {kind} container")
    if parse_v210_fmt(name) is not None or (fine and name in _V210_UNSUPPORTED):
        raise ValueError(f"{head} is a v210 container")
    rgb = parse_rgb_source(name)
    if rgb is not None:
        raise ValueError(f"{head} is a float RGB format" if fine and rgb.floating else f"{head} is an RGB format")
    fmt = parse_pix_fmt(name.replace("yuvj", "yuv"))
    if fine and fmt.alpha and not alpha_ok:
        raise ValueError(f"{head} carries alpha")
    return fmt


def _refuse_pass_options(not_taken: dict, tail: str, dither: str, chroma_loc: Optional[str], out_size) -> None:
    """ValueError for dither, chroma_loc or out_size with a second output / a second LUT (`tail`), in the words of `not_taken`."""
    for k, given in (("dither", dither != "none"), ("chroma_loc", chroma_loc is not None), ("out_size", out_size is not None)):
        if given:
            raise ValueError(f"{not_taken[k]} is not supported with {tail}")


def _refuse_keywords(kw: dict, not_taken: dict, tail: str, method: str) -> None:
    for k, what in not_taken.items():
        if k in kw:
            raise ValueError(f"{what} is not supported with {tail}: {method} takes no '{k}'")


def dual_side(name: Optional[str], what: str) -> PixFmt:
    """One side of `apply_yuv_dual`, a planar YUV format (yuvj* read as yuv*); ValueError for RGB, float, semi-planar and packed
    names.  `what` names the argument in the message."""
    return _pass_side(name, what, "two-output", "every side", False)


def check_dual_options(pix_fmt: str, out_pix_fmt: Optional[str], out2_pix_fmt: Optional[str], dither: str = "none",
                       chroma_loc: Optional[str] = None, out_size=None) -> Tuple[PixFmt, PixFmt, PixFmt]:
    """The checks `apply_yuv_dual` makes of its formats and options before any GPU work: three planar YUV
    sides, no dither, chroma_loc or out_size.  Returns the three parsed formats (source, first output, second output)."""
    fin = dual_side(pix_fmt, "pix_fmt")
    f1 = dual_side(out_pix_fmt or pix_fmt, "out_pix_fmt")
    f2 = dual_side(out2_pix_fmt, "out2_pix_fmt")
    _refuse_pass_options(_DUAL_NOT_TAKEN, "a second output", dither, chroma_loc, out_size)
    return fin, f1, f2


def refuse_dual_keywords(kw: dict) -> None:
    """ValueError when `kw` holds a keyword of `apply_yuv` that the two-output pass does not take, whatever its value."""
    _refuse_keywords(kw, _DUAL_NOT_TAKEN, "a second output", "apply_yuv_dual")


def chain_side(name: Optional[str], what: str) -> PixFmt:
    """One side of `apply_yuv_chain`, a planar YUV format without alpha (yuvj* read as yuv*); ValueError for alpha, RGB, float,
    semi-planar, packed and v210 names.  `what` names the argument in the message."""
    return _pass_side(name, what, "two-LUT", "both sides", True)


def check_chain_options(pix_fmt: str, out_pix_fmt: Optional[str], dither: str = "none", chroma_loc: Optional[str] = None,
                        out_size=None, second_pix_fmt: Optional[str] = None) -> Tuple[PixFmt, PixFmt]:
    """The checks `apply_yuv_chain` makes of its formats and options before any GPU work: two planar YUV sides
    without alpha, no dither, chroma_loc, out_size or second output.  Returns the two parsed formats."""
    fin = chain_side(pix_fmt, "pix_fmt")
    fout = chain_side(out_pix_fmt or pix_fmt, "out_pix_fmt")
    _refuse_pass_options(_CHAIN_NOT_TAKEN, "a second LUT", dither, chroma_loc, out_size)
    if second_pix_fmt is not None:
        raise ValueError("a second output is not supported with a second LUT")
    return fin, fout


def refuse_chain_keywords(kw: dict) -> None:
    """ValueError when `kw` holds a keyword of `apply_yuv` / `apply_yuv_dual` that the two-LUT pass does not take, whatever its
    value."""
    _refuse_keywords(kw, _CHAIN_NOT_TAKEN, "a second LUT", "apply_yuv_chain")


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



#: what a stage-stack pass does not take, by keyword of its check -> (the keyword's neutral value,
#: what the refusal calls it, `{v}` being the value given).  The CDL and lut1d passes, the stack's one-stage forerunners, word
#: theirs the same way.
_STACK_NOT_TAKEN = {
    "dither": ("none", "dither ('{v}')"), "engine_dither": (None, "dither (engine_dither='{v}')"),
    "chroma_loc": (None, "sited chroma resampling (chroma_loc)"), "out_size": (None, "a resize (out_size / resolution)"),
    "out2_pix_fmt": (None, "the two-output pass (out2_pix_fmt)"), "lut2": (False, "the two-LUT chain (a second LUT)"),
    "cdl": (False, "a CDL"), "alpha_mode": ("straight", "alpha_mode='{v}'"), "strength": (None, "a LUT strength (strength)"),
    "matte": (None, "a matte (matte)"),
    "intermediate_pix_fmt": (None, "the full-range two-stage composition (intermediate_pix_fmt)"),
}

#: what the refusals of the two newer stack passes call them
RGB_STACK_TAIL = "a stage stack on an RGB source (rgb_stages)"
YUV2RGB_STACK_TAIL = "a stage stack from a YUV source into an RGB frame (rgb_out_stages)"


def held_resources(eng, variant: bool = False, lut1d_of=None) -> dict:
    """What an engine holds, as the `lut` / `lut2` / `lut1d` / `prelut` keywords of `check_stage_list` and the stack checks (with
    `variant`, `variant` too).  `eng` is a `LutEngine`, a group's first engine -- the group itself, `lut1d_of`, then tells of the 1D
    LUT -- or any object with some of their attributes: one it has not counts as nothing held."""
    kw = dict(lut=bool(getattr(eng, "n", 0)), lut2=bool(getattr(eng, "n2", 0)),
              lut1d=bool(getattr(eng if lut1d_of is None else lut1d_of, "n1d", 0)), prelut=bool(getattr(eng, "_has_prelut", False)))
    if variant:
        kw["variant"] = getattr(eng, "_variant_name", None)
    return kw


def _refuse_stack_options(tail: str, kernel: str, variant: Optional[str], options: dict, vector=None) -> None:
    """ValueError, in the words of `_STACK_NOT_TAKEN`, for the first of `options` -- keyword -> value, in the order the pass
    called `tail` answers them -- that is not at its neutral value; then for the vec_lds variant (`kernel` names the pass there);
    then, with `vector` = (parsed stages, source depth, destination depth, source name, destination name), for vec_global where
    the names of the call already say that the vector kernel cannot take it.  Sizes, strides and alignment the vector kernel
    cannot take are the C layer's (LUTR_EINVAL: it sees the planes)."""
    for k, v in options.items():
        neutral, what = _STACK_NOT_TAKEN[k]
        if (v is not None) if neutral is None else (v != neutral):
            raise ValueError(f"{what.format(v=v)} is not supported with {tail}")
    if variant == "vec_lds":
        raise ValueError(f"variant vec_lds is not supported with {tail}: there is no LDS-window kernel for the {kernel} pass")
    if variant == "vec_global" and vector is not None:
        st, din, dout, src_name, dst_name = vector
        slow = [f"{k}:{m}" for k, m in st if m in ("pyramid", "prism")]
        if slow:
            raise ValueError(f"variant vec_global cannot take stage '{slow[0]}' of {tail}: the vector kernel has nearest, trilinear "
                             f"and tetrahedral")
        if din <= 8 and dout > 8:
            raise ValueError(f"variant vec_global cannot take an 8-bit source ('{src_name}') written as 16-bit words "
                             f"('{dst_name}') with {tail}: that container mix has no vector kernel")


def check_cdl_options(pix_fmt: Optional[str], out_pix_fmt: Optional[str] = None, *, dither: str = "none",
                      chroma_loc: Optional[str] = None, out_size=None, alpha_mode: str = "straight",
                      out2_pix_fmt: Optional[str] = None, lut2: bool = False, prelut: bool = False,
                      variant: Optional[str] = None) -> Tuple[PixFmt, PixFmt]:
    """The checks every layer makes of a CDL in front of the LUT before any GPU work, the one copy of its
    refusals: planar YUV on both sides (yuva* with straight alpha included), no .csp prelut on the LUT (`prelut`), no dither,
    chroma_loc or out_size, no second output (`out2_pix_fmt`), no second LUT (`lut2`), no premultiplied alpha, not the vec_lds
    variant.  Returns the two parsed formats."""
    tail = "a CDL"
    fin = _pass_side(pix_fmt, "pix_fmt", "CDL", "both sides", True, alpha_ok=True)
    fout = _pass_side(out_pix_fmt or pix_fmt, "out_pix_fmt", "CDL", "both sides", True, alpha_ok=True)
    if fin.family != "yuv" or fout.family != "yuv":
        bad, what = (pix_fmt, "pix_fmt") if fin.family != "yuv" else (out_pix_fmt, "out_pix_fmt")
        raise ValueError(f"the CDL pass takes planar YUV on both sides: {what} '{bad}' is an RGB format")
    if prelut:
        raise ValueError(f"a LUT with a .csp prelut is not supported with {tail}: the prelut's table is indexed by integer codes, "
                         f"and the CDL's output is not a code")
    _refuse_stack_options(tail, "CDL", variant, dict(dither=dither, chroma_loc=chroma_loc, out_size=out_size,
                                                     out2_pix_fmt=out2_pix_fmt, lut2=bool(lut2), alpha_mode=alpha_mode))
    return fin, fout


def check_lut1d_options(pix_fmt: Optional[str], out_pix_fmt: Optional[str] = None, *, interp1d: str = "linear",
                        dither: str = "none", chroma_loc: Optional[str] = None, out_size=None, alpha_mode: str = "straight",
                        out2_pix_fmt: Optional[str] = None, lut2: bool = False, cdl: bool = False, loaded: bool = True,
                        variant: Optional[str] = None) -> Tuple[PixFmt, PixFmt]:
    """The checks every layer makes of a 1D LUT, alone or in front of the 3D LUT, before any GPU work, the one
    copy of its refusals: planar YUV on both sides (yuva* with straight alpha included; packed RGB, float, semi-planar, packed
    4:2:2 and v210 names refused, and an RGB source with a YUV output), a mode lut1d has (`interp1d`), no dither, chroma_loc or
    out_size, no CDL (`cdl`), no second LUT (`lut2`), no second output (`out2_pix_fmt`), no premultiplied alpha, not the vec_lds
    variant, and a 1D LUT to apply (`loaded`).  Returns the two parsed formats."""
    tail = "a 1D LUT"
    if interp1d not in _native.INTERP1D:
        raise ValueError(f"lut1d has no interpolation mode '{interp1d}' ({' | '.join(_native.INTERP1D)})")
    src = parse_rgb_source(pix_fmt)
    if src is not None and parse_rgb_source(out_pix_fmt or pix_fmt) is None:
        raise ValueError(f"an RGB source with a YUV output ('{pix_fmt}' -> '{out_pix_fmt}') is not supported with {tail}")
    fin = _pass_side(pix_fmt, "pix_fmt", "lut1d", "both sides", True, alpha_ok=True)
    fout = _pass_side(out_pix_fmt or pix_fmt, "out_pix_fmt", "lut1d", "both sides", True, alpha_ok=True)
    if fin.family != "yuv" or fout.family != "yuv":
        bad, what = (pix_fmt, "pix_fmt") if fin.family != "yuv" else (out_pix_fmt, "out_pix_fmt")
        raise ValueError(f"the lut1d pass takes planar YUV on both sides: {what} '{bad}' is an RGB format")
    _refuse_stack_options(tail, "lut1d", variant, dict(dither=dither, chroma_loc=chroma_loc, out_size=out_size, cdl=bool(cdl),
                                                       lut2=bool(lut2), out2_pix_fmt=out2_pix_fmt, alpha_mode=alpha_mode))
    if not loaded:
        raise ValueError("no 1D LUT is loaded: call set_lut1d / load_lut1d first, or pass lut1d")
    return fin, fout


#: the stage kinds of a stack and enum lutr_stage_kind
STAGE_KINDS = _native.STAGE_KINDS
#: with the kind of 3.25, which only the matrix entry takes: what a stage list may name
ALL_STAGE_KINDS = {**_native.STAGE_KINDS, **_native.MATRIX_STAGE_KINDS}
MAX_STAGES = 4


def parse_stages(stages, interp: Optional[str] = None, interp2: Optional[str] = None) -> Tuple[Tuple[str, Optional[str]], ...]:
    """The one parser of a stage list.  `stages` is a comma string ("lut1d,cdl,lut3d:trilinear") or a sequence
    of names and (name, mode) pairs.  Returns ((kind, mode), ...): mode is a lut3d mode name for the two lut3d kinds -- the
    stage's own, else `interp` (lut3d) / `interp2` (lut3d2; None = `interp`), else tetrahedral -- and None for lut1d, cdl and
    matrix.  ValueError: an empty list, more than four stages, an unknown kind, a kind twice, a mode on lut1d / cdl / matrix, an
    unknown mode."""
    if isinstance(stages, str):
        items = [s.strip() for s in stages.split(",")] if stages.strip() else []
    elif stages is None:
        items = []
    else:
        items = list(stages)
    if not items:
        raise ValueError("the stage list is empty: a stack has 1 to 4 stages (lut3d | lut3d2 | lut1d | cdl | matrix)")
    if len(items) > MAX_STAGES:
        raise ValueError(f"the stage list has {len(items)} stages: a stack has 1 to {MAX_STAGES}")
    out = []
    for item in items:
        if isinstance(item, str):
            kind, colon, mode = (part.strip() for part in item.partition(":"))
            if colon and not mode:
                raise ValueError(f"stage '{item}' names no mode after ':'")
            mode = mode or None
        else:
            try:
                kind, mode = item
            except (TypeError, ValueError):
                raise ValueError(f"a stage is a name or a (name, mode) pair, not {item!r}") from None
        if kind not in ALL_STAGE_KINDS:
            raise ValueError(f"unknown stage kind '{kind}' ({' | '.join(ALL_STAGE_KINDS)})")
        if any(kind == k for k, _m in out):
            raise ValueError(f"stage kind '{kind}' is listed twice: each kind may appear once")
        if kind in ("lut3d", "lut3d2"):
            if mode is None:
                mode = (interp if kind == "lut3d" else (interp2 or interp)) or "tetrahedral"
            if mode not in _native.INTERP:
                raise ValueError(f"lut3d has no interpolation mode '{mode}' (stage '{kind}')")
        elif mode is not None:
            raise ValueError(f"stage '{kind}' takes no mode ('{mode}')")
        out.append((kind, mode))
    return tuple(out)


def stages_string(stages) -> str:
    """The comma string of a parsed stage list, every lut3d stage with its mode: what `--stages` carries."""
    return ",".join(k if m is None else f"{k}:{m}" for k, m in parse_stages(stages))


def check_strength(strength, nframes: Optional[int] = None):
    """The `strength` argument of a stage stack, checked on the host: None stays None (no mix); a number gives a
    float in [0, 1]; a sequence, NumPy array or CPU tensor gives a float32 array of one strength per frame -- of `nframes` entries
    when that is known -- each finite and in [0, 1].  ValueError otherwise, naming the index and the value."""
    if strength is None:
        return None
    if isinstance(strength, (bool, str, bytes)):
        raise ValueError(f"strength is a number in [0, 1] or one per frame, not {strength!r}")
    try:
        arr = np.asarray(strength.detach().cpu().numpy() if hasattr(strength, "detach") else strength, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"strength is a number in [0, 1] or one per frame, not {strength!r}") from None
    if arr.ndim == 0:
        s = float(arr)
        if not (np.isfinite(s) and 0.0 <= s <= 1.0):
            raise ValueError(f"strength {s!r} is outside [0, 1]")
        return s
    if arr.ndim != 1:
        raise ValueError(f"strength per frame is a flat sequence, not an array of shape {arr.shape}")
    if nframes is not None and arr.shape[0] != nframes:
        raise ValueError(f"strength has {arr.shape[0]} entries for {nframes} frames: a per-frame strength has one per frame")
    bad = np.flatnonzero(~(np.isfinite(arr) & (arr >= 0.0) & (arr <= 1.0)))
    if bad.size:
        i = int(bad[0])
        raise ValueError(f"strength[{i}] = {float(arr[i])!r} is outside [0, 1]")
    return arr.astype(np.float32)


#: what `--matte-pix-fmt` takes -> the matte's depth: one plane of unsigned codes, bytes at 8 bit, else
#: little-endian 16-bit words
MATTE_PIX_FMTS = {"gray": 8, "gray10le": 10, "gray12le": 12, "gray14le": 14, "gray16le": 16}


def check_matte(matte, matte_depth=None, matte_invert=False, *, w: int, h: int, nframes: int, device=None):
    """The `matte`, `matte_depth` and `matte_invert` arguments of a stage stack, the one copy of their checks.
    `matte` is a torch tensor [H, W], [1, H, W] (both a still: one matte for every frame) or [F, H, W] with the call's `nframes`
    frames, at the luma size `w` x `h` of the call, of dtype uint8 (depth 8, the default) or int16 / uint16 (`matte_depth` 9..16,
    required), dense along the row, on `device` (the engine's; None: not checked).  Returns (matte, depth, invert as 0 | 1,
    still).  ValueError otherwise, naming the argument and the fault."""
    if not (hasattr(matte, "dim") and hasattr(matte, "data_ptr") and hasattr(matte, "element_size")):
        raise ValueError(f"matte is a torch tensor [H,W], [1,H,W] or [F,H,W] on the engine's device, not {type(matte).__name__}")
    if device is not None and matte.device != device:
        raise ValueError(f"matte is on {matte.device}, the engine is on {device}: the matte must be on the engine's device")
    name = str(matte.dtype).replace("torch.", "")
    if name not in ("uint8", "int16", "uint16"):
        raise ValueError(f"matte has dtype {name}: a matte is uint8, or int16 / uint16 with matte_depth")
    wide = name != "uint8"
    if isinstance(matte_depth, bool) or (matte_depth is not None and not isinstance(matte_depth, (int, np.integer))):
        raise ValueError(f"matte_depth is an integer in 8..16, not {matte_depth!r}")
    if matte_depth is None:
        if wide:
            raise ValueError(f"matte_depth is required for a {name} matte (9..16: the bits of its codes)")
        matte_depth = 8
    depth = int(matte_depth)
    if not 8 <= depth <= 16:
        raise ValueError(f"matte_depth {depth} is outside 8..16")
    if wide and depth == 8:
        raise ValueError(f"matte_depth 8 is held in bytes: a {name} matte has matte_depth 9..16")
    if not wide and depth != 8:
        raise ValueError(f"matte_depth {depth} is held in 16-bit words: a uint8 matte has matte_depth 8")
    if not isinstance(matte_invert, (bool, np.bool_)):
        raise ValueError(f"matte_invert is True or False, not {matte_invert!r}")
    if matte.dim() not in (2, 3):
        raise ValueError(f"matte has shape {tuple(matte.shape)}: a matte is [H,W], [1,H,W] or [F,H,W]")
    if tuple(matte.shape[-2:]) != (h, w):
        raise ValueError(f"matte is {matte.shape[-1]}x{matte.shape[-2]}, the frame is {w}x{h}: a matte has the luma size of the frame")
    still = matte.dim() == 2 or matte.shape[0] == 1
    if not still and matte.shape[0] != nframes:
        raise ValueError(f"matte has {matte.shape[0]} frames for {nframes} frames: a matte has one frame (a still) or one per frame")
    if w > 1 and matte.stride(-1) != 1:
        raise ValueError("matte must be dense along the row")
    return matte, depth, int(bool(matte_invert)), still


def implied_stages(cube: bool, cube2: bool = False, lut1d: bool = False, cdl: bool = False) -> Tuple[str, ...]:
    """The stage list the options of a call without `stages` imply when a strength sends it to the stack: the
    order of the dedicated routes -- lut1d, cdl, lut3d, lut3d2.  A 1D LUT without `cube` is lut1d alone, as in `apply_lut`;
    otherwise the first lattice is listed whether it comes with the call or the engine holds it."""
    st = []
    if lut1d:
        st.append("lut1d")
    if cdl:
        st.append("cdl")
    if cube or not lut1d:
        st.append("lut3d")
    if cube2:
        st.append("lut3d2")
    return tuple(st)


def check_stage_list(stages, *, cdl: bool = False, lut: bool = True, lut2: bool = True, lut1d: bool = True, prelut: bool = False,
                     rgb_matrix: bool = False):
    """What every stack refuses about the list and its resources, whatever its sides: a list
    `parse_stages` takes; every listed stage's resource there and no CDL or matrix without its stage; no lut3d directly behind cdl
    or matrix when the first LUT carries a .csp prelut.  Returns the parsed stages."""
    st = parse_stages(stages)
    kinds = [k for k, _m in st]
    if "lut3d" in kinds and not lut:
        raise ValueError("stage 'lut3d' is listed and no 3D LUT is loaded: call set_lut / load_cube first, or pass cube")
    if "lut3d2" in kinds and not lut2:
        raise ValueError("stage 'lut3d2' is listed and no second LUT is loaded: call set_lut2 / load_cube2 first, or pass cube2")
    if "lut1d" in kinds and not lut1d:
        raise ValueError("stage 'lut1d' is listed and no 1D LUT is loaded: call set_lut1d / load_lut1d first, or pass lut1d")
    for kind, given, arg, name, its in (("cdl", cdl, "cdl", "a CDL", "the CDL's"),
                                        ("matrix", rgb_matrix, "rgb_matrix", "an RGB matrix", "the matrix's")):
        if kind in kinds and not given:
            raise ValueError(f"stage '{kind}' is listed and no {name.split(' ', 1)[1]} is given: pass {arg}")
        if given and kind not in kinds:
            raise ValueError(f"{name} is given and the stage list has no '{kind}' stage")
        if prelut and kind in kinds and kinds[kinds.index(kind) + 1:kinds.index(kind) + 2] == ["lut3d"]:
            raise ValueError(f"stage 'lut3d' directly behind '{kind}' is not supported with a LUT that carries a .csp prelut: the "
                             f"prelut's table is indexed by integer codes, and {its} output is not a code")
    return st


def check_stack_options(pix_fmt: Optional[str], out_pix_fmt: Optional[str] = None, *, stages, cdl: bool = False,
                        lut: bool = True, lut2: bool = True, lut1d: bool = True, prelut: bool = False, dither: str = "none",
                        chroma_loc: Optional[str] = None, out_size=None, alpha_mode: str = "straight",
                        out2_pix_fmt: Optional[str] = None, variant: Optional[str] = None, strength=None,
                        precision: Optional[str] = None, matte: bool = False, rgb_matrix: bool = False):
    """The checks every layer makes of a stage stack before any GPU work, the one copy of its refusals: a stage
    list `parse_stages` takes; every listed stage's resource there (`lut`, `lut2`, `lut1d`: a first / second lattice, a 1D LUT is
    loaded; `cdl`: a CDL is given) and no CDL without a cdl stage; no lut3d directly behind cdl when the first LUT carries a .csp
    prelut (`prelut`); planar YUV on both sides (yuva* with straight alpha included); no dither, chroma_loc, out_size, second
    output or premultiplied alpha; not the vec_lds variant.  With a `strength` (anything but None) every message
    names it beside the option, the strength itself is checked (`check_strength`) and a `precision` other than strict is refused.
    With `matte` (True: the call has a matte plane, which `check_matte` checks) every message names the matte as
    well, and `precision` is refused likewise.  `rgb_matrix` (True: an RGB matrix is given): a matrix stage and
    its matrix come together, lut3d directly behind matrix is refused with a prelut as behind cdl, and a strength or a matte
    together with a matrix stage is refused.
    Returns (parsed stages, source format, output format)."""
    mixed = strength is not None
    matte = matte is not None and matte is not False
    # what the mix is called beside an option, and in the name of the pass; None without a strength or a matte
    what, short = {(True, True): ("strength and a matte", "strength, matte"), (False, True): ("a matte", "matte"),
                   (True, False): ("strength", "strength"), (False, False): (None, None)}[(mixed, matte)]
    tail = f"a stage stack with {what}" if what else "a stage stack"
    noun = f"stack ({short})" if what else "stack"
    st = check_stage_list(stages, cdl=cdl, lut=lut, lut2=lut2, lut1d=lut1d, prelut=prelut, rgb_matrix=rgb_matrix)
    if what and "matrix" in [k for k, _m in st]:
        raise ValueError(f"stage 'matrix' is not supported with {what}: the matrix stage has no mix form")
    fin = _pass_side(pix_fmt, "pix_fmt", noun, "both sides", True, alpha_ok=True)
    fout = _pass_side(out_pix_fmt or pix_fmt, "out_pix_fmt", noun, "both sides", True, alpha_ok=True)
    _refuse_stack_options(tail, "stack", variant, dict(dither=dither, chroma_loc=chroma_loc, out_size=out_size,
                                                       out2_pix_fmt=out2_pix_fmt, alpha_mode=alpha_mode))
    if what and precision not in (None, "strict"):
        raise ValueError(f"precision='{precision}' is not supported with {what}: the mix is defined on the strict path only")
    if mixed:
        check_strength(strength)
    return st, fin, fout


#: how the colour planes of an alpha-carrying source stand to their alpha
ALPHA_MODES = ("straight", "premultiplied")


def check_alpha_mode(alpha_mode) -> bool:
    """True for "premultiplied", False for "straight" (the default everywhere: today's paths, bit for bit); ValueError for any
    other value."""
    if alpha_mode not in ALPHA_MODES:
        raise ValueError(f"unknown alpha_mode '{alpha_mode}' ({' | '.join(ALPHA_MODES)})")
    return alpha_mode == "premultiplied"


def has_prologue(depth: int, range_src: str = "tv", range_in: Optional[str] = None, lut_depth: Optional[int] = None) -> bool:
    """True when a YUV call from a source of `depth` bits has a prologue: a range conversion ahead of the LUT (range_in other
    than range_src) or a LUT depth other than the source's.  The reference's 8-bit intermediate has no alpha to carry."""
    return (range_in or range_src) != range_src or (lut_depth is not None and int(lut_depth) != depth)


def premul_to_yuv(pix_fmt: Optional[str], out_pix_fmt: Optional[str]) -> bool:
    """`check_premul_options`' `to_yuv` for a pair of format names: an RGB source whose output (`out_pix_fmt`, None = the
    source's) is not float."""
    src = parse_rgb_source(pix_fmt)
    out = parse_rgb_source(out_pix_fmt) if out_pix_fmt else src
    return src is not None and not (out is not None and out.floating)


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
    if has_prologue(side.depth, range_src, range_in, lut_depth):
        raise ValueError(f"{head} is not defined for a call with a prologue (range_src != range_in, or lut_depth other than the "
                         f"source's depth {side.depth}): such a call has no alpha to carry")
    return "yuv"


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


# ---------------------------------------------------------------- YUV in, RGB out
def parse_rgb_out(name: Optional[str]):
    """The RGB destination `name` of `LutEngine.apply_yuv_to_rgb`: a `PixFmt` of the gbr family (gbrp .. gbrp16le, gbrap*: three
    or four planes) or a packed `RgbSource` (a name of `_native.PACKED_FORMATS`: one [F,]H,W,C image).  ValueError for every
    other name, a float one included."""
    rgb = parse_rgb_source(name)
    if rgb is None:
        raise ValueError(f"'{name}' is not an RGB output format (gbrp .. gbrp16le, gbrap*, or a packed name such as rgb24, "
                         f"rgba, rgb48le)")
    if rgb.floating:
        raise ValueError(f"a float output ('{name}') from a YUV source is not supported: the LUT runs on integer codes at the "
                         f"output's depth")
    return rgb if rgb.packed else parse_pix_fmt(name)


def _yuv2rgb_sides(pix_fmt: Optional[str], out_pix_fmt: Optional[str], head: str):
    """The format checks of a YUV -> RGB pass called `head`: a planar YUV source (yuva* too), an RGB
    destination, no alpha into a 4-component packed one.  Returns (source `PixFmt`, destination `PixFmt` | packed `RgbSource`)."""
    if not pix_fmt:
        raise ValueError(f"{head} needs pix_fmt")
    name = pix_fmt.replace("yuvj", "yuv")
    if parse_semi_fmt(name) is not None:
        raise ValueError(f"{head} takes planar YUV sources: '{pix_fmt}' is a semi-planar container")
    if parse_packed_yuv_fmt(name) is not None or name in _PACKED_YUV_UNSUPPORTED:
        raise ValueError(f"{head} takes planar YUV sources: '{pix_fmt}' is a packed 4:2:2 container")
    if parse_v210_fmt(name) is not None:
        raise ValueError(f"{head} takes planar YUV sources: '{pix_fmt}' is a v210 container")
    if parse_rgb_source(name) is not None:
        raise ValueError(f"{head} takes planar YUV sources: '{pix_fmt}' is an RGB format (use apply_rgb / apply_packed)")
    fin = parse_pix_fmt(name)
    fout = parse_rgb_out(out_pix_fmt)
    if fin.alpha and isinstance(fout, RgbSource) and fout.ncomp == 4:
        raise ValueError(f"alpha from '{pix_fmt}' into the packed destination '{out_pix_fmt}' is not supported yet (a follow-up): "
                         f"use gbrap* to carry alpha, or a yuv* name / a 3-component destination to drop it")
    return fin, fout


#: what `apply_yuv_to_rgb` does not take, by keyword -> (its neutral value, what the refusal calls it)
_YUV2RGB_NOT_TAKEN = {
    "chroma_loc": (None, "sited chroma resampling (chroma_loc)"), "dither": ("none", "dither"),
    "engine_dither": (None, "dither (engine_dither)"), "out_size": (None, "a resize (out_size / resolution)"),
    "resize_chunk": (None, "a resize (out_size / resolution)"),
    "alpha_mode": ("straight", "alpha_mode='premultiplied'"), "cdl": (None, "an ASC CDL (cdl)"), "lut1d": (None, "a 1D LUT (lut1d)"),
    "stages": (None, "a stage stack (stages)"), "strength": (None, "a LUT strength (strength)"),
    "strength_keys": (None, "a LUT strength (strength_keys)"), "matte": (None, "a matte (matte)"),
    "out2_pix_fmt": (None, "a second output (out2_pix_fmt / second_pix_fmt)"), "cube2": (None, "a second LUT (cube2)"),
    "lut2": (False, "a second LUT (cube2)"), "interp2": (None, "a second LUT (interp2)"),
}


def check_yuv2rgb_options(pix_fmt: Optional[str], out_pix_fmt: Optional[str], **options):
    """The checks every layer makes of a YUV -> RGB call before any GPU work: a planar YUV source (yuva* too)
    and an RGB destination; ValueError, naming it, for every option the pass does not take (`_YUV2RGB_NOT_TAKEN`: a keyword at its
    neutral value passes), for a semi-planar, packed 4:2:2 or v210 source, and for alpha into a 4-component packed destination;
    TypeError for a keyword nothing knows.  Returns (source `PixFmt`, destination `PixFmt` | packed `RgbSource`)."""
    head = "YUV in with RGB out (apply_yuv_to_rgb)"
    for k, v in options.items():
        if k not in _YUV2RGB_NOT_TAKEN:
            raise TypeError(f"apply_yuv_to_rgb() got an unexpected keyword argument '{k}'")
        neutral, what = _YUV2RGB_NOT_TAKEN[k]
        if (v is not None) if neutral is None else (v != neutral):
            raise ValueError(f"{what} is not supported with {head}")
    return _yuv2rgb_sides(pix_fmt, out_pix_fmt, head)


# ---------------------------------------------------------------- the stage stack on RGB sources
def check_rgb_stack_options(pix_fmt: Optional[str], out_pix_fmt: Optional[str] = None, *, stages, cdl: bool = False,
                            lut: bool = True, lut2: bool = True, lut1d: bool = True, prelut: bool = False,
                            rgb_matrix: bool = False, dither: str = "none", chroma_loc: Optional[str] = None, out_size=None,
                            alpha_mode: str = "straight", out2_pix_fmt: Optional[str] = None, variant: Optional[str] = None,
                            strength=None, matte=None, intermediate_pix_fmt: Optional[str] = None):
    """The checks every layer makes of a stage stack on an RGB source before any GPU work, the one copy of its
    refusals: everything `check_stage_list` refuses; a source that is not integer RGB (`gbrp*`, `gbrap*`, a packed name) -- a float
    one by name; a destination that is neither planar YUV (4:2:0 / 4:2:2 / 4:4:4, yuva* included) nor `gbrp*` / `gbrap*` at the
    source's depth -- a packed one, and a gbrp one of another depth, by name; a packed source without `out_pix_fmt`; the
    full-range two-stage composition (`intermediate_pix_fmt`); dither, out_size, chroma_loc; strength / matte; premultiplied
    alpha; a second output; the vec_lds variant, and vec_global where the names of the call already say that the vector kernel
    cannot take it (a pyramid / prism stage, an 8-bit source written as 16-bit words).  `out_pix_fmt` None means `gbrp*` at the
    source's depth.
    Returns (parsed stages, source `RgbSource`, destination `PixFmt`)."""
    tail = RGB_STACK_TAIL
    st = check_stage_list(stages, cdl=cdl, lut=lut, lut2=lut2, lut1d=lut1d, prelut=prelut, rgb_matrix=rgb_matrix)
    fin = parse_rgb_source(pix_fmt)
    if fin is None:
        raise ValueError(f"{tail} takes gbrp*, gbrap* or packed RGB sources: '{pix_fmt}' is not an RGB format (planar YUV goes "
                         f"through stages / apply_yuv_stack)")
    if fin.floating:
        raise ValueError(f"a float source ('{pix_fmt}') is not supported with {tail}: the list runs on integer codes at the "
                         f"source's depth")
    if out_pix_fmt is None:
        if fin.packed:
            raise ValueError(f"a packed source ('{pix_fmt}') with {tail} needs out_pix_fmt: a planar YUV name, or gbrp* at the "
                             f"source's depth ({fin.depth} bit)")
        fout = PixFmt(fin.name, "gbr", fin.depth, 0, 0, True, fin.nplanes == 4)
    else:
        out = parse_rgb_source(out_pix_fmt)
        if out is not None and out.packed:
            raise ValueError(f"a packed RGB destination ('{out_pix_fmt}') is not supported with {tail}: the destination is planar "
                             f"YUV or gbrp* at the source's depth")
        if out is not None and out.floating:
            raise ValueError(f"a float destination ('{out_pix_fmt}') is not supported with {tail}")
        try:
            fout = parse_pix_fmt(out_pix_fmt.replace("yuvj", "yuv"))
        except ValueError:
            raise ValueError(f"'{out_pix_fmt}' is not a destination of {tail}: planar YUV (yuv420p .. yuv444p16le, yuva*) or "
                             f"gbrp* / gbrap* at the source's depth") from None
        if fout.family == "gbr" and fout.depth != fin.depth:
            raise ValueError(f"a gbrp destination of another depth ('{out_pix_fmt}', {fout.depth} bit, from '{pix_fmt}', "
                             f"{fin.depth} bit) is not supported with {tail}: the final codes are stored at the source's depth")
    _refuse_stack_options(tail, "RGB stack", variant, dict(
        intermediate_pix_fmt=intermediate_pix_fmt, dither=dither, out_size=out_size, chroma_loc=chroma_loc, strength=strength,
        matte=None if matte is False else matte, alpha_mode=alpha_mode, out2_pix_fmt=out2_pix_fmt),
        vector=(st, fin.depth, fout.depth, pix_fmt, fout.name))
    return st, fin, fout


# ---------------------------------------------------------------- the stage stack from YUV sources into RGB frames
def check_yuv2rgb_stack_options(pix_fmt: Optional[str], out_pix_fmt: Optional[str], *, stages, cdl: bool = False,
                                lut: bool = True, lut2: bool = True, lut1d: bool = True, prelut: bool = False,
                                rgb_matrix: bool = False, dither: str = "none", engine_dither: Optional[str] = None,
                                chroma_loc: Optional[str] = None, out_size=None, alpha_mode: str = "straight",
                                out2_pix_fmt: Optional[str] = None, variant: Optional[str] = None, strength=None, matte=None):
    """The checks every layer makes of a stage stack from a YUV source into an RGB frame before any GPU work,
    the one copy of its refusals: everything `check_stage_list` refuses; the format checks of `check_yuv2rgb_options` (a planar
    YUV source, yuva* too -- a semi-planar, packed 4:2:2 or v210 one by name; an integer RGB destination -- a float one by name;
    no alpha into a 4-component packed destination); chroma_loc, both dithers, out_size; strength / matte; premultiplied alpha;
    a second output; the vec_lds variant, and vec_global where the names of the call already say that the vector kernel cannot
    take it (a pyramid / prism stage, an 8-bit source written as 16-bit words).
    Returns (parsed stages, source `PixFmt`, destination `PixFmt` | packed `RgbSource`)."""
    tail = YUV2RGB_STACK_TAIL
    st = check_stage_list(stages, cdl=cdl, lut=lut, lut2=lut2, lut1d=lut1d, prelut=prelut, rgb_matrix=rgb_matrix)
    fin, fout = _yuv2rgb_sides(pix_fmt, out_pix_fmt, "the stage stack from YUV into RGB (apply_yuv_stack_to_rgb)")
    _refuse_stack_options(tail, "YUV -> RGB stack", variant, dict(
        chroma_loc=chroma_loc, dither=dither, engine_dither=engine_dither, out_size=out_size, strength=strength,
        matte=None if matte is False else matte, alpha_mode=alpha_mode, out2_pix_fmt=out2_pix_fmt),
        vector=(st, fin.depth, fout.depth, pix_fmt, fout.name))
    return st, fin, fout


# ---------------------------------------------------------------- the stage stack on semi-planar sides
SEMI_STACK_TAIL = "a stage stack on semi-planar frames (semi_stages)"

#: what every layer says when the list comes with another one
SEMI_STAGES_EXCLUSIVE = ("semi_stages and stages / rgb_stages / rgb_out_stages are mutually exclusive: semi_stages is the list of a "
                         "call with a semi-planar side, stages that of planar YUV on both sides, rgb_stages that of an RGB source, "
                         "rgb_out_stages that of a YUV source with rgb_out")

#: semi-planar names FFmpeg has that this path does not take: 4:4:4 pairs and big-endian containers
_SEMI_UNSUPPORTED = ("nv24", "nv42", "p410le", "p412le", "p416le", "p010be", "p012be", "p016be", "p210be", "p212be", "p216be",
                     "p410be", "p412be", "p416be")


def semi_stack_side(name: Optional[str], what: str):
    """One side of the stack on semi-planar frames: the `SemiFmt` of a semi-planar name or the `PixFmt` of a planar YUV one
    (yuvj* read as yuv*); ValueError, naming it, for a yuva*, packed 4:2:2, v210, RGB or float name and for a semi-planar name
    this path does not take (4:4:4 and big-endian ones)."""
    tail = SEMI_STACK_TAIL
    if name in _SEMI_UNSUPPORTED:
        raise ValueError(f"'{name}' is not supported with {tail}: a semi-planar side is 4:2:0 or 4:2:2, little-endian "
                         f"({', '.join(_native.SEMI_FORMATS)})")
    if parse_packed_yuv_fmt(name) is not None or name in _PACKED_YUV_UNSUPPORTED:
        raise ValueError(f"a packed 4:2:2 side ({what} '{name}') is not supported with {tail}")
    if parse_v210_fmt(name) is not None or name in _V210_UNSUPPORTED:
        raise ValueError(f"a v210 side ({what} '{name}') is not supported with {tail}")
    rgb = parse_rgb_source(name)
    if rgb is not None:
        kind = "a float" if rgb.floating else "an RGB"
        raise ValueError(f"{kind} side ({what} '{name}') is not supported with {tail}: both sides are YUV, planar or semi-planar")
    side = yuv_side(name)
    if getattr(side, "alpha", False):
        raise ValueError(f"alpha ({what} '{name}') is not supported with {tail}: semi-planar formats carry no alpha")
    return side


def check_semi_stack_options(pix_fmt: Optional[str], out_pix_fmt: Optional[str] = None, *, stages, cdl: bool = False,
                             lut: bool = True, lut2: bool = True, lut1d: bool = True, prelut: bool = False, dither: str = "none",
                             chroma_loc: Optional[str] = None, out_size=None, alpha_mode: str = "straight",
                             out2_pix_fmt: Optional[str] = None, variant: Optional[str] = None, strength=None,
                             precision: Optional[str] = None, matte=None, rgb_matrix: bool = False):
    """The checks every layer makes of a stage stack on semi-planar frames before any GPU work, the one copy of
    its refusals: a `matrix` stage or an RGB matrix; everything `check_stage_list` refuses; a side that is neither a semi-planar
    name of `_native.SEMI_FORMATS` nor planar YUV at 4:2:0 / 4:2:2 / 4:4:4 -- yuva*, packed 4:2:2, v210, RGB and float names, and
    4:4:4 or big-endian semi-planar ones, by name; both sides planar (that is `apply_yuv_stack`'s call); strength / matte; dither,
    chroma_loc, out_size; a second output; premultiplied alpha; the vec_lds variant, and vec_global where the names of the call
    already say that the vector kernel cannot take it (a pyramid / prism stage, an 8-bit source written as 16-bit words).  A
    `precision` other than strict is taken as the stack takes it without a strength: the pass runs strict.
    Returns (parsed stages, source side, destination side); a side is a `SemiFmt` or a planar `PixFmt`."""
    tail = SEMI_STACK_TAIL
    if rgb_matrix or "matrix" in [k for k, _m in parse_stages(stages)]:
        raise ValueError(f"stage 'matrix' is not supported with {tail}: the matrix stage has no semi-planar form")
    st = check_stage_list(stages, cdl=cdl, lut=lut, lut2=lut2, lut1d=lut1d, prelut=prelut)
    if not pix_fmt:
        raise ValueError(f"{tail} needs pix_fmt")
    fin = semi_stack_side(pix_fmt, "pix_fmt")
    fout = semi_stack_side(out_pix_fmt or pix_fmt, "out_pix_fmt")
    if not isinstance(fin, SemiFmt) and not isinstance(fout, SemiFmt):
        raise ValueError(f"both sides are planar: use apply_yuv_stack ('{pix_fmt}' -> '{out_pix_fmt or pix_fmt}' has no "
                         f"semi-planar side)")
    _refuse_stack_options(tail, "semi-planar stack", variant, dict(
        strength=strength, matte=None if matte is False else matte, dither=dither, chroma_loc=chroma_loc, out_size=out_size,
        out2_pix_fmt=out2_pix_fmt, alpha_mode=alpha_mode), vector=(st, fin.depth, fout.depth, pix_fmt, fout.name))
    return st, fin, fout


# ---------------------------------------------------------------- the stage stack on packed 4:2:2 / v210 frames
PACKED_STACK_TAIL = "a stage stack on packed 4:2:2 / v210 frames (packed_stages)"

#: what every layer says when the list comes with another one
PACKED_STAGES_EXCLUSIVE = ("packed_stages and stages / rgb_stages / rgb_out_stages / semi_stages are mutually exclusive: packed_stages "
                           "is the list of a call with a packed 4:2:2 or v210 side, stages that of planar YUV on both sides, rgb_stages "
                           "that of an RGB source, rgb_out_stages that of a YUV source with rgb_out, semi_stages that of a call with "
                           "a semi-planar side")


def packed_stack_side(name: Optional[str], what: str):
    """One side of the stack on capture frames: the `PackedYuvFmt` of a packed 4:2:2 name, the `V210Fmt` of v210 or the `PixFmt`
    of a planar YUV one (yuvj* read as yuv*); ValueError, naming it, for a yuva*, semi-planar, RGB or float name and for a packed
    name this path does not take (v210x, v410, packed 4:4:4 and big-endian ones)."""
    tail = PACKED_STACK_TAIL
    if name in _PACKED_YUV_UNSUPPORTED:
        raise ValueError(f"'{name}' is not supported with {tail}: packed YUV frames are taken as little-endian 4:2:2 "
                         f"({', '.join(_native.PACKED_YUV_FORMATS)})")
    if name in _V210_UNSUPPORTED:
        raise ValueError(f"'{name}' is not supported with {tail}: of this family only v210 is taken")
    if parse_semi_fmt(name) is not None or name in _SEMI_UNSUPPORTED:
        raise ValueError(f"a semi-planar side ({what} '{name}') is not supported with {tail}")
    rgb = parse_rgb_source(name)
    if rgb is not None:
        kind = "a float" if rgb.floating else "an RGB"
        raise ValueError(f"{kind} side ({what} '{name}') is not supported with {tail}: both sides are YUV, planar, packed 4:2:2 "
                         f"or v210")
    side = yuv_side(name)
    if getattr(side, "alpha", False):
        raise ValueError(f"alpha ({what} '{name}') is not supported with {tail}: packed 4:2:2 and v210 frames carry no alpha")
    return side


def check_packed_stack_options(pix_fmt: Optional[str], out_pix_fmt: Optional[str] = None, *, stages, cdl: bool = False,
                               lut: bool = True, lut2: bool = True, lut1d: bool = True, prelut: bool = False, dither: str = "none",
                               chroma_loc: Optional[str] = None, out_size=None, alpha_mode: str = "straight",
                               out2_pix_fmt: Optional[str] = None, variant: Optional[str] = None, strength=None,
                               precision: Optional[str] = None, matte=None, rgb_matrix: bool = False):
    """The checks every layer makes of a stage stack on packed 4:2:2 / v210 frames before any GPU work, the one
    copy of its refusals: a `matrix` stage or an RGB matrix; everything `check_stage_list` refuses; a side that is neither packed
    4:2:2, v210 nor planar YUV -- yuva*, semi-planar, RGB and float names, and v210x / v410 / packed 4:4:4 / big-endian ones, by
    name; both sides planar (that is `apply_yuv_stack`'s call); a packed 4:2:2 side together with a v210 side; a source that is not
    4:2:2 (the side rule of `apply_yuv` on these containers); strength / matte; dither, chroma_loc, out_size; a second output;
    premultiplied alpha; the vec_lds variant, and vec_global where the names of the call already say that the vector kernel
    cannot take it.  A `precision` other than strict is taken as the stack takes it without a strength: the pass runs strict.
    Returns (parsed stages, source side, destination side); a side is a `PackedYuvFmt`, a `V210Fmt` or a planar `PixFmt`."""
    tail = PACKED_STACK_TAIL
    if rgb_matrix or "matrix" in [k for k, _m in parse_stages(stages)]:
        raise ValueError(f"stage 'matrix' is not supported with {tail}: the matrix stage has no packed 4:2:2 / v210 form")
    st = check_stage_list(stages, cdl=cdl, lut=lut, lut2=lut2, lut1d=lut1d, prelut=prelut)
    if not pix_fmt:
        raise ValueError(f"{tail} needs pix_fmt")
    out_name = out_pix_fmt or pix_fmt
    fin = packed_stack_side(pix_fmt, "pix_fmt")
    fout = packed_stack_side(out_name, "out_pix_fmt")
    kinds = {type(s) for s in (fin, fout)}
    if not kinds & {PackedYuvFmt, V210Fmt}:
        raise ValueError(f"both sides are planar: use apply_yuv_stack ('{pix_fmt}' -> '{out_name}' has no packed 4:2:2 or v210 "
                         f"side)")
    if PackedYuvFmt in kinds and V210Fmt in kinds:
        raise ValueError(f"a packed 4:2:2 side together with a v210 side is not supported with {tail} ('{pix_fmt}' -> '{out_name}'): "
                         f"go through yuv422p10le")
    if fin.family != "yuv" or fout.family != "yuv":
        raise ValueError(f"packed 4:2:2 / v210 frames go with YUV formats on both sides ('{pix_fmt}' -> '{out_name}')")
    if (fin.csx, fin.csy) != (1, 0):
        short = "v210" if V210Fmt in kinds else "packed"
        raise ValueError(f"a {short} destination takes a 4:2:2 source: no chroma subsampling change into '{out_name}' "
                         f"('{pix_fmt}' -> '{out_name}')")
    _refuse_stack_options(tail, "packed 4:2:2 / v210 stack", variant, dict(
        strength=strength, matte=None if matte is False else matte, dither=dither, chroma_loc=chroma_loc, out_size=out_size,
        out2_pix_fmt=out2_pix_fmt, alpha_mode=alpha_mode), vector=(st, fin.depth, fout.depth, pix_fmt, fout.name))
    return st, fin, fout
