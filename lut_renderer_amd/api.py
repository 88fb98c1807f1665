"""`apply_lut`: the Python-side LUT-apply API with the reference's option vocabulary.

Where the reference hands a filter string to an ffmpeg child process
(/root/reference/src/lut_renderer/ffmpeg.py:195-247, :304-310, run at
task_manager.py:145-151), this applies the same chain to frames already resident in HBM:

    [scale=in_range=pc:out_range=R, format=<8-bit>]   full-range sources only
    (auto) YUV -> RGB at the negotiated depth          matrix from lut_input_matrix / colorspace
    lut3d=file=<cube>:interp=<mode>
    [zscale=dither=error_diffusion]                    option zscale_dither: the output quantisation is dithered
    [format=<pix_fmt>]                                 RGB -> YUV at the output depth

Options use the names and values of `ProcessingParams` (models.py:45-56) and `VideoInfo`
(media_info.py:25-34).  Unforced matrices fall back to BT.601, swscale's default for
untagged frames; the RGB->YUV side produces limited range, which is
what ffmpeg's auto-inserted scaler emits ahead of an encoder.
"""
from __future__ import annotations

import threading
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

from .cdl import as_cdl
from .rgbmatrix import as_rgb_matrix
from .cube import CubeLut, as_lut1d, read_cube, read_lut, read_lut1d
from .formats import (check_alpha_mode, check_cdl_options, check_chain_options, check_chroma_loc, check_container_options,
                      check_dual_options, check_lut1d_options, check_lut2, check_premul_options, check_stack_options,
                      PACKED_STAGES_EXCLUSIVE, SEMI_STAGES_EXCLUSIVE, check_packed_stack_options, check_rgb_stack_options, check_semi_stack_options, check_yuv2rgb_options, check_yuv2rgb_stack_options, implied_stages, packed_frame_width, parse_packed_yuv_fmt,
                      parse_pix_fmt, parse_rgb_source, parse_semi_fmt, parse_size, parse_stages, parse_v210_fmt, premul_to_yuv,
                      packed_stack_side, refuse_alpha_resize, semi_stack_side, source_bit_depth, v210_frame_width, yuv_side)
from .params import ProcessingParams, VideoInfo
from .plan import LutPlan, output_color_tags, resolve_lut_plan

#: FFmpeg lut3d has no "cubic"; the reference whitelists it anyway (ffmpeg.py:243) and ffmpeg
#: would reject the filtergraph.  The engine mirrors that as an error.
_ENGINE_INTERP = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")

_lut_cache: Dict[tuple, object] = {}
# engines apply_lut creates for itself, kept per device tuple: a context holds a stream, the device lattice and the
# kernels' work queue, and the reference calls the path once per task, not once per frame
_engine_cache: Dict[Tuple[int, ...], object] = {}
_cache_lock = threading.Lock()      # guards the two dictionaries; each engine carries its own lock for the calls on it


def _cached_engine(devices: Tuple[int, ...]):
    from .engine import LutEngine
    from .multigpu import LutEngineGroup
    with _cache_lock:
        eng = _engine_cache.get(devices)
        if eng is None:
            eng = LutEngine(devices[0]) if len(devices) == 1 else LutEngineGroup(devices)
            _engine_cache[devices] = eng
        return eng


def close_cached_engines() -> None:
    """Destroy the contexts `apply_lut` keeps between calls (also registered with atexit)."""
    with _cache_lock:
        engines = list(_engine_cache.values())
        _engine_cache.clear()
    for eng in engines:
        try:
            with eng._lock:
                eng.close()
        except Exception:
            pass


import atexit  # noqa: E402
atexit.register(close_cached_engines)


def _cached_cube(path: Path, reader=read_lut) -> CubeLut:
    """The parsed file, kept per (path, mtime, size); `reader` = `read_lut1d` for a 1D LUT file (a `Lut1D`; a path names one kind)."""
    st = path.stat()
    key = (str(path), st.st_mtime, st.st_size) if reader is read_lut else (str(path), st.st_mtime, st.st_size, "1d")
    with _cache_lock:
        lut = _lut_cache.get(key)
    if lut is None:
        lut = reader(path)                     # parsed outside the lock: two tasks may parse two files at once
        with _cache_lock:
            if len(_lut_cache) >= 16:          # up to 16 concurrent tasks (task_manager.py:229-235), each with its own LUT
                _lut_cache.clear()
            lut = _lut_cache.setdefault(key, lut)
    return lut


def _parsed_lut(cube) -> Optional[CubeLut]:
    """None, the parsed LUT that was given, or the file's -- parsed once and kept, so that the same object comes back the next
    time and the engine's device copy stands."""
    return None if cube is None else cube if isinstance(cube, CubeLut) else _cached_cube(Path(cube))


def engine_call_for(plan: LutPlan, pix_fmt: str, out_pix_fmt: Optional[str] = None, alpha_mode: str = "straight",
                    rgb_out: Optional[str] = None, semi_stack: bool = False, packed_stack: bool = False) -> dict:
    """Translate a LutPlan into keyword arguments of LutEngine.apply_yuv (`pix_fmt` / `out_pix_fmt` planar YUV -- yuva* too, DESIGN.md
    3.16: without `out_pix_fmt` the source's format, alpha included, is kept; a named output without alpha drops it, one with alpha
    on a source without is filled opaque; the full-range prologue's default output stays the 8-bit yuv4xxp -- , semi-planar names
    such as nv12 / p010le, DESIGN.md 3.11, or packed 4:2:2 names such as uyvy422 / y210le; `out_pix_fmt` defaults
    to the source's own format) -- or, for an RGB `pix_fmt` (gbrp* / a packed name / a
    float name) with a YUV `out_pix_fmt`, of LutEngine.apply_rgb_to_yuv (`is_rgb_call(kw)` tells the two apart).  A float
    `pix_fmt` (gbrpf32le / gbrapf32le) without `out_pix_fmt`, or with a float one, stays float:
    `is_float_out_call(kw)`, and LutEngine.apply_rgb_float takes `kw["interp"]`.
    alpha_mode="premultiplied"  adds `alpha_mode` to the arguments of a yuva* -> planar YUV call or of a gbrapf32le
    float call and is a ValueError for every other call; "straight" (the default) returns what it always returned.
    `rgb_out` (gbrp .. gbrp16le, gbrap*, or a packed name) asks for an RGB output from a planar YUV `pix_fmt`: the
    arguments are then those of LutEngine.apply_yuv_to_rgb (`is_rgb_out_call(kw)`), the LUT runs at that format's depth, and a plan
    with the full-range prologue (which lands at 8 bit) takes an 8-bit `rgb_out` only.  Not together with `out_pix_fmt`.
    `semi_stack`: the call is `LutEngine.apply_yuv_stack_semi`'s -- the sides are checked as that pass takes them
    (semi-planar or planar YUV, any pair of subsamplings) and not as `apply_yuv` does.
    `packed_stack`: the call is `LutEngine.apply_yuv_stack_packed`'s -- the sides are checked as that pass takes
    them (packed 4:2:2, v210 or planar YUV)."""
    if plan.interp not in _ENGINE_INTERP:
        raise ValueError(f"lut3d has no interpolation mode '{plan.interp}'")
    premul = check_alpha_mode(alpha_mode)
    if rgb_out is not None:
        if out_pix_fmt:
            raise ValueError(f"rgb_out ('{rgb_out}') and out_pix_fmt ('{out_pix_fmt}') are mutually exclusive: a call has one output")
        _fin, fout = check_yuv2rgb_options(pix_fmt, rgb_out, alpha_mode=alpha_mode)
        kw = dict(pix_fmt=pix_fmt.replace("yuvj", "yuv"), out_pix_fmt=rgb_out, interp=plan.interp,
                  matrix_in=plan.matrix or "smpte170m")
        if plan.prologue:
            # scale=in_range=pc:out_range=R, format=yuv4xxp (8 bit) ahead of lut3d: the LUT, and so the output, is at 8 bit
            if fout.depth != 8:
                raise ValueError(f"a source flagged full range is converted to 8 bit ahead of lut3d: it takes an 8-bit rgb_out "
                                 f"(gbrp, rgb24, rgba, ..), not '{rgb_out}'")
            kw.update(range_src="pc", range_in=plan.prologue_out_range)
        else:
            kw.update(range_src="tv", range_in="tv")
        return kw
    if semi_stack:
        # (the sides of the stack on semi-planar frames: its own refusals of a name, and any pair of subsamplings)
        semi_stack_side(pix_fmt, "pix_fmt")
        semi_stack_side(out_pix_fmt or pix_fmt, "out_pix_fmt")
    if packed_stack:
        # (the sides of the stack on packed 4:2:2 / v210 frames: its own refusals of a name)
        packed_stack_side(pix_fmt, "pix_fmt")
        packed_stack_side(out_pix_fmt or pix_fmt, "out_pix_fmt")
    rgb = parse_rgb_source(pix_fmt)
    if premul and rgb is not None:
        check_premul_options(pix_fmt, out_pix_fmt, to_yuv=premul_to_yuv(pix_fmt, out_pix_fmt))
    if rgb is not None and rgb.floating:
        out = parse_rgb_source(out_pix_fmt) if out_pix_fmt else rgb
        if out is not None and out.floating:
            # float in, float out: lut3d's float path alone, no format= behind it
            if plan.prologue:
                raise ValueError("a float source flagged full range has no float output: the reference converts it to 8-bit YUV "
                                 "ahead of lut3d; name a YUV out_pix_fmt")
            if out.nplanes > rgb.nplanes:
                raise ValueError(f"'{pix_fmt}' has no alpha plane to carry into '{out_pix_fmt}'")
            kw = dict(pix_fmt=pix_fmt, out_pix_fmt=out.name, interp=plan.interp)
            if premul:
                kw["alpha_mode"] = alpha_mode
            return kw
        if out is not None or parse_pix_fmt(out_pix_fmt.replace("yuvj", "yuv")).family != "yuv":
            raise ValueError(f"a float RGB source takes a float or a planar YUV out_pix_fmt, not '{out_pix_fmt}'")
    if rgb is not None:
        # an RGB source: lut3d runs on the RGB frame itself, then format=<pix_fmt>.  The engine has no encoder to
        # negotiate an output format with, so the caller names it.
        if not out_pix_fmt:
            raise ValueError("apply_lut takes planar YUV frames, or an RGB source with a YUV out_pix_fmt; for RGB output use "
                             "LutEngine.apply_rgb for gbrp planes / LutEngine.apply_packed for packed images")
        if parse_rgb_source(out_pix_fmt) is not None or parse_pix_fmt(out_pix_fmt.replace("yuvj", "yuv")).family != "yuv":
            raise ValueError(f"an RGB source takes a planar YUV out_pix_fmt, not '{out_pix_fmt}'; for RGB output use "
                             "LutEngine.apply_rgb for gbrp planes / LutEngine.apply_packed for packed images")
        kw = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, interp=plan.interp, matrix_out=plan.matrix or "smpte170m",
                  range_out="tv")
        if plan.prologue:
            # scale=in_range=pc:out_range=R, format=yuv4xxp (8 bit) AHEAD of lut3d: the two-stage composition of 3.9 point 6
            kw.update(intermediate_pix_fmt=plan.intermediate_pix_fmt, prologue_out_range=plan.prologue_out_range)
        return kw
    # a semi-planar source or output (nv12, p010le, ..) is the same chain on another container
    # (so is a packed 4:2:2 one: uyvy422, y210le, ..)
    # (and v210)
    if not semi_stack and not packed_stack:
        check_container_options(pix_fmt, out_pix_fmt, kinds=("v210", "packed"))     # names the packings this path does not take
    semi_src = parse_semi_fmt(pix_fmt) or parse_packed_yuv_fmt(pix_fmt) or parse_v210_fmt(pix_fmt)
    src = semi_src or parse_pix_fmt(pix_fmt)
    if src.family != "yuv":
        raise ValueError("apply_lut takes planar YUV frames; use LutEngine.apply_rgb for gbrp planes")
    if out_pix_fmt and parse_rgb_source(out_pix_fmt) is not None:
        raise ValueError(f"YUV frames with an RGB out_pix_fmt ('{out_pix_fmt}') are not supported: nothing in the reference's "
                         "chain produces them")
    matrix = plan.matrix or "smpte170m"
    kw = dict(pix_fmt=pix_fmt.replace("yuvj", "yuv"), interp=plan.interp, matrix_in=matrix, matrix_out=matrix,
              range_out="tv")
    if plan.prologue:
        # scale=in_range=pc:out_range=R , format=yuv4xxp (8 bit): the LUT then runs at 8 bit
        kw.update(range_src="pc", range_in=plan.prologue_out_range, lut_depth=8)
        # (the plan reads the subsampling off a yuv4xx name; a semi-planar source names its planar 8-bit twin itself)
        default_out = plan.intermediate_pix_fmt if semi_src is None else f"yuv{'420' if semi_src.csy else '422'}p"
    else:
        kw.update(range_src="tv", range_in="tv", lut_depth=src.depth)
        default_out = kw["pix_fmt"]
    kw["out_pix_fmt"] = out_pix_fmt or default_out
    if not semi_stack and not packed_stack:
        check_container_options(kw["pix_fmt"], kw["out_pix_fmt"])    # (one subsampling on both sides of a semi-planar call)
    if premul:
        check_premul_options(kw["pix_fmt"], kw["out_pix_fmt"], range_src=kw["range_src"], range_in=kw["range_in"],
                             lut_depth=kw["lut_depth"])
        kw["alpha_mode"] = alpha_mode
    return kw


def dual_call_for(kw: dict, second_pix_fmt: str, chroma_loc: Optional[str] = None, out_size=None) -> dict:
    """Keyword arguments of LutEngine.apply_yuv_dual from those `engine_call_for` returned for the first output
    (with `dither` filled in, if any) and the name of the second one.  ValueError for an RGB / float / semi-planar / packed side,
    dither, chroma_loc and a resize."""
    check_dual_options(kw.get("pix_fmt"), kw.get("out_pix_fmt"), second_pix_fmt, kw.get("dither", "none"), chroma_loc, out_size)
    dual = {k: v for k, v in kw.items() if k != "dither"}
    dual["out2_pix_fmt"] = second_pix_fmt.replace("yuvj", "yuv")
    return dual


def chain_call_for(kw: dict, interp2: Optional[str] = None, chroma_loc: Optional[str] = None, out_size=None,
                   second_pix_fmt: Optional[str] = None) -> dict:
    """Keyword arguments of LutEngine.apply_yuv_chain from those `engine_call_for` returned (with `dither` filled
    in, if any).  `interp2` goes through the whitelist / fallback `interp` went through (plan.py; None = the first LUT's mode).
    ValueError for an alpha / RGB / float / semi-planar / packed / v210 side, dither, chroma_loc, a resize and a second output."""
    from .plan import INTERP_WHITELIST
    check_chain_options(kw.get("pix_fmt"), kw.get("out_pix_fmt"), kw.get("dither", "none"), chroma_loc, out_size, second_pix_fmt)
    chain = {k: v for k, v in kw.items() if k != "dither"}
    if interp2 is not None:
        mode = interp2 if interp2 in INTERP_WHITELIST else "tetrahedral"
        if mode not in _ENGINE_INTERP:
            raise ValueError(f"lut3d has no interpolation mode '{mode}'")
        chain["interp2"] = mode
    return chain


def is_rgb_call(kw: dict) -> bool:
    """True when `engine_call_for` returned arguments of `apply_rgb_to_yuv` (an RGB source)."""
    return parse_rgb_source(kw.get("pix_fmt")) is not None


def is_rgb_out_call(kw: dict) -> bool:
    """True when `engine_call_for` returned arguments of `apply_yuv_to_rgb` (a YUV source with `rgb_out`)."""
    return parse_rgb_source(kw.get("pix_fmt")) is None and parse_rgb_source(kw.get("out_pix_fmt")) is not None


def is_float_out_call(kw: dict) -> bool:
    """True when `engine_call_for` returned a float source with a float output (LutEngine.apply_rgb_float)."""
    out = parse_rgb_source(kw.get("out_pix_fmt"))
    return out is not None and out.floating


def resolve_engine_dither(engine_dither: str, dither: str = "none") -> str:
    """The `dither` keyword of an engine call for the engine setting `engine_dither` beside the one
    `zscale_dither` selected: "blue_noise", or ValueError for an unknown value or for two dithers at once."""
    if engine_dither != "blue_noise":
        raise ValueError(f"unknown engine_dither '{engine_dither}' (blue_noise)")
    if dither == "error_diffusion":
        raise ValueError("two dithers were asked for: engine_dither='blue_noise' and zscale_dither='error_diffusion'")
    return "blue_noise"


def _stack_resources(st, cube, cube2, interp2, lut1d, interp1d, cdl, cdl_id, rgb_matrix, engine):
    """What `apply_lut(stages=)` and `apply_lut(rgb_stages=)` load for the parsed list `st`, with the caches the single-feature
    routes use: a stage for every file given, then (lattice | None, second lattice | None, 1D LUT | None, Cdl | None, RgbMatrix |
    None, `held(name)` -- what the engine of the call already holds -- , whether the first lattice carries a prelut)."""
    from . import _native
    kinds = [k for k, _m in st]
    if interp1d not in _native.INTERP1D:
        raise ValueError(f"lut1d has no interpolation mode '{interp1d}' ({' | '.join(_native.INTERP1D)})")
    for name, given, kind in (("cube", cube, "lut3d"), ("cube2", cube2, "lut3d2"), ("lut1d", lut1d, "lut1d"), ("cdl", cdl, "cdl")):
        if given is not None and kind not in kinds:
            raise ValueError(f"{name} is given and the stage list has no '{kind}' stage")
    if interp2 is not None and "lut3d2" not in kinds:
        raise ValueError("interp2 is the mode of the second LUT: the stage list has no 'lut3d2' stage")
    if cdl is None and cdl_id is not None:
        raise ValueError("cdl_id names a correction inside a CDL file: it needs cdl")
    lut, lut2 = _parsed_lut(cube), _parsed_lut(cube2)
    check_lut2(lut2)
    if lut1d is not None:
        lut1d = _cached_cube(Path(lut1d), read_lut1d) if isinstance(lut1d, (str, Path)) and Path(lut1d).is_file() else as_lut1d(lut1d)
    if cdl is not None:
        cdl = as_cdl(cdl, cdl_id)
    rgb_matrix = as_rgb_matrix(rgb_matrix)
    first = engine.engines[0] if engine is not None and hasattr(engine, "engines") else engine
    held = lambda name: bool(getattr(first, name, 0))                                  # noqa: E731
    prelut = getattr(lut, "prelut", None) is not None if lut is not None else held("_has_prelut")
    return lut, lut2, lut1d, cdl, rgb_matrix, held, prelut


def _stack_upload(eng, lut, lut2, lut1d, interp1d, precision) -> None:
    """The uploads and the precision of one task of `apply_lut`, under the engine's lock, and the one place that reads the
    engine's `_applied_*` markers: a resource the engine took from the same parsed object last time (the 1D LUT: and in the same
    mode) stands, its device copy with it; the engine's own setters clear the markers.  None uploads nothing."""
    if lut is not None and eng._applied_lut is not lut:
        eng.set_lut(lut)
        eng._applied_lut = lut
    if lut2 is not None and eng._applied_lut2 is not lut2:
        eng.set_lut2(lut2)
        eng._applied_lut2 = lut2
    if lut1d is not None:
        had = eng._applied_lut1d
        if not (had is not None and had[0] is lut1d and had[1] == interp1d):
            eng.set_lut1d(lut1d, interp1d)
            eng._applied_lut1d = (lut1d, interp1d)
    if eng.precision != precision:
        eng.set_precision(precision)


def _stack_route(planes, out, check, entry: str, names, listed, interp, cube, cube2, interp2, lut1d, interp1d, cdl, cdl_id, rgb_matrix,
                 engine, devices, precision, refusable: dict, call):
    """The one route behind `apply_lut`'s three stage lists -- `stages` (DESIGN.md 3.21 .. 3.23, 3.25), `rgb_stages` (3.26) and
    `rgb_out_stages` (3.27): parse `listed` with `interp` / `interp2` as the modes of the lut3d stages that spell none, load what
    it names with the caches the single-feature routes use (`_stack_resources`), make the family's `check` of the two format
    `names` with `refusable` -- the options of the call the pass does not take, or words its messages for, by the check's
    keyword -- and then, under the engine's lock, upload, set the precision and call the engine's `entry` with the parsed list,
    the CDL and `call()`: the family's other keywords, made behind the check.  The matrix travels when there is one, or where
    `call()` names `rgb_matrix` already."""
    from .plan import INTERP_WHITELIST
    mode2 = None if interp2 is None else interp2 if interp2 in INTERP_WHITELIST else "tetrahedral"
    st = parse_stages(listed, interp=interp, interp2=mode2)
    lut, lut2, lut1d, cdl, rgb_matrix, held, prelut = _stack_resources(st, cube, cube2, interp2, lut1d, interp1d, cdl, cdl_id,
                                                                      rgb_matrix, engine)
    if precision not in ("strict", "fast", "fma32"):
        raise ValueError(f"unknown precision '{precision}' (strict | fast | fma32)")
    check(*names, stages=st, cdl=cdl is not None, lut=lut is not None or held("n"), lut2=lut2 is not None or held("n2"),
          lut1d=lut1d is not None or held("n1d"), prelut=prelut, rgb_matrix=rgb_matrix is not None, **refusable)
    kw = dict(call(), stages=st, cdl=cdl)
    if rgb_matrix is not None or "rgb_matrix" in kw:
        kw["rgb_matrix"] = rgb_matrix
    own = engine is None
    eng = engine if engine is not None else _cached_engine(devices)
    with eng._lock:                 # uploads, precision and launch of ONE task, as in apply_lut
        _stack_upload(eng, lut, lut2, lut1d, interp1d, precision)
        result = getattr(eng, entry)(planes, out, **kw)
        if own:
            eng.sync()
    return result


def apply_lut(planes: Sequence, *, cube, interp: str = "tetrahedral", pix_fmt: str, width: Optional[int] = None,
              height: Optional[int] = None, input_matrix: str = "auto", colorspace: Optional[str] = None,
              color_range: Optional[str] = None, output_tags: str = "bt709", out_pix_fmt: Optional[str] = None,
              zscale_dither: str = "none", out: Optional[Sequence] = None, engine=None,
              devices: Sequence[int] = (0,), precision: str = "strict", chroma_loc: Optional[str] = None,
              resolution: Optional[str] = None, second_pix_fmt: Optional[str] = None, engine_dither: Optional[str] = None,
              cube2=None, interp2: Optional[str] = None, alpha_mode: str = "straight", cdl=None, cdl_id: Optional[str] = None,
              lut1d=None, interp1d: str = "linear", stages=None, strength=None, matte=None, matte_depth: Optional[int] = None,
              matte_invert: bool = False, rgb_out: Optional[str] = None, rgb_matrix=None, rgb_stages=None, rgb_out_stages=None,
              semi_stages=None, packed_stages=None):
    """Apply `cube` to planar YUV frames on the GPU.  `planes` = (Y, Cb, Cr) torch tensors on the
    engine's device, each [H,W] or [F,H,W].  A semi-planar `pix_fmt` / `out_pix_fmt` (nv12, nv21, nv16, p010le .. p216le; DESIGN.md
    3.11) makes that side (Y, CbCr): two tensors, the chroma one [..., ch, 2 * cw]; same subsampling on both sides, no dither,
    chroma_loc or resolution.  A packed 4:2:2 `pix_fmt` / `out_pix_fmt` (yuyv422, uyvy422, yvyu422, y210le, y212le, y216le;
    DESIGN.md 3.12) makes that side ONE tensor [..., h, 4 * ceil(w / 2)], bare or in a one-element list (`width` names an odd
    width); on the same terms, and a packed source may go to planar 4:2:0 / 4:4:4.  `pix_fmt` / `out_pix_fmt` = "v210" (DESIGN.md
    3.14) makes that side ONE int32 tensor [..., h, 32 * ceil(w / 48)] of 32-bit words, on the terms of a packed side; `width` is
    required when no planar side tells it, and `out_pix_fmt` defaults to v210.  With an RGB `pix_fmt` (gbrp* or a packed name such as rgb24) and a YUV
    `out_pix_fmt` (required then), `planes` is the three gbrp planes (G, B, R) or the one [F,]H,W,C packed tensor and the
    chain is lut3d on the RGB frame, then RGB -> YUV.  `pix_fmt` = gbrpf32le / gbrapf32le takes float32 planes
    (DESIGN.md 3.10): with a YUV `out_pix_fmt` the same chain, without one (or with a float one) float planes come back, an alpha
    plane copied through (one device, no dither, no resolution).  Returns (planes_out, tags) where `tags` is the colour
    metadata the reference would write for this policy (None = inherit / none).

    `engine` may be a LutEngine (or LutEngineGroup) that already holds the lattice (then `cube` may be
    None).  Otherwise `devices` names the GPUs: one device -> one context; several -> a LutEngineGroup that
    splits the rows of every frame over them inside this one process (lattice copied GPU to GPU, one launch
    per device, no host wait between launches).  Contexts made here are kept for the next call
    (`close_cached_engines`) and are safe to share between the threads of a task pool: the engine's lock is held from
    the lattice upload to the launch.

    `precision` is an ENGINE setting, not one of the reference's (models.py:45-56 has no such field): "strict" (default)
    is the bit-exact restatement of FFmpeg's scalar C in fp32; "fast" allows the tolerance-bounded kernels whose lattice
    is fp16 (<= 1 code from strict at 8 and 10 bit) where they exist and silently runs strict elsewhere
    (`engine.last_kernel` ends in `,fast` when they ran); "fma32" keeps strict's fp32 lattice and fuses the blend's
    multiply-adds (<= 1 code from strict), on the same terms (`,fma32`).

    `engine_dither` is an engine setting too: None (default) leaves the quantisation to `zscale_dither`;
    "blue_noise" quantises every output sample against a 64 x 64 void-and-cluster mask inside the LUT pass -- no scratch, rows
    and frames independent (a LutEngineGroup row-shards it), always strict arithmetic.  It is not `zscale_dither`, which keeps
    the reference's meaning; asking for both dithers is a ValueError, and so is any other value.

    `chroma_loc` is an engine setting too: None (default) replicates chroma over its block before the LUT and takes the
    block mean after it; "left" | "center" | "topleft" (ffprobe's chroma_location) resample chroma bilinearly at that
    siting (always strict arithmetic, no in-place output, not with error-diffusion dither).

    `out_pix_fmt` may change the chroma subsampling (4:2:0 / 4:2:2 / 4:4:4 either way, DESIGN.md 3.8: the reference's final
    `format=` with another layout, e.g. its ProRes 422 master of a 4:2:0 source); `chroma_loc` cannot be combined with that.

    `resolution` is `ProcessingParams.resolution`, a "WxH" string as ffmpeg's `-s` takes it: the output planes are resized to
    that size on the GPU after everything else, and `out` must have that size.  One device only (no
    LutEngineGroup): a row-sharded resize would need halos between the devices.

    An alpha-carrying `pix_fmt` / `out_pix_fmt` (yuva420p .. yuva444p16le, gbrap .. gbrap16le) makes that side FOUR
    planes, the last one alpha at the luma size and the format's depth.  Alpha never meets the LUT: it is copied, converted to the
    output depth (nearest code), dropped when `out_pix_fmt` has none, or filled opaque when only `out_pix_fmt` has it; it is
    treated as straight (a premultiplied source gets the LUT on its premultiplied colour, as in ffmpeg's chain).  Planar sides
    only; `resolution` with an alpha-carrying output is a ValueError.

    `alpha_mode` is an engine setting: "straight" (default) is the paragraph above; "premultiplied" says the colour
    of a yuva* or gbrapf32le source is premultiplied by its alpha (OpenEXR by specification, ProRes 4444 elements usually): the
    colour is divided by alpha in front of lut3d and multiplied by it behind, inside the LUT pass, and the alpha plane is written
    as before.  Planar yuva* in with planar YUV out, or gbrapf32le in and out; no prologue (a full-range source), dither,
    chroma_loc, resolution, second output or second LUT, and no RGB source into YUV: each is a ValueError, as is any other value.

    `second_pix_fmt` asks for a SECOND planar YUV output from the same pass (the reference's "pro" mode: the
    yuv422p10le master and the delivery format): the return value is then ((planes_out, planes_out2), tags), and `out`, if
    given, is the pair (planes, planes2).  Planar YUV on all three sides; no RGB / float / semi-planar / packed side, no dither,
    chroma_loc or resolution.

    `cube2` (a path or a parsed CubeLut) applies a SECOND LUT behind the first in the same pass (ffmpeg's
    `lut3d=file=A,lut3d=file=B`: a technical LUT, then a look): the frame stays integer RGB at the LUT depth between the two and
    is converted to YUV once.  `interp2` is the second LUT's mode (None = `interp`).  Planar YUV without alpha on both sides; the
    second LUT carries no prelut; no dither, chroma_loc, resolution or second output.  `interp2` without `cube2` is a ValueError.

    `cdl` (a `cdl.Cdl`, or the path of a .cc / .ccc / .cdl file with `cdl_id` naming the correction in it) applies an ASC CDL --
    slope, offset, power per channel, then saturation -- to the integer RGB ahead of `cube`, in the same pass (DESIGN.md 3.19:
    the per-clip colour decision in front of the show LUT).  Planar YUV on both sides (yuva* with straight alpha included), a
    LutEngineGroup row-shards it, always strict arithmetic; the identity CDL gives the bits of the call without it.  No LUT with
    a .csp prelut, dither, chroma_loc, resolution, second output, second LUT, premultiplied alpha, RGB / float / semi-planar /
    packed / v210 side: each is a ValueError naming it.

    `lut1d` (a `cube.Lut1D`, or the path of a .cube file with LUT_1D_SIZE) applies a 1D LUT to the integer RGB ahead of `cube`, in
    the same pass (ffmpeg's `lut1d=file=A,lut3d=file=B`), with lut1d's mode `interp1d` (nearest | linear | cosine
    | cubic | spline).  `cube=None` together with `lut1d` is lut1d alone.  Planar YUV on both sides (yuva* with straight alpha
    included), a LutEngineGroup row-shards it, always strict arithmetic; the identity 1D LUT gives the bits of the call without
    it.  No dither, chroma_loc, resolution, CDL, second LUT, second output, premultiplied alpha, RGB / float / semi-planar /
    packed / v210 side: each is a ValueError naming it.  Without `lut1d` the function is unchanged.

    `stages` (a sequence or comma string: "lut3d", "lut3d2", "lut1d", "cdl", a lut3d stage optionally with its mode as ("lut3d",
    "trilinear") or "lut3d:trilinear") runs `cube`, `cube2`, `lut1d` (+ `interp1d`) and `cdl` (+ `cdl_id`) in that
    order in ONE pass (LutEngine.apply_yuv_stack); `interp` / `interp2` are the modes of the two lut3d stages that spell none.
    Only with `stages` may these be combined freely.  Every stage listed needs its file (or an `engine` that holds it) and every
    file given needs its stage: anything else is a ValueError.  Planar YUV on both sides (yuva* with straight alpha included), a
    LutEngineGroup row-shards it, always strict arithmetic; no dither, chroma_loc, resolution, second output or premultiplied
    alpha.  Without `stages` the function is unchanged.

    `strength` (the intensity / opacity control of a grade) mixes the graded pixel with the source behind the
    stages, as RGB codes, in the same pass: a number in [0, 1] for every frame, or a sequence / NumPy array / CPU tensor of one
    number per frame (a ramp).  1 gives the bits of the call without it, 0 the source through the two conversion stages.  It runs
    the stage stack: with `stages` that list, without it the list the other options imply -- lut1d, cdl, lut3d, lut3d2 in that
    order, so `cube` is ("lut3d",), `cdl` + `cube` ("cdl", "lut3d"), `lut1d` + `cube` ("lut1d", "lut3d"), `lut1d` alone ("lut1d",),
    `cube` + `cube2` ("lut3d", "lut3d2") -- on the stack's terms: whatever the stack refuses is refused with `strength`, in a
    message that names both, and so is a `precision` other than strict.  A plain `cube` with a strength therefore runs the
    stack's gather kernel, not the LDS-window tile kernel.  None (default) leaves every route as it is.

    `matte` (a key, a power window, a wipe) is a strength per pixel: a tensor on the engine's device at the luma
    size of the frame, [H,W] or [1,H,W] (a still for every frame) or [F,H,W], uint8 or int16 / uint16 with `matte_depth` (9..16);
    `matte_invert` takes Mm - a.  The strength of a pixel is `strength` (1 when not given) times its matte sample over Mm, applied
    in RGB ahead of the chroma mean.  It routes to the stack as a strength does, on the same terms, in messages that name the
    matte.  None (default) leaves every route as it is; `matte_depth` / `matte_invert` without a matte are a ValueError.

    `rgb_out` (a DPX / TIFF / PNG pull, a review still, a preview) writes RGB from planar YUV frames in the same
    pass: gbrp .. gbrp16le (three planes G, B, R come back), gbrap* (four, alpha from a yuva* source or opaque) or a packed name
    such as rgb24, rgba, bgra, rgb48le, rgba64le (one [F,]H,W,C tensor, a fourth component opaque); `out` is then such planes or
    such a tensor.  The LUT runs at that format's depth, as ffmpeg's `lut3d=...,format=<rgb fmt>` does; a source flagged full
    range takes an 8-bit `rgb_out` only.  A LutEngineGroup row-shards it; always strict arithmetic.  Not together with
    `out_pix_fmt`, and no dither, chroma_loc, resolution, premultiplied alpha, second output, second LUT, CDL, 1D LUT, stages,
    strength or matte, nor a semi-planar / packed 4:2:2 / v210 source: each is a ValueError naming it.  None (default) leaves
    every route as it is.

    `rgb_matrix` (a gamut conversion, a white-balance or channel-mixer trim, a channel swap) is the resource of a
    "matrix" stage of `stages`: an `rgbmatrix.RgbMatrix` (nine numbers row-major and an offset in unit floats) or the path of a
    .spimtx file.  The stage computes clamp(M * rgb + offset, 0, 1) on unit RGB where the list places it, e.g.
    stages="lut1d,matrix,lut3d".  It has no implied position: `rgb_matrix` without `stages`, without a matrix stage in it, or a
    matrix stage without `rgb_matrix` is a ValueError, and so is a strength or matte together with it.

    `rgb_stages` is `stages` for an RGB `pix_fmt` -- gbrp*, gbrap* or a packed name: the same lists, the same
    resources (`cube`, `cube2`, `lut1d`, `cdl`, `rgb_matrix`), run on the source's own codes in ONE pass
    (LutEngine.apply_rgb_stack) into a planar YUV `out_pix_fmt`, or into gbrp* / gbrap* at the source's depth -- the default for
    a planar source.  It is valid only with an RGB `pix_fmt`; `stages` together with it, a float source, a packed RGB output, a
    gbrp output of another depth, a source flagged full range, dither, resolution, chroma_loc, strength, matte, premultiplied
    alpha and a second output are ValueErrors naming them.

    `rgb_out_stages` is `stages` for a planar YUV `pix_fmt` with `rgb_out`: the same lists, the same resources
    (`cube`, `cube2`, `lut1d`, `cdl`, `rgb_matrix`), run at the depth of `rgb_out` in ONE pass (LutEngine.apply_yuv_stack_to_rgb)
    between the conversion to integer RGB and the stores, e.g. rgb_out="rgb48le", rgb_out_stages="lut1d,cdl,lut3d".  It needs
    `rgb_out`; `stages` or `rgb_stages` together with it, dither, resolution, chroma_loc, strength, matte, premultiplied alpha
    and a second output are ValueErrors naming them, and the format rules are those of `rgb_out`.  None (default) leaves every
    route as it is.

    `semi_stages` is `stages` for a call with a semi-planar side -- `pix_fmt`, `out_pix_fmt` or both one of nv12,
    nv21, nv16, p010le .. p216le, that side (Y, CbCr) as above: the same lists without the matrix stage, the same resources (`cube`,
    `cube2`, `lut1d`, `cdl`), in ONE pass (LutEngine.apply_yuv_stack_semi) with no de-interleave ahead of it and no interleave
    behind it; the other side may be planar 4:2:0 / 4:2:2 / 4:4:4 at 8..16 bit, so p010le -> yuv422p10le is one call.  `stages`,
    `rgb_stages` or `rgb_out_stages` together with it, two planar sides, a matrix stage, strength, matte, dither, resolution,
    chroma_loc, premultiplied alpha, yuva*, a second output and a packed / v210 / RGB / float side are ValueErrors naming them.

    `packed_stages` is `stages` for a call with a packed 4:2:2 or v210 side -- `pix_fmt`, `out_pix_fmt` or both one
    of yuyv422, uyvy422, yvyu422, y210le, y212le, y216le, or v210, that side ONE tensor as `apply_yuv` takes it (`width` names a
    width the rows cannot tell): the same lists without the matrix stage, the same resources (`cube`, `cube2`, `lut1d`, `cdl`), in
    ONE pass (LutEngine.apply_yuv_stack_packed) with no unpacking ahead of it and no packing behind it; a packed / v210 source may
    go to planar 4:2:2 / 4:2:0 / 4:4:4 at 8..16 bit, a packed / v210 output takes a 4:2:2 source.  Another stage list together
    with it, two planar sides, a packed 4:2:2 side together with a v210 side, a matrix stage, strength, matte, dither, resolution,
    chroma_loc, premultiplied alpha, yuva*, a second output and a semi-planar / RGB / float side are ValueErrors naming them."""
    devices = tuple(int(d) for d in devices)
    if not devices:
        raise ValueError("devices must name at least one GPU")
    out_size = None
    if resolution is not None:
        if not isinstance(resolution, str):
            raise ValueError(f"resolution is a 'WxH' string, got {resolution!r}")
        out_size = parse_size(resolution)
        from .multigpu import LutEngineGroup
        if isinstance(engine, LutEngineGroup) or (engine is None and len(devices) > 1):
            raise ValueError("resolution needs a single device")
    if rgb_stages is not None and stages is not None:
        raise ValueError("stages and rgb_stages are mutually exclusive: stages is the list of a YUV source, rgb_stages that of an "
                         "RGB source")
    if rgb_out_stages is not None:
        if rgb_out is None:
            raise ValueError("rgb_out_stages is the stage list of a YUV source written as RGB: it needs rgb_out")
        if stages is not None or rgb_stages is not None:
            raise ValueError("rgb_out_stages and stages / rgb_stages are mutually exclusive: stages is the list of a YUV source with "
                             "a YUV output, rgb_stages that of an RGB source, rgb_out_stages that of a YUV source with rgb_out")
    if semi_stages is not None and (stages is not None or rgb_stages is not None or rgb_out_stages is not None):
        raise ValueError(SEMI_STAGES_EXCLUSIVE)
    if packed_stages is not None and (stages is not None or rgb_stages is not None or rgb_out_stages is not None
                                      or semi_stages is not None):
        raise ValueError(PACKED_STAGES_EXCLUSIVE)
    if rgb_matrix is not None and stages is None and rgb_stages is None and rgb_out_stages is None and semi_stages is None \
            and packed_stages is None:
        raise ValueError("rgb_matrix needs stages: a matrix stage has no implied position (e.g. stages='lut1d,matrix,lut3d')")
    rgb_src = parse_rgb_source(pix_fmt)
    if rgb_stages is not None and rgb_src is None:
        raise ValueError(f"rgb_stages is the stage list of an RGB source (gbrp*, gbrap*, a packed name): '{pix_fmt}' is not one; "
                         f"a YUV source takes stages")
    if rgb_src is not None and rgb_src.packed:
        got_w, got_h = planes.shape[-2], planes.shape[-3]
    else:
        first = planes if hasattr(planes, "shape") else planes[0]
        pk_src = parse_packed_yuv_fmt(pix_fmt)
        if parse_v210_fmt(pix_fmt) is not None:                # (padded rows: `width`, or the planes of a planar `out`, tell it)
            fout = None if out_pix_fmt is None or parse_rgb_source(out_pix_fmt) is not None else yuv_side(out_pix_fmt)
            got_w = v210_frame_width(parse_v210_fmt(pix_fmt), fout if fout is not None else parse_v210_fmt(pix_fmt), planes,
                                     out if fout is not None and not hasattr(out, "shape") else None, width)
        else:
            got_w = packed_frame_width(pk_src, planes, width) if pk_src is not None else first.shape[-1]
        got_h = first.shape[-2]
    if width is not None and got_w != width or height is not None and got_h != height:
        raise ValueError("plane shape does not match width/height")
    params = ProcessingParams(lut_interp=interp, lut_input_matrix=input_matrix, lut_output_tags=output_tags,
                              zscale_dither=zscale_dither)
    info = VideoInfo(width=width, height=height, pix_fmt=pix_fmt, bit_depth=source_bit_depth(pix_fmt), colorspace=colorspace,
                     color_range=color_range)
    # (the plan only carries the path into the filter string / notes; a parsed CubeLut or an engine that already holds the
    # lattice has none)
    plan = resolve_lut_plan(params, cube if isinstance(cube, (str, Path)) else "engine.cube", info)
    # (what every stage-stack route loads from, and where it runs: `_stack_route`'s arguments behind the list and its modes)
    loaded = (cube, cube2, interp2, lut1d, interp1d, cdl, cdl_id, rgb_matrix, engine, devices, precision)
    # ffmpeg.py:305-307: any value other than "error_diffusion" leaves the chain without a dither filter
    zdither = "error_diffusion" if getattr(params, "zscale_dither", "none") == "error_diffusion" else "none"
    if rgb_stages is not None:
        # the stage stack on an RGB source: a route of its own
        dither = zdither if engine_dither is None else resolve_engine_dither(engine_dither, zdither)
        if rgb_out is not None:
            raise ValueError(f"rgb_out ('{rgb_out}') names the RGB output of a YUV source: with rgb_stages the output is out_pix_fmt")
        result = _stack_route(
            planes, out, check_rgb_stack_options, "apply_rgb_stack", (pix_fmt, out_pix_fmt), rgb_stages, interp, *loaded,
            dict(dither=dither, chroma_loc=chroma_loc, out_size=out_size, alpha_mode=alpha_mode, out2_pix_fmt=second_pix_fmt,
                 strength=strength, matte=matte, intermediate_pix_fmt=plan.intermediate_pix_fmt if plan.prologue else None),
            lambda: dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, rgb_matrix=None, matrix_out=plan.matrix or "smpte170m",
                         range_out="tv"))
        return result, output_color_tags(plan.output_policy)
    if rgb_out is not None:
        # YUV in, RGB out: a route of its own, with none of the options below
        if rgb_out_stages is not None:
            # ... with the stage stack between the conversion and the stores
            if out_pix_fmt:
                raise ValueError(f"rgb_out ('{rgb_out}') and out_pix_fmt ('{out_pix_fmt}') are mutually exclusive: a call has one "
                                 f"output")
            refusable = dict(dither=zdither, engine_dither=engine_dither, chroma_loc=chroma_loc, out_size=out_size,
                             alpha_mode=alpha_mode, out2_pix_fmt=second_pix_fmt, strength=strength, matte=matte)
            # (the matrix and the ranges are those `engine_call_for(rgb_out=)` gives the plan)
            result = _stack_route(
                planes, out, check_yuv2rgb_stack_options, "apply_yuv_stack_to_rgb", (pix_fmt, rgb_out), rgb_out_stages, interp,
                *loaded, refusable, lambda: dict({k: v for k, v in engine_call_for(plan, pix_fmt, None, "straight",
                                                                                  rgb_out=rgb_out).items() if k != "interp"},
                                                 rgb_matrix=None))
            return result, output_color_tags(plan.output_policy)
        kw = engine_call_for(plan, pix_fmt, out_pix_fmt, alpha_mode, rgb_out=rgb_out)
        check_yuv2rgb_options(pix_fmt, rgb_out, chroma_loc=chroma_loc, engine_dither=engine_dither, out_size=out_size,
                              dither=zdither, cdl=cdl, lut1d=lut1d, stages=stages, strength=strength, matte=matte, out2_pix_fmt=second_pix_fmt,
                              cube2=cube2, interp2=interp2)
        if precision not in ("strict", "fast", "fma32"):
            raise ValueError(f"unknown precision '{precision}' (strict | fast | fma32)")
        own = engine is None
        eng = engine if engine is not None else _cached_engine(devices)
        lut = _parsed_lut(cube)
        with eng._lock:             # upload, precision and launch of ONE task, as below
            _stack_upload(eng, lut, None, None, interp1d, precision)
            result = eng.apply_yuv_to_rgb(planes, out, **kw)
            if own:
                eng.sync()
        return result, output_color_tags(plan.output_policy)
    # (semi_stages / packed_stages: that pass's own sides; its check below is told the alpha mode)
    kw = engine_call_for(plan, pix_fmt, out_pix_fmt, "straight", semi_stack=True) if semi_stages is not None else \
        engine_call_for(plan, pix_fmt, out_pix_fmt, "straight", packed_stack=True) if packed_stages is not None else \
        engine_call_for(plan, pix_fmt, out_pix_fmt, alpha_mode)
    refuse_alpha_resize(kw.get("out_pix_fmt"), out_size)        # (the resize takes three planes)
    kw["dither"] = zdither if engine_dither is None else resolve_engine_dither(engine_dither, zdither)
    if precision not in ("strict", "fast", "fma32"):
        raise ValueError(f"unknown precision '{precision}' (strict | fast | fma32)")
    if cube2 is None and interp2 is not None:
        raise ValueError("interp2 is the mode of the second LUT: it needs cube2")
    if semi_stages is not None:
        # the stage stack on semi-planar sides: a route of its own, opt-in by name
        call = {k: v for k, v in kw.items() if k not in ("dither", "interp", "alpha_mode")}
        result = _stack_route(
            planes, out, check_semi_stack_options, "apply_yuv_stack_semi", (kw["pix_fmt"], kw["out_pix_fmt"]), semi_stages,
            kw.get("interp"), *loaded, dict(dither=kw["dither"], chroma_loc=chroma_loc, out_size=out_size, alpha_mode=alpha_mode,
                                            out2_pix_fmt=second_pix_fmt, strength=strength, precision=precision, matte=matte),
            lambda: call)
        return result, output_color_tags(plan.output_policy)
    if packed_stages is not None:
        # the stage stack on packed 4:2:2 / v210 sides: a route of its own, opt-in by name
        call = {k: v for k, v in kw.items() if k not in ("dither", "interp", "alpha_mode")}
        if width is not None:
            call["width"] = width
        result = _stack_route(
            planes, out, check_packed_stack_options, "apply_yuv_stack_packed", (kw["pix_fmt"], kw["out_pix_fmt"]), packed_stages,
            kw.get("interp"), *loaded, dict(dither=kw["dither"], chroma_loc=chroma_loc, out_size=out_size, alpha_mode=alpha_mode,
                                            out2_pix_fmt=second_pix_fmt, strength=strength, precision=precision, matte=matte),
            lambda: call)
        return result, output_color_tags(plan.output_policy)
    if "alpha_mode" in kw:
        check_premul_options(kw["pix_fmt"], kw["out_pix_fmt"], dither=kw["dither"], chroma_loc=chroma_loc, out_size=out_size,
                             range_src=kw.get("range_src", "tv"), range_in=kw.get("range_in"), lut_depth=kw.get("lut_depth"),
                             out2_pix_fmt=second_pix_fmt, lut2=cube2 is not None)
    if matte is None and (matte_depth is not None or matte_invert is not False):
        raise ValueError("matte_depth / matte_invert describe a matte: they need matte")
    if stages is not None or strength is not None or matte is not None:
        # the stage stack: with a strength (3.22) or a matte (3.23) and no `stages`, the list the other options
        # imply; both travel to the engine with what `engine_call_for` returned
        if stages is None:
            stages = implied_stages(cube is not None, cube2 is not None, lut1d is not None, cdl is not None)
        call = {k: v for k, v in kw.items() if k not in ("dither", "interp", "alpha_mode")}
        if strength is not None:
            call["strength"] = strength
        if matte is not None:
            call.update(matte=matte, matte_depth=matte_depth, matte_invert=matte_invert)
        result = _stack_route(
            planes, out, check_stack_options, "apply_yuv_stack", (kw["pix_fmt"], kw["out_pix_fmt"]), stages, kw.get("interp"),
            *loaded, dict(dither=kw["dither"], chroma_loc=chroma_loc, out_size=out_size, alpha_mode=alpha_mode,
                          out2_pix_fmt=second_pix_fmt, strength=strength, precision=precision, matte=matte is not None),
            lambda: call)
        return result, output_color_tags(plan.output_policy)
    if lut1d is not None:
        check_lut1d_options(kw["pix_fmt"], kw["out_pix_fmt"], interp1d=interp1d, dither=kw["dither"], chroma_loc=chroma_loc,
                            out_size=out_size, alpha_mode=alpha_mode, out2_pix_fmt=second_pix_fmt, lut2=cube2 is not None,
                            cdl=cdl is not None)
        # (a file is parsed once and kept, like `cube`: the same object the next time, so the device table stands)
        lut1d = _cached_cube(Path(lut1d), read_lut1d) if isinstance(lut1d, (str, Path)) and Path(lut1d).is_file() else as_lut1d(lut1d)
    if cdl is None and cdl_id is not None:
        raise ValueError("cdl_id names a correction inside a CDL file: it needs cdl")
    if cdl is not None:
        cdl = as_cdl(cdl, cdl_id)
        # (a parsed LUT tells whether it carries a prelut; an engine that already holds the lattice knows it of its own)
        held = _parsed_lut(cube)
        prelut = getattr(held, "prelut", None) is not None if held is not None else bool(getattr(engine, "_has_prelut", False))
        check_cdl_options(kw["pix_fmt"], kw["out_pix_fmt"], dither=kw["dither"], chroma_loc=chroma_loc, out_size=out_size,
                          alpha_mode=alpha_mode, out2_pix_fmt=second_pix_fmt, lut2=cube2 is not None, prelut=prelut)
        kw["cdl"] = cdl
    if cube2 is not None:
        kw = chain_call_for(kw, interp2, chroma_loc, out_size, second_pix_fmt)
    elif second_pix_fmt is not None:
        # the second format is resolved beside engine_call_for's: the same chain, one more output stage; dual_call_for makes
        # every check of the formats and options
        kw = dual_call_for(kw, second_pix_fmt, chroma_loc, out_size)
    elif rgb_src is not None:
        if chroma_loc is not None:
            raise ValueError("chroma siting (chroma_loc) is not defined for an RGB source")
    else:
        kind = check_container_options(kw["pix_fmt"], kw["out_pix_fmt"], kw["dither"], chroma_loc, out_size)
        if kind in ("packed", "v210"):
            kw["width"] = got_w
        elif kind is None:
            check_chroma_loc(chroma_loc, kw["dither"], kw["pix_fmt"], kw["out_pix_fmt"])
    if chroma_loc is not None:
        kw["chroma_loc"] = chroma_loc
    if out_size is not None:
        kw["out_size"] = out_size
    float_out = is_float_out_call(kw)
    if float_out:
        from .multigpu import LutEngineGroup
        if kw["dither"] != "none" or out_size is not None:
            raise ValueError("a float output takes no dither and no resolution")
        if isinstance(engine, LutEngineGroup) or (engine is None and len(devices) > 1):
            raise ValueError("a float output needs a single device")
    own = engine is None
    eng = engine if engine is not None else _cached_engine(devices)
    lut, lut2 = _parsed_lut(cube), _parsed_lut(cube2)
    check_lut2(lut2)
    with eng._lock:                 # upload, precision and launch of ONE task: no other thread's call gets in between
        _stack_upload(eng, lut, lut2, lut1d, interp1d, precision)
        if lut1d is not None:
            # (cube=None with a 1D LUT is lut1d alone, whatever lattice the engine holds)
            kw1 = {k: v for k, v in kw.items() if k != "dither"}
            result = eng.apply_yuv_lut1d(planes, out, **dict(kw1, interp=kw1["interp"] if cube is not None else None))
        elif float_out:
            n_out = parse_rgb_source(kw["out_pix_fmt"]).nplanes
            result = eng.apply_rgb_float(planes[:n_out], out, interp=kw["interp"], alpha_mode=kw.get("alpha_mode", "straight"))
        elif cube2 is not None:
            result = eng.apply_yuv_chain(planes, out, **kw)
        elif second_pix_fmt is not None:
            o1, o2 = out if out is not None else (None, None)
            result = eng.apply_yuv_dual(planes, o1, o2, **kw)
        else:
            result = eng.apply_rgb_to_yuv(planes, out, **kw) if rgb_src is not None else eng.apply_yuv(planes, out, **kw)
        if own:
            eng.sync()
    return result, output_color_tags(plan.output_policy)
