"""argv twins of the reference's command builder, rendered from a LutPlan.

Call-compatible with
  build_command   /root/reference/src/lut_renderer/ffmpeg.py:179-414
  build_pipeline  /root/reference/src/lut_renderer/ffmpeg.py:436-487
  CommandStage    /root/reference/src/lut_renderer/ffmpeg.py:14-25
(same positional/keyword arguments, `notes` mutated in place, ValueError with the
reference's messages), so /root/reference/src/lut_renderer/task_manager.py:55,73-81 can use
them unchanged.  tests/test_dropin_argv.py pins the output against argv captured from the
reference itself (tests/golden/argv_cases.json).

The argv is assembled section by section (time structure, rate control, colour tags, ...)
from small helpers instead of one long function; the LUT part comes from plan.LutPlan.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional, Tuple

from .formats import (check_alpha_mode, check_cdl_options, check_chain_options, check_dual_options, check_lut1d_options,
                      check_premul_options, PACKED_STAGES_EXCLUSIVE, SEMI_STAGES_EXCLUSIVE, check_packed_stack_options, check_rgb_stack_options, check_semi_stack_options, check_stack_options, check_yuv2rgb_stack_options, implied_stages, parse_stages, stages_string, parse_rgb_source, premul_to_yuv)
from .params import ProcessingParams, Task, VideoInfo
from .plan import LutPlan, output_color_tags, resolve_lut_plan, resolve_pix_fmt

_RATE = re.compile(r"^\s*(\d+(?:\.\d+)?)([kKmMgG]?)\s*$")


@dataclass
class CommandStage:
    name: str
    source_path: Path
    output_path: Path
    params: ProcessingParams
    lut_path: Optional[Path] = None
    cleanup_on_success: bool = False
    notes: List[str] = field(default_factory=list)
    probe_source: bool = False      # probe the stage input right before building its command


# ---------------------------------------------------------------- small value helpers
def _trim_float(value: float) -> str:
    return f"{value:.3f}".rstrip("0").rstrip(".")


def _fraction(text: str) -> Optional[float]:
    text = (text or "").strip()
    if not text:
        return None
    try:
        if "/" in text:
            num, den = text.split("/", 1)
            return float(num) / float(den) if float(den) != 0 else None
        return float(text)
    except ValueError:
        return None


def _rate(text: Optional[str]) -> Optional[Tuple[float, str]]:
    m = _RATE.match(text) if text else None
    if not m or float(m.group(1)) <= 0:
        return None
    return float(m.group(1)), m.group(2) or ""


def _double_rate(text: str) -> Optional[str]:
    parsed = _rate(text)
    if not parsed:
        return None
    number, unit = parsed[0] * 2, parsed[1]
    return f"{int(round(number))}{unit}" if abs(number - round(number)) < 1e-6 else f"{number:g}{unit}"


def _kbps(text: Optional[str]) -> Optional[float]:
    parsed = _rate(text)
    if not parsed:
        return None
    return {"k": parsed[0], "m": parsed[0] * 1e3, "g": parsed[0] * 1e6}.get(parsed[1].lower())


def _inherit_tags(cmd: List[str], info: Optional[VideoInfo], notes: List[str]) -> None:
    if not info:
        return
    shown = []
    for flag, label, value in (("-color_primaries", "primaries", info.color_primaries),
                               ("-color_trc", "trc", info.color_trc),
                               ("-colorspace", "colorspace", info.colorspace),
                               ("-color_range", "range", info.color_range)):
        if value:
            cmd += [flag, value]
            shown.append(f"{label}={value}")
    if shown:
        notes.append(f"继承色彩元数据: {', '.join(shown)}")


# ---------------------------------------------------------------- argv sections
def _time_structure(cmd, params, info, notes) -> Optional[float]:
    """-fps_mode / -r (ffmpeg.py:259-285); returns the fps used for the automatic GOP."""
    if params.fps:
        fps_value, fps_text = _fraction(params.fps), params.fps
    elif info and info.fps:
        fps_value, fps_text = info.fps, _trim_float(info.fps)
    else:
        fps_value, fps_text = None, None
    if params.fps:
        cmd += ["-fps_mode", "cfr", "-r", params.fps]
        notes.append(f"时间结构: fps_mode=cfr, 输出帧率={params.fps}")
        return fps_value
    vfr = bool(info and info.is_vfr)
    if vfr and params.force_cfr:
        cmd += ["-fps_mode", "cfr"]
        if fps_text:
            cmd += ["-r", fps_text]
            notes.append(f"时间结构: 源为 VFR，已强制 CFR，输出帧率={fps_text}")
        else:
            notes.append("时间结构: 源为 VFR，已强制 CFR（未检测到帧率）")
    elif params.force_cfr and info is None:
        cmd += ["-fps_mode", "cfr"]
        notes.append("时间结构: fps_mode=cfr（未读取源信息）")
    else:
        cmd += ["-fps_mode", "passthrough"]
        notes.append("时间结构: 源为 VFR，fps_mode=passthrough（不重写时间戳）" if vfr
                     else "时间结构: 源为 CFR/未知，fps_mode=passthrough（避免时间戳重写）")
    return fps_value


def _rate_control(cmd, params, fps_value, notes) -> None:
    if params.resolution:
        cmd += ["-s", params.resolution]
    if params.bitrate:
        cmd += ["-b:v", params.bitrate]
        bufsize = _double_rate(params.bitrate)
        if bufsize:
            cmd += ["-maxrate", params.bitrate, "-bufsize", bufsize]
            notes.append(f"码率稳定: maxrate={params.bitrate}, bufsize={bufsize}")
    for flag, value in (("-crf", params.crf), ("-preset", params.preset), ("-tune", params.tune)):
        if value:
            cmd += [flag, value]
    if params.gop:
        cmd += ["-g", params.gop]
    elif fps_value:
        gop = max(1, round(fps_value))
        cmd += ["-g", str(gop)]
        notes.append(f"自动 GOP={gop} (fps={_trim_float(fps_value)})")
    for flag, value in (("-profile:v", params.profile), ("-level", params.level), ("-threads", params.threads)):
        if value:
            cmd += [flag, value]


def _colour_tags(cmd, params, info, plan: Optional[LutPlan], notes) -> None:
    """ffmpeg.py:348-386"""
    if plan is None:
        if params.inherit_color_metadata:
            _inherit_tags(cmd, info, notes)
        return
    tags = output_color_tags(plan.output_policy)
    if tags is not None:
        for key in ("color_primaries", "color_trc", "colorspace", "color_range"):
            cmd += [f"-{key}", tags[key]]
        notes.append("LUT 输出标记: bt709/bt709/bt709, range=tv" +
                     ("" if plan.output_policy == "bt709" else "（回退）"))
    elif plan.output_policy == "inherit":
        if params.inherit_color_metadata:
            _inherit_tags(cmd, info, notes)
    else:
        notes.append("LUT 输出标记: none（不写色彩元数据）")


# ---------------------------------------------------------------- public twins
def build_command(source: Path, output: Path, params: ProcessingParams, lut_path: Optional[Path] = None,
                  ffmpeg_bin: str = "ffmpeg", source_info: Optional[VideoInfo] = None,
                  notes: Optional[List[str]] = None) -> List[str]:
    notes = notes if notes is not None else []
    cmd = [ffmpeg_bin, "-hide_banner"]
    if params.overwrite:
        cmd.append("-y")
    cmd += ["-i", str(source)]

    plan = resolve_lut_plan(params, lut_path, source_info) if lut_path else None
    filters: List[str] = []
    if plan is not None:
        filters += plan.filters()
        notes.extend(plan.notes)

    if params.video_codec:
        cmd += ["-c:v", params.video_codec]
    if params.audio_codec:
        cmd += ["-c:a", params.audio_codec]
    if filters and params.video_codec == "copy":
        raise ValueError("启用 LUT/滤镜时不能使用视频 copy（streamcopy 与滤镜不可同时使用）。")

    if params.video_codec and params.video_codec != "copy":
        fps_value = _time_structure(cmd, params, source_info, notes)
        pix_fmt = resolve_pix_fmt(params, source_info, notes)
        if pix_fmt:
            if getattr(params, "zscale_dither", "none") == "error_diffusion":
                filters.append("zscale=dither=error_diffusion")
                notes.append("抖动: zscale=dither=error_diffusion")
            if plan is not None:
                filters.append(f"format={pix_fmt}")
            cmd += ["-pix_fmt", pix_fmt]
        _rate_control(cmd, params, fps_value, notes)
        _colour_tags(cmd, params, source_info, plan, notes)
        if "videotoolbox" in params.video_codec:
            kbps = _kbps(params.bitrate or (source_info.bitrate if source_info else ""))
            if kbps and kbps >= 50_000:
                notes.append("提示: h264_videotoolbox 在高码率/重负载时可能出现 PTS 重建/帧重排的节奏错觉；"
                             "如需更稳定建议用 libx264 或切到“专业母带”。")

    if filters:
        cmd += ["-vf", ",".join(filters)]
    if params.audio_codec and params.audio_codec != "copy":
        for flag, value in (("-b:a", params.audio_bitrate), ("-ar", params.sample_rate), ("-ac", params.channels)):
            if value:
                cmd += [flag, value]
    if params.faststart:
        cmd += ["-movflags", "+faststart"]
    cmd.append(str(output))
    return cmd


def _master_params(params: ProcessingParams) -> ProcessingParams:
    """ProRes 422 HQ mezzanine settings of the two-stage mode (ffmpeg.py:417-433)."""
    master = ProcessingParams.from_dict(params.to_dict())
    master.video_codec, master.audio_codec = "prores_ks", "copy"
    master.pix_fmt, master.profile = "yuv422p10le", "3"
    for name in ("level", "crf", "preset", "tune", "bitrate", "audio_bitrate", "sample_rate", "channels"):
        setattr(master, name, "")
    master.faststart = False
    master.bit_depth_policy = "preserve"
    return master


def build_pipeline(task: Task, ffmpeg_bin: str = "ffmpeg") -> List[CommandStage]:
    """One stage with the LUT ("fast"), or ProRes master WITH the LUT followed by a
    distribution encode WITHOUT it ("pro"): the LUT is applied exactly once per task."""
    params = task.params
    if params.processing_mode != "pro":
        return [CommandStage("快速交付", task.source_path, task.output_path, params, lut_path=task.lut_path)]
    if not task.intermediate_path:
        raise ValueError("专业母带模式需要显式设置中间文件路径（请在界面中设置母带缓存目录）。")
    return [
        CommandStage("ProRes 母带", task.source_path, task.intermediate_path, _master_params(params),
                     lut_path=task.lut_path, cleanup_on_success=True,
                     notes=["母带固定为 ProRes 422 HQ (yuv422p10le)"]),
        CommandStage("分发编码", task.intermediate_path, task.output_path, params, lut_path=None,
                     probe_source=True),
    ]


# ---------------------------------------------------------------- engine twin
def engine_command(source: Path, output: Path, params: ProcessingParams, lut_path: Path,
                   source_info: VideoInfo, python_bin: Optional[str] = None, device: int = 0,
                   notes: Optional[List[str]] = None, precision: str = "strict", chroma_loc: Optional[str] = None,
                   gpu_resize: bool = False, second_output: Optional[Path] = None,
                   second_pix_fmt: Optional[str] = None, engine_dither: Optional[str] = None,
                   cube2: Optional[Path] = None, interp2: Optional[str] = None, alpha_mode: str = "straight",
                   cdl=None, cdl_id: Optional[str] = None, lut1d: Optional[Path] = None,
                   interp1d: Optional[str] = None, stages=None, strength: Optional[float] = None,
                   strength_keys: Optional[str] = None, matte: Optional[Path] = None, matte_pix_fmt: Optional[str] = None,
                   matte_invert: bool = False, rgb_matrix=None, rgb_stages=None, rgb_out: Optional[str] = None,
                   rgb_out_stages=None, semi_stages=None, packed_stages=None) -> List[str]:
    """`build_command`'s twin for the LUT stage alone: the argv of the ENGINE CLI (`python -m lut_renderer_amd.cli`)
    that applies exactly the chain `build_command` would put into `-vf` -- the same `LutPlan`, rendered as CLI options
    instead of as a filter string (ffmpeg.py:195-247, :287-310).  `source` / `output` are rawvideo files (or `-`) in
    `source_info.pix_fmt` and the pixel format `resolve_pix_fmt` picks; `task_manager.py:145-151` can Popen the result
    unchanged (same `Duration:` / `time=` / exit-code / SIGTERM contract).  `notes` receives the plan's notes, like
    `build_command`'s out-parameter.  The copy guard of ffmpeg.py:255-256 applies: a LUT stage cannot be a stream copy.
    `precision` is the engine's own setting (`--precision`, default strict; the reference's records have no such field), and
    so is `chroma_loc` (`--chroma-loc`, rendered only when given: None keeps the replicating chroma contract).
    `gpu_resize` with `params.resolution` set moves the reference's `-s WxH` into the engine (`--out-size`); the
    output format must then be planar (ValueError for packed formats).  False (default) leaves the argv as it was.
    `second_output` / `second_pix_fmt` (both or neither) add a second rawvideo output from the same LUT pass (`--second-output`,
    `--second-pix-fmt`, DESIGN.md 3.13: the master and the delivery format of the "pro" mode together); rendered only when given.
    Planar YUV on every side; not with dither, `chroma_loc` or `gpu_resize`.
    `engine_dither` ("blue_noise") is an engine setting as well (`--engine-dither`, rendered only when given);
    not together with `params.zscale_dither` = error_diffusion, `chroma_loc` or a second output.
    `cube2` / `interp2` add a second LUT behind the first in the same pass (`--cube2`, `--interp2`, DESIGN.md 3.17: a technical LUT,
    then a look); rendered only when given, `interp2` through the whitelist of `interp`.  Planar YUV without alpha on both sides;
    not with dither, `chroma_loc`, `gpu_resize` or a second output.
    `alpha_mode` ("premultiplied") is an engine setting too (`--alpha-mode`, rendered only when premultiplied:
    "straight" keeps the argv as it was): a yuva* source with a planar YUV output or gbrapf32le kept float; not with a full-range
    prologue, dither, `chroma_loc`, `gpu_resize`, a second output or a second LUT.  ffmpeg's chain has no such step.
    `cdl` puts an ASC CDL in front of the LUT in the same pass, an engine setting as well: the path of a .cc / .ccc
    / .cdl file (`--cdl`, with `cdl_id` as `--cdl-id`) or a `cdl.Cdl` (`--cdl-sop`, and `--cdl-sat` unless it is 1); rendered only
    when given.  Planar YUV on both sides; not with dither, `chroma_loc`, `gpu_resize`, a second output, a second LUT or
    premultiplied alpha.  A LUT with a .csp prelut is refused where the LUT is loaded.
    `lut1d` / `interp1d` put a 1D LUT file in front of the LUT in the same pass (`--lut1d`, and `--interp1d` when
    given: ffmpeg's `lut1d=file=A,lut3d=file=B`); rendered only when given.  Planar YUV on both sides; not with dither,
    `chroma_loc`, `gpu_resize`, a CDL, a second LUT, a second output or premultiplied alpha.  `interp1d` without `lut1d` is a
    ValueError.
    `stages` (a sequence or comma string as `LutEngine.apply_yuv_stack` takes it) runs the LUT, `cube2`, `lut1d`
    and `cdl` as an ordered stack in one pass (`--stages`, every lut3d stage with its mode spelled out); rendered only when
    given, and only then may those be combined.  The list names `lut3d` (the LUT this stage renders) and a stage for every file
    given, and every other stage has its file; the refusals are `formats.check_stack_options`'s.
    `strength` (a number in [0, 1]) or `strength_keys` ("F:S,F:S,...", `params.strength_keys`) are engine settings
    beside `engine_dither` -- the reference's `ProcessingParams` has no such field: the graded frame mixed with the source in the
    same pass (`--strength` / `--strength-keys`, rendered only when given, never both).  They run the stage stack, with `stages`
    or with the list the other options imply, and on its terms: the refusals are `check_stack_options`'s and name the strength.
    `matte` (the path of raw gray frames of the source's size, one for the whole stream or one per frame),
    `matte_pix_fmt` (gray | gray10le | gray12le | gray14le | gray16le, default gray) and `matte_invert` are engine settings
    likewise: a strength per pixel in the same pass (`--matte`, `--matte-pix-fmt`, `--matte-invert`, rendered only when given).
    They run the stage stack as a strength does, in refusals that name the matte; `-` is refused, and so are `matte_pix_fmt` /
    `matte_invert` without `matte`.
    `rgb_matrix` is the resource of a `matrix` stage of `stages`, an engine setting as well: an
    `rgbmatrix.RgbMatrix` (`--rgb-matrix`, and `--rgb-matrix-offset` unless it is zero) or the path of a .spimtx file
    (`--rgb-matrix-file`); rendered only when given.  It needs `stages` with a matrix stage, and the stage needs it.
    `rgb_stages` is `stages` for an RGB source (`--rgb-stages`, rendered only when given: without it the argv
    is what it was): the same lists and files on gbrp* / gbrap* / packed RGB frames, into the resolved output format -- planar
    YUV, or gbrp* at the source's depth; the refusals are `formats.check_rgb_stack_options`'s.  Not together with `stages`.
    `rgb_out` with `rgb_out_stages` is `stages` for a planar YUV source written as RGB (`--rgb-out FMT
    --rgb-out-stages LIST`, rendered only when given: without them the argv is what it was): the same lists and files at the
    depth of `rgb_out` (gbrp*, gbrap* or a packed name), which takes the place of the resolved output format -- `params` must
    then resolve none, or that very name; the refusals are `formats.check_yuv2rgb_stack_options`'s.  Each needs the other; not together with
    `stages` / `rgb_stages`.
    `semi_stages` is `stages` for a stage with a semi-planar side (`--semi-stages`, rendered only when given:
    without it the argv is what it was): the same lists and files, without the matrix stage, on nv12 / p010le .. frames into the
    resolved output format -- semi-planar, or planar YUV at 4:2:0 / 4:2:2 / 4:4:4 -- or from planar YUV into a semi-planar one;
    the refusals are `formats.check_semi_stack_options`'s.  Not together with `stages` / `rgb_stages` / `rgb_out_stages`.
    `packed_stages` is `stages` for a stage with a packed 4:2:2 or v210 side (`--packed-stages`, rendered only
    when given: without it the argv is what it was): the same lists and files, without the matrix stage, on uyvy422 / y210le / v210 ..
    frames into the resolved output format -- the same kind of container, or planar YUV at 4:2:2 / 4:2:0 / 4:4:4 -- or from planar
    4:2:2 into a packed 4:2:2 / v210 one; the refusals are `formats.check_packed_stack_options`'s.  Not together with another
    stage list."""
    import sys as _sys
    premul = check_alpha_mode(alpha_mode)
    if precision not in ("strict", "fast", "fma32"):
        raise ValueError(f"unknown precision '{precision}' (strict | fast | fma32)")
    if chroma_loc is not None and chroma_loc not in ("left", "center", "topleft"):
        raise ValueError(f"unknown chroma location '{chroma_loc}' (left | center | topleft)")
    if lut_path is None:
        raise ValueError("engine_command renders the LUT stage: lut_path is required")
    if source_info is None or not source_info.pix_fmt or not source_info.width or not source_info.height:
        raise ValueError("engine_command needs source_info with pix_fmt, width and height (raw frames carry no header)")
    if params.video_codec == "copy":
        raise ValueError("启用 LUT/滤镜时不能使用视频 copy（streamcopy 与滤镜不可同时使用）。")
    notes = notes if notes is not None else []
    plan = resolve_lut_plan(params, lut_path, source_info)
    notes.extend(plan.notes)
    cmd = [python_bin or _sys.executable, "-m", "lut_renderer_amd.cli"]
    if params.overwrite:
        cmd.append("-y")
    cmd += ["-i", str(source), "-o", str(output), "--size", f"{source_info.width}x{source_info.height}",
            "--pix-fmt", source_info.pix_fmt]
    pix_fmt = resolve_pix_fmt(params, source_info, notes) if params.video_codec else ""
    if semi_stages is not None and (stages is not None or rgb_stages is not None or rgb_out_stages is not None):
        raise ValueError(SEMI_STAGES_EXCLUSIVE)
    if packed_stages is not None and (stages is not None or rgb_stages is not None or rgb_out_stages is not None
                                      or semi_stages is not None):
        raise ValueError(PACKED_STAGES_EXCLUSIVE)
    if rgb_out_stages is not None:
        if rgb_out is None:
            raise ValueError("rgb_out_stages is the stage list of a YUV source written as RGB: it needs rgb_out")
        if stages is not None or rgb_stages is not None:
            raise ValueError("rgb_out_stages and stages / rgb_stages are mutually exclusive: stages is the list of a YUV source with "
                             "a YUV output, rgb_stages that of an RGB source, rgb_out_stages that of a YUV source with rgb_out")
        if pix_fmt and pix_fmt != rgb_out:
            raise ValueError(f"rgb_out ('{rgb_out}') and out_pix_fmt ('{pix_fmt}') are mutually exclusive: a call has one output")
        pix_fmt = ""                                           # (--rgb-out names the output)
    elif rgb_out is not None:
        raise ValueError("engine_command renders rgb_out together with rgb_out_stages only")
    src_rgb = parse_rgb_source(str(source_info.pix_fmt))
    float_src = src_rgb is not None and src_rgb.floating
    if float_src:
        # a float source: without a resolved output format the stage stays float (no --out-pix-fmt, no dither)
        if chroma_loc is not None:
            raise ValueError("chroma siting (chroma_loc) is not defined for an RGB source")
    elif _is_rgb_source(source_info.pix_fmt):
        # an RGB source: the engine has no encoder to negotiate an output format with, and no chroma to site
        if not pix_fmt:
            raise ValueError(f"an RGB source ('{source_info.pix_fmt}') needs a resolved output pixel format (params.pix_fmt or a "
                             "bit-depth policy that picks one): the engine cannot leave it to the encoder")
        if chroma_loc is not None:
            raise ValueError("chroma siting (chroma_loc) is not defined for an RGB source")
    if pix_fmt:
        cmd += ["--out-pix-fmt", pix_fmt]
    cmd += ["--cube", str(plan.lut_path), "--interp", plan.interp, "--input-matrix", plan.matrix_policy,
            "--output-tags", plan.output_policy]
    if getattr(params, "zscale_dither", "none") == "error_diffusion" and (pix_fmt or rgb_out is not None):
        cmd += ["--zscale-dither", "error_diffusion"]
        notes.append("抖动: zscale=dither=error_diffusion")
    if source_info.colorspace:
        cmd += ["--colorspace", str(source_info.colorspace)]
    if source_info.color_range:
        cmd += ["--color-range", str(source_info.color_range)]
    if source_info.fps:
        cmd += ["--fps", fps_rational(source_info.fps)]
    if device:
        cmd += ["--device", str(int(device))]
    if precision != "strict":
        cmd += ["--precision", precision]
    if engine_dither is not None:
        from .api import resolve_engine_dither
        resolve_engine_dither(engine_dither, "error_diffusion" if "--zscale-dither" in cmd else "none")
        if not pix_fmt and float_src:
            raise ValueError("a float output takes no dither")
        cmd += ["--engine-dither", engine_dither]
    # (the dither of the call, as the checks below take it: rendered into cmd above)
    dither = "error_diffusion" if "--zscale-dither" in cmd else ("blue_noise" if "--engine-dither" in cmd else "none")
    if chroma_loc is not None:
        if "--zscale-dither" in cmd or "--engine-dither" in cmd:
            raise ValueError("error-diffusion dither is not defined with sited chroma resampling (chroma_loc)")
        cmd += ["--chroma-loc", chroma_loc]
    if gpu_resize and params.resolution:
        out_fmt = pix_fmt or str(source_info.pix_fmt)
        if not _PLANAR_RE.match(out_fmt):
            raise ValueError(f"gpu_resize needs a planar output format, not '{out_fmt}' (keep -s on the encoder)")
        if not _SIZE_RE.match(params.resolution):
            raise ValueError(f"bad resolution '{params.resolution}' (expected WxH)")
        cmd += ["--out-size", params.resolution]
    if (second_output is None) != (second_pix_fmt is None):
        raise ValueError("second_output and second_pix_fmt go together: give both or neither")
    if second_output is not None:
        if str(second_output) == "-":
            raise ValueError("second_output is a file or FIFO, not '-'")
        check_dual_options(str(source_info.pix_fmt), pix_fmt or None, second_pix_fmt, dither, chroma_loc,
                           params.resolution if "--out-size" in cmd else None)
        cmd += ["--second-output", str(second_output), "--second-pix-fmt", second_pix_fmt]
    if cube2 is None and interp2 is not None:
        raise ValueError("interp2 is the mode of the second LUT: it needs cube2")
    if strength is not None and strength_keys is not None:
        raise ValueError("strength and strength_keys are mutually exclusive: give one or neither")
    mixed = strength is not None or strength_keys is not None
    if matte is None and (matte_pix_fmt is not None or matte_invert):
        raise ValueError("matte_pix_fmt / matte_invert describe a matte: they need matte")
    if matte is not None:
        from .formats import MATTE_PIX_FMTS
        if str(matte) == "-":
            raise ValueError("matte is a file or FIFO, not '-': stdin carries the input")
        if (matte_pix_fmt or "gray") not in MATTE_PIX_FMTS:
            raise ValueError(f"unknown matte_pix_fmt '{matte_pix_fmt}' ({' | '.join(MATTE_PIX_FMTS)})")
    if rgb_stages is not None and stages is not None:
        raise ValueError("stages and rgb_stages are mutually exclusive: stages is the list of a YUV source, rgb_stages that of an "
                         "RGB source")
    if rgb_matrix is not None and stages is None and rgb_stages is None and rgb_out_stages is None and semi_stages is None \
            and packed_stages is None:
        raise ValueError("rgb_matrix needs stages: a matrix stage has no implied position (e.g. stages='lut1d,matrix,lut3d')")
    # the pairwise refusals below give way to check_stack_options / check_rgb_stack_options / check_yuv2rgb_stack_options at the end
    stack = stages is not None or mixed or matte is not None or rgb_stages is not None or rgb_out_stages is not None or \
        semi_stages is not None or packed_stages is not None
    if cube2 is not None:
        from .plan import INTERP_WHITELIST
        if not stack:
            check_chain_options(str(source_info.pix_fmt), pix_fmt or None, dither, chroma_loc,
                                params.resolution if "--out-size" in cmd else None, second_pix_fmt)
        cmd += ["--cube2", str(cube2)]
        if interp2 is not None:
            cmd += ["--interp2", interp2 if interp2 in INTERP_WHITELIST else "tetrahedral"]
    if premul:
        src_fmt = str(source_info.pix_fmt).replace("yuvj", "yuv")
        check_premul_options(src_fmt, pix_fmt or None, dither=dither, chroma_loc=chroma_loc,
                             out_size=params.resolution if "--out-size" in cmd else None,
                             range_src="pc" if plan.prologue else "tv", range_in=plan.prologue_out_range if plan.prologue else "tv",
                             lut_depth=8 if plan.prologue else None, out2_pix_fmt=second_pix_fmt, lut2=cube2 is not None,
                             to_yuv=premul_to_yuv(src_fmt, pix_fmt or None))
        cmd += ["--alpha-mode", "premultiplied"]
    if cdl is None and cdl_id is not None:
        raise ValueError("cdl_id names a correction inside a CDL file: it needs cdl")
    if cdl is not None:
        from .cdl import Cdl
        if not stack:
            check_cdl_options(str(source_info.pix_fmt).replace("yuvj", "yuv"), pix_fmt or None, dither=dither, chroma_loc=chroma_loc,
                              out_size=params.resolution if "--out-size" in cmd else None, alpha_mode=alpha_mode,
                              out2_pix_fmt=second_pix_fmt, lut2=cube2 is not None)
        if isinstance(cdl, Cdl):
            if cdl_id is not None:
                raise ValueError("cdl_id names a correction inside a CDL file, and cdl is a set of values")
            cmd += ["--cdl-sop", cdl.sop_text()]
            if cdl.saturation != 1.0:
                cmd += ["--cdl-sat", repr(cdl.saturation)]
        elif isinstance(cdl, (str, Path)):
            cmd += ["--cdl", str(cdl)]
            if cdl_id is not None:
                cmd += ["--cdl-id", str(cdl_id)]
        else:
            raise TypeError(f"cdl must be a Cdl or the path of a .cc / .ccc / .cdl file, not {type(cdl).__name__}")
    if lut1d is None and interp1d is not None:
        raise ValueError("interp1d is the mode of the 1D LUT: it needs lut1d")
    if lut1d is not None:
        if not isinstance(lut1d, (str, Path)):
            raise TypeError(f"lut1d must be the path of a 1D .cube file, not {type(lut1d).__name__}")
        if not stack:
            check_lut1d_options(str(source_info.pix_fmt).replace("yuvj", "yuv"), pix_fmt or None, interp1d=interp1d or "linear",
                                dither=dither, chroma_loc=chroma_loc, out_size=params.resolution if "--out-size" in cmd else None,
                                alpha_mode=alpha_mode, out2_pix_fmt=second_pix_fmt, lut2=cube2 is not None, cdl=cdl is not None)
        cmd += ["--lut1d", str(lut1d)]
        if interp1d is not None:
            cmd += ["--interp1d", interp1d]
    if stack:
        from . import _native
        from .plan import INTERP_WHITELIST
        mode2 = None if interp2 is None else interp2 if interp2 in INTERP_WHITELIST else "tetrahedral"
        listed = packed_stages if packed_stages is not None else semi_stages if semi_stages is not None else rgb_out_stages if rgb_out_stages is not None else \
            rgb_stages if rgb_stages is not None else stages if stages is not None else \
            implied_stages(True, cube2 is not None, lut1d is not None, cdl is not None)
        st = parse_stages(listed, interp=plan.interp, interp2=mode2)
        kinds = [k for k, _m in st]
        if (interp1d or "linear") not in _native.INTERP1D:
            raise ValueError(f"lut1d has no interpolation mode '{interp1d}' ({' | '.join(_native.INTERP1D)})")
        for name, given, kind in (("the LUT", lut_path, "lut3d"), ("cube2", cube2, "lut3d2"), ("lut1d", lut1d, "lut1d"),
                                  ("cdl", cdl, "cdl"), ("rgb_matrix", rgb_matrix, "matrix")):
            if given is not None and kind not in kinds:
                raise ValueError(f"{name} is given and the stage list has no '{kind}' stage")
        # what the three families' checks are told alike; each adds its own dither, and what only it takes
        told = dict(stages=st, cdl=cdl is not None, lut=True, lut2=cube2 is not None, lut1d=lut1d is not None,
                    rgb_matrix=rgb_matrix is not None, chroma_loc=chroma_loc, out_size=params.resolution if "--out-size" in cmd else None,
                    alpha_mode=alpha_mode, out2_pix_fmt=second_pix_fmt,
                    strength=(strength if strength_keys is None else 1.0) if mixed else None, matte=matte is not None)
        src_fmt = str(source_info.pix_fmt)
        if packed_stages is not None:
            check_packed_stack_options(src_fmt, pix_fmt or None, dither=dither, precision=precision, **told)
        elif semi_stages is not None:
            check_semi_stack_options(src_fmt, pix_fmt or None, dither=dither, precision=precision, **told)
        elif rgb_out_stages is not None:
            from .api import engine_call_for
            check_yuv2rgb_stack_options(src_fmt, rgb_out, dither="error_diffusion" if dither == "error_diffusion" else "none",
                                        engine_dither=engine_dither, **told)
            engine_call_for(plan, src_fmt, None, "straight", rgb_out=rgb_out)               # (a full-range source: 8 bit only)
        elif rgb_stages is not None:
            check_rgb_stack_options(src_fmt, pix_fmt or None, dither=dither,
                                    intermediate_pix_fmt=plan.intermediate_pix_fmt if plan.prologue else None, **told)
        else:
            check_stack_options(src_fmt.replace("yuvj", "yuv"), pix_fmt or None, dither=dither, precision=precision, **told)
        if rgb_matrix is not None:
            from .rgbmatrix import RgbMatrix
            if isinstance(rgb_matrix, RgbMatrix):
                cmd += ["--rgb-matrix", rgb_matrix.m_text()]
                if rgb_matrix.offset != (0.0, 0.0, 0.0):
                    cmd += ["--rgb-matrix-offset", rgb_matrix.offset_text()]
            elif isinstance(rgb_matrix, (str, Path)):
                cmd += ["--rgb-matrix-file", str(rgb_matrix)]
            else:
                raise TypeError(f"rgb_matrix must be an RgbMatrix or the path of a .spimtx file, not {type(rgb_matrix).__name__}")
        if packed_stages is not None:
            cmd += ["--packed-stages", stages_string(st)]
        elif semi_stages is not None:
            cmd += ["--semi-stages", stages_string(st)]
        elif rgb_out_stages is not None:
            cmd += ["--rgb-out", rgb_out, "--rgb-out-stages", stages_string(st)]
        elif rgb_stages is not None:
            cmd += ["--rgb-stages", stages_string(st)]
        elif stages is not None:
            cmd += ["--stages", stages_string(st)]
        if strength is not None:
            cmd += ["--strength", repr(float(strength))]
        if strength_keys is not None:
            from .params import strength_keys as parse_keys
            parse_keys(strength_keys)
            cmd += ["--strength-keys", str(strength_keys)]
        if matte is not None:
            cmd += ["--matte", str(matte)]
            if matte_pix_fmt is not None:
                cmd += ["--matte-pix-fmt", matte_pix_fmt]
            if matte_invert:
                cmd += ["--matte-invert"]
    return cmd


def _is_rgb_source(pix_fmt) -> bool:
    """gbrp* / gbrap* at any number of bits, or one of the packed RGB names the engine takes as a source
    (`_native.PACKED_FORMATS`).  Not `parse_rgb_source`: that one takes the float names too and no depth outside 8..16."""
    from ._native import PACKED_FORMATS
    name = str(pix_fmt or "")
    return name in PACKED_FORMATS or bool(re.match(r"^gbra?p(\d+)?(le)?$", name))


#: planar formats the engine's resize takes; packed RGB keeps -s on the encoder
_PLANAR_RE = re.compile(r"^(yuvj?(420|422|444)p|gbrp)(\d+)?(le)?$")
_SIZE_RE = re.compile(r"^[1-9][0-9]*x[1-9][0-9]*$")


def fps_rational(fps) -> str:
    """A frame rate as the rational ffprobe reported (`r_frame_rate`): `VideoInfo.fps` is that fraction parsed to a float
    (media_info.py:135-137), and printing it with six digits (29.97) makes timestamps drift against the source.  NTSC rates
    come back as N000/1001, everything else as the closest fraction with a denominator up to 1001."""
    from fractions import Fraction
    value = float(fps)
    for den in (1, 1001):
        num = round(value * den)
        if num > 0 and abs(num / den - value) <= 1e-6 * value:
            return str(num) if den == 1 else f"{num}/{den}"
    frac = Fraction(value).limit_denominator(1001)
    return str(frac.numerator) if frac.denominator == 1 else f"{frac.numerator}/{frac.denominator}"
