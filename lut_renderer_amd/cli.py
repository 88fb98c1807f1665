"""Engine CLI with the process contract `TaskRunner._run_stage` expects from ffmpeg
(/root/reference/src/lut_renderer/task_manager.py:134-190): started with Popen(stdout=PIPE,
stderr=STDOUT, text=True), it prints one `Duration: HH:MM:SS.xx` line, then `time=HH:MM:SS.xx`
progress lines (regexes at task_manager.py:14-15), exits 0 on success and non-zero with a message
on error, and stops on SIGTERM (task_manager.py:38-44).

It works on rawvideo files (planar frames back to back), i.e. the stage between a decoder and an
encoder; the options are the reference's own LUT vocabulary (models.py:45-56):

    python -m lut_renderer_amd.cli -i in.yuv -o out.yuv --size 3840x2160 --pix-fmt yuv420p10le \
        --cube look.cube --interp tetrahedral --colorspace bt2020nc --color-range tv

SURVEY.md 8f rank 1.  Frames stream through `stream.HostPipeline` (pinned ring, overlapped copies).
"""
from __future__ import annotations

import argparse
import os
import signal
import sys
import time

from .formats import (check_cdl_options, check_chroma_loc, check_container_options, check_lut1d_options, check_lut2, check_rgb_stack_options, check_stack_options, check_yuv2rgb_stack_options, implied_stages, parse_stages,
                      check_premul_options, parse_size, refuse_alpha_resize, source_bit_depth)


def _hms(seconds: float) -> str:
    seconds = max(0.0, seconds)
    h, rem = divmod(seconds, 3600)
    m, s = divmod(rem, 60)
    return f"{int(h):02d}:{int(m):02d}:{s:05.2f}"


def _rate(text: str) -> float:
    """'25', '29.97' or ffprobe's rational form '30000/1001'."""
    num, _, den = str(text).partition("/")
    value = float(num) / (float(den) if den else 1.0)
    if not value > 0:
        raise argparse.ArgumentTypeError(f"bad frame rate '{text}'")
    return value


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="lut_renderer_amd.cli", description=__doc__.split("\n\n")[0])
    ap.add_argument("-i", "--input", required=True)
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--size", required=True, help="WxH")
    ap.add_argument("--pix-fmt", required=True,
                    help="planar YUV (yuva* too: four planes, alpha last, kept unless --out-pix-fmt has none), semi-planar YUV (nv12, nv21, nv16, p010le .. p216le), packed 4:2:2 YUV (yuyv422, uyvy422, yvyu422, y210le, y212le, y216le), v210 (10-bit 4:2:2 in 32-bit words, rows of 128 * ceil(w / 48) bytes; in FFmpeg a codec / FourCC name, not a pix_fmt: its bytes are what `-c:v v210 -f rawvideo` writes), or an RGB source (gbrp* / gbrap* / rgb24, bgr24, rgba .., rgb48le, rgba64le) with a YUV --out-pix-fmt, "
                         "or float RGB (gbrpf32le / gbrapf32le): float out without --out-pix-fmt, else a YUV one")
    ap.add_argument("--out-pix-fmt", default=None)
    ap.add_argument("--rgb-out", default=None, metavar="FMT",
                    help="engine setting: write RGB from a planar YUV --pix-fmt in the same pass (DESIGN.md 3.24; ffmpeg's "
                         "lut3d=...,format=FMT): gbrp .. gbrp16le or gbrap* (planes G, B, R[, A] back to back) or a packed name "
                         "(rgb24, bgr24, rgba, bgra, argb, abgr, rgb48le, rgba64le, ..; a fourth component is opaque).  The LUT runs at "
                         "FMT's depth; a full-range source takes an 8-bit FMT.  Not with --out-pix-fmt, dither, --chroma-loc, "
                         "--out-size, --second-output, --cube2, --cdl, --lut1d, --stages, --strength, --matte or "
                         "--alpha-mode premultiplied")
    ap.add_argument("--cube", default=None, help="the 3D LUT; required unless --lut1d is given (lut1d alone)")
    ap.add_argument("--interp", default="tetrahedral")
    ap.add_argument("--input-matrix", default="auto")
    ap.add_argument("--output-tags", default="bt709")
    ap.add_argument("--zscale-dither", default="none", help="none | error_diffusion (models.py:46)")
    ap.add_argument("--colorspace", default=None)
    ap.add_argument("--color-range", default=None)
    ap.add_argument("--fps", type=_rate, default=25.0, help="frame rate, a number or a rational like 30000/1001")
    ap.add_argument("--precision", default="strict", choices=["strict", "fast", "fma32"],
                    help="engine setting (not one of the reference's options): strict = bit-exact fp32 restatement of FFmpeg's "
                         "scalar C (default); fast = tolerance-bounded kernels with an fp16 lattice, <= 1 code from strict; "
                         "fma32 = strict's fp32 lattice with a fused multiply-add blend, <= 1 code from strict")
    ap.add_argument("--chroma-loc", default=None, choices=["left", "center", "topleft"],
                    help="engine setting: resample chroma bilinearly at this siting (ffprobe's chroma_location) instead of "
                         "replicating it over its block; strict arithmetic")
    ap.add_argument("--engine-dither", default=None, choices=["blue_noise"],
                    help="engine setting: quantise the output against a 64 x 64 blue-noise mask inside the LUT pass (DESIGN.md "
                         "3.15); not together with --zscale-dither error_diffusion")
    ap.add_argument("--alpha-mode", default="straight", choices=["straight", "premultiplied"],
                    help="engine setting: how the colour of a yuva* / gbrapf32le source stands to its alpha (DESIGN.md 3.18). "
                         "premultiplied = divide by alpha in front of lut3d and multiply behind it, inside the LUT pass (OpenEXR, "
                         "most ProRes 4444 elements); not with dither, --chroma-loc, --out-size, --second-output, --cube2, a "
                         "full-range source or an RGB source into YUV")
    ap.add_argument("--out-size", default=None, metavar="WxH",
                    help="engine setting: resize the output frames to WxH on the GPU after the LUT (the reference's -s, "
                         "DESIGN.md 3.7); frames on -o have this size")
    ap.add_argument("--second-output", default=None, metavar="PATH",
                    help="engine setting: write a second rawvideo output from the same LUT pass (DESIGN.md 3.13) to this file or "
                         "FIFO (not -); needs --second-pix-fmt")
    ap.add_argument("--second-pix-fmt", default=None, metavar="FMT",
                    help="planar YUV format of --second-output; it may differ from --out-pix-fmt in depth and chroma subsampling")
    ap.add_argument("--cube2", default=None, metavar="PATH",
                    help="engine setting: a second LUT applied behind --cube in the same pass (DESIGN.md 3.17; ffmpeg's "
                         "lut3d=A,lut3d=B): planar YUV without alpha on both sides, no prelut on this LUT, no dither, "
                         "--chroma-loc, --out-size or --second-output")
    ap.add_argument("--interp2", default=None, metavar="MODE", help="interpolation mode of --cube2 (default: --interp)")
    ap.add_argument("--cdl", default=None, metavar="FILE",
                    help="engine setting: an ASC CDL (.cc / .ccc / .cdl) applied to the RGB ahead of --cube in the same pass "
                         "(DESIGN.md 3.19): planar YUV on both sides, no .csp prelut, dither, --chroma-loc, --out-size, "
                         "--second-output, --cube2 or --alpha-mode premultiplied")
    ap.add_argument("--cdl-id", default=None, metavar="ID", help="the id of the ColorCorrection to take from --cdl")
    ap.add_argument("--cdl-sop", default=None, metavar="\"S S S O O O P P P\"",
                    help="the CDL as literal values instead of a file: slope R G B, offset R G B, power R G B")
    ap.add_argument("--cdl-sat", default=None, type=float, metavar="X", help="the CDL's saturation as a literal value (default 1)")
    ap.add_argument("--lut1d", default=None, metavar="PATH",
                    help="engine setting: a 1D LUT (.cube with LUT_1D_SIZE) applied to the RGB ahead of --cube in the same pass "
                         "(DESIGN.md 3.20; ffmpeg's lut1d=A,lut3d=B), or alone without --cube: planar YUV on both sides, no dither, "
                         "--chroma-loc, --out-size, --cdl, --cube2, --second-output or --alpha-mode premultiplied")
    ap.add_argument("--interp1d", default="linear", metavar="MODE",
                    help="interpolation mode of --lut1d: nearest | linear | cosine | cubic | spline (default linear)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--stages", default=None, metavar="LIST",
                    help="engine setting: run --cube (lut3d), --cube2 (lut3d2), --lut1d (lut1d) and --cdl / --cdl-sop / --cdl-sat (cdl) "
                         "as an ordered stack in ONE pass (DESIGN.md 3.21), e.g. lut1d,cdl,lut3d:trilinear; each kind once, 1 to 4 "
                         "stages, a lut3d stage without a mode takes --interp / --interp2; every stage needs its file and every "
                         "file its stage; planar YUV on both sides, no dither, --chroma-loc, --out-size, --second-output or "
                         "--alpha-mode premultiplied")
    ap.add_argument("--rgb-stages", default=None, metavar="LIST",
                    help="engine setting: --stages for an RGB --pix-fmt (gbrp*, gbrap*, rgb24 .. rgba64le; DESIGN.md 3.26): the same "
                         "lists and files, run on the source's own codes in ONE pass into a planar YUV --out-pix-fmt, or into gbrp* "
                         "at the source's depth (the default for a planar source); no dither, --chroma-loc, --out-size, --strength, "
                         "--matte, --second-output or --alpha-mode premultiplied; not together with --stages")
    ap.add_argument("--rgb-out-stages", default=None, metavar="LIST",
                    help="engine setting: --stages for a planar YUV --pix-fmt with --rgb-out (DESIGN.md 3.27): the same lists and "
                         "files, run at the depth of --rgb-out in ONE pass between the conversion to RGB and the stores, e.g. "
                         "--rgb-out rgb48le --rgb-out-stages lut1d,cdl,lut3d; needs --rgb-out; no dither, --chroma-loc, --out-size, "
                         "--strength, --matte, --second-output or --alpha-mode premultiplied; not together with --stages or "
                         "--rgb-stages")
    ap.add_argument("--semi-stages", default=None, metavar="LIST",
                    help="engine setting: --stages for a call with a semi-planar side (--pix-fmt, --out-pix-fmt or both one of nv12, "
                         "nv21, nv16, p010le .. p216le; DESIGN.md 3.28): the same lists and files without the matrix stage, in ONE "
                         "pass with no de-interleave ahead of it and no interleave behind it; the other side may be planar 4:2:0 / "
                         "4:2:2 / 4:4:4, e.g. --pix-fmt p010le --out-pix-fmt yuv422p10le --semi-stages lut1d,cdl,lut3d; no dither, "
                         "--chroma-loc, --out-size, --strength, --matte, --second-output or --alpha-mode premultiplied; not "
                         "together with --stages, --rgb-stages or --rgb-out-stages")
    ap.add_argument("--packed-stages", default=None, metavar="LIST",
                    help="engine setting: --stages for a call with a packed 4:2:2 or v210 side (--pix-fmt, --out-pix-fmt or both one "
                         "of yuyv422, uyvy422, yvyu422, y210le, y212le, y216le, or v210; DESIGN.md 3.29): the same lists and files "
                         "without the matrix stage, in ONE pass with no unpacking ahead of it and no packing behind it; a packed / "
                         "v210 source may go to planar 4:2:2 / 4:2:0 / 4:4:4, e.g. --pix-fmt v210 --out-pix-fmt yuv422p10le "
                         "--packed-stages lut1d,cdl,lut3d; no dither, --chroma-loc, --out-size, --strength, --matte, "
                         "--second-output or --alpha-mode premultiplied; not together with --stages, --rgb-stages, "
                         "--rgb-out-stages or --semi-stages")
    ap.add_argument("--rgb-matrix", default=None, metavar="\"M00 M01 M02 M10 .. M22\"",
                    help="engine setting: the nine numbers, row-major, of the RGB matrix a 'matrix' stage of --stages applies "
                         "(DESIGN.md 3.25; a gamut conversion, a white-balance or channel-mixer trim, a channel swap): "
                         "clamp(M * rgb + offset, 0, 1) on unit RGB, e.g. --stages lut1d,matrix,lut3d.  Needs --stages with a "
                         "matrix stage; not together with --strength or --matte")
    ap.add_argument("--rgb-matrix-offset", default=None, metavar="\"O O O\"",
                    help="the offset of --rgb-matrix in unit floats (default 0 0 0)")
    ap.add_argument("--rgb-matrix-file", default=None, metavar="PATH",
                    help="the matrix of a 'matrix' stage from a .spimtx file (twelve numbers, row-major 3 x 4, the offset column in "
                         "16-bit codes) instead of --rgb-matrix / --rgb-matrix-offset")
    mix = ap.add_mutually_exclusive_group()
    mix.add_argument("--strength", default=None, type=float, metavar="X",
                     help="engine setting: LUT strength in [0, 1] (DESIGN.md 3.22; the intensity / opacity control of a grade) -- "
                          "the graded pixel is mixed with the source as RGB codes behind the stages, in the same pass: 1 = the "
                          "look, 0 = the source.  Runs the stage stack: with --stages that list, without it the list the other "
                          "options imply (lut1d, cdl, lut3d, lut3d2 in that order), on the stack's terms")
    mix.add_argument("--strength-keys", default=None, metavar="F:S,F:S,...",
                     help="engine setting: LUT strength by key frames -- frame F of the stream (counted from 0 across batches) "
                          "takes strength S, linear between the keys, held before the first and behind the last; e.g. 0:0,24:1 "
                          "ramps the look in over the first second.  Not together with --strength")
    ap.add_argument("--matte", default=None, metavar="PATH",
                    help="engine setting: a matte plane (DESIGN.md 3.23; a key, a power window, a wipe) -- raw gray frames of "
                         "--size, read in lockstep with the input; the strength of a pixel is --strength (1 when not given) times "
                         "its matte sample over the largest code, applied in RGB in the same pass.  A regular file of exactly one "
                         "frame is a still for the whole stream; a matte that ends before the input is an error.  A file or FIFO, "
                         "not '-'.  Runs the stage stack, as --strength does")
    ap.add_argument("--matte-pix-fmt", default=None, metavar="FMT",
                    help="pixel format of --matte: gray | gray10le | gray12le | gray14le | gray16le (default gray)")
    ap.add_argument("--matte-invert", action="store_true", help="use the largest code minus the matte sample (an outside window)")
    ap.add_argument("-y", action="store_true", help="overwrite the output (ffmpeg's -y)")
    ap.add_argument("--duration", type=float, default=None,
                    help="seconds of video, for the Duration: line when the input is a pipe (-i -) and cannot be measured")
    return ap


def cdl_from_args(args):
    """The `cdl.Cdl` the options name, or None: --cdl FILE [--cdl-id ID], or --cdl-sop / --cdl-sat; a file and literal values
    together are an error."""
    path, cc_id = getattr(args, "cdl", None), getattr(args, "cdl_id", None)
    sop, sat = getattr(args, "cdl_sop", None), getattr(args, "cdl_sat", None)
    if path is not None and (sop is not None or sat is not None):
        raise ValueError("--cdl names a file and --cdl-sop / --cdl-sat give literal values: use one or the other")
    if cc_id is not None and path is None:
        raise ValueError("--cdl-id names a correction inside a CDL file: it needs --cdl")
    if path is None and sop is None and sat is None:
        return None
    from .cdl import Cdl, read_cdl
    return read_cdl(path, cc_id) if path is not None else Cdl.from_sop_text(sop, sat)


def rgb_matrix_from_args(args):
    """The `rgbmatrix.RgbMatrix` the options name, or None: --rgb-matrix-file PATH, or --rgb-matrix [--rgb-matrix-offset]; a file
    and literal values together, and an offset without its matrix, are errors."""
    path, m, off = getattr(args, "rgb_matrix_file", None), getattr(args, "rgb_matrix", None), getattr(args, "rgb_matrix_offset", None)
    if path is not None and (m is not None or off is not None):
        raise ValueError("--rgb-matrix-file names a file and --rgb-matrix / --rgb-matrix-offset give literal values: use one or "
                         "the other")
    if off is not None and m is None:
        raise ValueError("--rgb-matrix-offset is the offset of a matrix: it needs --rgb-matrix")
    if path is None and m is None:
        return None
    from .rgbmatrix import RgbMatrix, read_rgb_matrix
    return read_rgb_matrix(path) if path is not None else RgbMatrix.from_text(m, off)


def _stage_list_from_args(args, interp, flag: str, text) -> dict:
    """What --stages, --rgb-stages and --rgb-out-stages (`flag`, its value `text`) share: the list parsed with `interp` (--interp
    as the plan resolved it) / --interp2 as the lut3d stages' defaults, a file for every stage and a stage for every file, and
    what `check_stage_list` and the option checks are told -- dict(stages, cdl, rgb_matrix, mix=the strength, key frames and
    matte that travel with a --stages call, list=the keywords of `check_stage_list`, options=those of the refusals by name)."""
    from .plan import INTERP_WHITELIST
    interp2 = getattr(args, "interp2", None)
    mode2 = None if interp2 is None else interp2 if interp2 in INTERP_WHITELIST else "tetrahedral"
    cube2, lut1d = getattr(args, "cube2", None), getattr(args, "lut1d", None)
    cdl, mtx = cdl_from_args(args), rgb_matrix_from_args(args)
    strength, keys = strength_from_args(args)
    matte = matte_from_args(args)
    st = parse_stages(text, interp=interp, interp2=mode2)
    kinds = [k for k, _m in st]
    for opt, given, kind in (("--cube", args.cube, "lut3d"), ("--cube2", cube2, "lut3d2"), ("--lut1d", lut1d, "lut1d"),
                             ("--cdl / --cdl-sop / --cdl-sat", cdl, "cdl"), ("--rgb-matrix / --rgb-matrix-file", mtx, "matrix")):
        if given is not None and kind not in kinds:
            raise ValueError(f"{opt} is given and {flag} has no '{kind}' stage")
    if interp2 is not None and "lut3d2" not in kinds:
        raise ValueError(f"--interp2 is the mode of the second LUT: {flag} has no 'lut3d2' stage")
    interp1d = getattr(args, "interp1d", None) or "linear"
    from . import _native
    if interp1d not in _native.INTERP1D:
        raise ValueError(f"lut1d has no interpolation mode '{interp1d}' ({' | '.join(_native.INTERP1D)})")
    prelut = False
    if ("cdl" in kinds or "matrix" in kinds) and args.cube is not None and os.path.isfile(args.cube):
        from pathlib import Path
        from . import engine  # noqa: F401  (torch first, as in plan_from_args)
        from .api import _cached_cube
        prelut = getattr(_cached_cube(Path(args.cube)), "prelut", None) is not None
    second_out, second_fmt = getattr(args, "second_output", None), getattr(args, "second_pix_fmt", None)
    mix = dict(matte or {})
    mix.update({k: v for k, v in (("strength", strength), ("strength_keys", keys)) if v is not None})
    return dict(
        stages=st, cdl=cdl, rgb_matrix=mtx, mix=mix,
        list=dict(cdl=cdl is not None, lut=args.cube is not None, lut2=cube2 is not None, lut1d=lut1d is not None, prelut=prelut,
                  rgb_matrix=mtx is not None),
        options=dict(chroma_loc=getattr(args, "chroma_loc", None), out_size=getattr(args, "out_size", None),
                     alpha_mode=getattr(args, "alpha_mode", None) or "straight",
                     out2_pix_fmt=second_fmt if second_fmt is not None else second_out,
                     strength=strength if keys is None else 1.0, matte=matte is not None))


def _stack_call(call: dict, r: dict, list_kw: str) -> dict:
    """`call` with what `_stage_list_from_args` resolved (`r`): the parsed list under `list_kw`, the CDL and the matrix where
    there is one."""
    call[list_kw] = r["stages"]
    call.update({k: r[k] for k in ("cdl", "rgb_matrix") if r[k] is not None})
    return call


def stack_call_from_args(args, kw: dict, cdl) -> dict:
    """The keyword arguments of `apply_yuv_stack` for --stages from those `engine_call_for` returned: the stage
    list parsed with --interp / --interp2 as the lut3d stages' defaults, every refusal of `check_stack_options`, and a file for
    every stage and a stage for every file.  With --strength / --strength-keys and no --stages the list is the
    one the other options imply (`formats.implied_stages`); `strength` or `strength_keys` (the parsed callable) go into the call.
    With --matte likewise; `matte` (the path), `matte_pix_fmt` and `matte_invert` go into the call.  With
    --rgb-matrix / --rgb-matrix-file `rgb_matrix` goes into the call; it needs --stages with a matrix stage."""
    listed = getattr(args, "stages", None)
    if listed is None:
        if rgb_matrix_from_args(args) is not None:
            raise ValueError("--rgb-matrix / --rgb-matrix-file need --stages: a matrix stage has no implied position "
                             "(e.g. --stages lut1d,matrix,lut3d)")
        listed = implied_stages(args.cube is not None, getattr(args, "cube2", None) is not None,
                                getattr(args, "lut1d", None) is not None, cdl is not None)
    r = _stage_list_from_args(args, kw.get("interp"), "--stages", listed)
    check_stack_options(kw["pix_fmt"], kw["out_pix_fmt"], stages=r["stages"], **r["list"],
                        dither="error_diffusion" if args.zscale_dither == "error_diffusion"
                        else getattr(args, "engine_dither", None) or "none",
                        precision=getattr(args, "precision", None), **r["options"])
    call = {k: v for k, v in kw.items() if k not in ("interp", "alpha_mode", "dither")}
    return dict(_stack_call(call, r, "stages"), **r["mix"])


def rgb_stack_call_from_args(args, plan) -> dict:
    """The keyword arguments of `apply_rgb_stack` for --rgb-stages, with `pix_fmt` / `out_pix_fmt` as every
    call of `plan_from_args` carries them and the parsed list under `rgb_stages`: the list parsed with --interp / --interp2 as
    the lut3d stages' defaults, every refusal of `check_rgb_stack_options`, and a file for every stage and a stage for every
    file."""
    if getattr(args, "stages", None) is not None:
        raise ValueError("--stages and --rgb-stages are mutually exclusive: --stages is the list of a YUV source, --rgb-stages "
                         "that of an RGB source")
    if getattr(args, "rgb_out", None) is not None:
        raise ValueError("--rgb-out names the RGB output of a YUV source: with --rgb-stages the output is --out-pix-fmt")
    r = _stage_list_from_args(args, plan.interp, "--rgb-stages", args.rgb_stages)
    _st, _fin, fout = check_rgb_stack_options(
        args.pix_fmt, args.out_pix_fmt, stages=r["stages"], **r["list"],
        dither="error_diffusion" if args.zscale_dither == "error_diffusion" else getattr(args, "engine_dither", None) or "none",
        intermediate_pix_fmt=plan.intermediate_pix_fmt if plan.prologue else None, **r["options"])
    return _stack_call(dict(pix_fmt=args.pix_fmt, out_pix_fmt=fout.name, matrix_out=plan.matrix or "smpte170m", range_out="tv"),
                       r, "rgb_stages")


def rgb_out_stack_call_from_args(args, plan) -> dict:
    """The keyword arguments of `apply_yuv_stack_to_rgb` for --rgb-out FMT --rgb-out-stages LIST, with
    `pix_fmt` / `out_pix_fmt` (= FMT) as every call of `plan_from_args` carries them and the parsed list under `rgb_out_stages`:
    the list as --rgb-stages parses it, every refusal of `check_yuv2rgb_stack_options`, the matrix and ranges of --rgb-out."""
    from .api import engine_call_for
    if getattr(args, "stages", None) is not None or getattr(args, "rgb_stages", None) is not None:
        raise ValueError("--rgb-out-stages and --stages / --rgb-stages are mutually exclusive: --stages is the list of a YUV source "
                         "with a YUV output, --rgb-stages that of an RGB source, --rgb-out-stages that of a YUV source with --rgb-out")
    if getattr(args, "rgb_out", None) is None:
        raise ValueError("--rgb-out-stages is the stage list of a YUV source written as RGB: it needs --rgb-out")
    if args.out_pix_fmt:
        raise ValueError(f"rgb_out ('{args.rgb_out}') and out_pix_fmt ('{args.out_pix_fmt}') are mutually exclusive: a call has one "
                         f"output")
    r = _stage_list_from_args(args, plan.interp, "--rgb-out-stages", args.rgb_out_stages)
    check_yuv2rgb_stack_options(args.pix_fmt, args.rgb_out, stages=r["stages"], **r["list"],
                                dither="error_diffusion" if args.zscale_dither == "error_diffusion" else "none",
                                engine_dither=getattr(args, "engine_dither", None), **r["options"])
    call = {k: v for k, v in engine_call_for(plan, args.pix_fmt, None, "straight", rgb_out=args.rgb_out).items() if k != "interp"}
    return _stack_call(call, r, "rgb_out_stages")


def semi_stack_call_from_args(args, plan) -> dict:
    """The keyword arguments of `apply_yuv_stack_semi` for --semi-stages, with `pix_fmt` / `out_pix_fmt` as every
    call of `plan_from_args` carries them and the parsed list under `semi_stages`: the list as --stages parses it, every refusal
    of `check_semi_stack_options`, the matrices and ranges `engine_call_for` gives the plan."""
    from .api import engine_call_for
    from .formats import SEMI_STAGES_EXCLUSIVE, check_semi_stack_options
    if any(getattr(args, k, None) is not None for k in ("stages", "rgb_stages", "rgb_out_stages")):
        raise ValueError(SEMI_STAGES_EXCLUSIVE)
    if getattr(args, "rgb_out", None) is not None:
        raise ValueError("--rgb-out names the RGB output of a planar YUV source: with --semi-stages the output is --out-pix-fmt")
    r = _stage_list_from_args(args, plan.interp, "--semi-stages", args.semi_stages)
    _st, fin, fout = check_semi_stack_options(
        args.pix_fmt, args.out_pix_fmt, stages=r["stages"], **r["list"],
        dither="error_diffusion" if args.zscale_dither == "error_diffusion" else getattr(args, "engine_dither", None) or "none",
        precision=getattr(args, "precision", None), **r["options"])
    kw = engine_call_for(plan, args.pix_fmt, args.out_pix_fmt, "straight", semi_stack=True)
    call = {k: v for k, v in kw.items() if k not in ("interp", "alpha_mode", "dither")}
    return _stack_call(call, r, "semi_stages")


def packed_stack_call_from_args(args, plan) -> dict:
    """The keyword arguments of `apply_yuv_stack_packed` for --packed-stages, with `pix_fmt` / `out_pix_fmt` as
    every call of `plan_from_args` carries them and the parsed list under `packed_stages`: the list as --stages parses it, every
    refusal of `check_packed_stack_options`, the matrices and ranges `engine_call_for` gives the plan."""
    from .api import engine_call_for
    from .formats import PACKED_STAGES_EXCLUSIVE, check_packed_stack_options
    if any(getattr(args, k, None) is not None for k in ("stages", "rgb_stages", "rgb_out_stages", "semi_stages")):
        raise ValueError(PACKED_STAGES_EXCLUSIVE)
    if getattr(args, "rgb_out", None) is not None:
        raise ValueError("--rgb-out names the RGB output of a planar YUV source: with --packed-stages the output is --out-pix-fmt")
    r = _stage_list_from_args(args, plan.interp, "--packed-stages", args.packed_stages)
    check_packed_stack_options(
        args.pix_fmt, args.out_pix_fmt, stages=r["stages"], **r["list"],
        dither="error_diffusion" if args.zscale_dither == "error_diffusion" else getattr(args, "engine_dither", None) or "none",
        precision=getattr(args, "precision", None), **r["options"])
    kw = engine_call_for(plan, args.pix_fmt, args.out_pix_fmt, "straight", packed_stack=True)
    call = {k: v for k, v in kw.items() if k not in ("interp", "alpha_mode", "dither")}
    return _stack_call(call, r, "packed_stages")


def matte_from_args(args):
    """None without --matte, else dict(matte=the path, matte_pix_fmt=, matte_invert=); --matte-pix-fmt / --matte-invert without
    --matte, '-' and an unknown format are errors."""
    from .formats import MATTE_PIX_FMTS
    path, fmt, invert = getattr(args, "matte", None), getattr(args, "matte_pix_fmt", None), bool(getattr(args, "matte_invert", False))
    if path is None:
        if fmt is not None or invert:
            raise ValueError("--matte-pix-fmt / --matte-invert describe a matte: they need --matte")
        return None
    if str(path) == "-":
        raise ValueError("--matte is a file or FIFO, not '-': stdin carries the input")
    fmt = fmt or "gray"
    if fmt not in MATTE_PIX_FMTS:
        raise ValueError(f"unknown --matte-pix-fmt '{fmt}' ({' | '.join(MATTE_PIX_FMTS)})")
    return dict(matte=str(path), matte_pix_fmt=fmt, matte_invert=invert)


def strength_from_args(args):
    """(--strength as a float or None, --strength-keys as `params.strength_keys`' callable or None); both together are an error
    (the parser refuses them already; a namespace made by hand gets here)."""
    strength, text = getattr(args, "strength", None), getattr(args, "strength_keys", None)
    if strength is not None and text is not None:
        raise ValueError("--strength and --strength-keys are mutually exclusive")
    if text is None:
        return strength, None
    from .params import strength_keys
    return None, strength_keys(text)


def plan_from_args(args):
    """The LutPlan and engine call the options select -- the same resolution `build_command` performs (plan.py)."""
    from .api import engine_call_for
    from .params import ProcessingParams, VideoInfo
    from .plan import resolve_lut_plan
    w, h = (int(v) for v in args.size.lower().split("x"))
    params = ProcessingParams(lut_interp=args.interp, lut_input_matrix=args.input_matrix,
                              lut_output_tags=args.output_tags, zscale_dither=args.zscale_dither)
    info = VideoInfo(width=w, height=h, pix_fmt=args.pix_fmt, bit_depth=source_bit_depth(args.pix_fmt),
                     colorspace=args.colorspace, color_range=args.color_range)
    lut1d = getattr(args, "lut1d", None)
    stages = getattr(args, "stages", None)
    rgb_stages = getattr(args, "rgb_stages", None)
    rgb_out_stages = getattr(args, "rgb_out_stages", None)
    semi_stages = getattr(args, "semi_stages", None)
    packed_stages = getattr(args, "packed_stages", None)
    if args.cube is None and lut1d is None and stages is None and rgb_stages is None and rgb_out_stages is None and semi_stages is None \
            and packed_stages is None:
        raise ValueError("--cube is required unless --lut1d is given")
    plan = resolve_lut_plan(params, args.cube if args.cube is not None else "engine.cube", info)
    alpha_mode = getattr(args, "alpha_mode", None) or "straight"
    rgb_out = getattr(args, "rgb_out", None)
    if packed_stages is not None:
        # the stage stack on packed 4:2:2 / v210 sides: a route of its own
        return plan, packed_stack_call_from_args(args, plan), w, h
    if semi_stages is not None:
        # the stage stack on semi-planar sides: a route of its own
        return plan, semi_stack_call_from_args(args, plan), w, h
    if rgb_out_stages is not None:
        # the stage stack from a YUV source into an RGB frame: a route of its own
        return plan, rgb_out_stack_call_from_args(args, plan), w, h
    if rgb_stages is not None:
        # the stage stack on an RGB source: a route of its own
        return plan, rgb_stack_call_from_args(args, plan), w, h
    if rgb_out is not None:
        # YUV in, RGB out: a route of its own, with none of the options below
        from .formats import check_yuv2rgb_options
        kw = engine_call_for(plan, args.pix_fmt, args.out_pix_fmt, alpha_mode, rgb_out=rgb_out)
        second = getattr(args, "second_pix_fmt", None)
        check_yuv2rgb_options(args.pix_fmt, rgb_out, chroma_loc=getattr(args, "chroma_loc", None),
                              dither="error_diffusion" if args.zscale_dither == "error_diffusion" else "none",
                              engine_dither=getattr(args, "engine_dither", None), out_size=getattr(args, "out_size", None),
                              cdl=cdl_from_args(args), lut1d=lut1d, stages=stages, strength=getattr(args, "strength", None),
                              strength_keys=getattr(args, "strength_keys", None), matte=getattr(args, "matte", None),
                              out2_pix_fmt=second if second is not None else getattr(args, "second_output", None),
                              cube2=getattr(args, "cube2", None), interp2=getattr(args, "interp2", None))
        return plan, kw, w, h
    if stages is None and rgb_matrix_from_args(args) is not None:
        raise ValueError("--rgb-matrix / --rgb-matrix-file need --stages: a matrix stage has no implied position "
                         "(e.g. --stages lut1d,matrix,lut3d)")
    kw = engine_call_for(plan, args.pix_fmt, args.out_pix_fmt, alpha_mode)
    from .api import is_float_out_call
    engine_dither = getattr(args, "engine_dither", None)
    if "alpha_mode" in kw:
        check_premul_options(kw["pix_fmt"], kw["out_pix_fmt"], chroma_loc=getattr(args, "chroma_loc", None),
                             dither="error_diffusion" if args.zscale_dither == "error_diffusion" else engine_dither or "none",
                             out_size=getattr(args, "out_size", None), range_src=kw.get("range_src", "tv"),
                             range_in=kw.get("range_in"), lut_depth=kw.get("lut_depth"),
                             out2_pix_fmt=getattr(args, "second_pix_fmt", None), lut2=getattr(args, "cube2", None) is not None)
    cdl = cdl_from_args(args)
    mixed = getattr(args, "strength", None) is not None or getattr(args, "strength_keys", None) is not None
    mixed = mixed or matte_from_args(args) is not None
    if stages is not None or mixed:
        return plan, stack_call_from_args(args, kw, cdl), w, h
    if lut1d is not None:
        check_lut1d_options(kw["pix_fmt"], kw["out_pix_fmt"], interp1d=getattr(args, "interp1d", None) or "linear",
                            chroma_loc=getattr(args, "chroma_loc", None),
                            dither="error_diffusion" if args.zscale_dither == "error_diffusion" else engine_dither or "none",
                            out_size=getattr(args, "out_size", None), alpha_mode=alpha_mode,
                            out2_pix_fmt=getattr(args, "second_pix_fmt", None), lut2=getattr(args, "cube2", None) is not None,
                            cdl=cdl is not None)
        if args.cube is None:
            kw["interp"] = None                               # lut1d alone
    if cdl is not None:
        prelut = False
        if os.path.isfile(args.cube):                         # (a LUT that is not there yet is met again where it is loaded)
            from pathlib import Path
            # torch first, as everywhere else: parsing loads liblutr, which must find the HIP runtime torch brings and not load
            # a second one into the process (the second cannot open the device)
            from . import engine  # noqa: F401
            from .api import _cached_cube
            prelut = getattr(_cached_cube(Path(args.cube)), "prelut", None) is not None
        check_cdl_options(kw["pix_fmt"], kw["out_pix_fmt"], chroma_loc=getattr(args, "chroma_loc", None),
                          dither="error_diffusion" if args.zscale_dither == "error_diffusion" else engine_dither or "none",
                          out_size=getattr(args, "out_size", None), alpha_mode=alpha_mode,
                          out2_pix_fmt=getattr(args, "second_pix_fmt", None), lut2=getattr(args, "cube2", None) is not None,
                          prelut=prelut)
        kw["cdl"] = cdl
    if is_float_out_call(kw) and (args.zscale_dither == "error_diffusion" or engine_dither or getattr(args, "out_size", None)):
        raise ValueError("a float output takes no dither and no --out-size")
    if args.zscale_dither == "error_diffusion":
        kw["dither"] = "error_diffusion"
    if engine_dither:
        from .api import resolve_engine_dither
        kw["dither"] = resolve_engine_dither(engine_dither, kw.get("dither", "none"))
    from .api import is_rgb_call
    if getattr(args, "chroma_loc", None) and is_rgb_call(kw):
        raise ValueError("chroma siting (--chroma-loc) is not defined for an RGB source")
    if not is_rgb_call(kw):
        check_container_options(kw["pix_fmt"], kw["out_pix_fmt"], kw.get("dither", "none"), getattr(args, "chroma_loc", None),
                                getattr(args, "out_size", None))
    if getattr(args, "chroma_loc", None):
        check_chroma_loc(args.chroma_loc, kw.get("dither", "none"), kw["pix_fmt"], kw["out_pix_fmt"])
        kw["chroma_loc"] = args.chroma_loc
    if getattr(args, "out_size", None):
        parse_size(args.out_size)
        refuse_alpha_resize(kw.get("out_pix_fmt"), args.out_size)
    second_out, second_fmt = getattr(args, "second_output", None), getattr(args, "second_pix_fmt", None)
    if (second_out is None) != (second_fmt is None):
        raise ValueError("--second-output and --second-pix-fmt go together: give both or neither")
    if second_out is not None:
        if second_out == "-":
            raise ValueError("--second-output is a file or FIFO, not '-': stdout carries the first output or the report")
        if args.output != "-" and os.path.realpath(second_out) == os.path.realpath(args.output):
            raise ValueError("--second-output names the same file as -o: the two outputs need a file each")
        from .api import dual_call_for
        if getattr(args, "cube2", None) is None:
            kw = dual_call_for(kw, second_fmt, kw.get("chroma_loc"), getattr(args, "out_size", None))
    cube2, interp2 = getattr(args, "cube2", None), getattr(args, "interp2", None)
    if cube2 is None and interp2 is not None:
        raise ValueError("--interp2 is the mode of the second LUT: it needs --cube2")
    if cube2 is not None:
        from .api import chain_call_for
        chroma_loc = kw.pop("chroma_loc", None)
        kw = chain_call_for(kw, interp2, chroma_loc, getattr(args, "out_size", None), second_fmt)
    return plan, kw, w, h


def main(argv=None) -> int:
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.cube is None and args.lut1d is None and args.stages is None and args.rgb_stages is None and args.rgb_out_stages is None \
            and args.semi_stages is None and args.packed_stages is None:
        ap.error("the following arguments are required: --cube (or --lut1d for a 1D LUT alone)")

    stop = {"flag": False}
    signal.signal(signal.SIGTERM, lambda *_: stop.__setitem__("flag", True))
    try:
        piped_in, piped_out = args.input == "-", args.output == "-"
        # with frames on stdout the report goes to stderr (the caller merges the two, task_manager.py:145-151)
        report = sys.stderr if piped_out else sys.stdout

        def say(text):
            print(text, file=report, flush=True)

        if not piped_out and os.path.exists(args.output) and not args.y:
            raise FileExistsError(f"{args.output} exists (pass -y to overwrite)")
        plan, kw, w, h = plan_from_args(args)
        second = args.second_output
        if second is not None and os.path.isfile(second) and not args.y:
            raise FileExistsError(f"{second} exists (pass -y to overwrite)")
        from .cube import read_lut, read_lut1d
        from .engine import LutEngine
        from .stream import HostPipeline, MatteReader

        lut2 = None if args.cube2 is None else read_lut(args.cube2)
        check_lut2(lut2)
        eng = LutEngine(args.device)
        eng.set_precision(args.precision)
        if args.cube is not None:
            eng.set_lut(read_lut(args.cube))
        if lut2 is not None:
            eng.set_lut2(lut2)
        if args.lut1d is not None:
            eng.set_lut1d(read_lut1d(args.lut1d), args.interp1d)
        from .api import is_rgb_out_call
        rgb_out = kw["out_pix_fmt"] if is_rgb_out_call(kw) else None
        pix_fmt, out_fmt = kw.pop("pix_fmt"), kw.pop("out_pix_fmt")
        if rgb_out is not None:
            out_fmt = None
        second_fmt = kw.pop("out2_pix_fmt", None)
        if "matte" in kw:
            kw["matte"] = MatteReader(kw.pop("matte"), kw.pop("matte_pix_fmt"), w, h)
        stacked = any(k in kw for k in ("stages", "rgb_stages", "rgb_out_stages", "semi_stages", "packed_stages"))   # (the list names its lut3d2 / lut1d stages)
        pipe = HostPipeline(eng, pix_fmt, w, h, batch=args.batch, out_pix_fmt=out_fmt, out_size=args.out_size,
                            second_pix_fmt=second_fmt, chain=lut2 is not None and not stacked,
                            lut1d=args.lut1d is not None and not stacked, rgb_out=rgb_out, **kw)
        fb = pipe.fin.frame_bytes
        if piped_in:
            total = None if args.duration is None else max(1, int(round(args.duration * args.fps)))
        else:
            total = os.path.getsize(args.input) // fb
            if total == 0:
                raise ValueError(f"{args.input}: no complete {w}x{h} {args.pix_fmt} frame ({fb} bytes each)")
        say(f"Input #0, rawvideo, from '{'pipe:0' if piped_in else args.input}':")
        if total is not None:
            say(f"  Duration: {_hms(total / args.fps)}, {total} frames, {w}x{h} {args.pix_fmt}")
        else:
            say(f"  Duration: N/A, {w}x{h} {args.pix_fmt}")
        for note in plan.notes:
            say(f"  {note}")
        t0 = time.time()
        state = {"done": 0}
        fi = sys.stdin.buffer if piped_in else open(args.input, "rb")
        fo = sys.stdout.buffer if piped_out else open(args.output, "wb")
        fo2 = None
        try:
            if second is not None:
                fo2 = open(second, "wb")

            def fill(buf, max_frames):
                view, got = memoryview(buf)[: max_frames * fb], 0
                while got < len(view):                       # a pipe returns short reads: collect the whole batch (or EOF)
                    n = fi.readinto(view[got:])
                    if not n:
                        break
                    got += n
                return got // fb                             # a trailing partial frame is dropped

            def drain(buf, n):
                fo.write(memoryview(buf))
                state["done"] += n
                el = max(time.time() - t0, 1e-9)
                say(f"frame={state['done']:6d} fps={state['done'] / el:7.1f} time={_hms(state['done'] / args.fps)}")

            pipe.run(fill, drain, total_frames=None if piped_in else total, stop=lambda: stop["flag"],
                     drain2=None if fo2 is None else lambda buf, n: fo2.write(memoryview(buf)))
            fo.flush()
        finally:
            if fo2 is not None:
                fo2.close()
            if not piped_in:
                fi.close()
            if not piped_out:
                fo.close()
        eng.close()
        if stop["flag"]:
            say("Exiting normally, received signal 15.")
            return 255
        say(f"video: {state['done']} frames written to '{'pipe:1' if piped_out else args.output}'")
        return 0
    except Exception as exc:  # the caller only sees text + exit code (task_manager.py:105-112)
        print(f"Error: {exc}", file=sys.stderr if getattr(args, "output", "") == "-" else sys.stdout, flush=True)
        return 1


if __name__ == "__main__":
    sys.exit(main())
