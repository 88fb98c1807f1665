"""decode -> raw pipe -> engine -> raw pipe -> encode: the LUT stage of a task run on the GPU engine with ffmpeg on both sides.

The reference runs ONE ffmpeg process per stage whose filtergraph does decode, `lut3d` and encode together
(`/root/reference/src/lut_renderer/ffmpeg.py:179-414`, spawned at `task_manager.py:134-190`).  With the per-pixel work moved to
`liblutr.so`, the same stage is three processes joined by OS pipes:

    ffmpeg -i SRC -f rawvideo -pix_fmt <src fmt> pipe:1          (decoder: the reference's input options, no filters)
      | python -m lut_renderer_amd.cli -i - -o - ...               (engine: `command.engine_command`, the same LutPlan)
      | ffmpeg -f rawvideo -pix_fmt <out fmt> -s WxH -r NUM/DEN -i pipe:0 -i SRC -map 0:v:0 -map 1:a? -map 1:s?
               -map_metadata 1 -map_chapters 1 <the reference's codec / rate / tag options> OUT

The encoder reads the source a second time for everything that is not video: the reference's single ffmpeg process carries the
source's audio (its `-c:a copy` / aac options), subtitles, chapters and container metadata into the output, and a raw pipe has
none of them.  The frame rate travels as the rational ffprobe reported (30000/1001, not 29.97).

`engine_stage_commands` derives all three argv lists from the arguments `build_command` takes; the encoder's options are what
`build_command` itself emits once the `-vf` chain is taken out (the engine has already applied it, including `format=`).
`run_stage` starts them, relays the engine's `Duration:` / `time=` lines and the three exit codes the way `TaskRunner._run_stage`
expects from a single child (non-zero if any stage failed; SIGTERM stops all three), so
`python -m lut_renderer_amd.pipe ...` can stand where `ffmpeg` stands in `CommandStage`.

There is no ffmpeg binary in this image: the tests drive the wrapper with `cat` on both sides.
"""
from __future__ import annotations

import signal
import subprocess
import sys
import threading
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional

from .command import build_command, engine_command, fps_rational
from .params import ProcessingParams, VideoInfo
from .plan import resolve_pix_fmt


@dataclass
class StageCommands:
    decoder: List[str]
    engine: List[str]
    encoder: List[str]
    notes: List[str]


def engine_stage_commands(source: Path, output: Path, params: ProcessingParams, lut_path: Path, source_info: VideoInfo,
                          ffmpeg_bin: str = "ffmpeg", python_bin: Optional[str] = None, device: int = 0,
                          precision: str = "strict", chroma_loc: Optional[str] = None, gpu_resize: bool = False,
                          engine_dither: Optional[str] = None, cube2: Optional[Path] = None,
                          interp2: Optional[str] = None, alpha_mode: str = "straight", cdl=None,
                          cdl_id: Optional[str] = None, lut1d: Optional[Path] = None,
                          interp1d: Optional[str] = None, stages=None, strength: Optional[float] = None,
                          strength_keys: Optional[str] = None, matte: Optional[Path] = None,
                          matte_pix_fmt: Optional[str] = None, matte_invert: bool = False, rgb_matrix=None,
                          rgb_stages=None, rgb_out: Optional[str] = None, rgb_out_stages=None,
                          semi_stages=None) -> StageCommands:
    """The three argv lists of one LUT stage.  Raises what `build_command` / `engine_command` raise (copy guard, missing
    geometry).  `chroma_loc` goes to the engine (`--chroma-loc`) and, as `-chroma_sample_location`, to the encoder, so the
    output stream declares the siting the engine assumed.  `gpu_resize` with `params.resolution` set resizes in the engine
    (`--out-size`): the raw input's `-s` is then the target size and the encoder's own `-s` is dropped.  `engine_dither` goes to
    the engine (`--engine-dither`), and so do `cube2` / `interp2` (`--cube2`, `--interp2`: a second LUT in the same
    pass).  `alpha_mode` ("premultiplied") goes to the engine alone (`--alpha-mode`): ffmpeg's chain
    has no such step, so the decoder and encoder argv are untouched.  The same holds for `cdl` / `cdl_id` (an ASC CDL ahead of the
    LUT, DESIGN.md 3.19: `--cdl` / `--cdl-id`, or `--cdl-sop` / `--cdl-sat` for a `cdl.Cdl`) and for `lut1d` / `interp1d` (a 1D LUT
    file ahead of the LUT, DESIGN.md 3.20: `--lut1d` / `--interp1d`), and for `stages` (these operators as an ordered stack in one
    pass, DESIGN.md 3.21: `--stages`, rendered only when given), and for `strength` / `strength_keys` (the LUT's strength, DESIGN.md
    3.22: `--strength` / `--strength-keys`, rendered only when given; the key frames count the frames of the stream), and for `matte` /
    `matte_pix_fmt` / `matte_invert` (a matte plane, DESIGN.md 3.23: `--matte` / `--matte-pix-fmt` / `--matte-invert`, rendered only
    when given; the matte file is raw gray frames at the size of the decoded source), and for `rgb_matrix` (the matrix of a
    `matrix` stage of `stages`, DESIGN.md 3.25: `--rgb-matrix` / `--rgb-matrix-offset` for an `rgbmatrix.RgbMatrix`,
    `--rgb-matrix-file` for a path, rendered only when given), and for `rgb_stages` (the stack on an RGB source, DESIGN.md 3.26:
    `--rgb-stages`, rendered only when given), and for `rgb_out` with `rgb_out_stages` (the stack from a YUV source into an RGB
    frame, DESIGN.md 3.27: `--rgb-out` / `--rgb-out-stages`, rendered only when given; the encoder then reads raw `rgb_out` frames),
    and for `semi_stages` (the stack on semi-planar sides, DESIGN.md 3.28: `--semi-stages`, rendered only when given)."""
    notes: List[str] = []
    engine = engine_command(Path("-"), Path("-"), params, lut_path, source_info, python_bin=python_bin, device=device, notes=notes,
                            precision=precision, chroma_loc=chroma_loc, gpu_resize=gpu_resize, engine_dither=engine_dither,
                            cube2=cube2, interp2=interp2, alpha_mode=alpha_mode, cdl=cdl, cdl_id=cdl_id, lut1d=lut1d,
                            interp1d=interp1d, **({} if stages is None else {"stages": stages}),
                            **({} if strength is None else {"strength": strength}),
                            **({} if strength_keys is None else {"strength_keys": strength_keys}),
                            **({} if matte is None and matte_pix_fmt is None and not matte_invert else
                               {"matte": matte, "matte_pix_fmt": matte_pix_fmt, "matte_invert": matte_invert}),
                            **({} if rgb_matrix is None else {"rgb_matrix": rgb_matrix}),
                            **({} if rgb_stages is None else {"rgb_stages": rgb_stages}),
                            **({} if rgb_out is None and rgb_out_stages is None else {"rgb_out": rgb_out, "rgb_out_stages": rgb_out_stages}),
                            **({} if semi_stages is None else {"semi_stages": semi_stages}))
    resized = gpu_resize and bool(params.resolution)
    if source_info.duration:
        engine += ["--duration", f"{float(source_info.duration):.3f}"]
    decoder = [ffmpeg_bin, "-hide_banner", "-nostdin", "-i", str(source), "-map", "0:v:0", "-f", "rawvideo",
               "-pix_fmt", str(source_info.pix_fmt), "pipe:1"]
    # the encoder side: build_command's own argv for this task WITHOUT a LUT (no -vf chain), reading raw frames from the pipe
    out_fmt = resolve_pix_fmt(params, source_info, []) if params.video_codec else ""
    if not out_fmt:
        out_fmt = str(source_info.pix_fmt)
        if engine.count("--out-pix-fmt"):
            out_fmt = engine[engine.index("--out-pix-fmt") + 1]
        if engine.count("--rgb-out"):
            out_fmt = engine[engine.index("--rgb-out") + 1]
    raw_in = ["-f", "rawvideo", "-pix_fmt", out_fmt,
              "-s", params.resolution if resized else f"{source_info.width}x{source_info.height}"]
    if source_info.fps:
        raw_in += ["-r", fps_rational(source_info.fps)]
    enc_notes: List[str] = []
    tail = build_command(Path("pipe:0"), output, params, lut_path=None, ffmpeg_bin=ffmpeg_bin, source_info=source_info,
                         notes=enc_notes)
    i = tail.index("-i")
    if resized:                                   # the frames already have the size: no scaler on the encoder
        j = tail.index("-s", i + 2)
        del tail[j:j + 2]
    # input 0 = the engine's frames, input 1 = the source again for audio / subtitles / chapters / metadata (`?`: optional
    # streams; video is taken from the pipe only, so the source's picture is never decoded a second time)
    side = ["-i", str(source), "-map", "0:v:0", "-map", "1:a?", "-map", "1:s?", "-map_metadata", "1", "-map_chapters", "1"]
    encoder = tail[:i] + raw_in + tail[i:i + 2] + side + tail[i + 2:]
    # colour tags are decided by the LUT policy (ffmpeg.py:348-383), which build_command only applies with a lut_path:
    # take them from the full command
    full = build_command(source, output, params, lut_path=lut_path, ffmpeg_bin=ffmpeg_bin, source_info=source_info, notes=[])
    for flag in ("-color_primaries", "-color_trc", "-colorspace", "-color_range"):
        if flag in encoder:
            j = encoder.index(flag)
            del encoder[j:j + 2]
    for flag in ("-color_primaries", "-color_trc", "-colorspace", "-color_range"):
        if flag in full:
            encoder[-1:-1] = [flag, full[full.index(flag) + 1]]
    if chroma_loc is not None:
        encoder[-1:-1] = ["-chroma_sample_location", chroma_loc]
    return StageCommands(decoder, engine, encoder, notes)


def run_stage(cmds: StageCommands, out=sys.stdout) -> int:
    """Run decoder | engine | encoder.  The engine's report (its stderr, since its stdout carries frames) is relayed line by
    line to `out`, which is what `TaskRunner._run_stage` parses; returns 0 only if all three exit 0."""
    dec = subprocess.Popen(cmds.decoder, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    eng = subprocess.Popen(cmds.engine, stdin=dec.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    enc = subprocess.Popen(cmds.encoder, stdin=eng.stdout, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    dec.stdout.close()          # the readers own the pipe ends now: a writer gets SIGPIPE when its reader dies
    eng.stdout.close()
    procs = [dec, eng, enc]

    def stop(*_):
        for p in procs:
            if p.poll() is None:
                p.terminate()

    old = signal.signal(signal.SIGTERM, stop) if threading.current_thread() is threading.main_thread() else None
    try:
        for raw in eng.stderr:
            out.write(raw.decode("utf-8", "replace"))
            out.flush()
        codes = [p.wait() for p in procs]
    finally:
        if old is not None:
            signal.signal(signal.SIGTERM, old)
    for name, code in zip(("decoder", "engine", "encoder"), codes):
        if code:
            out.write(f"Error: {name} exited with {code}\n")
            out.flush()
            return code if code > 0 else 255
    return 0


def main(argv=None) -> int:
    import argparse
    import json
    ap = argparse.ArgumentParser(prog="lut_renderer_amd.pipe", description=__doc__.split("\n\n")[0])
    ap.add_argument("-i", "--input", required=True)
    ap.add_argument("-o", "--output", required=True)
    ap.add_argument("--cube", required=True)
    ap.add_argument("--params", default="{}", help="ProcessingParams as JSON (models.py:58-122 dict form)")
    ap.add_argument("--info", required=True, help="VideoInfo fields as JSON: width, height, pix_fmt, fps, colorspace, ...")
    ap.add_argument("--ffmpeg", default="ffmpeg")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--precision", default="strict", choices=["strict", "fast", "fma32"], help="engine setting, see lut_renderer_amd.cli")
    ap.add_argument("--chroma-loc", default=None, choices=["left", "center", "topleft"], help="engine setting, see lut_renderer_amd.cli")
    ap.add_argument("--engine-dither", default=None, choices=["blue_noise"], help="engine setting, see lut_renderer_amd.cli")
    ap.add_argument("--cube2", default=None, help="engine setting: a second LUT behind --cube in the same pass, see lut_renderer_amd.cli")
    ap.add_argument("--interp2", default=None, help="interpolation mode of --cube2, see lut_renderer_amd.cli")
    ap.add_argument("--alpha-mode", default="straight", choices=["straight", "premultiplied"], help="engine setting, see lut_renderer_amd.cli")
    ap.add_argument("--cdl", default=None, help="engine setting: an ASC CDL file (.cc / .ccc / .cdl) ahead of --cube, see lut_renderer_amd.cli")
    ap.add_argument("--cdl-id", default=None, help="the id of the ColorCorrection to take from --cdl")
    ap.add_argument("--cdl-sop", default=None, help="the CDL as nine literal values, see lut_renderer_amd.cli")
    ap.add_argument("--cdl-sat", default=None, type=float, help="the CDL's saturation as a literal value")
    ap.add_argument("--lut1d", default=None, help="engine setting: a 1D LUT file ahead of --cube, see lut_renderer_amd.cli")
    ap.add_argument("--interp1d", default=None, help="interpolation mode of --lut1d, see lut_renderer_amd.cli")
    ap.add_argument("--stages", default=None, help="engine setting: the operators as an ordered stack, see lut_renderer_amd.cli")
    ap.add_argument("--rgb-stages", default=None, help="engine setting: the ordered stack on an RGB source, see lut_renderer_amd.cli")
    ap.add_argument("--semi-stages", default=None,
                    help="engine setting: the ordered stack on semi-planar frames (nv12, p010le, ..), see lut_renderer_amd.cli")
    ap.add_argument("--rgb-out", default=None, help="engine setting: the RGB format --rgb-out-stages writes, see lut_renderer_amd.cli")
    ap.add_argument("--rgb-out-stages", default=None,
                    help="engine setting: the ordered stack from a YUV source into --rgb-out, see lut_renderer_amd.cli")
    mix = ap.add_mutually_exclusive_group()
    mix.add_argument("--strength", default=None, type=float, help="engine setting: LUT strength in [0, 1], see lut_renderer_amd.cli")
    mix.add_argument("--strength-keys", default=None, help="engine setting: LUT strength by key frames F:S,F:S,..., see lut_renderer_amd.cli")
    ap.add_argument("--matte", default=None, help="engine setting: a matte plane (raw gray frames), see lut_renderer_amd.cli")
    ap.add_argument("--matte-pix-fmt", default=None, help="pixel format of --matte, see lut_renderer_amd.cli")
    ap.add_argument("--matte-invert", action="store_true", help="invert --matte, see lut_renderer_amd.cli")
    ap.add_argument("--rgb-matrix", default=None, help="engine setting: the matrix of a 'matrix' stage as nine literal values, see lut_renderer_amd.cli")
    ap.add_argument("--rgb-matrix-offset", default=None, help="the offset of --rgb-matrix as three literal values")
    ap.add_argument("--rgb-matrix-file", default=None, help="the matrix of a 'matrix' stage from a .spimtx file, see lut_renderer_amd.cli")
    ap.add_argument("--gpu-resize", action="store_true", help="resize to the params' resolution in the engine (--out-size) instead of the encoder")
    a = ap.parse_args(argv)
    try:
        params = ProcessingParams.from_dict(json.loads(a.params))
        info = VideoInfo(**json.loads(a.info))
        if a.cdl is not None and (a.cdl_sop is not None or a.cdl_sat is not None):
            raise ValueError("--cdl names a file and --cdl-sop / --cdl-sat give literal values: use one or the other")
        cdl = Path(a.cdl) if a.cdl is not None else None
        if a.cdl_sop is not None or a.cdl_sat is not None:
            from .cdl import Cdl
            cdl = Cdl.from_sop_text(a.cdl_sop, a.cdl_sat)
        from .cli import rgb_matrix_from_args
        mtx = rgb_matrix_from_args(a)                           # (the checks; a file travels to the engine as its path)
        if a.rgb_matrix_file is not None:
            mtx = Path(a.rgb_matrix_file)
        cmds = engine_stage_commands(Path(a.input), Path(a.output), params, Path(a.cube), info, ffmpeg_bin=a.ffmpeg, device=a.device,
                                     precision=a.precision, chroma_loc=a.chroma_loc, gpu_resize=a.gpu_resize,
                                     engine_dither=a.engine_dither, cube2=None if a.cube2 is None else Path(a.cube2),
                                     interp2=a.interp2, alpha_mode=a.alpha_mode, cdl=cdl, cdl_id=a.cdl_id,
                                     lut1d=None if a.lut1d is None else Path(a.lut1d), interp1d=a.interp1d,
                                     stages=a.stages, strength=a.strength, strength_keys=a.strength_keys,
                                     matte=None if a.matte is None else Path(a.matte), matte_pix_fmt=a.matte_pix_fmt,
                                     matte_invert=a.matte_invert, rgb_matrix=mtx, rgb_stages=a.rgb_stages,
                                     rgb_out=a.rgb_out, rgb_out_stages=a.rgb_out_stages, semi_stages=a.semi_stages)
    except Exception as exc:
        print(f"Error: {exc}", flush=True)
        return 1
    return run_stage(cmds)


if __name__ == "__main__":
    sys.exit(main())
