"""The stage stack on semi-planar sides without a GPU: the one copy of the pass's refusals
(`formats.check_semi_stack_options`), every layer refusing the same rows before an engine is touched, the CLI flag and its round
trip through `engine_command`, and the shape of a plane of pairs."""
import threading
from pathlib import Path
from types import SimpleNamespace

import pytest

from lut_renderer_amd import _native, cube, frames, semiplanar
from lut_renderer_amd.cdl import Cdl
from lut_renderer_amd.engine import LutEngine, _fresh_planes
from lut_renderer_amd.formats import PixFmt, SemiFmt, check_semi_stack_options, parse_semi_fmt, yuv_side

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
TAIL = r"a stage stack on semi-planar frames \(semi_stages\)"
FULL = dict(stages="lut1d,cdl,lut3d,lut3d2", cdl=True)
PLANAR = ["yuv420p", "yuv422p", "yuv444p", "yuv420p10le", "yuv422p12le", "yuv444p16le", "yuv444p9le"]
#: what the pass refuses, by keyword of the check -> the words of the refusal
OPTIONS = [(dict(dither="error_diffusion"), rf"dither \('error_diffusion'\) is not supported with {TAIL}"),
           (dict(dither="blue_noise"), rf"dither \('blue_noise'\) is not supported with {TAIL}"),
           (dict(chroma_loc="left"), rf"sited chroma resampling \(chroma_loc\) is not supported with {TAIL}"),
           (dict(out_size=(8, 4)), rf"a resize \(out_size / resolution\) is not supported with {TAIL}"),
           (dict(out2_pix_fmt="yuv420p"), rf"the two-output pass \(out2_pix_fmt\) is not supported with {TAIL}"),
           (dict(alpha_mode="premultiplied"), rf"alpha_mode='premultiplied' is not supported with {TAIL}"),
           (dict(strength=0.5), rf"a LUT strength \(strength\) is not supported with {TAIL}"),
           (dict(matte=True), rf"a matte \(matte\) is not supported with {TAIL}")]
SIDES = [("yuva420p", "alpha .* semi-planar formats carry no alpha"), ("uyvy422", "a packed 4:2:2 side"), ("y210le", "a packed 4:2:2 side"),
         ("v210", "a v210 side"), ("rgb24", "an RGB side"), ("gbrp10le", "an RGB side"), ("gbrpf32le", "a float side"),
         ("nv24", "a semi-planar side is 4:2:0 or 4:2:2"), ("p410le", "a semi-planar side is 4:2:0 or 4:2:2"),
         ("p010be", "little-endian")]


# ------------------------------------------------------------------ what the check takes
@pytest.mark.parametrize("name", list(_native.SEMI_FORMATS))
def test_every_semi_planar_name_on_either_side(name):
    fmt = parse_semi_fmt(name)
    st, fin, fout = check_semi_stack_options(name, None, **FULL)
    assert isinstance(fin, SemiFmt) and fout == fin and [k for k, _ in st] == ["lut1d", "cdl", "lut3d", "lut3d2"]
    for other in PLANAR:
        _, fin, fout = check_semi_stack_options(name, other, **FULL)
        assert (fin.name, fout.name) == (name, other) and isinstance(fout, PixFmt) and fout.nplanes == 3
        _, fin, fout = check_semi_stack_options(other, name, **FULL)
        assert (fin.name, fout.name) == (other, name) and isinstance(fin, PixFmt) and fout == fmt
    for other in _native.SEMI_FORMATS:
        check_semi_stack_options(name, other, **FULL)
    assert (fmt.csx, fmt.csy) in ((1, 1), (1, 0))                   # 4:4:4 cannot be on a semi-planar side: no such name


def test_the_eight_layout_pairs_and_no_ninth():
    names = {(1, 1): ("nv12", "yuv420p"), (1, 0): ("nv16", "yuv422p"), (0, 0): (None, "yuv444p")}
    seen = set()
    for a, (sa, pa) in names.items():
        for b, (sb, pb) in names.items():
            for src, dst in ((sa, pb), (pa, sb), (sa, sb)):
                if src is not None and dst is not None:
                    _, fin, fout = check_semi_stack_options(src, dst, stages="lut3d")
                    seen.add((fin.csx, fin.csy, fout.csx, fout.csy))
    assert len(seen) == 8 and (0, 0, 0, 0) not in seen
    with pytest.raises(ValueError, match="both sides are planar: use apply_yuv_stack"):
        check_semi_stack_options("yuv444p", "yuv444p", stages="lut3d")


def test_what_else_the_check_takes():
    check_semi_stack_options("yuvj420p", "nv12", stages="lut3d")       # yuvj* is read as yuv*
    check_semi_stack_options("nv12", None, stages="lut3d,cdl,lut3d2", cdl=True, prelut=True)     # a prelut where lut3d is fed codes
    for variant in (None, "auto", "generic", "vec_global"):
        check_semi_stack_options("p010le", "yuv422p10le", **FULL, variant=variant)
    for precision in (None, "strict", "fast", "fma32"):                 # as the stack without a strength: the pass runs strict
        check_semi_stack_options("p010le", None, **FULL, precision=precision)


# ------------------------------------------------------------------ what it refuses
@pytest.mark.parametrize("kw,message", OPTIONS, ids=[next(iter(k)) + str(i) for i, (k, _) in enumerate(OPTIONS)])
def test_every_option_the_pass_does_not_take(kw, message):
    with pytest.raises(ValueError, match=message):
        check_semi_stack_options("p010le", "yuv422p10le", **FULL, **kw)


@pytest.mark.parametrize("name,message", SIDES)
def test_a_side_the_pass_does_not_take(name, message):
    with pytest.raises(ValueError, match=message):
        check_semi_stack_options("nv12", name, stages="lut3d")
    with pytest.raises(ValueError, match=message):
        check_semi_stack_options(name, "nv12", stages="lut3d")


def test_the_list_and_the_variants():
    names = dict(pix_fmt="p010le", out_pix_fmt="p010le")
    for kw, message in ((dict(stages="lut1d,matrix,lut3d", rgb_matrix=True), rf"stage 'matrix' is not supported with {TAIL}"),
                        (dict(stages="lut3d", rgb_matrix=True), rf"stage 'matrix' is not supported with {TAIL}"),
                        (dict(stages="matrix"), rf"stage 'matrix' is not supported with {TAIL}"),
                        (dict(stages=""), "the stage list is empty"), (dict(stages="lut3d,lut3d"), "listed twice"),
                        (dict(stages="lut3d", lut=False), "no 3D LUT is loaded"), (dict(stages="lut3d2", lut2=False), "no second LUT is loaded"),
                        (dict(stages="lut1d", lut1d=False), "no 1D LUT is loaded"), (dict(stages="cdl"), "no CDL is given"),
                        (dict(stages="lut3d", cdl=True), "a CDL is given and the stage list has no 'cdl' stage"),
                        (dict(stages="cdl,lut3d", cdl=True, prelut=True), "directly behind 'cdl'"),
                        (dict(stages="lut3d", variant="vec_lds"), rf"variant vec_lds is not supported with {TAIL}"),
                        (dict(stages="lut3d:prism", variant="vec_global"), "variant vec_global cannot take stage 'lut3d:prism'")):
        with pytest.raises(ValueError, match=message):
            check_semi_stack_options(**{**names, **kw})
    with pytest.raises(ValueError, match="variant vec_global cannot take an 8-bit source"):
        check_semi_stack_options("nv12", "p010le", stages="lut3d", variant="vec_global")
    with pytest.raises(ValueError, match="needs pix_fmt"):
        check_semi_stack_options(None, "nv12", stages="lut3d")


# ------------------------------------------------------------------ every layer refuses the same rows before an engine is touched
def _p010(w=16, h=8):
    import torch
    y = frames.natural_yuv(w, h, 10, 1, 1)
    return [torch.from_numpy(p.view("int16")) for p in semiplanar.to_semi(y, "p010le")]


ROWS = [(kw, m) for kw, m in OPTIONS if "matte" not in kw] + [
    (dict(out_pix_fmt="yuva420p10le"), "carry no alpha"), (dict(out_pix_fmt="uyvy422"), "a packed 4:2:2 side"),
    (dict(out_pix_fmt="v210"), "a v210 side"), (dict(out_pix_fmt="rgb48le"), "an RGB side"), (dict(out_pix_fmt="gbrpf32le"), "a float side"),
    (dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le"), "both sides are planar: use apply_yuv_stack"),
    (dict(stages="lut1d,matrix,lut3d"), "stage 'matrix' is not supported"), (dict(stages=""), "empty"), (dict(stages="cdl,cdl"), "twice"),
    (dict(stages="lut3d"), "no 'cdl' stage"), (dict(cdl=None), "no CDL is given")]


def test_the_engine_refuses_before_it_is_touched():
    src = _p010()
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False, _variant_name="auto")
    full = dict(pix_fmt="p010le", out_pix_fmt="yuv422p10le", stages="lut1d,cdl,lut3d,lut3d2", cdl=Cdl())
    for kw, message in ROWS + [(dict(matte=src[0]), r"a matte \(matte\)")]:
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_yuv_stack_semi(held, src, **{**full, **kw})
    for name, message in (("n", "no 3D LUT is loaded"), ("n2", "no second LUT is loaded"), ("n1d", "no 1D LUT is loaded")):
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_yuv_stack_semi(SimpleNamespace(**{**vars(held), name: 0}), src, **full)
    with pytest.raises(ValueError, match="variant vec_lds is not supported"):
        LutEngine.apply_yuv_stack_semi(SimpleNamespace(**{**vars(held), "_variant_name": "vec_lds"}), src, **full)
    with pytest.raises(TypeError, match="cdl must be a lut_renderer_amd.cdl.Cdl"):
        LutEngine.apply_yuv_stack_semi(held, src, **{**full, "cdl": "shot.cc"})
    with pytest.raises(TypeError, match="unexpected keyword argument 'interp'"):
        LutEngine.apply_yuv_stack_semi(held, src, **full, interp="trilinear")
    assert not hasattr(held, "_lib")                                  # nothing reached the library


def test_the_group_checks_the_same_things_first():
    from lut_renderer_amd.multigpu import LutEngineGroup
    e0 = SimpleNamespace(n=33, n2=9, _has_prelut=False, _variant_name="auto")
    g = SimpleNamespace(_lock=threading.RLock(), n1d=17, engines=[e0])
    full = dict(pix_fmt="p010le", out_pix_fmt="yuv422p10le", stages="lut1d,cdl,lut3d,lut3d2", cdl=Cdl())
    for kw, message in ROWS + [(dict(row0=0), "the group owns the row partition")]:
        with pytest.raises(ValueError, match=message):
            LutEngineGroup.apply_yuv_stack_semi(g, _p010(), **{**full, **kw})


def _lut(n=2):
    import numpy as np
    return cube.CubeLut(n, np.ones(3, np.float32), cube.identity_lattice(n).astype(np.float32))


def test_apply_lut_refuses_while_planning():
    from lut_renderer_amd.api import apply_lut
    src = _p010()
    eng = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False, _variant_name="auto")
    base = dict(cube=None, pix_fmt="p010le", out_pix_fmt="yuv422p10le", engine=eng, semi_stages="lut1d,lut3d")
    for kw, message in ((dict(zscale_dither="error_diffusion"), r"dither \('error_diffusion'\) is not supported with a stage stack on semi"),
                        (dict(engine_dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a stage stack on semi"),
                        (dict(resolution="8x4"), "resize .* is not supported with a stage stack on semi"),
                        (dict(second_pix_fmt="yuv420p"), "two-output pass .* is not supported with a stage stack on semi"),
                        (dict(strength=0.5), r"a LUT strength \(strength\) is not supported with a stage stack on semi"),
                        (dict(matte=src[0]), r"a matte \(matte\) is not supported with a stage stack on semi"),
                        (dict(out_pix_fmt="yuva420p10le"), "carry no alpha"),
                        (dict(pix_fmt="yuv420p10le"), "both sides are planar: use apply_yuv_stack"),
                        (dict(semi_stages="lut1d,matrix,lut3d"), "stage 'matrix' is not supported"),
                        (dict(stages="lut3d"), "semi_stages and stages / rgb_stages / rgb_out_stages are mutually exclusive"),
                        (dict(rgb_stages="lut3d"), "mutually exclusive"),
                        (dict(rgb_out="rgb48le", rgb_out_stages="lut3d"), "mutually exclusive"),
                        (dict(semi_stages="lut1d,lut3d,cdl"), "stage 'cdl' is listed and no CDL is given"),
                        (dict(cube2=_lut()), "cube2 is given and the stage list has no 'lut3d2' stage")):
        planes = frames.natural_yuv(16, 8, 10, 1, 1) if kw.get("pix_fmt") else src
        with pytest.raises(ValueError, match=message):
            apply_lut(planes, **{**base, **kw})
    assert not hasattr(eng, "_lock")                                  # the engine's lock was never taken


def test_the_host_pipeline_refuses_the_same_rows():
    from lut_renderer_amd.stream import HostPipeline
    eng = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False)
    full = dict(out_pix_fmt="yuv422p10le", semi_stages="lut1d,cdl,lut3d,lut3d2", cdl=Cdl())
    for kw, message in [(k, m) for k, m in ROWS if "stages" not in k and "pix_fmt" not in k or "out_pix_fmt" in k and "pix_fmt" not in k]:
        kw = dict(kw)
        extra = dict(second_pix_fmt=kw.pop("out2_pix_fmt")) if "out2_pix_fmt" in kw else {}
        with pytest.raises(ValueError, match=message):
            HostPipeline(eng, "p010le", 16, 8, **{**full, **kw, **extra})
    for kw, message in ((dict(semi_stages="lut1d,matrix,lut3d"), "stage 'matrix' is not supported"),
                        (dict(stages="lut3d"), "mutually exclusive"), (dict(rgb_stages="lut3d"), "mutually exclusive"),
                        (dict(rgb_out="rgb48le"), "with semi_stages the output is out_pix_fmt"),
                        (dict(strength_keys="0:1"), r"strength_keys\) is not supported with a stage stack on semi"),
                        (dict(chain=True), "chain / lut1d are not set with semi_stages")):
        with pytest.raises(ValueError, match=message):
            HostPipeline(eng, "p010le", 16, 8, **{**full, **kw})
    with pytest.raises(ValueError, match="mutually exclusive"):
        HostPipeline(eng, "yuv420p10le", 16, 8, rgb_out="rgb48le", rgb_out_stages="lut3d", semi_stages="lut3d")
    with pytest.raises(ValueError, match="both sides are planar"):
        HostPipeline(eng, "yuv420p10le", 16, 8, out_pix_fmt="yuv422p10le", semi_stages="lut3d")


# ------------------------------------------------------------------ the CLI flag and the argv builder
def _args(*extra, pix_fmt="p010le", out="yuv422p10le"):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt, "--out-pix-fmt", out, *extra])


def test_cli_flag(cube_dir):
    from lut_renderer_amd.cli import plan_from_args
    a, b, t = str(cube_dir / "log709_33.cube"), str(cube_dir / "random_9.cube"), str(GOLDEN / "lut1d" / "curve17.cube")
    assert _args("--cube", a).semi_stages is None
    _, kw, w, h = plan_from_args(_args("--cube", a, "--cube2", b, "--lut1d", t, "--cdl-sat", "0.5", "--interp", "trilinear", "--interp2", "nearest",
                                       "--semi-stages", "lut1d,cdl,lut3d,lut3d2"))
    assert (w, h) == (16, 8) and (kw["pix_fmt"], kw["out_pix_fmt"]) == ("p010le", "yuv422p10le")
    assert kw["semi_stages"] == (("lut1d", None), ("cdl", None), ("lut3d", "trilinear"), ("lut3d2", "nearest")) and kw["cdl"] == Cdl(saturation=0.5)
    assert not {"interp", "dither", "alpha_mode", "stages"} & set(kw)
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--semi-stages", "lut3d", pix_fmt="yuv444p10le", out="p010le"))
    assert kw["semi_stages"] == (("lut3d", "tetrahedral"),) and kw["out_pix_fmt"] == "p010le"
    full = ("--cube", a, "--lut1d", t, "--semi-stages", "lut1d,lut3d")
    for extra, message in ((("--zscale-dither", "error_diffusion"), r"dither \('error_diffusion'\) is not supported with a stage stack on semi"),
                           (("--engine-dither", "blue_noise"), r"dither \('blue_noise'\) is not supported with a stage stack on semi"),
                           (("--out-size", "8x4"), "resize .* is not supported with a stage stack on semi"),
                           (("--chroma-loc", "left"), "chroma_loc.* is not supported with a stage stack on semi"),
                           (("--strength", "0.5"), r"a LUT strength \(strength\) is not supported with a stage stack on semi"),
                           (("--matte", "m.gray"), r"a matte \(matte\) is not supported with a stage stack on semi"),
                           (("--alpha-mode", "premultiplied"), "alpha_mode='premultiplied' is not supported with a stage stack on semi"),
                           (("--second-output", "c.yuv", "--second-pix-fmt", "yuv420p"), "two-output pass .* not supported with a stage stack on semi"),
                           (("--stages", "lut1d,lut3d"), "mutually exclusive"), (("--rgb-stages", "lut1d,lut3d"), "mutually exclusive"),
                           (("--rgb-out", "rgb48le", "--rgb-out-stages", "lut3d"), "mutually exclusive"),
                           (("--rgb-out", "rgb48le"), "with --semi-stages the output is --out-pix-fmt"),
                           (("--cdl-sat", "0.5"), "--cdl-sat is given and --semi-stages has no 'cdl' stage")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args(*full, *extra))
    with pytest.raises(ValueError, match="both sides are planar: use apply_yuv_stack"):
        plan_from_args(_args(*full, pix_fmt="yuv420p10le"))
    with pytest.raises(ValueError, match="stage 'matrix' is not supported"):
        plan_from_args(_args("--cube", a, "--rgb-matrix", "1 0 0 0 1 0 0 0 1", "--semi-stages", "matrix,lut3d"))


def test_engine_command_round_trips_the_flag(cube_dir):
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    from lut_renderer_amd.pipe import engine_stage_commands
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="p010le", color_range="tv", colorspace="bt709", fps=25.0)
    params = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")
    a, b, t = cube_dir / "log709_33.cube", cube_dir / "random_9.cube", GOLDEN / "lut1d" / "curve17.cube"
    io = (Path("-"), Path("-"), params, a, info)
    plain = engine_command(*io)
    assert "--semi-stages" not in plain and engine_command(*io, semi_stages=None) == plain       # byte for byte what it was
    assert engine_command(*io, semi_stages="lut3d") == plain + ["--semi-stages", "lut3d:tetrahedral"]
    grade = Cdl(slope=(1.1, 1.0, 0.9), saturation=0.6)
    cmd = engine_command(*io, cube2=b, interp2="nearest", cdl=grade, lut1d=t, interp1d="cubic", semi_stages=["lut1d", "cdl", "lut3d", "lut3d2"])
    assert cmd == plain + ["--cube2", str(b), "--interp2", "nearest", "--cdl-sop", grade.sop_text(), "--cdl-sat", repr(0.6), "--lut1d", str(t),
                           "--interp1d", "cubic", "--semi-stages", "lut1d,cdl,lut3d:tetrahedral,lut3d2:nearest"]
    args = build_parser().parse_args(cmd[3:])
    _, kw, _, _ = plan_from_args(args)
    assert kw["semi_stages"] == (("lut1d", None), ("cdl", None), ("lut3d", "tetrahedral"), ("lut3d2", "nearest")) and kw["cdl"] == grade
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("p010le", "yuv422p10le")
    cmds = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, lut1d=t, semi_stages="lut3d:trilinear,lut1d")
    assert cmds.engine[cmds.engine.index("--semi-stages") + 1] == "lut3d:trilinear,lut1d"
    same = dict(params.to_dict(), pix_fmt="p010le")                   # (the plain call keeps the source's subsampling)
    assert "--semi-stages" not in engine_stage_commands(Path("in.mov"), Path("out.mov"), ProcessingParams.from_dict(same), a, info).engine
    for kw, message in ((dict(semi_stages="lut1d"), "the LUT is given and the stage list has no 'lut3d' stage"),
                        (dict(semi_stages="lut3d", stages="lut3d"), "mutually exclusive"),
                        (dict(semi_stages="lut3d", rgb_stages="lut3d"), "mutually exclusive"),
                        (dict(semi_stages="lut3d", engine_dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a stage stack on semi"),
                        (dict(semi_stages="lut3d", chroma_loc="left"), "chroma_loc.* is not supported with a stage stack on semi"),
                        (dict(semi_stages="lut3d", strength=0.5), r"strength\) is not supported with a stage stack on semi"),
                        (dict(semi_stages="matrix,lut3d"), "stage 'matrix' is not supported")):
        with pytest.raises(ValueError, match=message):
            engine_command(*io, **kw)
    planar = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    with pytest.raises(ValueError, match="both sides are planar: use apply_yuv_stack"):
        engine_command(Path("-"), Path("-"), params, a, planar, semi_stages="lut3d")


# ------------------------------------------------------------------ a plane of pairs
@pytest.mark.parametrize("w,h", [(16, 8), (17, 8), (16, 9), (17, 9), (1, 1)])
def test_the_shape_of_a_fresh_destination(w, h):
    import torch
    like = torch.zeros((3, h, w), dtype=torch.int16)
    for name, rows in (("p010le", (h + 1) // 2), ("nv16", h)):
        fmt = yuv_side(name)
        y, pairs = _fresh_planes(fmt, w, h, like, "cpu")
        assert tuple(y.shape) == (3, h, w) and tuple(pairs.shape) == (3, rows, 2 * ((w + 1) // 2)), (name, w, h)
        assert y.dtype == pairs.dtype == (torch.int16 if fmt.depth > 8 else torch.uint8)
        # the span the C layer gives the plane: 2 * ceil(w / 2) samples a row, whole pairs even at an odd width
        assert pairs.shape[-1] % 2 == 0 and pairs.shape[-1] >= w
