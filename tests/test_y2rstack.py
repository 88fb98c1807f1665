"""The stage stack from YUV sources into RGB frames without a GPU: the twin's `[lut3d]` anchor against the
YUV -> RGB twin, its list walk against the pinned one of the RGB stack, the one copy of the refusals through every layer, the old
names still refusing in today's words, and the argv."""
import threading
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from lut_renderer_amd import cube, frames
from lut_renderer_amd.cdl import Cdl, read_cdl
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.formats import check_rgb_stack_options, check_yuv2rgb_options, check_yuv2rgb_stack_options
from lut_renderer_amd.rgbmatrix import RgbMatrix, read_rgb_matrix
from oracle.lut3d_numpy import yuv_to_rgb_codes
from tests import _lut1d_twin as l1t
from tests import _rgbstack_twin as rsk
from tests import _y2rstack_twin as twin
from tests import _yuv2rgb_twin as y2r

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
F = np.float32
I3 = RgbMatrix()
GAMUT = read_rgb_matrix(GOLDEN / "matrix" / "bt2020_to_709.spimtx")
NAMES = dict(pix_fmt="yuv420p10le", out_pix_fmt="rgb48le")


def _eq(got, want):
    if isinstance(want, np.ndarray):
        return isinstance(got, np.ndarray) and got.shape == want.shape and np.array_equal(got, want)
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _yuv(depth, lay):
    return f"yuv{lay}p" + ("" if depth == 8 else f"{depth}le")


def _luts():
    rng = np.random.default_rng(11)
    a = cube.CubeLut(9, np.ones(3, F), rng.uniform(-0.2, 1.2, (9, 9, 9, 3)).astype(F))
    b = cube.CubeLut(5, np.array([1.0, 0.5, 1.0], F), rng.uniform(0.0, 1.0, (5, 5, 5, 3)).astype(F))
    return a, b


# ------------------------------------------------------------------ the twin
@pytest.mark.parametrize("din,dl", [(8, 8), (10, 10), (10, 8), (8, 10)], ids=lambda v: str(v))
def test_lut3d_alone_is_the_yuv_to_rgb_twin(orc, din, dl):
    lut, _ = _luts()
    for lay, (icsx, icsy) in twin.LAYOUTS.items():
        src = frames.make_yuv("natural", 38, 14, din, icsx, icsy, k=din + dl)
        for out_fmt in {8: ("gbrp", "bgr24", "argb"), 10: ("gbrp10le",)}[dl]:
            for mode in ("tetrahedral", "prism"):
                want = y2r.apply(lut.table, lut.scale, mode, out_fmt, din, icsx, icsy, src)
                assert _eq(twin.apply([("lut3d", mode)], out_fmt, din, icsx, icsy, src, lut=lut), want), (lay, out_fmt, mode)


ORDERS = ("lut1d,matrix,lut3d", "lut3d,cdl,lut3d2", "cdl,lut3d", "matrix,cdl,lut1d", "lut1d,cdl,lut3d,lut3d2", "lut3d,matrix")


@pytest.mark.parametrize("stages", ORDERS)
def test_on_444_frames_the_walk_is_the_pinned_walk_of_the_rgb_stack(orc, stages):
    """For a yuv444p10le frame the twin's codes are the RGB stack's walk on the codes stage 1 produces."""
    a, b = _luts()
    grade = read_cdl(GOLDEN / "cdl" / "shot.cc")
    l1 = cube.read_lut1d(GOLDEN / "lut1d" / "curve17.cube")
    tab = l1t.table(l1.table, l1.scale, "linear", 10)
    planes = frames.natural_yuv(37, 13, 10, 0, 0, k=2)
    st = stages.split(",")
    res = dict(lut=a, lut2=b, l1d_tab=tab, cdl=grade if "cdl" in st else None, mtx=GAMUT if "matrix" in st else None)
    codes = yuv_to_rgb_codes(twin.consts("bt709", "tv", "tv", 10, 10), 0, 0, planes)
    assert _eq(twin.rgb_codes(st, "gbrp10le", 10, 0, 0, planes, **res), rsk.walk(st, 10, codes, **res))
    r, g, b_ = rsk.walk(st, 10, codes, **res)
    assert _eq(twin.apply(st, "gbrp10le", 10, 0, 0, planes, **res), [g.astype(np.uint16), b_.astype(np.uint16), r.astype(np.uint16)])


# ------------------------------------------------------------------ the one copy of the refusals
REFUSALS = (
    (dict(stages=""), "the stage list is empty"),
    (dict(stages="lut3d,lut3d"), "twice"),
    (dict(stages="lut3d", lut=False), "no 3D LUT is loaded"),
    (dict(stages="lut3d2", lut2=False), "no second LUT is loaded"),
    (dict(stages="lut1d", lut1d=False), "no 1D LUT is loaded"),
    (dict(stages="cdl,lut3d"), "no CDL is given"),
    (dict(stages="lut3d", cdl=True), "has no 'cdl' stage"),
    (dict(stages="matrix,lut3d"), "no RGB matrix is given"),
    (dict(stages="lut3d", rgb_matrix=True), "has no 'matrix' stage"),
    (dict(stages="cdl,lut3d", cdl=True, prelut=True), "directly behind 'cdl'"),
    (dict(stages="matrix,lut3d", rgb_matrix=True, prelut=True), "directly behind 'matrix'"),
    (dict(stages="lut3d", pix_fmt="gbrp10le"), "is an RGB format"),
    (dict(stages="lut3d", pix_fmt="nv12"), "is a semi-planar container"),
    (dict(stages="lut3d", pix_fmt="uyvy422"), "is a packed 4:2:2 container"),
    (dict(stages="lut3d", pix_fmt="v210"), "is a v210 container"),
    (dict(stages="lut3d", out_pix_fmt="yuv420p10le"), "is not an RGB output format"),
    (dict(stages="lut3d", out_pix_fmt="gbrpf32le"), "a float output"),
    (dict(stages="lut3d", pix_fmt="yuva420p10le", out_pix_fmt="rgba64le"), "a follow-up"),
    (dict(stages="lut3d", dither="error_diffusion"), r"dither \('error_diffusion'\) is not supported"),
    (dict(stages="lut3d", engine_dither="blue_noise"), r"dither \(engine_dither='blue_noise'\) is not supported"),
    (dict(stages="lut3d", out_size=(8, 8)), "a resize"),
    (dict(stages="lut3d", chroma_loc="left"), "chroma_loc"),
    (dict(stages="lut3d", strength=0.5), "strength"),
    (dict(stages="lut3d", matte=True), "a matte"),
    (dict(stages="lut3d", alpha_mode="premultiplied"), "alpha_mode='premultiplied'"),
    (dict(stages="lut3d", out2_pix_fmt="yuv420p"), "two-output"),
    (dict(stages="lut3d", variant="vec_lds"), "vec_lds"),
    (dict(stages="lut3d:prism", variant="vec_global"), "vec_global cannot take stage 'lut3d:prism'"),
    (dict(stages="lut3d", pix_fmt="yuv420p", variant="vec_global"), "vec_global cannot take an 8-bit source"),
)
IDS = [m for _, m in REFUSALS]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=IDS)
def test_check_yuv2rgb_stack_options_refuses(kw, message):
    with pytest.raises(ValueError, match=message):
        check_yuv2rgb_stack_options(**{**NAMES, **kw})


def test_what_check_yuv2rgb_stack_options_takes():
    st, fin, fout = check_yuv2rgb_stack_options("yuv422p10le", "gbrp10le", stages="lut1d,cdl,lut3d:trilinear", cdl=True)
    assert st == (("lut1d", None), ("cdl", None), ("lut3d", "trilinear")) and (fin.depth, fin.csx, fin.csy) == (10, 1, 0)
    assert (fout.name, fout.family, fout.depth, fout.alpha) == ("gbrp10le", "gbr", 10, False)
    for src, out in (("yuv420p", "rgba"), ("yuv444p12le", "gbrp12le"), ("yuva420p10le", "gbrap10le"), ("yuva420p10le", "gbrp10le"),
                     ("yuva444p", "bgr24"), ("yuvj420p", "rgb24"), ("yuv420p", "gbrp10le"), ("yuv420p10le", "rgba64le")):
        _, fin, fout = check_yuv2rgb_stack_options(src, out, stages="matrix", rgb_matrix=True)
        assert fin.name == src.replace("yuvj", "yuv") and fout.name == out


def _planes(pix_fmt="yuv420p10le"):
    import torch
    from lut_renderer_amd.formats import parse_pix_fmt
    f = parse_pix_fmt(pix_fmt)
    src = [torch.from_numpy(p.view(np.int16) if f.depth > 8 else p) for p in frames.natural_yuv(16, 8, f.depth, f.csx, f.csy)]
    return src + [torch.zeros_like(src[0])] if f.alpha else src


def _call_of(kw):
    """A row of REFUSALS as (what the engine holds, the keyword arguments of an `apply_yuv_stack_to_rgb` call)."""
    import torch
    kw = dict(kw)
    held = dict(n=33 if kw.pop("lut", True) else 0, n2=9 if kw.pop("lut2", True) else 0, n1d=17 if kw.pop("lut1d", True) else 0,
                _has_prelut=kw.pop("prelut", False), _variant_name=kw.pop("variant", None))
    call = {**NAMES, **kw}
    call["cdl"] = Cdl() if call.get("cdl") else None
    call["rgb_matrix"] = I3 if call.get("rgb_matrix") else None
    if call.get("matte"):
        call["matte"] = torch.zeros((8, 16), dtype=torch.uint8)
    return held, call


@pytest.mark.parametrize("kw,message", REFUSALS, ids=IDS)
def test_every_refusal_through_the_engine_and_the_group(kw, message):
    from lut_renderer_amd.multigpu import LutEngineGroup
    held, call = _call_of(kw)
    with pytest.raises(ValueError, match=message):
        LutEngine.apply_yuv_stack_to_rgb(SimpleNamespace(**held), _planes(), **call)
    g = SimpleNamespace(_lock=threading.RLock(), n1d=held.pop("n1d"), engines=[SimpleNamespace(**held)])
    with pytest.raises(ValueError, match=message):
        LutEngineGroup.apply_yuv_stack_to_rgb(g, _planes(), **call)


def test_the_engine_and_the_group_refuse_what_is_theirs():
    from lut_renderer_amd.multigpu import LutEngineGroup
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False)
    with pytest.raises(TypeError, match="unexpected keyword argument 'interp'"):
        LutEngine.apply_yuv_stack_to_rgb(held, _planes(), **NAMES, stages="lut3d", interp="nearest")
    with pytest.raises(TypeError, match="rgb_matrix must be a lut_renderer_amd.rgbmatrix.RgbMatrix"):
        LutEngine.apply_yuv_stack_to_rgb(held, _planes(), **NAMES, stages="matrix", rgb_matrix="a.spimtx")
    with pytest.raises(TypeError, match="cdl must be a lut_renderer_amd.cdl.Cdl"):
        LutEngine.apply_yuv_stack_to_rgb(held, _planes(), **NAMES, stages="cdl", cdl="shot.cc")
    g = SimpleNamespace(_lock=threading.RLock(), n1d=17, engines=[held])
    with pytest.raises(ValueError, match="the group owns the row partition"):
        LutEngineGroup.apply_yuv_stack_to_rgb(g, _planes(), **NAMES, stages="lut3d", row0=0)


def _lut(n=2):
    return cube.CubeLut(n, np.ones(3, F), cube.identity_lattice(n).astype(F))


#: the rows of REFUSALS a layer above the engine cannot be asked: it has no variant argument ...
_NO_VARIANT = ("vec_lds", "vec_global")
#: ... and, where the layer loads the LUT from the call, no way to have a listed lut3d without one or a prelut it cannot see
_NO_HELD = ("no 3D LUT is loaded", "directly behind 'cdl'", "directly behind 'matrix'")


def _rows(skip):
    rows = [r for r in REFUSALS if not r[1].startswith(skip)]
    return dict(argvalues=rows, ids=[m for _, m in rows])


@pytest.mark.parametrize("kw,message", **_rows(_NO_VARIANT))
def test_every_refusal_through_apply_lut(kw, message):
    from lut_renderer_amd.api import apply_lut
    held, call = _call_of(kw)
    kinds = [s.partition(":")[0] for s in call["stages"].split(",")]
    eng = SimpleNamespace(**{k: v for k, v in held.items() if k != "_variant_name"})
    with pytest.raises(ValueError, match=message):
        apply_lut(_planes(call["pix_fmt"]) if not call["pix_fmt"].startswith(("gbr", "nv", "uyvy", "v210")) else _planes(),
                  cube=_lut() if "lut3d" in kinds and held["n"] and not held["_has_prelut"] else None, pix_fmt=call["pix_fmt"],
                  rgb_out=call["out_pix_fmt"], rgb_out_stages=call["stages"], cdl=call["cdl"], rgb_matrix=call["rgb_matrix"],
                  engine=eng, width=8 if call["pix_fmt"] in ("uyvy422", "v210") else None,   # (the planes stand in for a packed row of 8 pixels)
                  zscale_dither=call.get("dither", "none"), engine_dither=call.get("engine_dither"),
                  resolution="8x8" if call.get("out_size") else None, chroma_loc=call.get("chroma_loc"),
                  strength=call.get("strength"), matte=call.get("matte"), alpha_mode=call.get("alpha_mode", "straight"),
                  second_pix_fmt=call.get("out2_pix_fmt"))


@pytest.mark.parametrize("kw,message", **_rows(_NO_VARIANT))
def test_every_refusal_through_host_pipeline(kw, message):
    from lut_renderer_amd.stream import HostPipeline
    held, call = _call_of(kw)
    extra = {k: call[k] for k in ("dither", "engine_dither", "chroma_loc", "strength", "matte", "alpha_mode") if k in call}
    with pytest.raises(ValueError, match=message):
        HostPipeline(SimpleNamespace(**held), call["pix_fmt"], 16, 8, rgb_out=call["out_pix_fmt"], rgb_out_stages=call["stages"],
                     cdl=call["cdl"], rgb_matrix=call["rgb_matrix"], out_size="8x8" if call.get("out_size") else None,
                     second_pix_fmt=call.get("out2_pix_fmt"), **extra)


def _args(*extra, pix_fmt="yuv420p10le", rgb_out="rgb48le"):
    from lut_renderer_amd.cli import build_parser
    head = ["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt]
    return build_parser().parse_args(head + ([] if rgb_out is None else ["--rgb-out", rgb_out]) + list(extra))


def _flags_of(kw, cube_path):
    """A row of REFUSALS as the options of the CLI."""
    kinds = [s.partition(":")[0] for s in kw["stages"].split(",")] if kw["stages"] else []
    extra = ["--rgb-out-stages", kw["stages"]]
    if kw.get("lut", True) and ("lut3d" in kinds or not kinds):
        extra += ["--cube", str(cube_path)]
    if kw.get("lut2", True) and "lut3d2" in kinds:
        extra += ["--cube2", str(cube_path)]
    if kw.get("lut1d", True) and "lut1d" in kinds:
        extra += ["--lut1d", str(GOLDEN / "lut1d" / "curve17.cube")]
    if kw.get("cdl"):
        extra += ["--cdl-sat", "0.5"]
    if kw.get("rgb_matrix"):
        extra += ["--rgb-matrix", I3.m_text()]
    if kw.get("dither") == "error_diffusion":
        extra += ["--zscale-dither", "error_diffusion"]
    if kw.get("engine_dither"):
        extra += ["--engine-dither", kw["engine_dither"]]
    if kw.get("out_size"):
        extra += ["--out-size", "8x8"]
    if kw.get("chroma_loc"):
        extra += ["--chroma-loc", kw["chroma_loc"]]
    if kw.get("strength") is not None:
        extra += ["--strength", str(kw["strength"])]
    if kw.get("matte"):
        extra += ["--matte", "m.gray"]
    if kw.get("alpha_mode"):
        extra += ["--alpha-mode", kw["alpha_mode"]]
    if kw.get("out2_pix_fmt"):
        extra += ["--second-output", "c", "--second-pix-fmt", kw["out2_pix_fmt"]]
    return extra


@pytest.mark.parametrize("kw,message", **_rows(_NO_VARIANT + _NO_HELD[1:]))
def test_every_refusal_through_the_cli(cube_dir, kw, message):
    from lut_renderer_amd.cli import plan_from_args
    kw = {**NAMES, **kw}
    with pytest.raises(ValueError, match=message):
        plan_from_args(_args(*_flags_of(kw, cube_dir / "log709_33.cube"), pix_fmt=kw["pix_fmt"], rgb_out=kw["out_pix_fmt"]))


def test_the_cli_sees_a_prelut_in_the_lut_file(tmp_path):
    from lut_renderer_amd.cli import plan_from_args
    from tests._csp_files import write_csp_with_prelut
    shapers = [(np.array([0.0, 0.5, 1.0]), np.array([0.0, 0.7, 1.0]))] * 3
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 5, cube.log709_lattice(5), shapers)
    for flags, message in ((("--rgb-out-stages", "cdl,lut3d", "--cdl-sat", "0.5"), "directly behind 'cdl'"),
                           (("--rgb-out-stages", "matrix,lut3d", "--rgb-matrix", I3.m_text()), "directly behind 'matrix'")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args("--cube", str(p), *flags))


@pytest.mark.parametrize("kw,message", **_rows(_NO_VARIANT + _NO_HELD))
def test_every_refusal_through_engine_command(kw, message):
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    kw = {**NAMES, **kw}
    stages = kw["stages"]
    if stages and "lut3d" not in [s.partition(":")[0] for s in stages.split(",")]:
        stages += ",lut3d"                                   # (the builder's LUT needs its stage: that refusal comes first)
    info = VideoInfo(width=64, height=8, pix_fmt=kw["pix_fmt"], fps=25.0)
    params = ProcessingParams(video_codec="", zscale_dither="error_diffusion" if kw.get("dither") == "error_diffusion" else "none",
                              resolution="8x8" if kw.get("out_size") else None)
    extra = dict(rgb_out=kw["out_pix_fmt"], rgb_out_stages=stages, cdl=Cdl() if kw.get("cdl") else None,
                 rgb_matrix=I3 if kw.get("rgb_matrix") else None, engine_dither=kw.get("engine_dither"),
                 gpu_resize=bool(kw.get("out_size")), chroma_loc=kw.get("chroma_loc"), strength=kw.get("strength"),
                 alpha_mode=kw.get("alpha_mode", "straight"), matte=Path("m.gray") if kw.get("matte") else None,
                 lut1d=GOLDEN / "lut1d" / "curve17.cube" if "lut1d" in stages and kw.get("lut1d", True) else None,
                 cube2=Path("y.cube") if "lut3d2" in stages and kw.get("lut2", True) else None)
    if kw.get("out2_pix_fmt"):
        extra.update(second_output=Path("b.yuv"), second_pix_fmt=kw["out2_pix_fmt"])
    with pytest.raises(ValueError, match=_BUILDER_WORDS.get(message, message)):
        engine_command(Path("-"), Path("-"), params, Path("x.cube"), info, **extra)


#: the rows an older check of `engine_command`'s own answers first, in that check's words
_BUILDER_WORDS = {
    "alpha_mode='premultiplied'": "alpha_mode='premultiplied' needs a source that carries alpha",
    "is an RGB format": "an RGB source .* needs a resolved output pixel format",
}


# ------------------------------------------------------------------ the rules of the new name itself
def test_rgb_out_stages_needs_rgb_out_and_excludes_the_other_lists(cube_dir):
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.cli import plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    from lut_renderer_amd.stream import HostPipeline
    a = str(cube_dir / "log709_33.cube")
    eng = SimpleNamespace(n=33, n2=0, n1d=0, _has_prelut=False)
    info = VideoInfo(width=64, height=8, pix_fmt="yuv420p10le", fps=25.0)
    io = (Path("-"), Path("-"), ProcessingParams(video_codec=""), Path(a), info)
    # without rgb_out
    with pytest.raises(ValueError, match="it needs rgb_out"):
        apply_lut(_planes(), cube=_lut(), pix_fmt="yuv420p10le", rgb_out_stages="lut3d", engine=eng)
    with pytest.raises(ValueError, match="it needs rgb_out"):
        HostPipeline(eng, "yuv420p10le", 16, 8, rgb_out_stages="lut3d")
    with pytest.raises(ValueError, match="it needs --rgb-out"):
        plan_from_args(_args("--cube", a, "--rgb-out-stages", "lut3d", rgb_out=None))
    with pytest.raises(ValueError, match="it needs rgb_out"):
        engine_command(*io, rgb_out_stages="lut3d")
    # together with stages / rgb_stages
    for other in ("stages", "rgb_stages"):
        with pytest.raises(ValueError, match="mutually exclusive"):
            apply_lut(_planes(), cube=_lut(), pix_fmt="yuv420p10le", rgb_out="rgb48le", rgb_out_stages="lut3d", engine=eng,
                      **{other: "lut3d"})
        with pytest.raises(ValueError, match="mutually exclusive"):
            HostPipeline(eng, "yuv420p10le", 16, 8, rgb_out="rgb48le", rgb_out_stages="lut3d", **{other: "lut3d"})
        with pytest.raises(ValueError, match="mutually exclusive"):
            plan_from_args(_args("--cube", a, "--rgb-out-stages", "lut3d", "--" + other.replace("_", "-"), "lut3d"))
        with pytest.raises(ValueError, match="mutually exclusive"):
            engine_command(*io, rgb_out="rgb48le", rgb_out_stages="lut3d", **{other: "lut3d"})
    # together with out_pix_fmt
    with pytest.raises(ValueError, match="mutually exclusive"):
        apply_lut(_planes(), cube=_lut(), pix_fmt="yuv420p10le", out_pix_fmt="yuv420p", rgb_out="rgb48le", rgb_out_stages="lut3d",
                  engine=eng)
    with pytest.raises(ValueError, match="mutually exclusive"):
        HostPipeline(eng, "yuv420p10le", 16, 8, out_pix_fmt="yuv420p", rgb_out="rgb48le", rgb_out_stages="lut3d")
    with pytest.raises(ValueError, match="mutually exclusive"):
        plan_from_args(_args("--cube", a, "--rgb-out-stages", "lut3d", "--out-pix-fmt", "yuv420p"))
    with pytest.raises(ValueError, match="mutually exclusive"):
        engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx264", pix_fmt="yuv420p"), Path(a), info,
                       rgb_out="rgb48le", rgb_out_stages="lut3d")
    # a file without its stage, a source flagged full range into more than 8 bit
    with pytest.raises(ValueError, match="cube is given and the stage list has no 'lut3d' stage"):
        apply_lut(_planes(), cube=_lut(), pix_fmt="yuv420p10le", rgb_out="rgb48le", rgb_out_stages="cdl", cdl=Cdl(), engine=eng)
    with pytest.raises(ValueError, match="--lut1d is given and --rgb-out-stages has no 'lut1d' stage"):
        plan_from_args(_args("--cube", a, "--rgb-out-stages", "lut3d", "--lut1d", str(GOLDEN / "lut1d" / "curve17.cube")))
    with pytest.raises(ValueError, match="--rgb-out-stages has no 'lut3d2' stage"):
        plan_from_args(_args("--cube", a, "--rgb-out-stages", "lut3d", "--interp2", "nearest"))
    with pytest.raises(ValueError, match="takes an 8-bit rgb_out"):
        plan_from_args(_args("--cube", a, "--rgb-out-stages", "lut3d", "--color-range", "pc"))
    with pytest.raises(ValueError, match="takes an 8-bit rgb_out"):
        apply_lut(_planes(), cube=_lut(), pix_fmt="yuv420p10le", color_range="pc", rgb_out="rgb48le", rgb_out_stages="lut3d", engine=eng)


# ------------------------------------------------------------------ the old names still refuse, in today's words
def test_no_existing_refusal_is_lifted(cube_dir):
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.cli import plan_from_args
    a = str(cube_dir / "log709_33.cube")
    with pytest.raises(ValueError, match=r"a stage stack \(stages\) is not supported with YUV in with RGB out \(apply_yuv_to_rgb\)"):
        check_yuv2rgb_options("yuv420p10le", "rgb48le", stages="lut3d")
    for name, value, what in (("cdl", Cdl(), "an ASC CDL"), ("lut1d", "a.cube", "a 1D LUT"), ("strength", 0.5, "a LUT strength"),
                              ("matte", True, "a matte"), ("cube2", "b.cube", "a second LUT")):
        with pytest.raises(ValueError, match=what):
            check_yuv2rgb_options("yuv420p10le", "rgb48le", **{name: value})
    for flags, what in ((("--stages", "lut3d"), "a stage stack"), (("--lut1d", a), "a 1D LUT"), (("--cdl-sat", "0.5"), "an ASC CDL"),
                        (("--cube2", a), "a second LUT"), (("--strength", "0.5"), "a LUT strength"), (("--matte", "m.gray"), "a matte")):
        with pytest.raises(ValueError, match=what + r".* is not supported with YUV in with RGB out \(apply_yuv_to_rgb\)"):
            plan_from_args(_args("--cube", a, *flags))
    with pytest.raises(ValueError, match="--rgb-out names the RGB output of a YUV source"):
        plan_from_args(_args("--cube", a, "--rgb-stages", "lut3d", pix_fmt="gbrp10le", rgb_out="gbrp10le"))
    with pytest.raises(ValueError, match="a packed RGB destination"):
        check_rgb_stack_options("gbrp10le", "rgb48le", stages="lut3d")
    eng = SimpleNamespace(n=33, n2=0, n1d=0, _has_prelut=False)
    with pytest.raises(ValueError, match="a stage stack"):
        apply_lut(_planes(), cube=_lut(), pix_fmt="yuv420p10le", rgb_out="rgb48le", stages="lut3d", engine=eng)
    with pytest.raises(ValueError, match="rgb_out"):
        apply_lut([p for p in _planes("yuv444p10le")], cube=_lut(), pix_fmt="gbrp10le", rgb_out="gbrp10le", rgb_stages="lut3d", engine=eng)
    with pytest.raises(ValueError, match="a follow-up"):
        check_yuv2rgb_options("yuva420p10le", "rgba64le")


# ------------------------------------------------------------------ what the layers hand down
def test_apply_lut_hands_the_engine_the_call():
    from lut_renderer_amd.api import apply_lut

    class _Lock:
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    class _Eng:
        _lock, precision, _applied_lut, _applied_lut2, _applied_lut1d, _has_prelut = _Lock(), "strict", None, None, None, False
        n = n2 = n1d = 0

        def __init__(self): self.calls = []
        def apply_yuv_stack_to_rgb(self, planes, out, **kw): self.calls.append(kw); return out
        def set_lut(self, lut): pass

    eng = _Eng()
    apply_lut(_planes(), cube=_lut(), pix_fmt="yuv420p10le", engine=eng, rgb_out="rgb48le", rgb_out_stages="matrix,lut3d:nearest",
              rgb_matrix=GAMUT)
    call = eng.calls[-1]
    assert call == dict(stages=(("matrix", None), ("lut3d", "nearest")), cdl=None, rgb_matrix=GAMUT, pix_fmt="yuv420p10le",
                        out_pix_fmt="rgb48le", matrix_in="smpte170m", range_src="tv", range_in="tv")
    apply_lut(_planes("yuv420p"), cube=_lut(), interp="trilinear", pix_fmt="yuvj420p", colorspace="bt709", color_range="pc", engine=eng,
              rgb_out="bgra", rgb_out_stages="cdl,lut3d", cdl=Cdl())
    call = eng.calls[-1]
    assert call["stages"] == (("cdl", None), ("lut3d", "trilinear")) and call["out_pix_fmt"] == "bgra" and call["pix_fmt"] == "yuv420p"
    assert call["matrix_in"] == "bt709" and call["range_src"] == "pc" and call["range_in"] in ("tv", "pc") and call["cdl"] == Cdl()


@pytest.mark.parametrize("rgb_out,frame_bytes", [("gbrp10le", 16 * 8 * 3 * 2), ("rgb24", 16 * 8 * 3), ("rgba64le", 16 * 8 * 8),
                                                 ("gbrap", 16 * 8 * 4)])
def test_plan_from_args_gives_the_call_and_the_frame_sizes(cube_dir, rgb_out, frame_bytes):
    from lut_renderer_amd.cli import plan_from_args
    from lut_renderer_amd.stream import input_layout, output_layout
    a, t, cc = str(cube_dir / "log709_33.cube"), str(GOLDEN / "lut1d" / "curve17.cube"), str(GOLDEN / "cdl" / "shot.cc")
    f = str(GOLDEN / "matrix" / "bt2020_to_709.spimtx")
    src = "yuv420p" if y2r.dest_depth(rgb_out) == 8 else "yuv420p10le"
    assert _args("--cube", a).rgb_out_stages is None
    _, kw, w, h = plan_from_args(_args("--cube", a, "--rgb-out-stages", "lut3d", pix_fmt=src, rgb_out=rgb_out))
    assert kw == dict(pix_fmt=src, out_pix_fmt=rgb_out, rgb_out_stages=(("lut3d", "tetrahedral"),), matrix_in="smpte170m",
                      range_src="tv", range_in="tv") and (w, h) == (16, 8)
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--interp", "trilinear", "--lut1d", t, "--cdl", cc, "--rgb-matrix-file", f,
                                       "--colorspace", "bt709", "--rgb-out-stages", "lut1d,cdl,matrix,lut3d", pix_fmt=src,
                                       rgb_out=rgb_out))
    assert kw["rgb_out_stages"] == (("lut1d", None), ("cdl", None), ("matrix", None), ("lut3d", "trilinear"))
    assert kw["cdl"] == read_cdl(cc) and kw["rgb_matrix"] == read_rgb_matrix(f) and kw["matrix_in"] == "bt709"
    assert output_layout(rgb_out, w, h).frame_bytes == frame_bytes
    assert input_layout(src, w, h).frame_bytes == 16 * 8 * 3 // 2 * (1 if src == "yuv420p" else 2)
    # no --cube: none is needed for a list without lut3d
    _, kw, _, _ = plan_from_args(_args("--rgb-out-stages", "matrix", "--rgb-matrix", I3.m_text(), pix_fmt=src, rgb_out=rgb_out))
    assert kw["rgb_matrix"] == I3 and kw["out_pix_fmt"] == rgb_out


def test_engine_command_renders_the_flags_only_when_given(cube_dir):
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    from lut_renderer_amd.pipe import engine_stage_commands
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv422p10le", color_range="tv", colorspace="bt709", fps=25.0)
    a, t, f = cube_dir / "log709_33.cube", GOLDEN / "lut1d" / "curve17.cube", GOLDEN / "matrix" / "bt2020_to_709.spimtx"
    for params in (ProcessingParams(video_codec=""), ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")):
        io = (Path("-"), Path("-"), params, a, info)
        plain = engine_command(*io)
        assert "--rgb-out" not in plain and "--rgb-out-stages" not in plain
        assert engine_command(*io, rgb_out=None, rgb_out_stages=None) == plain
        base = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info)
        assert base == engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, rgb_out=None, rgb_out_stages=None)
        assert "--rgb-out" not in base.engine
    params = ProcessingParams(video_codec="")
    io = (Path("-"), Path("-"), params, a, info)
    plain = engine_command(*io)
    assert engine_command(*io, rgb_out="gbrp10le", rgb_out_stages="lut3d") == plain + ["--rgb-out", "gbrp10le", "--rgb-out-stages",
                                                                                      "lut3d:tetrahedral"]
    # params that resolve the very format rgb_out names: --rgb-out takes the place of --out-pix-fmt
    same = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="dpx", pix_fmt="gbrp10le"), a, info, rgb_out="gbrp10le",
                          rgb_out_stages="lut3d")
    assert "--out-pix-fmt" not in same and same[-4:] == ["--rgb-out", "gbrp10le", "--rgb-out-stages", "lut3d:tetrahedral"]
    grade = Cdl(slope=(1.1, 1.0, 0.9), saturation=0.8)
    cmd = engine_command(*io, lut1d=t, cdl=grade, rgb_matrix=f, rgb_out="rgb48le", rgb_out_stages="lut1d,cdl,matrix,lut3d")
    assert cmd == plain + ["--cdl-sop", grade.sop_text(), "--cdl-sat", repr(0.8), "--lut1d", str(t), "--rgb-matrix-file", str(f),
                           "--rgb-out", "rgb48le", "--rgb-out-stages", "lut1d,cdl,matrix,lut3d:tetrahedral"]
    # the round trip: the CLI parses what the builder rendered into the same call
    _, kw, w, h = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert kw["rgb_out_stages"] == (("lut1d", None), ("cdl", None), ("matrix", None), ("lut3d", "tetrahedral")) and (w, h) == (64, 8)
    assert kw["cdl"] == grade and kw["rgb_matrix"] == read_rgb_matrix(f) and kw["out_pix_fmt"] == "rgb48le"
    assert kw["pix_fmt"] == "yuv422p10le" and kw["matrix_in"] == "bt709"
    cmds = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, rgb_out="rgb48le", rgb_out_stages="lut3d:trilinear")
    assert cmds.engine[cmds.engine.index("--rgb-out-stages") + 1] == "lut3d:trilinear"
    assert cmds.encoder[cmds.encoder.index("-pix_fmt") + 1] == "rgb48le"            # the encoder reads what the engine writes
    with pytest.raises(ValueError, match="together with rgb_out_stages only"):
        engine_command(*io, rgb_out="rgb48le")
