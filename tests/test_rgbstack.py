"""The stage stack on RGB sources without a GPU: the twin's list walk against the pinned one of the YUV stack, its
`[lut3d]` anchor against the RGB -> YUV twin, the one copy of the refusals through every layer, the old names still refusing RGB,
and the argv."""
import threading
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from lut_renderer_amd import cube, frames
from lut_renderer_amd.cdl import Cdl, read_cdl
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.formats import check_rgb_stack_options, check_stack_options
from lut_renderer_amd.rgbmatrix import RgbMatrix, read_rgb_matrix
from oracle.lut3d_numpy import yuv_to_rgb_codes
from tests import _lut1d_twin as l1t
from tests import _matrix_twin as mxt
from tests import _rgb2yuv_twin as r2y
from tests import _rgbstack_twin as twin

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
F = np.float32
I3 = RgbMatrix()
GAMUT = read_rgb_matrix(GOLDEN / "matrix" / "bt2020_to_709.spimtx")
NAMES = dict(pix_fmt="gbrp10le", out_pix_fmt="yuv422p10le")


def _eq(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _luts():
    rng = np.random.default_rng(11)
    a = cube.CubeLut(9, np.ones(3, F), rng.uniform(-0.2, 1.2, (9, 9, 9, 3)).astype(F))
    b = cube.CubeLut(5, np.array([1.0, 0.5, 1.0], F), rng.uniform(0.0, 1.0, (5, 5, 5, 3)).astype(F))
    return a, b


# ------------------------------------------------------------------ the twin
ORDERS = ("lut1d,matrix,lut3d", "lut3d,cdl,lut3d2", "cdl,lut3d", "matrix,cdl,lut1d", "lut1d,cdl,lut3d,lut3d2", "lut3d,matrix")


@pytest.mark.parametrize("stages", ORDERS)
def test_the_walk_is_the_pinned_walk_of_the_yuv_stack(orc, stages):
    """For a yuv444p10le frame the codes stage 1 produces, walked by the new twin, are what the YUV stack's twin sends to stage 3."""
    a, b = _luts()
    grade = read_cdl(GOLDEN / "cdl" / "shot.cc")
    l1 = cube.read_lut1d(GOLDEN / "lut1d" / "curve17.cube")
    tab = l1t.table(l1.table, l1.scale, "linear", 10)
    planes = frames.natural_yuv(37, 13, 10, 0, 0, k=2)
    k = mxt.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 0, 0)
    st = stages.split(",")
    res = dict(lut=a, lut2=b, l1d_tab=tab, cdl=grade if "cdl" in st else None, mtx=GAMUT if "matrix" in st else None)
    codes = yuv_to_rgb_codes(k, 0, 0, planes)
    assert _eq(twin.walk(st, 10, codes, **res), mxt.rgb_out(st, k, 10, 0, 0, planes, **res))


@pytest.mark.parametrize("pix_fmt", ["gbrp10le", "rgb24", "rgba64le"])
def test_lut3d_alone_is_the_rgb_to_yuv_twin(orc, pix_fmt):
    from tests.test_gpu_rgb2yuv import make_source
    lut, _ = _luts()
    dl = r2y.source_depth(pix_fmt)
    src = make_source(pix_fmt, "natural", 37, 13, k=3)
    for dout in {8: (8, 10), 10: (10, 8), 16: (10, 8)}[dl]:
        for lay, (ocsx, ocsy) in r2y.LAYOUTS.items():
            k = twin.consts("smpte170m", "tv", dl, dout, ocsx, ocsy)
            for mode in ("tetrahedral", "prism"):
                want = r2y.apply(lut.table, lut.scale, mode, k, pix_fmt, dout, ocsx, ocsy, src)
                assert _eq(twin.apply_yuv([("lut3d", mode)], k, pix_fmt, dout, ocsx, ocsy, src, lut=lut), want), (dout, lay, mode)


def test_a_word_above_m_enters_as_m_and_identities_give_the_source():
    g, b, r = frames.uniform_rgb(16, 4, 10, k=1)
    high = [g.copy(), b.copy(), r.copy()]
    high[0][0, :4] = [1024, 2047, 65535, 1023]
    clamped = [np.minimum(p, 1023) for p in high]
    assert _eq(twin.apply_rgb(["cdl"], "gbrp10le", high, cdl=Cdl()), clamped)
    assert _eq(twin.apply_rgb(["matrix"], "gbrp10le", high, mtx=I3), clamped)


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
    (dict(stages="lut3d", pix_fmt="yuv420p10le"), "is not an RGB format"),
    (dict(stages="lut3d", pix_fmt="gbrpf32le"), "a float source"),
    (dict(stages="lut3d", out_pix_fmt="rgb48le"), "a packed RGB destination"),
    (dict(stages="lut3d", out_pix_fmt="gbrpf32le"), "a float destination"),
    (dict(stages="lut3d", out_pix_fmt="gbrp12le"), "a gbrp destination of another depth"),
    (dict(stages="lut3d", out_pix_fmt="nv12"), "is not a destination"),
    (dict(stages="lut3d", pix_fmt="rgb24", out_pix_fmt=None), "needs out_pix_fmt"),
    (dict(stages="lut3d", intermediate_pix_fmt="yuv420p"), "full-range two-stage composition"),
    (dict(stages="lut3d", dither="error_diffusion"), r"dither \('error_diffusion'\) is not supported"),
    (dict(stages="lut3d", dither="blue_noise"), r"dither \('blue_noise'\) is not supported"),
    (dict(stages="lut3d", out_size=(8, 8)), "a resize"),
    (dict(stages="lut3d", chroma_loc="left"), "chroma_loc"),
    (dict(stages="lut3d", strength=0.5), "strength"),
    (dict(stages="lut3d", matte=True), "a matte"),
    (dict(stages="lut3d", alpha_mode="premultiplied"), "alpha_mode='premultiplied'"),
    (dict(stages="lut3d", out2_pix_fmt="yuv420p"), "two-output"),
    (dict(stages="lut3d", variant="vec_lds"), "vec_lds"),
    (dict(stages="lut3d:prism", variant="vec_global"), "vec_global cannot take stage 'lut3d:prism'"),
    (dict(stages="lut3d", pix_fmt="rgb24", out_pix_fmt="yuv422p10le", variant="vec_global"), "vec_global cannot take an 8-bit source"),
)


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[m for _, m in REFUSALS])
def test_check_rgb_stack_options_refuses(kw, message):
    with pytest.raises(ValueError, match=message):
        check_rgb_stack_options(**{**NAMES, **kw})


def test_what_check_rgb_stack_options_takes():
    st, fin, fout = check_rgb_stack_options("gbrp10le", None, stages="lut1d,cdl,lut3d:trilinear", cdl=True)
    assert st == (("lut1d", None), ("cdl", None), ("lut3d", "trilinear")) and fin.depth == 10
    assert (fout.name, fout.family, fout.depth, fout.alpha) == ("gbrp10le", "gbr", 10, False)
    assert check_rgb_stack_options("gbrap12le", None, stages="lut3d")[2].alpha
    for src, out in (("gbrp", "yuv420p10le"), ("rgb48le", "gbrp16le"), ("rgba", "yuva420p"), ("gbrp16le", "yuv444p"), ("bgr24", "gbrap")):
        _, fin, fout = check_rgb_stack_options(src, out, stages="matrix", rgb_matrix=True)
        assert fin.name == src and fout.name == out


def _planes(depth=10):
    import torch
    return [torch.from_numpy(p.view(np.int16)) for p in frames.natural_rgb(16, 8, depth)]


def test_the_engine_refuses_before_it_is_touched():
    src = _planes()
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False)
    for kw, message in ((dict(stages="matrix,lut3d"), "no RGB matrix is given"), (dict(stages="cdl"), "no CDL is given"),
                        (dict(stages="lut3d", pix_fmt="gbrpf32le"), "a float source"),
                        (dict(stages="lut3d", out_pix_fmt="rgb24"), "a packed RGB destination"),
                        (dict(stages="lut3d", out_pix_fmt="gbrp"), "another depth"),
                        (dict(stages="lut3d", dither="blue_noise"), "dither"), (dict(stages="lut3d", out_size="8x8"), "a resize"),
                        (dict(stages="lut3d", chroma_loc="left"), "chroma_loc"), (dict(stages="lut3d", strength=1.0), "strength"),
                        (dict(stages="lut3d", matte=src[0]), "a matte"),
                        (dict(stages="lut3d", alpha_mode="premultiplied"), "premultiplied"),
                        (dict(stages="lut3d", out2_pix_fmt="yuv420p"), "two-output"),
                        (dict(stages="lut3d", intermediate_pix_fmt="yuv420p"), "full-range")):
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_rgb_stack(held, src, **{**NAMES, **kw})
    with pytest.raises(ValueError, match="vec_lds"):
        LutEngine.apply_rgb_stack(SimpleNamespace(n=33, _variant_name="vec_lds"), src, **NAMES, stages="lut3d")
    with pytest.raises(ValueError, match="directly behind 'cdl'"):
        LutEngine.apply_rgb_stack(SimpleNamespace(n=33, _has_prelut=True), src, **NAMES, stages="cdl,lut3d", cdl=Cdl())
    with pytest.raises(TypeError, match="unexpected keyword argument 'interp'"):
        LutEngine.apply_rgb_stack(held, src, **NAMES, stages="lut3d", interp="nearest")
    with pytest.raises(TypeError, match="rgb_matrix must be a lut_renderer_amd.rgbmatrix.RgbMatrix"):
        LutEngine.apply_rgb_stack(held, src, **NAMES, stages="matrix", rgb_matrix="a.spimtx")


def test_the_group_checks_the_same_things_first():
    from lut_renderer_amd.multigpu import LutEngineGroup
    g = SimpleNamespace(_lock=threading.RLock(), n1d=17, engines=[SimpleNamespace(n=33, n2=0, _has_prelut=True)])
    for kw, message in ((dict(stages="matrix,lut3d"), "no RGB matrix is given"), (dict(stages="lut3d2"), "no second LUT"),
                        (dict(stages="cdl,lut3d", cdl=Cdl()), "directly behind 'cdl'"),
                        (dict(stages="lut3d", out_pix_fmt="bgra"), "a packed RGB destination"),
                        (dict(stages="lut3d", strength=0.5), "strength"), (dict(stages="lut3d", dither="blue_noise"), "dither"),
                        (dict(stages="lut3d", row0=0), "the group owns the row partition")):
        with pytest.raises(ValueError, match=message):
            LutEngineGroup.apply_rgb_stack(g, _planes(), **{**NAMES, **kw})


def _lut(n=2):
    return cube.CubeLut(n, np.ones(3, F), cube.identity_lattice(n).astype(F))


def test_apply_lut_refuses_while_planning_and_hands_the_engine_the_call():
    from lut_renderer_amd.api import apply_lut
    src = _planes()
    base = dict(pix_fmt="gbrp10le", out_pix_fmt="yuv422p10le", engine=SimpleNamespace(n=0, n2=0, n1d=0, _has_prelut=False))
    for kw, message in ((dict(cube=_lut(), rgb_stages="lut3d", stages="lut3d"), "stages and rgb_stages are mutually exclusive"),
                        (dict(cube=_lut(), rgb_stages="lut3d", pix_fmt="yuv420p10le"), "rgb_stages is the stage list of an RGB source"),
                        (dict(cube=_lut(), rgb_stages="cdl"), "cube is given and the stage list has no 'lut3d' stage"),
                        (dict(cube=None, rgb_stages="lut3d"), "no 3D LUT is loaded"),
                        (dict(cube=_lut(), rgb_stages="matrix,lut3d"), "no RGB matrix is given"),
                        (dict(cube=_lut(), rgb_stages="lut3d", rgb_matrix=I3), "has no 'matrix' stage"),
                        (dict(cube=_lut(), rgb_stages="lut3d", out_pix_fmt="rgb24"), "a packed RGB destination"),
                        (dict(cube=_lut(), rgb_stages="lut3d", out_pix_fmt="gbrp12le"), "another depth"),
                        (dict(cube=_lut(), rgb_stages="lut3d", pix_fmt="gbrpf32le"), "a float source"),
                        (dict(cube=_lut(), rgb_stages="lut3d", color_range="pc"), "full-range two-stage composition"),
                        (dict(cube=_lut(), rgb_stages="lut3d", zscale_dither="error_diffusion"), "dither"),
                        (dict(cube=_lut(), rgb_stages="lut3d", engine_dither="blue_noise"), "dither"),
                        (dict(cube=_lut(), rgb_stages="lut3d", resolution="8x8"), "a resize"),
                        (dict(cube=_lut(), rgb_stages="lut3d", chroma_loc="left"), "chroma_loc"),
                        (dict(cube=_lut(), rgb_stages="lut3d", strength=0.5), "strength"),
                        (dict(cube=_lut(), rgb_stages="lut3d", matte=src[0]), "a matte"),
                        (dict(cube=_lut(), rgb_stages="lut3d", alpha_mode="premultiplied"), "premultiplied"),
                        (dict(cube=_lut(), rgb_stages="lut3d", second_pix_fmt="yuv420p"), "two-output"),
                        (dict(cube=_lut(), rgb_stages="lut3d", rgb_out="gbrp10le"), "rgb_out")):
        with pytest.raises(ValueError, match=message):
            apply_lut(src, **{**base, **kw})

    class _Lock:
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    class _Eng:
        _lock, precision, _applied_lut, _applied_lut2, _applied_lut1d, _has_prelut = _Lock(), "strict", None, None, None, False
        n = n2 = n1d = 0

        def __init__(self): self.calls = []
        def apply_rgb_stack(self, planes, out, **kw): self.calls.append(kw); return out
        def set_lut(self, lut): pass

    eng = _Eng()
    apply_lut(src, cube=_lut(), pix_fmt="gbrp10le", engine=eng, rgb_stages="matrix,lut3d:nearest", rgb_matrix=GAMUT, cdl=None)
    call = eng.calls[-1]
    assert call["stages"] == (("matrix", None), ("lut3d", "nearest")) and call["rgb_matrix"] is GAMUT and call["out_pix_fmt"] is None
    assert call["matrix_out"] == "smpte170m" and call["range_out"] == "tv" and call["cdl"] is None
    apply_lut(src, cube=_lut(), interp="trilinear", pix_fmt="gbrp10le", out_pix_fmt="yuv420p", colorspace="bt709", engine=eng,
              rgb_stages="cdl,lut3d", cdl=Cdl())
    call = eng.calls[-1]
    assert call["stages"] == (("cdl", None), ("lut3d", "trilinear")) and call["out_pix_fmt"] == "yuv420p" and call["matrix_out"] == "bt709"


def test_host_pipeline_refuses_in_its_constructor():
    from lut_renderer_amd.stream import HostPipeline
    eng = SimpleNamespace(n=33, n2=0, n1d=0, _has_prelut=False)
    for kw, message in ((dict(rgb_stages="lut3d", stages="lut3d"), "mutually exclusive"),
                        (dict(rgb_stages="lut3d", rgb_out="gbrp10le"), "rgb_out"),
                        (dict(rgb_stages="lut3d", chain=True), "chain / lut1d are not set"),
                        (dict(rgb_stages="matrix,lut3d"), "no RGB matrix is given"),
                        (dict(rgb_stages="lut1d"), "no 1D LUT is loaded"),
                        (dict(rgb_stages="lut3d", out_size="8x8"), "a resize"),
                        (dict(rgb_stages="lut3d", second_pix_fmt="yuv420p"), "two-output"),
                        (dict(rgb_stages="lut3d", strength=0.5), "strength"),
                        (dict(rgb_stages="lut3d", strength_keys="0:1"), "strength_keys"),
                        (dict(rgb_stages="lut3d", dither="blue_noise"), "dither")):
        with pytest.raises(ValueError, match=message):
            HostPipeline(eng, "gbrp10le", 16, 8, **{"out_pix_fmt": "yuv422p10le", **kw})
    with pytest.raises(ValueError, match="a packed RGB destination"):
        HostPipeline(eng, "gbrp", 16, 8, out_pix_fmt="rgb24", rgb_stages="lut3d")


# ------------------------------------------------------------------ the old names still refuse RGB, in today's words
def test_the_yuv_stack_still_refuses_rgb(cube_dir):
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.cli import plan_from_args
    with pytest.raises(ValueError, match="is an RGB format"):
        check_stack_options("gbrp10le", None, stages="lut3d")
    with pytest.raises(ValueError, match="is an RGB format"):
        check_stack_options("yuv420p10le", "gbrp10le", stages="lut3d")
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False)
    with pytest.raises(ValueError, match="is an RGB format"):
        LutEngine.apply_yuv_stack(held, _planes(), pix_fmt="gbrp10le", stages="lut3d")
    with pytest.raises(ValueError):
        apply_lut(_planes(), cube=_lut(), pix_fmt="gbrp10le", stages="lut3d", engine=held)
    with pytest.raises(ValueError, match="is an RGB format"):
        apply_lut(_planes(), cube=_lut(), pix_fmt="gbrp10le", out_pix_fmt="yuv422p10le", stages="lut3d", engine=held)
    with pytest.raises(ValueError, match="is an RGB format"):
        plan_from_args(_args("--cube", str(cube_dir / "log709_33.cube"), "--stages", "lut3d"))


# ------------------------------------------------------------------ the CLI and the argv
def _args(*extra, pix_fmt="gbrp10le", out="yuv422p10le"):
    from lut_renderer_amd.cli import build_parser
    head = ["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt]
    return build_parser().parse_args(head + ([] if out is None else ["--out-pix-fmt", out]) + list(extra))


def test_cli_flags(cube_dir):
    from lut_renderer_amd.cli import plan_from_args
    a, t = str(cube_dir / "log709_33.cube"), str(GOLDEN / "lut1d" / "curve17.cube")
    f, cc = str(GOLDEN / "matrix" / "bt2020_to_709.spimtx"), str(GOLDEN / "cdl" / "shot.cc")
    assert _args("--cube", a).rgb_stages is None
    _, kw, w, h = plan_from_args(_args("--cube", a, "--rgb-stages", "lut3d"))
    assert kw == dict(pix_fmt="gbrp10le", out_pix_fmt="yuv422p10le", rgb_stages=(("lut3d", "tetrahedral"),), matrix_out="smpte170m",
                      range_out="tv") and (w, h) == (16, 8)
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--interp", "trilinear", "--lut1d", t, "--cdl", cc, "--rgb-matrix-file", f,
                                       "--rgb-stages", "lut1d,cdl,matrix,lut3d", out=None))
    assert kw["out_pix_fmt"] == "gbrp10le" and kw["rgb_stages"] == (("lut1d", None), ("cdl", None), ("matrix", None), ("lut3d", "trilinear"))
    assert kw["cdl"] == read_cdl(cc) and kw["rgb_matrix"] == read_rgb_matrix(f)
    _, kw, _, _ = plan_from_args(_args("--rgb-stages", "matrix", "--rgb-matrix", I3.m_text(), pix_fmt="rgb48le", out="gbrp16le"))
    assert kw["pix_fmt"] == "rgb48le" and kw["out_pix_fmt"] == "gbrp16le" and kw["rgb_matrix"] == I3      # no --cube: none is needed
    full = ("--cube", a, "--rgb-stages", "lut3d")
    for extra, message in ((("--stages", "lut3d"), "--stages and --rgb-stages are mutually exclusive"),
                           (("--lut1d", t), "--lut1d is given and --rgb-stages has no 'lut1d' stage"),
                           (("--interp2", "nearest"), "--rgb-stages has no 'lut3d2' stage"),
                           (("--engine-dither", "blue_noise"), r"dither \('blue_noise'\) is not supported"),
                           (("--zscale-dither", "error_diffusion"), "dither"), (("--out-size", "8x8"), "a resize"),
                           (("--chroma-loc", "left"), "chroma_loc"), (("--strength", "0.5"), "strength"),
                           (("--strength-keys", "0:1"), "strength"), (("--matte", "m.gray"), "a matte"),
                           (("--alpha-mode", "premultiplied"), "premultiplied"),
                           (("--second-output", "c", "--second-pix-fmt", "yuv420p"), "two-output"),
                           (("--color-range", "pc"), "full-range two-stage composition")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args(*full, *extra))
    for names, message in ((dict(pix_fmt="yuv420p10le"), "is not an RGB format"), (dict(pix_fmt="gbrpf32le"), "a float source"),
                           (dict(out="rgb24"), "a packed RGB destination"), (dict(out="gbrp"), "another depth"),
                           (dict(pix_fmt="rgb24", out=None), "needs out_pix_fmt")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args(*full, **names))


def test_engine_command_renders_the_flag_only_when_given(cube_dir):
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    from lut_renderer_amd.pipe import engine_stage_commands
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="gbrp10le", fps=25.0)
    params = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")
    a, t, f = cube_dir / "log709_33.cube", GOLDEN / "lut1d" / "curve17.cube", GOLDEN / "matrix" / "bt2020_to_709.spimtx"
    io = (Path("-"), Path("-"), params, a, info)
    plain = engine_command(*io)
    assert "--rgb-stages" not in plain and engine_command(*io, rgb_stages=None) == plain
    assert engine_command(*io, rgb_stages="lut3d") == plain + ["--rgb-stages", "lut3d:tetrahedral"]
    grade = Cdl(slope=(1.1, 1.0, 0.9), saturation=0.8)
    cmd = engine_command(*io, lut1d=t, cdl=grade, rgb_matrix=f, rgb_stages="lut1d,cdl,matrix,lut3d")
    assert cmd == plain + ["--cdl-sop", grade.sop_text(), "--cdl-sat", repr(0.8), "--lut1d", str(t), "--rgb-matrix-file", str(f),
                           "--rgb-stages", "lut1d,cdl,matrix,lut3d:tetrahedral"]
    # the round trip: the CLI parses what the builder rendered into the same call
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert kw["rgb_stages"] == (("lut1d", None), ("cdl", None), ("matrix", None), ("lut3d", "tetrahedral"))
    assert kw["cdl"] == grade and kw["rgb_matrix"] == read_rgb_matrix(f) and kw["out_pix_fmt"] == "yuv422p10le"
    # a YUV source: the argv without the flag is byte for byte what it was
    yinfo = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    assert engine_command(Path("-"), Path("-"), params, a, yinfo, rgb_stages=None) == engine_command(Path("-"), Path("-"), params, a, yinfo)
    cmds = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, rgb_stages="lut3d:trilinear")
    assert cmds.engine[cmds.engine.index("--rgb-stages") + 1] == "lut3d:trilinear"
    base = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info)
    assert "--rgb-stages" not in base.engine and base == engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, rgb_stages=None)
    for kw, message in ((dict(rgb_stages="lut3d", stages="lut3d"), "mutually exclusive"),
                        (dict(rgb_stages="cdl,lut3d"), "no CDL is given"),
                        (dict(rgb_stages="lut3d", rgb_matrix=I3), "rgb_matrix is given and the stage list has no 'matrix' stage"),
                        (dict(rgb_stages="lut3d", strength=0.5), "strength"),
                        (dict(rgb_stages="lut3d", engine_dither="blue_noise"), "dither"),
                        (dict(rgb_stages="lut3d", matte=Path("m.gray")), "a matte")):
        with pytest.raises(ValueError, match=message):
            engine_command(*io, **kw)
    with pytest.raises(ValueError, match="is not an RGB format"):
        engine_command(Path("-"), Path("-"), params, a, yinfo, rgb_stages="lut3d")


# ------------------------------------------------------------------ the whole table through the layers above the one function
def _call_of(kw):
    """A row of REFUSALS as (what the engine holds, the keyword arguments of an `apply_rgb_stack` call)."""
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


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[m for _, m in REFUSALS])
def test_every_refusal_through_the_engine_and_the_group(kw, message):
    from lut_renderer_amd.multigpu import LutEngineGroup
    held, call = _call_of(kw)
    with pytest.raises(ValueError, match=message):
        LutEngine.apply_rgb_stack(SimpleNamespace(**held), _planes(), **call)
    g = SimpleNamespace(_lock=threading.RLock(), n1d=held.pop("n1d"), engines=[SimpleNamespace(**held)])
    with pytest.raises(ValueError, match=message):
        LutEngineGroup.apply_rgb_stack(g, _planes(), **call)


#: what `engine_command` cannot be asked (it always renders a LUT, reads no LUT file and has no variant argument) ...
_NOT_THE_BUILDERS = ("no 3D LUT is loaded", "directly behind 'cdl'", "directly behind 'matrix'", "vec_lds", "vec_global")
#: ... and the one row an older check of its own answers first, in that check's words
_BUILDER_WORDS = {"needs out_pix_fmt": "needs a resolved output pixel format"}


@pytest.mark.parametrize("kw,message", [r for r in REFUSALS if not r[1].startswith(_NOT_THE_BUILDERS)],
                         ids=[m for _, m in REFUSALS if not m.startswith(_NOT_THE_BUILDERS)])
def test_every_refusal_through_engine_command(kw, message):
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    kw = {**NAMES, **kw}
    stages = kw["stages"]
    if stages and "lut3d" not in [s.partition(":")[0] for s in stages.split(",")]:
        stages += ",lut3d"                                   # (the builder's LUT needs its stage: that refusal comes first)
    info = VideoInfo(width=64, height=8, pix_fmt=kw["pix_fmt"], fps=25.0, color_range="pc" if kw.get("intermediate_pix_fmt") else None)
    params = ProcessingParams(video_codec="prores_ks", pix_fmt=kw["out_pix_fmt"] or "",
                              zscale_dither="error_diffusion" if kw.get("dither") == "error_diffusion" else "none",
                              resolution="8x8" if kw.get("out_size") else None)
    extra = dict(rgb_stages=stages, cdl=Cdl() if kw.get("cdl") else None, rgb_matrix=I3 if kw.get("rgb_matrix") else None,
                 engine_dither="blue_noise" if kw.get("dither") == "blue_noise" else None, gpu_resize=bool(kw.get("out_size")),
                 chroma_loc=kw.get("chroma_loc"), strength=kw.get("strength"), alpha_mode=kw.get("alpha_mode", "straight"),
                 matte=Path("m.gray") if kw.get("matte") else None)
    if kw.get("out2_pix_fmt"):
        extra.update(second_output=Path("b.yuv"), second_pix_fmt=kw["out2_pix_fmt"])
    with pytest.raises(ValueError, match=_BUILDER_WORDS.get(message, message)):
        engine_command(Path("-"), Path("-"), params, Path("x.cube"), info, **extra)
