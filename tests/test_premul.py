"""Premultiplied alpha without a GPU: the properties of the two integer steps over every code pair, the twin
against the references it must collapse to for opaque alpha, the float specials, the routing of `alpha_mode` through
`engine_call_for` / `plan_from_args` / `engine_command`, every refusal that has to come before any GPU work, and the two C-ABI
symbols."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _premul_twin as twin
from tests import _rgbf_twin as rf
from tests import _xsub_twin as xs

F = np.float32


# ------------------------------------------------------------------ the contract's properties
def _pairs(din, dl):
    ma, ml = (1 << din) - 1, (1 << dl) - 1
    c, a = np.meshgrid(np.arange(ml + 1, dtype=np.int64), np.arange(ma + 1, dtype=np.int64), indexing="ij")
    return c, a, ma, ml


@pytest.mark.parametrize("din,dl", [(8, 8), (10, 10), (10, 8)], ids=["8", "10", "alpha10_lut8"])
def test_properties_exhaustive(din, dl):
    c, a, ma, ml = _pairs(din, dl)
    # the numerators stay inside 32 bits
    assert int((c * ma + a // 2).max()) <= 2**32 - 1 and int((c * a + ma // 2).max()) <= 2**32 - 1
    s = twin.unpremul(c, a, ma, ml)
    assert s.min() >= 0 and s.max() <= ml
    # opaque: both steps are the identity (where the colour fits the LUT depth's scale: Ma == Ml)
    if ma == ml:
        assert np.array_equal(s[:, ma], c[:, ma]) and np.array_equal(twin.premul(c[:, ma], a[:, ma], ma), c[:, ma])
    # transparent: S = C, P = 0
    assert np.array_equal(s[:, 0], c[:, 0]) and not twin.premul(c[:, 0], a[:, 0], ma).any()
    # round trip of every valid premultiplied pair
    valid = c * ma <= a * ml
    assert valid.sum() > c.size // 3
    back = twin.premul(s, a, ma)
    assert np.array_equal(back[valid], c[valid])
    # P never exceeds the LUT's code range for a <= Ma
    assert int(twin.premul(np.full_like(a, ml), a, ma).max()) <= ml


def test_properties_16_bit_random():
    rng = np.random.default_rng(18)
    n, ma = 2_000_000, 65535
    a = rng.integers(0, ma + 1, size=n, dtype=np.int64)
    a[:5] = (0, 1, 2, ma - 1, ma)
    c = (rng.random(n) * (a + 1)).astype(np.int64)             # valid pairs: C <= a
    c = np.minimum(c, a)
    assert int((c * ma + a // 2).max()) <= 2**32 - 1 and twin.numerator_max(ma, ma) <= 2**32 - 1
    s = twin.unpremul(c, a, ma, ma)
    assert s.max() <= ma and np.array_equal(twin.premul(s, a, ma), c)
    full = rng.integers(0, ma + 1, size=n, dtype=np.int64)     # any colour code: the clamp holds, opaque is the identity
    assert twin.unpremul(full, a, ma, ma).max() <= ma
    assert np.array_equal(twin.unpremul(full, np.full(n, ma), ma, ma), full)
    assert np.array_equal(twin.premul(full, np.full(n, ma), ma), full)
    assert not twin.premul(full, np.zeros(n, np.int64), ma).any()


# ------------------------------------------------------------------ the twin collapses to what exists
@pytest.fixture(scope="module")
def lut():
    return cube.log709_lattice(17), (1.0, 1.0, 1.0)


@pytest.mark.parametrize("size", [(8, 6), (7, 5)], ids=["8x6", "7x5"])
@pytest.mark.parametrize("depth", [8, 10])
def test_opaque_twin_is_the_straight_contract(orc, lut, size, depth):
    table, scale = lut
    w, h = size
    for il, (icsx, icsy) in xs.LAYOUTS.items():
        src = frames.natural_yuv(w, h, depth, icsx, icsy, k=3)
        opaque = np.full((h, w), (1 << depth) - 1, np.uint8 if depth == 8 else np.uint16)
        for ol, (ocsx, ocsy) in xs.LAYOUTS.items():
            k = twin.consts(din=depth, dl=depth, dout=depth, ocsx=ocsx, ocsy=ocsy)
            for interp in ("tetrahedral", "prism"):
                got = twin.apply(table, scale, interp, k, depth, depth, depth, icsx, icsy, ocsx, ocsy, src, opaque)
                want = xs.apply(table, scale, interp, k, depth, depth, icsx, icsy, ocsx, ocsy, src)
                assert all(np.array_equal(g, x) for g, x in zip(got, want)), (il, ol, interp)
                if il == ol:
                    ref = orc.apply_yuv(table, scale, interp, k, depth, depth, depth, icsx, icsy, src)
                    assert all(np.array_equal(g, x) for g, x in zip(got, ref)), (il, interp)


def test_transparent_twin_is_black(lut):
    table, scale = lut
    src = frames.natural_yuv(8, 6, 10, 1, 1, k=1)
    k = twin.consts(din=10, dl=10, dout=10, ocsx=1, ocsy=1)
    y, cb, cr = twin.apply(table, scale, "tetrahedral", k, 10, 10, 10, 1, 1, 1, 1, src, np.zeros((6, 8), np.uint16))
    assert (y == 64).all() and (cb == 512).all() and (cr == 512).all()
    # and a soft edge differs from the straight call: that is what the option is for
    half = np.full((6, 8), 512, np.uint16)
    soft = twin.apply(table, scale, "tetrahedral", k, 10, 10, 10, 1, 1, 1, 1, src, half)
    straight = xs.apply(table, scale, "tetrahedral", k, 10, 10, 1, 1, 1, 1, src)
    assert not np.array_equal(soft[0], straight[0])


def test_float_twin():
    table = cube.log709_lattice(9)
    scale = (1.0, 1.0, 1.0)
    src = rf.make_float("hdr", 16, 4, k=2)
    one = np.ones((4, 16), F)
    for interp in ("nearest", "trilinear", "tetrahedral"):
        got = twin.apply_float(table, scale, interp, src + [one])
        want = rf.apply_float(table, scale, interp, src)
        assert all(np.array_equal(g.view(np.uint32), x.view(np.uint32)) for g, x in zip(got[:3], want))
        assert np.array_equal(got[3], one)
    # specials: alpha in {NaN, -1, 0, subnormal, 0.5, 1, 2, +inf} x colour in {NaN, +-inf, subnormal, 1e38}
    alphas = np.array([np.nan, -1.0, 0.0, 1e-42, 0.5, 1.0, 2.0, np.inf, -0.0, -np.inf], F)
    colours = np.array([np.nan, np.inf, -np.inf, 1e-42, 1e38, 0.25, -1e38], F)
    cc, aa = np.meshgrid(colours, alphas, indexing="ij")
    t = twin.alpha_t(aa)
    assert np.array_equal(t[0].view(np.uint32), np.array([0, 0, 0, F(1e-42).view(np.uint32), F(0.5).view(np.uint32), F(1).view(np.uint32),
                                                          F(1).view(np.uint32), F(1).view(np.uint32), 0, 0], np.uint32))
    s = twin.unpremul_float(cc, t)
    assert np.isfinite(s).all()
    fmax = np.finfo(F).max
    assert s[4, 3] == fmax and s[6, 3] == -fmax                # 1e38 / subnormal overflows: sanitised to +-FLT_MAX
    assert s[1, 4] == fmax and s[2, 4] == -fmax and s[0, 4] == 0   # +-inf, NaN sanitised before the division
    assert s[3, 3] == F(1e-42) / F(1e-42) and s[3, 4] == F(1e-42) / F(0.5)   # subnormals kept
    assert np.array_equal(s[:, 2], rf.sanitize(colours)) and np.array_equal(s[:, 0], rf.sanitize(colours))
    out = twin.apply_float(table, scale, "tetrahedral", [cc, cc.copy(), cc.copy(), aa])
    assert all(np.isfinite(p).all() for p in out[:3]) and not out[0][:, 2].any() and not out[0][:, 0].any()
    assert np.array_equal(out[3].view(np.uint32), aa.view(np.uint32))


# ------------------------------------------------------------------ routing
def _plan(pix_fmt, out_pix_fmt=None, alpha_mode=None, **info):
    from lut_renderer_amd.api import engine_call_for
    from lut_renderer_amd.engine import source_bit_depth
    from lut_renderer_amd.plan import resolve_lut_plan
    vi = VideoInfo(width=8, height=6, pix_fmt=pix_fmt, bit_depth=source_bit_depth(pix_fmt), **info)
    plan = resolve_lut_plan(ProcessingParams(), "look.cube", vi)
    if alpha_mode is None:
        return engine_call_for(plan, pix_fmt, out_pix_fmt)
    return engine_call_for(plan, pix_fmt, out_pix_fmt, alpha_mode=alpha_mode)


def test_engine_call_for():
    for src, out in (("yuva444p10le", None), ("yuva420p", "yuv422p"), ("yuva444p12le", "yuva444p12le"), ("gbrapf32le", None),
                     ("yuv420p", None), ("gbrap10le", "yuva444p10le")):
        assert _plan(src, out) == _plan(src, out, "straight") and "alpha_mode" not in _plan(src, out)
    kw = _plan("yuva444p10le", None, "premultiplied")
    assert kw == dict(_plan("yuva444p10le"), alpha_mode="premultiplied")
    kw = _plan("yuva420p10le", "yuv422p", "premultiplied")
    assert (kw["out_pix_fmt"], kw["alpha_mode"]) == ("yuv422p", "premultiplied")
    kw = _plan("gbrapf32le", None, "premultiplied")
    assert kw == dict(pix_fmt="gbrapf32le", out_pix_fmt="gbrapf32le", interp="tetrahedral", alpha_mode="premultiplied")
    for src, out, info, what in (("yuv420p", None, {}, "has none"),
                                 ("nv12", None, {}, "has none"),
                                 ("gbrpf32le", None, {}, "has none"),
                                 ("gbrap10le", "yuva444p10le", {}, "integer RGB"),
                                 ("rgba", "yuva420p", {}, "integer RGB"),
                                 ("gbrapf32le", "yuva444p10le", {}, "float source with an integer or YUV output"),
                                 ("gbrapf32le", "gbrpf32le", {}, "float source"),
                                 ("yuva444p10le", "nv12", {}, "alpha|planar"),
                                 ("yuva420p", None, {"color_range": "pc"}, "prologue")):
        with pytest.raises(ValueError, match=what):
            _plan(src, out, "premultiplied", **info)
    with pytest.raises(ValueError, match="unknown alpha_mode"):
        _plan("yuva444p10le", None, "associated")


def test_cli_and_command_argv():
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.pipe import engine_stage_commands
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    _, kw0, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuva444p10le"]))
    _, kw1, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuva444p10le", "--alpha-mode", "straight"]))
    assert kw0 == kw1 and "alpha_mode" not in kw0
    _, kw, w, h = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuva444p10le", "--alpha-mode", "premultiplied"]))
    assert kw == dict(kw0, alpha_mode="premultiplied") and (w, h) == (64, 36)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "gbrapf32le", "--alpha-mode", "premultiplied"]))
    assert kw["alpha_mode"] == "premultiplied" and kw["out_pix_fmt"] == "gbrapf32le"
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--pix-fmt", "yuva444p10le", "--alpha-mode", "associated"])
    pm = ["--alpha-mode", "premultiplied"]
    for extra, what in ((["--pix-fmt", "yuv420p"], "has none"),
                        (["--pix-fmt", "yuva420p", "--zscale-dither", "error_diffusion"], "dither"),
                        (["--pix-fmt", "yuva420p", "--engine-dither", "blue_noise"], "dither"),
                        (["--pix-fmt", "yuva420p", "--chroma-loc", "left"], "chroma_loc"),
                        (["--pix-fmt", "yuva420p", "--out-pix-fmt", "yuv420p", "--out-size", "32x18"], "resize"),
                        (["--pix-fmt", "yuva420p", "--second-output", "c", "--second-pix-fmt", "yuv420p"], "two-output"),
                        (["--pix-fmt", "yuva420p", "--cube2", "b.cube"], "two-LUT"),
                        (["--pix-fmt", "yuva420p", "--color-range", "pc"], "prologue"),
                        (["--pix-fmt", "gbrap12le", "--out-pix-fmt", "yuva444p12le"], "integer RGB"),
                        (["--pix-fmt", "rgba", "--out-pix-fmt", "yuva420p"], "integer RGB"),
                        (["--pix-fmt", "gbrapf32le", "--out-pix-fmt", "yuva444p10le"], "float source")):
        with pytest.raises(ValueError, match=what):
            plan_from_args(build_parser().parse_args(base + extra + pm))
    # engine_command: rendered only when premultiplied; its argv parses and routes
    info = VideoInfo(width=64, height=36, bit_depth=10, pix_fmt="yuva444p10le", fps=25.0)
    p = ProcessingParams(video_codec="prores_ks", pix_fmt="yuva444p10le")
    plain = engine_command(Path("-"), Path("-"), p, "look.cube", info, python_bin="python")
    assert plain == engine_command(Path("-"), Path("-"), p, "look.cube", info, python_bin="python", alpha_mode="straight")
    assert "--alpha-mode" not in plain
    cmd = engine_command(Path("-"), Path("-"), p, "look.cube", info, python_bin="python", alpha_mode="premultiplied")
    assert cmd == plain + ["--alpha-mode", "premultiplied"]
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["alpha_mode"]) == ("yuva444p10le", "yuva444p10le", "premultiplied")
    exr = VideoInfo(width=64, height=36, bit_depth=32, pix_fmt="gbrapf32le", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec=""), "look.cube", exr, python_bin="python",
                         alpha_mode="premultiplied")
    assert cmd[-2:] == ["--alpha-mode", "premultiplied"] and "--out-pix-fmt" not in cmd
    for kwargs, pp, vi, what in ((dict(alpha_mode="associated"), p, info, "unknown alpha_mode"),
                                 (dict(chroma_loc="left"), p, info, "chroma_loc"),
                                 (dict(engine_dither="blue_noise"), p, info, "dither"),
                                 (dict(cube2=Path("b.cube")), p, info, "alpha|two-LUT"),
                                 (dict(second_output=Path("c"), second_pix_fmt="yuv420p"), p, info, "two-output"),
                                 (dict(gpu_resize=True), ProcessingParams(video_codec="libx264", pix_fmt="yuv420p", resolution="32x18"),
                                  info, "resize"),
                                 ({}, ProcessingParams(video_codec="libx264", pix_fmt="yuv420p"),
                                  VideoInfo(width=64, height=36, bit_depth=8, pix_fmt="yuv420p", fps=25.0), "has none"),
                                 ({}, ProcessingParams(video_codec="libx264", pix_fmt="yuv420p"),
                                  VideoInfo(width=64, height=36, bit_depth=8, pix_fmt="yuva420p", fps=25.0, color_range="pc"), "prologue"),
                                 ({}, ProcessingParams(video_codec="prores_ks", pix_fmt="yuva444p10le"),
                                  VideoInfo(width=64, height=36, bit_depth=10, pix_fmt="gbrap10le", fps=25.0), "integer RGB"),
                                 ({}, ProcessingParams(video_codec="prores_ks", pix_fmt="yuva444p10le"), exr, "float source")):
        with pytest.raises(ValueError, match=what):
            engine_command(Path("-"), Path("-"), pp, "look.cube", vi, python_bin="python",
                           **dict(dict(alpha_mode="premultiplied"), **kwargs))
    # the stage: the engine's argv carries it, ffmpeg's two do not
    a = engine_stage_commands(Path("in.mov"), Path("out.mov"), p, "look.cube", info)
    b = engine_stage_commands(Path("in.mov"), Path("out.mov"), p, "look.cube", info, alpha_mode="premultiplied")
    assert a.decoder == b.decoder and a.encoder == b.encoder and b.engine == a.engine + ["--alpha-mode", "premultiplied"]
    assert a == engine_stage_commands(Path("in.mov"), Path("out.mov"), p, "look.cube", info, alpha_mode="straight")


# ------------------------------------------------------------------ refusals ahead of any GPU work
def test_rejections_before_any_gpu_work():
    import torch
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.engine import LutEngine, check_alpha_mode, check_premul_options
    from lut_renderer_amd.multigpu import LutEngineGroup
    from lut_renderer_amd.stream import HostPipeline
    assert check_alpha_mode("straight") is False and check_alpha_mode("premultiplied") is True
    with pytest.raises(ValueError, match="unknown alpha_mode"):
        check_alpha_mode(None)
    assert check_premul_options("yuva444p10le") == "yuv" and check_premul_options("yuva420p", "yuv444p16le") == "yuv"
    assert check_premul_options("gbrapf32le") == "float" and check_premul_options("gbrapf32le", "gbrapf32le") == "float"
    for args, kw, what in ((("yuv420p",), {}, "has none"),
                           (("p010le",), {}, "has none"),
                           (("uyvy422",), {}, "has none"),
                           (("v210",), {}, "has none"),
                           (("gbrpf32le",), {}, "has none"),
                           (("yuva420p",), dict(range_src="pc", range_in="tv", lut_depth=8), "prologue"),
                           (("yuva420p10le",), dict(lut_depth=8), "prologue"),
                           (("yuva420p",), dict(dither="error_diffusion"), "dither"),
                           (("yuva420p",), dict(dither="blue_noise"), "dither"),
                           (("yuva420p",), dict(chroma_loc="left"), "chroma_loc"),
                           (("yuva420p", "yuv420p"), dict(out_size=(4, 4)), "resize"),
                           (("yuva420p",), dict(out2_pix_fmt="yuv420p"), "two-output"),
                           (("yuva420p",), dict(lut2=True), "two-LUT"),
                           (("gbrap",), {}, "integer RGB"),
                           (("gbrap16le", "yuva444p16le"), dict(to_yuv=True), "integer RGB"),
                           (("rgba",), {}, "integer RGB"),
                           (("rgba64le", "yuva444p16le"), dict(to_yuv=True), "integer RGB"),
                           (("gbrapf32le", "yuva444p10le"), dict(to_yuv=True), "float source with an integer or YUV output"),
                           (("gbrapf32le", "gbrap16le"), {}, "float source"),
                           (("yuva444p10le", "p010le"), {}, "planar YUV output"),
                           (("yuva444p10le", "gbrap10le"), {}, "planar YUV output")):
        with pytest.raises(ValueError, match=what):
            check_premul_options(*args, **kw)
    planes = [torch.zeros((6, 8), dtype=torch.uint8) for _ in range(4)]
    fl = [torch.zeros((6, 8), dtype=torch.float32) for _ in range(4)]
    # LutEngine's own argument checking comes before anything of the engine is touched
    for kw, what in ((dict(pix_fmt="yuv420p"), "has none"),
                     (dict(pix_fmt="yuva420p", dither="blue_noise"), "dither"),
                     (dict(pix_fmt="yuva420p", chroma_loc="center"), "chroma_loc"),
                     (dict(pix_fmt="yuva420p", out_pix_fmt="yuv420p", out_size=(4, 4)), "resize"),
                     (dict(pix_fmt="yuva420p", range_src="pc", range_in="tv"), "prologue"),
                     (dict(pix_fmt="yuva420p", lut_depth=10), "prologue"),
                     (dict(pix_fmt="nv12"), "has none")):
        with pytest.raises(ValueError, match=what):
            LutEngine.apply_yuv(object(), planes, alpha_mode="premultiplied", **kw)
    with pytest.raises(ValueError, match="unknown alpha_mode"):
        LutEngine.apply_yuv(object(), planes, pix_fmt="yuva420p", alpha_mode="associated")
    with pytest.raises(ValueError, match="unknown alpha_mode"):
        LutEngine.apply_rgb_float(object(), fl, alpha_mode="associated")
    with pytest.raises(ValueError, match="has none"):
        LutEngine.apply_rgb_float(object(), fl[:3], alpha_mode="premultiplied")
    # the other entry points have no such keyword: an RGB source into YUV, the two-output pass and the chain stay straight
    import inspect
    for call in (LutEngine.apply_rgb_to_yuv, LutEngine.apply_yuv_dual, LutEngine.apply_yuv_chain, LutEngine.apply_rgb):
        assert "alpha_mode" not in inspect.signature(call).parameters
    with pytest.raises(TypeError, match="alpha_mode"):
        LutEngine.apply_rgb_to_yuv(object(), planes, pix_fmt="gbrap", out_pix_fmt="yuva420p", alpha_mode="premultiplied")
    with pytest.raises(ValueError, match="dither"):
        LutEngineGroup._apply_yuv(object(), planes, pix_fmt="yuva420p", dither="blue_noise", alpha_mode="premultiplied")
    with pytest.raises(ValueError, match="unknown alpha_mode"):
        LutEngineGroup._apply_yuv(object(), planes, pix_fmt="yuva420p", alpha_mode="associated")
    for kw, what in ((dict(pix_fmt="yuv420p"), "has none"),
                     (dict(pix_fmt="yuva420p", zscale_dither="error_diffusion"), "dither"),
                     (dict(pix_fmt="yuva420p", engine_dither="blue_noise"), "dither"),
                     (dict(pix_fmt="yuva420p", chroma_loc="left"), "chroma_loc"),
                     (dict(pix_fmt="yuva420p", out_pix_fmt="yuv420p", resolution="4x4"), "resize"),
                     (dict(pix_fmt="yuva420p", second_pix_fmt="yuv420p"), "two-output"),
                     (dict(pix_fmt="yuva420p", cube2="b.cube"), "two-LUT"),
                     (dict(pix_fmt="yuva420p", color_range="pc"), "prologue"),
                     (dict(pix_fmt="gbrap", out_pix_fmt="yuva420p"), "integer RGB"),
                     (dict(pix_fmt="gbrapf32le", out_pix_fmt="yuva420p"), "float source"),
                     (dict(pix_fmt="yuva420p", alpha_mode="associated"), "unknown alpha_mode")):
        with pytest.raises(ValueError, match=what):
            apply_lut(fl if "f32" in kw["pix_fmt"] else planes, cube="a.cube", engine=object(),
                      **dict(dict(alpha_mode="premultiplied"), **kw))
    for args, kw, what in ((("yuv420p",), {}, "has none"),
                           (("yuva420p",), dict(dither="blue_noise"), "dither"),
                           (("yuva420p",), dict(chroma_loc="left"), "chroma_loc"),
                           (("yuva420p",), dict(out_pix_fmt="yuv420p", out_size="4x4"), "resize"),
                           (("yuva420p",), dict(second_pix_fmt="yuv420p"), "two-output"),
                           (("yuva420p",), dict(chain=True), "two-LUT"),
                           (("gbrap",), dict(out_pix_fmt="yuva420p"), "integer RGB"),
                           (("gbrapf32le",), dict(out_pix_fmt="yuva420p"), "float source"),
                           (("yuva420p",), dict(alpha_mode="associated"), "unknown alpha_mode")):
        with pytest.raises(ValueError, match=what):
            HostPipeline(object(), *args, 8, 6, **dict(dict(alpha_mode="premultiplied"), **kw))


# ------------------------------------------------------------------ the C-ABI
def test_symbols_refuse_null_arguments():
    lib = _native.load()
    assert "lutr_apply_yuv_premul" in _native.SYMBOLS and "lutr_apply_planar_rgb_f32_premul" in _native.SYMBOLS
    p, pl, a = _native.YuvParams(), _native.Planes(), _native.AlphaSrc()
    assert lib.lutr_apply_yuv_premul(None, C.byref(p), 2, 8, 6, 1, C.byref(pl), C.byref(a), C.byref(pl), 0, 6) == _native.EINVAL
    assert b"null" in lib.lutr_last_error()
    assert lib.lutr_apply_yuv_premul(None, None, 2, 8, 6, 1, None, None, None, 0, 6) == _native.EINVAL
    assert lib.lutr_apply_planar_rgb_f32_premul(None, 2, 8, 6, 1, C.byref(pl), C.byref(a), C.byref(pl), 0, 6) == _native.EINVAL
    assert b"null" in lib.lutr_last_error()
    assert lib.lutr_apply_planar_rgb_f32_premul(None, 2, 8, 6, 1, None, None, None, 0, 6) == _native.EINVAL
    header = (Path(__file__).resolve().parent.parent / "include" / "lutr.h").read_text()
    assert "int lutr_apply_yuv_premul(" in header and "int lutr_apply_planar_rgb_f32_premul(" in header


def test_premultiplied_alpha_source_refusals_keep_their_words():
    """The alpha plane beside the colour planes of a premultiplied call: on the engine's device and with the colour planes'
    number of frames, for the YUV pass and the float pass alike (host only: an engine object without a context)."""
    import torch
    from lut_renderer_amd.engine import LutEngine
    eng = object.__new__(LutEngine)
    eng.device = torch.device("cpu")
    h, w = 6, 8

    def planes(dtype, alpha, n=4):
        return [torch.zeros((2, h, w), dtype=dtype) for _ in range(3)] + [alpha][:n - 3]

    for call, dtype, kw in ((eng.apply_yuv, torch.int16, dict(pix_fmt="yuva444p10le")), (eng.apply_rgb_float, torch.float32, {})):
        with pytest.raises(ValueError, match="^the alpha plane is on meta, engine is on cpu$"):
            call(planes(dtype, torch.zeros((2, h, w), dtype=dtype, device="meta")), planes(dtype, torch.zeros((2, h, w), dtype=dtype)),
                 alpha_mode="premultiplied", **kw)
        with pytest.raises(ValueError, match="^planes disagree on the number of frames$"):
            call(planes(dtype, torch.zeros((h, w), dtype=dtype)), planes(dtype, torch.zeros((2, h, w), dtype=dtype)),
                 alpha_mode="premultiplied", **kw)
