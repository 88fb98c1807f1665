"""Alpha-carrying frames without a GPU: the properties of the depth change over every code, the names and their
rawvideo layouts, the routing of `engine_call_for` / `plan_from_args` / `engine_command`, and every refusal that has to come
before any GPU work."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _alpha_twin as twin

ROOT = Path(__file__).resolve().parent.parent
PAIRS = [(a, b) for a in twin.DEPTHS for b in twin.DEPTHS if a != b]
#: the pairs on which the rounding expression evaluated in fp32 misses the nearest code
FP32_WRONG = {(10, 16), (12, 14), (12, 16), (14, 12), (14, 16), (16, 10), (16, 12), (16, 14)}


# ------------------------------------------------------------------ the depth change, every code of every pair
@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}to{b}" for a, b in PAIRS])
def test_depth_change_properties(pair):
    din, dout = pair
    mi, mo = (1 << din) - 1, (1 << dout) - 1
    codes = np.arange(mi + 1, dtype=np.int64)
    out = twin.convert(codes, din, dout)
    assert out[0] == 0 and out[-1] == mo                                   # opaque stays opaque
    assert np.all(np.diff(out) >= 0) and out.min() >= 0 and out.max() <= mo
    assert np.all((2 * codes * mo + mi) % (2 * mi) != 0)                   # no ties: Mi is odd
    assert np.all(np.abs(out * mi - codes * mo) * 2 < mi)                  # the nearest code, strictly
    if din < dout:
        assert np.array_equal(twin.convert(out, dout, din), codes)        # up, then down: the identity
    if pair == (8, 16):
        assert np.array_equal(out, codes * 257)
    assert np.array_equal(twin.convert_double(codes, din, dout), out)
    assert (not np.array_equal(twin.convert_fp32(codes, din, dout), out)) == (pair in FP32_WRONG)
    # words above Mi clamp to Mi
    assert np.all(twin.convert(np.array([mi + 1, 65535]), din, dout) == mo)


def test_same_depth_copies_the_words_and_fill_is_opaque():
    words = np.array([0, 5, 1023, 1024, 65535])
    assert np.array_equal(twin.convert(words, 10, 10), words)              # word for word: no clamp
    assert np.all(twin.fill((2, 3), 10) == 1023) and np.all(twin.fill((1,), 8) == 255)


def test_float_quantiser():
    a = np.array([np.nan, np.inf, -np.inf, -0.25, 0.0, 1.0, 1.5, 0.5 / 1023, 1.5 / 1023, 2.5 / 1023, 0.4999 / 1023], np.float32)
    # x.5 after the fp32 multiply rounds to the even code; the inputs are checked to land there
    halves = (a[7:10] * np.float32(1023)).tolist()
    assert halves == [0.5, 1.5, 2.5]
    assert twin.quantise(a, 10).tolist() == [0, 1023, 0, 0, 0, 1023, 1023, 0, 2, 2, 0]
    assert twin.quantise(np.array([1.0, 0.5], np.float32), 8).tolist() == [255, 128]
    assert twin.quantise(np.array([1.0], np.float32), 16).tolist() == [65535]


# ------------------------------------------------------------------ names and layouts
def test_names_parse():
    from lut_renderer_amd.engine import parse_pix_fmt, parse_rgb_source
    from lut_renderer_amd.stream import FrameLayout, input_layout, yuv_layout
    cases = {"yuva420p": (8, 1, 1), "yuva422p": (8, 1, 0), "yuva444p": (8, 0, 0), "yuva420p9le": (9, 1, 1),
             "yuva420p10le": (10, 1, 1), "yuva422p12le": (12, 1, 0), "yuva444p10le": (10, 0, 0), "yuva444p12le": (12, 0, 0),
             "yuva444p16le": (16, 0, 0), "yuva422p10": (10, 1, 0)}
    for name, (depth, csx, csy) in cases.items():
        f = parse_pix_fmt(name)
        assert (f.family, f.depth, f.csx, f.csy, f.alpha, f.nplanes, f.full_range) == ("yuv", depth, csx, csy, True, 4, False), name
        assert f.colour.name == name.replace("yuva", "yuv") and f.colour.nplanes == 3 and f.code == f.colour.code
        for w, h in ((7, 5), (8, 6)):
            cw, ch = (w + (1 << csx) - 1) >> csx, (h + (1 << csy) - 1) >> csy
            assert [f.plane_shape(i, w, h) for i in range(4)] == [(h, w), (ch, cw), (ch, cw), (h, w)]
            lay = yuv_layout(name, w, h)
            assert lay.frame_bytes == (2 * h * w + 2 * ch * cw) * (1 if depth == 8 else 2) and len(lay.plane_shapes) == 4
            assert isinstance(input_layout(name, w, h), FrameLayout)
    for name, depth in (("gbrap", 8), ("gbrap10le", 10), ("gbrap12le", 12), ("gbrap16le", 16)):
        f = parse_pix_fmt(name)
        assert (f.family, f.depth, f.csx, f.csy, f.alpha, f.nplanes) == ("gbr", depth, 0, 0, True, 4)
        assert f.colour.name == name.replace("gbrap", "gbrp")
        r = parse_rgb_source(name)
        assert (r.packed, r.floating, r.depth, r.nplanes, r.code) == (False, False, depth, 4, 0)
        for w, h in ((7, 5), (8, 6)):
            assert [f.plane_shape(i, w, h) for i in range(4)] == [(h, w)] * 4
            assert input_layout(name, w, h).frame_bytes == r.frame_bytes(w, h) == 4 * h * w * (1 if depth == 8 else 2)
    # the views of a rawvideo buffer: four planes back to back, alpha last
    import torch
    lay = yuv_layout("yuva420p10le", 8, 6)
    buf = torch.arange(2 * lay.frame_bytes, dtype=torch.int32).to(torch.uint8)
    views = lay.plane_views(buf, 2)
    assert [tuple(v.shape) for v in views] == [(2, 6, 8), (2, 3, 4), (2, 3, 4), (2, 6, 8)]
    assert views[3].storage_offset() == 6 * 8 + 2 * 3 * 4 and views[3].stride(0) == lay.frame_bytes // 2
    # a packed name's real alpha; a pad byte is none
    slots = {n: parse_rgb_source(n).alpha_slot for n in _native.PACKED_FORMATS}
    assert slots == {**{n: None for n in _native.PACKED_FORMATS}, "rgba": 3, "bgra": 3, "argb": 0, "abgr": 0, "rgba64le": 3,
                     "bgra64le": 3}
    # what stays refused, with the same text
    for bad in ("yuva420p8be", "yuva440p", "yuvaj420p", "gbrap7le", "gbrap17le", "yuva420p17le", "gbrap444p", "yuvap", "ya8",
                "yuva420", "gbra"):
        with pytest.raises(ValueError, match="unsupported"):
            parse_pix_fmt(bad)
    assert parse_rgb_source("yuva420p") is None


def test_existing_names_are_unchanged():
    from lut_renderer_amd.engine import PixFmt, parse_pix_fmt, parse_rgb_source
    from lut_renderer_amd.stream import input_layout
    for name, want in (("yuv420p", ("yuv", 8, 1, 1, False)), ("yuvj422p", ("yuv", 8, 1, 0, True)), ("yuv444p12le", ("yuv", 12, 0, 0, False)),
                       ("gbrp", ("gbr", 8, 0, 0, True)), ("gbrp10le", ("gbr", 10, 0, 0, True))):
        f = parse_pix_fmt(name)
        assert (f.family, f.depth, f.csx, f.csy, f.full_range) == want and not f.alpha and f.nplanes == 3 and f.colour is f
        assert len(input_layout(name, 8, 6).plane_shapes) == 3
    assert PixFmt("gbrp10", "gbr", 10, 0, 0, True).nplanes == 3            # positional construction keeps working
    assert input_layout("yuv420p10le", 8, 6).frame_bytes == 144 and input_layout("gbrp", 7, 5).frame_bytes == 105
    assert parse_rgb_source("gbrp12le").nplanes == 3 and parse_rgb_source("gbrapf32le").nplanes == 4
    assert input_layout("rgba", 7, 5).frame_bytes == 140 and input_layout("gbrapf32le", 7, 5).frame_bytes == 560


# ------------------------------------------------------------------ routing
def _plan(pix_fmt, out_pix_fmt=None, **info):
    from lut_renderer_amd.api import engine_call_for
    from lut_renderer_amd.engine import source_bit_depth
    from lut_renderer_amd.plan import resolve_lut_plan
    vi = VideoInfo(width=8, height=6, pix_fmt=pix_fmt, bit_depth=source_bit_depth(pix_fmt), **info)
    plan = resolve_lut_plan(ProcessingParams(), "look.cube", vi)
    return plan, engine_call_for(plan, pix_fmt, out_pix_fmt)


def test_engine_call_for():
    from lut_renderer_amd.api import is_float_out_call, is_rgb_call
    _, kw = _plan("yuva444p10le")                                          # keeps alpha
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["lut_depth"]) == ("yuva444p10le", "yuva444p10le", 10) and not is_rgb_call(kw)
    _, kw = _plan("yuva420p", "yuv420p")                                   # drops alpha
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["lut_depth"]) == ("yuva420p", "yuv420p", 8)
    _, kw = _plan("yuv420p10le", "yuva420p10le")                           # fills alpha
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("yuv420p10le", "yuva420p10le")
    _, kw = _plan("yuva444p12le", "yuva420p")                              # depth and subsampling change, alpha converted
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["lut_depth"]) == ("yuva444p12le", "yuva420p", 12)
    plan, kw = _plan("yuva444p10le", None, color_range="pc")               # the prologue's default output has no alpha
    assert plan.prologue and (kw["out_pix_fmt"], kw["lut_depth"], kw["range_src"]) == ("yuv444p", 8, "pc")
    plan, kw = _plan("yuva420p", "yuva420p", color_range="pc")             # ... a named one may: a prologue call FILLS it
    assert plan.prologue and (kw["pix_fmt"], kw["out_pix_fmt"], kw["lut_depth"]) == ("yuva420p", "yuva420p", 8)
    _, kw = _plan("rgba", "yuva420p")
    assert is_rgb_call(kw) and (kw["pix_fmt"], kw["out_pix_fmt"]) == ("rgba", "yuva420p") and "intermediate_pix_fmt" not in kw
    _, kw = _plan("gbrap10le", "yuva444p10le")
    assert is_rgb_call(kw) and (kw["pix_fmt"], kw["out_pix_fmt"]) == ("gbrap10le", "yuva444p10le")
    _, kw = _plan("gbrapf32le", "yuva444p10le")
    assert is_rgb_call(kw) and not is_float_out_call(kw) and kw["out_pix_fmt"] == "yuva444p10le"
    plan, kw = _plan("rgba", "yuva420p", color_range="pc")                 # the full-range composition (its output alpha is filled)
    assert plan.prologue and kw["intermediate_pix_fmt"] == "yuv420p" and kw["out_pix_fmt"] == "yuva420p"
    with pytest.raises(ValueError, match="needs|takes planar YUV frames, or an RGB source"):
        _plan("gbrap10le")                                                 # an RGB source still names its output


def test_dual_call_for():
    from lut_renderer_amd.api import dual_call_for
    from lut_renderer_amd.engine import check_dual_options
    from lut_renderer_amd.stream import dual_layout
    _, kw = _plan("yuva444p10le")
    dual = dual_call_for(kw, "yuv420p")
    assert (dual["pix_fmt"], dual["out_pix_fmt"], dual["out2_pix_fmt"]) == ("yuva444p10le", "yuva444p10le", "yuv420p")
    fin, f1, f2 = check_dual_options("yuv420p10le", "yuv422p10le", "yuva420p")
    assert (fin.nplanes, f1.nplanes, f2.nplanes) == (3, 3, 4)
    assert len(dual_layout("yuva444p10le", None, "yuva420p", 8, 6).plane_shapes) == 4
    with pytest.raises(ValueError, match="RGB format"):
        dual_call_for(kw, "gbrap10le")


def test_cli_and_command_argv():
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    _, kw, w, h = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuva444p10le"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["lut_depth"], w, h) == ("yuva444p10le", "yuva444p10le", 10, 64, 36)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuva444p10le", "--out-pix-fmt", "yuv420p"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("yuva444p10le", "yuv420p")
    _, kw, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuva420p", "--engine-dither", "blue_noise"]))
    assert (kw["out_pix_fmt"], kw["dither"]) == ("yuva420p", "blue_noise")
    _, kw, _, _ = plan_from_args(build_parser().parse_args(
        base + ["--pix-fmt", "yuva444p10le", "--second-output", "c", "--second-pix-fmt", "yuv420p"]))
    assert (kw["out_pix_fmt"], kw["out2_pix_fmt"]) == ("yuva444p10le", "yuv420p")
    _, kw, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "gbrap12le", "--out-pix-fmt", "yuva444p12le"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("gbrap12le", "yuva444p12le")
    # the stage's own argv parses and routes: no encoder -> the source's format, alpha included; an encoder -> its pix_fmt
    info = VideoInfo(width=64, height=36, bit_depth=10, pix_fmt="yuva444p10le", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec=""), "look.cube", info, python_bin="python")
    assert cmd[cmd.index("--pix-fmt") + 1] == "yuva444p10le" and "--out-pix-fmt" not in cmd
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("yuva444p10le", "yuva444p10le")
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="prores_ks", pix_fmt="yuva444p10le"), "look.cube", info,
                         python_bin="python")
    assert cmd[cmd.index("--out-pix-fmt") + 1] == "yuva444p10le"
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("yuva444p10le", "yuva444p10le")
    rgb = VideoInfo(width=64, height=36, bit_depth=10, pix_fmt="gbrap10le", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libvpx-vp9", pix_fmt="yuva420p"), "look.cube", rgb,
                         python_bin="python")
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("gbrap10le", "yuva420p")
    with pytest.raises(ValueError, match="needs a resolved output pixel format"):
        engine_command(Path("-"), Path("-"), ProcessingParams(video_codec=""), "look.cube", rgb, python_bin="python")


def test_pipe_stage_commands_carry_the_names():
    from lut_renderer_amd.pipe import engine_stage_commands
    info = VideoInfo(width=64, height=36, bit_depth=8, pix_fmt="yuva420p", fps=25.0)
    stages = engine_stage_commands(Path("in.webm"), Path("out.webm"), ProcessingParams(video_codec="libvpx-vp9", pix_fmt="yuva420p"),
                                   "look.cube", info)
    assert stages.decoder[stages.decoder.index("-pix_fmt") + 1] == "yuva420p"
    assert stages.engine[stages.engine.index("--pix-fmt") + 1] == "yuva420p"
    assert stages.engine[stages.engine.index("--out-pix-fmt") + 1] == "yuva420p"
    assert stages.encoder[stages.encoder.index("-f") + 3] == "yuva420p"      # -f rawvideo -pix_fmt <the engine's output>


# ------------------------------------------------------------------ refusals
def test_rejections_before_any_gpu_work():
    import torch
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.engine import LutEngine, check_container_options, refuse_alpha_resize
    from lut_renderer_amd.stream import HostPipeline
    assert check_container_options("yuva420p", None) is None and check_container_options("yuv420p", "yuva444p16le") is None
    # alpha with a container side
    for src, out, noun in (("yuva420p", "nv12", "semi-planar"), ("nv12", "yuva420p", "semi-planar"), ("yuva422p", "uyvy422", "packed 4:2:2"),
                           ("y210le", "yuva422p10le", "packed 4:2:2"), ("yuva422p10le", "v210", "v210"), ("v210", "yuva422p10le", "v210")):
        with pytest.raises(ValueError, match=f"alpha is carried between planar sides only, not with a {noun} side"):
            check_container_options(src, out)
        with pytest.raises(ValueError, match="alpha is carried between planar sides only"):
            _plan(src, out)
        with pytest.raises(ValueError, match="alpha is carried between planar sides only"):
            LutEngine.apply_yuv(object(), [], pix_fmt=src, out_pix_fmt=out)
    # a resize into an alpha-carrying output; an alpha source with an output without alpha passes the check
    refuse_alpha_resize("yuv420p", (4, 4))
    refuse_alpha_resize("yuva420p", None)
    refuse_alpha_resize("nv12", (4, 4))
    planes = [torch.zeros((6, 8), dtype=torch.uint8), torch.zeros((3, 4), dtype=torch.uint8), torch.zeros((3, 4), dtype=torch.uint8),
              torch.zeros((6, 8), dtype=torch.uint8)]
    for kw in (dict(pix_fmt="yuva420p"), dict(pix_fmt="yuva420p", out_pix_fmt="yuva444p10le"), dict(pix_fmt="yuv420p", out_pix_fmt="yuva420p")):
        src = planes[:3] if kw["pix_fmt"] == "yuv420p" else planes
        with pytest.raises(ValueError, match="not supported with an alpha-carrying output"):
            LutEngine.apply_yuv(object(), src, out_size=(4, 4), **kw)
        with pytest.raises(ValueError, match="not supported with an alpha-carrying output"):
            apply_lut(src, cube=None, resolution="4x4", engine=object(), **kw)
        with pytest.raises(ValueError, match="not supported with an alpha-carrying output"):
            HostPipeline(object(), kw["pix_fmt"], 8, 6, out_pix_fmt=kw.get("out_pix_fmt"), out_size=(4, 4))
    with pytest.raises(ValueError, match="not supported with an alpha-carrying output"):
        LutEngine.apply_rgb_to_yuv(object(), torch.zeros((6, 8, 4), dtype=torch.uint8), pix_fmt="rgba", out_pix_fmt="yuva420p", out_size=(4, 4))
    with pytest.raises(ValueError, match="not supported with an alpha-carrying output"):
        LutEngine.apply_rgb(object(), planes[:1] * 4, depth=8, out_size=(4, 4))
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    for extra, what in ((["--pix-fmt", "yuva420p", "--out-size", "32x18"], "alpha-carrying output"),
                        (["--pix-fmt", "yuv420p", "--out-pix-fmt", "yuva420p", "--out-size", "32x18"], "alpha-carrying output"),
                        (["--pix-fmt", "yuva420p", "--out-pix-fmt", "nv12"], "planar sides only"),
                        (["--pix-fmt", "yuva420p10le", "--out-pix-fmt", "p010le"], "planar sides only"),
                        (["--pix-fmt", "yuva422p10le", "--out-pix-fmt", "v210"], "planar sides only"),
                        (["--pix-fmt", "yuva420p", "--out-pix-fmt", "gbrap"], "RGB out_pix_fmt"),
                        (["--pix-fmt", "gbrap"], "RGB source with a YUV out_pix_fmt"),
                        (["--pix-fmt", "yuva440p"], "unsupported pixel format"),
                        (["--pix-fmt", "yuva420p", "--chroma-loc", "left", "--out-pix-fmt", "yuva444p"], "chroma_loc")):
        with pytest.raises(ValueError, match=what):
            plan_from_args(build_parser().parse_args(base + extra))
    plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuva420p", "--out-pix-fmt", "yuv420p", "--out-size", "32x18"]))
    # the options of the colour planes are checked under their three-plane names, ahead of any engine
    with pytest.raises(ValueError, match="chroma_loc"):
        LutEngine.apply_yuv(object(), planes, pix_fmt="yuva420p", out_pix_fmt="yuva444p", chroma_loc="left")
    with pytest.raises(ValueError, match="error-diffusion dither is not defined with sited"):
        LutEngine.apply_yuv(object(), planes, pix_fmt="yuva420p", chroma_loc="left", dither="error_diffusion")
    # the number of planes: four for an alpha name, and the old message for a three-plane one
    with pytest.raises(ValueError, match="'yuva420p' takes four planes"):
        LutEngine.apply_yuv(object(), planes[:3], pix_fmt="yuva420p")
    with pytest.raises(ValueError, match="expected three planes"):
        LutEngine.apply_yuv_dual(object(), planes, pix_fmt="yuv420p", out2_pix_fmt="yuva420p")
    with pytest.raises(ValueError, match="'yuva420p' takes four planes"):
        LutEngine.apply_yuv_dual(object(), planes[:3], pix_fmt="yuva420p", out2_pix_fmt="yuv420p")
    bad = planes[:3] + [torch.zeros((3, 4), dtype=torch.uint8)]
    with pytest.raises(ValueError, match=r"source plane 3 is \(3, 4\), 'yuva420p' at 8x6 needs \(6, 8\)"):
        LutEngine.apply_yuv(object(), bad, pix_fmt="yuva420p", out_pix_fmt="yuv420p")      # dropped, but still checked
    with pytest.raises(ValueError, match="source plane 3: 'yuva420p10le' takes 16-bit"):
        LutEngine.apply_yuv(object(), [t.to(torch.int16) for t in planes[:3]] + planes[3:], pix_fmt="yuva420p10le")
    with pytest.raises(ValueError, match="a second output"):
        LutEngine.apply_yuv_dual(object(), planes, pix_fmt="yuva420p", out2_pix_fmt="yuv420p", dither="blue_noise")


def test_alpha_layouts_refused_before_any_gpu_work():
    """An alpha source that is not dense along the row, and alpha planes that overlap other than in place, are refused before the
    colour pass is launched: nothing is written."""
    import torch
    from lut_renderer_amd.engine import LutEngine, _check_alpha_overlap
    h, w = 6, 8
    y, cb, cr = (torch.zeros(s, dtype=torch.int16) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2)))
    dst = [torch.zeros_like(t) for t in (y, cb, cr, y)]
    img = torch.zeros((h, w, 4), dtype=torch.int16)
    views = {"the A of a packed image": img[..., 3], "a constant made with expand": torch.tensor(1023, dtype=torch.int16).expand(h, w),
             "every second column": torch.zeros((h, 2 * w), dtype=torch.int16)[:, ::2]}
    for what, a in views.items():
        assert tuple(a.shape) == (h, w) and a.stride(-1) != 1, what
        with pytest.raises(ValueError, match="planes must be dense along the row"):
            LutEngine.apply_yuv(object(), [y, cb, cr, a], dst, pix_fmt="yuva420p10le")
        with pytest.raises(ValueError, match="planes must be dense along the row"):
            LutEngine.apply_yuv(object(), [y, cb, cr, a], dst[:3], pix_fmt="yuva420p10le", out_pix_fmt="yuv420p10le")
        with pytest.raises(ValueError, match="planes must be dense along the row"):
            LutEngine.apply_yuv_dual(object(), [y, cb, cr, a], dst, dst[:3], pix_fmt="yuva420p10le", out2_pix_fmt="yuv420p10le")
        with pytest.raises(ValueError, match="planes must be dense along the row"):
            LutEngine.apply_rgb(object(), [y, y.clone(), y.clone(), a], [torch.zeros_like(y) for _ in range(4)], depth=10)
        with pytest.raises(ValueError, match="planes must be dense along the row"):
            LutEngine._alpha_plane(object(), a, dst[3], 10, 10, w, h, 0, None)
    fa = torch.zeros((h, 2 * w), dtype=torch.float32)[:, ::2]
    f = [torch.zeros((h, w), dtype=torch.float32) for _ in range(3)]
    from lut_renderer_amd.engine import _check_float_planes, parse_rgb_source
    with pytest.raises(ValueError, match="planes must be dense along the row"):
        _check_float_planes(f + [fa], parse_rgb_source("gbrapf32le"), w, h, "source")
    # overlap: the same plane at the same depth is the no-op; everything else is refused ahead of the colour pass
    buf = torch.zeros((h + 2, w), dtype=torch.int16)
    src = [y, cb, cr, buf[:h]]
    _check_alpha_overlap(src[3], 10, [dst[0], dst[1], dst[2], src[3]], 10)
    _check_alpha_overlap(None, 10, dst, 10)
    LutEngine_apply = LutEngine.apply_yuv
    for d, kw, what in (([dst[0], dst[1], dst[2], buf[2:]], dict(pix_fmt="yuva420p10le"), "the alpha destination"),
                        ([dst[0], dst[1], dst[2], buf[:h]], dict(pix_fmt="yuva420p10le", out_pix_fmt="yuva420p12le"), "the alpha destination"),
                        ([buf[1:h + 1], dst[1], dst[2], dst[3]], dict(pix_fmt="yuva420p10le"), "destination plane 0")):
        with pytest.raises(ValueError, match=f"the alpha source overlaps {what}"):
            LutEngine_apply(object(), src, d, **kw)
    with pytest.raises(ValueError, match="the alpha source overlaps the alpha destination"):
        LutEngine.apply_rgb(object(), [y, y.clone(), y.clone(), buf[:h]], [dst[0], dst[3], y.clone(), buf[2:]], depth=10)
    with pytest.raises(ValueError, match="the alpha source overlaps the alpha destination"):
        LutEngine.apply_yuv_dual(object(), src, dst, [dst[0].clone(), dst[1].clone(), dst[2].clone(), buf[2:]], pix_fmt="yuva420p10le",
                                 out2_pix_fmt="yuva420p10le")
    assert not buf.any() and not any(t.any() for t in dst)


# ------------------------------------------------------------------ C-ABI without a device
def test_abi_symbol_struct_and_null_context():
    lib = _native.load()
    assert "lutr_alpha_plane" in _native.SYMBOLS and hasattr(lib, "lutr_alpha_plane")
    header = (ROOT / "include" / "lutr.h").read_text()
    assert "int lutr_alpha_plane(lutr_ctx *ctx, const lutr_alpha_src *src, int dout, void *dst, ptrdiff_t dst_stride," in header
    assert C.sizeof(_native.AlphaSrc) == 40 and _native.AlphaSrc.data.offset == 8 and _native.AlphaSrc.step.offset == 32
    assert C.sizeof(_native.Planes) == 72                                   # lutr_planes stays three planes
    a = _native.AlphaSrc()
    assert lib.lutr_alpha_plane(None, C.byref(a), 10, None, 0, 0, 8, 6, 1, 0, 6) == _native.EINVAL
    assert b"null argument" in lib.lutr_last_error()


def test_alpha_plane_source_refusals_keep_their_words():
    """`_alpha_plane`'s checks of its source, in order: dense along the row, on the engine's device, as many frames as the
    destination (host only: an engine object without a context)."""
    import torch
    from lut_renderer_amd.engine import LutEngine
    eng = object.__new__(LutEngine)
    eng.device = torch.device("cpu")
    dst = torch.zeros((2, 6, 8), dtype=torch.int16)
    with pytest.raises(ValueError, match="^planes must be dense along the row$"):
        eng._alpha_plane(torch.zeros((2, 6, 16), dtype=torch.int16, device="meta")[..., ::2], dst, 10, 10, 8, 6, 0, None)
    with pytest.raises(ValueError, match="^planes must be torch tensors resident on the engine's GPU$"):
        eng._alpha_plane(torch.zeros((2, 6, 8), dtype=torch.int16, device="meta"), dst, 10, 10, 8, 6, 0, None)
    with pytest.raises(ValueError, match="^src and dst disagree on the number of frames$"):
        eng._alpha_plane(torch.zeros((6, 8), dtype=torch.int16), dst, 10, 10, 8, 6, 0, None)
    with pytest.raises(ValueError, match="^src and dst disagree on the number of frames$"):
        eng._alpha_plane(torch.zeros((3, 6, 8, 4), dtype=torch.uint8), dst, 8, 10, 8, 6, 0, None, 3)
    with pytest.raises(ValueError, match="^planes must be dense along the row and resident on the engine's GPU$"):
        eng._alpha_plane(None, torch.zeros((2, 6, 8), dtype=torch.int16, device="meta"), 10, 10, 8, 6, 0, None)
