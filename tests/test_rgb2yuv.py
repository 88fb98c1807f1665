"""RGB sources with a YUV output without a GPU: the reference composition of tests/_rgb2yuv_twin.py against the
one-family oracle and known answers, the host-only constants, and the plumbing from the API down to the argv layer."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.engine import yuv_constants_rgb2yuv, yuv_constants_xsub
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from oracle.lut3d_numpy import yuv_to_rgb_codes
from tests import _rgb2yuv_twin as twin
from tests import _xsub_twin as xs

LAYOUTS = twin.LAYOUTS
OUT_KEYS = ("cyr", "cyg", "cyb", "yob", "cbr", "cbg", "cbb", "crr", "crg", "crb", "cob", "max_o")


def _gbrp(depth):
    return "gbrp" if depth == 8 else f"gbrp{depth}le"


# ------------------------------------------------------------------ the twin against the one-family oracle
def test_twin_on_the_rgb_of_a_444_frame_is_the_yuv_contract(orc, cube_dir):
    """For a 4:4:4 YUV frame P, the RGB path applied to stage 1's integer RGB of P is the YUV path 444 -> out applied to P."""
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for w, h in ((16, 8), (7, 5)):
        for din, dout in ((8, 8), (10, 10), (12, 12), (10, 8)):
            p = frames.uniform_yuv(w, h, din, 0, 0, k=din + w)
            for lay, (ocsx, ocsy) in LAYOUTS.items():
                k = xs.consts("bt709", "tv", "bt709", "tv", din, din, dout, ocsx, ocsy)
                r, g, b = yuv_to_rgb_codes(k, 0, 0, p)
                dt = np.uint8 if din == 8 else np.uint16
                src = (g.astype(dt), b.astype(dt), r.astype(dt))
                kr = twin.consts("bt709", "tv", din, dout, ocsx, ocsy)
                got = twin.apply(lut.table, lut.scale, "tetrahedral", kr, _gbrp(din), dout, ocsx, ocsy, src)
                want = xs.apply(lut.table, lut.scale, "tetrahedral", k, din, dout, 0, 0, ocsx, ocsy, p)
                assert all(np.array_equal(a, b_) for a, b_ in zip(got, want)), (w, h, din, dout, lay)


def _flat(pix_fmt, v, w=7, h=5):
    """A w x h source of one colour v = (r, g, b) in `pix_fmt`."""
    if pix_fmt in twin.PACKED:
        bits, nc, ro, go, bo = twin.PACKED[pix_fmt]
        img = np.zeros((h, w, nc), np.uint8 if bits == 8 else np.uint16)
        img[..., ro], img[..., go], img[..., bo] = v
        return img
    dt = np.uint8 if twin.source_depth(pix_fmt) == 8 else np.uint16
    return [np.full((h, w), v[i], dt) for i in (1, 2, 0)]


def test_known_answers_black_white_grey(orc):
    ident = cube.identity_lattice(17)
    one = np.ones(3, np.float32)
    for pix_fmt in ("gbrp", "rgb24", "gbrp10le"):
        dl = twin.source_depth(pix_fmt)
        ml = (1 << dl) - 1
        for dout, rng in ((8, "tv"), (10, "tv"), (8, "pc")):
            so, mo = 1 << (dout - 8), (1 << dout) - 1
            for name, code in (("black", 0), ("white", ml), ("grey", (ml + 1) // 2)):
                # the LUT's own answer for the grey pixel (an identity lattice may truncate one code down), then the textbook
                # equation in double, rounded half up
                v = orc.apply_pixel(ident, one, dl, "tetrahedral", (code,) * 3)[0]
                y = int(16 * so + 219 * so * v / ml + 0.5) if rng == "tv" else int(mo * v / ml + 0.5)
                if name != "grey":
                    assert v == code and y == {("black", "tv"): 16 * so, ("white", "tv"): 235 * so, ("black", "pc"): 0,
                                               ("white", "pc"): mo}[(name, rng)]
                for lay, (ocsx, ocsy) in LAYOUTS.items():
                    k = twin.consts("bt709", rng, dl, dout, ocsx, ocsy)
                    out = twin.apply(ident, one, "tetrahedral", k, pix_fmt, dout, ocsx, ocsy, _flat(pix_fmt, (code,) * 3))
                    assert out[0].shape == (5, 7) and out[1].shape == frames.chroma_shape(7, 5, ocsx, ocsy)
                    assert (out[0] == y).all() and (out[1] == 128 * so).all() and (out[2] == 128 * so).all(), \
                        (pix_fmt, dout, rng, name, lay, out[0][0, 0], y)


def test_known_answers_colour_bars(orc):
    """100 % bars, 8-bit BT.709 studio range: the codes tests/test_thirdparty_crosscheck.py uses (tabulated to whole codes from
    three-decimal equations, hence its one-code allowance, kept here)."""
    ident = cube.identity_lattice(33)
    one = np.ones(3, np.float32)
    bars = {"white": ((255, 255, 255), (235, 128, 128)), "black": ((0, 0, 0), (16, 128, 128)),
            "red": ((255, 0, 0), (63, 102, 240)), "green": ((0, 255, 0), (173, 42, 26)), "blue": ((0, 0, 255), (32, 240, 118)),
            "yellow": ((255, 255, 0), (219, 16, 138)), "cyan": ((0, 255, 255), (188, 154, 16)),
            "magenta": ((255, 0, 255), (78, 214, 230))}
    for pix_fmt in ("gbrp", "rgb24", "bgra"):
        for lay, (ocsx, ocsy) in LAYOUTS.items():
            k = twin.consts("bt709", "tv", 8, 8, ocsx, ocsy)
            for name, (rgb, yuv) in bars.items():
                out = twin.apply(ident, one, "trilinear", k, pix_fmt, 8, ocsx, ocsy, _flat(pix_fmt, rgb, 4, 4))
                got = tuple(int(p[0, 0]) for p in out)
                assert all(abs(a - b) <= 1 for a, b in zip(got, yuv)), (pix_fmt, lay, name, got)


# ------------------------------------------------------------------ constants
def test_constants_against_the_oracle_and_the_xsub_block(orc):
    for lay, (ocsx, ocsy) in LAYOUTS.items():
        for dl, dout in ((8, 8), (10, 10), (10, 8), (16, 10), (16, 8), (8, 10), (12, 12)):
            for m in ("bt709", "smpte170m", "bt2020nc"):
                for rng in ("tv", "pc"):
                    # matrix_in / range_src / range_in / fmt_in carry values that must be ignored
                    got = yuv_constants_rgb2yuv(fmt_in=_native.fmt_code(9, 1, 1), fmt_out=_native.fmt_code(dout, ocsx, ocsy),
                                                lut_depth=dl, matrix_in=2, matrix_out=_native.MATRIX[m], range_src=1, range_in=0,
                                                range_out=_native.RANGE[rng])
                    k = twin.consts(m, rng, dl, dout, ocsx, ocsy)
                    assert np.array_equal(got.view(np.uint32), k.as_block().view(np.uint32)), (lay, dl, dout, m, rng)
                    x = yuv_constants_xsub(fmt_in=_native.fmt_code(dl, 0, 0), fmt_out=_native.fmt_code(dout, ocsx, ocsy),
                                           lut_depth=dl, matrix_in=0, matrix_out=_native.MATRIX[m], range_src=0, range_in=0,
                                           range_out=_native.RANGE[rng])
                    names = [f[0] for f in type(k)._fields_]
                    for key in OUT_KEYS:
                        i = names.index(key)
                        assert got.view(np.uint32)[i] == x.view(np.uint32)[i], (key, lay, dl, dout, m, rng)


def test_abi_symbols_and_einval_without_a_gpu():
    lib = _native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    for sym in ("lutr_apply_rgb_to_yuv", "lutr_yuv_constants_rgb2yuv"):
        assert f" T {sym}\n" in nm and sym in _native.SYMBOLS
    assert lib.lutr_yuv_constants_rgb2yuv(None, (C.c_float * 32)()) == _native.EINVAL
    with pytest.raises(_native.LutrError) as e:            # 4:4:0 output
        yuv_constants_rgb2yuv(fmt_out=_native.fmt_code(10, 0, 1), lut_depth=10)
    assert e.value.code == _native.EINVAL
    with pytest.raises(_native.LutrError):                 # depth outside 8..16
        yuv_constants_rgb2yuv(fmt_out=_native.fmt_code(10, 1, 1), lut_depth=7)
    assert lib.lutr_apply_rgb_to_yuv(None, None, 2, 0, 0, 16, 16, 1, None, None, None, 0, 16) == _native.EINVAL
    assert lib.lutr_apply_rgb_to_yuv(None, None, 2, 7, 0, 16, 16, 1, None, None, None, 0, 16) == _native.EINVAL
    assert b"dither" in lib.lutr_last_error()


# ------------------------------------------------------------------ host plumbing
def _plan(pix_fmt, out_pix_fmt, **info_kw):
    from lut_renderer_amd.api import engine_call_for
    from lut_renderer_amd.plan import resolve_lut_plan
    info = VideoInfo(width=64, height=36, pix_fmt=pix_fmt, **info_kw)
    plan = resolve_lut_plan(ProcessingParams(), "look.cube", info)
    return plan, engine_call_for(plan, pix_fmt, out_pix_fmt)


def test_engine_call_for_rgb_sources():
    from lut_renderer_amd.api import is_rgb_call
    for src, out in (("gbrp10le", "yuv420p10le"), ("rgb24", "yuv420p"), ("rgb48le", "yuv422p10le")):
        plan, kw = _plan(src, out, colorspace="bt709")
        assert is_rgb_call(kw) and not plan.prologue
        assert kw == dict(pix_fmt=src, out_pix_fmt=out, interp="tetrahedral", matrix_out="bt709", range_out="tv")
    _, kw = _plan("rgb24", "yuv420p")
    assert kw["matrix_out"] == "smpte170m"                 # unforced: swscale's default for untagged frames
    # a source flagged full range: the reference's scale / format pair ahead of lut3d -> the two-stage plan
    plan, kw = _plan("rgb24", "yuv420p10le", color_range="pc")
    assert plan.prologue and (plan.intermediate_pix_fmt, plan.prologue_out_range) == ("yuv420p", "tv")
    assert kw["intermediate_pix_fmt"] == "yuv420p" and kw["prologue_out_range"] == "tv" and kw["out_pix_fmt"] == "yuv420p10le"
    _, kw = _plan("yuv420p10le", None)
    assert not is_rgb_call(kw) and kw["out_pix_fmt"] == "yuv420p10le"


def test_rejections_before_any_gpu_work():
    with pytest.raises(ValueError, match="apply_rgb"):     # no output format: today's pointer at apply_rgb / apply_packed
        _plan("gbrp10le", None)
    with pytest.raises(ValueError, match="apply_packed"):
        _plan("rgb24", None)
    with pytest.raises(ValueError, match="planar YUV"):    # RGB in, RGB out is apply_rgb / apply_packed
        _plan("rgb24", "gbrp")
    with pytest.raises(ValueError, match="RGB out_pix_fmt"):   # YUV in, RGB out stays undefined
        _plan("yuv420p", "rgb24")
    from lut_renderer_amd.cli import build_parser, plan_from_args
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    with pytest.raises(ValueError, match="chroma"):
        plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "rgb24", "--out-pix-fmt", "yuv420p", "--chroma-loc", "left"]))
    with pytest.raises(ValueError):
        plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "rgb24"]))


def test_plan_from_args_for_rgb_sources():
    from lut_renderer_amd.cli import build_parser, plan_from_args
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    for src, out in (("gbrp10le", "yuv420p10le"), ("rgb24", "yuv420p"), ("rgb48le", "yuv422p10le")):
        plan, kw, w, h = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", src, "--out-pix-fmt", out]))
        assert (kw["pix_fmt"], kw["out_pix_fmt"], w, h) == (src, out, 64, 36) and "intermediate_pix_fmt" not in kw
    _, kw, _, _ = plan_from_args(build_parser().parse_args(
        base + ["--pix-fmt", "rgb24", "--out-pix-fmt", "yuv420p", "--color-range", "pc", "--zscale-dither", "error_diffusion"]))
    assert kw["intermediate_pix_fmt"] == "yuv420p" and kw["prologue_out_range"] == "tv" and kw["dither"] == "error_diffusion"


def test_input_layouts_count_packed_bytes():
    from lut_renderer_amd.stream import FrameLayout, PackedFrameLayout, input_layout
    for name, bpp in (("rgb24", 3), ("bgr24", 3), ("rgba", 4), ("argb", 4), ("rgb48le", 6), ("rgba64le", 8)):
        lay = input_layout(name, 65, 33)
        assert isinstance(lay, PackedFrameLayout) and lay.frame_bytes == 33 * 65 * bpp and lay.fmt.name == name
    lay = input_layout("gbrp10le", 65, 33)
    assert isinstance(lay, FrameLayout) and lay.frame_bytes == 3 * 33 * 65 * 2
    assert input_layout("yuv420p", 65, 33).frame_bytes == 33 * 65 + 2 * 17 * 33
    import torch
    buf = torch.arange(2 * 4 * 3 * 3, dtype=torch.uint8)
    v = input_layout("rgb24", 3, 4).image_view(buf, 2)
    assert tuple(v.shape) == (2, 4, 3, 3) and int(v[1, 0, 0, 0]) == 36 and int(v[0, 1, 0, 2]) == 11


def test_argv_layer_for_rgb_sources():
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.pipe import engine_stage_commands
    info = VideoInfo(width=64, height=36, bit_depth=10, pix_fmt="gbrp10le", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx265"), Path("look.cube"), info, python_bin="python3")
    assert cmd[cmd.index("--pix-fmt") + 1] == "gbrp10le" and cmd[cmd.index("--out-pix-fmt") + 1] == "yuv420p10le"
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("gbrp10le", "yuv420p10le")
    info8 = VideoInfo(width=64, height=36, bit_depth=8, pix_fmt="rgb24", color_range="pc", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx264", bit_depth_policy="force_8bit"),
                         Path("look.cube"), info8, python_bin="python3")
    assert cmd[cmd.index("--out-pix-fmt") + 1] == "yuv420p" and cmd[cmd.index("--color-range") + 1] == "pc"
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert kw["intermediate_pix_fmt"] == "yuv420p" and kw["out_pix_fmt"] == "yuv420p"
    c = engine_stage_commands(Path("in.mov"), Path("out.mp4"), ProcessingParams(video_codec="libx265"), Path("look.cube"), info,
                              python_bin="python3")
    assert c.decoder[c.decoder.index("-pix_fmt") + 1] == "gbrp10le"
    assert c.engine[c.engine.index("--out-pix-fmt") + 1] == "yuv420p10le"
    assert c.encoder[c.encoder.index("-pix_fmt") + 1] == "yuv420p10le"
    # an RGB source the engine process could only fail on: refused where the argv is rendered
    with pytest.raises(ValueError, match="output pixel format"):
        engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx264"), Path("look.cube"),
                       VideoInfo(width=64, height=36, bit_depth=8, pix_fmt="rgb24"))
    with pytest.raises(ValueError, match="chroma"):
        engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx265"), Path("look.cube"), info, chroma_loc="left")
    with pytest.raises(ValueError, match="chroma"):
        engine_stage_commands(Path("in.mov"), Path("out.mp4"), ProcessingParams(video_codec="libx265"), Path("look.cube"), info,
                              chroma_loc="center")
