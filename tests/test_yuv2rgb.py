"""YUV sources with an RGB output without a GPU: the host-only constants against the reference of
tests/_yuv2rgb_twin.py, the grey anchors of every depth pair, the twin against the one-family oracle, and the plumbing from the
API down to the CLI's plan and the stream layouts."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
from tests import _yuv2rgb_twin as twin

LAYOUTS = twin.LAYOUTS
DEPTHS = (8, 10, 12, 16)
MATRICES = ("bt709", "smpte170m", "bt2020nc")


def _block(din, dl, m="bt709", rs="tv", ri=None, csx=1, csy=1):
    from lut_renderer_amd.engine import yuv_constants_yuv2rgb
    # fmt_out / matrix_out / range_out carry values that must be ignored
    return yuv_constants_yuv2rgb(fmt_in=_native.fmt_code(din, csx, csy), fmt_out=_native.fmt_code(9, 1, 0), lut_depth=dl,
                                 matrix_in=_native.MATRIX[m], matrix_out=2, range_src=_native.RANGE[rs],
                                 range_in=_native.RANGE[ri or rs], range_out=1)


def _consts_of(block, orc):
    """An oracle.binding.YuvConsts holding the floats of a 32-float block."""
    k = orc.YuvConsts()
    names = [f[0] for f in k._fields_]
    for i, name in enumerate(names):
        setattr(k, name, int(block[i]) if name == "pre" else float(block[i]))
    return k


# ------------------------------------------------------------------ constants
def test_constants_equal_the_twin_and_todays_input_entries(orc):
    from lut_renderer_amd.engine import yuv_constants
    for din in DEPTHS:
        for dl in DEPTHS:
            for m in MATRICES:
                for rng in ("tv", "pc"):
                    got = _block(din, dl, m, rng)
                    want = twin.consts(m, rng, rng, din, dl).as_block()
                    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (din, dl, m, rng)
                    assert got[20] == 0.0                      # no prologue: a depth change lives in the matrix constants
                    if din == dl:
                        today = yuv_constants(fmt_in=_native.fmt_code(din, 1, 1), fmt_out=_native.fmt_code(din, 1, 1), lut_depth=dl,
                                              matrix_in=_native.MATRIX[m], matrix_out=_native.MATRIX[m],
                                              range_src=_native.RANGE[rng], range_in=_native.RANGE[rng], range_out=0)
                        assert np.array_equal(got[:8].view(np.uint32), today[:8].view(np.uint32)), (din, m, rng)
                        # ... and the formula itself gives those entries at din == dl, bit for bit
                        f = twin.input_fields(m, rng, din, dl)
                        assert np.array_equal(np.array([f[n] for n in twin.INPUT_FIELDS], np.float32).view(np.uint32),
                                              today[:8].view(np.uint32)), (din, m, rng)
    # the full-range prologue: today's block for an output at (lut_depth, 4:4:4, matrix_in, range_in)
    for din in (8, 10):
        for ri in ("tv", "pc"):
            if ri == "pc":
                continue                                       # (range_src == range_in is the case above)
            got = _block(din, 8, "bt709", "pc", ri)
            want = twin.consts("bt709", "pc", ri, din, 8).as_block()
            assert got[20] == 1.0 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (din, ri)


def test_grey_anchors_of_every_depth_pair(orc):
    """Legal black gives code 0 and legal white gives Ml on every channel."""
    for din in (8, 9, 10, 12, 14, 16):
        for dl in DEPTHS:
            for m in MATRICES:
                for rng in ("tv", "pc"):
                    s, mi, ml = 1 << (din - 8), (1 << din) - 1, (1 << dl) - 1
                    black, white = (16 * s, 235 * s) if rng == "tv" else (0, mi)
                    dt = np.uint8 if din == 8 else np.uint16
                    k = _consts_of(_block(din, dl, m, rng), orc)
                    for y, code in ((black, 0), (white, ml)):
                        p = [np.full((2, 2), y, dt), np.full((1, 1), 128 * s, dt), np.full((1, 1), 128 * s, dt)]
                        r, g, b = yuv_to_rgb_codes(k, 1, 1, p)
                        assert (r == code).all() and (g == code).all() and (b == code).all(), (din, dl, m, rng, y, r[0, 0], g[0, 0])


def test_twin_on_a_444_frame_is_the_yuv_contract(orc, cube_dir):
    """For a 4:4:4 frame P at din == dl, stage 3 of the YUV contract on the twin's RGB of P is orc.apply_yuv on P."""
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for w, h in ((16, 8), (7, 5)):
        for d in (8, 10, 12):
            for mode in ("tetrahedral", "trilinear"):
                p = frames.uniform_yuv(w, h, d, 0, 0, k=d + w)
                k = orc.yuv_constants("bt709", "tv", "bt709", "tv", d, d, d, chroma_n=1)
                out = twin.apply(lut.table, lut.scale, mode, "gbrp" if d == 8 else f"gbrp{d}le", d, 0, 0, p)
                g, b, r = out
                got = rgb_codes_to_yuv(k, d, 0, 0, (r, g, b))
                want = orc.apply_yuv(lut.table, lut.scale, mode, k, d, d, d, 0, 0, p)
                assert all(np.array_equal(a, b_) for a, b_ in zip(got, want)), (w, h, d, mode)
    # the arrangement of a packed destination: the components at their indices, the fourth one opaque
    p = frames.uniform_yuv(6, 4, 10, 1, 1, k=3)
    g, b, r = twin.apply(lut.table, lut.scale, "tetrahedral", "gbrp16le", 10, 1, 1, p)
    img = twin.apply(lut.table, lut.scale, "tetrahedral", "rgba64le", 10, 1, 1, p)
    assert img.shape == (4, 6, 4) and np.array_equal(img[..., 0], r) and np.array_equal(img[..., 2], b) and (img[..., 3] == 65535).all()
    img = twin.apply(lut.table, lut.scale, "tetrahedral", "abgr", 10, 1, 1, p)
    assert img.dtype == np.uint8 and (img[..., 0] == 255).all()
    assert np.array_equal(img[..., 3], twin.apply(lut.table, lut.scale, "tetrahedral", "gbrp", 10, 1, 1, p)[2])


def test_abi_symbols_and_einval_without_a_gpu():
    lib = _native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    for sym in ("lutr_apply_yuv_to_rgb", "lutr_yuv_constants_yuv2rgb"):
        assert f" T {sym}\n" in nm and sym in _native.SYMBOLS
    assert lib.lutr_yuv_constants_yuv2rgb(None, (C.c_float * 32)()) == _native.EINVAL
    with pytest.raises(_native.LutrError) as e:            # a 4:4:0 source
        _block(10, 10, csx=0, csy=1)
    assert e.value.code == _native.EINVAL
    for din, dl in ((7, 8), (10, 17), (10, 7)):            # depths outside 8..16
        with pytest.raises(_native.LutrError):
            _block(din, dl)
    with pytest.raises(_native.LutrError, match="full-range"):     # a range prologue is a pc source's
        _block(10, 10, rs="tv", ri="pc")
    assert lib.lutr_apply_yuv_to_rgb(None, None, 2, 0, 16, 16, 1, None, None, None, 0, 16) == _native.EINVAL


# ------------------------------------------------------------------ host plumbing
def _plan(pix_fmt, out_pix_fmt=None, rgb_out=None, **info_kw):
    from lut_renderer_amd.api import engine_call_for
    from lut_renderer_amd.plan import resolve_lut_plan
    info = VideoInfo(width=64, height=36, pix_fmt=pix_fmt, **info_kw)
    plan = resolve_lut_plan(ProcessingParams(), "look.cube", info)
    return plan, engine_call_for(plan, pix_fmt, out_pix_fmt, rgb_out=rgb_out)


def test_engine_call_for_rgb_out():
    from lut_renderer_amd.api import is_float_out_call, is_rgb_call, is_rgb_out_call
    for src, out in (("yuv420p10le", "gbrp10le"), ("yuv420p10le", "rgb48le"), ("yuv422p", "rgb24"), ("yuva444p10le", "gbrap10le"),
                     ("yuv420p", "bgra")):
        plan, kw = _plan(src, rgb_out=out, colorspace="bt709")
        assert is_rgb_out_call(kw) and not is_rgb_call(kw) and not is_float_out_call(kw) and not plan.prologue
        assert kw == dict(pix_fmt=src, out_pix_fmt=out, interp="tetrahedral", matrix_in="bt709", range_src="tv", range_in="tv")
    _, kw = _plan("yuv420p", rgb_out="rgb24")
    assert kw["matrix_in"] == "smpte170m"                  # unforced: swscale's default for untagged frames
    _, kw = _plan("yuvj420p", rgb_out="rgb24")
    assert kw["pix_fmt"] == "yuv420p"
    # a source flagged full range: the prologue lands at 8 bit, so an 8-bit rgb_out only
    plan, kw = _plan("yuv420p10le", rgb_out="rgb24", color_range="pc")
    assert plan.prologue and (kw["range_src"], kw["range_in"]) == ("pc", plan.prologue_out_range)
    with pytest.raises(ValueError, match="8-bit rgb_out"):
        _plan("yuv420p10le", rgb_out="gbrp10le", color_range="pc")
    # the other calls are what they were
    for src, out in (("yuv420p10le", None), ("rgb24", "yuv420p"), ("yuv420p", "yuv444p")):
        _, kw = _plan(src, out)
        assert not is_rgb_out_call(kw)
    with pytest.raises(ValueError, match="mutually exclusive"):
        _plan("yuv420p", "yuv444p", rgb_out="rgb24")
    with pytest.raises(ValueError, match="RGB out_pix_fmt"):               # the old refusal stands, word for word
        _plan("yuv420p", "rgb24")


def test_refusals_name_what_is_not_taken():
    from lut_renderer_amd.formats import PixFmt, RgbSource, check_yuv2rgb_options
    fin, fout = check_yuv2rgb_options("yuv420p10le", "gbrp10le", chroma_loc=None, dither="none", alpha_mode="straight", lut2=False)
    assert isinstance(fin, PixFmt) and isinstance(fout, PixFmt) and (fout.family, fout.depth, fout.nplanes) == ("gbr", 10, 3)
    fin, fout = check_yuv2rgb_options("yuva420p", "rgb24")
    assert fin.alpha and isinstance(fout, RgbSource) and fout.ncomp == 3
    assert check_yuv2rgb_options("yuva444p12le", "gbrap12le")[1].nplanes == 4
    for kw, word in ((dict(chroma_loc="left"), "chroma_loc"), (dict(dither="error_diffusion"), "dither"),
                     (dict(dither="blue_noise"), "dither"), (dict(engine_dither="blue_noise"), "dither"),
                     (dict(out_size=(32, 18)), "out_size"), (dict(alpha_mode="premultiplied"), "premultiplied"),
                     (dict(cdl=object()), "cdl"), (dict(lut1d=object()), "lut1d"), (dict(stages=("lut3d",)), "stages"),
                     (dict(strength=0.5), "strength"), (dict(strength=np.array([0.5, 1.0])), "strength"),
                     (dict(matte=object()), "matte"), (dict(out2_pix_fmt="yuv420p"), "second output"),
                     (dict(cube2="b.cube"), "cube2"), (dict(lut2=True), "second LUT")):
        with pytest.raises(ValueError, match=word):
            check_yuv2rgb_options("yuv420p10le", "gbrp10le", **kw)
    with pytest.raises(TypeError, match="unexpected keyword"):
        check_yuv2rgb_options("yuv420p10le", "gbrp10le", colour="red")
    for src, word in (("nv12", "semi-planar"), ("p010le", "semi-planar"), ("uyvy422", "packed 4:2:2"), ("y210le", "packed 4:2:2"),
                      ("v210", "v210"), ("rgb24", "RGB format"), ("gbrp10le", "RGB format")):
        with pytest.raises(ValueError, match=word):
            check_yuv2rgb_options(src, "rgb24")
    for out, word in (("gbrpf32le", "float"), ("yuv444p", "not an RGB output"), ("rgb565", "not an RGB output"), (None, "not an RGB")):
        with pytest.raises(ValueError, match=word):
            check_yuv2rgb_options("yuv420p", out)
    for out in ("rgba", "bgra", "argb", "abgr", "rgba64le"):
        with pytest.raises(ValueError, match="follow-up"):
            check_yuv2rgb_options("yuva420p10le", out)


def test_plan_from_args_rgb_out():
    from lut_renderer_amd.api import is_rgb_out_call
    from lut_renderer_amd.cli import build_parser, plan_from_args
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    for src, out in (("yuv420p10le", "gbrp10le"), ("yuv420p", "rgb24"), ("yuv422p10le", "rgba64le"), ("yuva420p", "gbrap")):
        plan, kw, w, h = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", src, "--rgb-out", out, "--colorspace", "bt709"]))
        assert is_rgb_out_call(kw) and (kw["pix_fmt"], kw["out_pix_fmt"], kw["matrix_in"], w, h) == (src, out, "bt709", 64, 36)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuv420p10le", "--rgb-out", "rgb24", "--color-range", "pc"]))
    assert (kw["range_src"], kw["range_in"]) == ("pc", "tv")
    for extra, word in ((["--out-pix-fmt", "yuv444p"], "mutually exclusive"), (["--chroma-loc", "left"], "chroma_loc"),
                        (["--zscale-dither", "error_diffusion"], "dither"), (["--engine-dither", "blue_noise"], "dither"),
                        (["--out-size", "32x18"], "out_size"), (["--alpha-mode", "premultiplied"], "premultiplied"),
                        (["--cube2", "b.cube"], "cube2"), (["--lut1d", "c.cube"], "lut1d"), (["--stages", "lut3d"], "stages"),
                        (["--strength", "0.5"], "strength"), (["--strength-keys", "0:0,4:1"], "strength"),
                        (["--matte", "m.gray"], "matte"), (["--cdl-sat", "0.9"], "cdl"),
                        (["--second-output", "c.yuv", "--second-pix-fmt", "yuv420p"], "second output")):
        src = "yuva420p" if "premultiplied" in extra else "yuv420p"
        with pytest.raises(ValueError, match=word):
            plan_from_args(build_parser().parse_args(base + ["--pix-fmt", src, "--rgb-out", "rgb24"] + extra))
    with pytest.raises(ValueError, match="semi-planar"):
        plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "nv12", "--rgb-out", "rgb24"]))
    with pytest.raises(ValueError, match="8-bit rgb_out"):
        plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuv420p", "--rgb-out", "rgb48le", "--color-range", "pc"]))
    # the existing refusal of an RGB --out-pix-fmt stands
    with pytest.raises(ValueError, match="RGB out_pix_fmt"):
        plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuv420p", "--out-pix-fmt", "rgb24"]))


def test_output_layouts_count_bytes():
    import torch
    from lut_renderer_amd.stream import FrameLayout, PackedFrameLayout, output_layout
    lay = output_layout("gbrp10le", 65, 33)
    assert isinstance(lay, FrameLayout) and lay.frame_bytes == 3 * 33 * 65 * 2 and lay.plane_shapes == [(33, 65)] * 3
    assert output_layout("gbrap", 65, 33).frame_bytes == 4 * 33 * 65
    for name, bpp in (("rgb24", 3), ("bgr24", 3), ("rgba", 4), ("rgb48le", 6), ("rgba64le", 8)):
        lay = output_layout(name, 65, 33)
        assert isinstance(lay, PackedFrameLayout) and lay.frame_bytes == 33 * 65 * bpp and lay.fmt.name == name
    v = output_layout("rgba64le", 3, 4).image_view(torch.zeros(2 * 4 * 3 * 8, dtype=torch.uint8), 2)
    assert tuple(v.shape) == (2, 4, 3, 4) and v.dtype == torch.int16
    for name in ("yuv420p", "gbrpf32le", "nv12"):
        with pytest.raises(ValueError):
            output_layout(name, 64, 36)
