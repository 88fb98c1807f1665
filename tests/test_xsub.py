"""Chroma subsampling change inside the fused YUV pass -- host side.

The reference (tests/_xsub_twin.py) pinned to the oracle's one-layout contract wherever the two must agree, the constant
block, the argument checks and the argv of the professional master stage.  GPU parity is tests/test_gpu_xsub.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.engine import yuv_constants, yuv_constants_xsub
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _xsub_twin as twin

LAYOUTS = twin.LAYOUTS
SIZES = ((24, 12), (17, 11))                 # even and odd width / height
DEPTHS = ((8, 8, 8), (10, 10, 10), (10, 10, 8), (12, 12, 12))


def _lut(cube_dir):
    return cube.read_lut(cube_dir / "log709_33.cube")


def _eq(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _k(din, dl, dout, ocsx, ocsy):
    return twin.consts("bt709", "tv", "bt709", "tv", din, dl, dout, ocsx, ocsy)


def test_equal_layouts_are_the_oracle(orc, cube_dir):
    lut = _lut(cube_dir)
    for lay, (csx, csy) in LAYOUTS.items():
        for w, h in SIZES:
            for din, dl, dout in DEPTHS:
                src = frames.natural_yuv(w, h, din, csx, csy, k=din + w)
                k = _k(din, dl, dout, csx, csy)
                for mode in ("tetrahedral", "prism"):
                    got = twin.apply(lut.table, lut.scale, mode, k, dl, dout, csx, csy, csx, csy, src)
                    want = orc.apply_yuv(lut.table, lut.scale, mode, k, din, dl, dout, csx, csy, src)
                    assert _eq(got, want), (lay, w, h, din, dout, mode)


def test_420_to_422_is_422_with_duplicated_chroma_rows(orc, cube_dir):
    lut = _lut(cube_dir)
    for w, h in SIZES:
        for din, dl, dout in DEPTHS:
            y, cb, cr = frames.natural_yuv(w, h, din, 1, 1, k=3)
            k = _k(din, dl, dout, 1, 0)
            got = twin.apply(lut.table, lut.scale, "trilinear", k, dl, dout, 1, 1, 1, 0, (y, cb, cr))
            dup = [y] + [np.repeat(c, 2, axis=0)[:h] for c in (cb, cr)]
            want = orc.apply_yuv(lut.table, lut.scale, "trilinear", k, din, dl, dout, 1, 0, dup)
            assert _eq(got, want), (w, h, din, dout)


def test_422_to_420_is_444_to_420_on_replicated_chroma(cube_dir):
    lut = _lut(cube_dir)
    for w, h in SIZES:
        y, cb, cr = frames.natural_yuv(w, h, 10, 1, 0, k=4)
        k = _k(10, 10, 10, 1, 1)
        got = twin.apply(lut.table, lut.scale, "tetrahedral", k, 10, 10, 1, 0, 1, 1, (y, cb, cr))
        rep = [y] + [np.repeat(c, 2, axis=1)[:, :w] for c in (cb, cr)]
        want = twin.apply(lut.table, lut.scale, "tetrahedral", k, 10, 10, 0, 0, 1, 1, rep)
        assert _eq(got, want), (w, h)
        assert got[1].shape == frames.chroma_shape(w, h, 1, 1)


def test_444_to_420_with_blockwise_constant_chroma_is_the_420_oracle(orc, cube_dir):
    lut = _lut(cube_dir)
    for w, h in SIZES:
        for din, dl, dout in DEPTHS:
            y, cb, cr = frames.natural_yuv(w, h, din, 1, 1, k=5)
            c444 = [np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)[:h, :w] for c in (cb, cr)]
            k = _k(din, dl, dout, 1, 1)
            got = twin.apply(lut.table, lut.scale, "nearest", k, dl, dout, 0, 0, 1, 1, [y] + c444)
            want = orc.apply_yuv(lut.table, lut.scale, "nearest", k, din, dl, dout, 1, 1, (y, cb, cr))
            assert _eq(got, want), (w, h, din, dout)


def test_dither_twin_without_error_is_the_rounded_twin(cube_dir):
    """The unquantised planes round (floor of x + 0.5) to exactly the quantised contract: pass 1 of the dither path is stage 3."""
    lut = _lut(cube_dir)
    src = frames.natural_yuv(17, 11, 10, 1, 1, k=6)
    k = _k(10, 10, 10, 1, 0)
    rgb = twin.lut_rgb(lut.table, lut.scale, "tetrahedral", k, 10, 1, 1, src)
    x = twin.unquantised(k, 1, 0, rgb)
    want = twin.apply(lut.table, lut.scale, "tetrahedral", k, 10, 10, 1, 1, 1, 0, src)
    for a, b in zip(x, want):
        assert np.array_equal(np.clip(np.floor(a.astype(np.float64) + 0.5), 0, 1023).astype(np.uint16), b)


def _params(din, dl, dout, a, b, rs="tv", mo=0):
    return dict(fmt_in=_native.fmt_code(din, *LAYOUTS[a]), fmt_out=_native.fmt_code(dout, *LAYOUTS[b]), lut_depth=dl,
                matrix_in=0, matrix_out=mo, range_src=_native.RANGE[rs], range_in=0, range_out=0)


def test_constants_are_the_oracle_at_the_output_block(orc):
    for a in LAYOUTS:
        for b in LAYOUTS:
            ocsx, ocsy = LAYOUTS[b]
            for din, dl, dout, rs in ((10, 10, 10, "tv"), (8, 8, 8, "tv"), (10, 10, 8, "tv"), (10, 8, 10, "pc"), (16, 16, 16, "tv")):
                kw = _params(din, dl, dout, a, b, rs, mo=2)
                k = orc.yuv_constants("bt709", "tv", "bt2020nc", "tv", din, dl, dout, chroma_n=1 << (ocsx + ocsy),
                                      prologue=rs == "pc")
                assert np.array_equal(yuv_constants_xsub(**kw).view(np.uint32), k.as_block().view(np.uint32)), (a, b, din, rs)
                if a == b:
                    assert np.array_equal(yuv_constants_xsub(**kw).view(np.uint32), yuv_constants(**kw).view(np.uint32))
                else:
                    with pytest.raises(_native.LutrError):          # the one-layout block keeps refusing a layout change
                        yuv_constants(**kw)


def test_440_and_bad_arguments_are_einval_without_a_gpu():
    lib = _native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    for sym in ("lutr_apply_yuv_xsub", "lutr_yuv_constants_xsub"):
        assert f" T {sym}\n" in nm and sym in _native.SYMBOLS
    ok = _params(10, 10, 10, "420", "422")
    for bad in (dict(fmt_in=_native.fmt_code(10, 0, 1)), dict(fmt_out=_native.fmt_code(10, 0, 1)),
                dict(lut_depth=7), dict(fmt_out=_native.fmt_code(17, 1, 0))):
        with pytest.raises(_native.LutrError) as e:
            yuv_constants_xsub(**{**ok, **bad})
        assert e.value.code == _native.EINVAL and e.value.message
    assert lib.lutr_yuv_constants_xsub(None, (C.c_float * 32)()) == _native.EINVAL
    assert lib.lutr_apply_yuv_xsub(None, None, 2, 0, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
    assert lib.lutr_apply_yuv_xsub(None, None, 2, 7, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
    assert b"dither" in lib.lutr_last_error()


def test_chroma_loc_with_a_layout_change_is_a_value_error_before_any_gpu_work(cube_dir):
    from lut_renderer_amd import api
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.engine import changes_subsampling, check_chroma_loc
    assert changes_subsampling("yuv420p10le", "yuv422p10le") and changes_subsampling("yuvj444p", "yuv420p")
    assert not changes_subsampling("yuv420p10le", "yuv420p") and not changes_subsampling("yuv422p", None)
    check_chroma_loc("left", "none", "yuv420p10le", "yuv420p")           # same layout: sited resampling is defined
    check_chroma_loc(None, "none", "yuv420p10le", "yuv444p10le")         # replicate: a layout change is defined
    with pytest.raises(ValueError, match="subsampling"):
        check_chroma_loc("left", "none", "yuv420p10le", "yuv422p10le")
    y, cb, cr = frames.natural_yuv(16, 8, 10, 1, 1)
    with pytest.raises(ValueError, match="subsampling"):
        api.apply_lut((y, cb, cr), cube=None, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", chroma_loc="center",
                      engine=object())
    args = build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", "yuv422p10le", "--out-pix-fmt",
                                      "yuv420p10le", "--cube", str(cube_dir / "log709_33.cube"), "--chroma-loc", "left"])
    with pytest.raises(ValueError, match="subsampling"):
        plan_from_args(args)


def test_pro_master_stage_renders_the_422_target_for_a_420_source():
    """Stage 1 of the two-stage mode is ProRes 422 HQ (yuv422p10le) whatever the source: the engine writes 4:2:2 and the encoder
    reads 4:2:2."""
    from lut_renderer_amd.command import _master_params, engine_command
    from lut_renderer_amd.pipe import engine_stage_commands
    master = _master_params(ProcessingParams(video_codec="libx264", crf="18"))
    info = VideoInfo(width=1920, height=1080, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709",
                     fps=25.0, duration=4.0)
    cmd = engine_command(Path("-"), Path("-"), master, Path("look.cube"), info, python_bin="python3")
    assert cmd[cmd.index("--pix-fmt") + 1] == "yuv420p10le" and cmd[cmd.index("--out-pix-fmt") + 1] == "yuv422p10le"
    c = engine_stage_commands(Path("in.mp4"), Path("master.mov"), master, Path("look.cube"), info, python_bin="python3")
    assert c.engine[c.engine.index("--out-pix-fmt") + 1] == "yuv422p10le"
    e = c.encoder
    assert e[e.index("-pix_fmt") + 1] == "yuv422p10le" and e.index("-pix_fmt") < e.index("-i")
    assert e[e.index("-c:v") + 1] == "prores_ks"
    # the CLI resolves the same call: a 4:2:0 source written as 4:2:2, replicate chroma
    from lut_renderer_amd.cli import build_parser, plan_from_args
    args = build_parser().parse_args([a for a in cmd[3:]])
    _, kw, w, h = plan_from_args(args)
    assert (kw["pix_fmt"], kw["out_pix_fmt"], w, h) == ("yuv420p10le", "yuv422p10le", 1920, 1080)
    assert "chroma_loc" not in kw
