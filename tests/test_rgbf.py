"""Planar float RGB sources without a GPU: the reference composition of tests/_rgbf_twin.py pinned to the C
oracle through code-valued floats, known answers for the sanitiser and the quantiser, and the plumbing from the API down to the
argv layer."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, frames
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _rgbf_twin as twin
from tests._csp_files import write_csp_with_prelut

F = np.float32
MODES3 = ("nearest", "trilinear", "tetrahedral")


# ------------------------------------------------------------------ the twin against the C oracle
def _codes(depth, w=41, h=23, k=0):
    return frames.make_rgb("uniform", w, h, depth, k=k)


@pytest.mark.parametrize("depth", (8, 10, 12, 16))
def test_twin_on_code_valued_floats_is_the_c_oracle(orc, depth):
    """fl(code * fl(1 / M)) through the twin, then lut3d's integer store, is the oracle's lut3d on the codes: a lattice that leaves
    [0, 1] (the store clips) and a scaled domain."""
    rng = np.random.default_rng(17)
    table = rng.uniform(-0.2, 1.3, size=(17, 17, 17, 3)).astype(F)
    scale = np.array([1.0, 1.0, 0.75], F)
    planes = _codes(depth, k=depth)
    for mode in MODES3:
        got = twin.to_codes(twin.apply_float(table, scale, mode, twin.code_frame(planes, depth)), depth)
        want = orc.apply_rgb(table, scale, depth, mode, planes)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (depth, mode)


@pytest.mark.parametrize("depth", (8, 10, 12, 16))
def test_twin_with_a_prelut_is_the_c_oracle(orc, tmp_path, depth):
    from lut_renderer_amd import cube
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, cube.log709_lattice(17), shapers)
    _n, scale, table, pre = orc.parse_lut_file_ex(p)
    assert pre is not None
    planes = _codes(depth, k=3 + depth)
    for mode in MODES3:
        got = twin.to_codes(twin.apply_float(table, scale, mode, twin.code_frame(planes, depth), prelut=pre), depth)
        want = orc.apply_rgb(table, scale, depth, mode, planes, prelut=pre)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), (depth, mode)


# ------------------------------------------------------------------ known answers
def test_sanitize_known_answers():
    bits = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xffffffff, 0x7fa55aa5,     # NaN: either sign, quiet / signalling, payloads
                     0x7f800000, 0xff800000,                                         # +inf, -inf
                     0x80000000, 0x00000001, 0x807fffff, 0x00400000,                 # -0.0 and denormals: unchanged
                     0x3f800000, 0xc1200000, 0x7f7fffff, 0xff7fffff], np.uint32)     # 1, -10, +-FLT_MAX: unchanged
    got = twin.sanitize(bits.view(F)).view(np.uint32)
    want = bits.copy()
    want[:5] = 0
    want[5], want[6] = 0x7f7fffff, 0xff7fffff
    assert np.array_equal(got, want), [hex(v) for v in got]
    assert twin.FLT_MAX == np.array([0x7f7fffff], np.uint32).view(F)[0]


def test_quantiser_known_answers():
    q = twin.quantise
    assert q(np.array([0.5 / 65535], F))[0] == 0            # ties go to the even code
    assert q(np.array([1.5 / 65535], F))[0] == 2
    assert q(np.array([2.5 / 65535], F))[0] == 2
    assert np.array_equal(q(np.array([-0.25, -1e-9, -twin.FLT_MAX], F)), np.zeros(3, F))
    assert np.array_equal(q(np.array([1.0, 1.0000001, 8.0, twin.FLT_MAX], F)), np.full(4, 65535, F))
    assert np.array_equal(q(np.array([0.0, 1.0 / 65535, 0.25], F)), np.array([0, 1, 16384], F))


def test_outputs_are_not_clipped():
    """Float in, float out keeps what the lattice holds: values below 0 and above 1 survive."""
    rng = np.random.default_rng(3)
    table = rng.uniform(-0.2, 1.2, size=(9, 9, 9, 3)).astype(F)
    out = twin.apply_float(table, np.ones(3, F), "tetrahedral", twin.make_float("uniform", 64, 32))
    assert min(p.min() for p in out) < 0.0 and max(p.max() for p in out) > 1.0


def test_abi_symbols_and_einval_without_a_gpu():
    lib = _native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    for sym in ("lutr_apply_planar_rgb_f32", "lutr_apply_rgbf_to_yuv"):
        assert f" T {sym}\n" in nm and sym in _native.SYMBOLS
    assert lib.lutr_apply_planar_rgb_f32(None, 2, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
    assert lib.lutr_apply_rgbf_to_yuv(None, None, 2, 0, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
    assert lib.lutr_apply_rgbf_to_yuv(None, None, 2, 7, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
    assert b"dither" in lib.lutr_last_error()


# ------------------------------------------------------------------ host plumbing
def _plan(pix_fmt, out_pix_fmt, **info_kw):
    from lut_renderer_amd.api import engine_call_for
    from lut_renderer_amd.plan import resolve_lut_plan
    info = VideoInfo(width=64, height=36, pix_fmt=pix_fmt, **info_kw)
    plan = resolve_lut_plan(ProcessingParams(), "look.cube", info)
    return plan, engine_call_for(plan, pix_fmt, out_pix_fmt)


def test_parse_rgb_source_takes_the_float_names():
    from lut_renderer_amd.engine import parse_pix_fmt, parse_rgb_source
    for name, planes in (("gbrpf32le", 3), ("gbrapf32le", 4)):
        s = parse_rgb_source(name)
        assert s is not None and s.floating and not s.packed and s.nplanes == planes and s.itemsize == 4 and s.depth == 16
        assert s.frame_bytes(65, 33) == planes * 33 * 65 * 4
    assert not parse_rgb_source("gbrp10le").floating and not parse_rgb_source("rgb24").floating
    assert parse_rgb_source("gbrpf32be") is None and parse_rgb_source("gbrpf16le") is None
    with pytest.raises(ValueError):                         # parse_pix_fmt keeps describing integer planar frames
        parse_pix_fmt("gbrpf32le")


def test_input_layouts_count_float_bytes():
    import torch
    from lut_renderer_amd.stream import FloatFrameLayout, input_layout
    for name, planes in (("gbrpf32le", 3), ("gbrapf32le", 4)):
        lay = input_layout(name, 65, 33)
        assert isinstance(lay, FloatFrameLayout) and lay.frame_bytes == planes * 4 * 65 * 33 and lay.fmt.name == name
    lay = input_layout("gbrapf32le", 3, 2)
    buf = torch.arange(2 * 4 * 6, dtype=torch.float32).view(torch.uint8)
    v = lay.plane_views(buf, 2)
    assert len(v) == 4 and all(tuple(t.shape) == (2, 2, 3) and t.dtype == torch.float32 for t in v)
    assert float(v[0][0, 0, 0]) == 0 and float(v[1][0, 0, 0]) == 6 and float(v[3][1, 1, 2]) == 47 and float(v[2][1, 0, 1]) == 37


def test_engine_call_for_float_sources():
    from lut_renderer_amd.api import is_float_out_call, is_rgb_call
    for src in ("gbrpf32le", "gbrapf32le"):
        for out in (None, src, "gbrpf32le"):
            plan, kw = _plan(src, out, colorspace="bt709")
            assert is_float_out_call(kw) and is_rgb_call(kw) and not plan.prologue
            assert kw == dict(pix_fmt=src, out_pix_fmt=out or src, interp="tetrahedral")
        for out in ("yuv420p10le", "yuv422p", "yuv444p16le"):
            _, kw = _plan(src, out, colorspace="bt709")
            assert not is_float_out_call(kw) and is_rgb_call(kw)
            assert kw == dict(pix_fmt=src, out_pix_fmt=out, interp="tetrahedral", matrix_out="bt709", range_out="tv")
    _, kw = _plan("gbrpf32le", "yuv420p")
    assert kw["matrix_out"] == "smpte170m"
    plan, kw = _plan("gbrpf32le", "yuv420p10le", color_range="pc")       # flagged full range: the two-stage plan of 3.9
    assert plan.prologue and kw["intermediate_pix_fmt"] == "yuv420p" and kw["prologue_out_range"] == "tv"
    _, kw = _plan("gbrp10le", "yuv420p10le")
    assert not is_float_out_call(kw)


def test_rejections_before_any_gpu_work():
    for out in ("gbrp10le", "gbrp", "rgb24", "rgba64le", "nv12", "gray"):    # any other output
        with pytest.raises(ValueError):
            _plan("gbrpf32le", out)
    with pytest.raises(ValueError, match="alpha"):
        _plan("gbrpf32le", "gbrapf32le")
    with pytest.raises(ValueError):                         # float out of an integer or YUV source stays undefined
        _plan("gbrp10le", "gbrpf32le")
    with pytest.raises(ValueError):
        _plan("yuv420p", "gbrpf32le")
    with pytest.raises(ValueError, match="full range"):
        _plan("gbrpf32le", None, color_range="pc")
    from lut_renderer_amd.cli import build_parser, plan_from_args
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    for extra in (["--out-pix-fmt", "yuv420p10le"], []):
        with pytest.raises(ValueError, match="chroma"):
            plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "gbrpf32le", "--chroma-loc", "left"] + extra))
    with pytest.raises(ValueError, match="dither"):
        plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "gbrpf32le", "--zscale-dither", "error_diffusion"]))
    from lut_renderer_amd.api import apply_lut
    import torch
    planes = [torch.zeros((4, 8), dtype=torch.float32) for _ in range(3)]
    with pytest.raises(ValueError, match="chroma"):         # raised ahead of any engine
        apply_lut(planes, cube=None, pix_fmt="gbrpf32le", out_pix_fmt="yuv420p", chroma_loc="left", engine=object())
    with pytest.raises(ValueError, match="chroma"):
        apply_lut(planes, cube=None, pix_fmt="gbrpf32le", chroma_loc="center", engine=object())
    with pytest.raises(ValueError):
        apply_lut(planes, cube=None, pix_fmt="gbrpf32le", out_pix_fmt="gbrp16le", engine=object())


def test_plan_from_args_for_float_sources():
    from lut_renderer_amd.cli import build_parser, plan_from_args
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    _, kw, w, h = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "gbrpf32le"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"], w, h) == ("gbrpf32le", "gbrpf32le", 64, 36)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(
        base + ["--pix-fmt", "gbrapf32le", "--out-pix-fmt", "yuv420p10le", "--zscale-dither", "error_diffusion"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["dither"]) == ("gbrapf32le", "yuv420p10le", "error_diffusion")


def test_argv_layer_for_float_sources():
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.pipe import engine_stage_commands
    info = VideoInfo(width=64, height=36, pix_fmt="gbrpf32le", fps=25.0)
    # an explicit output format: the fused float -> YUV stage
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx265", pix_fmt="yuv420p10le"), Path("look.cube"),
                         info, python_bin="python3")
    assert cmd[:3] == ["python3", "-m", "lut_renderer_amd.cli"]
    assert cmd[cmd.index("--pix-fmt") + 1] == "gbrpf32le" and cmd[cmd.index("--out-pix-fmt") + 1] == "yuv420p10le"
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("gbrpf32le", "yuv420p10le")
    # no resolved output format: the stage stays float
    info4 = VideoInfo(width=64, height=36, pix_fmt="gbrapf32le", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx264"), Path("look.cube"), info4, python_bin="python3")
    assert cmd[cmd.index("--pix-fmt") + 1] == "gbrapf32le" and "--out-pix-fmt" not in cmd
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("gbrapf32le", "gbrapf32le")
    c = engine_stage_commands(Path("in.exr"), Path("out.mov"), ProcessingParams(video_codec="libx265", pix_fmt="yuv422p10le"),
                              Path("look.cube"), info, python_bin="python3")
    assert c.decoder[c.decoder.index("-pix_fmt") + 1] == "gbrpf32le"
    assert c.engine[c.engine.index("--pix-fmt") + 1] == "gbrpf32le" and c.engine[c.engine.index("--out-pix-fmt") + 1] == "yuv422p10le"
    assert c.encoder[c.encoder.index("-pix_fmt") + 1] == "yuv422p10le"
    c = engine_stage_commands(Path("in.exr"), Path("out.mov"), ProcessingParams(video_codec="libx264"), Path("look.cube"), info,
                              python_bin="python3")
    assert "--out-pix-fmt" not in c.engine and c.encoder[c.encoder.index("-pix_fmt") + 1] == "gbrpf32le"
    with pytest.raises(ValueError, match="chroma"):
        engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx265", pix_fmt="yuv420p10le"), Path("look.cube"), info,
                       chroma_loc="left")
    with pytest.raises(ValueError, match="chroma"):
        engine_stage_commands(Path("in.exr"), Path("out.mov"), ProcessingParams(video_codec="libx264"), Path("look.cube"), info,
                              chroma_loc="center")
