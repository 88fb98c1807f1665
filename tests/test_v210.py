"""v210 frames without a GPU: the words themselves, the planar <-> v210 shuffles, strides and rawvideo layouts, the
routing of `engine_call_for` / `plan_from_args` / `engine_command`, every rejection that has to come before any GPU work, and the
argument checks of lutr_apply_yuv_v210 that need no device."""
import ctypes as C
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native
from lut_renderer_amd.params import ProcessingParams, VideoInfo

ROOT = Path(__file__).resolve().parent.parent


def _planes(w, h, seed=0):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1024, size=s, dtype=np.int64).astype(np.uint16) for s in ((h, w), (h, (w + 1) >> 1), (h, (w + 1) >> 1))]


# ------------------------------------------------------------------ the words
def test_known_answer_and_a_hand_written_group():
    from lut_renderer_amd.v210 import to_planar, to_v210
    one = to_v210([np.array([[2]], np.uint16), np.array([[1]], np.uint16), np.array([[3]], np.uint16)], 1)
    assert one.dtype == np.uint32 and one.shape == (1, 32) and int(one[0, 0]) == 0x00300801
    # six luma samples, three pairs, written out slot by slot: a = bits 0-9, b = bits 10-19, c = bits 20-29
    y = np.array([[100, 101, 102, 103, 104, 105]], np.uint16)
    cb = np.array([[200, 201, 202]], np.uint16)
    cr = np.array([[300, 301, 302]], np.uint16)
    want = [200 | 100 << 10 | 300 << 20,          # Cb0 Y0 Cr0
            101 | 201 << 10 | 102 << 20,          # Y1 Cb1 Y2
            301 | 103 << 10 | 202 << 20,          # Cr1 Y3 Cb2
            104 | 302 << 10 | 105 << 20]          # Y4 Cr2 Y5
    buf = to_v210([y, cb, cr], 6)
    assert buf[0, :4].tolist() == want and not buf[0, 4:].any()
    assert [p.tolist() for p in to_planar(buf, 6)] == [y.tolist(), cb.tolist(), cr.tolist()]
    assert [p.tolist() for p in to_planar(np.array([want], np.uint32), 6)] == [y.tolist(), cb.tolist(), cr.tolist()]
    # the extreme codes keep to their slots
    top = to_v210([np.full((1, 6), 1023, np.uint16), np.zeros((1, 3), np.uint16), np.full((1, 3), 1023, np.uint16)], 6)
    assert top[0, :4].tolist() == [1023 << 10 | 1023 << 20, 1023 | 1023 << 20, 1023 | 1023 << 10, 1023 | 1023 << 10 | 1023 << 20]


@pytest.mark.parametrize("size", [(48, 2), (50, 3), (7, 5), (1, 1)])
def test_round_trip(size):
    import torch
    from lut_renderer_amd.v210 import row_bytes, to_planar, to_v210
    w, h = size
    planes = _planes(w, h, seed=w)
    buf = to_v210(planes, w)
    assert buf.shape == (h, row_bytes(w) // 4) and buf.dtype == np.uint32
    back = to_planar(buf, w)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype and a.shape == b.shape for a, b in zip(back, planes))
    assert not (buf >> 30).any()
    # torch tensors (words travel as int32 bits, codes as int16) give the same bytes
    tt = [torch.from_numpy(p.view(np.int16)) for p in planes]
    tb = to_v210(tt, w)
    assert tb.dtype == torch.int32 and np.array_equal(tb.numpy().view(np.uint32), buf)
    assert all(t.dtype == torch.int16 and np.array_equal(t.numpy().view(np.uint16), p) for t, p in zip(to_planar(tb, w), planes))
    # a batch keeps its leading axis
    bb = to_v210([np.stack([p, p]) for p in planes], w)
    assert bb.shape == (2,) + buf.shape and np.array_equal(bb[1], buf)
    assert all(np.array_equal(a[0], b) for a, b in zip(to_planar(bb, w), planes))


def test_slots_beyond_the_frame():
    from lut_renderer_amd.v210 import CB_SLOTS, CR_SLOTS, LUMA_SLOTS, to_planar, to_v210
    code = lambda words, slot: (words[..., slot[0]] >> slot[1]) & 0x3ff           # noqa: E731
    for w in (7, 50, 1, 4, 5):
        h = 3
        planes = _planes(w, h, seed=w)
        g = (w + 5) // 6
        buf = to_v210(planes, w)
        last = buf[:, 4 * (g - 1):4 * g]
        nl, nc = w - 6 * (g - 1), ((w + 1) >> 1) - 3 * (g - 1)                   # real luma samples / pairs of the last group
        for l in range(6):                                      # a luma slot beyond the frame repeats the last real luma sample
            assert np.array_equal(code(last, LUMA_SLOTS[l]), planes[0][:, -1] if l >= nl else planes[0][:, 6 * (g - 1) + l]), (w, l)
        for k in range(3):                                      # a pair beyond the frame repeats the last real pair
            assert np.array_equal(code(last, CB_SLOTS[k]), planes[1][:, -1] if k >= nc else planes[1][:, 3 * (g - 1) + k]), (w, k)
            assert np.array_equal(code(last, CR_SLOTS[k]), planes[2][:, -1] if k >= nc else planes[2][:, 3 * (g - 1) + k]), (w, k)
        assert not (buf >> 30).any() and not buf[:, 4 * g:].any()
        # input: bits 30-31, the slots beyond the frame and the words past the last group are ignored, whatever they hold
        rng = np.random.default_rng(w)
        ones = [np.full(p.shape, 1023, np.uint16) for p in planes]
        wide = [np.concatenate([ones[0], np.zeros((h, 6 * g - w), np.uint16)], axis=1)] + \
               [np.concatenate([c, np.zeros((h, 3 * g - c.shape[1]), np.uint16)], axis=1) for c in ones[1:]]
        mask = to_v210(wide, 6 * g)                             # 0x3ff in every slot that carries a real sample
        dirty = (buf & mask) | (rng.integers(0, 1 << 32, size=buf.shape, dtype=np.uint64).astype(np.uint32) & ~mask)
        assert (dirty >> 30).any() and (dirty != buf).any()
        assert all(np.array_equal(a, b) for a, b in zip(to_planar(dirty, w), planes)), w


def test_strides_and_frame_bytes():
    import torch
    from lut_renderer_amd.engine import PixFmt, V210Fmt
    from lut_renderer_amd.stream import FrameLayout, input_layout
    from lut_renderer_amd.v210 import frame_bytes, min_row_bytes, row_bytes, to_planar, to_v210
    assert [row_bytes(w) for w in (1920, 1280, 3840, 7, 48, 49)] == [5120, 3456, 10240, 128, 128, 256]
    assert [min_row_bytes(w) for w in (1920, 1280, 7, 6, 1)] == [5120, 3424, 32, 16, 16]
    for w, h, want in ((1280, 720, 3456 * 720), (1920, 1080, 5120 * 1080), (7, 5, 128 * 5)):
        lay = input_layout("v210", w, h)
        assert isinstance(lay, FrameLayout) and isinstance(lay.fmt, V210Fmt)
        assert lay.frame_bytes == want == frame_bytes(w, h) and lay.itemsize == 4
        assert lay.fmt.plane_shape(0, w, h) == (h, row_bytes(w) // 4)
    lay = input_layout("v210", 7, 5)
    buf = torch.arange(2 * lay.frame_bytes // 4, dtype=torch.int32).view(torch.uint8)
    v = lay.plane_views(buf, 2)
    assert [tuple(t.shape) for t in v] == [(2, 5, 32)] and v[0].dtype == torch.int32
    assert int(v[0][1, 0, 0]) == 5 * 32 and int(v[0][1, 2, 5]) == 5 * 32 + 2 * 32 + 5
    assert isinstance(input_layout("yuv422p10le", 7, 5).fmt, PixFmt)
    # a custom stride: any multiple of 4 that holds the groups
    planes = _planes(50, 3, seed=1)
    tight = to_v210(planes, 50, stride=144)
    loose = to_v210(planes, 50, stride=400)
    assert tight.shape == (3, 36) and loose.shape == (3, 100) and np.array_equal(loose[:, :36], tight) and not loose[:, 36:].any()
    assert np.array_equal(tight, to_v210(planes, 50)[:, :36])
    assert all(np.array_equal(a, b) for a, b in zip(to_planar(loose, 50), planes))
    for bad in (140, 146, 0):
        with pytest.raises(ValueError, match="stride"):
            to_v210(planes, 50, stride=bad)
    with pytest.raises(ValueError):
        to_planar(tight[:, :35], 50)
    with pytest.raises(ValueError):
        to_v210([planes[0], planes[1][:, :-1], planes[2][:, :-1]], 50)
    with pytest.raises(ValueError):
        to_v210(planes, 49)


# ------------------------------------------------------------------ parser and routing
def test_format_table_and_parsers():
    from lut_renderer_amd.engine import (V210Fmt, parse_packed_yuv_fmt, parse_pix_fmt, parse_semi_fmt, parse_v210_fmt, source_bit_depth,
                                         yuv_side)
    assert set(_native.V210_FORMATS) == {"v210"}
    assert "v210" not in _native.SEMI_FORMATS and "v210" not in _native.PACKED_YUV_FORMATS
    f = parse_v210_fmt("v210")
    assert isinstance(f, V210Fmt) and isinstance(yuv_side("v210"), V210Fmt)
    assert (f.name, f.depth, f.csx, f.csy, f.nplanes, f.family, f.full_range) == ("v210", 10, 1, 0, 1, "yuv", False)
    assert f.planar == "yuv422p10le" and f.code == parse_pix_fmt("yuv422p10le").code == _native.fmt_code(10, 1, 0)
    assert f.plane_shape(0, 1920, 1080) == (1080, 1280) and f.plane_shape(0, 50, 3) == (3, 64)
    assert source_bit_depth("v210") == 10
    for other in ("v210x", "v410", "r210", "y210le", "uyvy422", "p210le", "yuv422p10le", "", None):
        assert parse_v210_fmt(other) is None
    with pytest.raises(ValueError, match="unsupported pixel format"):
        parse_pix_fmt("v210")
    assert parse_semi_fmt("v210") is None and parse_packed_yuv_fmt("v210") is None


def _plan(pix_fmt, out_pix_fmt, **info_kw):
    from lut_renderer_amd.api import engine_call_for
    from lut_renderer_amd.plan import resolve_lut_plan
    info = VideoInfo(width=64, height=36, pix_fmt=pix_fmt, **info_kw)
    plan = resolve_lut_plan(ProcessingParams(), "look.cube", info)
    return plan, engine_call_for(plan, pix_fmt, out_pix_fmt)


def test_engine_call_for_routes_the_name():
    from lut_renderer_amd.api import is_float_out_call, is_rgb_call
    _, kw = _plan("v210", None, colorspace="bt709")
    assert not is_rgb_call(kw) and not is_float_out_call(kw)
    assert kw == dict(pix_fmt="v210", out_pix_fmt="v210", interp="tetrahedral", matrix_in="bt709", matrix_out="bt709", range_src="tv",
                      range_in="tv", range_out="tv", lut_depth=10)
    for src, out in (("v210", "v210"), ("v210", "yuv422p10le"), ("v210", "yuv422p"), ("yuv422p", "v210"), ("yuv422p16le", "v210"),
                     ("v210", "yuv420p10le"), ("v210", "yuv420p"), ("v210", "yuv444p10le"), ("yuvj422p", "v210")):
        _, kw = _plan(src, out)
        assert (kw["pix_fmt"], kw["out_pix_fmt"]) == (src.replace("yuvj", "yuv"), out)
    # a full-range source: the 8-bit intermediate is planar yuv422p, as the planar rule gives
    plan, kw = _plan("v210", None, color_range="pc")
    assert plan.prologue and (kw["out_pix_fmt"], kw["lut_depth"], kw["range_src"]) == ("yuv422p", 8, "pc")
    plan, kw = _plan("v210", "v210", color_range="pc")
    assert (kw["out_pix_fmt"], kw["lut_depth"], kw["range_in"]) == ("v210", 8, "tv")


def test_cli_and_command_argv():
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    _, kw, w, h = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "v210"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["lut_depth"], w, h) == ("v210", "v210", 10, 64, 36)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "v210", "--out-pix-fmt", "yuv420p"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["lut_depth"]) == ("v210", "yuv420p", 10)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuv422p10le", "--out-pix-fmt", "v210"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("yuv422p10le", "v210")
    assert "FourCC" in build_parser().format_help() and "v210" in build_parser().format_help()
    info = VideoInfo(width=64, height=36, bit_depth=10, pix_fmt="v210", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec=""), "look.cube", info, python_bin="python")
    assert cmd[cmd.index("--pix-fmt") + 1] == "v210" and cmd[cmd.index("--size") + 1] == "64x36" and "--out-pix-fmt" not in cmd
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))       # the stage's own argv parses and routes
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("v210", "v210")
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx265"), "look.cube", info, python_bin="python")
    out = cmd[cmd.index("--out-pix-fmt") + 1]
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("v210", out)


# ------------------------------------------------------------------ refusals
def test_rejections_before_any_gpu_work():
    import torch
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.engine import LutEngine, check_container_options, check_dual_options
    assert check_container_options("v210", None) == "v210" and check_container_options("yuv422p", "v210") == "v210"
    assert check_container_options("v210", "yuv420p") == "v210" and check_container_options("v210", "yuv444p16le") == "v210"
    assert check_container_options("v210", None, width=50) == "v210"
    # a v210 destination whose source is not 4:2:2
    for src in ("yuv420p10le", "yuv444p10le", "yuv420p"):
        with pytest.raises(ValueError, match="a v210 destination takes a 4:2:2 source"):
            _plan(src, "v210")
    # a v210 side together with a semi-planar or packed 4:2:2 side
    for src, out in (("v210", "nv16"), ("p210le", "v210"), ("nv12", "v210"), ("v210", "p010le")):
        with pytest.raises(ValueError, match="a semi-planar side together with a v210 side"):
            _plan(src, out)
    for src, out in (("v210", "y210le"), ("uyvy422", "v210"), ("y216le", "v210")):
        with pytest.raises(ValueError, match="a packed 4:2:2 side together with a v210 side"):
            _plan(src, out)
    # an RGB or float side
    for src in ("gbrp", "gbrp10le", "rgb24", "rgba64le", "gbrpf32le", "gbrapf32le"):
        with pytest.raises(ValueError):
            _plan(src, "v210")
        with pytest.raises(ValueError, match="an RGB source"):
            check_container_options(src, "v210")
    for out in ("rgb24", "gbrp10le", "gbrpf32le"):
        with pytest.raises(ValueError):
            _plan("v210", out)
    with pytest.raises(ValueError, match="v210 frames go with YUV formats on both sides"):
        check_container_options("v210", "rgb24")
    with pytest.raises(ValueError, match="v210 frames go with YUV formats on both sides"):
        check_container_options("v210", "gbrp10le")
    # the relatives
    for name in ("v210x", "v410", "r210"):
        with pytest.raises(ValueError, match="only v210 is taken"):
            _plan(name, None)
        with pytest.raises(ValueError, match="only v210 is taken"):
            check_container_options("v210", name)
    # chroma_loc, dither, out_size
    for kw, what in ((dict(chroma_loc="left"), r"chroma_loc\) is not supported with a v210 side"),
                     (dict(dither="error_diffusion"), "dither is not supported with a v210 side"),
                     (dict(out_size=(32, 18)), r"out_size\) is not supported with a v210 side")):
        for src, out in (("v210", None), ("yuv422p", "v210"), ("v210", "yuv420p10le")):
            with pytest.raises(ValueError, match=what):
                check_container_options(src, out, **kw)
    # the dual-output path
    for names in (("v210", "yuv422p10le", "yuv420p"), ("yuv422p10le", "v210", "yuv420p"), ("yuv422p10le", "yuv420p", "v210")):
        with pytest.raises(ValueError, match="v210 container"):
            check_dual_options(*names)
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    for extra, what in ((["--pix-fmt", "yuv420p", "--out-pix-fmt", "v210"], "4:2:2 source"),
                        (["--pix-fmt", "v210", "--out-pix-fmt", "nv16"], "semi-planar"),
                        (["--pix-fmt", "v210", "--out-pix-fmt", "uyvy422"], "packed 4:2:2"),
                        (["--pix-fmt", "v210", "--chroma-loc", "left"], "chroma_loc"),
                        (["--pix-fmt", "yuv422p", "--out-pix-fmt", "v210", "--zscale-dither", "error_diffusion"], "dither"),
                        (["--pix-fmt", "v210", "--out-size", "32x18"], "out_size"),
                        (["--pix-fmt", "rgb24", "--out-pix-fmt", "v210"], None),
                        (["--pix-fmt", "v210", "--second-output", "c", "--second-pix-fmt", "yuv420p"], "v210 container"),
                        (["--pix-fmt", "v410"], "only v210")):
        with pytest.raises(ValueError, match=what):
            plan_from_args(build_parser().parse_args(base + extra))
    # apply_lut raises ahead of any engine; a missing width
    buf = torch.zeros((4, 32), dtype=torch.int32)
    for kw, what in ((dict(chroma_loc="left"), "chroma_loc"), (dict(zscale_dither="error_diffusion"), "dither"),
                     (dict(resolution="16x8"), "out_size"), (dict(out_pix_fmt="nv16"), "semi-planar"),
                     (dict(out_pix_fmt="y210le"), "packed 4:2:2"), (dict(second_pix_fmt="yuv420p"), "v210 container")):
        with pytest.raises(ValueError, match=what):
            apply_lut(buf, cube=None, pix_fmt="v210", width=48, engine=object(), **kw)
    with pytest.raises(ValueError, match="width is required"):
        apply_lut(buf, cube=None, pix_fmt="v210", engine=object())
    with pytest.raises(ValueError, match="4:2:2 source"):
        apply_lut([torch.zeros((4, 8), dtype=torch.int16)] + [torch.zeros((2, 4), dtype=torch.int16)] * 2, cube=None,
                  pix_fmt="yuv420p10le", out_pix_fmt="v210", engine=object())
    # LutEngine.apply_yuv makes the same checks before it looks at its context or its tensors
    for kw, what in ((dict(pix_fmt="v210", chroma_loc="left"), "chroma_loc"), (dict(pix_fmt="v210", dither="error_diffusion"), "dither"),
                     (dict(pix_fmt="v210", out_size=(8, 4)), "out_size"), (dict(pix_fmt="v210", out_pix_fmt="nv16"), "semi-planar"),
                     (dict(pix_fmt="v210", out_pix_fmt="uyvy422"), "packed 4:2:2"),
                     (dict(pix_fmt="yuv420p", out_pix_fmt="v210"), "4:2:2 source"), (dict(pix_fmt="v410"), "only v210"),
                     (dict(pix_fmt="v210", out_pix_fmt="rgb24"), "YUV formats on both sides")):
        with pytest.raises(ValueError, match=what):
            LutEngine.apply_yuv(object(), buf, **kw)


def test_width_rules():
    import torch
    from lut_renderer_amd.engine import parse_pix_fmt, parse_v210_fmt, v210_frame_width
    v, p = parse_v210_fmt("v210"), parse_pix_fmt("yuv422p10le")
    buf = [torch.zeros((4, 32), dtype=torch.int32)]
    planes = [torch.zeros((4, 50), dtype=torch.int16)] + [torch.zeros((4, 25), dtype=torch.int16)] * 2
    with pytest.raises(ValueError, match="width is required"):
        v210_frame_width(v, v, buf, None)
    with pytest.raises(ValueError, match="width is required"):
        v210_frame_width(v, p, buf, None)                         # a planar destination still to be allocated tells nothing
    assert v210_frame_width(v, v, buf, None, 47) == 47
    assert v210_frame_width(p, v, planes, None) == 50 and v210_frame_width(v, p, buf, planes) == 50
    assert v210_frame_width(p, v, planes, None, 50) == 50
    with pytest.raises(ValueError, match="does not match"):
        v210_frame_width(p, v, planes, None, 48)


def test_recorded_container_options_are_unchanged():
    """The recorded comparison of tests/test_container_options.py, replayed from here: no outcome for any pair of the recorded
    names moved when the kind "v210" joined `check_container_options`, and the recorded tables were not extended."""
    sys.path.insert(0, str(ROOT / "tools"))
    import record_container_options as rec
    from lut_renderer_amd.api import engine_call_for
    from lut_renderer_amd.engine import check_container_options, check_packed_options, check_semi_options
    golden = json.loads((ROOT / "tests" / "golden" / "container_options.json").read_text())
    assert golden["names"] == list(rec.NAMES) and "v210" not in rec.NAMES and "v210" not in rec.layout_names()
    for a in rec.NAMES:
        default, full = rec.plans(a)
        for b in rec.NAMES + (None,):
            for plan, r in zip((default, full), golden["calls"][f"{a}->{b}"]):
                assert rec.outcome(engine_call_for, plan, a, b) == golden["outcomes"][r], (a, b)
            if b is None:
                continue
            for opt, (semi_ref, packed_ref) in zip(rec.OPTIONS, golden["checks"][f"{a}->{b}"]):
                semi, packed = golden["outcomes"][semi_ref], golden["outcomes"][packed_ref]
                assert rec.outcome(check_semi_options, a, b, *opt) == semi, (a, b, opt)
                assert rec.outcome(check_packed_options, a, b, *opt) == packed, (a, b, opt)
                got = rec.outcome(check_container_options, a, b, *opt)
                assert got.get("return") != "v210", (a, b, opt)
                if "raise" in packed:
                    assert got == packed, (a, b, opt)
                elif packed["return"]:
                    assert got == {"return": "packed"}, (a, b, opt)
                elif "raise" in semi:
                    assert got == semi, (a, b, opt)
                else:
                    assert got == {"return": "semi" if semi["return"] else None}, (a, b, opt)
    for name in rec.layout_names():
        for size in rec.LAYOUT_SIZES:
            assert rec.layout_record(name, *size) == golden["layouts"][f"{name}@{size[0]}x{size[1]}"], (name, size)


# ------------------------------------------------------------------ C-ABI without a device
def test_abi_symbol_and_null_context():
    lib = _native.load()
    assert "lutr_apply_yuv_v210" in _native.SYMBOLS and hasattr(lib, "lutr_apply_yuv_v210")
    header = (ROOT / "include" / "lutr.h").read_text()
    assert "int lutr_apply_yuv_v210(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int in_v210, int out_v210, int w, int h," in header
    p = _native.YuvParams(_native.fmt_code(10, 1, 0), _native.fmt_code(10, 1, 0), 10, 0, 0, 0, 0, 0)
    pl = _native.Planes()
    rc = lib.lutr_apply_yuv_v210(None, C.byref(p), 2, 1, 1, 48, 4, 1, C.byref(pl), C.byref(pl), 0, 4)
    assert rc == _native.EINVAL and lib.lutr_last_error()
    assert lib.lutr_apply_yuv_v210(None, None, 2, 1, 1, 48, 4, 1, None, None, 0, 4) == _native.EINVAL


def test_library_exports_the_entry_and_the_twin_does_not_use_the_oracle():
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    assert " T lutr_apply_yuv_v210" in nm
    text = (ROOT / "lut_renderer_amd" / "v210.py").read_text()
    assert "import oracle" not in text and "from oracle" not in text


def test_apply_lut_reaches_the_engine():
    """apply_lut's own checks pass for a v210 source and for a v210 destination and reach the engine (a stub that stops at its
    lock)."""
    import torch
    from lut_renderer_amd.api import apply_lut

    class Reached(Exception):
        pass

    class Lock:
        def __enter__(self):
            raise Reached()

        def __exit__(self, *exc):
            return False

    class Engine:
        precision, _applied_lut, _lock = "strict", None, Lock()

    i16 = lambda *s: torch.zeros(s, dtype=torch.int16)          # noqa: E731
    words = torch.zeros((4, 32), dtype=torch.int32)
    for planes, kw in ((words, dict(pix_fmt="v210", width=48)), ([words], dict(pix_fmt="v210", out_pix_fmt="yuv420p", width=7)),
                       ([i16(4, 50), i16(4, 25), i16(4, 25)], dict(pix_fmt="yuv422p10le", out_pix_fmt="v210")),
                       ([words], dict(pix_fmt="v210", out_pix_fmt="yuv422p10le", out=[i16(4, 48), i16(4, 24), i16(4, 24)]))):
        with pytest.raises(Reached):
            apply_lut(planes, cube=None, engine=Engine(), **kw)
