"""Packed 4:2:2 YUV frames without a GPU: the format table, the planar <-> packed shuffles, rawvideo layouts,
the routing of `engine_call_for` / `plan_from_args` / `engine_command`, every rejection that has to come before any GPU work, and
the argument checks of lutr_apply_yuv_packed that need no device."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native
from lut_renderer_amd.params import ProcessingParams, VideoInfo

# name -> (depth, group as written in memory, shift, container dtype): the table of DESIGN.md 3.12, written out
TABLE = {
    "yuyv422": (8, "Y0 Cb Y1 Cr", 0, np.uint8), "uyvy422": (8, "Cb Y0 Cr Y1", 0, np.uint8), "yvyu422": (8, "Y0 Cr Y1 Cb", 0, np.uint8),
    "y210le": (10, "Y0 Cb Y1 Cr", 6, np.uint16), "y212le": (12, "Y0 Cb Y1 Cr", 4, np.uint16), "y216le": (16, "Y0 Cb Y1 Cr", 0, np.uint16),
}
ORDER = {"Y0 Cb Y1 Cr": 0, "Cb Y0 Cr Y1": 1, "Y0 Cr Y1 Cb": 2}
PLANAR = {"yuyv422": "yuv422p", "uyvy422": "yuv422p", "yvyu422": "yuv422p", "y210le": "yuv422p10le", "y212le": "yuv422p12le",
          "y216le": "yuv422p16le"}


def _planar_codes(name, w, h, seed=0):
    depth, _, _, dt = TABLE[name]
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1 << depth, size=s, dtype=np.int64).astype(dt) for s in ((h, w), (h, (w + 1) >> 1), (h, (w + 1) >> 1))]


# ------------------------------------------------------------------ format table
def test_format_table():
    from lut_renderer_amd.engine import PackedYuvFmt, parse_packed_yuv_fmt, parse_pix_fmt, parse_semi_fmt
    assert set(_native.PACKED_YUV_FORMATS) == set(TABLE)
    for name, (depth, group, shift, dt) in TABLE.items():
        f = parse_packed_yuv_fmt(name)
        assert isinstance(f, PackedYuvFmt)
        assert (f.name, f.depth, f.order, f.shift, f.np_dtype) == (name, depth, ORDER[group], shift, dt), name
        assert (f.csx, f.csy, f.nplanes, f.family) == (1, 0, 1, "yuv")
        assert f.planar == PLANAR[name] and f.code == parse_pix_fmt(PLANAR[name]).code
        assert f.plane_shape(0, 37, 23) == (23, 76) and f.plane_shape(0, 64, 8) == (8, 128)
    for other in ("vuyx", "xv30le", "ayuv64le", "y210be", "nv12", "p210le", "yuv422p", "rgb24", "", None):
        assert parse_packed_yuv_fmt(other) is None
    for name in TABLE:                                       # the two older parsers say what they said before
        with pytest.raises(ValueError, match="unsupported pixel format"):
            parse_pix_fmt(name)
        assert parse_semi_fmt(name) is None


# ------------------------------------------------------------------ to_packed / to_planar
@pytest.mark.parametrize("name", sorted(TABLE))
@pytest.mark.parametrize("size", [(33, 5), (64, 8)])
def test_round_trip(name, size):
    import torch
    from lut_renderer_amd.packedyuv import to_packed, to_planar
    w, h = size
    depth, group, shift, dt = TABLE[name]
    g = (w + 1) >> 1
    planes = _planar_codes(name, w, h, seed=w)
    buf = to_packed(planes, name)
    assert buf.shape == (h, 4 * g) and buf.dtype == dt
    back = to_planar(buf, name, w)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype and a.shape == b.shape for a, b in zip(back, planes))
    # the words themselves, slot by slot of the group as the table writes it
    y = planes[0].astype(np.uint32)
    ypad = np.concatenate([y, y[:, -1:]], axis=1) if w % 2 else y        # odd width: the last real luma sample again
    want = {"Y0": ypad[:, 0::2], "Y1": ypad[:, 1::2], "Cb": planes[1].astype(np.uint32), "Cr": planes[2].astype(np.uint32)}
    for slot, what in enumerate(group.split()):
        assert np.array_equal(buf[:, slot::4], want[what] << shift), (name, slot, what)
    if shift:
        assert not (buf & ((1 << shift) - 1)).any()
    # torch tensors (16-bit buffers travel as int16 bits) give the same bytes
    tt = [torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p) for p in planes]
    tb = to_packed(tt, name)
    assert np.array_equal(tb.numpy().view(dt), buf)
    assert all(np.array_equal(t.numpy().view(dt), p) for t, p in zip(to_planar(tb, name, w), planes))
    # a batch keeps its leading axis
    bb = to_packed([np.stack([p, p]) for p in planes], name)
    assert bb.shape == (2,) + buf.shape and np.array_equal(bb[1], buf)
    assert all(np.array_equal(a[0], b) for a, b in zip(to_planar(bb, name, w), planes))


def test_odd_width_and_low_bits():
    from lut_renderer_amd.packedyuv import to_packed, to_planar
    y = np.array([[1, 2, 3]], np.uint8)
    cb, cr = np.array([[10, 11]], np.uint8), np.array([[20, 21]], np.uint8)
    assert to_packed([y, cb, cr], "yuyv422").tolist() == [[1, 10, 2, 20, 3, 11, 3, 21]]
    assert to_packed([y, cb, cr], "uyvy422").tolist() == [[10, 1, 20, 2, 11, 3, 21, 3]]
    assert to_packed([y, cb, cr], "yvyu422").tolist() == [[1, 20, 2, 10, 3, 21, 3, 11]]
    y10 = np.array([[1, 1023, 3]], np.uint16)
    b10 = to_packed([y10, cb.astype(np.uint16), cr.astype(np.uint16)], "y210le")
    assert b10.tolist() == [[1 << 6, 10 << 6, 1023 << 6, 20 << 6, 3 << 6, 11 << 6, 3 << 6, 21 << 6]]
    # input: the second luma sample of the last group is ignored, whatever it holds
    junk = np.array([[1, 10, 2, 20, 3, 11, 99, 21]], np.uint8)
    assert [p.tolist() for p in to_planar(junk, "yuyv422", 3)] == [[[1, 2, 3]], [[10, 11]], [[20, 21]]]
    assert to_planar(junk, "yuyv422")[0].tolist() == [[1, 2, 3, 99]]
    # to_planar drops whatever the low bits hold
    rng = np.random.default_rng(3)
    for name in ("y210le", "y212le"):
        shift = TABLE[name][2]
        planes = _planar_codes(name, 33, 5, seed=5)
        buf = to_packed(planes, name)
        dirty = buf | rng.integers(0, 1 << shift, size=buf.shape).astype(np.uint16)
        assert (dirty & ((1 << shift) - 1)).any()
        assert all(np.array_equal(a, b) for a, b in zip(to_planar(dirty, name, 33), planes))
    with pytest.raises(ValueError):
        to_packed([y, cb, cr], "yuv422p")
    with pytest.raises(ValueError):
        to_planar(junk, "nv16")
    with pytest.raises(ValueError):
        to_planar(junk, "yuyv422", 5)                         # 5 columns are three groups, not two
    with pytest.raises(ValueError):
        to_packed([y, cb[:, :1], cr[:, :1]], "yuyv422")


# ------------------------------------------------------------------ rawvideo layouts
def test_input_layouts():
    import torch
    from lut_renderer_amd.engine import PackedYuvFmt, PixFmt, SemiFmt
    from lut_renderer_amd.stream import FrameLayout, input_layout
    lay = input_layout("uyvy422", 65, 33)
    assert isinstance(lay, FrameLayout) and isinstance(lay.fmt, PackedYuvFmt)
    assert lay.frame_bytes == 33 * 4 * 33 and lay.fmt.name == "uyvy422"
    v = lay.plane_views(torch.zeros(2 * lay.frame_bytes, dtype=torch.uint8), 2)
    assert [tuple(t.shape) for t in v] == [(2, 33, 132)] and v[0].dtype == torch.uint8
    lay = input_layout("y210le", 64, 8)
    assert isinstance(lay.fmt, PackedYuvFmt) and lay.frame_bytes == 2 * 8 * 128 and lay.itemsize == 2
    buf = torch.arange(2 * lay.frame_bytes // 2, dtype=torch.int32).to(torch.int16).view(torch.uint8)
    v = lay.plane_views(buf, 2)
    assert [tuple(t.shape) for t in v] == [(2, 8, 128)] and v[0].dtype == torch.int16
    assert int(v[0][1, 0, 0]) == 8 * 128 and int(v[0][1, 2, 5]) == 8 * 128 + 2 * 128 + 5
    assert isinstance(input_layout("yuv422p", 65, 33).fmt, PixFmt) and isinstance(input_layout("nv16", 65, 33).fmt, SemiFmt)


# ------------------------------------------------------------------ routing
def _plan(pix_fmt, out_pix_fmt, **info_kw):
    from lut_renderer_amd.api import engine_call_for
    from lut_renderer_amd.plan import resolve_lut_plan
    info = VideoInfo(width=64, height=36, pix_fmt=pix_fmt, **info_kw)
    plan = resolve_lut_plan(ProcessingParams(), "look.cube", info)
    return plan, engine_call_for(plan, pix_fmt, out_pix_fmt)


def test_engine_call_for_routes_packed_names():
    from lut_renderer_amd.api import is_float_out_call, is_rgb_call
    for src in TABLE:
        _, kw = _plan(src, None, colorspace="bt709")
        assert not is_rgb_call(kw) and not is_float_out_call(kw)
        assert kw == dict(pix_fmt=src, out_pix_fmt=src, interp="tetrahedral", matrix_in="bt709", matrix_out="bt709", range_src="tv",
                          range_in="tv", range_out="tv", lut_depth=TABLE[src][0])
    for src, out in (("uyvy422", "uyvy422"), ("y210le", "yuv422p10le"), ("yuv422p", "yuyv422"), ("y210le", "yuyv422"),
                     ("uyvy422", "yuv420p"), ("y210le", "yuv420p10le"), ("uyvy422", "yuv444p"), ("yuvj422p", "uyvy422")):
        _, kw = _plan(src, out)
        assert (kw["pix_fmt"], kw["out_pix_fmt"]) == (src.replace("yuvj", "yuv"), out)
    # a full-range source: the 8-bit intermediate is planar yuv422p, as the planar rule gives
    plan, kw = _plan("y210le", None, color_range="pc")
    assert plan.prologue and (kw["out_pix_fmt"], kw["lut_depth"], kw["range_src"]) == ("yuv422p", 8, "pc")
    plan, kw = _plan("y210le", "yuyv422", color_range="pc")
    assert (kw["out_pix_fmt"], kw["lut_depth"], kw["range_in"]) == ("yuyv422", 8, "tv")


def test_cli_and_command_argv():
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.pipe import engine_stage_commands
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    _, kw, w, h = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "y210le"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["lut_depth"], w, h) == ("y210le", "y210le", 10, 64, 36)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "uyvy422", "--out-pix-fmt", "yuv420p"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["lut_depth"]) == ("uyvy422", "yuv420p", 8)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuv422p10le", "--out-pix-fmt", "y210le"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("yuv422p10le", "y210le")
    info = VideoInfo(width=64, height=36, bit_depth=10, pix_fmt="y210le", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx265"), "look.cube", info, python_bin="python")
    assert cmd[cmd.index("--pix-fmt") + 1] == "y210le" and cmd[cmd.index("--size") + 1] == "64x36"
    out = cmd[cmd.index("--out-pix-fmt") + 1]
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))       # the stage's own argv parses and routes
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("y210le", out)
    stages = engine_stage_commands(Path("in.mov"), Path("out.mov"), ProcessingParams(video_codec="libx265"), "look.cube", info)
    assert stages.decoder[stages.decoder.index("-pix_fmt") + 1] == "y210le"            # the decoder hands the packed surface over
    assert stages.engine[stages.engine.index("--pix-fmt") + 1] == "y210le"
    assert stages.encoder[stages.encoder.index("-pix_fmt") + 1] == stages.engine[stages.engine.index("--out-pix-fmt") + 1]


def test_rejections_before_any_gpu_work():
    import torch
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.engine import LutEngine, check_packed_options
    # a semi-planar side together with a packed side
    for src, out in (("uyvy422", "nv16"), ("nv16", "uyvy422"), ("y210le", "p210le"), ("p010le", "y210le")):
        with pytest.raises(ValueError, match="semi-planar"):
            _plan(src, out)
    # a packed destination with a layout change
    for src, out in (("yuv420p", "uyvy422"), ("yuv444p10le", "y210le"), ("yuv420p10le", "yuyv422")):
        with pytest.raises(ValueError, match="subsampling"):
            _plan(src, out)
    # an RGB or float source with a packed output; a packed source with an RGB output
    for src in ("gbrp", "gbrp10le", "rgb24", "rgba64le", "gbrpf32le", "gbrapf32le"):
        for out in ("uyvy422", "y210le"):
            with pytest.raises(ValueError):
                _plan(src, out)
    with pytest.raises(ValueError):
        _plan("uyvy422", "rgb24")
    # packed 4:4:4 and big-endian containers
    for name in ("vuyx", "xv30le", "ayuv64le", "y210be"):
        with pytest.raises(ValueError, match="not supported"):
            _plan(name, None)
        with pytest.raises(ValueError, match="not supported"):
            _plan("yuv422p", name)
        with pytest.raises(ValueError, match="not supported"):
            check_packed_options("uyvy422", name)
    # chroma_loc, dither, out_size
    assert check_packed_options("yuv420p", "yuv422p", "error_diffusion", "left", (4, 4)) is False    # not this path's business
    assert check_packed_options("nv12", None) is False
    assert check_packed_options("uyvy422", None) is True and check_packed_options("yuv422p", "y216le") is True
    for kw, what in ((dict(chroma_loc="left"), "chroma_loc"), (dict(dither="error_diffusion"), "dither"),
                     (dict(out_size=(32, 18)), "out_size")):
        for src, out in (("uyvy422", None), ("yuv422p", "yuyv422"), ("y210le", "yuv420p10le")):
            with pytest.raises(ValueError, match=what):
                check_packed_options(src, out, **kw)
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    for extra, what in ((["--pix-fmt", "yuv420p", "--out-pix-fmt", "uyvy422"], "subsampling"),
                        (["--pix-fmt", "uyvy422", "--out-pix-fmt", "nv16"], "semi-planar"),
                        (["--pix-fmt", "uyvy422", "--chroma-loc", "left"], "chroma_loc"),
                        (["--pix-fmt", "yuv422p", "--out-pix-fmt", "yuyv422", "--zscale-dither", "error_diffusion"], "dither"),
                        (["--pix-fmt", "y210le", "--out-size", "32x18"], "out_size"),
                        (["--pix-fmt", "rgb24", "--out-pix-fmt", "uyvy422"], None),
                        (["--pix-fmt", "gbrpf32le", "--out-pix-fmt", "y210le"], None),
                        (["--pix-fmt", "xv30le"], "not supported")):
        with pytest.raises(ValueError, match=what):
            plan_from_args(build_parser().parse_args(base + extra))
    # apply_lut raises ahead of any engine
    buf = torch.zeros((4, 16), dtype=torch.uint8)
    for kw, what in ((dict(chroma_loc="left"), "chroma_loc"), (dict(zscale_dither="error_diffusion"), "dither"),
                     (dict(resolution="16x8"), "out_size"), (dict(out_pix_fmt="nv16"), "semi-planar"), (dict(width=5), "width")):
        with pytest.raises(ValueError, match=what):
            apply_lut(buf, cube=None, pix_fmt="uyvy422", engine=object(), **kw)
    with pytest.raises(ValueError, match="subsampling"):
        apply_lut([torch.zeros((4, 8), dtype=torch.uint8)] + [torch.zeros((2, 4), dtype=torch.uint8)] * 2, cube=None,
                  pix_fmt="yuv420p", out_pix_fmt="uyvy422", engine=object())
    # LutEngine.apply_yuv makes the same checks before it looks at its context or its tensors
    for kw, what in ((dict(pix_fmt="uyvy422", chroma_loc="left"), "chroma_loc"), (dict(pix_fmt="uyvy422", dither="error_diffusion"), "dither"),
                     (dict(pix_fmt="uyvy422", out_size=(8, 4)), "out_size"), (dict(pix_fmt="uyvy422", out_pix_fmt="nv16"), "semi-planar"),
                     (dict(pix_fmt="yuv420p", out_pix_fmt="uyvy422"), "subsampling"), (dict(pix_fmt="vuyx"), "not supported"),
                     (dict(pix_fmt="yuv422p", width=8), "width")):
        with pytest.raises(ValueError, match=what):
            LutEngine.apply_yuv(object(), buf, **kw)


# ------------------------------------------------------------------ C-ABI without a device
def test_abi_symbol_and_null_context():
    lib = _native.load()
    assert "lutr_apply_yuv_packed" in _native.SYMBOLS and hasattr(lib, "lutr_apply_yuv_packed")
    assert C.sizeof(_native.YuvPacking) == 12
    header = (Path(_native.__file__).resolve().parents[1] / "include" / "lutr.h").read_text()
    for line in ("#define LUTR_PK_YUYV 0", "#define LUTR_PK_UYVY 1", "#define LUTR_PK_YVYU 2", "typedef struct lutr_yuv_packing {"):
        assert line in header, line
    p = _native.YuvParams(_native.fmt_code(10, 1, 0), _native.fmt_code(10, 1, 0), 10, 0, 0, 0, 0, 0)
    pk = _native.YuvPacking(1, 0, 6)
    pl = _native.Planes()
    rc = lib.lutr_apply_yuv_packed(None, C.byref(p), 2, C.byref(pk), C.byref(pk), 16, 16, 1, C.byref(pl), C.byref(pl), 0, 16)
    assert rc == _native.EINVAL and lib.lutr_last_error()
    assert lib.lutr_apply_yuv_packed(None, None, 2, None, None, 16, 16, 1, None, None, 0, 16) == _native.EINVAL


def test_library_exports_the_entry_and_still_does_not_link_the_oracle():
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    assert " T lutr_apply_yuv_packed" in nm
    assert "orc_" not in subprocess.run(["nm", "-D", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    ldd = subprocess.run(["ldd", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    assert "oracle" not in ldd and "liblut3d" not in ldd
    text = (Path(_native.__file__).resolve().parent / "packedyuv.py").read_text()
    assert "import oracle" not in text and "from oracle" not in text


def test_apply_lut_prologue_for_every_source_family():
    """apply_lut's own checks run for RGB, planar, semi-planar and packed sources alike and reach the engine (a stub that stops
    at its lock): the packed names must not get in the way of the other families."""
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

    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)  # noqa: E731
    for planes, kw in ((u8(4, 8, 3), dict(pix_fmt="rgb24", out_pix_fmt="yuv420p")),
                       ([u8(4, 8), u8(2, 4), u8(2, 4)], dict(pix_fmt="yuv420p")),
                       ([u8(4, 8), u8(2, 8)], dict(pix_fmt="nv12")),
                       (u8(4, 16), dict(pix_fmt="uyvy422")), ([u8(4, 16)], dict(pix_fmt="uyvy422", out_pix_fmt="yuv420p", width=7)),
                       ([torch.zeros((4, 8), dtype=torch.float32)] * 3, dict(pix_fmt="gbrpf32le"))):
        with pytest.raises(Reached):
            apply_lut(planes, cube=None, engine=Engine(), **kw)


def test_container_sides_with_the_wrong_number_of_planes_keep_their_words():
    """What `apply_yuv` says of a semi-planar, packed or v210 call whose source has the wrong number of planes, before it looks
    at anything else (host only: an engine object without a context)."""
    import torch
    from lut_renderer_amd.engine import LutEngine
    eng = object.__new__(LutEngine)
    eng.device = torch.device("cpu")
    y = torch.zeros((4, 16), dtype=torch.uint8)
    for planes, kw, text in (([y], dict(pix_fmt="nv12"), "'nv12' takes 2 planes"),
                             (y, dict(pix_fmt="nv12"), "'nv12' takes 2 planes"),
                             ([y, y, y], dict(pix_fmt="nv12", out_pix_fmt="yuv420p"), "'nv12' takes 2 planes"),
                             ([y, y], dict(pix_fmt="yuv420p", out_pix_fmt="nv12"), "'yuv420p' takes 3 planes"),
                             ([y, y], dict(pix_fmt="uyvy422"), "'uyvy422' takes 1 plane"),
                             (y, dict(pix_fmt="yuv422p", out_pix_fmt="uyvy422"), "'yuv422p' takes 3 planes"),
                             ([y, y], dict(pix_fmt="v210", width=6), "'v210' takes 1 plane"),
                             (y, dict(pix_fmt="yuv422p10le", out_pix_fmt="v210"), "'yuv422p10le' takes 3 planes"),
                             ([y, y], dict(pix_fmt="yuv422p10le", out_pix_fmt="v210"), "'yuv422p10le' takes 3 planes")):
        with pytest.raises(ValueError) as e:
            eng.apply_yuv(planes, **kw)
        assert str(e.value) == text, (kw, str(e.value))
