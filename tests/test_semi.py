"""Semi-planar YUV frames without a GPU: the format table, the planar <-> semi-planar shuffles, rawvideo layouts,
the routing of `engine_call_for` / `plan_from_args`, and the argument checks of lutr_apply_yuv_semi that need no device."""
import ctypes as C

import numpy as np
import pytest

from lut_renderer_amd import _native
from lut_renderer_amd.params import ProcessingParams, VideoInfo

# name -> (depth, csx, csy, swap, shift, container dtype): the table of the issue, written out
TABLE = {
    "nv12": (8, 1, 1, 0, 0, np.uint8), "nv21": (8, 1, 1, 1, 0, np.uint8), "nv16": (8, 1, 0, 0, 0, np.uint8),
    "p010le": (10, 1, 1, 0, 6, np.uint16), "p012le": (12, 1, 1, 0, 4, np.uint16), "p016le": (16, 1, 1, 0, 0, np.uint16),
    "p210le": (10, 1, 0, 0, 6, np.uint16), "p212le": (12, 1, 0, 0, 4, np.uint16), "p216le": (16, 1, 0, 0, 0, np.uint16),
}
PLANAR = {"nv12": "yuv420p", "nv21": "yuv420p", "nv16": "yuv422p", "p010le": "yuv420p10le", "p012le": "yuv420p12le",
          "p016le": "yuv420p16le", "p210le": "yuv422p10le", "p212le": "yuv422p12le", "p216le": "yuv422p16le"}


def _planar_codes(name, w, h, seed=0):
    depth, csx, csy, _, _, dt = TABLE[name]
    rng = np.random.default_rng(seed)
    ch, cw = (h + (1 << csy) - 1) >> csy, (w + 1) >> 1
    return [rng.integers(0, 1 << depth, size=s, dtype=np.int64).astype(dt) for s in ((h, w), (ch, cw), (ch, cw))]


# ------------------------------------------------------------------ format table
def test_format_table():
    from lut_renderer_amd.engine import parse_pix_fmt, parse_semi_fmt
    assert set(_native.SEMI_FORMATS) == set(TABLE)
    for name, (depth, csx, csy, swap, shift, dt) in TABLE.items():
        f = parse_semi_fmt(name)
        assert (f.name, f.depth, f.csx, f.csy, f.swap, f.shift, f.np_dtype) == (name, depth, csx, csy, swap, shift, dt), name
        assert f.planar == PLANAR[name] and f.code == parse_pix_fmt(PLANAR[name]).code
        assert f.plane_shape(0, 37, 23) == (23, 37) and f.plane_shape(1, 37, 23) == ((23 + csy) >> csy, 38)
    for other in ("nv24", "nv42", "p010be", "p410le", "yuv420p", "rgb24", "", None):
        assert parse_semi_fmt(other) is None
    for name in TABLE:                                       # parse_pix_fmt keeps describing three-plane frames
        with pytest.raises(ValueError):
            parse_pix_fmt(name)


# ------------------------------------------------------------------ to_semi / to_planar
@pytest.mark.parametrize("name", sorted(TABLE))
@pytest.mark.parametrize("size", [(37, 23), (64, 16)])
def test_round_trip(name, size):
    import torch
    from lut_renderer_amd.semiplanar import to_planar, to_semi
    w, h = size
    depth, csx, csy, swap, shift, dt = TABLE[name]
    planes = _planar_codes(name, w, h, seed=w)
    semi = to_semi(planes, name)
    assert len(semi) == 2 and semi[0].shape == (h, w) and semi[1].shape == (planes[1].shape[0], 2 * planes[1].shape[1])
    assert all(p.dtype == dt for p in semi)
    back = to_planar(semi, name)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(back, planes))
    # the words themselves
    first, second = semi[1][:, 0::2], semi[1][:, 1::2]
    cb, cr = (second, first) if swap else (first, second)
    assert np.array_equal(cb, planes[1].astype(np.uint32) << shift) and np.array_equal(cr, planes[2].astype(np.uint32) << shift)
    assert np.array_equal(semi[0], planes[0].astype(np.uint32) << shift)
    # torch tensors (16-bit planes travel as int16 bits) give the same bytes
    tt = [torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p) for p in planes]
    ts = to_semi(tt, name)
    assert all(np.array_equal(t.numpy().view(dt), s) for t, s in zip(ts, semi))
    tb = to_planar(ts, name)
    assert all(np.array_equal(t.numpy().view(dt), p) for t, p in zip(tb, planes))
    # a batch keeps its leading axis
    batch = [np.stack([p, p]) for p in planes]
    sb = to_semi(batch, name)
    assert sb[1].shape == (2,) + semi[1].shape and np.array_equal(sb[1][1], semi[1])


def test_words_of_p010le_and_pairs_of_nv21():
    from lut_renderer_amd.semiplanar import to_planar, to_semi
    y = np.array([[1, 2], [3, 1023]], np.uint16)
    cb, cr = np.array([[512]], np.uint16), np.array([[700]], np.uint16)
    s = to_semi([y, cb, cr], "p010le")
    assert s[0].tolist() == [[1 << 6, 2 << 6], [3 << 6, 1023 << 6]] and s[1].tolist() == [[512 << 6, 700 << 6]]
    s8 = to_semi([y.astype(np.uint8), np.array([[10]], np.uint8), np.array([[20]], np.uint8)], "nv21")
    assert s8[1].tolist() == [[20, 10]]
    assert to_semi([y.astype(np.uint8), np.array([[10]], np.uint8), np.array([[20]], np.uint8)], "nv12")[1].tolist() == [[10, 20]]
    # to_planar drops whatever the low bits hold
    rng = np.random.default_rng(3)
    planes = _planar_codes("p010le", 37, 23, seed=5)
    semi = to_semi(planes, "p010le")
    dirty = [p | rng.integers(0, 64, size=p.shape).astype(np.uint16) for p in semi]
    assert any((d & 63).any() for d in dirty)
    assert all(np.array_equal(a, b) for a, b in zip(to_planar(dirty, "p010le"), planes))
    with pytest.raises(ValueError):
        to_semi(planes, "yuv420p")
    with pytest.raises(ValueError):
        to_planar(semi, "nv24")


# ------------------------------------------------------------------ rawvideo layouts
def test_input_layouts():
    import torch
    from lut_renderer_amd.engine import PixFmt, SemiFmt
    from lut_renderer_amd.stream import FrameLayout, input_layout
    lay = input_layout("nv12", 65, 33)
    assert isinstance(lay, FrameLayout) and isinstance(lay.fmt, SemiFmt)
    assert lay.frame_bytes == 65 * 33 + 2 * 33 * 17 and lay.fmt.name == "nv12"
    v = lay.plane_views(torch.zeros(2 * lay.frame_bytes, dtype=torch.uint8), 2)
    assert [tuple(t.shape) for t in v] == [(2, 33, 65), (2, 17, 66)] and all(t.dtype == torch.uint8 for t in v)
    lay = input_layout("p210le", 65, 33)
    assert isinstance(lay.fmt, SemiFmt) and lay.frame_bytes == 2 * (65 * 33 + 2 * 33 * 33) and lay.itemsize == 2
    buf = torch.arange(2 * lay.frame_bytes // 2, dtype=torch.int32).to(torch.int16).view(torch.uint8)
    v = lay.plane_views(buf, 2)
    assert [tuple(t.shape) for t in v] == [(2, 33, 65), (2, 33, 66)] and all(t.dtype == torch.int16 for t in v)
    fe = lay.frame_bytes // 2
    assert int(v[0][1, 0, 0]) == np.int16(fe) and int(v[1][0, 0, 0]) == 65 * 33 and int(v[1][1, 2, 5]) == np.int16(fe + 65 * 33 + 2 * 66 + 5)
    assert isinstance(input_layout("yuv420p", 65, 33), FrameLayout) and isinstance(input_layout("yuv420p", 65, 33).fmt, PixFmt)


# ------------------------------------------------------------------ routing
def _plan(pix_fmt, out_pix_fmt, **info_kw):
    from lut_renderer_amd.api import engine_call_for
    from lut_renderer_amd.plan import resolve_lut_plan
    info = VideoInfo(width=64, height=36, pix_fmt=pix_fmt, **info_kw)
    plan = resolve_lut_plan(ProcessingParams(), "look.cube", info)
    return plan, engine_call_for(plan, pix_fmt, out_pix_fmt)


def test_engine_call_for_routes_semi_planar_names():
    from lut_renderer_amd.api import is_float_out_call, is_rgb_call
    for src in TABLE:
        _, kw = _plan(src, None, colorspace="bt709")
        assert not is_rgb_call(kw) and not is_float_out_call(kw)
        assert kw == dict(pix_fmt=src, out_pix_fmt=src, interp="tetrahedral", matrix_in="bt709", matrix_out="bt709", range_src="tv",
                          range_in="tv", range_out="tv", lut_depth=TABLE[src][0])
    for src, out in (("nv12", "yuv420p"), ("yuv420p", "nv12"), ("yuv420p10le", "p010le"), ("p010le", "nv12"), ("nv21", "nv12"),
                     ("p210le", "yuv422p10le"), ("nv16", "p210le"), ("yuvj420p", "nv12")):
        _, kw = _plan(src, out)
        assert (kw["pix_fmt"], kw["out_pix_fmt"]) == (src.replace("yuvj", "yuv"), out)
    # a full-range source: the 8-bit intermediate is the planar twin of the source's subsampling, as for planar sources
    plan, kw = _plan("p210le", None, color_range="pc")
    assert plan.prologue and (kw["out_pix_fmt"], kw["lut_depth"], kw["range_src"]) == ("yuv422p", 8, "pc")
    plan, kw = _plan("p010le", "nv12", color_range="pc")
    assert (kw["out_pix_fmt"], kw["lut_depth"], kw["range_in"]) == ("nv12", 8, "tv")


def test_rejections_before_any_gpu_work():
    import torch
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.engine import check_semi_options
    for src, out in (("nv12", "yuv422p"), ("nv12", "nv16"), ("yuv444p", "nv12"), ("p010le", "p210le"), ("yuv422p10le", "p010le")):
        with pytest.raises(ValueError, match="subsampling"):
            _plan(src, out)
    for src in ("gbrp", "gbrp10le", "rgb24", "rgba64le", "gbrpf32le", "gbrapf32le"):      # RGB and float sources
        for out in ("nv12", "p010le"):
            with pytest.raises(ValueError):
                _plan(src, out)
    with pytest.raises(ValueError):
        _plan("nv12", "rgb24")
    assert check_semi_options("yuv420p", "yuv422p", "error_diffusion", "left", (4, 4)) is False     # not this path's business
    assert check_semi_options("nv12", None) is True
    for kw, what in ((dict(chroma_loc="left"), "chroma_loc"), (dict(dither="error_diffusion"), "dither"),
                     (dict(out_size=(32, 18)), "out_size")):
        for src, out in (("nv12", None), ("yuv420p", "nv12"), ("p010le", "yuv420p10le")):
            with pytest.raises(ValueError, match=what):
                check_semi_options(src, out, **kw)
    base = ["-i", "a", "-o", "b", "--size", "64x36", "--cube", "look.cube"]
    _, kw, w, h = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "p010le"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["lut_depth"], w, h) == ("p010le", "p010le", 10, 64, 36)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(base + ["--pix-fmt", "yuv420p10le", "--out-pix-fmt", "p010le"]))
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("yuv420p10le", "p010le")
    for extra, what in ((["--pix-fmt", "nv12", "--out-pix-fmt", "yuv422p"], "subsampling"),
                        (["--pix-fmt", "nv12", "--chroma-loc", "left"], "chroma_loc"),
                        (["--pix-fmt", "yuv420p", "--out-pix-fmt", "nv12", "--zscale-dither", "error_diffusion"], "dither"),
                        (["--pix-fmt", "p010le", "--out-size", "32x18"], "out_size"),
                        (["--pix-fmt", "rgb24", "--out-pix-fmt", "nv12"], None),
                        (["--pix-fmt", "gbrpf32le", "--out-pix-fmt", "nv12"], None)):
        with pytest.raises(ValueError, match=what):
            plan_from_args(build_parser().parse_args(base + extra))
    # apply_lut raises ahead of any engine
    semi = [torch.zeros((4, 8), dtype=torch.uint8), torch.zeros((2, 8), dtype=torch.uint8)]
    for kw, what in ((dict(chroma_loc="left"), "chroma_loc"), (dict(zscale_dither="error_diffusion"), "dither"),
                     (dict(resolution="16x8"), "out_size"), (dict(out_pix_fmt="yuv444p"), "subsampling")):
        with pytest.raises(ValueError, match=what):
            apply_lut(semi, cube=None, pix_fmt="nv12", engine=object(), **kw)


# ------------------------------------------------------------------ C-ABI without a device
def test_abi_symbol_and_null_context():
    lib = _native.load()
    assert "lutr_apply_yuv_semi" in _native.SYMBOLS and hasattr(lib, "lutr_apply_yuv_semi")
    assert C.sizeof(_native.YuvLayout) == 12
    p = _native.YuvParams(_native.fmt_code(10, 1, 1), _native.fmt_code(10, 1, 1), 10, 0, 0, 0, 0, 0)
    lay = _native.YuvLayout(1, 0, 6)
    pl = _native.Planes()
    rc = lib.lutr_apply_yuv_semi(None, C.byref(p), 2, C.byref(lay), C.byref(lay), 16, 16, 1, C.byref(pl), C.byref(pl), 0, 16)
    assert rc == _native.EINVAL and lib.lutr_last_error()
    assert lib.lutr_apply_yuv_semi(None, None, 2, None, None, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
