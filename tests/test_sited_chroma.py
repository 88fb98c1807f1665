"""Sited bilinear chroma resampling: `chroma_loc` = left | center | topleft.

CPU: the NumPy twin (tests/_sited_twin.py) pinned to hand-written weights and to the oracle's replicate contract where the
two must agree; the constants, the argv rendering and the argument checks.  GPU: lutr_apply_yuv_sited bit-exact against
the twin."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.engine import yuv_constants, yuv_constants_sited
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _sited_twin as twin
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
LAYOUTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}


# ------------------------------------------------------------------ CPU: the twin against hand-written weights
def test_up_weights_one_axis_by_hand():
    c = np.array([[0, 100, 200, 300]])
    s, wsum = twin.upsample(c, 1, 8, 1, 0, "left")            # co-sited: 4 C[k] | 2 C[k] + 2 C[k+1]
    assert wsum == 4 and s[0].tolist() == [0, 200, 400, 600, 800, 1000, 1200, 1200]
    s, _ = twin.upsample(c, 1, 8, 1, 0, "center")             # interstitial: C[k-1] + 3 C[k] | 3 C[k] + C[k+1]
    assert s[0].tolist() == [0, 100, 300, 500, 700, 900, 1100, 1200]
    s, _ = twin.upsample(c, 1, 7, 1, 0, "center")             # odd width: the last luma column is even
    assert s[0].tolist() == [0, 100, 300, 500, 700, 900, 1100]
    s, wsum = twin.upsample(np.array([[5], [9]]), 4, 1, 0, 1, "topleft")   # vertical axis only (4:4:0-like test of the table)
    assert wsum == 4 and s[:, 0].tolist() == [20, 28, 36, 36]
    s, _ = twin.upsample(np.array([[5], [9]]), 4, 1, 0, 1, "left")         # left is vertically interstitial
    assert s[:, 0].tolist() == [20, 24, 32, 36]


def test_up_weights_two_axes_by_hand():
    c = np.array([[0, 16], [32, 64]])
    s, wsum = twin.upsample(c, 4, 4, 1, 1, "topleft")
    assert wsum == 16
    # (1,1): rows 2 C[0] + 2 C[1], columns 2 C[0] + 2 C[1] -> 4 * (0 + 16 + 32 + 64)
    assert s[0, 0] == 0 and s[1, 1] == 4 * (0 + 16 + 32 + 64) and s[0, 1] == 8 * (0 + 16) and s[3, 3] == 16 * 64
    s, _ = twin.upsample(c, 4, 4, 1, 1, "center")
    # (1,1): rows 3 C[0] + C[1], columns 3 C[0] + C[1]
    assert s[1, 1] == 9 * 0 + 3 * 16 + 3 * 32 + 1 * 64
    s, _ = twin.upsample(c, 4, 4, 1, 1, "left")
    # (2,1): rows C[0] + 3 C[1] (interstitial, even), columns 2 C[0] + 2 C[1] (co-sited, odd)
    assert s[2, 1] == 1 * 2 * 0 + 1 * 2 * 16 + 3 * 2 * 32 + 3 * 2 * 64


def test_down_weights_by_hand():
    ramp = np.arange(8)[None, :]
    assert twin.downsample(ramp, 1, 0, "left")[0].tolist() == [1, 8, 16, 24]          # 1 2 1 over 2i-1, 2i, 2i+1
    assert twin.downsample(ramp, 1, 0, "center")[0].tolist() == [1, 5, 9, 13]         # 1 1 over 2i, 2i+1
    odd = np.arange(7)[None, :]
    assert twin.downsample(odd, 1, 0, "left")[0].tolist() == [1, 8, 16, 23]
    assert twin.downsample(odd, 1, 0, "center")[0].tolist() == [1, 5, 9, 12]
    col = np.arange(4)[:, None] * 10 + np.zeros((1, 2), np.int64)
    # 4:2:0 topleft: rows 1 2 1 x columns 1 2 1 on a frame constant along x: 4 * (r[2j-1] + 2 r[2j] + r[2j+1])
    assert twin.downsample(col, 1, 1, "topleft")[:, 0].tolist() == [4 * (0 + 0 + 10), 4 * (10 + 40 + 30)]
    assert twin.downsample(col, 1, 1, "left")[:, 0].tolist() == [4 * 10, 4 * 50]
    assert twin.down_n("left", 1, 1) == 8 and twin.down_n("topleft", 1, 1) == 16 and twin.down_n("center", 1, 0) == 2


def _lut(cube_dir, name):
    return cube.read_lut(cube_dir / name)


def test_444_and_flat_frames_equal_the_replicate_oracle(orc, cube_dir):
    lut = _lut(cube_dir, "log709_33.cube")
    k1 = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 10, 10, 1)
    for loc in twin.LOCS:
        # 4:4:4 through the twin's own stages 1 and 3 (its apply_yuv hands 4:4:4 to the oracle): weight 1 on both axes
        src = frames.natural_yuv(21, 13, 10, 0, 0, k=3)
        rq, gq, bq = twin.stage1(k1, 0, 0, loc, src)
        g, b, r = orc.apply_rgb(lut.table, lut.scale, 10, "tetrahedral", tuple(a.astype(np.uint16) for a in (gq, bq, rq)))
        got = twin.stage3(k1, 10, 0, 0, loc, (r, g, b))
        want = orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k1, 10, 10, 10, 0, 0, src)
        assert all(np.array_equal(g_, w) for g_, w in zip(got, want)), loc
        for lay, (csx, csy) in LAYOUTS.items():
            for w, h in ((16, 8), (9, 7)):
                ch, cw = frames.chroma_shape(w, h, csx, csy)
                flat = [np.full((h, w), 612, np.uint16), np.full((ch, cw), 300, np.uint16), np.full((ch, cw), 790, np.uint16)]
                k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, csx, csy, loc)
                got = twin.apply_yuv(lut.table, lut.scale, "trilinear", k, 10, 10, 10, csx, csy, loc, flat)
                k0 = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 10, 10, 1 << (csx + csy))
                want = orc.apply_yuv(lut.table, lut.scale, "trilinear", k0, 10, 10, 10, csx, csy, flat)
                assert all(np.array_equal(g, w_) for g, w_ in zip(got, want)), (loc, lay, w, h)


def test_center_with_constant_chroma_equals_the_oracle(orc, cube_dir):
    """Constant chroma makes the up-sampling exact; center's [1 1] x [1 1] down-sampling is today's block mean."""
    lut = _lut(cube_dir, "log709_33.cube")
    for csx, csy in ((1, 1), (1, 0)):
        for w, h in ((32, 18), (17, 11)):
            y = frames.natural_yuv(w, h, 10, csx, csy, k=5)[0]
            ch, cw = frames.chroma_shape(w, h, csx, csy)
            src = [y, np.full((ch, cw), 410, np.uint16), np.full((ch, cw), 655, np.uint16)]
            k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, csx, csy, "center")
            got = twin.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, csx, csy, "center", src)
            k0 = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 10, 10, 1 << (csx + csy))
            want = orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k0, 10, 10, 10, csx, csy, src)
            assert all(np.array_equal(g, w_) for g, w_ in zip(got, want)), (csx, csy, w, h)


def test_sited_constant_blocks_match_the_twin(orc):
    for lay, (csx, csy) in LAYOUTS.items():
        for din, dl, dout, rs in ((10, 10, 10, "tv"), (8, 8, 8, "tv"), (10, 10, 8, "tv"), (10, 8, 8, "pc"), (16, 16, 16, "tv")):
            kw = dict(fmt_in=_native.fmt_code(din, csx, csy), fmt_out=_native.fmt_code(dout, csx, csy), lut_depth=dl,
                      matrix_in=0, matrix_out=2, range_src=_native.RANGE[rs], range_in=0, range_out=0)
            assert np.array_equal(yuv_constants_sited(None, **kw), yuv_constants(**kw))
            for loc in twin.LOCS:
                k = twin.consts("bt709", "tv", "bt2020nc", "tv", din, dl, dout, csx, csy, loc, prologue=rs == "pc")
                assert np.array_equal(yuv_constants_sited(loc, **kw), k.as_block()), (lay, din, dl, dout, loc)


# ------------------------------------------------------------------ CPU: options, argv and checks
def test_symbols_and_bad_enum_without_a_gpu():
    lib = _native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    for sym in ("lutr_apply_yuv_sited", "lutr_yuv_constants_sited"):
        assert f" T {sym}\n" in nm and sym in _native.SYMBOLS
    for bad in (-1, 4, 99):
        assert lib.lutr_apply_yuv_sited(None, None, 2, bad, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
        assert b"chroma location" in lib.lutr_last_error()
        p = _native.YuvParams(_native.fmt_code(10, 1, 1), _native.fmt_code(10, 1, 1), 10, 0, 0, 0, 0, 0)
        assert lib.lutr_yuv_constants_sited(C.byref(p), bad, (C.c_float * 32)()) == _native.EINVAL


def test_unknown_names_and_dither_are_value_errors():
    from lut_renderer_amd import api
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.engine import check_chroma_loc
    for bad in ("top", "bottomleft", "Left", "replicate", ""):
        with pytest.raises(ValueError):
            check_chroma_loc(bad)
        with pytest.raises(ValueError):
            api.apply_lut([np.zeros((2, 2))] * 3, cube=None, pix_fmt="yuv420p10le", chroma_loc=bad)
    with pytest.raises(ValueError, match="dither"):
        api.apply_lut([np.zeros((2, 2))] * 3, cube=None, pix_fmt="yuv420p10le", zscale_dither="error_diffusion",
                      chroma_loc="left")
    args = build_parser().parse_args(["-i", "a", "-o", "b", "--size", "64x32", "--pix-fmt", "yuv420p10le", "--cube", "x.cube",
                                      "--chroma-loc", "topleft"])
    assert plan_from_args(args)[1]["chroma_loc"] == "topleft"
    args = build_parser().parse_args(["-i", "a", "-o", "b", "--size", "64x32", "--pix-fmt", "yuv420p10le", "--cube", "x.cube",
                                      "--chroma-loc", "left", "--zscale-dither", "error_diffusion"])
    with pytest.raises(ValueError, match="dither"):
        plan_from_args(args)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-i", "a", "-o", "b", "--size", "8x8", "--pix-fmt", "yuv420p", "--cube", "x",
                                   "--chroma-loc", "bottom"])


def test_argv_renders_chroma_loc_only_when_given():
    from lut_renderer_amd import pipe
    from lut_renderer_amd.command import engine_command
    info = VideoInfo(width=64, height=32, bit_depth=10, pix_fmt="yuv420p10le", fps=25.0)
    base = engine_command(Path("in.yuv"), Path("out.yuv"), ProcessingParams(), Path("x.cube"), info, python_bin="py")
    assert "--chroma-loc" not in base
    for loc in twin.LOCS:
        cmd = engine_command(Path("in.yuv"), Path("out.yuv"), ProcessingParams(), Path("x.cube"), info, python_bin="py",
                             chroma_loc=loc)
        assert cmd[:len(base)] == base and cmd[len(base):] == ["--chroma-loc", loc]
        sc = pipe.engine_stage_commands(Path("in.mov"), Path("out.mov"), ProcessingParams(video_codec="libx265"), Path("x.cube"),
                                        info, chroma_loc=loc)
        assert sc.engine[sc.engine.index("--chroma-loc") + 1] == loc
        assert sc.encoder[sc.encoder.index("-chroma_sample_location") + 1] == loc and sc.encoder[-1] == "out.mov"
    sc = pipe.engine_stage_commands(Path("in.mov"), Path("out.mov"), ProcessingParams(video_codec="libx265"), Path("x.cube"), info)
    assert "--chroma-loc" not in sc.engine and "-chroma_sample_location" not in sc.encoder
    with pytest.raises(ValueError):
        engine_command(Path("a"), Path("b"), ProcessingParams(), Path("x.cube"), info, chroma_loc="bottom")


# ------------------------------------------------------------------ GPU
def _dev(planes, device):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to(device)
            for p in planes]


def _host(tensors, dout):
    return [t.cpu().numpy().view(np.uint16) if dout > 8 else t.cpu().numpy() for t in tensors]


def _fmt(depth, lay):
    return f"yuv{lay}p" + ("" if depth == 8 else f"{depth}le")


def _edges(w, h, depth, csx, csy, k):
    """Saturated chroma edges (skin against sky, titles): blocks of extreme chroma codes over a luma ramp."""
    rng = np.random.default_rng(100 + k)
    s = 1 << (depth - 8)
    ch, cw = frames.chroma_shape(w, h, csx, csy)
    dt = np.uint8 if depth == 8 else np.uint16
    y = (16 * s + (np.arange(w)[None, :] * 7 + np.arange(h)[:, None] * 3) % (219 * s)).astype(dt)
    lv = np.array([16 * s, 240 * s, 128 * s, 60 * s], np.int64)
    cb = lv[rng.integers(0, 4, size=(ch // 3 + 1, cw // 3 + 1))].repeat(3, 0).repeat(3, 1)[:ch, :cw].astype(dt)
    cr = lv[rng.integers(0, 4, size=(ch // 3 + 1, cw // 3 + 1))].repeat(3, 0).repeat(3, 1)[:ch, :cw].astype(dt)
    return [y, cb, cr]


def _content(kind, w, h, depth, csx, csy, k=0):
    if kind == "edges":
        return _edges(w, h, depth, csx, csy, k)
    return frames.make_yuv("natural" if kind == "natural" else "noise16", w, h, depth, csx, csy, k=k)


def _want(lut, mode, loc, din, dl, dout, csx, csy, src, rs="tv", rin="tv", prelut=None):
    k = twin.consts("bt709", rin, "bt709", "tv", din, dl, dout, csx, csy, loc, prologue=(rs == "pc"))
    return twin.apply_yuv(lut.table, lut.scale, mode, k, din, dl, dout, csx, csy, loc, src, prelut=prelut)


def _eq(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


_DEPTHS = ((8, 8, 8), (10, 10, 10), (10, 10, 8), (8, 8, 10), (16, 16, 16))
_LUTS = ("identity_17.cube", "log709_33.cube", "random_9.cube", "domain_2.cube")


@pytest.mark.gpu
@pytest.mark.parametrize("loc", twin.LOCS)
@pytest.mark.parametrize("lay", tuple(LAYOUTS))
def test_parity_matrix(engine, cube_dir, loc, lay):
    csx, csy = LAYOUTS[lay]
    for w, h in ((72, 38), (70, 37)):
        _parity_size(engine, cube_dir, loc, lay, csx, csy, w, h)


def _kernel_for(w, din, dout, mode, lay):
    """The instance the launcher must pick for a dense frame: the vector one for equal widths, w % 4 == 0 and the 4-tap /
    nearest modes; the scalar one otherwise (4:4:4 runs lutr_apply_yuv's kernels)."""
    if lay == "444":
        return None
    vec = w % 4 == 0 and din == dout and mode in ("nearest", "trilinear", "tetrahedral")
    return "k_yuv_sited_vec<" if vec else "k_yuv_sited<"


def _parity_size(engine, cube_dir, loc, lay, csx, csy, w, h):
    for lname in _LUTS:
        lut = engine.load_cube(cube_dir / lname)
        for din, dl, dout in _DEPTHS:
            for ci, kind in enumerate(("natural", "noise", "edges")):
                src = _content(kind, w, h, din, csx, csy, k=ci)
                dev = _dev(src, engine.device)
                for mode in ("nearest", "trilinear", "tetrahedral", "pyramid", "prism"):
                    out = engine.apply_yuv(dev, pix_fmt=_fmt(din, lay), out_pix_fmt=_fmt(dout, lay), interp=mode, chroma_loc=loc)
                    got = _host(out, dout)
                    want = _want(lut, mode, loc, din, dl, dout, csx, csy, src)
                    assert _eq(got, want), (w, h, lname, din, dout, kind, mode, engine.last_kernel)
                    want_k = _kernel_for(w, din, dout, mode, lay)
                    assert want_k is None or engine.last_kernel.startswith(want_k), (w, din, dout, mode, engine.last_kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("loc", twin.LOCS)
def test_awkward_sizes_strides_and_batches(engine, cube_dir, loc):
    import torch
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for lay in ("420", "422"):
        csx, csy = LAYOUTS[lay]
        for w, h in ((1, 1), (2, 2), (3, 5), (5, 3), (33, 17), (127, 9), (130, 67), (300, 4)):
            src = frames.natural_yuv(w, h, 10, csx, csy, k=w + h)
            out = engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(10, lay), chroma_loc=loc)
            assert _eq(_host(out, 10), _want(lut, "tetrahedral", loc, 10, 10, 10, csx, csy, src)), (lay, w, h)
            assert engine.last_kernel.startswith(_kernel_for(w, 10, 10, "tetrahedral", lay)), (w, engine.last_kernel)
        # padded rows on both sides (views into wider buffers), 8-bit: odd pads (scalar instance) and 4-byte pads (vector)
        for w, h, ps, pd in ((45, 23, 13, 7), (64, 23, 4, 12), (64, 22, 5, 4)):
            src = frames.natural_yuv(w, h, 8, csx, csy, k=9)
            pad_s = [torch.zeros((p.shape[0], p.shape[1] + ps), dtype=torch.uint8, device=engine.device) for p in src]
            pad_d = [torch.zeros((p.shape[0], p.shape[1] + pd), dtype=torch.uint8, device=engine.device) for p in src]
            for t, p in zip(pad_s, src):
                t[:, :p.shape[1]] = torch.from_numpy(p).to(engine.device)
            sv = [t[:, :p.shape[1]] for t, p in zip(pad_s, src)]
            dv = [t[:, :p.shape[1]] for t, p in zip(pad_d, src)]
            engine.apply_yuv(sv, dv, pix_fmt=_fmt(8, lay), interp="trilinear", chroma_loc=loc)
            assert _eq([t.cpu().numpy() for t in dv], _want(lut, "trilinear", loc, 8, 8, 8, csx, csy, src)), (lay, w, ps, pd)
            aligned = w % 4 == 0 and ps % 4 == 0 and pd % 4 == 0
            assert engine.last_kernel.startswith("k_yuv_sited_vec<" if aligned else "k_yuv_sited<"), engine.last_kernel
        # batches of frames, unaligned and aligned widths
        for w in (66, 68):
            fr = [frames.natural_yuv(w, 34, 10, csx, csy, k=20 + i) for i in range(3)]
            dev = [torch.stack([_dev(f, engine.device)[c] for f in fr]) for c in range(3)]
            out = engine.apply_yuv(dev, pix_fmt=_fmt(10, lay), chroma_loc=loc)
            assert engine.last_kernel.startswith(_kernel_for(w, 10, 10, "tetrahedral", lay)), engine.last_kernel
            for i, f in enumerate(fr):
                assert _eq(_host([o[i] for o in out], 10), _want(lut, "tetrahedral", loc, 10, 10, 10, csx, csy, f)), (lay, w, i)


@pytest.mark.gpu
def test_negative_strides_through_the_c_abi(engine, cube_dir):
    """Bottom-up planes (negative linesize, FFmpeg's vflip layout) straight through lutr_apply_yuv_sited."""
    import torch
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 36, 21                     # an aligned width: the negative strides alone send it to the scalar instance
    src = frames.natural_yuv(w, h, 10, 1, 1, k=4)
    flipped = [np.ascontiguousarray(p[::-1]) for p in src]
    ds = _dev(flipped, engine.device)
    dd = [torch.zeros_like(t) for t in ds]
    s, d = _native.Planes(), _native.Planes()
    for i in range(3):
        rows, row_bytes = ds[i].shape[0], ds[i].stride(0) * 2
        s.data[i] = ds[i].data_ptr() + (rows - 1) * row_bytes
        d.data[i] = dd[i].data_ptr() + (rows - 1) * row_bytes
        s.stride[i] = d.stride[i] = -row_bytes
    p = _native.YuvParams(_native.fmt_code(10, 1, 1), _native.fmt_code(10, 1, 1), 10, 0, 0, 0, 0, 0)
    for loc in twin.LOCS:
        with engine._lock:
            engine._bind_stream()
            _native.check(engine._lib.lutr_apply_yuv_sited(engine._ctx, C.byref(p), 2, _native.CHROMA_LOC[loc], w, h, 1,
                                                           C.byref(s), C.byref(d), 0, h))
        got = [a[::-1] for a in _host(dd, 10)]
        assert _eq(got, _want(lut, "tetrahedral", loc, 10, 10, 10, 1, 1, src)), loc
        assert engine.last_kernel.startswith("k_yuv_sited<"), engine.last_kernel


@pytest.mark.gpu
def test_prologue_and_prelut(engine, cube_dir, tmp_path):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for loc in twin.LOCS:
        for din, lay in ((8, "420"), (10, "422"), (10, "420")):
            csx, csy = LAYOUTS[lay]
            src = frames.uniform_yuv(50 if din == 8 else 52, 26, din, csx, csy, k=din, full_range=True)
            out = engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(din, lay), out_pix_fmt=_fmt(8, lay), range_src="pc",
                                   range_in="tv", lut_depth=8, interp="trilinear", chroma_loc=loc)
            want = _want(lut, "trilinear", loc, din, 8, 8, csx, csy, src, rs="pc", rin="tv")
            assert _eq(_host(out, 8), want), (loc, din, lay)
    tab = cube.log709_lattice(17)
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, tab, shapers)
    lut = engine.load_cube(p)
    assert lut.prelut is not None
    from oracle import binding as orc
    pre = orc.parse_lut_file_ex(p)[3]
    for loc in twin.LOCS:
        src = frames.natural_yuv(46 if loc == "center" else 48, 30, 10, 1, 1, k=2)
        for mode in ("tetrahedral", "prism"):
            out = engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le", interp=mode, chroma_loc=loc)
            assert _eq(_host(out, 10), _want(lut, mode, loc, 10, 10, 10, 1, 1, src, prelut=pre)), (loc, mode)


@pytest.mark.gpu
def test_row_shards_and_group(engine, cube_dir):
    import torch
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for lay in ("420", "422"):
        csx, csy = LAYOUTS[lay]
        w, h = (54, 23) if lay == "420" else (56, 23)
        src = frames.natural_yuv(w, h, 10, csx, csy, k=8)
        dev = _dev(src, engine.device)
        for loc in twin.LOCS:
            whole = _host(engine.apply_yuv(dev, pix_fmt=_fmt(10, lay), chroma_loc=loc), 10)
            assert _eq(whole, _want(lut, "tetrahedral", loc, 10, 10, 10, csx, csy, src))
            for r0 in range(2, h, 2):
                dst = [torch.full_like(t, 0) for t in dev]
                engine.apply_yuv(dev, dst, pix_fmt=_fmt(10, lay), chroma_loc=loc, row0=0, rows=r0)
                engine.apply_yuv(dev, dst, pix_fmt=_fmt(10, lay), chroma_loc=loc, row0=r0, rows=h - r0)
                assert _eq(_host(dst, 10), whole), (lay, loc, r0)
            with LutEngineGroup([0, 0], treat_as_remote=True) as g:
                g.set_lut(lut)
                got = _host(g.apply_yuv(dev, pix_fmt=_fmt(10, lay), chroma_loc=loc), 10)
                assert g.last_remote == 1 and _eq(got, whole), (lay, loc)
            with LutEngineGroup([0, 0, 0], treat_as_remote=True) as g:
                g.set_lut(lut)
                assert _eq(_host(g.apply_yuv(dev, pix_fmt=_fmt(10, lay), chroma_loc=loc), 10), whole), (lay, loc)


@pytest.mark.gpu
def test_whole_uhd_frame(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    src = frames.natural_yuv(3840, 2160, 10, 1, 1, k=1)
    dev = _dev(src, engine.device)
    for loc in ("left", "topleft"):
        got = _host(engine.apply_yuv(dev, pix_fmt="yuv420p10le", chroma_loc=loc), 10)
        assert engine.last_kernel == f"k_yuv_sited_vec<16,420,{loc},2>", engine.last_kernel
        want = _want(lut, "tetrahedral", loc, 10, 10, 10, 1, 1, src)
        for r in range(0, 2160, 270):          # strips, so that a failure names where
            assert np.array_equal(got[0][r:r + 270], want[0][r:r + 270]), (loc, r)
            assert np.array_equal(got[1][r // 2:(r + 270) // 2], want[1][r // 2:(r + 270) // 2]), (loc, r)
            assert np.array_equal(got[2][r // 2:(r + 270) // 2], want[2][r // 2:(r + 270) // 2]), (loc, r)


@pytest.mark.gpu
def test_fast_precision_gives_strict_bits(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    src = frames.natural_yuv(128, 64, 10, 1, 1, k=6)
    dev = _dev(src, engine.device)
    try:
        for prec in ("fast", "fma32"):
            engine.set_precision(prec)
            for loc in twin.LOCS:
                out = engine.apply_yuv(dev, pix_fmt="yuv420p10le", chroma_loc=loc)
                assert _eq(_host(out, 10), _want(lut, "tetrahedral", loc, 10, 10, 10, 1, 1, src)), (prec, loc)
                assert "fast" not in engine.last_kernel and "fma32" not in engine.last_kernel
    finally:
        engine.set_precision("strict")


@pytest.mark.gpu
def test_replicate_is_plain_apply_yuv_and_in_place_is_rejected(engine, cube_dir):
    import torch
    engine.load_cube(cube_dir / "log709_33.cube")
    for lay in ("420", "444"):
        csx, csy = LAYOUTS[lay]
        src = frames.natural_yuv(256, 64, 10, csx, csy, k=7)
        dev = _dev(src, engine.device)
        a = _host(engine.apply_yuv(dev, pix_fmt=_fmt(10, lay)), 10)
        ka = engine.last_kernel
        b = _host(engine.apply_yuv(dev, pix_fmt=_fmt(10, lay), chroma_loc=None), 10)
        assert _eq(a, b) and engine.last_kernel == ka
        if lay == "444":
            for loc in twin.LOCS:             # 4:4:4: every siting is replicate
                assert _eq(_host(engine.apply_yuv(dev, pix_fmt=_fmt(10, lay), chroma_loc=loc), 10), a)
                assert engine.last_kernel == ka
    src = frames.natural_yuv(64, 32, 10, 1, 1, k=7)
    dev = _dev(src, engine.device)
    for loc in twin.LOCS:
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv(dev, dev, pix_fmt="yuv420p10le", chroma_loc=loc)
        assert e.value.code == _native.EINVAL and "in place" in e.value.message
        swapped = [dev[0].clone(), dev[2], dev[1].clone()]         # a chroma plane written where the other is read
        with pytest.raises(_native.LutrError):
            engine.apply_yuv(dev, swapped, pix_fmt="yuv420p10le", chroma_loc=loc)
    with pytest.raises(ValueError):
        engine.apply_yuv(dev, pix_fmt="yuv420p10le", chroma_loc="left", dither="error_diffusion")
    with pytest.raises(ValueError):
        engine.apply_yuv(dev, pix_fmt="yuv420p10le", chroma_loc="bottom")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("w", (62, 64))
def test_cli_output_equals_the_twin(cube_dir, tmp_path, w):
    h, n = 34, 3
    src = [frames.natural_yuv(w, h, 10, 1, 1, k=30 + i) for i in range(n)]
    (tmp_path / "in.yuv").write_bytes(b"".join(p.tobytes() for f in src for p in f))
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for loc in twin.LOCS:
        out = tmp_path / f"out_{loc}.yuv"
        cmd = [sys.executable, "-m", "lut_renderer_amd.cli", "-y", "-i", str(tmp_path / "in.yuv"), "-o", str(out),
               "--size", f"{w}x{h}", "--pix-fmt", "yuv420p10le", "--cube", str(cube_dir / "log709_33.cube"),
               "--colorspace", "bt709", "--color-range", "tv", "--batch", "2", "--chroma-loc", loc]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        want = b"".join(p.tobytes() for f in src for p in _want(lut, "tetrahedral", loc, 10, 10, 10, 1, 1, f))
        assert out.read_bytes() == want, loc
