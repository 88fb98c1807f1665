"""Output resize: the engine's separable bicubic after the LUT, standing in for the reference's `-s WxH`.

CPU: the kernel function, the Q14 tables of lutr_resize_filter against the NumPy twin (tests/_resize_twin.py), the limits,
the integer pass by hand, and the argv / option plumbing.  GPU: lutr_resize_planes and the LUT + resize composition bit-exact
against the twin."""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _resize_twin as tw
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
LAYOUTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
LOCS = (None, "left", "center", "topleft")


# ------------------------------------------------------------------ CPU: kernel and tables
def test_kernel_values():
    assert tw.k(0.0) == 1.0
    assert tw.k(0.5) == pytest.approx(0.575, abs=1e-15)
    assert tw.k(-0.5) == tw.k(0.5)
    assert tw.k(1.5) == pytest.approx(-0.075, abs=1e-15)
    assert tw.k(1.0) == pytest.approx(0.0, abs=1e-15) and tw.k(2.0) == 0.0 and tw.k(2.5) == 0.0


def test_rows_sum_to_one_and_simple_shapes():
    for src, dst in ((3840, 1920), (1919, 1280), (1080, 2160), (7, 5), (100, 800), (800, 100)):
        for cs, co in ((0, False), (1, False), (1, True)):
            start, w = _native.resize_filter(src, dst, cs, co)
            assert (w.astype(np.int64).sum(1) == 16384).all(), (src, dst, cs, co)
            assert np.abs(w.astype(np.int64)).sum(1).max() <= 22118
    # identity: one tap of 16384 on the sample itself, for luma and both chroma sitings
    for cs, co in ((0, False), (1, False), (1, True)):
        start, w = _native.resize_filter(1920, 1920, cs, co)
        n_out = (1920 + cs) >> cs
        assert (w == 16384).sum(1).tolist() == [1] * n_out and (np.count_nonzero(w, axis=1) == 1).all()
        assert (start + np.argmax(w, axis=1) == np.arange(n_out)).all()
    # 2:1 luma: 8 symmetric taps around 2u + 1/2
    start, w = _native.resize_filter(3840, 1920)
    assert w.shape == (1920, 8)
    assert (w == w[:, ::-1]).all() and (start == 2 * np.arange(1920) - 3).all()
    assert tw.position(3840, 1920, 0, False, 5) == 10.5
    # 4:2:0 chroma at 2:1: interstitial is centred on 2j + 1/2 (symmetric), co-sited on 2j + 1/4 (not symmetric)
    s_i, w_i = _native.resize_filter(3840, 1920, 1, False)
    s_c, w_c = _native.resize_filter(3840, 1920, 1, True)
    assert tw.position(3840, 1920, 1, False, 7) == 14.5 and tw.position(3840, 1920, 1, True, 7) == 14.25
    assert (w_i == w_i[:, ::-1]).all()
    assert not (w_c == w_c[:, ::-1]).all()


@pytest.mark.parametrize("src,dst", [(3840, 1920), (3840, 1280), (3840, 720), (3840, 481), (1080, 2160), (1919, 1280),
                                     (1079, 719), (17, 5), (5, 17), (33, 33), (800, 100), (100, 1600), (8, 1), (1, 16),
                                     (1, 1), (2, 1)])
def test_library_tables_equal_the_twin(src, dst):
    for cs, co in ((0, False), (1, False), (1, True)):
        start, w = _native.resize_filter(src, dst, cs, co)
        t_start, t_w = tw.table(src, dst, cs, co)
        assert np.array_equal(start, t_start) and np.array_equal(w, t_w), (src, dst, cs, co)


def test_ratio_limits_are_rejected():
    for src, dst in ((801, 100), (100, 1601), (3840, 479), (1, 17), (0, 5), (5, 0)):
        with pytest.raises(_native.LutrError) as e:
            _native.resize_filter(src, dst)
        assert e.value.code == _native.EINVAL
        if src and dst:
            with pytest.raises(ValueError):
                tw.table(src, dst)
    with pytest.raises(_native.LutrError):
        _native.resize_filter(100, 50, 2, False)        # subsampling beyond 2:1
    assert _native.resize_filter(800, 100)[1].shape[1] == 32    # x8: the most taps
    assert _native.resize_filter(100, 1600)[1].shape[1] == 4


# ------------------------------------------------------------------ CPU: the integer pass
def test_identity_and_constant_planes():
    rng = np.random.default_rng(3)
    for depth in (8, 10, 12, 16):
        p = rng.integers(0, 1 << depth, size=(2, 9, 13)).astype(np.uint16)
        assert np.array_equal(tw.resize([p, p[:, :5, :7], p[:, :5, :7]], depth, 1, 1, (13, 9), (13, 9))[0], p)
        c = np.full((11, 17), (1 << depth) - 7, np.uint16)
        for size in ((5, 3), (40, 31), (17, 11)):
            out = tw.resize([c, c[:6, :9], c[:6, :9]], depth, 1, 1, (17, 11), size, "left")
            assert all((o == (1 << depth) - 7).all() for o in out), (depth, size)


def test_hand_computed_rows():
    """8 -> 4 and 4 -> 8 of one row (one row of height 1: the vertical pass is the identity), at 8 bit."""
    row = np.array([[0, 0, 0, 0, 255, 255, 255, 255]], np.uint16)
    # 8 -> 4: f = 2, stretch 2, 8 taps; output 1 sits at 2.5: taps 0..7 at distances -2.5 .. 4.5 scaled by 1/2
    raw = [tw.k((i - 2.5) / 2) for i in range(8)]
    q = [np.floor(v / sum(raw) * 16384 + 0.5) for v in raw]
    q[int(np.argmax(q))] += 16384 - sum(q)
    t = (int(sum(qq * s for qq, s in zip(q, row[0]))) + 32) >> 6          # d = 8: 2^(d-3), >> (d-2)
    v = 16384 * t
    want1 = min(255, max(0, (v + (1 << 21)) >> 22))
    out = tw.resize_plane(row, 8, tw.table(8, 4), tw.table(1, 1))
    assert out[0, 1] == want1
    assert out[0].tolist() == [0, want1, 255 - want1, 255]       # symmetric ramp
    # 4 -> 8: f = 1/2, 4 taps; output 1 sits at 0.25: weights k(-1.25) k(-0.25) k(0.75) k(1.75) on samples -1 (clamped) .. 2
    row = np.array([[0, 100, 200, 255]], np.uint16)
    raw = [tw.k(d) for d in (-1.25, -0.25, 0.75, 1.75)]
    q = [np.floor(v / sum(raw) * 16384 + 0.5) for v in raw]
    q[int(np.argmax(q))] += 16384 - sum(q)
    t = (int(q[0] * 0 + q[1] * 0 + q[2] * 100 + q[3] * 200) + 32) >> 6
    out = tw.resize_plane(row, 8, tw.table(4, 8), tw.table(1, 1))
    assert out[0, 1] == min(255, max(0, (16384 * t + (1 << 21)) >> 22))
    assert out[0, 0] <= out[0, 1] <= out[0, 2] and out.shape == (1, 8)


def test_16bit_checkerboard_stays_in_int32():
    """0 / 65535 checkerboard: the largest |v| the tables allow; resize_plane asserts int32 on every intermediate (in int64)."""
    cb = ((np.indices((64, 64)).sum(0) & 1) * 65535).astype(np.uint16)
    for src, dst in ((64, 8), (64, 1024), (64, 128), (64, 33), (64, 21)):
        tx = tw.table(src, dst)
        out = tw.resize_plane(cb, 16, tx, tx)
        assert out.dtype == np.uint16


# ------------------------------------------------------------------ CPU: argv and options
def _info():
    return VideoInfo(width=3840, height=2160, bit_depth=10, pix_fmt="yuv420p10le", fps=25.0, duration=2.0)


def test_engine_command_gpu_resize():
    from lut_renderer_amd.command import engine_command
    params = ProcessingParams(video_codec="libx265", pix_fmt="yuv420p10le", resolution="1920x1080")
    base = engine_command(Path("-"), Path("-"), params, Path("x.cube"), _info(), python_bin="py")
    assert base == engine_command(Path("-"), Path("-"), params, Path("x.cube"), _info(), python_bin="py", gpu_resize=False)
    cmd = engine_command(Path("-"), Path("-"), params, Path("x.cube"), _info(), python_bin="py", gpu_resize=True)
    assert cmd == base + ["--out-size", "1920x1080"]
    # no resolution: nothing to move
    plain = ProcessingParams(video_codec="libx265", pix_fmt="yuv420p10le")
    assert engine_command(Path("-"), Path("-"), plain, Path("x.cube"), _info(), python_bin="py", gpu_resize=True) == \
        engine_command(Path("-"), Path("-"), plain, Path("x.cube"), _info(), python_bin="py")
    with pytest.raises(ValueError):
        engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx264", pix_fmt="rgb24", resolution="1920x1080"),
                       Path("x.cube"), _info(), python_bin="py", gpu_resize=True)


def test_stage_commands_gpu_resize():
    from lut_renderer_amd import pipe
    params = ProcessingParams(video_codec="libx265", pix_fmt="yuv420p10le", resolution="1920x1080")
    a = pipe.engine_stage_commands(Path("in.mov"), Path("out.mov"), params, Path("x.cube"), _info(), python_bin="py")
    b = pipe.engine_stage_commands(Path("in.mov"), Path("out.mov"), params, Path("x.cube"), _info(), python_bin="py",
                                   gpu_resize=True)
    assert "--out-size" not in a.engine and a.engine == pipe.engine_stage_commands(
        Path("in.mov"), Path("out.mov"), params, Path("x.cube"), _info(), python_bin="py", gpu_resize=False).engine
    i = b.engine.index("--out-size")
    assert b.engine[i + 1] == "1920x1080" and b.engine[:i] + b.engine[i + 2:] == a.engine
    assert b.decoder == a.decoder
    # encoder: raw input -s is the target, the output -s is gone, everything else identical
    ia, ib = a.encoder.index("pipe:0"), b.encoder.index("pipe:0")
    assert a.encoder[a.encoder.index("-s")] == "-s" and a.encoder[a.encoder.index("-s") + 1] == "3840x2160"
    assert b.encoder[b.encoder.index("-s") + 1] == "1920x1080"
    assert a.encoder[ia:].count("-s") == 1 and b.encoder[ib:].count("-s") == 0
    ja = a.encoder.index("-s", ia)
    strip_a = a.encoder[:ja] + a.encoder[ja + 2:]
    strip_a[strip_a.index("-s") + 1] = "1920x1080"
    assert strip_a == b.encoder
    with pytest.raises(ValueError):
        pipe.engine_stage_commands(Path("in.mov"), Path("out.mov"),
                                   ProcessingParams(video_codec="libx264", pix_fmt="bgr24", resolution="1280x720"),
                                   Path("x.cube"), _info(), python_bin="py", gpu_resize=True)


def test_cli_parses_out_size():
    from lut_renderer_amd.cli import build_parser, plan_from_args
    args = build_parser().parse_args(["-i", "-", "-o", "-", "--size", "64x32", "--pix-fmt", "yuv420p10le", "--cube", "x.cube",
                                      "--out-size", "32x16"])
    assert args.out_size == "32x16"
    args.out_size = "32by16"
    with pytest.raises(ValueError):
        plan_from_args(args)


def test_apply_lut_resolution_checks_before_touching_a_device():
    from lut_renderer_amd.api import apply_lut

    class Plane:
        shape = (2160, 3840)

    planes = [Plane(), Plane(), Plane()]
    with pytest.raises(ValueError, match="single device"):
        apply_lut(planes, cube=None, pix_fmt="yuv420p10le", resolution="1920x1080", devices=(0, 1))
    for bad in ("1920:1080", "1920x", "x1080", "0x1080", (1920, 1080)):
        with pytest.raises(ValueError):
            apply_lut(planes, cube=None, pix_fmt="yuv420p10le", resolution=bad)


def test_parse_size_and_packed_resize_names():
    from lut_renderer_amd.engine import parse_pix_fmt, parse_size
    assert parse_size("1920x1080") == (1920, 1080) and parse_size((3, 2)) == (3, 2)
    for bad in ("1920X1080", "1920x1080x3", "-1x5", ""):
        with pytest.raises(ValueError):
            parse_size(bad)
    with pytest.raises(ValueError):
        parse_pix_fmt("rgb48le")


# ------------------------------------------------------------------ GPU
def _dev(planes, device):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p).view(np.int16 if p.dtype == np.uint16 else np.uint8)).to(device)
            for p in planes]


def _host(planes, depth):
    return [t.cpu().numpy().view(np.uint16 if depth > 8 else np.uint8) for t in planes]


def _eq(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _fmt(depth, lay):
    if lay == "gbrp":
        return "gbrp" if depth == 8 else f"gbrp{depth}le"
    return f"yuv{lay}p" if depth == 8 else f"yuv{lay}p{depth}le"


def _planes(lay, w, h, depth, k, nframes=1):
    rng = np.random.default_rng(100 + k)
    csx, csy = (0, 0) if lay == "gbrp" else LAYOUTS[lay]
    dt = np.uint8 if depth <= 8 else np.uint16
    shapes = [(h, w)] + [frames.chroma_shape(w, h, csx, csy)] * 2
    # smooth content plus noise plus hard edges: exercises negative lobes and the clamp
    out = []
    for (ph, pw) in shapes:
        yy, xx = np.mgrid[0:ph, 0:pw]
        base = ((np.sin(xx / 5.0 + k) + np.cos(yy / 3.0)) * 0.25 + 0.5) * ((1 << depth) - 1)
        base[:, pw // 3: pw // 3 + 3] = (1 << depth) - 1
        base[ph // 2, :] = 0
        p = np.clip(base + rng.normal(0, (1 << depth) / 64, size=(nframes, ph, pw)), 0, (1 << depth) - 1)
        out.append(p.astype(dt) if nframes > 1 else p[0].astype(dt))
    return out


_GEOMS = ((64, 36, 32, 18), (70, 37, 27, 19), (1919 // 16, 1079 // 16, 1280 // 16, 719 // 16), (41, 23, 82, 47),
          (96, 48, 12, 6), (12, 6, 192, 96), (33, 17, 33, 17))


@pytest.mark.gpu
@pytest.mark.parametrize("lay", ("420", "422", "444", "gbrp"))
@pytest.mark.parametrize("depth", (8, 10, 12, 16))
def test_resize_planes_equal_the_twin(engine, lay, depth):
    csx, csy = (0, 0) if lay == "gbrp" else LAYOUTS[lay]
    for gi, (sw, sh, dw, dh) in enumerate(_GEOMS):
        src = _planes(lay, sw, sh, depth, gi)
        for loc in (LOCS if lay in ("420", "422") else (None,)):
            got = _host(engine.resize(_dev(src, engine.device), pix_fmt=_fmt(depth, lay), size=(dw, dh), chroma_loc=loc), depth)
            want = tw.resize(src, depth, csx, csy, (sw, sh), (dw, dh), loc)
            assert _eq(got, want), (lay, depth, (sw, sh, dw, dh), loc)
    assert engine.last_kernel == ("k_resize<8>" if depth == 8 else "k_resize<16>")


@pytest.mark.gpu
def test_resize_batch_with_padded_strides(engine):
    import torch
    sw, sh, dw, dh, nf = 150, 84, 1280 // 8, 720 // 8, 5
    src = _planes("420", sw, sh, 10, 7, nframes=nf)
    dev = []
    for p in src:                        # padded rows and padded frames
        buf = torch.zeros((nf, p.shape[1] + 3, p.shape[2] + 10), dtype=torch.int16, device=engine.device)
        view = buf[:, 1:1 + p.shape[1], 2:2 + p.shape[2]]
        view.copy_(torch.from_numpy(p.view(np.int16)))
        dev.append(view)
    dst = []
    for i in range(3):
        ph, pw = (dh, dw) if i == 0 else frames.chroma_shape(dw, dh, 1, 1)
        big = torch.full((nf, ph + 2, pw + 6), -1, dtype=torch.int16, device=engine.device)
        dst.append(big[:, 1:1 + ph, 3:3 + pw])
    engine.resize(dev, dst, pix_fmt="yuv420p10le", size=f"{dw}x{dh}", chroma_loc="left")
    want = tw.resize(src, 10, 1, 1, (sw, sh), (dw, dh), "left")
    assert _eq(_host(dst, 10), want)
    for d in dst:                         # padding untouched
        base = d._base if d._base is not None else d
        b = base.cpu().numpy()
        assert (b[:, 0] == -1).all() and (b[:, :, :3] == -1).all()


@pytest.mark.gpu
def test_ratio_edges_and_identity_copy(engine):
    for sw, sh, dw, dh in ((256, 64, 32, 8), (16, 8, 256, 128)):
        src = _planes("420", sw, sh, 10, 1)
        got = _host(engine.resize(_dev(src, engine.device), pix_fmt="yuv420p10le", size=(dw, dh)), 10)
        assert _eq(got, tw.resize(src, 10, 1, 1, (sw, sh), (dw, dh)))
    for depth in (8, 16):
        src = _planes("422", 77, 31, depth, 2)
        got = _host(engine.resize(_dev(src, engine.device), pix_fmt=_fmt(depth, "422"), size=(77, 31), chroma_loc="left"), depth)
        assert all(g.tobytes() == s.tobytes() for g, s in zip(got, src))
    with pytest.raises(_native.LutrError):
        engine.resize(_dev(_planes("420", 257, 64, 10, 1), engine.device), pix_fmt="yuv420p10le", size=(32, 8))
    with pytest.raises(_native.LutrError):
        engine.resize(_dev(_planes("420", 16, 8, 10, 1), engine.device), pix_fmt="yuv420p10le", size=(257, 8))


def _resized(engine, out, fmt_out, size, loc=None):
    f = _fmt_parse(fmt_out)
    h, w = out[0].shape[-2], out[0].shape[-1]
    return tw.resize(_host(out, f.depth), f.depth, f.csx, f.csy, (w, h), size, loc)


def _fmt_parse(name):
    from lut_renderer_amd.engine import parse_pix_fmt
    return parse_pix_fmt(name)


@pytest.mark.gpu
def test_apply_yuv_out_size_equals_twin_of_apply_yuv(engine, cube_dir, tmp_path):
    engine.load_cube(cube_dir / "log709_33.cube")
    src = frames.natural_yuv(96, 54, 10, 1, 1, k=4)
    dev = _dev(src, engine.device)
    cases = [dict(), dict(out_pix_fmt="yuv420p"), dict(dither="error_diffusion"), dict(chroma_loc="left"),
             dict(interp="trilinear", chroma_loc="topleft")]
    for size in ((48, 27), (160, 90)):
        for kw in cases:
            for prec in ("strict", "fma32"):
                engine.set_precision(prec)
                try:
                    full = engine.apply_yuv(dev, pix_fmt="yuv420p10le", **kw)
                    got = engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_size=size, **kw)
                finally:
                    engine.set_precision("strict")
                fo = kw.get("out_pix_fmt", "yuv420p10le")
                want = _resized(engine, full, fo, size, kw.get("chroma_loc"))
                assert _eq(_host(got, _fmt_parse(fo).depth), want), (size, kw, prec)
                assert engine.last_kernel.startswith("k_resize<")
    # a cineSpace prelut
    tab = cube.log709_lattice(17)
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 3
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, tab, shapers)
    lut = engine.load_cube(p)
    assert lut.prelut is not None
    full = engine.apply_yuv(dev, pix_fmt="yuv420p10le")
    got = engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_size="64x36")
    assert _eq(_host(got, 10), _resized(engine, full, "yuv420p10le", (64, 36)))
    # planar RGB
    engine.load_cube(cube_dir / "log709_33.cube")
    g = _dev(frames.natural_rgb(70, 40, 10, k=2), engine.device)
    full = engine.apply_rgb(g, depth=10)
    got = engine.apply_rgb(g, depth=10, out_size=(35, 20))
    assert _eq(_host(got, 10), tw.resize(_host(full, 10), 10, 0, 0, (70, 40), (35, 20)))


@pytest.mark.gpu
def test_every_chunk_size_gives_the_same_bytes(engine, cube_dir):
    engine.load_cube(cube_dir / "log709_33.cube")
    src = [np.stack(p) for p in zip(*[frames.natural_yuv(128, 72, 10, 1, 1, k=20 + i) for i in range(7)])]
    dev = _dev(src, engine.device)
    outs = [_host(engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_size=(64, 36), resize_chunk=c), 10) for c in (1, 3, 4, 16)]
    full = engine.apply_yuv(dev, pix_fmt="yuv420p10le")
    want = _resized(engine, full, "yuv420p10le", (64, 36))
    for o in outs:
        assert _eq(o, want)


@pytest.mark.gpu
def test_apply_lut_resolution(cube_dir):
    import torch
    from lut_renderer_amd.api import apply_lut
    src = frames.natural_yuv(96, 54, 10, 1, 1, k=9)
    dev = _dev(src, torch.device("cuda", 0))
    kw = dict(cube=cube_dir / "log709_33.cube", pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv")
    full, _ = apply_lut(dev, **kw)
    got, _ = apply_lut(dev, resolution="48x26", **kw)
    assert tuple(got[0].shape) == (26, 48) and tuple(got[1].shape) == (13, 24)
    assert _eq(_host(got, 10), tw.resize(_host(full, 10), 10, 1, 1, (96, 54), (48, 26)))


@pytest.mark.gpu
def test_host_pipeline_and_cli_out_size(engine, cube_dir, tmp_path):
    from lut_renderer_amd.stream import HostPipeline
    w, h, n, size = 64, 34, 5, (40, 22)
    src = [frames.natural_yuv(w, h, 10, 1, 1, k=40 + i) for i in range(n)]
    raw = b"".join(p.tobytes() for f in src for p in f)
    engine.load_cube(cube_dir / "log709_33.cube")
    want = b""
    for f in src:
        full = engine.apply_yuv(_dev(f, engine.device), pix_fmt="yuv420p10le", matrix_in="bt709")
        want += b"".join(p.tobytes() for p in _resized(engine, full, "yuv420p10le", size))
    pipe = HostPipeline(engine, "yuv420p10le", w, h, batch=2, out_size=size, matrix_in="bt709", matrix_out="bt709")
    assert pipe.fout.width == 40 and pipe.fout.height == 22
    fb, got = pipe.fin.frame_bytes, []
    pos = {"i": 0}

    def fill(buf, m):
        k = min(m, n - pos["i"])
        buf[: k * fb] = np.frombuffer(raw[pos["i"] * fb:(pos["i"] + k) * fb], np.uint8)
        pos["i"] += k
        return k

    pipe.run(fill, lambda buf, m: got.append(bytes(buf)))
    assert b"".join(got) == want
    out = tmp_path / "out.yuv"
    cmd = [sys.executable, "-m", "lut_renderer_amd.cli", "-y", "-i", "-", "-o", "-", "--size", f"{w}x{h}",
           "--pix-fmt", "yuv420p10le", "--cube", str(cube_dir / "log709_33.cube"), "--colorspace", "bt709",
           "--color-range", "tv", "--batch", "2", "--out-size", "40x22", "--duration", str(n / 25)]
    r = subprocess.run(cmd, input=raw, capture_output=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == want
    assert b"Duration:" in r.stderr and b"time=" in r.stderr
    out.write_bytes(r.stdout)


@pytest.mark.gpu
def test_resize_errors(engine, cube_dir):
    engine.load_cube(cube_dir / "log709_33.cube")
    dev = _dev(frames.natural_yuv(64, 32, 10, 1, 1, k=1), engine.device)
    with pytest.raises(ValueError, match="whole frames"):
        engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_size=(32, 16), row0=0, rows=16)
    with pytest.raises(ValueError, match="in place"):
        engine.apply_yuv(dev, dev, pix_fmt="yuv420p10le", out_size=(64, 32))
    with pytest.raises(ValueError, match="in place"):
        engine.resize(dev, dev, pix_fmt="yuv420p10le", size=(64, 32))
    with pytest.raises(ValueError):
        engine.resize(dev, pix_fmt="rgb48le", size=(32, 16))
    with pytest.raises(ValueError):
        engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_size="32*16")
