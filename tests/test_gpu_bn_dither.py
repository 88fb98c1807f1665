"""Blue-noise dither in the output stage on the GPU: bit for bit against the reference of tests/_bn_twin.py.

Frames of 136 x 132 and 139 x 131: more than two periods of the 64 x 64 mask wide and tall, so luma and both shifted chroma planes
cross the wrap in x and in y; the second size is ragged, so a call on padded rows is split between the vector kernel and the generic
one (where the union block is one row high: an odd height with a two-row block is all generic).  Two frames, padded strides."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from tests import _bn_twin as twin
from tests import _resize_twin as rz
from tests import _rgb2yuv_twin as r2y
from tests import _rgbf_twin as rgbf
from tests import _xsub_twin as xs
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
LAYOUTS = xs.LAYOUTS
PAIRS = [(a, b) for a in LAYOUTS for b in LAYOUTS]
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
SIZES = ((136, 132), (139, 131))
NF = 2


def _fmt(depth, lay):
    return f"yuv{lay}p" + ("" if depth == 8 else f"{depth}le")


def _np_dtype(depth):
    return np.uint16 if depth > 8 else np.uint8


def _padded(shapes, depth, device, fill=0):
    """[NF, h, w] views of padded buffers: rows of a multiple of 16 samples plus 16, one spare row per frame."""
    import torch
    bufs, views = [], []
    for h, w in shapes:
        pad = (w + 15) // 16 * 16 + 16
        t = torch.full((NF, h + 1, pad), fill, dtype=torch.int16 if depth > 8 else torch.uint8, device=device)
        bufs.append(t)
        views.append(t[:, :h, :w])
    return bufs, views


def _upload(fs, depth, device):
    """The frames `fs` (each Y, Cb, Cr on the host) as three padded [NF, h, w] device views."""
    import torch
    _, views = _padded([p.shape for p in fs[0]], depth, device)
    for i, v in enumerate(views):
        host = np.stack([f[i] for f in fs])
        v.copy_(torch.from_numpy(host.view(np.int16) if depth > 8 else host).to(device))
    return views


def _host(tensors, dout):
    return [t.cpu().numpy().view(np.uint16) if dout > 8 else t.cpu().numpy() for t in tensors]


def _eq(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


def _unit(din, dout):
    return 8 if (din > 8 and dout <= 8) or din <= 8 else 4


def _kernel(din, dout, a, b, mode, w, h):
    """The kernel an `auto` call on padded rows reports: the vector kernel when it takes at least the aligned part."""
    (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
    vec = mode in MODES[:3] and not (din <= 8 and dout > 8) and h % (1 << max(icsy, ocsy)) == 0 and w >= _unit(din, dout)
    if not vec:
        return "k_yuv_bn_generic"
    return f"k_yuv_bn_vec<{int(din > 8)},{int(dout > 8)},{icsx},{icsy},{ocsx},{ocsy},{MODES.index(mode)}>"


_sources = {}


def _frames(w, h, din, lay):
    """NF natural frames, made once per (size, depth, layout) and never modified."""
    key = (w, h, din, lay)
    if key not in _sources:
        _sources[key] = [frames.natural_yuv(w, h, din, *LAYOUTS[lay], k=7 + i + din) for i in range(NF)]
    return _sources[key]


def _want(lut, mode, din, dout, a, b, f, rin="tv", prologue=False, matrix="bt709", prelut=None, dl=None):
    (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
    dl = din if dl is None else dl
    k = xs.consts(matrix, rin, matrix, "tv", din, dl, dout, ocsx, ocsy, prologue=prologue)
    return twin.apply(lut.table, lut.scale, mode, k, dl, dout, icsx, icsy, ocsx, ocsy, f, prelut=prelut)


def _check(engine, lut, w, h, din, dout, a, b, mode, variants=("auto", "generic"), **kw):
    """One pair at one size through `variants`: kernel names, bits of both frames, nothing written past a row."""
    ocsx, ocsy = LAYOUTS[b]
    fs = _frames(w, h, din, a)
    dev = _upload(fs, din, engine.device)
    wants = [_want(lut, mode, din, dout, a, b, f, **kw) for f in fs]
    oshape = [(h, w)] + [frames.chroma_shape(w, h, ocsx, ocsy)] * 2
    for variant in variants:
        bufs, dst = _padded(oshape, dout, engine.device, fill=0x55)
        with _variant(engine, variant):
            engine.apply_yuv(dev, dst, pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(dout, b), interp=mode, dither="blue_noise",
                             lut_depth=kw.get("dl"), range_src="pc" if kw.get("prologue") else "tv", range_in="tv",
                             matrix_in=kw.get("matrix", "bt709"))
            name = engine.last_kernel
        assert name == ("k_yuv_bn_generic" if variant == "generic" else _kernel(din, dout, a, b, mode, w, h)), (variant, name)
        got = _host(dst, dout)
        for i, wnt in enumerate(wants):
            assert _eq([g[i] for g in got], wnt), (w, h, din, dout, a, b, mode, variant, i)
        assert all((g[:, :s[0], s[1]:] == 0x55).all() and (g[:, s[0]:] == 0x55).all() for g, s in zip(_host(bufs, dout), oshape))


# ------------------------------------------------------------------ parity
@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_nine_pairs_16_to_8_bit_tetrahedral(engine, cube_dir, size):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for a, b in PAIRS:
        _check(engine, lut, size[0], size[1], 10, 8, a, b, "tetrahedral")


@pytest.mark.gpu
@pytest.mark.parametrize("depths", ((8, 8), (10, 10), (10, 8)), ids=lambda d: f"{d[0]}to{d[1]}")
def test_containers_and_modes(engine, cube_dir, depths):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for a, b in (("420", "420"), ("420", "422"), ("444", "420")):
        for mode in ("nearest", "trilinear"):
            for w, h in SIZES:
                _check(engine, lut, w, h, depths[0], depths[1], a, b, mode)


@pytest.mark.gpu
def test_generic_only_modes_and_the_8_to_16_bit_mix(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for mode in ("pyramid", "prism"):
        for a, b in (("420", "420"), ("422", "444")):
            _check(engine, lut, 139, 131, 10, 8, a, b, mode, variants=("auto",))
    for a, b in (("420", "420"), ("444", "422")):
        _check(engine, lut, 136, 132, 8, 10, a, b, "tetrahedral", variants=("auto",))
        assert engine.last_kernel == "k_yuv_bn_generic"
    _check(engine, lut, 139, 131, 12, 9, "422", "420", "tetrahedral", variants=("auto",))       # any depth pair in 8..16


@pytest.mark.gpu
def test_full_range_prologue(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for a, b in (("420", "420"), ("422", "420")):
        for w, h in SIZES:
            _check(engine, lut, w, h, 10, 8, a, b, "tetrahedral", rin="tv", prologue=True, dl=8, matrix="smpte170m")


@pytest.mark.gpu
def test_prelut(engine, tmp_path):
    from oracle import binding as orc
    tab = cube.log709_lattice(17)
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, tab, shapers)
    lut = engine.load_cube(p)
    pre = orc.parse_lut_file_ex(p)[3]
    for a, b in (("420", "420"), ("444", "422")):
        _check(engine, lut, 139, 131, 10, 8, a, b, "tetrahedral", prelut=pre)
        _check(engine, lut, 136, 132, 10, 10, a, b, "trilinear", variants=("auto",), prelut=pre)


@pytest.mark.gpu
def test_variants(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    _check(engine, lut, 136, 132, 10, 8, "420", "420", "tetrahedral", variants=("vec_global",))
    dev = _upload(_frames(136, 132, 10, "420"), 10, engine.device)
    ragged = _upload(_frames(139, 131, 10, "444"), 10, engine.device)
    kw = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv420p", dither="blue_noise")
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv(dev, **kw)
        assert e.value.code == _native.EINVAL
    with _variant(engine, "vec_global"):
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv(ragged, pix_fmt="yuv444p10le", out_pix_fmt="yuv444p", dither="blue_noise")
        assert e.value.code == _native.EINVAL
        with pytest.raises(_native.LutrError):                 # pyramid has no vector kernel
            engine.apply_yuv(dev, interp="pyramid", **kw)
        with pytest.raises(_native.LutrError):                 # 8 -> 16 bit has none either
            engine.apply_yuv(_upload(_frames(136, 132, 8, "420"), 8, engine.device), pix_fmt="yuv420p", out_pix_fmt="yuv420p10le",
                             dither="blue_noise")
    with pytest.raises(ValueError, match="chroma_loc"):
        engine.apply_yuv(dev, chroma_loc="left", **kw)
    with pytest.raises(ValueError, match="unknown dither mode"):
        engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv420p", dither="ordered")


@pytest.mark.gpu
def test_whole_frame_entry_point_is_the_same_call(engine, cube_dir):
    """lutr_apply_yuv_dither with LUTR_DITHER_BLUE_NOISE: the rows [0, h) of lutr_apply_yuv_xsub, same kernel and bits."""
    import torch
    from lut_renderer_amd.engine import _planes_struct, parse_pix_fmt
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    fs = _frames(136, 132, 10, "420")
    dev = _upload(fs, 10, engine.device)
    _, dst = _padded([(132, 136), (66, 68), (66, 68)], 8, engine.device)
    fi, fo = parse_pix_fmt("yuv420p10le"), parse_pix_fmt("yuv420p")
    p = _native.YuvParams(fi.code, fo.code, 10, 0, 0, 0, 0, 0)
    s, nf = _planes_struct(dev, engine.device)
    d, _ = _planes_struct(dst, engine.device)
    with engine._lock:
        engine._bind_stream()
        assert engine._lib.lutr_apply_yuv_dither(engine._ctx, C.byref(p), 2, _native.DITHER["blue_noise"], 136, 132, nf, C.byref(s),
                                                 C.byref(d)) == 0
    torch.cuda.synchronize()
    assert engine.last_kernel == _kernel(10, 8, "420", "420", "tetrahedral", 136, 132)
    got = _host(dst, 8)
    for i, f in enumerate(fs):
        assert _eq([g[i] for g in got], _want(lut, "tetrahedral", 10, 8, "420", "420", f))


# ------------------------------------------------------------------ row shards
@pytest.mark.gpu
def test_row_shards_stitch_to_the_whole_frame(engine, cube_dir):
    engine.load_cube(cube_dir / "log709_33.cube")
    for (w, h), a, b, cuts in (((136, 132), "420", "420", (2, 64, 70, 128)), ((136, 132), "420", "422", (66,)),
                               ((139, 131), "444", "420", (62, 130)), ((139, 131), "422", "444", (1, 65, 127))):
        dev = _upload(_frames(w, h, 10, a), 10, engine.device)
        kw = dict(pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(8, b), dither="blue_noise")
        whole = _host(engine.apply_yuv(dev, **kw), 8)
        for r0 in cuts:
            out = engine.apply_yuv(dev, row0=0, rows=r0, **kw)
            engine.apply_yuv(dev, out, row0=r0, rows=h - r0, **kw)
            assert _eq(_host(out, 8), whole), (w, h, a, b, r0)
        out = engine.apply_yuv(dev, row0=cuts[0], rows=cuts[-1] - cuts[0], **kw)       # three shards, the middle one first
        engine.apply_yuv(dev, out, row0=0, rows=cuts[0], **kw)
        engine.apply_yuv(dev, out, row0=cuts[-1], rows=h - cuts[-1], **kw)
        assert _eq(_host(out, 8), whole), (w, h, a, b, "three")
    dev = _upload(_frames(136, 132, 10, "420"), 10, engine.device)
    with pytest.raises(_native.LutrError) as e:
        engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv420p", dither="blue_noise", row0=1, rows=131)
    assert e.value.code == _native.EINVAL and "union" in e.value.message
    # batches: one frame at a time gives the bits of the batch
    kw = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv420p", dither="blue_noise")
    whole = _host(engine.apply_yuv(dev, **kw), 8)
    for i in range(NF):
        one = _host(engine.apply_yuv([t[i] for t in dev], **kw), 8)
        assert _eq(one, [g[i] for g in whole]), i


# ------------------------------------------------------------------ group
@pytest.mark.gpu
def test_group_row_shards_equal_one_device(engine, cube_dir):
    """Two and three contexts on one GPU, every one after the first on the copy-there-and-back path: the slice that travels is
    anchored where the pattern starts over, so the stitched result is the one-device result."""
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    engine.set_lut(lut)
    for (w, h), a, b in (((136, 132), "420", "420"), ((139, 131), "420", "444"), ((136, 132), "444", "420")):
        fs = _frames(w, h, 10, a)
        dev = _upload(fs, 10, engine.device)
        kw = dict(pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(8, b), dither="blue_noise")
        one = _host(engine.apply_yuv(dev, **kw), 8)
        for i, f in enumerate(fs):
            assert _eq([g[i] for g in one], _want(lut, "tetrahedral", 10, 8, a, b, f))
        for n in (2, 3):
            with LutEngineGroup([0] * n, treat_as_remote=True) as g:
                g.set_lut(lut)
                got = _host(g.apply_yuv(dev, **kw), 8)
                g.sync()
                assert g.last_remote == n - 1 and all("k_yuv_bn" in k for k in g.last_kernels), g.last_kernels
                assert _eq(got, one), (w, h, a, b, n)
                with pytest.raises(ValueError, match="cannot be row-sharded"):
                    g.apply_yuv(dev, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(8, b), dither="error_diffusion")
    src = _rgb_source("rgb24", 72, 134, 5)
    kw = dict(pix_fmt="rgb24", out_pix_fmt="yuv444p", dither="blue_noise")
    one = _host(engine.apply_rgb_to_yuv(_t(src, engine.device), **kw), 8)
    with LutEngineGroup([0, 0], treat_as_remote=True) as g:
        g.set_lut(lut)
        got = _host(g.apply_rgb_to_yuv(_t(src, engine.device), **kw), 8)
        g.sync()
        assert g.last_remote == 1 and _eq(got, one)


# ------------------------------------------------------------------ other sources and paths
def _t(a, device):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def _rgb_source(pix_fmt, w, h, k):
    """gbrp planes (G, B, R) or one packed image [H, W, C] whose fourth component is noise (tests/test_gpu_rgb2yuv.make_source)."""
    dl = r2y.source_depth(pix_fmt)
    g, b, r = frames.make_rgb("natural", w, h, dl, k=k)
    if pix_fmt not in r2y.PACKED:
        return [g, b, r]
    _bits, nc, ro, go, bo = r2y.PACKED[pix_fmt]
    img = np.random.default_rng(1000 + k).integers(0, 1 << dl, size=(h, w, nc)).astype(g.dtype)
    img[..., ro], img[..., go], img[..., bo] = r, g, b
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("pix_fmt,w,h", [("gbrp10le", 136, 132), ("rgb24", 139, 131), ("rgba64le", 72, 70), ("gbrpf32le", 70, 67)])
def test_rgb_and_float_sources_to_yuv420p(engine, cube_dir, pix_fmt, w, h):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    if pix_fmt == "gbrpf32le":
        src = rgbf.make_float("natural", w, h, k=3)
        want = twin.apply_rgbf(lut.table, lut.scale, "tetrahedral", rgbf.consts("smpte170m", "tv", 8, 1, 1), 8, 1, 1, src)
        name = "k_rgbf2yuv_bn_generic"
    else:
        src = _rgb_source(pix_fmt, w, h, 3)
        k = r2y.consts("smpte170m", "tv", r2y.source_depth(pix_fmt), 8, 1, 1)
        want = twin.apply_rgb(lut.table, lut.scale, "tetrahedral", k, pix_fmt, 8, 1, 1, src)
        name = "k_rgb2yuv_bn_generic"
    dev = _t(src, engine.device) if isinstance(src, np.ndarray) else [_t(p, engine.device) for p in src]
    kw = dict(pix_fmt=pix_fmt, out_pix_fmt="yuv420p", dither="blue_noise")
    for variant in ("auto", "generic"):
        with _variant(engine, variant):
            got = _host(engine.apply_rgb_to_yuv(dev, **kw), 8)
            assert engine.last_kernel == name
        assert _eq(got, want), (pix_fmt, variant)
    for variant in ("vec_global", "vec_lds"):                    # no vector kernel for these sources yet
        with _variant(engine, variant):
            with pytest.raises(_native.LutrError) as e:
                engine.apply_rgb_to_yuv(dev, **kw)
            assert e.value.code == _native.EINVAL
    r0 = 66
    out = engine.apply_rgb_to_yuv(dev, row0=0, rows=r0, **kw)
    engine.apply_rgb_to_yuv(dev, out, row0=r0, rows=h - r0, **kw)
    assert _eq(_host(out, 8), want), (pix_fmt, "shards")


@pytest.mark.gpu
def test_apply_lut_and_the_cli_over_a_pipe(engine, cube_dir):
    from lut_renderer_amd.api import apply_lut
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    w, h = 72, 66
    fs = [frames.natural_yuv(w, h, 10, 1, 1, k=30 + i) for i in range(3)]
    wants = [_want(lut, "tetrahedral", 10, 8, "420", "420", f) for f in fs]
    got, _ = apply_lut([_t(p, engine.device) for p in fs[0]], cube=lut, pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv",
                       out_pix_fmt="yuv420p", engine=engine, engine_dither="blue_noise")
    assert _eq(_host(got, 8), wants[0]) and engine.last_kernel.startswith("k_yuv_bn_")
    cmd = [sys.executable, "-m", "lut_renderer_amd.cli", "-i", "-", "-o", "-", "--size", f"{w}x{h}", "--pix-fmt", "yuv420p10le",
           "--out-pix-fmt", "yuv420p", "--cube", str(cube_dir / "log709_33.cube"), "--colorspace", "bt709", "--color-range", "tv",
           "--engine-dither", "blue_noise", "--duration", "0.12", "--batch", "2"]
    r = subprocess.run(cmd, input=b"".join(p.tobytes() for f in fs for p in f), capture_output=True, cwd=ROOT, timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == b"".join(p.tobytes() for wnt in wants for p in wnt)


@pytest.mark.gpu
def test_out_size_runs_after_the_dither(engine, cube_dir):
    import torch
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 72, 68
    fs = [frames.natural_yuv(w, h, 10, 1, 1, k=40 + i) for i in range(3)]
    dev = [torch.stack([_t(f[i], engine.device) for f in fs]) for i in range(3)]
    got = _host(engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv420p", dither="blue_noise", out_size=(48, 40),
                                 resize_chunk=2), 8)
    for i, f in enumerate(fs):
        want = rz.resize(_want(lut, "tetrahedral", 10, 8, "420", "420", f), 8, 1, 1, (w, h), (48, 40))
        assert _eq([g[i] for g in got], want), i


# ------------------------------------------------------------------ what must not have changed
@pytest.mark.gpu
def test_error_diffusion_and_no_dither_are_what_they_were(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for (w, h), a, b in (((136, 132), "420", "420"), ((139, 131), "420", "422")):
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        fs = _frames(w, h, 10, a)
        dev = _upload(fs, 10, engine.device)
        k = xs.consts("bt709", "tv", "bt709", "tv", 10, 10, 8, ocsx, ocsy)
        for dither, fn in (("error_diffusion", xs.apply_dither), ("none", xs.apply)):
            got = _host(engine.apply_yuv(dev, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(8, b), dither=dither), 8)
            name = engine.last_kernel
            assert "bn" not in name and (name == "k_yuv_float+k_dither_ed") == (dither == "error_diffusion"), name
            for i, f in enumerate(fs):
                want = fn(lut.table, lut.scale, "tetrahedral", k, 10, 8, icsx, icsy, ocsx, ocsy, f)
                assert _eq([g[i] for g in got], want), (w, h, a, b, dither, i)
        with pytest.raises(ValueError, match="whole frames only"):
            engine.apply_yuv(dev, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(8, b), dither="error_diffusion", row0=0, rows=64)
