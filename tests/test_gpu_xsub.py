"""Chroma subsampling change inside the fused YUV pass on the GPU: lutr_apply_yuv_xsub bit-exact against the
reference composition of tests/_xsub_twin.py (stage 1 at the input layout, the C oracle's lut3d, stage 3 at the output layout)."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _resize_twin as rz
from tests import _xsub_twin as twin
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
DEPTHS = ((8, 8), (10, 10), (10, 8), (12, 12))


def _fmt(depth, lay):
    return f"yuv{lay}p" + ("" if depth == 8 else f"{depth}le")


def _dev(planes, device):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to(device)
            for p in planes]


def _host(tensors, dout):
    return [t.cpu().numpy().view(np.uint16) if dout > 8 else t.cpu().numpy() for t in tensors]


def _eq(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _want(lut, mode, din, dl, dout, a, b, src, rin="tv", prologue=False, matrix="bt709", prelut=None, dither=False):
    (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
    k = twin.consts(matrix, rin, matrix, "tv", din, dl, dout, ocsx, ocsy, prologue=prologue)
    fn = twin.apply_dither if dither else twin.apply
    return fn(lut.table, lut.scale, mode, k, dl, dout, icsx, icsy, ocsx, ocsy, src, prelut=prelut)


def _vec_name(din, dout, a, b, mode):
    (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
    return f"k_yuv_xsub_vec<{int(din > 8)},{int(dout > 8)},{icsx},{icsy},{ocsx},{ocsy},{MODES.index(mode)}>"


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


# ------------------------------------------------------------------ layouts, depths, modes and routing
@pytest.mark.gpu
@pytest.mark.parametrize("pair", twin.CROSS_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_cross_pairs_all_depths_and_modes(engine, cube_dir, pair):
    a, b = pair
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 64, 32
    for din, dout in DEPTHS:
        src = frames.natural_yuv(w, h, din, *LAYOUTS[a], k=din + dout)
        dev = _dev(src, engine.device)
        for mode in MODES:
            want = _want(lut, mode, din, din, dout, a, b, src)
            with _variant(engine, "generic"):
                got = _host(engine.apply_yuv(dev, pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(dout, b), interp=mode), dout)
                assert engine.last_kernel == "k_yuv_xsub_generic"
            assert _eq(got, want), (pair, din, dout, mode, "generic")
            if mode not in VEC_MODES:
                continue
            for variant in ("auto", "vec_global"):
                with _variant(engine, variant):
                    got = _host(engine.apply_yuv(dev, pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(dout, b), interp=mode), dout)
                    assert engine.last_kernel == _vec_name(din, dout, a, b, mode), (variant, engine.last_kernel)
                assert _eq(got, want), (pair, din, dout, mode, variant)


@pytest.mark.gpu
def test_other_luts_and_the_8_to_16_bit_mix(engine, cube_dir):
    """Lattices that clip and leave the [0, 1] range; an 8-bit source written as 10 bit (no vector kernel: generic)."""
    for name in ("random_9.cube", "domain_2.cube", "identity_17.cube"):
        lut = engine.load_cube(cube_dir / name)
        for a, b in twin.CROSS_PAIRS:
            src = frames.make_yuv("noise16", 48, 20, 10, *LAYOUTS[a], k=2)
            got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b)), 10)
            assert _eq(got, _want(lut, "tetrahedral", 10, 10, 10, a, b, src)), (name, a, b)
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for a, b in (("420", "422"), ("444", "420")):
        src = frames.natural_yuv(32, 16, 8, *LAYOUTS[a], k=3)
        got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(8, a), out_pix_fmt=_fmt(10, b), lut_depth=8), 10)
        assert engine.last_kernel == "k_yuv_xsub_generic"
        assert _eq(got, _want(lut, "tetrahedral", 8, 8, 10, a, b, src)), (a, b)


# ------------------------------------------------------------------ shapes
@pytest.mark.gpu
def test_odd_sizes_ragged_padded_rows_and_batches(engine, cube_dir):
    import torch
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for a, b in twin.CROSS_PAIRS:
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        # odd width and height: the generic kernel, partial output blocks take the edge again
        for w, h in ((37, 23), (9, 1), (1, 5)):
            src = frames.natural_yuv(w, h, 10, icsx, icsy, k=w)
            got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b)), 10)
            assert engine.last_kernel == "k_yuv_xsub_generic"
            assert _eq(got, _want(lut, "tetrahedral", 10, 10, 10, a, b, src)), (a, b, w, h)
        # a ragged width on padded (aligned) rows: the vector kernel up to the last unit, the generic kernel for the tail
        w, h, pad = 70, 22, 96
        src = frames.natural_yuv(w, h, 10, icsx, icsy, k=4)
        sp = [torch.zeros((p.shape[0], pad), dtype=torch.int16, device=engine.device) for p in src]
        for t, p in zip(sp, src):
            t[:, :p.shape[1]] = torch.from_numpy(p.view(np.int16)).to(engine.device)
        src_v = [t[:, :p.shape[1]] for t, p in zip(sp, src)]
        oshape = [(h, w)] + [frames.chroma_shape(w, h, ocsx, ocsy)] * 2
        dp = [torch.full((s[0], pad), -1, dtype=torch.int16, device=engine.device) for s in oshape]
        dst_v = [t[:, :s[1]] for t, s in zip(dp, oshape)]
        engine.apply_yuv(src_v, dst_v, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b))
        assert engine.last_kernel == _vec_name(10, 10, a, b, "tetrahedral"), engine.last_kernel
        assert _eq(_host(dst_v, 10), _want(lut, "tetrahedral", 10, 10, 10, a, b, src)), (a, b, "ragged")
        assert all((t[:, s[1]:] == -1).all() for t, s in zip(dp, oshape)), "wrote past the row"
        # a batch of 3 frames [F, H, W], vector and generic kernels
        for w, h in ((64, 24), (33, 17)):
            fs = [frames.natural_yuv(w, h, 10, icsx, icsy, k=10 + i) for i in range(3)]
            dev = [torch.stack([_dev(f, engine.device)[i] for f in fs]) for i in range(3)]
            out = _host(engine.apply_yuv(dev, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b)), 10)
            for i, f in enumerate(fs):
                assert _eq([o[i] for o in out], _want(lut, "tetrahedral", 10, 10, 10, a, b, f)), (a, b, w, h, i)


@pytest.mark.gpu
def test_row_shards_on_the_union_block(engine, cube_dir):
    import torch
    engine.load_cube(cube_dir / "log709_33.cube")
    for a, b in twin.CROSS_PAIRS:
        bh = 1 << max(LAYOUTS[a][1], LAYOUTS[b][1])
        for w, h in ((64, 22), (31, 23)):
            src = frames.natural_yuv(w, h, 10, *LAYOUTS[a], k=12)
            dev = _dev(src, engine.device)
            whole = _host(engine.apply_yuv(dev, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b)), 10)
            for r0 in range(bh, h, 3 * bh):
                out = engine.apply_yuv(dev, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), row0=0, rows=r0)
                engine.apply_yuv(dev, out, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), row0=r0, rows=h - r0)
                assert _eq(_host(out, 10), whole), (a, b, w, h, r0)
            if bh == 2:
                with pytest.raises(_native.LutrError) as e:
                    engine.apply_yuv(dev, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), row0=1, rows=h - 1)
                assert e.value.code == _native.EINVAL and "union" in e.value.message
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the reference's chains
@pytest.mark.gpu
def test_case_d_exactly(engine, cube_dir):
    """SURVEY.md Appendix D case D: pc10 4:2:2 source, scale=in_range=pc:out_range=tv,format=yuv422p, lut3d,
    format=yuv420p10le -- through apply_lut."""
    from lut_renderer_amd.api import apply_lut
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for w, h in ((64, 36), (35, 21)):
        src = frames.uniform_yuv(w, h, 10, 1, 0, k=10, full_range=True)
        got, _tags = apply_lut(_dev(src, engine.device), cube=lut, pix_fmt="yuv422p10le", colorspace="smpte170m",
                               color_range="pc", out_pix_fmt="yuv420p10le", engine=engine)
        want = _want(lut, "tetrahedral", 10, 8, 10, "422", "420", src, rin="tv", prologue=True, matrix="smpte170m")
        assert _eq(_host(got, 10), want), (w, h, engine.last_kernel)


def _pro_master_cmd(cube_path, w, h, nf):
    from lut_renderer_amd.command import _master_params, engine_command
    info = VideoInfo(width=w, height=h, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), _master_params(ProcessingParams(video_codec="libx264")), cube_path, info,
                         python_bin=sys.executable)
    return cmd + ["--duration", f"{nf / 25.0:.3f}", "--batch", "2"]


@pytest.mark.gpu
def test_pro_master_stage_through_apply_lut_and_the_cli(engine, cube_dir):
    """Stage 1 of the two-stage mode: a 4:2:0 10-bit source written as ProRes 422 HQ's yuv422p10le."""
    from lut_renderer_amd.api import apply_lut
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    w, h, nf = 64, 34, 3
    fs = [frames.natural_yuv(w, h, 10, 1, 1, k=30 + i) for i in range(nf)]
    wants = [_want(lut, "tetrahedral", 10, 10, 10, "420", "422", f) for f in fs]
    got, _ = apply_lut(_dev(fs[0], engine.device), cube=lut, pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv",
                       out_pix_fmt="yuv422p10le", engine=engine)
    assert _eq(_host(got, 10), wants[0])
    cmd = _pro_master_cmd(cube_dir / "log709_33.cube", w, h, nf)
    assert cmd[cmd.index("--out-pix-fmt") + 1] == "yuv422p10le"
    r = subprocess.run(cmd, input=b"".join(p.tobytes() for f in fs for p in f), capture_output=True, cwd=ROOT, timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == b"".join(p.tobytes() for wnt in wants for p in wnt)


# ------------------------------------------------------------------ other options
@pytest.mark.gpu
def test_prelut(engine, tmp_path):
    from oracle import binding as orc
    tab = cube.log709_lattice(17)
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, tab, shapers)
    lut = engine.load_cube(p)
    assert lut.prelut is not None
    pre = orc.parse_lut_file_ex(p)[3]
    for a, b in (("420", "422"), ("444", "420"), ("422", "444")):
        src = frames.natural_yuv(48, 30, 10, *LAYOUTS[a], k=2)
        for mode in ("tetrahedral", "prism"):
            got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), interp=mode), 10)
            assert _eq(got, _want(lut, mode, 10, 10, 10, a, b, src, prelut=pre)), (a, b, mode, engine.last_kernel)


@pytest.mark.gpu
def test_error_diffusion(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for a, b in twin.CROSS_PAIRS:
        for w, h in ((64, 32), (37, 19)):
            for din, dout in ((10, 8), (10, 10)):
                src = frames.natural_yuv(w, h, din, *LAYOUTS[a], k=w + dout)
                got = engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(dout, b),
                                       dither="error_diffusion")
                assert engine.last_kernel == "k_yuv_float+k_dither_ed"
                want = _want(lut, "tetrahedral", din, din, dout, a, b, src, dither=True)
                assert _eq(_host(got, dout), want), (a, b, w, h, din, dout)
    src = frames.natural_yuv(64, 32, 10, 1, 1)
    with pytest.raises(ValueError):
        engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le", out_pix_fmt="yuv422p", dither="error_diffusion",
                         row0=0, rows=16)


@pytest.mark.gpu
def test_fast_and_fma32_run_strict(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    try:
        for prec in ("fast", "fma32"):
            engine.set_precision(prec)
            for a, b in (("420", "422"), ("422", "420"), ("444", "420")):
                src = frames.natural_yuv(128, 64, 10, *LAYOUTS[a], k=6)
                got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b)), 10)
                assert _eq(got, _want(lut, "tetrahedral", 10, 10, 10, a, b, src)), (prec, a, b)
                assert engine.last_kernel == _vec_name(10, 10, a, b, "tetrahedral"), engine.last_kernel
    finally:
        engine.set_precision("strict")


@pytest.mark.gpu
def test_out_size_after_a_layout_change(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 64, 36
    for a, b in (("420", "422"), ("422", "420"), ("444", "420")):
        (ocsx, ocsy) = LAYOUTS[b]
        fs = [frames.natural_yuv(w, h, 10, *LAYOUTS[a], k=40 + i) for i in range(3)]
        import torch
        dev = [torch.stack([_dev(f, engine.device)[i] for f in fs]) for i in range(3)]
        for size in ((48, 20), (96, 54)):
            got = _host(engine.apply_yuv(dev, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), out_size=size, resize_chunk=2), 10)
            for i, f in enumerate(fs):
                mid = _want(lut, "tetrahedral", 10, 10, 10, a, b, f)
                want = rz.resize(mid, 10, ocsx, ocsy, (w, h), size)
                assert _eq([g[i] for g in got], want), (a, b, size, i)


# ------------------------------------------------------------------ equal layouts and routing
def _abi_xsub(engine, dev, out, fin, fout, interp=2, dither=0, row0=0, rows=None):
    from lut_renderer_amd.engine import _planes_struct, parse_pix_fmt
    fi, fo = parse_pix_fmt(fin), parse_pix_fmt(fout)
    p = _native.YuvParams(fi.code, fo.code, fi.depth, 0, 0, 0, 0, 0)
    s, nf = _planes_struct(dev, engine.device)
    d, _ = _planes_struct(out, engine.device)
    h, w = dev[0].shape[-2], dev[0].shape[-1]
    with engine._lock:
        engine._bind_stream()
        return engine._lib.lutr_apply_yuv_xsub(engine._ctx, C.byref(p), interp, dither, w, h, nf, C.byref(s), C.byref(d), row0,
                                               h if rows is None else rows)


@pytest.mark.gpu
def test_equal_layouts_are_apply_yuv(engine, cube_dir):
    import torch
    engine.load_cube(cube_dir / "log709_33.cube")
    for lay in LAYOUTS:
        for w, h in ((256, 64), (37, 21)):
            src = frames.natural_yuv(w, h, 10, *LAYOUTS[lay], k=7)
            dev = _dev(src, engine.device)
            for dither in ("none", "error_diffusion"):
                a = _host(engine.apply_yuv(dev, pix_fmt=_fmt(10, lay), dither=dither), 10)
                ka = engine.last_kernel
                out = [torch.empty_like(t) for t in dev]
                assert _abi_xsub(engine, dev, out, _fmt(10, lay), _fmt(10, lay), dither=_native.DITHER[dither]) == 0
                torch.cuda.synchronize()
                assert _eq(_host(out, 10), a) and engine.last_kernel == ka, (lay, w, h, dither, engine.last_kernel, ka)


@pytest.mark.gpu
def test_variant_routing(engine, cube_dir):
    engine.load_cube(cube_dir / "log709_33.cube")
    src = frames.natural_yuv(64, 32, 10, 1, 1, k=8)
    dev = _dev(src, engine.device)
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
        assert e.value.code == _native.EINVAL
    odd = _dev(frames.natural_yuv(37, 21, 10, 1, 1, k=8), engine.device)
    with _variant(engine, "vec_global"):
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv(odd, pix_fmt="yuv420p10le", out_pix_fmt="yuv444p10le")
        assert e.value.code == _native.EINVAL
        with pytest.raises(_native.LutrError):                 # pyramid has no vector kernel
            engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv444p10le", interp="pyramid")
    with pytest.raises(ValueError, match="subsampling"):
        engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", chroma_loc="left")


# ------------------------------------------------------------------ multi-GPU row sharding
@pytest.mark.gpu
def test_group_shards_on_the_union_block(engine, cube_dir):
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for a, b in (("420", "422"), ("422", "420"), ("444", "420")):
        for w, h in ((64, 23), (34, 37)):
            src = frames.natural_yuv(w, h, 10, *LAYOUTS[a], k=9)
            want = _want(lut, "tetrahedral", 10, 10, 10, a, b, src)
            for n in (2, 3):
                with LutEngineGroup([0] * n, treat_as_remote=True) as g:
                    g.set_lut(lut)
                    got = _host(g.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b)), 10)
                    assert g.last_remote == n - 1
                    assert all(r0 % 2 == 0 for r0, _ in g.last_blocks), g.last_blocks
                    assert _eq(got, want), (a, b, w, h, n)
