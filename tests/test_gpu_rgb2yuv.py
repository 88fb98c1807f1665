"""RGB sources with a YUV output on the GPU: lutr_apply_rgb_to_yuv bit for bit against the reference composition
of tests/_rgb2yuv_twin.py (the C oracle's lut3d at the source's depth, then stage 3 of the YUV contract at the output layout).
The tolerance is zero: both sides are the same fp32 operations in the same order, as for every strict path."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _resize_twin as rz
from tests import _rgb2yuv_twin as twin
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
SOURCES = ("gbrp", "gbrp10le", "gbrp12le", "gbrp16le", "rgb24", "bgr24", "rgba", "bgra", "argb", "abgr", "rgb48le", "rgba64le")
#: output depths per source depth: the pairs (8, 8), (8, 10), (10, 10), (10, 8), (16, 10), (16, 8), and 12 bit on both sides
DOUTS = {8: (8, 10), 10: (10, 8), 12: (12, 8), 16: (10, 8)}


def _yuv(depth, lay):
    return f"yuv{lay}p" + ("" if depth == 8 else f"{depth}le")


def make_source(pix_fmt, dist, w, h, k=0):
    """A host source in `pix_fmt`: gbrp planes (G, B, R), or one packed image [H,W,C] whose fourth component is noise."""
    dl = twin.source_depth(pix_fmt)
    g, b, r = frames.make_rgb(dist, w, h, dl, k=k)
    if pix_fmt not in twin.PACKED:
        return [g, b, r]
    _bits, nc, ro, go, bo = twin.PACKED[pix_fmt]
    img = np.random.default_rng(1000 + k).integers(0, 1 << dl, size=(h, w, nc)).astype(g.dtype)
    img[..., ro], img[..., go], img[..., bo] = r, g, b
    return img


def _t(a, device):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def _dev(src, device):
    return _t(src, device) if isinstance(src, np.ndarray) else [_t(p, device) for p in src]


def _host(tensors, dout):
    return [t.cpu().numpy().view(np.uint16) if dout > 8 else t.cpu().numpy() for t in tensors]


def _eq(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _want(lut, mode, pix_fmt, dout, lay, src, matrix="smpte170m", rng="tv", prelut=None, dither=False, use_lut=True):
    ocsx, ocsy = LAYOUTS[lay]
    k = twin.consts(matrix, rng, twin.source_depth(pix_fmt), dout, ocsx, ocsy)
    if dither:
        return twin.apply_dither(lut.table, lut.scale, mode, k, pix_fmt, dout, ocsx, ocsy, src, prelut=prelut)
    return twin.apply(lut.table, lut.scale, mode, k, pix_fmt, dout, ocsx, ocsy, src, prelut=prelut, lut=use_lut)


def _vec_name(pix_fmt, dout, lay, mode):
    ocsx, ocsy = LAYOUTS[lay]
    nc = twin.PACKED[pix_fmt][1] if pix_fmt in twin.PACKED else 1
    m = "nolut" if mode is None else str(MODES.index(mode))
    return f"k_rgb2yuv_vec<{int(twin.source_depth(pix_fmt) > 8)},{nc},{int(dout > 8)},{ocsx},{ocsy},{m}>"


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


# ------------------------------------------------------------------ sources, layouts, depths, modes and routing
@pytest.mark.gpu
@pytest.mark.parametrize("pix_fmt", SOURCES)
def test_sources_layouts_depths_and_modes(engine, cube_dir, pix_fmt):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    dl = twin.source_depth(pix_fmt)
    w, h = 64, 32
    for dist in ("natural", "uniform"):
        src = make_source(pix_fmt, dist, w, h, k=dl)
        dev = _dev(src, engine.device)
        for lay in LAYOUTS:
            for dout in DOUTS[dl]:
                kw = dict(pix_fmt=pix_fmt, out_pix_fmt=_yuv(dout, lay))
                for mode in MODES if dist == "natural" else ("tetrahedral",):
                    want = _want(lut, mode, pix_fmt, dout, lay, src)
                    with _variant(engine, "generic"):
                        got = _host(engine.apply_rgb_to_yuv(dev, interp=mode, **kw), dout)
                        assert engine.last_kernel == "k_rgb2yuv_generic"
                    assert _eq(got, want), (pix_fmt, dist, lay, dout, mode, "generic")
                    has_vec = mode in VEC_MODES and not (dl == 8 and dout > 8)
                    for variant in ("auto", "vec_global"):
                        with _variant(engine, variant):
                            if not has_vec and variant == "vec_global":
                                with pytest.raises(_native.LutrError) as e:
                                    engine.apply_rgb_to_yuv(dev, interp=mode, **kw)
                                assert e.value.code == _native.EINVAL
                                continue
                            got = _host(engine.apply_rgb_to_yuv(dev, interp=mode, **kw), dout)
                            name = _vec_name(pix_fmt, dout, lay, mode) if has_vec else "k_rgb2yuv_generic"
                            assert engine.last_kernel == name, (variant, engine.last_kernel, name)
                        assert _eq(got, want), (pix_fmt, dist, lay, dout, mode, variant)


@pytest.mark.gpu
def test_other_luts_and_matrices(engine, cube_dir):
    """Lattices that clip and leave the [0, 1] range, a scaled domain, and every matrix / range on the output side."""
    for name in ("random_9.cube", "domain_2.cube", "identity_17.cube"):
        lut = engine.load_cube(cube_dir / name)
        for pix_fmt in ("gbrp10le", "rgb24", "rgba64le"):
            src = make_source(pix_fmt, "uniform", 48, 20, k=2)
            dev = _dev(src, engine.device)
            for lay in LAYOUTS:
                got = _host(engine.apply_rgb_to_yuv(dev, pix_fmt=pix_fmt, out_pix_fmt=_yuv(10, lay)), 10)
                assert _eq(got, _want(lut, "tetrahedral", pix_fmt, 10, lay, src)), (name, pix_fmt, lay)
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    src = make_source("gbrp10le", "natural", 64, 16, k=3)
    dev = _dev(src, engine.device)
    for m in ("bt709", "smpte170m", "bt2020nc"):
        for rng in ("tv", "pc"):
            got = _host(engine.apply_rgb_to_yuv(dev, pix_fmt="gbrp10le", out_pix_fmt="yuv420p10le", matrix_out=m, range_out=rng), 10)
            assert _eq(got, _want(lut, "tetrahedral", "gbrp10le", 10, "420", src, matrix=m, rng=rng)), (m, rng)


@pytest.mark.gpu
def test_without_the_lut(engine, cube_dir):
    """Stage 0 of the full-range composition: the source codes straight to the output stage (no lattice is read)."""
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for pix_fmt in ("gbrp10le", "rgb24", "bgra", "rgb48le"):
        for w, h in ((64, 32), (37, 19)):
            src = make_source(pix_fmt, "uniform", w, h, k=5)
            for lay in LAYOUTS:
                for rng in ("tv", "pc"):
                    got = _host(engine.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt=pix_fmt, out_pix_fmt=_yuv(8, lay),
                                                        lut=False, range_out=rng), 8)
                    vec = w % 8 == 0
                    assert engine.last_kernel == (_vec_name(pix_fmt, 8, lay, None) if vec else "k_rgb2yuv_generic")
                    assert _eq(got, _want(lut, None, pix_fmt, 8, lay, src, rng=rng, use_lut=False)), (pix_fmt, w, h, lay, rng)


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
    for pix_fmt in ("gbrp10le", "rgb24", "rgb48le"):
        src = make_source(pix_fmt, "natural", 48, 30, k=2)
        for lay in LAYOUTS:
            for mode in ("tetrahedral", "prism"):
                got = _host(engine.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt=pix_fmt, out_pix_fmt=_yuv(10, lay),
                                                    interp=mode), 10)
                assert _eq(got, _want(lut, mode, pix_fmt, 10, lay, src, prelut=pre)), (pix_fmt, lay, mode, engine.last_kernel)


# ------------------------------------------------------------------ shapes
@pytest.mark.gpu
def test_odd_sizes_ragged_padded_negative_strides_and_batches(engine, cube_dir):
    import torch
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for pix_fmt in ("gbrp10le", "rgb24", "rgba", "rgb48le"):
        packed = pix_fmt in twin.PACKED
        for lay in LAYOUTS:
            ocsx, ocsy = LAYOUTS[lay]
            out_fmt = _yuv(10 if twin.source_depth(pix_fmt) > 8 else 8, lay)
            dout = 10 if twin.source_depth(pix_fmt) > 8 else 8
            odt = torch.int16 if dout > 8 else torch.uint8
            # odd width and height: the generic kernel, partial output blocks take the edge again
            for w, h in ((1, 1), (3, 5), (65, 33)):
                src = make_source(pix_fmt, "natural", w, h, k=w)
                got = _host(engine.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt=pix_fmt, out_pix_fmt=out_fmt), dout)
                assert engine.last_kernel == "k_rgb2yuv_generic", engine.last_kernel     # (65 wide: dense rows are not aligned)
                assert _eq(got, _want(lut, "tetrahedral", pix_fmt, dout, lay, src)), (pix_fmt, lay, w, h)
            # a ragged width on padded (aligned) rows: the vector kernel up to the last unit, the generic kernel for the tail
            w, h, pad = 70, 22, 96
            src = make_source(pix_fmt, "natural", w, h, k=4)
            dev = _dev(src, engine.device)
            if packed:
                sp = torch.zeros((h, pad, src.shape[2]), dtype=dev.dtype, device=engine.device)
                sp[:, :w] = dev
                src_v = sp[:, :w]
            else:
                sp = [torch.zeros((h, pad), dtype=torch.int16, device=engine.device) for _ in range(3)]
                for t, p in zip(sp, dev):
                    t[:, :w] = p
                src_v = [t[:, :w] for t in sp]
            oshape = [(h, w)] + [frames.chroma_shape(w, h, ocsx, ocsy)] * 2
            dp = [torch.full((s[0], pad), -1 if dout > 8 else 255, dtype=odt, device=engine.device) for s in oshape]
            dst_v = [t[:, :s[1]] for t, s in zip(dp, oshape)]
            engine.apply_rgb_to_yuv(src_v, dst_v, pix_fmt=pix_fmt, out_pix_fmt=out_fmt)
            assert engine.last_kernel == _vec_name(pix_fmt, dout, lay, "tetrahedral"), engine.last_kernel
            assert _eq(_host(dst_v, dout), _want(lut, "tetrahedral", pix_fmt, dout, lay, src)), (pix_fmt, lay, "ragged")
            assert all((t[:, s[1]:] == (-1 if dout > 8 else 255)).all() for t, s in zip(dp, oshape)), "wrote past the row"
            # a batch of 3 frames with a padded frame stride, vector and generic kernels
            for w, h in ((64, 24), (33, 17)):
                fs = [make_source(pix_fmt, "natural", w, h, k=10 + i) for i in range(3)]
                if packed:
                    big = torch.zeros((3, h + 2) + fs[0].shape[1:], dtype=_t(fs[0], "cpu").dtype, device=engine.device)
                    for i, f in enumerate(fs):
                        big[i, :h] = _t(f, engine.device)
                    dev = big[:, :h]
                else:
                    big = [torch.zeros((3, h + 2, w), dtype=torch.int16, device=engine.device) for _ in range(3)]
                    for i, f in enumerate(fs):
                        for t, p in zip(big, f):
                            t[i, :h] = _t(p, engine.device)
                    dev = [t[:, :h] for t in big]
                out = _host(engine.apply_rgb_to_yuv(dev, pix_fmt=pix_fmt, out_pix_fmt=out_fmt), dout)
                for i, f in enumerate(fs):
                    assert _eq([o[i] for o in out], _want(lut, "tetrahedral", pix_fmt, dout, lay, f)), (pix_fmt, lay, w, h, i)
    # negative row strides (a bottom-up image; torch has none, so through the C-ABI): the generic kernel
    from lut_renderer_amd.engine import _planes_struct
    w, h = 64, 16
    src = make_source("gbrp10le", "natural", w, h, k=7)
    base = [_t(p[::-1], engine.device) for p in src]               # rows stored bottom-up
    st, _ = _planes_struct(base, engine.device)
    for i in range(3):
        st.data[i] = base[i].data_ptr() + (h - 1) * w * 2
        st.stride[i] = -w * 2
    dst = [torch.zeros(s_, dtype=torch.int16, device=engine.device) for s_ in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    d, _ = _planes_struct(dst, engine.device)
    p = _native.YuvParams(0, _native.fmt_code(10, 1, 1), 10, 0, _native.MATRIX["smpte170m"], 0, 0, 0)
    for variant, rc in (("auto", 0), ("vec_global", _native.EINVAL)):
        with _variant(engine, variant), engine._lock:
            engine._bind_stream()
            assert engine._lib.lutr_apply_rgb_to_yuv(engine._ctx, C.byref(p), 2, 0, 0, w, h, 1, C.byref(st), None, C.byref(d), 0, h) == rc
    assert engine.last_kernel == "k_rgb2yuv_generic"
    assert _eq(_host(dst, 10), _want(lut, "tetrahedral", "gbrp10le", 10, "420", src))


@pytest.mark.gpu
def test_row_shards_and_their_alignment(engine, cube_dir):
    engine.load_cube(cube_dir / "log709_33.cube")
    for pix_fmt in ("gbrp10le", "rgb24"):
        dout = 10 if pix_fmt == "gbrp10le" else 8
        for lay in LAYOUTS:
            bh = 1 << LAYOUTS[lay][1]
            kw = dict(pix_fmt=pix_fmt, out_pix_fmt=_yuv(dout, lay))
            for w, h in ((64, 22), (31, 23)):
                dev = _dev(make_source(pix_fmt, "natural", w, h, k=12), engine.device)
                whole = _host(engine.apply_rgb_to_yuv(dev, **kw), dout)
                for r0 in range(bh, h, 3 * bh):
                    out = engine.apply_rgb_to_yuv(dev, row0=0, rows=r0, **kw)
                    engine.apply_rgb_to_yuv(dev, out, row0=r0, rows=h - r0, **kw)
                    assert _eq(_host(out, dout), whole), (pix_fmt, lay, w, h, r0)
                if bh == 2:
                    with pytest.raises(_native.LutrError) as e:
                        engine.apply_rgb_to_yuv(dev, row0=1, rows=h - 1, **kw)
                    assert e.value.code == _native.EINVAL and "block height" in e.value.message


def _abi(engine, pix_fmt, out_fmt, src, dst, interp=2, dither=0):
    """lutr_apply_rgb_to_yuv itself, past the Python layer's own checks."""
    from lut_renderer_amd.engine import parse_pix_fmt, parse_rgb_source
    fin, fout = parse_rgb_source(pix_fmt), parse_pix_fmt(out_fmt)
    planar, packed, w, h, nf, _ = engine._rgb_source(src, fin)
    from lut_renderer_amd.engine import _planes_struct
    d, _ = _planes_struct(dst, engine.device)
    p = _native.YuvParams(0, fout.code, fin.depth, 0, 1, 0, 0, 0)
    with engine._lock:
        engine._bind_stream()
        return engine._lib.lutr_apply_rgb_to_yuv(engine._ctx, C.byref(p), interp, dither, fin.code, w, h, nf,
                                                 C.byref(planar) if planar is not None else None,
                                                 C.byref(packed) if packed is not None else None, C.byref(d), 0, h)


@pytest.mark.gpu
def test_overlap_and_variant_rejections(engine, cube_dir):
    import torch
    engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 64, 16
    # one buffer holding the source planes and, overlapping the last of them, the destination luma plane
    buf = torch.zeros(3 * h * w + h * w, dtype=torch.uint8, device=engine.device)
    buf[:3 * h * w] = 77
    src = [buf[i * h * w:(i + 1) * h * w].view(h, w) for i in range(3)]
    dst = [buf[2 * h * w + 8:3 * h * w + 8].view(h, w),
           torch.zeros((h // 2, w // 2), dtype=torch.uint8, device=engine.device),
           torch.zeros((h // 2, w // 2), dtype=torch.uint8, device=engine.device)]
    with pytest.raises(ValueError, match="in place"):
        engine.apply_rgb_to_yuv(src, dst, pix_fmt="gbrp", out_pix_fmt="yuv420p")
    assert _abi(engine, "gbrp", "yuv420p", src, dst) == _native.EINVAL
    assert b"in place" in engine._lib.lutr_last_error()
    torch.cuda.synchronize()
    assert bool((buf[:3 * h * w] == 77).all()) and bool((buf[3 * h * w:] == 0).all()), "a rejected call touched its buffers"
    img = torch.zeros((h, w, 3), dtype=torch.uint8, device=engine.device)
    flat = img.view(-1)
    dst = [flat[:h * w].view(h, w)] + dst[1:]
    with pytest.raises(ValueError, match="in place"):
        engine.apply_rgb_to_yuv(img, dst, pix_fmt="rgb24", out_pix_fmt="yuv420p")
    assert _abi(engine, "rgb24", "yuv420p", img, dst) == _native.EINVAL
    dev = _dev(make_source("gbrp10le", "natural", w, h), engine.device)
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError) as e:
            engine.apply_rgb_to_yuv(dev, pix_fmt="gbrp10le", out_pix_fmt="yuv420p10le")
        assert e.value.code == _native.EINVAL
    with pytest.raises(ValueError, match="chroma"):
        engine.apply_rgb_to_yuv(dev, pix_fmt="gbrp10le", out_pix_fmt="yuv420p10le", chroma_loc="left")
    with pytest.raises(ValueError):
        engine.apply_rgb_to_yuv(dev, pix_fmt="gbrp10le", out_pix_fmt="gbrp10le")
    with pytest.raises(ValueError):
        engine.apply_rgb_to_yuv(dev, pix_fmt="yuv444p10le", out_pix_fmt="yuv420p10le")
    with pytest.raises(ValueError, match="planar YUV"):
        engine.apply_yuv(dev, pix_fmt="yuv444p10le", out_pix_fmt="gbrp10le")
    with pytest.raises(_native.LutrError):                 # 4:4:0 output
        p = _native.YuvParams(0, _native.fmt_code(10, 0, 1), 10, 0, 1, 0, 0, 0)
        from lut_renderer_amd.engine import _planes_struct
        s, _ = _planes_struct(dev, engine.device)
        _native.check(engine._lib.lutr_apply_rgb_to_yuv(engine._ctx, C.byref(p), 2, 0, 0, w, h, 1, C.byref(s), None, C.byref(s), 0, h))


# ------------------------------------------------------------------ other options
@pytest.mark.gpu
def test_error_diffusion(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for pix_fmt, dout in (("gbrp10le", 8), ("gbrp10le", 10), ("rgb24", 8), ("rgb48le", 10)):
        for lay in LAYOUTS:
            for w, h in ((64, 32), (37, 19)):
                src = make_source(pix_fmt, "natural", w, h, k=w + dout)
                got = engine.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt=pix_fmt, out_pix_fmt=_yuv(dout, lay),
                                              dither="error_diffusion")
                assert engine.last_kernel == "k_rgb2yuv_float+k_dither_ed"
                want = _want(lut, "tetrahedral", pix_fmt, dout, lay, src, dither=True)
                assert _eq(_host(got, dout), want), (pix_fmt, dout, lay, w, h)
    with pytest.raises(ValueError):
        engine.apply_rgb_to_yuv(_dev(make_source("gbrp10le", "natural", 64, 32), engine.device), pix_fmt="gbrp10le",
                                out_pix_fmt="yuv420p", dither="error_diffusion", row0=0, rows=16)


@pytest.mark.gpu
def test_fast_and_fma32_run_strict(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    try:
        for prec in ("fast", "fma32"):
            engine.set_precision(prec)
            for pix_fmt, dout in (("gbrp10le", 10), ("rgb24", 8)):
                src = make_source(pix_fmt, "natural", 128, 64, k=6)
                got = _host(engine.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt=pix_fmt, out_pix_fmt=_yuv(dout, "420")), dout)
                assert _eq(got, _want(lut, "tetrahedral", pix_fmt, dout, "420", src)), (prec, pix_fmt)
                assert engine.last_kernel == _vec_name(pix_fmt, dout, "420", "tetrahedral"), engine.last_kernel
    finally:
        engine.set_precision("strict")


@pytest.mark.gpu
def test_out_size(engine, cube_dir):
    import torch
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 64, 36
    for pix_fmt, dout in (("gbrp10le", 10), ("rgb24", 8)):
        for lay in ("420", "444"):
            ocsx, ocsy = LAYOUTS[lay]
            fs = [make_source(pix_fmt, "natural", w, h, k=40 + i) for i in range(3)]
            dev = torch.stack([_t(f, engine.device) for f in fs]) if pix_fmt in twin.PACKED else \
                [torch.stack([_t(f[i], engine.device) for f in fs]) for i in range(3)]
            for size in ((48, 20), (96, 54)):
                got = _host(engine.apply_rgb_to_yuv(dev, pix_fmt=pix_fmt, out_pix_fmt=_yuv(dout, lay), out_size=size,
                                                    resize_chunk=2), dout)
                for i, f in enumerate(fs):
                    mid = _want(lut, "tetrahedral", pix_fmt, dout, lay, f)
                    want = rz.resize(mid, dout, ocsx, ocsy, (w, h), size)
                    assert _eq([g[i] for g in got], want), (pix_fmt, lay, size, i)


# ------------------------------------------------------------------ sources flagged full range
@pytest.mark.gpu
def test_full_range_composition(engine, cube_dir):
    """3.9 point 6 through apply_lut: stage 0 without the LUT into an 8-bit frame, then today's apply_yuv (a tile kernel under
    the test processes' LUTR_SMALL_JOB_MPX=0)."""
    from lut_renderer_amd.api import apply_lut
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for pix_fmt, out_fmt, dout, lay in (("rgb24", "yuv420p", 8, "420"), ("gbrp10le", "yuv420p10le", 10, "420"),
                                        ("rgb48le", "yuv422p10le", 10, "422")):
        for w, h in ((256, 64), (35, 21)):
            src = make_source(pix_fmt, "natural", w, h, k=10)
            for tags, rng in (("bt709", "tv"), ("none", "pc")):
                got, _tags = apply_lut(_dev(src, engine.device), cube=lut, pix_fmt=pix_fmt, colorspace="bt709", color_range="pc",
                                       out_pix_fmt=out_fmt, output_tags=tags, engine=engine)
                want = twin.apply_full_range(lut.table, lut.scale, "tetrahedral", pix_fmt, src, "420", rng, "bt709", dout, lay)
                assert _eq(_host(got, dout), want), (pix_fmt, w, h, rng, engine.last_kernel)
                if w == 256 and dout == 8:
                    assert engine.last_kernel.startswith("k_yuv_tile2"), engine.last_kernel


# ------------------------------------------------------------------ multi-GPU row sharding
@pytest.mark.gpu
def test_group_row_shards(engine, cube_dir, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for pix_fmt, dout in (("gbrp10le", 10), ("rgb24", 8)):
        for lay in ("420", "444"):
            for w, h in ((64, 23), (34, 37)):
                src = make_source(pix_fmt, "natural", w, h, k=9)
                want = _want(lut, "tetrahedral", pix_fmt, dout, lay, src)
                for n in (2, 3):
                    with LutEngineGroup([0] * n, treat_as_remote=True) as g:
                        g.set_lut(lut)
                        got = _host(g.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt=pix_fmt, out_pix_fmt=_yuv(dout, lay)), dout)
                        assert g.last_remote == n - 1
                        assert all(r0 % (1 << LAYOUTS[lay][1]) == 0 for r0, _ in g.last_blocks), g.last_blocks
                        assert _eq(got, want), (pix_fmt, lay, w, h, n)
    src = make_source("rgb24", "natural", 64, 24, k=3)
    want = _want(lut, "tetrahedral", "rgb24", 8, "420", src)
    with LutEngineGroup([0, 0]) as g:                      # same device: launches on the caller's buffers
        g.set_lut(lut)
        assert _eq(_host(g.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt="rgb24", out_pix_fmt="yuv420p"), 8), want)
        assert g.last_remote == 0
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    with LutEngineGroup([0, 0]) as g:
        g.set_lut(lut)
        assert _eq(_host(g.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt="rgb24", out_pix_fmt="yuv420p"), 8), want)
        assert g.last_remote == 1


# ------------------------------------------------------------------ apply_lut, HostPipeline and the CLI
@pytest.mark.gpu
def test_apply_lut_and_host_pipeline(engine, cube_dir):
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.stream import HostPipeline
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    w, h, nf = 64, 34, 5
    for pix_fmt, out_fmt, dout in (("rgb24", "yuv420p", 8), ("gbrp10le", "yuv420p10le", 10)):
        fs = [make_source(pix_fmt, "natural", w, h, k=30 + i) for i in range(nf)]
        wants = [_want(lut, "tetrahedral", pix_fmt, dout, "420", f, matrix="bt709") for f in fs]
        got, tags = apply_lut(_dev(fs[0], engine.device), cube=lut, pix_fmt=pix_fmt, colorspace="bt709", out_pix_fmt=out_fmt,
                              width=w, height=h, engine=engine)
        assert _eq(_host(got, dout), wants[0]) and tags["colorspace"] == "bt709"
        pipe = HostPipeline(engine, pix_fmt, w, h, batch=2, out_pix_fmt=out_fmt, interp="tetrahedral", matrix_out="bt709")
        raw = [f.tobytes() if isinstance(f, np.ndarray) else b"".join(p.tobytes() for p in f) for f in fs]
        assert all(len(r) == pipe.fin.frame_bytes for r in raw)
        state = {"i": 0, "out": b""}

        def fill(buf, n):
            k = min(n, nf - state["i"])
            for j in range(k):
                buf[j * len(raw[0]):(j + 1) * len(raw[0])] = np.frombuffer(raw[state["i"] + j], np.uint8)
            state["i"] += k
            return k

        def drain(buf, n):
            state["out"] += bytes(buf)

        assert pipe.run(fill, drain) == nf
        assert state["out"] == b"".join(p.tobytes() for wnt in wants for p in wnt), pix_fmt


def _stage_cmd(cube_path, info, params, nf):
    from lut_renderer_amd.command import engine_command
    cmd = engine_command(Path("-"), Path("-"), params, cube_path, info, python_bin=sys.executable)
    return cmd + ["--duration", f"{nf / 25.0:.3f}", "--batch", "2"]


@pytest.mark.gpu
def test_cli_end_to_end(engine, cube_dir, tmp_path):
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    w, h, nf = 64, 34, 3
    # a rawvideo file: rgb24 in, yuv420p out, with the Duration: / time= lines
    fs = [make_source("rgb24", "natural", w, h, k=50 + i) for i in range(nf)]
    (tmp_path / "in.rgb").write_bytes(b"".join(f.tobytes() for f in fs))
    cmd = [sys.executable, "-m", "lut_renderer_amd.cli", "-i", str(tmp_path / "in.rgb"), "-o", str(tmp_path / "out.yuv"), "--size",
           f"{w}x{h}", "--pix-fmt", "rgb24", "--out-pix-fmt", "yuv420p", "--cube", str(cube_dir / "log709_33.cube"), "--batch", "2"]
    r = subprocess.run(cmd, capture_output=True, cwd=ROOT, timeout=180, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    wants = [_want(lut, "tetrahedral", "rgb24", 8, "420", f) for f in fs]
    assert (tmp_path / "out.yuv").read_bytes() == b"".join(p.tobytes() for wnt in wants for p in wnt)
    assert "Duration: 00:00:00.12" in r.stdout and "time=00:00:00.12" in r.stdout
    # the stages engine_command renders for the two sources of the issue run to exit code 0
    info = VideoInfo(width=w, height=h, bit_depth=10, pix_fmt="gbrp10le", fps=25.0)
    fs = [make_source("gbrp10le", "natural", w, h, k=60 + i) for i in range(nf)]
    cmd = _stage_cmd(cube_dir / "log709_33.cube", info, ProcessingParams(video_codec="libx265"), nf)
    r = subprocess.run(cmd, input=b"".join(p.tobytes() for f in fs for p in f), capture_output=True, cwd=ROOT, timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    wants = [_want(lut, "tetrahedral", "gbrp10le", 10, "420", f) for f in fs]
    assert r.stdout == b"".join(p.tobytes() for wnt in wants for p in wnt)
    info = VideoInfo(width=w, height=h, bit_depth=8, pix_fmt="rgb24", color_range="pc", fps=25.0)
    fs = [make_source("rgb24", "natural", w, h, k=70 + i) for i in range(nf)]
    cmd = _stage_cmd(cube_dir / "log709_33.cube", info, ProcessingParams(video_codec="libx264", bit_depth_policy="force_8bit"), nf)
    r = subprocess.run(cmd, input=b"".join(f.tobytes() for f in fs), capture_output=True, cwd=ROOT, timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    wants = [twin.apply_full_range(lut.table, lut.scale, "tetrahedral", "rgb24", f, "420", "tv", None, 8, "420") for f in fs]
    assert r.stdout == b"".join(p.tobytes() for wnt in wants for p in wnt)
