"""Planar float RGB sources on the GPU: lutr_apply_planar_rgb_f32 and lutr_apply_rgbf_to_yuv bit for bit against
the reference composition of tests/_rgbf_twin.py.  The tolerance is zero everywhere: both sides are the same fp32 operations in
the same order.  Pyramid and prism, which the NumPy lattice does not have, are pinned to the C oracle through code-valued floats
(fl(code * fl(1 / M)) in, lut3d's integer store on what comes out); on the YUV path they are checked against the twin's quantiser
and output stage fed with the float kernel's (so pinned) lattice output."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from tests import _rgbf_twin as twin
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
F = np.float32
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
LUTS = ("log709_33.cube", "random_9.cube", "domain_2.cube", "identity_17.cube")


def _yuv(depth, lay):
    return f"yuv{lay}p" + ("" if depth == 8 else f"{depth}le")


def _t(a, device):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def _dev(src, device):
    return [_t(p, device) for p in src]


def _hostf(tensors):
    return [t.cpu().numpy() for t in tensors]


def _hosty(tensors, dout):
    return [t.cpu().numpy().view(np.uint16) if dout > 8 else t.cpu().numpy() for t in tensors]


def _eqf(got, want):
    """Float planes bit for bit."""
    return all(g.shape == w.shape and np.array_equal(np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32))
               for g, w in zip(got, want))


def _eq(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _vec_name(dout, lay, mode):
    ocsx, ocsy = LAYOUTS[lay]
    return f"k_rgbf2yuv_vec<{int(dout > 8)},{ocsx},{ocsy},{'nolut' if mode is None else MODES.index(mode)}>"


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


def _want_yuv(lut, mode, dout, lay, src, matrix="smpte170m", rng="tv", prelut=None, dither=False, use_lut=True):
    ocsx, ocsy = LAYOUTS[lay]
    k = twin.consts(matrix, rng, dout, ocsx, ocsy)
    if dither:
        return twin.apply_dither(lut.table, lut.scale, mode, k, dout, ocsx, ocsy, src, prelut=prelut)
    return twin.apply_yuv(lut.table, lut.scale, mode, k, dout, ocsx, ocsy, src, prelut=prelut, lut=use_lut)


# ------------------------------------------------------------------ float to float
@pytest.mark.gpu
@pytest.mark.parametrize("lut_name", LUTS)
def test_float_to_float_sources_modes_and_variants(engine, cube_dir, lut_name):
    lut = engine.load_cube(cube_dir / lut_name)
    w, h = 64, 32
    for dist in ("natural", "uniform", "hdr", "nonfinite"):
        src = twin.make_float(dist, w, h, k=len(lut_name))
        if dist == "nonfinite":
            assert not all(np.isfinite(p).all() for p in src)
        dev = _dev(src, engine.device)
        for mode in VEC_MODES:
            want = twin.apply_float(lut.table, lut.scale, mode, src)
            assert all(np.isfinite(p).all() for p in want)
            for variant in ("generic", "auto", "vec_global"):
                with _variant(engine, variant):
                    got = _hostf(engine.apply_rgb_float(dev, interp=mode))
                    name = "k_rgbf_generic" if variant == "generic" else f"k_rgbf_vec<{MODES.index(mode)}>"
                    assert engine.last_kernel == name, (variant, engine.last_kernel)
                assert _eqf(got, want), (lut_name, dist, mode, variant)
            if lut_name == "random_9.cube" and dist == "uniform" and mode != "nearest":
                assert min(p.min() for p in got) < 0.0 and max(p.max() for p in got) > 1.0, "the float output was clipped"


@pytest.mark.gpu
def test_pyramid_and_prism_against_the_c_oracle(engine, cube_dir, orc):
    for lut_name in ("log709_33.cube", "random_9.cube", "domain_2.cube"):
        lut = engine.load_cube(cube_dir / lut_name)
        for depth in (10, 16):
            planes = frames.make_rgb("uniform", 64, 24, depth, k=depth)
            dev = _dev(twin.code_frame(planes, depth), engine.device)
            for mode in MODES:
                got = twin.to_codes(_hostf(engine.apply_rgb_float(dev, interp=mode)), depth)
                assert engine.last_kernel == (f"k_rgbf_vec<{MODES.index(mode)}>" if mode in VEC_MODES else "k_rgbf_generic")
                assert _eq(got, orc.apply_rgb(lut.table, lut.scale, depth, mode, planes)), (lut_name, depth, mode)
            for mode in ("pyramid", "prism"):
                with _variant(engine, "vec_global"):
                    with pytest.raises(_native.LutrError) as e:
                        engine.apply_rgb_float(dev, interp=mode)
                    assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_float_layouts_batches_in_place_ragged_negative_strides_and_shards(engine, cube_dir):
    import torch
    from lut_renderer_amd.engine import _planes_struct
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    dv = engine.device
    # odd sizes on dense rows: the generic kernel (rows of 65 floats are not 16-byte aligned)
    for w, h in ((1, 1), (3, 5), (65, 33)):
        src = twin.make_float("natural", w, h, k=w)
        got = _hostf(engine.apply_rgb_float(_dev(src, dv)))
        assert engine.last_kernel == "k_rgbf_generic", engine.last_kernel
        assert _eqf(got, twin.apply_float(lut.table, lut.scale, "tetrahedral", src)), (w, h)
    # padded strides, whole and ragged widths: the vector kernel, with the generic kernel for a ragged tail
    for w, h, pad in ((64, 22, 96), (70, 22, 96), (67, 9, 80)):
        src = twin.make_float("hdr", w, h, k=4)
        sp = [torch.zeros((h, pad), dtype=torch.float32, device=dv) for _ in range(3)]
        dp = [torch.full((h, pad), -7.0, dtype=torch.float32, device=dv) for _ in range(3)]
        for t, p in zip(sp, _dev(src, dv)):
            t[:, :w] = p
        dst_v = [t[:, :w] for t in dp]
        engine.apply_rgb_float([t[:, :w] for t in sp], dst_v)
        assert engine.last_kernel == "k_rgbf_vec<2>", engine.last_kernel
        assert _eqf(_hostf(dst_v), twin.apply_float(lut.table, lut.scale, "tetrahedral", src)), (w, h, "padded")
        assert all(bool((t[:, w:] == -7.0).all()) for t in dp), "wrote past the row"
        with _variant(engine, "vec_global"):
            if w % 4:
                with pytest.raises(_native.LutrError):
                    engine.apply_rgb_float([t[:, :w] for t in sp], dst_v)
            else:
                engine.apply_rgb_float([t[:, :w] for t in sp], dst_v)
    # batches of 3 frames with a padded frame stride, vector and generic kernels, out of place and in place
    for w, h in ((64, 24), (33, 17)):
        fs = [twin.make_float("natural", w, h, k=10 + i) for i in range(3)]
        big = [torch.zeros((3, h + 2, w), dtype=torch.float32, device=dv) for _ in range(3)]
        for i, f in enumerate(fs):
            for t, p in zip(big, f):
                t[i, :h] = _t(p, dv)
        dev = [t[:, :h] for t in big]
        wants = [twin.apply_float(lut.table, lut.scale, "trilinear", f) for f in fs]
        out = _hostf(engine.apply_rgb_float(dev, interp="trilinear"))
        assert engine.last_kernel == ("k_rgbf_vec<1>" if w == 64 else "k_rgbf_generic")
        for i in range(3):
            assert _eqf([o[i] for o in out], wants[i]), (w, h, i)
        back = engine.apply_rgb_float(dev, dev, interp="trilinear")         # in place
        assert back[0].data_ptr() == dev[0].data_ptr()
        for i in range(3):
            assert _eqf([o[i] for o in _hostf(dev)], wants[i]), (w, h, i, "in place")
        assert all(bool((t[:, h:] == 0).all()) for t in big), "wrote between the frames"
    # row shards (any row: the operation is pixelwise)
    for w, h in ((64, 22), (31, 23)):
        src = twin.make_float("natural", w, h, k=12)
        dev = _dev(src, dv)
        want = twin.apply_float(lut.table, lut.scale, "tetrahedral", src)
        for r0 in (1, 7, h - 1):
            out = [torch.zeros_like(t) for t in dev]
            engine.apply_rgb_float(dev, out, row0=0, rows=r0)
            assert all(bool((t[r0:] == 0).all()) for t in out)
            engine.apply_rgb_float(dev, out, row0=r0, rows=h - r0)
            assert _eqf(_hostf(out), want), (w, h, r0)
    # negative row strides (a bottom-up image; torch has none, so through the C-ABI): the generic kernel
    w, h = 64, 16
    src = twin.make_float("natural", w, h, k=7)
    base = [_t(p[::-1], dv) for p in src]                          # rows stored bottom-up
    st, _ = _planes_struct(base, dv)
    for i in range(3):
        st.data[i] = base[i].data_ptr() + (h - 1) * w * 4
        st.stride[i] = -w * 4
    dst = [torch.zeros((h, w), dtype=torch.float32, device=dv) for _ in range(3)]
    d, _ = _planes_struct(dst, dv)
    for variant, rc in (("auto", 0), ("vec_global", _native.EINVAL)):
        with _variant(engine, variant), engine._lock:
            engine._bind_stream()
            assert engine._lib.lutr_apply_planar_rgb_f32(engine._ctx, 2, w, h, 1, C.byref(st), C.byref(d), 0, h) == rc
    assert engine.last_kernel == "k_rgbf_generic"
    assert _eqf(_hostf(dst), twin.apply_float(lut.table, lut.scale, "tetrahedral", src))


# ------------------------------------------------------------------ float to YUV
@pytest.mark.gpu
@pytest.mark.parametrize("lay", list(LAYOUTS))
def test_yuv_layouts_depths_modes_and_variants(engine, cube_dir, lay):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 64, 32
    for dist in ("natural", "hdr", "nonfinite"):
        src = twin.make_float(dist, w, h, k=3)
        dev = _dev(src, engine.device)
        for dout in (8, 10, 16):
            kw = dict(pix_fmt="gbrpf32le", out_pix_fmt=_yuv(dout, lay))
            for mode in (MODES if dist == "natural" else ("tetrahedral",)) + (None,):
                call = dict(kw, lut=False) if mode is None else dict(kw, interp=mode)
                if mode in ("pyramid", "prism"):
                    # the float kernel's lattice output (pinned to the C oracle above) through the twin's quantiser and output stage
                    with _variant(engine, "generic"):
                        g, b, r = _hostf(engine.apply_rgb_float(dev, interp=mode))
                    ocsx, ocsy = LAYOUTS[lay]
                    want = twin.rgb_codes_to_yuv(twin.consts("smpte170m", "tv", dout, ocsx, ocsy), dout, ocsx, ocsy,
                                                 [twin.quantise(p) for p in (r, g, b)])
                else:
                    want = _want_yuv(lut, mode, dout, lay, src, use_lut=mode is not None)
                has_vec = mode is None or mode in VEC_MODES
                for variant in ("generic", "auto", "vec_global"):
                    with _variant(engine, variant):
                        if variant == "vec_global" and not has_vec:
                            with pytest.raises(_native.LutrError) as e:
                                engine.apply_rgb_to_yuv(dev, **call)
                            assert e.value.code == _native.EINVAL
                            continue
                        got = _hosty(engine.apply_rgb_to_yuv(dev, **call), dout)
                        name = "k_rgbf2yuv_generic" if variant == "generic" or not has_vec else _vec_name(dout, lay, mode)
                        assert engine.last_kernel == name, (variant, engine.last_kernel, name)
                    assert _eq(got, want), (lay, dist, dout, mode, variant)


@pytest.mark.gpu
def test_yuv_other_luts_matrices_and_ranges(engine, cube_dir):
    for name in ("random_9.cube", "domain_2.cube", "identity_17.cube"):
        lut = engine.load_cube(cube_dir / name)
        src = twin.make_float("hdr" if name == "domain_2.cube" else "uniform", 48, 20, k=2)
        for lay in LAYOUTS:
            got = _hosty(engine.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt="gbrpf32le", out_pix_fmt=_yuv(10, lay)), 10)
            assert _eq(got, _want_yuv(lut, "tetrahedral", 10, lay, src)), (name, lay)
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    src = twin.make_float("natural", 64, 16, k=3)
    for m in ("bt709", "smpte170m", "bt2020nc"):
        for rng in ("tv", "pc"):
            got = _hosty(engine.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt="gbrpf32le", out_pix_fmt="yuv420p10le",
                                                 matrix_out=m, range_out=rng), 10)
            assert _eq(got, _want_yuv(lut, "tetrahedral", 10, "420", src, matrix=m, rng=rng)), (m, rng)


@pytest.mark.gpu
def test_yuv_odd_sizes_ragged_batches_and_row_shards(engine, cube_dir):
    import torch
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    dv = engine.device
    for lay in LAYOUTS:
        ocsx, ocsy = LAYOUTS[lay]
        bh = 1 << ocsy
        kw = dict(pix_fmt="gbrpf32le", out_pix_fmt=_yuv(10, lay))
        for w, h in ((1, 1), (3, 5), (65, 33)):
            src = twin.make_float("natural", w, h, k=w)
            got = _hosty(engine.apply_rgb_to_yuv(_dev(src, dv), **kw), 10)
            assert engine.last_kernel == "k_rgbf2yuv_generic", engine.last_kernel
            assert _eq(got, _want_yuv(lut, "tetrahedral", 10, lay, src)), (lay, w, h)
        # a ragged width on padded rows: the split
        w, h, pad = 70, 22, 96
        src = twin.make_float("natural", w, h, k=4)
        sp = [torch.zeros((h, pad), dtype=torch.float32, device=dv) for _ in range(3)]
        for t, p in zip(sp, _dev(src, dv)):
            t[:, :w] = p
        oshape = [(h, w)] + [frames.chroma_shape(w, h, ocsx, ocsy)] * 2
        dp = [torch.full((s[0], pad), -1, dtype=torch.int16, device=dv) for s in oshape]
        dst_v = [t[:, :s[1]] for t, s in zip(dp, oshape)]
        engine.apply_rgb_to_yuv([t[:, :w] for t in sp], dst_v, **kw)
        assert engine.last_kernel == _vec_name(10, lay, "tetrahedral"), engine.last_kernel
        assert _eq(_hosty(dst_v, 10), _want_yuv(lut, "tetrahedral", 10, lay, src)), (lay, "ragged")
        assert all(bool((t[:, s[1]:] == -1).all()) for t, s in zip(dp, oshape)), "wrote past the row"
        # a batch of 3 frames with a padded frame stride
        for w, h in ((64, 24), (33, 17)):
            fs = [twin.make_float("natural", w, h, k=10 + i) for i in range(3)]
            big = [torch.zeros((3, h + 2, w), dtype=torch.float32, device=dv) for _ in range(3)]
            for i, f in enumerate(fs):
                for t, p in zip(big, f):
                    t[i, :h] = _t(p, dv)
            out = _hosty(engine.apply_rgb_to_yuv([t[:, :h] for t in big], **kw), 10)
            for i, f in enumerate(fs):
                assert _eq([o[i] for o in out], _want_yuv(lut, "tetrahedral", 10, lay, f)), (lay, w, h, i)
        # row shards on the output chroma block, and the alignment error
        for w, h in ((64, 22), (31, 23)):
            dev = _dev(twin.make_float("natural", w, h, k=12), dv)
            whole = _hosty(engine.apply_rgb_to_yuv(dev, **kw), 10)
            for r0 in range(bh, h, 3 * bh):
                out = engine.apply_rgb_to_yuv(dev, row0=0, rows=r0, **kw)
                engine.apply_rgb_to_yuv(dev, out, row0=r0, rows=h - r0, **kw)
                assert _eq(_hosty(out, 10), whole), (lay, w, h, r0)
            if bh == 2:
                with pytest.raises(_native.LutrError) as e:
                    engine.apply_rgb_to_yuv(dev, row0=1, rows=h - 1, **kw)
                assert e.value.code == _native.EINVAL and "block height" in e.value.message


@pytest.mark.gpu
def test_yuv_error_diffusion(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for dout in (8, 10):
        for lay in LAYOUTS:
            for w, h in ((64, 32), (37, 19)):
                src = twin.make_float("natural", w, h, k=w + dout)
                got = engine.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt="gbrpf32le", out_pix_fmt=_yuv(dout, lay),
                                              dither="error_diffusion")
                assert engine.last_kernel == "k_rgbf2yuv_float+k_dither_ed"
                assert _eq(_hosty(got, dout), _want_yuv(lut, "tetrahedral", dout, lay, src, dither=True)), (dout, lay, w, h)
    with pytest.raises(ValueError):
        engine.apply_rgb_to_yuv(_dev(twin.make_float("natural", 64, 32), engine.device), pix_fmt="gbrpf32le",
                                out_pix_fmt="yuv420p", dither="error_diffusion", row0=0, rows=16)


@pytest.mark.gpu
def test_full_range_composition(engine, cube_dir):
    from lut_renderer_amd.api import apply_lut
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for out_fmt, dout, lay in (("yuv420p", 8, "420"), ("yuv420p10le", 10, "420"), ("yuv422p10le", 10, "422")):
        for w, h in ((256, 64), (35, 21)):
            src = twin.make_float("natural", w, h, k=10)
            for tags, rng in (("bt709", "tv"), ("none", "pc")):
                got, _tags = apply_lut(_dev(src, engine.device), cube=lut, pix_fmt="gbrpf32le", colorspace="bt709", color_range="pc",
                                       out_pix_fmt=out_fmt, output_tags=tags, engine=engine)
                want = twin.apply_full_range(lut.table, lut.scale, "tetrahedral", src, "420", rng, "bt709", dout, lay)
                assert _eq(_hosty(got, dout), want), (out_fmt, w, h, rng, engine.last_kernel)
    src = twin.make_float("hdr", 64, 32, k=1)                      # the engine call itself
    got = engine.apply_rgb_full_range(_dev(src, engine.device), pix_fmt="gbrpf32le", out_pix_fmt="yuv420p10le",
                                      intermediate_pix_fmt="yuv420p", prologue_out_range="tv", matrix=None)
    assert _eq(_hosty(got, 10), twin.apply_full_range(lut.table, lut.scale, "tetrahedral", src, "420", "tv", None, 10, "420"))


# ------------------------------------------------------------------ prelut
@pytest.mark.gpu
def test_prelut_on_both_paths(engine, tmp_path):
    from oracle import binding as orc
    tab = cube.log709_lattice(17)
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, tab, shapers)
    lut = engine.load_cube(p)
    assert lut.prelut is not None
    pre = orc.parse_lut_file_ex(p)[3]
    for dist in ("natural", "hdr"):
        src = twin.make_float(dist, 64, 30, k=2)
        dev = _dev(src, engine.device)
        for variant in ("auto", "generic"):
            with _variant(engine, variant):
                for mode in VEC_MODES:
                    got = _hostf(engine.apply_rgb_float(dev, interp=mode))
                    assert engine.last_kernel == ("k_rgbf_generic" if variant == "generic" else f"k_rgbf_vec<{MODES.index(mode)}>")
                    assert _eqf(got, twin.apply_float(lut.table, lut.scale, mode, src, prelut=pre)), (dist, variant, mode)
                for lay in LAYOUTS:
                    got = _hosty(engine.apply_rgb_to_yuv(dev, pix_fmt="gbrpf32le", out_pix_fmt=_yuv(10, lay)), 10)
                    assert engine.last_kernel == ("k_rgbf2yuv_generic" if variant == "generic" else _vec_name(10, lay, "tetrahedral"))
                    assert _eq(got, _want_yuv(lut, "tetrahedral", 10, lay, src, prelut=pre)), (dist, variant, lay)
    # pyramid / prism with the prelut: code-valued floats against the C oracle
    planes = frames.make_rgb("uniform", 48, 20, 12, k=5)
    dev = _dev(twin.code_frame(planes, 12), engine.device)
    for mode in ("pyramid", "prism"):
        got = twin.to_codes(_hostf(engine.apply_rgb_float(dev, interp=mode)), 12)
        assert _eq(got, orc.apply_rgb(lut.table, lut.scale, 12, mode, planes, prelut=pre)), mode
    # a new LUT without a prelut drops the uploaded table
    lut2 = engine.load_cube(_identity_cube(tmp_path))
    src = twin.make_float("natural", 64, 16, k=8)
    assert _eqf(_hostf(engine.apply_rgb_float(_dev(src, engine.device))), twin.apply_float(lut2.table, lut2.scale, "tetrahedral", src))


def _identity_cube(tmp_path):
    return cube.write_cube(tmp_path / "identity_9.cube", cube.identity_lattice(9))


# ------------------------------------------------------------------ rejections
@pytest.mark.gpu
def test_rejections_leave_the_buffers_alone(engine, cube_dir):
    import torch
    from lut_renderer_amd.engine import _planes_struct
    engine.load_cube(cube_dir / "log709_33.cube")
    dv = engine.device
    w, h = 64, 16
    src = [torch.full((h, w), 0.25, dtype=torch.float32, device=dv) for _ in range(3)]
    fdst = [torch.full((h, w), -3.0, dtype=torch.float32, device=dv) for _ in range(3)]
    ydst = [torch.full(s, 77, dtype=torch.uint8, device=dv) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]

    def untouched():
        torch.cuda.synchronize()
        return all(bool((t == 0.25).all()) for t in src) and all(bool((t == -3.0).all()) for t in fdst) and \
            all(bool((t == 77).all()) for t in ydst)

    def abi_f(s, d, interp=2):
        a, _ = _planes_struct(s, dv)
        b, _ = _planes_struct(d, dv)
        with engine._lock:
            engine._bind_stream()
            return engine._lib.lutr_apply_planar_rgb_f32(engine._ctx, interp, w, h, 1, C.byref(a), C.byref(b), 0, h), a, b

    def abi_y(s, d, fmt_out=_native.fmt_code(8, 1, 1), lut_depth=16, interp=2):
        a, _ = _planes_struct(s, dv)
        b, _ = _planes_struct(d, dv)
        p = _native.YuvParams(0, fmt_out, lut_depth, 0, 1, 0, 0, 0)
        with engine._lock:
            engine._bind_stream()
            return engine._lib.lutr_apply_rgbf_to_yuv(engine._ctx, C.byref(p), interp, 0, w, h, 1, C.byref(a), C.byref(b), 0, h)

    with _variant(engine, "vec_lds"):                      # there is no LDS kernel
        with pytest.raises(_native.LutrError) as e:
            engine.apply_rgb_float(src, fdst)
        assert e.value.code == _native.EINVAL
        with pytest.raises(_native.LutrError) as e:
            engine.apply_rgb_to_yuv(src, ydst, pix_fmt="gbrpf32le", out_pix_fmt="yuv420p")
        assert e.value.code == _native.EINVAL
    assert untouched()
    for depth in (8, 10, 15):                              # lut_depth != 16
        assert abi_y(src, ydst, lut_depth=depth) == _native.EINVAL
        assert b"lut_depth" in engine._lib.lutr_last_error()
    assert abi_y(src, ydst, fmt_out=_native.fmt_code(8, 0, 1)) == _native.EINVAL       # 4:4:0 output
    for interp in (5, -2):                                 # unknown interp (-1 is the YUV path's "no LUT" only)
        assert abi_f(src, fdst, interp)[0] == _native.EINVAL and abi_y(src, ydst, interp=interp) == _native.EINVAL
    assert abi_f(src, fdst, -1)[0] == _native.EINVAL
    assert untouched()
    # a stride that is not a multiple of 4 (described by hand: torch cannot make one)
    a, _ = _planes_struct(src, dv)
    b, _ = _planes_struct(fdst, dv)
    a.stride[1] = w * 4 + 2
    p = _native.YuvParams(0, _native.fmt_code(8, 1, 1), 16, 0, 1, 0, 0, 0)
    y, _ = _planes_struct(ydst, dv)
    with engine._lock:
        engine._bind_stream()
        assert engine._lib.lutr_apply_planar_rgb_f32(engine._ctx, 2, w, h, 1, C.byref(a), C.byref(b), 0, h) == _native.EINVAL
        assert b"multiples of 4" in engine._lib.lutr_last_error()
        assert engine._lib.lutr_apply_planar_rgb_f32(engine._ctx, 2, w, h, 1, C.byref(b), C.byref(a), 0, h) == _native.EINVAL
        assert engine._lib.lutr_apply_rgbf_to_yuv(engine._ctx, C.byref(p), 2, 0, w, h, 1, C.byref(a), C.byref(y), 0, h) == _native.EINVAL
    assert untouched()
    # overlapping source and destination on the YUV path: one buffer holding the source planes and, over the last of them, luma
    buf = torch.zeros(3 * h * w * 4 + h * w, dtype=torch.uint8, device=dv)
    fsrc = [buf[i * h * w * 4:(i + 1) * h * w * 4].view(torch.float32).view(h, w) for i in range(3)]
    for t in fsrc:
        t.fill_(0.5)
    odst = [buf[2 * h * w * 4 + 16:2 * h * w * 4 + 16 + h * w].view(h, w)] + ydst[1:]
    keep = buf.clone()
    with pytest.raises(ValueError, match="in place"):
        engine.apply_rgb_to_yuv(fsrc, odst, pix_fmt="gbrpf32le", out_pix_fmt="yuv420p")
    assert abi_y(fsrc, odst) == _native.EINVAL
    assert b"in place" in engine._lib.lutr_last_error()
    torch.cuda.synchronize()
    assert bool((buf == keep).all()) and untouched(), "a rejected call touched its buffers"
    # the Python layer's own refusals
    with pytest.raises(ValueError, match="chroma"):
        engine.apply_rgb_to_yuv(src, ydst, pix_fmt="gbrpf32le", out_pix_fmt="yuv420p", chroma_loc="left")
    with pytest.raises(ValueError):
        engine.apply_rgb_to_yuv(src, pix_fmt="gbrpf32le", out_pix_fmt="gbrp10le")
    with pytest.raises(ValueError, match="float32"):
        engine.apply_rgb_float([t.to(torch.float64) for t in src])
    with pytest.raises(ValueError, match="float32"):
        engine.apply_rgb_to_yuv([t.view(torch.int32) for t in src], ydst, pix_fmt="gbrpf32le", out_pix_fmt="yuv420p")
    assert untouched()


@pytest.mark.gpu
def test_fast_and_fma32_run_strict(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    src = twin.make_float("natural", 128, 64, k=6)
    try:
        for prec in ("fast", "fma32"):
            engine.set_precision(prec)
            got = _hostf(engine.apply_rgb_float(_dev(src, engine.device)))
            assert engine.last_kernel == "k_rgbf_vec<2>" and _eqf(got, twin.apply_float(lut.table, lut.scale, "tetrahedral", src))
            got = _hosty(engine.apply_rgb_to_yuv(_dev(src, engine.device), pix_fmt="gbrpf32le", out_pix_fmt="yuv420p10le"), 10)
            assert engine.last_kernel == _vec_name(10, "420", "tetrahedral")
            assert _eq(got, _want_yuv(lut, "tetrahedral", 10, "420", src)), prec
    finally:
        engine.set_precision("strict")


# ------------------------------------------------------------------ multi-GPU row sharding
@pytest.mark.gpu
def test_group_row_shards(engine, cube_dir):
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for name in ("gbrpf32le", "gbrapf32le"):
        for lay in ("420", "444"):
            for w, h in ((64, 23), (34, 37)):
                src = twin.make_float("natural", w, h, k=9)
                planes = src + ([np.full((h, w), 0.5, F)] if name == "gbrapf32le" else [])
                dev = _dev(planes, engine.device)
                single = _hosty(engine_apply(engine, lut, dev, name, lay), 10)
                assert _eq(single, _want_yuv(lut, "tetrahedral", 10, lay, src))
                for remote in (True, False):
                    with LutEngineGroup([0, 0], treat_as_remote=remote) as g:
                        g.set_lut(lut)
                        got = _hosty(g.apply_rgb_to_yuv(dev, pix_fmt=name, out_pix_fmt=_yuv(10, lay)), 10)
                        assert g.last_remote == int(remote)
                        assert all(r0 % (1 << LAYOUTS[lay][1]) == 0 for r0, _ in g.last_blocks), g.last_blocks
                        assert _eq(got, single), (name, lay, w, h, remote)


def engine_apply(engine, lut, dev, name, lay):
    engine.set_lut(lut)
    return engine.apply_rgb_to_yuv(dev, pix_fmt=name, out_pix_fmt=_yuv(10, lay))


# ------------------------------------------------------------------ apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut_routes(engine, cube_dir):
    from lut_renderer_amd.api import apply_lut
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    w, h = 64, 34
    src = twin.make_float("hdr", w, h, k=30)
    alpha = np.random.default_rng(1).uniform(0, 1, size=(h, w)).astype(F)
    want = twin.apply_float(lut.table, lut.scale, "trilinear", src)
    got, tags = apply_lut(_dev(src, engine.device), cube=lut, pix_fmt="gbrpf32le", interp="trilinear", width=w, height=h, engine=engine)
    assert engine.last_kernel == "k_rgbf_vec<1>" and _eqf(_hostf(got), want) and tags["colorspace"] == "bt709"
    got, _ = apply_lut(_dev(src + [alpha], engine.device), cube=lut, pix_fmt="gbrapf32le", out_pix_fmt="gbrapf32le", interp="trilinear",
                       engine=engine)
    assert len(got) == 4 and _eqf(_hostf(got), want + [alpha])
    got, _ = apply_lut(_dev(src + [alpha], engine.device), cube=lut, pix_fmt="gbrapf32le", out_pix_fmt="gbrpf32le", interp="trilinear",
                       engine=engine)
    assert len(got) == 3 and _eqf(_hostf(got), want)
    got, _ = apply_lut(_dev(src + [alpha], engine.device), cube=lut, pix_fmt="gbrapf32le", out_pix_fmt="yuv422p10le", colorspace="bt709",
                       engine=engine)
    assert _eq(_hosty(got, 10), _want_yuv(lut, "tetrahedral", 10, "422", src, matrix="bt709"))
    with pytest.raises(ValueError):
        apply_lut(_dev(src, engine.device), cube=lut, pix_fmt="gbrpf32le", zscale_dither="error_diffusion", engine=engine)


@pytest.mark.gpu
def test_cli_round_trip_over_pipes(engine, cube_dir):
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    w, h, nf = 64, 34, 3
    base = [sys.executable, "-m", "lut_renderer_amd.cli", "-i", "-", "-o", "-", "--size", f"{w}x{h}", "--cube",
            str(cube_dir / "log709_33.cube"), "--batch", "2", "--duration", f"{nf / 25.0:.3f}"]
    # gbrpf32le -> gbrpf32le
    fs = [twin.make_float("hdr", w, h, k=50 + i) for i in range(nf)]
    r = subprocess.run(base + ["--pix-fmt", "gbrpf32le"], input=b"".join(p.tobytes() for f in fs for p in f), capture_output=True,
                       cwd=ROOT, timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    engine.set_lut(lut)
    wants = [_hostf(engine.apply_rgb_float(_dev(f, engine.device))) for f in fs]
    assert all(_eqf(wnt, twin.apply_float(lut.table, lut.scale, "tetrahedral", f)) for wnt, f in zip(wants, fs))
    assert r.stdout == b"".join(p.tobytes() for wnt in wants for p in wnt)
    assert b"Duration: 00:00:00.12" in r.stderr and b"time=00:00:00.12" in r.stderr
    # gbrapf32le -> gbrapf32le: the alpha plane comes back unchanged
    rng = np.random.default_rng(5)
    alphas = [rng.uniform(-1, 2, size=(h, w)).astype(F) for _ in range(nf)]
    raw = b"".join(p.tobytes() for f, a in zip(fs, alphas) for p in f + [a])
    r = subprocess.run(base + ["--pix-fmt", "gbrapf32le"], input=raw, capture_output=True, cwd=ROOT, timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == b"".join(p.tobytes() for wnt, a in zip(wants, alphas) for p in wnt + [a])
    # gbrapf32le -> yuv420p10le: the alpha plane is dropped
    r = subprocess.run(base + ["--pix-fmt", "gbrapf32le", "--out-pix-fmt", "yuv420p10le"], input=raw, capture_output=True, cwd=ROOT,
                       timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    ywants = [_hosty(engine.apply_rgb_to_yuv(_dev(f, engine.device), pix_fmt="gbrpf32le", out_pix_fmt="yuv420p10le"), 10) for f in fs]
    assert all(_eq(wnt, _want_yuv(lut, "tetrahedral", 10, "420", f)) for wnt, f in zip(ywants, fs))
    assert r.stdout == b"".join(p.tobytes() for wnt in ywants for p in wnt)
