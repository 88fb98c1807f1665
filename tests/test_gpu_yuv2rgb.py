"""YUV sources with an RGB output on the GPU: lutr_apply_yuv_to_rgb bit for bit against the reference
composition of tests/_yuv2rgb_twin.py (stage 1 of the YUV contract, then the C oracle's lut3d at the destination's depth).  The
tolerance is zero: both sides are the same fp32 operations in the same order, as for every strict path."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from tests import _yuv2rgb_twin as twin
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
DESTS = ("gbrp", "gbrp10le", "gbrp12le", "gbrp16le", "rgb24", "bgr24", "rgba", "bgra", "argb", "abgr", "rgb48le", "rgba64le")
#: the depth pairs (din, dl) of the sweep, by destination depth dl
PAIRS = ((8, 8), (10, 10), (10, 8), (10, 16), (12, 12), (8, 10), (16, 8))
DINS = {dl: tuple(din for din, d in PAIRS if d == dl) for dl in (8, 10, 12, 16)}
CHILD_LIMIT_S = 240


def _yuv(depth, lay, alpha=False):
    return f"yuv{'a' if alpha else ''}{lay}p" + ("" if depth == 8 else f"{depth}le")


def _t(a, device):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def _dev(planes, device):
    return [_t(p, device) for p in planes]


def _host(out, out_fmt):
    """What a call returned, as the twin arranges it: a list of planes or one image, unsigned."""
    wide = twin.dest_depth(out_fmt) > 8
    conv = lambda t: t.cpu().numpy().view(np.uint16) if wide else t.cpu().numpy()    # noqa: E731
    return conv(out) if out_fmt in twin.PACKED else [conv(t) for t in out]


def _eq(got, want):
    if isinstance(want, np.ndarray):
        return isinstance(got, np.ndarray) and got.shape == want.shape and np.array_equal(got, want)
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _vec_name(din, lay, out_fmt, mode):
    icsx, icsy = LAYOUTS[lay]
    nc = twin.PACKED[out_fmt][1] if out_fmt in twin.PACKED else 1
    m = "nolut" if mode is None else str(MODES.index(mode))
    return f"k_yuv2rgb_vec<{int(din > 8)},{icsx},{icsy},{nc},{int(twin.dest_depth(out_fmt) > 8)},{m}>"


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


def _want(lt, mode, out_fmt, din, lay, src, **kw):
    icsx, icsy = LAYOUTS[lay]
    return twin.apply(lt.table, lt.scale, mode, out_fmt, din, icsx, icsy, src, **kw)


# ------------------------------------------------------------------ sources, destinations, depths, modes and routing
@pytest.mark.gpu
@pytest.mark.parametrize("out_fmt", DESTS)
def test_layouts_destinations_depths_and_modes(engine, cube_dir, out_fmt):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    dl = twin.dest_depth(out_fmt)
    w, h = 64, 32
    for dist in ("natural", "uniform"):
        for lay, (icsx, icsy) in LAYOUTS.items():
            for din in DINS[dl]:
                src = frames.make_yuv(dist, w, h, din, icsx, icsy, k=din + dl)
                dev = _dev(src, engine.device)
                kw = dict(pix_fmt=_yuv(din, lay), out_pix_fmt=out_fmt)
                for mode in MODES if dist == "natural" else ("tetrahedral",):
                    want = _want(lut, mode, out_fmt, din, lay, src)
                    with _variant(engine, "generic"):
                        got = _host(engine.apply_yuv_to_rgb(dev, interp=mode, **kw), out_fmt)
                        assert engine.last_kernel == "k_yuv2rgb_generic"
                    assert _eq(got, want), (out_fmt, dist, lay, din, mode, "generic")
                    has_vec = mode in VEC_MODES and not (din == 8 and dl > 8)
                    for variant in ("auto", "vec_global"):
                        with _variant(engine, variant):
                            if not has_vec and variant == "vec_global":
                                with pytest.raises(_native.LutrError) as e:
                                    engine.apply_yuv_to_rgb(dev, interp=mode, **kw)
                                assert e.value.code == _native.EINVAL
                                continue
                            got = _host(engine.apply_yuv_to_rgb(dev, interp=mode, **kw), out_fmt)
                            name = _vec_name(din, lay, out_fmt, mode) if has_vec else "k_yuv2rgb_generic"
                            assert engine.last_kernel == name, (variant, engine.last_kernel, name)
                        assert _eq(got, want), (out_fmt, dist, lay, din, mode, variant)


# ------------------------------------------------------------------ more than one workgroup, padded strides, sentinels
@pytest.mark.gpu
def test_block_boundary_padded_strides_and_sentinels(engine, cube_dir):
    """136 x 38 x 3 frames at 4:2:0: 17 x 19 x 3 units of the vector kernel, more than one 256-thread block and the last one
    partial.  Source and destination are views into larger buffers (padded rows, padded frames); nothing outside the views may
    change."""
    import torch
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    w, h, nf, padw, padh, x0 = 136, 38, 3, 160, 42, 8
    for din, out_fmt in ((10, "gbrp10le"), (8, "rgb24"), (10, "rgba64le"), (10, "rgb24")):
        fs = [frames.natural_yuv(w, h, din, 1, 1, k=20 + i) for i in range(nf)]
        sdt = torch.int16 if din > 8 else torch.uint8
        shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
        sbuf = [torch.full((nf, padh, padw), 77, dtype=sdt, device=engine.device) for _ in range(3)]
        src = [b[:, 2:2 + s[0], x0:x0 + s[1]] for b, s in zip(sbuf, shapes)]
        for i, f in enumerate(fs):
            for v, p in zip(src, f):
                v[i] = _t(p, engine.device)
        dl = twin.dest_depth(out_fmt)
        ddt = torch.int16 if dl > 8 else torch.uint8
        sentinel = -21846 if dl > 8 else 0xAA                      # 0xAAAA
        for variant in ("auto", "generic"):
            if out_fmt in twin.PACKED:
                nc = twin.PACKED[out_fmt][1]
                dbuf = [torch.full((nf, padh, padw, nc), sentinel, dtype=ddt, device=engine.device)]
                dst = dbuf[0][:, 2:2 + h, x0:x0 + w]
                views = [dst]
            else:
                dbuf = [torch.full((nf, padh, padw), sentinel, dtype=ddt, device=engine.device) for _ in range(3)]
                dst = [b[:, 2:2 + h, x0:x0 + w] for b in dbuf]
                views = dst
            with _variant(engine, variant):
                engine.apply_yuv_to_rgb(src, dst, pix_fmt=_yuv(din, "420"), out_pix_fmt=out_fmt)
                name = _vec_name(din, "420", out_fmt, "tetrahedral") if variant == "auto" else "k_yuv2rgb_generic"
                assert engine.last_kernel == name, (engine.last_kernel, name)
            got = _host(dst, out_fmt)
            for i, f in enumerate(fs):
                want = _want(lut, "tetrahedral", out_fmt, din, "420", f)
                one = got[i] if out_fmt in twin.PACKED else [g[i] for g in got]
                assert _eq(one, want), (din, out_fmt, variant, i)
            for b, v in zip(dbuf, views):
                v.fill_(sentinel)
                assert bool((b == sentinel).all()), (din, out_fmt, variant, "wrote outside the destination")
        assert all(bool((b[:, :2] == 77).all()) and bool((b[:, :, :x0] == 77).all()) for b in sbuf)


# ------------------------------------------------------------------ shapes
@pytest.mark.gpu
def test_ragged_odd_negative_strides_and_a_misaligned_base(engine, cube_dir):
    import torch
    from lut_renderer_amd.engine import _packed_struct, _planes_struct
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for din, out_fmt in ((10, "gbrp10le"), (8, "rgb24"), (10, "rgba64le"), (10, "bgr24")):
        dl = twin.dest_depth(out_fmt)
        sdt, ddt = (torch.int16 if din > 8 else torch.uint8), (torch.int16 if dl > 8 else torch.uint8)
        fill = -1 if dl > 8 else 255
        for lay, (icsx, icsy) in LAYOUTS.items():
            kw = dict(pix_fmt=_yuv(din, lay), out_pix_fmt=out_fmt)
            # a ragged width on padded (aligned) rows: the vector kernel up to the last unit, the generic kernel for the tail
            w, h, pad = 70, 22, 96
            f = frames.natural_yuv(w, h, din, icsx, icsy, k=4)
            sp = [torch.zeros((p.shape[0], pad), dtype=sdt, device=engine.device) for p in f]
            src = []
            for t, p in zip(sp, f):
                t[:, :p.shape[1]] = _t(p, engine.device)
                src.append(t[:, :p.shape[1]])
            if out_fmt in twin.PACKED:
                dp = torch.full((h, pad, twin.PACKED[out_fmt][1]), fill, dtype=ddt, device=engine.device)
                dst, tails = dp[:, :w], [dp[:, w:]]
            else:
                dp = [torch.full((h, pad), fill, dtype=ddt, device=engine.device) for _ in range(3)]
                dst, tails = [t[:, :w] for t in dp], [t[:, w:] for t in dp]
            engine.apply_yuv_to_rgb(src, dst, **kw)
            assert engine.last_kernel == _vec_name(din, lay, out_fmt, "tetrahedral"), engine.last_kernel
            assert _eq(_host(dst, out_fmt), _want(lut, "tetrahedral", out_fmt, din, lay, f)), (din, out_fmt, lay, "ragged")
            assert all(bool((t == fill).all()) for t in tails), "wrote past the row"
            with _variant(engine, "vec_global"):
                with pytest.raises(_native.LutrError):
                    engine.apply_yuv_to_rgb(src, dst, **kw)
            # odd width and height: the generic kernel, partial chroma blocks at the right and bottom edges
            for w, h in ((67, 21), (1, 1), (3, 5)):
                f = frames.natural_yuv(w, h, din, icsx, icsy, k=w)
                got = _host(engine.apply_yuv_to_rgb(_dev(f, engine.device), **kw), out_fmt)
                assert engine.last_kernel == "k_yuv2rgb_generic", engine.last_kernel
                assert _eq(got, _want(lut, "tetrahedral", out_fmt, din, lay, f)), (din, out_fmt, lay, w, h)
    # a base pointer one sample off the vector kernel's alignment: generic under auto, EINVAL under vec_global
    w, h = 64, 16
    f = frames.natural_yuv(w, h, 10, 1, 1, k=6)
    big = torch.zeros((h, w + 8), dtype=torch.int16, device=engine.device)
    big[:, 1:w + 1] = _t(f[0], engine.device)
    src = [big[:, 1:w + 1]] + _dev(f[1:], engine.device)
    got = _host(engine.apply_yuv_to_rgb(src, pix_fmt="yuv420p10le", out_pix_fmt="gbrp10le"), "gbrp10le")
    assert engine.last_kernel == "k_yuv2rgb_generic"
    assert _eq(got, _want(lut, "tetrahedral", "gbrp10le", 10, "420", f))
    dimg = torch.zeros((h, w + 2, 3), dtype=torch.uint8, device=engine.device)
    dflat = dimg.view(-1)[1:1 + h * (w + 2) * 3 - 3].as_strided((h, w, 3), ((w + 2) * 3, 3, 1))      # one byte off a dword
    got = engine.apply_yuv_to_rgb(_dev(f, engine.device), dflat, pix_fmt="yuv420p10le", out_pix_fmt="rgb24")
    assert engine.last_kernel == "k_yuv2rgb_generic"
    assert _eq(_host(got, "rgb24"), _want(lut, "tetrahedral", "rgb24", 10, "420", f))
    with _variant(engine, "vec_global"):
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv_to_rgb(src, pix_fmt="yuv420p10le", out_pix_fmt="gbrp10le")
        assert e.value.code == _native.EINVAL
    # negative row strides on both sides (bottom-up images; torch has none, so through the C ABI): the generic kernel
    base = [_t(p[::-1], engine.device) for p in f]                 # rows stored bottom-up
    st, _ = _planes_struct(base, engine.device)
    for i, p in enumerate(f):
        st.data[i] = base[i].data_ptr() + (p.shape[0] - 1) * p.shape[1] * 2
        st.stride[i] = -p.shape[1] * 2
    p = _native.YuvParams(_native.fmt_code(10, 1, 1), 0, 10, 0, 0, 0, 0, 0)
    dst = [torch.zeros((h, w), dtype=torch.int16, device=engine.device) for _ in range(3)]
    d, _ = _planes_struct(dst, engine.device)
    for i in range(3):
        d.data[i] = dst[i].data_ptr() + (h - 1) * w * 2
        d.stride[i] = -w * 2
    for variant, rc in (("auto", 0), ("vec_global", _native.EINVAL)):
        with _variant(engine, variant), engine._lock:
            engine._bind_stream()
            assert engine._lib.lutr_apply_yuv_to_rgb(engine._ctx, C.byref(p), 2, 0, w, h, 1, C.byref(st), C.byref(d), None, 0, h) == rc
    assert engine.last_kernel == "k_yuv2rgb_generic"
    want = _want(lut, "tetrahedral", "gbrp10le", 10, "420", f)
    assert _eq([g[::-1] for g in _host(dst, "gbrp10le")], want)
    img = torch.zeros((h, w, 4), dtype=torch.uint8, device=engine.device)
    pk = _packed_struct(img, "bgra", 4, 8, engine.device, True)
    pk.data = img.data_ptr() + (h - 1) * w * 4
    pk.stride = -w * 4
    p8 = _native.YuvParams(_native.fmt_code(10, 1, 1), 0, 8, 0, 0, 0, 0, 0)
    with engine._lock:
        engine._bind_stream()
        code = _native.packed_code(*_native.PACKED_FORMATS["bgra"])
        assert engine._lib.lutr_apply_yuv_to_rgb(engine._ctx, C.byref(p8), 2, code, w, h, 1, C.byref(st), None, C.byref(pk), 0, h) == 0
    assert _eq(_host(img, "bgra")[::-1], _want(lut, "tetrahedral", "bgra", 10, "420", f))


# ------------------------------------------------------------------ lattices and options
@pytest.mark.gpu
def test_other_luts_matrices_ranges_prologue_and_no_lut(engine, cube_dir, tmp_path):
    from oracle import binding as orc
    for name in ("random_9.cube", "domain_2.cube", "identity_17.cube"):
        lut = engine.load_cube(cube_dir / name)
        for din, out_fmt in ((10, "gbrp10le"), (8, "rgb24"), (10, "rgba64le")):
            for lay, (icsx, icsy) in LAYOUTS.items():
                f = frames.uniform_yuv(48, 20, din, icsx, icsy, k=2)
                got = _host(engine.apply_yuv_to_rgb(_dev(f, engine.device), pix_fmt=_yuv(din, lay), out_pix_fmt=out_fmt), out_fmt)
                assert _eq(got, _want(lut, "tetrahedral", out_fmt, din, lay, f)), (name, out_fmt, lay)
    # a .csp prelut
    tab = cube.log709_lattice(17)
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    path = tmp_path / "shaped.csp"
    write_csp_with_prelut(path, 17, tab, shapers)
    lut = engine.load_cube(path)
    assert lut.prelut is not None
    pre = orc.parse_lut_file_ex(path)[3]
    for din, out_fmt in ((10, "gbrp10le"), (8, "rgb24"), (10, "rgb48le")):
        f = frames.natural_yuv(48, 30, din, 1, 1, k=2)
        for mode in ("tetrahedral", "prism"):
            got = _host(engine.apply_yuv_to_rgb(_dev(f, engine.device), pix_fmt=_yuv(din, "420"), out_pix_fmt=out_fmt, interp=mode),
                        out_fmt)
            assert _eq(got, _want(lut, mode, out_fmt, din, "420", f, prelut=pre)), (out_fmt, mode, engine.last_kernel)
    # every matrix x range, at equal depths and across a depth change
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for m in ("bt709", "smpte170m", "bt2020nc"):
        for rng in ("tv", "pc"):
            for din, out_fmt in ((10, "gbrp10le"), (10, "rgb24"), (8, "gbrp12le")):
                f = frames.make_yuv("natural", 64, 16, din, 1, 1, k=3, full_range=rng == "pc")
                got = _host(engine.apply_yuv_to_rgb(_dev(f, engine.device), pix_fmt=_yuv(din, "420"), out_pix_fmt=out_fmt,
                                                    matrix_in=m, range_src=rng), out_fmt)
                assert _eq(got, _want(lut, "tetrahedral", out_fmt, din, "420", f, matrix=m, range_src=rng)), (m, rng, out_fmt)
    # the pc-source prologue into an 8-bit destination (the reference's scale=in_range=pc:...,format=yuv4xxp ahead of lut3d)
    for din in (8, 10):
        for out_fmt in ("gbrp", "rgb24", "bgra"):
            for lay, (icsx, icsy) in LAYOUTS.items():
                f = frames.make_yuv("natural", 64, 16, din, icsx, icsy, k=8, full_range=True)
                for variant in ("auto", "generic"):
                    with _variant(engine, variant):
                        got = _host(engine.apply_yuv_to_rgb(_dev(f, engine.device), pix_fmt=_yuv(din, lay), out_pix_fmt=out_fmt,
                                                            range_src="pc", range_in="tv"), out_fmt)
                    want = _want(lut, "tetrahedral", out_fmt, din, lay, f, range_src="pc", range_in="tv")
                    assert _eq(got, want), (din, out_fmt, lay, variant)
    with pytest.raises(_native.LutrError, match="full-range"):           # a tv source has no range prologue, as today
        engine.apply_yuv_to_rgb(_dev(frames.natural_yuv(64, 16, 10, 0, 0), engine.device), pix_fmt=_yuv(10, "444"),
                                out_pix_fmt="rgb24", range_src="tv", range_in="pc")
    # lut=False: the converted codes are stored (no lattice is read)
    for din, out_fmt in ((10, "gbrp10le"), (8, "rgb24"), (10, "abgr"), (16, "rgb48le")):
        for w, h in ((64, 32), (37, 19)):
            for lay, (icsx, icsy) in LAYOUTS.items():
                f = frames.uniform_yuv(w, h, din, icsx, icsy, k=5)
                got = _host(engine.apply_yuv_to_rgb(_dev(f, engine.device), pix_fmt=_yuv(din, lay), out_pix_fmt=out_fmt, lut=False),
                            out_fmt)
                assert engine.last_kernel == (_vec_name(din, lay, out_fmt, None) if w % 8 == 0 else "k_yuv2rgb_generic")
                assert _eq(got, _want(lut, None, out_fmt, din, lay, f, lut=False)), (out_fmt, w, h, lay)


@pytest.mark.gpu
def test_fast_and_fma32_run_strict(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    try:
        for prec in ("fast", "fma32"):
            engine.set_precision(prec)
            for din, out_fmt in ((10, "gbrp10le"), (8, "rgb24")):
                f = frames.natural_yuv(128, 64, din, 1, 1, k=6)
                got = _host(engine.apply_yuv_to_rgb(_dev(f, engine.device), pix_fmt=_yuv(din, "420"), out_pix_fmt=out_fmt), out_fmt)
                assert _eq(got, _want(lut, "tetrahedral", out_fmt, din, "420", f)), (prec, out_fmt)
                assert engine.last_kernel == _vec_name(din, "420", out_fmt, "tetrahedral"), engine.last_kernel
    finally:
        engine.set_precision("strict")


# ------------------------------------------------------------------ host layers
@pytest.mark.gpu
def test_row_shards_reproduce_the_whole_call(engine, cube_dir):
    engine.load_cube(cube_dir / "log709_33.cube")
    for din, out_fmt in ((10, "gbrp10le"), (8, "rgb24"), (10, "rgba64le")):
        for lay, (icsx, icsy) in LAYOUTS.items():
            bh = 1 << icsy
            kw = dict(pix_fmt=_yuv(din, lay), out_pix_fmt=out_fmt)
            for w, h in ((64, 22), (31, 23)):
                dev = _dev(frames.natural_yuv(w, h, din, icsx, icsy, k=12), engine.device)
                whole = _host(engine.apply_yuv_to_rgb(dev, **kw), out_fmt)
                for r0 in range(bh, h, bh):                        # every (row0, rows) on the block rule, as a pair of calls
                    out = engine.apply_yuv_to_rgb(dev, row0=0, rows=r0, **kw)
                    engine.apply_yuv_to_rgb(dev, out, row0=r0, rows=h - r0, **kw)
                    assert _eq(_host(out, out_fmt), whole), (out_fmt, lay, w, h, r0)
                if bh == 2:
                    with pytest.raises(_native.LutrError) as e:
                        engine.apply_yuv_to_rgb(dev, row0=1, rows=h - 1, **kw)
                    assert e.value.code == _native.EINVAL and "block height" in e.value.message


@pytest.mark.gpu
def test_group_row_shards(engine, cube_dir):
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for din, out_fmt, alpha in ((10, "gbrp10le", False), (8, "rgb24", False), (10, "rgba64le", False), (10, "gbrap10le", True)):
        for lay in ("420", "444"):
            icsx, icsy = LAYOUTS[lay]
            for w, h in ((64, 23), (34, 37)):
                f = frames.natural_yuv(w, h, din, icsx, icsy, k=9)
                want = _want(lut, "tetrahedral", out_fmt, din, lay, f)
                if alpha:
                    a = np.random.default_rng(5).integers(0, 1 << din, size=(h, w)).astype(np.uint16)
                    f, want = f + [a], want[:3] + [a]
                for n in (2, 3):
                    with LutEngineGroup([0] * n, treat_as_remote=True) as g:
                        g.set_lut(lut)
                        got = _host(g.apply_yuv_to_rgb(_dev(f, engine.device), pix_fmt=_yuv(din, lay, alpha), out_pix_fmt=out_fmt),
                                    out_fmt)
                        assert g.last_remote == n - 1
                        assert all(r0 % (1 << icsy) == 0 for r0, _ in g.last_blocks), g.last_blocks
                        assert _eq(got, want), (out_fmt, lay, w, h, n)
    f = frames.natural_yuv(64, 24, 8, 1, 1, k=3)
    with LutEngineGroup([0, 0]) as g:                      # same device: launches on the caller's buffers
        g.set_lut(lut)
        got = _host(g.apply_yuv_to_rgb(_dev(f, engine.device), pix_fmt="yuv420p", out_pix_fmt="bgra"), "bgra")
        assert g.last_remote == 0 and _eq(got, _want(lut, "tetrahedral", "bgra", 8, "420", f))


@pytest.mark.gpu
def test_alpha_sources(engine, cube_dir):
    """yuva420p10le -> gbrap10le carries alpha (converted when the depths differ), -> gbrp10le / a 3-component name drops it, a
    yuv* source fills it opaque, and a 4-component packed destination is refused by name."""
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 64, 22
    f = frames.natural_yuv(w, h, 10, 1, 1, k=31)
    a = np.random.default_rng(9).integers(0, 1024, size=(h, w)).astype(np.uint16)
    dev = _dev(f + [a], engine.device)
    want = _want(lut, "tetrahedral", "gbrp10le", 10, "420", f)
    got = engine.apply_yuv_to_rgb(dev, pix_fmt="yuva420p10le", out_pix_fmt="gbrap10le")
    assert len(got) == 4 and _eq(_host(got, "gbrap10le"), want + [a])
    assert engine.last_kernel.startswith(_vec_name(10, "420", "gbrp10le", "tetrahedral") + "+k_alpha"), engine.last_kernel
    got = engine.apply_yuv_to_rgb(dev, pix_fmt="yuva420p10le", out_pix_fmt="gbrp10le")
    assert len(got) == 3 and _eq(_host(got, "gbrp10le"), want)
    got = engine.apply_yuv_to_rgb(dev, pix_fmt="yuva420p10le", out_pix_fmt="rgb24")
    assert _eq(_host(got, "rgb24"), _want(lut, "tetrahedral", "rgb24", 10, "420", f))
    got = _host(engine.apply_yuv_to_rgb(dev[:3], pix_fmt="yuv420p10le", out_pix_fmt="gbrap10le"), "gbrap10le")
    assert _eq(got, want + [np.full((h, w), 1023, np.uint16)])
    got = _host(engine.apply_yuv_to_rgb(dev, pix_fmt="yuva420p10le", out_pix_fmt="gbrap"), "gbrap")      # 10 -> 8 bit: nearest code
    a8 = ((a.astype(np.uint64) * 255 * 2 + 1023) // (2 * 1023)).astype(np.uint8)
    assert _eq(got, _want(lut, "tetrahedral", "gbrp", 10, "420", f) + [a8])
    for out in ("rgba", "bgra", "argb", "rgba64le"):
        with pytest.raises(ValueError, match="follow-up"):
            engine.apply_yuv_to_rgb(dev, pix_fmt="yuva420p10le", out_pix_fmt=out)
    with pytest.raises(ValueError):                        # three planes for a four-plane name
        engine.apply_yuv_to_rgb(dev[:3], pix_fmt="yuva420p10le", out_pix_fmt="gbrp10le")


@pytest.mark.gpu
def test_engine_refusals_and_allocation(engine, cube_dir):
    import torch
    engine.load_cube(cube_dir / "log709_33.cube")
    f = frames.natural_yuv(64, 16, 10, 1, 1, k=1)
    dev = _dev(f, engine.device)
    kw = dict(pix_fmt="yuv420p10le", out_pix_fmt="gbrp10le")
    for extra, word in ((dict(chroma_loc="left"), "chroma_loc"), (dict(dither="error_diffusion"), "dither"),
                        (dict(dither="blue_noise"), "dither"), (dict(out_size=(32, 8)), "out_size"),
                        (dict(alpha_mode="premultiplied"), "premultiplied"), (dict(cdl=object()), "cdl"), (dict(lut1d=object()), "lut1d"),
                        (dict(stages=("lut3d",)), "stages"), (dict(strength=0.5), "strength"), (dict(matte=dev[0]), "matte"),
                        (dict(out2_pix_fmt="yuv420p"), "second output"), (dict(cube2="b.cube"), "cube2")):
        with pytest.raises(ValueError, match=word):
            engine.apply_yuv_to_rgb(dev, **kw, **extra)
    for src_fmt, word in (("nv12", "semi-planar"), ("uyvy422", "packed 4:2:2"), ("v210", "v210")):
        with pytest.raises(ValueError, match=word):
            engine.apply_yuv_to_rgb(dev, pix_fmt=src_fmt, out_pix_fmt="rgb24")
    with pytest.raises(ValueError, match="float"):
        engine.apply_yuv_to_rgb(dev, pix_fmt="yuv420p10le", out_pix_fmt="gbrpf32le")
    with pytest.raises(ValueError, match="planar YUV"):    # the old entry point still refuses
        engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_pix_fmt="gbrp10le")
    # allocation: uint8 up to 8 bit, int16 above; planes or one [F,]H,W,C tensor
    out = engine.apply_yuv_to_rgb(dev, pix_fmt="yuv420p10le", out_pix_fmt="gbrp")
    assert len(out) == 3 and all(t.dtype == torch.uint8 and tuple(t.shape) == (16, 64) for t in out)
    out = engine.apply_yuv_to_rgb(dev, pix_fmt="yuv420p10le", out_pix_fmt="gbrp16le")
    assert all(t.dtype == torch.int16 for t in out)
    out = engine.apply_yuv_to_rgb([t.unsqueeze(0) for t in dev], pix_fmt="yuv420p10le", out_pix_fmt="rgba64le")
    assert out.dtype == torch.int16 and tuple(out.shape) == (1, 16, 64, 4)
    out = engine.apply_yuv_to_rgb(dev, pix_fmt="yuv420p10le", out_pix_fmt="bgr24")
    assert out.dtype == torch.uint8 and tuple(out.shape) == (16, 64, 3)


@pytest.mark.gpu
def test_apply_lut_host_pipeline_and_cli(engine, cube_dir, tmp_path):
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.stream import HostPipeline
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    w, h, nf = 64, 36, 3
    for din, out_fmt in ((10, "rgb48le"), (8, "rgb24"), (10, "gbrp10le")):
        src_fmt = _yuv(din, "420")
        fs = [frames.natural_yuv(w, h, din, 1, 1, k=30 + i) for i in range(nf)]
        wants = [_want(lut, "tetrahedral", out_fmt, din, "420", f, matrix="bt709") for f in fs]
        got, tags = apply_lut(_dev(fs[0], engine.device), cube=lut, pix_fmt=src_fmt, colorspace="bt709", rgb_out=out_fmt, width=w,
                              height=h, engine=engine)
        assert _eq(_host(got, out_fmt), wants[0]) and tags["colorspace"] == "bt709"
        raw_out = b"".join((wnt.tobytes() if isinstance(wnt, np.ndarray) else b"".join(p.tobytes() for p in wnt)) for wnt in wants)
        pipe = HostPipeline(engine, src_fmt, w, h, batch=2, rgb_out=out_fmt, interp="tetrahedral", matrix_in="bt709")
        raw = [b"".join(p.tobytes() for p in f) for f in fs]
        assert all(len(r) == pipe.fin.frame_bytes for r in raw) and pipe.fout.frame_bytes * nf == len(raw_out)
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
        assert state["out"] == raw_out, out_fmt
    with pytest.raises(ValueError, match="mutually exclusive"):
        apply_lut(_dev(fs[0], engine.device), cube=lut, pix_fmt="yuv420p10le", out_pix_fmt="yuv444p10le", rgb_out="rgb24", engine=engine)
    with pytest.raises(ValueError, match="chroma_loc"):
        apply_lut(_dev(fs[0], engine.device), cube=lut, pix_fmt="yuv420p10le", rgb_out="rgb24", chroma_loc="left", engine=engine)
    # the CLI on a rawvideo file: yuv420p10le in, rgb48le and gbrp10le out
    fs = [frames.natural_yuv(w, h, 10, 1, 1, k=50 + i) for i in range(nf)]
    (tmp_path / "in.yuv").write_bytes(b"".join(p.tobytes() for f in fs for p in f))
    for out_fmt in ("rgb48le", "gbrp10le"):
        out_path = tmp_path / f"out_{out_fmt}.raw"
        cmd = [sys.executable, "-m", "lut_renderer_amd.cli", "-i", str(tmp_path / "in.yuv"), "-o", str(out_path), "--size", f"{w}x{h}",
               "--pix-fmt", "yuv420p10le", "--rgb-out", out_fmt, "--cube", str(cube_dir / "log709_33.cube"), "--batch", "2"]
        r = subprocess.run(cmd, capture_output=True, cwd=ROOT, timeout=180, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        wants = [_want(lut, "tetrahedral", out_fmt, 10, "420", f, matrix="smpte170m") for f in fs]
        raw_out = b"".join((wnt.tobytes() if isinstance(wnt, np.ndarray) else b"".join(p.tobytes() for p in wnt)) for wnt in wants)
        assert out_path.read_bytes() == raw_out, out_fmt
        assert "Duration: 00:00:00.12" in r.stdout and "time=00:00:00.12" in r.stdout


# ------------------------------------------------------------------ the generic kernel several trips deep
@pytest.mark.gpu
def test_generic_kernel_many_trips_deep(orc, cube_dir, tmp_path):
    """k_yuv2rgb_generic under LUTR_MAX_BLOCKS=1 on 136 x 36 x 3 frames: one workgroup walks 68 x 18 x 3 = 3672 blocks, 15 trips a
    thread and the last one partial.  The variable is read once per process, so a child runs it (tests/_yuv2rgb_stride_worker.py)."""
    from tests import _yuv2rgb_stride_worker as worker
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    w, h, nf = 136, 36, 3
    env = dict(os.environ, LUTR_MAX_BLOCKS="1")
    for din, out_fmt in ((10, "gbrp10le"), (8, "rgba")):
        out = tmp_path / f"stride_{out_fmt}.npz"
        cmd = [sys.executable, str(ROOT / "tests" / "_yuv2rgb_stride_worker.py"), str(cube_dir / "log709_33.cube"), str(out), str(w),
               str(h), str(nf), str(din), out_fmt]
        try:
            p = subprocess.run(cmd, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"the LUTR_MAX_BLOCKS=1 child did not finish within {CHILD_LIMIT_S} s:\n{str(e.stderr)[-2000:]}", pytrace=False)
        assert p.returncode == 0, p.stderr[-3000:]
        z = np.load(out)
        assert str(z["kernel"]) == "k_yuv2rgb_generic"
        src = worker.source(w, h, nf, din)
        wide = twin.dest_depth(out_fmt) > 8
        got = [z[f"p{i}"].view(np.uint16) if wide else z[f"p{i}"] for i in range(len(z.files) - 1)]
        for i in range(nf):
            want = _want(lut, "tetrahedral", out_fmt, din, "420", [s[i] for s in src])
            one = got[0][i] if out_fmt in twin.PACKED else [g[i] for g in got]
            assert _eq(one, want), (out_fmt, i)


# ------------------------------------------------------------------ the C ABI's refusals
@pytest.mark.gpu
def test_abi_refusals(engine, cube_dir):
    import torch
    from lut_renderer_amd.engine import _packed_struct, _planes_struct
    engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 64, 16
    lib, ctx = engine._lib, engine._ctx

    def call(p, kind, s, d_planar, d_packed, rows=h):
        with engine._lock:
            engine._bind_stream()
            return lib.lutr_apply_yuv_to_rgb(ctx, C.byref(p), 2, kind, w, h, 1, C.byref(s), None if d_planar is None else C.byref(d_planar),
                                             None if d_packed is None else C.byref(d_packed), 0, rows)

    # overlap: one buffer holding the source planes and, over the end of the last of them, the first destination plane
    buf = torch.zeros(h * w + 2 * (h // 2) * (w // 2) + 3 * h * w, dtype=torch.uint8, device=engine.device)
    n_src = h * w + 2 * (h // 2) * (w // 2)
    buf[:n_src] = 77
    src = [buf[:h * w].view(h, w), buf[h * w:h * w + (h // 2) * (w // 2)].view(h // 2, w // 2),
           buf[h * w + (h // 2) * (w // 2):n_src].view(h // 2, w // 2)]
    dst = [buf[n_src - 8 + i * h * w:n_src - 8 + (i + 1) * h * w].view(h, w) for i in range(3)]
    with pytest.raises(ValueError, match="in place"):
        engine.apply_yuv_to_rgb(src, dst, pix_fmt="yuv420p", out_pix_fmt="gbrp")
    s, _ = _planes_struct(src, engine.device)
    d, _ = _planes_struct(dst, engine.device)
    p8 = _native.YuvParams(_native.fmt_code(8, 1, 1), 0, 8, 0, 0, 0, 0, 0)
    assert call(p8, 0, s, d, None) == _native.EINVAL and b"in place" in lib.lutr_last_error()
    img = buf[n_src - 8:n_src - 8 + h * w * 3].view(h, w, 3)
    pk = _packed_struct(img, "rgb24", 3, 8, engine.device, True)
    rgb24 = _native.packed_code(*_native.PACKED_FORMATS["rgb24"])
    assert call(p8, rgb24, s, None, pk) == _native.EINVAL and b"in place" in lib.lutr_last_error()
    torch.cuda.synchronize()
    assert bool((buf[:n_src] == 77).all()) and bool((buf[n_src:] == 0).all()), "a rejected call touched its buffers"
    # a good destination from here on
    good = [torch.zeros((h, w), dtype=torch.uint8, device=engine.device) for _ in range(3)]
    d, _ = _planes_struct(good, engine.device)
    gimg = torch.zeros((h, w, 3), dtype=torch.uint8, device=engine.device)
    pk = _packed_struct(gimg, "rgb24", 3, 8, engine.device, True)
    assert call(p8, 0, s, d, None) == 0 and call(p8, rgb24, s, None, pk) == 0
    # 4:4:0
    p440 = _native.YuvParams(_native.fmt_code(8, 0, 1), 0, 8, 0, 0, 0, 0, 0)
    assert call(p440, 0, s, d, None) == _native.EINVAL and b"4:4:0" in lib.lutr_last_error()
    # a lut_depth that is no depth of a destination, and packed bits other than lut_depth
    for dl in (7, 17, 0):
        bad = _native.YuvParams(_native.fmt_code(8, 1, 1), 0, dl, 0, 0, 0, 0, 0)
        assert call(bad, 0, s, d, None) == _native.EINVAL
    p10 = _native.YuvParams(_native.fmt_code(8, 1, 1), 0, 10, 0, 0, 0, 0, 0)
    assert call(p10, rgb24, s, None, pk) == _native.EINVAL and b"lut_depth" in lib.lutr_last_error()
    p16 = _native.YuvParams(_native.fmt_code(8, 1, 1), 0, 16, 0, 0, 0, 0, 0)
    assert call(p16, rgb24, s, None, pk) == _native.EINVAL and b"lut_depth" in lib.lutr_last_error()
    assert call(p8, _native.packed_code(12, 3, 0, 1, 2), s, None, pk) == _native.EINVAL          # no such packed format
    # rows off the chroma block, null planes, vec_lds
    assert call(p8, 0, s, d, None, rows=5) == _native.EINVAL and b"block height" in lib.lutr_last_error()
    assert call(p8, 0, s, None, None) == _native.EINVAL
    with _variant(engine, "vec_lds"):
        assert call(p8, 0, s, d, None) == _native.EINVAL
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv_to_rgb(src, good, pix_fmt="yuv420p", out_pix_fmt="gbrp")
        assert e.value.code == _native.EINVAL
