"""Packed 4:2:2 YUV frames in and out of the fused LUT pass on the GPU.  The expected output is the C oracle's
fused YUV result on the de-interleaved (`to_planar`) frames passed through `to_packed`; for a 4:2:0 / 4:4:4 destination it is the
subsampling-change twin (tests/_xsub_twin.py).  Every comparison is array_equal on whole buffers."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.engine import parse_packed_yuv_fmt, yuv_side
from lut_renderer_amd.packedyuv import to_packed, to_planar
from tests import _xsub_twin as twin
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
PACKED = ("yuyv422", "uyvy422", "yvyu422", "y210le", "y212le", "y216le")
# packed <-> planar both ways, the orders against each other, 10 -> 8 bit (and 8 -> 10, which has no vector kernel)
MIXES = (("uyvy422", "yuv422p"), ("yuv422p", "yuyv422"), ("y210le", "yuv422p10le"), ("yuv422p10le", "y210le"),
         ("yvyu422", "uyvy422"), ("y210le", "yuyv422"), ("y210le", "yuv422p"), ("yuv422p10le", "uyvy422"), ("uyvy422", "y210le"))
XSUB = (("uyvy422", "yuv420p"), ("y210le", "yuv420p10le"), ("y210le", "yuv420p"))
W, H = 64, 8

_luts = {}
_refs = {}


def _lut(engine, cube_dir, name):
    """The parsed LUT (read once per session), uploaded to the engine."""
    if name not in _luts:
        _luts[name] = cube.read_lut(cube_dir / name)
    engine.set_lut(_luts[name])
    return _luts[name]


def _planar_name(name):
    f = parse_packed_yuv_fmt(name)
    return f.planar if f is not None else name


def _want(orc, lutname, lut, mode, src_name, out_name, dist, w, h, k, rng_src="tv", lut_depth=None, prelut=None):
    """(planar source codes, planar expected codes) of one frame, computed once per distinct case and shared (never modified).
    The source goes through `to_packed` / `to_planar` first, so it is the frame the packed buffer really holds."""
    fin, fout = yuv_side(src_name), yuv_side(out_name)
    dl = lut_depth or fin.depth
    key = (lutname, mode, fin.depth, fout.depth, fout.csx, fout.csy, dist, w, h, k, rng_src, dl)
    if key not in _refs:
        src = frames.make_yuv(dist, w, h, fin.depth, 1, 0, k=k, full_range=(rng_src == "pc"))
        src = to_planar(to_packed(src, "yuyv422" if fin.depth == 8 else "y216le"), "yuyv422" if fin.depth == 8 else "y216le", w)
        prologue = fin.depth != dl
        if (fout.csx, fout.csy) == (1, 0):
            kc = orc.yuv_constants("bt709", rng_src, "bt709", "tv", fin.depth, dl, fout.depth, 2, prologue=prologue)
            out = orc.apply_yuv(lut.table, lut.scale, mode, kc, fin.depth, dl, fout.depth, 1, 0, src, prelut=prelut)
        else:
            kc = twin.consts("bt709", rng_src, "bt709", "tv", fin.depth, dl, fout.depth, fout.csx, fout.csy, prologue=prologue)
            out = twin.apply(lut.table, lut.scale, mode, kc, dl, fout.depth, 1, 0, fout.csx, fout.csy, src, prelut=prelut)
        for p in list(src) + list(out):
            p.setflags(write=False)
        _refs[key] = (src, out)
    return _refs[key]


def _side(planes, name):
    """Planar codes -> what `apply_yuv` takes for the container `name`: [one packed buffer] or the three planes."""
    return [to_packed(planes, name)] if parse_packed_yuv_fmt(name) is not None else list(planes)


def _dev(planes, device):
    import torch
    return [torch.from_numpy(np.array(p).view(np.int16) if p.dtype == np.uint16 else np.array(p)).to(device)   # (a copy: the shared
            for p in planes]                                                                                   # references are read-only)


def _host(tensors, name):
    wide = yuv_side(name).depth > 8
    tensors = [tensors] if hasattr(tensors, "shape") else tensors
    return [t.cpu().numpy().view(np.uint16) if wide else t.cpu().numpy() for t in tensors]


def _eq(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


def _batch(per_frame):
    """[frame][plane] -> [plane] stacked over frames."""
    return [np.stack([f[i] for f in per_frame]) for i in range(len(per_frame[0]))]


class _variant:
    def __init__(self, engine, name):
        self.engine, self.name = engine, name

    def __enter__(self):
        self.engine.set_variant(self.name)

    def __exit__(self, *exc):
        self.engine.set_variant("auto")


def _run_pair(engine, orc, cube_dir, src_name, out_name, luts=("log709_33.cube", "random_9.cube"), **kw):
    """One (source, destination) pair at 64x8: two contents; three modes on vec_global (where the mix has a vector kernel), five
    on generic."""
    okw = {k: v for k, v in kw.items() if k in ("lut_depth",)}
    rng = kw.get("range_src", "tv")
    fin, fout = yuv_side(src_name), yuv_side(out_name)
    has_vec = not (fin.depth == 8 and fout.depth > 8)
    for lutname in luts:
        lut = _lut(engine, cube_dir, lutname)
        for dist in ("uniform", "natural"):
            for variant, modes in ((("vec_global", VEC_MODES),) if has_vec else ()) + (("generic", MODES),):
                for mode in modes:
                    src, out = _want(orc, lutname, lut, mode, src_name, out_name, dist, W, H, 20, rng, **okw)
                    dev = _dev(_side(src, src_name), engine.device)
                    with _variant(engine, variant):
                        got = _host(engine.apply_yuv(dev, pix_fmt=src_name, out_pix_fmt=out_name, interp=mode, **kw), out_name)
                        name = engine.last_kernel
                    assert _eq(got, _side(out, out_name)), (src_name, out_name, lutname, dist, variant, mode, name)
                    if variant == "vec_global":
                        assert name.startswith("k_yuv_pk_vec<") and name.endswith(f",{MODES.index(mode)}>"), name
                    else:
                        assert name == "k_yuv_pk_generic"


# ------------------------------------------------------------------ formats, mixes, modes and routing
@pytest.mark.gpu
@pytest.mark.parametrize("name", PACKED)
def test_every_format_to_itself(engine, orc, cube_dir, name):
    _run_pair(engine, orc, cube_dir, name, name)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", MIXES, ids=lambda p: f"{p[0]}-{p[1]}")
def test_mixed_sides(engine, orc, cube_dir, pair):
    _run_pair(engine, orc, cube_dir, *pair, luts=("log709_33.cube", "domain_2.cube"))


@pytest.mark.gpu
@pytest.mark.parametrize("pair", XSUB, ids=lambda p: f"{p[0]}-{p[1]}")
def test_packed_source_to_planar_420(engine, orc, cube_dir, pair):
    _run_pair(engine, orc, cube_dir, *pair, luts=("log709_33.cube",))


@pytest.mark.gpu
def test_packed_source_to_planar_444_runs_generic(engine, orc, cube_dir):
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for src_name, out_name in (("uyvy422", "yuv444p"), ("y210le", "yuv444p10le")):
        for w, h in ((W, H), (33, 5)):
            for mode in MODES:
                src, out = _want(orc, "log709_33.cube", lut, mode, src_name, out_name, "natural", w, h, 3)
                got = engine.apply_yuv(_dev(_side(src, src_name), engine.device), pix_fmt=src_name, out_pix_fmt=out_name, interp=mode,
                                       width=w)
                assert engine.last_kernel == "k_yuv_pk_generic"
                assert _eq(_host(got, out_name), list(out)), (src_name, out_name, w, h, mode)
        with _variant(engine, "vec_global"):
            with pytest.raises(_native.LutrError) as e:
                engine.apply_yuv(_dev(_side(src, src_name), engine.device), pix_fmt=src_name, out_pix_fmt=out_name, width=33)
            assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_full_range_prologue_at_8_bit(engine, orc, cube_dir):
    _run_pair(engine, orc, cube_dir, "y210le", "yuyv422", luts=("log709_33.cube",), range_src="pc", lut_depth=8)
    _run_pair(engine, orc, cube_dir, "y210le", "yuv422p", luts=("log709_33.cube",), range_src="pc", lut_depth=8)


# ------------------------------------------------------------------ shapes
@pytest.mark.gpu
def test_odd_width_runs_generic(engine, orc, cube_dir):
    """33x5: the last group's second luma sample is ignored on input (it holds junk here) and comes out as a copy of the last
    real one; 4:2:0 with an odd height besides."""
    lut = _lut(engine, cube_dir, "log709_33.cube")
    w, h = 33, 5
    for src_name, out_name in (("yuyv422", "yuyv422"), ("uyvy422", "uyvy422"), ("yvyu422", "yvyu422"), ("y210le", "y210le"),
                               ("y216le", "y216le"), ("y210le", "yuv422p10le"), ("yuv422p", "uyvy422"), ("y210le", "yuyv422"),
                               ("uyvy422", "yuv420p"), ("y210le", "yuv420p10le")):
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", src_name, out_name, "natural", w, h, 3)
        host = _side(src, src_name)
        fin = parse_packed_yuv_fmt(src_name)
        if fin is not None:
            host[0][:, -4 + (3 if fin.order == 1 else 2)] = 77 << fin.shift           # the ignored sample
        got = engine.apply_yuv(_dev(host, engine.device), pix_fmt=src_name, out_pix_fmt=out_name, width=w)
        assert engine.last_kernel == "k_yuv_pk_generic"
        assert _eq(_host(got, out_name), _side(out, out_name)), (src_name, out_name)
    dev = _dev(_side(src, "y210le"), engine.device)
    with pytest.raises(ValueError, match="width"):
        engine.apply_yuv(dev, pix_fmt="y210le", width=31)
    assert engine.apply_yuv(dev, pix_fmt="y210le")[0].shape == (5, 68)        # no width: two columns per group


@pytest.mark.gpu
def test_ragged_width_on_padded_rows(engine, orc, cube_dir):
    """70 columns on rows padded to an aligned stride: the vector kernel up to the last whole unit, the generic kernel for the
    tail -- the same bytes as the all-generic run, and nothing past the row is written."""
    import torch
    lut = _lut(engine, cube_dir, "log709_33.cube")
    w, h, pad = 70, 6, 192
    for src_name, out_name in (("uyvy422", "uyvy422"), ("y210le", "y210le"), ("y210le", "yuyv422"), ("yuv422p10le", "y210le"),
                               ("yvyu422", "yuv422p"), ("uyvy422", "yuv420p")):
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", src_name, out_name, "natural", w, h, 4)
        sp = _dev(_side(src, src_name), engine.device)
        fout = yuv_side(out_name)
        odt = torch.uint8 if fout.depth <= 8 else torch.int16
        fill = -1 if odt == torch.int16 else 255
        oshape = [fout.plane_shape(i, w, h) for i in range(fout.nplanes)]

        def padded(tensors):
            big = [torch.full((t.shape[0], pad), -1 if t.dtype == torch.int16 else 255, dtype=t.dtype, device=engine.device) for t in tensors]
            for b, t in zip(big, tensors):
                b[:, :t.shape[1]] = t
            return big, [b[:, :t.shape[1]] for b, t in zip(big, tensors)]

        _, src_v = padded(sp)
        results = {}
        for variant in ("auto", "generic"):
            big, dst_v = padded([torch.full(s, fill, dtype=odt, device=engine.device) for s in oshape])
            with _variant(engine, variant):
                engine.apply_yuv(src_v, dst_v, pix_fmt=src_name, out_pix_fmt=out_name, width=w)
                name = engine.last_kernel
            results[variant] = _host(dst_v, out_name)
            assert all(bool((b[:, s[1]:] == fill).all()) for b, s in zip(big, oshape)), (src_name, out_name, variant, "wrote past the row")
            assert name.startswith("k_yuv_pk_vec<") if variant == "auto" else name == "k_yuv_pk_generic", name
        assert _eq(results["auto"], results["generic"]) and _eq(results["auto"], _side(out, out_name)), (src_name, out_name)


# ------------------------------------------------------------------ other layouts
@pytest.mark.gpu
def test_row_shard_leaves_the_rest_alone(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for src_name, out_name, r0, nr in (("uyvy422", "uyvy422", 3, 2), ("y210le", "y210le", 3, 2), ("y210le", "yuv422p10le", 3, 2),
                                       ("uyvy422", "yuv420p", 2, 4), ("y210le", "yuv420p10le", 2, 4)):
        fout = yuv_side(out_name)
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", src_name, out_name, "natural", W, H, 5)
        want = _side(out, out_name)
        dev = _dev(_side(src, src_name), engine.device)
        for variant in ("auto", "generic"):
            dst = [torch.full(fout.plane_shape(i, W, H), 77, dtype=torch.uint8 if fout.depth <= 8 else torch.int16, device=engine.device)
                   for i in range(fout.nplanes)]
            with _variant(engine, variant):
                engine.apply_yuv(dev, dst, pix_fmt=src_name, out_pix_fmt=out_name, row0=r0, rows=nr)
                assert engine.last_kernel.startswith("k_yuv_pk_vec<" if variant == "auto" else "k_yuv_pk_generic")
            for i, (g, wnt) in enumerate(zip(_host(dst, out_name), want)):
                a, b = (r0, r0 + nr) if i == 0 else (r0 >> fout.csy, (r0 + nr) >> fout.csy)
                assert np.array_equal(g[a:b], wnt[a:b]), (src_name, out_name, variant, i)
                assert (g[:a] == 77).all() and (g[b:] == 77).all(), (src_name, out_name, variant, i, "bytes outside the shard changed")
    with pytest.raises(_native.LutrError) as e:                  # a 4:2:0 destination takes even rows
        engine.apply_yuv(_dev(_side(src, "y210le"), engine.device), pix_fmt="y210le", out_pix_fmt="yuv420p10le", row0=3, rows=2)
    assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_three_frame_batch_with_padded_strides(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir, "log709_33.cube")
    nf = 3
    for src_name, out_name in (("uyvy422", "uyvy422"), ("y210le", "y210le"), ("y210le", "yuv422p10le"), ("uyvy422", "yuv420p")):
        refs = [_want(orc, "log709_33.cube", lut, "tetrahedral", src_name, out_name, "natural", W, H, 20 + i) for i in range(nf)]
        dense = _dev(_batch([_side(s, src_name) for s, _ in refs]), engine.device)
        fout = yuv_side(out_name)
        odt = torch.uint8 if fout.depth <= 8 else torch.int16

        def spaced(shape, dt):                                     # rows 32 samples longer than the frame, a spare row per frame
            big = torch.zeros((shape[0], shape[1] + 1, shape[2] + 32), dtype=dt, device=engine.device)
            return big[:, :shape[1], :shape[2]]

        src_v = []
        for t in dense:
            v = spaced(t.shape, t.dtype)
            v.copy_(t)
            src_v.append(v)
        dst_v = [spaced((nf,) + fout.plane_shape(i, W, H), odt) for i in range(fout.nplanes)]
        engine.apply_yuv(src_v, dst_v, pix_fmt=src_name, out_pix_fmt=out_name)
        assert engine.last_kernel.startswith("k_yuv_pk_vec<"), engine.last_kernel
        assert _eq(_host([d.contiguous() for d in dst_v], out_name), _batch([_side(o, out_name) for _, o in refs])), (src_name, out_name)


def _abi(engine, src_name, out_name, w, h, nf, s, d, interp=2, row0=0, rows=None, pk=None):
    fin, fout = yuv_side(src_name), yuv_side(out_name)
    p = _native.YuvParams(fin.code, fout.code, fin.depth, 0, 0, 0, 0, 0)
    pi, po = pk or [_native.YuvPacking(int(f.nplanes == 1), getattr(f, "order", 0), getattr(f, "shift", 0)) for f in (fin, fout)]
    with engine._lock:
        engine._bind_stream()
        return engine._lib.lutr_apply_yuv_packed(engine._ctx, C.byref(p), interp, C.byref(pi), C.byref(po), w, h, nf, C.byref(s),
                                                 C.byref(d), row0, h if rows is None else rows)


def _planes_desc(tensors, flip=False):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        stride = t.stride(-2) * t.element_size()
        st.data[i] = t.data_ptr() + ((t.shape[-2] - 1) * stride if flip else 0)
        st.stride[i] = -stride if flip else stride
        st.frame_stride[i] = 0
    return st


@pytest.mark.gpu
def test_bottom_up_strides(engine, orc, cube_dir):
    """Negative row strides (a bottom-up surface) through the C-ABI: the generic kernel, the same picture."""
    import torch
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for name in ("uyvy422", "y210le"):
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", name, name, "natural", W, H, 5)
        dev = _dev([np.ascontiguousarray(p[::-1]) for p in _side(src, name)], engine.device)      # stored bottom row first
        dst = [torch.zeros_like(t) for t in dev]
        assert _abi(engine, name, name, W, H, 1, _planes_desc(dev, flip=True), _planes_desc(dst, flip=True)) == 0
        torch.cuda.synchronize()
        assert engine.last_kernel == "k_yuv_pk_generic"
        assert _eq([g[::-1] for g in _host(dst, name)], _side(out, name)), name
        with _variant(engine, "vec_global"):
            assert _abi(engine, name, name, W, H, 1, _planes_desc(dev, flip=True), _planes_desc(dst, flip=True)) == _native.EINVAL


@pytest.mark.gpu
def test_base_offset_breaks_the_alignment(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for name in ("uyvy422", "y210le"):
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", name, name, "natural", W, H, 5)
        dev = _dev(_side(src, name), engine.device)[0]
        flat = torch.zeros(dev.numel() + 2, dtype=dev.dtype, device=engine.device)
        off = flat[2:].view(dev.shape)                           # 2 or 4 bytes off a 16-byte boundary
        off.copy_(dev)
        assert (off.data_ptr() - flat.data_ptr()) % 16 != 0
        got = engine.apply_yuv(off, pix_fmt=name)
        assert engine.last_kernel == "k_yuv_pk_generic"
        assert _eq(_host(got, name), _side(out, name)), name
        with _variant(engine, "vec_global"):
            with pytest.raises(_native.LutrError) as e:
                engine.apply_yuv(off, pix_fmt=name)
            assert e.value.code == _native.EINVAL


# ------------------------------------------------------------------ the container's low bits
@pytest.mark.gpu
def test_low_bits_are_ignored_on_input_and_zero_on_output(engine, orc, cube_dir):
    lut = _lut(engine, cube_dir, "log709_33.cube")
    rng = np.random.default_rng(11)
    src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", "y210le", "y210le", "natural", W, H, 5)
    clean = to_packed(src, "y210le")
    dirty = clean | rng.integers(0, 64, size=clean.shape).astype(np.uint16)
    assert (dirty & 63).any()
    want8 = _want(orc, "log709_33.cube", lut, "tetrahedral", "y210le", "yuyv422", "natural", W, H, 5)[1]
    for variant in ("auto", "generic"):
        with _variant(engine, variant):
            a = _host(engine.apply_yuv(_dev([clean], engine.device), pix_fmt="y210le"), "y210le")
            b = _host(engine.apply_yuv(_dev([dirty], engine.device), pix_fmt="y210le"), "y210le")
            c = _host(engine.apply_yuv(_dev([dirty], engine.device), pix_fmt="y210le", out_pix_fmt="yuyv422"), "yuyv422")
        assert _eq(a, b) and _eq(a, [to_packed(out, "y210le")]), variant
        assert not (b[0] & 63).any(), variant
        assert _eq(c, [to_packed(want8, "yuyv422")]), variant


# ------------------------------------------------------------------ in place
@pytest.mark.gpu
def test_in_place(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for name in ("uyvy422", "y210le"):
        for (w, h), variant in (((W, H), "auto"), ((W, H), "generic"), ((70, 6), "auto"), ((33, 5), "auto")):
            src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", name, name, "natural", w, h, {W: 5, 70: 4, 33: 3}[w])
            dev = _dev(_side(src, name), engine.device)
            with _variant(engine, variant):
                res = engine.apply_yuv(dev, dev, pix_fmt=name, width=w)
            assert res is dev and _eq(_host(dev, name), _side(out, name)), (name, w, h, variant)
        # a bare tensor in, the same bare tensor out
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", name, name, "natural", W, H, 5)
        t = _dev(_side(src, name), engine.device)[0]
        assert engine.apply_yuv(t, t, pix_fmt=name) is t and _eq(_host(t, name), _side(out, name))
    # partial overlap, or another container over the same bytes: refused before any launch
    t = _dev(_side(src, "y210le"), engine.device)[0]
    big = torch.zeros((H + 1, t.shape[1]), dtype=t.dtype, device=engine.device)
    big[:H] = t
    for dst, out_name in ((big[1:], "y210le"), (t, "y216le")):
        with pytest.raises(_native.LutrError, match="in place") as e:
            engine.apply_yuv(big[:H] if dst is not t else t, dst, pix_fmt="y210le", out_pix_fmt=out_name)
        assert e.value.code == _native.EINVAL


# ------------------------------------------------------------------ prelut, variants, precision
@pytest.mark.gpu
def test_prelut(engine, orc, tmp_path):
    tab = cube.log709_lattice(17)
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, tab, shapers)
    lut = engine.load_cube(p)
    assert lut.prelut is not None
    pre = orc.parse_lut_file_ex(p)[3]
    for src_name, out_name in (("y210le", "y210le"), ("uyvy422", "yuv422p"), ("uyvy422", "yuv420p")):
        src, out = _want(orc, "shaped.csp", lut, "tetrahedral", src_name, out_name, "natural", W, H, 5, prelut=pre)
        for variant in ("auto", "generic"):
            with _variant(engine, variant):
                got = engine.apply_yuv(_dev(_side(src, src_name), engine.device), pix_fmt=src_name, out_pix_fmt=out_name)
            assert _eq(_host(got, out_name), _side(out, out_name)), (src_name, out_name, variant, engine.last_kernel)


@pytest.mark.gpu
def test_variants_and_precisions(engine, orc, cube_dir):
    lut = _lut(engine, cube_dir, "log709_33.cube")
    src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", "y210le", "y210le", "natural", W, H, 5)
    dev = _dev(_side(src, "y210le"), engine.device)
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv(dev, pix_fmt="y210le")
        assert e.value.code == _native.EINVAL
    with _variant(engine, "vec_global"):
        engine.apply_yuv(dev, pix_fmt="y210le")
        assert engine.last_kernel == "k_yuv_pk_vec<1,1,1,1,0,2>"
        engine.apply_yuv(dev, pix_fmt="y210le", out_pix_fmt="yuv420p")
        assert engine.last_kernel == "k_yuv_pk_vec<1,0,1,0,1,2>"
        with pytest.raises(_native.LutrError):                 # pyramid has no vector kernel
            engine.apply_yuv(dev, pix_fmt="y210le", interp="pyramid")
        with pytest.raises(_native.LutrError):                 # nor has 8 -> 16 bit
            engine.apply_yuv(_dev(_side(frames.natural_yuv(W, H, 8, 1, 0), "uyvy422"), engine.device), pix_fmt="uyvy422",
                             out_pix_fmt="y210le")
    try:
        for prec in ("fast", "fma32"):
            engine.set_precision(prec)
            got = engine.apply_yuv(dev, pix_fmt="y210le")
            assert engine.last_kernel == "k_yuv_pk_vec<1,1,1,1,0,2>", engine.last_kernel
            assert _eq(_host(got, "y210le"), _side(out, "y210le")), prec
    finally:
        engine.set_precision("strict")
    with pytest.raises(ValueError):
        engine.apply_yuv(dev + dev, pix_fmt="y210le")              # two buffers for a one-buffer format
    with pytest.raises(ValueError):
        engine.apply_yuv([dev[0][:, :-2]], pix_fmt="y210le")       # not whole groups
    with pytest.raises(ValueError):
        engine.apply_yuv(dev, [dev[0][:, :-4].contiguous()], pix_fmt="y210le")


@pytest.mark.gpu
def test_planar_sides_are_the_planar_calls_and_bad_packings_are_refused(engine, cube_dir):
    import torch
    _lut(engine, cube_dir, "log709_33.cube")
    PK = _native.YuvPacking
    for src_name, out_name in (("yuv422p10le", "yuv422p10le"), ("yuv422p10le", "yuv420p10le")):
        fin, fout = yuv_side(src_name), yuv_side(out_name)
        dev = _dev(frames.natural_yuv(W, H, 10, fin.csx, fin.csy, k=7), engine.device)
        a = _host(engine.apply_yuv(dev, pix_fmt=src_name, out_pix_fmt=out_name), out_name)
        ka = engine.last_kernel
        out = [torch.zeros(fout.plane_shape(i, W, H), dtype=torch.int16, device=engine.device) for i in range(3)]
        assert _abi(engine, src_name, out_name, W, H, 1, _planes_desc(dev), _planes_desc(out)) == 0
        torch.cuda.synchronize()
        assert engine.last_kernel == ka and _eq(_host(out, out_name), a), (engine.last_kernel, ka)
    # bad packings: LUTR_EINVAL with a message
    src = frames.natural_yuv(W, H, 10, 1, 0, k=7)
    buf = _dev(_side(src, "y210le"), engine.device)
    sd, dd = _planes_desc(buf), _planes_desc([torch.zeros_like(buf[0])])
    for pi, po in ((PK(1, 0, 5), PK(1, 0, 6)), (PK(1, 0, 6), PK(1, 0, 2)), (PK(2, 0, 6), PK(1, 0, 6)), (PK(1, 3, 6), PK(1, 0, 6)),
                   (PK(1, -1, 6), PK(1, 0, 6)), (PK(0, 1, 0), PK(1, 0, 6)), (PK(0, 0, 6), PK(1, 0, 6))):
        assert _abi(engine, "y210le", "y210le", W, H, 1, sd, dd, pk=(pi, po)) == _native.EINVAL
        assert engine._lib.lutr_last_error()
    b8 = _dev(_side(frames.natural_yuv(W, H, 8, 1, 0), "uyvy422"), engine.device)
    assert _abi(engine, "uyvy422", "uyvy422", W, H, 1, _planes_desc(b8), _planes_desc([torch.zeros_like(b8[0])]),
                pk=(PK(1, 1, 2), PK(1, 1, 0))) == _native.EINVAL                 # a shift at 8 bit
    # a packed side whose format is not 4:2:2; a packed destination whose fmt_in is not 4:2:2
    assert _abi(engine, "yuv420p10le", "yuv420p10le", W, H, 1, sd, dd, pk=(PK(1, 0, 6), PK(1, 0, 6))) == _native.EINVAL
    p420 = _dev(frames.natural_yuv(W, H, 10, 1, 1, k=7), engine.device)
    assert _abi(engine, "yuv420p10le", "yuv422p10le", W, H, 1, _planes_desc(p420), dd, pk=(PK(0, 0, 0), PK(1, 0, 6))) == _native.EINVAL
    assert _abi(engine, "yuv422p10le", "yuv420p10le", W, H, 1, _planes_desc(_dev(src, engine.device)), dd,
                pk=(PK(0, 0, 0), PK(1, 0, 6))) == _native.EINVAL
    null = _planes_desc(buf)
    null.data[0] = None
    assert _abi(engine, "y210le", "y210le", W, H, 1, null, dd) == _native.EINVAL
    odd = _planes_desc(buf)
    odd.data[0] = buf[0].data_ptr() + 1
    assert _abi(engine, "y210le", "y210le", W, H, 1, odd, dd) == _native.EINVAL
    assert b"aligned" in engine._lib.lutr_last_error()
    odd = _planes_desc(buf)
    odd.stride[0] += 1
    assert _abi(engine, "y210le", "y210le", W, H, 1, odd, dd) == _native.EINVAL
    # data[1] / data[2] of a packed side may be NULL: that is what _planes_desc left there
    assert sd.data[1] is None and _abi(engine, "y210le", "y210le", W, H, 1, sd, dd) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ host pipeline, CLI, row-sharded group
@pytest.mark.gpu
def test_host_pipeline_depth_change_and_odd_width(engine, orc, cube_dir):
    from lut_renderer_amd.stream import HostPipeline
    lut = _lut(engine, cube_dir, "log709_33.cube")
    nf = 3
    for src_name, out_name, w, h in (("y210le", "yuyv422", W, H), ("uyvy422", "uyvy422", 33, 5)):
        refs = [_want(orc, "log709_33.cube", lut, "tetrahedral", src_name, out_name, "natural", w, h, 20 + i) for i in range(nf)]
        stream_in = b"".join(to_packed(s, src_name).tobytes() for s, _ in refs)
        want = b"".join(to_packed(o, out_name).tobytes() for _, o in refs)
        pipe = HostPipeline(engine, src_name, w, h, batch=2, out_pix_fmt=out_name)
        g = (w + 1) // 2
        assert pipe.fin.frame_bytes == 4 * g * h * pipe.fin.itemsize and pipe.fout.frame_bytes == 4 * g * h * pipe.fout.itemsize
        pos, chunks = {"i": 0}, []

        def fill(buf, max_frames):
            n = min(max_frames, nf - pos["i"])
            nb = n * pipe.fin.frame_bytes
            buf[:nb] = np.frombuffer(stream_in, np.uint8, nb, pos["i"] * pipe.fin.frame_bytes)
            pos["i"] += n
            return n

        assert pipe.run(fill, lambda buf, n: chunks.append(bytes(buf)), total_frames=nf) == nf
        assert b"".join(chunks) == want, (src_name, out_name)


@pytest.mark.gpu
def test_cli_round_trip_over_pipes(engine, orc, cube_dir):
    lut = _lut(engine, cube_dir, "log709_33.cube")
    nf = 3
    refs = [_want(orc, "log709_33.cube", lut, "tetrahedral", "y210le", "yuv420p10le", "natural", W, H, 20 + i) for i in range(nf)]
    cmd = [sys.executable, "-m", "lut_renderer_amd.cli", "-i", "-", "-o", "-", "--size", f"{W}x{H}", "--pix-fmt", "y210le",
           "--out-pix-fmt", "yuv420p10le", "--cube", str(cube_dir / "log709_33.cube"), "--colorspace", "bt709", "--batch", "2",
           "--duration", f"{nf / 25.0:.3f}"]
    r = subprocess.run(cmd, input=b"".join(to_packed(s, "y210le").tobytes() for s, _ in refs), capture_output=True, cwd=ROOT,
                       timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == b"".join(p.tobytes() for _, o in refs for p in o)


@pytest.mark.gpu
def test_group_passes_packed_frames_through(engine, orc, cube_dir, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = _lut(engine, cube_dir, "log709_33.cube")
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    for src_name, out_name, w, h, blocks in (("y210le", "y210le", W, 6, [(0, 3), (3, 6)]), ("uyvy422", "yuv420p", W, H, [(0, 4), (4, 8)]),
                                             ("uyvy422", "uyvy422", 33, 5, None)):
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", src_name, out_name, "natural", w, h, {W: 5, 33: 3}[w])
        with LutEngineGroup([0, 0]) as g:
            g.set_lut(lut)
            got = g.apply_yuv(_dev(_side(src, src_name), engine.device), pix_fmt=src_name, out_pix_fmt=out_name, width=w)
            assert g.last_remote == 1 and (blocks is None or g.last_blocks == blocks), g.last_blocks
            assert all(r0 % (1 << yuv_side(out_name).csy) == 0 for r0, _ in g.last_blocks)
            assert _eq(_host(got, out_name), _side(out, out_name)), (src_name, out_name)
