"""Semi-planar YUV frames in and out of the fused LUT pass on the GPU.  The expected output is the C oracle's fused
YUV result on the planar frames (called as tests/test_gpu_parity.py::test_yuv_parity calls it) passed through `to_semi`; every
comparison is array_equal on whole planes."""
import ctypes as C

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.engine import parse_semi_fmt, yuv_side
from lut_renderer_amd.semiplanar import to_planar, to_semi
from tests._csp_files import write_csp_with_prelut

MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
SEMI = ("nv12", "nv21", "nv16", "p010le", "p012le", "p016le", "p210le", "p212le", "p216le")
MIXES = (("nv12", "yuv420p"), ("yuv420p", "nv12"), ("p010le", "yuv420p10le"), ("yuv420p10le", "p010le"),
         ("p210le", "yuv422p10le"), ("nv21", "nv12"), ("p010le", "nv12"))
W, H, NF = 64, 16, 2

_luts = {}
_refs = {}


def _lut(engine, cube_dir, name):
    """The parsed LUT (read once per session), uploaded to the engine."""
    if name not in _luts:
        _luts[name] = cube.read_lut(cube_dir / name)
    engine.set_lut(_luts[name])
    return _luts[name]


def _planar_name(name):
    f = parse_semi_fmt(name)
    return f.planar if f is not None else name


def _src(fin, dist, w, h, k, full_range=False):
    """Planar source codes for one frame of the format's depth and subsampling."""
    return frames.make_yuv(dist, w, h, fin.depth, fin.csx, fin.csy, k=k, full_range=full_range)


def _want(orc, lutname, lut, mode, src_name, out_name, dist, w, h, k, rng_src="tv", lut_depth=None, prelut=None):
    """The oracle's planar output for one frame, computed once per distinct case and shared (never modified)."""
    fin, fout = yuv_side(src_name), yuv_side(out_name)
    dl = lut_depth or fin.depth
    key = (lutname, mode, fin.depth, fin.csy, fout.depth, dist, w, h, k, rng_src, dl)
    if key not in _refs:
        prologue = fin.depth != dl
        kc = orc.yuv_constants("bt709", rng_src, "bt709", "tv", fin.depth, dl, fout.depth, 1 << (fin.csx + fin.csy), prologue=prologue)
        src = _src(fin, dist, w, h, k, full_range=(rng_src == "pc"))
        out = orc.apply_yuv(lut.table, lut.scale, mode, kc, fin.depth, dl, fout.depth, fin.csx, fin.csy, src, prelut=prelut)
        for p in out:
            p.setflags(write=False)
        _refs[key] = (src, out)
    return _refs[key]


def _side(planes, name):
    """Planar codes -> the planes of the container `name` (semi-planar or planar)."""
    return to_semi(planes, name) if parse_semi_fmt(name) is not None else list(planes)


def _dev(planes, device):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to(device)
            for p in planes]


def _host(tensors, name):
    wide = yuv_side(name).depth > 8
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


def _run_pair(engine, orc, cube_dir, src_name, out_name, **kw):
    """The main case for one (source, destination) pair: two LUTs, two contents, a batch of two frames; three modes under auto
    (the vector kernel), five under generic; the engine's own planar call gives the same samples."""
    okw = {k: v for k, v in kw.items() if k in ("lut_depth",)}
    rng = kw.get("range_src", "tv")
    for lutname in ("log709_33.cube", "random_9.cube"):
        lut = _lut(engine, cube_dir, lutname)
        for dist in ("uniform", "natural"):
            for variant, modes in (("auto", VEC_MODES), ("generic", MODES)):
                for mode in modes:
                    refs = [_want(orc, lutname, lut, mode, src_name, out_name, dist, W, H, 20 + i, rng, **okw) for i in range(NF)]
                    dev = _dev(_batch([_side(s, src_name) for s, _ in refs]), engine.device)
                    want = _batch([_side(o, out_name) for _, o in refs])
                    with _variant(engine, variant):
                        got = _host(engine.apply_yuv(dev, pix_fmt=src_name, out_pix_fmt=out_name, interp=mode, **kw), out_name)
                        name = engine.last_kernel
                    assert _eq(got, want), (src_name, out_name, lutname, dist, variant, mode, name)
                    if variant == "auto":
                        assert name.startswith("k_yuv_semi_vec<") and name.endswith(f",{MODES.index(mode)}>"), name
                    else:
                        assert name == "k_yuv_semi_generic"
            # the same samples in three planes through the engine's planar call
            refs = [_want(orc, lutname, lut, "tetrahedral", src_name, out_name, dist, W, H, 20 + i, rng, **okw) for i in range(NF)]
            planar = engine.apply_yuv(_dev(_batch([s for s, _ in refs]), engine.device), pix_fmt=_planar_name(src_name),
                                      out_pix_fmt=_planar_name(out_name), **kw)
            assert _eq(_host(planar, _planar_name(out_name)), _batch([o for _, o in refs])), (src_name, out_name, dist)


# ------------------------------------------------------------------ formats, mixes, modes and routing
@pytest.mark.gpu
@pytest.mark.parametrize("name", SEMI)
def test_every_format_to_itself(engine, orc, cube_dir, name):
    _run_pair(engine, orc, cube_dir, name, name)


@pytest.mark.gpu
@pytest.mark.parametrize("pair", MIXES, ids=lambda p: f"{p[0]}-{p[1]}")
def test_mixed_sides(engine, orc, cube_dir, pair):
    _run_pair(engine, orc, cube_dir, *pair)


@pytest.mark.gpu
def test_full_range_prologue_at_8_bit(engine, orc, cube_dir):
    _run_pair(engine, orc, cube_dir, "p010le", "nv12", range_src="pc", lut_depth=8)


# ------------------------------------------------------------------ shapes
@pytest.mark.gpu
def test_odd_sizes_run_generic(engine, orc, cube_dir):
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for w, h in ((37, 23), (1, 1)):
        for src_name, out_name in (("nv12", "nv12"), ("nv21", "nv21"), ("nv16", "nv16"), ("p010le", "p010le"), ("p210le", "p210le"),
                                   ("p016le", "p016le"), ("p010le", "yuv420p10le"), ("yuv420p", "nv12"), ("p010le", "nv12")):
            src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", src_name, out_name, "natural", w, h, 3)
            got = engine.apply_yuv(_dev(_side(src, src_name), engine.device), pix_fmt=src_name, out_pix_fmt=out_name)
            assert engine.last_kernel == "k_yuv_semi_generic"
            assert _eq(_host(got, out_name), _side(out, out_name)), (w, h, src_name, out_name)


@pytest.mark.gpu
def test_ragged_width_on_padded_rows(engine, orc, cube_dir):
    """70 columns on rows padded to an aligned stride: the vector kernel up to the last whole unit, the generic kernel for the
    tail -- the same bytes as the all-generic run, and nothing past the row is written."""
    import torch
    lut = _lut(engine, cube_dir, "log709_33.cube")
    w, h, pad = 70, 16, 96
    for src_name, out_name in (("nv12", "nv12"), ("p010le", "p010le"), ("p010le", "nv12"), ("yuv420p10le", "p010le"),
                               ("nv16", "yuv422p"), ("p210le", "p210le")):
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", src_name, out_name, "natural", w, h, 4)
        sp = _dev(_side(src, src_name), engine.device)
        fout = yuv_side(out_name)
        odt = torch.uint8 if fout.depth <= 8 else torch.int16
        oshape = [fout.plane_shape(i, w, h) for i in range(fout.nplanes)]

        def padded(tensors):
            big = [torch.full((t.shape[0], pad), -1 if t.dtype == torch.int16 else 255, dtype=t.dtype, device=engine.device) for t in tensors]
            for b, t in zip(big, tensors):
                b[:, :t.shape[1]] = t
            return big, [b[:, :t.shape[1]] for b, t in zip(big, tensors)]

        _, src_v = padded(sp)
        results = {}
        for variant in ("auto", "generic"):
            big, dst_v = padded([torch.zeros(s, dtype=odt, device=engine.device) for s in oshape])
            for b in big:
                b.fill_(-1 if odt == torch.int16 else 255)
            with _variant(engine, variant):
                engine.apply_yuv(src_v, dst_v, pix_fmt=src_name, out_pix_fmt=out_name)
                name = engine.last_kernel
            results[variant] = _host(dst_v, out_name)
            fill = -1 if odt == torch.int16 else 255
            assert all(bool((b[:, s[1]:] == fill).all()) for b, s in zip(big, oshape)), (src_name, out_name, variant, "wrote past the row")
            assert name.startswith("k_yuv_semi_vec<") if variant == "auto" else name == "k_yuv_semi_generic", name
        assert _eq(results["auto"], results["generic"]) and _eq(results["auto"], _side(out, out_name)), (src_name, out_name)


# ------------------------------------------------------------------ other layouts
@pytest.mark.gpu
def test_row_shard_leaves_the_rest_alone(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for src_name, out_name in (("nv12", "nv12"), ("p010le", "p010le"), ("p210le", "p210le"), ("p010le", "yuv420p10le")):
        fout = yuv_side(out_name)
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", src_name, out_name, "natural", W, H, 5)
        want = _side(out, out_name)
        dev = _dev(_side(src, src_name), engine.device)
        for variant in ("auto", "generic"):
            dst = [torch.full(fout.plane_shape(i, W, H), 77, dtype=torch.uint8 if fout.depth <= 8 else torch.int16, device=engine.device)
                   for i in range(fout.nplanes)]
            with _variant(engine, variant):
                engine.apply_yuv(dev, dst, pix_fmt=src_name, out_pix_fmt=out_name, row0=4, rows=8)
            got = _host(dst, out_name)
            for i, (g, wnt) in enumerate(zip(got, want)):
                a, b = (4, 12) if i == 0 else (4 >> fout.csy, 12 >> fout.csy)
                assert np.array_equal(g[a:b], wnt[a:b]), (src_name, out_name, variant, i)
                assert (g[:a] == 77).all() and (g[b:] == 77).all(), (src_name, out_name, variant, i, "bytes outside the shard changed")
    with pytest.raises(_native.LutrError) as e:
        engine.apply_yuv(_dev(_side(src, "p010le"), engine.device), pix_fmt="p010le", row0=1, rows=15)
    assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_frame_strided_batch(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for name in ("nv12", "p010le"):
        refs = [_want(orc, "log709_33.cube", lut, "tetrahedral", name, name, "natural", W, H, 20 + i) for i in range(NF)]
        dense = _dev(_batch([_side(s, name) for s, _ in refs]), engine.device)
        spaced = []
        for t in dense:                                            # every other frame of a batch twice as long
            big = torch.zeros((2 * NF,) + tuple(t.shape[1:]), dtype=t.dtype, device=engine.device)
            big[::2] = t
            spaced.append(big[::2])
        dst = [torch.zeros_like(b.repeat_interleave(2, 0))[::2] for b in dense]
        engine.apply_yuv(spaced, dst, pix_fmt=name)
        assert engine.last_kernel.startswith("k_yuv_semi_vec<")
        assert _eq(_host(dst, name), _batch([_side(o, name) for _, o in refs])), name


def _abi(engine, src_name, out_name, w, h, nf, s, d, interp=2, row0=0, rows=None, lay=None):
    fin, fout = yuv_side(src_name), yuv_side(out_name)
    p = _native.YuvParams(fin.code, fout.code, fin.depth, 0, 0, 0, 0, 0)
    li, lo = lay or [_native.YuvLayout(int(f.nplanes == 2), getattr(f, "swap", 0), getattr(f, "shift", 0)) for f in (fin, fout)]
    with engine._lock:
        engine._bind_stream()
        return engine._lib.lutr_apply_yuv_semi(engine._ctx, C.byref(p), interp, C.byref(li), C.byref(lo), w, h, nf, C.byref(s),
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
    for name in ("nv12", "p010le"):
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", name, name, "natural", W, H, 5)
        dev = _dev([np.ascontiguousarray(p[::-1]) for p in _side(src, name)], engine.device)      # stored bottom row first
        dst = [torch.zeros_like(t) for t in dev]
        assert _abi(engine, name, name, W, H, 1, _planes_desc(dev, flip=True), _planes_desc(dst, flip=True)) == 0
        torch.cuda.synchronize()
        assert engine.last_kernel == "k_yuv_semi_generic"
        assert _eq([g[::-1] for g in _host(dst, name)], _side(out, name)), name
        with _variant(engine, "vec_global"):
            assert _abi(engine, name, name, W, H, 1, _planes_desc(dev, flip=True), _planes_desc(dst, flip=True)) == _native.EINVAL


@pytest.mark.gpu
def test_chroma_plane_offset_by_one_sample(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for name in ("nv12", "p010le"):
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", name, name, "natural", W, H, 5)
        dev = _dev(_side(src, name), engine.device)
        flat = torch.zeros(dev[1].numel() + 1, dtype=dev[1].dtype, device=engine.device)
        off = flat[1:].view(dev[1].shape)
        off.copy_(dev[1])
        assert off.data_ptr() - flat.data_ptr() == off.element_size()
        got = engine.apply_yuv([dev[0], off], pix_fmt=name)
        assert engine.last_kernel == "k_yuv_semi_generic"
        assert _eq(_host(got, name), _side(out, name)), name
        with _variant(engine, "vec_global"):
            with pytest.raises(_native.LutrError) as e:
                engine.apply_yuv([dev[0], off], pix_fmt=name)
            assert e.value.code == _native.EINVAL


# ------------------------------------------------------------------ the container's low bits
@pytest.mark.gpu
def test_low_bits_are_ignored_on_input_and_zero_on_output(engine, orc, cube_dir):
    lut = _lut(engine, cube_dir, "log709_33.cube")
    rng = np.random.default_rng(11)
    src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", "p010le", "p010le", "natural", W, H, 5)
    clean = to_semi(src, "p010le")
    dirty = [p | rng.integers(0, 64, size=p.shape).astype(np.uint16) for p in clean]
    assert all((d & 63).any() for d in dirty)
    for variant in ("auto", "generic"):
        with _variant(engine, variant):
            a = _host(engine.apply_yuv(_dev(clean, engine.device), pix_fmt="p010le"), "p010le")
            b = _host(engine.apply_yuv(_dev(dirty, engine.device), pix_fmt="p010le"), "p010le")
            c = _host(engine.apply_yuv(_dev(dirty, engine.device), pix_fmt="p010le", out_pix_fmt="nv12"), "nv12")
        assert _eq(a, b) and _eq(a, to_semi(out, "p010le")), variant
        assert not any((p & 63).any() for p in b), variant
        want8 = _want(orc, "log709_33.cube", lut, "tetrahedral", "p010le", "nv12", "natural", W, H, 5)[1]
        assert _eq(c, to_semi(want8, "nv12")), variant


# ------------------------------------------------------------------ in place
@pytest.mark.gpu
def test_in_place(engine, orc, cube_dir):
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for name in ("nv12", "p010le"):
        for (w, h), variant in (((W, H), "auto"), ((W, H), "generic"), ((37, 23), "auto")):
            src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", name, name, "natural", w, h, 5 if w == W else 3)
            dev = _dev(_side(src, name), engine.device)
            with _variant(engine, variant):
                res = engine.apply_yuv(dev, dev, pix_fmt=name)
            assert res is dev and _eq(_host(dev, name), _side(out, name)), (name, w, h, variant)


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
    for src_name, out_name in (("p010le", "p010le"), ("nv12", "yuv420p")):
        src, out = _want(orc, "shaped.csp", lut, "tetrahedral", src_name, out_name, "natural", W, H, 5, prelut=pre)
        for variant in ("auto", "generic"):
            with _variant(engine, variant):
                got = engine.apply_yuv(_dev(_side(src, src_name), engine.device), pix_fmt=src_name, out_pix_fmt=out_name)
            assert _eq(_host(got, out_name), _side(out, out_name)), (src_name, out_name, variant, engine.last_kernel)


@pytest.mark.gpu
def test_variants_and_precisions(engine, orc, cube_dir):
    lut = _lut(engine, cube_dir, "log709_33.cube")
    src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", "p010le", "p010le", "natural", W, H, 5)
    dev = _dev(_side(src, "p010le"), engine.device)
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv(dev, pix_fmt="p010le")
        assert e.value.code == _native.EINVAL
    with _variant(engine, "vec_global"):
        engine.apply_yuv(dev, pix_fmt="p010le")
        assert engine.last_kernel == "k_yuv_semi_vec<1,1,1,1,1,1,2>"
        with pytest.raises(_native.LutrError):                 # pyramid has no vector kernel
            engine.apply_yuv(dev, pix_fmt="p010le", interp="pyramid")
        with pytest.raises(_native.LutrError):                 # nor has 8 -> 16 bit
            engine.apply_yuv(_dev(to_semi(frames.natural_yuv(W, H, 8, 1, 1), "nv12"), engine.device), pix_fmt="nv12", out_pix_fmt="p010le")
    try:
        for prec in ("fast", "fma32"):
            engine.set_precision(prec)
            got = engine.apply_yuv(dev, pix_fmt="p010le")
            assert engine.last_kernel == "k_yuv_semi_vec<1,1,1,1,1,1,2>", engine.last_kernel
            assert _eq(_host(got, "p010le"), _side(out, "p010le")), prec
    finally:
        engine.set_precision("strict")
    # option checks come before any GPU work
    for kw in (dict(chroma_loc="left"), dict(dither="error_diffusion"), dict(out_size=(32, 8)), dict(out_pix_fmt="p210le")):
        with pytest.raises(ValueError):
            engine.apply_yuv(dev, pix_fmt="p010le", **kw)
    with pytest.raises(ValueError):
        engine.apply_yuv(dev + [dev[1]], pix_fmt="p010le")         # three planes for a two-plane format
    with pytest.raises(ValueError):
        engine.apply_yuv([dev[0], dev[1][:, :-2]], pix_fmt="p010le")


@pytest.mark.gpu
def test_planar_layouts_are_apply_yuv_and_bad_layouts_are_refused(engine, cube_dir):
    import torch
    _lut(engine, cube_dir, "log709_33.cube")
    src = frames.natural_yuv(W, H, 10, 1, 1, k=7)
    dev = _dev(src, engine.device)
    a = _host(engine.apply_yuv(dev, pix_fmt="yuv420p10le"), "yuv420p10le")
    ka = engine.last_kernel
    out = [torch.zeros_like(t) for t in dev]
    assert _abi(engine, "yuv420p10le", "yuv420p10le", W, H, 1, _planes_desc(dev), _planes_desc(out)) == 0
    torch.cuda.synchronize()
    assert engine.last_kernel == ka and _eq(_host(out, "yuv420p10le"), a), (engine.last_kernel, ka)
    # bad layouts: LUTR_EINVAL with a message
    semi = _dev(to_semi(src, "p010le"), engine.device)
    sd, dd = _planes_desc(semi), _planes_desc([torch.zeros_like(t) for t in semi])
    L = _native.YuvLayout
    for li, lo in ((L(1, 0, 5), L(1, 0, 6)), (L(1, 0, 6), L(1, 0, 2)), (L(2, 0, 6), L(1, 0, 6)), (L(0, 1, 6), L(1, 0, 6))):
        assert _abi(engine, "p010le", "p010le", W, H, 1, sd, dd, lay=(li, lo)) == _native.EINVAL
        assert engine._lib.lutr_last_error()
    s8 = _dev(to_semi(frames.natural_yuv(W, H, 8, 1, 1), "nv12"), engine.device)
    assert _abi(engine, "nv12", "nv12", W, H, 1, _planes_desc(s8), _planes_desc([torch.zeros_like(t) for t in s8]),
                lay=(L(1, 0, 2), L(1, 0, 0))) == _native.EINVAL
    null = _planes_desc(semi)
    null.data[1] = None
    assert _abi(engine, "p010le", "p010le", W, H, 1, null, dd) == _native.EINVAL
    odd = _planes_desc(semi)
    odd.data[1] = semi[1].data_ptr() + 1
    assert _abi(engine, "p010le", "p010le", W, H, 1, odd, dd) == _native.EINVAL
    assert b"aligned" in engine._lib.lutr_last_error()
    # a shifted planar container (yuv420p10 in the high bits) is taken too: the generic kernel
    hi = _dev([p << 6 for p in src], engine.device)
    dst = [torch.zeros_like(t) for t in hi]
    assert _abi(engine, "yuv420p10le", "yuv420p10le", W, H, 1, _planes_desc(hi), _planes_desc(dst), lay=(L(0, 0, 6), L(0, 0, 6))) == 0
    torch.cuda.synchronize()
    assert engine.last_kernel == "k_yuv_semi_generic" and _eq(_host(dst, "yuv420p10le"), [p << 6 for p in a])


# ------------------------------------------------------------------ host pipeline, row-sharded group
@pytest.mark.gpu
def test_host_pipeline_nv12_to_p010le(engine, orc, cube_dir):
    from lut_renderer_amd.stream import HostPipeline
    lut = _lut(engine, cube_dir, "log709_33.cube")
    nf = 3
    refs = [_want(orc, "log709_33.cube", lut, "tetrahedral", "nv12", "p010le", "natural", W, H, 20 + i) for i in range(nf)]
    stream_in = b"".join(p.tobytes() for s, _ in refs for p in to_semi(s, "nv12"))
    want = b"".join(p.tobytes() for _, o in refs for p in to_semi(o, "p010le"))
    direct = engine.apply_yuv(_dev(_batch([to_semi(s, "nv12") for s, _ in refs]), engine.device), pix_fmt="nv12", out_pix_fmt="p010le")
    assert b"".join(np.ascontiguousarray(p[i]).tobytes() for i in range(nf) for p in _host(direct, "p010le")) == want
    pipe = HostPipeline(engine, "nv12", W, H, batch=2, out_pix_fmt="p010le")
    assert pipe.fin.frame_bytes == W * H * 3 // 2 and pipe.fout.frame_bytes == W * H * 3
    pos, chunks = {"i": 0}, []

    def fill(buf, max_frames):
        n = min(max_frames, nf - pos["i"])
        nb = n * pipe.fin.frame_bytes
        buf[:nb] = np.frombuffer(stream_in, np.uint8, nb, pos["i"] * pipe.fin.frame_bytes)
        pos["i"] += n
        return n

    assert pipe.run(fill, lambda buf, n: chunks.append(bytes(buf)), total_frames=nf) == nf
    assert b"".join(chunks) == want


@pytest.mark.gpu
def test_group_passes_semi_planar_frames_through(engine, orc, cube_dir):
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = _lut(engine, cube_dir, "log709_33.cube")
    for src_name, out_name in (("p010le", "p010le"), ("nv12", "yuv420p")):
        src, out = _want(orc, "log709_33.cube", lut, "tetrahedral", src_name, out_name, "natural", W, H, 5)
        with LutEngineGroup([0, 0], treat_as_remote=True) as g:
            g.set_lut(lut)
            got = g.apply_yuv(_dev(_side(src, src_name), engine.device), pix_fmt=src_name, out_pix_fmt=out_name)
            assert g.last_remote == 1 and g.last_blocks == [(0, 8), (8, 16)]
            assert _eq(_host(got, out_name), _side(out, out_name)), (src_name, out_name)
