"""Premultiplied alpha on the GPU: every comparison is bit for bit against tests/_premul_twin.py -- the two
integer steps over every (code, alpha) pair, every layout pair and container mix on both kernels, LUT kinds, shapes, row shards,
the group, the refusals, the float path with its specials, and the CLI over pipes."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from tests import _premul_twin as twin
from tests import _rgbf_twin as rf

ROOT = Path(__file__).resolve().parent.parent
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
GENERIC = "k_yuva_premul_generic"
F = np.float32


def _t(a, device):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def _dev(planes, device):
    return [_t(p, device) for p in planes]


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _host(planes):
    return [_np(t) for t in planes]


def _eq(got, want):
    return len(got) == len(want) and all(np.array_equal(g, w) for g, w in zip(got, want))


def _words(a, depth):
    return np.asarray(a).astype(np.uint8 if depth <= 8 else np.uint16)


def _fmt(depth, lay, alpha=True):
    return f"yuv{'a' if alpha else ''}{lay}p" + ("" if depth == 8 else f"{depth}le")


def _vec(din, dout, a, b, interp):
    (ix, iy), (ox, oy) = LAYOUTS[a], LAYOUTS[b]
    return f"k_yuva_premul_vec<{int(din > 8)},{int(dout > 8)},{ix},{iy},{ox},{oy},{_native.INTERP[interp]}>"


def _alpha_name(din, dout, variant="auto"):
    """The alpha kernel of a 64-column plane under the colour call's variant."""
    return "k_alpha_generic" if variant == "generic" else f"k_alpha_vec<{int(din > 8)},{int(dout > 8)}>"


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


def _alpha(w, h, depth, k=0, lead=()):
    """Noise alpha with both end points and their neighbours."""
    ma = (1 << depth) - 1
    rng = np.random.default_rng(300 + k)
    a = rng.integers(0, ma + 1, size=lead + (h, w), dtype=np.int64)
    a[..., 0, :min(w, 5)] = (0, ma, 1, ma - 1, 2)[:min(w, 5)]
    return _words(a, depth)


def _src(w, h, depth, lay, k=0):
    """Four source planes: a natural frame and noise alpha."""
    csx, csy = LAYOUTS[lay]
    return frames.natural_yuv(w, h, depth, csx, csy, k=k) + [_alpha(w, h, depth, k)]


_luts = {}


def _load(engine, path):
    """Loads `path` into the engine; returns (parsed LUT, the oracle's prelut or None)."""
    from oracle import binding as orc
    if path not in _luts:
        _luts[path] = (cube.read_lut(path), orc.parse_lut_file_ex(path)[3] if str(path).endswith(".csp") else None)
    engine.load_cube(path)
    return _luts[path]


_refs = {}


def _want(lut, pre, interp, din, dout, a, b, src, key):
    """The twin's colour planes, computed once per case."""
    rk = (id(lut), interp, din, dout, a, b, key)
    if rk not in _refs:
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        k = twin.consts(din=din, dl=din, dout=dout, ocsx=ocsx, ocsy=ocsy)
        _refs[rk] = twin.apply(lut.table, lut.scale, interp, k, din, din, dout, icsx, icsy, ocsx, ocsy, src[:3], src[3], prelut=pre)
    return _refs[rk]


# ------------------------------------------------------------------ every (code, alpha) pair
@pytest.mark.gpu
def test_every_code_pair_at_8_bit(engine, cube_dir):
    lut, pre = _load(engine, cube_dir / "log709_33.cube")
    y = np.tile(np.arange(256, dtype=np.uint8), (256, 1))            # a column ramp
    a = np.ascontiguousarray(y.T)                                    # a row ramp
    for cb, cr in ((128, 128), (64, 200), (220, 90)):
        src = [y, np.full((256, 256), cb, np.uint8), np.full((256, 256), cr, np.uint8), a]
        dev = _dev(src, engine.device)
        want = _want(lut, pre, "tetrahedral", 8, 8, "444", "444", src, ("codes", cb))
        for variant, name in (("vec_global", _vec(8, 8, "444", "444", "tetrahedral")), ("generic", GENERIC)):
            with _variant(engine, variant):
                got = engine.apply_yuv(dev, pix_fmt="yuva444p", alpha_mode="premultiplied")
            assert engine.last_kernel == f"{name}+{_alpha_name(8, 8, variant)}"
            assert _eq(_host(got[:3]), want), (cb, cr, variant)
            assert np.array_equal(_np(got[3]), a)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [10, 16])
def test_code_pairs_at_10_and_16_bit(engine, cube_dir, depth):
    lut, pre = _load(engine, cube_dir / "log709_33.cube")
    ma = (1 << depth) - 1
    w, h = 256, 64
    rng = np.random.default_rng(depth)
    y = _words(np.tile(np.round(np.linspace(0, ma, w)).astype(np.int64), (h, 1)), depth)
    rows = np.concatenate([[0, 1, 2, ma - 1, ma, ma // 2, ma // 2 + 1, 3], rng.integers(0, ma + 1, size=h - 8)])
    a = _words(np.tile(rows.reshape(h, 1), (1, w)), depth)
    for cb, cr in ((ma // 2 + 1, ma // 2 + 1), (ma // 4, 3 * ma // 4)):
        src = [y, _words(np.full((h, w), cb), depth), _words(np.full((h, w), cr), depth), a]
        dev = _dev(src, engine.device)
        want = _want(lut, pre, "tetrahedral", depth, depth, "444", "444", src, ("codes", cb))
        for variant, name in (("vec_global", _vec(depth, depth, "444", "444", "tetrahedral")), ("generic", GENERIC)):
            with _variant(engine, variant):
                got = engine.apply_yuv(dev, pix_fmt=_fmt(depth, "444"), alpha_mode="premultiplied")
            assert engine.last_kernel == f"{name}+{_alpha_name(depth, depth, variant)}"
            assert _eq(_host(got[:3]), want), (depth, cb, variant)


# ------------------------------------------------------------------ all nine layout pairs, every container mix
@pytest.mark.gpu
@pytest.mark.parametrize("depths", [(8, 8), (10, 10), (10, 8), (12, 12)], ids=["8_8", "10_10", "10_8", "12_12"])
def test_layout_pairs(engine, cube_dir, depths):
    din, dout = depths
    lut, pre = _load(engine, cube_dir / "log709_33.cube")
    w, h = 64, 32
    for a in LAYOUTS:
        src = _src(w, h, din, a, k=din)
        dev = _dev(src, engine.device)
        for b in LAYOUTS:
            names = dict(pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(dout, b), alpha_mode="premultiplied")
            for interp in MODES:
                want = _want(lut, pre, interp, din, dout, a, b, src, "pairs")
                runs = [("generic", GENERIC)]
                if interp in VEC_MODES:
                    runs += [("auto", _vec(din, dout, a, b, interp)), ("vec_global", _vec(din, dout, a, b, interp))]
                for variant, name in runs:
                    with _variant(engine, variant):
                        got = engine.apply_yuv(dev, interp=interp, **names)
                    assert engine.last_kernel == f"{name}+{_alpha_name(din, dout, variant)}", (a, b, interp, variant)
                    assert _eq(_host(got[:3]), want), (a, b, interp, variant)


@pytest.mark.gpu
def test_8_to_10_bit_takes_the_generic_kernel(engine, cube_dir):
    lut, pre = _load(engine, cube_dir / "log709_33.cube")
    for a, b in (("420", "444"), ("444", "420"), ("422", "422")):
        src = _src(64, 32, 8, a, k=5)
        dev = _dev(src, engine.device)
        got = engine.apply_yuv(dev, pix_fmt=_fmt(8, a), out_pix_fmt=_fmt(10, b), alpha_mode="premultiplied")
        assert engine.last_kernel == f"{GENERIC}+k_alpha_vec<0,1>"
        assert _eq(_host(got[:3]), _want(lut, pre, "tetrahedral", 8, 10, a, b, src, "8to10")), (a, b)
        with _variant(engine, "vec_global"):
            with pytest.raises(_native.LutrError) as e:
                engine.apply_yuv(dev, pix_fmt=_fmt(8, a), out_pix_fmt=_fmt(10, b), alpha_mode="premultiplied")
        assert e.value.code == _native.EINVAL


# ------------------------------------------------------------------ LUT kinds
@pytest.mark.gpu
def test_luts(engine, cube_dir, tmp_path):
    from tests._csp_files import write_csp_with_prelut
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    write_csp_with_prelut(tmp_path / "shaped.csp", 17, cube.log709_lattice(17), shapers)
    for path in (cube_dir / "random_9.cube", cube_dir / "domain_2.cube", tmp_path / "shaped.csp"):
        lut, pre = _load(engine, path)
        assert (pre is not None) == (path.suffix == ".csp")
        for din, a, b in ((10, "420", "422"), (8, "444", "444")):
            src = _src(64, 32, din, a, k=7)
            dev = _dev(src, engine.device)
            for variant, interp in (("auto", "tetrahedral"), ("auto", "trilinear"), ("generic", "prism"), ("generic", "nearest")):
                with _variant(engine, variant):
                    got = engine.apply_yuv(dev, pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(din, b), interp=interp,
                                           alpha_mode="premultiplied")
                assert engine.last_kernel.startswith(GENERIC if variant == "generic" else "k_yuva_premul_vec<")
                assert _eq(_host(got[:3]), _want(lut, pre, interp, din, din, a, b, src, path.name)), (path.name, din, interp)


# ------------------------------------------------------------------ shapes
@pytest.mark.gpu
def test_odd_sizes(engine, cube_dir):
    lut, pre = _load(engine, cube_dir / "log709_33.cube")
    for w, h in ((37, 23), (9, 1), (1, 5)):
        for a, b in (("420", "422"), ("444", "420"), ("420", "420"), ("422", "444")):
            src = _src(w, h, 10, a, k=w)
            got = engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), alpha_mode="premultiplied")
            assert engine.last_kernel.startswith(GENERIC + "+k_alpha_")
            assert _eq(_host(got[:3]), _want(lut, pre, "tetrahedral", 10, 10, a, b, src, ("odd", w, h))), (w, h, a, b)
            assert np.array_equal(_np(got[3]), src[3])


@pytest.mark.gpu
def test_ragged_width_on_padded_rows_and_a_batch(engine, cube_dir):
    import torch
    lut, pre = _load(engine, cube_dir / "log709_33.cube")
    nf, w, h, pad, fpad = 3, 70, 12, 96, 2
    a, b = "420", "422"
    fs = [_src(w, h, 10, a, k=20 + i) for i in range(nf)]
    shapes = [p.shape for p in fs[0]]
    sp = [torch.zeros((nf, s[0] + fpad, pad), dtype=torch.int16, device=engine.device) for s in shapes]
    for i, f in enumerate(fs):
        for t, p in zip(sp, f):
            t[i, :p.shape[0], :p.shape[1]] = torch.from_numpy(p.view(np.int16)).to(engine.device)
    oshape = [(h, w)] + [frames.chroma_shape(w, h, *LAYOUTS[b])] * 2 + [(h, w)]
    dp = [torch.full((nf, s[0] + fpad, pad), -1, dtype=torch.int16, device=engine.device) for s in oshape]
    src_v = [t[:, :s[0], :s[1]] for t, s in zip(sp, shapes)]
    dst_v = [t[:, :s[0], :s[1]] for t, s in zip(dp, oshape)]
    engine.apply_yuv(src_v, dst_v, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), alpha_mode="premultiplied")
    # 70 = 68 columns of the vector kernel (units of 4) and 2 of the generic one
    assert engine.last_kernel.startswith(_vec(10, 10, a, b, "tetrahedral") + "+" + GENERIC + "+k_alpha_")
    out = _host(dst_v)
    for i, f in enumerate(fs):
        assert _eq([o[i] for o in out[:3]], _want(lut, pre, "tetrahedral", 10, 10, a, b, f, ("batch", i))), i
        assert np.array_equal(out[3][i], f[3])
    assert all((t[:, s[0]:, :] == -1).all() and (t[:, :, s[1]:] == -1).all() for t, s in zip(dp, oshape)), "wrote into the padding"


def _desc(tensors, flip=False):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        stride = t.stride(-2) * t.element_size()
        st.data[i] = t.data_ptr() + ((t.shape[-2] - 1) * stride if flip else 0)
        st.stride[i] = -stride if flip else stride
        st.frame_stride[i] = 0
    return st


def _alpha_desc(t, depth, flip=False):
    a = _native.AlphaSrc()
    stride = t.stride(-2) * t.element_size()
    a.kind, a.depth, a.step, a.offset = (_native.ALPHA_FLOAT, 0, 1, 0) if depth == 0 else (_native.ALPHA_INT, depth, 1, 0)
    a.data = t.data_ptr() + ((t.shape[-2] - 1) * stride if flip else 0)
    a.stride, a.frame_stride = (-stride if flip else stride), 0
    return a


def _abi(engine, a, b, depth, w, h, src, alpha, dst, row0=0, rows=None):
    from lut_renderer_amd.engine import _yuv_params, parse_pix_fmt
    p = _yuv_params(parse_pix_fmt(_fmt(depth, a, False)).code, parse_pix_fmt(_fmt(depth, b, False)).code, depth, "bt709", "bt709",
                    "tv", "tv", "tv")
    engine._bind_stream()
    return engine._lib.lutr_apply_yuv_premul(engine._ctx, C.byref(p), _native.INTERP["tetrahedral"], w, h, 1, C.byref(src),
                                             C.byref(alpha), C.byref(dst), row0, h - row0 if rows is None else rows)


@pytest.mark.gpu
def test_bottom_up_strides(engine, cube_dir):
    import torch
    lut, pre = _load(engine, cube_dir / "log709_33.cube")
    w, h, a, b = 64, 16, "420", "444"
    src = _src(w, h, 10, a, k=9)
    flipped = _dev([np.ascontiguousarray(p[::-1]) for p in src], engine.device)
    dst = [torch.zeros((h, w), dtype=torch.int16, device=engine.device) for _ in range(3)]
    assert _abi(engine, a, b, 10, w, h, _desc(flipped[:3], True), _alpha_desc(flipped[3], 10, True), _desc(dst, True)) == 0
    assert engine._lib.lutr_ctx_last_kernel(engine._ctx).decode() == GENERIC
    torch.cuda.synchronize()
    assert _eq([p[::-1] for p in _host(dst)], _want(lut, pre, "tetrahedral", 10, 10, a, b, src, "flip"))
    with _variant(engine, "vec_global"):
        assert _abi(engine, a, b, 10, w, h, _desc(flipped[:3], True), _alpha_desc(flipped[3], 10, True), _desc(dst, True)) == _native.EINVAL
    # the alpha plane alone off the vector kernel's alignment: the generic kernel, the same picture
    shifted = torch.zeros((h, w + 8), dtype=torch.int16, device=engine.device)
    shifted[:, 1:w + 1] = _t(src[3], engine.device)
    dev = _dev(src, engine.device)
    got = engine.apply_yuv(dev[:3] + [shifted[:, 1:w + 1]], pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b, False), alpha_mode="premultiplied")
    assert engine.last_kernel == GENERIC
    assert _eq(_host(got), _want(lut, pre, "tetrahedral", 10, 10, a, b, src, "flip"))


# ------------------------------------------------------------------ opaque, transparent, the output's alpha plane
@pytest.mark.gpu
def test_opaque_is_the_straight_call_and_transparent_is_black(engine, cube_dir):
    _load(engine, cube_dir / "log709_33.cube")
    for din, dout, a, b in ((10, 10, "420", "420"), (10, 10, "444", "444"), (10, 8, "420", "422"), (8, 8, "422", "420"), (12, 12, "444", "420")):
        src = _src(64, 32, din, a, k=3)
        names = dict(pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(dout, b))
        src[3] = np.full_like(src[3], (1 << din) - 1)
        dev = _dev(src, engine.device)
        for variant in ("auto", "generic"):
            with _variant(engine, variant):
                straight = _host(engine.apply_yuv(dev, **names))
                assert "premul" not in engine.last_kernel
                assert _eq(_host(engine.apply_yuv(dev, alpha_mode="straight", **names)), straight)
                assert _eq(_host(engine.apply_yuv(dev, alpha_mode="premultiplied", **names)), straight), (din, dout, a, b, variant)
                assert "premul" in engine.last_kernel
        dev[3].zero_()
        y, cb, cr, al = _host(engine.apply_yuv(dev, alpha_mode="premultiplied", **names))
        assert (y == 16 << (dout - 8)).all() and (cb == 128 << (dout - 8)).all() and (cr == 128 << (dout - 8)).all() and not al.any()


@pytest.mark.gpu
def test_the_output_alpha_plane_is_the_straight_call_s(engine, cube_dir):
    lut, pre = _load(engine, cube_dir / "log709_33.cube")
    for din, dout, a, b in ((10, 10, "444", "444"), (10, 8, "420", "422"), (8, 16, "422", "444"), (12, 10, "444", "420")):
        src = _src(64, 32, din, a, k=4)
        dev = _dev(src, engine.device)
        names = dict(pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(dout, b))
        straight = engine.apply_yuv(dev, **names)
        alpha_kernel = engine.last_kernel.split("+")[-1]
        got = engine.apply_yuv(dev, alpha_mode="premultiplied", **names)
        assert engine.last_kernel.split("+")[-1] == alpha_kernel and engine.last_kernel.startswith("k_yuva_premul_")
        assert np.array_equal(_np(got[3]), _np(straight[3])), (din, dout)
        assert _eq(_host(got[:3]), _want(lut, pre, "tetrahedral", din, dout, a, b, src, "alpha_out"))
        # an output without alpha: three planes back, no alpha kernel
        got = engine.apply_yuv(dev, alpha_mode="premultiplied", pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(dout, b, False))
        assert len(got) == 3 and "+k_alpha" not in engine.last_kernel and engine.last_kernel.startswith("k_yuva_premul_")
        assert _eq(_host(got), _want(lut, pre, "tetrahedral", din, dout, a, b, src, "alpha_out"))


@pytest.mark.gpu
def test_straight_runs_todays_kernels(engine, cube_dir):
    _load(engine, cube_dir / "log709_33.cube")
    import torch
    src = _src(64, 32, 10, "420", k=2)
    dev = _dev(src, engine.device)
    for kw in (dict(pix_fmt="yuva420p10le"), dict(pix_fmt="yuva420p10le", out_pix_fmt="yuva422p10le"),
               dict(pix_fmt="yuva420p10le", out_pix_fmt="yuv420p"), dict(pix_fmt="yuva420p10le", dither="blue_noise"),
               dict(pix_fmt="yuva420p10le", chroma_loc="left")):
        a = _host(engine.apply_yuv(dev, **kw))
        ka = engine.last_kernel
        b = _host(engine.apply_yuv(dev, alpha_mode="straight", **kw))
        assert engine.last_kernel == ka and "premul" not in ka and _eq(a, b), kw
    assert _eq(_host(engine.apply_yuv(dev[:3], pix_fmt="yuv420p10le", alpha_mode="straight")), _host(engine.apply_yuv(dev[:3], pix_fmt="yuv420p10le")))
    fl = [torch.from_numpy(p).to(engine.device) for p in rf.make_float("hdr", 64, 8)] + [torch.rand((8, 64), device=engine.device)]
    a = [t.cpu().numpy() for t in engine.apply_rgb_float(fl)]
    ka = engine.last_kernel
    b = [t.cpu().numpy() for t in engine.apply_rgb_float(fl, alpha_mode="straight")]
    assert ka == engine.last_kernel == "k_rgbf_vec<2>" and _eq([p.view(np.uint32) for p in a], [p.view(np.uint32) for p in b])


# ------------------------------------------------------------------ rows, the group
@pytest.mark.gpu
def test_row_shards_on_the_union_block(engine, cube_dir):
    import torch
    _load(engine, cube_dir / "log709_33.cube")
    w, h = 64, 16
    src = _src(w, h, 10, "420", k=6)
    dev = _dev(src, engine.device)
    for b, variant in (("420", "auto"), ("422", "auto"), ("444", "generic")):
        ocsy = LAYOUTS[b][1]
        names = dict(pix_fmt=_fmt(10, "420"), out_pix_fmt=_fmt(10, b), alpha_mode="premultiplied")
        with _variant(engine, variant):
            whole = _host(engine.apply_yuv(dev, **names))
            out = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=engine.device) for p in whole]
            engine.apply_yuv(dev, out, row0=2, rows=6, **names)
            got = _host(out)
            for i, (g, wh) in enumerate(zip(got, whole)):
                r0, r1 = (2, 8) if i in (0, 3) else (2 >> ocsy, 8 >> ocsy)
                assert np.array_equal(g[r0:r1], wh[r0:r1]), (b, variant, i)
                assert (g[:r0] == 0x5a5a).all() and (g[r1:] == 0x5a5a).all(), (b, variant, i, "wrote outside the block")
            engine.apply_yuv(dev, out, row0=0, rows=2, **names)
            engine.apply_yuv(dev, out, row0=8, rows=8, **names)
            assert _eq(_host(out), whole), (b, variant)
    with pytest.raises(_native.LutrError, match="union") as e:
        engine.apply_yuv(dev, pix_fmt=_fmt(10, "420"), out_pix_fmt=_fmt(10, "422"), alpha_mode="premultiplied", row0=1, rows=h - 1)
    assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_group_shards_with_remote_blocks(engine, cube_dir, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    lut, pre = _load(engine, cube_dir / "log709_33.cube")
    for (w, h), a, b in (((64, 32), "420", "422"), ((33, 7), "444", "420")):
        src = _src(w, h, 10, a, k=8)
        names = dict(pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), alpha_mode="premultiplied")
        single = _host(engine.apply_yuv(_dev(src, engine.device), **names))
        assert _eq(single[:3], _want(lut, pre, "tetrahedral", 10, 10, a, b, src, ("group", w)))
        for n in (2, 3):
            with LutEngineGroup([0] * n) as g:
                assert g.treat_as_remote
                g.set_lut(lut)
                got = g.apply_yuv(_dev(src, engine.device), **names)
                assert g.last_remote == sum(1 for r0, r1 in g.last_blocks[1:] if r1 > r0) and g.last_remote >= 1
                assert all(r0 % 2 == 0 for r0, _ in g.last_blocks), g.last_blocks
                assert all("premul" in k for k in g.last_kernels if k)
                assert _eq(_host(got), single), (w, h, n)


# ------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_refusals_leave_the_destination_untouched(engine, cube_dir):
    import torch
    _load(engine, cube_dir / "log709_33.cube")
    w, h = 64, 32
    dev = _dev(_src(w, h, 10, "444", k=1), engine.device)
    out = [torch.full_like(t, 0x5a5a) for t in dev]
    names = dict(pix_fmt="yuva444p10le", alpha_mode="premultiplied")
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError, match="vec_lds") as e:
            engine.apply_yuv(dev, out, **names)
    assert e.value.code == _native.EINVAL
    # in place, and the alpha source as a colour destination: Python's checks first, then the library's own
    with pytest.raises(ValueError, match="in place"):
        engine.apply_yuv(dev, dev, **names)
    with pytest.raises(ValueError, match="alpha source overlaps destination plane 1"):
        engine.apply_yuv(dev, [out[0], dev[3], out[2], out[3]], **names)
    assert _abi(engine, "444", "444", 10, w, h, _desc(dev[:3]), _alpha_desc(dev[3], 10), _desc(dev[:3])) == _native.EINVAL
    assert b"cannot run in place: the byte range of source plane 0" in engine._lib.lutr_last_error()
    assert _abi(engine, "444", "444", 10, w, h, _desc(dev[:3]), _alpha_desc(dev[3], 10), _desc([out[0], dev[3], out[2]])) == _native.EINVAL
    assert b"source plane 3 overlaps that of destination plane 1" in engine._lib.lutr_last_error()
    # the alpha descriptor: another kind, depth, step; a prologue
    for change, what in ((dict(kind=_native.ALPHA_NONE), b"carries alpha"), (dict(kind=_native.ALPHA_FLOAT), b"kind"),
                         (dict(depth=8), b"depth"), (dict(step=4), b"step"), (dict(data=None), b"null alpha")):
        a = _alpha_desc(dev[3], 10)
        for k, v in change.items():
            setattr(a, k, v)
        assert _abi(engine, "444", "444", 10, w, h, _desc(dev[:3]), a, _desc(out[:3])) == _native.EINVAL
        assert what in engine._lib.lutr_last_error(), (change, engine._lib.lutr_last_error())
    from lut_renderer_amd.engine import _yuv_params, parse_pix_fmt
    code = parse_pix_fmt("yuv444p10le").code
    for p in (_yuv_params(code, code, 8, "bt709", "bt709", "pc", "tv", "tv"), _yuv_params(code, code, 10, "bt709", "bt709", "pc", "tv", "tv")):
        s, a, d = _desc(dev[:3]), _alpha_desc(dev[3], 10), _desc(out[:3])
        assert engine._lib.lutr_apply_yuv_premul(engine._ctx, C.byref(p), 2, w, h, 1, C.byref(s), C.byref(a), C.byref(d), 0, h) == _native.EINVAL
        assert b"prologue" in engine._lib.lutr_last_error()
    torch.cuda.synchronize()
    assert all((t == 0x5a5a).all() for t in out), "a refused call wrote to a destination"


# ------------------------------------------------------------------ float RGB
def _bits(planes):
    return [np.ascontiguousarray(p).view(np.uint32) for p in planes]


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(64, 16), (33, 5)], ids=["64x16", "33x5"])
def test_float(engine, cube_dir, size):
    import torch
    w, h = size
    lut, _ = _load(engine, cube_dir / "log709_33.cube")
    rng = np.random.default_rng(w)
    src = rf.make_float("hdr", w, h, k=1)
    alpha = rng.uniform(-0.1, 1.2, size=(h, w)).astype(F)
    alpha.reshape(-1)[:4] = (0.0, 1.0, 0.5, 1e-3)
    prem = [(p * np.clip(alpha, 0, 1)).astype(F) for p in src] + [alpha]
    dev = [torch.from_numpy(p).to(engine.device) for p in prem]
    for interp in MODES:
        # (`_interp` has nearest, trilinear and tetrahedral; pyramid and prism are pinned through the code-valued frame below)
        runs = [("generic", "k_rgbaf_premul_generic")]
        if interp in VEC_MODES and w % 4 == 0:
            runs += [("auto", f"k_rgbaf_premul_vec<{_native.INTERP[interp]}>"), ("vec_global", f"k_rgbaf_premul_vec<{_native.INTERP[interp]}>")]
        else:
            runs += [("auto", "k_rgbaf_premul_generic")]      # (rows of 33 floats are not 16-byte aligned: no split either)
        outs = []
        for variant, name in runs:
            with _variant(engine, variant):
                got = [t.cpu().numpy() for t in engine.apply_rgb_float(dev, interp=interp, alpha_mode="premultiplied")]
            assert engine.last_kernel == name, (interp, variant)
            outs.append(_bits(got))
        assert all(_eq(o, outs[0]) for o in outs[1:]), interp
        if interp in VEC_MODES:
            assert _eq(outs[0], _bits(twin.apply_float(lut.table, lut.scale, interp, prem))), interp
    # pyramid / prism against the C oracle: code-valued colour under alpha 1 and 0.5 (x / 0.5 and y * 0.5 are exact)
    codes = frames.make_rgb("natural", w, h, 10, k=2)
    cf = rf.code_frame(codes, 10)
    half = [(p * F(0.5)).astype(F) for p in cf] + [np.full((h, w), 0.5, F)]
    for interp in ("pyramid", "prism"):
        want = orc_rgb(lut, interp, codes)
        got = [t.cpu().numpy() for t in engine.apply_rgb_float([torch.from_numpy(p).to(engine.device) for p in half], interp=interp,
                                                               alpha_mode="premultiplied")]
        assert _eq(rf.to_codes([(p * F(2)).astype(F) for p in got[:3]], 10), want), interp
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError, match="vec_lds") as e:
            engine.apply_rgb_float(dev, alpha_mode="premultiplied")
    assert e.value.code == _native.EINVAL


def orc_rgb(lut, interp, codes):
    from oracle import binding as orc
    return list(orc.apply_rgb(lut.table, lut.scale, 10, interp, codes))


@pytest.mark.gpu
def test_float_specials_in_place_and_opaque(engine, cube_dir):
    import torch
    lut, _ = _load(engine, cube_dir / "random_9.cube")
    alphas = np.array([np.nan, -1.0, 0.0, 1e-42, 0.5, 1.0, 2.0, np.inf, -0.0, -np.inf, 1e-30, 0.99999994], F)
    colours = np.array([np.nan, np.inf, -np.inf, 1e-42, 1e38, 0.25, -1e38, -0.0, 0.7, 1.5, 3e-39, -2e-40], F)
    cc, aa = np.meshgrid(colours, alphas, indexing="ij")                  # 12 x 12
    nb = aa.view(np.uint32).copy()
    nb[1, 0], nb[2, 0] = 0x7fc00001, 0xff800001                          # a quiet NaN with a payload, a signalling one
    aa = nb.view(F)
    src = [cc, np.ascontiguousarray(cc[::-1]), np.ascontiguousarray(cc[:, ::-1]), aa]
    for interp in VEC_MODES:
        want = _bits(twin.apply_float(lut.table, lut.scale, interp, src))
        for variant in ("auto", "generic"):
            dev = [torch.from_numpy(p.copy()).to(engine.device) for p in src]
            with _variant(engine, variant):
                got = engine.apply_rgb_float(dev, dev, interp=interp, alpha_mode="premultiplied")       # in place
            assert got[0].data_ptr() == dev[0].data_ptr()
            assert _eq(_bits([t.cpu().numpy() for t in got]), want), (interp, variant)
    # t == 1 is today's call, bit for bit
    hdr = rf.make_float("hdr", 64, 8, k=3)
    for a in (np.ones((8, 64), F), np.full((8, 64), 3.0, F)):
        dev = [torch.from_numpy(p).to(engine.device) for p in hdr + [a]]
        today = _bits([t.cpu().numpy() for t in engine.apply_rgb_float(dev)])
        assert engine.last_kernel == "k_rgbf_vec<2>"
        assert _eq(_bits([t.cpu().numpy() for t in engine.apply_rgb_float(dev, alpha_mode="premultiplied")]), today)
        assert engine.last_kernel == "k_rgbaf_premul_vec<2>"
    # the alpha source as a colour destination is refused, nothing written
    dev = [torch.from_numpy(p).to(engine.device) for p in hdr + [np.ones((8, 64), F)]]
    with pytest.raises(ValueError, match="alpha source overlaps"):
        engine.apply_rgb_float(dev, [dev[3], dev[1], dev[2], dev[0]], alpha_mode="premultiplied")
    s, d = _desc(dev[:3]), _desc([dev[3], dev[1], dev[2]])
    a = _alpha_desc(dev[3], 0)
    engine._bind_stream()
    assert engine._lib.lutr_apply_planar_rgb_f32_premul(engine._ctx, 2, 64, 8, 1, C.byref(s), C.byref(a), C.byref(d), 0, 8) == _native.EINVAL
    assert b"alpha source overlaps" in engine._lib.lutr_last_error()


# ------------------------------------------------------------------ apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut(engine, cube_dir):
    from lut_renderer_amd.api import apply_lut
    lut, pre = _load(engine, cube_dir / "log709_33.cube")
    src = _src(64, 32, 10, "444", k=11)
    got, _ = apply_lut(_dev(src, engine.device), cube=lut, pix_fmt="yuva444p10le", colorspace="bt709", color_range="tv",
                       out_pix_fmt="yuva422p10le", engine=engine, alpha_mode="premultiplied")
    assert engine.last_kernel == _vec(10, 10, "444", "422", "tetrahedral") + "+k_alpha_vec<1,1>"
    assert _eq(_host(got[:3]), _want(lut, pre, "tetrahedral", 10, 10, "444", "422", src, "apply_lut"))
    assert np.array_equal(_np(got[3]), src[3])


@pytest.mark.gpu
def test_cli_over_pipes(cube_dir):
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    w, h = 64, 36
    path = cube_dir / "log709_33.cube"
    lut = cube.read_lut(path)
    fs = [_src(w, h, 10, "444", k=30 + i) for i in range(2)]
    k = twin.consts(din=10, dl=10, dout=10, ocsx=0, ocsy=0)
    want = b""
    for f in fs:
        out = twin.apply(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 0, 0, 0, 0, f[:3], f[3])
        want += b"".join(np.ascontiguousarray(p).astype(np.uint16).tobytes() for p in list(out) + [f[3]])
    info = VideoInfo(width=w, height=h, bit_depth=10, pix_fmt="yuva444p10le", color_range="tv", colorspace="bt709", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="prores_ks", pix_fmt="yuva444p10le"), path, info,
                         python_bin=sys.executable, alpha_mode="premultiplied")
    assert cmd[-2:] == ["--alpha-mode", "premultiplied"] and cmd[cmd.index("--pix-fmt") + 1] == "yuva444p10le"
    r = subprocess.run(cmd + ["--duration", "0.080"], input=b"".join(p.tobytes() for f in fs for p in f), capture_output=True, cwd=ROOT,
                       timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == want
