"""Two LUTs in one fused pass on the GPU: lutr_apply_yuv_chain bit-exact, whole planes, against the composition of
oracle calls in tests/_chain_twin.py (stage 1 at the input layout, the C oracle's lut3d with the first LUT, the C oracle's lut3d
again with the second, stage 3 at the output layout)."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from tests import _chain_twin as twin

ROOT = Path(__file__).resolve().parent.parent
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
GENERIC = "k_yuv_chain_generic"
W, H = 64, 8
#: the format pairs of the vector kernels' tests: (input depth, input layout, output depth, output layout)
VEC_PAIRS = [(10, "420", 10, "420"), (8, "420", 8, "420"), (10, "420", 8, "420"), (10, "420", 10, "422"), (10, "422", 10, "420"),
             (10, "444", 10, "444"), (8, "422", 8, "444")]
_refs = {}           # expected planes, computed once per case and shared (never written to)


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


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


def _vec_name(din, dout, a, b, mode):
    (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
    return f"k_yuv_chain_vec<{int(din > 8)},{int(dout > 8)},{icsx},{icsy},{ocsx},{ocsy},{MODES.index(mode)}>"


@pytest.fixture(scope="module")
def pairs(cube_dir, tmp_path_factory):
    """name -> (path of A, path of B, A parsed, B parsed, A's oracle prelut or None)"""
    return {name: (a, b, cube.read_lut(a), cube.read_lut(b), pre)
            for name, (a, b, pre) in twin.lut_pairs(cube_dir, tmp_path_factory.mktemp("chain_luts")).items()}


def _load(engine, pairs, name):
    a, b, A, B, pre = pairs[name]
    engine.load_cube(a)
    engine.load_cube2(b)
    return A, B, pre


def _want(pairs, name, ia, ib, din, dl, dout, a, b, src, key, rin="tv", prologue=False):
    rk = (name, ia, ib, din, dl, dout, a, b, key, rin, prologue)
    if rk not in _refs:
        _, _, A, B, pre = pairs[name]
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        k = twin.consts("bt709", rin, "bt709", "tv", din, dl, dout, ocsx, ocsy, prologue=prologue)
        _refs[rk] = twin.apply(A, B, ia, ib, k, dl, dout, icsx, icsy, ocsx, ocsy, src, prelut_a=pre)
    return _refs[rk]


def _src(dist, w, h, depth, lay, k=1):
    rk = ("src", dist, w, h, depth, lay, k)
    if rk not in _refs:
        _refs[rk] = frames.make_yuv(dist, w, h, depth, *LAYOUTS[lay], k=k)
    return _refs[rk]


# ------------------------------------------------------------------ the vector kernels
@pytest.mark.gpu
@pytest.mark.parametrize("case", VEC_PAIRS, ids=lambda c: f"{_fmt(c[0], c[1])}-{_fmt(c[2], c[3])}")
def test_vector_kernels(engine, pairs, case):
    din, a, dout, b = case
    for name in pairs:
        _load(engine, pairs, name)
        for dist in ("uniform", "natural"):
            src = _src(dist, W, H, din, a)
            dev = _dev(src, engine.device)
            for mode in VEC_MODES:
                with _variant(engine, "vec_global"):
                    got = engine.apply_yuv_chain(dev, pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(dout, b), interp=mode)
                    kernel = engine.last_kernel
                assert kernel.startswith("k_yuv_chain_vec<") and kernel == _vec_name(din, dout, a, b, mode), kernel
                assert _eq(_host(got, dout), _want(pairs, name, mode, mode, din, din, dout, a, b, src, dist)), (name, dist, mode)


# ------------------------------------------------------------------ the generic kernel
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["log709_random", "wide_domain", "csp_random"])
def test_generic_kernel_every_mode_and_mixed_pairs(engine, pairs, name):
    _load(engine, pairs, name)
    src = _src("natural", W, H, 10, "420")
    dev = _dev(src, engine.device)
    f = _fmt(10, "420")
    for ia, ib in [(m, m) for m in MODES] + [("tetrahedral", "trilinear"), ("nearest", "prism"), ("pyramid", "tetrahedral")]:
        with _variant(engine, "generic"):
            got = engine.apply_yuv_chain(dev, pix_fmt=f, interp=ia, interp2=ib)
            assert engine.last_kernel == GENERIC
        want = _want(pairs, name, ia, ib, 10, 10, 10, "420", "420", src, "natural")
        assert _eq(_host(got, 10), want), (name, ia, ib)
        if ia != ib or ia not in VEC_MODES:
            # auto: a pair of different modes, and the modes the vector kernels do not have, go to the generic kernel
            assert _eq(_host(engine.apply_yuv_chain(dev, pix_fmt=f, interp=ia, interp2=ib), 10), want) and engine.last_kernel == GENERIC
            with _variant(engine, "vec_global"):
                with pytest.raises(_native.LutrError) as e:
                    engine.apply_yuv_chain(dev, pix_fmt=f, interp=ia, interp2=ib)
                assert e.value.code == _native.EINVAL
    # interp2=None means interp
    got = engine.apply_yuv_chain(dev, pix_fmt=f, interp="trilinear")
    assert _eq(_host(got, 10), _want(pairs, name, "trilinear", "trilinear", 10, 10, 10, "420", "420", src, "natural"))


def _desc(tensors, flip=False):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        stride = t.stride(-2) * t.element_size()
        st.data[i] = t.data_ptr() + ((t.shape[-2] - 1) * stride if flip else 0)
        st.stride[i] = -stride if flip else stride
        st.frame_stride[i] = 0
    return st


def _abi(engine, fin, fout, w, h, s, d, interp=2, interp2=2):
    from lut_renderer_amd.engine import parse_pix_fmt
    fi, fo = parse_pix_fmt(fin), parse_pix_fmt(fout)
    p = _native.YuvParams(fi.code, fo.code, fi.depth, 0, 0, 0, 0, 0)
    with engine._lock:
        engine._bind_stream()
        return engine._lib.lutr_apply_yuv_chain(engine._ctx, C.byref(p), interp, interp2, w, h, 1, C.byref(s), C.byref(d), 0, h)


@pytest.mark.gpu
def test_generic_kernel_8_to_16_bit_odd_frames_and_negative_strides(engine, pairs):
    import torch
    name = "wide_domain"
    _load(engine, pairs, name)
    # an 8-bit source written as 10 bit: no vector kernel
    src = _src("natural", W, H, 8, "420")
    got = engine.apply_yuv_chain(_dev(src, engine.device), pix_fmt="yuv420p", out_pix_fmt="yuv420p10le")
    assert engine.last_kernel == GENERIC
    assert _eq(_host(got, 10), _want(pairs, name, "tetrahedral", "tetrahedral", 8, 8, 10, "420", "420", src, "natural"))
    # odd frames: partial input and output blocks take the edge again
    for a, b in (("420", "420"), ("420", "422"), ("444", "420"), ("422", "444")):
        src = _src("natural", 33, 7, 10, a)
        got = engine.apply_yuv_chain(_dev(src, engine.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b))
        assert engine.last_kernel == GENERIC
        assert _eq(_host(got, 10), _want(pairs, name, "tetrahedral", "tetrahedral", 10, 10, 10, a, b, src, "odd")), (a, b)
    # negative row strides (a bottom-up surface; torch has none, so through the C-ABI): the generic kernel, the same picture
    src = _src("natural", W, H, 10, "420")
    want = _want(pairs, name, "tetrahedral", "tetrahedral", 10, 10, 10, "420", "422", src, "natural")
    dev = _dev([np.ascontiguousarray(p[::-1]) for p in src], engine.device)
    out = [torch.zeros((H, W), dtype=torch.int16, device=engine.device)] + \
          [torch.zeros((H, W // 2), dtype=torch.int16, device=engine.device) for _ in range(2)]
    assert _abi(engine, "yuv420p10le", "yuv422p10le", W, H, _desc(dev, flip=True), _desc(out, flip=True)) == 0
    torch.cuda.synchronize()
    assert engine.last_kernel == GENERIC and _eq([g[::-1] for g in _host(out, 10)], want)
    with _variant(engine, "vec_global"):
        assert _abi(engine, "yuv420p10le", "yuv422p10le", W, H, _desc(dev, flip=True), _desc(out, flip=True)) == _native.EINVAL


# ------------------------------------------------------------------ shapes
@pytest.mark.gpu
def test_auto_splits_a_ragged_width_between_the_two_kernels(engine, pairs):
    import torch
    name = "log709_random"
    _load(engine, pairs, name)
    w, h, pad = 70, 6, 96
    for a, b in (("420", "420"), ("420", "422")):
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        src = _src("natural", w, h, 10, a, k=4)
        sp = [torch.zeros((p.shape[0], pad), dtype=torch.int16, device=engine.device) for p in src]
        for t, p in zip(sp, src):
            t[:, :p.shape[1]] = torch.from_numpy(p.view(np.int16)).to(engine.device)
        src_v = [t[:, :p.shape[1]] for t, p in zip(sp, src)]
        oshape = [(h, w)] + [frames.chroma_shape(w, h, ocsx, ocsy)] * 2
        dp = [torch.full((s[0], pad), -1, dtype=torch.int16, device=engine.device) for s in oshape]
        dst_v = [t[:, :s[1]] for t, s in zip(dp, oshape)]
        engine.apply_yuv_chain(src_v, dst_v, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b))
        assert engine.last_kernel == _vec_name(10, 10, a, b, "tetrahedral") + "+" + GENERIC, engine.last_kernel
        assert _eq(_host(dst_v, 10), _want(pairs, name, "tetrahedral", "tetrahedral", 10, 10, 10, a, b, src, "ragged")), (a, b)
        assert all((t[:, s[1]:] == -1).all() for t, s in zip(dp, oshape)), "wrote past the row"


@pytest.mark.gpu
def test_full_range_source(engine, pairs):
    """range_src="pc" with lut_depth=8 on a 10-bit source: the prologue of lutr_apply_yuv ahead of both LUTs, which run at 8 bit."""
    name = "log709_random"
    _load(engine, pairs, name)
    src = frames.make_yuv("natural", W, H, 10, 1, 1, k=6, full_range=True)
    for dout, b in ((10, "420"), (8, "422")):
        got = engine.apply_yuv_chain(_dev(src, engine.device), pix_fmt="yuv420p10le", out_pix_fmt=_fmt(dout, b), range_src="pc",
                                     range_in="tv", lut_depth=8)
        assert engine.last_kernel == _vec_name(10, dout, "420", b, "tetrahedral")
        want = _want(pairs, name, "tetrahedral", "tetrahedral", 10, 8, dout, "420", b, src, "pc", rin="tv", prologue=True)
        assert _eq(_host(got, dout), want), (dout, b)


@pytest.mark.gpu
def test_a_batch_with_padded_row_and_frame_strides(engine, pairs):
    import torch
    name = "csp_random"
    _load(engine, pairs, name)
    nf, pad, fpad = 3, 96, 2
    fs = [_src("natural", W, H, 10, "420", k=10 + i) for i in range(nf)]
    shapes = [p.shape for p in fs[0]]
    sp = [torch.zeros((nf, s[0] + fpad, pad), dtype=torch.int16, device=engine.device) for s in shapes]
    for i, f in enumerate(fs):
        for t, p in zip(sp, f):
            t[i, :p.shape[0], :p.shape[1]] = torch.from_numpy(p.view(np.int16)).to(engine.device)
    oshape = [(H, W)] + [frames.chroma_shape(W, H, 1, 0)] * 2
    dp = [torch.full((nf, s[0] + fpad, pad), -1, dtype=torch.int16, device=engine.device) for s in oshape]
    src_v = [t[:, :s[0], :s[1]] for t, s in zip(sp, shapes)]
    dst_v = [t[:, :s[0], :s[1]] for t, s in zip(dp, oshape)]
    engine.apply_yuv_chain(src_v, dst_v, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
    assert engine.last_kernel == _vec_name(10, 10, "420", "422", "tetrahedral")
    out = _host(dst_v, 10)
    for i, f in enumerate(fs):
        want = _want(pairs, name, "tetrahedral", "tetrahedral", 10, 10, 10, "420", "422", f, ("batch", i))
        assert _eq([o[i] for o in out], want), i
    assert all((t[:, s[0]:, :] == -1).all() and (t[:, :, s[1]:] == -1).all() for t, s in zip(dp, oshape)), "wrote into the padding"


@pytest.mark.gpu
def test_a_row_block_into_sentinel_planes(engine, pairs):
    import torch
    _load(engine, pairs, "log709_random")
    src = _src("uniform", W, H, 10, "420")
    dev = _dev(src, engine.device)
    for b, variant in (("420", "auto"), ("422", "auto"), ("420", "generic")):
        ocsy = LAYOUTS[b][1]
        names = dict(pix_fmt="yuv420p10le", out_pix_fmt=_fmt(10, b))
        with _variant(engine, variant):
            whole = _host(engine.apply_yuv_chain(dev, **names), 10)
            out = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=engine.device) for p in whole]
            engine.apply_yuv_chain(dev, out, row0=2, rows=4, **names)
        got = _host(out, 10)
        for i, (g, wh) in enumerate(zip(got, whole)):
            r0, r1 = (2, 6) if i == 0 else (2 >> ocsy, 6 >> ocsy)
            assert np.array_equal(g[r0:r1], wh[r0:r1]), (b, variant, i)
            assert (g[:r0] == 0x5a5a).all() and (g[r1:] == 0x5a5a).all(), (b, variant, i, "wrote outside the block")
    with pytest.raises(_native.LutrError, match="union") as e:
        engine.apply_yuv_chain(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", row0=1, rows=H - 1)
    assert e.value.code == _native.EINVAL


# ------------------------------------------------------------------ the group
@pytest.mark.gpu
def test_group_shards_on_the_union_block(engine, pairs, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    name = "csp_random"
    _, _, A, B, _ = pairs[name]
    _load(engine, pairs, name)
    for (w, h), a, b in (((W, H), "420", "422"), ((33, 7), "422", "420")):
        src = _src("natural", w, h, 10, a)
        names = dict(pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), interp="tetrahedral", interp2="trilinear")
        single = _host(engine.apply_yuv_chain(_dev(src, engine.device), **names), 10)
        assert _eq(single, _want(pairs, name, "tetrahedral", "trilinear", 10, 10, 10, a, b, src, ("group", w)))
        for n in (2, 3):
            with LutEngineGroup([0] * n) as g:
                assert g.treat_as_remote
                g.set_lut(A)
                g.set_lut2(B)
                got = g.apply_yuv_chain(_dev(src, engine.device), **names)
                assert g.last_remote == sum(1 for r0, r1 in g.last_blocks[1:] if r1 > r0) and g.last_remote >= 1
                assert all(r0 % 2 == 0 for r0, _ in g.last_blocks), g.last_blocks
                assert _eq(_host(got, 10), single), (w, h, n)


# ------------------------------------------------------------------ nothing else changes
@pytest.mark.gpu
def test_a_second_lut_changes_no_other_call(engine, pairs):
    a, b, _, _, _ = pairs["log709_random"]
    engine.load_cube(a)
    engine.set_lut2(None)
    src = _src("natural", W, H, 10, "420")
    dev = _dev(src, engine.device)

    def calls():
        out = []
        for kw in (dict(pix_fmt="yuv420p10le"), dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")):
            got = _host(engine.apply_yuv(dev, **kw), 10)
            out.append((engine.last_kernel, got))
        g1, g2 = engine.apply_yuv_dual(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", out2_pix_fmt="yuv420p")
        out.append((engine.last_kernel, _host(g1, 10) + _host(g2, 8)))
        return out

    before = calls()
    engine.load_cube2(b)
    after = calls()
    engine.load_cube(a)                  # uploading the first LUT again leaves the second one alone
    got = engine.apply_yuv_chain(dev, pix_fmt="yuv420p10le")
    assert _eq(_host(got, 10), _want(pairs, "log709_random", "tetrahedral", "tetrahedral", 10, 10, 10, "420", "420", src, "natural"))
    for (k0, p0), (k1, p1) in zip(before, after):
        assert k0 == k1 and _eq(p0, p1), (k0, k1)
    assert before[1][0] == "k_yuv_xsub_vec<1,1,1,1,1,0,2>" and before[2][0].startswith("k_yuv_dual_vec<")


# ------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_refusals_leave_the_destination_untouched(engine, pairs):
    import torch
    a, b, _, _, _ = pairs["log709_random"]
    engine.load_cube(a)
    engine.set_lut2(None)
    dev = _dev(_src("natural", W, H, 10, "420"), engine.device)
    out = [torch.full_like(t, 0x5a5a) for t in dev]
    with pytest.raises(_native.LutrError, match="no second lattice") as e:
        engine.apply_yuv_chain(dev, out, pix_fmt="yuv420p10le")
    assert e.value.code == _native.EINVAL
    engine.load_cube2(b)
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError, match="vec_lds") as e:
            engine.apply_yuv_chain(dev, out, pix_fmt="yuv420p10le")
    assert e.value.code == _native.EINVAL
    with pytest.raises(_native.LutrError, match="cannot run in place: the byte range of source plane 0 overlaps") as e:
        engine.apply_yuv_chain(dev, dev, pix_fmt="yuv420p10le")
    assert e.value.code == _native.EINVAL
    # a destination plane inside a source plane: the destination's Cb is the upper left quarter of the source's luma
    inside = [out[0], dev[0][:H // 2, :W // 2], out[2]]
    with pytest.raises(_native.LutrError, match="source plane 0 overlaps that of destination plane 1") as e:
        engine.apply_yuv_chain(dev, inside, pix_fmt="yuv420p10le")
    assert e.value.code == _native.EINVAL
    torch.cuda.synchronize()
    assert all((t == 0x5a5a).all() for t in out), "a refused call wrote to a destination"
    with pytest.raises(_native.LutrError, match="non-finite"):
        engine.set_lut2(cube.CubeLut(2, np.ones(3, np.float32), np.full((2, 2, 2, 3), np.nan, np.float32)))
    engine.apply_yuv_chain(dev, out, pix_fmt="yuv420p10le")          # the second LUT of before is still there


# ------------------------------------------------------------------ apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut_with_a_second_lut(engine, pairs):
    from lut_renderer_amd.api import apply_lut
    name = "log709_random"
    _, _, A, B, _ = pairs[name]
    src = _src("natural", W, H, 10, "420")
    got, tags = apply_lut(_dev(src, engine.device), cube=A, cube2=B, interp2="trilinear", pix_fmt="yuv420p10le", colorspace="bt709",
                          color_range="tv", out_pix_fmt="yuv422p10le", engine=engine)
    assert engine.last_kernel == GENERIC and tags["colorspace"] == "bt709"
    assert _eq(_host(got, 10), _want(pairs, name, "tetrahedral", "trilinear", 10, 10, 10, "420", "422", src, "natural"))
    got, _ = apply_lut(_dev(src, engine.device), cube=pairs[name][0], cube2=pairs[name][1], pix_fmt="yuv420p10le",
                       colorspace="bt709", color_range="tv", out_pix_fmt="yuv422p10le", engine=engine)
    assert engine.last_kernel.startswith("k_yuv_chain_vec<")
    assert _eq(_host(got, 10), _want(pairs, name, "tetrahedral", "tetrahedral", 10, 10, 10, "420", "422", src, "natural"))


@pytest.mark.gpu
def test_cli_over_pipes_with_a_second_lut(pairs):
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    name = "csp_random"
    a, b, _, _, _ = pairs[name]
    src = _src("natural", W, H, 10, "420")
    want = b"".join(p.tobytes() for p in _want(pairs, name, "tetrahedral", "trilinear", 10, 10, 10, "420", "422", src, "natural"))
    info = VideoInfo(width=W, height=H, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le"), a, info,
                         python_bin=sys.executable, cube2=b, interp2="trilinear")
    r = subprocess.run(cmd + ["--duration", "0.040"], input=b"".join(p.tobytes() for p in src), capture_output=True, cwd=ROOT,
                       timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == want
