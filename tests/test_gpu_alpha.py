"""Alpha-carrying frames on the GPU: the alpha kernels against tests/_alpha_twin.py over every code, and every entry
point that carries, converts, fills or drops the plane -- its colour planes bit for bit those of the three-plane call."""
import ctypes as C

import numpy as np
import pytest

from lut_renderer_amd import _native, frames
from tests import _alpha_twin as twin

GENERIC = "k_alpha_generic"


def _t(a, device):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def _dev(planes, device):
    return [_t(p, device) for p in planes]


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _words(a, depth):
    return np.asarray(a).astype(np.uint8 if depth <= 8 else np.uint16)


def _alpha_values(w, h, depth, k=0, lead=()):
    """An alpha plane with both end points, a ramp and noise."""
    rng = np.random.default_rng(100 + k)
    a = rng.integers(0, 1 << depth, size=lead + (h, w), dtype=np.int64)
    a[..., 0, :2] = (0, (1 << depth) - 1)
    return _words(a, depth)


def _vec(din, dout):
    return f"k_alpha_vec<{2 if din is None else int(din > 8)},{int(dout > 8)}>"


def _raw_name(engine):
    return engine._lib.lutr_ctx_last_kernel(engine._ctx).decode()


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


def _same(got, want):
    return len(got) == len(want) and all(np.array_equal(_np(g), _np(w)) for g, w in zip(got, want))


def _yuva(w, h, depth, lay, k=0):
    """(four source planes as arrays) of a natural frame with an alpha plane"""
    csx, csy = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}[lay]
    return frames.natural_yuv(w, h, depth, csx, csy, k=k) + [_alpha_values(w, h, depth, k)]


# ------------------------------------------------------------------ every code of every pair, both kernels
@pytest.mark.gpu
def test_exhaustive_alpha(engine):
    import torch
    codes = np.arange(65536, dtype=np.int64).reshape(256, 256)
    for din in (8, 10, 12, 16):
        src_np = _words(codes & ((1 << din) - 1), din)
        src = _t(src_np, engine.device)
        for dout in (8, 10, 12, 16):
            want = twin.convert(src_np, din, dout)
            for variant, name in (("vec_global", _vec(din, dout)), ("generic", GENERIC)):
                dst = torch.zeros((256, 256), dtype=torch.uint8 if dout == 8 else torch.int16, device=engine.device)
                with _variant(engine, variant):
                    engine._alpha_plane(src, dst, din, dout, 256, 256, 0, None)
                assert _raw_name(engine) == name
                got = _np(dst).astype(np.int64)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (din, dout, variant, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])
    # words above Mi: clamped on a depth change (min(word, Mi)), copied as they are at equal depth
    src_np = _words(codes, 16)
    src = _t(src_np, engine.device)
    for din, dout in ((10, 8), (10, 12), (12, 16), (10, 10)):
        want = twin.convert(src_np, din, dout)
        assert din == dout or want.max() == (1 << dout) - 1
        for variant, name in (("vec_global", _vec(din, dout)), ("generic", GENERIC)):
            dst = torch.zeros((256, 256), dtype=torch.uint8 if dout == 8 else torch.int16, device=engine.device)
            with _variant(engine, variant):
                engine._alpha_plane(src, dst, din, dout, 256, 256, 0, None)
            assert _raw_name(engine) == name and np.array_equal(_np(dst).astype(np.int64), want), (din, dout, variant)
    # there is no LDS kernel; a layout the vector kernel cannot take is refused under vec_global
    dst = torch.zeros((256, 256), dtype=torch.int16, device=engine.device)
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError) as e:
            engine._alpha_plane(src, dst, 16, 10, 256, 256, 0, None)
    assert e.value.code == _native.EINVAL
    with _variant(engine, "vec_global"):
        with pytest.raises(_native.LutrError) as e:
            engine._alpha_plane(src[:, :33], dst[:, :33], 16, 10, 33, 256, 0, None)
    assert e.value.code == _native.EINVAL and not dst.any()


@pytest.mark.gpu
def test_float_alpha(engine):
    import torch
    rng = np.random.default_rng(5)
    special = [np.nan, -np.nan, np.inf, -np.inf, -0.25, -1e-30, -0.0, 0.0, 1e-42, 1.0, 1.0000001, 1.5, 3e38, -3e38, 0.99999994]
    a = np.concatenate([np.array(special, np.float32), rng.uniform(-0.1, 1.1, 128 - len(special) - 24).astype(np.float32)])
    for dout in (8, 10, 16):                        # values that land exactly on x.5 after the multiply: half to even
        mo = np.float32((1 << dout) - 1)
        halves = np.array([(k + 0.5) / float(mo) for k in (0, 1, 2, 3, 100, 101, 252, 253)], np.float32)
        halves = halves[(halves * mo) % 1 == 0.5]
        assert halves.size >= 4
        a = np.concatenate([a, np.resize(halves, 8)])
    a = a.reshape(8, 16)
    nan_bits = a.view(np.uint32).copy()
    nan_bits[0, 0] = 0x7fc00001                      # a quiet NaN with a payload, a signalling one
    nan_bits[0, 1] = 0xff800001
    a = nan_bits.view(np.float32)
    src = torch.from_numpy(a.copy()).to(engine.device)
    for dout in (8, 10, 16):
        want = twin.quantise(a, dout)
        assert want[0, 0] == 0 and want[0, 2] == (1 << dout) - 1 and want[0, 3] == 0
        for variant, name in (("vec_global", _vec(None, dout)), ("generic", GENERIC)):
            dst = torch.full((8, 16), 77, dtype=torch.uint8 if dout == 8 else torch.int16, device=engine.device)
            with _variant(engine, variant):
                engine._alpha_plane(src, dst, 0, dout, 16, 8, 0, None)
            assert _raw_name(engine) == name
            assert np.array_equal(_np(dst).astype(np.int64), want), (dout, variant, _np(dst), want)


# ------------------------------------------------------------------ shapes and rows, through apply_yuv
@pytest.mark.gpu
@pytest.mark.parametrize("out", [("yuva420p10le", 10), ("yuva420p", 8)], ids=["same_depth", "to_8_bit"])
def test_shapes(engine, cube_dir, out):
    import torch
    out_fmt, dout = out
    engine.load_cube(cube_dir / "log709_33.cube")
    dt = torch.uint8 if dout == 8 else torch.int16
    sentinel = 77

    def run(w, h, nf, pad):
        """`nf` frames whose alpha planes (source and destination) sit in rows of `pad` samples; returns (alpha out, want, name)"""
        fs = [_yuva(w, h, 10, "420", k=3 + i) for i in range(nf)]
        colour = [_t(np.stack([f[c] for f in fs]), engine.device) for c in range(3)]
        a_np = np.stack([f[3] for f in fs])
        sfull = torch.full((nf, h, pad), -1, dtype=torch.int16, device=engine.device)
        sfull[:, :, :w] = _t(a_np, engine.device)
        dfull = torch.full((nf, h, pad), sentinel, dtype=dt, device=engine.device)
        dst = [torch.empty((nf,) + tuple(c.shape[1:]), dtype=dt, device=engine.device) for c in colour] + [dfull[:, :, :w]]
        got = engine.apply_yuv(colour + [sfull[:, :, :w]], dst, pix_fmt="yuva420p10le", out_pix_fmt=out_fmt)
        assert got is dst and bool((dfull[:, :, w:] == sentinel).all())          # the padding keeps its sentinel
        return _np(dfull[:, :, :w]).astype(np.int64), twin.convert(a_np, 10, dout), engine.last_kernel

    got, want, name = run(64, 8, 2, 96)                                       # whole units on aligned rows
    assert np.array_equal(got, want) and name.endswith("+" + _vec(10, dout)), name
    got, want, name = run(70, 6, 2, 96)                                       # the last 6 columns go to the generic kernel
    assert np.array_equal(got, want) and name.endswith("+" + _vec(10, dout)), name
    got, want, name = run(33, 5, 1, 33)
    assert np.array_equal(got, want) and name.endswith("+" + GENERIC), name

    # a bottom-up source plane (negative stride): the C-ABI itself, the generic kernel
    a_np = _alpha_values(64, 8, 10, k=9)
    src = _t(a_np, engine.device)
    dst = torch.full((8, 64), sentinel, dtype=dt, device=engine.device)
    desc = _native.AlphaSrc(_native.ALPHA_INT, 10, src.data_ptr() + 7 * 128, -128, 0, 1, 0)
    engine._bind_stream()
    _native.check(engine._lib.lutr_alpha_plane(engine._ctx, C.byref(desc), dout, C.c_void_p(dst.data_ptr()),
                                               64 * dst.element_size(), 0, 64, 8, 1, 0, 8))
    assert _raw_name(engine) == GENERIC
    assert np.array_equal(_np(dst).astype(np.int64), twin.convert(a_np[::-1], 10, dout))

    # rows [0, 4) then [4, 8) give the whole call; rows outside a shard are not written
    src = _dev(_yuva(64, 8, 10, "420", k=11), engine.device)
    whole = engine.apply_yuv(src, pix_fmt="yuva420p10le", out_pix_fmt=out_fmt)
    part = [torch.full_like(t, sentinel) for t in whole]
    engine.apply_yuv(src, part, pix_fmt="yuva420p10le", out_pix_fmt=out_fmt, row0=0, rows=4)
    assert bool((part[3][4:] == sentinel).all()) and bool((part[0][4:] == sentinel).all())
    assert np.array_equal(_np(part[3][:4]), _np(whole[3][:4]))
    engine.apply_yuv(src, part, pix_fmt="yuva420p10le", out_pix_fmt=out_fmt, row0=4, rows=4)
    assert _same(part, whole)


# ------------------------------------------------------------------ the colour planes are those of the three-plane call
@pytest.mark.gpu
@pytest.mark.parametrize("case", [("420", "420", {}), ("420", "444", {}), ("444", "420", {}), ("420", "420", {"chroma_loc": "left"}),
                                  ("420", "420", {"dither": "error_diffusion"}), ("420", "420", {"dither": "blue_noise"}),
                                  ("420", "422", {"dither": "blue_noise"})],
                         ids=["same", "420to444", "444to420", "chroma_loc", "error_diffusion", "blue_noise", "blue_noise_xsub"])
def test_colour_untouched(engine, cube_dir, case):
    a, b, opts = case
    engine.load_cube(cube_dir / "log709_33.cube")
    src_np = _yuva(64, 8, 10, a, k=21)
    src = _dev(src_np, engine.device)
    for dout in (10, 8):
        tail = "p" if dout == 8 else "p10le"
        got = engine.apply_yuv(src, pix_fmt=f"yuva{a}p10le", out_pix_fmt=f"yuva{b}{tail}", **opts)
        name4 = engine.last_kernel
        want = engine.apply_yuv(src[:3], pix_fmt=f"yuv{a}p10le", out_pix_fmt=f"yuv{b}{tail}", **opts)
        name3 = engine.last_kernel
        assert len(got) == 4 and _same(got[:3], want), (case, dout)
        assert name4 == f"{name3}+{_vec(10, dout)}", (name4, name3)
        assert np.array_equal(_np(got[3]).astype(np.int64), twin.convert(src_np[3], 10, dout))      # never dithered


# ------------------------------------------------------------------ fill and drop
@pytest.mark.gpu
def test_fill_and_drop(engine, cube_dir):
    engine.load_cube(cube_dir / "log709_33.cube")
    for w, h in ((64, 8), (33, 5)):
        src_np = _yuva(w, h, 10, "420", k=31)
        src = _dev(src_np, engine.device)
        for out_fmt, plain, mo in (("yuva420p10le", "yuv420p10le", 1023), ("yuva420p", "yuv420p", 255)):
            got = engine.apply_yuv(src[:3], pix_fmt="yuv420p10le", out_pix_fmt=out_fmt)             # no alpha on the source: opaque
            name = engine.last_kernel
            want = engine.apply_yuv(src[:3], pix_fmt="yuv420p10le", out_pix_fmt=plain)
            assert _same(got[:3], want) and name == engine.last_kernel + "+k_alpha_fill"
            assert got[3].shape == (h, w) and np.all(_np(got[3]) == mo)
            got = engine.apply_yuv(src, pix_fmt="yuva420p10le", out_pix_fmt=plain)                  # no alpha on the output: dropped
            assert len(got) == 3 and _same(got, want) and "alpha" not in engine.last_kernel
    # a full-range prologue call fills too: the reference's 8-bit intermediate has no alpha, whatever the source carried
    src8_np = _yuva(64, 8, 8, "420", k=32)
    src8 = _dev(src8_np, engine.device)
    pro = dict(range_src="pc", range_in="tv", lut_depth=8)
    got = engine.apply_yuv(src8, pix_fmt="yuva420p", out_pix_fmt="yuva420p", **pro)
    name = engine.last_kernel
    want = engine.apply_yuv(src8[:3], pix_fmt="yuv420p", out_pix_fmt="yuv420p", **pro)
    assert _same(got[:3], want) and name == engine.last_kernel + "+k_alpha_fill" and np.all(_np(got[3]) == 255)
    assert not np.all(src8_np[3] == 255)
    got = engine.apply_yuv(src, pix_fmt="yuva420p10le", out_pix_fmt="yuva420p10le", range_src="pc", range_in="pc", lut_depth=8)
    assert engine.last_kernel.endswith("+k_alpha_fill") and np.all(_np(got[3]) == 1023)       # (a depth-only prologue)
    got1, got2 = engine.apply_yuv_dual(src8, pix_fmt="yuva420p", out_pix_fmt="yuva420p", out2_pix_fmt="yuva444p10le", **pro)
    assert np.all(_np(got1[3]) == 255) and np.all(_np(got2[3]) == 1023)
    # an empty call launches nothing and joins nothing; a three-plane call after an alpha-carrying one reads its own kernel
    engine.apply_yuv(src, pix_fmt="yuva420p10le")
    assert "+k_alpha" in engine.last_kernel
    engine.apply_yuv(src[:3], pix_fmt="yuv420p10le")
    assert "alpha" not in engine.last_kernel and engine._alpha_kernels is None
    engine._alpha_plane(src[3], _dev([src_np[3]], engine.device)[0], 10, 10, 33, 5, 0, None)
    assert engine.last_kernel == "k_alpha_generic"
    engine._alpha_plane(src[3], _dev([src_np[3]], engine.device)[0], 10, 10, 33, 5, 0, None)
    assert engine.last_kernel == "k_alpha_generic"                                              # (repeated direct calls do not pile up)
    with _variant(engine, "generic"):
        got = engine.apply_yuv(src[:3], pix_fmt="yuv420p10le", out_pix_fmt="yuva420p")
    assert engine.last_kernel.endswith("+k_alpha_fill") and np.all(_np(got[3]) == 255)


# ------------------------------------------------------------------ the other entry points
@pytest.mark.gpu
def test_dual_output(engine, cube_dir):
    engine.load_cube(cube_dir / "log709_33.cube")
    src_np = _yuva(64, 8, 10, "444", k=41)
    src = _dev(src_np, engine.device)
    got1, got2 = engine.apply_yuv_dual(src, pix_fmt="yuva444p10le", out_pix_fmt="yuva444p10le", out2_pix_fmt="yuv420p")
    name = engine.last_kernel
    want1, want2 = engine.apply_yuv_dual(src[:3], pix_fmt="yuv444p10le", out_pix_fmt="yuv444p10le", out2_pix_fmt="yuv420p")
    assert len(got1) == 4 and len(got2) == 3 and _same(got1[:3], want1) and _same(got2, want2)
    assert name == engine.last_kernel + "+" + _vec(10, 10) and np.array_equal(_np(got1[3]), src_np[3])
    # each output on its own: the first drops alpha, the second converts it
    got1, got2 = engine.apply_yuv_dual(src, pix_fmt="yuva444p10le", out_pix_fmt="yuv422p10le", out2_pix_fmt="yuva420p")
    assert len(got1) == 3 and len(got2) == 4 and engine.last_kernel.endswith("+" + _vec(10, 8))
    assert np.array_equal(_np(got2[3]).astype(np.int64), twin.convert(src_np[3], 10, 8))
    # a source without alpha: both outputs filled
    got1, got2 = engine.apply_yuv_dual(src[:3], pix_fmt="yuv444p10le", out_pix_fmt="yuva444p10le", out2_pix_fmt="yuva420p")
    assert engine.last_kernel.endswith("+k_alpha_fill+k_alpha_fill")
    assert np.all(_np(got1[3]) == 1023) and np.all(_np(got2[3]) == 255) and _same(got1[:3], want1) and _same(got2[:3], want2)


@pytest.mark.gpu
def test_rgb_entry_points(engine, cube_dir):
    import torch
    engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 64, 8
    # apply_rgb on gbrap10le: four planes in, four out, alpha copied
    src_np = frames.natural_rgb(w, h, 10, k=51) + [_alpha_values(w, h, 10, 51)]
    src = _dev(src_np, engine.device)
    got = engine.apply_rgb(src, depth=10)
    name = engine.last_kernel
    want = engine.apply_rgb(src[:3], depth=10)
    assert len(got) == 4 and _same(got[:3], want) and np.array_equal(_np(got[3]), src_np[3])
    assert name == engine.last_kernel + "+" + _vec(10, 10)
    # packed sources: A from the right byte; a pad byte is not alpha
    rng = np.random.default_rng(52)
    img_np = rng.integers(0, 256, size=(h, w, 4), dtype=np.int64).astype(np.uint8)
    img = torch.from_numpy(img_np).to(engine.device)
    for fmt, slot in (("rgba", 3), ("argb", 0), ("bgra", 3), ("abgr", 0)):
        got = engine.apply_rgb_to_yuv(img, pix_fmt=fmt, out_pix_fmt="yuva420p")
        name = engine.last_kernel
        want = engine.apply_rgb_to_yuv(img, pix_fmt=fmt, out_pix_fmt="yuv420p")
        assert len(got) == 4 and _same(got[:3], want) and name == engine.last_kernel + "+" + GENERIC, (fmt, name)
        assert np.array_equal(_np(got[3]), img_np[..., slot]), fmt
    got = engine.apply_rgb_to_yuv(img, pix_fmt="rgb0", out_pix_fmt="yuva420p")
    assert engine.last_kernel.endswith("+k_alpha_fill") and np.all(_np(got[3]) == 255)
    got = engine.apply_rgb_to_yuv(img, pix_fmt="rgba", out_pix_fmt="yuva420p10le")                  # 8 -> 10 bit
    assert np.array_equal(_np(got[3]).astype(np.int64), twin.convert(img_np[..., 3], 8, 10))
    img16_np = rng.integers(0, 65536, size=(2, h, w, 4), dtype=np.int64).astype(np.uint16)          # a batch of 16-bit pixels
    got = engine.apply_rgb_to_yuv(_t(img16_np, engine.device), pix_fmt="rgba64le", out_pix_fmt="yuva444p10le")
    assert np.array_equal(_np(got[3]).astype(np.int64), twin.convert(img16_np[..., 3], 16, 10))
    # planar sources
    src_np = frames.natural_rgb(w, h, 12, k=53) + [_alpha_values(w, h, 12, 53)]
    src = _dev(src_np, engine.device)
    got = engine.apply_rgb_to_yuv(src, pix_fmt="gbrap12le", out_pix_fmt="yuva444p12le")
    name = engine.last_kernel
    want = engine.apply_rgb_to_yuv(src[:3], pix_fmt="gbrp12le", out_pix_fmt="yuv444p12le")
    assert _same(got[:3], want) and np.array_equal(_np(got[3]), src_np[3]) and name == engine.last_kernel + "+" + _vec(12, 12)
    got = engine.apply_rgb_to_yuv(src, pix_fmt="gbrap12le", out_pix_fmt="yuv444p12le")              # dropped
    assert len(got) == 3 and _same(got, want)
    got = engine.apply_rgb_to_yuv(src[:3], pix_fmt="gbrp12le", out_pix_fmt="yuva444p12le")          # filled
    assert np.all(_np(got[3]) == 4095)
    fl_np = [rng.uniform(0, 1, size=(h, w)).astype(np.float32) for _ in range(3)] + [rng.uniform(-0.1, 1.1, size=(h, w)).astype(np.float32)]
    fl = [torch.from_numpy(p).to(engine.device) for p in fl_np]
    got = engine.apply_rgb_to_yuv(fl, pix_fmt="gbrapf32le", out_pix_fmt="yuva444p10le")
    name = engine.last_kernel
    want = engine.apply_rgb_to_yuv(fl[:3], pix_fmt="gbrpf32le", out_pix_fmt="yuv444p10le")
    assert _same(got[:3], want) and name == engine.last_kernel + "+" + _vec(None, 10)
    assert np.array_equal(_np(got[3]).astype(np.int64), twin.quantise(fl_np[3], 10))
    # a source flagged full range: the 8-bit intermediate has no alpha, the output's is filled
    got = engine.apply_rgb_to_yuv(img, pix_fmt="rgba", out_pix_fmt="yuva420p", intermediate_pix_fmt="yuv420p", prologue_out_range="tv")
    want = engine.apply_rgb_to_yuv(img, pix_fmt="rgba", out_pix_fmt="yuv420p", intermediate_pix_fmt="yuv420p", prologue_out_range="tv")
    assert _same(got[:3], want) and np.all(_np(got[3]) == 255)


# ------------------------------------------------------------------ overlap
@pytest.mark.gpu
def test_overlap(engine, cube_dir):
    import torch
    engine.load_cube(cube_dir / "log709_33.cube")
    src_np = _yuva(64, 8, 10, "420", k=61)
    src = _dev(src_np, engine.device)
    want = engine.apply_yuv(src, pix_fmt="yuva420p10le")
    got = engine.apply_yuv(src, src, pix_fmt="yuva420p10le")                   # in place at equal formats: alpha is a no-op
    assert got is src and _same(src, want) and np.array_equal(_np(src[3]), src_np[3])
    assert _raw_name(engine) == "k_alpha_nop" and engine.last_kernel.endswith("+k_alpha_nop")
    # any other overlap of the two byte ranges: refused, nothing written
    buf = _t(_alpha_values(64, 12, 10, k=62), engine.device)
    before = _np(buf).copy()
    for a, b, din, dout in ((buf[0:8], buf[2:10], 10, 10), (buf[2:10], buf[0:8], 10, 10), (buf[0:8], buf[0:8], 12, 10),
                            (buf[0:8, :32], buf[0:8, 16:48], 10, 10)):
        with pytest.raises(_native.LutrError) as e:
            engine._alpha_plane(a, b, din, dout, a.shape[1], 8, 0, None)
        assert e.value.code == _native.EINVAL and "overlap" in e.value.message
    assert np.array_equal(_np(buf), before)
    # the other refusals of the entry point, none of which reaches the device
    dst = torch.zeros((8, 64), dtype=torch.int16, device=engine.device)
    for desc, dout, rows, what in ((_native.AlphaSrc(3, 10, buf.data_ptr(), 128, 0, 1, 0), 10, 8, "kind"),
                                   (_native.AlphaSrc(1, 7, buf.data_ptr(), 128, 0, 1, 0), 10, 8, "depth"),
                                   (_native.AlphaSrc(1, 10, buf.data_ptr(), 128, 0, 1, 0), 17, 8, "depth"),
                                   (_native.AlphaSrc(1, 10, None, 128, 0, 1, 0), 10, 8, "null"),
                                   (_native.AlphaSrc(1, 10, buf.data_ptr() + 1, 128, 0, 1, 0), 10, 8, "2-byte aligned"),
                                   (_native.AlphaSrc(1, 10, buf.data_ptr(), 127, 0, 1, 0), 10, 8, "2-byte aligned"),
                                   (_native.AlphaSrc(2, 0, buf.data_ptr() + 2, 256, 0, 1, 0), 10, 8, "4-byte aligned"),
                                   (_native.AlphaSrc(1, 10, buf.data_ptr(), 128, 0, 0, 0), 10, 8, "step"),
                                   (_native.AlphaSrc(1, 10, buf.data_ptr(), 128, 0, 4, 4), 10, 8, "offset"),
                                   (_native.AlphaSrc(1, 10, buf.data_ptr(), 128, 0, 1, 0), 10, 9, "geometry")):
        rc = engine._lib.lutr_alpha_plane(engine._ctx, C.byref(desc), dout, C.c_void_p(dst.data_ptr()), 128, 0, 64, 8, 1, 0, rows)
        assert rc == _native.EINVAL and what in engine._lib.lutr_last_error().decode(), what
    assert not dst.any()


# ------------------------------------------------------------------ sharding and streaming
@pytest.mark.gpu
def test_group_shards_alpha_with_luma(engine, cube_dir):
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    src_np = _yuva(64, 16, 10, "420", k=71)
    src = _dev(src_np, engine.device)
    rgb_np = frames.natural_rgb(64, 16, 10, k=72) + [_alpha_values(64, 16, 10, 72)]
    rgb = _dev(rgb_np, engine.device)
    calls = [dict(pix_fmt="yuva420p10le"), dict(pix_fmt="yuva420p10le", out_pix_fmt="yuva420p"),
             dict(pix_fmt="yuva420p10le", out_pix_fmt="yuva444p10le"), dict(pix_fmt="yuv420p10le", out_pix_fmt="yuva420p10le"),
             dict(pix_fmt="yuva420p10le", out_pix_fmt="yuv420p"), dict(pix_fmt="yuva420p10le", chroma_loc="left"),
             dict(pix_fmt="yuva420p10le", out_pix_fmt="yuva420p", dither="blue_noise")]
    want = [engine.apply_yuv(src if kw["pix_fmt"].startswith("yuva") else src[:3], **kw) for kw in calls]
    want_dual = engine.apply_yuv_dual(src, pix_fmt="yuva420p10le", out_pix_fmt="yuva422p10le", out2_pix_fmt="yuva420p")
    want_rgb = engine.apply_rgb_to_yuv(rgb, pix_fmt="gbrap10le", out_pix_fmt="yuva420p")
    for remote in (False, True):
        with LutEngineGroup([0, 0], treat_as_remote=remote) as g:
            g.set_lut(lut)
            for kw, w_ in zip(calls, want):
                got = g.apply_yuv(src if kw["pix_fmt"].startswith("yuva") else src[:3], **kw)
                assert [tuple(b) for b in g.last_blocks] == [(0, 8), (8, 16)] and g.last_remote == int(remote)
                assert _same(got, w_), (remote, kw)
            got1, got2 = g.apply_yuv_dual(src, pix_fmt="yuva420p10le", out_pix_fmt="yuva422p10le", out2_pix_fmt="yuva420p")
            assert _same(got1, want_dual[0]) and _same(got2, want_dual[1]), remote
            assert _same(g.apply_rgb_to_yuv(rgb, pix_fmt="gbrap10le", out_pix_fmt="yuva420p"), want_rgb), remote


@pytest.mark.gpu
def test_host_pipeline(engine, cube_dir):
    from lut_renderer_amd.stream import HostPipeline
    engine.load_cube(cube_dir / "log709_33.cube")
    w, h, nf = 64, 8, 3
    fs = [_yuva(w, h, 8, "420", k=81 + i) for i in range(nf)]
    stream_in = b"".join(p.tobytes() for f in fs for p in f)                  # rawvideo: Y, Cb, Cr, A of each frame back to back
    batch = _dev([np.stack([f[c] for f in fs]) for c in range(4)], engine.device)
    for out_fmt, dout in (("yuva420p", 8), ("yuv420p", 8), ("yuva420p10le", 10)):
        direct = [_np(t) for t in engine.apply_yuv(batch, pix_fmt="yuva420p", out_pix_fmt=out_fmt)]
        want = b"".join(p[i].tobytes() for i in range(nf) for p in direct)
        pipe = HostPipeline(engine, "yuva420p", w, h, batch=2, out_pix_fmt=out_fmt)
        assert pipe.fin.frame_bytes == w * h * 5 // 2
        assert pipe.fout.frame_bytes == (w * h * 5 // 2 if "yuva" in out_fmt else w * h * 3 // 2) * (2 if dout > 8 else 1)
        pos, out = {"i": 0}, []

        def fill(buf, max_frames):
            n = min(max_frames, nf - pos["i"])
            nb = n * pipe.fin.frame_bytes
            buf[:nb] = np.frombuffer(stream_in, np.uint8, nb, pos["i"] * pipe.fin.frame_bytes)
            pos["i"] += n
            return n

        assert pipe.run(fill, lambda buf, n: out.append(bytes(buf)), total_frames=nf) == nf
        assert b"".join(out) == want, out_fmt
