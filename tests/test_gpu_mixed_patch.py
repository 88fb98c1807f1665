"""Mixed tiles of the YUV tile kernels: a tile with some lanes inside the grey tube and some outside runs the tube body once, and
the outside lanes fetch their taps from the global lattice inside that body (lutr_tile2.hip, tile_body MIX / patch_taps).

The content here straddles the tube boundary on purpose: a chroma ramp (Cb across the width, Cr down the height, sigma-6 noise per
sample) has tiles with one, a few, about half and nearly all lanes outside somewhere along each axis; sigma-8 / sigma-16 frames
have scattered outliers.  Every case that claims the path asserts `mixed_tiles > 0`, and every output is compared bit for bit
with a reference computed from scratch: the oracle for strict, tests/_fma32_twin.py for fma32.  Destinations start as a sentinel."""
import numpy as np
import pytest
import torch

from lut_renderer_amd import cube, frames
from lut_renderer_amd.engine import LutEngine
from tests import _fma32_twin
from tests._csp_files import write_csp_with_prelut
from tests._deep_content import ramp_yuv, unit_lattice as _unit_lattice

F = np.float32
MODES = ("tetrahedral", "nearest", "trilinear")


# ------------------------------------------------------------------ content
def _content(name, w, h, depth, csx, csy, seed, full_range=False):
    if name == "ramp":
        return ramp_yuv(w, h, depth, csx, csy, seed, full_range)
    return frames.make_yuv(name, w, h, depth, csx, csy, k=seed, full_range=full_range)


def test_ramp_frame_straddles_the_tube(orc):
    """No GPU: the generator must yield chroma on both sides of the tube's bound -- |gv - rv| and |bu - gv| (RGB codes, chroma
    alone) against (H + 1) / kappa, kappa = lattice cells per code, H = 7 -- a fair share of each, along both axes,
    so that a later change to it cannot silently empty the GPU tests below."""
    k = orc.yuv_constants(din=10)
    _, cb, cr = ramp_yuv(512, 136, 10, 1, 1, seed=1)
    again = ramp_yuv(512, 136, 10, 1, 1, seed=1)
    assert np.array_equal(cb, again[1]) and np.array_equal(cr, again[2])          # deterministic
    cbd, crd = cb.astype(F) - F(k.coff), cr.astype(F) - F(k.coff)
    rv, gv, bu = F(k.krv) * crd, F(k.kgu) * cbd + F(k.kgv) * crd, F(k.kbu) * cbd
    worst = np.maximum(np.abs(gv - rv), np.abs(bu - gv))
    bound = (7 + 1) / (32.0 / 1023.0)
    inside = worst <= bound
    assert 0.2 < inside.mean() < 0.8, inside.mean()
    # a 64 x 4 block of samples is one tile of the headline layout (16 x 4 lanes of 4 x 1 samples): tiles wholly inside, wholly
    # outside, and with few, about half and nearly all samples outside
    out = (~inside).reshape(68 // 4, 4, 256 // 64, 64).sum(axis=(1, 3))
    assert (out == 0).any() and (out == 256).any(), out
    assert ((out > 0) & (out <= 16)).any() and ((out > 96) & (out < 160)).any() and ((out >= 224) & (out < 256)).any(), out
    # ... and along each axis: some column and some row of tiles runs from (nearly) inside to (nearly) outside
    for axis in (0, 1):
        assert ((out.min(axis=axis) <= 16) & (out.max(axis=axis) >= 224)).any(), (axis, out)


# ------------------------------------------------------------------ helpers
def _dev(planes):
    return [torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to("cuda:0")
            for p in planes]


def _sentinel(shapes, depth):
    if depth > 8:
        return [torch.full(s, -1, dtype=torch.int16, device="cuda:0") for s in shapes]
    return [torch.full(s, 0xA5, dtype=torch.uint8, device="cuda:0") for s in shapes]


def _np(tensors, depth):
    return [t.cpu().numpy().view(np.uint16) if depth > 8 else t.cpu().numpy() for t in tensors]


def _eq(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: plane {i} {a.shape} {a.dtype} != {b.shape} {b.dtype}"
        if not np.array_equal(a, b):
            diff = np.abs(a.astype(np.int64) - b.astype(np.int64))
            bad = np.argwhere(diff > 0)
            raise AssertionError(f"{what}: plane {i} differs at {len(bad)} samples, max |d|={diff.max()}, "
                                 f"first {bad[0].tolist()} got {a[tuple(bad[0])]} want {b[tuple(bad[0])]}")


def _lut(table, prelut=None):
    return cube.CubeLut(n=table.shape[0], table=np.ascontiguousarray(table, dtype=F), scale=np.ones(3, dtype=F), prelut=prelut)


LUTS = {n: _lut(_unit_lattice(n, n)) for n in (33, 25)}


@pytest.fixture(scope="module")
def eng():
    with LutEngine(0) as e:
        e.set_variant("vec_lds")
        yield e


def _apply(eng, src, fmt, dout, **kw):
    """One apply into sentinel planes with the tile counters on: (host planes, stats, kernel name)."""
    dst = _sentinel([p.shape for p in src], dout)
    eng.tile_stats(True)
    eng.apply_yuv(_dev(src), dst, pix_fmt=fmt, **kw)
    st = eng.tile_stats(False)
    return _np(dst, dout), st, eng.last_kernel


def _reference(orc, kern, lut, mode, k, din, dl, dout, cs, src, prelut=None):
    if ",fma32" in kern:
        return _fma32_twin.apply_yuv(lut.table, lut.scale, mode, k, din, dl, dout, cs[0], cs[1], src)
    return orc.apply_yuv(lut.table, lut.scale, mode, k, din, dl, dout, cs[0], cs[1], src, prelut=prelut)


def _check_names(kern, st, mode, prec, mixed=True):
    """The tile kernel ran, with a tube where the mode has one (nearest rounds to a node: no tube, nothing mixed), at the precision
    asked for, and -- where the case claims it -- through mixed tiles."""
    assert "k_yuv_tile2" in kern, kern
    assert ",fast" not in kern, kern
    if mode == "nearest":
        assert "+tube" not in kern and st["mixed_tiles"] == 0, (kern, st)
        return
    assert "+tube" in kern, kern
    if prec == "fma32":
        assert ",fma32" in kern, kern
    if mixed:
        assert st["mixed_tiles"] > 0, (kern, st)


# ------------------------------------------------------------------ shapes and layouts, strict and fma32, tetrahedral
# (format, input depth, output format or None, output depth, chroma shifts, width, height, content)
SHAPES = [
    ("yuv420p10le", 10, None, 10, (1, 1), 512, 136, "ramp"),           # 4 x 17 tiles of 128 x 8 px
    ("yuv420p10le", 10, None, 10, (1, 1), 520, 140, "ramp"),           # right and bottom edge tiles: clamped duplicate lanes
    ("yuv420p10le", 10, None, 10, (1, 1), 512, 136, "noise16"),
    ("yuv420p10le", 10, None, 10, (1, 1), 512, 136, "noise8"),
    ("yuv420p", 8, None, 8, (1, 1), 512, 136, "ramp"),                 # corner form: the lane's verdict only
    ("yuv422p10le", 10, None, 10, (1, 0), 512, 68, "ramp"),
    ("yuv444p10le", 10, None, 10, (0, 0), 512, 68, "ramp"),
    ("yuv420p10le", 10, "yuv420p", 8, (1, 1), 512, 136, "ramp"),       # 10-bit in, 8-bit out
]


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["strict", "fma32"])
@pytest.mark.parametrize("fmt,din,ofmt,dout,cs,w,h,content", SHAPES, ids=lambda v: str(v).replace(" ", ""))
def test_mixed_tiles_shapes(orc, eng, prec, fmt, din, ofmt, dout, cs, w, h, content):
    lut = LUTS[33]
    eng.set_lut(lut)
    eng.set_precision(prec)
    try:
        src = _content(content, w, h, din, cs[0], cs[1], seed=3)
        k = orc.yuv_constants("bt709", "tv", "bt709", "tv", din, din, dout, 1 << sum(cs))
        kw = dict(out_pix_fmt=ofmt) if ofmt else {}
        got, st, kern = _apply(eng, src, fmt, dout, interp="tetrahedral", **kw)
        print(f"{fmt}->{ofmt} {w}x{h} {content} {prec}: {kern} {st}")
        _check_names(kern, st, "tetrahedral", prec)
        _eq(got, _reference(orc, kern, lut, "tetrahedral", k, din, din, dout, cs, src), f"{fmt} {w}x{h} {content} {prec}")
    finally:
        eng.set_precision("strict")


# ------------------------------------------------------------------ modes x precisions x LUT sizes on the core shape
@pytest.mark.gpu
@pytest.mark.parametrize("n", [33, 25])
@pytest.mark.parametrize("prec", ["strict", "fma32"])
@pytest.mark.parametrize("mode", MODES)
def test_mixed_tiles_modes(orc, eng, mode, prec, n):
    """25^3 is above the strict kernels' whole-lattice limit, so it has a tube too.  The fma32 trilinear kernels have no mixed
    tiles (their tiles outside the tube go to the windows): bit-exactness only."""
    lut = LUTS[n]
    eng.set_lut(lut)
    eng.set_precision(prec)
    try:
        src = ramp_yuv(512, 136, 10, 1, 1, seed=5)
        k = orc.yuv_constants(din=10)
        got, st, kern = _apply(eng, src, "yuv420p10le", 10, interp=mode)
        print(f"{mode} {prec} {n}^3: {kern} {st}")
        _check_names(kern, st, mode, prec, mixed=not (mode == "trilinear" and prec == "fma32"))
        _eq(got, _reference(orc, kern, lut, mode, k, 10, 10, 10, (1, 1), src), f"{mode} {prec} {n}^3")
    finally:
        eng.set_precision("strict")


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,din,cs,h", [("yuv420p", 8, (1, 1), 136), ("yuv422p10le", 10, (1, 0), 68), ("yuv444p10le", 10, (0, 0), 68)])
def test_mixed_tiles_trilinear_layouts(orc, eng, fmt, din, cs, h):
    """Trilinear outside the headline layout: eight taps patched per pixel (4:4:4 at 16 bit keeps the gather pass for its outliers)."""
    lut = LUTS[33]
    eng.set_lut(lut)
    src = ramp_yuv(512, h, din, cs[0], cs[1], seed=6)
    k = orc.yuv_constants("bt709", "tv", "bt709", "tv", din, din, din, 1 << sum(cs))
    got, st, kern = _apply(eng, src, fmt, din, interp="trilinear")
    print(f"trilinear {fmt}: {kern} {st}")
    _check_names(kern, st, "trilinear", "strict")
    _eq(got, _reference(orc, kern, lut, "trilinear", k, din, din, din, cs, src), f"trilinear {fmt}")


# ------------------------------------------------------------------ a row shard, the prologue, a shared shaper
@pytest.mark.gpu
def test_mixed_tiles_row_shard(orc, eng):
    lut = LUTS[33]
    eng.set_lut(lut)
    src = ramp_yuv(256, 96, 10, 1, 1, seed=7)
    k = orc.yuv_constants(din=10)
    full = orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, src)
    got, st, kern = _apply(eng, src, "yuv420p10le", 10, row0=8, rows=64)
    _check_names(kern, st, "tetrahedral", "strict")
    want = [np.full(p.shape, 0xFFFF, np.uint16) for p in src]
    want[0][8:72] = full[0][8:72]
    want[1][4:36], want[2][4:36] = full[1][4:36], full[2][4:36]
    _eq(got, want, "row shard 8..72 of 256x96")


@pytest.mark.gpu
def test_mixed_tiles_prologue(orc, eng):
    """The config-5 prologue: full-range 10-bit source, limited-range LUT at 8-bit depth."""
    lut = LUTS[33]
    eng.set_lut(lut)
    src = ramp_yuv(512, 136, 10, 1, 1, seed=8, full_range=True)
    k5 = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 8, 10, 4, prologue=True)
    got, st, kern = _apply(eng, src, "yuv420p10le", 10, range_src="pc", range_in="tv", lut_depth=8)
    print(f"prologue: {kern} {st}")
    assert "pre" in kern, kern
    _check_names(kern, st, "tetrahedral", "strict")
    _eq(got, orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k5, 10, 8, 10, 1, 1, src), "prologue")


@pytest.mark.gpu
def test_mixed_tiles_shared_shaper(orc, eng, tmp_path):
    """A mild shared .csp shaper (slope within 1 +- 0.4): the tube's bound comes from the folded prelut, the patch from the same
    coordinates."""
    n = 33
    xs = np.linspace(0.0, 1.0, 33)
    p = tmp_path / "mild.csp"
    write_csp_with_prelut(p, n, _unit_lattice(n, 9), [(xs, xs + 0.4 * xs * (1.0 - xs))] * 3)
    eng.set_lut(cube.read_lut(p))
    _, sc, t, pre = orc.parse_lut_file_ex(p)
    src = ramp_yuv(512, 136, 10, 1, 1, seed=9)
    k = orc.yuv_constants(din=10)
    got, st, kern = _apply(eng, src, "yuv420p10le", 10)
    print(f"mild shaper: {kern} {st}")
    _check_names(kern, st, "tetrahedral", "strict")
    _eq(got, orc.apply_yuv(t, sc, "tetrahedral", k, 10, 10, 10, 1, 1, src, prelut=pre), "mild shaper")


# ------------------------------------------------------------------ routing keeps no state
@pytest.mark.gpu
def test_mixed_tiles_same_engine_different_content(orc):
    """One engine, content that is mixed, all tube, scattered outliers, saturated, then the first frame again: each output
    against the oracle, and the first frame's routing counters come back as they were."""
    lut = LUTS[33]
    k = orc.yuv_constants(din=10)
    seq = [("ramp", 11), ("natural", 12), ("noise16", 13), ("vivid", 14), ("uniform", 15), ("ramp", 11)]
    stats = []
    with LutEngine(0) as e:
        e.set_variant("vec_lds")
        e.set_lut(lut)
        for name, seed in seq:
            src = _content(name, 512, 136, 10, 1, 1, seed)
            got, st, kern = _apply(e, src, "yuv420p10le", 10)
            assert "k_yuv_tile2" in kern and "+tube" in kern, kern
            _eq(got, orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, src), f"{name} in sequence")
            stats.append(st)
    assert stats[0]["mixed_tiles"] > 0 and stats[2]["mixed_tiles"] > 0, stats
    for key in ("tiles", "tube_tiles", "mixed_tiles"):
        assert stats[0][key] == stats[-1][key], (key, stats[0], stats[-1])
