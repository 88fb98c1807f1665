"""The per-code coordinate table with INTEGER cells, and the legality test by OR, of the YUV tile kernels (lutr_tile2.hip).

Integer cells.  The table holds {int32 prev, float frac}; the LDS tap address is an fp32 fma chain on the cells' BITS (struct Win:
exact in fp32 denormals), the global tap address of mixed and gather tiles is plain integer arithmetic, the second-level test and
the restage take integer minima and maxima.  Every strict case must equal the oracle bit for bit, fast the fast oracle (and stay
within one code of strict, tests/test_fast_variant.py), fma32 its twin (tests/_fma32_twin.py): depths 8 / 10 / 12 and a 16-bit
container, the full-range prologue, a shared .csp prelut, lattices 17^3 (whole-lattice mode), 33^3 and 65^3 (no tube), the three
modes, frames of code 0 and of the top codes (the last padded table entries), a container holding 0xFFFF (the gather body's clamp),
and the RGB tube kernels, which keep the float table of lutr_tube.h.

Legality.  "No luma sample above 2^depth - 1" is judged from the OR of a unit's luma words.  One illegal sample anywhere in a unit
must send exactly its tile to the gather body, whatever bit it sets; the largest legal code must change nothing.

Small frames: 256 x 72 (2 x 9 tiles of 128 x 8 px, the bottom ones clamped) and 256 x 16 (four tiles, one unit per lane).  The
references are computed once per case on the CPU."""
import numpy as np
import pytest

from lut_renderer_amd import cube, frames
from tests import _deep_content as dc
from tests import _fma32_twin

pytestmark = pytest.mark.gpu
ONE = np.ones(3, np.float32)
W, H = 256, 72


def _dev(planes):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to("cuda:0")
            for p in planes]


def _host(tensors, depth):
    return [t.cpu().numpy().view(np.uint16) if depth > 8 else t.cpu().numpy() for t in tensors]


def _same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, a.dtype, b.shape, b.dtype)
        if not np.array_equal(a, b):
            d = np.abs(a.astype(np.int64) - b.astype(np.int64))
            bad = np.argwhere(d > 0)
            raise AssertionError(f"{what}: plane {i} differs at {len(bad)} samples, max |d| = {d.max()}, first {bad[0].tolist()}")


def _halves(depth, csx, csy, seed, full_range=False, w=W, h=H):
    """Natural content in the left half of the frame, vivid in the right: tube, mixed, window and gather tiles in one launch."""
    a = frames.make_yuv("natural", w, h, depth, csx, csy, k=seed, full_range=full_range)
    b = frames.make_yuv("vivid", w, h, depth, csx, csy, k=seed + 1, full_range=full_range)
    out = []
    for p, q in zip(a, b):
        r = p.copy()
        r[:, r.shape[1] // 2:] = q[:, r.shape[1] // 2:]
        out.append(r)
    return out


@pytest.fixture()
def eng(engine):
    engine.set_variant("vec_lds")
    engine.set_precision("strict")
    yield engine
    engine.set_precision("strict")
    engine.set_variant("auto")


def _apply_and_check(eng, orc, lut, fmt, depth, csx, csy, src, mode, prec, what, kw=None, dl=None, prelut=None, table=None, scale=None):
    """One apply under `prec`, against that precision's reference.  Returns the kernel's name."""
    kw = kw or {}
    dl = depth if dl is None else dl
    table = lut.table if table is None else table
    scale = lut.scale if scale is None else scale
    eng.set_precision(prec)
    got = _host(eng.apply_yuv(_dev(src), pix_fmt=fmt, interp=mode, **kw), depth)
    kern = eng.last_kernel
    k = orc.yuv_constants("bt709", "tv", "bt709", "tv", depth, dl, depth, 1 << (csx + csy), prologue="range_src" in kw)
    strict = orc.apply_yuv(table, scale, mode, k, depth, dl, depth, csx, csy, src, prelut=prelut)
    if ",fast" in kern:
        _same(got, orc.apply_yuv(table, scale, mode, k, depth, dl, depth, csx, csy, src, fast=True), f"{what} [{kern}] against the fast oracle")
        # ... and within one code of strict, the tolerance of tests/test_fast_variant.py.  That tolerance is stated in codes of the
        # LUT's depth: where the output is deeper than the LUT (the prologue cases with lut_depth below the container's depth) one
        # LUT code is several output codes, and the comparison with the fast oracle above is the check.
        if dl >= depth:
            for g, s in zip(got, strict):
                assert np.abs(g.astype(np.int32) - s.astype(np.int32)).max() <= 1, (what, kern)
    elif ",fma32" in kern:
        _same(got, _fma32_twin.apply_yuv(table, scale, mode, k, depth, dl, depth, csx, csy, src), f"{what} [{kern}] against the fma32 twin")
    else:
        _same(got, strict, f"{what} [{kern}] against the oracle")
    return kern


# ================================================================== integer cells
FORMATS = (("yuv420p", 8, 1, 1), ("yuv420p10le", 10, 1, 1), ("yuv422p10le", 10, 1, 0), ("yuv444p10le", 10, 0, 0),
           ("yuv420p12le", 12, 1, 1), ("yuv420p16le", 16, 1, 1))


@pytest.mark.parametrize("fmt,depth,csx,csy", FORMATS)
@pytest.mark.parametrize("mode", ("nearest", "trilinear", "tetrahedral"))
def test_depths_modes_and_precisions(eng, orc, fmt, depth, csx, csy, mode):
    """8 and 10 bit take the table variants (12 and 16 the computed coordinates, converted once), under all three precisions."""
    lut, _ = dc.make_lut("u33", None)
    eng.set_lut(lut)
    src = _halves(depth, csx, csy, 11)
    for prec in ("strict", "fast", "fma32"):
        kern = _apply_and_check(eng, orc, lut, fmt, depth, csx, csy, src, mode, prec, f"{fmt} {mode} {prec}")
        assert "k_yuv_tile2" in kern and ((",tab" in kern) == (depth <= 10)), kern
        if depth <= 10 and mode != "nearest":
            assert (",fast" in kern) == (prec == "fast") and (",fma32" in kern) == (prec == "fma32"), kern


@pytest.mark.parametrize("fmt,depth,kw", [("yuv420p10le", 10, dict(range_src="pc", range_in="tv", lut_depth=8)),
                                          ("yuv420p", 8, dict(range_src="pc", range_in="tv")),
                                          ("yuv420p12le", 12, dict(range_src="pc", range_in="tv", lut_depth=10))])
def test_prologue(eng, orc, fmt, depth, kw):
    """range_src="pc": the table is indexed with the prologue's codes at the LUT's depth, in a container of another depth."""
    lut, _ = dc.make_lut("u33", None)
    eng.set_lut(lut)
    src = _halves(depth, 1, 1, 13, full_range=True)
    for mode in ("trilinear", "tetrahedral"):
        for prec in ("strict", "fast", "fma32"):
            kern = _apply_and_check(eng, orc, lut, fmt, depth, 1, 1, src, mode, prec, f"{fmt} pc {mode} {prec}", kw=kw,
                                    dl=kw.get("lut_depth", depth))
            assert ",pre," in kern and ",tab" in kern, kern


def test_shared_prelut(eng, orc, tmp_path):
    """A shared .csp shaper: the table holds the cells of the folded coordinate."""
    lut, path = dc.make_lut("shaper", tmp_path)
    eng.set_lut(lut)
    _, scale, table, prelut = orc.parse_lut_file_ex(path)
    src = _halves(10, 1, 1, 15)
    for mode in ("trilinear", "tetrahedral"):
        kern = _apply_and_check(eng, orc, lut, "yuv420p10le", 10, 1, 1, src, mode, "strict", f"shaper {mode}", prelut=prelut,
                                table=table, scale=scale)
        assert ",tab" in kern and "+tube" in kern, kern


@pytest.mark.parametrize("name,whole,tube", [("u17", True, False), ("u33", False, True), ("log65", False, False)])
def test_lattice_sizes(eng, orc, name, whole, tube):
    """17^3: the whole lattice in LDS (float4 nodes for strict tetrahedral); 33^3: tube and windows; 65^3: windows alone."""
    lut, _ = dc.make_lut(name, None)
    eng.set_lut(lut)
    src = _halves(10, 1, 1, 17)
    for mode in ("nearest", "trilinear", "tetrahedral"):
        for prec in ("strict", "fast", "fma32"):
            kern = _apply_and_check(eng, orc, lut, "yuv420p10le", 10, 1, 1, src, mode, prec, f"{name} {mode} {prec}")
            assert ("+whole-lattice" in kern) == whole, kern
            if mode != "nearest":
                assert ("+tube" in kern) == tube, kern


@pytest.mark.parametrize("fmt,depth", [("yuv420p", 8), ("yuv420p10le", 10)])
def test_first_and_last_table_entries(eng, orc, fmt, depth):
    """Frames of code 0, of the top code, and of (Y top, Cr top) with Cb 0: the largest sums the YUV -> RGB matrix can make, i.e. the
    last padded entries of the table, and index 0."""
    lut, _ = dc.make_lut("u33", None)
    eng.set_lut(lut)
    top = (1 << depth) - 1
    dt = np.uint8 if depth == 8 else np.uint16
    shape_y, shape_c = (H, W), (H // 2, W // 2)
    for name, (y, cb, cr) in {"zero": (0, 0, 0), "top": (top, top, top), "y-cr-top": (top, 0, top), "y-cb-top": (top, top, 0)}.items():
        src = [np.full(shape_y, y, dt), np.full(shape_c, cb, dt), np.full(shape_c, cr, dt)]
        for mode in ("nearest", "trilinear", "tetrahedral"):
            for prec in ("strict", "fast", "fma32"):
                _apply_and_check(eng, orc, lut, fmt, depth, 1, 1, src, mode, prec, f"{fmt} {name} {mode} {prec}")


def test_container_values_above_the_depth_take_the_clamping_body(eng, orc):
    """0xFFFF in a 10-bit frame's 16-bit containers, in each plane in turn: the gather body clamps the table index."""
    lut, _ = dc.make_lut("u33", None)
    eng.set_lut(lut)
    clean = _grey_frame(10, 7, W, H)              # wholly inside the tube: no gather tile without the sample
    for plane, (r, c) in ((0, (5, 7)), (1, (3, 3)), (2, (20, 90))):
        src = [p.copy() for p in clean]
        src[plane][r, c] = 0xFFFF
        for mode in ("trilinear", "tetrahedral"):
            for prec in ("strict", "fast", "fma32"):
                eng.tile_stats(True)
                _apply_and_check(eng, orc, lut, "yuv420p10le", 10, 1, 1, clean, mode, prec, f"clean {mode} {prec}")
                assert eng.tile_stats(False)["global_tiles"] == 0
                eng.tile_stats(True)
                _apply_and_check(eng, orc, lut, "yuv420p10le", 10, 1, 1, src, mode, prec, f"0xFFFF in plane {plane} {mode} {prec}")
                assert eng.tile_stats(False)["global_tiles"] == 1


def test_rgb_tube_kernels_keep_their_float_table(eng, orc):
    """rgb24 and gbrp10le through k_rgb_tube (lutr_rgb2.hip), which shares lutr_tube.h and keeps the float {prev, frac} table."""
    import torch
    lut, _ = dc.make_lut("u33", None)
    eng.set_lut(lut)
    g, b, r = frames.make_rgb("natural", W, H, 8, k=21)
    img = np.stack([r, g, b], axis=-1)
    got = eng.apply_packed(torch.from_numpy(img).to("cuda:0"), pix_fmt="rgb24", interp="tetrahedral")
    assert eng.last_kernel.startswith("k_rgb_tube<ly2,"), eng.last_kernel
    assert np.array_equal(got.cpu().numpy(), orc.apply_packed(lut.table, lut.scale, "rgb24", "tetrahedral", img))
    src = frames.make_rgb("vivid", W, H, 10, k=22)
    got = _host(eng.apply_rgb(_dev(src), depth=10, interp="tetrahedral"), 10)
    assert eng.last_kernel.startswith("k_rgb_tube<ly1,"), eng.last_kernel
    _same(got, orc.apply_rgb(lut.table, lut.scale, 10, "tetrahedral", src), "gbrp10le")


# ================================================================== legality by OR
def _grey_frame(depth, seed, w=256, h=16):
    """Natural luma, chroma within +-6 codes (10-bit scale) of mid grey: wholly inside the tube."""
    rng = np.random.default_rng(990000 + seed)
    y = frames.natural_yuv(w, h, depth, 1, 1, k=seed)[0]
    s, mid = (1 << depth) // 1024 or 1, 1 << (depth - 1)
    c = [(mid + rng.integers(-6 * s, 6 * s + 1, size=(h // 2, w // 2))).astype(y.dtype) for _ in range(2)]
    return [y] + c


def _run(eng, orc, lut, fmt, depth, src, what):
    eng.tile_stats(True)
    kern = _apply_and_check(eng, orc, lut, fmt, depth, 1, 1, src, "tetrahedral", "strict", what)
    return eng.tile_stats(False), kern


def test_one_illegal_sample_sends_exactly_its_tile_to_the_gather_body(eng, orc):
    """A 10-bit 4:2:0 frame of 2 x 2 tiles that lies wholly in the tube.  A lane's unit is 8 x 2 luma samples and 4 x 1 samples of
    each chroma plane; the unit of lane (3, 1) of the tile at (1, 0) gets one sample of 1024, 0x8000 or 0xFFFF at each of its
    positions in turn, plane by plane.  1024 is the smallest illegal code and sets one bit that no legal sample has; 0x8000 sets the
    top bit alone; 0xFFFF every bit.  Each frame must equal the oracle and count one gather tile more than the clean frame (which has
    none: all four tiles take the tube).
    1023, the largest legal code, in luma must leave every counter as it is.  In a chroma plane it cannot -- 1023 is far outside the
    tube, whose vote is on chroma -- but it is legal: the tile stays out of the gather body (it becomes a mixed tile)."""
    lut, _ = dc.make_lut("u33", None)
    eng.set_lut(lut)
    clean = _grey_frame(10, 3)
    st0, kern = _run(eng, orc, lut, "yuv420p10le", 10, clean, "clean")
    assert kern == "k_yuv_tile2<11,11,2,tab,unit>+tube", kern
    assert st0["tiles"] == 4 and st0["tube_tiles"] == 4 and st0["global_tiles"] == 0, st0
    # tile (1, 0): luma rows 8..15, columns 0..127; lane (3, 1): luma columns 24..31, rows 10..11; chroma columns 12..15, row 5
    spots = [(0, 10 + dy, 24 + dx) for dy in range(2) for dx in range(8)] + [(p, 5, 12 + dx) for p in (1, 2) for dx in range(4)]
    for value in (1024, 0x8000, 0xFFFF):
        for plane, r, c in spots:
            src = [p.copy() for p in clean]
            src[plane][r, c] = value
            st, _ = _run(eng, orc, lut, "yuv420p10le", 10, src, f"{value:#x} in plane {plane} at ({r}, {c})")
            assert st["global_tiles"] == 1 and st["tube_tiles"] == 3 and st["tiles"] == 4, (value, plane, r, c, st)
    for plane, r, c in spots:
        src = [p.copy() for p in clean]
        src[plane][r, c] = 1023
        st, _ = _run(eng, orc, lut, "yuv420p10le", 10, src, f"1023 in plane {plane} at ({r}, {c})")
        if plane == 0:
            assert st == st0, (plane, r, c, st, st0)
        else:
            assert st["global_tiles"] == 0 and st["tube_tiles"] == 3 and st["mixed_tiles"] == 1, (plane, r, c, st)


@pytest.mark.parametrize("depth", (9, 12, 14))
def test_legality_at_other_depths_in_16_bit_containers(eng, orc, depth):
    """2^depth in luma or in a chroma plane is illegal at every depth (one gather tile more than the clean frame); 2^depth - 1 in luma
    is not (no counter moves)."""
    lut, _ = dc.make_lut("u33", None)
    eng.set_lut(lut)
    fmt = f"yuv420p{depth}le"
    clean = _grey_frame(depth, 5)
    st0, kern = _run(eng, orc, lut, fmt, depth, clean, f"{fmt} clean")
    assert "k_yuv_tile2<11,11" in kern and (",tab" in kern) == (depth <= 10), kern
    for dy, dx in ((0, 0), (1, 7)):
        src = [p.copy() for p in clean]
        src[0][10 + dy, 24 + dx] = 1 << depth
        st, _ = _run(eng, orc, lut, fmt, depth, src, f"{fmt} 2^{depth} at ({dy}, {dx})")
        assert st["global_tiles"] == st0["global_tiles"] + 1, (st, st0)
        src[0][10 + dy, 24 + dx] = (1 << depth) - 1
        st, _ = _run(eng, orc, lut, fmt, depth, src, f"{fmt} 2^{depth} - 1 at ({dy}, {dx})")
        assert st["global_tiles"] == st0["global_tiles"] and st["tube_tiles"] == st0["tube_tiles"], (st, st0)
    for plane in (1, 2):
        src = [p.copy() for p in clean]
        src[plane][5, 13] = 1 << depth
        st, _ = _run(eng, orc, lut, fmt, depth, src, f"{fmt} 2^{depth} in plane {plane}")
        assert st["global_tiles"] == st0["global_tiles"] + 1, (plane, st, st0)
