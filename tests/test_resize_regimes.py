"""The resize kernel in the tile regimes real downscales run in, and the contract against a plain resampler.

The host plans every resize launch (`resize_plan` in lutr_api.cpp, exported host-only as lutr_resize_plan): `th`, the output rows
of a tile (64, 32 or 16: the tallest whose LDS stays within 40 KiB with one staged row), `rows`, the source rows a wave stages per
step (8 down to 1: the most whose LDS stays within 64 KiB), and with the footprints `spx` / `spy` the depth of the kernel's two
loops: `xiters = ceil(spx / 256)` trips of the footprint copy and `ceil(spy / (4 rows))` row steps of the horizontal pass.

Regimes covered before: every geometry of the other GPU tests plans `(th, rows)` = `(64, 8)` with one trip of the copy; the one
exception, 256x64 -> 32x8, plans `(32, 8)` on a single tile.  `th = 16`, `rows < 8`, a second or third trip of the copy and
`oy0 = ty * A.th` with `ty > 0` below 64 rows never ran.  Covered after (`CASES`, each re-derived on the CPU from the twin's
tables by this module's own statement of the rule and pinned to the UHD geometry it stands for): `(th, rows, xiters, row steps)` =
(32, 8, 1, 4) as UHD -> 720p, (16, 8, 2, 3) as UHD -> 540p, (16, 8, 2, 4) as UHD -> 640x360, (16, 5, 2, 7) as UHD -> 548x308,
(16, 3, 3, 13) as UHD -> 480x270 (also with a ragged source and a ragged destination), (64, 8, 3, 3) as UHD -> 480x2160,
(16, 8, 1, 5) for a vertical-only reduction, and the launch at the LDS limit itself, on 3 x 3 or 3 x 5 luma tiles with the last
tile ragged in both directions.  On the GPU every case is bit-exact against the twin, into sentinel-filled destinations.

Largest LDS of the sweep of legal ratios (`test_no_legal_geometry_is_refused_for_lds`): exactly 65536 bytes, at
511x512 -> 64x74 4:2:0; `launch_resize` refuses more than that, so the size is launched (`full-lds`).

Largest derived bound of `test_twin_stays_within_the_derived_bound_of_the_plain_resampler`, in codes: 0.89 at 8 bit, 2.07 at
10 bit, 101.1 at 16 bit, all at 8:1 on both axes with 32 taps each (the Q14 rounding of the taps times the code range, plus the
two rounding shifts); the twin stays within it on every sample, and a resampler half a source sample off, or with the other
chroma siting, does not.

That the GPU cases can fail was checked once by hand with two in-bounds mutations of k_resize, neither committed.  With
`oy0 = min(ty * 64, P.dh - 1)` in place of `ty * A.th` (the tile's row origin as if every tile were 64 rows tall, kept inside the
plane so that every table read and every store stays valid) every case below `th = 64` failed -- r3, r4, r6, r7, r8 in every
variant, both r8-odd, y8, full-lds and the composition case, 31 tests; x8 (`th = 64`) and all of tests/test_resize.py passed.
With `rstep = 4 * kRzRows` in place of `4 * A.rows` (source rows left out of T whenever `rows < 8`: reads of LDS the block owns
but never wrote) r7, r8 in every variant, both r8-odd, full-lds and the composition case failed, 13 tests; every `rows = 8` case
and all of tests/test_resize.py passed.

Defects found: none -- the plan, the kernel in every regime and the contract against the plain resampler hold."""
import functools
import math

import numpy as np
import pytest

from lut_renderer_amd import _native, frames
from tests import _resize_twin as tw
from tests.test_resize import LAYOUTS, _dev, _eq, _fmt, _host, _planes

UHD = (3840, 2160)
#: UHD 4:2:0 -> size: (th, rows, xiters, row steps, LDS bytes)
PRODUCTION = {(1920, 1080): (64, 8, 1, 5, 47488), (1280, 720): (32, 8, 1, 4, 44800), (960, 540): (16, 8, 2, 3, 42048),
              (640, 360): (16, 8, 2, 4, 62912), (548, 308): (16, 5, 2, 7, 63616), (480, 270): (16, 3, 3, 13, 62336),
              (480, 2160): (64, 8, 3, 3, 61184)}
#: id -> (sw, sh, dw, dh), (th, rows, xiters, row steps), the UHD target it stands for
CASES = {
    "r3": ((392, 264, 130, 88), (32, 8, 1, 4), (1280, 720)),
    "r4": ((520, 280, 130, 70), (16, 8, 2, 3), (960, 540)),
    "r6": ((780, 420, 130, 70), (16, 8, 2, 4), (640, 360)),
    "r7": ((910, 490, 130, 70), (16, 5, 2, 7), (548, 308)),
    "r8": ((1040, 560, 130, 70), (16, 3, 3, 13), (480, 270)),
    "r8-odd-src": ((1037, 557, 130, 70), (16, 3, 3, 13), (480, 270)),
    "r8-odd-dst": ((1040, 560, 131, 71), (16, 3, 3, 13), (480, 270)),
    "x8": ((1040, 70, 130, 70), (64, 8, 3, 3), (480, 2160)),
    "y8": ((130, 560, 130, 70), (16, 8, 1, 5), None),
    "full-lds": ((511, 512, 64, 74), (16, 5, 3, None), None),
}
WIDE = ("r3", "r4", "r8")            # the cases that also run in other layouts, depths and as a padded batch


# ================================================================== this module's own statement of the plan
@functools.lru_cache(maxsize=None)
def _axis(src, dst, cs, cosited):
    """(taps, {run length: most source samples an aligned run of that many outputs reads}) of one axis table of the twin."""
    start, w = tw.table(src, dst, cs, cosited)
    n, m = w.shape[1], len(start)
    return n, {run: max(int(start[min(u0 + run, m) - 1]) + n - int(start[u0]) for u0 in range(0, m, run)) for run in (64, 32, 16)}


def _lds(th, rows, spx, spy, nx, ny):
    """T [spy][64], WX [nx][64], XS [64], WY [th][ny], YS [th] as int32; then 4 waves x rows x spx staged uint16 samples."""
    return (spy * 64 + nx * 64 + 64 + th * ny + th) * 4 + 4 * rows * spx * 2


def _ceil(n, d):
    return -(-n // d)


def plan(sw, sh, dw, dh, csx, csy, loc):
    cox, coy = tw.COSITED[loc]
    ax = [_axis(sw, dw, cx, bool(cox and cx)) for cx in (0, csx, csx)]
    ay = [_axis(sh, dh, cy, bool(coy and cy)) for cy in (0, csy, csy)]
    spx = max(a[1][64] for a in ax)
    spx += spx & 1
    nx, ny = max(a[0] for a in ax), max(a[0] for a in ay)
    for th in (64, 32, 16):
        spy = max(a[1][th] for a in ay)
        if th == 16 or _lds(th, 1, spx, spy, nx, ny) <= 40 * 1024:
            break
    rows = 8
    while rows > 1 and _lds(th, rows, spx, spy, nx, ny) > 64 * 1024:
        rows -= 1
    tiles = sum(_ceil(_ceil(dw, 1 << cx), 64) * _ceil(_ceil(dh, 1 << cy), th) for cx, cy in ((0, 0), (csx, csy), (csx, csy)))
    return dict(th=th, rows=rows, lds=_lds(th, rows, spx, spy, nx, ny), spx=spx, spy=spy, nx_max=nx, ny_max=ny,
                tiles_per_frame=tiles)


def regime(p):
    return p["th"], p["rows"], _ceil(p["spx"], 256), _ceil(p["spy"], 4 * p["rows"])


def _native_plan(sw, sh, dw, dh, csx, csy, loc, family="yuv", depth=10):
    return _native.resize_plan(family, depth, csx, csy, loc, sw, sh, dw, dh)


# ================================================================== CPU: the plan
def test_plan_equals_the_formula_on_the_production_table_and_the_cases():
    for (dw, dh), (th, rows, xiters, steps, lds) in PRODUCTION.items():
        p = plan(*UHD, dw, dh, 1, 1, None)
        assert p == _native_plan(*UHD, dw, dh, 1, 1, None), (dw, dh)
        assert regime(p) == (th, rows, xiters, steps) and p["lds"] == lds, (dw, dh, p)
    for cid, (geom, _, _) in CASES.items():
        for csx, csy, loc in ((1, 1, None), (1, 1, "topleft"), (1, 0, "left"), (0, 0, None)):
            assert plan(*geom, csx, csy, loc) == _native_plan(*geom, csx, csy, loc), (cid, csx, csy, loc)
        assert plan(*geom, 0, 0, None) == _native_plan(*geom, 0, 0, None, family="gbr", depth=16), cid
    # the one earlier case off (64, 8), and a plain upscale
    assert regime(plan(256, 64, 32, 8, 1, 1, None))[:2] == (32, 8)
    assert regime(plan(41, 23, 82, 47, 1, 1, None)) == (64, 8, 1, 1)


def test_plan_applies_the_argument_checks_of_resize_planes():
    ok = dict(family="yuv", depth=10, csx=1, csy=1, chroma_loc=None, sw=64, sh=36, dw=32, dh=18)
    assert _native.resize_plan(**ok)["th"] == 64
    for bad in (dict(depth=7), dict(depth=17), dict(csx=2), dict(csy=-1), dict(family="gbr"), dict(sw=0), dict(dh=0),
                dict(sw=257, dw=32), dict(dw=16 * 64 + 1), dict(sh=8 * 18 + 1), dict(dh=16 * 36 + 1)):
        with pytest.raises(_native.LutrError) as e:
            _native.resize_plan(**{**ok, **bad})
        assert e.value.code == _native.EINVAL and e.value.message, bad
    lib = _native.load()
    assert lib.lutr_resize_plan(7, 10, 1, 1, 0, 64, 36, 32, 18, (_native.C.c_int * 8)()) == _native.EINVAL      # family
    assert lib.lutr_resize_plan(0, 10, 1, 1, 4, 64, 36, 32, 18, (_native.C.c_int * 8)()) == _native.EINVAL      # chroma_loc
    assert lib.lutr_resize_plan(0, 10, 1, 1, 0, 64, 36, 32, 18, None) == _native.EINVAL


SWEEP_RATIOS = (8, 7.9, 7, 6.5, 6, 5, 4, 3, 2, 1.5, 1, 1 / 2, 1 / 16)
SWEEP_SIZES = tuple(c + e for c in (64, 128, 512, 1040) for e in (-1, 0, 1))
SWEEP_LAYOUTS = ((1, 1, None), (1, 1, "topleft"), (0, 0, None))


def _sweep_axes():
    """(src, dst) per axis: every sweep size at every sweep ratio, dst the smallest size the ratio allows."""
    return [(s, math.ceil(s / r)) for s in SWEEP_SIZES for r in SWEEP_RATIOS]


def test_no_legal_geometry_is_refused_for_lds():
    """The LDS of the plan over the sweep: every horizontal axis with every vertical axis, by this module's formula (the plan is
    a function of the two axes' tables alone).  The largest seen is exactly 65536 bytes, at 511x512 -> 64x74 4:2:0 (both chroma
    sitings): the limit `launch_resize` still launches.  No legal geometry is refused."""
    axes = _sweep_axes()
    assert all(tw.in_limits(s, d) for s, d in axes)
    worst = (0, None)
    for csx, csy, loc in SWEEP_LAYOUTS:
        for sw, dw in axes:
            for sh, dh in axes:
                p = plan(sw, sh, dw, dh, csx, csy, loc)
                assert p["lds"] <= 65536 and 1 <= p["rows"] <= 8, (sw, sh, dw, dh, csx, csy, loc, p)
                if p["lds"] > worst[0]:
                    worst = (p["lds"], (sw, sh, dw, dh, csx, csy, loc))
    print(f"largest LDS of the sweep: {worst[0]} bytes, first at {worst[1]}")
    assert worst[0] == 65536
    assert plan(511, 512, 64, 74, 1, 1, None)["lds"] == _native_plan(511, 512, 64, 74, 1, 1, None)["lds"] == 65536


def test_plan_equals_the_formula_over_the_sweep():
    """lutr_resize_plan against the formula, field by field: every sweep axis horizontally with every ratio vertically on a
    source height of the same size group, and the same with the axes exchanged."""
    axes = _sweep_axes()
    n = 0
    for csx, csy, loc in SWEEP_LAYOUTS:
        for s, d in axes:
            group = [a for a in axes if abs(a[0] - s) <= 2]
            for s2, d2 in group:
                for geom in ((s, s2, d, d2), (s2, s, d2, d)):
                    assert plan(*geom, csx, csy, loc) == _native_plan(*geom, csx, csy, loc), (geom, csx, csy, loc)
                    n += 1
    assert n == 2 * 3 * len(axes) * 3 * len(SWEEP_RATIOS)


def _tiles(size, th, cx, cy):
    return _ceil(_ceil(size[0], 1 << cx), 64), _ceil(_ceil(size[1], 1 << cy), th)


def test_every_case_reaches_its_regime():
    for cid, (geom, want, stands) in CASES.items():
        p = plan(*geom, 1, 1, None)
        got = regime(p)
        assert got[:3] == want[:3] and (want[3] is None or got[3] == want[3]), (cid, got, p)
        if stands is not None:                       # the regime of the UHD geometry it names, by the same formula
            assert got == regime(plan(*UHD, *stands, 1, 1, None)) == PRODUCTION[stands][:4], cid
        th, (dw, dh) = p["th"], geom[2:]
        cw, ch = _ceil(dw, 2), _ceil(dh, 2)
        if cid in ("r3", "r4", "r6", "r7", "r8", "r8-odd-src", "r8-odd-dst"):
            # tile indices above 0 in both directions on luma and chroma, the last tile ragged in both directions
            assert _tiles((dw, dh), th, 0, 0)[0] >= 2 and _tiles((dw, dh), th, 0, 0)[1] >= 3, cid
            assert _tiles((dw, dh), th, 1, 1)[1] >= 2, cid
            assert dw % 64 and dh % th and cw % 64 and ch % th, cid
        else:                                        # one axis only, or the limit: more than one tile row on luma, ragged
            assert _tiles((dw, dh), th, 0, 0)[1] >= 2 and dh % th, cid
        # every layout the wide cases run in keeps the regime (the chroma planes never set a larger footprint than luma's)
        if cid in WIDE:
            for csx, csy, loc in ((1, 1, "topleft"), (1, 0, "left"), (0, 0, None)):
                assert regime(plan(*geom, csx, csy, loc)) == got, (cid, csx, csy, loc)
    assert plan(*CASES["r6"][0], 1, 1, None)["lds"] == 62912
    assert plan(*CASES["full-lds"][0], 1, 1, None)["lds"] == 65536
    # and what the suite ran before: one corner
    from tests.test_resize import _GEOMS
    assert {regime(plan(*g, 1, 1, None))[:3] for g in _GEOMS} == {(64, 8, 1)}


# ================================================================== CPU: the contract against a plain resampler
def _kernel(t):
    """Bicubic, B = 0, C = 0.6."""
    a = np.abs(t)
    inner, outer = 1.4 * a ** 3 - 2.4 * a ** 2 + 1.0, -0.6 * a ** 3 + 3.0 * a ** 2 - 4.8 * a + 2.4
    return np.where(a < 1.0, inner, np.where(a < 2.0, outer, 0.0))


def _ideal_axis(src, dst, cs, cosited, shift=0.0):
    """Source indices [n_out, n] (unclamped) and float64 weights [n_out, n] of one axis of one plane, from the text of 3.7;
    `shift` moves every position by that many source samples (the negative control)."""
    f = src / dst
    stretch = max(1.0, f)
    n = 2 * math.ceil(2.0 * stretch)
    step = 1 << cs
    o = 0.0 if cosited else (step - 1) / 2.0
    j = np.arange(_ceil(dst, step), dtype=np.float64)
    x = ((step * j + o + 0.5) * f - 0.5 - o) / step + shift
    idx = (np.floor(x).astype(np.int64) - n // 2 + 1)[:, None] + np.arange(n)[None, :]
    w = _kernel((idx - x[:, None]) / stretch)
    return idx, w / w.sum(1, keepdims=True)


def ideal(plane, sizes, cs, cosited, depth, shift=0.0):
    """The resampler of DESIGN.md 3.7 in float64 with no Q14 and no intermediate rounding: `plane` [H, W] of a frame of luma
    size sizes[0] = (w, h) resampled to sizes[1], cs = (csx, csy) the plane's subsampling, cosited = (x, y)."""
    (sw, sh), (dw, dh) = sizes
    p = np.asarray(plane, np.float64)
    ix, wx = _ideal_axis(sw, dw, cs[0], cosited[0], shift)
    iy, wy = _ideal_axis(sh, dh, cs[1], cosited[1], shift)
    t = (p[:, np.clip(ix, 0, p.shape[1] - 1)] * wx).sum(-1)                     # [H, n_out_x]
    out = (t[np.clip(iy, 0, p.shape[0] - 1), :] * wy[:, :, None]).sum(1)        # [n_out_y, n_out_x]
    return np.clip(out, 0.0, float((1 << depth) - 1))


def _axis_terms(src, dst, cs, cosited):
    """Per output sample of one axis: sum |a|, sum |a - a*|, sum |a*| with a = the twin's Q14 row / 2^14 and a* the float64 row,
    matched on the source index."""
    start, wq = tw.table(src, dst, cs, cosited)
    idx, ws = _ideal_axis(src, dst, cs, cosited)
    n = wq.shape[1]
    lo = np.minimum(start, idx[:, 0])
    a = np.zeros((len(start), n + int(np.abs(start - idx[:, 0]).max())))
    s = np.zeros_like(a)
    rows = np.arange(len(start))[:, None]
    a[rows, (start - lo)[:, None] + np.arange(n)] = wq / 16384.0
    s[rows, (idx[:, 0] - lo)[:, None] + np.arange(n)] = ws
    return np.abs(a).sum(1), np.abs(a - s).sum(1), np.abs(s).sum(1)


def _bound(sizes, cs, cosited, depth):
    """|twin - ideal| per output sample [n_out_y, n_out_x], from the actual table rows:
    M (sum|b| sum|a - a*| + sum|b - b*| sum|a*|) + 0.5 2^(d-16) sum|b| + 0.5."""
    (sw, sh), (dw, dh) = sizes
    _, da, sas = _axis_terms(sw, dw, cs[0], cosited[0])
    sb, db, _ = _axis_terms(sh, dh, cs[1], cosited[1])
    m = float((1 << depth) - 1)
    return m * (sb[:, None] * da[None, :] + db[:, None] * sas[None, :]) + (0.5 * 2.0 ** (depth - 16) * sb + 0.5)[:, None]


def _content(lay, w, h, depth, k, nframes=1):
    """`_planes` of tests/test_resize.py (smooth + noise + hard edges) plus a ramp along x and against y, an eighth of the code
    range each across the plane, clamped: no two tiles hold alike content, and both ends of the range stay in the picture."""
    m = (1 << depth) - 1
    out = []
    for p in _planes(lay, w, h, depth, k, nframes):
        ph, pw = p.shape[-2:]
        yy, xx = np.mgrid[0:ph, 0:pw]
        ramp = (xx * (m // 8)) // pw - (yy * (m // 8)) // ph
        out.append(np.clip(p.astype(np.int64) + ramp, 0, m).astype(p.dtype))
    return out


IDEAL_CASES = {cid: CASES[cid][0] for cid in ("r3", "r4", "r8", "x8", "y8")}
IDEAL_CASES.update({"up2": (65, 37, 130, 74), "up16": (20, 12, 320, 192)})


@pytest.mark.parametrize("cid", list(IDEAL_CASES))
def test_twin_stays_within_the_derived_bound_of_the_plain_resampler(cid):
    """The integer contract (tw.resize) against `ideal`, per output sample, under the bound of `_bound` -- derived from the Q14
    rows and the two rounding shifts, not measured.  Luma and 4:2:0 chroma at both sitings, 8, 10 and 16 bit.  The largest bound
    over all cases, in codes: 0.891 at 8 bit, 2.069 at 10 bit, 101.043 at 16 bit, all on r8 (printed below; recorded, not
    asserted).  Negative controls on the same content: the ideal moved by half a source sample, and the ideal with the other
    chroma siting, both exceed the bound somewhere -- the bound tells a misplaced resampler from a rounded one."""
    sw, sh, dw, dh = IDEAL_CASES[cid]
    sizes = ((sw, sh), (dw, dh))
    for depth in (8, 10, 16):
        src = _content("420", sw, sh, depth, 3)
        worst = 0.0
        for loc in (None, "topleft"):
            got = tw.resize(src, depth, 1, 1, *sizes, loc)
            co = tw.COSITED[loc]
            for pi, cs, cosited in ((0, (0, 0), (False, False)), (1, (1, 1), co)):
                if pi == 0 and loc is not None:
                    continue                                     # luma does not depend on the siting
                b = _bound(sizes, cs, cosited, depth)
                worst = max(worst, float(b.max()))
                err = np.abs(got[pi].astype(np.float64) - ideal(src[pi], sizes, cs, cosited, depth))
                assert (err <= b).all(), (cid, depth, loc, pi, float((err - b).max()))
                moved = np.abs(got[pi].astype(np.float64) - ideal(src[pi], sizes, cs, cosited, depth, shift=0.5))
                assert (moved > b).any(), (cid, depth, loc, pi, "shifted ideal passes")
                if pi:
                    other = (not cosited[0], not cosited[1])
                    swapped = np.abs(got[pi].astype(np.float64) - ideal(src[pi], sizes, cs, other, depth))
                    assert (swapped > b).any(), (cid, depth, loc, "swapped siting passes")
        print(f"{cid} depth {depth}: largest derived bound {worst:.3f} codes")


# ================================================================== GPU: every regime, bit for bit against the twin
def _variants():
    out = [(cid, "420", None, 10, 1) for cid in CASES]
    for cid in WIDE:
        out += [(cid, "420", "topleft", 10, 1), (cid, "422", "left", 10, 1), (cid, "444", None, 10, 1), (cid, "gbrp", None, 10, 1),
                (cid, "420", None, 8, 1), (cid, "420", None, 16, 1), (cid, "420", None, 10, 3)]
    return out


def _padded(planes, device, fill, pad_rows, pad_cols, row0, col0):
    """Device views [F, H, W] holding `planes` (or, with planes = shapes, nothing yet) inside buffers of `fill` with spare rows,
    spare columns and so padded frames."""
    import torch
    views = []
    for p in planes:
        shape = p if isinstance(p, tuple) else p.shape
        dt = torch.uint8 if fill >= 0 else torch.int16
        buf = torch.full((shape[0], shape[1] + pad_rows, shape[2] + pad_cols), fill, dtype=dt, device=device)
        view = buf[:, row0:row0 + shape[1], col0:col0 + shape[2]]
        if not isinstance(p, tuple):
            view.copy_(torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).to(device))
        views.append(view)
    return views


def _sentinel_intact(views, fill, row0, col0):
    """Everything of the views' buffers outside the views still holds `fill`."""
    for v in views:
        b = v._base.cpu().numpy()
        spare = np.ones(b.shape, bool)
        spare[:, row0:row0 + v.shape[1], col0:col0 + v.shape[2]] = False
        if not (b[spare] == fill).all():
            return False
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("cid,lay,loc,depth,nf", _variants(), ids=lambda v: "none" if v is None else str(v))
def test_resize_cases_equal_the_twin(engine, cid, lay, loc, depth, nf):
    """engine.resize in the regime of `cid` (re-derived by `plan`, equal to the library's own) bit for bit against the twin, into
    destinations that are views of sentinel-filled buffers with a spare row above and below and spare columns on both sides; the
    batch of 3 also reads its source through padded rows and padded frames.  The spare area keeps the sentinel.

    The `full-lds` launch asks for exactly 65536 bytes of dynamic LDS, the most `launch_resize` allows: the runtime takes it and
    the result is exact.  The module docstring tells which kernel mutations these cases were seen to catch."""
    import torch
    sw, sh, dw, dh = CASES[cid][0]
    csx, csy = (0, 0) if lay == "gbrp" else LAYOUTS[lay]
    family = "gbr" if lay == "gbrp" else "yuv"
    p = _native.resize_plan(family, depth, csx, csy, loc, sw, sh, dw, dh)
    assert p == plan(sw, sh, dw, dh, csx, csy, loc)
    want_regime = CASES[cid][1]
    assert regime(p)[:3] == want_regime[:3] and (want_regime[3] is None or regime(p)[3] == want_regime[3])
    src = _content(lay, sw, sh, depth, 11, nframes=nf)
    src3 = [s.reshape((nf,) + s.shape[-2:]) for s in src]
    fill = 0xA5 if depth == 8 else -1
    shapes = [(nf, dh, dw)] + [(nf,) + frames.chroma_shape(dw, dh, csx, csy)] * 2
    dst = _padded(shapes, engine.device, fill, 2, 6, 1, 3)
    dev = _padded(src3, engine.device, 0 if depth == 8 else -1, 3, 10, 1, 2) if nf > 1 else _dev(src3, engine.device)
    engine.resize(dev, dst, pix_fmt=_fmt(depth, lay), size=(dw, dh), chroma_loc=loc)
    torch.cuda.synchronize()
    assert engine.last_kernel == ("k_resize<8>" if depth == 8 else "k_resize<16>")
    want = tw.resize(src3, depth, csx, csy, (sw, sh), (dw, dh), loc)
    got = _host(dst, depth)
    for i, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(g != w)
        assert not len(bad), (cid, lay, loc, depth, nf, f"plane {i}: {len(bad)} samples differ, first at (f, y, x) = {bad[0]}")
    assert _sentinel_intact(dst, fill, 1, 3)


@pytest.mark.gpu
def test_apply_yuv_out_size_in_the_deepest_regime(engine, cube_dir):
    """LUT + resize, 5 frames of 1040x560 in chunks of 2 (the last chunk a single frame) into 130x70: the r8 regime behind the
    engine's scratch.  Equal to the twin's resize of the un-resized apply_yuv output."""
    engine.load_cube(cube_dir / "log709_33.cube")
    sw, sh, dw, dh = CASES["r8"][0]
    src = [np.stack(p) for p in zip(*[frames.natural_yuv(sw, sh, 10, 1, 1, k=60 + i) for i in range(5)])]
    dev = _dev(src, engine.device)
    got = _host(engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_size=(dw, dh), resize_chunk=2), 10)
    assert engine.last_kernel == "k_resize<16>"
    full = _host(engine.apply_yuv(dev, pix_fmt="yuv420p10le"), 10)
    assert _eq(got, tw.resize(full, 10, 1, 1, (sw, sh), (dw, dh)))
