"""Engine output against call history.  `api.apply_lut` keeps one LutEngine per device tuple for the life of the process and a
context carries state derived from earlier calls: the fp16 / fp32 pre-multiplied lattice copies, the folded prelut tables, the
`unit` flag, the resize tables, the work-queue words every tile and tube launch leaves at zero, and two memos in the tile
launcher.  Every result here is compared with a reference computed from scratch (the oracle, or the fast / fma32 / sited /
resize twins), never with another GPU run -- except the tube tile count of case A, which is compared with an engine that saw
only the one shaper.  Destinations start as a sentinel so that an unwritten sample cannot pass."""
import os
import random

import numpy as np
import pytest
import torch

from lut_renderer_amd import cube, frames
from lut_renderer_amd.engine import LutEngine
from tests import _fma32_twin, _resize_twin, _sited_twin
from tests._csp_files import write_csp_with_prelut

pytestmark = pytest.mark.gpu
F = np.float32
N = 33                  # 33^3: the tile kernels stage a tube (17^3 would be staged whole and has none)


# ------------------------------------------------------------------ helpers
def _dev(planes, device="cuda:0"):
    return [torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to(device)
            for p in planes]


def _np(tensors, depth):
    return [t.cpu().numpy().view(np.uint16) if depth > 8 else t.cpu().numpy() for t in tensors]


def _sentinel(shapes, depth, device="cuda:0"):
    """Output planes pre-filled with a value no kernel writes at 9-16 bit (0xffff); 0xa5 at 8 bit."""
    if depth > 8:
        return [torch.full(s, -1, dtype=torch.int16, device=device) for s in shapes]
    return [torch.full(s, 0xA5, dtype=torch.uint8, device=device) for s in shapes]


def _eq(got, want, what, log=None):
    for i, (a, b) in enumerate(zip(got, want)):
        if a.shape != b.shape or not np.array_equal(a, b):
            if a.shape != b.shape:
                msg = f"{what}: plane {i} shape {a.shape} != {b.shape}"
            else:
                diff = np.abs(a.astype(np.int64) - b.astype(np.int64))
                bad = np.argwhere(diff > 0)
                msg = (f"{what}: plane {i} differs at {len(bad)} samples, max |d|={diff.max()}, "
                       f"first {bad[0].tolist()} got {a[tuple(bad[0])]} want {b[tuple(bad[0])]}")
            if log:
                msg += "\nstep log (replay these in order on one engine):\n  " + "\n  ".join(log)
            raise AssertionError(msg)


def _run_yuv(eng, src, fmt, depth, **kw):
    """apply_yuv into sentinel planes of the source's shapes; returns the host planes."""
    dst = _sentinel([p.shape for p in src], depth)
    eng.apply_yuv(_dev(src), dst, pix_fmt=fmt, **kw)
    return _np(dst, depth)


def _unit_lattice(n, k):
    """A lattice with every node in [0, 1] (so the `unit` kernels apply), different for each k."""
    t = 0.6 * cube.log709_lattice(n) + 0.4 * cube.identity_lattice(n)
    rng = np.random.default_rng(1000 + k)
    t = np.clip(t + rng.uniform(-0.02, 0.02, size=t.shape), 0.0, 1.0)
    return t.astype(F)


def _lut(table, scale=(1.0, 1.0, 1.0), prelut=None):
    return cube.CubeLut(n=table.shape[0], table=np.ascontiguousarray(table, dtype=F), scale=np.array(scale, dtype=F),
                        prelut=prelut)


# ------------------------------------------------------------------ A. the prelut tube bound follows the shaper
XS = np.linspace(0.0, 1.0, 33)
SHAPER_A = XS.copy()
# B equals A up to 0.5, rises to 0.75 by 0.5625 (slope 4), then climbs back onto A by 31/32; A and B agree on the first and the
# last segment, so their folded tables agree on s[1] and s[maxi].  (lut3d resamples a cineSpace shaper into a staircase with a
# jump at every input point -- DESIGN.md 8 -- so a rise of 0.2 per segment, as with slope 6.4, would give B no tube at all at
# H = 5: slope 4 keeps a small bound, 32 codes at 10 bit and 8 at 8 bit, against A's 157 and 39.)
SHAPER_B = np.where(XS <= 0.5, XS, np.where(XS <= 0.5625, 0.5 + 4.0 * (XS - 0.5),
                                             0.75 + (XS - 0.5625) * (0.96875 - 0.75) / (0.96875 - 0.5625)))
SHAPER_B[-1] = 1.0


def fold_prelut(pre, n, depth, ch=0):
    """liblutr's folded prelut table of one channel (lutr_api.cpp prelut_table): the lattice coordinate of every code at this
    LUT depth, float for float."""
    maxi = (1 << depth) - 1
    pmax = pre.table.shape[1] - 1
    lut_max = F(n - 1)
    s = np.arange(maxi + 1, dtype=F) * (F(1.0) / F(maxi))
    x = np.clip((s - pre.min[ch]) * pre.scale[ch], F(0), F(pmax)).astype(F)
    prev = x.astype(np.int32)
    nxt = np.minimum(prev + 1, pmax)
    p, q = pre.table[ch][prev], pre.table[ch][nxt]
    v = (p + (q - p) * (x - prev.astype(F))).astype(F)
    return np.clip((v * lut_max).astype(F), F(0), lut_max)


def tube_bound(s, h):
    """The largest d with D(d) = max over x of s(x + d) - s(x) <= h - 0.002 (lutr_tile2.hip prelut_tube_bound)."""
    lim = F(h) - F(2e-3)
    d = 0
    for c in range(1, len(s)):
        if (s[c:] - s[:-c]).max() > lim:
            break
        d = c
    return d


@pytest.fixture(scope="module")
def shapers(orc, tmp_path_factory):
    d = tmp_path_factory.mktemp("shapers")
    tab = cube.log709_lattice(N)
    out = {}
    for name, ys in (("A", SHAPER_A), ("B", SHAPER_B)):
        p = d / f"{name}.csp"
        write_csp_with_prelut(p, N, tab, [(XS, ys)] * 3)
        _, sc, t, pre = orc.parse_lut_file_ex(p)
        out[name] = dict(path=p, lut=cube.read_lut(p), table=t, scale=sc, pre=pre)
    return out


def _chroma_spread(k):
    """The smallest and largest chroma -> RGB-code gain the tube's chroma bound R divides by (T2_ENTRY, both axis forms)."""
    s = [abs(k.kgu) + abs(k.kgv - k.krv), abs(k.kbu - k.kgu) + abs(k.kgv), abs(k.kbu) + abs(k.krv)]
    return min(s), max(s)


def _steep_band_frame(orc, sh, fmt, din, dl, k, seed):
    """Near-grey 4:2:0 content whose RGB sits in B's steep band and whose chroma offsets (in LUT-depth codes, after any
    prologue) lie between what B's bound admits to the tube and what A's admits."""
    h = 5
    da = tube_bound(fold_prelut(sh["A"]["pre"], N, dl), h)
    db = tube_bound(fold_prelut(sh["B"]["pre"], N, dl), h)
    smin, smax = _chroma_spread(k)
    lo = int(np.floor(0.99 * (db - 0.5) / smin)) + 2
    hi = int(np.floor(0.99 * (da - 0.5) / smax)) - 1
    assert db > 0 and da > 4 * db and lo < hi, (da, db, lo, hi)
    rng = np.random.default_rng(seed)
    w, hh = 1024, 256
    sc = 1 << (dl - 8)
    y = np.round((16 + 219 * 0.53) * sc + rng.integers(-3 * sc, 3 * sc + 1, size=(hh, w)))
    off = rng.integers(lo, hi + 1, size=(2, hh // 2, w // 2)) * rng.choice([-1, 1], size=(2, hh // 2, w // 2))
    cb, cr = 128 * sc + off
    planes = [y, cb, cr]
    if din != dl:           # a full-range source behind the prologue: a raw code that lands on each wanted code
        codes = np.arange(1 << din, dtype=F)
        fy = np.clip(np.floor(F(k.py) * codes + F(k.pyb)), 0, k.pre_max)
        fc = np.clip(np.floor(F(k.pc) * codes + F(k.pcb)), 0, k.pre_max)
        planes = [np.searchsorted(fy, y), np.searchsorted(fc, cb), np.searchsorted(fc, cr)]
        assert np.array_equal(fc[planes[1]], cb) and np.array_equal(fy[planes[0]], y)
    dt = np.uint16 if din > 8 else np.uint8
    return [p.astype(dt) for p in planes], (da, db, lo, hi)


CASES_A = [("yuv420p10le", 10, 10), ("yuv420p", 8, 8), ("yuv420p10le", 10, 8)]


def _kw_a(din, dl):
    return dict(range_src="pc", range_in="tv", lut_depth=dl) if din != dl else {}


def _consts_a(orc, din, dl):
    if din != dl:
        return orc.yuv_constants("bt709", "tv", "bt709", "tv", din, dl, din, 4, prologue=True)
    return orc.yuv_constants(din=din)


def _apply_a(eng, src, fmt, din, dl):
    eng.tile_stats(True)
    got = _run_yuv(eng, src, fmt, din, **_kw_a(din, dl))
    st = eng.tile_stats(False)
    return got, st, eng.last_kernel


@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("fmt,din,dl", CASES_A)
def test_prelut_tube_bound_follows_the_shaper(orc, shapers, order, fmt, din, dl):
    """Two shared shapers with the same toe and end point on one engine (the same slot, so the same host table address):
    the second must get its own tube bound.  A stale bound too large admits pixels whose taps lie outside the staged tube
    (wrong output, A then B); one too small loses tube tiles (B then A).  The tube tile count is compared with an engine
    that only ever saw the second shaper; the first engine stays open so that the second one's table cannot share its
    address."""
    first, second = (shapers["A"], shapers["B"]) if order == "AB" else (shapers["B"], shapers["A"])
    k = _consts_a(orc, din, dl)
    src, bounds = _steep_band_frame(orc, shapers, fmt, din, dl, k, seed=11 + dl)
    want = {name: orc.apply_yuv(s["table"], s["scale"], "tetrahedral", k, din, dl, din, 1, 1, src, prelut=s["pre"])
            for name, s in shapers.items()}
    with LutEngine(0) as e1:
        e1.set_variant("vec_lds")
        e1.set_lut(first["lut"])
        got, _, kern = _apply_a(e1, src, fmt, din, dl)
        assert "k_yuv_tile2" in kern, kern
        _eq(got, want[order[0]], f"{order[0]} first {fmt} dl={dl}")
        e1.set_lut(second["lut"])
        got, st1, kern1 = _apply_a(e1, src, fmt, din, dl)
        assert "k_yuv_tile2" in kern1 and "+tube" in kern1, kern1
        _eq(got, want[order[1]], f"{order[1]} after {order[0]} {fmt} dl={dl} bounds {bounds} stats {st1} {kern1}")
        with LutEngine(0) as e2:
            e2.set_variant("vec_lds")
            e2.set_lut(second["lut"])
            got2, st2, kern2 = _apply_a(e2, src, fmt, din, dl)
            _eq(got2, want[order[1]], f"{order[1]} alone {fmt} dl={dl}")
    assert kern1 == kern2, (kern1, kern2)
    assert (st1["tube_tiles"], st1["mixed_tiles"]) == (st2["tube_tiles"], st2["mixed_tiles"]), (order, bounds, st1, st2)
    if order == "BA" and "+tube" in kern2:
        assert st2["tube_tiles"] + st2["mixed_tiles"] > 0, st2      # A's bound admits this content: the check has teeth


def test_prelut_tube_bound_across_contexts(orc, shapers):
    """A on one engine, closed; B on a fresh one.  Whether the allocator hands the second context the first one's table
    address is not guaranteed (best effort), but the output must equal the oracle either way."""
    fmt, din, dl = CASES_A[0]
    k = _consts_a(orc, din, dl)
    src, _ = _steep_band_frame(orc, shapers, fmt, din, dl, k, seed=21)
    b = shapers["B"]
    want = orc.apply_yuv(b["table"], b["scale"], "tetrahedral", k, din, dl, din, 1, 1, src, prelut=b["pre"])
    for _ in range(2):
        with LutEngine(0) as e1:
            e1.set_variant("vec_lds")
            e1.set_lut(shapers["A"]["lut"])
            _run_yuv(e1, src, fmt, din)
        with LutEngine(0) as e2:
            e2.set_variant("vec_lds")
            e2.set_lut(b["lut"])
            got = _run_yuv(e2, src, fmt, din)
            assert "k_yuv_tile2" in e2.last_kernel, e2.last_kernel
        _eq(got, want, "B on a fresh context after A on a closed one")


# ------------------------------------------------------------------ B. lattice copies follow the lattice
def _twin_yuv(prec, lut, mode, k, din, dl, src):
    """The reference for one fused YUV apply at this precision, from scratch."""
    from oracle import binding as orc
    if prec == "fast":
        return orc.apply_yuv(lut.table, lut.scale, mode, k, din, dl, din, 1, 1, src, fast=True)
    if prec == "fma32":
        return _fma32_twin.apply_yuv(lut.table, lut.scale, mode, k, din, dl, din, 1, 1, src)
    return orc.apply_yuv(lut.table, lut.scale, mode, k, din, dl, din, 1, 1, src, prelut=lut.prelut)


@pytest.mark.parametrize("prec", ["fast", "fma32"])
@pytest.mark.parametrize("fmt,depth", [("yuv420p10le", 10), ("yuv420p", 8)])
def test_lattice_copies_follow_the_lattice(orc, prec, fmt, depth):
    """The fp16 / fp32 pre-multiplied copies and the `unit` flag are derived from the lattice and built lazily per depth.
    A new lattice of the same n (no reallocation), one with a node outside [0, 1], and a precision flipped with a LUT change
    in between must each reach the kernel."""
    k = orc.yuv_constants(din=depth)
    src = frames.make_yuv("natural", 512, 128, depth, 1, 1, k=31)
    l1, l2 = _lut(_unit_lattice(N, 1)), _lut(_unit_lattice(N, 2))
    bad = _unit_lattice(N, 3)
    bad[5, 7, 9, 0] = 1.04                  # one node above 1: not `unit`, so no fast / fma32 kernel
    l3 = _lut(bad)
    tag = "," + prec
    with LutEngine(0) as eng:
        eng.set_precision(prec)
        for step, lut in (("l1", l1), ("l2 same n", l2), ("l1 again", l1)):
            eng.set_lut(lut)
            got = _run_yuv(eng, src, fmt, depth)
            assert tag in eng.last_kernel, (step, eng.last_kernel)
            _eq(got, _twin_yuv(prec, lut, "tetrahedral", k, depth, depth, src), f"{prec} {fmt} {step}")
        eng.set_lut(l3)
        got = _run_yuv(eng, src, fmt, depth)
        assert tag not in eng.last_kernel, eng.last_kernel
        _eq(got, _twin_yuv("strict", l3, "tetrahedral", k, depth, depth, src), f"{prec} {fmt} node outside [0, 1]")
        eng.set_lut(l1)                     # back to unit: the copy must be rebuilt from l1, not the l3 / l2 nodes
        got = _run_yuv(eng, src, fmt, depth, interp="trilinear")
        assert tag in eng.last_kernel, eng.last_kernel
        _eq(got, _twin_yuv(prec, l1, "trilinear", k, depth, depth, src), f"{prec} {fmt} unit again")
        # precision flipped with a LUT change in between
        eng.set_precision("strict")
        got = _run_yuv(eng, src, fmt, depth)
        _eq(got, _twin_yuv("strict", l1, "tetrahedral", k, depth, depth, src), f"{fmt} strict between")
        eng.set_lut(l2)
        eng.set_precision(prec)
        got = _run_yuv(eng, src, fmt, depth)
        assert tag in eng.last_kernel, eng.last_kernel
        _eq(got, _twin_yuv(prec, l2, "tetrahedral", k, depth, depth, src), f"{prec} {fmt} after strict + set_lut")


@pytest.mark.parametrize("prec", ["fast", "fma32"])
def test_lattice_copies_on_a_broadcast_receiver(orc, prec):
    """LutEngineGroup([0, 0], treat_as_remote=True): the second engine receives the lattice by a peer copy.  Its lazily built
    copies must follow each new lattice; its row block is checked against the twin."""
    from lut_renderer_amd.multigpu import LutEngineGroup
    k = orc.yuv_constants(din=10)
    src = frames.make_yuv("natural", 512, 128, 10, 1, 1, k=32)
    l1, l2 = _lut(_unit_lattice(N, 4)), _lut(_unit_lattice(N, 5))
    with LutEngineGroup([0, 0], treat_as_remote=True) as grp:
        grp.set_precision(prec)
        for step, lut in (("l1", l1), ("l2", l2)):
            grp.set_lut(lut)
            got = grp.apply_yuv(_dev(src), pix_fmt="yuv420p10le")
            grp.sync()
            torch.cuda.synchronize()
            assert grp.last_remote == 1 and all("," + prec in name for name in grp.last_kernels), grp.last_kernels
            _eq(_np(got, 10), _twin_yuv(prec, lut, "tetrahedral", k, 10, 10, src), f"group {prec} {step}")


# ------------------------------------------------------------------ C. prelut tables across LUT changes
def test_prelut_tables_across_lut_changes(orc, shapers, tmp_path):
    """shared .csp -> .cube of the same n (the prelut must be gone) -> per-channel .csp (off the tile kernels) -> shared .csp
    again, at both LUT depth slots, through apply_yuv and planar apply_rgb after every step."""
    tab = cube.log709_lattice(N)
    plain = cube.write_cube(tmp_path / "plain.cube", tab)
    per = tmp_path / "per_channel.csp"
    write_csp_with_prelut(per, N, tab, [(XS, SHAPER_A), (XS, SHAPER_B), (XS, XS ** 0.8)])
    steps = [("shared A", shapers["A"]["path"]), ("cube", plain), ("per channel", per), ("shared B", shapers["B"]["path"])]
    with LutEngine(0) as eng:
        eng.set_variant("vec_lds")
        for what, path in steps:
            eng.load_cube(path)
            _, sc, t, pre = orc.parse_lut_file_ex(path)
            assert (pre is None) == (what == "cube")
            for fmt, depth in (("yuv420p10le", 10), ("yuv420p", 8)):
                k = orc.yuv_constants(din=depth)
                src = frames.make_yuv("natural", 256, 64, depth, 1, 1, k=40 + depth)
                got = _run_yuv(eng, src, fmt, depth)
                if what == "per channel":
                    assert "k_yuv_tile2" not in eng.last_kernel, eng.last_kernel
                else:
                    assert "k_yuv_tile2" in eng.last_kernel, eng.last_kernel
                _eq(got, orc.apply_yuv(t, sc, "tetrahedral", k, depth, depth, depth, 1, 1, src, prelut=pre), f"{what} {fmt}")
                rgb = frames.make_rgb("natural", 256, 48, depth, k=50 + depth)
                dst = _sentinel([p.shape for p in rgb], depth)
                eng.apply_rgb(_dev(rgb), dst, depth=depth)
                _eq(_np(dst, depth), orc.apply_rgb(t, sc, depth, "tetrahedral", rgb, prelut=pre), f"{what} gbrp{depth}")


# ------------------------------------------------------------------ D. kernel families interleaved on one context
def _yuv_ref(orc, eng, lut, mode, k, din, dl, dout, src, **kw):
    """The reference for the kernel that just ran: its precision tag picks the twin (fast / fma32 exist only on the fused YUV
    tile kernels; everything else is strict)."""
    name = eng.last_kernel
    if ",fast" in name:
        return orc.apply_yuv(lut.table, lut.scale, mode, k, din, dl, dout, 1, 1, src, fast=True)
    if ",fma32" in name:
        return _fma32_twin.apply_yuv(lut.table, lut.scale, mode, k, din, dl, dout, 1, 1, src)
    return orc.apply_yuv(lut.table, lut.scale, mode, k, din, dl, dout, 1, 1, src, prelut=lut.prelut, **kw)


def test_kernel_families_interleaved(orc, cube_dir):
    """Every family that shares the context's queue and stats words, in a fixed alternating order, twice over, with an
    nframes = 0 call, a row shard and tile_stats toggles in between.  Each output against its reference, no sentinel left."""
    lut = cube.read_cube(cube_dir / "log709_33.cube")
    k10 = orc.yuv_constants(din=10)
    src = frames.make_yuv("natural", 512, 96, 10, 1, 1, k=61)
    rgb = frames.make_rgb("vivid", 384, 64, 10, k=62)
    g, b, r = frames.natural_rgb(256, 48, 8, k=63)
    img = np.stack([r, g, b], axis=-1)
    want_yuv = orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k10, 10, 10, 10, 1, 1, src)
    kd = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 10, 8, 4)
    kloc = _sited_twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 1, 1, "left")
    seen = set()
    with LutEngine(0) as eng:
        eng.set_lut(lut)
        for rnd in range(2):
            tag = f"round {rnd}"
            eng.set_variant("vec_lds")
            eng.tile_stats(True)
            _eq(_run_yuv(eng, src, "yuv420p10le", 10), want_yuv, f"{tag} tile2")
            seen.add(eng.last_kernel.split("<")[0])
            st = eng.tile_stats(rnd == 0)
            assert st["tiles"] > 0, st
            dst = _sentinel([p.shape for p in rgb], 10)
            eng.apply_rgb(_dev(rgb), dst, depth=10)
            seen.add(eng.last_kernel.split("<")[0])
            _eq(_np(dst, 10), orc.apply_rgb(lut.table, lut.scale, 10, "tetrahedral", rgb), f"{tag} planar rgb tube")
            empty = [torch.empty((0,) + p.shape, dtype=torch.int16, device="cuda:0") for p in src]
            eng.apply_yuv(empty, [t.clone() for t in empty], pix_fmt="yuv420p10le")        # nframes = 0: a no-op
            out = torch.full(img.shape, 0xA5, dtype=torch.uint8, device="cuda:0")
            eng.apply_packed(torch.from_numpy(img).cuda(), out, pix_fmt="rgb24")
            seen.add(eng.last_kernel.split("<")[0])
            _eq([out.cpu().numpy()], [orc.apply_packed(lut.table, lut.scale, "rgb24", "tetrahedral", img)], f"{tag} rgb24")
            eng.set_variant("auto")
            dst = _sentinel([p.shape for p in rgb], 10)
            eng.apply_rgb(_dev(rgb), dst, depth=10, interp="trilinear")
            seen.add(eng.last_kernel.split("<")[0])
            _eq(_np(dst, 10), orc.apply_rgb(lut.table, lut.scale, 10, "trilinear", rgb), f"{tag} planar rgb trilinear")
            got = _run_yuv(eng, src, "yuv420p10le", 10, row0=16, rows=48)                    # a row shard into sentinels
            want = [np.full(p.shape, 0xFFFF, np.uint16) for p in src]
            want[0][16:64] = want_yuv[0][16:64]
            want[1][8:32], want[2][8:32] = want_yuv[1][8:32], want_yuv[2][8:32]
            _eq(got, want, f"{tag} row shard")
            dst = _sentinel([p.shape for p in src], 8)
            eng.apply_yuv(_dev(src), dst, pix_fmt="yuv420p10le", out_pix_fmt="yuv420p", dither="error_diffusion")
            seen.add(eng.last_kernel.split("<")[0])
            _eq(_np(dst, 8), orc.apply_yuv(lut.table, lut.scale, "tetrahedral", kd, 10, 10, 8, 1, 1, src,
                                          dither="error_diffusion"), f"{tag} dither")
            got = _run_yuv(eng, src, "yuv420p10le", 10, chroma_loc="left")
            seen.add(eng.last_kernel.split("<")[0])
            _eq(got, _sited_twin.apply_yuv(lut.table, lut.scale, "tetrahedral", kloc, 10, 10, 10, 1, 1, "left", src),
                f"{tag} sited")
            eng.tile_stats(rnd == 1)
            eng.set_variant("generic")
            _eq(_run_yuv(eng, src, "yuv420p10le", 10, interp="trilinear"),
                orc.apply_yuv(lut.table, lut.scale, "trilinear", k10, 10, 10, 10, 1, 1, src), f"{tag} generic")
            seen.add(eng.last_kernel.split("<")[0])
            eng.set_variant("auto")
            sz = (300, 70)
            dst = _sentinel([(70, 300), (35, 150), (35, 150)], 10)
            eng.resize(_dev(src), dst, pix_fmt="yuv420p10le", size=sz)
            _eq(_np(dst, 10), _resize_twin.resize(src, 10, 1, 1, (512, 96), sz), f"{tag} resize")
            eng.tile_stats(False)
    assert {"k_yuv_tile2", "k_yuv_generic"} <= seen and any("sited" in s for s in seen), seen
    assert any(s.startswith("k_rgb_t") for s in seen), seen


def test_resize_tables_past_the_reset(orc):
    """More distinct geometries on one context than the resize table cache keeps (58 axis tables; a 4:2:0 geometry adds 4),
    then the first geometry again: every output against the twin."""
    src = frames.make_yuv("natural", 96, 64, 10, 1, 1, k=71)
    sizes = [(40 + 4 * i, 20 + 2 * i) for i in range(18)]
    with LutEngine(0) as eng:
        for sz in sizes + sizes[:2]:
            got = _np(eng.resize(_dev(src), pix_fmt="yuv420p10le", size=sz), 10)
            _eq(got, _resize_twin.resize(src, 10, 1, 1, (96, 64), sz), f"resize to {sz}")


# ------------------------------------------------------------------ E. a seeded history walk
SIZES = (2, 9, 17, 33, 41, 65)
KINDS = ("cube", "domain", "csp shared", "csp per channel")


def _walk_lut(path, n, kind, rng):
    tab = (cube.log709_lattice(n) if rng.random() < 0.5 else _unit_lattice(n, int(rng.integers(1000)))).astype(F)
    if kind == "cube":
        return cube.write_cube(path.with_suffix(".cube"), tab)
    if kind == "domain":
        return cube.write_cube(path.with_suffix(".cube"), tab, domain_min=(0, 0, 0), domain_max=(1.25, 1.25, 1.25))
    curves = [(XS, SHAPER_A), (XS, SHAPER_B), (XS, XS ** 0.8), (XS, XS + 0.4 * XS * (1.0 - XS))]
    pick = [curves[int(rng.integers(len(curves)))]]
    pick = pick * 3 if kind == "csp shared" else pick + [curves[int(rng.integers(len(curves)))] for _ in range(2)]
    p = path.with_suffix(".csp")
    write_csp_with_prelut(p, n, tab, pick)
    return p


def test_seeded_history_walk(orc, tmp_path):
    """Fifty random state changes and applies on one engine (fixed seed): LUT size and file kind, precision, variant,
    format and depth, chroma_loc and out_size.  Every apply against its reference; a mismatch prints the step log."""
    rng = random.Random(20261016)
    log = []
    with LutEngine(0) as eng:
        ref = None
        for step in range(50):
            act = "lut" if ref is None else rng.choice(("lut", "precision", "variant", "apply", "apply", "apply"))
            if act == "lut":
                n, kind = rng.choice(SIZES), rng.choice(KINDS)
                path = _walk_lut(tmp_path / f"s{step}", n, kind, np.random.default_rng(step))
                eng.load_cube(path)
                _, sc, t, pre = orc.parse_lut_file_ex(path)
                ref = _lut(t, sc, pre)
                log.append(f"{step}: load {kind} n={n} ({path.name})")
                continue
            if act == "precision":
                p = rng.choice(("strict", "fast", "fma32"))
                eng.set_precision(p)
                log.append(f"{step}: precision {p}")
                continue
            if act == "variant":
                v = rng.choice(("auto", "auto", "vec_lds", "vec_global", "generic"))
                eng.set_variant(v)
                log.append(f"{step}: variant {v}")
                continue
            fmt = rng.choice(("yuv420p10le", "yuv420p", "yuv444p10le", "gbrp10", "rgb24"))
            mode = rng.choice(("tetrahedral", "trilinear"))
            w, h = rng.choice(((256, 64), (384, 48), (1024, 32)))
            if fmt == "gbrp10":
                src = frames.make_rgb("natural", w, h, 10, k=step)
                dst = _sentinel([p.shape for p in src], 10)
                eng.apply_rgb(_dev(src), dst, depth=10, interp=mode)
                log.append(f"{step}: apply {fmt} {w}x{h} {mode} -> {eng.last_kernel}")
                _eq(_np(dst, 10), orc.apply_rgb(ref.table, ref.scale, 10, mode, src, prelut=ref.prelut), f"step {step}", log)
                continue
            if fmt == "rgb24":
                g, b, r = frames.natural_rgb(w, h, 8, k=step)
                img = np.stack([r, g, b], axis=-1)
                if ref.prelut is not None:          # (the oracle's packed entry takes no prelut: planar at 8 bit is the same)
                    continue
                out = torch.full(img.shape, 0xA5, dtype=torch.uint8, device="cuda:0")
                eng.apply_packed(torch.from_numpy(img).cuda(), out, pix_fmt=fmt, interp=mode)
                log.append(f"{step}: apply {fmt} {w}x{h} {mode} -> {eng.last_kernel}")
                _eq([out.cpu().numpy()], [orc.apply_packed(ref.table, ref.scale, fmt, mode, img)], f"step {step}", log)
                continue
            depth = 8 if fmt == "yuv420p" else 10
            cs = (0, 0) if "444" in fmt else (1, 1)
            src = frames.make_yuv(rng.choice(("natural", "vivid", "noise16")), w, h, depth, cs[0], cs[1], k=step)
            loc = rng.choice((None, None, "left", "topleft")) if cs == (1, 1) else None
            size = rng.choice((None, None, (w // 2 + 6, h + 10))) if eng.precision == "strict" and cs == (1, 1) else None
            kw = dict(interp=mode, chroma_loc=loc)
            if size is None:
                got = _run_yuv(eng, src, fmt, depth, **kw)
            else:
                dst = _sentinel([(size[1], size[0]), (size[1] // 2, size[0] // 2), (size[1] // 2, size[0] // 2)], depth)
                eng.apply_yuv(_dev(src), dst, pix_fmt=fmt, out_size=size, **kw)
                got = _np(dst, depth)
            log.append(f"{step}: apply {fmt} {w}x{h} {mode} loc={loc} out_size={size} -> {eng.last_kernel}")
            if loc is not None:
                k = _sited_twin.consts("bt709", "tv", "bt709", "tv", depth, depth, depth, 1, 1, loc)
                want = _sited_twin.apply_yuv(ref.table, ref.scale, mode, k, depth, depth, depth, 1, 1, loc, src, prelut=ref.prelut)
            elif size is not None:
                k = orc.yuv_constants(din=depth, chroma_n=4)
                want = orc.apply_yuv(ref.table, ref.scale, mode, k, depth, depth, depth, 1, 1, src, prelut=ref.prelut)
            else:
                k = orc.yuv_constants(din=depth, chroma_n=1 << sum(cs))
                want = _yuv_ref(orc, eng, ref, mode, k, depth, depth, depth, src) if cs == (1, 1) else \
                    _yuv_ref444(orc, eng, ref, mode, k, depth, src)
            if size is not None:
                want = _resize_twin.resize(want, depth, 1, 1, (w, h), size, chroma_loc=loc)
            _eq(got, want, f"step {step}", log)


def _yuv_ref444(orc, eng, lut, mode, k, depth, src):
    name = eng.last_kernel
    if ",fast" in name:
        return orc.apply_yuv(lut.table, lut.scale, mode, k, depth, depth, depth, 0, 0, src, fast=True)
    if ",fma32" in name:
        return _fma32_twin.apply_yuv(lut.table, lut.scale, mode, k, depth, depth, depth, 0, 0, src)
    return orc.apply_yuv(lut.table, lut.scale, mode, k, depth, depth, depth, 0, 0, src, prelut=lut.prelut)


# ------------------------------------------------------------------ F. apply_lut on a kept engine
def test_apply_lut_on_kept_engines(orc, cube_dir, tmp_path):
    """Two LUT files alternated through the cached engine; one path rewritten with new contents (its cache key moves with
    the mtime); a direct set_lut between two apply_lut(engine=eng) calls with the same cube object."""
    from lut_renderer_amd import api
    src = frames.make_yuv("natural", 256, 64, 10, 1, 1, k=91)
    k = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 10, 10, 4)
    dev = _dev(src)
    call = dict(pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv")

    def want(lut):
        return orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, src, prelut=lut.prelut)

    names = ("log709_33.cube", "random_9.cube")
    wants = {nm: want(cube.read_cube(cube_dir / nm)) for nm in names}
    try:
        for nm in names + names:
            out, _ = api.apply_lut(dev, cube=cube_dir / nm, **call)
            _eq(_np(out, 10), wants[nm], f"apply_lut {nm}")
        p = tmp_path / "rewritten.cube"
        for i, tab in enumerate((cube.log709_lattice(17), _unit_lattice(17, 9))):
            cube.write_cube(p, tab)
            os.utime(p, (1_700_000_000 + i, 1_700_000_000 + i))
            out, _ = api.apply_lut(dev, cube=p, **call)
            _eq(_np(out, 10), want(cube.read_cube(p)), f"rewritten path, version {i}")
        with LutEngine(0) as eng:
            a, b = cube.read_cube(cube_dir / names[0]), cube.read_cube(cube_dir / names[1])
            for _ in range(2):
                out, _ = api.apply_lut(dev, cube=a, engine=eng, **call)
                eng.sync()
                _eq(_np(out, 10), wants[names[0]], "apply_lut(engine=eng)")
                eng.set_lut(b)
    finally:
        api.close_cached_engines()
