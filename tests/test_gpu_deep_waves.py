"""The persistent tile loops many tiles deep, on small frames.

The three persistent-grid kernel families (lutr_tile2.hip, lutr_rgb2.hip, lutr_tile.hip) carry state from one tile to the next
inside a wave -- the window and its raw box, `l2run` and its re-box, the one-tile-ahead pipeline, every `claim_chunk` after the
first with its LDS ticket and 8-deep ring, the reset of the queue words -- and the frames the other GPU tests use give each wave
one chunk of one or two tiles.  Here a child process (tests/_gpu_capped_worker.py) runs with LUTR_MAX_WAVES=16 (one workgroup
of the YUV and tube kernels), a second one with 32 (two): 1600 tiles then put a launch where the headline's 2 M tiles put it --
about 100 tiles and 25 claims per wave, the full-width tube, 4096-pixel chunks.

Every case is a test of its own: the reference is recomputed from scratch in this process (the oracle for strict and fast,
tests/_fma32_twin.py for fma32) and every plane is compared bit for bit; the child's LUTR_DEBUG line proves the regime (blocks,
chunk height, tube width), its counters the depth and the paths the content was built to reach, `last_kernel` the kernel.
The content's own properties are checked on the CPU (the unmarked tests below).

Found by these cases: `y-ramp-fast` differed from the oracle by one code at 65 samples, with and without the cap -- not the tile
loop, but k_make_lat16 (lutr_lat16.hip) rounding `node * M` to fp16 once where the CPU twin rounds twice; and DESIGN.md 5.2 gave
windows of 139 / 367 nodes where the launcher leaves 134 / 366.  No YUV launch reaches lutr_tile.hip any more (its k_yuv_tile is
gone): that family is covered through k_rgb_tile."""
import json
import os
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native
from tests import _deep_content as dc
from tests import _fma32_twin

F = np.float32
ROOT = Path(__file__).resolve().parent.parent
WORKER = ROOT / "tests" / "_gpu_capped_worker.py"
# waves per workgroup of the three launchers (LUTR_T2_WPB, LUTR_R2_WPB, LUTR_WPB)
WPB = {"t2": 16, "r2": 16, "t1": 8}
# The limit of a child: torch import and GPU start-up (a few seconds, tens on a cold machine), the content of its cases (up to 0.3 s
# each on the CPU), one code-object load per kernel, launches of a few ms.  Measured: 6 s and 2.5 s.  A limit, not a measurement.
CHILD_LIMIT_S = {16: 120, 32: 60}


# ================================================================== content, on the CPU
def _tube_verdict(k, cb, cr, h_cells=7, n=33, depth=10):
    """Per chroma sample: outside the grey tube's bound, on chroma alone, as test_ramp_frame_straddles_the_tube states it --
    |gv - rv| and |bu - gv| (RGB codes) against (H + 1) / kappa, kappa = lattice cells per code, H = 7."""
    cbd, crd = cb.astype(F) - F(k.coff), cr.astype(F) - F(k.coff)
    rv, gv, bu = F(k.krv) * crd, F(k.kgu) * cbd + F(k.kgv) * crd, F(k.kbu) * cbd
    worst = np.maximum(np.abs(gv - rv), np.abs(bu - gv))
    return worst > (h_cells + 1) / ((n - 1) / float((1 << depth) - 1))


def _per_tile(a, th, tw):
    """[H, W] -> [H / th, W / tw, th * tw]: the samples of every tile."""
    h, w = a.shape
    return a.reshape(h // th, th, w // tw, tw).transpose(0, 2, 1, 3).reshape(h // th, w // tw, th * tw)


BASE = (1536, 1088)       # 12 x 136 tiles of 128 x 8 px = 64 x 4 chroma samples at 10-bit 4:2:0


def _outside_per_tile(orc, name, seed):
    k = orc.yuv_constants(din=10)
    src = dc.yuv_content(name, *BASE, 10, 1, 1, seed)
    return _per_tile(_tube_verdict(k, src[1], src[2]), 4, 64).sum(axis=2), src


def test_generators_are_seeded():
    for name in ("natural", "noise16", "vivid", "uniform", "ramp", "quadrants"):
        a, b, c = (dc.yuv_content(name, 256, 64, 10, 1, 1, s) for s in (3, 3, 4))
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), name
        assert not all(np.array_equal(x, y) for x, y in zip(a, c)), name


def test_quadrants_frame_lies_wholly_outside_the_tube_and_its_boxes_fail(orc):
    """Every 128 x 8 tile of the case's frame has all its chroma outside the tube's bound (no tube tile, no mixed tile), its
    chroma is flat (the cells of a window hold from tile to tile) and its luma spans more than three lattice cells of 32 codes
    (sigma-60 noise, clipped at the range's ends: a raw box fails)."""
    out, src = _outside_per_tile(orc, "quadrants", dc.BY_ID["y-quadrants"]["seed"])
    assert out.shape == (136, 12) and (out == 256).all(), out
    for p in src[1:]:
        t = _per_tile(p.astype(np.int64), 4, 64)
        assert (t.max(axis=2) == t.min(axis=2)).all()
    y = _per_tile(src[0].astype(np.int64), 8, 128)
    assert ((y.max(axis=2) - y.min(axis=2)) > 100).all()


def _sheared_nodes(k, src, depth, csx, csy, n, th, tw):
    """Per tile: the nodes it touches in the window's sheared coordinates (r, g - r, b - r) -- the box of its pixels' cells, one
    node more per axis."""
    top = (1 << depth) - 1
    r, g, b = (np.clip(c, 0, top) * (n - 1) // top for c in _fma32_twin.yuv_to_rgb_codes(k, csx, csy, src))
    nodes = 1
    for axis in (r, g - r, b - r):
        t = _per_tile(axis, th, tw)
        nodes = nodes * (t.max(axis=2) - t.min(axis=2) + 2)
    return nodes


def test_vivid_frames_have_tiles_for_the_windows(orc):
    """What the `vivid` cases assert on the GPU -- windows staged, and tiles served by a window an earlier tile of the same wave
    staged -- needs tiles wholly outside the tube (one lane inside makes a tile a mixed one) whose cells fit a window, one below
    the other (a chunk walks down a strip).  Every `vivid` case with a tube and no prologue, in its own layout, shape, tile shape
    and seed: a fair share of tiles wholly outside, tube tiles too, and vertical pairs of tiles that fit the smallest window any
    kernel has here (134 nodes)."""
    seen = 0
    for case in dc.CASES:
        if case["content"] != "vivid" or not _has_tube(case) or case["full_range"]:
            continue
        depth, csx, csy = dc.YUV_FMT[case["fmt"]]
        n = int(case["lut"][1:]) if case["lut"] in ("u33", "u25") else 33
        k = orc.yuv_constants("bt709", "tv", "bt709", "tv", depth, depth, depth, 1 << (csx + csy))
        src = dc.make_source(case)
        if case["shard"]:
            r0, rows = case["shard"]
            src = [src[0][r0:r0 + rows], src[1][r0 >> csy:(r0 + rows) >> csy], src[2][r0 >> csy:(r0 + rows) >> csy]]
        tiles, px = _tile_geom(case)
        tw = {1024: 128, 2048: 256, 512: 256}[px] if not case["id"].endswith("-edge") else 64
        th = px // tw
        h, w = src[0].shape[0] // th * th, src[0].shape[1] // tw * tw            # (whole tiles only)
        src = [src[0][:h, :w], src[1][:h >> csy, :w >> csx], src[2][:h >> csy, :w >> csx]]
        out = _per_tile(_tube_verdict(k, src[1], src[2], n=n, depth=depth), th >> csy, tw >> csx)
        whole = out.sum(axis=2) == out.shape[2]
        inside = out.sum(axis=2) == 0
        fits = whole & (_sheared_nodes(k, src, depth, csx, csy, n, th, tw) <= 134)
        pairs = int((fits[1:] & fits[:-1]).sum())
        assert whole.mean() > 0.05 and inside.mean() > 0.1 and pairs > 10, (case["id"], whole.mean(), inside.mean(), pairs)
        seen += 1
    assert seen >= 12, seen


def test_natural_frame_lies_mostly_inside_the_tube(orc):
    out, _ = _outside_per_tile(orc, "natural", dc.BY_ID["y-natural"]["seed"])
    assert (out == 0).mean() > 0.75, (out == 0).mean()


def test_ramp_and_noise16_frames_have_mixed_tiles(orc):
    for name in ("ramp", "noise16"):
        out, _ = _outside_per_tile(orc, name, dc.BY_ID[f"y-{name}"]["seed"])
        assert ((out > 0) & (out < 256)).mean() > 0.1, (name, ((out > 0) & (out < 256)).mean())


def test_uniform_frame_has_no_tile_that_fits_a_window(orc):
    """No tile of the uniform frame comes near the nodes of a strict window, nor the 755 of the largest
    window a kernel without a tube has at 33^3: all go to the gather body."""
    k = orc.yuv_constants(din=10)
    src = dc.yuv_content("uniform", *BASE, 10, 1, 1, dc.BY_ID["y-uniform"]["seed"])
    nodes = _sheared_nodes(k, src, 10, 1, 1, 33, 8, 128)
    assert nodes.shape == (136, 12) and nodes.min() > 755, nodes.min()


def test_every_case_reaches_the_long_launch_thresholds():
    """The launcher's own rule: at least 100 x cap tiles (the tube at full width; 64 x cap for the 4096-pixel chunks)."""
    for case in dc.CASES:
        tiles = _tiles(case)
        assert tiles >= 100 * case["cap"], (case["id"], tiles)
        assert tiles < 130 * case["cap"], (case["id"], tiles)           # ... and the smallest shapes that do


# ================================================================== the knob's validation rule, on the CPU
def test_max_waves_knob_validation():
    """The function the three launchers judge LUTR_MAX_WAVES with (capped_waves, lutr_launch.h), through the C ABI."""
    knob = _native.max_waves_knob
    for wpb in (8, 16):
        full = 256 * 16
        assert knob(None, wpb, full) == full                                            # unset
        for ok in (wpb, 2 * wpb, 32 * wpb, full):
            assert knob(str(ok), wpb, full) == ok
        for bad in ("0", "-16", "-0", str(wpb - 1), str(wpb + 1), str(3 * wpb // 2), str(full + wpb), str(full + 1), "99999999999999999999",
                    "", " 16", "16 ", "+16", "16x", "x16", "1e2", "0x10", "16.0", "sixteen"):
            assert knob(bad, wpb, full) == full, (bad, wpb)
    assert knob("16", 16, 8) == 8 and knob("8", 8, 8) == 8                               # never above the real maximum
    assert knob("24", 8, 4096) == 24 and knob("24", 16, 4096) == 4096                    # a multiple of THIS launcher's workgroup


# ================================================================== geometry the cases are expected to get
def _tile_geom(case):
    """(tiles, pixels per tile) as the launchers lay the frame out (lane shapes: DESIGN.md 5.2 / lutr_rgb2.hip / lutr_tile.hip)."""
    w, h = case["w"], case["shard"][1] if case["shard"] else case["h"]
    nf = len(case["content"]) if isinstance(case["content"], tuple) else 1
    if case["family"] == "t2":
        depth, csx, csy = dc.YUV_FMT[case["fmt"]]
        pxt = 8 if depth > 8 else 16
        lw, lh = (16, 4) if csy else (32, 2)
        if case["id"].endswith("-edge"):            # 193 x 546 units: 8 x 8 lanes waste 2 % fewer of them than 16 x 4
            lw, lh = 8, 8
        tw, th = lw * pxt, lh << csy
    elif case["family"] == "r2":
        px, wide = {"gbrp10le": (8, 1), "rgb24": (16, 0), "bgr48le": (8, 1)}[case["fmt"]]
        lw, lh = (32, 2) if wide else (8, 8)
        tw, th = lw * px, lh
    else:                                           # k_rgb_tile: 64 lanes of 8 px along one row wherever that wastes none
        lw, lh = 64, 1
        tw, th = lw * 8, lh
    return nf * -(-w // tw) * -(-h // th), 64 * (tw // lw) * (th // lh)


def _tiles(case):
    return _tile_geom(case)[0]


def _long_chunk(case):
    """Tiles per claimed chunk of a long launch: 4096 pixels; round 1's kernel: 16 tile rows."""
    return 16 if case["family"] == "t1" else -(-4096 // _tile_geom(case)[1])


def _has_tube(case):
    return case["family"] == "t2" and case["mode"] != "nearest" and case["lut"] in ("u33", "u25", "wide33", "shaper")


def _tube_h(case):
    """The tube width DESIGN.md 5.2 states for a long launch, where it states one: 7 cells strict (12-byte nodes; fma32 shares
    them), 8 fast at 33^3 -- the same rule, 8 (N - 1) / 32 cells rounded, gives 6 at 25^3, which fits both budgets."""
    if not _has_tube(case) or case["mode"] != "tetrahedral":
        return None
    if case["lut"] == "u25":
        return 6
    return 8 if case["prec"] == "fast" else 7


# ================================================================== the children
def _run_child(cap, out_dir):
    ids = [c["id"] for c in dc.CASES if c["cap"] == cap]
    env = dict(os.environ, LUTR_MAX_WAVES=str(cap), LUTR_DEBUG="1")
    t0 = time.monotonic()
    try:
        p = subprocess.run([sys.executable, str(WORKER), str(out_dir)] + ids, env=env, cwd=str(ROOT), capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S[cap])
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode("utf-8", "replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"the LUTR_MAX_WAVES={cap} child did not finish within {CHILD_LIMIT_S[cap]} s; its last lines:\n{err[-3000:]}",
                    pytrace=False)
    wall = time.monotonic() - t0
    print(f"LUTR_MAX_WAVES={cap} child: {len(ids)} cases, exit {p.returncode}, wall {wall:.1f} s")
    if p.returncode != 0:
        pytest.fail(f"the LUTR_MAX_WAVES={cap} child ended with {p.returncode} after {wall:.1f} s; its last lines:\n{p.stderr[-3000:]}",
                    pytrace=False)
    debug, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"\[case (\S+)\]", line)
        if m:
            cur = m.group(1)
            debug[cur] = []
        elif cur and re.match(r"\[lutr (t2|r2|t1)\]", line):
            debug[cur].append(line)
    results = {}
    for cid in ids:
        with np.load(out_dir / f"{cid}.npz") as z:
            results[cid] = dict(planes=[z[f"p{i}"] for i in range(len(z.files) - 2)], stats=json.loads(str(z["stats"])),
                                kernel=str(z["kernel"]), debug=debug.get(cid, []), wall=wall)
    return results


@pytest.fixture(scope="module")
def capped(tmp_path_factory):
    """Both children's results by case id.  The second child starts only if the first exited 0; a non-zero exit, a death by
    signal or the time limit fails this fixture for every case, and nothing is started after it -- no retry, and no case is
    lifted into this process."""
    out_dir = tmp_path_factory.mktemp("deep")
    results = _run_child(16, out_dir)
    results.update(_run_child(32, out_dir))
    return results


# ================================================================== references, from scratch
def _first_diff(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: plane {i} {a.shape} {a.dtype} != {b.shape} {b.dtype}"
        if not np.array_equal(a, b):
            diff = np.abs(a.astype(np.int64) - b.astype(np.int64))
            bad = np.argwhere(diff > 0)
            raise AssertionError(f"{what}: plane {i} differs at {len(bad)} samples, max |d|={diff.max()}, "
                                 f"first {bad[0].tolist()} got {a[tuple(bad[0])]} want {b[tuple(bad[0])]}")


def _sentinel_like(shape, depth):
    return np.full(shape, 0xFFFF, np.uint16) if depth > 8 else np.full(shape, 0xA5, np.uint8)


def _reference(orc, case, tmp_dir):
    """What the case's destination planes must hold, sentinel included."""
    lut, path = dc.make_lut(case["lut"], tmp_dir)
    table, scale, prelut = lut.table, lut.scale, None
    if path is not None:                            # a file: the oracle's own parser reads it
        _, scale, table, prelut = orc.parse_lut_file_ex(path)
    src = dc.make_source(case)
    mode = case["mode"]
    if case["api"] == "rgb":
        return list(orc.apply_rgb(table, scale, 10, mode, src))
    if case["api"] == "packed":
        return [orc.apply_packed(table, scale, case["fmt"], mode, src)]
    din, csx, csy = dc.YUV_FMT[case["fmt"]]
    dout = dc.YUV_FMT[case["ofmt"] or case["fmt"]][0]
    dl = case["kw"].get("lut_depth", din)
    k = orc.yuv_constants("bt709", "tv", "bt709", "tv", din, dl, dout, 1 << (csx + csy), prologue="range_src" in case["kw"])

    def one(planes):
        if case["prec"] == "fma32":
            return _fma32_twin.apply_yuv(table, scale, mode, k, din, dl, dout, csx, csy, planes)
        return orc.apply_yuv(table, scale, mode, k, din, dl, dout, csx, csy, planes, fast=case["prec"] == "fast", prelut=prelut)

    if src[0].ndim == 3:                            # a batch on frame strides with a spare row, which keeps the sentinel
        want = [_sentinel_like((p.shape[0], p.shape[1] + 1, p.shape[2]), dout) for p in src]
        for f in range(src[0].shape[0]):
            for dst, plane in zip(want, one([p[f] for p in src])):
                dst[f, :-1] = plane
        return want
    full = one(src)
    if case["shard"]:
        r0, rows = case["shard"]
        want = [_sentinel_like(p.shape, dout) for p in full]
        want[0][r0:r0 + rows] = full[0][r0:r0 + rows]
        for c in (1, 2):
            want[c][r0 >> csy:(r0 + rows) >> csy] = full[c][r0 >> csy:(r0 + rows) >> csy]
        return want
    return list(full)


# ================================================================== the claims of a case
def _field(line, key):
    m = re.search(rf"\b{re.escape(key)} (-?\d+(?:\.\d+)?)", line)
    assert m, (key, line)
    return float(m.group(1)) if "." in m.group(1) else int(m.group(1))


def _check_regime(case, res):
    assert len(res["debug"]) == 1, res["debug"]
    line = res["debug"][0]
    assert line.startswith(f"[lutr {case['family']}]"), line
    assert _field(line, "blocks") == case["cap"] // WPB[case["family"]], line
    assert _field(line, "chunk") == _long_chunk(case), (line, _long_chunk(case))
    h = _field(line, "tube h")
    want_h = _tube_h(case)
    if want_h is not None:
        assert h == want_h, (line, want_h)
        assert _field(line, "t") > 0 and _field(line, "plane") >= (2 * h + 3) ** 2, line
        if case["lut"] == "u33" and case["fmt"] == "yuv420p10le" and not case["kw"]:      # the window DESIGN.md 5.2 states beside it
            assert _field(line, "win_nodes") == (366 if case["prec"] == "fast" else 134), line
    elif _has_tube(case):
        assert h >= 3, line
    elif case["family"] == "t2":
        assert h == 0, line


def _check_names(case, kern):
    if case["family"] == "r2":
        assert kern.startswith("k_rgb_tube<ly%d," % {"gbrp10le": 1, "rgb24": 2, "bgr48le": 3}[case["fmt"]]), kern
        assert ("," + {"tetrahedral": "2", "trilinear": "1"}[case["mode"]]) in kern and kern.endswith("+tube"), kern
        return
    if case["family"] == "t1":
        assert kern.startswith("k_rgb_tile<1,1"), kern
        return
    assert "k_yuv_tile2" in kern, kern
    assert ("+tube" in kern) == _has_tube(case), kern
    assert ("+whole-lattice" in kern) == (case["lut"] == "u17"), kern
    assert (",fast" in kern) == (case["prec"] == "fast"), kern
    assert (",fma32" in kern) == (case["prec"] == "fma32" and case["mode"] != "nearest"), kern
    assert (",pre," in kern) == ("range_src" in case["kw"]), kern
    assert (",tab" in kern) == (case["lut"] != "domains"), kern
    assert (",unit" in kern) == (case["lut"] not in ("domains", "wide33")), kern


def _check_paths(case, st):
    """Only `> 0`: with a dynamic queue the exact counts vary from run to run."""
    assert st["tiles"] >= 100 * case["cap"], st
    content = case["content"]
    if case["family"] == "r2":
        assert st["tube_tiles"] + st["global_tiles"] == st["tiles"], st
        if content == "natural":
            assert st["tube_tiles"] > st["tiles"] // 2, st
        else:
            assert st["global_tiles"] > 0, st
        return
    if case["family"] == "t1":
        if content == "uniform":
            assert st["global_tiles"] > 0, st
        else:
            assert st["staged"] > 0 and st["tiles"] - st["misses"] > 0, st
        return
    if case["lut"] == "u17":
        assert st["global_tiles"] == st["misses"] == st["staged"] == 0, st
        return
    reused = st["tiles"] - st["tube_tiles"] - st["mixed_tiles"] - st["level2_tiles"]
    mixed_on = _has_tube(case) and case["prec"] != "fast"
    if not mixed_on:
        assert st["mixed_tiles"] == 0, st
    if not _has_tube(case):
        assert st["tube_tiles"] == 0, st
    if content == "natural":
        if _has_tube(case):
            assert st["tube_tiles"] > st["tiles"] // 2, st
        else:
            assert st["staged"] > 0 and reused > 0, st
    if content in ("ramp", "noise16") and mixed_on:
        assert st["mixed_tiles"] > 0, st
    if content == "vivid":
        # a tile served by a window that an earlier tile of the same wave staged
        assert st["staged"] > 0 and reused > 0, st
    if content == "quadrants":
        assert st["level2_tiles"] - st["misses"] > 0, st
    if content == "uniform":
        assert st["global_tiles"] > 0, st


# ================================================================== one test per case
@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c["id"] for c in dc.CASES])
def test_deep_case(orc, capped, tmp_path, cid):
    case, res = dc.BY_ID[cid], capped[cid]
    print(f"{cid}: {res['kernel']} {res['stats']}\n{res['debug']}\nchild wall {res['wall']:.1f} s")
    _check_regime(case, res)
    _check_names(case, res["kernel"])
    _check_paths(case, res["stats"])
    _first_diff(res["planes"], _reference(orc, case, tmp_path), cid)


@pytest.mark.gpu
def test_two_workgroups_leave_the_queue_as_they_found_it(capped):
    """ramp, vivid, ramp on one engine under two workgroups: the global atomic between them, and the last workgroup's reset of
    the queue words -- the third launch starts from what the second left, and must give the first one's planes."""
    a, c = capped["y32-a-ramp"], capped["y32-c-ramp"]
    _first_diff(c["planes"], a["planes"], "third launch against the first")
    assert a["kernel"] == c["kernel"] and a["stats"]["tiles"] == c["stats"]["tiles"], (a["stats"], c["stats"])


@pytest.mark.gpu
def test_knob_unset_changes_nothing_in_this_process(orc):
    """This process has no cap: the mixed-patch suite's core shape gets the kernel, the launch and the planes it gets there."""
    import torch
    from lut_renderer_amd.engine import LutEngine
    assert "LUTR_MAX_WAVES" not in os.environ
    lut, _ = dc.make_lut("u33", None)
    src = dc.ramp_yuv(512, 136, 10, 1, 1, seed=3)
    with LutEngine(0) as eng:
        eng.set_variant("vec_lds")
        eng.set_lut(lut)
        dst = [torch.full(p.shape, -1, dtype=torch.int16, device="cuda:0") for p in src]
        eng.tile_stats(True)
        eng.apply_yuv([torch.from_numpy(p.view(np.int16)).to("cuda:0") for p in src], dst, pix_fmt="yuv420p10le")
        st = eng.tile_stats(False)
        kern = eng.last_kernel
    assert kern == "k_yuv_tile2<11,11,2,tab,unit>+tube", kern
    assert st["tiles"] == 4 * 17 and st["mixed_tiles"] > 0, st
    k = orc.yuv_constants(din=10)
    _first_diff([t.cpu().numpy().view(np.uint16) for t in dst],
                orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, src), "knob unset")
