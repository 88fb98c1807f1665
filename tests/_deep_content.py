"""Seeded content, lattices and the case list shared by tests/_gpu_capped_worker.py (a child process that applies on the GPU and
computes no reference) and tests/test_gpu_deep_waves.py (the parent, which recomputes every reference from scratch) -- TEST
INFRASTRUCTURE ONLY.  Plain numpy: nothing here touches torch or the GPU.  tests/test_gpu_mixed_patch.py takes `ramp_yuv` from here."""
from __future__ import annotations

import numpy as np

from lut_renderer_amd import cube, frames
from tests._csp_files import write_csp_with_prelut

F = np.float32


# ------------------------------------------------------------------ content
def ramp_yuv(w, h, depth, csx, csy, seed, full_range=False):
    """Natural luma; Cb runs linearly from mid - 160 to mid + 160 codes (10-bit scale) across the width, Cr the same down the
    height; Gaussian noise of sigma 6 (10-bit scale) on every chroma sample.  Seeded."""
    rng = np.random.default_rng(770000 + seed)
    s = float(1 << depth) / 1024.0
    mid = float(1 << (depth - 1))
    ch, cw = frames.chroma_shape(w, h, csx, csy)
    y = frames.natural_yuv(w, h, depth, csx, csy, k=seed, full_range=full_range)[0]
    cb = mid + s * np.linspace(-160.0, 160.0, cw)[None, :] + rng.normal(0.0, 6.0 * s, size=(ch, cw))
    cr = mid + s * np.linspace(-160.0, 160.0, ch)[:, None] + rng.normal(0.0, 6.0 * s, size=(ch, cw))
    top = (1 << depth) - 1
    dt = np.uint16 if depth > 8 else np.uint8
    return [y, np.clip(np.rint(cb), 1, top - 1).astype(dt), np.clip(np.rint(cr), 1, top - 1).astype(dt)]


def quadrants_yuv(w, h, depth, csx, csy, seed):
    """The saturated frame of test_grey_tube_serves_low_saturation_tiles...: a luma ramp across the width under sigma-60 noise
    (10-bit scale), chroma at mid +- 300 codes in four flat fields (Cb changes sign at half the width, Cr at half the height).  Raw boxes fail on
    the luma noise while the cells of a window hold.  Seeded."""
    rng = np.random.default_rng(880000 + seed)
    s = float(1 << depth) / 1024.0
    mid = 1 << (depth - 1)
    ch, cw = frames.chroma_shape(w, h, csx, csy)
    dt = np.uint16 if depth > 8 else np.uint8
    y = np.clip(np.linspace(64 * s, 940 * s, w)[None, :] + rng.normal(0, 60 * s, size=(h, w)), 64 * s, 940 * s).astype(dt)
    cb = np.full((ch, cw), mid, np.int32)
    cr = cb.copy()
    d = int(300 * s)
    cb[:, : cw // 2] += d; cb[:, cw // 2:] -= d
    cr[: ch // 2, :] += d; cr[ch // 2:, :] -= d
    return [y, cb.astype(dt), cr.astype(dt)]


def yuv_content(name, w, h, depth, csx, csy, seed, full_range=False):
    if name == "ramp":
        return ramp_yuv(w, h, depth, csx, csy, seed, full_range)
    if name == "quadrants":
        return quadrants_yuv(w, h, depth, csx, csy, seed)
    return frames.make_yuv(name, w, h, depth, csx, csy, k=seed, full_range=full_range)


# ------------------------------------------------------------------ lattices
def unit_lattice(n, seed):
    """Every node in [0, 1] (the clip-free and fma32 kernels apply) and no two nodes alike: a wrong tap shows."""
    t = 0.6 * cube.log709_lattice(n) + 0.4 * cube.identity_lattice(n)
    rng = np.random.default_rng(4200 + seed)
    return np.clip(t + rng.uniform(-0.02, 0.02, size=t.shape), 0.0, 1.0).astype(F)


def make_lut(name, tmp_dir):
    """The LUT of a case as the engine takes it (a CubeLut).  "shaper" and "domains" go through a file in `tmp_dir`, which the
    parent hands to the oracle's own parser: (CubeLut, path or None)."""
    one = np.ones(3, dtype=F)
    if name in ("u33", "u25", "u17"):
        n = int(name[1:])
        return cube.CubeLut(n=n, table=unit_lattice(n, n), scale=one), None
    if name == "log65":
        return cube.CubeLut(n=65, table=np.ascontiguousarray(cube.log709_lattice(65), dtype=F), scale=one), None
    if name == "wide33":            # nodes outside [0, 1]: the output clip stays live (kernel ",tab" without ",unit")
        t = (1.3 * unit_lattice(33, 33).astype(np.float64) - 0.15).astype(F)
        return cube.CubeLut(n=33, table=t, scale=one), None
    if name == "shaper":            # the mild shared .csp shaper of test_mixed_tiles_shared_shaper
        xs = np.linspace(0.0, 1.0, 33)
        p = tmp_dir / "mild.csp"
        write_csp_with_prelut(p, 33, unit_lattice(33, 9), [(xs, xs + 0.4 * xs * (1.0 - xs))] * 3)
        return cube.read_lut(p), p
    if name == "domains":           # DOMAIN_MAX differs per channel: three scales, no shared coordinate table
        p = tmp_dir / "domains.cube"
        cube.write_cube(p, unit_lattice(33, 7), domain_min=(0.0, 0.0, 0.0), domain_max=(1.0, 1.25, 1.5))
        return cube.read_cube(p), p
    raise ValueError(name)


# ------------------------------------------------------------------ cases
# fmt: the source format; ofmt: the output format where it differs; (w, h): the frame (of each frame of a batch; of the whole
# frame of a row shard); content: a generator's name, or a tuple of names = one frame each of a batch; kw: extra keywords of the
# apply call; family: which launcher's LUTR_DEBUG line the case expects (t2 = lutr_tile2.hip, r2 = lutr_rgb2.hip, t1 = lutr_tile.hip).
YUV_FMT = {"yuv420p10le": (10, 1, 1), "yuv420p": (8, 1, 1), "yuv422p10le": (10, 1, 0), "yuv444p10le": (10, 0, 0)}


def _c(cid, cap, family, api, fmt, w, h, content, seed, mode="tetrahedral", prec="strict", lut="u33", ofmt=None, kw=None,
       shard=None, env=None, full_range=False):
    return dict(id=cid, cap=cap, family=family, api=api, fmt=fmt, w=w, h=h, content=content, seed=seed, mode=mode, prec=prec,
                lut=lut, ofmt=ofmt, kw=kw or {}, shard=shard, env=env or {}, full_range=full_range)


def _cases():
    out = []
    base = ("yuv420p10le", 1536, 1088)
    for i, name in enumerate(("natural", "noise16", "vivid", "uniform", "ramp", "quadrants")):
        out.append(_c(f"y-{name}", 16, "t2", "yuv", *base, name, 10 + i))
    for name in ("vivid", "ramp"):
        out.append(_c(f"y-{name}-trilinear", 16, "t2", "yuv", *base, name, 20, mode="trilinear"))
        out.append(_c(f"y-{name}-fma32", 16, "t2", "yuv", *base, name, 21, prec="fma32"))
        out.append(_c(f"y-{name}-fast", 16, "t2", "yuv", *base, name, 22, prec="fast"))
        out.append(_c(f"y-{name}-nearest", 16, "t2", "yuv", *base, name, 23, mode="nearest"))
        out.append(_c(f"y-{name}-edge", 16, "t2", "yuv", "yuv420p10le", 1544, 1092, name, 24))
        out.append(_c(f"y-{name}-420p8", 16, "t2", "yuv", "yuv420p", 2048, 1664, name, 25))
        out.append(_c(f"y-{name}-422p10", 16, "t2", "yuv", "yuv422p10le", 1024, 832, name, 26))
        out.append(_c(f"y-{name}-444p10", 16, "t2", "yuv", "yuv444p10le", 1024, 832, name, 26))      # (the same frame, 4:4:4)
        out.append(_c(f"y-{name}-10to8", 16, "t2", "yuv", *base, name, 28, ofmt="yuv420p"))
        out.append(_c(f"y-{name}-25", 16, "t2", "yuv", *base, name, 29, lut="u25"))
        out.append(_c(f"y-{name}-prologue", 16, "t2", "yuv", *base, name, 30, full_range=True,
                      kw=dict(range_src="pc", range_in="tv", lut_depth=8)))
        out.append(_c(f"y-{name}-shaper", 16, "t2", "yuv", *base, name, 31, lut="shaper"))
        out.append(_c(f"y-{name}-wide", 16, "t2", "yuv", *base, name, 32, lut="wide33"))
        out.append(_c(f"y-{name}-domains", 16, "t2", "yuv", *base, name, 33, lut="domains"))
    out.append(_c("y-batch", 16, "t2", "yuv", "yuv420p10le", 1024, 416, ("natural", "vivid", "uniform", "ramp"), 40))
    out.append(_c("y-shard", 16, "t2", "yuv", "yuv420p10le", 1536, 1632, "vivid", 41, shard=(272, 1088)))
    out.append(_c("y-natural-65", 16, "t2", "yuv", *base, "natural", 42, lut="log65"))
    out.append(_c("y-vivid-65", 16, "t2", "yuv", *base, "vivid", 43, lut="log65"))
    out.append(_c("y-uniform-17", 16, "t2", "yuv", *base, "uniform", 44, lut="u17"))
    # RGB: the tube kernels (planar trilinear needs LUTR_RGB2=all, read per call), then planar trilinear on round 1's k_rgb_tile
    for name in ("natural", "vivid", "uniform"):
        out.append(_c(f"r-gbrp10-{name}", 16, "r2", "rgb", "gbrp10le", 1024, 832, name, 50))
        out.append(_c(f"r-rgb24-{name}", 16, "r2", "packed", "rgb24", 1536, 1088, name, 51))
        out.append(_c(f"r-bgr48-{name}", 16, "r2", "packed", "bgr48le", 1024, 832, name, 52))
        out.append(_c(f"r-gbrp10-{name}-t1", 16, "t1", "rgb", "gbrp10le", 1024, 832, name, 53, mode="trilinear"))
    out.append(_c("r-gbrp10-vivid-trilinear", 16, "r2", "rgb", "gbrp10le", 1024, 832, "vivid", 54, mode="trilinear",
                  env={"LUTR_RGB2": "all"}))
    out.append(_c("r-rgb24-vivid-trilinear", 16, "r2", "packed", "rgb24", 1536, 1088, "vivid", 55, mode="trilinear"))
    out.append(_c("r-bgr48-vivid-trilinear", 16, "r2", "packed", "bgr48le", 1024, 832, "vivid", 56, mode="trilinear"))
    # two workgroups: the global atomic between them, and the last workgroup's reset of the queue words, three launches in a row
    for tag, name in (("a", "ramp"), ("b", "vivid"), ("c", "ramp")):
        out.append(_c(f"y32-{tag}-{name}", 32, "t2", "yuv", "yuv420p10le", 2048, 1664, name, 60))
    return out


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}
PACKED = {"rgb24": (8, 3, (0, 1, 2)), "bgr48le": (16, 3, (2, 1, 0))}          # bits, components, offsets of (R, G, B)


def make_source(case):
    """The source of a case as host arrays: YUV planes (Y, Cb, Cr), planar RGB in gbrp order (G, B, R), or one packed image
    [H, W, C].  A batch: arrays with a leading frame axis."""
    w, h, seed = case["w"], case["h"], case["seed"]
    if case["api"] == "yuv":
        depth, csx, csy = YUV_FMT[case["fmt"]]
        if isinstance(case["content"], tuple):
            per = [yuv_content(n, w, h, depth, csx, csy, seed + i, case["full_range"]) for i, n in enumerate(case["content"])]
            return [np.stack([f[p] for f in per]) for p in range(3)]
        return yuv_content(case["content"], w, h, depth, csx, csy, seed, case["full_range"])
    if case["api"] == "rgb":
        return frames.make_rgb(case["content"], w, h, 10, k=seed)
    bits, nc, (ro, go, bo) = PACKED[case["fmt"]]
    g, b, r = frames.make_rgb(case["content"], w, h, bits, k=seed)
    img = np.empty((h, w, nc), dtype=g.dtype)
    img[..., ro], img[..., go], img[..., bo] = r, g, b
    return img
