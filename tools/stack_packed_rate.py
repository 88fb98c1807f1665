#!/usr/bin/env python3
"""tools/stack_packed_rate.py -- the stage stack on packed 4:2:2 / v210 frames: the fused pass against the planar
stack kernel on the same samples in yuv422p*, and against what a user needed without it -- an unpacking pass, the stack, a packing
pass.

The batch: `frames.make_yuv` 4:2:2 frames tiled to 64 UHD frames on the device, at 10 bit (v210, y210le) and at 8 bit (uyvy422);
lattice 33^3 (`cube.log709_lattice(33)`), tetrahedral, strict precision; 1D LUT = a 1024-point gamma curve, linear; the CDL of
tests/golden/cdl/shot.cc (saturation 0.6); content natural and sigma-16 noise; the list [lut1d, cdl, lut3d].  Per content and pair
of containers (v210 -> v210, uyvy422 -> uyvy422, y210le -> y210le, v210 -> yuv422p10le), all in ONE process:
  (a) fused      apply_yuv_stack_packed on the containers                    k_yuv_stack_v210_vec / k_yuv_stack_pk_vec
  (b) planar     apply_yuv_stack on the same samples, planar in and out      k_yuv_stack_vec
  (c) three      what a user needs today, the container passes timed: v210.to_planar / packedyuv.to_planar on the device (torch:
                 shifts, masks, fresh planes), (b), then v210.to_v210 / packedyuv.to_packed on the device where the destination is
                 a container
Before anything is timed the bits of (a) are compared with those of (c) on the whole batch.  Paths are timed in alternating rounds
with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is the median round, and the rounds are
kept (their spread is the noise of the run).  Prints one JSON line (and writes it to `--out` when given): Gpx/s and ms per path and
the ratios (a)/(b) and (a)/(c).

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 900 python tools/stack_packed_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/stack_packed_rate.json
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from lut_renderer_amd import cube, frames, packedyuv, v210  # noqa: E402
from lut_renderer_amd.cdl import Cdl  # noqa: E402
from lut_renderer_amd.engine import LutEngine  # noqa: E402
from lut_renderer_amd.formats import yuv_side  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
PAIRS = (("v210", "v210"), ("uyvy422", "uyvy422"), ("y210le", "y210le"), ("v210", "yuv422p10le"))
STAGES = "lut1d,cdl,lut3d"
GRADE = dict(slope=(1.3, 1.25, 1.1), offset=(-0.08, 0.0, 0.05), power=(0.8, 1.0, 1.2), saturation=0.6)


def planar_name(side):
    return side.planar if side.nplanes == 1 else side.name


def to_container(planes, name):
    """planar 4:2:2 codes on the device -> the one buffer of the container `name` (a planar name: the planes themselves)"""
    if name == "v210":
        return v210.to_v210(planes, W)
    return packedyuv.to_packed(planes, name) if yuv_side(name).nplanes == 1 else planes


def to_planes(buf, name):
    if name == "v210":
        return v210.to_planar(buf, W)
    return packedyuv.to_planar(buf, name, W) if yuv_side(name).nplanes == 1 else buf


def batch(dev, dist, depth, nframes, unique):
    """planar 4:2:2 codes at `depth`, tiled to nframes on the device"""
    planes = [[], [], []]
    for k in range(unique):
        f = frames.make_yuv(dist, W, H, depth, 1, 0, k=k)
        for i in range(3):
            p = np.ascontiguousarray(f[i])
            planes[i].append(torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p))
    reps = (nframes + unique - 1) // unique
    return [torch.stack(p).to(dev).repeat(reps, 1, 1)[:nframes].contiguous() for p in planes]


def same(x, y):
    xs, ys = (x if isinstance(x, list) else [x]), (y if isinstance(y, list) else [y])
    return all(torch.equal(p, q) for p, q in zip(xs, ys))


def time_paths(paths, args):
    """paths: name -> (callable that launches the path once, callable that names its kernel).  Returns name -> figures."""
    kern = {}
    for n, (run, name) in paths.items():
        for _ in range(args.warmup):
            run()
        kern[n] = name()
    torch.cuda.synchronize()
    secs = {n: [] for n in paths}
    for _ in range(args.rounds):
        for n, (run, _) in paths.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                run()
            ev1.record()
            torch.cuda.synchronize()
            secs[n].append(ev0.elapsed_time(ev1) / 1e3 / args.steps)
    px = args.frames * W * H
    return {n: {"gpx_s": round(px / statistics.median(s) / 1e9, 1), "ms": round(statistics.median(s) * 1e3, 3),
                "rounds_ms": [round(v * 1e3, 3) for v in s], "kernel": kern[n]} for n, s in secs.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10, help="launches per timed round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches of each path before the first round")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds over the paths")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--unique", type=int, default=4, help="distinct synthetic frames tiled to --frames")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stack_packed_rate.py needs a GPU")
    ones = np.ones(3, np.float32)
    lut = cube.CubeLut(33, ones, cube.log709_lattice(33))
    x = np.linspace(0.0, 1.0, 1024)
    l1 = cube.Lut1D(np.tile((x ** (1 / 2.2)).astype(np.float32), (3, 1)), ones)
    grade = Cdl(**GRADE)
    eng = LutEngine(0)
    eng.set_lut(lut)
    eng.set_lut1d(l1, "linear")
    dev = eng.device
    res = {}
    for dist in DISTS:
        res[dist] = {}
        planes = {}                                            # the planar batch of a depth, made once per content
        for a, b in PAIRS:
            fa, fb = yuv_side(a), yuv_side(b)
            pa, pb = planar_name(fa), planar_name(fb)
            if fa.depth not in planes:
                planes[fa.depth] = batch(dev, dist, fa.depth, args.frames, args.unique)
            planar = planes[fa.depth]
            held = to_container(planar, a)
            pout = [torch.empty_like(p) for p in planar]
            names = dict(stages=STAGES, cdl=grade)
            out = eng.apply_yuv_stack_packed(held, None, pix_fmt=a, out_pix_fmt=b, width=W, **names)   # (the engine's own fresh destination)

            def fused():
                eng.apply_yuv_stack_packed(held, out, pix_fmt=a, out_pix_fmt=b, width=W, **names)

            def plain():
                eng.apply_yuv_stack(planar, pout, pix_fmt=pa, out_pix_fmt=pb, **names)

            def three():
                eng.apply_yuv_stack(to_planes(held, a), pout, pix_fmt=pa, out_pix_fmt=pb, **names)
                return to_container(pout, b)

            fused()
            equal = same(out, three())
            torch.cuda.synchronize()
            k = lambda: eng.last_kernel                                               # noqa: E731
            r = time_paths({"fused": (fused, k), "planar": (plain, k), "three": (three, k)}, args)
            r["fused_equals_three"] = bool(equal)
            r["fused_time_vs_planar"] = round(r["fused"]["ms"] / r["planar"]["ms"], 3)
            r["fused_time_vs_three"] = round(r["fused"]["ms"] / r["three"]["ms"], 3)
            res[dist][f"{a}->{b}"] = r
            del held, out, pout
            torch.cuda.empty_cache()
        del planes
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps({"tool": "stack_packed_rate", "frames": args.frames, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "stages": STAGES, "lut1d": {"rows": 1024, "interp1d": "linear"}, "cdl": GRADE,
                       "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
                       "results": res})
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
