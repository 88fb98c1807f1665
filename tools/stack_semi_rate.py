#!/usr/bin/env python3
"""tools/stack_semi_rate.py -- the stage stack on semi-planar sides: the semi form of the stack kernel against the
plain form on the same samples in three planes, and against what a user needed without it -- a de-interleave pass, the stack, an
interleave pass.

The batch: `frames.make_yuv` frames tiled to 64 UHD frames on the device, 4:2:0 at 10 bit (p010le) and at 8 bit (nv12); lattice
33^3 (`cube.log709_lattice(33)`), tetrahedral, strict precision; 1D LUT = a 1024-point gamma curve, linear; the CDL of
tests/golden/cdl/shot.cc (saturation 0.6); content natural and sigma-16 noise; lists [lut1d, cdl, lut3d] and [lut3d].  Per
content, list and pair of containers (p010le -> p010le, nv12 -> nv12, p010le -> yuv422p10le), all in ONE process:
  (a) semi       apply_yuv_stack_semi on the containers                      k_yuv_stack_semi_vec
  (b) planar     apply_yuv_stack on the same samples, planar in and out      k_yuv_stack_vec
  (c) three      what a user needs today, the container passes timed: semiplanar.to_planar on the device (torch: slices, a shift,
                 fresh planes), (b), then semiplanar.to_semi on the device where the destination is semi-planar
Paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is
the median round, and the rounds are kept.  Prints one JSON line (and writes it to `--out` when given): Gpx/s and ms per path and
the ratios (a)/(b) and (a)/(c).

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 900 python tools/stack_semi_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/stack_semi_rate.json
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from lut_renderer_amd import cube, frames, semiplanar  # noqa: E402
from lut_renderer_amd.cdl import Cdl  # noqa: E402
from lut_renderer_amd.engine import LutEngine  # noqa: E402
from lut_renderer_amd.formats import yuv_side  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
PAIRS = (("p010le", "p010le"), ("nv12", "nv12"), ("p010le", "yuv422p10le"))
LISTS = ("lut1d,cdl,lut3d", "lut3d")
GRADE = dict(slope=(1.3, 1.25, 1.1), offset=(-0.08, 0.0, 0.05), power=(0.8, 1.0, 1.2), saturation=0.6)


def planar_name(side):
    return side.planar if side.nplanes == 2 else side.name


def batch(dev, dist, depth, nframes, unique):
    """planar 4:2:0 codes at `depth`, tiled to nframes on the device"""
    planes = [[], [], []]
    for k in range(unique):
        f = frames.make_yuv(dist, W, H, depth, 1, 1, k=k)
        for i in range(3):
            p = np.ascontiguousarray(f[i])
            planes[i].append(torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p))
    reps = (nframes + unique - 1) // unique
    return [torch.stack(p).to(dev).repeat(reps, 1, 1)[:nframes].contiguous() for p in planes]


def empty(dev, side, nframes):
    dt = torch.int16 if side.depth > 8 else torch.uint8
    return [torch.empty((nframes,) + side.plane_shape(i, W, H), dtype=dt, device=dev) for i in range(side.nplanes)]


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
        raise SystemExit("stack_semi_rate.py needs a GPU")
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
        for a, b in PAIRS:
            fa, fb = yuv_side(a), yuv_side(b)
            pa, pb = planar_name(fa), planar_name(fb)
            planar = batch(dev, dist, fa.depth, args.frames, args.unique)
            held = semiplanar.to_semi(planar, a)
            out, pout = empty(dev, fb, args.frames), empty(dev, yuv_side(pb), args.frames)
            res[dist][f"{a}->{b}"] = {}
            for stages in LISTS:
                cdl = grade if "cdl" in stages else None

                def semi():
                    eng.apply_yuv_stack_semi(held, out, pix_fmt=a, out_pix_fmt=b, stages=stages, cdl=cdl)

                def plain():
                    eng.apply_yuv_stack(planar, pout, pix_fmt=pa, out_pix_fmt=pb, stages=stages, cdl=cdl)

                def three():
                    p = semiplanar.to_planar(held, a)
                    eng.apply_yuv_stack(p, pout, pix_fmt=pa, out_pix_fmt=pb, stages=stages, cdl=cdl)
                    return semiplanar.to_semi(pout, b) if fb.nplanes == 2 else pout

                k = lambda: eng.last_kernel                                               # noqa: E731
                r = time_paths({"semi": (semi, k), "planar": (plain, k), "three": (three, k)}, args)
                r["semi_time_vs_planar"] = round(r["semi"]["ms"] / r["planar"]["ms"], 3)
                r["semi_time_vs_three"] = round(r["semi"]["ms"] / r["three"]["ms"], 3)
                res[dist][f"{a}->{b}"][stages] = r
            del planar, held, out, pout
            torch.cuda.empty_cache()
    eng.close()
    line = json.dumps({"tool": "stack_semi_rate", "frames": args.frames, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "lut1d": {"rows": 1024, "interp1d": "linear"}, "cdl": GRADE, "steps": args.steps,
                       "warmup": args.warmup, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
