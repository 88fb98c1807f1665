#!/usr/bin/env python3
"""tools/chain_rate.py -- two LUTs in one fused pass against one LUT, and against the two launches it replaces.

The batch: `frames.make_yuv` frames tiled to 64 UHD yuv420p10le frames on the device; A = `cube.log709_lattice(33)`, B = a 33^3
look (A with another saturation and exposure); tetrahedral on both, strict precision; content natural and sigma-16 noise.  Paths
timed per content and output layout (-> yuv420p10le, -> yuv422p10le), all in ONE process:
  chain        lutr_apply_yuv_chain on the vector kernel (k_yuv_chain_vec)
  single_vec   the single-LUT launch of the same layout pair under variant vec_global (k_yuv_vec / k_yuv_xsub_vec): the yardstick
               for what the second gather costs
  two_launch   what a user needs without the chain: apply_yuv with A -> yuv444p10le, then apply_yuv with B -> the output format
               (default variant, two engines on one stream).  Its BITS DIFFER from the chain's -- the frame goes through YUV
               between the LUTs -- so it is a time yardstick only.
Paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is
the median round.  Prints one JSON line: Gpx/s per path, and chain over single_vec and over two_launch.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/chain_rate.py --steps 10 --warmup 3 --rounds 3
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from lut_renderer_amd import cube, frames  # noqa: E402
from lut_renderer_amd.engine import LutEngine, parse_pix_fmt  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
SRC = "yuv420p10le"
OUTS = ("yuv420p10le", "yuv422p10le")
MID = "yuv444p10le"


def batch(dev, dist, nframes, unique):
    planes = [[], [], []]
    for k in range(unique):
        f = frames.make_yuv(dist, W, H, 10, 1, 1, k=k)
        for i in range(3):
            planes[i].append(torch.from_numpy(np.ascontiguousarray(f[i]).view(np.int16)))
    reps = (nframes + unique - 1) // unique
    return [torch.stack(p).to(dev).repeat(reps, 1, 1)[:nframes].contiguous() for p in planes]


def empty(dev, name, nframes):
    f = parse_pix_fmt(name)
    return [torch.empty((nframes,) + f.plane_shape(i, W, H), dtype=torch.int16, device=dev) for i in range(3)]


def time_paths(paths, args):
    """paths: name -> (callable that launches the path once, callable that names its kernels).  Returns name -> figures."""
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
    return {n: {"gpx_s": round(px / statistics.median(s) / 1e9, 1), "rounds_gpx_s": [round(px / v / 1e9, 1) for v in s],
                "kernel": kern[n]} for n, s in secs.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10, help="launches per timed round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches of each path before the first round")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds over the paths")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--unique", type=int, default=4, help="distinct synthetic frames tiled to --frames")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chain_rate.py needs a GPU")
    lut_a = cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33))
    lut_b = cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33, saturation=0.9, exposure=1.1))
    chain, single, first, second = (LutEngine(0) for _ in range(4))
    chain.set_lut(lut_a)
    chain.set_lut2(lut_b)
    single.set_lut(lut_a)
    single.set_variant("vec_global")
    first.set_lut(lut_a)
    second.set_lut(lut_b)
    dev = chain.device
    mid = empty(dev, MID, args.frames)
    res = {}
    for dist in DISTS:
        src = batch(dev, dist, args.frames, args.unique)
        res[dist] = {}
        for fo in OUTS:
            out = {n: empty(dev, fo, args.frames) for n in ("chain", "single_vec", "two_launch")}

            def two(fo=fo, out=out):
                first.apply_yuv(src, mid, pix_fmt=SRC, out_pix_fmt=MID, interp="tetrahedral")
                second.apply_yuv(mid, out["two_launch"], pix_fmt=MID, out_pix_fmt=fo, interp="tetrahedral")

            paths = {
                "chain": (lambda fo=fo, out=out: chain.apply_yuv_chain(src, out["chain"], pix_fmt=SRC, out_pix_fmt=fo,
                                                                         interp="tetrahedral"), lambda: chain.last_kernel),
                "single_vec": (lambda fo=fo, out=out: single.apply_yuv(src, out["single_vec"], pix_fmt=SRC, out_pix_fmt=fo,
                                                                       interp="tetrahedral"), lambda: single.last_kernel),
                "two_launch": (two, lambda: f"{first.last_kernel} ; {second.last_kernel}"),
            }
            r = time_paths(paths, args)
            r["chain_vs_single_vec"] = round(r["chain"]["gpx_s"] / r["single_vec"]["gpx_s"], 3)
            r["chain_vs_two_launch"] = round(r["chain"]["gpx_s"] / r["two_launch"]["gpx_s"], 3)
            res[dist][fo] = r
            del paths, out
        del src
        torch.cuda.empty_cache()
    for e in (chain, single, first, second):
        e.close()
    print(json.dumps({"tool": "chain_rate", "frames": args.frames, "size": f"{W}x{H}", "src": SRC, "luts": [33, 33],
                      "interp": "tetrahedral", "precision": "strict", "steps": args.steps, "warmup": args.warmup,
                      "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
