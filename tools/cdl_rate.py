#!/usr/bin/env python3
"""tools/cdl_rate.py -- an ASC CDL in front of the LUT in the fused pass against the same call without it.

The batch: `frames.make_yuv` frames tiled to 64 UHD yuv420p10le frames on the device; LUT = `cube.log709_lattice(33)`, tetrahedral,
strict precision; content natural and sigma-16 noise; yuv420p10le out.  Paths timed per content, all in ONE process:
  plain_vec    the call without a CDL under variant vec_global (k_yuv_vec): the yardstick, a kernel of the same family that was
               there before the CDL pass
  cdl_sat1     the CDL pass with saturation 1: three table reads per pixel, the mix skipped (k_yuv_cdl_vec)
  cdl_sat      the CDL pass with saturation 0.85: the table reads and the mix
  plain_auto   the call without a CDL on auto (the LDS-window tile kernels): what having no LDS kernel costs the CDL pass
Paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is
the median round.  Prints one JSON line (and writes it to `--out` when given): Gpx/s per path, and each CDL path over plain_vec and
over plain_auto.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/cdl_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/cdl_rate.json
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
from lut_renderer_amd.cdl import Cdl  # noqa: E402
from lut_renderer_amd.engine import LutEngine, parse_pix_fmt  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
FMT = "yuv420p10le"
SOP = dict(slope=(1.3, 1.25, 1.1), offset=(-0.08, 0.0, 0.05), power=(0.8, 1.0, 1.2))


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
                "rounds_gpx_s": [round(px / v / 1e9, 1) for v in s], "kernel": kern[n]} for n, s in secs.items()}


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
        raise SystemExit("cdl_rate.py needs a GPU")
    lut = cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33))
    vec, auto, cdl1, cdl2 = (LutEngine(0) for _ in range(4))
    for e in (vec, auto, cdl1, cdl2):
        e.set_lut(lut)
    vec.set_variant("vec_global")
    sat1, sat = Cdl(**SOP, saturation=1.0), Cdl(**SOP, saturation=0.85)
    dev = vec.device
    res = {}
    for dist in DISTS:
        src = batch(dev, dist, args.frames, args.unique)
        out = {n: empty(dev, FMT, args.frames) for n in ("plain_vec", "cdl_sat1", "cdl_sat", "plain_auto")}
        paths = {
            "plain_vec": (lambda: vec.apply_yuv(src, out["plain_vec"], pix_fmt=FMT, interp="tetrahedral"), lambda: vec.last_kernel),
            "cdl_sat1": (lambda: cdl1.apply_yuv(src, out["cdl_sat1"], pix_fmt=FMT, interp="tetrahedral", cdl=sat1),
                         lambda: cdl1.last_kernel),
            "cdl_sat": (lambda: cdl2.apply_yuv(src, out["cdl_sat"], pix_fmt=FMT, interp="tetrahedral", cdl=sat),
                        lambda: cdl2.last_kernel),
            "plain_auto": (lambda: auto.apply_yuv(src, out["plain_auto"], pix_fmt=FMT, interp="tetrahedral"),
                           lambda: auto.last_kernel),
        }
        r = time_paths(paths, args)
        for n in ("cdl_sat1", "cdl_sat"):
            r[f"{n}_vs_plain_vec"] = round(r[n]["gpx_s"] / r["plain_vec"]["gpx_s"], 3)
            r[f"{n}_vs_plain_auto"] = round(r[n]["gpx_s"] / r["plain_auto"]["gpx_s"], 3)
        res[dist] = r
        del paths, out, src
        torch.cuda.empty_cache()
    for e in (vec, auto, cdl1, cdl2):
        e.close()
    line = json.dumps({"tool": "cdl_rate", "frames": args.frames, "size": f"{W}x{H}", "pix_fmt": FMT, "lut": 33,
                       "interp": "tetrahedral", "precision": "strict", "cdl": {**SOP, "saturations": [1.0, 0.85]},
                       "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
