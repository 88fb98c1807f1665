#!/usr/bin/env python3
"""tools/lut1d_rate.py -- a 1D LUT alone or in front of the 3D LUT in the fused pass, the table in LDS and in
global memory, against kernels that were there before it.

The batch: `frames.make_yuv` frames tiled to 64 UHD yuv420p10le frames on the device; 3D LUT = `cube.log709_lattice(33)`,
tetrahedral, strict precision; 1D LUT = a 1024-point gamma curve, linear; content natural and sigma-16 noise; yuv420p10le and
yuv422p10le out.  Paths timed per content and output layout, all in ONE process (LUTR_L1D_LDS is read at every launch):
  plain_vec        the call without a 1D LUT under variant vec_global (k_yuv_vec / k_yuv_xsub_vec): a yardstick
  cdl_sat1         the CDL pass with saturation 1 (k_yuv_cdl_vec): the same taps plus three table reads of twice the bytes, a yardstick
  l1d_l3d_lds      lut1d -> lut3d, the table staged into LDS once per workgroup
  l1d_l3d_global   lut1d -> lut3d, the table read from global memory
  l1d_lds          lut1d alone, table in LDS
  l1d_global       lut1d alone, table in global memory
and once, on the natural content: planar gbrp10le lut1d alone (k_rgb_l1d) against torch `copy_` of the same three planes.
Paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is
the median round.  Prints one JSON line (and writes it to `--out` when given): Gpx/s per path and the ratios over the yardsticks.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/lut1d_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/lut1d_rate.json
"""
import argparse
import json
import os
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
OUTS = ("yuv420p10le", "yuv422p10le")
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


def placed(knob, call):
    """`call` with LUTR_L1D_LDS = knob for the launch (the launcher reads it every time)."""
    def run():
        os.environ["LUTR_L1D_LDS"] = knob
        try:
            return call()
        finally:
            del os.environ["LUTR_L1D_LDS"]
    return run


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
        raise SystemExit("lut1d_rate.py needs a GPU")
    lut = cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33))
    x = np.linspace(0.0, 1.0, 1024)
    l1 = cube.Lut1D(np.tile((x ** (1 / 2.2)).astype(np.float32), (3, 1)), np.ones(3, np.float32))
    vec, cdl, one = (LutEngine(0) for _ in range(3))
    for e in (vec, cdl, one):
        e.set_lut(lut)
    vec.set_variant("vec_global")
    one.set_lut1d(l1, "linear")
    sat1 = Cdl(**SOP, saturation=1.0)
    dev = vec.device
    res = {}
    for dist in DISTS:
        src = batch(dev, dist, args.frames, args.unique)
        res[dist] = {}
        for out_fmt in OUTS:
            out = empty(dev, out_fmt, args.frames)
            names = dict(pix_fmt=FMT, out_pix_fmt=out_fmt)

            def l1d(interp):
                return lambda: one.apply_yuv_lut1d(src, out, interp=interp, **names)

            paths = {
                "plain_vec": (lambda: vec.apply_yuv(src, out, interp="tetrahedral", **names), lambda: vec.last_kernel),
                "cdl_sat1": (lambda: cdl.apply_yuv(src, out, interp="tetrahedral", cdl=sat1, **names), lambda: cdl.last_kernel),
                "l1d_l3d_lds": (placed("1", l1d("tetrahedral")), lambda: one.last_kernel),
                "l1d_l3d_global": (placed("0", l1d("tetrahedral")), lambda: one.last_kernel),
                "l1d_lds": (placed("1", l1d(None)), lambda: one.last_kernel),
                "l1d_global": (placed("0", l1d(None)), lambda: one.last_kernel),
            }
            r = time_paths(paths, args)
            for n in ("l1d_l3d_lds", "l1d_l3d_global", "l1d_lds", "l1d_global"):
                r[f"{n}_vs_plain_vec"] = round(r[n]["gpx_s"] / r["plain_vec"]["gpx_s"], 3)
                r[f"{n}_vs_cdl_sat1"] = round(r[n]["gpx_s"] / r["cdl_sat1"]["gpx_s"], 3)
            r["lds_vs_global_l1d_l3d"] = round(r["l1d_l3d_lds"]["gpx_s"] / r["l1d_l3d_global"]["gpx_s"], 3)
            r["lds_vs_global_l1d"] = round(r["l1d_lds"]["gpx_s"] / r["l1d_global"]["gpx_s"], 3)
            res[dist][out_fmt] = r
            del paths, out
        del src
        torch.cuda.empty_cache()
    # planar RGB: lut1d alone against a copy of the same planes
    rgb = [torch.from_numpy(np.ascontiguousarray(p).view(np.int16)) for p in frames.make_rgb("natural", W, H, 10, k=1)]
    rgb = [p.to(dev).unsqueeze(0).repeat(args.frames, 1, 1).contiguous() for p in rgb]
    rout = [torch.empty_like(p) for p in rgb]

    def copy():
        for d, s in zip(rout, rgb):
            d.copy_(s)

    r = time_paths({"rgb_l1d": (lambda: one.apply_rgb_lut1d(rgb, rout, depth=10), lambda: one.last_kernel),
                    "torch_copy": (copy, lambda: "torch.Tensor.copy_ x 3")}, args)
    r["rgb_l1d_vs_copy"] = round(r["rgb_l1d"]["gpx_s"] / r["torch_copy"]["gpx_s"], 3)
    res["gbrp10le"] = r
    for e in (vec, cdl, one):
        e.close()
    line = json.dumps({"tool": "lut1d_rate", "frames": args.frames, "size": f"{W}x{H}", "pix_fmt": FMT, "lut": 33,
                       "interp": "tetrahedral", "precision": "strict", "lut1d": {"rows": 1024, "interp1d": "linear"},
                       "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
