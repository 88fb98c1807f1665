#!/usr/bin/env python3
"""tools/dual_rate.py -- the fused two-output pass against the two single-output launches it replaces.

The batch: synthetic `yuv420p10le` frames (`frames.make_yuv`) tiled to 64 UHD frames on the device, `cube.log709_lattice(33)`,
tetrahedral, strict precision; content natural and sigma-16 noise.  The job is the reference's "pro" mode: a yuv422p10le master
and a yuv420p delivery frame from the same source.  Paths timed per content:
  dual              yuv420p10le -> yuv422p10le + yuv420p in ONE launch   k_yuv_dual_vec (variant vec_global)
  vg_422p10         yuv420p10le -> yuv422p10le   k_yuv_xsub_vec (variant vec_global)
  vg_420p           yuv420p10le -> yuv420p       k_yuv_vec      (variant vec_global)
  auto_422p10       the same two launches with variant auto: what the engine picks for a batch of this size (the LDS tile
  auto_420p         kernel where one exists)
All paths run in one process, timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches
of each; the figure is the median round.  Prints one JSON line (and writes it to --out when given): milliseconds per launch
and Gpx/s per path, and the fused launch's time as a fraction of the sum of the pair it replaces (`dual_vs_vg_pair`,
`dual_vs_auto_pair`: below 1 the fused launch is faster).

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/dual_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/dual_rate.json
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
SRC, MASTER, DELIVERY = "yuv420p10le", "yuv422p10le", "yuv420p"
#: name -> (variant, output formats)
PATHS = {
    "dual": ("vec_global", (MASTER, DELIVERY)),
    "vg_422p10": ("vec_global", (MASTER,)),
    "vg_420p": ("vec_global", (DELIVERY,)),
    "auto_422p10": ("auto", (MASTER,)),
    "auto_420p": ("auto", (DELIVERY,)),
}


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def source(eng, dist, nframes, unique):
    """`nframes` device frames of SRC: `unique` distinct synthetic frames, tiled."""
    reps = (nframes + unique - 1) // unique
    f = parse_pix_fmt(SRC)
    fs = [frames.make_yuv(dist, W, H, f.depth, f.csx, f.csy, k=k) for k in range(unique)]
    return [torch.stack([_dev(x[i]) for x in fs]).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for i in range(3)]


def planes(eng, name, nframes):
    f = parse_pix_fmt(name)
    dt = torch.uint8 if f.depth <= 8 else torch.int16
    return [torch.empty((nframes,) + f.plane_shape(i, W, H), dtype=dt, device=eng.device) for i in range(3)]


def call(eng, src, outs, name):
    variant, fmts = PATHS[name]
    eng.set_variant(variant)
    if len(fmts) == 2:
        eng.apply_yuv_dual(src, outs[fmts[0]], outs[fmts[1]], pix_fmt=SRC, out_pix_fmt=fmts[0], out2_pix_fmt=fmts[1],
                           interp="tetrahedral")
    else:
        eng.apply_yuv(src, outs[fmts[0]], pix_fmt=SRC, out_pix_fmt=fmts[0], interp="tetrahedral")


def time_paths(eng, dist, args):
    src = source(eng, dist, args.frames, args.unique)
    outs = {MASTER: planes(eng, MASTER, args.frames), DELIVERY: planes(eng, DELIVERY, args.frames)}
    kern = {}
    for n in PATHS:
        for _ in range(args.warmup):
            call(eng, src, outs, n)
        kern[n] = eng.last_kernel
    torch.cuda.synchronize()
    secs = {n: [] for n in PATHS}
    for _ in range(args.rounds):
        for n in PATHS:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                call(eng, src, outs, n)
            ev1.record()
            torch.cuda.synchronize()
            secs[n].append(ev0.elapsed_time(ev1) / 1e3 / args.steps)
    px = args.frames * W * H
    res = {}
    for n, s in secs.items():
        med = statistics.median(s)
        res[n] = {"ms": round(med * 1e3, 3), "rounds_ms": [round(v * 1e3, 3) for v in s], "gpx_s": round(px / med / 1e9, 1),
                  "kernel": kern[n]}
    for tag in ("vg", "auto"):
        pair = res[f"{tag}_422p10"]["ms"] + res[f"{tag}_420p"]["ms"]
        res[f"{tag}_pair_ms"] = round(pair, 3)
        res[f"dual_vs_{tag}_pair"] = round(res["dual"]["ms"] / pair, 3)
    return res


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
        raise SystemExit("dual_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    res = {}
    for dist in DISTS:
        res[dist] = time_paths(eng, dist, args)
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps({"tool": "dual_rate", "frames": args.frames, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
