#!/usr/bin/env python3
"""tools/precision_rate.py -- strict / fast / fma32 side by side on the headline batch, in one process.

The batch is built as bench.py builds it: `frames.make_yuv` frames tiled to 256 UHD yuv420p10le frames on the device and
`cube.log709_lattice(33)`, LDS-window tile kernels.  Per case (33^3 tetrahedral on natural frames, trilinear on natural
frames, tetrahedral on sigma-16 noise) the three precisions are timed in alternating rounds with HIP events around `--steps`
launches, after `--warmup` launches of each; the figure per precision is the median round.  Each precision's output is also
compared with strict's (max |d| over the batch, which must be <= 1).  Prints one JSON line.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 900 python tools/precision_rate.py --steps 10 --warmup 5 --rounds 3
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
from lut_renderer_amd.engine import LutEngine  # noqa: E402

PRECISIONS = ("strict", "fast", "fma32")
CASES = {"tetrahedral_natural": ("tetrahedral", "natural"), "trilinear_natural": ("trilinear", "natural"),
         "tetrahedral_noise16": ("tetrahedral", "noise16")}


def batch(eng, dist, w, h, nframes, unique):
    planes = [[], [], []]
    for k in range(unique):
        f = frames.make_yuv(dist, w, h, 10, 1, 1, k=k)
        for i in range(3):
            planes[i].append(torch.from_numpy(np.ascontiguousarray(f[i]).view(np.int16)))
    reps = (nframes + unique - 1) // unique
    return [torch.stack(p).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for p in planes]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10, help="launches per timed round")
    ap.add_argument("--warmup", type=int, default=5, help="untimed launches of each precision before the first round")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds (strict, fast, fma32, strict, ...)")
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--unique", type=int, default=4, help="distinct synthetic frames tiled to --frames")
    ap.add_argument("--lut", type=int, default=33)
    ap.add_argument("--cases", default=",".join(CASES), help="comma list of " + ", ".join(CASES))
    ap.add_argument("--precisions", default=",".join(PRECISIONS))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("precision_rate.py needs a GPU")
    w, h = 3840, 2160
    precs = args.precisions.split(",")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(args.lut, np.ones(3, np.float32), cube.log709_lattice(args.lut)))
    eng.set_variant("vec_lds")
    res = {}
    srcs = {}
    for case in args.cases.split(","):
        mode, dist = CASES[case]
        if dist not in srcs:
            srcs[dist] = batch(eng, dist, w, h, args.frames, args.unique)
        src = srcs[dist]
        outs = {p: [torch.empty_like(t) for t in src] for p in precs}
        kern = {}
        for p in precs:
            eng.set_precision(p)
            for _ in range(args.warmup):
                eng.apply_yuv(src, outs[p], pix_fmt="yuv420p10le", interp=mode)
            kern[p] = eng.last_kernel
        torch.cuda.synchronize()
        secs = {p: [] for p in precs}
        for _ in range(args.rounds):
            for p in precs:
                eng.set_precision(p)
                ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                ev0.record()
                for _ in range(args.steps):
                    eng.apply_yuv(src, outs[p], pix_fmt="yuv420p10le", interp=mode)
                ev1.record()
                torch.cuda.synchronize()
                secs[p].append(ev0.elapsed_time(ev1) / 1e3 / args.steps)
        px = args.frames * w * h
        entry = {}
        for p in precs:
            med = statistics.median(secs[p])
            d = 0
            if "strict" in outs and p != "strict":
                d = max(int((a.to(torch.int32) - b.to(torch.int32)).abs().max().item()) for a, b in zip(outs[p], outs["strict"]))
            entry[p] = {"gpx_s": round(px / med / 1e9, 1), "ms": round(med * 1e3, 3),
                        "rounds_gpx_s": [round(px / s / 1e9, 1) for s in secs[p]], "max_diff_vs_strict": d, "kernel": kern[p]}
        res[case] = entry
        del outs
    eng.set_precision("strict")
    eng.close()
    print(json.dumps({"tool": "precision_rate", "frames": args.frames, "size": f"{w}x{h}", "pix_fmt": "yuv420p10le",
                      "lut": args.lut, "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                      "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
