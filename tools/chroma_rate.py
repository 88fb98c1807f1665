#!/usr/bin/env python3
"""tools/chroma_rate.py -- sited chroma resampling against the replicating chroma contract, on one batch.

The batch: `frames.make_yuv` frames tiled to 64 UHD yuv420p10le frames on the device, `cube.log709_lattice(33)`, tetrahedral,
strict precision; content natural and sigma-16 noise.  Paths timed per content:
  replicate       chroma_loc=None on the default path (auto: the LDS-window tile kernels at this size)
  replicate_vec   chroma_loc=None on the global-gather vector kernel -- a child process with LUTR_NO_TILE2=1, because the
                  library reads its knobs once per process
  left, center, topleft   the sited kernels (lutr_sited.hip)
and 4:2:2 10-bit with `left` (`left_422`).  In-process paths are timed in alternating rounds with HIP events around `--steps`
launches, after `--warmup` launches of each; the figure is the median round.  Prints one JSON line with Gpx/s per path and
left / replicate_vec.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/chroma_rate.py --steps 10 --warmup 3 --rounds 3
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from lut_renderer_amd import cube, frames  # noqa: E402
from lut_renderer_amd.engine import LutEngine  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")


def batch(eng, dist, csy, nframes, unique):
    planes = [[], [], []]
    for k in range(unique):
        f = frames.make_yuv(dist, W, H, 10, 1, csy, k=k)
        for i in range(3):
            planes[i].append(torch.from_numpy(np.ascontiguousarray(f[i]).view(np.int16)))
    reps = (nframes + unique - 1) // unique
    return [torch.stack(p).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for p in planes]


def time_paths(eng, paths, args):
    """paths: name -> (src, pix_fmt, chroma_loc).  Returns name -> (median Gpx/s, rounds, kernel)."""
    outs = {n: [torch.empty_like(t) for t in src] for n, (src, _, _) in paths.items()}
    kern = {}
    for n, (src, fmt, loc) in paths.items():
        for _ in range(args.warmup):
            eng.apply_yuv(src, outs[n], pix_fmt=fmt, interp="tetrahedral", chroma_loc=loc)
        kern[n] = eng.last_kernel
    torch.cuda.synchronize()
    secs = {n: [] for n in paths}
    for _ in range(args.rounds):
        for n, (src, fmt, loc) in paths.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                eng.apply_yuv(src, outs[n], pix_fmt=fmt, interp="tetrahedral", chroma_loc=loc)
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
    ap.add_argument("--child", action="store_true", help="(internal) time replicate only and print its JSON")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("chroma_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    res = {}
    for dist in DISTS:
        src = batch(eng, dist, 1, args.frames, args.unique)
        if args.child:
            res[dist] = time_paths(eng, {"replicate_vec": (src, "yuv420p10le", None)}, args)
            continue
        paths = {"replicate": (src, "yuv420p10le", None)}
        for loc in ("left", "center", "topleft"):
            paths[loc] = (src, "yuv420p10le", loc)
        if dist == "natural":
            paths["left_422"] = (batch(eng, dist, 0, args.frames, args.unique), "yuv422p10le", "left")
        res[dist] = time_paths(eng, paths, args)
        del paths, src
        torch.cuda.empty_cache()
    eng.close()
    if args.child:
        print(json.dumps(res))
        return
    # the vector-kernel replicate baseline: a process of its own (knobs are read once per process)
    cmd = [sys.executable, __file__, "--child", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--rounds", str(args.rounds), "--frames", str(args.frames), "--unique", str(args.unique)]
    child = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, LUTR_NO_TILE2="1"), timeout=600)
    if child.returncode != 0:
        raise SystemExit(f"child run failed ({child.returncode}):\n{child.stdout}\n{child.stderr}")
    vec = json.loads(child.stdout.strip().splitlines()[-1])
    for dist in DISTS:
        res[dist]["replicate_vec"] = vec[dist]["replicate_vec"]
        base = res[dist]["replicate_vec"]["gpx_s"]
        res[dist]["left_vs_replicate_vec"] = round(res[dist]["left"]["gpx_s"] / base, 3)
    print(json.dumps({"tool": "chroma_rate", "frames": args.frames, "size": f"{W}x{H}", "pix_fmt": "yuv420p10le", "lut": 33,
                      "interp": "tetrahedral", "precision": "strict", "steps": args.steps, "warmup": args.warmup,
                      "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
