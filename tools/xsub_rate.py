#!/usr/bin/env python3
"""tools/xsub_rate.py -- the fused YUV pass with a chroma subsampling change against the same-layout pass.

The batch: `frames.make_yuv` frames tiled to 64 UHD 10-bit frames on the device, `cube.log709_lattice(33)`, tetrahedral, strict
precision; content natural and sigma-16 noise.  Paths timed per content:
  420to422, 422to420, 420to444   lutr_apply_yuv_xsub on the vector kernel (k_yuv_xsub_vec)
  same_tile                      yuv420p10le -> yuv420p10le on the default path (auto: the LDS-window tile kernels at this size)
  same_vec                       the same call on the global-gather vector kernel k_yuv_vec -- a child process with
                                 LUTR_NO_TILE2=1, because the library reads its knobs once per process
In-process paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each;
the figure is the median round.  Prints one JSON line: Gpx/s per path, each cross path over same_vec, and `roofline_bytes_px`
from the real plane sizes (420p10 -> 422p10: 3 + 4 = 7 B/px).

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/xsub_rate.py --steps 10 --warmup 3 --rounds 3
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
from lut_renderer_amd.engine import LutEngine, parse_pix_fmt  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
LAYOUTS = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}
#: name -> (input layout, output layout)
CROSS = {"420to422": ("420", "422"), "422to420": ("422", "420"), "420to444": ("420", "444")}


def batch(eng, dist, lay, nframes, unique):
    planes = [[], [], []]
    for k in range(unique):
        f = frames.make_yuv(dist, W, H, 10, *LAYOUTS[lay], k=k)
        for i in range(3):
            planes[i].append(torch.from_numpy(np.ascontiguousarray(f[i]).view(np.int16)))
    reps = (nframes + unique - 1) // unique
    return [torch.stack(p).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for p in planes]


def bytes_px(fin, fout):
    """Bytes per luma pixel read and written: the planes' real sizes."""
    total = 0
    for name in (fin, fout):
        f = parse_pix_fmt(name)
        total += sum(a * b for a, b in (f.plane_shape(i, W, H) for i in range(3))) * (1 if f.depth <= 8 else 2)
    return total / (W * H)


def time_paths(eng, paths, args):
    """paths: name -> (src, pix_fmt, out_pix_fmt).  Returns name -> {gpx_s, rounds_gpx_s, kernel, roofline_bytes_px}."""
    outs = {}
    for n, (src, fi, fo) in paths.items():
        f = parse_pix_fmt(fo)
        outs[n] = [torch.empty((args.frames,) + f.plane_shape(i, W, H), dtype=torch.int16, device=eng.device) for i in range(3)]
    kern = {}
    for n, (src, fi, fo) in paths.items():
        for _ in range(args.warmup):
            eng.apply_yuv(src, outs[n], pix_fmt=fi, out_pix_fmt=fo, interp="tetrahedral")
        kern[n] = eng.last_kernel
    torch.cuda.synchronize()
    secs = {n: [] for n in paths}
    for _ in range(args.rounds):
        for n, (src, fi, fo) in paths.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                eng.apply_yuv(src, outs[n], pix_fmt=fi, out_pix_fmt=fo, interp="tetrahedral")
            ev1.record()
            torch.cuda.synchronize()
            secs[n].append(ev0.elapsed_time(ev1) / 1e3 / args.steps)
    px = args.frames * W * H
    return {n: {"gpx_s": round(px / statistics.median(s) / 1e9, 1), "rounds_gpx_s": [round(px / v / 1e9, 1) for v in s],
                "kernel": kern[n], "roofline_bytes_px": bytes_px(paths[n][1], paths[n][2])} for n, s in secs.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10, help="launches per timed round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches of each path before the first round")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds over the paths")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--unique", type=int, default=4, help="distinct synthetic frames tiled to --frames")
    ap.add_argument("--child", action="store_true", help="(internal) time same_vec only and print its JSON")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("xsub_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    res = {}
    for dist in DISTS:
        src = {lay: batch(eng, dist, lay, args.frames, args.unique) for lay in ("420", "422")}
        if args.child:
            res[dist] = time_paths(eng, {"same_vec": (src["420"], "yuv420p10le", "yuv420p10le")}, args)
            continue
        paths = {name: (src[a], f"yuv{a}p10le", f"yuv{b}p10le") for name, (a, b) in CROSS.items()}
        paths["same_tile"] = (src["420"], "yuv420p10le", "yuv420p10le")
        res[dist] = time_paths(eng, paths, args)
        del paths, src
        torch.cuda.empty_cache()
    eng.close()
    if args.child:
        print(json.dumps(res))
        return
    # the vector-kernel baseline: a process of its own (knobs are read once per process)
    cmd = [sys.executable, __file__, "--child", "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--rounds", str(args.rounds), "--frames", str(args.frames), "--unique", str(args.unique)]
    child = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, LUTR_NO_TILE2="1"), timeout=600)
    if child.returncode != 0:
        raise SystemExit(f"child run failed ({child.returncode}):\n{child.stdout}\n{child.stderr}")
    vec = json.loads(child.stdout.strip().splitlines()[-1])
    for dist in DISTS:
        res[dist]["same_vec"] = vec[dist]["same_vec"]
        base = res[dist]["same_vec"]["gpx_s"]
        for name in CROSS:
            res[dist][f"{name}_vs_same_vec"] = round(res[dist][name]["gpx_s"] / base, 3)
    print(json.dumps({"tool": "xsub_rate", "frames": args.frames, "size": f"{W}x{H}", "depth": 10, "lut": 33,
                      "interp": "tetrahedral", "precision": "strict", "steps": args.steps, "warmup": args.warmup,
                      "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
