#!/usr/bin/env python3
"""tools/bn_rate.py -- blue-noise dither fused into the LUT pass against error diffusion and against no dither.

The batch: synthetic natural `yuv420p10le` frames (`frames.make_yuv`) tiled to 64 UHD frames on the device,
`cube.log709_lattice(33)`, tetrahedral, strict precision.  Two outputs, `yuv420p` (the 10 -> 8 bit delivery conversion, where banding
shows) and `yuv422p10le`.  Legs timed per output:
  blue_noise        dither="blue_noise", variant auto           k_yuv_bn_vec
  error_diffusion   dither="error_diffusion", variant auto      k_yuv_float[_xsub] + k_dither_ed (scratch, one workgroup per plane)
  none_vec_global   dither="none", variant vec_global           k_yuv_vec (equal layouts) / k_yuv_xsub_vec
All legs run in one process, timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of
each; the figure is the median round, the spread is (max - min) / median over the rounds.  Prints one JSON line (and writes it to
--out when given): milliseconds per launch and Gpx/s per leg, `bn_vs_ed` (blue-noise rate over error-diffusion rate; at least 4
is asked for) and `bn_vs_none` (blue-noise rate over the undithered vector kernel's; at least 0.75 for yuv420p and 0.85 for
yuv422p10le), and whether each bound is met.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/bn_rate.py --steps 10 --warmup 3 --rounds 5 --out profiles/bn_dither_rate.json
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
SRC = "yuv420p10le"
#: output format -> the least bn_vs_none asked for
OUTPUTS = {"yuv420p": 0.75, "yuv422p10le": 0.85}
MIN_BN_VS_ED = 4.0
#: leg -> (variant, dither)
LEGS = {
    "blue_noise": ("auto", "blue_noise"),
    "error_diffusion": ("auto", "error_diffusion"),
    "none_vec_global": ("vec_global", "none"),
}


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def source(eng, nframes, unique):
    """`nframes` device frames of SRC: `unique` distinct synthetic frames, tiled."""
    reps = (nframes + unique - 1) // unique
    f = parse_pix_fmt(SRC)
    fs = [frames.make_yuv("natural", W, H, f.depth, f.csx, f.csy, k=k) for k in range(unique)]
    return [torch.stack([_dev(x[i]) for x in fs]).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for i in range(3)]


def planes(eng, name, nframes):
    f = parse_pix_fmt(name)
    dt = torch.uint8 if f.depth <= 8 else torch.int16
    return [torch.empty((nframes,) + f.plane_shape(i, W, H), dtype=dt, device=eng.device) for i in range(3)]


def call(eng, src, dst, out_fmt, leg):
    variant, dither = LEGS[leg]
    eng.set_variant(variant)
    eng.apply_yuv(src, dst, pix_fmt=SRC, out_pix_fmt=out_fmt, interp="tetrahedral", dither=dither)


def time_legs(eng, src, out_fmt, args):
    dst = planes(eng, out_fmt, args.frames)
    kern = {}
    for leg in LEGS:
        for _ in range(args.warmup):
            call(eng, src, dst, out_fmt, leg)
        kern[leg] = eng.last_kernel
    torch.cuda.synchronize()
    secs = {leg: [] for leg in LEGS}
    for _ in range(args.rounds):
        for leg in LEGS:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                call(eng, src, dst, out_fmt, leg)
            ev1.record()
            torch.cuda.synchronize()
            secs[leg].append(ev0.elapsed_time(ev1) / 1e3 / args.steps)
    px = args.frames * W * H
    res = {}
    for leg, s in secs.items():
        med = statistics.median(s)
        res[leg] = {"ms": round(med * 1e3, 3), "rounds_ms": [round(v * 1e3, 3) for v in s],
                    "spread": round((max(s) - min(s)) / med, 4), "gpx_s": round(px / med / 1e9, 1), "kernel": kern[leg]}
    res["bn_vs_ed"] = round(res["error_diffusion"]["ms"] / res["blue_noise"]["ms"], 3)
    res["bn_vs_none"] = round(res["none_vec_global"]["ms"] / res["blue_noise"]["ms"], 3)
    res["bn_vs_ed_required"], res["bn_vs_none_required"] = MIN_BN_VS_ED, OUTPUTS[out_fmt]
    res["met"] = bool(res["bn_vs_ed"] >= MIN_BN_VS_ED and res["bn_vs_none"] >= OUTPUTS[out_fmt])
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10, help="launches per timed round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches of each leg before the first round")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds over the legs")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--unique", type=int, default=4, help="distinct synthetic frames tiled to --frames")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bn_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    src = source(eng, args.frames, args.unique)
    res = {}
    for out_fmt in OUTPUTS:
        res[out_fmt] = time_legs(eng, src, out_fmt, args)
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps({"tool": "bn_rate", "frames": args.frames, "size": f"{W}x{H}", "source": SRC, "content": "natural", "lut": 33,
                       "interp": "tetrahedral", "precision": "strict", "steps": args.steps, "warmup": args.warmup,
                       "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
