#!/usr/bin/env python3
"""tools/rgbf_rate.py -- the planar float RGB paths against the integer paths they are built like.

The batch: synthetic frames (`frames.make_rgb` at 16 bit; the float source is those codes / 65535) tiled to 64 UHD frames on the
device, `cube.log709_lattice(33)`, tetrahedral, strict precision; content natural and sigma-16 noise.  Paths timed per content:
  f32_to_f32       gbrpf32le -> gbrpf32le      k_rgbf_vec (24 B/px)
  f32_to_420p10    gbrpf32le -> yuv420p10le    k_rgbf2yuv_vec (15 B/px)
  gbrp16_vec       gbrp16le -> gbrp16le under set_variant("vec_global"): k_rgb_vec -- yardstick 1, the same gather at 12 B/px
  gbrp16_to_420p10 gbrp16le -> yuv420p10le     k_rgb2yuv_vec -- yardstick 2 (9 B/px)
All paths run in one process, timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches
of each; the figure is the median round.  Prints one JSON line (and writes it to --out when given): Gpx/s per path, the ratios
against the yardsticks, `bytes_px` from the real buffer sizes and the fraction of the HBM peak those bytes amount to.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/rgbf_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/rgbf_rate.json
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
HBM_PEAK_GB_S = 8000.0          # MI355X: 8 TB/s HBM3E
#: name -> (source is float, output format or None for the source's own, yardstick path or None)
PATHS = {
    "f32_to_f32": (True, None, "gbrp16_vec"),
    "gbrp16_vec": (False, None, None),
    "f32_to_420p10": (True, "yuv420p10le", "gbrp16_to_420p10"),
    "gbrp16_to_420p10": (False, "yuv420p10le", None),
}


def source(eng, dist, floating, nframes, unique):
    """`nframes` device frames, three planes (G, B, R): `unique` distinct synthetic frames, tiled."""
    reps = (nframes + unique - 1) // unique
    fs = [frames.make_rgb(dist, W, H, 16, k=k) for k in range(unique)]
    if floating:
        conv = lambda a: torch.from_numpy((a.astype(np.float32) / np.float32(65535)).astype(np.float32))  # noqa: E731
    else:
        conv = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16))  # noqa: E731
    return [torch.stack([conv(x[i]) for x in fs]).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for i in range(3)]


def out_planes(eng, floating, fout, nframes):
    if fout is None:
        return [torch.empty((nframes, H, W), dtype=torch.float32 if floating else torch.int16, device=eng.device) for _ in range(3)]
    f = parse_pix_fmt(fout)
    return [torch.empty((nframes,) + f.plane_shape(i, W, H), dtype=torch.int16, device=eng.device) for i in range(3)]


def bytes_px(src, out):
    """Bytes per luma pixel read and written: the buffers' real sizes."""
    return sum(t.numel() * t.element_size() for t in list(src) + list(out)) / (src[0].shape[0] * W * H)


def call(eng, src, out, floating, fout):
    if fout is not None:
        eng.apply_rgb_to_yuv(src, out, pix_fmt="gbrpf32le" if floating else "gbrp16le", out_pix_fmt=fout, interp="tetrahedral",
                             matrix_out="bt709")
    elif floating:
        eng.apply_rgb_float(src, out, interp="tetrahedral")
    else:
        eng.set_variant("vec_global")
        try:
            eng.apply_rgb(src, out, depth=16, interp="tetrahedral")
        finally:
            eng.set_variant("auto")


def time_paths(eng, dist, args):
    srcs, outs, kern = {}, {}, {}
    for n, (fl, fo, _) in PATHS.items():
        srcs[n] = source(eng, dist, fl, args.frames, args.unique)
        outs[n] = out_planes(eng, fl, fo, args.frames)
    for n, (fl, fo, _) in PATHS.items():
        for _ in range(args.warmup):
            call(eng, srcs[n], outs[n], fl, fo)
        kern[n] = eng.last_kernel
    torch.cuda.synchronize()
    secs = {n: [] for n in PATHS}
    for _ in range(args.rounds):
        for n, (fl, fo, _) in PATHS.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                call(eng, srcs[n], outs[n], fl, fo)
            ev1.record()
            torch.cuda.synchronize()
            secs[n].append(ev0.elapsed_time(ev1) / 1e3 / args.steps)
    px = args.frames * W * H
    res = {}
    for n, s in secs.items():
        gpx = px / statistics.median(s) / 1e9
        bpp = bytes_px(srcs[n], outs[n])
        res[n] = {"gpx_s": round(gpx, 1), "rounds_gpx_s": [round(px / v / 1e9, 1) for v in s], "kernel": kern[n],
                  "bytes_px": bpp, "gb_s": round(gpx * bpp, 1), "hbm_fraction": round(gpx * bpp / HBM_PEAK_GB_S, 3)}
    for n, (_, _, base) in PATHS.items():
        if base:
            res[f"{n}_vs_{base}"] = round(res[n]["gpx_s"] / res[base]["gpx_s"], 3)
            res[f"{n}_vs_{base}_bytes"] = round(res[n]["gb_s"] / res[base]["gb_s"], 3)
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
        raise SystemExit("rgbf_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    res = {}
    for dist in DISTS:
        res[dist] = time_paths(eng, dist, args)
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps({"tool": "rgbf_rate", "frames": args.frames, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "hbm_peak_gb_s": HBM_PEAK_GB_S, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
