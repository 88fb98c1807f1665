#!/usr/bin/env python3
"""tools/rgb2yuv_rate.py -- the fused pass for RGB sources with a YUV output against a YUV pass of the same size.

The batch: synthetic frames (`frames.make_rgb` / `frames.make_yuv`) tiled to 64 UHD frames on the device,
`cube.log709_lattice(33)`, tetrahedral, strict precision; content natural and sigma-16 noise.  Paths timed per content:
  gbrp10_to_420p10    gbrp10le -> yuv420p10le   k_rgb2yuv_vec (9 B/px)
  yuv444p10_to_420p10 yuv444p10le -> yuv420p10le k_yuv_xsub_vec: the yardstick -- same bytes in, same bytes out, the same
                      gather, plus a YUV -> RGB stage the RGB path does not have
  rgb24_to_420p       rgb24 -> yuv420p          k_rgb2yuv_vec (4.5 B/px)
  yuv444p_to_420p     yuv444p -> yuv420p        k_yuv_xsub_vec, its yardstick
  rgb48_to_420p10     rgb48le -> yuv420p10le    k_rgb2yuv_vec (9 B/px)
All paths run in one process, timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches
of each; the figure is the median round.  Prints one JSON line (and writes it to --out when given): Gpx/s per path, the two
ratios against the yardsticks, `bytes_px` from the real buffer sizes and the fraction of the HBM peak those bytes amount to.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/rgb2yuv_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/rgb2yuv_rate.json
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
from lut_renderer_amd.engine import LutEngine, parse_pix_fmt, parse_rgb_source  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
HBM_PEAK_GB_S = 8000.0          # MI355X: 8 TB/s HBM3E
#: name -> (pix_fmt, out_pix_fmt, yardstick path or None)
PATHS = {
    "gbrp10_to_420p10": ("gbrp10le", "yuv420p10le", "yuv444p10_to_420p10"),
    "yuv444p10_to_420p10": ("yuv444p10le", "yuv420p10le", None),
    "rgb24_to_420p": ("rgb24", "yuv420p", "yuv444p_to_420p"),
    "yuv444p_to_420p": ("yuv444p", "yuv420p", None),
    "rgb48_to_420p10": ("rgb48le", "yuv420p10le", None),
}


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def source(eng, dist, pix_fmt, nframes, unique):
    """`nframes` device frames of `pix_fmt`: `unique` distinct synthetic frames, tiled."""
    reps = (nframes + unique - 1) // unique
    rgb = parse_rgb_source(pix_fmt)
    if rgb is None:
        f = parse_pix_fmt(pix_fmt)
        fs = [frames.make_yuv(dist, W, H, f.depth, f.csx, f.csy, k=k) for k in range(unique)]
        return [torch.stack([_dev(x[i]) for x in fs]).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for i in range(3)]
    fs = [frames.make_rgb(dist, W, H, rgb.depth, k=k) for k in range(unique)]          # (G, B, R)
    if not rgb.packed:
        return [torch.stack([_dev(x[i]) for x in fs]).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for i in range(3)]
    img = torch.stack([_dev(np.stack([x[2], x[0], x[1]], axis=-1)) for x in fs])         # R, G, B interleaved
    return img.to(eng.device).repeat(reps, 1, 1, 1)[:nframes].contiguous()


def bytes_px(fin, fout):
    """Bytes per luma pixel read and written: the buffers' real sizes."""
    rgb = parse_rgb_source(fin)
    if rgb is not None:
        total = rgb.frame_bytes(W, H)
    else:
        f = parse_pix_fmt(fin)
        total = sum(a * b for a, b in (f.plane_shape(i, W, H) for i in range(3))) * (1 if f.depth <= 8 else 2)
    f = parse_pix_fmt(fout)
    total += sum(a * b for a, b in (f.plane_shape(i, W, H) for i in range(3))) * (1 if f.depth <= 8 else 2)
    return total / (W * H)


def call(eng, src, out, fin, fout):
    if parse_rgb_source(fin) is not None:
        eng.apply_rgb_to_yuv(src, out, pix_fmt=fin, out_pix_fmt=fout, interp="tetrahedral", matrix_out="bt709")
    else:
        eng.apply_yuv(src, out, pix_fmt=fin, out_pix_fmt=fout, interp="tetrahedral")


def time_paths(eng, dist, args):
    srcs, outs, kern = {}, {}, {}
    for n, (fi, fo, _) in PATHS.items():
        srcs[n] = source(eng, dist, fi, args.frames, args.unique)
        f = parse_pix_fmt(fo)
        dt = torch.uint8 if f.depth <= 8 else torch.int16
        outs[n] = [torch.empty((args.frames,) + f.plane_shape(i, W, H), dtype=dt, device=eng.device) for i in range(3)]
    for n, (fi, fo, _) in PATHS.items():
        for _ in range(args.warmup):
            call(eng, srcs[n], outs[n], fi, fo)
        kern[n] = eng.last_kernel
    torch.cuda.synchronize()
    secs = {n: [] for n in PATHS}
    for _ in range(args.rounds):
        for n, (fi, fo, _) in PATHS.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                call(eng, srcs[n], outs[n], fi, fo)
            ev1.record()
            torch.cuda.synchronize()
            secs[n].append(ev0.elapsed_time(ev1) / 1e3 / args.steps)
    px = args.frames * W * H
    res = {}
    for n, s in secs.items():
        gpx = px / statistics.median(s) / 1e9
        bpp = bytes_px(PATHS[n][0], PATHS[n][1])
        res[n] = {"gpx_s": round(gpx, 1), "rounds_gpx_s": [round(px / v / 1e9, 1) for v in s], "kernel": kern[n],
                  "bytes_px": bpp, "hbm_fraction": round(gpx * bpp / HBM_PEAK_GB_S, 3)}
    for n, (_, _, base) in PATHS.items():
        if base:
            res[f"{n}_vs_{base}"] = round(res[n]["gpx_s"] / res[base]["gpx_s"], 3)
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
        raise SystemExit("rgb2yuv_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    res = {}
    for dist in DISTS:
        res[dist] = time_paths(eng, dist, args)
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps({"tool": "rgb2yuv_rate", "frames": args.frames, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "hbm_peak_gb_s": HBM_PEAK_GB_S, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
