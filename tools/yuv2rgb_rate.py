#!/usr/bin/env python3
"""tools/yuv2rgb_rate.py -- the fused pass for YUV sources with an RGB output against a YUV pass of the same size.

The batch: synthetic frames (`frames.make_yuv`) tiled to 64 UHD frames on the device, `cube.log709_lattice(33)`, tetrahedral,
strict precision; content natural and sigma-16 noise.  Paths timed per content:
  420p10_to_gbrp10   yuv420p10le -> gbrp10le     k_yuv2rgb_vec (9 B/px)
  420p10_to_rgb48    yuv420p10le -> rgb48le      k_yuv2rgb_vec (9 B/px)
  420p10_to_444p10   yuv420p10le -> yuv444p10le  k_yuv_xsub_vec: their yardstick -- same bytes in, same bytes out, the same
                     gather, plus an RGB -> YUV stage the RGB output does not have
  420p_to_rgb24      yuv420p -> rgb24            k_yuv2rgb_vec (4.5 B/px)
  420p_to_rgba       yuv420p -> rgba             k_yuv2rgb_vec (5.5 B/px)
  420p_to_444p       yuv420p -> yuv444p          k_yuv_xsub_vec, their yardstick
  420p10_to_rgb24    yuv420p10le -> rgb24        k_yuv2rgb_vec (6 B/px)
  420p10_to_444p     yuv420p10le -> yuv444p      k_yuv_xsub_vec, its yardstick
All paths run in one process, timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches
of each; the figure is the median round.  Prints one JSON line (and writes it to --out when given): Gpx/s per path, the ratios
against the yardsticks, `bytes_px` from the real buffer sizes and the fraction of the HBM peak those bytes amount to.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/yuv2rgb_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/yuv2rgb_rate.json
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
from lut_renderer_amd.formats import RgbSource, parse_rgb_out  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
HBM_PEAK_GB_S = 8000.0          # MI355X: 8 TB/s HBM3E
#: name -> (pix_fmt, out_pix_fmt, yardstick path or None)
PATHS = {
    "420p10_to_gbrp10": ("yuv420p10le", "gbrp10le", "420p10_to_444p10"),
    "420p10_to_rgb48": ("yuv420p10le", "rgb48le", "420p10_to_444p10"),
    "420p10_to_444p10": ("yuv420p10le", "yuv444p10le", None),
    "420p_to_rgb24": ("yuv420p", "rgb24", "420p_to_444p"),
    "420p_to_rgba": ("yuv420p", "rgba", "420p_to_444p"),
    "420p_to_444p": ("yuv420p", "yuv444p", None),
    "420p10_to_rgb24": ("yuv420p10le", "rgb24", "420p10_to_444p"),
    "420p10_to_444p": ("yuv420p10le", "yuv444p", None),
}


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def _is_rgb(name):
    return not name.startswith("yuv")


def source(eng, dist, pix_fmt, nframes, unique):
    """`nframes` device frames of the planar YUV `pix_fmt`: `unique` distinct synthetic frames, tiled."""
    reps = (nframes + unique - 1) // unique
    f = parse_pix_fmt(pix_fmt)
    fs = [frames.make_yuv(dist, W, H, f.depth, f.csx, f.csy, k=k) for k in range(unique)]
    return [torch.stack([_dev(x[i]) for x in fs]).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for i in range(3)]


def _planar_bytes(f):
    return sum(a * b for a, b in (f.plane_shape(i, W, H) for i in range(3))) * (1 if f.depth <= 8 else 2)


def bytes_px(fin, fout):
    """Bytes per luma pixel read and written: the buffers' real sizes."""
    total = _planar_bytes(parse_pix_fmt(fin))
    if _is_rgb(fout):
        o = parse_rgb_out(fout)
        total += o.frame_bytes(W, H) if isinstance(o, RgbSource) else _planar_bytes(o)
    else:
        total += _planar_bytes(parse_pix_fmt(fout))
    return total / (W * H)


def destination(eng, fout, nframes):
    if _is_rgb(fout):
        o = parse_rgb_out(fout)
        dt = torch.uint8 if o.depth <= 8 else torch.int16
        if isinstance(o, RgbSource):
            return torch.empty((nframes, H, W, o.ncomp), dtype=dt, device=eng.device)
        return [torch.empty((nframes, H, W), dtype=dt, device=eng.device) for _ in range(3)]
    f = parse_pix_fmt(fout)
    dt = torch.uint8 if f.depth <= 8 else torch.int16
    return [torch.empty((nframes,) + f.plane_shape(i, W, H), dtype=dt, device=eng.device) for i in range(3)]


def call(eng, src, out, fin, fout):
    if _is_rgb(fout):
        eng.apply_yuv_to_rgb(src, out, pix_fmt=fin, out_pix_fmt=fout, interp="tetrahedral")
    else:
        eng.apply_yuv(src, out, pix_fmt=fin, out_pix_fmt=fout, interp="tetrahedral")


def time_paths(eng, dist, args):
    by_fmt, outs, kern = {}, {}, {}
    for n, (fi, fo, _) in PATHS.items():
        if fi not in by_fmt:                                   # (the paths of one source format read the same frames)
            by_fmt[fi] = source(eng, dist, fi, args.frames, args.unique)
        outs[n] = destination(eng, fo, args.frames)
    for n, (fi, fo, _) in PATHS.items():
        for _ in range(args.warmup):
            call(eng, by_fmt[fi], outs[n], fi, fo)
        kern[n] = eng.last_kernel
    torch.cuda.synchronize()
    secs = {n: [] for n in PATHS}
    for _ in range(args.rounds):
        for n, (fi, fo, _) in PATHS.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                call(eng, by_fmt[fi], outs[n], fi, fo)
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
        raise SystemExit("yuv2rgb_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    res = {}
    for dist in DISTS:
        res[dist] = time_paths(eng, dist, args)
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps({"tool": "yuv2rgb_rate", "frames": args.frames, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "hbm_peak_gb_s": HBM_PEAK_GB_S, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
