#!/usr/bin/env python3
"""tools/v210_rate.py -- the v210 path against the planar vector kernels on the same samples.

The batch: synthetic 10-bit 4:2:2 frames (`frames.make_yuv`) tiled to 64 UHD frames on the device, `cube.log709_lattice(33)`,
tetrahedral, strict precision; content natural and sigma-16 noise.  Paths timed per content:
  v210_to_v210      v210 -> v210            k_yuv_v210_vec<1,1,1,0,..>
  v210_to_422p10    v210 -> yuv422p10le     k_yuv_v210_vec<1,1,0,0,..>
  422p10_to_v210    yuv422p10le -> v210     k_yuv_v210_vec<1,0,1,0,..>
  yuv422p10_vec     yuv422p10le -> yuv422p10le under set_variant("vec_global"): k_yuv_vec -- the yardstick of the three above
  v210_to_420p10    v210 -> yuv420p10le     k_yuv_v210_vec<1,1,0,1,..>
  422p10_to_420p10  yuv422p10le -> yuv420p10le under set_variant("vec_global"): k_yuv_xsub_vec -- its yardstick
A v210 source is `v210.to_v210` of the planar one, so each pair of paths sees the same samples and the same arithmetic per pixel;
a v210 side moves 2.67 bytes per pixel where the planar one moves 4.  Both yardsticks predate the v210 kernels.  All paths run
in one process, timed in alternating rounds with HIP events around `--steps` launches,
after `--warmup` launches of each; the figure is the median round.  Prints one JSON line (and writes it to --out when given):
Gpx/s per path, the ratios against the yardsticks, `bytes_px` from the real buffer sizes and the fraction of the HBM peak.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/v210_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/v210_rate.json
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
from lut_renderer_amd.engine import LutEngine, yuv_side  # noqa: E402
from lut_renderer_amd.v210 import to_v210  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
HBM_PEAK_GB_S = 8000.0          # MI355X: 8 TB/s HBM3E
#: name -> (source format, output format, yardstick path or None)
PATHS = {
    "v210_to_v210": ("v210", "v210", "yuv422p10_vec"),
    "v210_to_422p10": ("v210", "yuv422p10le", "yuv422p10_vec"),
    "422p10_to_v210": ("yuv422p10le", "v210", "yuv422p10_vec"),
    "yuv422p10_vec": ("yuv422p10le", "yuv422p10le", None),
    "v210_to_420p10": ("v210", "yuv420p10le", "422p10_to_420p10"),
    "422p10_to_420p10": ("yuv422p10le", "yuv420p10le", None),
}


def planar_source(eng, dist, depth, nframes, unique):
    """`nframes` device frames, three planes (Y, Cb, Cr): `unique` distinct synthetic frames, tiled."""
    reps = (nframes + unique - 1) // unique
    fs = [frames.make_yuv(dist, W, H, depth, 1, 0, k=k) for k in range(unique)]
    conv = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a))  # noqa: E731
    return [torch.stack([conv(x[i]) for x in fs]).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for i in range(3)]


def out_planes(eng, fout, nframes):
    f = yuv_side(fout)
    dt = torch.int32 if fout == "v210" else (torch.uint8 if f.depth <= 8 else torch.int16)
    return [torch.zeros((nframes,) + f.plane_shape(i, W, H), dtype=dt, device=eng.device) for i in range(f.nplanes)]


def bytes_px(src, out):
    """Bytes per luma pixel read and written: the buffers' real sizes."""
    return sum(t.numel() * t.element_size() for t in list(src) + list(out)) / (src[0].shape[0] * W * H)


def call(eng, src, out, fin, fout, yardstick):
    if not yardstick:
        eng.apply_yuv(src, out, pix_fmt=fin, out_pix_fmt=fout, interp="tetrahedral", width=W if "v210" in (fin, fout) else None)
        return
    eng.set_variant("vec_global")
    try:
        eng.apply_yuv(src, out, pix_fmt=fin, out_pix_fmt=fout, interp="tetrahedral")
    finally:
        eng.set_variant("auto")


def time_paths(eng, dist, args):
    planar = {10: planar_source(eng, dist, 10, args.frames, args.unique)}
    srcs, outs, kern = {}, {}, {}
    for n, (fi, fo, base) in PATHS.items():
        f = yuv_side(fi)
        srcs[n] = planar[f.depth] if f.nplanes == 3 else [to_v210(planar[f.depth], W).contiguous()]
        outs[n] = out_planes(eng, fo, args.frames)
    for n, (fi, fo, base) in PATHS.items():
        for _ in range(args.warmup):
            call(eng, srcs[n], outs[n], fi, fo, base is None)
        kern[n] = eng.last_kernel
    torch.cuda.synchronize()
    secs = {n: [] for n in PATHS}
    for _ in range(args.rounds):
        for n, (fi, fo, base) in PATHS.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                call(eng, srcs[n], outs[n], fi, fo, base is None)
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
        raise SystemExit("v210_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    res = {}
    for dist in DISTS:
        res[dist] = time_paths(eng, dist, args)
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps({"tool": "v210_rate", "frames": args.frames, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "hbm_peak_gb_s": HBM_PEAK_GB_S, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
