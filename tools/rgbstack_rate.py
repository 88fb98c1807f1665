#!/usr/bin/env python3
"""tools/rgbstack_rate.py -- the stage stack on RGB sources: the RGB stack kernel against the dedicated RGB
kernels on the one list they serve, its two table placements, and the two launches a user needs without it.

The batch: `frames.make_rgb` frames tiled to 64 UHD frames on the device; lattice 33^3 (`cube.log709_lattice(33)`), tetrahedral,
strict precision; 1D LUT = a 1024-point gamma curve, linear; the CDL of tools/stack_rate.py (saturation 0.6); the matrix of
tests/golden/matrix/bt2020_to_709.spimtx; content natural and sigma-16 noise.  Three cases:
      gbrp10le -> yuv422p10le      gbrp10le -> gbrp10le      rgb48le -> yuv420p10le
Paths timed per content and case, all in ONE process (LUTR_STACK_LDS is read at every launch):
  (a) the price of the uniform step loop: the stack kernel on [lut3d] and the dedicated kernel in the same run
      s_l3d / ref                      k_rgb2yuv_vec (apply_rgb_to_yuv) or k_rgb_vec (apply_rgb), both under variant vec_global
  (b) the lists nothing else serves in one pass, tables in LDS and in global memory
      s_l1d_cdl_l3d_lds / _global      [lut1d, cdl, lut3d]
      s_l1d_mtx_l3d_lds / _global      [lut1d, matrix, lut3d]
  (c) [cdl, lut3d] (default placement) against the route a user has without the feature (a YUV destination only; other bits:
      a time yardstick)
      s_cdl_l3d / two_calls            apply_rgb_to_yuv(lut=False) -> yuv444p10le, then apply_yuv(cdl=) -> out
Paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is
the median round.  Prints one JSON line (and writes it to `--out` when given): Gpx/s and ms per path and the ratios.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 900 python tools/rgbstack_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/rgbstack_rate.json
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from lut_renderer_amd import cube, frames  # noqa: E402
from lut_renderer_amd.cdl import Cdl  # noqa: E402
from lut_renderer_amd.engine import LutEngine, parse_pix_fmt  # noqa: E402
from lut_renderer_amd.rgbmatrix import read_rgb_matrix  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
CASES = (("gbrp10le", "yuv422p10le"), ("gbrp10le", "gbrp10le"), ("rgb48le", "yuv420p10le"))
MID = "yuv444p10le"
GRADE = dict(slope=(1.3, 1.25, 1.1), offset=(-0.08, 0.0, 0.05), power=(0.8, 1.0, 1.2), saturation=0.6)


def batch(dev, dist, nframes, unique, packed):
    """64 frames of gbrp10le planes (G, B, R), or of rgb48le images holding the same 10-bit codes scaled to 16 bit."""
    fs = [frames.make_rgb(dist, W, H, 10, k=k) for k in range(unique)]
    reps = (nframes + unique - 1) // unique
    if packed:
        img = [torch.from_numpy(np.stack([(f[2].astype(np.uint32) * 65535 // 1023).astype(np.uint16),
                                          (f[0].astype(np.uint32) * 65535 // 1023).astype(np.uint16),
                                          (f[1].astype(np.uint32) * 65535 // 1023).astype(np.uint16)], axis=-1).view(np.int16)) for f in fs]
        return torch.stack(img).to(dev).repeat(reps, 1, 1, 1)[:nframes].contiguous()
    return [torch.stack([torch.from_numpy(np.ascontiguousarray(f[i]).view(np.int16)) for f in fs]).to(dev).repeat(reps, 1, 1)[:nframes]
            .contiguous() for i in range(3)]


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
                "rounds_ms": [round(v * 1e3, 3) for v in s], "kernel": kern[n]} for n, s in secs.items()}


def placed(knob, call):
    """`call` with LUTR_STACK_LDS = knob for the launch (the launcher reads it every time)."""
    def run():
        os.environ["LUTR_STACK_LDS"] = knob
        try:
            return call()
        finally:
            del os.environ["LUTR_STACK_LDS"]
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
        raise SystemExit("rgbstack_rate.py needs a GPU")
    ones = np.ones(3, np.float32)
    lut = cube.CubeLut(33, ones, cube.log709_lattice(33))
    x = np.linspace(0.0, 1.0, 1024)
    l1 = cube.Lut1D(np.tile((x ** (1 / 2.2)).astype(np.float32), (3, 1)), ones)
    grade = Cdl(**GRADE)
    gamut = read_rgb_matrix(ROOT / "tests" / "golden" / "matrix" / "bt2020_to_709.spimtx")
    # st: the stack calls; vec: the dedicated kernels under vec_global; two: the two-call route
    st, vec, two = (LutEngine(0) for _ in range(3))
    for e in (st, vec, two):
        e.set_lut(lut)
    vec.set_variant("vec_global")
    st.set_lut1d(l1, "linear")
    dev = st.device
    res = {}
    for dist in DISTS:
        res[dist] = {}
        for src_fmt, out_fmt in CASES:
            packed = src_fmt == "rgb48le"
            depth = 16 if packed else 10
            src = batch(dev, dist, args.frames, args.unique, packed)
            out = empty(dev, out_fmt, args.frames)
            to_rgb = out_fmt.startswith("gbrp")
            names = dict(pix_fmt=src_fmt, out_pix_fmt=out_fmt)

            def stack(stages, cdl=None, mtx=None):
                return lambda: st.apply_rgb_stack(src, out, stages=stages, cdl=cdl, rgb_matrix=mtx, **names)

            sk = lambda: st.last_kernel                                                   # noqa: E731
            if to_rgb:
                ref = lambda: vec.apply_rgb(src, out, depth=depth, interp="tetrahedral")  # noqa: E731
            else:
                ref = lambda: vec.apply_rgb_to_yuv(src, out, interp="tetrahedral", **names)   # noqa: E731
            paths = {
                "s_l3d": (stack("lut3d"), sk),
                "ref": (ref, lambda: vec.last_kernel),
                "s_l1d_cdl_l3d_lds": (placed("1", stack("lut1d,cdl,lut3d", grade)), sk),
                "s_l1d_cdl_l3d_global": (placed("0", stack("lut1d,cdl,lut3d", grade)), sk),
                "s_l1d_mtx_l3d_lds": (placed("1", stack("lut1d,matrix,lut3d", None, gamut)), sk),
                "s_l1d_mtx_l3d_global": (placed("0", stack("lut1d,matrix,lut3d", None, gamut)), sk),
                "s_cdl_l3d": (stack("cdl,lut3d", grade), sk),
            }
            mid = None
            if not to_rgb:
                mid = empty(dev, MID, args.frames)

                def two_calls():
                    two.apply_rgb_to_yuv(src, mid, pix_fmt=src_fmt, out_pix_fmt=MID, lut=False)
                    two.apply_yuv(mid, out, pix_fmt=MID, out_pix_fmt=out_fmt, interp="tetrahedral", cdl=grade, matrix_in="smpte170m")

                first = []
                paths["two_calls"] = (lambda: (two_calls(), first.append(two.last_kernel))[0], lambda: "k_rgb2yuv_vec<nolut>, then " + first[-1])
            r = time_paths(paths, args)
            r["s_l3d_time_vs_ref"] = round(r["s_l3d"]["ms"] / r["ref"]["ms"], 3)
            for n in ("s_l1d_cdl_l3d", "s_l1d_mtx_l3d"):
                r[f"{n}_lds_time_vs_global"] = round(r[n + "_lds"]["ms"] / r[n + "_global"]["ms"], 3)
            if not to_rgb:
                r["s_cdl_l3d_time_vs_two_calls"] = round(r["s_cdl_l3d"]["ms"] / r["two_calls"]["ms"], 3)
            res[dist][f"{src_fmt}->{out_fmt}"] = r
            del paths, out, src, mid
            torch.cuda.empty_cache()
    for e in (st, vec, two):
        e.close()
    line = json.dumps({"tool": "rgbstack_rate", "frames": args.frames, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "lut1d": {"rows": 1024, "interp1d": "linear"}, "cdl": GRADE,
                       "matrix": "bt2020_to_709.spimtx", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
