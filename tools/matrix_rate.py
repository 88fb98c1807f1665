#!/usr/bin/env python3
"""tools/matrix_rate.py -- the RGB matrix stage of the stage stack: the matrix form of the stack kernel against
the plain form on the same list without the matrix, and against the two engine calls a user needs without the stage.

The batch: `frames.make_yuv` frames tiled to 64 UHD yuv420p10le frames on the device; lattice 33^3 (`cube.log709_lattice(33)`),
tetrahedral, strict precision; 1D LUT = a 1024-point gamma curve, linear; the matrix = BT.2020 -> BT.709 primaries with a small
offset; content natural and sigma-16 noise; yuv420p10le and yuv422p10le out.  Paths timed per content and output layout, all in
ONE process on the same source:
  (a) the matrix form and, on the same list without the matrix, the plain form
      m_l1d_mtx_l3d / s_l1d_l3d        [lut1d, matrix, lut3d] / [lut1d, lut3d]
      m_mtx_l3d / s_l3d                [matrix, lut3d] / [lut3d]
  (b) the two engine calls a user needs today, through yuv444p10le, with a pass of their own on the 4:4:4 frames in between (not
      timed: the figure is a lower bound of what they pay; other bits, a time yardstick only)
      two_l1d_then_l3d                 apply_yuv_lut1d(interp=None) -> 444, then apply_yuv -> out
      two_copy_then_l3d                apply_yuv_stack([cdl], identity) -> 444, then apply_yuv -> out
Paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is
the median round.  Prints one JSON line (and writes it to `--out` when given): Gpx/s and ms per path and the ratios.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/matrix_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/matrix_rate.json
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from lut_renderer_amd import cube  # noqa: E402
from lut_renderer_amd.cdl import Cdl  # noqa: E402
from lut_renderer_amd.engine import LutEngine  # noqa: E402
from lut_renderer_amd.rgbmatrix import RgbMatrix  # noqa: E402
from tools.stack_rate import DISTS, FMT, H, MID, OUTS, W, batch, empty, time_paths  # noqa: E402

MATRIX = dict(m=(1.6605, -0.5876, -0.0728, -0.1246, 1.1329, -0.0083, -0.0182, -0.1006, 1.1187), offset=(0.01, 0.0, -0.005))


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
        raise SystemExit("matrix_rate.py needs a GPU")
    ones = np.ones(3, np.float32)
    lut = cube.CubeLut(33, ones, cube.log709_lattice(33))
    x = np.linspace(0.0, 1.0, 1024)
    l1 = cube.Lut1D(np.tile((x ** (1 / 2.2)).astype(np.float32), (3, 1)), ones)
    mtx = RgbMatrix(**MATRIX)
    # st: the stack calls, both forms; ded: the dedicated calls of the two-call paths
    st, ded = LutEngine(0), LutEngine(0)
    for e in (st, ded):
        e.set_lut(lut)
        e.set_lut1d(l1, "linear")
    dev = st.device
    res = {}
    for dist in DISTS:
        src = batch(dev, dist, args.frames, args.unique)
        mid = empty(dev, MID, args.frames)
        res[dist] = {}
        for out_fmt in OUTS:
            out = empty(dev, out_fmt, args.frames)
            names = dict(pix_fmt=FMT, out_pix_fmt=out_fmt)

            def stack(stages, m=None):
                return lambda: st.apply_yuv_stack(src, out, stages=stages, rgb_matrix=m, **names)

            def two_l1d_then_l3d():
                ded.apply_yuv_lut1d(src, mid, pix_fmt=FMT, out_pix_fmt=MID, interp=None)
                ded.apply_yuv(mid, out, pix_fmt=MID, out_pix_fmt=out_fmt, interp="tetrahedral")

            def two_copy_then_l3d():
                ded.apply_yuv_stack(src, mid, pix_fmt=FMT, out_pix_fmt=MID, stages="cdl", cdl=Cdl())
                ded.apply_yuv(mid, out, pix_fmt=MID, out_pix_fmt=out_fmt, interp="tetrahedral")

            sk = lambda: st.last_kernel                                                   # noqa: E731
            paths = {
                "m_l1d_mtx_l3d": (stack("lut1d,matrix,lut3d", mtx), sk),
                "s_l1d_l3d": (stack("lut1d,lut3d"), sk),
                "m_mtx_l3d": (stack("matrix,lut3d", mtx), sk),
                "s_l3d": (stack("lut3d"), sk),
                "two_l1d_then_l3d": (two_l1d_then_l3d, lambda: "k_yuv_l1d_vec, then " + ded.last_kernel),
                "two_copy_then_l3d": (two_copy_then_l3d, lambda: "k_yuv_stack_vec[cdl], then " + ded.last_kernel),
            }
            r = time_paths(paths, args)
            for a, b in (("m_l1d_mtx_l3d", "s_l1d_l3d"), ("m_mtx_l3d", "s_l3d"), ("m_l1d_mtx_l3d", "two_l1d_then_l3d"),
                         ("m_mtx_l3d", "two_copy_then_l3d")):
                r[f"{a}_time_vs_{b}"] = round(r[a]["ms"] / r[b]["ms"], 3)
            res[dist][out_fmt] = r
            del paths, out
        del src, mid
        torch.cuda.empty_cache()
    for e in (st, ded):
        e.close()
    line = json.dumps({"tool": "matrix_rate", "frames": args.frames, "size": f"{W}x{H}", "pix_fmt": FMT, "lut": 33,
                       "interp": "tetrahedral", "precision": "strict", "lut1d": {"rows": 1024, "interp1d": "linear"}, "matrix": MATRIX,
                       "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
