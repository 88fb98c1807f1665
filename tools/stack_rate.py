#!/usr/bin/env python3
"""tools/stack_rate.py -- an ordered stack of lut1d / CDL / lut3d stages in one fused pass: the stack kernel on
stacks nothing else serves, against the dedicated kernels on the stacks they serve, and against the launches a user needs without it.

The batch: `frames.make_yuv` frames tiled to 64 UHD yuv420p10le frames on the device; lattices 33^3 (`cube.log709_lattice(33)` and
a gamma-0.9 lattice as the second), tetrahedral, strict precision; 1D LUT = a 1024-point gamma curve, linear; the CDL of
tests/golden/cdl/shot.cc (saturation 0.6); content natural and sigma-16 noise; yuv420p10le and yuv422p10le out.  Paths timed per
content and output layout, all in ONE process (LUTR_STACK_LDS is read at every launch):
  (a) the stack kernel where nothing else serves, tables in LDS and in global memory
      s_l1d_cdl_l3d_lds / _global      [lut1d, cdl, lut3d]
      s_l3d_cdl_l3d2_lds / _global     [lut3d, cdl, lut3d2]
  (b) the stack kernel (default placement) on the four stacks a dedicated kernel serves, and that kernel in the same run
      s_l3d / plain_vec                [lut3d]          k_yuv_vec / k_yuv_xsub_vec under variant vec_global
      s_cdl_l3d / cdl                  [cdl, lut3d]     k_yuv_cdl_vec
      s_l1d_l3d / l1d                  [lut1d, lut3d]   k_yuv_l1d_vec (its default placement)
      s_l3d_l3d2 / chain               [lut3d, lut3d2]  k_yuv_chain_vec
  (c) the launches a user needs without the feature, through yuv444p10le between the calls (other bits: a time yardstick only)
      two_l1d_then_cdl                 apply_yuv_lut1d(interp=None) -> 444, then apply_yuv(cdl=) -> out
      two_l3d_then_cdl_l3d2            apply_yuv -> 444, then apply_yuv(cdl=) with the second lattice -> out
Paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is
the median round.  Prints one JSON line (and writes it to `--out` when given): Gpx/s and ms per path and the ratios.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 900 python tools/stack_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/stack_rate.json
"""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from lut_renderer_amd import cube, frames  # noqa: E402
from lut_renderer_amd.cdl import Cdl  # noqa: E402
from lut_renderer_amd.engine import LutEngine, parse_pix_fmt  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
FMT = "yuv420p10le"
MID = "yuv444p10le"
OUTS = ("yuv420p10le", "yuv422p10le")
GRADE = dict(slope=(1.3, 1.25, 1.1), offset=(-0.08, 0.0, 0.05), power=(0.8, 1.0, 1.2), saturation=0.6)


def batch(dev, dist, nframes, unique):
    planes = [[], [], []]
    for k in range(unique):
        f = frames.make_yuv(dist, W, H, 10, 1, 1, k=k)
        for i in range(3):
            planes[i].append(torch.from_numpy(np.ascontiguousarray(f[i]).view(np.int16)))
    reps = (nframes + unique - 1) // unique
    return [torch.stack(p).to(dev).repeat(reps, 1, 1)[:nframes].contiguous() for p in planes]


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
        raise SystemExit("stack_rate.py needs a GPU")
    ones = np.ones(3, np.float32)
    lut = cube.CubeLut(33, ones, cube.log709_lattice(33))
    lut2 = cube.CubeLut(33, ones, (cube.identity_lattice(33) ** 0.9).astype(np.float32))
    x = np.linspace(0.0, 1.0, 1024)
    l1 = cube.Lut1D(np.tile((x ** (1 / 2.2)).astype(np.float32), (3, 1)), ones)
    grade = Cdl(**GRADE)
    # st: the stack calls; vec: the plain call under vec_global; ded: the dedicated calls; second: the second lattice as a first one
    st, vec, ded, second = (LutEngine(0) for _ in range(4))
    for e in (st, vec, ded):
        e.set_lut(lut)
    second.set_lut(lut2)
    vec.set_variant("vec_global")
    for e in (st, ded):
        e.set_lut2(lut2)
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

            def stack(stages, cdl=None):
                return lambda: st.apply_yuv_stack(src, out, stages=stages, cdl=cdl, **names)

            def two_l1d_then_cdl():
                ded.apply_yuv_lut1d(src, mid, pix_fmt=FMT, out_pix_fmt=MID, interp=None)
                ded.apply_yuv(mid, out, pix_fmt=MID, out_pix_fmt=out_fmt, interp="tetrahedral", cdl=grade)

            def two_l3d_then_cdl_l3d2():
                vec.apply_yuv(src, mid, pix_fmt=FMT, out_pix_fmt=MID, interp="tetrahedral")
                second.apply_yuv(mid, out, pix_fmt=MID, out_pix_fmt=out_fmt, interp="tetrahedral", cdl=grade)

            sk = lambda: st.last_kernel                                                   # noqa: E731
            paths = {
                "s_l1d_cdl_l3d_lds": (placed("1", stack("lut1d,cdl,lut3d", grade)), sk),
                "s_l1d_cdl_l3d_global": (placed("0", stack("lut1d,cdl,lut3d", grade)), sk),
                "s_l3d_cdl_l3d2_lds": (placed("1", stack("lut3d,cdl,lut3d2", grade)), sk),
                "s_l3d_cdl_l3d2_global": (placed("0", stack("lut3d,cdl,lut3d2", grade)), sk),
                "s_l3d": (stack("lut3d"), sk),
                "plain_vec": (lambda: vec.apply_yuv(src, out, interp="tetrahedral", **names), lambda: vec.last_kernel),
                "s_cdl_l3d": (stack("cdl,lut3d", grade), sk),
                "cdl": (lambda: ded.apply_yuv(src, out, interp="tetrahedral", cdl=grade, **names), lambda: ded.last_kernel),
                "s_l1d_l3d": (stack("lut1d,lut3d"), sk),
                "l1d": (lambda: ded.apply_yuv_lut1d(src, out, interp="tetrahedral", **names), lambda: ded.last_kernel),
                "s_l3d_l3d2": (stack("lut3d,lut3d2"), sk),
                "chain": (lambda: ded.apply_yuv_chain(src, out, interp="tetrahedral", **names), lambda: ded.last_kernel),
                "two_l1d_then_cdl": (two_l1d_then_cdl, lambda: "k_yuv_l1d_vec, then " + ded.last_kernel),
                "two_l3d_then_cdl_l3d2": (two_l3d_then_cdl_l3d2, lambda: vec.last_kernel + ", then " + second.last_kernel),
            }
            r = time_paths(paths, args)
            for a, b in (("s_l3d", "plain_vec"), ("s_cdl_l3d", "cdl"), ("s_l1d_l3d", "l1d"), ("s_l3d_l3d2", "chain")):
                r[f"{a}_time_vs_{b}"] = round(r[a]["ms"] / r[b]["ms"], 3)
            for n in ("s_l1d_cdl_l3d", "s_l3d_cdl_l3d2"):
                r[f"{n}_lds_time_vs_global"] = round(r[n + "_lds"]["ms"] / r[n + "_global"]["ms"], 3)
            r["s_l1d_cdl_l3d_lds_time_vs_two_calls"] = round(r["s_l1d_cdl_l3d_lds"]["ms"] / r["two_l1d_then_cdl"]["ms"], 3)
            r["s_l3d_cdl_l3d2_lds_time_vs_two_calls"] = round(r["s_l3d_cdl_l3d2_lds"]["ms"] / r["two_l3d_then_cdl_l3d2"]["ms"], 3)
            res[dist][out_fmt] = r
            del paths, out
        del src, mid
        torch.cuda.empty_cache()
    for e in (st, vec, ded, second):
        e.close()
    line = json.dumps({"tool": "stack_rate", "frames": args.frames, "size": f"{W}x{H}", "pix_fmt": FMT, "lut": 33,
                       "interp": "tetrahedral", "precision": "strict", "lut1d": {"rows": 1024, "interp1d": "linear"}, "cdl": GRADE,
                       "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
