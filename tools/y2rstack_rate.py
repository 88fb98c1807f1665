#!/usr/bin/env python3
"""tools/y2rstack_rate.py -- the stage stack from YUV sources into RGB frames: the new kernel against the
dedicated YUV -> RGB kernel on the one list that serves, its two table placements, and the two launches a user needs without it.

The batch: `frames.make_yuv` frames tiled to 64 UHD frames on the device; lattice 33^3 (`cube.log709_lattice(33)`), tetrahedral,
strict precision; 1D LUT = a 1024-point gamma curve, linear; the CDL of tools/stack_rate.py (saturation 0.6); content natural and
sigma-16 noise.  Three cases:
      yuv420p10le -> gbrp10le      yuv420p10le -> rgb48le      yuv420p -> rgba
Paths timed per content and case, all in ONE process (LUTR_STACK_LDS is read at every launch):
  (a) the price of the uniform step loop: the stack kernel on [lut3d] and the dedicated kernel in the same run
      s_l3d / ref                      k_yuv2rgb_vec (apply_yuv_to_rgb under variant vec_global)
  (b) the lists nothing else serves in one pass, tables in LDS and in global memory (at 16 bit the tables do not fit LDS: both
      rows then run the global-memory placement, and the kernel names say so)
      s_cdl_l3d_lds / _global          [cdl, lut3d]
      s_l1d_cdl_l3d_lds / _global      [lut1d, cdl, lut3d]
  (c) the same lists (default placement) against the route a user has without the feature: apply_yuv_to_rgb(lut=False) into
      gbrp at the destination's depth, then apply_rgb_stack from gbrp into gbrp.  For a packed destination the user's own packing
      pass comes on top of that and is NOT counted.
      s_cdl_l3d / two_cdl_l3d          s_l1d_cdl_l3d / two_l1d_cdl_l3d
Paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is
the median round.  Prints one JSON line (and writes it to `--out` when given): Gpx/s and ms per path and the ratios.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 900 python tools/y2rstack_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/y2rstack_rate.json
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
from lut_renderer_amd.engine import LutEngine  # noqa: E402
from lut_renderer_amd.formats import parse_pix_fmt, parse_rgb_out  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
CASES = (("yuv420p10le", "gbrp10le"), ("yuv420p10le", "rgb48le"), ("yuv420p", "rgba"))
GRADE = dict(slope=(1.3, 1.25, 1.1), offset=(-0.08, 0.0, 0.05), power=(0.8, 1.0, 1.2), saturation=0.6)


def batch(dev, dist, nframes, unique, name):
    """`nframes` frames of planar YUV `name` (Y, Cb, Cr), `unique` distinct ones tiled."""
    f = parse_pix_fmt(name)
    fs = [frames.make_yuv(dist, W, H, f.depth, f.csx, f.csy, k=k) for k in range(unique)]
    reps = (nframes + unique - 1) // unique
    view = (lambda a: np.ascontiguousarray(a).view(np.int16)) if f.depth > 8 else np.ascontiguousarray
    return [torch.stack([torch.from_numpy(view(fr[i])) for fr in fs]).to(dev).repeat(reps, 1, 1)[:nframes].contiguous() for i in range(3)]


def gbrp_name(depth):
    return "gbrp" if depth == 8 else f"gbrp{depth}le"


def empty(dev, name, nframes):
    """An uninitialised destination: three gbrp planes, or one packed image."""
    f = parse_rgb_out(name)
    dt = torch.uint8 if f.depth <= 8 else torch.int16
    if hasattr(f, "ncomp") and f.packed:
        return torch.empty((nframes, H, W, f.ncomp), dtype=dt, device=dev)
    return [torch.empty((nframes, H, W), dtype=dt, device=dev) for _ in range(3)]


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
        raise SystemExit("y2rstack_rate.py needs a GPU")
    ones = np.ones(3, np.float32)
    lut = cube.CubeLut(33, ones, cube.log709_lattice(33))
    x = np.linspace(0.0, 1.0, 1024)
    l1 = cube.Lut1D(np.tile((x ** (1 / 2.2)).astype(np.float32), (3, 1)), ones)
    grade = Cdl(**GRADE)
    # st: the stack calls; vec: the dedicated kernel under vec_global; two: the two-call route
    st, vec, two = (LutEngine(0) for _ in range(3))
    for e in (st, vec, two):
        e.set_lut(lut)
    vec.set_variant("vec_global")
    st.set_lut1d(l1, "linear")
    two.set_lut1d(l1, "linear")
    dev = st.device
    res = {}
    for dist in DISTS:
        res[dist] = {}
        for src_fmt, out_fmt in CASES:
            depth = parse_rgb_out(out_fmt).depth
            src = batch(dev, dist, args.frames, args.unique, src_fmt)
            out = empty(dev, out_fmt, args.frames)
            mid, end = empty(dev, gbrp_name(depth), args.frames), empty(dev, gbrp_name(depth), args.frames)
            names = dict(pix_fmt=src_fmt, out_pix_fmt=out_fmt)

            def stack(stages, cdl=None):
                return lambda: st.apply_yuv_stack_to_rgb(src, out, stages=stages, cdl=cdl, **names)

            def two_calls(stages, log):
                def run():
                    two.apply_yuv_to_rgb(src, mid, pix_fmt=src_fmt, out_pix_fmt=gbrp_name(depth), lut=False)
                    two.apply_rgb_stack(mid, end, pix_fmt=gbrp_name(depth), stages=stages, cdl=grade)
                    log.append(two.last_kernel)
                return run

            sk = lambda: st.last_kernel                                                   # noqa: E731
            log_a, log_b = [], []
            paths = {
                "s_l3d": (stack("lut3d"), sk),
                "ref": (lambda: vec.apply_yuv_to_rgb(src, out, interp="tetrahedral", **names), lambda: vec.last_kernel),
                "s_cdl_l3d_lds": (placed("1", stack("cdl,lut3d", grade)), sk),
                "s_cdl_l3d_global": (placed("0", stack("cdl,lut3d", grade)), sk),
                "s_l1d_cdl_l3d_lds": (placed("1", stack("lut1d,cdl,lut3d", grade)), sk),
                "s_l1d_cdl_l3d_global": (placed("0", stack("lut1d,cdl,lut3d", grade)), sk),
                "s_cdl_l3d": (stack("cdl,lut3d", grade), sk),
                "s_l1d_cdl_l3d": (stack("lut1d,cdl,lut3d", grade), sk),
                "two_cdl_l3d": (two_calls("cdl,lut3d", log_a), lambda: "k_yuv2rgb_vec<nolut>, then " + log_a[-1]),
                "two_l1d_cdl_l3d": (two_calls("lut1d,cdl,lut3d", log_b), lambda: "k_yuv2rgb_vec<nolut>, then " + log_b[-1]),
            }
            r = time_paths(paths, args)
            r["s_l3d_time_vs_ref"] = round(r["s_l3d"]["ms"] / r["ref"]["ms"], 3)
            for n in ("s_cdl_l3d", "s_l1d_cdl_l3d"):
                r[f"{n}_lds_time_vs_global"] = round(r[n + "_lds"]["ms"] / r[n + "_global"]["ms"], 3)
                r[f"{n}_time_vs_two_calls"] = round(r[n]["ms"] / r[n.replace("s_", "two_", 1)]["ms"], 3)
            r["two_calls_count_the_packing_pass"] = False
            res[dist][f"{src_fmt}->{out_fmt}"] = r
            del paths, out, src, mid, end
            torch.cuda.empty_cache()
    for e in (st, vec, two):
        e.close()
    line = json.dumps({"tool": "y2rstack_rate", "frames": args.frames, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "lut1d": {"rows": 1024, "interp1d": "linear"}, "cdl": GRADE, "steps": args.steps,
                       "warmup": args.warmup, "rounds": args.rounds, "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
