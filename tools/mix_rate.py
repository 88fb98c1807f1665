#!/usr/bin/env python3
"""tools/mix_rate.py -- LUT strength in the fused stack pass: the mix forms of the stack kernels against the
stack kernel of the same list in the same run.

The batch: `frames.make_yuv` frames tiled to 64 UHD yuv420p10le frames on the device, written as yuv422p10le (4:2:0 -> 4:2:2);
lattice 33^3 (`cube.log709_lattice(33)`), tetrahedral, strict precision; 1D LUT = a 1024-point gamma curve, linear; the CDL of
tests/golden/cdl/shot.cc (saturation 0.6); content natural and sigma-16 noise.  Two lists, each timed three ways in ONE process:
      l3d / l3d_s06 / l3d_ramp                        [lut3d]
      l1d_cdl_l3d / l1d_cdl_l3d_s06 / l1d_cdl_l3d_ramp  [lut1d, cdl, lut3d]
  <list>        without a strength: the stack kernel of 3.21 (the yardstick)
  <list>_s06    strength 0.6 for every frame: the scalar in the kernel's arguments
  <list>_ramp   one strength per frame, 0 .. 1 over the batch: an array on the device, uploaded once before the timing (the
                upload of 64 floats per call is the host's cost, not the kernel's)
Paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is
the median round.  Prints one JSON line (and writes it to `--out` when given): Gpx/s and ms per path and the time ratios
<list>_s06_time_vs_plain and <list>_ramp_time_vs_plain.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/mix_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/mix_rate.json
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from lut_renderer_amd import _native, cube, frames  # noqa: E402
from lut_renderer_amd.cdl import Cdl  # noqa: E402
from lut_renderer_amd.engine import LutEngine, parse_pix_fmt  # noqa: E402

W, H = 3840, 2160
DISTS = ("natural", "noise16")
FMT, OUT = "yuv420p10le", "yuv422p10le"
GRADE = dict(slope=(1.3, 1.25, 1.1), offset=(-0.08, 0.0, 0.05), power=(0.8, 1.0, 1.2), saturation=0.6)
LISTS = (("l3d", "lut3d", False), ("l1d_cdl_l3d", "lut1d,cdl,lut3d", True))


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


def desc(tensors):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        st.data[i] = t.data_ptr()
        st.stride[i] = t.stride(-2) * t.element_size()
        st.frame_stride[i] = t.stride(0) * t.element_size()
    return st


def time_paths(paths, args, name):
    kern = {}
    for n, run in paths.items():
        for _ in range(args.warmup):
            run()
        kern[n] = name()
    torch.cuda.synchronize()
    secs = {n: [] for n in paths}
    for _ in range(args.rounds):
        for n, run in paths.items():
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
        raise SystemExit("mix_rate.py needs a GPU")
    ones = np.ones(3, np.float32)
    x = np.linspace(0.0, 1.0, 1024)
    grade = Cdl(**GRADE)
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, ones, cube.log709_lattice(33)))
    eng.set_lut1d(cube.Lut1D(np.tile((x ** (1 / 2.2)).astype(np.float32), (3, 1)), ones), "linear")
    dev = eng.device
    ramp = torch.linspace(0.0, 1.0, args.frames, dtype=torch.float32, device=dev)
    p = _native.YuvParams(_native.fmt_code(10, 1, 1), _native.fmt_code(10, 1, 0), 10, 0, 0, 0, 0, 0)
    cdl_st = _native.cdl_struct(grade)
    res = {}
    for dist in DISTS:
        src, out = batch(dev, dist, args.frames, args.unique), empty(dev, OUT, args.frames)
        s, d = desc(src), desc(out)
        paths = {}
        for tag, stages, with_cdl in LISTS:
            def plain(stages=stages, with_cdl=with_cdl):
                eng.apply_yuv_stack(src, out, pix_fmt=FMT, out_pix_fmt=OUT, stages=stages, cdl=grade if with_cdl else None)

            def scalar(stages=stages, with_cdl=with_cdl):
                eng.apply_yuv_stack(src, out, pix_fmt=FMT, out_pix_fmt=OUT, stages=stages, cdl=grade if with_cdl else None, strength=0.6)

            def per_frame(stages=stages, with_cdl=with_cdl):       # the C entry with the array that is on the device already
                arr = _native.stage_array(tuple((k, "tetrahedral" if k == "lut3d" else None) for k in stages.split(",")))
                with eng._lock:
                    eng._bind_stream()
                    _native.check(eng._lib.lutr_apply_yuv_stack_mix(
                        eng._ctx, C.byref(p), arr, len(arr), C.byref(cdl_st) if with_cdl else None, 1.0, C.c_void_p(ramp.data_ptr()),
                        W, H, args.frames, C.byref(s), C.byref(d), 0, H))

            paths.update({tag: plain, tag + "_s06": scalar, tag + "_ramp": per_frame})
        r = time_paths(paths, args, lambda: eng.last_kernel)
        for tag, _stages, _c in LISTS:
            for form in ("_s06", "_ramp"):
                r[f"{tag}{form}_time_vs_plain"] = round(r[tag + form]["ms"] / r[tag]["ms"], 3)
        res[dist] = r
        del paths, src, out
        torch.cuda.empty_cache()
    eng.close()
    line = json.dumps({"tool": "mix_rate", "frames": args.frames, "size": f"{W}x{H}", "pix_fmt": FMT, "out_pix_fmt": OUT, "lut": 33,
                       "interp": "tetrahedral", "precision": "strict", "lut1d": {"rows": 1024, "interp1d": "linear"}, "cdl": GRADE,
                       "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
