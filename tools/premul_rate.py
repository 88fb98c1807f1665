#!/usr/bin/env python3
"""tools/premul_rate.py -- what unpremultiply / premultiply around the LUT costs.

The batch: synthetic `yuv444p10le` frames (`frames.make_yuv`) tiled to 64 UHD frames on the device, their chroma decimated for the
4:2:0 source, an alpha plane of uniform noise in [3/4, 1] of full scale (a soft matte: most quotients stay below the clamp),
`cube.log709_lattice(33)`, tetrahedral, strict precision; content natural and sigma-16 noise.  Paths timed per content:
  premul_444        yuva444p10le -> yuva444p10le, alpha_mode="premultiplied"     k_yuva_premul_vec<1,1,0,0,0,0,2>+k_alpha_vec<1,1>
  straight_444_vg   the straight call of the same formats on variant vec_global: the like-for-like yardstick (global gather)
  straight_444      the straight call on variant auto (the LDS-window kernels at this size)
  premul_420_422    yuva420p10le -> yuva422p10le, premultiplied                  k_yuva_premul_vec<1,1,1,1,1,0,2>+k_alpha_vec<1,1>
  straight_420_422_vg / straight_420_422   its straight calls, likewise
and, on the natural content as floats (code / 1023, alpha in [3/4, 1]):
  premul_f32        gbrapf32le in and out, premultiplied                         k_rgbaf_premul_vec<2>
  straight_f32      the straight call                                            k_rgbf_vec<2>
All paths run in one process, timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of
each; the figure is the median round.  Prints one JSON line (and writes it to --out when given): milliseconds per launch and
Gpx/s per path, and per premultiplied path its rate over the straight call's (`vs_vec_global`, `vs_auto`: 1 = no cost).

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/premul_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/premul_rate.json
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
YUV_PATHS = ("premul_444", "straight_444_vg", "straight_444", "premul_420_422", "straight_420_422_vg", "straight_420_422")
F32_PATHS = ("premul_f32", "straight_f32")


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def planes(eng, name, nframes):
    f = parse_pix_fmt(name)
    return [torch.empty((nframes,) + f.plane_shape(i, W, H), dtype=torch.int16, device=eng.device) for i in range(f.nplanes)]


def timed(paths, call, kernel_of, args):
    kern = {}
    for n in paths:
        for _ in range(args.warmup):
            call(n)
        kern[n] = kernel_of()
    torch.cuda.synchronize()
    secs = {n: [] for n in paths}
    for _ in range(args.rounds):
        for n in paths:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                call(n)
            ev1.record()
            torch.cuda.synchronize()
            secs[n].append(ev0.elapsed_time(ev1) / 1e3 / args.steps)
    px = args.frames * W * H
    res = {}
    for n, s in secs.items():
        med = statistics.median(s)
        res[n] = {"ms": round(med * 1e3, 3), "gpx_s": round(px / med / 1e9, 1), "rounds_ms": [round(v * 1e3, 3) for v in s],
                  "kernel": kern[n]}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=10, help="launches per timed round")
    ap.add_argument("--warmup", type=int, default=3, help="untimed launches of each path before the first round")
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds over the paths")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--unique", type=int, default=2, help="distinct synthetic frames tiled to --frames")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("premul_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    nf = args.frames
    reps = (nf + args.unique - 1) // args.unique
    alpha = torch.randint(768, 1024, (nf, H, W), dtype=torch.int16, device=eng.device)
    o444, o422 = planes(eng, "yuva444p10le", nf), planes(eng, "yuva422p10le", nf)
    results = {}
    s444 = None
    for dist in ("noise16", "natural"):                # (natural last: its planes feed the float paths)
        fs = [frames.make_yuv(dist, W, H, 10, 0, 0, k=k) for k in range(args.unique)]
        s444 = [torch.stack([_dev(x[i]) for x in fs]).to(eng.device).repeat(reps, 1, 1)[:nf].contiguous() for i in range(3)]
        s420 = [s444[0], s444[1][:, ::2, ::2].contiguous(), s444[2][:, ::2, ::2].contiguous()]

        def call(name):
            premul = name.startswith("premul")
            eng.set_variant("vec_global" if name.endswith("_vg") else "auto")
            mode = dict(alpha_mode="premultiplied") if premul else {}
            if "444" in name:
                eng.apply_yuv(s444 + [alpha], o444, pix_fmt="yuva444p10le", interp="tetrahedral", **mode)
            else:
                eng.apply_yuv(s420 + [alpha], o422, pix_fmt="yuva420p10le", out_pix_fmt="yuva422p10le", interp="tetrahedral", **mode)

        res = timed(YUV_PATHS, call, lambda: eng.last_kernel, args)
        for p, vg, auto in (("premul_444", "straight_444_vg", "straight_444"),
                            ("premul_420_422", "straight_420_422_vg", "straight_420_422")):
            res[p]["vs_vec_global"] = round(res[vg]["ms"] / res[p]["ms"], 3)
            res[p]["vs_auto"] = round(res[auto]["ms"] / res[p]["ms"], 3)
        results[dist] = res
        del s420
    eng.set_variant("auto")
    del o444, o422
    f32 = [(p.to(torch.float32) * (1.0 / 1023.0)) for p in s444]
    del s444
    fa = (alpha.to(torch.float32) * (1.0 / 1023.0))
    del alpha
    fo = [torch.empty_like(p) for p in f32 + [fa]]

    def call_f(name):
        eng.apply_rgb_float(f32 + [fa], fo, interp="tetrahedral", **(dict(alpha_mode="premultiplied") if name == "premul_f32" else {}))

    res = timed(F32_PATHS, call_f, lambda: eng.last_kernel, args)
    res["premul_f32"]["vs_straight"] = round(res["straight_f32"]["ms"] / res["premul_f32"]["ms"], 3)
    results["natural_f32"] = res
    eng.close()
    line = json.dumps({"tool": "premul_rate", "frames": nf, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
