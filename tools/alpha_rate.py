#!/usr/bin/env python3
"""tools/alpha_rate.py -- what carrying an alpha plane costs.

The batch: synthetic natural `yuv444p10le` frames (`frames.make_yuv`) tiled to 64 UHD frames on the device, their chroma decimated
for the 4:2:0 source, a random alpha plane, `cube.log709_lattice(33)`, tetrahedral, strict precision.  Paths timed:
  alpha_10_10       the alpha plane alone, 10 -> 10 bit (a copy)      k_alpha_vec<1,1>
  alpha_10_8        the alpha plane alone, 10 -> 8 bit                k_alpha_vec<1,0>
  torch_copy        torch's device-to-device copy_ of the same plane: the yardstick of alpha_10_10
  yuva444           yuva444p10le -> yuva444p10le, the whole call      <colour kernel>+k_alpha_vec<1,1>
  yuv444            its three-plane twin, yuv444p10le -> yuv444p10le
  yuva420_8         yuva420p10le -> yuva420p, the whole call          <colour kernel>+k_alpha_vec<1,0>
  yuv420_8          its three-plane twin, yuv420p10le -> yuv420p
All paths run in one process, timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches
of each; the figure is the median round.  Prints one JSON line (and writes it to --out when given): milliseconds per launch per
path, bytes per second of the three plane movers (bytes read plus bytes written), `alpha_vs_copy` (alpha_10_10's time over
torch_copy's; the copy's own spread between rounds beside it), and per whole call the extra time over its twin as a fraction of
the alpha kernel's time alone (`extra_vs_alpha`: about 1 when an alpha-carrying call costs the three-plane call plus the plane).

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/alpha_rate.py --steps 10 --warmup 3 --rounds 3 --out profiles/alpha_rate.json
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
PATHS = ("alpha_10_10", "alpha_10_8", "torch_copy", "yuva444", "yuv444", "yuva420_8", "yuv420_8")


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def planes(eng, name, nframes):
    f = parse_pix_fmt(name)
    dt = torch.uint8 if f.depth <= 8 else torch.int16
    return [torch.empty((nframes,) + f.plane_shape(i, W, H), dtype=dt, device=eng.device) for i in range(f.nplanes)]


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
        raise SystemExit("alpha_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    nf = args.frames
    reps = (nf + args.unique - 1) // args.unique
    fs = [frames.make_yuv("natural", W, H, 10, 0, 0, k=k) for k in range(args.unique)]
    s444 = [torch.stack([_dev(x[i]) for x in fs]).to(eng.device).repeat(reps, 1, 1)[:nf].contiguous() for i in range(3)]
    alpha = torch.randint(0, 1024, (nf, H, W), dtype=torch.int16, device=eng.device)
    s420 = [s444[0], s444[1][:, ::2, ::2].contiguous(), s444[2][:, ::2, ::2].contiguous()]
    o444, o420 = planes(eng, "yuva444p10le", nf), planes(eng, "yuva420p", nf)
    a8 = o420[3]

    def call(name):
        if name == "alpha_10_10":
            eng._alpha_plane(alpha, o444[3], 10, 10, W, H, 0, None)
        elif name == "alpha_10_8":
            eng._alpha_plane(alpha, a8, 10, 8, W, H, 0, None)
        elif name == "torch_copy":
            o444[3].copy_(alpha)
        elif name == "yuva444":
            eng.apply_yuv(s444 + [alpha], o444, pix_fmt="yuva444p10le", interp="tetrahedral")
        elif name == "yuv444":
            eng.apply_yuv(s444, o444[:3], pix_fmt="yuv444p10le", interp="tetrahedral")
        elif name == "yuva420_8":
            eng.apply_yuv(s420 + [alpha], o420, pix_fmt="yuva420p10le", out_pix_fmt="yuva420p", interp="tetrahedral")
        else:
            eng.apply_yuv(s420, o420[:3], pix_fmt="yuv420p10le", out_pix_fmt="yuv420p", interp="tetrahedral")

    kern = {}
    for n in PATHS:
        for _ in range(args.warmup):
            call(n)
        # (the plane alone: the library's own name; LutEngine.last_kernel would prefix what ran before it)
        kern[n] = "copy_" if n == "torch_copy" else eng._lib.lutr_ctx_last_kernel(eng._ctx).decode() if n.startswith("alpha") \
            else eng.last_kernel
    torch.cuda.synchronize()
    secs = {n: [] for n in PATHS}
    for _ in range(args.rounds):
        for n in PATHS:
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                call(n)
            ev1.record()
            torch.cuda.synchronize()
            secs[n].append(ev0.elapsed_time(ev1) / 1e3 / args.steps)
    eng.close()
    res = {}
    for n, s in secs.items():
        med = statistics.median(s)
        res[n] = {"ms": round(med * 1e3, 3), "rounds_ms": [round(v * 1e3, 3) for v in s], "kernel": kern[n]}
    samples = nf * W * H
    for n, nbytes in (("alpha_10_10", 4 * samples), ("torch_copy", 4 * samples), ("alpha_10_8", 3 * samples)):
        res[n]["gb_s"] = round(nbytes / (res[n]["ms"] / 1e3) / 1e9, 1)
    copy = res["torch_copy"]["rounds_ms"]
    res["alpha_vs_copy"] = round(res["alpha_10_10"]["ms"] / res["torch_copy"]["ms"], 3)
    res["copy_spread"] = round((max(copy) - min(copy)) / res["torch_copy"]["ms"], 3)
    for whole, twin, a in (("yuva444", "yuv444", "alpha_10_10"), ("yuva420_8", "yuv420_8", "alpha_10_8")):
        res[f"{whole}_vs_twin"] = round(res[whole]["ms"] / res[twin]["ms"], 3)
        res[f"{whole}_extra_vs_alpha"] = round((res[whole]["ms"] - res[twin]["ms"]) / res[a]["ms"], 3)
    line = json.dumps({"tool": "alpha_rate", "frames": nf, "size": f"{W}x{H}", "lut": 33, "interp": "tetrahedral",
                       "precision": "strict", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                       "device": torch.cuda.get_device_name(0), "results": res})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
