#!/usr/bin/env python3
"""tools/matte_rate.py -- a matte plane in the fused stack pass: the matte forms of the stack kernels against
the mix kernel (k_yuv_stack_mix_vec) of the same list in the same run.

The batch: `frames.make_yuv` frames tiled to 64 UHD yuv420p10le frames on the device, written as yuv422p10le (4:2:0 -> 4:2:2);
lattice 33^3 (`cube.log709_lattice(33)`), tetrahedral, strict precision; 1D LUT = a 1024-point gamma curve, linear; the CDL of
tests/golden/cdl/shot.cc (saturation 0.6); content natural and sigma-16 noise; strength 0.6.  The matte is seeded noise with a
rectangle of the largest code, tiled like the frames.  Two lists, each timed five ways in ONE process:
      l3d_*            [lut3d]
      l1d_cdl_l3d_*    [lut1d, cdl, lut3d]
  <list>_mix        strength 0.6, no matte: the mix kernel of 3.22 (the yardstick)
  <list>_m8         an 8-bit matte per frame (bytes beside the 16-bit source: wm = 0)
  <list>_m10        a 10-bit matte per frame (16-bit words: wm = 1)
  <list>_m8_still   one 8-bit matte for every frame (frame stride 0)
  <list>_m10_still  one 10-bit matte for every frame
Paths are timed in alternating rounds with HIP events around `--steps` launches, after `--warmup` launches of each; the figure is
the median round.  Prints one JSON line (and writes it to `--out` when given): Gpx/s and ms per path and the time ratios
<path>_time_vs_mix.

`--alt-library PATH` names a second liblutr.so (built in another checkout); the tool then measures both, each in a child process of its own with LUTR_LIBRARY set, and writes both under
"placements" (`--name` / `--alt-name` label them; "chosen" is `--name`, the tree's).  `--resources FILE` carries a JSON object of
compile-time figures along under "resources": VGPRs / waves per SIMD / scratch of the instances, from
`hipcc -Rpass-analysis=kernel-resource-usage`, which needs no GPU.

Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/matte_rate.py --steps 100 --warmup 5 --rounds 5 --out profiles/matte_rate.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

W, H = 3840, 2160
DISTS = ("natural", "noise16")
FMT, OUT = "yuv420p10le", "yuv422p10le"
GRADE = dict(slope=(1.3, 1.25, 1.1), offset=(-0.08, 0.0, 0.05), power=(0.8, 1.0, 1.2), saturation=0.6)
LISTS = (("l3d", "lut3d", False), ("l1d_cdl_l3d", "lut1d,cdl,lut3d", True))
FORMS = ("_m8", "_m10", "_m8_still", "_m10_still")
STRENGTH = 0.6


def measure(args):
    """The measurement itself, in this process, with the library LUTR_LIBRARY names (or the tree's)."""
    import torch
    from lut_renderer_amd import cube, frames
    from lut_renderer_amd.cdl import Cdl
    from lut_renderer_amd.engine import LutEngine, parse_pix_fmt
    if not torch.cuda.is_available():
        raise SystemExit("matte_rate.py needs a GPU")

    def batch(dev, dist):
        planes = [[], [], []]
        for k in range(args.unique):
            f = frames.make_yuv(dist, W, H, 10, 1, 1, k=k)
            for i in range(3):
                planes[i].append(torch.from_numpy(np.ascontiguousarray(f[i]).view(np.int16)))
        reps = (args.frames + args.unique - 1) // args.unique
        return [torch.stack(p).to(dev).repeat(reps, 1, 1)[:args.frames].contiguous() for p in planes]

    def matte(dev, depth):
        rng = np.random.default_rng(depth)
        m = rng.integers(0, 1 << depth, size=(args.unique, H, W)).astype(np.uint8 if depth == 8 else np.uint16)
        m[:, H // 4:H // 2 | 1, W // 4 | 1:W // 2 | 1] = (1 << depth) - 1
        t = torch.from_numpy(m if depth == 8 else m.view(np.int16)).to(dev)
        reps = (args.frames + args.unique - 1) // args.unique
        return t.repeat(reps, 1, 1)[:args.frames].contiguous()

    def time_paths(paths, name):
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

    ones = np.ones(3, np.float32)
    x = np.linspace(0.0, 1.0, 1024)
    grade = Cdl(**GRADE)
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, ones, cube.log709_lattice(33)))
    eng.set_lut1d(cube.Lut1D(np.tile((x ** (1 / 2.2)).astype(np.float32), (3, 1)), ones), "linear")
    dev = eng.device
    fout = parse_pix_fmt(OUT)
    mattes = {8: matte(dev, 8), 10: matte(dev, 10)}
    res = {}
    for dist in DISTS:
        src = batch(dev, dist)
        out = [torch.empty((args.frames,) + fout.plane_shape(i, W, H), dtype=torch.int16, device=dev) for i in range(3)]
        paths = {}
        for tag, stages, with_cdl in LISTS:
            kw = dict(pix_fmt=FMT, out_pix_fmt=OUT, stages=stages, cdl=grade if with_cdl else None, strength=STRENGTH)

            def run(kw=kw, **more):
                eng.apply_yuv_stack(src, out, **kw, **more)

            paths[tag + "_mix"] = run
            for depth in (8, 10):
                m = mattes[depth]
                paths[f"{tag}_m{depth}"] = lambda run=run, m=m, depth=depth: run(matte=m, matte_depth=depth)
                paths[f"{tag}_m{depth}_still"] = lambda run=run, m=m, depth=depth: run(matte=m[0], matte_depth=depth)
        r = time_paths(paths, lambda: eng.last_kernel)
        for tag, _stages, _c in LISTS:
            for form in FORMS:
                r[f"{tag}{form}_time_vs_mix"] = round(r[tag + form]["ms"] / r[tag + "_mix"]["ms"], 3)
        res[dist] = r
        del paths, src, out
        torch.cuda.empty_cache()
    eng.close()
    return {"device": torch.cuda.get_device_name(0), "results": res}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=100, help="launches per timed round")
    ap.add_argument("--warmup", type=int, default=5, help="untimed launches of each path before the first round")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds over the paths")
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--unique", type=int, default=4, help="distinct synthetic frames (and mattes) tiled to --frames")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--name", default="top", help="label of the matte load placement the tree's library is built with")
    ap.add_argument("--alt-library", default=None, help="a liblutr.so built with the other placement: measured as well")
    ap.add_argument("--alt-name", default="late", help="label of --alt-library's placement")
    ap.add_argument("--resources", default=None, help="a JSON file of compile-time resource figures to carry along under 'resources'")
    ap.add_argument("--child-timeout", type=float, default=400.0, help="seconds each placement's process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args)))
        return
    head = {"tool": "matte_rate", "frames": args.frames, "size": f"{W}x{H}", "pix_fmt": FMT, "out_pix_fmt": OUT, "lut": 33,
            "interp": "tetrahedral", "precision": "strict", "lut1d": {"rows": 1024, "interp1d": "linear"}, "cdl": GRADE,
            "strength": STRENGTH, "yardstick": "k_yuv_stack_mix_vec on the same list in the same process",
            "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds, "chosen": args.name}
    if args.resources is not None:
        head["resources"] = json.loads(Path(args.resources).read_text())
    if args.alt_library is None:
        line = json.dumps({**head, "placement": args.name, **measure(args)})
    else:
        # one fresh process per library: the library is loaded once per process
        argv = [sys.executable, str(Path(__file__).resolve()), "--child", "--steps", str(args.steps), "--warmup", str(args.warmup),
                "--rounds", str(args.rounds), "--frames", str(args.frames), "--unique", str(args.unique)]
        placements = {}
        for name, lib in ((args.name, None), (args.alt_name, args.alt_library)):
            env = {k: v for k, v in os.environ.items() if k != "LUTR_LIBRARY"}
            if lib is not None:
                env["LUTR_LIBRARY"] = str(Path(lib).resolve())
            r = subprocess.run(argv, capture_output=True, text=True, env=env, cwd=ROOT, timeout=args.child_timeout)
            if r.returncode != 0:                              # (nothing more is started on the GPU after a failure)
                raise SystemExit(f"the measurement of placement '{name}' failed ({r.returncode}):\n{r.stderr}")
            placements[name] = json.loads(r.stdout.strip().splitlines()[-1])
        line = json.dumps({**head, "placements": placements})
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
