#!/usr/bin/env python3
"""tools/resize_rate.py -- the output resize: the kernel alone, and LUT + resize against the LUT alone.

The batch: `frames.make_yuv("natural")` frames tiled to 64 UHD yuv420p10le frames on the device, `cube.log709_lattice(33)`,
tetrahedral, strict precision.  Timed, each as the median of `--rounds` alternating rounds of `--steps` calls between HIP
events, after `--warmup` calls:
  resize_<size>        LutEngine.resize alone: UHD -> 1920x1080, UHD -> 1280x720, and 1080p -> UHD (a 1080p batch).
                       Gpx/s of OUTPUT luma pixels, and TB/s of the kernel's own bytes (every source plane read once, every
                       output plane written once) against the 8 TB/s HBM peak.
  lut                  apply_yuv alone (source-size output).
  lut_resize_c<N>      apply_yuv(out_size=1920x1080, resize_chunk=N) for N = 1, 4, 16, 64; Gpx/s of SOURCE pixels, and the
                       ratio to `lut`.
Also the bytes per frame a host pipeline copies device -> host with and without the resize (arithmetic, not timed).
Prints one JSON line.  Needs a GPU; run it under a time limit of its own, e.g.
    timeout -k 10 600 python tools/resize_rate.py --steps 5 --warmup 2 --rounds 3
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

HBM_PEAK = 8.0e12
FMT = "yuv420p10le"


def batch(eng, w, h, nframes, unique):
    planes = [[], [], []]
    for k in range(unique):
        f = frames.make_yuv("natural", w, h, 10, 1, 1, k=k)
        for i in range(3):
            planes[i].append(torch.from_numpy(np.ascontiguousarray(f[i]).view(np.int16)))
    reps = (nframes + unique - 1) // unique
    return [torch.stack(p).to(eng.device).repeat(reps, 1, 1)[:nframes].contiguous() for p in planes]


def frame_bytes(w, h):
    f = parse_pix_fmt(FMT)
    return sum(a * b for a, b in (f.plane_shape(i, w, h) for i in range(3))) * 2


def time_calls(calls, args):
    """calls: name -> zero-argument callable.  Returns name -> (median seconds per call, [seconds per round])."""
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    secs = {n: [] for n in calls}
    for _ in range(args.rounds):
        for n, fn in calls.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(args.steps):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            secs[n].append(ev0.elapsed_time(ev1) / 1e3 / args.steps)
    return {n: (statistics.median(s), s) for n, s in secs.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--unique", type=int, default=4)
    ap.add_argument("--only", default=None, help="resize | compose (default: both)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_rate.py needs a GPU")
    eng = LutEngine(0)
    eng.set_lut(cube.CubeLut(33, np.ones(3, np.float32), cube.log709_lattice(33)))
    nf = args.frames
    res = {}
    uhd = batch(eng, 3840, 2160, nf, args.unique)
    if args.only in (None, "resize"):
        fhd = batch(eng, 1920, 1080, nf, args.unique)
        jobs = {"resize_uhd_to_1080p": (uhd, (3840, 2160), (1920, 1080)),
                "resize_uhd_to_720p": (uhd, (3840, 2160), (1280, 720)),
                "resize_1080p_to_uhd": (fhd, (1920, 1080), (3840, 2160))}
        outs, calls = {}, {}
        for n, (src, _, (dw, dh)) in jobs.items():
            outs[n] = eng.resize(src, pix_fmt=FMT, size=(dw, dh))
            calls[n] = (lambda s=src, o=outs[n], sz=(dw, dh): eng.resize(s, o, pix_fmt=FMT, size=sz))
        t = time_calls(calls, args)
        for n, (src, (sw, sh), (dw, dh)) in jobs.items():
            sec, rounds = t[n]
            nbytes = nf * (frame_bytes(sw, sh) + frame_bytes(dw, dh))
            res[n] = {"gpx_s_out": round(nf * dw * dh / sec / 1e9, 1), "tb_s": round(nbytes / sec / 1e12, 2),
                      "of_hbm_peak": round(nbytes / sec / HBM_PEAK, 3), "ms": round(sec * 1e3, 3),
                      "rounds_ms": [round(s * 1e3, 3) for s in rounds], "bytes": nbytes, "kernel": eng.last_kernel}
        del fhd, outs, calls
        torch.cuda.empty_cache()
    if args.only in (None, "compose"):
        full = [torch.empty_like(t) for t in uhd]
        small = eng.resize(uhd, pix_fmt=FMT, size=(1920, 1080))
        calls = {"lut": lambda: eng.apply_yuv(uhd, full, pix_fmt=FMT)}
        for c in (1, 4, 16, 64):
            calls[f"lut_resize_c{c}"] = (lambda c=c: eng.apply_yuv(uhd, small, pix_fmt=FMT, out_size=(1920, 1080), resize_chunk=c))
        t = time_calls(calls, args)
        base = t["lut"][0]
        for n, (sec, rounds) in t.items():
            res[n] = {"gpx_s_src": round(nf * 3840 * 2160 / sec / 1e9, 1), "ms": round(sec * 1e3, 3),
                      "rounds_ms": [round(s * 1e3, 3) for s in rounds], "vs_lut": round(base / sec, 3)}
        res["d2h_bytes_per_frame"] = {"uhd": frame_bytes(3840, 2160), "1080p": frame_bytes(1920, 1080),
                                      "720p": frame_bytes(1280, 720)}
    eng.close()
    print(json.dumps({"tool": "resize_rate", "frames": nf, "pix_fmt": FMT, "lut": 33, "interp": "tetrahedral",
                      "precision": "strict", "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
                      "hbm_peak_tb_s": HBM_PEAK / 1e12, "device": torch.cuda.get_device_name(0), "results": res}))


if __name__ == "__main__":
    main()
