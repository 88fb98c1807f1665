"""Worker of tests/test_gpu_stride_trips.py: a fresh child process whose environment caps every grid-stride grid (LUTR_MAX_BLOCKS,
DESIGN.md's knob appendix) so that frames of a few thousand units run each thread for several trips, the last one partial.

    python tests/_gpu_stride_worker.py OUT_DIR CASE_ID [CASE_ID ...]

For every case of tests/_stride_cases.py named on the command line, in that order and on ONE LutEngine(0): build the source,
apply into sentinel-filled destinations (views with a spare row a frame and spare columns, all of which is saved) and write the
planes and `last_kernel` to OUT_DIR/<id>.npz.  A line `[case <id>]` goes to stderr in front of each call, so that the parent can
tell which LUTR_DEBUG lines belong to it.  No reference is computed here: the parent does that, from scratch.
"""
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from lut_renderer_amd.engine import LutEngine  # noqa: E402
from tests import _stride_cases as sc  # noqa: E402

_VIEW = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}


def _dev(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(_VIEW.get(a.dtype, a.dtype))).to("cuda:0")


def _src_view(case, a):
    """The source array on the device: dense, or for a `pad` case a view of rows of RAGGED_COLS samples."""
    t = _dev(a)
    if not case["pad"]:
        return t
    big = torch.zeros(t.shape[:2] + (sc.RAGGED_COLS,) + t.shape[3:], dtype=t.dtype, device="cuda:0")
    big[:, :, :t.shape[2]] = t
    return big[:, :, :t.shape[2]]


def _dst(case):
    """[(the sentinel-filled tensor, its destination view)] per plane of the case's output."""
    out = []
    for shape, dt in sc.out_layout(case):
        fill = sc.SENTINEL[np.dtype(dt)]
        tdt = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.int16, np.dtype(np.float32): torch.float32}[np.dtype(dt)]
        big = torch.full(sc.spare_shape(case, shape), -1 if tdt == torch.int16 else fill, dtype=tdt, device="cuda:0")
        out.append((big, big[:, :shape[1], :shape[2]]))
    return out


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def run_case(eng, case):
    res = sc.resources()
    host = sc.source(case)
    src = [_src_view(case, p) for p in sc.container(case, host["src"])]
    dst = _dst(case)
    views = [v for _, v in dst]
    kind = case["kind"]
    eng.set_variant(case["variant"])
    saved = {k: os.environ.get(k) for k in case["env"]}          # (a placement knob the launchers read per call)
    os.environ.update(case["env"])
    try:
        print(f"[case {case['id']}]", file=sys.stderr, flush=True)
        if kind == "stack":
            kw = {}
            if case["strength"] is not None:
                kw["strength"] = case["strength"]
            if case["matte"]:
                depth, _, invert = case["matte"]
                m = host["matte"]
                kw.update(matte=_src_view(case, m) if m.ndim == 3 else _src_view(case, m[None])[0], matte_depth=depth, matte_invert=invert)
            eng.apply_yuv_stack(src, views, pix_fmt=sc.yuv_name(case["din"], case["a"]), out_pix_fmt=sc.yuv_name(case["dout"], case["b"]),
                                stages=case["stages"], cdl=res["cdl"], **kw)
        elif kind == "lut1d":
            eng.apply_yuv_lut1d(src, views, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", interp=case["mode"])
        elif kind == "rgb_l1d":
            eng.apply_rgb_lut1d(src, views, depth=10)
        elif kind == "alpha":
            eng.apply_yuv(src, views, pix_fmt="yuva420p10le" if case["src_alpha"] else "yuv420p10le",
                          out_pix_fmt=sc.yuv_name(case["dout"], "420", alpha=True))
        elif kind == "yuv":
            eng.apply_yuv(src, views, pix_fmt="yuv420p10le", row0=case["shard"][0], rows=case["shard"][1])
        elif kind == "dither":
            eng.apply_yuv(src, views, pix_fmt="yuv420p10le", dither="error_diffusion")
        elif kind == "rgb":
            eng.apply_rgb(src, views, depth=10)
        elif kind == "packed":
            eng.apply_packed(src[0], views[0], pix_fmt=case["fmt"])
        elif kind == "rgbf":
            eng.apply_rgb_float(src, views)
        elif kind == "rgbaf":
            eng.apply_rgb_float(src, views, alpha_mode="premultiplied")
        elif kind == "v210":
            eng.apply_yuv(src, views, pix_fmt="v210", out_pix_fmt="yuv422p10le", width=case["w"])
        elif kind == "semi":
            eng.apply_yuv(src, views, pix_fmt=case["fmt"], out_pix_fmt=case["fmt"])
        else:
            raise ValueError(kind)
        kern = eng.last_kernel
        planes = [_host(big) for big, _ in dst]
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return planes, kern


def main():
    out_dir = Path(sys.argv[1])
    res = sc.resources()
    with LutEngine(0) as eng:
        eng.set_lut(res["lut"])
        eng.set_lut1d(*res["l1"])
        for cid in sys.argv[2:]:
            planes, kern = run_case(eng, sc.BY_ID[cid])
            np.savez(out_dir / f"{cid}.npz", kernel=kern, **{f"p{i}": p for i, p in enumerate(planes)})
    print("[done]", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
