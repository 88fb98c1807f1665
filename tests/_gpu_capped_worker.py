"""Worker of tests/test_gpu_deep_waves.py: a fresh child process whose environment caps the persistent grids (LUTR_MAX_WAVES,
DESIGN.md's knob appendix) so that frames of 1.6 to 3.4 Mpx run the tile loops as deep as a long launch does.

    python tests/_gpu_capped_worker.py OUT_DIR CASE_ID [CASE_ID ...]

For every case of tests/_deep_content.py named on the command line, in that order and on ONE LutEngine(0) under
set_variant("vec_lds"): build the seeded source, apply into sentinel-filled destinations with the tile counters armed, and save
the output planes, the counters and `last_kernel` as OUT_DIR/<id>.npz.  A line `[case <id>]` goes to stderr in front of each apply,
so that the parent can tell which LUTR_DEBUG lines belong to it.  No reference is computed here: the parent does that, from scratch.
"""
import json
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from lut_renderer_amd.engine import LutEngine  # noqa: E402
from tests import _deep_content as dc  # noqa: E402


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16) if a.dtype == np.uint16 else np.ascontiguousarray(a)).to("cuda:0")


def _sentinel(shape, depth):
    if depth > 8:
        return torch.full(shape, -1, dtype=torch.int16, device="cuda:0")
    return torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda:0")


def _host(t, depth):
    a = t.cpu().numpy()
    return a.view(np.uint16) if depth > 8 else a


def _with_spare_row(a, sentinel_depth=None):
    """A batch [F, H, W] on frame strides of H + 1 rows: (the [F, H + 1, W] tensor, its [F, H, W] view).  `a`'s samples go into the
    view, or -- for a destination -- the whole tensor is filled with the sentinel of `sentinel_depth`."""
    f, h, w = a.shape
    if sentinel_depth is not None:
        big = _sentinel((f, h + 1, w), sentinel_depth)
    else:
        frames_ = _dev(a)
        big = torch.zeros((f, h + 1, w), dtype=frames_.dtype, device="cuda:0")
        big[:, :h] = frames_
    return big, big[:, :h]


def run_case(eng, case, tmp_dir):
    lut, _ = dc.make_lut(case["lut"], tmp_dir)
    eng.set_lut(lut)
    eng.set_precision(case["prec"])
    src = dc.make_source(case)
    saved = {k: os.environ.get(k) for k in case["env"]}          # (a policy knob the launchers read per call)
    os.environ.update(case["env"])
    try:
        print(f"[case {case['id']}]", file=sys.stderr, flush=True)
        eng.tile_stats(True)
        if case["api"] == "yuv":
            dout = dc.YUV_FMT[case["ofmt"] or case["fmt"]][0]
            kw = dict(case["kw"])
            if case["ofmt"]:
                kw["out_pix_fmt"] = case["ofmt"]
            if case["shard"]:
                kw["row0"], kw["rows"] = case["shard"]
            if src[0].ndim == 3:
                keep = [_with_spare_row(p) for p in src]
                out = [_with_spare_row(p, dout) for p in src]
                eng.apply_yuv([v for _, v in keep], [v for _, v in out], pix_fmt=case["fmt"], interp=case["mode"], **kw)
                dst = [big for big, _ in out]                     # (the spare rows are saved too: they must keep the sentinel)
            else:
                dst = [_sentinel(p.shape, dout) for p in src]
                eng.apply_yuv([_dev(p) for p in src], dst, pix_fmt=case["fmt"], interp=case["mode"], **kw)
            planes = [_host(t, dout) for t in dst]
        elif case["api"] == "rgb":
            dst = [_sentinel(p.shape, 10) for p in src]
            eng.apply_rgb([_dev(p) for p in src], dst, depth=10, interp=case["mode"])
            planes = [_host(t, 10) for t in dst]
        else:
            bits = dc.PACKED[case["fmt"]][0]
            dst = _sentinel(src.shape, bits)
            eng.apply_packed(_dev(src), dst, pix_fmt=case["fmt"], interp=case["mode"])
            planes = [_host(dst, bits)]
        st = eng.tile_stats(False)
        kern = eng.last_kernel
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    return planes, st, kern


def main():
    out_dir = Path(sys.argv[1])
    ids = sys.argv[2:]
    with LutEngine(0) as eng:
        eng.set_variant("vec_lds")
        for cid in ids:
            case = dc.BY_ID[cid]
            planes, st, kern = run_case(eng, case, out_dir)
            np.savez(out_dir / f"{cid}.npz", kernel=kern, stats=json.dumps({k: int(v) for k, v in st.items()}),
                     **{f"p{i}": p for i, p in enumerate(planes)})
    print("[done]", file=sys.stderr, flush=True)


if __name__ == "__main__":
    main()
