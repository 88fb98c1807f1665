"""Worker of tests/test_gpu_rgbmatrix_stride.py -- TEST INFRASTRUCTURE ONLY.

A fresh child process whose environment caps every grid-stride grid (LUTR_MAX_BLOCKS) so that the matrix forms of the stack
kernels run each thread for several trips on a small frame, the last one partial.

    python tests/_gpu_rgbmatrix_stride_worker.py OUT.npz LUT3D.cube LUT1D.cube MATRIX.spimtx vec|generic

One `apply_yuv_stack` call on 136 x 36 x 3 frames of 4:2:0 -> 4:2:2 at 10 bit with [lut1d, matrix, lut3d], into
sentinel-filled destinations with a spare row a frame and spare columns, all of which is saved with `last_kernel`.  No reference
is computed here: the parent does that.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

W, H, NF = 136, 36, 3
STAGES = "lut1d,matrix,lut3d"
SPARE_ROWS, SPARE_COLS = 1, 8


def source():
    from lut_renderer_amd import frames
    fs = [frames.make_yuv("natural", W, H, 10, 1, 1, k=40 + i) for i in range(NF)]
    return [np.stack([f[i] for f in fs]) for i in range(3)]


def main(out, lut3d, lut1d, spimtx, which):
    import torch
    from lut_renderer_amd.engine import LutEngine
    from lut_renderer_amd.rgbmatrix import read_rgb_matrix
    src = [torch.from_numpy(p.view(np.int16)).to("cuda:0") for p in source()]
    shapes = [(H, W), (H, W // 2), (H, W // 2)]                      # 4:2:2 out
    big = [torch.full((NF, r + SPARE_ROWS, c + SPARE_COLS), 0x5a5a, dtype=torch.int16, device="cuda:0") for r, c in shapes]
    views = [t[:, :r, :c] for t, (r, c) in zip(big, shapes)]
    with LutEngine(0) as eng:
        eng.load_cube(lut3d)
        eng.load_lut1d(lut1d, "cubic")
        eng.set_variant("generic" if which == "generic" else "auto")
        eng.apply_yuv_stack(src, views, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=STAGES, rgb_matrix=read_rgb_matrix(spimtx))
        kern = eng.last_kernel
        planes = [t.cpu().numpy().view(np.uint16) for t in big]
    np.savez(out, kernel=kern, **{f"p{i}": p for i, p in enumerate(planes)})
    print("[done]", file=sys.stderr, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:6]))
