"""Worker of tests/test_gpu_lut1d.py::test_lds_and_global_tables_give_the_same_bytes -- TEST INFRASTRUCTURE ONLY.

The placement of the 1D table (LDS or global memory) is read from LUTR_L1D_LDS when the kernel is launched; the
parent starts this file once per setting and compares what it writes to stdout byte for byte: the output planes of a few
`apply_yuv_lut1d` calls at the depths whose table fits LDS (8, 10, 12) and one that does not (16), then of `apply_rgb_lut1d`.

    python tests/_gpu_lut1d_worker.py LUT3D.cube LUT1D.cube
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main(lut3d, lut1d):
    import torch
    from lut_renderer_amd import frames
    from lut_renderer_amd.engine import LutEngine
    out = []
    with LutEngine(0) as eng:
        eng.load_cube(lut3d)
        eng.load_lut1d(lut1d, "cubic")
        for depth, a, b, interp in ((8, (1, 1), "yuv420p", "tetrahedral"), (10, (1, 1), "yuv422p10le", "tetrahedral"),
                                    (10, (0, 0), "yuv444p10le", None), (12, (1, 0), "yuv420p12le", "trilinear"),
                                    (16, (1, 1), "yuv420p16le", "nearest")):
            fs = [frames.make_yuv("natural", 136, 36, depth, *a, k=3 + i) for i in range(2)]
            src = [np.stack([f[i] for f in fs]) for i in range(3)]
            dev = [torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).to(eng.device) for p in src]
            name = {(1, 1): "420", (1, 0): "422", (0, 0): "444"}[a]
            got = eng.apply_yuv_lut1d(dev, pix_fmt=f"yuv{name}p" + ("" if depth == 8 else f"{depth}le"), out_pix_fmt=b, interp=interp)
            assert eng.last_kernel.startswith("k_yuv_l1d_vec<"), eng.last_kernel
            out += [t.cpu().numpy().tobytes() for t in got]
        for depth in (8, 10, 16):
            rgb = frames.make_rgb("natural", 136, 36, depth, k=2)
            dev = [torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).to(eng.device) for p in rgb]
            got = eng.apply_rgb_lut1d(dev, depth=depth)
            assert eng.last_kernel.startswith("k_rgb_l1d<"), eng.last_kernel
            out += [t.cpu().numpy().tobytes() for t in got]
    sys.stdout.buffer.write(b"".join(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
