"""Worker of tests/test_gpu_rgbmatrix.py::test_lds_and_global_tables_give_the_same_bytes -- TEST INFRASTRUCTURE ONLY.

Where the stack kernels read the CDL and 1D tables (LDS or global memory) is read from LUTR_STACK_LDS when the
kernel is launched; the parent starts this file once per setting and compares what it writes to stdout byte for byte: the output
planes of a few `apply_yuv_stack` calls with a matrix stage at depths whose tables fit LDS and ones that do not.
The placement that ran goes to stderr, one digit per call.

    python tests/_gpu_rgbmatrix_worker.py LUT3D.cube LUT1D.cube CDL.cc MATRIX.spimtx
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def main(lut3d, lut1d, cc, spimtx):
    import torch
    from lut_renderer_amd import frames
    from lut_renderer_amd.cdl import read_cdl
    from lut_renderer_amd.engine import LutEngine
    from lut_renderer_amd.rgbmatrix import read_rgb_matrix
    out = []
    grade, mtx = read_cdl(cc), read_rgb_matrix(spimtx)
    with LutEngine(0) as eng:
        eng.load_cube(lut3d)
        eng.load_lut1d(lut1d, "cubic")
        for depth, a, b, stages in ((8, (1, 1), "yuv420p", "lut1d,matrix,lut3d"), (10, (1, 1), "yuv422p10le", "matrix,cdl,lut1d,lut3d"),
                                    (12, (1, 0), "yuv420p12le", "matrix,lut1d"), (12, (1, 1), "yuv420p12le", "cdl,matrix,lut3d"),
                                    (16, (1, 1), "yuv420p16le", "lut1d,matrix")):
            fs = [frames.make_yuv("natural", 136, 36, depth, *a, k=3 + i) for i in range(2)]
            src = [np.stack([f[i] for f in fs]) for i in range(3)]
            dev = [torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).to(eng.device) for p in src]
            name = {(1, 1): "420", (1, 0): "422", (0, 0): "444"}[a]
            got = eng.apply_yuv_stack(dev, pix_fmt=f"yuv{name}p" + ("" if depth == 8 else f"{depth}le"), out_pix_fmt=b, stages=stages,
                                      cdl=grade if "cdl" in stages else None, rgb_matrix=mtx)
            assert eng.last_kernel.startswith("k_yuv_stack_mtx_vec<"), eng.last_kernel
            out += [t.cpu().numpy().tobytes() for t in got]
            sys.stderr.write(eng.last_kernel.split(">")[0][-1])         # the placement that ran: the parent checks the five digits
    sys.stdout.buffer.write(b"".join(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:5]))
