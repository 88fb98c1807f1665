"""Worker of tests/test_gpu_stack_semi.py -- TEST INFRASTRUCTURE ONLY.

The knobs the semi form of the stack kernels shares with the plain form are read when a kernel is launched:
LUTR_STACK_LDS (where the CDL and 1D tables are read) and LUTR_MAX_BLOCKS (the cap on the workgroups of a grid-stride launch).
The parent starts this file in a fresh process per setting; the cases below are the parent's (CASES), their output planes go to
OUT_DIR/<id>.npz with the kernel that ran, and `[case <id>]` on stderr goes ahead of each case's `[lutr gs]` debug lines.

    python tests/_gpu_stack_semi_worker.py OUT_DIR LUT3D.cube LUT1D.cube CDL.cc ID [ID ...]
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

STAGES = "lut1d,cdl,lut3d"
#: id -> (source name, destination name, w, h, frames)
CASES = {
    "p010_p010": ("p010le", "p010le", 136, 36, 6),
    "nv12_nv12": ("nv12", "nv12", 136, 36, 6),
    "p010_422p": ("p010le", "yuv422p10le", 136, 36, 6),
    "p010_nv12": ("p010le", "nv12", 136, 36, 6),
    "nv16_nv12_small": ("nv16", "nv12", 67, 21, 6),
    "p010_p010_small": ("p010le", "p010le", 67, 21, 6),
}


def source(name, w, h, nf):
    """The planar samples of a case and the same samples in the container `name`."""
    from lut_renderer_amd import frames, semiplanar
    from lut_renderer_amd.formats import yuv_side
    side = yuv_side(name)
    fs = [frames.make_yuv("natural", w, h, side.depth, side.csx, side.csy, k=5 + 3 * i) for i in range(nf)]
    planar = [np.stack([f[i] for f in fs]) for i in range(3)]
    return planar, (semiplanar.to_semi(planar, name) if side.nplanes == 2 else planar)


def main(out_dir, lut3d, lut1d, cc, ids):
    import torch
    from lut_renderer_amd.cdl import read_cdl
    from lut_renderer_amd.engine import LutEngine
    grade = read_cdl(cc)
    with LutEngine(0) as eng:
        eng.load_cube(lut3d)
        eng.load_lut1d(lut1d, "cubic")
        for cid in ids:
            a, b, w, h, nf = CASES[cid]
            _planar, held = source(a, w, h, nf)
            dev = [torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).to(eng.device) for p in held]
            sys.stderr.write(f"[case {cid}]\n")
            sys.stderr.flush()
            got = eng.apply_yuv_stack_semi(dev, pix_fmt=a, out_pix_fmt=b, stages=STAGES, cdl=grade)
            eng.sync()
            planes = {f"p{i}": t.cpu().numpy() for i, t in enumerate(got)}
            np.savez(Path(out_dir) / f"{cid}.npz", kernel=np.array(eng.last_kernel), **planes)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5:]))
