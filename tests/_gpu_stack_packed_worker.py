"""Worker of tests/test_gpu_stack_packed.py -- TEST INFRASTRUCTURE ONLY.

The knobs the stack kernels on packed 4:2:2 / v210 frames share with the planar ones are read when a kernel is
launched: LUTR_STACK_LDS (where the CDL and 1D tables are read) and LUTR_MAX_BLOCKS (the cap on the workgroups of a grid-stride
launch).  The parent starts this file in a fresh process per setting; the cases below are the parent's (CASES), their output
buffers go to OUT_DIR/<id>.npz with the kernel that ran, and `[case <id>]` on stderr goes ahead of each case's `[lutr gs]` debug
lines.

    python tests/_gpu_stack_packed_worker.py OUT_DIR LUT3D.cube LUT1D.cube CDL.cc ID [ID ...]
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

STAGES = "lut1d,cdl,lut3d"
#: id -> (source name, destination name, w, h, frames); the `_small` ones have rows no vector kernel can take
CASES = {
    "uyvy_uyvy": ("uyvy422", "uyvy422", 136, 36, 6),
    "v210_v210": ("v210", "v210", 144, 36, 6),
    "y210_422p": ("y210le", "yuv422p10le", 136, 36, 6),
    "v210_420p": ("v210", "yuv420p", 144, 36, 6),
    "uyvy_uyvy_small": ("uyvy422", "uyvy422", 67, 21, 6),
    "v210_422p_small": ("v210", "yuv422p10le", 67, 21, 6),
}


def held(planar, name, w):
    """planar samples (numpy) in the container `name`: a list of planes, or the one buffer of a packed 4:2:2 / v210 side"""
    from lut_renderer_amd import packedyuv, v210
    from lut_renderer_amd.formats import yuv_side
    side = yuv_side(name)
    if side.nplanes == 3:
        return list(planar)
    return v210.to_v210(planar, w) if name == "v210" else packedyuv.to_packed(planar, name)


def to_device(buf, device):
    """a list of planes or one buffer -> tensors as the engine takes them (16-bit codes as int16, v210 words as int32)"""
    import torch

    def one(p):
        p = np.ascontiguousarray(p)
        return torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p.view(np.int32) if p.dtype == np.uint32 else p).to(device)
    return [one(p) for p in buf] if isinstance(buf, list) else one(buf)


def source(name, w, h, nf):
    """The planar samples of a case and the same samples in the container `name`."""
    from lut_renderer_amd import frames
    from lut_renderer_amd.formats import yuv_side
    side = yuv_side(name)
    fs = [frames.make_yuv("natural", w, h, side.depth, side.csx, side.csy, k=5 + 3 * i) for i in range(nf)]
    planar = [np.stack([f[i] for f in fs]) for i in range(3)]
    return planar, held(planar, name, w)


def main(out_dir, lut3d, lut1d, cc, ids):
    from lut_renderer_amd.cdl import read_cdl
    from lut_renderer_amd.engine import LutEngine
    grade = read_cdl(cc)
    with LutEngine(0) as eng:
        eng.load_cube(lut3d)
        eng.load_lut1d(lut1d, "cubic")
        for cid in ids:
            a, b, w, h, nf = CASES[cid]
            _planar, buf = source(a, w, h, nf)
            sys.stderr.write(f"[case {cid}]\n")
            sys.stderr.flush()
            got = eng.apply_yuv_stack_packed(to_device(buf, eng.device), pix_fmt=a, out_pix_fmt=b, stages=STAGES, cdl=grade, width=w)
            eng.sync()
            got = got if isinstance(got, list) else [got]
            planes = {f"p{i}": t.cpu().numpy() for i, t in enumerate(got)}
            np.savez(Path(out_dir) / f"{cid}.npz", kernel=np.array(eng.last_kernel), **planes)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5:]))
