"""Child process of tests/test_gpu_yuv2rgb.py::test_generic_kernel_many_trips_deep -- TEST INFRASTRUCTURE ONLY.

Started with LUTR_MAX_BLOCKS in its environment (the variable is read once per process): runs k_yuv2rgb_generic on the frames
the parent names by seed and writes what came back into an .npz for the parent to compare with the reference.

    python tests/_yuv2rgb_stride_worker.py <cube> <out.npz> <w> <h> <nframes> <din> <out_fmt>
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def source(w, h, nframes, din):
    """The frames of the case, one [F,H,W] array per plane (4:2:0)."""
    from lut_renderer_amd import frames
    fs = [frames.natural_yuv(w, h, din, 1, 1, k=90 + i) for i in range(nframes)]
    return [np.stack([f[i] for f in fs]) for i in range(3)]


def main(argv):
    import torch
    from lut_renderer_amd.engine import LutEngine
    cube_path, out = argv[0], argv[1]
    w, h, nf, din = (int(v) for v in argv[2:6])
    out_fmt = argv[6]
    src = source(w, h, nf, din)
    with LutEngine(0) as eng:
        eng.load_cube(cube_path)
        eng.set_variant("generic")
        dev = [torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).to(eng.device) for p in src]
        got = eng.apply_yuv_to_rgb(dev, pix_fmt="yuv420p" + ("" if din == 8 else f"{din}le"), out_pix_fmt=out_fmt)
        torch.cuda.synchronize()
        kernel = eng.last_kernel
        arrays = [got] if isinstance(got, torch.Tensor) else list(got)
        np.savez(out, kernel=np.array(kernel), **{f"p{i}": t.cpu().numpy() for i, t in enumerate(arrays)})
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
