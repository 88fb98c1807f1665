"""Worker of tests/test_gpu_y2rstack.py's child-process comparisons -- TEST INFRASTRUCTURE ONLY.

Where the YUV -> RGB stack kernels read the CDL and 1D tables (LUTR_STACK_LDS) and how many workgroups a grid-stride launch gets
(LUTR_MAX_BLOCKS) are read from the environment when a kernel is launched; the parent starts this file once per setting, as a
fresh process, and compares what it writes to stdout byte for byte: the output of a few `apply_yuv_stack_to_rgb` calls on
136 x 36 x 2 frames.  The kernel of every call goes to stderr, one name per line.

    python tests/_gpu_y2rstack_worker.py LUT3D.cube LUT1D.cube CDL.cc
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

CASES = (("yuv420p", "rgba", "lut1d,cdl,lut3d"), ("yuv422p10le", "gbrp10le", "lut1d,cdl,lut3d"),
         ("yuv420p10le", "rgb48le", "lut3d:trilinear,cdl"), ("yuv444p12le", "gbrp12le", "lut3d,lut1d"),
         ("yuv420p10le", "bgr24", "cdl,lut1d"), ("yuv420p16le", "gbrp16le", "lut1d,cdl"), ("yuv420p10le", "gbrp10le", "cdl,lut3d"))


def main(lut3d, lut1d, cc):
    import torch
    from lut_renderer_amd.cdl import read_cdl
    from lut_renderer_amd.engine import LutEngine
    from tests.test_gpu_y2rstack import _dev, _src
    out = []
    grade = read_cdl(cc)
    with LutEngine(0) as eng:
        eng.load_cube(lut3d)
        eng.load_lut1d(lut1d, "cubic")
        for pix_fmt, out_fmt, stages in CASES:
            src = _src(pix_fmt, "natural", 136, 36, nf=2, k=3)
            got = eng.apply_yuv_stack_to_rgb(_dev(src, eng.device), pix_fmt=pix_fmt, out_pix_fmt=out_fmt, stages=stages,
                                             cdl=grade if "cdl" in stages else None)
            torch.cuda.synchronize()
            assert eng.last_kernel.startswith("k_yuv2rgb_stack_vec<"), eng.last_kernel
            out += [t.cpu().numpy().tobytes() for t in ([got] if isinstance(got, torch.Tensor) else got)]
            sys.stderr.write(eng.last_kernel + "\n")
    sys.stdout.buffer.write(b"".join(out))
    return 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
