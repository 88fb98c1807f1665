"""The matrix forms of the stack kernels several grid-stride trips deep, on small frames.

A child process (tests/_gpu_rgbmatrix_stride_worker.py) runs one vector case and one generic case on 136 x 36 x 3 frames under
LUTR_MAX_BLOCKS=2 and =1: 1836 vector units and 3672 generic units against 512 / 256 threads a trip are four to fifteen trips,
the last one partial, with consecutive trips of a thread in different frames -- the stride itself, the output words zeroed again,
the fences across trips, the LDS table read on later trips.  Every (case, cap) is a child of its own with its own time limit;
every plane is compared bit for bit with the twin, the spare row and columns around it included (they keep the sentinel), and
the child's `[lutr gs]` line proves the regime."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube
from lut_renderer_amd.rgbmatrix import read_rgb_matrix
from tests import _gpu_rgbmatrix_stride_worker as wk
from tests import _matrix_twin as twin

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
SPIMTX = GOLDEN / "matrix" / "bt2020_to_709.spimtx"
LUT1D = GOLDEN / "lut1d" / "gamma1024.cube"
CHILD_LIMIT_S = 180          # a limit, not a measurement: a child runs for seconds
#: which -> (the family of its `[lutr gs]` line, its units: 4 luma samples x 2 rows a vector thread, a 2 x 2 union block a generic one)
CASES = {"vec": ("k_yuv_stack_mtx_vec", (wk.W // 4) * (wk.H // 2) * wk.NF), "generic": ("k_yuv_stack_mtx_generic", (wk.W // 2) * (wk.H // 2) * wk.NF)}
_ref = {}


def test_every_case_reaches_its_regime():
    for family, units in CASES.values():
        for cap in (2, 1):
            per_trip = 256 * cap
            assert -(-units // per_trip) >= 3 and units % per_trip != 0 and (units // wk.NF) % per_trip != 0, (family, cap)


def _reference(cube_dir):
    if not _ref:
        lut, l1 = cube.read_lut(cube_dir / "log709_33.cube"), cube.read_lut1d(LUT1D)
        k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 1, 0)
        src = wk.source()
        per = [twin.apply(wk.STAGES.split(","), k, 10, 10, 1, 1, 1, 0, [p[i] for p in src], lut=lut, mtx=read_rgb_matrix(SPIMTX),
                          l1d_tab=_native.lut1d_table(l1, "cubic", 10)) for i in range(wk.NF)]
        want = []
        for i in range(3):
            p = np.stack([f[i] for f in per]).astype(np.uint16)
            big = np.full((wk.NF, p.shape[1] + wk.SPARE_ROWS, p.shape[2] + wk.SPARE_COLS), 0x5a5a, np.uint16)
            big[:, :p.shape[1], :p.shape[2]] = p
            big.setflags(write=False)
            want.append(big)
        _ref["want"] = want
    return _ref["want"]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [2, 1])
@pytest.mark.parametrize("which", list(CASES))
def test_stride_case(cube_dir, tmp_path, which, cap):
    family, units = CASES[which]
    env = dict(os.environ, LUTR_MAX_BLOCKS=str(cap), LUTR_DEBUG="1")
    env.pop("LUTR_STACK_LDS", None)
    out = tmp_path / "out.npz"
    try:
        p = subprocess.run([sys.executable, str(ROOT / "tests" / "_gpu_rgbmatrix_stride_worker.py"), str(out), str(cube_dir / "log709_33.cube"),
                            str(LUT1D), str(SPIMTX), which], env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode("utf-8", "replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"the LUTR_MAX_BLOCKS={cap} child did not finish within {CHILD_LIMIT_S} s; its last lines:\n{err[-3000:]}", pytrace=False)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = dict(re.findall(r"^\[lutr gs\] (\S+) (units \d+ blocks \d+)$", p.stderr, re.M))
    assert lines.get(family) == f"units {units} blocks {cap}", p.stderr[-2000:]
    with np.load(out) as z:
        kern, planes = str(z["kernel"]), [z[f"p{i}"] for i in range(3)]
    assert kern == ("k_yuv_stack_mtx_vec<1,1,1,1,1,0,0,1>" if which == "vec" else family) + "[lut1d,matrix,lut3d:2]", kern
    for i, (got, want) in enumerate(zip(planes, _reference(cube_dir))):
        assert got.shape == want.shape
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{which} cap {cap}: plane {i} differs at {len(bad)} samples, first {bad[0].tolist()} got "
                                 f"{got[tuple(bad[0])]} want {want[tuple(bad[0])]}")
