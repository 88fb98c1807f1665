"""The per-code table of DESIGN.md 3.20 against a real `ffmpeg` binary: `lut1d` on a gbrp / gbrp10le / gbrp16le frame that holds
every code, in the five modes, must give lutr_lut1d_table's entries.  Skipped unless `ffmpeg` is on PATH (none is in the build
image): this is what pins the restated semantics the day an FFmpeg is at hand.  Cosine is report-only: it depends on the C
library's cosf."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

FFMPEG = shutil.which("ffmpeg")
GOLDEN = Path(__file__).resolve().parent / "golden" / "lut1d"

pytestmark = pytest.mark.skipif(FFMPEG is None, reason="no ffmpeg binary on PATH (lut1d's semantics stay unpinned)")


def _lut1d(path, mode, pix_fmt, planes, w, h):
    cmd = [FFMPEG, "-v", "error", "-f", "rawvideo", "-pix_fmt", pix_fmt, "-s", f"{w}x{h}", "-i", "-", "-vf",
           f"lut1d=file={path}:interp={mode}", "-f", "rawvideo", "-pix_fmt", pix_fmt, "-"]
    r = subprocess.run(cmd, input=b"".join(p.tobytes() for p in planes), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return r.stdout


@pytest.mark.parametrize("name", ["curve17", "gamma1024", "invert33", "range64"])
@pytest.mark.parametrize("pix_fmt,depth", [("gbrp", 8), ("gbrp10le", 10), ("gbrp16le", 16)])
@pytest.mark.parametrize("mode", ["nearest", "linear", "cosine", "cubic", "spline"])
def test_ffmpegs_lut1d_gives_the_table(name, pix_fmt, depth, mode, capsys):
    from lut_renderer_amd import _native, cube
    l1 = cube.read_lut1d(GOLDEN / f"{name}.cube")
    tab = _native.lut1d_table(l1, mode, depth)
    n = 1 << depth
    w, h = 256, n // 256
    dt = np.uint8 if depth == 8 else np.dtype("<u2")
    ramp = np.arange(n).astype(dt).reshape(h, w)
    out = np.frombuffer(_lut1d(GOLDEN / f"{name}.cube", mode, pix_fmt, [ramp] * 3, w, h), dt).reshape(3, n)    # G, B, R
    got = np.stack([out[2], out[0], out[1]]).astype(np.int64)
    diff = np.abs(got - tab.astype(np.int64))
    if mode == "cosine":
        with capsys.disabled():
            print(f"\n  cosine {name} {pix_fmt}: {int((diff != 0).sum())} of {diff.size} entries differ from ffmpeg, max {int(diff.max())}")
        return
    assert not diff.any(), (name, pix_fmt, mode, int((diff != 0).sum()), int(diff.max()))
