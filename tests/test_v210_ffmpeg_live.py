"""The v210 layout of DESIGN.md 3.14 against a real `ffmpeg` binary: the bytes its v210 encoder writes for a `testsrc` frame,
unpacked with `v210.to_planar`, must be ffmpeg's own yuv422p10le of the same frame.  Skipped unless `ffmpeg` is on PATH (none is
in the build image): this is what pins the layout, written from recall, the day an FFmpeg is at hand."""
import shutil
import subprocess

import numpy as np
import pytest

FFMPEG = shutil.which("ffmpeg")

pytestmark = pytest.mark.skipif(FFMPEG is None, reason="no ffmpeg binary on PATH (the v210 layout stays unpinned)")


def _testsrc(w, h, tail):
    cmd = [FFMPEG, "-v", "error", "-f", "lavfi", "-i", f"testsrc=size={w}x{h}:rate=1", "-frames:v", "1", "-vf", "format=yuv422p10le"]
    r = subprocess.run(cmd + tail + ["-f", "rawvideo", "-"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return r.stdout


@pytest.mark.parametrize("size", [(96, 8), (100, 6), (1280, 4)])
def test_to_planar_of_ffmpegs_v210_is_ffmpegs_yuv422p10le(size):
    from lut_renderer_amd.v210 import frame_bytes, row_bytes, to_planar, to_v210
    w, h = size
    packed = _testsrc(w, h, ["-c:v", "v210"])
    planar = _testsrc(w, h, ["-c:v", "rawvideo", "-pix_fmt", "yuv422p10le"])
    assert len(packed) == frame_bytes(w, h) and len(planar) == 2 * (w * h + 2 * ((w + 1) // 2) * h)
    buf = np.frombuffer(packed, "<u4").reshape(h, row_bytes(w) // 4)
    flat = np.frombuffer(planar, "<u2")
    cw = (w + 1) // 2
    want = [flat[:w * h].reshape(h, w), flat[w * h:w * h + cw * h].reshape(h, cw), flat[w * h + cw * h:].reshape(h, cw)]
    got = to_planar(buf, w)
    assert all(np.array_equal(g, x) for g, x in zip(got, want))
    assert not (buf >> 30).any()
    # our packing of ffmpeg's planes differs from ffmpeg's bytes at most in the slots beyond the frame (ffmpeg writes zeros there)
    assert all(np.array_equal(g, x) for g, x in zip(to_planar(to_v210(want, w), w), want))
