"""`HostPipeline` on the stage-stack routes (DESIGN.md 3.21 .. 3.27) on the GPU: the bytes the pipeline drains are, bit for bit,
those of the same frames through one direct call of the route's engine entry.  16 x 8 frames -- two of the vector kernels'
8-sample units and one 4:2:0 block row pair -- and 3 frames with batch=2, slots=2: a full batch, a short one, and a slot that is
used twice.  The kernels themselves are pinned elsewhere (test_gpu_stack, test_gpu_matte, test_gpu_rgbstack, test_gpu_y2rstack);
what is tested here is which entry a batch goes through, with which arguments, and how its source and destination are viewed."""
import faulthandler
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import cube, frames
from lut_renderer_amd.cdl import read_cdl
from lut_renderer_amd.params import strength_keys

GOLDEN = Path(__file__).resolve().parent / "golden"
W, H, NF = 16, 8, 3
KEYS = "0:0.25,2:1.0"


@pytest.fixture(scope="module")
def eng(cube_dir):
    """The module's one engine: log709_33 as the lattice, gamma1024 (cubic) as the 1D LUT."""
    from lut_renderer_amd.engine import LutEngine
    e = LutEngine(0)
    e.load_cube(cube_dir / "log709_33.cube")
    e.set_lut1d(cube.read_lut1d(GOLDEN / "lut1d" / "gamma1024.cube"), "cubic")
    yield e
    e.close()


@pytest.fixture(autouse=True)
def time_limit():
    """A case that hangs ends the process with a traceback (the neighbours' child processes have a timeout of 180 s)."""
    faulthandler.dump_traceback_later(180, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(planes, device):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to(device)
            for p in planes]


def _bytes(out):
    """What a direct call returned -- planes [F,h,w] or one image [F,H,W,C] -- as rawvideo: frame after frame, plane after plane."""
    planes = [out] if hasattr(out, "shape") else list(out)
    host = [p.cpu().numpy() for p in planes]
    return b"".join(p[i].tobytes() for i in range(NF) for p in host)


def _drained(pipe, fs):
    raw = [b"".join(p.tobytes() for p in f) for f in fs]
    assert all(len(r) == pipe.fin.frame_bytes for r in raw)
    state = {"i": 0, "out": b"", "batches": []}

    def fill(buf, n):
        k = min(n, NF - state["i"])
        for j in range(k):
            buf[j * len(raw[0]):(j + 1) * len(raw[0])] = np.frombuffer(raw[state["i"] + j], np.uint8)
        state["i"] += k
        return k

    def drain(buf, n):
        state["out"] += bytes(buf)
        state["batches"].append(n)

    assert pipe.run(fill, drain) == NF and state["batches"] == [2, 1]
    return state["out"]


def _stacked(fs):
    return [np.stack([f[i] for f in fs]) for i in range(len(fs[0]))]


@pytest.mark.gpu
def test_yuv_stack_route(eng):
    from lut_renderer_amd.stream import HostPipeline
    grade = read_cdl(GOLDEN / "cdl" / "shot.cc")
    fs = [frames.natural_yuv(W, H, 10, 1, 1, k=60 + i) for i in range(NF)]
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
    want = eng.apply_yuv_stack(_dev(_stacked(fs), eng.device), stages="lut1d,cdl,lut3d", cdl=grade, **names)
    pipe = HostPipeline(eng, "yuv420p10le", W, H, batch=2, slots=2, out_pix_fmt="yuv422p10le", stages="lut1d,cdl,lut3d", cdl=grade)
    assert _drained(pipe, fs) == _bytes(want)


@pytest.mark.gpu
def test_yuv_stack_route_with_strength_keys_and_a_matte_per_frame(eng, tmp_path):
    import torch
    from lut_renderer_amd.stream import HostPipeline, MatteReader
    grade = read_cdl(GOLDEN / "cdl" / "shot.cc")
    fs = [frames.natural_yuv(W, H, 10, 1, 1, k=70 + i) for i in range(NF)]
    rng = np.random.default_rng(23)
    mattes = rng.integers(0, 256, (NF, H, W), dtype=np.uint8)
    (tmp_path / "m.gray").write_bytes(mattes.tobytes())
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
    want = eng.apply_yuv_stack(_dev(_stacked(fs), eng.device), stages="lut1d,cdl,lut3d", cdl=grade, **names,
                               strength=strength_keys(KEYS)(0, NF), matte=torch.from_numpy(mattes).to(eng.device))
    reader = MatteReader(tmp_path / "m.gray", "gray", W, H)
    assert reader.still is None                                        # (three frames: a matte per frame, read with every batch)
    pipe = HostPipeline(eng, "yuv420p10le", W, H, batch=2, slots=2, out_pix_fmt="yuv422p10le", stages="lut1d,cdl,lut3d", cdl=grade,
                        strength_keys=KEYS, matte=reader)
    try:
        got = _drained(pipe, fs)
    finally:
        reader.close()
    assert got == _bytes(want)
    plain = eng.apply_yuv_stack(_dev(_stacked(fs), eng.device), stages="lut1d,cdl,lut3d", cdl=grade, **names)
    assert got != _bytes(plain)                                        # (the strength and the matte did reach the engine)


@pytest.mark.gpu
def test_rgb_stack_route(eng):
    from lut_renderer_amd.stream import HostPipeline
    grade = read_cdl(GOLDEN / "cdl" / "shot.cc")
    fs = [frames.natural_rgb(W, H, 10, k=80 + i) for i in range(NF)]
    want = eng.apply_rgb_stack(_dev(_stacked(fs), eng.device), pix_fmt="gbrp10le", out_pix_fmt="yuv420p10le", stages="cdl,lut3d",
                               cdl=grade)
    pipe = HostPipeline(eng, "gbrp10le", W, H, batch=2, slots=2, out_pix_fmt="yuv420p10le", rgb_stages="cdl,lut3d", cdl=grade)
    assert _drained(pipe, fs) == _bytes(want)


@pytest.mark.gpu
def test_yuv_stack_to_rgb_route(eng):
    from lut_renderer_amd.stream import HostPipeline
    fs = [frames.natural_yuv(W, H, 10, 1, 1, k=90 + i) for i in range(NF)]
    want = eng.apply_yuv_stack_to_rgb(_dev(_stacked(fs), eng.device), pix_fmt="yuv420p10le", out_pix_fmt="rgb48le",
                                      stages="lut1d,lut3d")
    assert tuple(want.shape) == (NF, H, W, 3)
    pipe = HostPipeline(eng, "yuv420p10le", W, H, batch=2, slots=2, rgb_out="rgb48le", rgb_out_stages="lut1d,lut3d")
    assert _drained(pipe, fs) == _bytes(want)
