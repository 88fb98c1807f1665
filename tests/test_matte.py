"""A matte plane on the stage stack without a GPU: the facts about the normalisation the contract rests on, the
twin's identities and bounds, `formats.check_matte` and the refusals through every layer (each message names the option and the
matte), the argv, and the stream's matte reader."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lut_renderer_amd import cube, frames
from lut_renderer_amd.cdl import Cdl
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.formats import MATTE_PIX_FMTS, check_matte, check_stack_options
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _matte_twin as twin
from tests import _mix_twin as mix
from tests.test_mix import NAMES, REFUSED, _Eng, _lut, _pairs, _planes

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
F = np.float32
DEPTHS = list(range(8, 17))


# ------------------------------------------------------------------ the normalisation
@pytest.mark.parametrize("depth", DEPTHS)
def test_the_normalisation_is_monotone_at_most_1_and_1_at_the_top(depth):
    mm = (1 << depth) - 1
    t = twin.matte_t(np.arange(mm + 1), depth)
    assert t.dtype == F and t[0] == 0.0 and t[mm] == F(1.0)
    assert (np.diff(t) > 0).all() and (t <= F(1.0)).all()
    assert np.array_equal(twin.matte_t(np.arange(mm + 1), depth, invert=True), t[::-1])


def _triples(depth):
    """(q0, q1, a): at 8 bit every pair of codes against each of six matte codes, else 2^20 random triples with the extremes."""
    if depth == 8:
        a, b = _pairs(8)
        codes = np.array([0, 1, 127, 128, 254, 255])
        return np.tile(a, codes.size), np.tile(b, codes.size), np.repeat(codes, a.size)
    a, b = _pairs(depth)
    m = np.random.default_rng(100 + depth).integers(0, 1 << depth, a.size)
    m[:4] = [0, (1 << depth) - 1, (1 << depth) - 1, 0]
    return a, b, m


# ------------------------------------------------------------------ the identities
@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("s", [1.0, 0.37, 0.0])
def test_a_full_matte_is_the_strength_and_an_empty_one_is_the_source(depth, s):
    a, b, _ = _triples(depth)
    mm = (1 << depth) - 1
    full, none = np.full(a.shape, mm), np.zeros(a.shape, np.int64)
    want = mix.mix_codes(s, [a], [b])[0]
    assert np.array_equal(twin.weight(s, full, depth), np.full(a.shape, F(s)))         # w = s' exactly
    assert np.array_equal(twin.mix_codes(twin.weight(s, full, depth), [a], [b])[0], want)
    assert np.array_equal(twin.mix_codes(twin.weight(s, none, depth, invert=True), [a], [b])[0], want)
    assert np.array_equal(twin.mix_codes(twin.weight(s, none, depth), [a], [b])[0], a)
    assert np.array_equal(twin.mix_codes(twin.weight(s, full, depth, invert=True), [a], [b])[0], a)


@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("s", [1.0, 0.37, 1.0 / 3.0])
def test_the_mix_stays_between_source_and_grade(depth, s):
    a, b, m = _triples(depth)
    w = twin.weight(s, m, depth)
    assert w.dtype == F and (w >= 0).all() and (w <= F(1.0)).all()
    q = twin.mix_codes(w, [a], [b])[0]
    assert (q >= np.minimum(a, b)).all() and (q <= np.maximum(a, b)).all()
    exact = a + float(F(s)) * (m / ((1 << depth) - 1)) * (b - a)
    assert np.abs(q - exact).max() <= 0.5 + 2.0 ** (depth - 21)


@pytest.mark.parametrize("depth", [8, 10, 12, 16])
def test_invert_of_invert_and_the_clamp_above_the_top(depth):
    mm = (1 << depth) - 1
    m = np.arange(mm + 1)
    assert np.array_equal(twin.matte_t(mm - m, depth, invert=True), twin.matte_t(m, depth))
    if depth < 16:                                             # a 16-bit container may hold more than `depth` bits
        above = np.array([mm + 1, 2 * mm, 0xffff])
        assert np.array_equal(twin.matte_t(above, depth), np.full(3, F(1.0)))
        assert np.array_equal(twin.matte_t(above, depth, invert=True), np.zeros(3, F))


def test_a_matte_broadcasts_over_the_frames_and_moves_the_planes():
    """The whole twin on a 4:2:0 -> 4:2:2 batch: a still against the same matte per frame, a full matte against the strength's twin,
    and a matte edge inside a chroma block against the blend of two YUV results (which it is not)."""
    lut = cube.CubeLut(9, np.ones(3, F), np.random.default_rng(11).uniform(0.0, 1.0, (9, 9, 9, 3)).astype(F))
    fs = [frames.natural_yuv(38, 12, 10, 1, 1, k=i) for i in range(3)]
    src = [np.stack([f[i] for f in fs]) for i in range(3)]
    k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 1, 0)
    grade = Cdl(slope=(0.9, 1.1, 1.0), offset=(0.02, 0.0, -0.01), power=(1.2, 1.0, 0.9), saturation=0.8)
    res = dict(lut=lut, cdl=grade)
    s = [0.0, 1.0, 0.6]
    m = np.random.default_rng(2).integers(0, 256, (12, 38)).astype(np.uint8)
    m[3:9, 5:21] = 255
    still = twin.apply(("cdl", "lut3d"), s, m, 8, False, k, 10, 10, 1, 1, 1, 0, src, **res)
    per = twin.apply(("cdl", "lut3d"), s, np.stack([m] * 3), 8, False, k, 10, 10, 1, 1, 1, 0, src, **res)
    one = twin.apply(("cdl", "lut3d"), s, m[None], 8, False, k, 10, 10, 1, 1, 1, 0, src, **res)
    full = twin.apply(("cdl", "lut3d"), s, np.full((12, 38), 255, np.uint8), 8, False, k, 10, 10, 1, 1, 1, 0, src, **res)
    want = mix.apply(("cdl", "lut3d"), s, k, 10, 10, 1, 1, 1, 0, src, **res)
    for i in range(3):
        assert np.array_equal(still[i], per[i]) and np.array_equal(still[i], one[i]) and np.array_equal(full[i], want[i])
    assert not np.array_equal(still[0][2], want[0][2])
    # inside the rectangle the strength's planes, and a single frame gives the batch's frame
    assert np.array_equal(still[0][2][4:8, 6:20], want[0][2][4:8, 6:20])
    f2 = twin.apply(("cdl", "lut3d"), 0.6, m, 8, False, k, 10, 10, 1, 1, 1, 0, fs[2], **res)
    assert all(np.array_equal(f2[i], still[i][2]) for i in range(3))
    # an odd frame: the twin takes any size
    odd = frames.natural_yuv(7, 3, 10, 1, 1, k=5)
    got = twin.apply(("cdl", "lut3d"), 0.8, m[:3, :7], 8, True, k, 10, 10, 1, 1, 1, 0, odd, **res)
    assert got[0].shape == (3, 7) and got[1].shape == (3, 4)


# ------------------------------------------------------------------ check_matte
def test_check_matte_takes_and_refuses():
    cpu = torch.device("cpu")
    m8 = torch.zeros((8, 16), dtype=torch.uint8)
    m16 = torch.zeros((4, 8, 16), dtype=torch.int16)
    kw = dict(w=16, h=8, nframes=4, device=cpu)
    assert check_matte(m8, **kw) == (m8, 8, 0, True)
    assert check_matte(m8[None], 8, True, **kw)[1:] == (8, 1, True)
    assert check_matte(m16, 10, **kw)[1:] == (10, 0, False) and check_matte(m16, np.int64(16), np.bool_(True), **kw)[1:] == (16, 1, False)
    assert check_matte(m16.view(torch.uint16), 12, **kw)[1:] == (12, 0, False)
    assert check_matte(m16[:1], 12, w=16, h=8, nframes=1, device=None)[3] is True
    wide = torch.zeros((8, 40), dtype=torch.uint8)
    assert check_matte(wide[:, 3:19], **kw)[3] is True          # a padded stride, any base
    for args, message in (((np.zeros((8, 16), np.uint8),), "matte is a torch tensor .* not ndarray"),
                          ((None,), "matte is a torch tensor"),
                          ((m8.float(),), "matte has dtype float32"), ((m8.to(torch.int32),), "matte has dtype int32"),
                          ((m16,), "matte_depth is required for a int16 matte"), ((m16, 8), "matte_depth 8 is held in bytes"),
                          ((m16, 17), "matte_depth 17 is outside 8..16"), ((m8, 7), "matte_depth 7 is outside"),
                          ((m8, 10), "matte_depth 10 is held in 16-bit words"), ((m16, 10.0), "matte_depth is an integer"),
                          ((m16, True), "matte_depth is an integer"), ((m8, None, 1), "matte_invert is True or False"),
                          ((m8, None, "yes"), "matte_invert is True or False"),
                          ((m8[0],), r"matte has shape \(16,\)"), ((m16[None], 10), "matte has shape"),
                          ((m8[:, :15],), "matte is 15x8, the frame is 16x8"), ((m8[:7],), "matte is 16x7, the frame is 16x8"),
                          ((m16[:3], 10), "matte has 3 frames for 4 frames"),
                          ((torch.zeros((8, 32), dtype=torch.uint8)[:, ::2],), "matte must be dense along the row")):
        with pytest.raises(ValueError, match=message):
            check_matte(*args, **kw)
    with pytest.raises(ValueError, match="matte is on cpu, the engine is on cuda:0"):
        check_matte(m8, w=16, h=8, nframes=4, device=torch.device("cuda", 0))
    assert MATTE_PIX_FMTS == {"gray": 8, "gray10le": 10, "gray12le": 12, "gray14le": 14, "gray16le": 16}


# ------------------------------------------------------------------ refusals, layer by layer
@pytest.mark.parametrize("kw,word", REFUSED, ids=[w for _, w in REFUSED])
def test_check_stack_options_names_the_option_and_the_matte(kw, word):
    for strength in (None, 0.5):
        with pytest.raises(ValueError) as e:
            check_stack_options(**{**NAMES, "stages": "lut3d", "strength": strength, "matte": True, **kw})
        assert word in str(e.value) and "matte" in str(e.value) and ("strength" in str(e.value)) == (strength is not None)
    # without a matte, today's messages: no word of it
    with pytest.raises(ValueError) as e:
        check_stack_options(**{**NAMES, "stages": "lut3d", "strength": 0.5, "matte": False, **kw})
    assert "matte" not in str(e.value)


def test_the_engine_the_group_and_apply_lut_refuse_before_they_are_touched():
    import threading
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.multigpu import LutEngineGroup
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False)
    m = torch.zeros((8, 16), dtype=torch.uint8)
    for kw, message in ((dict(dither="blue_noise"), "dither .* with a matte"), (dict(out_size=(8, 4)), "out_size .* with a matte"),
                        (dict(strength=0.5, chroma_loc="left"), "chroma_loc.* with strength and a matte"),
                        (dict(strength=1.2), r"strength 1\.2 is outside")):
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_yuv_stack(held, _planes(), **{**NAMES, "stages": "lut3d", "matte": m, **kw})
    g = SimpleNamespace(_lock=threading.RLock(), n1d=17, engines=[SimpleNamespace(n=33, n2=0, _has_prelut=False)])
    src = [torch.from_numpy(p.view(np.int16)) for p in _planes(4)]
    for kw, message in ((dict(dither="blue_noise"), "dither .* with a matte"), (dict(matte=m[:, :15]), "matte is 15x8"),
                        (dict(matte=torch.zeros((3, 8, 16), dtype=torch.uint8)), "matte has 3 frames for 4 frames"),
                        (dict(matte_depth=10), "matte_depth 10 is held in 16-bit words")):
        with pytest.raises(ValueError, match=message):
            LutEngineGroup.apply_yuv_stack(g, src, **{**NAMES, "stages": "lut3d", "matte": m, **kw})
    base = dict(NAMES, cube=_lut(), engine=SimpleNamespace(n=0, n2=0, n1d=0, _has_prelut=False))
    for kw, message in ((dict(engine_dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a stage stack with a matte"),
                        (dict(resolution="8x4"), r"\(out_size / resolution\) is not supported with a stage stack with a matte"),
                        (dict(precision="fma32"), "precision='fma32' is not supported with a matte"),
                        (dict(precision="fast", strength=0.5), "precision='fast' is not supported with strength and a matte"),
                        (dict(out_pix_fmt="p010le"), r"stack \(matte\) pass .* semi-planar"),
                        (dict(pix_fmt="gbrp10le", strength=0.5), r"stack \(strength, matte\) pass .* RGB")):
        with pytest.raises(ValueError, match=message):
            apply_lut(_planes(), **{**base, "matte": m, **kw})
    for kw in (dict(matte_depth=10), dict(matte_invert=True)):
        with pytest.raises(ValueError, match="they need matte"):
            apply_lut(_planes(), **{**base, **kw})


def test_apply_lut_routes_a_matte_to_the_stack():
    from lut_renderer_amd.api import apply_lut
    eng, y, A = _Eng(), _planes(), _lut(2)
    m = torch.zeros((8, 16), dtype=torch.int16)
    apply_lut(y, **NAMES, engine=eng, cube=A)
    assert eng.calls[-1][0] == "yuv" and "matte" not in eng.calls[-1][1]           # no matte: the dedicated route, as it was
    apply_lut(y, **NAMES, engine=eng, cube=A, cdl=Cdl(saturation=0.5), matte=m, matte_depth=10, matte_invert=True)
    name, call = eng.calls[-1]
    assert name == "stack" and call["stages"] == (("cdl", None), ("lut3d", "tetrahedral")) and "strength" not in call
    assert call["matte"] is m and call["matte_depth"] == 10 and call["matte_invert"] is True
    apply_lut(y, **NAMES, engine=eng, cube=A, matte=m, matte_depth=10, strength=0.5, stages="lut3d:trilinear")
    assert eng.calls[-1][1]["strength"] == 0.5 and eng.calls[-1][1]["stages"] == (("lut3d", "trilinear"),)
    apply_lut(y, **NAMES, engine=eng, cube=A, strength=0.5)
    assert "matte" not in eng.calls[-1][1]


# ------------------------------------------------------------------ the CLI and the argv
def _args(*extra, pix_fmt="yuv420p10le", out="yuv422p10le"):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt, "--out-pix-fmt", out, *extra])


def test_cli_flags(cube_dir):
    from lut_renderer_amd.cli import plan_from_args
    a = str(cube_dir / "log709_33.cube")
    _, plain, _, _ = plan_from_args(_args("--cube", a))
    assert "stages" not in plain and "matte" not in plain
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--strength", "0.6"))
    assert "matte" not in kw and "matte_invert" not in kw
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--matte", "m.raw"))
    assert kw["stages"] == (("lut3d", "tetrahedral"),) and "strength" not in kw
    assert (kw["matte"], kw["matte_pix_fmt"], kw["matte_invert"]) == ("m.raw", "gray", False)
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--cdl-sat", "0.5", "--matte", "m.raw", "--matte-pix-fmt", "gray12le", "--matte-invert",
                                       "--strength-keys", "0:0,24:1"))
    assert kw["stages"] == (("cdl", None), ("lut3d", "tetrahedral")) and callable(kw["strength_keys"])
    assert (kw["matte"], kw["matte_pix_fmt"], kw["matte_invert"]) == ("m.raw", "gray12le", True)
    for extra, message in ((("--matte", "-"), "--matte is a file or FIFO, not '-'"), (("--matte-invert",), "they need --matte"),
                           (("--matte-pix-fmt", "gray"), "they need --matte"),
                           (("--matte", "m", "--matte-pix-fmt", "gray9le"), "unknown --matte-pix-fmt 'gray9le'"),
                           (("--matte", "m", "--engine-dither", "blue_noise"), "dither .* with a matte"),
                           (("--matte", "m", "--out-size", "8x4"), "out_size .* with a matte"),
                           (("--matte", "m", "--strength", "0.5", "--chroma-loc", "left"), "chroma_loc.* with strength and a matte"),
                           (("--matte", "m", "--precision", "fast"), "precision='fast' is not supported with a matte"),
                           (("--matte", "m", "--second-output", "x", "--second-pix-fmt", "yuv420p"), "out2_pix_fmt.* with a matte")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args("--cube", a, *extra))
    with pytest.raises(ValueError, match=r"stack \(matte\) pass .* semi-planar"):
        plan_from_args(_args("--cube", a, "--matte", "m", pix_fmt="nv12", out="nv12"))


def test_engine_command_renders_the_flags_and_round_trips(cube_dir):
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.pipe import engine_stage_commands
    a = cube_dir / "log709_33.cube"
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    params = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")
    io = (Path("-"), Path("-"), params, a, info)
    plain = engine_command(*io)
    assert engine_command(*io, matte=None, matte_pix_fmt=None, matte_invert=False) == plain and "--matte" not in plain
    assert engine_command(*io, matte=Path("m.raw")) == plain + ["--matte", "m.raw"]
    assert engine_command(*io, strength=0.6, matte="m.raw", matte_pix_fmt="gray10le", matte_invert=True) == \
        plain + ["--strength", "0.6", "--matte", "m.raw", "--matte-pix-fmt", "gray10le", "--matte-invert"]
    cmd = engine_command(*io, cdl=Cdl(saturation=0.5), stages="cdl,lut3d:trilinear", matte="m.raw", matte_pix_fmt="gray16le", matte_invert=True)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert kw["stages"] == (("cdl", None), ("lut3d", "trilinear")) and kw["cdl"] == Cdl(saturation=0.5)
    assert (kw["matte"], kw["matte_pix_fmt"], kw["matte_invert"]) == ("m.raw", "gray16le", True)
    _, kw, _, _ = plan_from_args(build_parser().parse_args(engine_command(*io, matte="m.raw")[3:]))
    assert (kw["matte"], kw["matte_pix_fmt"], kw["matte_invert"]) == ("m.raw", "gray", False)
    stage = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, matte=Path("m.raw"), matte_pix_fmt="gray10le")
    assert stage.engine[stage.engine.index("--matte") + 1] == "m.raw" and "--matte" not in stage.encoder
    assert "--matte-invert" not in stage.engine and "--matte" not in engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info).engine
    for kw, message in ((dict(matte="-"), "matte is a file or FIFO, not '-'"), (dict(matte_invert=True), "they need matte"),
                        (dict(matte_pix_fmt="gray"), "they need matte"), (dict(matte="m", matte_pix_fmt="gray9"), "unknown matte_pix_fmt"),
                        (dict(matte="m", engine_dither="blue_noise"), "dither .* with a matte"),
                        (dict(matte="m", precision="fast"), "precision='fast' is not supported with a matte"),
                        (dict(matte="m", strength=0.5, chroma_loc="left"), "chroma_loc.* with strength and a matte")):
        with pytest.raises(ValueError, match=message):
            engine_command(*io, **kw)


# ------------------------------------------------------------------ the stream's matte reader
def test_the_matte_reader_still_per_frame_and_short(tmp_path):
    from lut_renderer_amd.stream import HostPipeline, MatteReader
    w, h = 6, 4
    m = np.random.default_rng(1).integers(0, 1024, (5, h, w)).astype("<u2")
    (tmp_path / "five.raw").write_bytes(m.tobytes())
    (tmp_path / "one.raw").write_bytes(m[3].tobytes())
    (tmp_path / "bytes.raw").write_bytes(m.astype(np.uint8).tobytes())
    still = MatteReader(tmp_path / "one.raw", "gray10le", w, h)
    assert still.depth == 10 and still.still.shape == (h, w) and np.array_equal(still.still, m[3]) and still._f is None
    per = MatteReader(tmp_path / "five.raw", "gray10le", w, h)
    assert per.still is None and per.frame_bytes == 2 * w * h
    got = [per.read(n) for n in (2, 2, 1)]                     # five frames in batches of two
    assert [g.shape for g in got] == [(2, h, w), (2, h, w), (1, h, w)] and np.array_equal(np.concatenate(got), m) and per.frames_read == 5
    with pytest.raises(ValueError, match=r"five\.raw' ended at frame 5: the input goes on"):
        per.read(1)
    per.close()
    short = MatteReader(tmp_path / "five.raw", "gray10le", w, h)
    short.read(2)
    with pytest.raises(ValueError, match="ended at frame 5"):   # the batch of frames 2..5 finds three
        short.read(4)
    short.close()
    eight = MatteReader(tmp_path / "bytes.raw", "gray", w, h)
    assert eight.depth == 8 and eight.still is None and np.array_equal(eight.read(5), m.astype(np.uint8))
    eight.close()
    # five 8-bit frames of 6 x 4 are one 16-bit frame of 10 x 6: exactly one frame is a still
    assert MatteReader(tmp_path / "bytes.raw", "gray16le", 10, 6).still.shape == (6, 10)
    for path, fmt, message in (("-", "gray", "not '-'"), (tmp_path / "one.raw", "gray9le", "unknown matte pixel format 'gray9le'")):
        with pytest.raises(ValueError, match=message):
            MatteReader(path, fmt, w, h)
    with pytest.raises(FileNotFoundError):
        MatteReader(tmp_path / "none.raw", "gray", w, h)
    # the pipeline's bookkeeping without a device: the matte travels into the call, beside the key frames' strengths
    seen = []
    eng = SimpleNamespace(apply_yuv_stack=lambda src, dst, **kw: seen.append(kw))
    pipe = SimpleNamespace(stack=True, kw={"stages": "lut3d", "matte_depth": 10}, strength_keys=None, frames_submitted=0, eng=eng)
    HostPipeline._run_stack(pipe, None, None, 2, "the batch's matte")
    HostPipeline._run_stack(pipe, None, None, 2)
    assert seen[0]["matte"] == "the batch's matte" and seen[0]["matte_depth"] == 10 and "matte" not in seen[1]
    assert pipe.frames_submitted == 4 and "matte" not in pipe.kw
    t = HostPipeline._matte_tensor(m[0])
    assert t.dtype == torch.int16 and np.array_equal(t.numpy().view(np.uint16), m[0])
    assert HostPipeline._matte_tensor(m[0].astype(np.uint8)).dtype == torch.uint8
    no_stack = dict(stages=None, matte=still)
    with pytest.raises(ValueError, match="a matte runs in the stage stack"):
        HostPipeline(SimpleNamespace(n=33), "yuv420p10le", w, h, **no_stack)
    with pytest.raises(ValueError, match="the matte is 6x4, the frames are 8x4"):
        HostPipeline(SimpleNamespace(n=33), "yuv420p10le", 8, h, stages="lut3d", matte=still)
