"""Blue-noise dither in the output stage -- host side: the committed mask, the definition of the quantisation on
the reference of tests/_bn_twin.py, the plumbing of the engine setting and the argument checks.  GPU parity is
tests/test_gpu_bn_dither.py."""
import ctypes as C
import threading
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _bn_twin as twin

F = np.float32
LEVELS = (1 / 16, 1 / 8, 1 / 4, 1 / 2, 3 / 4, 7 / 8, 15 / 16)


# ------------------------------------------------------------------ the mask
def test_mask_is_a_permutation_and_every_offset_is_exact_in_float32():
    rank = _native.dither_mask()
    assert rank.shape == (64, 64) and rank.dtype == np.uint16
    assert np.array_equal(np.sort(rank.ravel()), np.arange(4096))
    exact = (2 * rank.astype(np.int64) - 4095) / 8192.0                      # float64: exact
    d = twin.offsets()
    assert d.dtype == F and np.array_equal(d.astype(np.float64), exact)
    assert d.min() == F(-4095 / 8192) and d.max() == F(4095 / 8192) and np.all(np.abs(d) < 0.5)


def test_mask_header_is_what_the_library_returns():
    """The committed header is the contract: the numbers in it are the ones lutr_dither_mask hands out."""
    text = (Path(__file__).resolve().parent.parent / "lut_renderer_amd" / "csrc" / "lutr_bn_mask.h").read_text()
    body = text[text.index("{") + 1:text.index("}")]
    vals = np.array([int(v) for v in body.replace("\n", " ").split(",") if v.strip()], dtype=np.uint16)
    assert np.array_equal(vals.reshape(64, 64), _native.dither_mask())


def test_spectrum_is_blue_at_every_level():
    """Binary pattern rank < 4096 g: the mean power over the non-zero frequencies of radius <= 8 (and <= 4) is at most 0.15 of the
    mean over all non-zero frequencies.  White noise gives about 1."""
    rank = _native.dither_mask().astype(np.int64)
    f = np.fft.fftfreq(64) * 64
    radius = np.hypot(*np.meshgrid(f, f, indexing="ij"))
    nz = radius > 0
    for g in LEVELS:
        p = (rank < 4096 * g).astype(np.float64)
        power = np.abs(np.fft.fft2(p - p.mean())) ** 2
        for r in (8, 4):
            ratio = power[nz & (radius <= r)].mean() / power[nz].mean()
            print(f"level {g:.4f} radius <= {r}: {ratio:.4f}")
            assert ratio <= 0.15, (g, r, ratio)


# ------------------------------------------------------------------ the quantisation, on the twin
def test_flat_field_lights_exactly_k_samples_of_a_tile():
    """c = 100.5 + k / 4096: over one 64 x 64 tile of each plane's offsets exactly k samples reach 101 (d >= 0.5 - k / 4096
    holds for the k largest ranks; every sum is exact in float32)."""
    for plane in range(3):
        for k in (0, 1, 100, 2048, 4095):
            c = np.full((64, 64), F(100.5) + F(k / 4096), dtype=F)
            q = twin.quantise_plane(c, plane, 255.0, False)
            assert set(np.unique(q)) <= {100, 101}
            assert int((q == 101).sum()) == k, (plane, k)


def test_plane_offsets_are_the_shifted_mask():
    d = twin.offsets()
    for plane in range(3):
        t = twin.plane_offsets(plane, 70, 130)
        for y, x in ((0, 0), (5, 9), (63, 63), (64, 64), (69, 129), (27, 40)):
            assert t[y, x] == d[(y + twin.OY[plane]) & 63, (x + twin.OX[plane]) & 63]
    assert all(o % 8 == 0 for o in twin.OX)                  # an aligned run of 8 samples never wraps


def test_zero_offsets_are_the_undithered_contract(cube_dir):
    """With d = 0 the quantisation is stage 3 of the existing twin, bit for bit."""
    from lut_renderer_amd import cube, frames
    from tests import _xsub_twin as xs
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    zero = np.zeros((64, 64), F)
    for (icsx, icsy), (ocsx, ocsy), dout in (((1, 1), (1, 1), 8), ((1, 1), (1, 0), 10), ((0, 0), (1, 1), 8)):
        src = frames.natural_yuv(37, 23, 10, icsx, icsy, k=3)
        k = xs.consts("bt709", "tv", "bt709", "tv", 10, 10, dout, ocsx, ocsy)
        rgb = xs.lut_rgb(lut.table, lut.scale, "tetrahedral", k, 10, icsx, icsy, src)
        got = [twin.quantise_plane(c, p, float(k.max_o), dout > 8, zero) for p, c in enumerate(twin.unrounded(k, ocsx, ocsy, rgb))]
        want = xs.apply(lut.table, lut.scale, "tetrahedral", k, 10, dout, icsx, icsy, ocsx, ocsy, src)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_debanding_of_a_slow_ramp():
    """A ramp rising 6 codes over 256 columns: the 8 x 8 block means of the dithered output follow the unquantised ramp at least
    four times closer than those of the plain rounding."""
    c = np.tile((F(100.5) + np.arange(256, dtype=F) * F(6 / 256)).astype(F), (64, 1))

    def block_err(q):
        means = lambda a: a.astype(np.float64).reshape(8, 8, 32, 8).mean(axis=(1, 3))
        return np.abs(means(q) - means(c - F(0.5))).mean()

    plain = block_err(twin.quantise_plane(c, 0, 255.0, False, np.zeros((64, 64), F)))
    for plane in range(3):
        bn = block_err(twin.quantise_plane(c, plane, 255.0, False))
        print(f"plane {plane}: blue noise {bn:.4f} plain {plain:.4f} ratio {bn / plain:.4f}")
        assert bn <= plain / 4, (plane, bn, plain)


# ------------------------------------------------------------------ plumbing
class _FakeEngine:
    """Records the keywords of the engine call `apply_lut` / a group makes."""

    def __init__(self, device="cpu"):
        import torch
        self._lock, self._applied_lut, self.precision, self.calls = threading.RLock(), None, "strict", []
        self.device = torch.device(device)

    def apply_yuv(self, src, dst=None, **kw):
        self.calls.append(("yuv", kw))
        return dst

    def apply_rgb_to_yuv(self, src, dst=None, **kw):
        self.calls.append(("rgb", kw))
        return dst


def _cpu_planes(w, h, csx, csy, dtype=None):
    import torch
    dtype = dtype or torch.int16
    return [torch.zeros((h, w), dtype=dtype)] + [torch.zeros(((h + (1 << csy) - 1) >> csy, (w + (1 << csx) - 1) >> csx), dtype=dtype)] * 2


def test_apply_lut_engine_dither():
    from lut_renderer_amd.api import apply_lut
    planes = _cpu_planes(16, 8, 1, 1)
    kw = dict(cube=None, pix_fmt="yuv420p10le", out_pix_fmt="yuv420p", colorspace="bt709", color_range="tv")
    eng = _FakeEngine()
    apply_lut(planes, engine=eng, engine_dither="blue_noise", **kw)
    apply_lut(planes, engine=eng, zscale_dither="error_diffusion", **kw)
    apply_lut(planes, engine=eng, **kw)
    apply_lut(planes, engine=eng, zscale_dither="ordered", **kw)           # the reference: anything else is no dither filter
    assert [c[1]["dither"] for c in eng.calls] == ["blue_noise", "error_diffusion", "none", "none"]
    with pytest.raises(ValueError, match="two dithers"):
        apply_lut(planes, engine=eng, engine_dither="blue_noise", zscale_dither="error_diffusion", **kw)
    for bad in ("ordered", "error_diffusion", "none", ""):
        with pytest.raises(ValueError, match="engine_dither"):
            apply_lut(planes, engine=eng, engine_dither=bad, **kw)
    assert len(eng.calls) == 4
    import torch
    rgb = torch.zeros((8, 16, 3), dtype=torch.uint8)
    apply_lut(rgb, engine=eng, cube=None, pix_fmt="rgb24", out_pix_fmt="yuv420p", engine_dither="blue_noise")
    assert eng.calls[-1][0] == "rgb" and eng.calls[-1][1]["dither"] == "blue_noise"


def _cli_args(cube_dir, *extra, pix_fmt="yuv420p10le", out="yuv420p"):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt, "--out-pix-fmt", out, "--cube",
                                      str(cube_dir / "log709_33.cube"), *extra])


def test_cli_flag_and_the_rendered_commands(cube_dir):
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.pipe import engine_stage_commands
    assert plan_from_args(_cli_args(cube_dir, "--engine-dither", "blue_noise"))[1]["dither"] == "blue_noise"
    assert plan_from_args(_cli_args(cube_dir, "--zscale-dither", "error_diffusion"))[1]["dither"] == "error_diffusion"
    assert plan_from_args(_cli_args(cube_dir))[1].get("dither", "none") == "none"
    with pytest.raises(ValueError, match="two dithers"):
        plan_from_args(_cli_args(cube_dir, "--engine-dither", "blue_noise", "--zscale-dither", "error_diffusion"))
    with pytest.raises(SystemExit):
        build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", "yuv420p", "--cube", "c", "--engine-dither",
                                   "ordered"])
    # the refusals that stay, with the messages they have
    with pytest.raises(ValueError, match="semi-planar"):
        plan_from_args(_cli_args(cube_dir, "--engine-dither", "blue_noise", pix_fmt="nv12", out="nv12"))
    with pytest.raises(ValueError, match="chroma_loc"):
        plan_from_args(_cli_args(cube_dir, "--engine-dither", "blue_noise", "--chroma-loc", "left"))
    with pytest.raises(ValueError, match="second output"):
        plan_from_args(_cli_args(cube_dir, "--engine-dither", "blue_noise", "--second-output", "x.yuv", "--second-pix-fmt",
                                 "yuv422p10le"))
    with pytest.raises(ValueError, match="float output"):
        plan_from_args(build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", "gbrpf32le", "--cube",
                                                  str(cube_dir / "log709_33.cube"), "--engine-dither", "blue_noise"]))
    params = ProcessingParams(video_codec="libx264")
    info = VideoInfo(width=64, height=32, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    plain = engine_command(Path("-"), Path("-"), params, Path("look.cube"), info, python_bin="python3")
    assert "--engine-dither" not in plain
    cmd = engine_command(Path("-"), Path("-"), params, Path("look.cube"), info, python_bin="python3", engine_dither="blue_noise")
    assert cmd[cmd.index("--engine-dither") + 1] == "blue_noise" and [a for a in cmd if a not in ("--engine-dither", "blue_noise")] == plain
    assert plan_from_args(build_parser().parse_args(cmd[3:]))[1]["dither"] == "blue_noise"
    stage = engine_stage_commands(Path("in.mp4"), Path("out.mp4"), params, Path("look.cube"), info, python_bin="python3",
                                  engine_dither="blue_noise")
    assert stage.engine[stage.engine.index("--engine-dither") + 1] == "blue_noise"
    with pytest.raises(ValueError, match="two dithers"):
        engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx264", zscale_dither="error_diffusion"),
                       Path("look.cube"), info, engine_dither="blue_noise")
    with pytest.raises(ValueError, match="engine_dither"):
        engine_command(Path("-"), Path("-"), params, Path("look.cube"), info, engine_dither="ordered")


def _fake_group(n):
    from lut_renderer_amd.multigpu import LutEngineGroup
    g = object.__new__(LutEngineGroup)
    g._lock, g.treat_as_remote = threading.RLock(), False
    g.engines = [_FakeEngine() for _ in range(n)]
    return g


def test_group_row_shards_blue_noise_and_keeps_refusing_error_diffusion():
    import torch
    g = _fake_group(2)
    src = _cpu_planes(16, 12, 1, 1)
    g.apply_yuv(src, pix_fmt="yuv420p10le", out_pix_fmt="yuv420p", dither="blue_noise")
    calls = [e.calls[0][1] for e in g.engines]
    assert [(c["row0"], c["rows"], c["dither"]) for c in calls] == [(0, 6, "blue_noise"), (6, 6, "blue_noise")]
    g.apply_rgb_to_yuv(torch.zeros((12, 16, 3), dtype=torch.uint8), pix_fmt="rgb24", out_pix_fmt="yuv420p", dither="blue_noise")
    assert [(e.calls[1][1]["row0"], e.calls[1][1]["dither"]) for e in g.engines] == [(0, "blue_noise"), (6, "blue_noise")]
    for call in (lambda: g.apply_yuv(src, pix_fmt="yuv420p10le", dither="error_diffusion"),
                 lambda: g.apply_rgb_to_yuv(torch.zeros((12, 16, 3), dtype=torch.uint8), pix_fmt="rgb24", out_pix_fmt="yuv420p",
                                            dither="error_diffusion")):
        with pytest.raises(ValueError, match="cannot be row-sharded"):
            call()
    with pytest.raises(ValueError, match="semi-planar"):
        g.apply_yuv(src[:2], pix_fmt="nv12", dither="blue_noise")


def test_group_anchor_of_a_slice_that_travels():
    from lut_renderer_amd.multigpu import _bn_anchor
    assert [_bn_anchor(r, 0) for r in (0, 63, 64, 130)] == [0, 0, 64, 128]
    assert [_bn_anchor(r, 1) for r in (0, 66, 128, 200, 256)] == [0, 0, 128, 128, 256]
    d = twin.offsets()
    for ocsy in (0, 1):
        for r0 in (66, 130, 258):
            a = _bn_anchor(r0, ocsy)
            assert a <= r0 and a % 64 == 0 and (a >> ocsy) % 64 == 0
            # the slice's own rows see the frame's pattern
            assert np.array_equal(twin.plane_offsets(1, r0 + 8 - a, 8)[r0 - a:], twin.plane_offsets(1, r0 + 8, 8, d)[r0:])


def test_host_pipeline_carries_the_keyword(monkeypatch):
    import torch
    from lut_renderer_amd import stream
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self: self)
    monkeypatch.setattr(torch.cuda, "Stream", lambda dev=None: None)
    monkeypatch.setattr(torch.cuda, "Event", lambda: None)
    pipe = stream.HostPipeline(_FakeEngine(), "yuv420p10le", 16, 8, batch=1, out_pix_fmt="yuv420p", dither="blue_noise")
    assert pipe.kw["dither"] == "blue_noise" and pipe.kw["out_pix_fmt"] == "yuv420p"
    with pytest.raises(ValueError, match="second output"):
        stream.HostPipeline(_FakeEngine(), "yuv420p10le", 16, 8, batch=1, out_pix_fmt="yuv420p", second_pix_fmt="yuv422p10le",
                            dither="blue_noise")


def test_refusals_that_stay():
    from lut_renderer_amd.engine import LutEngine, check_chroma_loc, check_container_options, check_dual_options
    with pytest.raises(ValueError, match="not defined with sited chroma resampling"):
        check_chroma_loc("left", "blue_noise", "yuv420p10le", "yuv420p")
    for fmt, word in (("nv12", "semi-planar"), ("yuyv422", "packed"), ("v210", "v210")):
        with pytest.raises(ValueError, match=f"dither is not supported with a {word}"):
            check_container_options(fmt, None, "blue_noise")
    with pytest.raises(ValueError, match="dither is not supported with a second output"):
        check_dual_options("yuv420p10le", "yuv422p10le", "yuv420p", "blue_noise")
    for call in (LutEngine.apply_yuv, LutEngine.apply_rgb_to_yuv):
        with pytest.raises(ValueError, match="unknown dither mode 'ordered'"):
            call(None, [], pix_fmt="yuv420p", out_pix_fmt="yuv420p", dither="ordered")
    assert _native.DITHER == {"none": 0, "error_diffusion": 1, "blue_noise": 2}


# ------------------------------------------------------------------ the C ABI without a GPU
def test_abi_argument_checks_without_a_gpu():
    import subprocess
    lib = _native.load()
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    assert " T lutr_dither_mask\n" in nm and "lutr_dither_mask" in _native.SYMBOLS
    assert lib.lutr_dither_mask(None) == _native.EINVAL
    out = (C.c_uint16 * 4096)()
    assert lib.lutr_dither_mask(out) == 0 and sorted(out) == list(range(4096))
    bn = _native.DITHER["blue_noise"]
    assert lib.lutr_apply_yuv_xsub(None, None, 2, bn, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
    assert b"dither" not in lib.lutr_last_error()                       # the mode is known: the null context is what fails
    assert lib.lutr_apply_yuv_dither(None, None, 2, bn, 16, 16, 1, None, None) == _native.EINVAL
    assert lib.lutr_apply_rgb_to_yuv(None, None, 2, bn, 0, 16, 16, 1, None, None, None, 0, 16) == _native.EINVAL
    assert lib.lutr_apply_rgbf_to_yuv(None, None, 2, bn, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
    assert b"dither" not in lib.lutr_last_error()
    assert lib.lutr_apply_yuv_xsub(None, None, 2, 3, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
    assert b"unknown dither mode 3" in lib.lutr_last_error()
