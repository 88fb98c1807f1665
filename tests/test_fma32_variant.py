"""The FMA32 precision (include/lutr.h LUTR_PRECISION_FMA32, csrc/lutr_tile2.hip V_FMA32).

Strict's fp32 lattice, coordinates, weights, taps, truncation and YUV stages; only the blend changes: nodes pre-multiplied by
M = 2^depth - 1 in fp32 and one rounding per step (an fma chain).  Pinned here:
  (1) CPU: the NumPy twin (tests/_fma32_twin.py) really fuses, stays within one code of the strict oracle over modes x
      formats x LUTs x content, and equals it exactly for nearest; the names reach every layer;
  (2) GPU: the fma32 tile kernels equal the twin bit for bit, everything fma32 does not cover runs strict bit-exact, and a
      lattice change never leaves a stale pre-multiplied copy behind.
"""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import cube, frames
from tests import _fma32_twin as twin

ROOT = Path(__file__).resolve().parent.parent
MODES = ("tetrahedral", "trilinear", "nearest")
# (name, pix_fmt in, pix_fmt out, din, dout, csx, csy)
FORMATS = (("yuv420p10le", "yuv420p10le", "yuv420p10le", 10, 10, 1, 1), ("yuv420p", "yuv420p", "yuv420p", 8, 8, 1, 1),
           ("yuv422p10le", "yuv422p10le", "yuv422p10le", 10, 10, 1, 0), ("yuv444p", "yuv444p", "yuv444p", 8, 8, 0, 0),
           ("10to8", "yuv420p10le", "yuv420p", 10, 8, 1, 1))


def _luts():
    rng = np.random.default_rng(3)
    yield "log709_33", cube.log709_lattice(33)
    yield "identity_17", cube.identity_lattice(17)
    yield "random_9", rng.uniform(0.0, 1.0, size=(9, 9, 9, 3)).astype(np.float32)
    yield "log709_65", cube.log709_lattice(65)


def _max_diff(a, b):
    return max(int(np.abs(x.astype(np.int32) - y.astype(np.int32)).max()) for x, y in zip(a, b))


# ------------------------------------------------------------------ CPU
def test_twin_fma_is_fused():
    f = np.float32
    a = b = f(1.0 + 2.0 ** -12)
    c = f(-(1.0 + 2.0 ** -11))
    unfused = (a * b).astype(f) + c                  # a * b rounds to 1 + 2^-11 (a tie, to even): the sum is 0
    assert unfused == 0.0
    assert twin.fma(a, b, c) == f(2.0 ** -24)        # one rounding keeps the 2^-24 of the exact product


@pytest.mark.parametrize("name,fin,fout,din,dout,csx,csy", FORMATS)
def test_twin_is_within_one_code_of_the_strict_oracle(orc, name, fin, fout, din, dout, csx, csy):
    one = np.ones(3, np.float32)
    k = orc.yuv_constants("bt709", "tv", "bt709", "tv", din, din, dout, 1 << (csx + csy))
    worst, differ, total = 0, 0, 0
    for lname, lat in _luts():
        for dist in ("natural", "uniform", "noise16"):
            src = frames.make_yuv(dist, 128, 64, din, csx, csy, k=5)
            for mode in MODES:
                strict = orc.apply_yuv(lat, one, mode, k, din, din, dout, csx, csy, src)
                got = twin.apply_yuv(lat, one, mode, k, din, din, dout, csx, csy, src)
                if mode == "nearest":        # one node times M, rounded once either way
                    for g, s in zip(got, strict):
                        assert np.array_equal(g, s), (lname, dist)
                    continue
                for g, s in zip(got, strict):
                    d = np.abs(g.astype(np.int32) - s.astype(np.int32))
                    worst = max(worst, int(d.max()))
                    differ += int((d > 0).sum())
                    total += d.size
                assert worst <= 1, (lname, dist, mode, worst)
    print(f"fma32 vs strict, {name}: {differ} of {total} samples differ ({differ / total:.4%}), max |d| = {worst}")
    assert worst <= 1


def test_twin_with_the_config5_prologue_is_within_one_code_of_strict(orc):
    """The pc -> tv prologue with an 8-bit LUT: the bound is one code of the LUT's depth (lut3d's output), which the 10-bit
    RGB -> YUV stage then scales by about 1023 / 255."""
    from oracle import lut3d_numpy
    lat = cube.log709_lattice(33)
    one = np.ones(3, np.float32)
    k5 = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 8, 10, 4, prologue=True)
    src = frames.make_yuv("natural", 128, 64, 10, 1, 1, k=4, full_range=True)
    rgb = lut3d_numpy.yuv_to_rgb_codes(k5, 1, 1, src)
    for mode in ("tetrahedral", "trilinear"):
        strict = lut3d_numpy.lut3d_codes(lat, one, 8, mode, *rgb)
        got = twin.lut3d_codes(lat, one, 8, mode, *rgb)
        assert _max_diff(got, strict) <= 1, mode
        assert np.array_equal(lut3d_numpy.rgb_codes_to_yuv(k5, 10, 1, 1, strict)[0],
                              orc.apply_yuv(lat, one, mode, k5, 10, 8, 10, 1, 1, src)[0])     # (the NumPy stages are the oracle's)


def test_fma32_name_reaches_every_layer():
    from lut_renderer_amd import _native, cli, command, pipe
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    assert _native.PRECISION["fma32"] == 2
    assert _native.PRECISION["strict"] == 0 and _native.PRECISION["fast"] == 1
    header = (ROOT / "include" / "lutr.h").read_text()
    assert "LUTR_PRECISION_FMA32 = 2" in header
    info = VideoInfo(width=64, height=32, pix_fmt="yuv420p10le", fps=25.0)
    cmd = command.engine_command(Path("a.yuv"), Path("b.yuv"), ProcessingParams(), Path("x.cube"), info, python_bin="py",
                                 precision="fma32")
    assert cmd[cmd.index("--precision") + 1] == "fma32"
    assert cli.build_parser().parse_args(cmd[3:]).precision == "fma32"
    with pytest.raises(ValueError, match="fma32"):
        command.engine_command(Path("a.yuv"), Path("b.yuv"), ProcessingParams(), Path("x.cube"), info, precision="fp16")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(cmd[3:cmd.index("--precision")] + ["--precision", "fp16"])
    # pipe.py: the option travels into the engine stage's argv
    seen = {}

    def fake_run(cmds):
        seen["engine"] = cmds.engine
        return 0

    orig = pipe.run_stage
    pipe.run_stage = fake_run
    try:
        rc = pipe.main(["-i", "in.mov", "-o", "out.mov", "--cube", "x.cube", "--precision", "fma32",
                        "--info", '{"width": 64, "height": 32, "pix_fmt": "yuv420p10le", "fps": 25.0}'])
    finally:
        pipe.run_stage = orig
    assert rc == 0 and seen["engine"][seen["engine"].index("--precision") + 1] == "fma32"
    sc = pipe.engine_stage_commands(Path("in.mov"), Path("out.mov"), ProcessingParams(), Path("x.cube"), info, precision="fma32")
    assert sc.engine[sc.engine.index("--precision") + 1] == "fma32"


# ------------------------------------------------------------------ GPU
def _dev(planes, device):
    import torch
    return [torch.from_numpy(p.view(np.int16) if p.dtype == np.uint16 else p).to(device) for p in planes]


def _host(tensors, dout):
    return [t.cpu().numpy().view(np.uint16) if dout > 8 else t.cpu().numpy() for t in tensors]


def _equal(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        if not np.array_equal(a, b):
            d = np.abs(a.astype(np.int64) - b.astype(np.int64))
            raise AssertionError(f"{what}: plane {i} differs at {int((d > 0).sum())} samples, max |d| = {int(d.max())}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,fin,fout,din,dout,csx,csy", FORMATS)
def test_fma32_kernels_match_the_twin_and_stay_within_one_code_of_strict(engine, orc, name, fin, fout, din, dout, csx, csy):
    one = np.ones(3, np.float32)
    k = orc.yuv_constants("bt709", "tv", "bt709", "tv", din, din, dout, 1 << (csx + csy))
    engine.set_variant("vec_lds")
    engine.set_precision("fma32")
    try:
        for lname, lat in _luts():
            engine.set_lut(cube.CubeLut(lat.shape[0], one, lat))
            for dist in ("natural", "uniform", "noise16", "noise64"):
                src = frames.make_yuv(dist, 256, 72, din, csx, csy, k=6)
                for mode in MODES:
                    got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt=fin, out_pix_fmt=fout, interp=mode), dout)
                    kern = engine.last_kernel
                    assert "k_yuv_tile2" in kern, kern
                    assert (",fma32" in kern) == (mode != "nearest"), kern
                    if lname == "identity_17" and mode == "tetrahedral":
                        assert "+whole-lattice" in kern, kern
                    want = twin.apply_yuv(lat, one, mode, k, din, din, dout, csx, csy, src)
                    _equal(got, want, f"{name} {lname} {dist} {mode} ({kern})")
                    strict = orc.apply_yuv(lat, one, mode, k, din, din, dout, csx, csy, src)
                    assert _max_diff(got, strict) <= 1, (name, lname, dist, mode)
    finally:
        engine.set_precision("strict")
        engine.set_variant("auto")


@pytest.mark.gpu
def test_fma32_tube_windows_gather_and_prologue(engine, orc):
    """33^3 natural frames run on the grey tube; 65^3 sigma-64 noise on windows and the gather body (the tile counters say
    which); the config-5 full-range prologue with an 8-bit LUT, 10- and 8-bit out."""
    one = np.ones(3, np.float32)
    engine.set_variant("vec_lds")
    engine.set_precision("fma32")
    try:
        lat = cube.log709_lattice(33)
        engine.set_lut(cube.CubeLut(33, one, lat))
        k = orc.yuv_constants(din=10)
        src = frames.make_yuv("natural", 1024, 256, 10, 1, 1, k=21)
        for mode in ("tetrahedral", "trilinear"):
            got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le", interp=mode), 10)
            assert ",fma32" in engine.last_kernel and "+tube" in engine.last_kernel, engine.last_kernel
            _equal(got, twin.apply_yuv(lat, one, mode, k, 10, 10, 10, 1, 1, src), f"tube {mode}")
        lat65 = cube.log709_lattice(65)
        engine.set_lut(cube.CubeLut(65, one, lat65))
        seen = {"staged": 0, "global_tiles": 0}
        for dist in ("vivid", "noise64"):
            src = frames.make_yuv(dist, 1024, 256, 10, 1, 1, k=22)
            for mode in ("tetrahedral", "trilinear"):
                engine.tile_stats(True)
                got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le", interp=mode), 10)
                st = engine.tile_stats(False)
                assert ",fma32" in engine.last_kernel, engine.last_kernel
                seen = {key: v + st[key] for key, v in seen.items()}
                _equal(got, twin.apply_yuv(lat65, one, mode, k, 10, 10, 10, 1, 1, src), f"windows / gather {dist} {mode}")
        assert seen["staged"] > 0 and seen["global_tiles"] > 0, seen
        engine.set_lut(cube.CubeLut(33, one, lat))
        s5 = frames.make_yuv("natural", 256, 72, 10, 1, 1, k=4, full_range=True)
        for out_fmt, dout in (("yuv420p10le", 10), ("yuv420p", 8)):
            k5 = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 8, dout, 4, prologue=True)
            for mode in ("tetrahedral", "trilinear"):
                got = _host(engine.apply_yuv(_dev(s5, engine.device), pix_fmt="yuv420p10le", out_pix_fmt=out_fmt, interp=mode,
                                             range_src="pc", range_in="tv", lut_depth=8), dout)
                assert ",pre," in engine.last_kernel and ",fma32" in engine.last_kernel, engine.last_kernel
                _equal(got, twin.apply_yuv(lat, one, mode, k5, 10, 8, dout, 1, 1, s5), f"config 5 {out_fmt} {mode}")
        # the prologue on a lattice small enough to be staged whole
        lat17 = cube.log709_lattice(17)
        engine.set_lut(cube.CubeLut(17, one, lat17))
        k5 = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 8, 10, 4, prologue=True)
        got = _host(engine.apply_yuv(_dev(s5, engine.device), pix_fmt="yuv420p10le", range_src="pc", range_in="tv", lut_depth=8), 10)
        assert ",fma32" in engine.last_kernel and "+whole-lattice" in engine.last_kernel, engine.last_kernel
        _equal(got, twin.apply_yuv(lat17, one, "tetrahedral", k5, 10, 8, 10, 1, 1, s5), "config 5 whole lattice")
    finally:
        engine.set_precision("strict")
        engine.set_variant("auto")


@pytest.mark.gpu
def test_fma32_whole_uhd_frame(engine, orc, cube_dir):
    import torch
    lut = cube.read_cube(cube_dir / "log709_33.cube")
    engine.set_lut(lut)
    engine.set_variant("vec_lds")
    src = frames.natural_yuv(3840, 2160, 10, 1, 1, k=3)
    dev = _dev(src, engine.device)
    try:
        strict = [t.clone() for t in engine.apply_yuv(dev, pix_fmt="yuv420p10le")]
        engine.set_precision("fma32")
        out = engine.apply_yuv(dev, pix_fmt="yuv420p10le")
        assert ",fma32" in engine.last_kernel, engine.last_kernel
        for a, b in zip(strict, out):
            assert (a.to(torch.int32) - b.to(torch.int32)).abs().max().item() <= 1
        got = _host(out, 10)
        k = orc.yuv_constants(din=10)
        for r0 in (0, 1024, 2096):
            strip = [src[0][r0:r0 + 64], src[1][r0 // 2:r0 // 2 + 32], src[2][r0 // 2:r0 // 2 + 32]]
            want = twin.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, strip)
            _equal([got[0][r0:r0 + 64], got[1][r0 // 2:r0 // 2 + 32], got[2][r0 // 2:r0 // 2 + 32]], want, f"UHD rows {r0}")
    finally:
        engine.set_precision("strict")
        engine.set_variant("auto")


@pytest.mark.gpu
def test_fma32_falls_back_to_strict_where_it_does_not_apply(engine, orc, tmp_path):
    from tests.test_lut_formats import _csp_with_prelut
    one = np.ones(3, np.float32)
    k = orc.yuv_constants(din=10)
    src = frames.make_yuv("natural", 256, 72, 10, 1, 1, k=31)
    engine.set_precision("fma32")
    try:
        engine.set_variant("vec_lds")
        # a lattice outside [0, 1]
        rng = np.random.default_rng(9)
        lat = rng.uniform(-0.2, 1.2, size=(9, 9, 9, 3)).astype(np.float32)
        engine.set_lut(cube.CubeLut(9, one, lat))
        for mode in ("tetrahedral", "trilinear"):
            got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le", interp=mode), 10)
            assert "fma32" not in engine.last_kernel, engine.last_kernel
            _equal(got, orc.apply_yuv(lat, one, mode, k, 10, 10, 10, 1, 1, src), f"non-unit {mode}")
        # a .csp prelut
        tab = cube.log709_lattice(33)
        xs = np.linspace(0.0, 1.0, 33)
        p = tmp_path / "shared.csp"
        _csp_with_prelut(p, 33, tab, [(xs, xs ** 0.55)] * 3)
        engine.set_lut(cube.read_lut(p))
        _, s2, t2, pre = orc.parse_lut_file_ex(p)
        got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le"), 10)
        assert "fma32" not in engine.last_kernel, engine.last_kernel
        _equal(got, orc.apply_yuv(t2, s2, "tetrahedral", k, 10, 10, 10, 1, 1, src, prelut=pre), "prelut")
        lat = cube.log709_lattice(33)
        engine.set_lut(cube.CubeLut(33, one, lat))
        # dither
        got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le", out_pix_fmt="yuv420p",
                                     dither="error_diffusion"), 8)
        assert "fma32" not in engine.last_kernel, engine.last_kernel
        k8 = orc.yuv_constants(din=10, dl=10, dout=8)
        _equal(got, orc.apply_yuv(lat, one, "tetrahedral", k8, 10, 10, 8, 1, 1, src, dither="error_diffusion"), "dither")
        # planar RGB
        rgb = frames.make_rgb("natural", 256, 64, 10, k=32)
        got = [t.cpu().numpy().view(np.uint16) for t in engine.apply_rgb(_dev(rgb, engine.device), depth=10)]
        assert "fma32" not in engine.last_kernel, engine.last_kernel
        _equal(got, orc.apply_rgb(lat, one, 10, "tetrahedral", rgb), "planar rgb")
        # a ragged width: the tile kernels take the aligned columns, the generic kernel the rest
        # (rows padded to an aligned stride, as a decoder leaves them: dense rows of a ragged width go to the generic kernel whole)
        engine.set_variant("auto")
        import torch
        rsrc = frames.make_yuv("natural", 250, 72, 10, 1, 1, k=33)
        sdev, ddev = [], []
        for a in rsrc:
            buf = torch.zeros((a.shape[0], 256), dtype=torch.int16, device=engine.device)
            buf[:, :a.shape[1]] = torch.from_numpy(a.view(np.int16)).to(engine.device)
            sdev.append(buf[:, :a.shape[1]])
            ddev.append(torch.zeros_like(buf)[:, :a.shape[1]])
        got = _host(engine.apply_yuv(sdev, ddev, pix_fmt="yuv420p10le"), 10)
        kern = engine.last_kernel
        assert ",fma32" in kern, kern
        want = twin.apply_yuv(lat, one, "tetrahedral", k, 10, 10, 10, 1, 1, rsrc)
        _equal([got[0][:, :248], got[1][:, :124], got[2][:, :124]], [want[0][:, :248], want[1][:, :124], want[2][:, :124]],
               "ragged width, tile part")
        assert _max_diff(got, orc.apply_yuv(lat, one, "tetrahedral", k, 10, 10, 10, 1, 1, rsrc)) <= 1
    finally:
        engine.set_precision("strict")
        engine.set_variant("auto")


@pytest.mark.gpu
def test_fma32_lattice_changes_leave_no_stale_copy(engine, orc):
    from lut_renderer_amd.multigpu import LutEngineGroup
    one = np.ones(3, np.float32)
    k = orc.yuv_constants(din=10)
    src = frames.make_yuv("natural", 256, 72, 10, 1, 1, k=41)
    lat_a = cube.log709_lattice(33)
    lat_b = np.ascontiguousarray(lat_a[..., ::-1]) * np.float32(0.9)        # same size, other nodes
    engine.set_variant("vec_lds")
    engine.set_precision("fma32")
    try:
        for lat in (lat_a, lat_b):
            engine.set_lut(cube.CubeLut(33, one, lat))
            got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le"), 10)
            assert ",fma32" in engine.last_kernel, engine.last_kernel
            _equal(got, twin.apply_yuv(lat, one, "tetrahedral", k, 10, 10, 10, 1, 1, src), "one engine, lattice change")
    finally:
        engine.set_precision("strict")
        engine.set_variant("auto")
    with LutEngineGroup([0, 0]) as grp:
        grp.set_variant("vec_lds")
        grp.set_precision("fma32")
        recv = grp.engines[1]
        for lat in (lat_a, lat_b):
            grp.set_lut(cube.CubeLut(33, one, lat))            # lutr_lut_broadcast into the second context
            got = _host(recv.apply_yuv(_dev(src, recv.device), pix_fmt="yuv420p10le"), 10)
            assert ",fma32" in recv.last_kernel, recv.last_kernel
            _equal(got, twin.apply_yuv(lat, one, "tetrahedral", k, 10, 10, 10, 1, 1, src), "broadcast receiver")
        got = _host(grp.apply_yuv(_dev(src, recv.device), pix_fmt="yuv420p10le"), 10)
        _equal(got, twin.apply_yuv(lat_b, one, "tetrahedral", k, 10, 10, 10, 1, 1, src), "group apply")


@pytest.mark.gpu
def test_fma32_through_apply_lut_and_the_cli(orc, cube_dir, tmp_path):
    from lut_renderer_amd import api
    lut = cube.read_cube(cube_dir / "log709_33.cube")
    k = orc.yuv_constants(din=10)
    src = frames.natural_yuv(512, 128, 10, 1, 1, k=55)
    want = twin.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, src)
    try:
        eng = api._cached_engine((0,))
        eng.set_variant("vec_lds")
        out, _ = api.apply_lut(_dev(src, "cuda:0"), cube=lut, pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv",
                               precision="fma32")
        assert ",fma32" in eng.last_kernel, eng.last_kernel
        _equal(_host(out, 10), want, "apply_lut fma32")
        with pytest.raises(ValueError, match="fma32"):
            api.apply_lut(_dev(src, "cuda:0"), cube=lut, pix_fmt="yuv420p10le", precision="fp16")
    finally:
        api.close_cached_engines()
    src = frames.natural_yuv(256, 64, 10, 1, 1, k=56)
    want = twin.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, src)
    raw = tmp_path / "in.yuv"
    raw.write_bytes(b"".join(np.ascontiguousarray(p).tobytes() for p in src) * 3)
    out = tmp_path / "out.yuv"
    cmd = [sys.executable, "-m", "lut_renderer_amd.cli", "-y", "-i", "-", "-o", "-", "--size", "256x64",
           "--pix-fmt", "yuv420p10le", "--cube", str(cube_dir / "log709_33.cube"), "--colorspace", "bt709",
           "--color-range", "tv", "--fps", "25", "--precision", "fma32"]
    env = dict(__import__("os").environ, LUTR_SMALL_JOB_MPX="0")
    with open(raw, "rb") as fi, open(out, "wb") as fo:
        r = subprocess.run(cmd, cwd=ROOT, stdin=fi, stdout=fo, stderr=subprocess.PIPE, text=False, timeout=300, env=env)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-2000:]
    data = np.frombuffer(out.read_bytes(), dtype=np.uint16)
    flat = np.concatenate([p.reshape(-1) for p in want])
    assert data.size == 3 * flat.size
    for f in range(3):
        assert np.array_equal(data[f * flat.size:(f + 1) * flat.size], flat), f


@pytest.mark.gpu
def test_precision_switches_on_one_context(engine, orc, cube_dir):
    lut = cube.read_cube(cube_dir / "log709_33.cube")
    engine.set_lut(lut)
    engine.set_variant("vec_lds")
    k = orc.yuv_constants(din=10)
    src = frames.make_yuv("natural", 256, 72, 10, 1, 1, k=61)
    strict = orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, src)
    fma32 = twin.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, src)
    try:
        for prec, want in (("strict", strict), ("fma32", fma32), ("strict", strict), ("fast", None), ("fma32", fma32)):
            engine.set_precision(prec)
            got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le"), 10)
            kern = engine.last_kernel
            assert (",fma32" in kern) == (prec == "fma32") and (",fast" in kern) == (prec == "fast"), (prec, kern)
            if want is not None:
                _equal(got, want, prec)
        with pytest.raises(ValueError, match="fma32"):
            engine.set_precision("fp16")
    finally:
        engine.set_precision("strict")
        engine.set_variant("auto")
