"""LUT strength without a GPU: the twin's two identities and its bounds, the clamp, the key frames of
`params.strength_keys`, the refusals through every layer (each message names the option and the strength), the stage lists the
options imply, and the argv."""
import threading
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from lut_renderer_amd import cube, frames
from lut_renderer_amd.cdl import Cdl
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.formats import check_stack_options, check_strength, implied_stages
from lut_renderer_amd.params import ProcessingParams, VideoInfo, strength_keys
from tests import _mix_twin as twin
from tests import _stack_twin as stk

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
F = np.float32
NAMES = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")


def _pairs(depth):
    """(q0, q1) code arrays: every pair of codes at 8 bit, a million random pairs with the extremes among them above."""
    m = (1 << depth) - 1
    if depth == 8:
        a, b = np.meshgrid(np.arange(m + 1), np.arange(m + 1), indexing="ij")
        return a.ravel(), b.ravel()
    rng = np.random.default_rng(depth)
    a, b = rng.integers(0, m + 1, 1 << 20), rng.integers(0, m + 1, 1 << 20)
    a[:4], b[:4] = [0, m, 0, m], [m, 0, 0, m]
    return a, b


# ------------------------------------------------------------------ the arithmetic
@pytest.mark.parametrize("depth", [8, 10, 16])
def test_strength_0_is_the_source_and_1_is_the_grade(depth):
    a, b = _pairs(depth)
    assert np.array_equal(twin.mix_codes(0.0, [a], [b])[0], a)
    assert np.array_equal(twin.mix_codes(1.0, [a], [b])[0], b)
    assert np.array_equal(twin.mix_codes(-0.0, [a], [b])[0], a)


@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("s", [0.25, 0.5, 1.0 / 3.0, 0.999])
def test_the_mix_stays_between_source_and_grade(depth, s):
    a, b = _pairs(depth)
    q = twin.mix_codes(s, [a], [b])[0]
    assert (q >= np.minimum(a, b)).all() and (q <= np.maximum(a, b)).all()
    # and it is the rounded blend: within half a code (and the three fp32 roundings) of the exact value
    exact = a + float(F(s)) * (b - a)
    assert np.abs(q - exact).max() <= 0.5 + 2.0 ** (depth - 22)


def test_the_clamp():
    assert twin.clamp(1.5) == F(1.0) and twin.clamp(-1.0) == F(0.0) and twin.clamp(np.nan) == F(0.0)
    assert twin.clamp(0.37) == F(0.37)
    a, b = _pairs(10)
    for s, like in ((1.5, 1.0), (-1.0, 0.0), (np.nan, 0.0)):
        assert np.array_equal(twin.mix_codes(s, [a], [b])[0], twin.mix_codes(like, [a], [b])[0])
    got = twin.clamp(np.array([1.5, -1.0, np.nan, 0.5]))
    assert got.dtype == F and np.array_equal(got, np.array([1.0, 0.0, 0.0, 0.5], F))


def test_a_strength_per_frame_broadcasts_over_the_frames():
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 1024, (4, 6, 8)), rng.integers(0, 1024, (4, 6, 8))
    s = [0.0, 1.0, 0.37, 0.5]
    q = twin.mix_codes(np.array(s), [a], [b])[0]
    for f in range(4):
        assert np.array_equal(q[f], twin.mix_codes(s[f], [a[f]], [b[f]])[0])
    assert np.array_equal(q[0], a[0]) and np.array_equal(q[1], b[1])


def test_the_twin_on_frames():
    """The whole twin on a 4:2:0 -> 4:2:2 batch: frame 0 (s = 0) is stages 1 and 3 alone, frame 1 (s = 1) the stack's twin."""
    from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
    lut = cube.CubeLut(9, np.ones(3, F), np.random.default_rng(11).uniform(0.0, 1.0, (9, 9, 9, 3)).astype(F))
    fs = [frames.natural_yuv(38, 12, 10, 1, 1, k=i) for i in range(3)]
    src = [np.stack([f[i] for f in fs]) for i in range(3)]
    k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 1, 0)
    grade = Cdl(slope=(0.9, 1.1, 1.0), offset=(0.02, 0.0, -0.01), power=(1.2, 1.0, 0.9), saturation=0.8)
    got = twin.apply(("cdl", "lut3d"), [0.0, 1.0, 0.6], k, 10, 10, 1, 1, 1, 0, src, lut=lut, cdl=grade)
    plain = rgb_codes_to_yuv(k, 10, 1, 0, yuv_to_rgb_codes(k, 1, 1, fs[0]))
    full = stk.apply(("cdl", "lut3d"), k, 10, 10, 1, 1, 1, 0, fs[1], lut=lut, cdl=grade)
    one = twin.apply(("cdl", "lut3d"), 0.6, k, 10, 10, 1, 1, 1, 0, fs[2], lut=lut, cdl=grade)
    for i in range(3):
        assert np.array_equal(got[i][0], plain[i]) and np.array_equal(got[i][1], full[i]) and np.array_equal(got[i][2], one[i])
    assert not np.array_equal(one[0], full[0])


# ------------------------------------------------------------------ key frames
def test_strength_keys_known_answers():
    ramp = strength_keys("0:0,24:1")
    got = ramp(0, 25)
    assert got.dtype == F and got.shape == (25,)
    assert np.array_equal(got, (np.arange(25, dtype=np.float64) / 24.0).astype(F))
    assert got[0] == 0.0 and got[12] == F(0.5) and got[24] == 1.0
    # held before the first key and behind the last
    late = strength_keys("10:0.25, 20:0.75")
    assert np.array_equal(late(0, 11), np.full(11, 0.25, F)) and np.array_equal(late(20, 5), np.full(5, 0.75, F))
    assert np.array_equal(late(14, 3), np.array([0.45, 0.5, 0.55], np.float64).astype(F))
    # a batch that straddles a key, and batches that tile the stream give the stream's values
    tri = strength_keys("0:0,3:1,5:0")
    assert np.array_equal(tri(2, 3), np.array([2.0 / 3.0, 1.0, 0.5]).astype(F))
    whole = tri(0, 9)
    assert np.array_equal(np.concatenate([tri(0, 2), tri(2, 2), tri(4, 5)]), whole)
    assert np.array_equal(whole, np.array([0, 1.0 / 3.0, 2.0 / 3.0, 1, 0.5, 0, 0, 0, 0]).astype(F))
    assert np.array_equal(strength_keys("7:0.3")(0, 4), np.full(4, 0.3, F)) and tri(4, 0).shape == (0,)


@pytest.mark.parametrize("text,fault", [("", "no key"), ("3:1,0:0", "unsorted"), ("0:0,2:1,1:0.5", "unsorted"), ("0:0,0:1", "duplicate"),
                                        ("0:0,4:1,0:1", "duplicate"), ("a:1", "malformed"), ("0", "malformed"), ("0:", "malformed"),
                                        ("0:0,,2:1", "malformed"), ("1.5:1", "malformed"), ("0:x", "malformed"), ("0:1.2", "outside"),
                                        ("0:-0.1", "outside"), ("0:nan", "outside"), ("0:inf", "outside"), ("-1:0.5", "negative")])
def test_strength_keys_refusals(text, fault):
    with pytest.raises(ValueError, match=fault) as e:
        strength_keys(text)
    assert f"'{text}'" in str(e.value)


# ------------------------------------------------------------------ the strength argument
def test_check_strength():
    assert check_strength(None) is None
    assert check_strength(0.6) == 0.6 and check_strength(1) == 1.0 and check_strength(np.float32(0.5)) == 0.5
    got = check_strength([0.0, 1.0, 0.37, 0.5], 4)
    assert got.dtype == F and np.array_equal(got, np.array([0.0, 1.0, 0.37, 0.5], F))
    assert np.array_equal(check_strength(np.linspace(0, 1, 5)), np.linspace(0, 1, 5).astype(F))
    import torch
    assert np.array_equal(check_strength(torch.tensor([0.25, 0.75]), 2), np.array([0.25, 0.75], F))
    for bad, message in ((1.2, r"strength 1\.2 is outside \[0, 1\]"), (float("nan"), "strength nan is outside"), (-0.5, "strength -0.5"),
                         ([0.5, 0.5, 0.5], "strength has 3 entries for 4 frames"), ([0.1, 0.2, 1.2, 0.3], r"strength\[2\] = 1\.2"),
                         ([0.1, float("nan"), 0.2, 0.3], r"strength\[1\] = nan"), ([0.1, float("inf"), 0.2, 0.3], r"strength\[1\] = inf"),
                         ([[0.1, 0.2], [0.3, 0.4]], "flat sequence"), ("0.5", "strength is a number")):
        with pytest.raises(ValueError, match=message):
            check_strength(bad, 4)


# ------------------------------------------------------------------ refusals, layer by layer
REFUSED = ((dict(dither="blue_noise"), "dither"), (dict(chroma_loc="left"), "chroma_loc"), (dict(out_size=(8, 4)), "out_size"),
           (dict(out2_pix_fmt="yuv420p"), "out2_pix_fmt"), (dict(alpha_mode="premultiplied"), "alpha_mode"),
           (dict(out_pix_fmt="nv12"), "semi-planar"), (dict(out_pix_fmt="v210"), "v210"), (dict(out_pix_fmt="uyvy422"), "packed"),
           (dict(pix_fmt="gbrp10le"), "RGB"), (dict(pix_fmt="gbrpf32le"), "float"), (dict(precision="fast"), "precision"),
           (dict(variant="vec_lds"), "vec_lds"))


@pytest.mark.parametrize("kw,word", REFUSED, ids=[w for _, w in REFUSED])
def test_check_stack_options_names_the_option_and_the_strength(kw, word):
    with pytest.raises(ValueError) as e:
        check_stack_options(**{**NAMES, "stages": "lut3d", "strength": 0.5, **kw})
    assert word in str(e.value) and "strength" in str(e.value)
    if word != "precision":                                    # today's message without a strength: no word of it
        with pytest.raises(ValueError) as e:
            check_stack_options(**{**NAMES, "stages": "lut3d", **kw})
        assert word in str(e.value) and "strength" not in str(e.value)
    else:
        check_stack_options(**{**NAMES, "stages": "lut3d", **kw})


def test_check_stack_options_checks_the_strength_itself():
    for bad, message in ((1.2, r"strength 1\.2"), (float("nan"), "strength nan"), ([0.5, 2.0], r"strength\[1\] = 2\.0")):
        with pytest.raises(ValueError, match=message):
            check_stack_options(**NAMES, stages="lut3d", strength=bad)
    st, fin, fout = check_stack_options(**NAMES, stages="lut3d", strength=[0.0, 1.0], precision="strict")
    assert st == (("lut3d", "tetrahedral"),) and fin.name == "yuv420p10le" and fout.name == "yuv422p10le"


def _planes(nf=None):
    y = frames.natural_yuv(16, 8, 10, 1, 1)
    return y if nf is None else [np.stack([p] * nf) for p in y]


def test_the_engine_and_the_group_refuse_before_they_are_touched():
    from lut_renderer_amd.multigpu import LutEngineGroup
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False)
    for kw, message in ((dict(dither="blue_noise"), "dither .* with strength"), (dict(out_size=(8, 4)), "out_size .* with strength"),
                        (dict(strength=1.2), r"strength 1\.2 is outside"), (dict(strength=float("nan")), "strength nan"),
                        (dict(strength=[0.1, 0.2, 7.0]), r"strength\[2\] = 7\.0")):
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_yuv_stack(held, _planes(), **{**NAMES, "stages": "lut3d", "strength": 0.5, **kw})
    g = SimpleNamespace(_lock=threading.RLock(), n1d=17, engines=[SimpleNamespace(n=33, n2=0, _has_prelut=False)])
    for kw, message in ((dict(dither="blue_noise"), "dither .* with strength"), (dict(strength=1.2), r"strength 1\.2"),
                        (dict(strength=[0.5] * 3), "strength has 3 entries for 4 frames")):
        with pytest.raises(ValueError, match=message):
            LutEngineGroup.apply_yuv_stack(g, _planes(4), **{**NAMES, "stages": "lut3d", "strength": 0.5, **kw})


def _lut(n=2):
    return cube.CubeLut(n, np.ones(3, F), cube.identity_lattice(n).astype(F))


def test_apply_lut_refuses_while_planning():
    from lut_renderer_amd.api import apply_lut
    base = dict(NAMES, cube=_lut(), engine=SimpleNamespace(n=0, n2=0, n1d=0, _has_prelut=False))
    for kw, message in ((dict(engine_dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a stage stack with strength"),
                        (dict(zscale_dither="error_diffusion"), "dither .* with strength"),
                        (dict(resolution="8x4"), r"\(out_size / resolution\) is not supported with a stage stack with strength"),
                        (dict(chroma_loc="left"), "chroma_loc.* with strength"), (dict(second_pix_fmt="yuv420p"), "out2_pix_fmt.* with strength"),
                        (dict(precision="fma32"), "precision='fma32' is not supported with strength"),
                        (dict(out_pix_fmt="p010le"), r"stack \(strength\) pass .* semi-planar"),
                        (dict(pix_fmt="gbrp10le"), r"stack \(strength\) pass .* RGB"),
                        (dict(strength=1.2), r"strength 1\.2 is outside"), (dict(strength=float("nan")), "strength nan is outside"),
                        (dict(strength=[0.2, 1.2]), r"strength\[1\] = 1\.2"),
                        (dict(stages="lut3d", engine_dither="blue_noise"), "dither .* with strength")):
        with pytest.raises(ValueError, match=message):
            apply_lut(_planes(), **{**base, "strength": 0.5, **kw})


class _Lock:
    def __enter__(self): return self
    def __exit__(self, *exc): return False


class _Eng:
    """What `apply_lut` needs of an engine: it records the call it is handed."""
    _lock, precision, _applied_lut, _applied_lut2, _applied_lut1d, _has_prelut = _Lock(), "strict", None, None, None, False
    n = n2 = n1d = 0

    def __init__(self): self.calls = []
    def apply_yuv(self, planes, out, **kw): self.calls.append(("yuv", kw)); return out
    def apply_yuv_lut1d(self, planes, out, **kw): self.calls.append(("lut1d", kw)); return out
    def apply_yuv_chain(self, planes, out, **kw): self.calls.append(("chain", kw)); return out
    def apply_yuv_stack(self, planes, out, **kw): self.calls.append(("stack", kw)); return out
    def set_lut1d(self, l1, mode): pass
    def set_lut(self, lut): pass
    def set_lut2(self, lut): pass


def test_the_stage_lists_the_options_imply():
    from lut_renderer_amd.api import apply_lut
    assert implied_stages(True) == ("lut3d",) and implied_stages(True, cdl=True) == ("cdl", "lut3d")
    assert implied_stages(True, lut1d=True) == ("lut1d", "lut3d") and implied_stages(False, lut1d=True) == ("lut1d",)
    assert implied_stages(True, cube2=True) == ("lut3d", "lut3d2")
    assert implied_stages(True, True, True, True) == ("lut1d", "cdl", "lut3d", "lut3d2")
    assert implied_stages(False) == ("lut3d",)                 # (an engine that already holds the lattice)
    eng, y = _Eng(), _planes()
    A, B, l1, grade = _lut(2), _lut(3), cube.Lut1D.identity(16), Cdl(saturation=0.6)
    T = "tetrahedral"
    cases = ((dict(cube=A), "yuv", (("lut3d", T),)),
             (dict(cube=A, cdl=grade), "yuv", (("cdl", None), ("lut3d", T))),
             (dict(cube=A, lut1d=l1), "lut1d", (("lut1d", None), ("lut3d", T))),
             (dict(cube=None, lut1d=l1), "lut1d", (("lut1d", None),)),
             (dict(cube=A, cube2=B, interp2="nearest"), "chain", (("lut3d", T), ("lut3d2", "nearest"))))
    for kw, route, want in cases:
        apply_lut(y, **NAMES, engine=eng, **kw)
        assert eng.calls[-1][0] == route and "strength" not in eng.calls[-1][1], kw     # no strength: the dedicated route, as it was
        apply_lut(y, **NAMES, engine=eng, strength=0.5, **kw)
        name, call = eng.calls[-1]
        assert name == "stack" and call["stages"] == want and call["strength"] == 0.5, kw
        assert call["cdl"] == kw.get("cdl") and call["out_pix_fmt"] == "yuv422p10le"
    # with `stages` the list is used as given, and a sequence travels as it is
    apply_lut(y, **NAMES, engine=eng, cube=A, lut1d=l1, stages="lut3d,lut1d", strength=[0.25])
    assert eng.calls[-1][1]["stages"] == (("lut3d", T), ("lut1d", None)) and eng.calls[-1][1]["strength"] == [0.25]
    apply_lut(y, **NAMES, engine=eng, cube=A, stages="lut3d")
    assert "strength" not in eng.calls[-1][1]


# ------------------------------------------------------------------ the CLI and the argv
def _args(*extra, pix_fmt="yuv420p10le", out="yuv422p10le"):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt, "--out-pix-fmt", out, *extra])


def test_cli_flags(cube_dir, capsys):
    from lut_renderer_amd.cli import plan_from_args
    a, t = str(cube_dir / "log709_33.cube"), str(GOLDEN / "lut1d" / "curve17.cube")
    _, plain, _, _ = plan_from_args(_args("--cube", a))
    assert "stages" not in plain and "strength" not in plain
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--strength", "0.6"))
    assert kw["stages"] == (("lut3d", "tetrahedral"),) and kw["strength"] == 0.6 and "strength_keys" not in kw
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--cdl-sat", "0.5", "--interp", "trilinear", "--strength-keys", "0:0,24:1"))
    assert kw["stages"] == (("cdl", None), ("lut3d", "trilinear")) and "strength" not in kw
    assert np.array_equal(kw["strength_keys"](23, 3), np.array([23.0 / 24.0, 1.0, 1.0]).astype(F))
    _, kw, _, _ = plan_from_args(_args("--lut1d", t, "--strength", "1"))
    assert kw["stages"] == (("lut1d", None),)
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--lut1d", t, "--stages", "lut3d,lut1d", "--strength", "0"))
    assert kw["stages"] == (("lut3d", "tetrahedral"), ("lut1d", None)) and kw["strength"] == 0.0
    with pytest.raises(SystemExit):                             # both flags together: the parser's own refusal
        _args("--cube", a, "--strength", "0.5", "--strength-keys", "0:0,24:1")
    assert "--strength-keys" in capsys.readouterr().err
    with pytest.raises(ValueError, match="mutually exclusive"):
        plan_from_args(SimpleNamespace(**{**vars(_args("--cube", a, "--strength", "0.5")), "strength_keys": "0:1"}))
    for extra, message in ((("--strength", "1.2"), r"strength 1\.2 is outside"), (("--strength", "nan"), "strength nan"),
                           (("--strength-keys", "3:1,0:0"), "strength keys '3:1,0:0': the keys are unsorted"),
                           (("--strength", "0.5", "--engine-dither", "blue_noise"), "dither .* with strength"),
                           (("--strength", "0.5", "--zscale-dither", "error_diffusion"), "dither .* with strength"),
                           (("--strength-keys", "0:1", "--out-size", "8x4"), "out_size .* with strength"),
                           (("--strength", "0.5", "--chroma-loc", "left"), "chroma_loc.* with strength"),
                           (("--strength", "0.5", "--precision", "fast"), "precision='fast' is not supported with strength"),
                           (("--strength", "0.5", "--second-output", "x", "--second-pix-fmt", "yuv420p"), "out2_pix_fmt.* with strength")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args("--cube", a, *extra))
    with pytest.raises(ValueError, match=r"stack \(strength\) pass .* semi-planar"):
        plan_from_args(_args("--cube", a, "--strength", "0.5", pix_fmt="nv12", out="nv12"))
    with pytest.raises(ValueError, match=r"stack \(strength\) pass .* RGB"):
        plan_from_args(_args("--cube", a, "--strength", "0.5", pix_fmt="gbrp10le"))


def test_engine_command_renders_the_flags_and_round_trips(cube_dir):
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.pipe import engine_stage_commands
    a = cube_dir / "log709_33.cube"
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    params = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")
    io = (Path("-"), Path("-"), params, a, info)
    plain = engine_command(*io)
    assert engine_command(*io, strength=None, strength_keys=None) == plain and "--strength" not in plain
    assert engine_command(*io, strength=0.6) == plain + ["--strength", "0.6"]
    assert engine_command(*io, strength_keys="0:0,24:1") == plain + ["--strength-keys", "0:0,24:1"]
    grade = Cdl(saturation=0.5)
    cmd = engine_command(*io, cdl=grade, strength=0.25)
    assert cmd[-2:] == ["--strength", "0.25"] and "--stages" not in cmd
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert kw["stages"] == (("cdl", None), ("lut3d", "tetrahedral")) and kw["strength"] == 0.25 and kw["cdl"] == grade
    cmd = engine_command(*io, stages="lut3d:trilinear", strength_keys="0:0,3:1")
    assert cmd[-4:] == ["--stages", "lut3d:trilinear", "--strength-keys", "0:0,3:1"]
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert kw["stages"] == (("lut3d", "trilinear"),) and np.array_equal(kw["strength_keys"](0, 4), strength_keys("0:0,3:1")(0, 4))
    stage = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, strength_keys="0:0,24:1")
    assert stage.engine[stage.engine.index("--strength-keys") + 1] == "0:0,24:1" and "--strength-keys" not in stage.encoder
    assert "--strength" in engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, strength=0.5).engine
    for kw, message in ((dict(strength=0.5, strength_keys="0:1"), "mutually exclusive"), (dict(strength=1.2), r"strength 1\.2"),
                        (dict(strength_keys="0:0,0:1"), "duplicate"), (dict(strength=0.5, engine_dither="blue_noise"), "dither .* with strength"),
                        (dict(strength=0.5, precision="fast"), "precision='fast' is not supported with strength"),
                        (dict(strength=0.5, chroma_loc="left"), "chroma_loc.* with strength")):
        with pytest.raises(ValueError, match=message):
            engine_command(*io, **kw)


def test_the_stream_counts_frames_across_batches():
    """HostPipeline's bookkeeping without a device: the keys are read at the frame's number in the stream."""
    from lut_renderer_amd.stream import HostPipeline
    seen = []
    eng = SimpleNamespace(apply_yuv_stack=lambda src, dst, **kw: seen.append(kw["strength"]))
    pipe = SimpleNamespace(stack=True, kw={"stages": "lut3d"}, strength_keys=strength_keys("0:0,3:1"), frames_submitted=0, eng=eng)
    for n in (2, 2, 1):
        HostPipeline._run_stack(pipe, None, None, n)
    assert [s.tolist() for s in seen] == [strength_keys("0:0,3:1")(f, n).tolist() for f, n in ((0, 2), (2, 2), (4, 1))]
    assert np.array_equal(np.concatenate(seen), np.array([0, 1.0 / 3.0, 2.0 / 3.0, 1, 1]).astype(F)) and pipe.frames_submitted == 5
