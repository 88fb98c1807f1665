"""The stage stack on packed 4:2:2 / v210 frames without a GPU: the one copy of the pass's refusals
(`formats.check_packed_stack_options`), every layer refusing the same rows before an engine is touched, the routing of `apply_lut`,
`HostPipeline` and the CLI against a fake engine, the CLI flag and its round trip through `engine_command`, and the old names
still refusing these sides."""
import threading
from pathlib import Path
from types import SimpleNamespace

import pytest

from lut_renderer_amd import _native, cube, frames, packedyuv, v210
from lut_renderer_amd.cdl import Cdl
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.formats import (PackedYuvFmt, PixFmt, V210Fmt, check_packed_stack_options, check_semi_stack_options,
                                      check_stack_options)

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
TAIL = r"a stage stack on packed 4:2:2 / v210 frames \(packed_stages\)"
FULL = dict(stages="lut1d,cdl,lut3d,lut3d2", cdl=True)
PACKED = list(_native.PACKED_YUV_FORMATS)
PLANAR_DST = ["yuv422p", "yuv420p", "yuv444p", "yuv422p10le", "yuv420p12le", "yuv444p16le", "yuv422p9le"]
PLANAR_SRC = ["yuv422p", "yuv422p10le", "yuv422p12le", "yuv422p16le"]
#: what the pass refuses, by keyword of the check -> the words of the refusal
OPTIONS = [(dict(dither="error_diffusion"), rf"dither \('error_diffusion'\) is not supported with {TAIL}"),
           (dict(dither="blue_noise"), rf"dither \('blue_noise'\) is not supported with {TAIL}"),
           (dict(chroma_loc="left"), rf"sited chroma resampling \(chroma_loc\) is not supported with {TAIL}"),
           (dict(out_size=(8, 4)), rf"a resize \(out_size / resolution\) is not supported with {TAIL}"),
           (dict(out2_pix_fmt="yuv420p"), rf"the two-output pass \(out2_pix_fmt\) is not supported with {TAIL}"),
           (dict(alpha_mode="premultiplied"), rf"alpha_mode='premultiplied' is not supported with {TAIL}"),
           (dict(strength=0.5), rf"a LUT strength \(strength\) is not supported with {TAIL}"),
           (dict(matte=True), rf"a matte \(matte\) is not supported with {TAIL}")]
SIDES = [("yuva422p10le", rf"alpha .* is not supported with {TAIL}: packed 4:2:2 and v210 frames carry no alpha"),
         ("nv16", rf"a semi-planar side .* is not supported with {TAIL}"), ("p210le", rf"a semi-planar side .* is not supported with {TAIL}"),
         ("nv24", rf"a semi-planar side .* is not supported with {TAIL}"),
         ("rgb24", rf"an RGB side .* is not supported with {TAIL}"), ("gbrp10le", rf"an RGB side .* is not supported with {TAIL}"),
         ("gbrpf32le", rf"a float side .* is not supported with {TAIL}"),
         ("v210x", rf"'v210x' is not supported with {TAIL}: of this family only v210 is taken"),
         ("v410", rf"'v410' is not supported with {TAIL}: of this family only v210 is taken"),
         ("vuya", rf"'vuya' is not supported with {TAIL}: packed YUV frames are taken as little-endian 4:2:2"),
         ("xv30le", rf"'xv30le' is not supported with {TAIL}"), ("y210be", rf"'y210be' is not supported with {TAIL}")]


# ------------------------------------------------------------------ what the check takes
@pytest.mark.parametrize("name", PACKED + ["v210"])
def test_every_container_on_either_side(name):
    kind = V210Fmt if name == "v210" else PackedYuvFmt
    st, fin, fout = check_packed_stack_options(name, None, **FULL)
    assert isinstance(fin, kind) and fout == fin and [k for k, _ in st] == ["lut1d", "cdl", "lut3d", "lut3d2"]
    assert (fin.csx, fin.csy) == (1, 0)
    for other in PLANAR_DST:                                           # a packed / v210 source: 4:2:2, 4:2:0 or 4:4:4 at 8..16 bit
        _, fin, fout = check_packed_stack_options(name, other, **FULL)
        assert (fin.name, fout.name) == (name, other) and isinstance(fout, PixFmt) and fout.nplanes == 3
    for other in PLANAR_SRC:                                           # a packed / v210 destination: a 4:2:2 source
        _, fin, fout = check_packed_stack_options(other, name, **FULL)
        assert (fin.name, fout.name) == (other, name) and isinstance(fin, PixFmt) and isinstance(fout, kind)
    for other in ("yuv420p", "yuv444p10le"):
        with pytest.raises(ValueError, match=rf"destination takes a 4:2:2 source: no chroma subsampling change into '{name}'"):
            check_packed_stack_options(other, name, **FULL)


def test_packed_names_mix_with_each_other_and_not_with_v210():
    for a in PACKED:
        for b in PACKED:
            check_packed_stack_options(a, b, stages="lut3d")
        for src, dst in ((a, "v210"), ("v210", a)):
            with pytest.raises(ValueError, match=rf"a packed 4:2:2 side together with a v210 side is not supported with {TAIL} "
                                                 rf"\('{src}' -> '{dst}'\)"):
                check_packed_stack_options(src, dst, stages="lut3d")
    with pytest.raises(ValueError, match="both sides are planar: use apply_yuv_stack"):
        check_packed_stack_options("yuv422p10le", "yuv422p10le", stages="lut3d")
    with pytest.raises(ValueError, match="both sides are planar: use apply_yuv_stack"):
        check_packed_stack_options("yuv422p", None, stages="lut3d")


def test_what_else_the_check_takes():
    check_packed_stack_options("yuvj422p", "uyvy422", stages="lut3d")     # yuvj* is read as yuv*
    check_packed_stack_options("v210", None, stages="lut3d,cdl,lut3d2", cdl=True, prelut=True)   # a prelut where lut3d is fed codes
    for variant in (None, "auto", "generic", "vec_global"):
        check_packed_stack_options("v210", "yuv422p10le", **FULL, variant=variant)
    for precision in (None, "strict", "fast", "fma32"):                 # as the stack without a strength: the pass runs strict
        check_packed_stack_options("y210le", None, **FULL, precision=precision)


# ------------------------------------------------------------------ what it refuses
@pytest.mark.parametrize("kw,message", OPTIONS, ids=[next(iter(k)) + str(i) for i, (k, _) in enumerate(OPTIONS)])
def test_every_option_the_pass_does_not_take(kw, message):
    for names in (("v210", "yuv422p10le"), ("uyvy422", None), ("yuv422p10le", "y210le")):
        with pytest.raises(ValueError, match=message):
            check_packed_stack_options(*names, **FULL, **kw)


@pytest.mark.parametrize("name,message", SIDES)
def test_a_side_the_pass_does_not_take(name, message):
    for mine in ("uyvy422", "v210"):
        with pytest.raises(ValueError, match=message):
            check_packed_stack_options(mine, name, stages="lut3d")
        with pytest.raises(ValueError, match=message):
            check_packed_stack_options(name, mine, stages="lut3d")


def test_the_list_and_the_variants():
    names = dict(pix_fmt="v210", out_pix_fmt="v210")
    for kw, message in ((dict(stages="lut1d,matrix,lut3d", rgb_matrix=True), rf"stage 'matrix' is not supported with {TAIL}"),
                        (dict(stages="lut3d", rgb_matrix=True), rf"stage 'matrix' is not supported with {TAIL}"),
                        (dict(stages="matrix"), rf"stage 'matrix' is not supported with {TAIL}"),
                        (dict(stages=""), "the stage list is empty"), (dict(stages="lut3d,lut3d"), "listed twice"),
                        (dict(stages="lut3d", lut=False), "no 3D LUT is loaded"), (dict(stages="lut3d2", lut2=False), "no second LUT is loaded"),
                        (dict(stages="lut1d", lut1d=False), "no 1D LUT is loaded"), (dict(stages="cdl"), "no CDL is given"),
                        (dict(stages="lut3d", cdl=True), "a CDL is given and the stage list has no 'cdl' stage"),
                        (dict(stages="cdl,lut3d", cdl=True, prelut=True), "directly behind 'cdl'"),
                        (dict(stages="lut3d", variant="vec_lds"), rf"variant vec_lds is not supported with {TAIL}"),
                        (dict(stages="lut3d:prism", variant="vec_global"), "variant vec_global cannot take stage 'lut3d:prism'")):
        with pytest.raises(ValueError, match=message):
            check_packed_stack_options(**{**names, **kw})
    with pytest.raises(ValueError, match="variant vec_global cannot take an 8-bit source"):
        check_packed_stack_options("yuv422p", "v210", stages="lut3d", variant="vec_global")
    with pytest.raises(ValueError, match="needs pix_fmt"):
        check_packed_stack_options(None, "v210", stages="lut3d")


# ------------------------------------------------------------------ the old names still refuse these sides
def test_the_old_names_still_refuse_these_sides():
    for name in ("uyvy422", "y210le", "v210"):
        with pytest.raises(ValueError):
            check_stack_options(name, None, stages="lut3d")
        with pytest.raises(ValueError):
            check_stack_options("yuv422p10le", name, stages="lut3d")
    for name, message in (("uyvy422", "a packed 4:2:2 side"), ("y210le", "a packed 4:2:2 side"), ("v210", "a v210 side")):
        with pytest.raises(ValueError, match=rf"{message} .* is not supported with a stage stack on semi-planar frames"):
            check_semi_stack_options("nv12", name, stages="lut3d")
        with pytest.raises(ValueError, match=rf"{message} .* is not supported with a stage stack on semi-planar frames"):
            check_semi_stack_options(name, "nv16", stages="lut3d")
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False, _variant_name="auto")
    for name, src in (("uyvy422", _uyvy()), ("v210", _v210())):
        with pytest.raises(ValueError):
            LutEngine.apply_yuv_stack(held, [src], pix_fmt=name, stages="lut3d")
        with pytest.raises(ValueError, match="is not supported with a stage stack on semi-planar frames"):
            LutEngine.apply_yuv_stack_semi(held, [src], pix_fmt=name, stages="lut3d")
    assert not hasattr(held, "_lib")


# ------------------------------------------------------------------ every layer refuses the same rows before an engine is touched
def _uyvy(w=16, h=8):
    import torch
    return torch.from_numpy(packedyuv.to_packed(frames.natural_yuv(w, h, 8, 1, 0), "uyvy422"))


def _v210(w=12, h=4):
    import torch
    return torch.from_numpy(v210.to_v210(frames.natural_yuv(w, h, 10, 1, 0), w).view("int32"))


ROWS = [(kw, m) for kw, m in OPTIONS if "matte" not in kw] + [
    (dict(out_pix_fmt="yuva422p10le"), "carry no alpha"), (dict(out_pix_fmt="nv16"), "a semi-planar side"),
    (dict(out_pix_fmt="rgb48le"), "an RGB side"), (dict(out_pix_fmt="gbrpf32le"), "a float side"),
    (dict(out_pix_fmt="uyvy422"), "a packed 4:2:2 side together with a v210 side"),
    (dict(pix_fmt="yuv422p10le", out_pix_fmt="yuv422p10le"), "both sides are planar: use apply_yuv_stack"),
    (dict(pix_fmt="yuv420p10le", out_pix_fmt="v210"), "takes a 4:2:2 source"),
    (dict(stages="lut1d,matrix,lut3d"), "stage 'matrix' is not supported"), (dict(stages=""), "empty"), (dict(stages="cdl,cdl"), "twice"),
    (dict(stages="lut3d"), "no 'cdl' stage"), (dict(cdl=None), "no CDL is given")]


def test_the_engine_refuses_before_it_is_touched():
    src = _v210()
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False, _variant_name="auto")
    full = dict(pix_fmt="v210", out_pix_fmt="yuv422p10le", stages="lut1d,cdl,lut3d,lut3d2", cdl=Cdl(), width=12)
    for kw, message in ROWS + [(dict(matte=src), r"a matte \(matte\)")]:
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_yuv_stack_packed(held, src, **{**full, **kw})
    for name, message in (("n", "no 3D LUT is loaded"), ("n2", "no second LUT is loaded"), ("n1d", "no 1D LUT is loaded")):
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_yuv_stack_packed(SimpleNamespace(**{**vars(held), name: 0}), src, **full)
    with pytest.raises(ValueError, match="variant vec_lds is not supported"):
        LutEngine.apply_yuv_stack_packed(SimpleNamespace(**{**vars(held), "_variant_name": "vec_lds"}), src, **full)
    with pytest.raises(TypeError, match="cdl must be a lut_renderer_amd.cdl.Cdl"):
        LutEngine.apply_yuv_stack_packed(held, src, **{**full, "cdl": "shot.cc"})
    with pytest.raises(TypeError, match="unexpected keyword argument 'interp'"):
        LutEngine.apply_yuv_stack_packed(held, src, **full, interp="trilinear")
    # the shapes `apply_yuv` takes for these containers, checked before the library is reached
    short = dict(pix_fmt="v210", stages="lut3d")
    with pytest.raises(ValueError, match="width is required with v210 frames"):
        LutEngine.apply_yuv_stack_packed(held, src, **short)
    with pytest.raises(ValueError, match="rows hold whole groups of four samples"):
        LutEngine.apply_yuv_stack_packed(held, _uyvy()[..., :30], pix_fmt="uyvy422", stages="lut3d")
    with pytest.raises(ValueError, match="the stack pass cannot run in place"):
        LutEngine.apply_yuv_stack_packed(held, src, src, **short, width=12)
    assert not hasattr(held, "_lib")                                  # nothing reached the library


def test_the_group_checks_the_same_things_first():
    from lut_renderer_amd.multigpu import LutEngineGroup
    e0 = SimpleNamespace(n=33, n2=9, _has_prelut=False, _variant_name="auto")
    g = SimpleNamespace(_lock=threading.RLock(), n1d=17, engines=[e0])
    full = dict(pix_fmt="v210", out_pix_fmt="yuv422p10le", stages="lut1d,cdl,lut3d,lut3d2", cdl=Cdl(), width=12)
    for kw, message in ROWS + [(dict(row0=0), "the group owns the row partition")]:
        with pytest.raises(ValueError, match=message):
            LutEngineGroup.apply_yuv_stack_packed(g, _v210(), **{**full, **kw})


def _lut(n=2):
    import numpy as np
    return cube.CubeLut(n, np.ones(3, np.float32), cube.identity_lattice(n).astype(np.float32))


def test_apply_lut_refuses_while_planning():
    from lut_renderer_amd.api import apply_lut
    src = _v210()
    eng = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False, _variant_name="auto")
    base = dict(cube=None, pix_fmt="v210", out_pix_fmt="yuv422p10le", width=12, engine=eng, packed_stages="lut1d,lut3d")
    tail = "is not supported with a stage stack on packed 4:2:2 / v210 frames"
    for kw, message in ((dict(zscale_dither="error_diffusion"), rf"dither \('error_diffusion'\) {tail}"),
                        (dict(engine_dither="blue_noise"), rf"dither \('blue_noise'\) {tail}"),
                        (dict(resolution="8x4"), rf"resize .* {tail}"),
                        (dict(second_pix_fmt="yuv420p"), rf"two-output pass .* {tail}"),
                        (dict(strength=0.5), rf"a LUT strength \(strength\) {tail}"),
                        (dict(matte=src), rf"a matte \(matte\) {tail}"),
                        (dict(chroma_loc="left"), rf"chroma_loc\) {tail}"),
                        (dict(alpha_mode="premultiplied"), rf"alpha_mode='premultiplied' {tail}"),
                        (dict(out_pix_fmt="yuva422p10le"), "carry no alpha"),
                        (dict(out_pix_fmt="p210le"), rf"a semi-planar side .* {tail}"),
                        (dict(out_pix_fmt="y210le"), "a packed 4:2:2 side together with a v210 side"),
                        (dict(packed_stages="lut1d,matrix,lut3d"), "stage 'matrix' is not supported"),
                        (dict(stages="lut3d"), "packed_stages and stages / rgb_stages / rgb_out_stages / semi_stages are mutually exclusive"),
                        (dict(rgb_stages="lut3d"), "mutually exclusive"), (dict(semi_stages="lut3d"), "mutually exclusive"),
                        (dict(rgb_out="rgb48le", rgb_out_stages="lut3d"), "mutually exclusive"),
                        (dict(packed_stages="lut1d,lut3d,cdl"), "stage 'cdl' is listed and no CDL is given"),
                        (dict(cube2=_lut()), "cube2 is given and the stage list has no 'lut3d2' stage")):
        with pytest.raises(ValueError, match=message):
            apply_lut(src, **{**base, **kw})
    with pytest.raises(ValueError, match="both sides are planar: use apply_yuv_stack"):
        apply_lut(frames.natural_yuv(16, 8, 10, 1, 0), **{**base, "pix_fmt": "yuv422p10le", "width": None})
    assert not hasattr(eng, "_lock")                                  # the engine's lock was never taken


# ------------------------------------------------------------------ routing against a fake engine
class FakeEngine:
    """What `apply_lut` and `HostPipeline` ask of an engine, recording the one call that reaches it."""
    n, n2, n1d, _has_prelut, _variant_name, precision = 33, 9, 17, False, "auto", "strict"
    _applied_lut = _applied_lut2 = _applied_lut1d = None

    def __init__(self):
        self._lock = threading.RLock()
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("apply_"):
            raise AttributeError(name)

        def entry(src, dst=None, **kw):
            self.calls.append((name, kw))
            return dst
        return entry


def test_apply_lut_routes_to_the_new_entry():
    from lut_renderer_amd.api import apply_lut
    eng = FakeEngine()
    grade = Cdl(saturation=0.5)
    apply_lut(_v210(), cube=None, pix_fmt="v210", out_pix_fmt="yuv422p10le", width=12, engine=eng, cdl=grade,
              packed_stages="lut1d,cdl,lut3d", interp="trilinear")
    (name, kw), = eng.calls
    assert name == "apply_yuv_stack_packed"
    assert (kw["pix_fmt"], kw["out_pix_fmt"], kw["width"]) == ("v210", "yuv422p10le", 12)
    assert kw["stages"] == (("lut1d", None), ("cdl", None), ("lut3d", "trilinear")) and kw["cdl"] == grade
    assert kw["lut_depth"] == 10 and not {"interp", "dither", "alpha_mode", "rgb_matrix"} & set(kw)
    eng = FakeEngine()                                                 # a packed side tells its own width; the output keeps the name
    apply_lut(_uyvy(), cube=None, pix_fmt="uyvy422", engine=eng, packed_stages="lut3d")
    (name, kw), = eng.calls
    assert name == "apply_yuv_stack_packed" and (kw["pix_fmt"], kw["out_pix_fmt"]) == ("uyvy422", "uyvy422") and "width" not in kw
    eng = FakeEngine()                                                 # the full-range prologue lands at 8 bit, as for planar frames
    apply_lut(_uyvy(), cube=None, pix_fmt="uyvy422", color_range="pc", engine=eng, packed_stages="lut3d")
    (name, kw), = eng.calls
    assert name == "apply_yuv_stack_packed" and kw["range_src"] == "pc" and kw["lut_depth"] == 8 and kw["out_pix_fmt"] == "yuv422p"
    eng = FakeEngine()                                                 # without the flag the call is what it was
    apply_lut(_uyvy(), cube=None, pix_fmt="uyvy422", engine=eng)
    assert [n for n, _ in eng.calls] == ["apply_yuv"]


def test_the_host_pipeline_routes_and_refuses(monkeypatch):
    from lut_renderer_amd.stream import HostPipeline
    monkeypatch.setattr(HostPipeline, "_allocate", lambda self, engine, slots: None)
    eng = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False)
    grade = Cdl()
    pipe = HostPipeline(eng, "v210", 48, 4, out_pix_fmt="yuv422p10le", packed_stages="lut1d,cdl,lut3d", cdl=grade, lut_depth=10)
    assert pipe.entry == "apply_yuv_stack_packed" and pipe.packed_stack and not pipe.semi_stack and not pipe.rgb_stack
    assert pipe.kw == dict(cdl=grade, lut_depth=10, stages=(("lut1d", None), ("cdl", None), ("lut3d", "tetrahedral")), pix_fmt="v210",
                           out_pix_fmt="yuv422p10le", width=48)
    assert (pipe.fin.fmt.name, pipe.fout.fmt.name) == ("v210", "yuv422p10le")
    pipe = HostPipeline(eng, "yuv422p", 33, 5, out_pix_fmt="yuyv422", packed_stages="lut3d")
    assert pipe.entry == "apply_yuv_stack_packed" and pipe.kw["width"] == 33 and pipe.fout.fmt.name == "yuyv422"
    assert HostPipeline(eng, "uyvy422", 16, 8).entry == "apply_yuv"  # without the flag the route is what it was
    full = dict(out_pix_fmt="yuv422p10le", packed_stages="lut1d,cdl,lut3d,lut3d2", cdl=Cdl())
    for kw, message in [(k, m) for k, m in ROWS if "stages" not in k and "pix_fmt" not in k or "out_pix_fmt" in k and "pix_fmt" not in k]:
        kw = dict(kw)
        extra = dict(second_pix_fmt=kw.pop("out2_pix_fmt")) if "out2_pix_fmt" in kw else {}
        with pytest.raises(ValueError, match=message):
            HostPipeline(eng, "v210", 48, 4, **{**full, **kw, **extra})
    for kw, message in ((dict(packed_stages="lut1d,matrix,lut3d"), "stage 'matrix' is not supported"),
                        (dict(stages="lut3d"), "mutually exclusive"), (dict(rgb_stages="lut3d"), "mutually exclusive"),
                        (dict(semi_stages="lut3d"), "mutually exclusive"),
                        (dict(rgb_out="rgb48le"), "with packed_stages the output is out_pix_fmt"),
                        (dict(strength_keys="0:1"), r"strength_keys\) is not supported with a stage stack on packed 4:2:2 / v210 frames"),
                        (dict(chain=True), "chain / lut1d are not set with packed_stages")):
        with pytest.raises(ValueError, match=message):
            HostPipeline(eng, "v210", 48, 4, **{**full, **kw})
    with pytest.raises(ValueError, match="mutually exclusive"):
        HostPipeline(eng, "yuv422p10le", 16, 8, rgb_out="rgb48le", rgb_out_stages="lut3d", packed_stages="lut3d")
    with pytest.raises(ValueError, match="both sides are planar"):
        HostPipeline(eng, "yuv422p10le", 16, 8, out_pix_fmt="yuv420p10le", packed_stages="lut3d")


# ------------------------------------------------------------------ the CLI flag and the argv builder
def _args(*extra, pix_fmt="v210", out="yuv422p10le", size="48x4"):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", size, "--pix-fmt", pix_fmt, "--out-pix-fmt", out, *extra])


def test_cli_flag(cube_dir):
    from lut_renderer_amd.cli import plan_from_args
    a, b, t = str(cube_dir / "log709_33.cube"), str(cube_dir / "random_9.cube"), str(GOLDEN / "lut1d" / "curve17.cube")
    assert _args("--cube", a).packed_stages is None
    _, kw, w, h = plan_from_args(_args("--cube", a, "--cube2", b, "--lut1d", t, "--cdl-sat", "0.5", "--interp", "trilinear", "--interp2", "nearest",
                                       "--packed-stages", "lut1d,cdl,lut3d,lut3d2"))
    assert (w, h) == (48, 4) and (kw["pix_fmt"], kw["out_pix_fmt"]) == ("v210", "yuv422p10le")
    assert kw["packed_stages"] == (("lut1d", None), ("cdl", None), ("lut3d", "trilinear"), ("lut3d2", "nearest")) and kw["cdl"] == Cdl(saturation=0.5)
    assert not {"interp", "dither", "alpha_mode", "stages", "semi_stages"} & set(kw)
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--packed-stages", "lut3d", pix_fmt="yuv422p", out="uyvy422"))
    assert kw["packed_stages"] == (("lut3d", "tetrahedral"),) and kw["out_pix_fmt"] == "uyvy422"
    tail = "is not supported with a stage stack on packed 4:2:2 / v210 frames"
    full = ("--cube", a, "--lut1d", t, "--packed-stages", "lut1d,lut3d")
    for extra, message in ((("--zscale-dither", "error_diffusion"), rf"dither \('error_diffusion'\) {tail}"),
                           (("--engine-dither", "blue_noise"), rf"dither \('blue_noise'\) {tail}"),
                           (("--out-size", "8x4"), rf"resize .* {tail}"),
                           (("--chroma-loc", "left"), rf"chroma_loc.* {tail}"),
                           (("--strength", "0.5"), rf"a LUT strength \(strength\) {tail}"),
                           (("--matte", "m.gray"), rf"a matte \(matte\) {tail}"),
                           (("--alpha-mode", "premultiplied"), rf"alpha_mode='premultiplied' {tail}"),
                           (("--second-output", "c.yuv", "--second-pix-fmt", "yuv420p"), rf"two-output pass .* {tail}"),
                           (("--stages", "lut1d,lut3d"), "mutually exclusive"), (("--rgb-stages", "lut1d,lut3d"), "mutually exclusive"),
                           (("--semi-stages", "lut1d,lut3d"), "mutually exclusive"),
                           (("--rgb-out", "rgb48le", "--rgb-out-stages", "lut3d"), "mutually exclusive"),
                           (("--rgb-out", "rgb48le"), "with --packed-stages the output is --out-pix-fmt"),
                           (("--cdl-sat", "0.5"), "--cdl-sat is given and --packed-stages has no 'cdl' stage")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args(*full, *extra))
    with pytest.raises(ValueError, match="both sides are planar: use apply_yuv_stack"):
        plan_from_args(_args(*full, pix_fmt="yuv422p10le"))
    with pytest.raises(ValueError, match="a packed 4:2:2 side together with a v210 side"):
        plan_from_args(_args(*full, out="uyvy422"))
    with pytest.raises(ValueError, match="stage 'matrix' is not supported"):
        plan_from_args(_args("--cube", a, "--rgb-matrix", "1 0 0 0 1 0 0 0 1", "--packed-stages", "matrix,lut3d"))


def test_engine_command_round_trips_the_flag(cube_dir):
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    info = VideoInfo(width=48, height=4, bit_depth=10, pix_fmt="v210", color_range="tv", colorspace="bt709", fps=25.0)
    params = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")
    a, b, t = cube_dir / "log709_33.cube", cube_dir / "random_9.cube", GOLDEN / "lut1d" / "curve17.cube"
    io = (Path("-"), Path("-"), params, a, info)
    plain = engine_command(*io)
    assert "--packed-stages" not in plain and engine_command(*io, packed_stages=None) == plain   # byte for byte what it was
    assert engine_command(*io, packed_stages="lut3d") == plain + ["--packed-stages", "lut3d:tetrahedral"]
    grade = Cdl(slope=(1.1, 1.0, 0.9), saturation=0.6)
    cmd = engine_command(*io, cube2=b, interp2="nearest", cdl=grade, lut1d=t, interp1d="cubic", packed_stages=["lut1d", "cdl", "lut3d", "lut3d2"])
    assert cmd == plain + ["--cube2", str(b), "--interp2", "nearest", "--cdl-sop", grade.sop_text(), "--cdl-sat", repr(0.6), "--lut1d", str(t),
                           "--interp1d", "cubic", "--packed-stages", "lut1d,cdl,lut3d:tetrahedral,lut3d2:nearest"]
    args = build_parser().parse_args(cmd[3:])
    _, kw, _, _ = plan_from_args(args)
    assert kw["packed_stages"] == (("lut1d", None), ("cdl", None), ("lut3d", "tetrahedral"), ("lut3d2", "nearest")) and kw["cdl"] == grade
    assert (kw["pix_fmt"], kw["out_pix_fmt"]) == ("v210", "yuv422p10le")
    tail = "is not supported with a stage stack on packed 4:2:2 / v210 frames"
    for kw, message in ((dict(packed_stages="lut1d"), "the LUT is given and the stage list has no 'lut3d' stage"),
                        (dict(packed_stages="lut3d", stages="lut3d"), "mutually exclusive"),
                        (dict(packed_stages="lut3d", rgb_stages="lut3d"), "mutually exclusive"),
                        (dict(packed_stages="lut3d", semi_stages="lut3d"), "mutually exclusive"),
                        (dict(packed_stages="lut3d", engine_dither="blue_noise"), rf"dither \('blue_noise'\) {tail}"),
                        (dict(packed_stages="lut3d", chroma_loc="left"), rf"chroma_loc.* {tail}"),
                        (dict(packed_stages="lut3d", strength=0.5), rf"strength\) {tail}"),
                        (dict(packed_stages="matrix,lut3d"), "stage 'matrix' is not supported")):
        with pytest.raises(ValueError, match=message):
            engine_command(*io, **kw)
    planar = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv422p10le", color_range="tv", colorspace="bt709", fps=25.0)
    with pytest.raises(ValueError, match="both sides are planar: use apply_yuv_stack"):
        engine_command(Path("-"), Path("-"), params, a, planar, packed_stages="lut3d")


def test_the_stage_pipeline_has_no_such_flag():
    """`pipe.py`'s argv is not covered: its parser refuses the flag by name."""
    from lut_renderer_amd import pipe
    with pytest.raises(SystemExit):
        pipe.main(["--packed-stages", "lut3d"])
