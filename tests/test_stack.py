"""The stage stack without a GPU: the twin's anchors to the four existing contracts, the rounding rule by known
answers, the identity CDL over every code, a stack no dedicated pass serves against its composition written out, the one parser
of a stage list, the one copy of the refusals through every layer, what stays refused without `stages`, and the argv."""
import threading
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.cdl import Cdl, read_cdl
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.formats import check_stack_options, parse_stages, stages_string
from tests import _cdl_twin as cdlt
from tests import _chain_twin as cht
from tests import _lut1d_twin as l1t
from tests import _stack_twin as twin
from tests import _xsub_twin as xs

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
F = np.float32
#: (din, dl, dout): the 8 / 10 / 16-bit depth mixes of the anchors
DEPTH_MIXES = ((8, 8, 8), (10, 10, 10), (16, 16, 8), (8, 8, 10))
PAIRS = (("420", "422"), ("444", "420"))


def _eq(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _luts():
    rng = np.random.default_rng(11)
    a = cube.CubeLut(9, np.ones(3, F), rng.uniform(-0.2, 1.2, (9, 9, 9, 3)).astype(F))
    b = cube.CubeLut(5, np.array([1.0, 0.5, 1.0], F), rng.uniform(0.0, 1.0, (5, 5, 5, 3)).astype(F))
    return a, b


def _cases():
    for a, b in PAIRS:
        for din, dl, dout in DEPTH_MIXES:
            (icsx, icsy), (ocsx, ocsy) = twin.LAYOUTS[a], twin.LAYOUTS[b]
            src = frames.natural_yuv(37, 13, din, icsx, icsy, k=2)
            k = twin.consts("bt709", "tv", "bt709", "tv", din, dl, dout, ocsx, ocsy)
            yield (a, b, din, dl, dout), k, dl, dout, icsx, icsy, ocsx, ocsy, src


# ------------------------------------------------------------------ the twin's anchors
def test_a_lut3d_stack_is_the_xsub_twin(orc):
    A, _ = _luts()
    for tag, k, dl, dout, icsx, icsy, ocsx, ocsy, src in _cases():
        for mode in ("tetrahedral", "prism"):
            got = twin.apply([("lut3d", mode)], k, dl, dout, icsx, icsy, ocsx, ocsy, src, lut=A)
            assert _eq(got, xs.apply(A.table, A.scale, mode, k, dl, dout, icsx, icsy, ocsx, ocsy, src)), (tag, mode)


def test_a_cdl_lut3d_stack_is_the_cdl_twin(orc):
    A, _ = _luts()
    grade = read_cdl(GOLDEN / "cdl" / "shot.cc")
    for tag, k, dl, dout, icsx, icsy, ocsx, ocsy, src in _cases():
        for c in (grade, Cdl(slope=grade.slope, offset=grade.offset, power=grade.power, saturation=1.0)):
            got = twin.apply(["cdl", ("lut3d", "trilinear")], k, dl, dout, icsx, icsy, ocsx, ocsy, src, lut=A, cdl=c)
            assert _eq(got, cdlt.apply(A, c, "trilinear", k, dl, dout, icsx, icsy, ocsx, ocsy, src)), tag


def test_the_lut1d_stacks_are_the_lut1d_twin(orc):
    A, _ = _luts()
    l1 = cube.read_lut1d(GOLDEN / "lut1d" / "curve17.cube")
    for tag, k, dl, dout, icsx, icsy, ocsx, ocsy, src in _cases():
        tab = l1t.table(l1.table, l1.scale, "linear", dl)
        got = twin.apply(["lut1d", "lut3d"], k, dl, dout, icsx, icsy, ocsx, ocsy, src, lut=A, l1d_tab=tab)
        assert _eq(got, l1t.apply(tab, A, "tetrahedral", k, dl, dout, icsx, icsy, ocsx, ocsy, src)), tag
        got = twin.apply(["lut1d"], k, dl, dout, icsx, icsy, ocsx, ocsy, src, l1d_tab=tab)
        assert _eq(got, l1t.apply(tab, None, None, k, dl, dout, icsx, icsy, ocsx, ocsy, src)), tag


def test_a_lut3d_lut3d2_stack_is_the_chain_twin(orc):
    A, B = _luts()
    for tag, k, dl, dout, icsx, icsy, ocsx, ocsy, src in _cases():
        got = twin.apply([("lut3d", "tetrahedral"), ("lut3d2", "nearest")], k, dl, dout, icsx, icsy, ocsx, ocsy, src, lut=A, lut2=B)
        assert _eq(got, cht.apply(A, B, "tetrahedral", "nearest", k, dl, dout, icsx, icsy, ocsx, ocsy, src)), tag


# ------------------------------------------------------------------ the rounding rule
def test_the_rounding_rule_by_known_answers():
    for dl in (8, 10, 12, 16):
        m = (1 << dl) - 1
        one = lambda v: int(twin.round_codes((np.array([v], F),) * 3, dl)[0][0])      # noqa: E731
        assert one(0.0) == 0 and one(1.0) == m
        # 0.5 / M: the product is 0.5 or one ulp beside it, and 0.5 + 0.5 rounds to 1 or stays just below
        half = F(0.5) / F(m)
        assert one(half) == int(F(F(half * F(m)) + F(0.5)))
        assert one(half) in (0, 1)
        for k in (0, 1, m // 2, m - 1):
            # the float just below (k + 0.5) / M: its product with M is below k + 0.5 (or rounds onto it), never above it
            edge = np.nextafter(F((k + 0.5) / m), F(0))
            want = int(F(F(edge * F(m)) + F(0.5)))                  # the two roundings written out by hand
            assert one(edge) == want and want in (k, k + 1)
            assert one(F(k) / F(m)) == k                            # a code's own unit value comes back
    # hand-computed at 8 bit: 0.3 * 255 = 76.5 (fl: 76.50001), + 0.5 -> 77
    assert int(twin.round_codes((np.array([0.3], F),) * 3, 8)[0][0]) == 77
    assert int(twin.round_codes((np.array([0.298], F),) * 3, 8)[0][0]) == 76      # 75.99 + 0.5 = 76.49


@pytest.mark.parametrize("dl", [8, 10, 12, 16])
def test_the_identity_cdl_returns_every_code(dl):
    """(int)(fl(fl(k * fl(1 / M)) * M) + 0.5f) == k for every k: what makes [cdl] with the identity CDL the two conversion stages
    alone.  Checked on the twin's table and on the product's own."""
    m = (1 << dl) - 1
    codes = np.arange(m + 1)
    for tab in (cdlt.table(Cdl(), dl), _native.cdl_table(Cdl(), dl)):
        assert np.array_equal(tab[0], (np.arange(m + 1, dtype=F) * (F(1.0) / F(m))).astype(F))
        back = twin.round_codes((tab[0], tab[1], tab[2]), dl)
        assert all(np.array_equal(b, codes) for b in back), dl


def test_a_cdl_stack_with_the_identity_cdl_is_stages_1_and_3(orc):
    from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
    for tag, k, dl, dout, icsx, icsy, ocsx, ocsy, src in _cases():
        got = twin.apply(["cdl"], k, dl, dout, icsx, icsy, ocsx, ocsy, src, cdl=Cdl())
        assert _eq(got, rgb_codes_to_yuv(k, dout, ocsx, ocsy, yuv_to_rgb_codes(k, icsx, icsy, src))), tag


# ------------------------------------------------------------------ stacks no dedicated pass serves
def test_lut3d_then_lut1d_is_the_composition_written_out(orc):
    from oracle import binding as orcb
    from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
    A, _ = _luts()
    l1 = cube.read_lut1d(GOLDEN / "lut1d" / "gamma1024.cube")
    for tag, k, dl, dout, icsx, icsy, ocsx, ocsy, src in _cases():
        tab = l1t.table(l1.table, l1.scale, "cubic", dl)
        r, g, b = yuv_to_rgb_codes(k, icsx, icsy, src)
        dt = np.uint8 if dl <= 8 else np.uint16
        go, bo, ro = orcb.apply_rgb(A.table, A.scale, dl, "tetrahedral", (g.astype(dt), b.astype(dt), r.astype(dt)))
        want = rgb_codes_to_yuv(k, dout, ocsx, ocsy, (tab[0][ro].astype(np.int64), tab[1][go].astype(np.int64), tab[2][bo].astype(np.int64)))
        assert _eq(twin.apply(["lut3d", "lut1d"], k, dl, dout, icsx, icsy, ocsx, ocsy, src, lut=A, l1d_tab=tab), want), tag


def test_cdl_then_lut1d_rounds_in_between(orc):
    from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
    grade = read_cdl(GOLDEN / "cdl" / "shot.cc")
    l1 = cube.read_lut1d(GOLDEN / "lut1d" / "invert33.cube")
    (icsx, icsy), (ocsx, ocsy) = twin.LAYOUTS["420"], twin.LAYOUTS["422"]
    src = frames.natural_yuv(37, 13, 10, icsx, icsy, k=2)
    k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, ocsx, ocsy)
    tab, ct = l1t.table(l1.table, l1.scale, "linear", 10), cdlt.table(grade, 10)
    r, g, b = yuv_to_rgb_codes(k, icsx, icsy, src)
    o = cdlt.saturate(grade.saturation, [ct[0][r], ct[1][g], ct[2][b]])
    q = [((v * F(1023)).astype(F) + F(0.5)).astype(F).astype(np.int64) for v in o]
    want = rgb_codes_to_yuv(k, 10, ocsx, ocsy, (tab[0][q[0]].astype(np.int64), tab[1][q[1]].astype(np.int64), tab[2][q[2]].astype(np.int64)))
    assert _eq(twin.apply(["cdl", "lut1d"], k, 10, 10, icsx, icsy, ocsx, ocsy, src, cdl=grade, l1d_tab=tab), want)


# ------------------------------------------------------------------ the parser
def test_parse_stages():
    assert parse_stages("lut1d,cdl,lut3d:trilinear") == (("lut1d", None), ("cdl", None), ("lut3d", "trilinear"))
    assert parse_stages(["lut3d", ("lut3d2", "nearest")]) == (("lut3d", "tetrahedral"), ("lut3d2", "nearest"))
    assert parse_stages(" lut3d , lut3d2 ", interp="prism") == (("lut3d", "prism"), ("lut3d2", "prism"))
    assert parse_stages("lut3d,lut3d2", interp="prism", interp2="pyramid") == (("lut3d", "prism"), ("lut3d2", "pyramid"))
    assert parse_stages("lut3d:nearest", interp="prism") == (("lut3d", "nearest"),)
    st = parse_stages(("cdl", "lut1d", "lut3d", "lut3d2"))
    assert parse_stages(st) == st and parse_stages(stages_string(st)) == st
    assert stages_string("lut1d,lut3d") == "lut1d,lut3d:tetrahedral"
    for bad, message in (("", "the stage list is empty"), ([], "the stage list is empty"), (None, "the stage list is empty"),
                         ("lut3d,lut3d2,lut1d,cdl,lut3d", "has 5 stages"), ("lut3d,gamma", "unknown stage kind 'gamma'"),
                         ("lut3d,cdl,lut3d", "stage kind 'lut3d' is listed twice"), ("cdl:linear", "stage 'cdl' takes no mode"),
                         ("lut1d:cubic", "stage 'lut1d' takes no mode"), ("lut3d:cubic", "lut3d has no interpolation mode 'cubic'"),
                         ("lut3d:", "names no mode"), ([("lut3d", "tetrahedral", 3)], "a stage is a name or a"),
                         ([3], "a stage is a name or a")):
        with pytest.raises(ValueError, match=message):
            parse_stages(bad)
    header = (ROOT / "include" / "lutr.h").read_text()
    for name, code in (("LUT3D", 1), ("LUT3D_2", 2), ("LUT1D", 3), ("CDL", 4)):
        assert f"LUTR_STAGE_{name}" in header
    assert _native.STAGE_KINDS == {"lut3d": 1, "lut3d2": 2, "lut1d": 3, "cdl": 4}
    assert "lutr_apply_yuv_stack" in _native.SYMBOLS and hasattr(_native.load(), "lutr_apply_yuv_stack")
    arr = _native.stage_array(parse_stages("lut1d,lut3d2:prism"))
    assert [(s.kind, s.interp) for s in arr] == [(3, 0), (2, 4)]


# ------------------------------------------------------------------ one copy of the refusals
NAMES = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
FULL = dict(stages="lut1d,cdl,lut3d,lut3d2", cdl=True)
REFUSALS = [(dict(stages=""), "the stage list is empty"),
            (dict(stages="lut3d,lut3d"), "listed twice"),
            (dict(stages="lut3d", lut=False), "stage 'lut3d' is listed and no 3D LUT is loaded"),
            (dict(stages="lut3d2", lut2=False), "stage 'lut3d2' is listed and no second LUT is loaded"),
            (dict(stages="lut1d", lut1d=False), "stage 'lut1d' is listed and no 1D LUT is loaded"),
            (dict(stages="cdl,lut3d", cdl=False), "stage 'cdl' is listed and no CDL is given"),
            (dict(stages="lut3d", cdl=True), "a CDL is given and the stage list has no 'cdl' stage"),
            (dict(stages="cdl,lut3d", cdl=True, prelut=True), "'lut3d' directly behind 'cdl' is not supported with a LUT that carries a .csp prelut"),
            (dict(FULL, dither="error_diffusion"), r"dither \('error_diffusion'\) is not supported with a stage stack"),
            (dict(FULL, dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a stage stack"),
            (dict(FULL, chroma_loc="left"), r"chroma_loc\) is not supported with a stage stack"),
            (dict(FULL, out_size=(8, 4)), r"resize \(out_size / resolution\) is not supported with a stage stack"),
            (dict(FULL, out2_pix_fmt="yuv420p"), r"two-output pass \(out2_pix_fmt\) is not supported with a stage stack"),
            (dict(FULL, alpha_mode="premultiplied"), "alpha_mode='premultiplied' is not supported with a stage stack"),
            (dict(FULL, variant="vec_lds"), "variant vec_lds is not supported with a stage stack")]
SIDES = [("nv12", "a semi-planar container"), ("p010le", "a semi-planar container"), ("uyvy422", "a packed container"),
         ("y210le", "a packed container"), ("v210", "a v210 container"), ("gbrp10le", "an RGB format"), ("rgb24", "an RGB format"),
         ("gbrpf32le", "a float RGB format")]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_check_stack_options_refuses(kw, message):
    with pytest.raises(ValueError, match=message):
        check_stack_options(**NAMES, **kw)


@pytest.mark.parametrize("name,word", SIDES)
def test_a_side_that_is_not_planar_yuv_is_a_value_error(name, word):
    with pytest.raises(ValueError, match=f"the stack pass takes planar YUV on both sides: out_pix_fmt '{name}' is {word}"):
        check_stack_options("yuv422p10le", name, **FULL)
    with pytest.raises(ValueError, match=f"pix_fmt '{name}' is {word}"):
        check_stack_options(name, None, **FULL)


def test_what_check_stack_options_takes():
    st, fin, fout = check_stack_options(**NAMES, **FULL)
    assert [k for k, _ in st] == ["lut1d", "cdl", "lut3d", "lut3d2"] and (fin.name, fout.name) == ("yuv420p10le", "yuv422p10le")
    _, fin, fout = check_stack_options("yuva444p10le", "yuva444p10le", stages="cdl", cdl=True)
    assert fin.alpha and fout.alpha                                 # straight alpha goes through the alpha tail
    # a prelut is fine wherever lut3d is fed codes
    check_stack_options(**NAMES, stages="lut3d,cdl,lut3d2", cdl=True, prelut=True)
    check_stack_options(**NAMES, stages="cdl,lut1d,lut3d", cdl=True, prelut=True)
    check_stack_options(**NAMES, stages="cdl,lut3d2,lut3d", cdl=True, prelut=True)
    for variant in (None, "auto", "generic", "vec_global"):
        check_stack_options(**NAMES, **FULL, variant=variant)


def _planes(depth, csx, csy, alpha=False):
    import torch
    y = frames.natural_yuv(16, 8, depth, csx, csy)
    return [torch.from_numpy(p.view(np.int16)) for p in (list(y) + ([y[0]] if alpha else []))]


def test_the_engine_refuses_before_it_is_touched():
    src = _planes(10, 1, 1)
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False)
    full = dict(NAMES, stages="lut1d,cdl,lut3d,lut3d2", cdl=Cdl())
    for kw, message in ((dict(dither="blue_noise"), "dither"), (dict(chroma_loc="left"), "chroma_loc"), (dict(out_size=(8, 4)), "resize"),
                        (dict(out2_pix_fmt="yuv420p"), "two-output"), (dict(alpha_mode="premultiplied"), "alpha_mode"),
                        (dict(out_pix_fmt="nv12"), "semi-planar"), (dict(out_pix_fmt="v210"), "v210"),
                        (dict(out_pix_fmt="uyvy422"), "packed"), (dict(pix_fmt="gbrp10le"), "RGB"),
                        (dict(stages=""), "empty"), (dict(stages="cdl,cdl"), "twice"), (dict(stages="lut3d"), "no 'cdl' stage"),
                        (dict(cdl=None), "no CDL is given")):
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_yuv_stack(held, src, **{**full, **kw})
    for name, message in (("n", "no 3D LUT is loaded"), ("n2", "no second LUT is loaded"), ("n1d", "no 1D LUT is loaded")):
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_yuv_stack(SimpleNamespace(**{**vars(held), name: 0}), src, **full)
    with pytest.raises(ValueError, match="directly behind 'cdl'"):
        LutEngine.apply_yuv_stack(SimpleNamespace(n=33, _has_prelut=True), src, **NAMES, stages="cdl,lut3d", cdl=Cdl())
    with pytest.raises(TypeError, match="cdl must be a lut_renderer_amd.cdl.Cdl"):
        LutEngine.apply_yuv_stack(held, src, **{**full, "cdl": "shot.cc"})
    with pytest.raises(TypeError, match="unexpected keyword argument 'interp'"):
        LutEngine.apply_yuv_stack(held, src, **full, interp="trilinear")


def test_the_group_checks_the_same_things_first():
    from lut_renderer_amd.multigpu import LutEngineGroup
    e0 = SimpleNamespace(n=33, n2=0, _has_prelut=True)
    g = SimpleNamespace(_lock=threading.RLock(), n1d=17, engines=[e0])
    for kw, message in ((dict(stages="lut1d,lut3d", dither="blue_noise"), "dither .* is not supported with a stage stack"),
                        (dict(stages="lut3d,lut3d2"), "no second LUT is loaded"), (dict(stages="cdl,lut3d", cdl=Cdl()), "directly behind"),
                        (dict(stages="lut1d", out_pix_fmt="p010le"), "semi-planar"), (dict(stages="lut1d", row0=0), "the group owns the row partition")):
        with pytest.raises(ValueError, match=message):
            LutEngineGroup.apply_yuv_stack(g, _planes(10, 1, 1), **{**NAMES, **kw})


def _lut(n=2):
    return cube.CubeLut(n, np.ones(3, F), cube.identity_lattice(n).astype(F))


def test_apply_lut_refuses_while_planning():
    from lut_renderer_amd.api import apply_lut
    y = frames.natural_yuv(16, 8, 10, 1, 1)
    l1 = cube.Lut1D.identity(4)
    base = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", engine=SimpleNamespace(n=0, n2=0, n1d=0, _has_prelut=False))
    for kw, message in ((dict(cube=_lut(), stages="lut1d,lut3d"), "no 1D LUT is loaded"),
                        (dict(cube=None, stages="lut3d"), "no 3D LUT is loaded"),
                        (dict(cube=_lut(), stages="lut3d,lut3d2"), "no second LUT is loaded"),
                        (dict(cube=_lut(), stages="cdl,lut3d"), "no CDL is given"),
                        (dict(cube=_lut(), stages="lut1d"), "cube is given and the stage list has no 'lut3d' stage"),
                        (dict(cube=_lut(), cube2=_lut(), stages="lut3d"), "cube2 is given and the stage list has no 'lut3d2' stage"),
                        (dict(cube=_lut(), lut1d=l1, stages="lut3d"), "lut1d is given and the stage list has no 'lut1d' stage"),
                        (dict(cube=_lut(), cdl=Cdl(), stages="lut3d"), "cdl is given and the stage list has no 'cdl' stage"),
                        (dict(cube=_lut(), interp2="nearest", stages="lut3d"), "interp2 is the mode of the second LUT"),
                        (dict(cube=_lut(), cdl_id="a", stages="lut3d"), "cdl_id names a correction"),
                        (dict(cube=_lut(), lut1d=l1, interp1d="bicubic", stages="lut1d,lut3d"), "lut1d has no interpolation mode 'bicubic'"),
                        (dict(cube=_lut(), stages="lut3d,gamma"), "unknown stage kind 'gamma'"),
                        (dict(cube=_lut(), stages=""), "the stage list is empty"),
                        (dict(cube=_lut(), stages="lut3d", zscale_dither="error_diffusion"), r"dither \('error_diffusion'\) is not supported with a stage stack"),
                        (dict(cube=_lut(), stages="lut3d", engine_dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a stage stack"),
                        (dict(cube=_lut(), stages="lut3d", chroma_loc="left"), "chroma_loc.* is not supported with a stage stack"),
                        (dict(cube=_lut(), stages="lut3d", resolution="8x4"), "resize .* is not supported with a stage stack"),
                        (dict(cube=_lut(), stages="lut3d", second_pix_fmt="yuv420p"), "two-output pass .* is not supported with a stage stack")):
        with pytest.raises(ValueError, match=message):
            apply_lut(y, **base, **kw)
    ya = list(y) + [y[0]]
    with pytest.raises(ValueError, match="alpha_mode='premultiplied' is not supported with a stage stack"):
        apply_lut(ya, **{**base, "pix_fmt": "yuva420p10le", "out_pix_fmt": "yuva420p10le"}, cube=_lut(), stages="lut3d",
                  alpha_mode="premultiplied")
    for name, _ in SIDES[:5]:
        with pytest.raises(ValueError, match=name):
            apply_lut(y, **{**base, "out_pix_fmt": name}, cube=_lut(), stages="lut3d")


def test_without_stages_the_combinations_stay_refused(cube_dir):
    """No existing refusal is lifted: the messages are today's."""
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.cli import plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    y = frames.natural_yuv(16, 8, 10, 1, 1)
    base = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", engine=object())
    with pytest.raises(ValueError, match="a CDL is not supported with a 1D LUT"):
        apply_lut(y, cube=None, cdl=Cdl(), lut1d=cube.Lut1D.identity(4), **base)
    with pytest.raises(ValueError, match="two-LUT chain .* is not supported with a CDL"):
        apply_lut(y, cube=_lut(), cube2=_lut(), cdl=Cdl(), **base)
    with pytest.raises(ValueError, match="two-LUT chain .* is not supported with a 1D LUT"):
        apply_lut(y, cube=_lut(), cube2=_lut(), lut1d=cube.Lut1D.identity(4), **base)
    a, t = str(cube_dir / "log709_33.cube"), str(GOLDEN / "lut1d" / "curve17.cube")
    with pytest.raises(ValueError, match="two-LUT chain .* is not supported with a CDL"):
        plan_from_args(_args("--cube", a, "--cdl-sat", "0.5", "--cube2", a))
    with pytest.raises(ValueError, match="a CDL is not supported with a 1D LUT"):
        plan_from_args(_args("--cube", a, "--lut1d", t, "--cdl-sat", "0.5"))
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    params = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")
    with pytest.raises(ValueError, match="a CDL is not supported with a 1D LUT"):
        engine_command(Path("-"), Path("-"), params, Path(a), info, lut1d=Path(t), cdl=Cdl(saturation=0.5))
    with pytest.raises(ValueError, match="two-LUT chain .* is not supported with a CDL"):
        engine_command(Path("-"), Path("-"), params, Path(a), info, cube2=Path(a), cdl=Cdl(saturation=0.5))
    held = SimpleNamespace(n1d=17)
    with pytest.raises(ValueError, match="a CDL"):
        LutEngine.apply_yuv_lut1d(held, _planes(10, 1, 1), **NAMES, cdl=Cdl())
    with pytest.raises(ValueError, match="a LUT with a .csp prelut is not supported with a CDL"):
        LutEngine.apply_yuv(SimpleNamespace(_has_prelut=True), _planes(10, 1, 1), pix_fmt="yuv420p10le", cdl=Cdl())


def test_apply_lut_hands_the_engine_the_stack():
    from lut_renderer_amd.api import apply_lut

    class _Lock:
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    class _Eng:
        _lock, precision, _applied_lut, _applied_lut2, _applied_lut1d, _has_prelut = _Lock(), "strict", None, None, None, False
        n = n2 = n1d = 0

        def __init__(self): self.calls, self.sets = [], []
        def apply_yuv(self, planes, out, **kw): self.calls.append(("yuv", kw)); return out
        def apply_yuv_stack(self, planes, out, **kw): self.calls.append(("stack", kw)); return out
        def set_lut1d(self, l1, mode): self.sets.append(("lut1d", l1, mode))
        def set_lut(self, lut): self.sets.append(("lut", lut))
        def set_lut2(self, lut): self.sets.append(("lut2", lut))

    eng, y = _Eng(), frames.natural_yuv(16, 8, 10, 1, 1)
    A, B, l1, grade = _lut(2), _lut(3), cube.Lut1D.identity(16), Cdl(saturation=0.6)
    apply_lut(y, cube=A, pix_fmt="yuv420p10le", engine=eng)
    assert eng.calls[-1][0] == "yuv"                                   # without stages: the call it always made
    plain = {k: v for k, v in eng.calls[-1][1].items() if k not in ("dither", "interp")}
    eng.sets.clear()
    apply_lut(y, cube=A, cube2=B, lut1d=l1, cdl=grade, interp="trilinear", interp2="nearest", interp1d="cubic", pix_fmt="yuv420p10le",
              engine=eng, stages="lut1d,cdl,lut3d,lut3d2")
    want = (("lut1d", None), ("cdl", None), ("lut3d", "trilinear"), ("lut3d2", "nearest"))
    assert eng.calls[-1] == ("stack", {**plain, "stages": want, "cdl": grade})
    assert eng.sets == [("lut2", B), ("lut1d", l1, "cubic")]          # (A stands from the call before: the same object)
    apply_lut(y, cube=A, cube2=B, lut1d=l1, cdl=grade, interp1d="cubic", pix_fmt="yuv420p10le", engine=eng,
              stages=["lut3d2", ("lut3d", "prism"), "cdl", "lut1d"])
    assert len(eng.sets) == 2                                          # the same objects and mode: the device copies stand
    assert eng.calls[-1][1]["stages"] == (("lut3d2", "tetrahedral"), ("lut3d", "prism"), ("cdl", None), ("lut1d", None))
    apply_lut(y, cube=None, cdl=GOLDEN / "cdl" / "shot.cc", pix_fmt="yuv420p10le", engine=eng, stages="cdl")
    assert eng.calls[-1][1]["stages"] == (("cdl", None),) and eng.calls[-1][1]["cdl"] == read_cdl(GOLDEN / "cdl" / "shot.cc")
    apply_lut(list(y) + [y[0]], cube=A, pix_fmt="yuva420p10le", engine=eng, stages="lut3d")
    assert eng.calls[-1][1]["out_pix_fmt"] == "yuva420p10le"
    apply_lut(y, cube=A, pix_fmt="yuv420p10le", color_range="pc", colorspace="bt709", engine=eng, stages="lut3d")
    assert eng.calls[-1][1]["lut_depth"] == 8 and eng.calls[-1][1]["range_src"] == "pc"


# ------------------------------------------------------------------ the CLI and the argv
def _args(*extra, pix_fmt="yuv420p10le", out="yuv422p10le"):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt, "--out-pix-fmt", out, *extra])


def test_cli_flags(cube_dir):
    from lut_renderer_amd.cli import plan_from_args
    a, b, t = str(cube_dir / "log709_33.cube"), str(cube_dir / "random_9.cube"), str(GOLDEN / "lut1d" / "curve17.cube")
    plain = _args("--cube", a)
    assert plain.stages is None
    _, kw, _, _ = plan_from_args(plain)
    base = {k: v for k, v in kw.items() if k != "interp"}
    _, kw1, _, _ = plan_from_args(_args("--cube", a, "--cube2", b, "--lut1d", t, "--cdl-sat", "0.5", "--interp", "trilinear", "--interp2",
                                        "nearest", "--stages", "lut1d,cdl,lut3d,lut3d2"))
    assert kw1 == {**base, "stages": (("lut1d", None), ("cdl", None), ("lut3d", "trilinear"), ("lut3d2", "nearest")),
                   "cdl": Cdl(saturation=0.5)}
    _, kw2, _, _ = plan_from_args(_args("--cdl", str(GOLDEN / "cdl" / "shot.cc"), "--stages", "cdl"))
    assert kw2["stages"] == (("cdl", None),) and "interp" not in kw2    # no --cube: none is needed
    _, kw3, _, _ = plan_from_args(_args("--cube", a, "--lut1d", t, "--stages", "lut3d:prism,lut1d"))
    assert kw3["stages"] == (("lut3d", "prism"), ("lut1d", None)) and "cdl" not in kw3
    full = ("--cube", a, "--lut1d", t, "--stages", "lut1d,lut3d")
    for extra, message in ((("--zscale-dither", "error_diffusion"), r"dither \('error_diffusion'\) is not supported with a stage stack"),
                           (("--engine-dither", "blue_noise"), r"dither \('blue_noise'\) is not supported with a stage stack"),
                           (("--out-size", "8x4"), "resize .* is not supported with a stage stack"),
                           (("--cdl-sat", "0.5"), "--cdl-sat is given and --stages has no 'cdl' stage"),
                           (("--second-output", "c.yuv", "--second-pix-fmt", "yuv420p"), "two-output pass .* not supported with a stage stack"),
                           (("--cube2", b), "--cube2 is given and --stages has no 'lut3d2' stage"),
                           (("--interp2", "nearest"), "--interp2 is the mode of the second LUT"),
                           (("--interp1d", "bicubic"), "lut1d has no interpolation mode 'bicubic'")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args(*full, *extra))
    for stages, message in (("lut1d,lut3d,cdl", "stage 'cdl' is listed and no CDL is given"), ("lut1d,lut3d,lut3d2", "no second LUT is loaded"),
                            ("lut1d", "--cube is given and --stages has no 'lut3d' stage"), ("", "the stage list is empty"),
                            ("lut1d,lut3d,lut1d", "listed twice")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args("--cube", a, "--lut1d", t, "--stages", stages))
    with pytest.raises(ValueError, match="no 3D LUT is loaded"):
        plan_from_args(_args("--lut1d", t, "--stages", "lut1d,lut3d"))
    with pytest.raises(ValueError, match="chroma_loc.* is not supported with a stage stack"):
        plan_from_args(_args(*full, "--chroma-loc", "left", out="yuv420p10le"))
    with pytest.raises(ValueError, match="alpha_mode='premultiplied' is not supported with a stage stack"):
        plan_from_args(_args(*full, "--alpha-mode", "premultiplied", pix_fmt="yuva444p10le", out="yuv444p10le"))
    with pytest.raises(ValueError, match="is an RGB format"):
        plan_from_args(_args(*full, pix_fmt="gbrp10le", out="yuv420p10le"))


def test_engine_command_renders_the_flag_only_when_given(cube_dir):
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    from lut_renderer_amd.pipe import engine_stage_commands
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    params = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")
    a, b, t = cube_dir / "log709_33.cube", cube_dir / "random_9.cube", GOLDEN / "lut1d" / "curve17.cube"
    io = (Path("-"), Path("-"), params, a, info)
    plain = engine_command(*io)
    assert "--stages" not in plain and engine_command(*io, stages=None) == plain       # byte for byte what it was
    assert engine_command(*io, lut1d=t) == plain + ["--lut1d", str(t)]
    assert engine_command(*io, stages="lut3d") == plain + ["--stages", "lut3d:tetrahedral"]
    grade = Cdl(slope=(1.1, 1.0, 0.9), saturation=0.6)
    cmd = engine_command(*io, cube2=b, interp2="nearest", cdl=grade, lut1d=t, interp1d="cubic", stages=["lut1d", "cdl", "lut3d", "lut3d2"])
    assert cmd == plain + ["--cube2", str(b), "--interp2", "nearest", "--cdl-sop", grade.sop_text(), "--cdl-sat", repr(0.6), "--lut1d", str(t),
                           "--interp1d", "cubic", "--stages", "lut1d,cdl,lut3d:tetrahedral,lut3d2:nearest"]
    # the round trip: the CLI parses what the builder rendered into the same call
    args = build_parser().parse_args(cmd[3:])
    _, kw, _, _ = plan_from_args(args)
    assert kw["stages"] == (("lut1d", None), ("cdl", None), ("lut3d", "tetrahedral"), ("lut3d2", "nearest")) and kw["cdl"] == grade
    assert (args.cube2, args.lut1d, args.interp1d) == (str(b), str(t), "cubic")
    cmds = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, lut1d=t, stages="lut3d:trilinear,lut1d")
    assert cmds.engine[cmds.engine.index("--stages") + 1] == "lut3d:trilinear,lut1d"
    assert "--stages" not in engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, lut1d=t).engine
    for kw, message in ((dict(stages="lut1d"), "the LUT is given and the stage list has no 'lut3d' stage"),
                        (dict(stages="lut3d", lut1d=t), "lut1d is given and the stage list has no 'lut1d' stage"),
                        (dict(stages="lut3d,cdl"), "stage 'cdl' is listed and no CDL is given"),
                        (dict(stages="lut3d,lut3d2"), "no second LUT is loaded"),
                        (dict(stages="lut3d", engine_dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a stage stack"),
                        (dict(stages="lut3d", chroma_loc="left"), "chroma_loc.* is not supported with a stage stack"),
                        (dict(stages="lut3d,lut3d"), "listed twice")):
        with pytest.raises(ValueError, match=message):
            engine_command(*io, **kw)
