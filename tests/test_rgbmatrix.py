"""The RGB matrix stage of the stage stack without a GPU: the matrix line by known answers, the twin's equalities
with the stacks that exist, `matrix, cdl` against its composition written out, the parser, the one copy of the refusals through
every layer, the .spimtx reader and the argv."""
import threading
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.cdl import Cdl, read_cdl
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.formats import check_stack_options, parse_stages, stages_string
from lut_renderer_amd.rgbmatrix import RgbMatrix, as_rgb_matrix, read_rgb_matrix
from tests import _cdl_twin as cdlt
from tests import _lut1d_twin as l1t
from tests import _matrix_twin as twin
from tests import _stack_twin as skt

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
F = np.float32
I3 = RgbMatrix()
SWAP = RgbMatrix((0, 0, 1, 0, 1, 0, 1, 0, 0))
TWICE = RgbMatrix((2, 0, 0, 0, 2, 0, 0, 0, 2))
NEG = RgbMatrix((-1.0, -0.5, 0.0, 0.25, 0.5, 0.25, 0.0, -2.0, 1.0), (0.25, 0.0, 0.5))
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


def _codes_through(mtx, dl):
    """Every code k as the pixel (k, k', k'') through the matrix and the rounding: k' and k'' walk the codes in other orders."""
    m = (1 << dl) - 1
    k = np.arange(m + 1)
    px = (k, k[::-1].copy(), (k * 7) % (m + 1))
    return px, twin.round_codes(twin.matrix_unit(mtx, twin.unit_of_codes(px, dl)), dl)


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("dl", [8, 10, 12, 16])
def test_known_answers_over_every_code(dl):
    m = (1 << dl) - 1
    px, out = _codes_through(I3, dl)
    assert _eq(out, px)                                             # (int)(fl(fl(k * fl(1 / M)) * M) + 0.5f) == k (3.21)
    px, out = _codes_through(SWAP, dl)
    assert _eq(out, (px[2], px[1], px[0]))                          # exactly a channel swap
    px, out = _codes_through(TWICE, dl)
    for p, o in zip(px, out):
        assert (o[2 * p >= m] == m).all() and (o[2 * p < m] < m).all() and (o >= p).all()
    # a negative row with an offset: R' = 0.25 - r - g / 2 is below 0 wherever r + g / 2 > 0.25, and clamps there
    px, out = _codes_through(NEG, dl)
    r, g = px[0] / m, px[1] / m
    assert (out[0][r + g / 2 > 0.2501] == 0).all() and (out[0] >= 0).all() and (out[0][r + g / 2 < 0.2] > 0).all()
    assert all((o >= 0).all() and (o <= m).all() for o in out)


def test_the_matrix_line_one_operation_at_a_time():
    """Entries that are no float32 and a pixel written out by hand: every product and sum rounded on its own, in the order given."""
    mtx = read_rgb_matrix(GOLDEN / "matrix" / "bt2020_to_709.spimtx")
    u = [np.array([v], F) for v in (0.3, 0.6, 0.9)]
    got = twin.matrix_unit(mtx, u)
    for row in range(3):
        m0, m1, m2, off = (F(v) for v in (*mtx.m[3 * row:3 * row + 3], mtx.offset[row]))
        t = F(F(F(F(m0 * u[0][0]) + F(m1 * u[1][0])) + F(m2 * u[2][0])) + off)
        assert got[row][0] == min(max(t, F(0)), F(1)) and got[row].dtype == F
    assert twin.matrix_unit(TWICE, u)[2][0] == F(1) and twin.matrix_unit(NEG, u)[0][0] == F(0)


# ------------------------------------------------------------------ the twin's equalities
def test_the_identity_matrix_is_the_identity_cdl(orc):
    A, _ = _luts()
    l1 = cube.read_lut1d(GOLDEN / "lut1d" / "curve17.cube")
    for tag, k, dl, dout, icsx, icsy, ocsx, ocsy, src in _cases():
        io = (k, dl, dout, icsx, icsy, ocsx, ocsy, src)
        assert _eq(twin.apply(["matrix"], *io, mtx=I3), skt.apply(["cdl"], *io, cdl=Cdl())), tag
        for mode in ("nearest", "trilinear", "tetrahedral"):
            got = twin.apply(["matrix", ("lut3d", mode)], *io, lut=A, mtx=I3)
            assert _eq(got, skt.apply(["cdl", ("lut3d", mode)], *io, lut=A, cdl=Cdl())), (tag, mode)
        assert _eq(twin.apply(["lut3d", "matrix"], *io, lut=A, mtx=I3), skt.apply(["lut3d"], *io, lut=A)), tag
        tab = l1t.table(l1.table, l1.scale, "linear", dl)
        assert _eq(twin.apply(["matrix", "lut1d"], *io, l1d_tab=tab, mtx=I3), skt.apply(["lut1d"], *io, l1d_tab=tab)), tag


def test_without_a_matrix_the_twin_is_the_stack_twin(orc):
    A, B = _luts()
    grade = read_cdl(GOLDEN / "cdl" / "shot.cc")
    for tag, k, dl, dout, icsx, icsy, ocsx, ocsy, src in _cases():
        io = (k, dl, dout, icsx, icsy, ocsx, ocsy, src)
        st = ["lut3d", "cdl", ("lut3d2", "trilinear")]
        assert _eq(twin.apply(st, *io, lut=A, lut2=B, cdl=grade), skt.apply(st, *io, lut=A, lut2=B, cdl=grade)), tag


def test_matrix_then_cdl_rounds_in_between(orc):
    from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
    grade = read_cdl(GOLDEN / "cdl" / "shot.cc")
    mtx = read_rgb_matrix(GOLDEN / "matrix" / "bt2020_to_709.spimtx")
    (icsx, icsy), (ocsx, ocsy) = twin.LAYOUTS["420"], twin.LAYOUTS["422"]
    src = frames.natural_yuv(37, 13, 10, icsx, icsy, k=2)
    k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, ocsx, ocsy)
    ct = cdlt.table(grade, 10)
    r, g, b = yuv_to_rgb_codes(k, icsx, icsy, src)
    rcp = F(1.0) / F(1023)
    u = [(c.astype(F) * rcp).astype(F) for c in (r, g, b)]
    o = []
    for row in range(3):
        m0, m1, m2, off = (F(v) for v in (*mtx.m[3 * row:3 * row + 3], mtx.offset[row]))
        t = ((((m0 * u[0]).astype(F) + (m1 * u[1]).astype(F)).astype(F) + (m2 * u[2]).astype(F)).astype(F) + off).astype(F)
        o.append(np.minimum(np.maximum(t, F(0)), F(1)))
    q = [((v * F(1023)).astype(F) + F(0.5)).astype(F).astype(np.int64) for v in o]        # the CDL's table is per code
    graded = cdlt.saturate(grade.saturation, [ct[0][q[0]], ct[1][q[1]], ct[2][q[2]]])
    q2 = [((v * F(1023)).astype(F) + F(0.5)).astype(F).astype(np.int64) for v in graded]
    want = rgb_codes_to_yuv(k, 10, ocsx, ocsy, tuple(q2))
    assert _eq(twin.apply(["matrix", "cdl"], k, 10, 10, icsx, icsy, ocsx, ocsy, src, cdl=grade, mtx=mtx), want)
    # and the matrix behind the CDL takes its unit floats as they are
    graded = cdlt.saturate(grade.saturation, [ct[0][r], ct[1][g], ct[2][b]])
    want = rgb_codes_to_yuv(k, 10, ocsx, ocsy, twin.round_codes(twin.matrix_unit(mtx, graded), 10))
    assert _eq(twin.apply(["cdl", "matrix"], k, 10, 10, icsx, icsy, ocsx, ocsy, src, cdl=grade, mtx=mtx), want)


# ------------------------------------------------------------------ the value type and the reader
def test_rgb_matrix_values():
    assert I3.is_identity and RgbMatrix.identity() == I3 and not SWAP.is_identity
    assert RgbMatrix([[1, 0, 0], [0, 1, 0], [0, 0, 1]]) == I3
    assert RgbMatrix.from_text(NEG.m_text(), NEG.offset_text()) == NEG and RgbMatrix.from_text(None) == I3
    assert RgbMatrix.from_text("0,0,1, 0,1,0, 1,0,0") == SWAP
    assert RgbMatrix((65536,) + (0,) * 8, (-65536, 0, 0)).m[0] == 65536.0
    for bad, message in ((dict(m=(1, 0, 0)), "m must be 9 numbers, got 3"), (dict(m="identity"), "m must be 9 numbers"),
                         (dict(offset=(0, 0)), "offset must be 3 numbers, got 2"),
                         (dict(m=(float("nan"),) + (0,) * 8), r"m\[0\] is not finite"),
                         (dict(offset=(0, float("inf"), 0)), r"offset\[1\] is not finite"),
                         (dict(m=(0,) * 8 + (65537,)), r"m\[8\] is above 65536 in magnitude"),
                         (dict(offset=(0, 0, -1e6)), r"offset\[2\] is above 65536 in magnitude")):
        with pytest.raises(ValueError, match=message):
            RgbMatrix(**bad)
    with pytest.raises(ValueError, match="--rgb-matrix takes 9 numbers, got 3"):
        RgbMatrix.from_text("1 0 0")
    with pytest.raises(ValueError, match="--rgb-matrix-offset takes 3 numbers"):
        RgbMatrix.from_text(None, "a b c")
    st = _native.rgb_matrix_struct(NEG)
    assert list(st.m) == [F(v) for v in NEG.m] and list(st.offset) == [F(v) for v in NEG.offset]
    import ctypes as C
    assert C.sizeof(_native.RgbMatrixStruct) == 12 * 4


def test_the_spimtx_reader(tmp_path):
    mtx = read_rgb_matrix(GOLDEN / "matrix" / "bt2020_to_709.spimtx")
    assert mtx.m == (1.6605, -0.5876, -0.0728, -0.1246, 1.1329, -0.0083, -0.0182, -0.1006, 1.1187)
    assert mtx.offset == (655.35 / 65535.0, 0.0, -327.675 / 65535.0)               # the fourth column is in 16-bit codes
    assert as_rgb_matrix(str(GOLDEN / "matrix" / "bt2020_to_709.spimtx")) == mtx and as_rgb_matrix(mtx) is mtx and as_rgb_matrix(None) is None
    with pytest.raises(ValueError, match=r"eleven\.spimtx: holds 11 numbers, expected 12"):
        read_rgb_matrix(GOLDEN / "matrix" / "eleven.spimtx")
    with pytest.raises(ValueError, match=r"nan\.spimtx: RGB matrix m\[4\] is not finite"):
        read_rgb_matrix(GOLDEN / "matrix" / "nan.spimtx")
    with pytest.raises(ValueError, match=r"nope\.spimtx: cannot read"):
        read_rgb_matrix(tmp_path / "nope.spimtx")
    (tmp_path / "word.spimtx").write_text("1 0 0 0 0 one 0 0 0 0 1 0")
    with pytest.raises(ValueError, match=r"word\.spimtx: entry 6 is 'one', not a number"):
        read_rgb_matrix(tmp_path / "word.spimtx")
    with pytest.raises(TypeError, match="rgb_matrix must be an RgbMatrix or the path"):
        as_rgb_matrix(3)


# ------------------------------------------------------------------ the parser
def test_parse_stages_takes_matrix():
    assert parse_stages("lut1d,matrix,lut3d:trilinear") == (("lut1d", None), ("matrix", None), ("lut3d", "trilinear"))
    st = parse_stages(("matrix", "cdl", "lut1d", "lut3d"))
    assert parse_stages(st) == st and parse_stages(stages_string(st)) == st and stages_string("matrix") == "matrix"
    for bad, message in (("matrix:x", r"stage 'matrix' takes no mode \('x'\)"), ("matrix,lut3d,matrix", "stage kind 'matrix' is listed twice"),
                         ("matrix,cdl,lut1d,lut3d,lut3d2", "has 5 stages"), ("matrix,gamma", "unknown stage kind 'gamma'")):
        with pytest.raises(ValueError, match=message):
            parse_stages(bad)
    header = (ROOT / "include" / "lutr.h").read_text()
    assert "LUTR_STAGE_MATRIX  = 5" in header and "lutr_apply_yuv_stack_matrix" in header
    assert _native.STAGE_KINDS == {"lut3d": 1, "lut3d2": 2, "lut1d": 3, "cdl": 4} and _native.MATRIX_STAGE_KINDS == {"matrix": 5}
    assert "lutr_apply_yuv_stack_matrix" in _native.SYMBOLS and hasattr(_native.load(), "lutr_apply_yuv_stack_matrix")
    arr = _native.stage_array(parse_stages("lut1d,matrix,lut3d2:prism"))
    assert [(s.kind, s.interp) for s in arr] == [(3, 0), (5, 0), (2, 4)]


# ------------------------------------------------------------------ one copy of the refusals
NAMES = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
REFUSALS = [(dict(stages="matrix,lut3d"), "stage 'matrix' is listed and no RGB matrix is given"),
            (dict(stages="lut3d", rgb_matrix=True), "an RGB matrix is given and the stage list has no 'matrix' stage"),
            (dict(stages="matrix,lut3d", rgb_matrix=True, prelut=True),
             "'lut3d' directly behind 'matrix' is not supported with a LUT that carries a .csp prelut"),
            (dict(stages="cdl,matrix,lut3d", cdl=True, rgb_matrix=True, prelut=True), "'lut3d' directly behind 'matrix'"),
            (dict(stages="matrix,lut3d", rgb_matrix=True, strength=0.5), "stage 'matrix' is not supported with strength"),
            (dict(stages="matrix,lut3d", rgb_matrix=True, matte=True), "stage 'matrix' is not supported with a matte"),
            (dict(stages="matrix", rgb_matrix=True, strength=1.0, matte=True), "stage 'matrix' is not supported with strength and a matte"),
            (dict(stages="matrix", rgb_matrix=True, dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a stage stack"),
            (dict(stages="matrix", rgb_matrix=True, variant="vec_lds"), "variant vec_lds is not supported with a stage stack")]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_check_stack_options_refuses(kw, message):
    with pytest.raises(ValueError, match=message):
        check_stack_options(**NAMES, **kw)


def test_what_check_stack_options_takes():
    st, fin, fout = check_stack_options(**NAMES, stages="matrix,cdl,lut1d,lut3d", cdl=True, rgb_matrix=True)
    assert [k for k, _ in st] == ["matrix", "cdl", "lut1d", "lut3d"] and (fin.name, fout.name) == ("yuv420p10le", "yuv422p10le")
    _, fin, fout = check_stack_options("yuva444p10le", "yuva444p10le", stages="matrix", rgb_matrix=True)
    assert fin.alpha and fout.alpha                                 # straight alpha goes through the alpha tail
    # a prelut is fine wherever lut3d is fed codes
    check_stack_options(**NAMES, stages="lut3d,matrix", rgb_matrix=True, prelut=True)
    check_stack_options(**NAMES, stages="matrix,lut1d,lut3d", rgb_matrix=True, prelut=True)
    check_stack_options(**NAMES, stages="matrix,lut3d2,lut3d", rgb_matrix=True, prelut=True)
    with pytest.raises(ValueError, match="an RGB format"):
        check_stack_options("gbrp10le", None, stages="matrix", rgb_matrix=True)


def _planes(depth, csx, csy):
    import torch
    return [torch.from_numpy(p.view(np.int16)) for p in frames.natural_yuv(16, 8, depth, csx, csy)]


def test_the_engine_refuses_before_it_is_touched():
    src = _planes(10, 1, 1)
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False)
    for kw, message in ((dict(stages="matrix,lut3d"), "no RGB matrix is given"),
                        (dict(stages="lut3d", rgb_matrix=I3), "has no 'matrix' stage"),
                        (dict(stages="matrix,lut3d", rgb_matrix=I3, strength=0.5), "stage 'matrix' is not supported with strength"),
                        (dict(stages="matrix,lut3d", rgb_matrix=I3, matte=src[0]), "stage 'matrix' is not supported with a matte"),
                        (dict(stages="matrix,matrix", rgb_matrix=I3), "twice"), (dict(stages="matrix:x", rgb_matrix=I3), "takes no mode"),
                        (dict(stages="matrix", rgb_matrix=I3, out_pix_fmt="nv12"), "semi-planar")):
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_yuv_stack(held, src, **{**NAMES, **kw})
    with pytest.raises(ValueError, match="directly behind 'matrix'"):
        LutEngine.apply_yuv_stack(SimpleNamespace(n=33, _has_prelut=True), src, **NAMES, stages="matrix,lut3d", rgb_matrix=I3)
    with pytest.raises(TypeError, match="rgb_matrix must be a lut_renderer_amd.rgbmatrix.RgbMatrix"):
        LutEngine.apply_yuv_stack(held, src, **NAMES, stages="matrix", rgb_matrix="a.spimtx")


def test_the_group_checks_the_same_things_first():
    from lut_renderer_amd.multigpu import LutEngineGroup
    g = SimpleNamespace(_lock=threading.RLock(), n1d=17, engines=[SimpleNamespace(n=33, n2=0, _has_prelut=True)])
    for kw, message in ((dict(stages="matrix,lut3d"), "no RGB matrix is given"), (dict(stages="lut1d", rgb_matrix=I3), "has no 'matrix' stage"),
                        (dict(stages="matrix,lut3d", rgb_matrix=I3), "directly behind 'matrix'"),
                        (dict(stages="matrix", rgb_matrix=I3, strength=0.5), "stage 'matrix' is not supported with strength"),
                        (dict(stages="matrix", rgb_matrix=I3, row0=0), "the group owns the row partition")):
        with pytest.raises(ValueError, match=message):
            LutEngineGroup.apply_yuv_stack(g, _planes(10, 1, 1), **{**NAMES, **kw})


def _lut(n=2):
    return cube.CubeLut(n, np.ones(3, F), cube.identity_lattice(n).astype(F))


def test_apply_lut_refuses_while_planning_and_hands_the_engine_the_matrix():
    from lut_renderer_amd.api import apply_lut
    y = frames.natural_yuv(16, 8, 10, 1, 1)
    base = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", engine=SimpleNamespace(n=0, n2=0, n1d=0, _has_prelut=False))
    for kw, message in ((dict(cube=_lut(), rgb_matrix=I3), "rgb_matrix needs stages: a matrix stage has no implied position"),
                        (dict(cube=_lut(), rgb_matrix=I3, strength=0.5), "rgb_matrix needs stages"),
                        (dict(cube=_lut(), stages="matrix,lut3d"), "stage 'matrix' is listed and no RGB matrix is given"),
                        (dict(cube=_lut(), stages="lut3d", rgb_matrix=I3), "an RGB matrix is given and the stage list has no 'matrix' stage"),
                        (dict(cube=_lut(), stages="matrix,lut3d", rgb_matrix=I3, strength=0.5), "stage 'matrix' is not supported with strength"),
                        (dict(cube=_lut(), stages="matrix,lut3d", rgb_matrix=GOLDEN / "matrix" / "eleven.spimtx"), "holds 11 numbers"),
                        (dict(cube=_lut(), stages="matrix,lut3d", rgb_matrix=I3, rgb_out="gbrp10le", out_pix_fmt=None), "stages")):
        with pytest.raises(ValueError, match=message):
            apply_lut(y, **{**base, **kw})
    with pytest.raises(TypeError, match="rgb_matrix must be an RgbMatrix or the path"):
        apply_lut(y, **base, cube=_lut(), stages="matrix,lut3d", rgb_matrix=(1, 0, 0))

    class _Lock:
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    class _Eng:
        _lock, precision, _applied_lut, _applied_lut2, _applied_lut1d, _has_prelut = _Lock(), "strict", None, None, None, False
        n = n2 = n1d = 0

        def __init__(self): self.calls = []
        def apply_yuv_stack(self, planes, out, **kw): self.calls.append(kw); return out
        def set_lut(self, lut): pass

    eng = _Eng()
    apply_lut(y, cube=_lut(), pix_fmt="yuv420p10le", engine=eng, stages="lut3d")
    assert "rgb_matrix" not in eng.calls[-1]                           # without a matrix: the call it always made
    apply_lut(y, cube=_lut(), pix_fmt="yuv420p10le", engine=eng, stages="matrix,lut3d:nearest", rgb_matrix=NEG)
    assert eng.calls[-1]["rgb_matrix"] is NEG and eng.calls[-1]["stages"] == (("matrix", None), ("lut3d", "nearest"))
    apply_lut(y, cube=None, pix_fmt="yuv420p10le", engine=eng, stages="matrix", rgb_matrix=GOLDEN / "matrix" / "bt2020_to_709.spimtx")
    assert eng.calls[-1]["rgb_matrix"] == read_rgb_matrix(GOLDEN / "matrix" / "bt2020_to_709.spimtx")


def test_host_pipeline_refuses_in_its_constructor():
    from lut_renderer_amd.stream import HostPipeline
    eng = SimpleNamespace(n=33, n2=0, n1d=0, _has_prelut=False)
    for kw, message in ((dict(rgb_matrix=I3), "an RGB matrix is a stage of the stage stack: it needs stages"),
                        (dict(stages="lut3d", rgb_matrix=I3), "has no 'matrix' stage"),
                        (dict(stages="matrix,lut3d"), "no RGB matrix is given"),
                        (dict(stages="matrix,lut3d", rgb_matrix=None), "no RGB matrix is given"),
                        (dict(stages="matrix,lut3d", rgb_matrix=I3, strength=0.5), "stage 'matrix' is not supported with strength")):
        with pytest.raises(ValueError, match=message):
            HostPipeline(eng, "yuv420p10le", 16, 8, out_pix_fmt="yuv422p10le", **kw)


# ------------------------------------------------------------------ the CLI and the argv
def _args(*extra, pix_fmt="yuv420p10le", out="yuv422p10le"):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt, "--out-pix-fmt", out, *extra])


def test_cli_flags(cube_dir):
    from lut_renderer_amd.cli import plan_from_args
    a, t = str(cube_dir / "log709_33.cube"), str(GOLDEN / "lut1d" / "curve17.cube")
    f = str(GOLDEN / "matrix" / "bt2020_to_709.spimtx")
    plain = _args("--cube", a)
    assert plain.rgb_matrix is None and plain.rgb_matrix_offset is None and plain.rgb_matrix_file is None
    _, kw, _, _ = plan_from_args(_args("--cube", a, "--stages", "lut3d"))
    assert "rgb_matrix" not in kw
    _, kw1, _, _ = plan_from_args(_args("--cube", a, "--lut1d", t, "--stages", "lut1d,matrix,lut3d", "--rgb-matrix", NEG.m_text(),
                                        "--rgb-matrix-offset", NEG.offset_text()))
    assert kw1 == {**kw, "stages": (("lut1d", None), ("matrix", None), ("lut3d", "tetrahedral")), "rgb_matrix": NEG}
    _, kw2, _, _ = plan_from_args(_args("--stages", "matrix", "--rgb-matrix-file", f))
    assert kw2["stages"] == (("matrix", None),) and kw2["rgb_matrix"] == read_rgb_matrix(f)       # no --cube: none is needed
    _, kw3, _, _ = plan_from_args(_args("--stages", "matrix", "--rgb-matrix", SWAP.m_text()))
    assert kw3["rgb_matrix"] == SWAP
    full = ("--cube", a, "--stages", "matrix,lut3d")
    for extra, message in ((("--rgb-matrix", "1 0 0"), "--rgb-matrix takes 9 numbers, got 3"),
                           (("--rgb-matrix-offset", "0 0 0"), "--rgb-matrix-offset is the offset of a matrix: it needs --rgb-matrix"),
                           (("--rgb-matrix", I3.m_text(), "--rgb-matrix-file", f), "use one or the other"),
                           (("--rgb-matrix-file", str(GOLDEN / "matrix" / "nan.spimtx")), r"nan\.spimtx: RGB matrix m\[4\] is not finite"),
                           ((), "stage 'matrix' is listed and no RGB matrix is given"),
                           (("--rgb-matrix", I3.m_text(), "--strength", "0.5"), "stage 'matrix' is not supported with strength"),
                           (("--rgb-matrix", I3.m_text(), "--matte", "m.gray"), "stage 'matrix' is not supported with a matte"),
                           (("--rgb-matrix", I3.m_text(), "--engine-dither", "blue_noise"), r"dither \('blue_noise'\) is not supported")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args(*full, *extra))
    with pytest.raises(ValueError, match="--rgb-matrix / --rgb-matrix-file is given and --stages has no 'matrix' stage"):
        plan_from_args(_args("--cube", a, "--stages", "lut3d", "--rgb-matrix", I3.m_text()))
    for extra in ((), ("--strength", "0.5"), ("--lut1d", t)):
        with pytest.raises(ValueError, match="--rgb-matrix / --rgb-matrix-file need --stages"):
            plan_from_args(_args("--cube", a, "--rgb-matrix", I3.m_text(), *extra))
    with pytest.raises(ValueError, match="directly behind 'matrix'"):
        from tests._csp_files import write_csp_with_prelut
        import tempfile
        with tempfile.TemporaryDirectory() as d:
            p = Path(d) / "shaped.csp"
            write_csp_with_prelut(p, 5, cube.log709_lattice(5), [(np.linspace(0.0, 1.0, 5), np.linspace(0.0, 1.0, 5) ** 0.7)] * 3)
            plan_from_args(_args("--cube", str(p), "--stages", "matrix,lut3d", "--rgb-matrix", I3.m_text()))


def test_engine_command_renders_the_flags_only_when_given(cube_dir):
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    from lut_renderer_amd.pipe import engine_stage_commands
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    params = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")
    a, t, f = cube_dir / "log709_33.cube", GOLDEN / "lut1d" / "curve17.cube", GOLDEN / "matrix" / "bt2020_to_709.spimtx"
    io = (Path("-"), Path("-"), params, a, info)
    plain = engine_command(*io)
    assert not any(x.startswith("--rgb-matrix") for x in plain) and engine_command(*io, rgb_matrix=None) == plain
    assert engine_command(*io, stages="lut3d", rgb_matrix=None) == plain + ["--stages", "lut3d:tetrahedral"]
    cmd = engine_command(*io, lut1d=t, stages="lut1d,matrix,lut3d", rgb_matrix=NEG)
    assert cmd == plain + ["--lut1d", str(t), "--rgb-matrix", NEG.m_text(), "--rgb-matrix-offset", NEG.offset_text(), "--stages",
                           "lut1d,matrix,lut3d:tetrahedral"]
    assert engine_command(*io, stages="matrix,lut3d", rgb_matrix=SWAP) == plain + ["--rgb-matrix", SWAP.m_text(), "--stages",
                                                                                  "matrix,lut3d:tetrahedral"]
    assert engine_command(*io, stages="lut3d,matrix", rgb_matrix=f) == plain + ["--rgb-matrix-file", str(f), "--stages",
                                                                               "lut3d:tetrahedral,matrix"]
    # the round trip: the CLI parses what the builder rendered into the same call
    _, kw, _, _ = plan_from_args(build_parser().parse_args(cmd[3:]))
    assert kw["stages"] == (("lut1d", None), ("matrix", None), ("lut3d", "tetrahedral")) and kw["rgb_matrix"] == NEG
    cmds = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, stages="matrix,lut3d:trilinear", rgb_matrix=NEG)
    assert cmds.engine[cmds.engine.index("--rgb-matrix") + 1] == NEG.m_text()
    assert cmds.engine[cmds.engine.index("--stages") + 1] == "matrix,lut3d:trilinear"
    assert not any(x.startswith("--rgb-matrix") for x in engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info).engine)
    for kw, message in ((dict(rgb_matrix=I3), "rgb_matrix needs stages"),
                        (dict(stages="lut3d", rgb_matrix=I3), "rgb_matrix is given and the stage list has no 'matrix' stage"),
                        (dict(stages="matrix,lut3d"), "stage 'matrix' is listed and no RGB matrix is given"),
                        (dict(stages="matrix,lut3d", rgb_matrix=I3, strength=0.5), "stage 'matrix' is not supported with strength"),
                        (dict(stages="matrix,lut3d", rgb_matrix=I3, matte=Path("m.gray")), "stage 'matrix' is not supported with a matte"),
                        (dict(stages="matrix,lut3d", rgb_matrix=I3, chroma_loc="left"), "chroma_loc.* is not supported with a stage stack")):
        with pytest.raises(ValueError, match=message):
            engine_command(*io, **kw)
    with pytest.raises(TypeError, match="rgb_matrix must be an RgbMatrix or the path"):
        engine_command(*io, stages="matrix,lut3d", rgb_matrix=3)
