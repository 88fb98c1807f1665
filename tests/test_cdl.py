"""ASC CDL in front of the LUT -- host side: the file reader, the host table builder against the twin's, the twin
pinned to the C oracle, the refusals that run before any GPU work, and the CLI / command-layer options.  GPU parity is
tests/test_gpu_cdl.py."""
import ctypes as C
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.cdl import Cdl, as_cdl, read_cdl
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.formats import check_cdl_options
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from tests import _cdl_twin as twin
from tests import _xsub_twin as xsub
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "cdl"
F = np.float32
LAYOUTS = twin.LAYOUTS
#: slopes around 1.3, offsets -0.08 and +0.05, powers 0.8 and 1.2, different per channel
GRADE = Cdl((1.3, 1.25, 1.1), (-0.08, 0.0, 0.05), (0.8, 1.0, 1.2), 0.6)


def _eq(got, want):
    return all(np.asarray(g).shape == np.asarray(w).shape and np.array_equal(g, w) for g, w in zip(got, want))


def _ulps(a, b):
    """Distance in float32 steps between two arrays of finite non-negative floats."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------ the reader
def test_a_cc_file():
    c = read_cdl(GOLDEN / "shot.cc")
    assert c == Cdl((1.3, 1.25, 1.1), (-0.08, 0.0, 0.05), (0.8, 1.0, 1.2), 0.6) == GRADE
    assert read_cdl(GOLDEN / "shot.cc", "shot_010") == c and read_cdl(str(GOLDEN / "shot.cc")) == c
    assert as_cdl(GOLDEN / "shot.cc") == c and as_cdl(c) is c and as_cdl(None) is None


def test_a_ccc_file_with_three_ids():
    assert read_cdl(GOLDEN / "reel.ccc", "a001") == Cdl((1.1, 1.1, 1.1), (0.01, 0.02, 0.03), (1.0, 1.0, 1.0), 1.0)
    assert read_cdl(GOLDEN / "reel.ccc", "a002") == Cdl((0.9, 1.0, 1.2), (-0.02, 0.0, 0.02), (1.2, 1.1, 0.9), 1.7)
    third = read_cdl(GOLDEN / "reel.ccc", "a003")                   # no SOPNode: identity slope / offset / power
    assert third == Cdl(saturation=0.0) and third.slope == (1.0, 1.0, 1.0) and third.power == (1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match=r"reel\.ccc: 3 corrections in the file \('a001', 'a002', 'a003'\)"):
        read_cdl(GOLDEN / "reel.ccc")
    with pytest.raises(ValueError, match=r"reel\.ccc: no <ColorCorrection> with id 'a004' \(ids in the file: 'a001', 'a002', 'a003'\)"):
        read_cdl(GOLDEN / "reel.ccc", "a004")


def test_a_cdl_file_a_namespace_and_a_missing_sat_node():
    assert read_cdl(GOLDEN / "edit.cdl") == Cdl((1.05, 0.95, 1.0), (0.0, 0.03, -0.04), (1.0, 0.9, 1.1), 0.85)
    assert read_cdl(GOLDEN / "edit.cdl", "cd_0042").saturation == 0.85
    assert read_cdl(GOLDEN / "namespaced_v12.cc") == Cdl((1.2, 1.0, 0.8), (0.1, 0.0, -0.1), (1.0, 1.5, 2.0), 1.25)
    nosat = read_cdl(GOLDEN / "no_sat.cc")
    assert nosat == Cdl((0.5, 0.6, 0.7), (0.25, 0.2, 0.15), (2.0, 1.0, 0.5)) and nosat.saturation == 1.0


def test_any_asc_namespace_and_no_other(tmp_path):
    body = "<SOPNode><Slope>2 2 2</Slope></SOPNode>"
    for ns in ("urn:ASC:CDL:v1.01", "urn:ASC:CDL:v1.2", "urn:ASC:CDL:v2.0"):
        p = tmp_path / "ns.cc"
        p.write_text(f'<ColorCorrection xmlns="{ns}" id="x">{body}</ColorCorrection>')
        assert read_cdl(p) == Cdl(slope=(2, 2, 2))
    p.write_text(f'<ColorCorrection xmlns="http://www.w3.org/1999/xhtml">{body}</ColorCorrection>')
    with pytest.raises(ValueError, match="namespace is not an ASC CDL one"):
        read_cdl(p)
    p.write_text("<Look><ColorCorrection/></Look>")
    with pytest.raises(ValueError, match=r"ns\.cc: the root element is <Look>"):
        read_cdl(p)
    p.write_text("<ColorCorrectionCollection/>")
    with pytest.raises(ValueError, match="no <ColorCorrection> in it"):
        read_cdl(p)


def test_malformed_files_name_the_file_and_the_fault(tmp_path):
    with pytest.raises(ValueError, match=r"bad_two_slopes\.cc: <Slope> holds 2 numbers, expected 3"):
        read_cdl(GOLDEN / "bad_two_slopes.cc")
    with pytest.raises(ValueError, match=r"bad_negative_power\.cc: CDL power of G must be above 0 \(-0\.5\)"):
        read_cdl(GOLDEN / "bad_negative_power.cc")
    with pytest.raises(ValueError, match=r"not_xml\.cc: not an XML file"):
        read_cdl(GOLDEN / "not_xml.cc")
    with pytest.raises(ValueError, match=r"missing\.cc: cannot read"):
        read_cdl(tmp_path / "missing.cc")
    p = tmp_path / "words.cc"
    p.write_text("<ColorCorrection><SatNode><Saturation>lots</Saturation></SatNode></ColorCorrection>")
    with pytest.raises(ValueError, match=r"words\.cc: <Saturation> holds 'lots'"):
        read_cdl(p)
    with pytest.raises(TypeError, match="cdl must be a Cdl or the path"):
        as_cdl(1.5)


def test_the_value_type_validates_and_is_frozen():
    assert Cdl.identity() == Cdl() and Cdl.identity().is_identity and not GRADE.is_identity
    assert Cdl([1, 2, 3]).slope == (1.0, 2.0, 3.0) and hash(Cdl()) == hash(Cdl.identity())
    with pytest.raises(Exception):
        Cdl().saturation = 2.0
    for kw, message in ((dict(slope=(1, -0.1, 1)), "slope of G is negative"), (dict(power=(0, 1, 1)), "power of R must be above 0"),
                        (dict(power=(1, 1, -2)), "power of B must be above 0"), (dict(saturation=-0.5), "saturation is negative"),
                        (dict(offset=(0, float("nan"), 0)), "offset of G is not finite"),
                        (dict(slope=(float("inf"), 1, 1)), "slope of R is not finite"),
                        (dict(saturation=float("nan")), "saturation is not finite"), (dict(slope=(1, 1)), "three numbers"),
                        (dict(offset="abc"), "three numbers")):
        with pytest.raises(ValueError, match=message):
            Cdl(**kw)
    assert Cdl(slope=(0, 0, 0), saturation=0).slope == (0.0, 0.0, 0.0)          # the edges of the valid range
    c = Cdl.from_sop_text("1.3 1.25 1.1 -0.08 0 0.05 0.8 1 1.2", 0.6)
    assert c == GRADE and Cdl.from_sop_text(c.sop_text(), c.saturation) == c
    assert Cdl.from_sop_text(None, 0.5) == Cdl(saturation=0.5) and Cdl.from_sop_text("1,1,1,0,0,0,1,1,1") == Cdl()
    with pytest.raises(ValueError, match="nine numbers"):
        Cdl.from_sop_text("1 1 1")


# ------------------------------------------------------------------ lutr_cdl_table against the twin's own build
CASES = {"identity": Cdl(), "grade": GRADE, "slope0": Cdl((0, 0, 0), (0.25, 0.5, 1.5), (2.0, 1.0, 0.5)),
         "clamps": Cdl((4, 4, 4), (-1.5, -1.5, -1.5), (1.0, 0.45, 2.2)), "power": Cdl(power=(0.8, 1.2, 2.4))}


@pytest.mark.parametrize("depth", [8, 10, 16])
@pytest.mark.parametrize("name", list(CASES))
def test_the_host_table_is_the_twins(name, depth):
    """Bit-equal where power == 1; elsewhere at most ONE float32 ulp apart: two correctly working double pows may differ in the
    last double bit, which can flip the rounding to float32, and nothing larger is acceptable."""
    c = CASES[name]
    got, want = _native.cdl_table(c, depth), twin.table(c, depth)
    assert got.shape == want.shape == (3, 1 << depth) and got.dtype == np.float32
    for ch in range(3):
        if c.power[ch] == 1.0:
            assert np.array_equal(got[ch], want[ch]), (name, depth, ch)
        else:
            assert int(_ulps(got[ch], want[ch]).max()) <= 1, (name, depth, ch)
    assert np.isfinite(got).all() and got.min() >= 0.0 and got.max() <= 1.0


@pytest.mark.parametrize("depth", [8, 10, 12, 16])
def test_known_answers_of_the_host_table(depth):
    m = (1 << depth) - 1
    k = np.arange(m + 1, dtype=F)
    ident = (k * (F(1.0) / F(m))).astype(F)                          # fl(k * fl(1 / M)), every k
    got = _native.cdl_table(Cdl(), depth)
    assert all(np.array_equal(got[ch], ident) for ch in range(3))
    # slope 0: the constant clamp(offset)^power
    got = _native.cdl_table(CASES["slope0"], depth)
    assert (got[0] == F(0.0625)).all() and (got[1] == F(0.5)).all() and (got[2] == F(1.0)).all()
    # an offset that clamps both ends: 4 x - 1.5 is below 0 up to x = 0.375 and above 1 from x = 0.625
    got = _native.cdl_table(CASES["clamps"], depth)
    lo, hi = int(np.floor(0.37 * m)), int(np.ceil(0.63 * m))
    assert (got[:, :lo] == 0).all() and (got[:, hi:] == 1).all()
    mid = got[0][lo:hi]
    assert mid.min() >= 0 and mid.max() <= 1 and (np.diff(got, axis=1) >= 0).all()
    x = float(ident[m // 2])
    assert got[0][m // 2] == F(4.0 * x - 1.5)                        # power 1: the clamped line itself, rounded once
    # pow(0, p) == 0 for every valid p, and pow(1, p) == 1
    got = _native.cdl_table(Cdl(power=(0.01, 1.2, 7.5)), depth)
    assert (got[:, 0] == 0).all() and (got[:, m] == 1).all()


def test_the_c_entry_refuses_with_a_message():
    lib = _native.load()
    out = (C.c_float * 256)()
    good = _native.cdl_struct(Cdl())
    for args, word in (((None, 8, 0, out), b"null"), ((C.byref(good), 8, 0, None), b"null"), ((C.byref(good), 7, 0, out), b"depth 7"),
                       ((C.byref(good), 17, 0, out), b"depth 17"), ((C.byref(good), 8, 3, out), b"channel 3")):
        assert lib.lutr_cdl_table(*args) == _native.EINVAL and word in lib.lutr_last_error()
    for field, i, value, word in (("slope", 1, float("nan"), b"not finite"), ("slope", 0, -1.0, b"slope of R is negative"),
                                  ("power", 2, 0.0, b"power of B must be above 0"), ("offset", 0, float("inf"), b"not finite")):
        bad = _native.cdl_struct(Cdl())
        getattr(bad, field)[i] = value
        assert lib.lutr_cdl_table(C.byref(bad), 8, 0, out) == _native.EINVAL and word in lib.lutr_last_error(), field
    bad = _native.cdl_struct(Cdl())
    bad.saturation = -0.25
    assert lib.lutr_cdl_table(C.byref(bad), 8, 0, out) == _native.EINVAL and b"saturation is negative" in lib.lutr_last_error()


def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "lutr.h").read_text()
    assert "typedef struct lutr_cdl {" in header
    assert "int lutr_cdl_table(const lutr_cdl *cdl, int depth, int channel, float *out);" in header
    assert "int lutr_apply_yuv_cdl(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, const lutr_cdl *cdl, int w, int h, " \
           "int nframes," in header
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    for sym in ("lutr_cdl_table", "lutr_apply_yuv_cdl"):
        assert sym in _native.SYMBOLS and f" T {sym}\n" in nm
    lib = _native.load()
    assert len(lib.lutr_apply_yuv_cdl.argtypes) == 11 and C.sizeof(_native.CdlStruct) == 40
    # no context, no planes: refused before anything touches a device
    assert lib.lutr_apply_yuv_cdl(None, None, 2, None, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
    assert b"null" in lib.lutr_last_error()


# ------------------------------------------------------------------ the twin pinned to the oracle
@pytest.fixture(scope="module")
def luts(cube_dir):
    return {"log709_33": cube.read_lut(cube_dir / "log709_33.cube"), "random_9": cube.read_lut(cube_dir / "random_9.cube"),
            "domain_2": cube.read_lut(cube_dir / "domain_2.cube")}


@pytest.mark.parametrize("a", list(LAYOUTS))
@pytest.mark.parametrize("b", list(LAYOUTS))
def test_the_identity_cdl_is_the_subsampling_twin_on_every_layout_pair(orc, luts, a, b):
    (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
    src = frames.make_yuv("natural", 37, 11, 10, icsx, icsy, k=3)
    k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, ocsx, ocsy)
    for name, mode in (("log709_33", "tetrahedral"), ("random_9", "trilinear"), ("domain_2", "nearest")):
        lut = luts[name]
        got = twin.apply(lut, Cdl(), mode, k, 10, 10, icsx, icsy, ocsx, ocsy, src)
        assert _eq(got, xsub.apply(lut.table, lut.scale, mode, k, 10, 10, icsx, icsy, ocsx, ocsy, src)), (name, mode)


@pytest.mark.parametrize("depths", [(8, 8, 8), (10, 10, 8), (8, 8, 10), (12, 12, 12), (16, 16, 16), (10, 8, 10)])
def test_the_identity_cdl_is_the_subsampling_twin_at_every_depth_mix(orc, luts, depths):
    din, dl, dout = depths
    prologue = dl != din
    src = frames.make_yuv("uniform", 24, 6, din, 1, 1, k=5, full_range=prologue)
    k = twin.consts("bt709", "tv", "bt709", "tv", din, dl, dout, 1, 0, prologue=prologue)
    lut = luts["random_9"]
    got = twin.apply(lut, Cdl(), "tetrahedral", k, dl, dout, 1, 1, 1, 0, src)
    assert _eq(got, xsub.apply(lut.table, lut.scale, "tetrahedral", k, dl, dout, 1, 1, 1, 0, src))


def test_saturation_0_is_a_source_made_grey_by_hand(luts):
    """sat = 0 feeds the lattice R = G = B = l: the twin's output is the lattice on the luma computed here, one rounded float32
    operation per line, and fed in as three equal planes."""
    lut = luts["random_9"]
    c = Cdl(GRADE.slope, GRADE.offset, GRADE.power, 0.0)
    src = frames.make_yuv("natural", 22, 6, 10, 1, 1, k=8)
    k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 0, 0)
    from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
    r, g, b = yuv_to_rgb_codes(k, 1, 1, src)
    tab = twin.table(c, 10)
    pr = (F(0.2126) * tab[0][r]).astype(F)
    pg = (F(0.7152) * tab[1][g]).astype(F)
    pb = (F(0.0722) * tab[2][b]).astype(F)
    grey = np.clip(((pr + pg).astype(F) + pb).astype(F), F(0), F(1))
    unit = twin.unit_rgb(c, k, 10, 1, 1, src)
    assert all(np.array_equal(u, grey) for u in unit)
    want = rgb_codes_to_yuv(k, 10, 0, 0, twin.lattice_codes(lut, "tetrahedral", 10, [grey, grey, grey]))
    assert _eq(twin.apply(lut, c, "tetrahedral", k, 10, 10, 1, 1, 0, 0, src), want)
    # a grey lattice input makes the three outputs of an identity-like LUT equal too
    q = twin.lattice_codes(cube.CubeLut(2, np.ones(3, F), cube.identity_lattice(2).astype(F)), "trilinear", 10, [grey, grey, grey])
    assert np.array_equal(q[0], q[1]) and np.array_equal(q[1], q[2])


def test_slope_0_feeds_the_lattice_a_constant(luts):
    c = CASES["slope0"]
    src = frames.make_yuv("natural", 16, 4, 10, 1, 1, k=9)
    k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 1, 1)
    unit = twin.unit_rgb(c, k, 10, 1, 1, src)
    assert [float(u.min()) for u in unit] == [float(u.max()) for u in unit] == [0.0625, 0.5, 1.0]
    got = twin.apply(luts["log709_33"], c, "tetrahedral", k, 10, 10, 1, 1, 1, 1, src)
    assert all(len(np.unique(p)) == 1 for p in got)


def test_the_saturation_mix_rounds_every_step(luts):
    """A hand-worked pixel: stage B in Python floats rounded with np.float32 after every operation."""
    t = [np.array([v], F) for v in (0.75, 0.25, 0.5)]
    lum = F(F(F(0.2126) * F(0.75)) + F(F(0.7152) * F(0.25))) + F(F(0.0722) * F(0.5))
    lum = F(lum)
    for sat in (0.0, 0.6, 1.7, 3.0):
        want = [min(max(F(lum + F(F(sat) * F(v[0] - lum))), F(0)), F(1)) for v in t]
        got = twin.saturate(sat, t)
        assert [float(g[0]) for g in got] == [float(w) for w in want], sat
    assert all(g is v for g, v in zip(twin.saturate(1.0, t), t))       # sat == 1: not a single operation


# ------------------------------------------------------------------ refusals, before the engine is touched
def _planes(depth, csx, csy, w=16, h=8, alpha=False):
    dt = torch.uint8 if depth <= 8 else torch.int16
    cs = ((h + (1 << csy) - 1) >> csy, (w + (1 << csx) - 1) >> csx)
    return [torch.zeros((h, w), dtype=dt), torch.zeros(cs, dtype=dt), torch.zeros(cs, dtype=dt)] + \
        ([torch.zeros((h, w), dtype=dt)] if alpha else [])


NAMES = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
#: every refused combination: (options of check_cdl_options, what the message must name)
REFUSALS = [(dict(prelut=True), r"\.csp prelut is not supported with a CDL"),
            (dict(dither="error_diffusion"), r"dither \('error_diffusion'\) is not supported with a CDL"),
            (dict(dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a CDL"),
            (dict(chroma_loc="left"), r"chroma_loc\) is not supported with a CDL"),
            (dict(out_size=(8, 4)), r"resize \(out_size / resolution\) is not supported with a CDL"),
            (dict(out2_pix_fmt="yuv420p"), r"two-output pass \(out2_pix_fmt\) is not supported with a CDL"),
            (dict(lut2=True), r"two-LUT chain \(a second LUT\) is not supported with a CDL"),
            (dict(alpha_mode="premultiplied"), "alpha_mode='premultiplied' is not supported with a CDL"),
            (dict(variant="vec_lds"), "variant vec_lds is not supported with a CDL")]
SIDES = [("nv12", "a semi-planar container"), ("p010le", "a semi-planar container"), ("uyvy422", "a packed container"),
         ("y210le", "a packed container"), ("v210", "a v210 container"), ("gbrp10le", "an RGB format"), ("rgb24", "an RGB format"),
         ("gbrpf32le", "a float RGB format")]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[next(iter(k)) + "-" + str(next(iter(k.values()))) for k, _ in REFUSALS])
def test_check_cdl_options_refuses(kw, message):
    with pytest.raises(ValueError, match=message):
        check_cdl_options(**NAMES, **kw)


@pytest.mark.parametrize("side", ["pix_fmt", "out_pix_fmt"])
@pytest.mark.parametrize("name,word", SIDES)
def test_a_side_that_is_not_planar_yuv_is_a_value_error(side, name, word):
    with pytest.raises(ValueError, match=f"the CDL pass takes planar YUV on both sides: {side} '{name}' is {word}"):
        check_cdl_options(**{**NAMES, side: name})


def test_what_check_cdl_options_takes():
    fin, fout = check_cdl_options(**NAMES)
    assert (fin.name, fout.name) == ("yuv420p10le", "yuv422p10le")
    fin, fout = check_cdl_options("yuva444p10le", "yuva444p10le")          # straight alpha goes through the alpha tail
    assert fin.alpha and fout.alpha
    assert check_cdl_options("yuvj420p")[1].name == "yuv420p"
    for variant in (None, "auto", "generic", "vec_global"):
        check_cdl_options(**NAMES, variant=variant)


def test_the_engine_refuses_before_it_is_touched():
    src = _planes(10, 1, 1)
    for kw, message in ((dict(dither="blue_noise"), "dither"), (dict(dither="error_diffusion"), "dither"),
                        (dict(chroma_loc="left", out_pix_fmt="yuv420p10le"), "chroma_loc"), (dict(out_size=(8, 4)), "resize"),
                        (dict(out_pix_fmt="nv12"), "semi-planar"), (dict(out_pix_fmt="v210"), "v210"),
                        (dict(out_pix_fmt="uyvy422"), "packed")):
        with pytest.raises(ValueError, match=message + ".*|.*CDL"):
            LutEngine.apply_yuv(object(), src, **{**NAMES, **kw}, cdl=GRADE)
    with pytest.raises(ValueError, match="alpha_mode='premultiplied' is not supported with a CDL"):
        LutEngine.apply_yuv(object(), _planes(10, 0, 0, alpha=True), pix_fmt="yuva444p10le", alpha_mode="premultiplied", cdl=GRADE)
    with pytest.raises(ValueError, match="prelut is not supported with a CDL"):
        LutEngine.apply_yuv(SimpleNamespace(_has_prelut=True), src, **NAMES, cdl=GRADE)
    with pytest.raises(TypeError, match="cdl must be a lut_renderer_amd.cdl.Cdl"):
        LutEngine.apply_yuv(object(), src, **NAMES, cdl=(1, 0, 1))


def test_the_group_checks_the_same_things_first():
    from lut_renderer_amd.multigpu import LutEngineGroup
    for kw, message in ((dict(dither="blue_noise"), "dither .* is not supported with a CDL"),
                        (dict(chroma_loc="left"), "chroma_loc\\) is not supported with a CDL"),
                        (dict(alpha_mode="premultiplied", pix_fmt="yuva444p10le", out_pix_fmt="yuv444p10le"), "alpha_mode"),
                        (dict(out_pix_fmt="p010le"), "semi-planar")):
        with pytest.raises(ValueError, match=message):
            LutEngineGroup._apply_yuv(SimpleNamespace(), _planes(10, 1, 1), **{**NAMES, **kw}, cdl=GRADE)
    with pytest.raises(ValueError, match="prelut is not supported with a CDL"):
        LutEngineGroup._apply_yuv(SimpleNamespace(_has_prelut=True), _planes(10, 1, 1), **NAMES, cdl=GRADE)


# ------------------------------------------------------------------ apply_lut(cdl=)
def test_apply_lut_refuses_every_combination_while_planning(tmp_path):
    from lut_renderer_amd.api import apply_lut
    B = cube.CubeLut(2, np.ones(3, F), cube.identity_lattice(2).astype(F))
    y = frames.natural_yuv(16, 8, 10, 1, 1)
    base = dict(cube=None, cdl=GRADE, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", engine=object())
    for kw, message in ((dict(zscale_dither="error_diffusion"), r"dither \('error_diffusion'\) is not supported with a CDL"),
                        (dict(engine_dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a CDL"),
                        (dict(chroma_loc="left"), "chroma_loc.* is not supported with a CDL"),
                        (dict(resolution="8x4"), "resize .* is not supported with a CDL"),
                        (dict(second_pix_fmt="yuv420p"), "two-output pass .* is not supported with a CDL"),
                        (dict(cube2=B), "two-LUT chain .* is not supported with a CDL")):
        with pytest.raises(ValueError, match=message):
            apply_lut(y, **base, **kw)
    for name, word in SIDES[:5]:
        with pytest.raises(ValueError, match=name):          # (a container's own refusal may come first: it names the format too)
            apply_lut(y, **{**base, "out_pix_fmt": name})
    ya = list(y) + [y[0]]
    with pytest.raises(ValueError, match="alpha_mode='premultiplied' is not supported with a CDL"):
        apply_lut(ya, **{**base, "pix_fmt": "yuva420p10le", "out_pix_fmt": "yuva420p10le"}, alpha_mode="premultiplied")
    g, b, r = frames.natural_rgb(16, 8, 8, k=1)
    with pytest.raises(ValueError, match="pix_fmt 'gbrp' is an RGB format"):
        apply_lut((g, b, r), cube=None, cdl=GRADE, pix_fmt="gbrp", out_pix_fmt="yuv420p", engine=object())
    with pytest.raises(ValueError, match="pix_fmt 'gbrpf32le' is a float RGB format"):
        apply_lut([np.zeros((8, 16), F)] * 3, cube=None, cdl=GRADE, pix_fmt="gbrpf32le", engine=object())
    # a LUT with a prelut: told by the parsed LUT, by the file, and by an engine that already holds one
    shapers = [(np.array([0.0, 0.5, 1.0]), np.array([0.0, 0.7, 1.0]))] * 3
    write_csp_with_prelut(tmp_path / "shaped.csp", 2, cube.identity_lattice(2), shapers)
    for cube_arg, eng in ((cube.read_lut(tmp_path / "shaped.csp"), object()), (tmp_path / "shaped.csp", object()),
                          (None, SimpleNamespace(_has_prelut=True))):
        with pytest.raises(ValueError, match=r"\.csp prelut is not supported with a CDL"):
            apply_lut(y, **{**base, "cube": cube_arg, "engine": eng})
    with pytest.raises(ValueError, match="cdl_id names a correction inside a CDL file: it needs cdl"):
        apply_lut(y, cube=None, cdl_id="a001", pix_fmt="yuv420p10le", engine=object())
    with pytest.raises(ValueError, match=r"reel\.ccc: 3 corrections"):
        apply_lut(y, **{**base, "cdl": GOLDEN / "reel.ccc"})


def test_apply_lut_hands_the_engine_the_cdl():
    from lut_renderer_amd.api import apply_lut

    class _Lock:
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    class _Eng:
        _lock, precision, _applied_lut, _has_prelut = _Lock(), "strict", None, False

        def __init__(self): self.calls = []
        def apply_yuv(self, planes, out, **kw): self.calls.append(kw); return out

    eng, y = _Eng(), frames.natural_yuv(16, 8, 10, 1, 1)
    apply_lut(y, cube=None, pix_fmt="yuv420p10le", engine=eng)
    assert "cdl" not in eng.calls[-1]                                 # without cdl: the call it always made
    plain = eng.calls[-1]
    apply_lut(y, cube=None, pix_fmt="yuv420p10le", engine=eng, cdl=GRADE)
    assert eng.calls[-1] == {**plain, "cdl": GRADE}
    apply_lut(y, cube=None, pix_fmt="yuv420p10le", engine=eng, cdl=str(GOLDEN / "reel.ccc"), cdl_id="a002")
    assert eng.calls[-1]["cdl"] == Cdl((0.9, 1.0, 1.2), (-0.02, 0.0, 0.02), (1.2, 1.1, 0.9), 1.7)
    apply_lut(list(y) + [y[0]], cube=None, pix_fmt="yuva420p10le", engine=eng, cdl=GOLDEN / "shot.cc")
    assert eng.calls[-1]["cdl"] == GRADE and eng.calls[-1]["out_pix_fmt"] == "yuva420p10le"
    apply_lut(y, cube=None, pix_fmt="yuv420p10le", color_range="pc", colorspace="bt709", engine=eng, cdl=GRADE)
    assert eng.calls[-1]["lut_depth"] == 8 and eng.calls[-1]["range_src"] == "pc" and eng.calls[-1]["cdl"] == GRADE


# ------------------------------------------------------------------ the CLI
def _args(cube_path, *extra, pix_fmt="yuv420p10le", out="yuv422p10le"):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt, "--out-pix-fmt", out, "--cube",
                                      str(cube_path), *extra])


def test_cli_flags(cube_dir):
    from lut_renderer_amd.cli import cdl_from_args, plan_from_args
    a = cube_dir / "log709_33.cube"
    plain = _args(a)
    assert (plain.cdl, plain.cdl_id, plain.cdl_sop, plain.cdl_sat) == (None, None, None, None) and cdl_from_args(plain) is None
    _, kw, _, _ = plan_from_args(plain)
    assert "cdl" not in kw
    _, kw1, _, _ = plan_from_args(_args(a, "--cdl", str(GOLDEN / "shot.cc")))
    assert kw1 == {**kw, "cdl": GRADE}
    _, kw2, _, _ = plan_from_args(_args(a, "--cdl", str(GOLDEN / "reel.ccc"), "--cdl-id", "a003"))
    assert kw2["cdl"] == Cdl(saturation=0.0)
    _, kw3, _, _ = plan_from_args(_args(a, "--cdl-sop", "1.3 1.25 1.1 -0.08 0 0.05 0.8 1 1.2", "--cdl-sat", "0.6"))
    assert kw3 == kw1
    assert plan_from_args(_args(a, "--cdl-sat", "1.7"))[1]["cdl"] == Cdl(saturation=1.7)
    assert plan_from_args(_args(a, "--cdl-sop", "2 2 2 0 0 0 1 1 1"))[1]["cdl"] == Cdl(slope=(2, 2, 2))
    for extra, message in ((("--cdl", "x.cc", "--cdl-sop", "1 1 1 0 0 0 1 1 1"), "use one or the other"),
                           (("--cdl", "x.cc", "--cdl-sat", "0.5"), "use one or the other"),
                           (("--cdl-id", "a001"), "--cdl-id names a correction inside a CDL file: it needs --cdl"),
                           (("--cdl-sop", "1 1 1"), "nine numbers"), (("--cdl-sop", "1 1 1 0 0 0 1 -1 1"), "power of G"),
                           (("--cdl", str(GOLDEN / "reel.ccc")), "3 corrections"),
                           (("--cdl", str(GOLDEN / "reel.ccc"), "--cdl-id", "nope"), "no <ColorCorrection> with id 'nope'"),
                           (("--cdl", str(GOLDEN / "not_xml.cc")), "not an XML file")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args(a, *extra))


def test_cli_refuses_every_combination_while_planning(cube_dir, tmp_path):
    from lut_renderer_amd.cli import plan_from_args
    a, cc = cube_dir / "log709_33.cube", ("--cdl", str(GOLDEN / "shot.cc"))
    for extra, message in ((("--zscale-dither", "error_diffusion"), r"dither \('error_diffusion'\) is not supported with a CDL"),
                           (("--engine-dither", "blue_noise"), r"dither \('blue_noise'\) is not supported with a CDL"),
                           (("--out-size", "8x4"), "resize .* is not supported with a CDL"),
                           (("--second-output", "c.yuv", "--second-pix-fmt", "yuv420p"), "two-output pass .* not supported with a CDL"),
                           (("--cube2", "look.cube"), "two-LUT chain .* is not supported with a CDL")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args(a, *cc, *extra))
    with pytest.raises(ValueError, match="chroma_loc.* is not supported with a CDL"):
        plan_from_args(_args(a, *cc, "--chroma-loc", "left", out="yuv420p10le"))
    with pytest.raises(ValueError, match="alpha_mode='premultiplied' is not supported with a CDL"):
        plan_from_args(_args(a, *cc, "--alpha-mode", "premultiplied", pix_fmt="yuva444p10le", out="yuv444p10le"))
    for fmt, word in (("gbrp10le", "an RGB format"), ("uyvy422", "packed"), ("nv12", "semi-planar"), ("v210", "v210"),
                      ("gbrpf32le", "a float RGB format")):
        with pytest.raises(ValueError, match=word):
            plan_from_args(_args(a, *cc, pix_fmt=fmt, out="yuv422p10le" if fmt != "nv12" else "yuv420p"))
    shapers = [(np.array([0.0, 0.5, 1.0]), np.array([0.0, 0.7, 1.0]))] * 3
    write_csp_with_prelut(tmp_path / "shaped.csp", 2, cube.identity_lattice(2), shapers)
    with pytest.raises(ValueError, match=r"\.csp prelut is not supported with a CDL"):
        plan_from_args(_args(tmp_path / "shaped.csp", *cc))


def test_planning_with_a_cdl_keeps_one_hip_runtime_in_the_process(cube_dir):
    """Planning parses the LUT to see whether it carries a prelut, which loads liblutr; torch has to be loaded first, or liblutr
    brings a second HIP runtime into the process and the engine made afterwards finds no device."""
    import sys
    code = ("import sys; from lut_renderer_amd import cli; "
            "a = cli.build_parser().parse_args(sys.argv[1:]); cli.plan_from_args(a); "
            "from lut_renderer_amd.engine import LutEngine; "
            "print(len({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}))")
    r = subprocess.run([sys.executable, "-c", code, "-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", "yuv420p10le", "--cube",
                        str(cube_dir / "log709_33.cube"), "--cdl", str(GOLDEN / "shot.cc")], capture_output=True, text=True, cwd=ROOT,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "1", r.stdout + r.stderr


def test_cli_reports_a_bad_cdl_and_makes_no_output(cube_dir, tmp_path, capsys):
    from lut_renderer_amd import cli
    rc = cli.main(["-i", "a", "-o", str(tmp_path / "o.yuv"), "--size", "16x8", "--pix-fmt", "yuv420p10le", "--cube",
                   str(cube_dir / "log709_33.cube"), "--cdl", str(GOLDEN / "bad_two_slopes.cc")])
    assert rc == 1 and "bad_two_slopes.cc: <Slope> holds 2 numbers" in capsys.readouterr().out
    assert not (tmp_path / "o.yuv").exists()


# ------------------------------------------------------------------ the command layer
def test_engine_command_round_trips_the_options():
    from lut_renderer_amd.cli import build_parser, plan_from_args
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.pipe import engine_stage_commands
    params = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")
    info = VideoInfo(width=1920, height=1080, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709",
                     fps=25.0, duration=4.0)

    def cmd(**kw):
        return engine_command(Path("-"), Path("-"), params, Path("show.cube"), info, python_bin="python3", **kw)

    plain = cmd()
    assert not any(a.startswith("--cdl") for a in plain) and cmd(cdl=None, cdl_id=None) == plain
    shot = str(GOLDEN / "shot.cc")
    assert cmd(cdl=Path(shot)) == plain + ["--cdl", shot] == cmd(cdl=shot)
    reel = cmd(cdl=GOLDEN / "reel.ccc", cdl_id="a002")
    assert reel == plain + ["--cdl", str(GOLDEN / "reel.ccc"), "--cdl-id", "a002"]
    lit = cmd(cdl=GRADE)
    assert lit[:len(plain)] == plain and lit[len(plain)] == "--cdl-sop" and lit[len(plain) + 2:] == ["--cdl-sat", "0.6"]
    assert cmd(cdl=Cdl(slope=(2, 2, 2)))[len(plain):] == ["--cdl-sop", "2.0 2.0 2.0 0.0 0.0 0.0 1.0 1.0 1.0"]
    # the CLI resolves what the command rendered, to the same values
    odd = Cdl((1 / 3, 1.1, 0.7), (-1e-3, 1 / 7, 0.0), (0.45, 2.4, 1.0), 1 / 9)
    for c, argv in ((GRADE, lit), (odd, cmd(cdl=odd)), (GRADE, cmd(cdl=shot)), (Cdl((0.9, 1.0, 1.2), (-0.02, 0.0, 0.02), (1.2, 1.1, 0.9), 1.7), reel)):
        assert plan_from_args(build_parser().parse_args(argv[3:]))[1]["cdl"] == c
    for kwargs, message in ((dict(cdl_id="a001"), "it needs cdl"), (dict(cdl=GRADE, cdl_id="a001"), "cdl is a set of values"),
                            (dict(cdl=GRADE, chroma_loc="left"), "chroma_loc"),
                            (dict(cdl=GRADE, engine_dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a CDL"),
                            (dict(cdl=GRADE, cube2=Path("l.cube")), "two-LUT chain .* is not supported with a CDL"),
                            (dict(cdl=GRADE, second_output=Path("d.yuv"), second_pix_fmt="yuv420p"), "two-output pass"),
                            (dict(cdl=shot, alpha_mode="premultiplied"), "alpha")):
        with pytest.raises(ValueError, match=message):
            cmd(**kwargs)
    with pytest.raises(TypeError, match="cdl must be a Cdl or the path"):
        cmd(cdl=1.5)
    sized = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le", resolution="1280x720")
    with pytest.raises(ValueError, match="resize .* is not supported with a CDL"):
        engine_command(Path("-"), Path("-"), sized, Path("show.cube"), info, python_bin="python3", gpu_resize=True, cdl=GRADE)
    rgb = VideoInfo(width=64, height=32, bit_depth=8, pix_fmt="rgb24", fps=25.0)
    with pytest.raises(ValueError, match="pix_fmt 'rgb24' is an RGB format"):
        engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx264", pix_fmt="yuv420p"), Path("show.cube"), rgb,
                       python_bin="python3", cdl=GRADE)
    # the three-process stage: only the engine's argv changes
    base = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, Path("show.cube"), info, python_bin="python3")
    assert engine_stage_commands(Path("in.mov"), Path("out.mov"), params, Path("show.cube"), info, python_bin="python3", cdl=None) == base
    staged = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, Path("show.cube"), info, python_bin="python3",
                                   cdl=GOLDEN / "reel.ccc", cdl_id="a001")
    assert (staged.decoder, staged.encoder) == (base.decoder, base.encoder)
    i = staged.engine.index("--cdl")
    assert staged.engine[i:i + 4] == ["--cdl", str(GOLDEN / "reel.ccc"), "--cdl-id", "a001"]
    assert staged.engine[:i] + staged.engine[i + 4:] == base.engine


def test_host_pipeline_checks_a_cdl_before_it_allocates():
    from lut_renderer_amd.stream import HostPipeline
    for kw, message in ((dict(out_pix_fmt="nv12"), "semi-planar"), (dict(second_pix_fmt="yuv420p"), "two-output pass"),
                        (dict(out_size=(8, 4)), "resize"), (dict(dither="blue_noise"), "dither"), (dict(chain=True), "two-LUT chain"),
                        (dict(chroma_loc="center"), "chroma_loc")):
        with pytest.raises(ValueError, match=message):
            HostPipeline(SimpleNamespace(), "yuv420p10le", 16, 8, cdl=GRADE, **kw)
    with pytest.raises(ValueError, match="an RGB format"):
        HostPipeline(SimpleNamespace(), "rgb24", 16, 8, out_pix_fmt="yuv420p", cdl=GRADE)
    with pytest.raises(ValueError, match="prelut is not supported with a CDL"):
        HostPipeline(SimpleNamespace(_has_prelut=True), "yuv420p10le", 16, 8, cdl=GRADE)
