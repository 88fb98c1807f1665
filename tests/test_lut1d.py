"""1D LUT files without a GPU: the reader on fixtures and refusals, lutr_lut1d_table against the NumPy formulas of
tests/_lut1d_twin.py entry for entry, identity and clipping, the one copy of the option refusals through every layer, and the
twin's anchors to the existing contract."""
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.formats import check_lut1d_options
from tests import _lut1d_twin as twin
from tests import _xsub_twin as xs

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "lut1d"
F = np.float32
FIXTURES = ("curve17", "gamma1024", "invert33", "range64")
EXACT_MODES = ("nearest", "linear", "cubic", "spline")
DEPTHS = (8, 10, 12, 16)


def _write(path, text):
    path.write_text(text)
    return path


def _rows(n, f=lambda v: (v, v, v)):
    return "".join("%.9g %.9g %.9g\n" % tuple(f(i / (n - 1))) for i in range(n))


def _parse_fails(path, code, *words):
    with pytest.raises(_native.LutrError) as e:
        cube.read_lut1d(path)
    assert e.value.code == code, e.value.message
    assert Path(path).name in e.value.message, e.value.message
    for w in words:
        assert w in e.value.message, e.value.message


# ------------------------------------------------------------------ the reader
def test_fixtures_size_and_scale():
    c = cube.read_lut1d(GOLDEN / "curve17.cube")
    assert c.n == 17 and c.table.shape == (3, 17) and c.table.dtype == F
    # DOMAIN_MAX 1 0.9 1.1: 1 / 0.9 clips to 1, 1 / 1.1 in double rounded to float
    assert c.scale.tolist() == [1.0, 1.0, float(F(1.0 / float(F(1.1) - F(0.0))))]
    assert c.table[0, 0] == 0 and c.table[1, 0] == F(0.05) and c.table[2, 16] == 1
    g = cube.read_lut1d(GOLDEN / "gamma1024.cube")
    assert g.n == 1024 and g.scale.tolist() == [1.0, 1.0, 1.0]
    assert g.table.min() < 0 and g.table.max() > 1                    # the under- and overshoot are kept as written
    i = cube.read_lut1d(GOLDEN / "invert33.cube")
    assert i.n == 33 and i.table[0, 0] == 1 and i.table[0, 32] == 0
    r = cube.read_lut1d(GOLDEN / "range64.cube")
    assert r.n == 64 and r.scale.tolist() == [1.0] * 3                # 1 / (0.9 - 0.1) = 1.25 clips to 1


def test_domain_and_input_range_arithmetic(tmp_path):
    # the subtraction is in float: (float)1.9 - (float)0.3, then the division in double, then the clip in float
    p = _write(tmp_path / "d.cube", "LUT_1D_SIZE 2\nDOMAIN_MIN 0.3 0.3 0.3\nDOMAIN_MAX 1.9 1.9 3.3\n0 0 0\n1 1 1\n")
    s = cube.read_lut1d(p).scale
    assert s[0] == F(1.0 / float(F(1.9) - F(0.3))) and s[2] == F(1.0 / float(F(3.3) - F(0.3)))
    assert s[0] != F(1.0 / (1.9 - 0.3)) or F(1.9) - F(0.3) == F(1.9 - 0.3)
    p = _write(tmp_path / "r.cube", "LUT_1D_SIZE 2\nLUT_1D_INPUT_RANGE -1 3\n0 0 0\n1 1 1\n")
    assert cube.read_lut1d(p).scale.tolist() == [0.25] * 3
    # DOMAIN_ lines count between the size line and the last row only; the last one wins
    p = _write(tmp_path / "o.cube", "DOMAIN_MAX 4 4 4\nLUT_1D_SIZE 3\n0 0 0\nDOMAIN_MAX 2 2 2\n.5 .5 .5\n1 1 1\nDOMAIN_MAX 8 8 8\n")
    assert cube.read_lut1d(p).scale.tolist() == [0.5] * 3
    # comments, blank lines, TITLE, CRLF
    p = _write(tmp_path / "c.cube", "# a\r\nTITLE \"x\"\r\n\r\nLUT_1D_SIZE 2\r\n# b\r\n\r\nTITLE \"y\"\r\n0 0.5 1\r\n1 0.5 0\r\n")
    assert cube.read_lut1d(p).table.tolist() == [[0, 1], [0.5, 0.5], [1, 0]]
    # a min above the max: a negative ratio clips to 0
    p = _write(tmp_path / "n.cube", "LUT_1D_SIZE 2\nLUT_1D_INPUT_RANGE 1 0\n0 0 0\n1 1 1\n")
    assert cube.read_lut1d(p).scale.tolist() == [0.0] * 3


def test_every_refusal_names_the_file(tmp_path):
    _parse_fails(_write(tmp_path / "both.cube", "LUT_1D_SIZE 2\nLUT_1D_INPUT_RANGE 0 1\nLUT_3D_SIZE 2\n" + _rows(2) + _rows(8)),
                 _native.EINVAL, "LUT_1D_SIZE and LUT_3D_SIZE")
    _parse_fails(_write(tmp_path / "both2.cube", "LUT_3D_SIZE 2\nLUT_1D_SIZE 2\n" + _rows(2) + _rows(8)), _native.EINVAL, "LUT_3D_SIZE")
    _parse_fails(_write(tmp_path / "both3.cube", "LUT_1D_SIZE 2\n" + _rows(2) + "LUT_3D_SIZE 2\n" + _rows(8)), _native.EINVAL,
                 "LUT_3D_SIZE")
    _parse_fails(_write(tmp_path / "short.cube", "LUT_1D_SIZE 5\n" + _rows(4)), _native.EILSEQ, "EOF after 4 of 5 rows")
    _parse_fails(_write(tmp_path / "two.cube", "LUT_1D_SIZE 3\n0 0 0\n0.5 0.5\n1 1 1\n"), _native.EILSEQ, "row 1", "three numbers")
    _parse_fails(_write(tmp_path / "nan.cube", "LUT_1D_SIZE 2\n0 nan 0\n1 1 1\n"), _native.EILSEQ, "non-finite")
    _parse_fails(_write(tmp_path / "inf.cube", "LUT_1D_SIZE 2\n0 0 0\n1 inf 1\n"), _native.EILSEQ, "non-finite")
    _parse_fails(_write(tmp_path / "small.cube", "LUT_1D_SIZE 1\n0 0 0\n"), _native.EINVAL, "invalid 1D LUT size 1")
    _parse_fails(_write(tmp_path / "big.cube", "LUT_1D_SIZE 65537\n"), _native.EINVAL, "invalid 1D LUT size 65537")
    _parse_fails(_write(tmp_path / "none.cube", "TITLE \"x\"\n0 0 0\n"), _native.EILSEQ, "no LUT_1D_SIZE")
    _parse_fails(_write(tmp_path / "dom.cube", "LUT_1D_SIZE 2\nDOMAIN_MID 0 0 0\n0 0 0\n1 1 1\n"), _native.EILSEQ, "DOMAIN_")
    _parse_fails(tmp_path / "absent.cube", _native.ENOENT, "cannot open")
    _parse_fails(_write(tmp_path / "x.dat", "LUT_1D_SIZE 2\n0 0 0\n1 1 1\n"), _native.EINVAL, "extension")
    # a 3D file is not a 1D one, and a 1D file is still not a 3D one
    cube.write_cube(tmp_path / "three.cube", cube.identity_lattice(2))
    _parse_fails(tmp_path / "three.cube", _native.EINVAL, "3D LUT")
    for reader in (cube.read_lut, cube.read_cube):
        with pytest.raises(_native.LutrError) as e:
            reader(GOLDEN / "curve17.cube")
        assert e.value.code == _native.EILSEQ and "no LUT_3D_SIZE" in e.value.message


def test_hostile_input_is_an_error_not_a_crash(tmp_path):
    good = "LUT_1D_SIZE 4\n" + _rows(4)
    for k, cut in enumerate((5, 13, 20, len(good) - 3)):
        p = tmp_path / f"cut{k}.cube"
        p.write_bytes(good.encode()[:cut])
        with pytest.raises(_native.LutrError):
            cube.read_lut1d(p)
    (tmp_path / "garbage.cube").write_bytes(bytes(np.random.default_rng(1).integers(0, 256, 4096, dtype=np.uint8)))
    (tmp_path / "nul.cube").write_bytes(b"LUT_1D_SIZE 3\n0 0 0\n\x00\x00\x000.5 \x00 0.5 0.5\n1 1 1\n")
    (tmp_path / "long.cube").write_bytes(b"LUT_1D_SIZE 2\n" + b"7" * 70000 + b"\n1 1 1\n")
    (tmp_path / "longsize.cube").write_bytes(b"LUT_1D_SIZE " + b"9" * 70000 + b"\n")
    (tmp_path / "empty.cube").write_bytes(b"")
    for name in ("garbage", "nul", "long", "longsize", "empty"):
        with pytest.raises(_native.LutrError) as e:
            cube.read_lut1d(tmp_path / f"{name}.cube")
        assert f"{name}.cube" in e.value.message
    # 65536 rows is the largest file
    big = cube.write_lut1d(tmp_path / "max.cube", np.tile(np.linspace(0, 1, 65536, dtype=F), (3, 1)))
    assert cube.read_lut1d(big).n == 65536


# ------------------------------------------------------------------ the table
def _tables(n):
    rng = np.random.default_rng(n)
    if n == 2:
        return np.array([[0.1, 0.9], [1.0, 0.0], [-0.1, 1.2]], F)
    x = np.linspace(0, 1, n)
    return (np.stack([x ** 0.45, 1 - x ** 2, x]) + rng.normal(0, 0.01, (3, n))).astype(F)


@pytest.mark.parametrize("n", [2, 17, 1024, 65536])
def test_table_equals_the_twin_entry_for_entry(n, tmp_path):
    """A file of n rows written and read back, three different scales: nearest, linear, cubic and spline, every depth and channel."""
    p = cube.write_lut1d(tmp_path / "t.cube", _tables(n), domain_min=(0, 0, 0), domain_max=(1, 1.25, 3))
    l1 = cube.read_lut1d(p)
    assert l1.n == n and l1.scale.tolist() == [1.0, float(F(0.8)), float(F(1.0 / 3.0))]
    for mode in EXACT_MODES:
        for depth in DEPTHS:
            got, want = _native.lut1d_table(l1, mode, depth), twin.table(l1.table, l1.scale, mode, depth)
            assert got.dtype == np.uint16 and got.shape == (3, 1 << depth)
            assert np.array_equal(got, want), (n, mode, depth, int((got != want).sum()))


@pytest.mark.parametrize("name", FIXTURES)
def test_table_of_every_fixture(name, capsys):
    l1 = cube.read_lut1d(GOLDEN / f"{name}.cube")
    for depth in DEPTHS:
        for mode in EXACT_MODES:
            assert np.array_equal(_native.lut1d_table(l1, mode, depth), twin.table(l1.table, l1.scale, mode, depth)), (mode, depth)
        # cosine: two faithfully rounded cosf move v * factor by a few ulp of a value below 2^16, far below one code
        got, want = _native.lut1d_table(l1, "cosine", depth).astype(np.int64), twin.table(l1.table, l1.scale, "cosine", depth)
        with capsys.disabled():
            print(f"\n  cosine {name} at {depth} bit: {int((got != want).sum())} of {got.size} entries differ from NumPy's cos", end="")
        assert np.abs(got - want).max() <= 1, (name, depth)


def test_identity_and_clipping():
    for depth in range(8, 17):
        m = (1 << depth) - 1
        ident = _native.lut1d_table(cube.Lut1D.identity(m + 1), "linear", depth)
        assert np.array_equal(ident, np.tile(np.arange(m + 1, dtype=np.uint16), (3, 1))), depth
    rng = np.random.default_rng(5)
    for n in (2, 17, 1000):
        tab = rng.uniform(0.1, 0.9, (3, n)).astype(F)
        tab[:, -1] = [0.25, 0.5, 0.75]
        l1 = cube.Lut1D(tab, np.ones(3, F))
        for depth in DEPTHS:
            m = (1 << depth) - 1
            for mode in twin.MODES:            # the last code reads node n - 1 exactly: mu == 0 there
                t = _native.lut1d_table(l1, mode, depth)
                assert t[:, m].tolist() == [int(F(v) * F(m)) for v in (0.25, 0.5, 0.75)], (n, depth, mode)
                assert t[:, 0].tolist() == [int(F(v) * F(m)) for v in tab[:, 0]], (n, depth, mode)
    out = cube.Lut1D(np.array([[-0.5, 1.5], [-1e30, 1e30], [2.0, -3.0]], F), np.ones(3, F))
    for depth in DEPTHS:
        m = (1 << depth) - 1
        for mode in ("nearest", "linear", "cosine"):
            t = _native.lut1d_table(out, mode, depth)
            assert t[0, 0] == 0 and t[0, m] == m and t[1, 0] == 0 and t[1, m] == m and t[2, 0] == m and t[2, m] == 0
            assert set(np.unique(t[1])) <= {0, m}


def test_table_refuses_bad_arguments():
    l1 = cube.Lut1D.identity(4)
    with pytest.raises(ValueError, match="unknown interp1d 'bicubic'"):
        _native.lut1d_table(l1, "bicubic", 10)
    lib = _native.load()
    import ctypes as C
    tab = np.ascontiguousarray(l1.table)
    ptr, sc = tab.ctypes.data_as(C.POINTER(C.c_float)), (C.c_float * 3)(1, 1, 1)
    out = np.zeros(65536, np.uint16)
    o = out.ctypes.data_as(C.POINTER(C.c_uint16))
    for args, word in (((None, 4, sc, 1, 10, 0, o), "null"), ((ptr, 1, sc, 1, 10, 0, o), "size 1"), ((ptr, 65537, sc, 1, 10, 0, o), "size"),
                       ((ptr, 4, sc, 5, 10, 0, o), "mode 5"), ((ptr, 4, sc, -1, 10, 0, o), "mode -1"), ((ptr, 4, sc, 1, 7, 0, o), "depth 7"),
                       ((ptr, 4, sc, 1, 17, 0, o), "depth 17"), ((ptr, 4, sc, 1, 10, 3, o), "channel 3"),
                       ((ptr, 4, (C.c_float * 3)(2, 1, 1), 1, 10, 0, o), "scale[0]"), ((ptr, 4, sc, 1, 10, 0, None), "null")):
        assert lib.lutr_lut1d_table(*args) == _native.EINVAL
        assert word in lib.lutr_last_error().decode(), (word, lib.lutr_last_error().decode())
    bad = tab.copy()
    bad[1, 2] = np.nan
    assert lib.lutr_lut1d_table(bad.ctypes.data_as(C.POINTER(C.c_float)), 4, sc, 1, 10, 1, o) == _native.EINVAL
    assert "not finite" in lib.lutr_last_error().decode()
    assert lib.lutr_lut1d_table(bad.ctypes.data_as(C.POINTER(C.c_float)), 4, sc, 1, 10, 0, o) == 0     # (channel 0 is fine)
    with pytest.raises(ValueError, match="expected \\(3, n\\)"):
        cube.Lut1D(np.zeros((3, 1), F), np.ones(3, F))


def test_abi_lists_the_new_entry_points():
    for sym in ("lutr_lut1d_parse", "lutr_lut1d_table", "lutr_ctx_set_lut1d", "lutr_apply_yuv_lut1d", "lutr_apply_planar_rgb_lut1d"):
        assert sym in _native.SYMBOLS and hasattr(_native.load(), sym)
    header = (ROOT / "include" / "lutr.h").read_text()
    for name, code in _native.INTERP1D.items():
        assert f"LUTR_INTERP1D_{name.upper()}" in header and f"= {code}" in header


# ------------------------------------------------------------------ host plumbing: one copy of the refusals
NAMES = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
REFUSALS = [(dict(dither="error_diffusion"), r"dither \('error_diffusion'\) is not supported with a 1D LUT"),
            (dict(dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a 1D LUT"),
            (dict(chroma_loc="left"), r"chroma_loc\) is not supported with a 1D LUT"),
            (dict(out_size=(8, 4)), r"resize \(out_size / resolution\) is not supported with a 1D LUT"),
            (dict(cdl=True), "a CDL is not supported with a 1D LUT"),
            (dict(lut2=True), r"two-LUT chain \(a second LUT\) is not supported with a 1D LUT"),
            (dict(out2_pix_fmt="yuv420p"), r"two-output pass \(out2_pix_fmt\) is not supported with a 1D LUT"),
            (dict(alpha_mode="premultiplied"), "alpha_mode='premultiplied' is not supported with a 1D LUT"),
            (dict(variant="vec_lds"), "variant vec_lds is not supported with a 1D LUT"),
            (dict(interp1d="bicubic"), "lut1d has no interpolation mode 'bicubic'"),
            (dict(loaded=False), "no 1D LUT is loaded")]
SIDES = [("nv12", "a semi-planar container"), ("p010le", "a semi-planar container"), ("uyvy422", "a packed container"),
         ("y210le", "a packed container"), ("v210", "a v210 container"), ("gbrp10le", "an RGB format"), ("rgb24", "an RGB format"),
         ("gbrpf32le", "a float RGB format")]


def _planes(depth, csx, csy, alpha=False):
    import torch
    y = frames.natural_yuv(16, 8, depth, csx, csy)
    return [torch.from_numpy(p.view(np.int16)) for p in (list(y) + ([y[0]] if alpha else []))]


@pytest.mark.parametrize("kw,message", REFUSALS, ids=[next(iter(k)) + "-" + str(next(iter(k.values()))) for k, _ in REFUSALS])
def test_check_lut1d_options_refuses(kw, message):
    with pytest.raises(ValueError, match=message):
        check_lut1d_options(**NAMES, **kw)


@pytest.mark.parametrize("name,word", SIDES)
def test_a_side_that_is_not_planar_yuv_is_a_value_error(name, word):
    with pytest.raises(ValueError, match=f"the lut1d pass takes planar YUV on both sides: out_pix_fmt '{name}' is {word}"):
        check_lut1d_options("yuv422p10le", name)
    with pytest.raises(ValueError, match=f"pix_fmt '{name}' is {word}"):
        check_lut1d_options(name, None)
    if "RGB" in word:
        with pytest.raises(ValueError, match="an RGB source with a YUV output .* is not supported with a 1D LUT"):
            check_lut1d_options(name, "yuv420p")


def test_what_check_lut1d_options_takes():
    fin, fout = check_lut1d_options(**NAMES)
    assert (fin.name, fout.name) == ("yuv420p10le", "yuv422p10le")
    fin, fout = check_lut1d_options("yuva444p10le", "yuva444p10le")         # straight alpha goes through the alpha tail
    assert fin.alpha and fout.alpha
    assert check_lut1d_options("yuvj420p")[1].name == "yuv420p"
    for mode in _native.INTERP1D:
        check_lut1d_options(**NAMES, interp1d=mode)
    for variant in (None, "auto", "generic", "vec_global"):
        check_lut1d_options(**NAMES, variant=variant)


def test_the_engine_refuses_before_it_is_touched():
    src = _planes(10, 1, 1)
    held = SimpleNamespace(n1d=17)
    for kw, message in ((dict(dither="blue_noise"), "dither"), (dict(chroma_loc="left"), "chroma_loc"), (dict(out_size=(8, 4)), "resize"),
                        (dict(cdl=object()), "a CDL"), (dict(cube2="b.cube"), "two-LUT chain"), (dict(out2_pix_fmt="yuv420p"), "two-output"),
                        (dict(alpha_mode="premultiplied"), "alpha_mode"), (dict(out_pix_fmt="nv12"), "semi-planar"),
                        (dict(out_pix_fmt="v210"), "v210"), (dict(out_pix_fmt="uyvy422"), "packed"), (dict(pix_fmt="gbrp10le"), "RGB")):
        with pytest.raises(ValueError, match=message):
            LutEngine.apply_yuv_lut1d(held, src, **{**NAMES, **kw})
    with pytest.raises(ValueError, match="no 1D LUT is loaded"):
        LutEngine.apply_yuv_lut1d(object(), src, **NAMES)
    with pytest.raises(ValueError, match="lut3d has no interpolation mode 'cubic'"):
        LutEngine.apply_yuv_lut1d(held, src, **NAMES, interp="cubic")
    with pytest.raises(TypeError, match="unexpected keyword argument 'gamma'"):
        LutEngine.apply_yuv_lut1d(held, src, **NAMES, gamma=2.2)
    with pytest.raises(ValueError, match="no 1D LUT is loaded"):
        LutEngine.apply_rgb_lut1d(object(), src[:1] * 3, depth=10)
    with pytest.raises(ValueError, match="unsupported depth 7"):
        LutEngine.apply_rgb_lut1d(held, src[:1] * 3, depth=7)
    with pytest.raises(ValueError, match="unknown interp1d 'bicubic'"):
        LutEngine.set_lut1d(object(), cube.Lut1D.identity(4), "bicubic")
    with pytest.raises(TypeError, match="lut1d must be a lut_renderer_amd.cube.Lut1D"):
        LutEngine.set_lut1d(object(), "tech.cube")


def test_the_group_checks_the_same_things_first():
    import threading
    from lut_renderer_amd.multigpu import LutEngineGroup
    g = SimpleNamespace(_lock=threading.RLock(), n1d=17)
    for kw, message in ((dict(dither="blue_noise"), "dither .* is not supported with a 1D LUT"),
                        (dict(chroma_loc="left"), "chroma_loc\\) is not supported with a 1D LUT"), (dict(cdl=object()), "a CDL"),
                        (dict(out_pix_fmt="p010le"), "semi-planar"), (dict(row0=0), "the group owns the row partition")):
        with pytest.raises(ValueError, match=message):
            LutEngineGroup.apply_yuv_lut1d(g, _planes(10, 1, 1), **{**NAMES, **kw})
    with pytest.raises(ValueError, match="no 1D LUT is loaded"):
        LutEngineGroup.apply_yuv_lut1d(SimpleNamespace(_lock=threading.RLock(), n1d=0), _planes(10, 1, 1), **NAMES)


def test_apply_lut_refuses_every_combination_while_planning():
    from lut_renderer_amd.api import apply_lut
    from lut_renderer_amd.cdl import Cdl
    B = cube.CubeLut(2, np.ones(3, F), cube.identity_lattice(2).astype(F))
    y = frames.natural_yuv(16, 8, 10, 1, 1)
    base = dict(cube=None, lut1d=cube.Lut1D.identity(4), pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", engine=object())
    for kw, message in ((dict(zscale_dither="error_diffusion"), r"dither \('error_diffusion'\) is not supported with a 1D LUT"),
                        (dict(engine_dither="blue_noise"), r"dither \('blue_noise'\) is not supported with a 1D LUT"),
                        (dict(chroma_loc="left"), "chroma_loc.* is not supported with a 1D LUT"),
                        (dict(resolution="8x4"), "resize .* is not supported with a 1D LUT"),
                        (dict(cdl=Cdl()), "a CDL is not supported with a 1D LUT"),
                        (dict(second_pix_fmt="yuv420p"), "two-output pass .* is not supported with a 1D LUT"),
                        (dict(cube2=B), "two-LUT chain .* is not supported with a 1D LUT"),
                        (dict(interp1d="bicubic"), "lut1d has no interpolation mode 'bicubic'")):
        with pytest.raises(ValueError, match=message):
            apply_lut(y, **base, **kw)
    for name, _ in SIDES[:5]:
        with pytest.raises(ValueError, match=name):          # (a container's own refusal may come first: it names the format too)
            apply_lut(y, **{**base, "out_pix_fmt": name})
    ya = list(y) + [y[0]]
    with pytest.raises(ValueError, match="alpha_mode='premultiplied' is not supported with a 1D LUT"):
        apply_lut(ya, **{**base, "pix_fmt": "yuva420p10le", "out_pix_fmt": "yuva420p10le"}, alpha_mode="premultiplied")
    g, b, r = frames.natural_rgb(16, 8, 8, k=1)
    with pytest.raises(ValueError, match="an RGB source with a YUV output .* is not supported with a 1D LUT"):
        apply_lut((g, b, r), **{**base, "pix_fmt": "gbrp", "out_pix_fmt": "yuv420p"})
    with pytest.raises(ValueError, match="pix_fmt 'gbrpf32le' is a float RGB format"):
        apply_lut([np.zeros((8, 16), F)] * 3, **{**base, "pix_fmt": "gbrpf32le", "out_pix_fmt": None})
    with pytest.raises(TypeError, match="lut1d must be a Lut1D or the path"):
        apply_lut(y, **{**base, "lut1d": 3})
    with pytest.raises(_native.LutrError, match="absent.cube"):
        apply_lut(y, **{**base, "lut1d": GOLDEN / "absent.cube"})


def test_apply_lut_hands_the_engine_the_1d_lut():
    from lut_renderer_amd.api import apply_lut

    class _Lock:
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    class _Eng:
        _lock, precision, _applied_lut, _applied_lut1d, _has_prelut = _Lock(), "strict", None, None, False

        def __init__(self): self.calls, self.sets = [], []
        def apply_yuv(self, planes, out, **kw): self.calls.append(("yuv", kw)); return out
        def apply_yuv_lut1d(self, planes, out, **kw): self.calls.append(("lut1d", kw)); return out
        def set_lut1d(self, l1, mode): self.sets.append((l1, mode))
        def set_lut(self, lut): pass

    eng, y = _Eng(), frames.natural_yuv(16, 8, 10, 1, 1)
    apply_lut(y, cube=None, pix_fmt="yuv420p10le", engine=eng)
    assert eng.calls[-1][0] == "yuv" and not eng.sets                 # without lut1d: the call it always made
    plain = {k: v for k, v in eng.calls[-1][1].items() if k != "dither"}
    l1 = cube.Lut1D.identity(16)
    apply_lut(y, cube=None, pix_fmt="yuv420p10le", engine=eng, lut1d=l1)
    assert eng.calls[-1] == ("lut1d", {**plain, "interp": None}) and eng.sets == [(l1, "linear")]      # cube=None: lut1d alone
    apply_lut(y, cube=None, pix_fmt="yuv420p10le", engine=eng, lut1d=l1)
    assert len(eng.sets) == 1                                         # the same object and mode: the device copy stands
    apply_lut(y, cube=None, pix_fmt="yuv420p10le", engine=eng, lut1d=l1, interp1d="cubic")
    assert eng.sets[-1] == (l1, "cubic")
    B = cube.CubeLut(2, np.ones(3, F), cube.identity_lattice(2).astype(F))
    apply_lut(y, cube=B, interp="trilinear", pix_fmt="yuv420p10le", engine=eng, lut1d=GOLDEN / "curve17.cube")
    assert eng.calls[-1] == ("lut1d", {**plain, "interp": "trilinear"}) and eng.sets[-1][0].n == 17
    apply_lut(list(y) + [y[0]], cube=B, pix_fmt="yuva420p10le", engine=eng, lut1d=l1)
    assert eng.calls[-1][1]["out_pix_fmt"] == "yuva420p10le"
    apply_lut(y, cube=B, pix_fmt="yuv420p10le", color_range="pc", colorspace="bt709", engine=eng, lut1d=l1)
    assert eng.calls[-1][1]["lut_depth"] == 8 and eng.calls[-1][1]["range_src"] == "pc"


# ------------------------------------------------------------------ the CLI and the argv
def _args(*extra, pix_fmt="yuv420p10le", out="yuv422p10le"):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt, "--out-pix-fmt", out, *extra])


def test_cli_flags(cube_dir):
    from lut_renderer_amd.cli import plan_from_args
    a, t = str(cube_dir / "log709_33.cube"), str(GOLDEN / "curve17.cube")
    plain = _args("--cube", a)
    assert (plain.lut1d, plain.interp1d) == (None, "linear")
    _, kw, _, _ = plan_from_args(plain)
    _, kw1, _, _ = plan_from_args(_args("--cube", a, "--lut1d", t, "--interp1d", "spline"))
    assert kw1 == kw                                                   # (the 1D LUT is engine state: HostPipeline(lut1d=True))
    _, kw2, _, _ = plan_from_args(_args("--lut1d", t))
    assert kw2 == {**kw, "interp": None}                               # no --cube: lut1d alone
    with pytest.raises(ValueError, match="--cube is required unless --lut1d is given"):
        plan_from_args(_args())
    for extra, message in ((("--zscale-dither", "error_diffusion"), r"dither \('error_diffusion'\) is not supported with a 1D LUT"),
                           (("--engine-dither", "blue_noise"), r"dither \('blue_noise'\) is not supported with a 1D LUT"),
                           (("--out-size", "8x4"), "resize .* is not supported with a 1D LUT"),
                           (("--cdl-sat", "0.5"), "a CDL is not supported with a 1D LUT"),
                           (("--second-output", "c.yuv", "--second-pix-fmt", "yuv420p"), "two-output pass .* not supported with a 1D LUT"),
                           (("--cube2", "look.cube"), "two-LUT chain .* is not supported with a 1D LUT"),
                           (("--interp1d", "bicubic"), "lut1d has no interpolation mode 'bicubic'")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args("--cube", a, "--lut1d", t, *extra))
    with pytest.raises(ValueError, match="chroma_loc.* is not supported with a 1D LUT"):
        plan_from_args(_args("--cube", a, "--lut1d", t, "--chroma-loc", "left", out="yuv420p10le"))
    with pytest.raises(ValueError, match="alpha_mode='premultiplied' is not supported with a 1D LUT"):
        plan_from_args(_args("--cube", a, "--lut1d", t, "--alpha-mode", "premultiplied", pix_fmt="yuva444p10le", out="yuv444p10le"))
    with pytest.raises(ValueError, match="an RGB source with a YUV output"):
        plan_from_args(_args("--cube", a, "--lut1d", t, pix_fmt="gbrp10le", out="yuv420p10le"))


def test_cli_without_cube_and_without_lut1d_exits_2(tmp_path):
    r = subprocess.run([sys.executable, "-m", "lut_renderer_amd.cli", "-i", str(tmp_path / "a.yuv"), "-o", str(tmp_path / "b.yuv"),
                        "--size", "16x8", "--pix-fmt", "yuv420p"], capture_output=True, cwd=ROOT, timeout=120)
    assert r.returncode == 2 and b"--cube" in r.stderr and not (tmp_path / "b.yuv").exists()


def test_engine_command_renders_the_two_flags(cube_dir):
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    from lut_renderer_amd.pipe import engine_stage_commands
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    params = ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le")
    a, t = cube_dir / "log709_33.cube", GOLDEN / "curve17.cube"
    plain = engine_command(Path("-"), Path("-"), params, a, info)
    assert "--lut1d" not in plain and "--interp1d" not in plain
    assert engine_command(Path("-"), Path("-"), params, a, info, lut1d=t) == plain + ["--lut1d", str(t)]
    assert engine_command(Path("-"), Path("-"), params, a, info, lut1d=t, interp1d="cubic") == plain + ["--lut1d", str(t), "--interp1d", "cubic"]
    cmds = engine_stage_commands(Path("in.mov"), Path("out.mov"), params, a, info, lut1d=t, interp1d="nearest")
    assert cmds.engine[-4:] == ["--lut1d", str(t), "--interp1d", "nearest"]
    with pytest.raises(ValueError, match="interp1d is the mode of the 1D LUT: it needs lut1d"):
        engine_command(Path("-"), Path("-"), params, a, info, interp1d="cubic")
    with pytest.raises(ValueError, match="lut1d has no interpolation mode 'bicubic'"):
        engine_command(Path("-"), Path("-"), params, a, info, lut1d=t, interp1d="bicubic")
    with pytest.raises(ValueError, match="a CDL is not supported with a 1D LUT"):
        from lut_renderer_amd.cdl import Cdl
        engine_command(Path("-"), Path("-"), params, a, info, lut1d=t, cdl=Cdl(saturation=0.5))
    with pytest.raises(ValueError, match="two-LUT chain .* is not supported with a 1D LUT"):
        engine_command(Path("-"), Path("-"), params, a, info, lut1d=t, cube2=a)
    with pytest.raises(ValueError, match=r"dither \('blue_noise'\) is not supported with a 1D LUT"):
        engine_command(Path("-"), Path("-"), params, a, info, lut1d=t, engine_dither="blue_noise")


# ------------------------------------------------------------------ twin anchors
def test_with_the_identity_1d_lut_the_twin_is_the_xsub_twin(orc):
    lut = cube.CubeLut(9, np.ones(3, F), np.random.default_rng(7).uniform(-0.2, 1.2, (9, 9, 9, 3)).astype(F))
    for depth in (8, 10):
        tab = twin.table(cube.Lut1D.identity(1 << depth).table, np.ones(3, F), "linear", depth)
        assert np.array_equal(tab, np.tile(np.arange(1 << depth, dtype=np.uint16), (3, 1)))
        for a, b in (("420", "422"), ("444", "420"), ("422", "422")):
            (icsx, icsy), (ocsx, ocsy) = twin.LAYOUTS[a], twin.LAYOUTS[b]
            src = frames.natural_yuv(67, 21, depth, icsx, icsy, k=2)
            k = twin.consts("bt709", "tv", "bt709", "tv", depth, depth, depth, ocsx, ocsy)
            for mode in ("tetrahedral", "prism"):
                got = twin.apply(tab, lut, mode, k, depth, depth, icsx, icsy, ocsx, ocsy, src)
                want = xs.apply(lut.table, lut.scale, mode, k, depth, depth, icsx, icsy, ocsx, ocsy, src)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), (depth, a, b, mode)


def test_lut1d_alone_on_a_444_frame_is_the_lookup_of_stage_1(orc):
    """The integer RGB between the two filters is T[yuv_to_rgb_codes]: checked on the twin's own intermediate, with no matrix
    identity needed, and through stage 3 applied to it."""
    from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
    l1 = cube.read_lut1d(GOLDEN / "gamma1024.cube")
    tab = twin.table(l1.table, l1.scale, "cubic", 10)
    src = frames.natural_yuv(48, 16, 10, 0, 0, k=3)
    k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 0, 0)
    r, g, b = yuv_to_rgb_codes(k, 0, 0, src)
    mid = twin.rgb_codes(tab, k, 0, 0, src)
    assert np.array_equal(mid[0], tab[0][r]) and np.array_equal(mid[1], tab[1][g]) and np.array_equal(mid[2], tab[2][b])
    got = twin.apply(tab, None, None, k, 10, 10, 0, 0, 0, 0, src)
    want = rgb_codes_to_yuv(k, 10, 0, 0, (tab[0][r].astype(np.int64), tab[1][g].astype(np.int64), tab[2][b].astype(np.int64)))
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
    # planar RGB: channel order and the clamp of container values above M
    planes = [np.array([[0, 1023, 1024, 65535]], np.uint16)] * 3
    out = twin.apply_rgb(tab, 10, planes)
    assert out[0].tolist() == [[tab[1][0], tab[1][1023], tab[1][1023], tab[1][1023]]] and out[2][0, 0] == tab[0][0]
