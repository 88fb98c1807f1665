"""1D LUT alone or in front of lut3d on the GPU: lutr_apply_yuv_lut1d and lutr_apply_planar_rgb_lut1d bit-exact,
whole planes, against the composition in tests/_lut1d_twin.py.  The twin is fed the product's own host table (lutr_lut1d_table,
pinned entry for entry to the twin's own build in tests/test_lut1d.py), so that cosf cannot fail a kernel test."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from tests import _lut1d_twin as twin

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "lut1d"
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
GENERIC = "k_yuv_l1d_generic"
#: 136 x 36, 2 frames: at 8 samples per thread 612 threads -- two full workgroups and a partial one, across the frame stride
W, H, NF = 136, 36, 2
_refs = {}           # sources and expected planes, computed once per case and shared (never written to)


def _fmt(depth, lay, alpha=False):
    return f"yuv{'a' if alpha else ''}{lay}p" + ("" if depth == 8 else f"{depth}le")


def _dev(planes, device):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to(device)
            for p in planes]


def _host(tensors, dout):
    return [t.cpu().numpy().view(np.uint16) if dout > 8 else t.cpu().numpy() for t in tensors]


def _eq(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


def _vec_name(din, dout, a, b, mode):
    (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
    return f"k_yuv_l1d_vec<{int(din > 8)},{int(dout > 8)},{icsx},{icsy},{ocsx},{ocsy},{-1 if mode is None else MODES.index(mode)}>"


@pytest.fixture(scope="module")
def luts(cube_dir):
    return {n: (cube_dir / f"{n}.cube", cube.read_lut(cube_dir / f"{n}.cube")) for n in ("log709_33", "random_9")}


@pytest.fixture(scope="module")
def l1ds():
    return {n: cube.read_lut1d(GOLDEN / f"{n}.cube") for n in ("curve17", "gamma1024", "invert33", "range64")}


def _src(dist, w, h, depth, lay, k=1, nf=1, full_range=False):
    """(Y, Cb, Cr), each [nf, rows, cols] (or [rows, cols] for nf = 1)."""
    rk = ("src", dist, w, h, depth, lay, k, nf, full_range)
    if rk not in _refs:
        fs = [frames.make_yuv(dist, w, h, depth, *LAYOUTS[lay], k=k + 7 * i, full_range=full_range) for i in range(nf)]
        _refs[rk] = fs[0] if nf == 1 else [np.stack([f[i] for f in fs]) for i in range(3)]
    return _refs[rk]


def _want(l1, m1, lut, mode, din, dl, dout, a, b, src, key, rin="tv", prologue=False, prelut=None):
    """The twin's planes for `src` ([rows, cols] or [nf, rows, cols] planes), with the product's own table of (l1, m1) at dl."""
    rk = (id(l1), m1, id(lut), mode, din, dl, dout, a, b, key, rin, prologue)
    if rk not in _refs:
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        k = twin.consts("bt709", rin, "bt709", "tv", din, dl, dout, ocsx, ocsy, prologue=prologue)
        tab = _native.lut1d_table(l1, m1, dl)
        if src[0].ndim == 2:
            _refs[rk] = twin.apply(tab, lut, mode, k, dl, dout, icsx, icsy, ocsx, ocsy, src, prelut=prelut)
        else:
            per = [twin.apply(tab, lut, mode, k, dl, dout, icsx, icsy, ocsx, ocsy, [p[i] for p in src], prelut=prelut)
                   for i in range(src[0].shape[0])]
            _refs[rk] = [np.stack([f[i] for f in per]) for i in range(3)]
    return _refs[rk]


# ------------------------------------------------------------------ layouts, container mixes, modes
@pytest.mark.gpu
@pytest.mark.parametrize("a", list(LAYOUTS))
@pytest.mark.parametrize("b", list(LAYOUTS))
def test_all_nine_layout_pairs_at_10_bit(engine, luts, l1ds, a, b):
    engine.load_cube(luts["log709_33"][0])
    engine.set_lut1d(l1ds["gamma1024"], "cubic")
    src = _src("natural", W, H, 10, a, nf=NF)
    for mode in ("tetrahedral", None):
        got = engine.apply_yuv_lut1d(_dev(src, engine.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), interp=mode)
        assert engine.last_kernel == _vec_name(10, 10, a, b, mode), engine.last_kernel
        assert _eq(_host(got, 10), _want(l1ds["gamma1024"], "cubic", luts["log709_33"][1], mode, 10, 10, 10, a, b, src, "nine")), mode


@pytest.mark.gpu
@pytest.mark.parametrize("din,dout", [(8, 8), (10, 8), (16, 8), (8, 10), (12, 12)], ids=lambda v: str(v))
def test_container_mixes_on_420_to_422(engine, luts, l1ds, din, dout):
    engine.load_cube(luts["random_9"][0])
    engine.set_lut1d(l1ds["curve17"], "spline")
    src = _src("uniform", W, H, din, "420", nf=NF)
    got = engine.apply_yuv_lut1d(_dev(src, engine.device), pix_fmt=_fmt(din, "420"), out_pix_fmt=_fmt(dout, "422"))
    # an 8-bit source written as 16-bit words has no vector kernel
    assert engine.last_kernel == (GENERIC if din == 8 and dout > 8 else _vec_name(din, dout, "420", "422", "tetrahedral"))
    assert _eq(_host(got, dout), _want(l1ds["curve17"], "spline", luts["random_9"][1], "tetrahedral", din, din, dout, "420", "422", src, "mix"))


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [12, 16])
def test_both_ends_of_the_table_are_read(engine, luts, l1ds, depth):
    """A frame whose RGB reaches codes 0 and M: 16 bit is the 3 x 65536 table in global memory, 12 bit the largest one in LDS."""
    m = (1 << depth) - 1
    engine.load_cube(luts["log709_33"][0])
    engine.set_lut1d(l1ds["invert33"], "linear")
    src = [p.copy() for p in _src("uniform", 64, 8, depth, "420", k=2)]
    src[0][0, :8] = [0, m, 0, m, 1, m - 1, (m + 1) // 2, m]
    src[1][0, :4] = [0, m, (m + 1) // 2, (m + 1) // 2]
    src[2][0, :4] = [m, 0, (m + 1) // 2, (m + 1) // 2]
    tab = _native.lut1d_table(l1ds["invert33"], "linear", depth)
    assert tab.shape == (3, m + 1) and tab[0, 0] == m and tab[0, m] == 0
    from oracle.lut3d_numpy import yuv_to_rgb_codes
    k = twin.consts("bt709", "tv", "bt709", "tv", depth, depth, depth, 1, 1)
    rgb = yuv_to_rgb_codes(k, 1, 1, src)
    assert min(int(c.min()) for c in rgb) == 0 and max(int(c.max()) for c in rgb) == m
    for mode in ("tetrahedral", None):
        got = engine.apply_yuv_lut1d(_dev(src, engine.device), pix_fmt=_fmt(depth, "420"), interp=mode)
        assert engine.last_kernel == _vec_name(depth, depth, "420", "420", mode)
        assert _eq(_host(got, depth), twin.apply(tab, luts["log709_33"][1], mode, k, depth, depth, 1, 1, 1, 1, src)), mode


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_modes(engine, luts, l1ds, mode):
    """nearest / trilinear / tetrahedral on the vector kernel (and the generic one), pyramid / prism on the generic kernel."""
    engine.load_cube(luts["random_9"][0])
    engine.set_lut1d(l1ds["gamma1024"], "linear")
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, engine.device)
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", interp=mode)
    want = _want(l1ds["gamma1024"], "linear", luts["random_9"][1], mode, 10, 10, 10, "420", "422", src, "modes")
    if mode in MODES[:3]:
        with _variant(engine, "vec_global"):
            got = engine.apply_yuv_lut1d(dev, **names)
            assert engine.last_kernel == _vec_name(10, 10, "420", "422", mode)
        assert _eq(_host(got, 10), want)
    else:
        got = engine.apply_yuv_lut1d(dev, **names)
        assert engine.last_kernel == GENERIC
        assert _eq(_host(got, 10), want)
        with _variant(engine, "vec_global"):
            with pytest.raises(_native.LutrError) as e:
                engine.apply_yuv_lut1d(dev, **names)
            assert e.value.code == _native.EINVAL
    with _variant(engine, "generic"):
        got = engine.apply_yuv_lut1d(dev, **names)
        assert engine.last_kernel == GENERIC
    assert _eq(_host(got, 10), want)


# ------------------------------------------------------------------ shapes
@pytest.mark.gpu
def test_ragged_widths(engine, luts, l1ds):
    """140 x 36 at 8 bit (8 samples a thread) and 138 x 36 at 10 bit (4 a thread) on padded (aligned) rows: the vector kernel up to
    column 136, the generic kernel for the rest.  67 x 21: the generic kernel's alone, odd edges on both layouts."""
    import torch
    engine.load_cube(luts["log709_33"][0])
    engine.set_lut1d(l1ds["curve17"], "cubic")
    pad = 160
    for (w, h), depth, a, b, mode, split in (((140, 36), 8, "420", "422", "tetrahedral", True), ((140, 36), 8, "444", "420", None, True),
                                             ((138, 36), 10, "420", "422", "tetrahedral", True), ((138, 36), 10, "422", "444", None, True),
                                             ((67, 21), 10, "420", "422", "tetrahedral", False), ((67, 21), 10, "422", "420", None, False)):
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        dt, fill = (torch.uint8, 255) if depth == 8 else (torch.int16, -1)
        src = _src("natural", w, h, depth, a, k=4)
        sp = [torch.zeros((p.shape[0], pad), dtype=dt, device=engine.device) for p in src]
        for t, p in zip(sp, _dev(src, engine.device)):
            t[:, :p.shape[1]] = p
        src_v = [t[:, :p.shape[1]] for t, p in zip(sp, src)]
        oshape = [(h, w)] + [frames.chroma_shape(w, h, ocsx, ocsy)] * 2
        dp = [torch.full((s[0], pad), fill, dtype=dt, device=engine.device) for s in oshape]
        dst_v = [t[:, :s[1]] for t, s in zip(dp, oshape)]
        engine.apply_yuv_lut1d(src_v, dst_v, pix_fmt=_fmt(depth, a), out_pix_fmt=_fmt(depth, b), interp=mode)
        name = _vec_name(depth, depth, a, b, mode) + "+" + GENERIC if split else GENERIC
        assert engine.last_kernel == name, (engine.last_kernel, name)
        want = _want(l1ds["curve17"], "cubic", luts["log709_33"][1], mode, depth, depth, depth, a, b, src, ("ragged", w, h))
        assert _eq(_host(dst_v, depth), want), (w, h, depth, a, b)
        assert all((t[:, s[1]:] == fill).all() for t, s in zip(dp, oshape)), "wrote past the row"


# ------------------------------------------------------------------ other paths
@pytest.mark.gpu
def test_full_range_prologue(engine, luts, l1ds):
    """A full-range 8-bit source with range_in="tv": lutr_apply_yuv's prologue ahead of the 1D LUT."""
    engine.load_cube(luts["log709_33"][0])
    engine.set_lut1d(l1ds["gamma1024"], "linear")
    src = _src("natural", W, H, 8, "420", k=6, nf=NF, full_range=True)
    for mode in ("tetrahedral", None):
        got = engine.apply_yuv_lut1d(_dev(src, engine.device), pix_fmt="yuv420p", out_pix_fmt="yuv422p", range_src="pc", range_in="tv",
                                     lut_depth=8, interp=mode)
        assert engine.last_kernel == _vec_name(8, 8, "420", "422", mode)
        want = _want(l1ds["gamma1024"], "linear", luts["log709_33"][1], mode, 8, 8, 8, "420", "422", src, "pc", rin="tv", prologue=True)
        assert _eq(_host(got, 8), want), mode


@pytest.mark.gpu
def test_a_csp_prelut_on_the_3d_lut_is_taken(engine, l1ds, tmp_path):
    from oracle import binding as orc
    from tests._csp_files import write_csp_with_prelut
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, cube.log709_lattice(17), shapers)
    lut = engine.load_cube(p)
    assert lut.prelut is not None
    pre = orc.parse_lut_file_ex(p)[3]
    engine.set_lut1d(l1ds["curve17"], "linear")
    src = _src("natural", W, H, 10, "420", nf=NF)
    for mode in ("tetrahedral", "prism"):
        got = engine.apply_yuv_lut1d(_dev(src, engine.device), pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", interp=mode)
        want = _want(l1ds["curve17"], "linear", lut, mode, 10, 10, 10, "420", "422", src, "prelut", prelut=pre)
        assert _eq(_host(got, 10), want), (mode, engine.last_kernel)


@pytest.mark.gpu
def test_row_shards_are_the_whole_call(engine, luts, l1ds):
    import torch
    engine.load_cube(luts["log709_33"][0])
    engine.set_lut1d(l1ds["gamma1024"], "spline")
    src = _src("uniform", W, H, 10, "420", nf=NF)
    dev = _dev(src, engine.device)
    for b, variant in (("420", "auto"), ("422", "auto"), ("444", "generic")):
        ocsy = LAYOUTS[b][1]
        names = dict(pix_fmt="yuv420p10le", out_pix_fmt=_fmt(10, b))
        whole = _want(l1ds["gamma1024"], "spline", luts["log709_33"][1], "tetrahedral", 10, 10, 10, "420", b, src, "shard")
        with _variant(engine, variant):
            out = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=engine.device) for p in whole]
            engine.apply_yuv_lut1d(dev, out, row0=10, rows=14, **names)
            got = _host(out, 10)
            for i, (g, wh) in enumerate(zip(got, whole)):
                r0, r1 = (10, 24) if i == 0 else (10 >> ocsy, 24 >> ocsy)
                assert np.array_equal(g[:, r0:r1], wh[:, r0:r1]), (b, variant, i)
                assert (g[:, :r0] == 0x5a5a).all() and (g[:, r1:] == 0x5a5a).all(), (b, variant, i, "wrote outside the block")
            engine.apply_yuv_lut1d(dev, out, row0=0, rows=10, **names)
            engine.apply_yuv_lut1d(dev, out, row0=24, rows=H - 24, **names)
        assert _eq(_host(out, 10), whole), (b, variant)
    with pytest.raises(_native.LutrError, match="union") as e:
        engine.apply_yuv_lut1d(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", row0=1, rows=H - 1)
    assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_group_shards_on_the_union_block(engine, luts, l1ds, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    l1 = l1ds["gamma1024"]
    for (w, h), a, b in (((W, H), "420", "422"), ((33, 7), "422", "420")):
        src = _src("natural", w, h, 10, a, k=9)
        names = dict(pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b))
        want = _want(l1, "linear", luts["log709_33"][1], "tetrahedral", 10, 10, 10, a, b, src, ("group", w))
        with LutEngineGroup([0, 0]) as g:
            assert g.treat_as_remote
            g.set_lut(luts["log709_33"][1])
            g.set_lut1d(l1)
            got = g.apply_yuv_lut1d(_dev(src, engine.device), **names)
            assert g.last_remote == 1 and all(r0 % 2 == 0 for r0, _ in g.last_blocks), g.last_blocks
            assert all(k.startswith("k_yuv_l1d_") for k in g.last_kernels), g.last_kernels
            assert _eq(_host(got, 10), want), (w, h)
            rgb = frames.make_rgb("natural", 67, 21, 10, k=3)
            got = g.apply_rgb_lut1d(_dev(rgb, engine.device), depth=10)
            assert _eq(_host(got, 10), twin.apply_rgb(_native.lut1d_table(l1, "linear", 10), 10, rgb))


# ------------------------------------------------------------------ engine state
@pytest.mark.gpu
def test_replacing_the_table_between_two_calls(engine, luts, l1ds, tmp_path):
    """set_lut1d with another file between two calls on one engine, no host wait in between: each call uses the table that was
    set when it was issued.  Then two files that share their first 512 rows (a memo keyed by a host address or a prefix would
    keep the first), and removal."""
    engine.load_cube(luts["random_9"][0])
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, engine.device)
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
    order = [("gamma1024", "linear"), ("invert33", "linear"), ("gamma1024", "cubic"), ("gamma1024", "linear")]
    outs = []
    for n, m in order:
        engine.set_lut1d(l1ds[n], m)
        outs.append(engine.apply_yuv_lut1d(dev, **names))
    for got, (n, m) in zip(outs, order):
        assert _eq(_host(got, 10), _want(l1ds[n], m, luts["random_9"][1], "tetrahedral", 10, 10, 10, "420", "422", src, "aba")), (n, m)
    base = l1ds["gamma1024"].table
    other = base.copy()
    other[:, 512:] = 1.0 - other[:, 512:]
    cube.write_lut1d(tmp_path / "a.cube", base)
    cube.write_lut1d(tmp_path / "b.cube", other)
    pair = [cube.read_lut1d(tmp_path / "a.cube"), cube.read_lut1d(tmp_path / "b.cube")]
    assert np.array_equal(pair[0].table[:, :512], pair[1].table[:, :512]) and not np.array_equal(pair[0].table, pair[1].table)
    outs = []
    for l1 in pair:
        engine.set_lut1d(l1)
        outs.append(_host(engine.apply_yuv_lut1d(dev, **names), 10))
    wants = [_want(l1, "linear", luts["random_9"][1], "tetrahedral", 10, 10, 10, "420", "422", src, "shared") for l1 in pair]
    assert _eq(outs[0], wants[0]) and _eq(outs[1], wants[1]) and not _eq(wants[0], wants[1])
    engine.set_lut1d(None)
    with pytest.raises(ValueError, match="no 1D LUT is loaded"):
        engine.apply_yuv_lut1d(dev, **names)
    s, d = _desc(dev), _desc(_dev(_want(l1ds["gamma1024"], "linear", luts["random_9"][1], "tetrahedral", 10, 10, 10, "420", "422",
                                        src, "aba"), engine.device))
    rc, msg = _abi(engine, 1, 0, W, H, s, d, nf=1)
    assert rc == _native.EINVAL and "no 1D LUT set" in msg, msg


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_the_identity_1d_lut_is_the_plain_call_bit_for_bit(engine, luts, mode):
    engine.load_cube(luts["random_9"][0])
    engine.set_lut1d(cube.Lut1D.identity(1024), "linear")
    for a, b in (("420", "422"), ("420", "420"), ("444", "444")):
        src = _src("natural", W, H, 10, a, nf=NF)
        dev = _dev(src, engine.device)
        names = dict(pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), interp=mode)
        plain = _host(engine.apply_yuv(dev, **names), 10)
        got = engine.apply_yuv_lut1d(dev, **names)
        assert engine.last_kernel == (_vec_name(10, 10, a, b, mode) if mode in MODES[:3] else GENERIC)
        assert _eq(_host(got, 10), plain), (mode, a, b)


@pytest.mark.gpu
def test_a_yuva_frame_carries_its_alpha_past_the_1d_lut(engine, luts, l1ds):
    engine.load_cube(luts["log709_33"][0])
    engine.set_lut1d(l1ds["gamma1024"], "linear")
    src = _src("natural", W, H, 10, "444", k=11)
    alpha = np.random.default_rng(3).integers(0, 1024, size=(H, W)).astype(np.uint16)
    got = engine.apply_yuv_lut1d(_dev(list(src) + [alpha], engine.device), pix_fmt="yuva444p10le")
    assert engine.last_kernel.startswith(_vec_name(10, 10, "444", "444", "tetrahedral") + "+k_alpha_"), engine.last_kernel
    out = _host(got, 10)
    assert len(out) == 4 and np.array_equal(out[3], alpha)
    three = _host(engine.apply_yuv_lut1d(_dev(src, engine.device), pix_fmt="yuv444p10le"), 10)
    assert _eq(out[:3], three)
    assert _eq(three, _want(l1ds["gamma1024"], "linear", luts["log709_33"][1], "tetrahedral", 10, 10, 10, "444", "444", src, "yuva"))


# ------------------------------------------------------------------ planar RGB
@pytest.mark.gpu
@pytest.mark.parametrize("depth", [8, 10, 16])
def test_planar_rgb(engine, luts, l1ds, depth, orc):
    import torch
    l1 = l1ds["gamma1024"]
    engine.load_cube(luts["log709_33"][0])
    engine.set_lut1d(l1, "cubic")
    tab = _native.lut1d_table(l1, "cubic", depth)
    # 136 x 36 x 2: the dword kernel
    fs = [frames.make_rgb("natural", W, H, depth, k=1 + i) for i in range(NF)]
    src = [np.stack([f[i] for f in fs]) for i in range(3)]
    if depth == 10:                    # a 10-bit container holding codes above 1023: they take T[1023]
        src = [p.copy() for p in src]
        src[0][0, 0, :4] = [1024, 4095, 65535, 1023]
        src[2][1, 5, 7] = 2048
    want = twin.apply_rgb(tab, depth, src)
    if depth == 10:
        assert want[0][0, 0, 0] == tab[1][1023] and want[2][1, 5, 7] == tab[0][1023]
    dev = _dev(src, engine.device)
    got = engine.apply_rgb_lut1d(dev, depth=depth)
    assert engine.last_kernel == f"k_rgb_l1d<{int(depth > 8)}>", engine.last_kernel
    assert _eq(_host(got, depth), want)
    # in place
    engine.apply_rgb_lut1d(dev, dev, depth=depth)
    assert _eq(_host(dev, depth), want)
    # 67 x 21: the columns past the last whole dword, and rows that are not dword aligned
    small = frames.make_rgb("uniform", 67, 21, depth, k=5)
    got = engine.apply_rgb_lut1d(_dev(small, engine.device), depth=depth)
    assert engine.last_kernel == "k_rgb_l1d_generic", engine.last_kernel         # (a 67-sample dense row is not a whole dword)
    assert _eq(_host(got, depth), twin.apply_rgb(tab, depth, small))
    dt = torch.uint8 if depth == 8 else torch.int16
    padded = [torch.zeros((21, 80), dtype=dt, device=engine.device) for _ in range(3)]
    for t, p in zip(padded, _dev(small, engine.device)):
        t[:, :67] = p
    out = [torch.full((21, 80), -1 if depth > 8 else 255, dtype=dt, device=engine.device) for _ in range(3)]
    engine.apply_rgb_lut1d([t[:, :67] for t in padded], [t[:, :67] for t in out], depth=depth)
    assert engine.last_kernel == f"k_rgb_l1d<{int(depth > 8)}>+k_rgb_l1d_generic", engine.last_kernel
    assert _eq(_host([t[:, :67] for t in out], depth), twin.apply_rgb(tab, depth, small))
    assert all((t[:, 67:] == (-1 if depth > 8 else 255)).all() for t in out), "wrote past the row"
    # lut1d, then lut3d: the twin's lookup followed by the oracle's lut3d
    got = engine.apply_rgb_lut1d(_dev(small, engine.device), depth=depth, interp="tetrahedral")
    lut = luts["log709_33"][1]
    assert _eq(_host(got, depth), orc.apply_rgb(lut.table, lut.scale, depth, "tetrahedral", twin.apply_rgb(tab, depth, small)))


# ------------------------------------------------------------------ refusals
def _desc(tensors):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        st.data[i] = t.data_ptr()
        st.stride[i] = t.stride(-2) * t.element_size()
        st.frame_stride[i] = 0
    return st


def _abi(engine, interp, csy_in, w, h, s, d, nf=1):
    p = _native.YuvParams(_native.fmt_code(10, 1, 1), _native.fmt_code(10, 1, csy_in), 10, 0, 0, 0, 0, 0)
    with engine._lock:
        engine._bind_stream()
        rc = engine._lib.lutr_apply_yuv_lut1d(engine._ctx, C.byref(p), interp, w, h, nf, C.byref(s), C.byref(d), 0, h)
    return rc, engine._lib.lutr_last_error().decode()


@pytest.mark.gpu
def test_refusals_leave_the_destination_untouched(engine, luts, l1ds):
    import torch
    w, h = 64, 8
    engine.load_cube(luts["log709_33"][0])
    engine.set_lut1d(l1ds["curve17"], "linear")
    src = _src("natural", w, h, 10, "420")
    dev = _dev(src, engine.device)
    out = [torch.full_like(t, 0x5a5a) for t in dev]
    with _variant(engine, "vec_lds"):
        rc, msg = _abi(engine, 2, 1, w, h, _desc(dev), _desc(out))
        assert rc == _native.EINVAL and "vec_lds" in msg, msg
        with pytest.raises(_native.LutrError) as e:
            engine.apply_rgb_lut1d([dev[0]] * 3, depth=10)
        assert e.value.code == _native.EINVAL
    rc, msg = _abi(engine, 2, 1, w, h, _desc(dev), _desc(dev))
    assert rc == _native.EINVAL and "cannot run in place: the byte range of source plane 0 overlaps" in msg, msg
    inside = [out[0], dev[0][:h // 2, :w // 2], out[2]]
    rc, msg = _abi(engine, 2, 1, w, h, _desc(dev), _desc(inside))
    assert rc == _native.EINVAL and "source plane 0 overlaps that of destination plane 1" in msg, msg
    with pytest.raises(ValueError, match="lut1d pass cannot run in place"):
        engine.apply_yuv_lut1d(dev, dev, pix_fmt="yuv420p10le")
    # 4:4:0
    p = _native.YuvParams(_native.fmt_code(10, 0, 1), _native.fmt_code(10, 0, 1), 10, 0, 0, 0, 0, 0)
    with engine._lock:
        engine._bind_stream()
        rc = engine._lib.lutr_apply_yuv_lut1d(engine._ctx, C.byref(p), 2, w, h, 1, C.byref(_desc(dev)), C.byref(_desc(out)), 0, h)
    assert rc == _native.EINVAL, engine._lib.lutr_last_error().decode()
    with pytest.raises(ValueError):
        engine.apply_yuv_lut1d(dev, out, pix_fmt="yuv440p10le")
    # a mode lut3d does not have; lut1d alone needs no lattice, lut1d -> lut3d does
    rc, msg = _abi(engine, 5, 1, w, h, _desc(dev), _desc(out))
    assert rc == _native.EINVAL and "interpolation mode" in msg, msg
    torch.cuda.synchronize()
    assert all((t == 0x5a5a).all() for t in out), "a refused call wrote to a destination"
    rc, msg = _abi(engine, 2, 1, w, h, _desc(dev), _desc(out))
    assert rc == 0, msg
    assert _eq(_host(out, 10), _want(l1ds["curve17"], "linear", luts["log709_33"][1], "tetrahedral", 10, 10, 10, "420", "420", src, "abi"))
    from lut_renderer_amd.engine import LutEngine
    with LutEngine(0) as bare:                                        # no lattice on this context
        bare.set_lut1d(l1ds["curve17"])
        got = bare.apply_yuv_lut1d(dev, pix_fmt="yuv420p10le", interp=None)
        assert _eq(_host(got, 10), _want(l1ds["curve17"], "linear", None, None, 10, 10, 10, "420", "420", src, "bare"))
        with pytest.raises(_native.LutrError, match="no lattice"):
            bare.apply_yuv_lut1d(dev, pix_fmt="yuv420p10le")


# ------------------------------------------------------------------ table placement
@pytest.mark.gpu
def test_lds_and_global_tables_give_the_same_bytes(luts):
    """LUTR_L1D_LDS=1 / 0 in two child processes (the knob is read at launch): the same output bytes at 8, 10, 12 and 16 bit."""
    outs = []
    for knob in ("1", "0"):
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "_gpu_lut1d_worker.py"), str(luts["log709_33"][0]),
                            str(GOLDEN / "gamma1024.cube")], capture_output=True, cwd=ROOT, timeout=180,
                           env=dict(os.environ, LUTR_L1D_LDS=knob))
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        outs.append(r.stdout)
    assert len(outs[0]) > 100000 and outs[0] == outs[1]


# ------------------------------------------------------------------ apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut_with_a_1d_lut_file(engine, luts, l1ds):
    from lut_renderer_amd.api import apply_lut
    src = _src("natural", W, H, 10, "420", nf=NF)
    l1 = l1ds["gamma1024"]
    got, tags = apply_lut(_dev(src, engine.device), cube=luts["log709_33"][1], lut1d=GOLDEN / "gamma1024.cube", interp1d="cubic",
                          pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv", out_pix_fmt="yuv422p10le", engine=engine)
    assert engine.last_kernel == _vec_name(10, 10, "420", "422", "tetrahedral") and tags["colorspace"] == "bt709"
    assert _eq(_host(got, 10), _want(l1, "cubic", luts["log709_33"][1], "tetrahedral", 10, 10, 10, "420", "422", src, "nine"))
    got, _ = apply_lut(_dev(src, engine.device), cube=None, lut1d=l1, pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv",
                       out_pix_fmt="yuv422p10le", engine=engine)
    assert engine.last_kernel == _vec_name(10, 10, "420", "422", None)
    assert _eq(_host(got, 10), _want(l1, "linear", None, None, 10, 10, 10, "420", "422", src, "alone"))


@pytest.mark.gpu
def test_cli_over_pipes_with_a_1d_lut_file(luts, l1ds):
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    src = _src("natural", 64, 8, 10, "420")
    want = b"".join(p.tobytes() for p in _want(l1ds["gamma1024"], "spline", luts["log709_33"][1], "tetrahedral", 10, 10, 10, "420",
                                               "422", src, "cli"))
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le"), luts["log709_33"][0],
                         info, python_bin=sys.executable, lut1d=GOLDEN / "gamma1024.cube", interp1d="spline")
    assert cmd[-4:] == ["--lut1d", str(GOLDEN / "gamma1024.cube"), "--interp1d", "spline"]
    r = subprocess.run(cmd + ["--duration", "0.040"], input=b"".join(p.tobytes() for p in src), capture_output=True, cwd=ROOT,
                       timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == want
