"""The stage stack on RGB sources on the GPU: lutr_apply_rgb_stack bit for bit, whole planes, against the list
walk of tests/_rgbstack_twin.py, and against the existing entry points on the same engine where the contracts meet.  The twin is
fed the product's own host tables (lutr_cdl_table, lutr_lut1d_table), so that a last-bit difference between two pows or cosf
cannot fail a kernel test.  The tolerance is zero: the contract is a composition of pinned pieces."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube
from lut_renderer_amd.cdl import Cdl, read_cdl
from lut_renderer_amd.formats import parse_stages
from lut_renderer_amd.rgbmatrix import RgbMatrix, read_rgb_matrix
from tests import _rgbstack_twin as twin
from tests.test_gpu_rgb2yuv import make_source

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
GENERIC = "k_rgb_stack_generic"
#: 136 x 36, 2 frames: at 8 samples per thread 612 threads -- two full workgroups and a partial one, across the frame stride
W, H, NF = 136, 36, 2
I3 = RgbMatrix()
GAMUT = read_rgb_matrix(GOLDEN / "matrix" / "bt2020_to_709.spimtx")
_refs = {}           # sources and expected planes, computed once per case and shared (never written to)


def _yuv(depth, lay, alpha=False):
    return f"yuv{'a' if alpha else ''}{lay}p" + ("" if depth == 8 else f"{depth}le")


def _t(a, device):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def _dev(src, device):
    return _t(src, device) if isinstance(src, np.ndarray) else [_t(p, device) for p in src]


def _host(tensors, depth):
    return [t.cpu().numpy().view(np.uint16) if depth > 8 else t.cpu().numpy() for t in tensors]


def _eq(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


def _list(stages):
    """The stage list as `last_kernel` spells it."""
    return "[" + ",".join(k if m is None else f"{k}:{MODES.index(m)}" for k, m in parse_stages(stages)) + "]"


def _lds(stages, dl):
    """The default placement: the tables the stack uses fit 24 KB together."""
    kinds = [k for k, _ in parse_stages(stages)]
    size = (3 * (1 << dl) * 4 if "cdl" in kinds else 0) + (3 * (1 << dl) * 2 if "lut1d" in kinds else 0)
    return 0 < size <= 24 * 1024


def _vec_name(pix_fmt, out, stages, lds=None):
    """`out`: a YUV (depth, layout) pair, or None for gbrp* at the source's depth."""
    dl = twin.source_depth(pix_fmt)
    nc = twin.r2y.PACKED[pix_fmt][1] if pix_fmt in twin.r2y.PACKED else 1
    dout, (ocsx, ocsy), sink = (dl, (0, 0), 1) if out is None else (out[0], LAYOUTS[out[1]], 0)
    tri = int(any(m == "trilinear" for _, m in parse_stages(stages)))
    lds = _lds(stages, dl) if lds is None else lds
    return f"k_rgb_stack_vec<{int(dl > 8)},{nc},{int(dout > 8)},{sink},{ocsx},{ocsy},{tri},{int(lds)}>" + _list(stages)


def _src(pix_fmt, dist, w, h, nf=1, k=0):
    """A host source: gbrp planes (G, B, R), each [nf, h, w] (or [h, w]), or one packed image [nf, h, w, c] (or [h, w, c])."""
    rk = ("src", pix_fmt, dist, w, h, nf, k)
    if rk not in _refs:
        fs = [make_source(pix_fmt, dist, w, h, k=k + 7 * i) for i in range(nf)]
        if nf == 1:
            _refs[rk] = fs[0]
        else:
            _refs[rk] = np.stack(fs) if isinstance(fs[0], np.ndarray) else [np.stack([f[i] for f in fs]) for i in range(3)]
    return _refs[rk]


def _frames_of(src):
    """The frames of a host source, one by one."""
    if isinstance(src, np.ndarray):
        return [src] if src.ndim == 3 else list(src)
    return [src] if src[0].ndim == 2 else [[p[i] for p in src] for i in range(src[0].shape[0])]


def _want(res, stages, cdl, mtx, pix_fmt, out, src, key, matrix_out="smpte170m", range_out="tv"):
    """The twin's planes for `src` with the resources `res` (the `loaded` fixture's) and the product's own tables.  `out`: a YUV
    (depth, layout) pair, or None for gbrp* at the source's depth."""
    st = parse_stages(stages)
    rk = (id(res["lut"]), id(res["lut2"]), id(res["l1"][0]), res["l1"][1], id(res["prelut"]), st,
          None if cdl is None else (cdl.sop_text(), cdl.saturation), None if mtx is None else (mtx.m, mtx.offset), pix_fmt, out, key,
          matrix_out, range_out)
    if rk not in _refs:
        dl = twin.source_depth(pix_fmt)
        kinds = [s for s, _ in st]
        kw = dict(lut=res["lut"], lut2=res["lut2"], prelut=res["prelut"], cdl=cdl, mtx=mtx,
                  l1d_tab=_native.lut1d_table(*res["l1"], dl) if "lut1d" in kinds else None,
                  cdl_tab=_native.cdl_table(cdl, dl) if "cdl" in kinds else None)
        if out is None:
            per = [twin.apply_rgb(st, pix_fmt, f, **kw) for f in _frames_of(src)]
        else:
            dout, (ocsx, ocsy) = out[0], LAYOUTS[out[1]]
            k = twin.consts(matrix_out, range_out, dl, dout, ocsx, ocsy)
            per = [twin.apply_yuv(st, k, pix_fmt, dout, ocsx, ocsy, f, **kw) for f in _frames_of(src)]
        batch = (src.ndim == 4) if isinstance(src, np.ndarray) else (src[0].ndim == 3)
        _refs[rk] = [np.stack([f[i] for f in per]) for i in range(3)] if batch else list(per[0])
    return _refs[rk]


def _out_name(pix_fmt, out):
    dl = twin.source_depth(pix_fmt)
    return ("gbrp" if dl == 8 else f"gbrp{dl}le") if out is None else _yuv(*out)


def _depth(pix_fmt, out):
    return twin.source_depth(pix_fmt) if out is None else out[0]


@pytest.fixture(scope="module")
def luts(cube_dir):
    return {n: (cube_dir / f"{n}.cube", cube.read_lut(cube_dir / f"{n}.cube")) for n in ("log709_33", "random_9")}


@pytest.fixture(scope="module")
def l1ds():
    return {n: cube.read_lut1d(GOLDEN / "lut1d" / f"{n}.cube") for n in ("curve17", "gamma1024")}


@pytest.fixture(scope="module")
def grade():
    return read_cdl(GOLDEN / "cdl" / "shot.cc")


@pytest.fixture()
def loaded(engine, luts, l1ds):
    """The engine with log709_33 as the first lattice, random_9 as the second and gamma1024 (cubic) as the 1D LUT."""
    engine.load_cube(luts["log709_33"][0])
    engine.load_cube2(luts["random_9"][0])
    engine.set_lut1d(l1ds["gamma1024"], "cubic")
    engine._res = dict(lut=luts["log709_33"][1], lut2=luts["random_9"][1], l1=(l1ds["gamma1024"], "cubic"), prelut=None)
    return engine


def _sat(c, sat):
    return Cdl(slope=c.slope, offset=c.offset, power=c.power, saturation=sat)


def _run(engine, src, pix_fmt, out, stages, cdl=None, mtx=None, dst=None, **kw):
    got = engine.apply_rgb_stack(_dev(src, engine.device) if dst is None else dst[0], None if dst is None else dst[1],
                                 pix_fmt=pix_fmt, out_pix_fmt=None if out is None and pix_fmt.startswith("gbr") else _out_name(pix_fmt, out),
                                 stages=stages, cdl=cdl, rgb_matrix=mtx, **kw)
    return _host(got, _depth(pix_fmt, out))


# ------------------------------------------------------------------ source kinds x destinations
@pytest.mark.gpu
@pytest.mark.parametrize("pix_fmt", ["gbrp10le", "rgb24", "bgr24", "rgba", "rgb48le", "rgba64le"])
def test_source_kinds_and_destinations(loaded, grade, pix_fmt):
    stages = "lut1d,cdl,lut3d"
    dl = twin.source_depth(pix_fmt)
    src = _src(pix_fmt, "natural", W, H, nf=NF, k=dl)
    for out in ((8, "420"), (10, "422"), (10, "444"), None):
        want = _want(loaded._res, stages, grade, None, pix_fmt, out, src, "kinds")
        got = _run(loaded, src, pix_fmt, out, stages, grade)
        # an 8-bit source written as 16-bit words has no vector kernel: rgb24 / bgr24 / rgba into the 10-bit layouts run the
        # generic kernel under every variant but vec_global
        has_vec = not (dl == 8 and out is not None and out[0] > 8)
        assert loaded.last_kernel == (_vec_name(pix_fmt, out, stages) if has_vec else GENERIC + _list(stages)), loaded.last_kernel
        assert _eq(got, want), (pix_fmt, out, "auto")
        with _variant(loaded, "vec_global"):
            if has_vec:
                assert _eq(_run(loaded, src, pix_fmt, out, stages, grade), want), (pix_fmt, out, "vec_global")
            else:
                with pytest.raises(ValueError, match="vec_global cannot take an 8-bit source"):
                    _run(loaded, src, pix_fmt, out, stages, grade)
        with _variant(loaded, "generic"):
            got = _run(loaded, src, pix_fmt, out, stages, grade)
            assert loaded.last_kernel == GENERIC + _list(stages)
        assert _eq(got, want), (pix_fmt, out, "generic")


ORDERS = ("lut1d,cdl,lut3d", "cdl,lut3d", "lut3d,cdl,lut3d2", "cdl,lut1d", "lut1d,matrix,lut3d", "matrix,cdl,lut3d", "lut3d,matrix",
          "matrix,lut3d,lut3d2:trilinear")


@pytest.mark.gpu
@pytest.mark.parametrize("stages", ORDERS)
def test_orders_on_gbrp10le_to_422(loaded, grade, stages):
    src = _src("gbrp10le", "natural", W, H, nf=NF)
    out = (10, "422")
    mtx = GAMUT if "matrix" in stages else None
    for sat in (1.0, 0.6) if "cdl" in stages else (None,):
        c = None if sat is None else _sat(grade, sat)
        want = _want(loaded._res, stages, c, mtx, "gbrp10le", out, src, "orders")
        got = _run(loaded, src, "gbrp10le", out, stages, c, mtx)
        assert loaded.last_kernel == _vec_name("gbrp10le", out, stages), loaded.last_kernel
        assert _eq(got, want), (stages, sat, "vec")
        with _variant(loaded, "generic"):
            got = _run(loaded, src, "gbrp10le", out, stages, c, mtx)
            assert loaded.last_kernel == GENERIC + _list(stages)
        assert _eq(got, want), (stages, sat, "generic")


@pytest.mark.gpu
@pytest.mark.parametrize("dl,dout", [(8, 8), (10, 8), (16, 8), (8, 10), (12, 12)], ids=lambda v: str(v))
def test_depth_mixes(loaded, grade, dl, dout):
    pix_fmt = "gbrp" if dl == 8 else f"gbrp{dl}le"
    src = _src(pix_fmt, "uniform", W, H, nf=NF, k=2)
    for stages in ("lut1d,matrix,lut3d", "matrix,cdl,lut3d2"):
        c = grade if "cdl" in stages else None
        got = _run(loaded, src, pix_fmt, (dout, "420"), stages, c, GAMUT)
        # an 8-bit source written as 16-bit words has no vector kernel
        name = GENERIC + _list(stages) if dl == 8 and dout > 8 else _vec_name(pix_fmt, (dout, "420"), stages)
        assert loaded.last_kernel == name, loaded.last_kernel
        assert _eq(got, _want(loaded._res, stages, c, GAMUT, pix_fmt, (dout, "420"), src, "mix")), stages


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [12, 16])
def test_frames_that_reach_codes_0_and_m(loaded, grade, depth):
    """12 bit: the 1D table alone fits LDS (24 KB exactly), the CDL's does not; 16 bit: everything in global memory."""
    m = (1 << depth) - 1
    pix_fmt = f"gbrp{depth}le"
    src = [p.copy() for p in make_source(pix_fmt, "uniform", 64, 8, k=2)]
    src[0][0, :8] = [0, m, 0, m, 1, m - 1, (m + 1) // 2, m]
    src[1][0, :8] = [0, m, m, 0, 0, m, m, 0]
    src[2][0, :8] = [m, 0, 0, m, m, 1, m - 1, 0]
    for stages, lds in (("lut1d,lut3d", depth == 12), ("cdl,lut3d", False), ("lut1d,cdl", False), ("matrix", False)):
        c = grade if "cdl" in stages else None
        mtx = I3 if "matrix" in stages else None
        for out in ((depth, "420"), None):
            got = _run(loaded, src, pix_fmt, out, stages, c, mtx)
            assert loaded.last_kernel == _vec_name(pix_fmt, out, stages, lds), loaded.last_kernel
            assert _eq(got, _want(loaded._res, stages, c, mtx, pix_fmt, out, src, ("ends", depth))), (stages, out)


@pytest.mark.gpu
def test_a_10_bit_word_above_m_acts_as_m(loaded, grade):
    """Both kernels, every stage kind as the first of the list: a word above 1023 gives what 1023 gives."""
    src = [p.copy() for p in make_source("gbrp10le", "natural", 64, 8, k=5)]
    high = [p.copy() for p in src]
    for i, v in enumerate((1024, 4095, 65535)):
        high[i][1, 3:60:5] = v
        src[i][1, 3:60:5] = 1023
    for stages in ("lut1d,lut3d", "cdl,lut3d", "matrix,lut3d", "lut3d"):
        c = grade if "cdl" in stages else None
        mtx = GAMUT if "matrix" in stages else None
        for out in ((10, "420"), None):
            want = _want(loaded._res, stages, c, mtx, "gbrp10le", out, src, "clamped")
            for variant in ("auto", "generic"):
                with _variant(loaded, variant):
                    assert _eq(_run(loaded, high, "gbrp10le", out, stages, c, mtx), want), (stages, out, variant)


@pytest.mark.gpu
def test_kernel_split_by_size(loaded, grade):
    """A ragged width on aligned (padded) rows: the vector kernel up to the last whole unit of 8 columns, the generic one for the
    rest -- 139 x 37 where the output block is one row high and 140 x 36 into 4:2:0; the padding keeps its sentinel.  139 x 37
    into 4:2:0 ends in half a block: the generic kernel's alone.  Then 16 x 4 and 67 x 21 on the generic kernel."""
    import torch
    pad = 160
    stages = "lut1d,cdl,lut3d"
    for (w, h), pix_fmt, out, name in (((139, 37), "gbrp10le", (10, "422"), "split"), ((139, 37), "gbrp10le", None, "split"),
                                       ((139, 37), "rgb24", (8, "444"), "split"), ((139, 37), "gbrp10le", (10, "420"), "generic"),
                                       ((140, 36), "gbrp", (8, "420"), "split"), ((140, 36), "rgba64le", (10, "420"), "split")):
        depth = _depth(pix_fmt, out)
        dt, fill = (torch.uint8, 255) if depth == 8 else (torch.int16, -1)
        src = _src(pix_fmt, "natural", w, h, k=4)
        want = _want(loaded._res, stages, grade, None, pix_fmt, out, src, ("split", w, h))
        if isinstance(src, np.ndarray):
            t = _t(src, loaded.device)
            wide = torch.zeros((h, pad, src.shape[-1]), dtype=t.dtype, device=loaded.device)
            wide[:, :w] = t
            src_v = wide[:, :w]
        else:
            sp = [torch.zeros((h, pad), dtype=p.dtype, device=loaded.device) for p in _dev(src, loaded.device)]
            for t, p in zip(sp, _dev(src, loaded.device)):
                t[:, :w] = p
            src_v = [t[:, :w] for t in sp]
        dp = [torch.full((wt.shape[0], pad), fill, dtype=dt, device=loaded.device) for wt in want]
        dst_v = [t[:, :wt.shape[1]] for t, wt in zip(dp, want)]
        loaded.apply_rgb_stack(src_v, dst_v, pix_fmt=pix_fmt, out_pix_fmt=_out_name(pix_fmt, out), stages=stages, cdl=grade)
        if name == "split":
            assert loaded.last_kernel == _vec_name(pix_fmt, out, stages).replace("[", "+" + GENERIC + "[", 1), loaded.last_kernel
        else:
            assert loaded.last_kernel == GENERIC + _list(stages), loaded.last_kernel
        assert _eq(_host(dst_v, depth), want), (w, h, pix_fmt, out)
        assert all((t[:, wt.shape[1]:] == fill).all() for t, wt in zip(dp, want)), (w, h, pix_fmt, out, "wrote into the padding")
    for (w, h), pix_fmt, out in (((16, 4), "gbrp10le", (10, "422")), ((67, 21), "gbrp10le", (10, "420")), ((67, 21), "bgra", None)):
        src = _src(pix_fmt, "natural", w, h, k=5)
        with _variant(loaded, "generic"):
            got = _run(loaded, src, pix_fmt, out, stages, grade)
            assert loaded.last_kernel == GENERIC + _list(stages)
        assert _eq(got, _want(loaded._res, stages, grade, None, pix_fmt, out, src, ("small", w, h))), (w, h, pix_fmt, out)


@pytest.mark.gpu
@pytest.mark.parametrize("m1,m2", [("pyramid", "nearest"), ("trilinear", "prism"), ("tetrahedral", "trilinear"), ("nearest", "tetrahedral"),
                                   ("prism", "pyramid")])
def test_the_five_lut3d_modes_in_mixed_pairs(loaded, m1, m2):
    """Both lattices fed codes (all five modes in the twin); a pyramid or prism stage sends the call to the generic kernel."""
    src = _src("gbrp10le", "natural", W, H, nf=NF)
    stages = ("lut1d", ("lut3d", m1), ("lut3d2", m2))
    all_vec = m1 in MODES[:3] and m2 in MODES[:3]
    for out in ((10, "422"), None):
        want = _want(loaded._res, stages, None, None, "gbrp10le", out, src, "modes")
        got = _run(loaded, src, "gbrp10le", out, stages)
        assert loaded.last_kernel == (_vec_name("gbrp10le", out, stages) if all_vec else GENERIC + _list(stages)), loaded.last_kernel
        assert _eq(got, want), (m1, m2, out)
        with _variant(loaded, "vec_global"):
            if all_vec:
                assert _eq(_run(loaded, src, "gbrp10le", out, stages), want)
            else:
                with pytest.raises(ValueError, match="vec_global cannot take stage"):      # (before any GPU work)
                    _run(loaded, src, "gbrp10le", out, stages)
        with _variant(loaded, "generic"):
            assert _eq(_run(loaded, src, "gbrp10le", out, stages), want)


@pytest.mark.gpu
def test_a_csp_prelut_where_the_lattice_is_fed_codes(loaded, grade, tmp_path):
    from oracle import binding as orc
    from tests._csp_files import write_csp_with_prelut
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, cube.log709_lattice(17), shapers)
    lut = loaded.load_cube(p)
    assert lut.prelut is not None
    res = dict(loaded._res, lut=lut, prelut=orc.parse_lut_file_ex(p)[3])
    src = _src("gbrp10le", "natural", W, H, nf=NF)
    for stages in ("lut3d", "lut1d,lut3d", "lut3d,cdl,lut3d2", "cdl,lut1d,lut3d"):
        c = grade if "cdl" in stages else None
        for out in ((10, "422"), None):
            got = _run(loaded, src, "gbrp10le", out, stages, c)
            assert _eq(got, _want(res, stages, c, None, "gbrp10le", out, src, "prelut")), (stages, out, loaded.last_kernel)
    for stages, mtx in (("cdl,lut3d", None), ("matrix,lut3d", I3)):
        with pytest.raises(ValueError, match="directly behind"):
            _run(loaded, src, "gbrp10le", None, stages, grade if mtx is None else None, mtx)


# ------------------------------------------------------------------ where the contracts meet, on the same engine
@pytest.mark.gpu
def test_existing_entry_points_bit_for_bit(loaded):
    for pix_fmt in ("gbrp10le", "rgb24", "rgba64le", "gbrp"):
        dl = twin.source_depth(pix_fmt)
        src = _src(pix_fmt, "natural", W, H, nf=NF, k=1)
        dev = _dev(src, loaded.device)
        for mode in ("tetrahedral", "trilinear", "prism"):
            for lay in ("420", "422", "444"):
                ref = _host(loaded.apply_rgb_to_yuv(dev, pix_fmt=pix_fmt, out_pix_fmt=_yuv(dl, lay), interp=mode), dl)
                got = _run(loaded, src, pix_fmt, (dl, lay), [("lut3d", mode)])
                assert "k_rgb_stack_" in loaded.last_kernel
                assert _eq(got, ref), (pix_fmt, mode, lay)
            if pix_fmt.startswith("gbrp"):
                ref = _host(loaded.apply_rgb(dev, depth=dl, interp=mode), dl)
                assert _eq(_run(loaded, src, pix_fmt, None, [("lut3d", mode)]), ref), (pix_fmt, mode, "gbrp")
        if pix_fmt.startswith("gbrp"):
            ref = _host(loaded.apply_rgb_lut1d(dev, depth=dl), dl)
            assert _eq(_run(loaded, src, pix_fmt, None, "lut1d"), ref), (pix_fmt, "lut1d")


@pytest.mark.gpu
def test_identity_cdl_and_identity_matrix_give_the_source(loaded):
    for pix_fmt in ("gbrp", "gbrp10le", "gbrp12le", "gbrp16le"):
        src = _src(pix_fmt, "uniform", 64, 8, k=3)
        for variant in ("auto", "generic"):
            with _variant(loaded, variant):
                assert _eq(_run(loaded, src, pix_fmt, None, "cdl", Cdl()), src), (pix_fmt, "cdl", variant)
                assert _eq(_run(loaded, src, pix_fmt, None, "matrix", None, I3), src), (pix_fmt, "matrix", variant)
    img = _src("rgba", "uniform", 64, 8, k=3)
    r, g, b = twin.r2y.source_rgb("rgba", img)
    assert _eq(_run(loaded, img, "rgba", None, "cdl", Cdl()), [g, b, r])


@pytest.mark.gpu
def test_in_place_on_the_source_planes(loaded, grade):
    stages = "lut1d,cdl,lut3d"
    src = _src("gbrp10le", "natural", W, H, nf=NF)
    want = _want(loaded._res, stages, grade, None, "gbrp10le", None, src, "orders")
    for variant in ("auto", "generic"):
        with _variant(loaded, variant):
            dev = _dev(src, loaded.device)
            got = loaded.apply_rgb_stack(dev, dev, pix_fmt="gbrp10le", stages=stages, cdl=grade)
            assert got is dev and _eq(_host(dev, 10), want), variant
    dev = _dev(src, loaded.device)
    with pytest.raises(ValueError, match="in place"):
        loaded.apply_rgb_stack(dev, [dev[1], dev[0], dev[2]], pix_fmt="gbrp10le", stages=stages, cdl=grade)
    with pytest.raises(ValueError, match="in place"):
        loaded.apply_rgb_stack(dev, dev, pix_fmt="gbrp10le", out_pix_fmt="yuv444p10le", stages=stages, cdl=grade)


@pytest.mark.gpu
def test_alpha_goes_past_the_list(loaded, grade):
    stages = "lut1d,cdl,lut3d"
    src = _src("gbrp10le", "natural", W, H, k=11)
    alpha = np.random.default_rng(3).integers(0, 1024, size=(H, W)).astype(np.uint16)
    dev = _dev(list(src) + [alpha], loaded.device)
    for out, name in (((10, "444"), "yuva444p10le"), (None, "gbrap10le")):
        got = loaded.apply_rgb_stack(dev, pix_fmt="gbrap10le", out_pix_fmt=name, stages=stages, cdl=grade)
        assert len(got) == 4 and "+k_alpha" in loaded.last_kernel and loaded.last_kernel.startswith("k_rgb_stack_vec<"), loaded.last_kernel
        got = _host(got, 10)
        assert _eq(got[:3], _want(loaded._res, stages, grade, None, "gbrp10le", out, src, "alpha")), name
        assert np.array_equal(got[3], alpha), name
    img = _src("rgba", "natural", W, H, k=12)
    got = _host(loaded.apply_rgb_stack(_dev(img, loaded.device), pix_fmt="rgba", out_pix_fmt="yuva420p", stages=stages, cdl=grade), 8)
    assert _eq(got[:3], _want(loaded._res, stages, grade, None, "rgba", (8, "420"), img, "alpha"))
    assert np.array_equal(got[3], img[..., 3])
    # a source without alpha fills the plane opaque
    got = _host(loaded.apply_rgb_stack(_dev(src, loaded.device), pix_fmt="gbrp10le", out_pix_fmt="yuva444p10le", stages=stages, cdl=grade), 10)
    assert (got[3] == 1023).all()


@pytest.mark.gpu
def test_row_shards_are_the_whole_call(loaded, grade):
    import torch
    stages = "lut3d,cdl,lut3d2"
    src = _src("gbrp10le", "uniform", W, H, nf=NF)
    dev = _dev(src, loaded.device)
    for out, variant in (((10, "420"), "auto"), (None, "auto"), ((10, "422"), "generic")):
        ocsy = 0 if out is None else LAYOUTS[out[1]][1]
        names = dict(pix_fmt="gbrp10le", out_pix_fmt=_out_name("gbrp10le", out), stages=stages, cdl=grade)
        whole = _want(loaded._res, stages, grade, None, "gbrp10le", out, src, "shard")
        with _variant(loaded, variant):
            dst = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=loaded.device) for p in whole]
            loaded.apply_rgb_stack(dev, dst, row0=10, rows=14, **names)
            got = _host(dst, 10)
            for i, (g, wh) in enumerate(zip(got, whole)):
                r0, r1 = (10, 24) if i == 0 or out is None else (10 >> ocsy, 24 >> ocsy)
                assert np.array_equal(g[:, r0:r1], wh[:, r0:r1]), (out, variant, i)
                assert (g[:, :r0] == 0x5a5a).all() and (g[:, r1:] == 0x5a5a).all(), (out, variant, i, "wrote outside the block")
            loaded.apply_rgb_stack(dev, dst, row0=0, rows=10, **names)
            loaded.apply_rgb_stack(dev, dst, row0=24, rows=H - 24, **names)
        assert _eq(_host(dst, 10), whole), (out, variant)
    with pytest.raises(_native.LutrError, match="chroma block") as e:
        loaded.apply_rgb_stack(dev, pix_fmt="gbrp10le", out_pix_fmt="yuv420p10le", stages=stages, cdl=grade, row0=1, rows=H - 1)
    assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_group_shards_with_remote_blocks(loaded, luts, l1ds, grade, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    stages = "lut1d,cdl,matrix,lut3d"
    for pix_fmt, (w, h), out in (("gbrp10le", (W, H), (10, "420")), ("gbrp10le", (33, 7), None), ("rgb48le", (33, 7), (10, "420"))):
        src = _src(pix_fmt, "natural", w, h, k=9)
        want = _want(loaded._res, stages, grade, GAMUT, pix_fmt, out, src, ("group", w))
        with LutEngineGroup([0, 0]) as g:
            assert g.treat_as_remote
            g.set_lut(luts["log709_33"][1])
            g.set_lut1d(l1ds["gamma1024"], "cubic")
            got = g.apply_rgb_stack(_dev(src, loaded.device), pix_fmt=pix_fmt, out_pix_fmt=_out_name(pix_fmt, out), stages=stages,
                                    cdl=grade, rgb_matrix=GAMUT)
            assert g.last_remote == 1 and (out is None or all(r0 % 2 == 0 for r0, _ in g.last_blocks)), g.last_blocks
            assert all(k.startswith("k_rgb_stack_") for k in g.last_kernels), g.last_kernels
            assert _eq(_host(got, _depth(pix_fmt, out)), want), (pix_fmt, w, h)


@pytest.mark.gpu
def test_resources_replaced_between_calls(loaded, l1ds, grade):
    """CDL a, b, a on one engine, and a 1D LUT replaced between calls: every call gives its own resources' planes."""
    src = _src("gbrp10le", "natural", W, H, nf=NF)
    other = Cdl(slope=(0.8, 1.1, 0.95), offset=(0.02, -0.01, 0.0), power=(1.2, 0.9, 1.0), saturation=1.3)
    for c in (grade, other, grade):
        assert _eq(_run(loaded, src, "gbrp10le", (10, "422"), "cdl,lut3d", c),
                   _want(loaded._res, "cdl,lut3d", c, None, "gbrp10le", (10, "422"), src, "orders"))
    first = _run(loaded, src, "gbrp10le", None, "lut1d,lut3d")
    assert _eq(first, _want(loaded._res, "lut1d,lut3d", None, None, "gbrp10le", None, src, "replace"))
    loaded.set_lut1d(l1ds["curve17"], "linear")
    res = dict(loaded._res, l1=(l1ds["curve17"], "linear"))
    second = _run(loaded, src, "gbrp10le", None, "lut1d,lut3d")
    assert _eq(second, _want(res, "lut1d,lut3d", None, None, "gbrp10le", None, src, "replace")) and not _eq(first, second)


# ------------------------------------------------------------------ child processes: table placement, grid-stride trips
def _worker(luts, env_change):
    env = {k: v for k, v in os.environ.items() if k not in ("LUTR_STACK_LDS", "LUTR_MAX_BLOCKS")}
    env.update(env_change)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "_gpu_rgbstack_worker.py"), str(luts["log709_33"][0]),
                        str(GOLDEN / "lut1d" / "gamma1024.cube"), str(GOLDEN / "cdl" / "shot.cc")], capture_output=True, cwd=ROOT,
                       timeout=180, env=env)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return r.stdout, [ln for ln in r.stderr.decode().splitlines() if ln.startswith("k_rgb_stack_vec<")]


@pytest.fixture(scope="module")
def default_run(luts):
    """The worker without either knob: its bytes and kernels, shared by the two comparisons below."""
    return _worker(luts, {})


@pytest.mark.gpu
def test_table_placement_gives_the_same_bytes(luts, default_run):
    """LUTR_STACK_LDS unset / 0 in child processes (the knob is read at launch): the same output bytes, and the placements that ran."""
    from tests._gpu_rgbstack_worker import CASES
    base, names = default_run
    placed = [n.split(">")[0][-1] for n in names]
    assert placed == ["1" if _lds(st, twin.source_depth(f)) else "0" for f, _o, st in CASES], names
    assert "1" in placed and "0" in placed and len(base) > 100000
    out, names0 = _worker(luts, {"LUTR_STACK_LDS": "0"})
    assert out == base and all(n.split(">")[0][-1] == "0" for n in names0), names0
    assert [n.replace(",1>", ",0>") for n in names] == names0


@pytest.mark.gpu
def test_grid_stride_trips_give_the_same_bytes(luts, default_run):
    """LUTR_MAX_BLOCKS=2 in a child process: two workgroups walk the 612 units of a 4:2:0 call in two trips and the 1224 of a
    full-size one in three, the last partial, behind one staging of the tables; the same bytes from the same kernels."""
    base, names = default_run
    out, names2 = _worker(luts, {"LUTR_MAX_BLOCKS": "2"})
    assert out == base and names2 == names


# ------------------------------------------------------------------ the C ABI's refusals
def _desc(tensors):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        st.data[i] = t.data_ptr()
        st.stride[i] = t.stride(-2) * t.element_size()
        st.frame_stride[i] = t.stride(0) * t.element_size() if t.dim() == 3 else 0
    return st


def _abi(engine, stages, w, h, s, d, *, cdl=None, mtx=None, src_kind=0, packed=None, dst_kind=0, fmt_out=None, lut_depth=10, nf=1,
         row0=0, rows=None, params=True):
    """lutr_apply_rgb_stack with raw (kind, interp) pairs; returns (rc, message)."""
    p = _native.YuvParams(_native.fmt_code(lut_depth, 0, 0), _native.fmt_code(10, 1, 1) if fmt_out is None else fmt_out, lut_depth,
                          1, 1, 0, 0, 0)
    arr = (_native.StageStruct * max(len(stages), 1))()
    for i, (kind, interp) in enumerate(stages):
        arr[i].kind, arr[i].interp = kind, interp
    k = None if cdl is None else C.byref(_native.cdl_struct(cdl))
    m = None if mtx is None else C.byref(mtx if isinstance(mtx, _native.RgbMatrixStruct) else _native.rgb_matrix_struct(mtx))
    with engine._lock:
        engine._bind_stream()
        rc = engine._lib.lutr_apply_rgb_stack(engine._ctx, C.byref(p) if params else None, arr, len(stages), k, m, src_kind, w, h, nf,
                                              None if s is None else C.byref(s), None if packed is None else C.byref(packed), dst_kind,
                                              C.byref(d), row0, h if rows is None else rows)
    return rc, engine._lib.lutr_last_error().decode()


@pytest.mark.gpu
def test_abi_refusals_leave_the_destination_untouched(loaded, grade):
    import torch
    from lut_renderer_amd.engine import LutEngine
    w, h = 64, 8
    src = _src("gbrp10le", "natural", w, h)
    dev = _dev(src, loaded.device)
    yuv = [torch.full((h >> (i > 0), w >> (i > 0)), 0x5a5a, dtype=torch.int16, device=loaded.device) for i in range(3)]
    rgb = [torch.full_like(t, 0x5a5a) for t in dev]
    s, dy, dr = _desc(dev), _desc(yuv), _desc(rgb)
    L3, L32, L1, CD, MX = 1, 2, 3, 4, 5
    huge = _native.rgb_matrix_struct(I3)             # an entry `rgbmatrix.RgbMatrix` itself refuses
    huge.m[0] = 1e9
    bad = [
        (dict(stages=[]), "1 to 4"),
        (dict(stages=[(L3, 2)] * 5), "1 to 4"),
        (dict(stages=[(9, 0)]), "unknown kind"),
        (dict(stages=[(L3, 2), (L3, 2)]), "listed twice"),
        (dict(stages=[(L3, 7)]), "interpolation mode"),
        (dict(stages=[(CD, 0)]), "CDL is null"),
        (dict(stages=[(L3, 2)], cdl=grade), "no cdl stage"),
        (dict(stages=[(MX, 0)]), "matrix is null"),
        (dict(stages=[(L3, 2)], mtx=I3), "no matrix stage"),
        (dict(stages=[(MX, 0)], mtx=huge), "65536"),
        (dict(stages=[(L3, 2)], dst_kind=3), "destination kind"),
        (dict(stages=[(L3, 2)], dst_kind=17), "destination kind"),
        (dict(stages=[(L3, 2)], params=False), "null yuv params"),
        (dict(stages=[(L3, 2)], row0=1, rows=h - 1), "chroma block"),
        (dict(stages=[(L3, 2)], rows=h + 1), "geometry"),
        (dict(stages=[(L3, 2)], src_kind=_native.packed_code(8, 3, 0, 1, 2), packed=_native.Packed(), s=None), "lut_depth"),
        (dict(stages=[(L3, 2)], src_kind=_native.packed_code(8, 3, 0, 1, 2), packed=_native.Packed(), s=None, dst_kind=10), "source's depth"),
    ]
    for kw, text in bad:
        kw = dict(kw)
        sk = kw.pop("s", s)
        d = dr if kw.get("dst_kind", 0) >= 8 else dy
        rc, msg = _abi(loaded, kw.pop("stages"), w, h, sk, d, **kw)
        assert rc == _native.EINVAL and text in msg, (kw, msg)
    # overlaps: a YUV destination on the source, and a gbrp destination that is not the source plane by plane
    rc, msg = _abi(loaded, [(L3, 2)], w, h, s, _desc([dev[0], yuv[1], yuv[2]]), fmt_out=_native.fmt_code(10, 1, 1))
    assert rc == _native.EINVAL and "in place" in msg, msg
    rc, msg = _abi(loaded, [(L3, 2)], w, h, s, _desc([dev[1], dev[0], dev[2]]), dst_kind=10)
    assert rc == _native.EINVAL and "overlaps" in msg, msg
    with _variant(loaded, "vec_lds"):
        rc, msg = _abi(loaded, [(L3, 2)], w, h, s, dy)
        assert rc == _native.EINVAL and "vec_lds" in msg, msg
    with _variant(loaded, "vec_global"):         # a prism stage, and a ragged width (w - 4 on these rows): no vector kernel
        for st, ww in (([(L3, 4)], w), ([(L3, 2)], w - 4)):
            rc, msg = _abi(loaded, st, ww, h, s, dy)
            assert rc == _native.EINVAL and "variant cannot take this layout" in msg, msg
    with LutEngine(0) as bare:
        for st, text in (([(L3, 2)], "no lattice"), ([(L32, 2)], "second lattice"), ([(L1, 0)], "1D LUT")):
            rc, msg = _abi(bare, st, w, h, s, dy)
            assert rc == _native.EINVAL and text in msg, msg
    torch.cuda.synchronize()
    assert all((t == 0x5a5a).all() for t in yuv + rgb) and _eq(_host(dev, 10), src)
    # and the calls the refusals surround do run
    rc, msg = _abi(loaded, [(L1, 0), (L3, 2)], w, h, s, dr, dst_kind=10, params=False)
    assert rc == 0, msg
    assert _eq(_host(rgb, 10), _want(loaded._res, "lut1d,lut3d", None, None, "gbrp10le", None, src, "abi"))


# ------------------------------------------------------------------ apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut_with_rgb_stages(loaded, luts, grade):
    from lut_renderer_amd.api import apply_lut
    stages = "lut1d,cdl,matrix,lut3d"
    src = _src("gbrp10le", "natural", W, H, nf=NF)
    common = dict(cube=luts["log709_33"][1], lut1d=GOLDEN / "lut1d" / "gamma1024.cube", interp1d="cubic", cdl=GOLDEN / "cdl" / "shot.cc",
                  rgb_matrix=GOLDEN / "matrix" / "bt2020_to_709.spimtx", rgb_stages=stages, pix_fmt="gbrp10le", engine=loaded)
    got, _tags = apply_lut(_dev(src, loaded.device), out_pix_fmt="yuv422p10le", **common)
    assert loaded.last_kernel == _vec_name("gbrp10le", (10, "422"), stages), loaded.last_kernel
    assert _eq(_host(got, 10), _want(loaded._res, stages, grade, GAMUT, "gbrp10le", (10, "422"), src, "api"))
    got, _tags = apply_lut(_dev(src, loaded.device), **common)
    assert _eq(_host(got, 10), _want(loaded._res, stages, grade, GAMUT, "gbrp10le", None, src, "api"))
    with pytest.raises(ValueError, match="stages"):
        apply_lut(_dev(src, loaded.device), stages="lut3d", **common)


@pytest.mark.gpu
def test_cli_over_pipes(loaded, luts, grade):
    stages = "lut1d,cdl,lut3d"
    for pix_fmt, out in (("rgb48le", (10, "420")), ("gbrp10le", None)):
        src = _src(pix_fmt, "natural", W, H, nf=NF, k=2)
        want = b"".join(b"".join(p[i].tobytes() for p in _want(loaded._res, stages, grade, None, pix_fmt, out, src, "cli")) for i in range(NF))
        raw = src.tobytes() if isinstance(src, np.ndarray) else b"".join(b"".join(p[i].tobytes() for p in src) for i in range(NF))
        cmd = [sys.executable, "-m", "lut_renderer_amd.cli", "-i", "-", "-o", "-", "--size", f"{W}x{H}", "--pix-fmt", pix_fmt,
               "--cube", str(luts["log709_33"][0]), "--lut1d", str(GOLDEN / "lut1d" / "gamma1024.cube"), "--interp1d", "cubic",
               "--cdl", str(GOLDEN / "cdl" / "shot.cc"), "--rgb-stages", stages]
        if out is not None:
            cmd += ["--out-pix-fmt", _yuv(*out)]
        r = subprocess.run(cmd, input=raw, capture_output=True, cwd=ROOT, timeout=180)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        assert r.stdout == want, (pix_fmt, out)
