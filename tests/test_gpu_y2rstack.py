"""The stage stack from YUV sources into RGB frames on the GPU: lutr_apply_yuv_stack_to_rgb bit for bit, whole
tensors, against the composition of tests/_y2rstack_twin.py, and against the existing entry points on the same engine where the
contracts meet.  The twin is fed the product's own host tables (lutr_cdl_table, lutr_lut1d_table), so that a last-bit difference
between two pows or cosf cannot fail a kernel test.  The tolerance is zero: the contract is a composition of pinned pieces."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.cdl import Cdl, read_cdl
from lut_renderer_amd.formats import parse_stages
from lut_renderer_amd.rgbmatrix import RgbMatrix, read_rgb_matrix
from tests import _y2rstack_twin as twin

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
GENERIC = "k_yuv2rgb_stack_generic"
#: 136 x 36, 2 frames: 17 units of 8 samples wide -- at 4:2:0 612 threads, two full workgroups and a partial one, across the frame
#: stride; under LUTR_MAX_BLOCKS=2 the grid stride makes more than one trip
W, H, NF = 136, 36, 2
I3 = RgbMatrix()
GAMUT = read_rgb_matrix(GOLDEN / "matrix" / "bt2020_to_709.spimtx")
DESTS = ("gbrp", "gbrp10le", "rgb24", "bgr24", "rgba", "bgra", "argb", "rgb48le", "rgba64le")
_refs = {}           # sources and expected codes, computed once per case and shared (never written to)


def _fmt(name):
    """(depth, layout key, alpha) of a planar YUV name."""
    from lut_renderer_amd.formats import parse_pix_fmt
    f = parse_pix_fmt(name)
    return f.depth, {(1, 1): "420", (1, 0): "422", (0, 0): "444"}[(f.csx, f.csy)], f.alpha


def _yuv(depth, lay, alpha=False):
    return f"yuv{'a' if alpha else ''}{lay}p" + ("" if depth == 8 else f"{depth}le")


def _gbrp(depth, alpha=False):
    return ("gbrap" if alpha else "gbrp") + ("" if depth == 8 else f"{depth}le")


def _t(a, device):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(device)


def _dev(planes, device):
    return [_t(p, device) for p in planes]


def _host(out, out_fmt):
    """What a call returned, as the twin arranges it: a list of planes or one image, unsigned."""
    wide = twin.dest_depth(out_fmt) > 8
    conv = lambda t: t.cpu().numpy().view(np.uint16) if wide else t.cpu().numpy()    # noqa: E731
    return conv(out) if out_fmt in twin.PACKED else [conv(t) for t in out]


def _eq(got, want):
    if isinstance(want, np.ndarray):
        return isinstance(got, np.ndarray) and got.shape == want.shape and np.array_equal(got, want)
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


def _vec_name(pix_fmt, out_fmt, stages, lds=None):
    din, lay, _a = _fmt(pix_fmt)
    icsx, icsy = LAYOUTS[lay]
    dl = twin.dest_depth(out_fmt)
    nc = twin.PACKED[out_fmt][1] if out_fmt in twin.PACKED else 1
    tri = int(any(m == "trilinear" for _, m in parse_stages(stages)))
    lds = _lds(stages, dl) if lds is None else lds
    return f"k_yuv2rgb_stack_vec<{int(din > 8)},{icsx},{icsy},{nc},{int(dl > 8)},{tri},{int(lds)}>" + _list(stages)


def _has_vec(pix_fmt, out_fmt, stages):
    """An 8-bit source written as 16-bit words has no vector kernel, nor has a pyramid / prism stage."""
    return not (_fmt(pix_fmt)[0] == 8 and twin.dest_depth(out_fmt) > 8) and all(m in (None,) + MODES[:3] for _, m in parse_stages(stages))


def _src(pix_fmt, dist, w, h, nf=1, k=0, full_range=False):
    """A host source: (Y, Cb, Cr), each [nf, h', w'] (or [h', w'])."""
    rk = ("src", pix_fmt, dist, w, h, nf, k, full_range)
    if rk not in _refs:
        din, lay, _a = _fmt(pix_fmt)
        icsx, icsy = LAYOUTS[lay]
        fs = [frames.make_yuv(dist, w, h, din, icsx, icsy, k=k + 7 * i, full_range=full_range) for i in range(nf)]
        _refs[rk] = list(fs[0]) if nf == 1 else [np.stack([f[i] for f in fs]) for i in range(3)]
    return _refs[rk]


def _frames_of(src):
    return [src] if src[0].ndim == 2 else [[p[i] for p in src] for i in range(src[0].shape[0])]


def _codes(res, stages, cdl, mtx, pix_fmt, dl, src, key, **yuv):
    """The twin's final (R, G, B) codes at depth dl for `src`, with the resources `res` (the `loaded` fixture's) and the product's
    own tables; shared by every destination of that depth."""
    st = parse_stages(stages)
    rk = (id(res["lut"]), id(res["lut2"]), id(res["l1"][0]), res["l1"][1], id(res["prelut"]), st,
          None if cdl is None else (cdl.sop_text(), cdl.saturation), None if mtx is None else (mtx.m, mtx.offset), pix_fmt, dl, key,
          tuple(sorted(yuv.items())))
    if rk not in _refs:
        din, lay, _a = _fmt(pix_fmt)
        icsx, icsy = LAYOUTS[lay]
        kinds = [s for s, _ in st]
        kw = dict(lut=res["lut"], lut2=res["lut2"], prelut=res["prelut"], cdl=cdl, mtx=mtx,
                  l1d_tab=_native.lut1d_table(*res["l1"], dl) if "lut1d" in kinds else None,
                  cdl_tab=_native.cdl_table(cdl, dl) if "cdl" in kinds else None)
        per = [twin.rgb_codes(st, _gbrp(dl), din, icsx, icsy, f[:3], **yuv, **kw) for f in _frames_of(src)]
        _refs[rk] = per
    return _refs[rk]


def _want(res, stages, cdl, mtx, pix_fmt, out_fmt, src, key, **yuv):
    per = [twin.arrange(out_fmt, c) for c in _codes(res, stages, cdl, mtx, pix_fmt, twin.dest_depth(out_fmt), src, key, **yuv)]
    if src[0].ndim == 2:
        return per[0]
    return np.stack(per) if out_fmt in twin.PACKED else [np.stack([f[i] for f in per]) for i in range(len(per[0]))]


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


def _run(engine, src, pix_fmt, out_fmt, stages, cdl=None, mtx=None, **kw):
    got = engine.apply_yuv_stack_to_rgb(_dev(src, engine.device), pix_fmt=pix_fmt, out_pix_fmt=out_fmt, stages=stages, cdl=cdl,
                                        rgb_matrix=mtx, **kw)
    return _host(got, out_fmt)


# ------------------------------------------------------------------ sources x destinations x variants
@pytest.mark.gpu
@pytest.mark.parametrize("pix_fmt", ["yuv420p", "yuv422p10le", "yuv444p10le", "yuv420p10le"])
def test_sources_destinations_and_variants(loaded, grade, pix_fmt):
    stages = "lut1d,cdl,lut3d"
    din = _fmt(pix_fmt)[0]
    src = _src(pix_fmt, "natural", W, H, nf=NF, k=din)
    for out_fmt in DESTS:
        want = _want(loaded._res, stages, grade, None, pix_fmt, out_fmt, src, "sweep")
        has_vec = _has_vec(pix_fmt, out_fmt, stages)
        got = _run(loaded, src, pix_fmt, out_fmt, stages, grade)
        assert loaded.last_kernel == (_vec_name(pix_fmt, out_fmt, stages) if has_vec else GENERIC + _list(stages)), loaded.last_kernel
        assert _eq(got, want), (pix_fmt, out_fmt, "auto")
        with _variant(loaded, "vec_global"):
            if has_vec:
                assert _eq(_run(loaded, src, pix_fmt, out_fmt, stages, grade), want), (pix_fmt, out_fmt, "vec_global")
                assert loaded.last_kernel == _vec_name(pix_fmt, out_fmt, stages)
            else:
                with pytest.raises(ValueError, match="vec_global cannot take an 8-bit source"):
                    _run(loaded, src, pix_fmt, out_fmt, stages, grade)
        with _variant(loaded, "generic"):
            got = _run(loaded, src, pix_fmt, out_fmt, stages, grade)
            assert loaded.last_kernel == GENERIC + _list(stages)
        assert _eq(got, want), (pix_fmt, out_fmt, "generic")


ORDERS = ("lut1d,cdl,lut3d", "cdl,lut3d", "lut3d,cdl,lut3d2", "cdl,lut1d", "lut1d,matrix,lut3d", "matrix,cdl,lut3d", "lut3d,matrix",
          "matrix,lut3d,lut3d2:trilinear")


@pytest.mark.gpu
@pytest.mark.parametrize("stages", ORDERS)
def test_orders_with_and_without_a_matrix(loaded, grade, stages):
    pix_fmt = "yuv420p10le"
    src = _src(pix_fmt, "natural", W, H, nf=NF)
    mtx = GAMUT if "matrix" in stages else None
    for sat in (1.0, 0.6) if "cdl" in stages else (None,):
        c = None if sat is None else _sat(grade, sat)
        for out_fmt in ("gbrp10le", "rgb24"):
            want = _want(loaded._res, stages, c, mtx, pix_fmt, out_fmt, src, "orders")
            got = _run(loaded, src, pix_fmt, out_fmt, stages, c, mtx)
            assert loaded.last_kernel == _vec_name(pix_fmt, out_fmt, stages), loaded.last_kernel
            assert _eq(got, want), (stages, sat, out_fmt, "vec")
            with _variant(loaded, "generic"):
                got = _run(loaded, src, pix_fmt, out_fmt, stages, c, mtx)
                assert loaded.last_kernel == GENERIC + _list(stages)
            assert _eq(got, want), (stages, sat, out_fmt, "generic")


@pytest.mark.gpu
@pytest.mark.parametrize("m1,m2", [("pyramid", "nearest"), ("trilinear", "prism"), ("tetrahedral", "trilinear"), ("nearest", "tetrahedral"),
                                   ("prism", "pyramid")])
def test_the_five_lut3d_modes_in_mixed_pairs(loaded, m1, m2):
    """Both lattices fed codes (all five modes in the twin); a pyramid or prism stage sends the call to the generic kernel."""
    stages = ("lut1d", ("lut3d", m1), ("lut3d2", m2))
    for pix_fmt, out_fmt in (("yuv422p10le", "gbrp10le"), ("yuv420p", "bgra")):
        src = _src(pix_fmt, "natural", W, H, nf=NF)
        all_vec = _has_vec(pix_fmt, out_fmt, stages)
        want = _want(loaded._res, stages, None, None, pix_fmt, out_fmt, src, "modes")
        got = _run(loaded, src, pix_fmt, out_fmt, stages)
        assert loaded.last_kernel == (_vec_name(pix_fmt, out_fmt, stages) if all_vec else GENERIC + _list(stages)), loaded.last_kernel
        assert _eq(got, want), (m1, m2, out_fmt)
        with _variant(loaded, "vec_global"):
            if all_vec:
                assert _eq(_run(loaded, src, pix_fmt, out_fmt, stages), want)
            else:
                with pytest.raises(ValueError, match="vec_global cannot take stage"):      # (before any GPU work)
                    _run(loaded, src, pix_fmt, out_fmt, stages)
        with _variant(loaded, "generic"):
            assert _eq(_run(loaded, src, pix_fmt, out_fmt, stages), want)


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
    pix_fmt = "yuv420p10le"
    src = _src(pix_fmt, "natural", W, H, nf=NF)
    dev = _dev(src, loaded.device)
    for stages in ("lut3d", "lut1d,lut3d", "lut3d,cdl,lut3d2", "cdl,lut1d,lut3d"):
        c = grade if "cdl" in stages else None
        for out_fmt in ("gbrp10le", "rgb48le"):
            got = _run(loaded, src, pix_fmt, out_fmt, stages, c)
            assert _eq(got, _want(res, stages, c, None, pix_fmt, out_fmt, src, "prelut")), (stages, out_fmt, loaded.last_kernel)
    # [lut3d] with a prelut is apply_yuv_to_rgb with a prelut
    for mode in ("tetrahedral", "prism"):
        ref = _host(loaded.apply_yuv_to_rgb(dev, pix_fmt=pix_fmt, out_pix_fmt="rgb48le", interp=mode), "rgb48le")
        assert _eq(_run(loaded, src, pix_fmt, "rgb48le", [("lut3d", mode)]), ref), mode
    for stages, mtx in (("cdl,lut3d", None), ("matrix,lut3d", I3)):
        with pytest.raises(ValueError, match="directly behind"):
            _run(loaded, src, pix_fmt, "gbrp10le", stages, grade if mtx is None else None, mtx)


# ------------------------------------------------------------------ depths and tables
@pytest.mark.gpu
@pytest.mark.parametrize("din,dl", [(8, 8), (10, 10), (10, 8), (12, 12), (16, 16), (8, 10), (10, 16)], ids=lambda v: str(v))
def test_depth_pairs(loaded, grade, din, dl):
    """(8, 10) has no vector kernel (an 8-bit source written as 16-bit words); every pair also runs the generic kernel."""
    pix_fmt = _yuv(din, "420")
    src = _src(pix_fmt, "uniform", W, H, nf=NF, k=2)
    for stages in ("lut1d,matrix,lut3d", "matrix,cdl,lut3d2"):
        c = grade if "cdl" in stages else None
        for out_fmt in (_gbrp(dl),) + ({8: ("bgra",), 16: ("rgb48le",)}.get(dl, ())):
            want = _want(loaded._res, stages, c, GAMUT, pix_fmt, out_fmt, src, "pairs")
            got = _run(loaded, src, pix_fmt, out_fmt, stages, c, GAMUT)
            name = _vec_name(pix_fmt, out_fmt, stages) if _has_vec(pix_fmt, out_fmt, stages) else GENERIC + _list(stages)
            assert loaded.last_kernel == name, loaded.last_kernel
            assert _eq(got, want), (stages, out_fmt, "auto")
            with _variant(loaded, "generic"):
                assert _eq(_run(loaded, src, pix_fmt, out_fmt, stages, c, GAMUT), want), (stages, out_fmt, "generic")
                assert loaded.last_kernel == GENERIC + _list(stages)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [12, 16])
def test_frames_whose_codes_reach_0_and_m(loaded, grade, depth):
    """12 bit: the 1D table alone fits LDS (24 KB exactly), the CDL's does not; 16 bit: everything in global memory."""
    m = (1 << depth) - 1
    pix_fmt = _yuv(depth, "420")
    src = [p.copy() for p in _src(pix_fmt, "uniform", 64, 8, k=2)]
    src[0][0, :8] = [0, m, 0, m, 1, m - 1, (m + 1) // 2, m]           # luma far outside the legal range: the conversion clips
    src[0][1, :8] = [m, 0, m, 0, m, 1, 0, m]
    src[1][0, :4] = [(m + 1) // 2, (m + 1) // 2, 0, m]
    src[2][0, :4] = [(m + 1) // 2, (m + 1) // 2, m, 0]
    r, g, b = twin.rgb_codes((("matrix", None),), _gbrp(depth), depth, 1, 1, src, mtx=I3)
    assert min(r.min(), g.min(), b.min()) == 0 and max(r.max(), g.max(), b.max()) == m
    for stages, lds in (("lut1d,lut3d", depth == 12), ("cdl,lut3d", False), ("lut1d,cdl", False), ("matrix", False)):
        c = grade if "cdl" in stages else None
        mtx = I3 if "matrix" in stages else None
        for out_fmt in (_gbrp(depth),) + (("rgba64le",) if depth == 16 else ()):
            got = _run(loaded, src, pix_fmt, out_fmt, stages, c, mtx)
            assert loaded.last_kernel == _vec_name(pix_fmt, out_fmt, stages, lds), loaded.last_kernel
            assert _eq(got, _want(loaded._res, stages, c, mtx, pix_fmt, out_fmt, src, ("ends", depth))), (stages, out_fmt)


# ------------------------------------------------------------------ sizes and layouts
@pytest.mark.gpu
def test_kernel_split_by_size(loaded, grade):
    """A ragged width on aligned (padded) rows: the vector kernel up to the last whole unit of 8 columns, the generic one for the
    rest -- 139 x 37 where the input block is one row high and 140 x 36 from 4:2:0; the padding keeps its sentinel.  139 x 37 from
    4:2:0 ends in half a block: the generic kernel's alone.  Then 16 x 4 and 67 x 21 on the generic kernel."""
    import torch
    pad = 160
    stages = "lut1d,cdl,lut3d"
    for (w, h), pix_fmt, out_fmt, name in (((139, 37), "yuv422p10le", "gbrp10le", "split"), ((139, 37), "yuv444p10le", "rgb48le", "split"),
                                           ((139, 37), "yuv422p", "rgb24", "split"), ((139, 37), "yuv420p10le", "gbrp10le", "generic"),
                                           ((140, 36), "yuv420p", "bgra", "split"), ((140, 36), "yuv420p10le", "gbrp10le", "split"),
                                           ((140, 36), "yuv420p10le", "rgb24", "split")):
        dl = twin.dest_depth(out_fmt)
        dt, fill = (torch.uint8, 0xA5) if dl == 8 else (torch.int16, -23131)                      # 0xA5A5
        src = _src(pix_fmt, "natural", w, h, k=4)
        want = _want(loaded._res, stages, grade, None, pix_fmt, out_fmt, src, ("split", w, h))
        sp = [torch.full((p.shape[0], pad), 77, dtype=p.dtype, device=loaded.device) for p in _dev(src, loaded.device)]
        for t, p in zip(sp, _dev(src, loaded.device)):
            t[:, :p.shape[1]] = p
        src_v = [t[:, :p.shape[1]] for t, p in zip(sp, src)]
        if out_fmt in twin.PACKED:
            dp = [torch.full((h, pad, twin.PACKED[out_fmt][1]), fill, dtype=dt, device=loaded.device)]
            dst_v = dp[0][:, :w]
        else:
            dp = [torch.full((h, pad), fill, dtype=dt, device=loaded.device) for _ in range(3)]
            dst_v = [t[:, :w] for t in dp]
        loaded.apply_yuv_stack_to_rgb(src_v, dst_v, pix_fmt=pix_fmt, out_pix_fmt=out_fmt, stages=stages, cdl=grade)
        if name == "split":
            assert loaded.last_kernel == _vec_name(pix_fmt, out_fmt, stages).replace("[", "+" + GENERIC + "[", 1), loaded.last_kernel
        else:
            assert loaded.last_kernel == GENERIC + _list(stages), loaded.last_kernel
        assert _eq(_host(dst_v, out_fmt), want), (w, h, pix_fmt, out_fmt)
        assert all(bool((t[:, w:] == fill).all()) for t in dp), (w, h, pix_fmt, out_fmt, "wrote into the padding")
        assert all(bool((t[:, p.shape[1]:] == 77).all()) for t, p in zip(sp, src)), "wrote into the source"
        with _variant(loaded, "vec_global"):
            with pytest.raises(_native.LutrError) as e:
                loaded.apply_yuv_stack_to_rgb(src_v, dst_v, pix_fmt=pix_fmt, out_pix_fmt=out_fmt, stages=stages, cdl=grade)
            assert e.value.code == _native.EINVAL
    for (w, h), pix_fmt, out_fmt in (((16, 4), "yuv422p10le", "gbrp10le"), ((67, 21), "yuv420p10le", "gbrp10le"),
                                     ((67, 21), "yuv420p", "bgra"), ((67, 21), "yuv422p10le", "rgb48le")):
        src = _src(pix_fmt, "natural", w, h, k=5)
        with _variant(loaded, "generic"):
            got = _run(loaded, src, pix_fmt, out_fmt, stages, grade)
            assert loaded.last_kernel == GENERIC + _list(stages)
        assert _eq(got, _want(loaded._res, stages, grade, None, pix_fmt, out_fmt, src, ("small", w, h))), (w, h, pix_fmt, out_fmt)
    # odd sizes under auto: no whole unit, or an odd height from 4:2:0 -- the generic kernel
    src = _src("yuv420p10le", "natural", 67, 21, k=5)
    assert _eq(_run(loaded, src, "yuv420p10le", "gbrp10le", stages, grade),
               _want(loaded._res, stages, grade, None, "yuv420p10le", "gbrp10le", src, ("small", 67, 21)))
    assert loaded.last_kernel == GENERIC + _list(stages)


def _desc(tensors):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        st.data[i] = t.data_ptr()
        st.stride[i] = t.stride(-2) * t.element_size()
        st.frame_stride[i] = t.stride(0) * t.element_size() if t.dim() == 3 else 0
    return st


def _abi(engine, stages, w, h, s, d_planar, d_packed=None, *, cdl=None, mtx=None, dst_kind=0, fmt_in=None, lut_depth=10, nf=1, row0=0,
         rows=None, params=True, range_src=0, range_in=0):
    """lutr_apply_yuv_stack_to_rgb with raw (kind, interp) pairs; returns (rc, message)."""
    p = _native.YuvParams(_native.fmt_code(10, 1, 1) if fmt_in is None else fmt_in, 0, lut_depth, 0, 0, range_src, range_in, 0)
    arr = (_native.StageStruct * max(len(stages), 1))()
    for i, (kind, interp) in enumerate(stages):
        arr[i].kind, arr[i].interp = kind, interp
    k = None if cdl is None else C.byref(_native.cdl_struct(cdl))
    m = None if mtx is None else C.byref(mtx if isinstance(mtx, _native.RgbMatrixStruct) else _native.rgb_matrix_struct(mtx))
    with engine._lock:
        engine._bind_stream()
        rc = engine._lib.lutr_apply_yuv_stack_to_rgb(engine._ctx, C.byref(p) if params else None, arr, len(stages), k, m, dst_kind, w, h,
                                                     nf, None if s is None else C.byref(s),
                                                     None if d_planar is None else C.byref(d_planar),
                                                     None if d_packed is None else C.byref(d_packed), row0, h if rows is None else rows)
    return rc, engine._lib.lutr_last_error().decode()


@pytest.mark.gpu
def test_negative_strides_and_a_misaligned_base_fall_to_the_generic_kernel(loaded, grade):
    import torch
    from lut_renderer_amd.engine import _packed_struct
    stages = "lut1d,cdl,lut3d"
    w, h = 64, 16
    pix_fmt = "yuv420p10le"
    f = _src(pix_fmt, "natural", w, h, k=6)
    # a base pointer one sample off the vector kernel's alignment: generic under auto, EINVAL under vec_global
    big = torch.zeros((h, w + 8), dtype=torch.int16, device=loaded.device)
    big[:, 1:w + 1] = _t(f[0], loaded.device)
    src = [big[:, 1:w + 1]] + _dev(f[1:], loaded.device)
    want = _want(loaded._res, stages, grade, None, pix_fmt, "gbrp10le", f, "odd")
    got = loaded.apply_yuv_stack_to_rgb(src, pix_fmt=pix_fmt, out_pix_fmt="gbrp10le", stages=stages, cdl=grade)
    assert loaded.last_kernel == GENERIC + _list(stages)
    assert _eq(_host(got, "gbrp10le"), want)
    dimg = torch.zeros((h, w + 2, 3), dtype=torch.uint8, device=loaded.device)
    dflat = dimg.view(-1)[1:1 + h * (w + 2) * 3 - 3].as_strided((h, w, 3), ((w + 2) * 3, 3, 1))      # one byte off a dword
    got = loaded.apply_yuv_stack_to_rgb(_dev(f, loaded.device), dflat, pix_fmt=pix_fmt, out_pix_fmt="rgb24", stages=stages, cdl=grade)
    assert loaded.last_kernel == GENERIC + _list(stages)
    assert _eq(_host(got, "rgb24"), _want(loaded._res, stages, grade, None, pix_fmt, "rgb24", f, "odd"))
    with _variant(loaded, "vec_global"):
        with pytest.raises(_native.LutrError) as e:
            loaded.apply_yuv_stack_to_rgb(src, pix_fmt=pix_fmt, out_pix_fmt="gbrp10le", stages=stages, cdl=grade)
        assert e.value.code == _native.EINVAL
    # negative row strides on both sides (bottom-up images; torch has none, so through the C ABI): the generic kernel
    L3, L1, CD = 1, 3, 4
    raw = [(L1, 0), (CD, 0), (L3, 2)]
    base = [_t(p[::-1], loaded.device) for p in f]                 # rows stored bottom-up
    st = _desc(base)
    for i, p in enumerate(f):
        st.data[i] = base[i].data_ptr() + (p.shape[0] - 1) * p.shape[1] * 2
        st.stride[i] = -p.shape[1] * 2
    dst = [torch.zeros((h, w), dtype=torch.int16, device=loaded.device) for _ in range(3)]
    d = _desc(dst)
    for i in range(3):
        d.data[i] = dst[i].data_ptr() + (h - 1) * w * 2
        d.stride[i] = -w * 2
    for variant, rc in (("auto", 0), ("vec_global", _native.EINVAL)):
        with _variant(loaded, variant):
            assert _abi(loaded, raw, w, h, st, d, cdl=grade)[0] == rc
    assert loaded.last_kernel == GENERIC + _list(stages)
    assert _eq([g[::-1] for g in _host(dst, "gbrp10le")], want)
    img = torch.zeros((h, w, 4), dtype=torch.uint8, device=loaded.device)
    pk = _packed_struct(img, "bgra", 4, 8, loaded.device, True)
    pk.data = img.data_ptr() + (h - 1) * w * 4
    pk.stride = -w * 4
    code = _native.packed_code(*_native.PACKED_FORMATS["bgra"])
    assert _abi(loaded, raw, w, h, st, None, pk, cdl=grade, dst_kind=code, lut_depth=8)[0] == 0
    assert loaded.last_kernel == GENERIC + _list(stages)
    assert _eq(_host(img, "bgra")[::-1], _want(loaded._res, stages, grade, None, pix_fmt, "bgra", f, "odd"))


# ------------------------------------------------------------------ where the contracts meet, on the same engine
@pytest.mark.gpu
def test_lut3d_alone_is_apply_yuv_to_rgb(loaded):
    for pix_fmt, outs in (("yuv420p10le", ("gbrp10le", "rgb48le", "rgb24")), ("yuv422p", ("gbrp", "bgra")), ("yuv444p10le", ("gbrp10le",))):
        src = _src(pix_fmt, "natural", W, H, nf=NF, k=1)
        dev = _dev(src, loaded.device)
        for out_fmt in outs:
            for mode in MODES:
                ref = _host(loaded.apply_yuv_to_rgb(dev, pix_fmt=pix_fmt, out_pix_fmt=out_fmt, interp=mode), out_fmt)
                got = _run(loaded, src, pix_fmt, out_fmt, [("lut3d", mode)])
                assert "k_yuv2rgb_stack_" in loaded.last_kernel
                assert _eq(got, ref), (pix_fmt, out_fmt, mode)


@pytest.mark.gpu
def test_identity_cdl_and_identity_matrix_are_the_conversion_alone(loaded):
    for pix_fmt, out_fmt in (("yuv420p", "gbrp"), ("yuv420p10le", "gbrp10le"), ("yuv422p12le", "gbrp12le"), ("yuv444p16le", "gbrp16le"),
                             ("yuv420p10le", "rgba64le"), ("yuv420p10le", "bgr24")):
        src = _src(pix_fmt, "uniform", 64, 8, k=3)
        ref = _host(loaded.apply_yuv_to_rgb(_dev(src, loaded.device), pix_fmt=pix_fmt, out_pix_fmt=out_fmt, lut=False), out_fmt)
        for variant in ("auto", "generic"):
            with _variant(loaded, variant):
                assert _eq(_run(loaded, src, pix_fmt, out_fmt, "cdl", Cdl()), ref), (pix_fmt, out_fmt, "cdl", variant)
                assert _eq(_run(loaded, src, pix_fmt, out_fmt, "matrix", None, I3), ref), (pix_fmt, out_fmt, "matrix", variant)


@pytest.mark.gpu
@pytest.mark.parametrize("lay", ["420", "422", "444"])
def test_any_list_is_the_rgb_stack_on_the_converted_planes(loaded, grade, lay):
    """apply_yuv_to_rgb(lut=False) into gbrp at dl, then apply_rgb_stack gbrp -> gbrp: the planar result; `arrange` for a packed one."""
    for din, dl in ((10, 10), (8, 8), (10, 16)):
        pix_fmt = _yuv(din, lay)
        src = _src(pix_fmt, "natural", W, H, nf=NF, k=2)
        dev = _dev(src, loaded.device)
        planes = loaded.apply_yuv_to_rgb(dev, pix_fmt=pix_fmt, out_pix_fmt=_gbrp(dl), lut=False)
        for stages in ("lut1d,cdl,lut3d", "matrix,lut3d"):
            c = grade if "cdl" in stages else None
            mtx = GAMUT if "matrix" in stages else None
            two = _host(loaded.apply_rgb_stack(planes, pix_fmt=_gbrp(dl), stages=stages, cdl=c, rgb_matrix=mtx), _gbrp(dl))
            assert _eq(_run(loaded, src, pix_fmt, _gbrp(dl), stages, c, mtx), two), (pix_fmt, dl, stages)
            g, b, r = two
            for out_fmt in {8: ("rgb24", "argb"), 10: (), 16: ("rgb48le", "rgba64le")}[dl]:
                assert _eq(_run(loaded, src, pix_fmt, out_fmt, stages, c, mtx), twin.arrange(out_fmt, (r, g, b))), (pix_fmt, out_fmt, stages)


# ------------------------------------------------------------------ other conditions
@pytest.mark.gpu
def test_every_matrix_and_range_and_the_pc_prologue(loaded, grade):
    stages = "lut1d,cdl,lut3d"
    for m in ("bt709", "smpte170m", "bt2020nc"):
        for rng in ("tv", "pc"):
            for pix_fmt, out_fmt in (("yuv420p10le", "gbrp10le"), ("yuv420p10le", "rgb24")):
                src = _src(pix_fmt, "natural", 64, 16, k=3, full_range=rng == "pc")
                got = _run(loaded, src, pix_fmt, out_fmt, stages, grade, matrix_in=m, range_src=rng)
                assert _eq(got, _want(loaded._res, stages, grade, None, pix_fmt, out_fmt, src, "mr", matrix=m, range_src=rng)), (m, rng, out_fmt)
    # the pc-source prologue lands at 8 bit: into rgb24
    for pix_fmt in ("yuv420p", "yuv422p10le"):
        src = _src(pix_fmt, "natural", 64, 16, k=8, full_range=True)
        want = _want(loaded._res, stages, grade, None, pix_fmt, "rgb24", src, "prologue", range_src="pc", range_in="tv")
        for variant in ("auto", "generic"):
            with _variant(loaded, variant):
                assert _eq(_run(loaded, src, pix_fmt, "rgb24", stages, grade, range_src="pc", range_in="tv"), want), (pix_fmt, variant)
    with pytest.raises(_native.LutrError, match="full-range"):           # a tv source has no range prologue, as in apply_yuv_to_rgb
        _run(loaded, _src("yuv444p10le", "natural", 64, 16), "yuv444p10le", "rgb24", stages, grade, range_src="tv", range_in="pc")


@pytest.mark.gpu
def test_alpha_is_carried_into_gbrap_and_dropped_for_gbrp(loaded, grade):
    stages = "lut1d,cdl,lut3d"
    src = _src("yuv420p10le", "natural", W, H, k=11)
    alpha = np.random.default_rng(3).integers(0, 1024, size=(H, W)).astype(np.uint16)
    dev = _dev(list(src) + [alpha], loaded.device)
    want = _want(loaded._res, stages, grade, None, "yuv420p10le", "gbrp10le", src, "alpha")
    got = loaded.apply_yuv_stack_to_rgb(dev, pix_fmt="yuva420p10le", out_pix_fmt="gbrap10le", stages=stages, cdl=grade)
    assert len(got) == 4 and "+k_alpha" in loaded.last_kernel and loaded.last_kernel.startswith("k_yuv2rgb_stack_vec<"), loaded.last_kernel
    got = _host(got, "gbrap10le")
    assert _eq(got[:3], want) and np.array_equal(got[3], alpha)
    got = loaded.apply_yuv_stack_to_rgb(dev, pix_fmt="yuva420p10le", out_pix_fmt="gbrp10le", stages=stages, cdl=grade)
    assert len(got) == 3 and _eq(_host(got, "gbrp10le"), want)
    # a source without alpha fills the plane opaque; alpha into a 4-component packed destination stays the follow-up
    got = _host(loaded.apply_yuv_stack_to_rgb(dev[:3], pix_fmt="yuv420p10le", out_pix_fmt="gbrap10le", stages=stages, cdl=grade), "gbrap10le")
    assert _eq(got[:3], want) and (got[3] == 1023).all()
    with pytest.raises(ValueError, match="a follow-up"):
        loaded.apply_yuv_stack_to_rgb(dev, pix_fmt="yuva420p10le", out_pix_fmt="rgba64le", stages=stages, cdl=grade)


@pytest.mark.gpu
def test_every_row_shard_on_the_block_rule(loaded, grade):
    stages = "lut3d,cdl,lut3d2"
    for pix_fmt, out_fmt in (("yuv420p10le", "gbrp10le"), ("yuv420p", "rgb24"), ("yuv422p10le", "rgba64le")):
        bh = 1 << LAYOUTS[_fmt(pix_fmt)[1]][1]
        kw = dict(pix_fmt=pix_fmt, out_pix_fmt=out_fmt, stages=stages, cdl=grade)
        for w, h in ((64, 22), (31, 23)):
            src = _src(pix_fmt, "natural", w, h, k=12)
            dev = _dev(src, loaded.device)
            whole = _want(loaded._res, stages, grade, None, pix_fmt, out_fmt, src, ("shard", w, h))
            assert _eq(_host(loaded.apply_yuv_stack_to_rgb(dev, **kw), out_fmt), whole)
            for r0 in range(bh, h, bh):                        # every (row0, rows) on the block rule, as a pair of calls
                out = loaded.apply_yuv_stack_to_rgb(dev, row0=0, rows=r0, **kw)
                loaded.apply_yuv_stack_to_rgb(dev, out, row0=r0, rows=h - r0, **kw)
                assert _eq(_host(out, out_fmt), whole), (out_fmt, w, h, r0)
            if bh == 2:
                with pytest.raises(_native.LutrError) as e:
                    loaded.apply_yuv_stack_to_rgb(dev, row0=1, rows=h - 1, **kw)
                assert e.value.code == _native.EINVAL and "block height" in e.value.message


@pytest.mark.gpu
def test_group_shards_with_remote_blocks(loaded, luts, l1ds, grade, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    stages = "lut1d,cdl,matrix,lut3d"
    for pix_fmt, (w, h), out_fmt in (("yuv420p10le", (W, H), "gbrp10le"), ("yuv420p10le", (34, 37), "rgb48le"), ("yuv444p", (33, 7), "bgra")):
        src = _src(pix_fmt, "natural", w, h, k=9)
        want = _want(loaded._res, stages, grade, GAMUT, pix_fmt, out_fmt, src, ("group", w))
        with LutEngineGroup([0, 0]) as g:
            assert g.treat_as_remote
            g.set_lut(luts["log709_33"][1])
            g.set_lut1d(l1ds["gamma1024"], "cubic")
            got = g.apply_yuv_stack_to_rgb(_dev(src, loaded.device), pix_fmt=pix_fmt, out_pix_fmt=out_fmt, stages=stages, cdl=grade,
                                           rgb_matrix=GAMUT)
            bh = 1 << LAYOUTS[_fmt(pix_fmt)[1]][1]
            assert g.last_remote == 1 and all(r0 % bh == 0 for r0, _ in g.last_blocks), g.last_blocks
            assert all(k.startswith("k_yuv2rgb_stack_") for k in g.last_kernels), g.last_kernels
            assert _eq(_host(got, out_fmt), want), (pix_fmt, w, h)


@pytest.mark.gpu
def test_resources_replaced_between_calls(loaded, l1ds, grade):
    """CDL a, b, a on one engine, and a 1D LUT replaced between calls: every call gives its own resources' frames."""
    pix_fmt = "yuv420p10le"
    src = _src(pix_fmt, "natural", W, H, nf=NF)
    other = Cdl(slope=(0.8, 1.1, 0.95), offset=(0.02, -0.01, 0.0), power=(1.2, 0.9, 1.0), saturation=1.3)
    for c in (grade, other, grade):
        assert _eq(_run(loaded, src, pix_fmt, "gbrp10le", "cdl,lut3d", c),
                   _want(loaded._res, "cdl,lut3d", c, None, pix_fmt, "gbrp10le", src, "orders"))
    first = _run(loaded, src, pix_fmt, "rgb24", "lut1d,lut3d")
    assert _eq(first, _want(loaded._res, "lut1d,lut3d", None, None, pix_fmt, "rgb24", src, "replace"))
    loaded.set_lut1d(l1ds["curve17"], "linear")
    res = dict(loaded._res, l1=(l1ds["curve17"], "linear"))
    second = _run(loaded, src, pix_fmt, "rgb24", "lut1d,lut3d")
    assert _eq(second, _want(res, "lut1d,lut3d", None, None, pix_fmt, "rgb24", src, "replace")) and not _eq(first, second)


# ------------------------------------------------------------------ child processes: table placement, grid-stride trips
def _worker(luts, env_change):
    env = {k: v for k, v in os.environ.items() if k not in ("LUTR_STACK_LDS", "LUTR_MAX_BLOCKS")}
    env.update(env_change)
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "_gpu_y2rstack_worker.py"), str(luts["log709_33"][0]),
                        str(GOLDEN / "lut1d" / "gamma1024.cube"), str(GOLDEN / "cdl" / "shot.cc")], capture_output=True, cwd=ROOT,
                       timeout=180, env=env)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return r.stdout, [ln for ln in r.stderr.decode().splitlines() if ln.startswith("k_yuv2rgb_stack_vec<")]


@pytest.fixture(scope="module")
def default_run(luts):
    """The worker without either knob: its bytes and kernels, shared by the two comparisons below."""
    return _worker(luts, {})


@pytest.mark.gpu
def test_table_placement_gives_the_same_bytes(luts, default_run):
    """LUTR_STACK_LDS unset / 0 in child processes (the knob is read at launch): the same output bytes, and the placements that ran."""
    from tests._gpu_y2rstack_worker import CASES
    base, names = default_run
    placed = [n.split(">")[0][-1] for n in names]
    assert placed == ["1" if _lds(st, twin.dest_depth(o)) else "0" for _f, o, st in CASES], names
    assert "1" in placed and "0" in placed and len(base) > 100000
    out, names0 = _worker(luts, {"LUTR_STACK_LDS": "0"})
    assert out == base and all(n.split(">")[0][-1] == "0" for n in names0), names0
    assert [n.replace(",1>", ",0>") for n in names] == names0


@pytest.mark.gpu
def test_grid_stride_trips_give_the_same_bytes(luts, default_run):
    """LUTR_MAX_BLOCKS=2 in a child process: two workgroups walk the 612 units of a 4:2:0 call in two trips and the 1224 of a
    4:2:2 or 4:4:4 one in three, the last partial, behind one staging of the tables; the same bytes from the same kernels."""
    base, names = default_run
    out, names2 = _worker(luts, {"LUTR_MAX_BLOCKS": "2"})
    assert out == base and names2 == names


# ------------------------------------------------------------------ the C ABI's refusals
@pytest.mark.gpu
def test_abi_refusals_leave_the_destination_untouched(loaded, grade):
    import torch
    from lut_renderer_amd.engine import LutEngine, _packed_struct
    w, h = 64, 8
    src = _src("yuv420p10le", "natural", w, h)
    dev = _dev(src, loaded.device)
    rgb = [torch.full((h, w), 0x5a5a, dtype=torch.int16, device=loaded.device) for _ in range(3)]
    img = torch.full((h, w, 3), 0x5a5a, dtype=torch.int16, device=loaded.device)
    s, d = _desc(dev), _desc(rgb)
    pk = _packed_struct(img, "rgb48le", 3, 16, loaded.device, True)
    rgb48 = _native.packed_code(*_native.PACKED_FORMATS["rgb48le"])
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
        (dict(stages=[(L3, 2)], params=False), "null yuv params"),
        (dict(stages=[(L3, 2)], row0=1, rows=h - 1), "chroma block"),
        (dict(stages=[(L3, 2)], rows=h + 1), "geometry"),
        (dict(stages=[(L3, 2)], fmt_in=_native.fmt_code(10, 0, 1)), "4:4:0"),
        (dict(stages=[(L3, 2)], fmt_in=_native.fmt_code(7, 1, 1)), "bit depth"),
        (dict(stages=[(L3, 2)], dst_kind=rgb48, lut_depth=10, packed=True), "lut_depth"),
        (dict(stages=[(L3, 2)], range_src=0, range_in=1), "full-range"),
    ]
    for kw, text in bad:
        kw = dict(kw)
        packed = kw.pop("packed", False)
        rc, msg = _abi(loaded, kw.pop("stages"), w, h, s, None if packed else d, pk if packed else None, **kw)
        assert rc == _native.EINVAL and text in msg, (kw, msg)
    # null sides; an overlap of the destination with a source plane
    assert _abi(loaded, [(L3, 2)], w, h, None, d)[0] == _native.EINVAL
    assert _abi(loaded, [(L3, 2)], w, h, s, None)[0] == _native.EINVAL
    rc, msg = _abi(loaded, [(L3, 2)], w, h, s, _desc([rgb[0], dev[0], rgb[2]]))
    assert rc == _native.EINVAL and "in place" in msg, msg
    with _variant(loaded, "vec_lds"):
        rc, msg = _abi(loaded, [(L3, 2)], w, h, s, d)
        assert rc == _native.EINVAL and "vec_lds" in msg, msg
    with _variant(loaded, "vec_global"):         # a prism stage, and a ragged width (w - 4 on these rows): no vector kernel
        for st, ww in (([(L3, 4)], w), ([(L3, 2)], w - 4)):
            rc, msg = _abi(loaded, st, ww, h, s, d)
            assert rc == _native.EINVAL and "variant cannot take this layout" in msg, msg
    with LutEngine(0) as bare:
        for st, text in (([(L3, 2)], "no lattice"), ([(L32, 2)], "second lattice"), ([(L1, 0)], "1D LUT")):
            rc, msg = _abi(bare, st, w, h, s, d)
            assert rc == _native.EINVAL and text in msg, msg
    torch.cuda.synchronize()
    assert all(bool((t == 0x5a5a).all()) for t in rgb + [img]) and _eq(_host(dev, "gbrp10le"), src)
    # and the calls the refusals surround do run
    rc, msg = _abi(loaded, [(L1, 0), (L3, 2)], w, h, s, d)
    assert rc == 0, msg
    assert _eq(_host(rgb, "gbrp10le"), _want(loaded._res, "lut1d,lut3d", None, None, "yuv420p10le", "gbrp10le", src, "abi"))
    rc, msg = _abi(loaded, [(L1, 0), (L3, 2)], w, h, s, None, pk, dst_kind=rgb48, lut_depth=16)
    assert rc == 0, msg
    assert _eq(_host(img, "rgb48le"), _want(loaded._res, "lut1d,lut3d", None, None, "yuv420p10le", "rgb48le", src, "abi"))
    # an empty call touches nothing and reads no plane
    assert _abi(loaded, [(L3, 2)], w, h, s, d, rows=0)[0] == 0


# ------------------------------------------------------------------ apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut_with_rgb_out_stages(loaded, luts, grade):
    from lut_renderer_amd.api import apply_lut
    stages = "lut1d,cdl,matrix,lut3d"
    pix_fmt = "yuv420p10le"
    src = _src(pix_fmt, "natural", W, H, nf=NF)
    common = dict(cube=luts["log709_33"][1], lut1d=GOLDEN / "lut1d" / "gamma1024.cube", interp1d="cubic", cdl=GOLDEN / "cdl" / "shot.cc",
                  rgb_matrix=GOLDEN / "matrix" / "bt2020_to_709.spimtx", rgb_out_stages=stages, pix_fmt=pix_fmt, colorspace="bt709",
                  engine=loaded)
    for out_fmt in ("rgb48le", "gbrp10le"):
        got, _tags = apply_lut(_dev(src, loaded.device), rgb_out=out_fmt, **common)
        assert loaded.last_kernel == _vec_name(pix_fmt, out_fmt, stages), loaded.last_kernel
        assert _eq(_host(got, out_fmt), _want(loaded._res, stages, grade, GAMUT, pix_fmt, out_fmt, src, "api"))
    with pytest.raises(ValueError, match="mutually exclusive"):
        apply_lut(_dev(src, loaded.device), rgb_out="rgb48le", stages="lut3d", **common)
    with pytest.raises(ValueError, match="it needs rgb_out"):
        apply_lut(_dev(src, loaded.device), **common)


@pytest.mark.gpu
def test_cli_over_pipes(loaded, luts, grade):
    stages = "lut1d,cdl,lut3d"
    for pix_fmt, out_fmt in (("yuv420p10le", "rgb48le"), ("yuv422p10le", "gbrp10le"), ("yuv420p", "rgba")):
        src = _src(pix_fmt, "natural", W, H, nf=NF, k=2)
        want = _want(loaded._res, stages, grade, None, pix_fmt, out_fmt, src, "cli", matrix="smpte170m")
        want = want.tobytes() if isinstance(want, np.ndarray) else b"".join(b"".join(p[i].tobytes() for p in want) for i in range(NF))
        raw = b"".join(b"".join(p[i].tobytes() for p in src) for i in range(NF))
        cmd = [sys.executable, "-m", "lut_renderer_amd.cli", "-i", "-", "-o", "-", "--size", f"{W}x{H}", "--pix-fmt", pix_fmt,
               "--cube", str(luts["log709_33"][0]), "--lut1d", str(GOLDEN / "lut1d" / "gamma1024.cube"), "--interp1d", "cubic",
               "--cdl", str(GOLDEN / "cdl" / "shot.cc"), "--rgb-out", out_fmt, "--rgb-out-stages", stages]
        r = subprocess.run(cmd, input=raw, capture_output=True, cwd=ROOT, timeout=180)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        assert r.stdout == want, (pix_fmt, out_fmt)
