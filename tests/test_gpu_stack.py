"""The stage stack on the GPU: lutr_apply_yuv_stack bit-exact, whole planes, against the composition in
tests/_stack_twin.py, and against the four dedicated entry points on the same engine.  The twin is fed the product's own host
tables (lutr_cdl_table, lutr_lut1d_table; pinned to the twins' own builds in tests/test_cdl.py and tests/test_lut1d.py), so that a
last-bit difference between two pows or cosf cannot fail a kernel test."""
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
from tests import _stack_twin as twin

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
GENERIC = "k_yuv_stack_generic"
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


def _list(stages):
    """The stage list as `last_kernel` spells it."""
    return "[" + ",".join(k if m is None else f"{k}:{MODES.index(m)}" for k, m in parse_stages(stages)) + "]"


def _vec_name(din, dout, a, b, stages, lds):
    (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
    tri = int(any(m == "trilinear" for _, m in parse_stages(stages)))
    return f"k_yuv_stack_vec<{int(din > 8)},{int(dout > 8)},{icsx},{icsy},{ocsx},{ocsy},{tri},{int(lds)}>" + _list(stages)


def _lds(stages, dl):
    """The default placement: the tables the stack uses fit 24 KB together."""
    kinds = [k for k, _ in parse_stages(stages)]
    size = (3 * (1 << dl) * 4 if "cdl" in kinds else 0) + (3 * (1 << dl) * 2 if "lut1d" in kinds else 0)
    return 0 < size <= 24 * 1024


@pytest.fixture(scope="module")
def luts(cube_dir):
    return {n: (cube_dir / f"{n}.cube", cube.read_lut(cube_dir / f"{n}.cube")) for n in ("log709_33", "random_9")}


@pytest.fixture(scope="module")
def l1ds():
    return {n: cube.read_lut1d(GOLDEN / "lut1d" / f"{n}.cube") for n in ("curve17", "gamma1024", "invert33")}


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


def _src(dist, w, h, depth, lay, k=1, nf=1, full_range=False):
    """(Y, Cb, Cr), each [nf, rows, cols] (or [rows, cols] for nf = 1)."""
    rk = ("src", dist, w, h, depth, lay, k, nf, full_range)
    if rk not in _refs:
        fs = [frames.make_yuv(dist, w, h, depth, *LAYOUTS[lay], k=k + 7 * i, full_range=full_range) for i in range(nf)]
        _refs[rk] = fs[0] if nf == 1 else [np.stack([f[i] for f in fs]) for i in range(3)]
    return _refs[rk]


def _want(res, stages, cdl, din, dl, dout, a, b, src, key, rin="tv", prologue=False):
    """The twin's planes for `src` ([rows, cols] or [nf, rows, cols] planes) with the resources `res` (the `loaded` fixture's) and
    the product's own tables at dl."""
    st = parse_stages(stages)
    rk = (id(res["lut"]), id(res["lut2"]), id(res["l1"][0]), res["l1"][1], st, None if cdl is None else (cdl.sop_text(), cdl.saturation),
          din, dl, dout, a, b, key, rin, prologue)
    if rk not in _refs:
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        k = twin.consts("bt709", rin, "bt709", "tv", din, dl, dout, ocsx, ocsy, prologue=prologue)
        kinds = [s for s, _ in st]
        kw = dict(lut=res["lut"], lut2=res["lut2"], prelut=res["prelut"], cdl=cdl,
                  l1d_tab=_native.lut1d_table(*res["l1"], dl) if "lut1d" in kinds else None,
                  cdl_tab=_native.cdl_table(cdl, dl) if "cdl" in kinds else None)
        if src[0].ndim == 2:
            _refs[rk] = twin.apply(st, k, dl, dout, icsx, icsy, ocsx, ocsy, src, **kw)
        else:
            per = [twin.apply(st, k, dl, dout, icsx, icsy, ocsx, ocsy, [p[i] for p in src], **kw) for i in range(src[0].shape[0])]
            _refs[rk] = [np.stack([f[i] for f in per]) for i in range(3)]
    return _refs[rk]


# ------------------------------------------------------------------ layouts, orders, container mixes, modes
@pytest.mark.gpu
@pytest.mark.parametrize("a", list(LAYOUTS))
@pytest.mark.parametrize("b", list(LAYOUTS))
def test_all_nine_layout_pairs_at_10_bit(loaded, grade, a, b):
    stages = "lut1d,cdl,lut3d"
    src = _src("natural", W, H, 10, a, nf=NF)
    got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), stages=stages, cdl=grade)
    assert loaded.last_kernel == _vec_name(10, 10, a, b, stages, True), loaded.last_kernel
    assert _eq(_host(got, 10), _want(loaded._res, stages, grade, 10, 10, 10, a, b, src, "nine"))


ORDERS = ("cdl", "lut3d,lut1d", "lut3d,cdl", "cdl,lut1d,lut3d", "lut3d,cdl,lut3d2", "lut3d2,lut3d", "lut1d,lut3d,lut3d2",
          "lut1d,cdl,lut3d,lut3d2", "cdl,lut3d,lut3d2,lut1d")


@pytest.mark.gpu
@pytest.mark.parametrize("stages", ORDERS)
def test_orders_on_420_to_422(loaded, grade, stages):
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, loaded.device)
    for sat in ((1.0, 0.6) if "cdl" in stages else (None,)):
        c = None if sat is None else _sat(grade, sat)
        got = loaded.apply_yuv_stack(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, cdl=c)
        assert loaded.last_kernel == _vec_name(10, 10, "420", "422", stages, _lds(stages, 10)), loaded.last_kernel
        assert _eq(_host(got, 10), _want(loaded._res, stages, c, 10, 10, 10, "420", "422", src, "orders")), sat
    with _variant(loaded, "generic"):
        c = _sat(grade, 0.6) if "cdl" in stages else None
        got = loaded.apply_yuv_stack(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, cdl=c)
        assert loaded.last_kernel == GENERIC + _list(stages)
    assert _eq(_host(got, 10), _want(loaded._res, stages, c, 10, 10, 10, "420", "422", src, "orders"))


@pytest.mark.gpu
@pytest.mark.parametrize("din,dout", [(8, 8), (10, 8), (16, 8), (8, 10), (12, 12)], ids=lambda v: str(v))
def test_container_mixes_on_420_to_422(loaded, grade, din, dout):
    src = _src("uniform", W, H, din, "420", nf=NF)
    for stages in ("lut1d,cdl,lut3d", "lut3d,cdl,lut3d2"):
        got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(din, "420"), out_pix_fmt=_fmt(dout, "422"), stages=stages,
                                     cdl=grade)
        # an 8-bit source written as 16-bit words has no vector kernel
        name = GENERIC + _list(stages) if din == 8 and dout > 8 else _vec_name(din, dout, "420", "422", stages, _lds(stages, din))
        assert loaded.last_kernel == name, loaded.last_kernel
        assert _eq(_host(got, dout), _want(loaded._res, stages, grade, din, din, dout, "420", "422", src, "mix")), stages


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [12, 16])
def test_both_ends_of_the_tables_are_read(loaded, grade, depth):
    """A frame whose RGB reaches codes 0 and M.  16 bit: 3 x 65536 tables in global memory.  12 bit: the 1D table alone is the
    largest that goes to LDS (24 KB); with a CDL (48 KB more) the tables are read from global memory."""
    from oracle.lut3d_numpy import yuv_to_rgb_codes
    m = (1 << depth) - 1
    src = [p.copy() for p in _src("uniform", 64, 8, depth, "420", k=2)]
    src[0][0, :8] = [0, m, 0, m, 1, m - 1, (m + 1) // 2, m]
    src[1][0, :4] = [0, m, (m + 1) // 2, (m + 1) // 2]
    src[2][0, :4] = [m, 0, (m + 1) // 2, (m + 1) // 2]
    k = twin.consts("bt709", "tv", "bt709", "tv", depth, depth, depth, 1, 1)
    rgb = yuv_to_rgb_codes(k, 1, 1, src)
    assert min(int(c.min()) for c in rgb) == 0 and max(int(c.max()) for c in rgb) == m
    for stages, lds in (("lut1d", depth == 12), ("lut3d,lut1d", depth == 12), ("cdl,lut1d", False), ("lut1d,cdl,lut3d", False)):
        c = grade if "cdl" in stages else None
        got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(depth, "420"), stages=stages, cdl=c)
        assert loaded.last_kernel == _vec_name(depth, depth, "420", "420", stages, lds), loaded.last_kernel
        assert _eq(_host(got, depth), _want(loaded._res, stages, c, depth, depth, depth, "420", "420", src, ("ends", depth))), stages


@pytest.mark.gpu
@pytest.mark.parametrize("m1,m2", [("pyramid", "nearest"), ("trilinear", "prism"), ("tetrahedral", "trilinear"), ("nearest", "tetrahedral"),
                                   ("prism", "pyramid")])
def test_modes_in_mixed_pairs(loaded, grade, m1, m2):
    """nearest / trilinear / tetrahedral on the vector kernel, each stage its own; a pyramid or prism stage sends the call to the
    generic kernel.  (The twin feeds pyramid / prism codes: behind the CDL it has the three vector modes.)"""
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, loaded.device)
    vec = m1 in MODES[:3] and m2 in MODES[:3]
    for stages, c in (((("lut3d", m1), ("lut3d2", m2)), None), (("lut1d", ("lut3d2", m2), "cdl", ("lut3d", "tetrahedral" if not vec else m1)), grade)):
        names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, cdl=c)
        want = _want(loaded._res, stages, c, 10, 10, 10, "420", "422", src, "modes")
        got = loaded.apply_yuv_stack(dev, **names)
        all_vec = all(m in MODES[:3] for _, m in parse_stages(stages) if m)
        assert loaded.last_kernel == (_vec_name(10, 10, "420", "422", stages, _lds(stages, 10)) if all_vec else GENERIC + _list(stages))
        assert _eq(_host(got, 10), want), stages
        with _variant(loaded, "vec_global"):
            if all_vec:
                assert _eq(_host(loaded.apply_yuv_stack(dev, **names), 10), want)
            else:
                with pytest.raises(_native.LutrError) as e:
                    loaded.apply_yuv_stack(dev, **names)
                assert e.value.code == _native.EINVAL
        with _variant(loaded, "generic"):
            assert _eq(_host(loaded.apply_yuv_stack(dev, **names), 10), want)
            assert loaded.last_kernel == GENERIC + _list(stages)


# ------------------------------------------------------------------ shapes
@pytest.mark.gpu
def test_ragged_widths_and_small_frames(loaded, grade):
    """Padded (aligned) rows whose width is no multiple of the thread's unit: the vector kernel up to column 136, the generic kernel
    for the rest -- 139 x 37 on 4:2:2 -> 4:4:4 (union block height 1) and 139 x 36 / 140 x 36 on the pairs with 4:2:0.  139 x 37
    with a 4:2:0 side ends in half a union block: the generic kernel's alone.  Then 16 x 4 and 67 x 21 on the generic kernel."""
    import torch
    pad = 160
    stages = "lut1d,cdl,lut3d"
    for (w, h), depth, a, b, name in (((139, 36), 10, "420", "422", "split"), ((139, 37), 10, "422", "444", "split"),
                                      ((139, 37), 10, "420", "422", "generic"), ((140, 36), 8, "444", "420", "split")):
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        dt, fill = (torch.uint8, 255) if depth == 8 else (torch.int16, -1)
        src = _src("natural", w, h, depth, a, k=4)
        sp = [torch.zeros((p.shape[0], pad), dtype=dt, device=loaded.device) for p in src]
        for t, p in zip(sp, _dev(src, loaded.device)):
            t[:, :p.shape[1]] = p
        src_v = [t[:, :p.shape[1]] for t, p in zip(sp, src)]
        oshape = [(h, w)] + [frames.chroma_shape(w, h, ocsx, ocsy)] * 2
        dp = [torch.full((s[0], pad), fill, dtype=dt, device=loaded.device) for s in oshape]
        dst_v = [t[:, :s[1]] for t, s in zip(dp, oshape)]
        loaded.apply_yuv_stack(src_v, dst_v, pix_fmt=_fmt(depth, a), out_pix_fmt=_fmt(depth, b), stages=stages, cdl=grade)
        if name == "split":
            vec = _vec_name(depth, depth, a, b, stages, True)
            assert loaded.last_kernel == vec.replace("[", "+" + GENERIC + "[", 1), loaded.last_kernel
            assert "+k_yuv_stack_generic" in loaded.last_kernel
        else:
            assert loaded.last_kernel == GENERIC + _list(stages), loaded.last_kernel
        assert _eq(_host(dst_v, depth), _want(loaded._res, stages, grade, depth, depth, depth, a, b, src, ("ragged", w, h))), (w, h, a, b)
        assert all((t[:, s[1]:] == fill).all() for t, s in zip(dp, oshape)), "wrote past the row"
    for (w, h), a, b in (((16, 4), "420", "422"), ((67, 21), "420", "422"), ((67, 21), "444", "420")):
        src = _src("natural", w, h, 10, a, k=5)
        with _variant(loaded, "generic"):
            got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), stages=stages, cdl=grade)
            assert loaded.last_kernel == GENERIC + _list(stages)
        assert _eq(_host(got, 10), _want(loaded._res, stages, grade, 10, 10, 10, a, b, src, ("small", w, h))), (w, h, a, b)


# ------------------------------------------------------------------ other paths
@pytest.mark.gpu
def test_full_range_prologue(loaded, grade):
    """A full-range 8-bit source with range_in="tv": lutr_apply_yuv's prologue ahead of the stack."""
    src = _src("natural", W, H, 8, "420", k=6, nf=NF, full_range=True)
    for stages in ("lut1d,cdl,lut3d", "cdl"):
        got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt="yuv420p", out_pix_fmt="yuv422p", range_src="pc", range_in="tv",
                                     lut_depth=8, stages=stages, cdl=grade)
        assert loaded.last_kernel == _vec_name(8, 8, "420", "422", stages, True)
        assert _eq(_host(got, 8), _want(loaded._res, stages, grade, 8, 8, 8, "420", "422", src, "pc", rin="tv", prologue=True)), stages


@pytest.mark.gpu
def test_a_csp_prelut_on_the_first_lattice(loaded, grade, tmp_path):
    from oracle import binding as orc
    from tests._csp_files import write_csp_with_prelut
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, cube.log709_lattice(17), shapers)
    lut = loaded.load_cube(p)
    assert lut.prelut is not None
    res = dict(loaded._res, lut=lut, prelut=orc.parse_lut_file_ex(p)[3])
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, loaded.device)
    for stages in ("lut1d,lut3d", "lut3d,cdl,lut3d2", "cdl,lut1d,lut3d"):
        c = grade if "cdl" in stages else None
        got = loaded.apply_yuv_stack(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, cdl=c)
        assert _eq(_host(got, 10), _want(res, stages, c, 10, 10, 10, "420", "422", src, "prelut")), (stages, loaded.last_kernel)
    with pytest.raises(ValueError, match="directly behind 'cdl'"):
        loaded.apply_yuv_stack(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages="cdl,lut3d", cdl=grade)
    out = [t.clone() for t in dev]
    rc, msg = _abi(loaded, [(4, 0), (1, 2)], grade, 1, W, H, _desc(dev), _desc(out), nf=NF)
    assert rc == _native.EINVAL and "prelut" in msg, msg


@pytest.mark.gpu
def test_the_four_dedicated_entry_points_bit_for_bit(loaded, grade):
    """The stack kernel against the four kernel families that already serve a stack, on the same engine and source."""
    for a, b in (("420", "422"), ("420", "420"), ("444", "444")):
        src = _src("natural", W, H, 10, a, nf=NF)
        dev = _dev(src, loaded.device)
        names = dict(pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b))
        for mode in ("tetrahedral", "trilinear", "prism"):
            plain = _host(loaded.apply_yuv(dev, interp=mode, **names), 10)
            assert _eq(_host(loaded.apply_yuv_stack(dev, stages=[("lut3d", mode)], **names), 10), plain), (a, b, mode, "lut3d")
            assert "k_yuv_stack_" in loaded.last_kernel
            for c in (grade, _sat(grade, 1.0)):
                ref = _host(loaded.apply_yuv(dev, interp=mode, cdl=c, **names), 10)
                assert _eq(_host(loaded.apply_yuv_stack(dev, stages=["cdl", ("lut3d", mode)], cdl=c, **names), 10), ref), (a, b, mode, "cdl")
            ref = _host(loaded.apply_yuv_lut1d(dev, interp=mode, **names), 10)
            assert _eq(_host(loaded.apply_yuv_stack(dev, stages=["lut1d", ("lut3d", mode)], **names), 10), ref), (a, b, mode, "lut1d")
            ref = _host(loaded.apply_yuv_chain(dev, interp=mode, interp2="tetrahedral", **names), 10)
            got = loaded.apply_yuv_stack(dev, stages=[("lut3d", mode), ("lut3d2", "tetrahedral")], **names)
            assert _eq(_host(got, 10), ref), (a, b, mode, "chain")
        ref = _host(loaded.apply_yuv_lut1d(dev, interp=None, **names), 10)
        assert _eq(_host(loaded.apply_yuv_stack(dev, stages="lut1d", **names), 10), ref), (a, b, "lut1d alone")


@pytest.mark.gpu
def test_the_identity_cdl_alone_is_the_two_conversions(loaded):
    from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
    for depth in (8, 10, 12, 16):
        src = _src("uniform", 64, 8, depth, "420", k=3)
        k = twin.consts("bt709", "tv", "bt709", "tv", depth, depth, depth, 1, 0)
        got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(depth, "420"), out_pix_fmt=_fmt(depth, "422"), stages="cdl", cdl=Cdl())
        assert _eq(_host(got, depth), rgb_codes_to_yuv(k, depth, 1, 0, yuv_to_rgb_codes(k, 1, 1, src))), depth


@pytest.mark.gpu
def test_row_shards_are_the_whole_call(loaded, grade):
    import torch
    stages = "lut3d,cdl,lut3d2"
    src = _src("uniform", W, H, 10, "420", nf=NF)
    dev = _dev(src, loaded.device)
    for b, variant in (("420", "auto"), ("422", "auto"), ("444", "generic")):
        ocsy = LAYOUTS[b][1]
        names = dict(pix_fmt="yuv420p10le", out_pix_fmt=_fmt(10, b), stages=stages, cdl=grade)
        whole = _want(loaded._res, stages, grade, 10, 10, 10, "420", b, src, "shard")
        with _variant(loaded, variant):
            out = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=loaded.device) for p in whole]
            loaded.apply_yuv_stack(dev, out, row0=10, rows=14, **names)
            got = _host(out, 10)
            for i, (g, wh) in enumerate(zip(got, whole)):
                r0, r1 = (10, 24) if i == 0 else (10 >> ocsy, 24 >> ocsy)
                assert np.array_equal(g[:, r0:r1], wh[:, r0:r1]), (b, variant, i)
                assert (g[:, :r0] == 0x5a5a).all() and (g[:, r1:] == 0x5a5a).all(), (b, variant, i, "wrote outside the block")
            loaded.apply_yuv_stack(dev, out, row0=0, rows=10, **names)
            loaded.apply_yuv_stack(dev, out, row0=24, rows=H - 24, **names)
        assert _eq(_host(out, 10), whole), (b, variant)
    with pytest.raises(_native.LutrError, match="union") as e:
        loaded.apply_yuv_stack(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, cdl=grade, row0=1, rows=H - 1)
    assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_group_shards_on_the_union_block(loaded, luts, l1ds, grade, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    stages = "lut1d,cdl,lut3d,lut3d2"
    for (w, h), a, b in (((W, H), "420", "422"), ((33, 7), "422", "420")):
        src = _src("natural", w, h, 10, a, k=9)
        want = _want(loaded._res, stages, grade, 10, 10, 10, a, b, src, ("group", w))
        with LutEngineGroup([0, 0]) as g:
            assert g.treat_as_remote
            g.set_lut(luts["log709_33"][1])
            g.set_lut2(luts["random_9"][1])
            g.set_lut1d(l1ds["gamma1024"], "cubic")
            got = g.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), stages=stages, cdl=grade)
            assert g.last_remote == 1 and all(r0 % 2 == 0 for r0, _ in g.last_blocks), g.last_blocks
            assert all(k.startswith("k_yuv_stack_") for k in g.last_kernels), g.last_kernels
            assert _eq(_host(got, 10), want), (w, h)


@pytest.mark.gpu
def test_a_yuva_frame_carries_its_alpha_past_the_stack(loaded, grade):
    stages = "lut1d,cdl,lut3d"
    src = _src("natural", W, H, 10, "444", k=11)
    alpha = np.random.default_rng(3).integers(0, 1024, size=(H, W)).astype(np.uint16)
    got = loaded.apply_yuv_stack(_dev(list(src) + [alpha], loaded.device), pix_fmt="yuva444p10le", stages=stages, cdl=grade)
    assert loaded.last_kernel.startswith(_vec_name(10, 10, "444", "444", stages, True) + "+k_alpha_"), loaded.last_kernel
    out = _host(got, 10)
    assert len(out) == 4 and np.array_equal(out[3], alpha)
    assert _eq(out[:3], _want(loaded._res, stages, grade, 10, 10, 10, "444", "444", src, "yuva"))


# ------------------------------------------------------------------ engine state
@pytest.mark.gpu
def test_cdl_a_b_a_and_a_replaced_1d_lut(loaded, grade, l1ds):
    """Per-clip CDLs on one engine with no host wait in between: each call uses the table of the CDL it was issued with; then the
    1D LUT replaced between two calls."""
    stages = "lut1d,cdl,lut3d"
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, loaded.device)
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages)
    other = Cdl(slope=(0.8, 1.2, 1.0), offset=(0.05, -0.02, 0.0), power=(1.3, 0.9, 1.0), saturation=1.25)
    order = [grade, other, grade]
    outs = [loaded.apply_yuv_stack(dev, cdl=c, **names) for c in order]
    for got, c in zip(outs, order):
        assert _eq(_host(got, 10), _want(loaded._res, stages, c, 10, 10, 10, "420", "422", src, "aba"))
    assert not _eq(_host(outs[0], 10), _host(outs[1], 10))
    outs = []
    for n, m in (("gamma1024", "cubic"), ("invert33", "linear"), ("gamma1024", "cubic")):
        loaded.set_lut1d(l1ds[n], m)
        outs.append((loaded.apply_yuv_stack(dev, cdl=grade, **names), dict(loaded._res, l1=(l1ds[n], m))))
    for got, res in outs:
        assert _eq(_host(got, 10), _want(res, stages, grade, 10, 10, 10, "420", "422", src, "aba"))
    loaded.set_lut1d(None)
    with pytest.raises(ValueError, match="no 1D LUT is loaded"):
        loaded.apply_yuv_stack(dev, cdl=grade, **names)


# ------------------------------------------------------------------ refusals at the ABI
def _desc(tensors):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        st.data[i] = t.data_ptr()
        st.stride[i] = t.stride(-2) * t.element_size()
        st.frame_stride[i] = t.stride(0) * t.element_size() if t.dim() == 3 else 0
    return st


def _raw_cdl(slope=(1.0, 1.0, 1.0), power=(1.0, 1.0, 1.0)):
    """struct lutr_cdl with numbers `cdl.Cdl` itself refuses."""
    st = _native.cdl_struct(Cdl())
    for i in range(3):
        st.slope[i], st.power[i] = slope[i], power[i]
    return st


def _abi(engine, stages, cdl, csy_out, w, h, s, d, nf=1, fmt_in=None):
    """lutr_apply_yuv_stack with raw (kind, interp) pairs at 10 bit, 4:2:0 in, 4:2:0 / 4:2:2 out; returns (rc, message)."""
    p = _native.YuvParams(_native.fmt_code(10, 1, 1) if fmt_in is None else fmt_in, _native.fmt_code(10, 1, csy_out), 10, 0, 0, 0, 0, 0)
    arr = (_native.StageStruct * max(len(stages), 1))()
    for i, (kind, interp) in enumerate(stages):
        arr[i].kind, arr[i].interp = kind, interp
    k = None if cdl is None else C.byref(cdl if isinstance(cdl, _native.CdlStruct) else _native.cdl_struct(cdl))
    with engine._lock:
        engine._bind_stream()
        rc = engine._lib.lutr_apply_yuv_stack(engine._ctx, C.byref(p), arr, len(stages), k, w, h, nf, C.byref(s), C.byref(d), 0, h)
    return rc, engine._lib.lutr_last_error().decode()


@pytest.mark.gpu
def test_refusals_leave_the_destination_untouched(loaded, grade):
    import torch
    from lut_renderer_amd.engine import LutEngine
    w, h = 64, 8
    src = _src("natural", w, h, 10, "420")
    dev = _dev(src, loaded.device)
    out = [torch.full_like(t, 0x5a5a) for t in dev]
    s, d = _desc(dev), _desc(out)
    L3, L32, L1, CD = 1, 2, 3, 4
    for stages, c, word in (([], None, "1 to 4"), ([(L3, 2)] * 5, None, "1 to 4"), ([(7, 0)], None, "unknown kind 7"),
                            ([(L3, 2), (L1, 0), (L3, 2)], None, "listed twice"), ([(L3, 5)], None, "interpolation mode 5"),
                            ([(L32, -1)], None, "interpolation mode -1"), ([(CD, 0), (L3, 2)], None, "the CDL is null"),
                            ([(L3, 2)], grade, "no cdl stage is listed"),
                            ([(CD, 0), (L3, 2)], _raw_cdl(slope=(-1.0, 1.0, 1.0)), "slope of R is negative"),
                            ([(CD, 0), (L3, 2)], _raw_cdl(power=(1.0, 0.0, 1.0)), "power of G must be above 0")):
        rc, msg = _abi(loaded, stages, c, 1, w, h, s, d)
        assert rc == _native.EINVAL and word in msg, (stages, msg)
    with _variant(loaded, "vec_lds"):
        rc, msg = _abi(loaded, [(L1, 0), (L3, 2)], None, 1, w, h, s, d)
        assert rc == _native.EINVAL and "vec_lds" in msg, msg
    rc, msg = _abi(loaded, [(L3, 2)], None, 1, w, h, s, s)
    assert rc == _native.EINVAL and "cannot run in place: the byte range of source plane 0 overlaps" in msg, msg
    inside = [out[0], dev[0][:h // 2, :w // 2], out[2]]
    rc, msg = _abi(loaded, [(L3, 2)], None, 1, w, h, s, _desc(inside))
    assert rc == _native.EINVAL and "source plane 0 overlaps that of destination plane 1" in msg, msg
    with pytest.raises(ValueError, match="stack pass cannot run in place"):
        loaded.apply_yuv_stack(dev, dev, pix_fmt="yuv420p10le", stages="lut3d")
    rc, msg = _abi(loaded, [(L3, 2)], None, 1, w, h, s, d, fmt_in=_native.fmt_code(10, 0, 1))      # 4:4:0
    assert rc == _native.EINVAL, msg
    with LutEngine(0) as bare:                                        # nothing loaded on this context
        for stages, word in (([(L3, 2)], "no lattice set"), ([(L32, 2)], "no second lattice set"), ([(L1, 0)], "no 1D LUT set")):
            rc, msg = _abi(bare, stages, None, 1, w, h, s, d)
            assert rc == _native.EINVAL and word in msg, msg
        rc, msg = _abi(bare, [(CD, 0)], grade, 1, w, h, s, d)        # a CDL alone needs nothing on the context
        assert rc == 0, msg
        bare.sync()
        assert _eq(_host(out, 10), _want(loaded._res, "cdl", grade, 10, 10, 10, "420", "420", src, "bare"))
        for t in out:
            t.fill_(0x5a5a)
    torch.cuda.synchronize()
    assert all((t == 0x5a5a).all() for t in out), "a refused call wrote to a destination"
    rc, msg = _abi(loaded, [(L1, 0), (CD, 0), (L3, 2)], grade, 1, w, h, s, d)
    assert rc == 0, msg
    assert loaded.last_kernel == "k_yuv_stack_vec<1,1,1,1,1,1,0,1>[lut1d,cdl,lut3d:2]"
    assert _eq(_host(out, 10), _want(loaded._res, "lut1d,cdl,lut3d", grade, 10, 10, 10, "420", "420", src, "abi"))


# ------------------------------------------------------------------ table placement
@pytest.mark.gpu
def test_lds_and_global_tables_give_the_same_bytes(luts):
    """LUTR_STACK_LDS unset / 0 in two child processes (the knob is read at launch): the same output bytes at 8, 10, 12 and 16
    bit, and the placements that ran."""
    outs = []
    for knob, placed in ((None, b"1111100"), ("0", b"0000000")):
        env = {k: v for k, v in os.environ.items() if k != "LUTR_STACK_LDS"}
        if knob is not None:
            env["LUTR_STACK_LDS"] = knob
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "_gpu_stack_worker.py"), str(luts["log709_33"][0]),
                            str(GOLDEN / "lut1d" / "gamma1024.cube"), str(GOLDEN / "cdl" / "shot.cc")], capture_output=True, cwd=ROOT,
                           timeout=180, env=env)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        assert r.stderr.endswith(placed), r.stderr[-200:]
        outs.append(r.stdout)
    assert len(outs[0]) > 100000 and outs[0] == outs[1]


# ------------------------------------------------------------------ apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut_with_stages(loaded, luts, l1ds, grade):
    from lut_renderer_amd.api import apply_lut
    src = _src("natural", W, H, 10, "420", nf=NF)
    stages = "lut1d,cdl,lut3d,lut3d2:nearest"
    got, tags = apply_lut(_dev(src, loaded.device), cube=luts["log709_33"][1], cube2=luts["random_9"][0],
                          lut1d=GOLDEN / "lut1d" / "gamma1024.cube", interp1d="cubic", cdl=GOLDEN / "cdl" / "shot.cc", stages=stages,
                          pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv", out_pix_fmt="yuv422p10le", engine=loaded)
    assert loaded.last_kernel == _vec_name(10, 10, "420", "422", stages, True) and tags["colorspace"] == "bt709"
    assert _eq(_host(got, 10), _want(loaded._res, stages, grade, 10, 10, 10, "420", "422", src, "api"))
    got, _ = apply_lut(_dev(src, loaded.device), cube=None, cdl=grade, stages=["cdl"], pix_fmt="yuv420p10le", colorspace="bt709",
                       color_range="tv", out_pix_fmt="yuv422p10le", engine=loaded)
    assert _eq(_host(got, 10), _want(loaded._res, "cdl", grade, 10, 10, 10, "420", "422", src, "api"))


@pytest.mark.gpu
def test_cli_over_pipes_with_stages(luts, l1ds, grade):
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    src = _src("natural", 64, 8, 10, "420")
    stages = "lut1d,cdl,lut3d,lut3d2:trilinear"
    res = dict(lut=luts["log709_33"][1], lut2=luts["random_9"][1], l1=(l1ds["gamma1024"], "spline"), prelut=None)
    want = b"".join(p.tobytes() for p in _want(res, stages, grade, 10, 10, 10, "420", "422", src, "cli"))
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le"), luts["log709_33"][0],
                         info, python_bin=sys.executable, cube2=luts["random_9"][0], lut1d=GOLDEN / "lut1d" / "gamma1024.cube",
                         interp1d="spline", cdl=GOLDEN / "cdl" / "shot.cc", stages=stages)
    assert cmd[-2:] == ["--stages", "lut1d,cdl,lut3d:tetrahedral,lut3d2:trilinear"]
    r = subprocess.run(cmd + ["--duration", "0.040"], input=b"".join(p.tobytes() for p in src), capture_output=True, cwd=ROOT,
                       timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == want
