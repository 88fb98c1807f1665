"""The RGB matrix stage of the stage stack on the GPU: lutr_apply_yuv_stack_matrix bit-exact, whole planes,
against the list walk of tests/_matrix_twin.py, and against lutr_apply_yuv_stack on the same engine where the two contracts meet.
The twin is fed the product's own host tables (lutr_cdl_table, lutr_lut1d_table), so that a last-bit difference between two pows
or cosf cannot fail a kernel test."""
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
from tests import _matrix_twin as twin
from tests.test_gpu_stack import H, LAYOUTS, MODES, NF, W, _desc, _dev, _eq, _fmt, _host, _lds, _list, _src, _variant

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
GENERIC = "k_yuv_stack_mtx_generic"
I3 = RgbMatrix()
SWAP = RgbMatrix((0, 0, 1, 0, 1, 0, 1, 0, 0))
TWICE = RgbMatrix((2, 0, 0, 0, 2, 0, 0, 0, 2))
NEG = RgbMatrix((-1.0, -0.5, 0.0, 0.25, 0.5, 0.25, 0.0, -2.0, 1.0), (0.25, 0.0, 0.5))
GAMUT = read_rgb_matrix(GOLDEN / "matrix" / "bt2020_to_709.spimtx")          # BT.2020 -> BT.709 primaries, entries no float32 holds
MATRICES = dict(identity=I3, swap=SWAP, twice=TWICE, negative=NEG, gamut=GAMUT)
_refs = {}           # expected planes, computed once per case and shared (never written to)


def _vec_name(din, dout, a, b, stages, lds):
    (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
    tri = int(any(m == "trilinear" for _, m in parse_stages(stages)))
    return f"k_yuv_stack_mtx_vec<{int(din > 8)},{int(dout > 8)},{icsx},{icsy},{ocsx},{ocsy},{tri},{int(lds)}>" + _list(stages)


@pytest.fixture(scope="module")
def luts(cube_dir):
    return {n: (cube_dir / f"{n}.cube", cube.read_lut(cube_dir / f"{n}.cube")) for n in ("log709_33", "random_9")}


@pytest.fixture(scope="module")
def l1ds():
    return {n: cube.read_lut1d(GOLDEN / "lut1d" / f"{n}.cube") for n in ("gamma1024",)}


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


def _want(res, stages, cdl, mtx, din, dl, dout, a, b, src, key, rin="tv", prologue=False):
    """The twin's planes for `src` ([rows, cols] or [nf, rows, cols] planes) with the resources `res` (the `loaded` fixture's), the
    matrix `mtx` and the product's own tables at dl."""
    st = parse_stages(stages)
    rk = (id(res["lut"]), id(res["lut2"]), id(res["l1"][0]), res["l1"][1], st, None if cdl is None else (cdl.sop_text(), cdl.saturation),
          None if mtx is None else (mtx.m, mtx.offset), din, dl, dout, a, b, key, rin, prologue)
    if rk not in _refs:
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        k = twin.consts("bt709", rin, "bt709", "tv", din, dl, dout, ocsx, ocsy, prologue=prologue)
        kinds = [s for s, _ in st]
        kw = dict(lut=res["lut"], lut2=res["lut2"], prelut=res["prelut"], cdl=cdl, mtx=mtx,
                  l1d_tab=_native.lut1d_table(*res["l1"], dl) if "lut1d" in kinds else None,
                  cdl_tab=_native.cdl_table(cdl, dl) if "cdl" in kinds else None)
        if src[0].ndim == 2:
            _refs[rk] = twin.apply(st, k, dl, dout, icsx, icsy, ocsx, ocsy, src, **kw)
        else:
            per = [twin.apply(st, k, dl, dout, icsx, icsy, ocsx, ocsy, [p[i] for p in src], **kw) for i in range(src[0].shape[0])]
            _refs[rk] = [np.stack([f[i] for f in per]) for i in range(3)]
    return _refs[rk]


# ------------------------------------------------------------------ layouts, orders, matrices, container mixes, modes
@pytest.mark.gpu
@pytest.mark.parametrize("a", list(LAYOUTS))
@pytest.mark.parametrize("b", list(LAYOUTS))
def test_all_nine_layout_pairs_at_10_bit(loaded, a, b):
    stages = "lut1d,matrix,lut3d"
    src = _src("natural", W, H, 10, a, nf=NF)
    got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), stages=stages, rgb_matrix=GAMUT)
    assert loaded.last_kernel == _vec_name(10, 10, a, b, stages, True), loaded.last_kernel
    assert _eq(_host(got, 10), _want(loaded._res, stages, None, GAMUT, 10, 10, 10, a, b, src, "nine"))


ORDERS = ("matrix", "matrix,lut3d", "lut3d,matrix", "matrix,lut1d", "cdl,matrix,lut3d", "matrix,cdl,lut3d", "matrix,lut3d,lut3d2",
          "matrix,cdl,lut1d,lut3d")


@pytest.mark.gpu
@pytest.mark.parametrize("stages", ORDERS)
def test_orders_on_420_to_422(loaded, grade, stages):
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, loaded.device)
    c = grade if "cdl" in stages else None
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, cdl=c)
    for mtx in (GAMUT, NEG):
        want = _want(loaded._res, stages, c, mtx, 10, 10, 10, "420", "422", src, "orders")
        got = loaded.apply_yuv_stack(dev, rgb_matrix=mtx, **names)
        assert loaded.last_kernel == _vec_name(10, 10, "420", "422", stages, _lds(stages, 10)), loaded.last_kernel
        assert _eq(_host(got, 10), want), mtx
        with _variant(loaded, "generic"):
            got = loaded.apply_yuv_stack(dev, rgb_matrix=mtx, **names)
            assert loaded.last_kernel == GENERIC + _list(stages)
        assert _eq(_host(got, 10), want), mtx


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MATRICES))
def test_matrices(loaded, name):
    from oracle.lut3d_numpy import rgb_codes_to_yuv, yuv_to_rgb_codes
    mtx = MATRICES[name]
    src = _src("uniform", W, H, 10, "420", nf=NF)
    dev = _dev(src, loaded.device)
    outs = {}
    for stages in ("matrix", "matrix,lut3d", "lut3d,matrix"):
        got = loaded.apply_yuv_stack(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, rgb_matrix=mtx)
        assert loaded.last_kernel == _vec_name(10, 10, "420", "422", stages, False), loaded.last_kernel
        outs[stages] = _host(got, 10)
        assert _eq(outs[stages], _want(loaded._res, stages, None, mtx, 10, 10, 10, "420", "422", src, "matrices")), stages
    if name in ("identity", "swap"):
        # known answers: the two conversion stages alone, with R and B exchanged in between for the permutation
        k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 1, 0)
        for i in range(NF):
            r, g, b = yuv_to_rgb_codes(k, 1, 1, [p[i] for p in src])
            want = rgb_codes_to_yuv(k, 10, 1, 0, (r, g, b) if name == "identity" else (b, g, r))
            assert _eq([p[i] for p in outs["matrix"]], want), i


@pytest.mark.gpu
@pytest.mark.parametrize("din,dout", [(8, 8), (10, 8), (16, 8), (12, 12), (8, 10)], ids=lambda v: str(v))
def test_container_mixes_on_420_to_422(loaded, grade, din, dout):
    src = _src("uniform", W, H, din, "420", nf=NF)
    for stages in ("lut1d,matrix,lut3d", "matrix,cdl,lut3d2"):
        c = grade if "cdl" in stages else None
        got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(din, "420"), out_pix_fmt=_fmt(dout, "422"), stages=stages,
                                     cdl=c, rgb_matrix=GAMUT)
        # an 8-bit source written as 16-bit words has no vector kernel
        name = GENERIC + _list(stages) if din == 8 and dout > 8 else _vec_name(din, dout, "420", "422", stages, _lds(stages, din))
        assert loaded.last_kernel == name, loaded.last_kernel
        assert _eq(_host(got, dout), _want(loaded._res, stages, c, GAMUT, din, din, dout, "420", "422", src, "mix")), stages


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [12, 16])
def test_frames_that_reach_codes_0_and_m(loaded, depth):
    from oracle.lut3d_numpy import yuv_to_rgb_codes
    m = (1 << depth) - 1
    src = [p.copy() for p in _src("uniform", 64, 8, depth, "420", k=2)]
    src[0][0, :8] = [0, m, 0, m, 1, m - 1, (m + 1) // 2, m]
    src[1][0, :4] = [0, m, (m + 1) // 2, (m + 1) // 2]
    src[2][0, :4] = [m, 0, (m + 1) // 2, (m + 1) // 2]
    k = twin.consts("bt709", "tv", "bt709", "tv", depth, depth, depth, 1, 1)
    rgb = yuv_to_rgb_codes(k, 1, 1, src)
    assert min(int(c.min()) for c in rgb) == 0 and max(int(c.max()) for c in rgb) == m
    for stages, mtx in (("matrix", I3), ("matrix", TWICE), ("matrix,lut1d", NEG), ("lut1d,matrix,lut3d", GAMUT)):
        got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(depth, "420"), stages=stages, rgb_matrix=mtx)
        assert loaded.last_kernel == _vec_name(depth, depth, "420", "420", stages, _lds(stages, depth)), loaded.last_kernel
        assert _eq(_host(got, depth), _want(loaded._res, stages, None, mtx, depth, depth, depth, "420", "420", src, ("ends", depth))), stages


@pytest.mark.gpu
@pytest.mark.parametrize("m1,m2", [("pyramid", "nearest"), ("trilinear", "prism"), ("tetrahedral", "trilinear"), ("nearest", "tetrahedral"),
                                   ("prism", "pyramid")])
def test_the_five_lut3d_modes_around_the_matrix(loaded, m1, m2):
    """The first lattice is fed codes (all five modes in the twin), the second unit floats behind the matrix; a pyramid or prism
    stage sends the call to the generic kernel.  (Behind the matrix the twin has the three vector modes.)"""
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, loaded.device)
    unit2 = m2 if m2 in MODES[:3] else "tetrahedral"
    for stages in ((("lut3d", m1), "matrix", ("lut3d2", unit2)), ("matrix", "lut1d", ("lut3d", m1), ("lut3d2", m2))):
        names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, rgb_matrix=GAMUT)
        want = _want(loaded._res, stages, None, GAMUT, 10, 10, 10, "420", "422", src, "modes")
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
def test_ragged_widths_and_small_frames(loaded):
    """Padded (aligned) rows whose width is no multiple of the thread's unit: the vector kernel up to column 136, the generic kernel
    for the rest -- 139 x 37 on 4:2:2 -> 4:4:4 (union block height 1) and 140 x 36 on a pair with 4:2:0; the padding keeps its
    sentinel.  139 x 37 with a 4:2:0 side ends in half a union block: the generic kernel's alone.  Then 16 x 4 and 67 x 21 on the
    generic kernel."""
    import torch
    pad = 160
    stages = "lut1d,matrix,lut3d"
    for (w, h), depth, a, b, name in (((139, 37), 10, "422", "444", "split"), ((139, 37), 10, "420", "422", "generic"),
                                      ((140, 36), 8, "444", "420", "split")):
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
        loaded.apply_yuv_stack(src_v, dst_v, pix_fmt=_fmt(depth, a), out_pix_fmt=_fmt(depth, b), stages=stages, rgb_matrix=GAMUT)
        if name == "split":
            vec = _vec_name(depth, depth, a, b, stages, True)
            assert loaded.last_kernel == vec.replace("[", "+" + GENERIC + "[", 1), loaded.last_kernel
        else:
            assert loaded.last_kernel == GENERIC + _list(stages), loaded.last_kernel
        assert _eq(_host(dst_v, depth), _want(loaded._res, stages, None, GAMUT, depth, depth, depth, a, b, src, ("ragged", w, h))), (w, h, a, b)
        assert all((t[:, s[1]:] == fill).all() for t, s in zip(dp, oshape)), "wrote past the row"
    for (w, h), a, b in (((16, 4), "420", "422"), ((67, 21), "420", "422"), ((67, 21), "444", "420")):
        src = _src("natural", w, h, 10, a, k=5)
        with _variant(loaded, "generic"):
            got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), stages=stages, rgb_matrix=NEG)
            assert loaded.last_kernel == GENERIC + _list(stages)
        assert _eq(_host(got, 10), _want(loaded._res, stages, None, NEG, 10, 10, 10, a, b, src, ("small", w, h))), (w, h, a, b)


# ------------------------------------------------------------------ other paths
@pytest.mark.gpu
def test_full_range_prologue(loaded):
    """A full-range 8-bit source with range_in="tv": lutr_apply_yuv's prologue ahead of the stack."""
    src = _src("natural", W, H, 8, "420", k=6, nf=NF, full_range=True)
    for stages in ("lut1d,matrix,lut3d", "matrix"):
        got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt="yuv420p", out_pix_fmt="yuv422p", range_src="pc", range_in="tv",
                                     lut_depth=8, stages=stages, rgb_matrix=GAMUT)
        assert loaded.last_kernel == _vec_name(8, 8, "420", "422", stages, _lds(stages, 8))
        assert _eq(_host(got, 8), _want(loaded._res, stages, None, GAMUT, 8, 8, 8, "420", "422", src, "pc", rin="tv", prologue=True)), stages


@pytest.mark.gpu
def test_a_csp_prelut_on_the_first_lattice(loaded, tmp_path):
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
    for stages in ("lut3d,matrix", "matrix,lut1d,lut3d", "matrix,lut3d2,lut3d"):
        got = loaded.apply_yuv_stack(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, rgb_matrix=GAMUT)
        assert _eq(_host(got, 10), _want(res, stages, None, GAMUT, 10, 10, 10, "420", "422", src, "prelut")), (stages, loaded.last_kernel)
    with pytest.raises(ValueError, match="directly behind 'matrix'"):
        loaded.apply_yuv_stack(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages="matrix,lut3d", rgb_matrix=GAMUT)
    out = [t.clone() for t in dev]
    rc, msg = _abi(loaded, [(5, 0), (1, 2)], None, GAMUT, 1, W, H, _desc(dev), _desc(out), nf=NF)
    assert rc == _native.EINVAL and "directly behind matrix" in msg and "prelut" in msg, msg


@pytest.mark.gpu
def test_bit_for_bit_with_the_plain_stack_entry(loaded):
    """Where the two contracts meet, on one engine and source: the identity matrix against the identity CDL, and behind lut3d
    against nothing at all."""
    for a, b, depth in (("420", "422", 10), ("444", "444", 8), ("422", "420", 16)):
        src = _src("natural", W, H, depth, a, nf=NF)
        dev = _dev(src, loaded.device)
        names = dict(pix_fmt=_fmt(depth, a), out_pix_fmt=_fmt(depth, b))
        for with_mtx, plain in (("matrix", "cdl"), ("matrix,lut3d", "cdl,lut3d"), ("matrix,lut3d:trilinear", "cdl,lut3d:trilinear"),
                                ("lut3d,matrix", "lut3d"), ("matrix,lut1d", "lut1d")):
            ref = _host(loaded.apply_yuv_stack(dev, stages=plain, cdl=Cdl() if "cdl" in plain else None, **names), depth)
            assert loaded.last_kernel.startswith(("k_yuv_stack_vec<", "k_yuv_stack_generic")), loaded.last_kernel
            got = _host(loaded.apply_yuv_stack(dev, stages=with_mtx, rgb_matrix=I3, **names), depth)
            assert loaded.last_kernel.startswith("k_yuv_stack_mtx_vec<"), loaded.last_kernel
            assert _eq(got, ref), (a, b, depth, with_mtx)


@pytest.mark.gpu
def test_row_shards_are_the_whole_call(loaded, grade):
    import torch
    stages = "matrix,cdl,lut3d"
    src = _src("uniform", W, H, 10, "420", nf=NF)
    dev = _dev(src, loaded.device)
    for b, variant in (("420", "auto"), ("422", "auto"), ("444", "generic")):
        ocsy = LAYOUTS[b][1]
        names = dict(pix_fmt="yuv420p10le", out_pix_fmt=_fmt(10, b), stages=stages, cdl=grade, rgb_matrix=GAMUT)
        whole = _want(loaded._res, stages, grade, GAMUT, 10, 10, 10, "420", b, src, "shard")
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
        loaded.apply_yuv_stack(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, cdl=grade, rgb_matrix=GAMUT, row0=1,
                               rows=H - 1)
    assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_group_shards_on_the_union_block(loaded, luts, l1ds, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    stages = "lut1d,matrix,lut3d,lut3d2"
    for (w, h), a, b in (((W, H), "420", "422"), ((33, 7), "422", "420")):
        src = _src("natural", w, h, 10, a, k=9)
        want = _want(loaded._res, stages, None, GAMUT, 10, 10, 10, a, b, src, ("group", w))
        with LutEngineGroup([0, 0]) as g:
            assert g.treat_as_remote
            g.set_lut(luts["log709_33"][1])
            g.set_lut2(luts["random_9"][1])
            g.set_lut1d(l1ds["gamma1024"], "cubic")
            got = g.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), stages=stages, rgb_matrix=GAMUT)
            assert g.last_remote == 1 and all(r0 % 2 == 0 for r0, _ in g.last_blocks), g.last_blocks
            assert all(k.startswith("k_yuv_stack_mtx_") for k in g.last_kernels), g.last_kernels
            assert _eq(_host(got, 10), want), (w, h)


@pytest.mark.gpu
def test_a_yuva_frame_carries_its_alpha_past_the_stack(loaded):
    stages = "lut1d,matrix,lut3d"
    src = _src("natural", W, H, 10, "444", k=11)
    alpha = np.random.default_rng(3).integers(0, 1024, size=(H, W)).astype(np.uint16)
    got = loaded.apply_yuv_stack(_dev(list(src) + [alpha], loaded.device), pix_fmt="yuva444p10le", stages=stages, rgb_matrix=GAMUT)
    assert loaded.last_kernel.startswith(_vec_name(10, 10, "444", "444", stages, True) + "+k_alpha_"), loaded.last_kernel
    out = _host(got, 10)
    assert len(out) == 4 and np.array_equal(out[3], alpha)
    assert _eq(out[:3], _want(loaded._res, stages, None, GAMUT, 10, 10, 10, "444", "444", src, "yuva"))


@pytest.mark.gpu
def test_matrices_a_b_a_on_one_engine(loaded):
    """Per-clip matrices with no host wait in between: the numbers travel with the launch, so each call uses its own."""
    stages = "lut1d,matrix,lut3d"
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, loaded.device)
    order = [GAMUT, NEG, GAMUT]
    outs = [loaded.apply_yuv_stack(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, rgb_matrix=m) for m in order]
    for got, m in zip(outs, order):
        assert _eq(_host(got, 10), _want(loaded._res, stages, None, m, 10, 10, 10, "420", "422", src, "aba"))
    assert not _eq(_host(outs[0], 10), _host(outs[1], 10))


# ------------------------------------------------------------------ refusals at the ABI
def _raw_mtx(**entries):
    """struct lutr_rgb_matrix with numbers `RgbMatrix` itself refuses: m3=..., off1=..."""
    st = _native.rgb_matrix_struct(I3)
    for name, v in entries.items():
        if name.startswith("off"):
            st.offset[int(name[3:])] = v
        else:
            st.m[int(name[1:])] = v
    return st


def _abi(engine, stages, cdl, mtx, csy_out, w, h, s, d, nf=1, entry="lutr_apply_yuv_stack_matrix"):
    """A stack entry with raw (kind, interp) pairs at 10 bit, 4:2:0 in, 4:2:0 / 4:2:2 out; returns (rc, message)."""
    p = _native.YuvParams(_native.fmt_code(10, 1, 1), _native.fmt_code(10, 1, csy_out), 10, 0, 0, 0, 0, 0)
    arr = (_native.StageStruct * max(len(stages), 1))()
    for i, (kind, interp) in enumerate(stages):
        arr[i].kind, arr[i].interp = kind, interp
    k = None if cdl is None else C.byref(_native.cdl_struct(cdl))
    x = None if mtx is None else C.byref(mtx if isinstance(mtx, _native.RgbMatrixStruct) else _native.rgb_matrix_struct(mtx))
    tail = (w, h, nf, C.byref(s), C.byref(d), 0, h)
    with engine._lock:
        engine._bind_stream()
        if entry == "lutr_apply_yuv_stack_matrix":
            rc = engine._lib.lutr_apply_yuv_stack_matrix(engine._ctx, C.byref(p), arr, len(stages), k, x, *tail)
        elif entry == "lutr_apply_yuv_stack":
            rc = engine._lib.lutr_apply_yuv_stack(engine._ctx, C.byref(p), arr, len(stages), k, *tail)
        else:
            rc = engine._lib.lutr_apply_yuv_stack_mix(engine._ctx, C.byref(p), arr, len(stages), k, 0.5, None, *tail)
    return rc, engine._lib.lutr_last_error().decode()


@pytest.mark.gpu
def test_refusals_leave_the_destination_untouched(loaded, grade):
    import torch
    w, h = 64, 8
    src = _src("natural", w, h, 10, "420")
    dev = _dev(src, loaded.device)
    out = [torch.full_like(t, 0x5a5a) for t in dev]
    s, d = _desc(dev), _desc(out)
    L3, L1, CD, MX = 1, 3, 4, 5
    inf, nan = float("inf"), float("nan")
    for stages, c, mtx, word in (([(MX, 0), (L3, 2)], None, None, "a matrix stage is listed and the matrix is null"),
                                 ([(L3, 2)], None, I3, "a matrix is given and no matrix stage is listed"),
                                 ([(MX, 0), (L3, 2), (MX, 0)], None, I3, "stage kind matrix is listed twice"),
                                 ([(MX, 0)], None, _raw_mtx(m4=nan), "m[4]"), ([(MX, 0)], None, _raw_mtx(m0=inf), "m[0]"),
                                 ([(MX, 0)], None, _raw_mtx(off2=-inf), "offset[2]"), ([(MX, 0)], None, _raw_mtx(m8=65537.0), "m[8]"),
                                 ([(MX, 0)], None, _raw_mtx(off0=-1e9), "above 65536 in magnitude"),
                                 ([], None, I3, "1 to 4"), ([(7, 0)], None, I3, "unknown kind 7"), ([(6, 0)], None, I3, "unknown kind 6"),
                                 ([(MX, 0), (L3, 5)], None, I3, "interpolation mode 5"),
                                 ([(MX, 0), (CD, 0)], None, I3, "the CDL is null"), ([(MX, 0)], grade, I3, "no cdl stage is listed")):
        rc, msg = _abi(loaded, stages, c, mtx, 1, w, h, s, d)
        assert rc == _native.EINVAL and word in msg, (stages, msg)
    # the three entries without a matrix refuse the kind by name; kind 7 stays unknown there
    for entry in ("lutr_apply_yuv_stack", "lutr_apply_yuv_stack_mix"):
        rc, msg = _abi(loaded, [(MX, 0), (L3, 2)], None, None, 1, w, h, s, d, entry=entry)
        assert rc == _native.EINVAL and "matrix stage" in msg and "lutr_apply_yuv_stack_matrix" in msg, msg
        rc, msg = _abi(loaded, [(7, 0)], None, None, 1, w, h, s, d, entry=entry)
        assert rc == _native.EINVAL and "unknown kind 7" in msg, msg
    with _variant(loaded, "vec_lds"):
        rc, msg = _abi(loaded, [(MX, 0), (L3, 2)], None, I3, 1, w, h, s, d)
        assert rc == _native.EINVAL and "vec_lds" in msg, msg
    rc, msg = _abi(loaded, [(MX, 0)], None, I3, 1, w, h, s, s)
    assert rc == _native.EINVAL and "cannot run in place" in msg, msg
    torch.cuda.synchronize()
    assert all((t == 0x5a5a).all() for t in out), "a refused call wrote to a destination"
    rc, msg = _abi(loaded, [(L1, 0), (MX, 0), (L3, 2)], None, _raw_mtx(m0=65536.0, off0=-65536.0), 1, w, h, s, d)   # the largest entries
    assert rc == 0, msg
    assert loaded.last_kernel == "k_yuv_stack_mtx_vec<1,1,1,1,1,1,0,1>[lut1d,matrix,lut3d:2]"
    big = RgbMatrix((65536.0, 0, 0, 0, 1, 0, 0, 0, 1), (-65536.0, 0, 0))
    assert _eq(_host(out, 10), _want(loaded._res, "lut1d,matrix,lut3d", None, big, 10, 10, 10, "420", "420", src, "abi"))


# ------------------------------------------------------------------ table placement
@pytest.mark.gpu
def test_lds_and_global_tables_give_the_same_bytes(luts):
    """LUTR_STACK_LDS unset / 0 in two child processes (the knob is read at launch): the same output bytes, and the placements
    that ran."""
    outs = []
    for knob, placed in ((None, b"11100"), ("0", b"00000")):
        env = {k: v for k, v in os.environ.items() if k != "LUTR_STACK_LDS"}
        if knob is not None:
            env["LUTR_STACK_LDS"] = knob
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "_gpu_rgbmatrix_worker.py"), str(luts["log709_33"][0]),
                            str(GOLDEN / "lut1d" / "gamma1024.cube"), str(GOLDEN / "cdl" / "shot.cc"),
                            str(GOLDEN / "matrix" / "bt2020_to_709.spimtx")], capture_output=True, cwd=ROOT, timeout=180, env=env)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        assert r.stderr.endswith(placed), r.stderr[-200:]
        outs.append(r.stdout)
    assert len(outs[0]) > 100000 and outs[0] == outs[1]


# ------------------------------------------------------------------ apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut_with_a_matrix(loaded, luts, grade):
    from lut_renderer_amd.api import apply_lut
    src = _src("natural", W, H, 10, "420", nf=NF)
    stages = "lut1d,matrix,cdl,lut3d:trilinear"
    got, tags = apply_lut(_dev(src, loaded.device), cube=luts["log709_33"][1], lut1d=GOLDEN / "lut1d" / "gamma1024.cube", interp1d="cubic",
                          cdl=GOLDEN / "cdl" / "shot.cc", rgb_matrix=GOLDEN / "matrix" / "bt2020_to_709.spimtx", stages=stages,
                          pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv", out_pix_fmt="yuv422p10le", engine=loaded)
    assert loaded.last_kernel == _vec_name(10, 10, "420", "422", stages, True) and tags["colorspace"] == "bt709"
    assert _eq(_host(got, 10), _want(loaded._res, stages, grade, GAMUT, 10, 10, 10, "420", "422", src, "api"))
    got, _ = apply_lut(_dev(src, loaded.device), cube=None, rgb_matrix=NEG, stages=["matrix"], pix_fmt="yuv420p10le", colorspace="bt709",
                       color_range="tv", out_pix_fmt="yuv422p10le", engine=loaded)
    assert _eq(_host(got, 10), _want(loaded._res, "matrix", None, NEG, 10, 10, 10, "420", "422", src, "api"))


@pytest.mark.gpu
def test_cli_over_pipes_with_a_matrix(luts, l1ds):
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    src = _src("natural", 64, 8, 10, "420")
    stages = "lut1d,matrix,lut3d:trilinear"
    res = dict(lut=luts["log709_33"][1], lut2=None, l1=(l1ds["gamma1024"], "spline"), prelut=None)
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    io = (Path("-"), Path("-"), ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le"), luts["log709_33"][0], info)
    for mtx, given in ((NEG, NEG), (GAMUT, GOLDEN / "matrix" / "bt2020_to_709.spimtx")):
        want = b"".join(p.tobytes() for p in _want(res, stages, None, mtx, 10, 10, 10, "420", "422", src, "cli"))
        cmd = engine_command(*io, python_bin=sys.executable, lut1d=GOLDEN / "lut1d" / "gamma1024.cube", interp1d="spline", stages=stages,
                             rgb_matrix=given)
        assert cmd[-2:] == ["--stages", "lut1d,matrix,lut3d:trilinear"]
        r = subprocess.run(cmd + ["--duration", "0.040"], input=b"".join(p.tobytes() for p in src), capture_output=True, cwd=ROOT,
                           timeout=180)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        assert r.stdout == want
