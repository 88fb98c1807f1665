"""ASC CDL in front of the LUT on the GPU: lutr_apply_yuv_cdl bit-exact, whole planes, against the composition in
tests/_cdl_twin.py.  The twin is fed the product's own host table (lutr_cdl_table, pinned to the twin's own build in
tests/test_cdl.py to one float32 ulp), so a last-bit difference between two pows cannot fail a kernel test."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.cdl import Cdl
from tests import _cdl_twin as twin

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "cdl"
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
GENERIC = "k_yuv_cdl_generic"
#: 136 x 36, 2 frames: at 8 samples per thread 612 threads -- two full workgroups and a partial one, across the frame stride
W, H, NF = 136, 36, 2
#: slopes around 1.3, offsets -0.08 and +0.05, powers 0.8 and 1.2, different per channel (tests/golden/cdl/shot.cc)
GRADE = Cdl((1.3, 1.25, 1.1), (-0.08, 0.0, 0.05), (0.8, 1.0, 1.2), 0.6)
OTHER = Cdl((0.9, 1.0, 1.2), (-0.02, 0.0, 0.02), (1.2, 1.1, 0.9), 1.7)
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
    return f"k_yuv_cdl_vec<{int(din > 8)},{int(dout > 8)},{icsx},{icsy},{ocsx},{ocsy},{MODES.index(mode)}>"


@pytest.fixture(scope="module")
def luts(cube_dir):
    return {n: (cube_dir / f"{n}.cube", cube.read_lut(cube_dir / f"{n}.cube")) for n in ("log709_33", "random_9")}


def _src(dist, w, h, depth, lay, k=1, nf=1, full_range=False):
    """(Y, Cb, Cr), each [nf, rows, cols] (or [rows, cols] for nf = 1)."""
    rk = ("src", dist, w, h, depth, lay, k, nf, full_range)
    if rk not in _refs:
        fs = [frames.make_yuv(dist, w, h, depth, *LAYOUTS[lay], k=k + 7 * i, full_range=full_range) for i in range(nf)]
        _refs[rk] = fs[0] if nf == 1 else [np.stack([f[i] for f in fs]) for i in range(3)]
    return _refs[rk]


def _want(luts, name, cdl, mode, din, dl, dout, a, b, src, key, rin="tv", prologue=False):
    """The twin's planes for `src` ([rows, cols] or [nf, rows, cols] planes), with the product's own stage A table."""
    rk = (name, cdl, mode, din, dl, dout, a, b, key, rin, prologue)
    if rk not in _refs:
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        k = twin.consts("bt709", rin, "bt709", "tv", din, dl, dout, ocsx, ocsy, prologue=prologue)
        tab = _native.cdl_table(cdl, dl)
        if src[0].ndim == 2:
            _refs[rk] = twin.apply(luts[name][1], cdl, mode, k, dl, dout, icsx, icsy, ocsx, ocsy, src, tab=tab)
        else:
            per = [twin.apply(luts[name][1], cdl, mode, k, dl, dout, icsx, icsy, ocsx, ocsy, [p[i] for p in src], tab=tab)
                   for i in range(src[0].shape[0])]
            _refs[rk] = [np.stack([f[i] for f in per]) for i in range(3)]
    return _refs[rk]


# ------------------------------------------------------------------ layouts, container mixes, modes
@pytest.mark.gpu
@pytest.mark.parametrize("a", list(LAYOUTS))
@pytest.mark.parametrize("b", list(LAYOUTS))
def test_all_nine_layout_pairs_at_10_bit(engine, luts, a, b):
    engine.load_cube(luts["log709_33"][0])
    src = _src("natural", W, H, 10, a, nf=NF)
    got = engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), cdl=GRADE)
    assert engine.last_kernel == _vec_name(10, 10, a, b, "tetrahedral"), engine.last_kernel
    assert _eq(_host(got, 10), _want(luts, "log709_33", GRADE, "tetrahedral", 10, 10, 10, a, b, src, "nine"))


@pytest.mark.gpu
@pytest.mark.parametrize("din,dout", [(8, 8), (10, 8), (16, 8), (8, 10), (12, 12)], ids=lambda v: str(v))
def test_container_mixes_on_420_to_422(engine, luts, din, dout):
    engine.load_cube(luts["random_9"][0])
    src = _src("uniform", W, H, din, "420", nf=NF)
    got = engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(din, "420"), out_pix_fmt=_fmt(dout, "422"), cdl=GRADE)
    # an 8-bit source written as 16-bit words has no vector kernel
    assert engine.last_kernel == (GENERIC if din == 8 and dout > 8 else _vec_name(din, dout, "420", "422", "tetrahedral"))
    assert _eq(_host(got, dout), _want(luts, "random_9", GRADE, "tetrahedral", din, din, dout, "420", "422", src, "mix"))


@pytest.mark.gpu
def test_a_16_bit_frame_that_holds_codes_0_and_65535(engine, luts):
    """The 3 x 65536 table, both of its ends read."""
    engine.load_cube(luts["log709_33"][0])
    src = [p.copy() for p in _src("uniform", 64, 8, 16, "420", k=2)]
    src[0][0, :8] = [0, 65535, 0, 65535, 1, 65534, 32768, 65535]
    src[1][0, :4] = [0, 65535, 32768, 32768]
    src[2][0, :4] = [65535, 0, 32768, 32768]
    tab = _native.cdl_table(GRADE, 16)
    assert tab.shape == (3, 65536)
    from oracle.lut3d_numpy import yuv_to_rgb_codes
    k = twin.consts("bt709", "tv", "bt709", "tv", 16, 16, 16, 1, 1)
    rgb = yuv_to_rgb_codes(k, 1, 1, src)
    assert min(int(c.min()) for c in rgb) == 0 and max(int(c.max()) for c in rgb) == 65535
    got = engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p16le", cdl=GRADE)
    assert engine.last_kernel == _vec_name(16, 16, "420", "420", "tetrahedral")
    assert _eq(_host(got, 16), twin.apply(luts["log709_33"][1], GRADE, "tetrahedral", k, 16, 16, 1, 1, 1, 1, src, tab=tab))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", VEC_MODES)
def test_three_modes_on_the_vector_kernel(engine, luts, mode):
    engine.load_cube(luts["random_9"][0])
    src = _src("natural", W, H, 10, "420", nf=NF)
    with _variant(engine, "vec_global"):
        got = engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", interp=mode, cdl=GRADE)
        assert engine.last_kernel == _vec_name(10, 10, "420", "422", mode)
    want = _want(luts, "random_9", GRADE, mode, 10, 10, 10, "420", "422", src, "modes")
    assert _eq(_host(got, 10), want)
    with _variant(engine, "generic"):
        got = engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", interp=mode, cdl=GRADE)
        assert engine.last_kernel == GENERIC
    assert _eq(_host(got, 10), want)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_the_identity_cdl_is_the_plain_call_bit_for_bit(engine, luts, mode):
    """Every mode -- pyramid and prism, which the twin's lattice does not have, are checked this way -- on the generic kernel, and
    the three vector modes on the vector kernel too."""
    engine.load_cube(luts["random_9"][0])
    for a, b in (("420", "422"), ("420", "420"), ("444", "444")):
        src = _src("natural", W, H, 10, a, nf=NF)
        dev = _dev(src, engine.device)
        names = dict(pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), interp=mode)
        plain = _host(engine.apply_yuv(dev, **names), 10)
        with _variant(engine, "generic"):
            got = engine.apply_yuv(dev, **names, cdl=Cdl.identity())
            assert engine.last_kernel == GENERIC
        assert _eq(_host(got, 10), plain), (mode, a, b)
        got = engine.apply_yuv(dev, **names, cdl=Cdl.identity())
        assert engine.last_kernel == (_vec_name(10, 10, a, b, mode) if mode in VEC_MODES else GENERIC)
        assert _eq(_host(got, 10), plain), (mode, a, b)
        if mode not in VEC_MODES:
            with _variant(engine, "vec_global"):
                with pytest.raises(_native.LutrError) as e:
                    engine.apply_yuv(dev, **names, cdl=Cdl.identity())
                assert e.value.code == _native.EINVAL


# ------------------------------------------------------------------ CDL values
@pytest.mark.gpu
@pytest.mark.parametrize("sat", [0.0, 0.6, 1.0, 1.7])
def test_saturations(engine, luts, sat):
    engine.load_cube(luts["random_9"][0])
    c = Cdl(GRADE.slope, GRADE.offset, GRADE.power, sat)
    src = _src("natural", W, H, 10, "420", nf=NF)
    got = engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le", out_pix_fmt="yuv444p10le", cdl=c)
    assert engine.last_kernel == _vec_name(10, 10, "420", "444", "tetrahedral")
    assert _eq(_host(got, 10), _want(luts, "random_9", c, "tetrahedral", 10, 10, 10, "420", "444", src, "sat"))


@pytest.mark.gpu
def test_slope_0_and_clamping_offsets(engine, luts):
    engine.load_cube(luts["log709_33"][0])
    src = _src("uniform", W, H, 10, "422", nf=NF)
    for c in (Cdl((0, 0, 0), (0.25, 0.5, 1.5), (2.0, 1.0, 0.5)), Cdl((4, 4, 4), (-1.5, -1.5, -1.5), (1.0, 0.45, 2.2), 1.3)):
        got = _host(engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv422p10le", cdl=c), 10)
        assert _eq(got, _want(luts, "log709_33", c, "tetrahedral", 10, 10, 10, "422", "422", src, "edge"))
        if c.slope == (0.0, 0.0, 0.0):
            assert all(len(np.unique(p)) == 1 for p in got)          # the lattice saw one constant


# ------------------------------------------------------------------ shapes
@pytest.mark.gpu
def test_a_ragged_frame_is_split_between_the_two_kernels(engine, luts):
    """139 x 37: an odd last row and column.  Rows of whole union blocks with a ragged width on padded (aligned) rows go to the
    vector kernel up to column 136 and to the generic kernel for the rest; an odd number of rows of a 4:2:0 side is the generic
    kernel's alone."""
    import torch
    engine.load_cube(luts["log709_33"][0])
    pad = 160
    for (w, h), a, b, split in (((139, 37), "444", "444", True), ((139, 36), "420", "422", True), ((139, 37), "420", "422", False),
                                ((139, 37), "422", "420", False)):
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        src = _src("natural", w, h, 10, a, k=4)
        sp = [torch.zeros((p.shape[0], pad), dtype=torch.int16, device=engine.device) for p in src]
        for t, p in zip(sp, src):
            t[:, :p.shape[1]] = torch.from_numpy(p.view(np.int16)).to(engine.device)
        src_v = [t[:, :p.shape[1]] for t, p in zip(sp, src)]
        oshape = [(h, w)] + [frames.chroma_shape(w, h, ocsx, ocsy)] * 2
        dp = [torch.full((s[0], pad), -1, dtype=torch.int16, device=engine.device) for s in oshape]
        dst_v = [t[:, :s[1]] for t, s in zip(dp, oshape)]
        engine.apply_yuv(src_v, dst_v, pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), cdl=GRADE)
        assert engine.last_kernel == (_vec_name(10, 10, a, b, "tetrahedral") + "+" + GENERIC if split else GENERIC), engine.last_kernel
        assert _eq(_host(dst_v, 10), _want(luts, "log709_33", GRADE, "tetrahedral", 10, 10, 10, a, b, src, ("ragged", w, h))), (a, b)
        assert all((t[:, s[1]:] == -1).all() for t, s in zip(dp, oshape)), "wrote past the row"


@pytest.mark.gpu
def test_a_tiny_frame_on_the_generic_kernel(engine, luts):
    engine.load_cube(luts["random_9"][0])
    for a, b in (("420", "420"), ("444", "420"), ("422", "444")):
        src = _src("natural", 16, 4, 10, a, k=5)
        with _variant(engine, "generic"):
            got = engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), cdl=OTHER)
            assert engine.last_kernel == GENERIC
        assert _eq(_host(got, 10), _want(luts, "random_9", OTHER, "tetrahedral", 10, 10, 10, a, b, src, "tiny")), (a, b)


# ------------------------------------------------------------------ other paths
@pytest.mark.gpu
def test_full_range_prologue(engine, luts):
    """range_src="pc" with lut_depth=8 on a 10-bit source: lutr_apply_yuv's prologue ahead of the CDL, which then runs at 8 bit
    (a 3 x 256 table)."""
    engine.load_cube(luts["log709_33"][0])
    src = _src("natural", W, H, 10, "420", k=6, nf=NF, full_range=True)
    for dout, b in ((10, "420"), (8, "422")):
        got = engine.apply_yuv(_dev(src, engine.device), pix_fmt="yuv420p10le", out_pix_fmt=_fmt(dout, b), range_src="pc",
                               range_in="tv", lut_depth=8, cdl=GRADE)
        assert engine.last_kernel == _vec_name(10, dout, "420", b, "tetrahedral")
        want = _want(luts, "log709_33", GRADE, "tetrahedral", 10, 8, dout, "420", b, src, "pc", rin="tv", prologue=True)
        assert _eq(_host(got, dout), want), (dout, b)


@pytest.mark.gpu
def test_row_shards_are_the_whole_call(engine, luts):
    import torch
    engine.load_cube(luts["log709_33"][0])
    src = _src("uniform", W, H, 10, "420", nf=NF)
    dev = _dev(src, engine.device)
    for b, variant in (("420", "auto"), ("422", "auto"), ("444", "generic")):
        ocsy = LAYOUTS[b][1]
        names = dict(pix_fmt="yuv420p10le", out_pix_fmt=_fmt(10, b), cdl=GRADE)
        whole = _want(luts, "log709_33", GRADE, "tetrahedral", 10, 10, 10, "420", b, src, "shard")
        with _variant(engine, variant):
            out = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=engine.device) for p in whole]
            engine.apply_yuv(dev, out, row0=10, rows=14, **names)
            got = _host(out, 10)
            for i, (g, wh) in enumerate(zip(got, whole)):
                r0, r1 = (10, 24) if i == 0 else (10 >> ocsy, 24 >> ocsy)
                assert np.array_equal(g[:, r0:r1], wh[:, r0:r1]), (b, variant, i)
                assert (g[:, :r0] == 0x5a5a).all() and (g[:, r1:] == 0x5a5a).all(), (b, variant, i, "wrote outside the block")
            engine.apply_yuv(dev, out, row0=0, rows=10, **names)
            engine.apply_yuv(dev, out, row0=24, rows=H - 24, **names)
        assert _eq(_host(out, 10), whole), (b, variant)
    with pytest.raises(_native.LutrError, match="union") as e:
        engine.apply_yuv(dev, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", row0=1, rows=H - 1, cdl=GRADE)
    assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_group_shards_on_the_union_block(engine, luts, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    for (w, h), a, b in (((W, H), "420", "422"), ((33, 7), "422", "420")):
        src = _src("natural", w, h, 10, a, k=9)
        names = dict(pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), cdl=GRADE)
        want = _want(luts, "log709_33", GRADE, "tetrahedral", 10, 10, 10, a, b, src, ("group", w))
        for n in (2, 3):
            with LutEngineGroup([0] * n) as g:
                assert g.treat_as_remote
                g.set_lut(luts["log709_33"][1])
                got = g.apply_yuv(_dev(src, engine.device), **names)
                assert g.last_remote == sum(1 for r0, r1 in g.last_blocks[1:] if r1 > r0) and g.last_remote >= 1
                assert all(r0 % 2 == 0 for r0, _ in g.last_blocks), g.last_blocks
                assert all(k.startswith("k_yuv_cdl_") for k in g.last_kernels), g.last_kernels
                assert _eq(_host(got, 10), want), (w, h, n)


@pytest.mark.gpu
def test_a_yuva_frame_carries_its_alpha_past_the_cdl(engine, luts):
    engine.load_cube(luts["log709_33"][0])
    src = _src("natural", W, H, 10, "444", k=11)
    alpha = np.random.default_rng(3).integers(0, 1024, size=(H, W)).astype(np.uint16)
    got = engine.apply_yuv(_dev(list(src) + [alpha], engine.device), pix_fmt="yuva444p10le", cdl=GRADE)
    assert engine.last_kernel.startswith(_vec_name(10, 10, "444", "444", "tetrahedral") + "+k_alpha_"), engine.last_kernel
    out = _host(got, 10)
    assert len(out) == 4 and np.array_equal(out[3], alpha)
    assert _eq(out[:3], _want(luts, "log709_33", GRADE, "tetrahedral", 10, 10, 10, "444", "444", src, "yuva"))


# ------------------------------------------------------------------ engine state
@pytest.mark.gpu
def test_one_engine_a_then_b_then_a_again(engine, luts):
    """Per-clip use: the table is replaced while the previous call's kernel may still be running; no host wait in between."""
    engine.load_cube(luts["random_9"][0])
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, engine.device)
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
    outs = [engine.apply_yuv(dev, **names, cdl=c) for c in (GRADE, OTHER, GRADE, GRADE, Cdl(GRADE.slope, GRADE.offset, GRADE.power, 1.7))]
    for got, c in zip(outs, (GRADE, OTHER, GRADE, GRADE, Cdl(GRADE.slope, GRADE.offset, GRADE.power, 1.7))):
        assert _eq(_host(got, 10), _want(luts, "random_9", c, "tetrahedral", 10, 10, 10, "420", "422", src, "aba")), c
    # a new lattice under the same CDL: the table stands, the lattice does not
    engine.load_cube(luts["log709_33"][0])
    got = engine.apply_yuv(dev, **names, cdl=GRADE)
    assert _eq(_host(got, 10), _want(luts, "log709_33", GRADE, "tetrahedral", 10, 10, 10, "420", "422", src, "aba"))


@pytest.mark.gpu
def test_one_cdl_at_8_then_10_then_8_bit(engine, luts):
    engine.load_cube(luts["log709_33"][0])
    for depth in (8, 10, 8, 12, 10):
        src = _src("natural", W, H, depth, "420", nf=NF)
        got = engine.apply_yuv(_dev(src, engine.device), pix_fmt=_fmt(depth, "420"), cdl=GRADE)
        assert _eq(_host(got, depth), _want(luts, "log709_33", GRADE, "tetrahedral", depth, depth, depth, "420", "420", src, "depths")), depth


@pytest.mark.gpu
def test_two_engines_with_different_cdls_interleaved(engine, luts):
    from lut_renderer_amd.engine import LutEngine
    engine.load_cube(luts["random_9"][0])
    src = _src("natural", W, H, 10, "420", nf=NF)
    dev = _dev(src, engine.device)
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
    with LutEngine(0) as second:
        second.load_cube(luts["random_9"][0])
        got = []
        for _ in range(2):
            got.append((engine.apply_yuv(dev, **names, cdl=GRADE), GRADE))
            got.append((second.apply_yuv(dev, **names, cdl=OTHER), OTHER))
        got.append((second.apply_yuv(dev, **names, cdl=GRADE), GRADE))
        got.append((engine.apply_yuv(dev, **names, cdl=OTHER), OTHER))
        for planes, c in got:
            assert _eq(_host(planes, 10), _want(luts, "random_9", c, "tetrahedral", 10, 10, 10, "420", "422", src, "aba")), c
    plain = _host(engine.apply_yuv(dev, **names), 10)              # the call without a CDL is what it always was
    assert engine.last_kernel == "k_yuv_xsub_vec<1,1,1,1,1,0,2>"
    assert _eq(_host(engine.apply_yuv(dev, **names, cdl=Cdl.identity()), 10), plain)


# ------------------------------------------------------------------ refusals at the ABI
def _desc(tensors):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        st.data[i] = t.data_ptr()
        st.stride[i] = t.stride(-2) * t.element_size()
        st.frame_stride[i] = 0
    return st


def _abi(engine, cdl_struct, w, h, s, d):
    p = _native.YuvParams(_native.fmt_code(10, 1, 1), _native.fmt_code(10, 1, 1), 10, 0, 0, 0, 0, 0)
    with engine._lock:
        engine._bind_stream()
        rc = engine._lib.lutr_apply_yuv_cdl(engine._ctx, C.byref(p), 2, C.byref(cdl_struct), w, h, 1, C.byref(s), C.byref(d), 0, h)
    return rc, engine._lib.lutr_last_error().decode()


@pytest.mark.gpu
def test_refusals_at_the_abi_leave_the_destination_untouched(engine, luts, tmp_path):
    import torch
    from tests._csp_files import write_csp_with_prelut
    w, h = 64, 8
    dev = _dev(_src("natural", w, h, 10, "420"), engine.device)
    out = [torch.full_like(t, 0x5a5a) for t in dev]
    good = _native.cdl_struct(GRADE)
    # a LUT with a .csp prelut
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 3
    write_csp_with_prelut(tmp_path / "shaped.csp", 17, cube.log709_lattice(17), shapers)
    engine.load_cube(tmp_path / "shaped.csp")
    rc, msg = _abi(engine, good, w, h, _desc(dev), _desc(out))
    assert rc == _native.EINVAL and "prelut" in msg, msg
    with pytest.raises(ValueError, match="prelut is not supported with a CDL"):
        engine.apply_yuv(dev, out, pix_fmt="yuv420p10le", cdl=GRADE)
    engine.load_cube(luts["log709_33"][0])                          # (a new lattice drops the prelut)
    # variant vec_lds
    with _variant(engine, "vec_lds"):
        rc, msg = _abi(engine, good, w, h, _desc(dev), _desc(out))
    assert rc == _native.EINVAL and "vec_lds" in msg, msg
    # an overlap: in place, and a destination plane inside a source plane
    rc, msg = _abi(engine, good, w, h, _desc(dev), _desc(dev))
    assert rc == _native.EINVAL and "cannot run in place: the byte range of source plane 0 overlaps" in msg, msg
    inside = [out[0], dev[0][:h // 2, :w // 2], out[2]]
    rc, msg = _abi(engine, good, w, h, _desc(dev), _desc(inside))
    assert rc == _native.EINVAL and "source plane 0 overlaps that of destination plane 1" in msg, msg
    with pytest.raises(ValueError, match="CDL pass cannot run in place"):
        engine.apply_yuv(dev, dev, pix_fmt="yuv420p10le", cdl=GRADE)
    # numbers the CDL cannot hold
    for field, i, value, word in (("slope", 1, float("nan"), "not finite"), ("slope", 2, -0.5, "slope of B is negative"),
                                  ("power", 0, 0.0, "power of R must be above 0"), ("offset", 0, float("inf"), "not finite")):
        bad = _native.cdl_struct(GRADE)
        getattr(bad, field)[i] = value
        rc, msg = _abi(engine, bad, w, h, _desc(dev), _desc(out))
        assert rc == _native.EINVAL and word in msg, (field, msg)
    bad = _native.cdl_struct(GRADE)
    bad.saturation = float("nan")
    rc, msg = _abi(engine, bad, w, h, _desc(dev), _desc(out))
    assert rc == _native.EINVAL and "saturation is not finite" in msg, msg
    torch.cuda.synchronize()
    assert all((t == 0x5a5a).all() for t in out), "a refused call wrote to a destination"
    # and the same planes through a good call
    rc, msg = _abi(engine, good, w, h, _desc(dev), _desc(out))
    assert rc == 0, msg
    src = _src("natural", w, h, 10, "420")
    assert _eq(_host(out, 10), _want(luts, "log709_33", GRADE, "tetrahedral", 10, 10, 10, "420", "420", src, "abi"))


# ------------------------------------------------------------------ apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut_with_a_cdl_file(engine, luts):
    from lut_renderer_amd.api import apply_lut
    src = _src("natural", W, H, 10, "420", nf=NF)
    got, tags = apply_lut(_dev(src, engine.device), cube=luts["log709_33"][1], cdl=GOLDEN / "shot.cc", pix_fmt="yuv420p10le",
                          colorspace="bt709", color_range="tv", out_pix_fmt="yuv422p10le", engine=engine)
    assert engine.last_kernel == _vec_name(10, 10, "420", "422", "tetrahedral") and tags["colorspace"] == "bt709"
    assert _eq(_host(got, 10), _want(luts, "log709_33", GRADE, "tetrahedral", 10, 10, 10, "420", "422", src, "nine"))
    got, _ = apply_lut(_dev(src, engine.device), cube=luts["log709_33"][0], cdl=GOLDEN / "reel.ccc", cdl_id="a002",
                       pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv", out_pix_fmt="yuv422p10le", engine=engine)
    assert _eq(_host(got, 10), _want(luts, "log709_33", OTHER, "tetrahedral", 10, 10, 10, "420", "422", src, "nine"))


@pytest.mark.gpu
def test_cli_over_pipes_with_a_cdl_file(luts):
    """python -m lut_renderer_amd.cli --pix-fmt yuv420p10le --out-pix-fmt yuv422p10le --cube look.cube --cdl shot.cc on a piped
    frame: the twin's bytes."""
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    src = _src("natural", 64, 8, 10, "420")
    want = b"".join(p.tobytes() for p in _want(luts, "log709_33", GRADE, "tetrahedral", 10, 10, 10, "420", "422", src, "cli"))
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le"), luts["log709_33"][0],
                         info, python_bin=sys.executable, cdl=GOLDEN / "shot.cc")
    assert cmd[-2:] == ["--cdl", str(GOLDEN / "shot.cc")]
    r = subprocess.run(cmd + ["--duration", "0.040"], input=b"".join(p.tobytes() for p in src), capture_output=True, cwd=ROOT,
                       timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == want
