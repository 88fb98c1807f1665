"""Two YUV outputs from one LUT pass on the GPU: each output of lutr_apply_yuv_dual bit-exact against the oracle
(oracle.binding's fused YUV for an unchanged layout, tests/_xsub_twin.py for a changed one) AND against what the single-output
call returns for it alone."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from oracle import binding as orc
from tests import _xsub_twin as twin
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
LAYOUTS = twin.LAYOUTS
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
GENERIC = "k_yuv_dual_generic"
_refs = {}           # expected planes, computed once per case and shared (never written to)


def _fmt(depth, lay):
    return f"yuv{lay}p" + ("" if depth == 8 else f"{depth}le")


def _dev(planes, device):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(p).view(np.int16) if p.dtype == np.uint16 else np.ascontiguousarray(p)).to(device)
            for p in planes]


def _host(tensors, dout):
    return [t.cpu().numpy().view(np.uint16) if dout > 8 else t.cpu().numpy() for t in tensors]


def _eq(got, want):
    return all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))


def _want(lut, mode, din, dl, dout, a, b, src, rin="tv", prologue=False, matrix="bt709", prelut=None):
    """One output's expected planes: the oracle's fused YUV when the layout stays, the twin's composition when it changes."""
    (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
    k = twin.consts(matrix, rin, matrix, "tv", din, dl, dout, ocsx, ocsy, prologue=prologue)
    if a == b:
        return orc.apply_yuv(lut.table, lut.scale, mode, k, din, dl, dout, icsx, icsy, src, prelut=prelut)
    return twin.apply(lut.table, lut.scale, mode, k, dl, dout, icsx, icsy, ocsx, ocsy, src, prelut=prelut)


def _vec_name(din, da, db, a, b, mode):
    """The vector kernel's name: output A is the 4:2:2 one, B has layout `b`."""
    (icsx, icsy), (bcsx, bcsy) = LAYOUTS[a], LAYOUTS[b]
    return f"k_yuv_dual_vec<{int(din > 8)},{int(da > 8)},{int(db > 8)},{icsx},{icsy},{bcsx},{bcsy},{MODES.index(mode)}>"


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


def _case(engine, lut, w, h, src_fmt, out1, out2, mode="tetrahedral", kernel=None, key=None, k=1, **kw):
    """Run the dual pass on a natural frame; both outputs against the oracle and against the single-output calls."""
    (din, a), (d1, b1), (d2, b2) = src_fmt, out1, out2
    rk = (key, w, h, src_fmt, out1, out2, mode, k)
    if rk not in _refs:
        src = frames.natural_yuv(w, h, din, *LAYOUTS[a], k=k)
        _refs[rk] = (src, _want(lut, mode, din, din, d1, a, b1, src), _want(lut, mode, din, din, d2, a, b2, src))
    src, want1, want2 = _refs[rk]
    dev = _dev(src, engine.device)
    names = dict(pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(d1, b1), out2_pix_fmt=_fmt(d2, b2))
    got1, got2 = engine.apply_yuv_dual(dev, interp=mode, **names, **kw)
    name = engine.last_kernel
    if kernel is not None:
        assert name == kernel, (name, kernel)
    assert _eq(_host(got1, d1), want1), (names, mode, name, "output 1 against the oracle")
    assert _eq(_host(got2, d2), want2), (names, mode, name, "output 2 against the oracle")
    for got, (d, b) in ((got1, out1), (got2, out2)):
        alone = engine.apply_yuv(dev, pix_fmt=_fmt(din, a), out_pix_fmt=_fmt(d, b), interp=mode, **kw)
        assert _eq(_host(got, d), _host(alone, d)), (names, mode, name, engine.last_kernel)
    return name


# ------------------------------------------------------------------ the pro-mode pairs: shapes, modes, variants
@pytest.mark.gpu
@pytest.mark.parametrize("second", [(8, "420"), (10, "420")], ids=["yuv420p", "yuv420p10le"])
def test_pro_mode_pairs(engine, cube_dir, second):
    """yuv420p10le -> yuv422p10le + delivery: 64x8 in two frames on padded rows (vector), 70x6 (vector + generic split), 33x5
    (generic, the edge rule in both layouts)."""
    import torch
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    src_fmt, master = (10, "420"), (10, "422")
    d2, b2 = second
    for mode in MODES:
        with _variant(engine, "generic"):
            _case(engine, lut, 64, 8, src_fmt, master, second, mode, kernel=GENERIC)
        if mode in VEC_MODES:
            with _variant(engine, "vec_global"):
                _case(engine, lut, 64, 8, src_fmt, master, second, mode, kernel=_vec_name(10, 10, d2, "420", b2, mode))
    assert _case(engine, lut, 64, 8, src_fmt, master, second) == _vec_name(10, 10, d2, "420", b2, "tetrahedral")
    assert _case(engine, lut, 33, 5, src_fmt, master, second) == GENERIC
    # two frames, every row padded to 96 samples; 64 columns = whole units, 70 = the last 6 columns go to the generic kernel
    for w, h in ((64, 8), (70, 6)):
        fs = [frames.natural_yuv(w, h, 10, 1, 1, k=3 + i) for i in range(2)]
        shapes = {"420": [(h, w), (h // 2, w // 2), (h // 2, w // 2)], "422": [(h, w), (h, w // 2), (h, w // 2)]}

        def padded(shape_list, dt, fill):
            full = [torch.full((2, s[0], 96), fill, dtype=dt, device=engine.device) for s in shape_list]
            return full, [t[:, :, :s[1]] for t, s in zip(full, shape_list)]
        sfull, sview = padded(shapes["420"], torch.int16, 0)
        for i, f in enumerate(fs):
            for v, p in zip(sview, f):
                v[i] = torch.from_numpy(p.view(np.int16)).to(engine.device)
        afull, aview = padded(shapes["422"], torch.int16, -1)
        bfull, bview = padded(shapes[b2], torch.int16 if d2 > 8 else torch.uint8, -1 if d2 > 8 else 255)
        engine.apply_yuv_dual(sview, aview, bview, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", out2_pix_fmt=_fmt(d2, b2))
        assert engine.last_kernel == _vec_name(10, 10, d2, "420", b2, "tetrahedral"), (w, engine.last_kernel)
        for i, f in enumerate(fs):
            assert _eq([o[i] for o in _host(aview, 10)], _want(lut, "tetrahedral", 10, 10, 10, "420", "422", f)), (w, i)
            assert _eq([o[i] for o in _host(bview, d2)], _want(lut, "tetrahedral", 10, 10, d2, "420", b2, f)), (w, i)
        for full, shape_list in ((afull, shapes["422"]), (bfull, shapes[b2])):
            assert all((t[:, :, s[1]:] == t[0, 0, 95]).all() for t, s in zip(full, shape_list)), "wrote past the row"


@pytest.mark.gpu
@pytest.mark.parametrize("a", list(LAYOUTS))
def test_every_input_layout_against_every_second_layout(engine, cube_dir, a):
    """The 4:2:2 master with each layout of the second output, in the three container mixes the vector kernels have."""
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for b in LAYOUTS:
        for din, da, db in ((10, 10, 10), (10, 10, 8), (8, 8, 8), (12, 12, 12)):
            name = _case(engine, lut, 64, 8, (din, a), (da, "422"), (db, b), k=din + db)
            assert name == _vec_name(din, da, db, a, b, "tetrahedral"), name
        # dense rows of 70 samples are not aligned to a thread's words: nothing to split, the generic kernel takes the frame
        assert _case(engine, lut, 70, 6, (10, a), (10, "422"), (8, b), "trilinear") == GENERIC
        assert _case(engine, lut, 72, 6, (10, a), (10, "422"), (8, b), "trilinear") == _vec_name(10, 10, 8, a, b, "trilinear")
        assert _case(engine, lut, 33, 5, (10, a), (10, "422"), (8, b), "trilinear") == GENERIC
        assert _case(engine, lut, 33, 5, (8, a), (8, "422"), (8, b), "nearest") == GENERIC


@pytest.mark.gpu
def test_the_8_plus_8_mix_roles_swapped_and_what_the_vector_set_leaves_out(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    assert _case(engine, lut, 64, 8, (8, "420"), (8, "422"), (8, "420")) == _vec_name(8, 8, 8, "420", "420", "tetrahedral")
    # 4:2:2 given as the SECOND output: the launcher swaps the roles and the vector kernel still runs
    assert _case(engine, lut, 64, 8, (10, "420"), (8, "420"), (10, "422")) == _vec_name(10, 10, 8, "420", "420", "tetrahedral")
    assert _case(engine, lut, 64, 8, (10, "444"), (10, "444"), (10, "422")) == _vec_name(10, 10, 10, "444", "444", "tetrahedral")
    assert _case(engine, lut, 72, 6, (8, "422"), (8, "420"), (8, "422")) == _vec_name(8, 8, 8, "422", "420", "tetrahedral")
    # both 4:2:2, only one of them wide: the wide one is A
    assert _case(engine, lut, 64, 8, (10, "420"), (8, "422"), (10, "422")) == _vec_name(10, 10, 8, "420", "422", "tetrahedral")
    # two outputs without a 4:2:2 one; an 8-bit source to a 10-bit master; a 16-bit source to two 8-bit outputs
    assert _case(engine, lut, 64, 8, (10, "420"), (10, "444"), (8, "420")) == GENERIC
    assert _case(engine, lut, 64, 8, (8, "420"), (10, "422"), (8, "420")) == GENERIC
    assert _case(engine, lut, 64, 8, (10, "420"), (8, "422"), (8, "420")) == GENERIC
    assert _case(engine, lut, 33, 5, (10, "444"), (12, "444"), (9, "444")) == GENERIC          # a 1 x 1 union block


@pytest.mark.gpu
def test_variants_that_cannot_take_the_call(engine, cube_dir):
    engine.load_cube(cube_dir / "log709_33.cube")
    dev = _dev(frames.natural_yuv(64, 8, 10, 1, 1, k=8), engine.device)
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", out2_pix_fmt="yuv420p")
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError, match="no LDS-window kernel for two outputs") as e:
            engine.apply_yuv_dual(dev, **names)
        assert e.value.code == _native.EINVAL
    with _variant(engine, "vec_global"):
        for kw in (dict(interp="pyramid"), dict(out_pix_fmt="yuv444p10le")):
            with pytest.raises(_native.LutrError, match="cannot take this layout") as e:
                engine.apply_yuv_dual(dev, **{**names, **kw})
            assert e.value.code == _native.EINVAL
        odd = _dev(frames.natural_yuv(33, 5, 10, 1, 1, k=8), engine.device)
        with pytest.raises(_native.LutrError, match="cannot take this layout"):
            engine.apply_yuv_dual(odd, **names)


# ------------------------------------------------------------------ everything *p expresses on the input side
@pytest.mark.gpu
def test_full_range_prologue_lut_depth_and_matrices(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    for w, h in ((64, 8), (33, 5)):
        # a yuvj420p-style source: pc 8 bit, the prologue to tv ahead of the LUT (lut_depth 8), bt601
        src = frames.uniform_yuv(w, h, 8, 1, 1, k=10, full_range=True)
        kw = dict(matrix_in="smpte170m", matrix_out="smpte170m", range_src="pc", range_in="tv", lut_depth=8)
        got1, got2 = engine.apply_yuv_dual(_dev(src, engine.device), pix_fmt="yuv420p", out_pix_fmt="yuv422p",
                                           out2_pix_fmt="yuv420p", **kw)
        assert engine.last_kernel == (_vec_name(8, 8, 8, "420", "420", "tetrahedral") if w == 64 else GENERIC)
        for got, b in ((got1, "422"), (got2, "420")):
            want = _want(lut, "tetrahedral", 8, 8, 8, "420", b, src, rin="tv", prologue=True, matrix="smpte170m")
            assert _eq(_host(got, 8), want), (w, h, b)
        # a 10-bit full-range 4:2:2 source, the LUT at 8 bit (SURVEY.md Appendix D case D), master and delivery at 10 bit
        src = frames.uniform_yuv(w, h, 10, 1, 0, k=11, full_range=True)
        got1, got2 = engine.apply_yuv_dual(_dev(src, engine.device), pix_fmt="yuv422p10le", out_pix_fmt="yuv422p10le",
                                           out2_pix_fmt="yuv420p10le", **kw)
        for got, b in ((got1, "422"), (got2, "420")):
            want = _want(lut, "tetrahedral", 10, 8, 10, "422", b, src, rin="tv", prologue=True, matrix="smpte170m")
            assert _eq(_host(got, 10), want), (w, h, b)


@pytest.mark.gpu
def test_prelut(engine, tmp_path):
    tab = cube.log709_lattice(17)
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, tab, shapers)
    lut = engine.load_cube(p)
    assert lut.prelut is not None
    pre = orc.parse_lut_file_ex(p)[3]
    for (w, h), mode in (((64, 8), "tetrahedral"), ((33, 5), "prism")):
        src = frames.natural_yuv(w, h, 10, 1, 1, k=2)
        got1, got2 = engine.apply_yuv_dual(_dev(src, engine.device), pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le",
                                           out2_pix_fmt="yuv420p", interp=mode)
        assert _eq(_host(got1, 10), _want(lut, mode, 10, 10, 10, "420", "422", src, prelut=pre)), (w, mode, engine.last_kernel)
        assert _eq(_host(got2, 8), _want(lut, mode, 10, 10, 8, "420", "420", src, prelut=pre)), (w, mode, engine.last_kernel)


@pytest.mark.gpu
def test_fast_and_fma32_run_strict(engine, cube_dir):
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    src = frames.natural_yuv(64, 8, 10, 1, 1, k=6)
    want1, want2 = (_want(lut, "tetrahedral", 10, 10, d, "420", b, src) for d, b in ((10, "422"), (8, "420")))
    try:
        for prec in ("fast", "fma32"):
            engine.set_precision(prec)
            got1, got2 = engine.apply_yuv_dual(_dev(src, engine.device), pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le",
                                               out2_pix_fmt="yuv420p")
            assert engine.last_kernel == _vec_name(10, 10, 8, "420", "420", "tetrahedral"), (prec, engine.last_kernel)
            assert _eq(_host(got1, 10), want1) and _eq(_host(got2, 8), want2), prec
    finally:
        engine.set_precision("strict")


# ------------------------------------------------------------------ rows, overlap, layouts through the C-ABI
@pytest.mark.gpu
def test_row_shards_on_the_union_block(engine, cube_dir):
    engine.load_cube(cube_dir / "log709_33.cube")
    names = dict(pix_fmt="yuv422p10le", out_pix_fmt="yuv422p10le", out2_pix_fmt="yuv420p")     # 4:2:0 only on the second output
    for w, h in ((64, 8), (33, 5)):
        dev = _dev(frames.natural_yuv(w, h, 10, 1, 0, k=12), engine.device)
        whole = engine.apply_yuv_dual(dev, **names)
        for r0 in (2, 4):
            a, b = engine.apply_yuv_dual(dev, row0=0, rows=r0, **names)
            engine.apply_yuv_dual(dev, a, b, row0=r0, rows=h - r0, **names)
            assert _eq(_host(a, 10), _host(whole[0], 10)) and _eq(_host(b, 8), _host(whole[1], 8)), (w, h, r0)
        for kw in (dict(row0=1, rows=h - 1), dict(row0=0, rows=3)):
            with pytest.raises(_native.LutrError, match="multiples of the union chroma block height 2") as e:
                engine.apply_yuv_dual(dev, **names, **kw)
            assert e.value.code == _native.EINVAL


def _desc(tensors, flip=False, offset=0):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        stride = t.stride(-2) * t.element_size()
        st.data[i] = t.data_ptr() + offset + ((t.shape[-2] - 1) * stride if flip else 0)
        st.stride[i] = -stride if flip else stride
        st.frame_stride[i] = 0
    return st


def _abi(engine, fin, f1, f2, w, h, s, d1, d2, interp=2, row0=0, rows=None, fmt2=None):
    from lut_renderer_amd.engine import parse_pix_fmt
    fi, fa, fb = (parse_pix_fmt(f) for f in (fin, f1, f2))
    p = _native.YuvParams(fi.code, fa.code, fi.depth, 0, 0, 0, 0, 0)
    with engine._lock:
        engine._bind_stream()
        return engine._lib.lutr_apply_yuv_dual(engine._ctx, C.byref(p), fb.code if fmt2 is None else fmt2, interp, w, h, 1,
                                               None if s is None else C.byref(s), None if d1 is None else C.byref(d1),
                                               None if d2 is None else C.byref(d2), row0, h if rows is None else rows)


@pytest.mark.gpu
def test_overlap_and_bad_arguments_are_refused(engine, cube_dir):
    import torch
    engine.load_cube(cube_dir / "log709_33.cube")
    names = dict(pix_fmt="yuv422p10le", out_pix_fmt="yuv422p10le", out2_pix_fmt="yuv422p10le")
    w, h = 64, 8
    dev = _dev(frames.natural_yuv(w, h, 10, 1, 0, k=13), engine.device)
    other = [torch.zeros_like(t) for t in dev]
    third = [torch.zeros_like(t) for t in dev]
    engine.apply_yuv_dual(dev, other, third, **names)
    torch.cuda.synchronize()
    before = [t.clone() for t in other + third]
    with pytest.raises(_native.LutrError, match="cannot run in place: the byte range of source plane 0 overlaps"):
        engine.apply_yuv_dual(dev, dev, other, **names)                                   # dst is src
    with pytest.raises(_native.LutrError, match="the two destinations overlap"):
        engine.apply_yuv_dual(dev, other, other, **names)                                 # dst2 is dst
    # a dst2 plane inside a src plane: the second destination's Cb is the lower half of the source's luma
    inside = [third[0], dev[0][:, :w // 2], third[2]]
    with pytest.raises(_native.LutrError, match=r"source plane 0 overlaps that of destination plane 1 .*second destination") as e:
        engine.apply_yuv_dual(dev, other, inside, **names)
    assert e.value.code == _native.EINVAL
    f = "yuv422p10le"
    s, d1, d2 = _desc(dev), _desc(other), _desc(third)
    for fmt2, word in ((_native.fmt_code(7, 1, 0), "fmt_out2"), (_native.fmt_code(17, 1, 0), "fmt_out2"),
                       (_native.fmt_code(10, 0, 1), "fmt_out2"), (1 << 12 | _native.fmt_code(10, 1, 0), "fmt_out2")):
        assert _abi(engine, f, f, f, w, h, s, d1, d2, fmt2=fmt2) == _native.EINVAL
        assert word in engine._lib.lutr_last_error().decode()
    assert _abi(engine, f, f, f, w, h, s, d1, None) == _native.EINVAL and "null" in engine._lib.lutr_last_error().decode()
    gap = _desc(third)
    gap.data[1] = None
    assert _abi(engine, f, f, f, w, h, s, d1, gap) == _native.EINVAL and "null plane 1" in engine._lib.lutr_last_error().decode()
    for bad, word in (((_desc(dev, offset=1), d1, d2), "source plane 0"), ((s, d1, _desc(third, offset=1)), "second destination plane 0")):
        assert _abi(engine, f, f, f, w, h, *bad) == _native.EINVAL
        msg = engine._lib.lutr_last_error().decode()
        assert word in msg and "2-byte aligned" in msg
    odd = _desc(third)
    odd.stride[2] += 1
    assert _abi(engine, f, f, f, w, h, s, d1, odd) == _native.EINVAL
    assert "second destination plane 2" in engine._lib.lutr_last_error().decode()
    assert _abi(engine, f, f, "yuv420p10le", w, h, s, d1, d2, row0=1, rows=h - 1) == _native.EINVAL
    assert "union" in engine._lib.lutr_last_error().decode()
    assert _abi(engine, f, f, f, w, h, s, d1, d2, interp=7) == _native.EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, other + third)), "a refused call wrote to a destination"


@pytest.mark.gpu
def test_bottom_up_rows_and_a_base_offset_that_breaks_alignment(engine, cube_dir):
    import torch
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    w, h = 64, 8
    src = frames.natural_yuv(w, h, 10, 1, 1, k=14)
    want1, want2 = (_want(lut, "tetrahedral", 10, 10, d, "420", b, src) for d, b in ((10, "422"), (8, "420")))
    fin, f1, f2 = "yuv420p10le", "yuv422p10le", "yuv420p"
    # negative row strides (a bottom-up surface; torch has none, so through the C-ABI): the generic kernel, the same picture
    dev = _dev([np.ascontiguousarray(p[::-1]) for p in src], engine.device)
    a = [torch.zeros((h, w), dtype=torch.int16, device=engine.device)] + \
        [torch.zeros((h, w // 2), dtype=torch.int16, device=engine.device) for _ in range(2)]
    b = [torch.zeros((h, w), dtype=torch.uint8, device=engine.device)] + \
        [torch.zeros((h // 2, w // 2), dtype=torch.uint8, device=engine.device) for _ in range(2)]
    assert _abi(engine, fin, f1, f2, w, h, _desc(dev, flip=True), _desc(a, flip=True), _desc(b, flip=True)) == 0
    torch.cuda.synchronize()
    assert engine.last_kernel == GENERIC
    assert _eq([g[::-1] for g in _host(a, 10)], want1) and _eq([g[::-1] for g in _host(b, 8)], want2)
    with _variant(engine, "vec_global"):
        assert _abi(engine, fin, f1, f2, w, h, _desc(dev, flip=True), _desc(a, flip=True), _desc(b, flip=True)) == _native.EINVAL
    # the second output's luma starts one byte into its allocation: no whole-word stores, the generic kernel, equal bits
    dev = _dev(src, engine.device)
    flat = torch.zeros(h * w + 1, dtype=torch.uint8, device=engine.device)
    off = flat[1:].view(h, w)
    assert off.data_ptr() % 4 == 1 or off.data_ptr() % 2 == 1
    got1, got2 = engine.apply_yuv_dual(dev, None, [off, b[1], b[2]], pix_fmt=fin, out_pix_fmt=f1, out2_pix_fmt=f2)
    assert engine.last_kernel == GENERIC
    assert _eq(_host(got1, 10), want1) and _eq(_host(got2, 8), want2)
    with _variant(engine, "vec_global"):
        with pytest.raises(_native.LutrError):
            engine.apply_yuv_dual(dev, None, [off, b[1], b[2]], pix_fmt=fin, out_pix_fmt=f1, out2_pix_fmt=f2)


# ------------------------------------------------------------------ apply_lut, host pipeline, CLI, group
def _stream(lut, w, h, nf):
    fs = [frames.natural_yuv(w, h, 10, 1, 1, k=30 + i) for i in range(nf)]
    want1 = b"".join(p.tobytes() for f in fs for p in _want(lut, "tetrahedral", 10, 10, 10, "420", "422", f))
    want2 = b"".join(p.tobytes() for f in fs for p in _want(lut, "tetrahedral", 10, 10, 8, "420", "420", f))
    return fs, b"".join(p.tobytes() for f in fs for p in f), want1, want2


@pytest.mark.gpu
def test_apply_lut_with_a_second_format(engine, cube_dir):
    from lut_renderer_amd.api import apply_lut
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    src = frames.natural_yuv(64, 8, 10, 1, 1, k=30)
    (got1, got2), tags = apply_lut(_dev(src, engine.device), cube=lut, pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv",
                                   out_pix_fmt="yuv422p10le", second_pix_fmt="yuv420p", engine=engine)
    assert engine.last_kernel.startswith("k_yuv_dual_vec<")
    alone, tags1 = apply_lut(_dev(src, engine.device), cube=lut, pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv",
                             out_pix_fmt="yuv422p10le", engine=engine)
    assert tags == tags1 and _eq(_host(got1, 10), _host(alone, 10))
    assert _eq(_host(got1, 10), _want(lut, "tetrahedral", 10, 10, 10, "420", "422", src))
    assert _eq(_host(got2, 8), _want(lut, "tetrahedral", 10, 10, 8, "420", "420", src))


@pytest.mark.gpu
def test_host_pipeline_with_a_second_ring(engine, cube_dir):
    from lut_renderer_amd.stream import HostPipeline
    lut = engine.load_cube(cube_dir / "log709_33.cube")
    w, h, nf = 64, 8, 5
    _, stream_in, want1, want2 = _stream(lut, w, h, nf)
    pipe = HostPipeline(engine, "yuv420p10le", w, h, batch=2, out_pix_fmt="yuv422p10le", second_pix_fmt="yuv420p")
    assert pipe.fout.frame_bytes == w * h * 4 and pipe.fout2.frame_bytes == w * h * 3 // 2
    pos, one, two = {"i": 0}, [], []

    def fill(buf, max_frames):
        n = min(max_frames, nf - pos["i"])
        nb = n * pipe.fin.frame_bytes
        buf[:nb] = np.frombuffer(stream_in, np.uint8, nb, pos["i"] * pipe.fin.frame_bytes)
        pos["i"] += n
        return n

    assert pipe.run(fill, lambda buf, n: one.append(bytes(buf)), total_frames=nf, drain2=lambda buf, n: two.append(bytes(buf))) == nf
    assert b"".join(one) == want1 and b"".join(two) == want2
    with pytest.raises(ValueError, match="drain2 goes with second_pix_fmt"):
        pipe.run(fill, lambda buf, n: None, total_frames=nf)


@pytest.mark.gpu
def test_cli_over_pipes_with_a_second_file(cube_dir, tmp_path):
    from lut_renderer_amd.command import _master_params, engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    w, h, nf = 64, 8, 3
    _, stream_in, want1, want2 = _stream(lut, w, h, nf)
    info = VideoInfo(width=w, height=h, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    second = tmp_path / "delivery.yuv"
    cmd = engine_command(Path("-"), Path("-"), _master_params(ProcessingParams(video_codec="libx264")), cube_dir / "log709_33.cube",
                         info, python_bin=sys.executable, second_output=second, second_pix_fmt="yuv420p")
    r = subprocess.run(cmd + ["--duration", f"{nf / 25.0:.3f}", "--batch", "2"], input=stream_in, capture_output=True, cwd=ROOT,
                       timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == want1 and second.read_bytes() == want2
    report = r.stderr.decode()
    assert "Duration: 00:00:00.12" in report and "time=00:00:00.12" in report


@pytest.mark.gpu
def test_group_shards_on_the_union_block(engine, cube_dir):
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = cube.read_lut(cube_dir / "log709_33.cube")
    for w, h in ((64, 8), (33, 5)):
        src = frames.natural_yuv(w, h, 10, 1, 0, k=9)
        want1 = _want(lut, "tetrahedral", 10, 10, 10, "422", "422", src)
        want2 = _want(lut, "tetrahedral", 10, 10, 8, "422", "420", src)
        for n in (2, 3):
            with LutEngineGroup([0] * n, treat_as_remote=True) as g:
                g.set_lut(lut)
                got1, got2 = g.apply_yuv_dual(_dev(src, engine.device), pix_fmt="yuv422p10le", out_pix_fmt="yuv422p10le",
                                              out2_pix_fmt="yuv420p")
                assert g.last_remote == sum(1 for r0, r1 in g.last_blocks[1:] if r1 > r0)
                assert all(r0 % 2 == 0 for r0, _ in g.last_blocks), g.last_blocks
                assert _eq(_host(got1, 10), want1) and _eq(_host(got2, 8), want2), (w, h, n)
