"""v210 frames in and out of the fused LUT pass on the GPU.  The expected output is the C oracle's fused YUV result
on the `to_planar` frames -- the subsampling-change twin (tests/_xsub_twin.py) for a 4:2:0 / 4:4:4 destination -- packed with
`to_v210` where the destination is v210.  Every comparison is array_equal on whole buffers.

Shapes: 48 x 4 -- whole units of every vector kernel (6, 12 and 24 luma samples); 50 x 6 -- split, eight whole groups on the
vector kernel and the partial ninth on the generic one; 7 x 5 -- generic alone, a partial group, odd rows into 4:2:0."""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.engine import parse_v210_fmt, yuv_side
from lut_renderer_amd.v210 import min_row_bytes, row_bytes, to_planar, to_v210
from tests import _xsub_twin as twin
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
MODES = ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")
VEC_MODES = MODES[:3]
SHAPES = ((48, 4), (50, 6), (7, 5))
TO_PLANAR = ("yuv422p10le", "yuv422p12le", "yuv422p16le", "yuv422p")
FROM_PLANAR = ("yuv422p10le", "yuv422p", "yuv422p12le", "yuv422p16le")
XSUB = ("yuv420p10le", "yuv420p", "yuv444p10le", "yuv444p")
LUT = "log709_33.cube"

_luts = {}
_refs = {}


def _lut(engine, cube_dir, name=LUT):
    if name not in _luts:
        _luts[name] = cube.read_lut(cube_dir / name)
    engine.set_lut(_luts[name])
    return _luts[name]


def _is_v(name):
    return parse_v210_fmt(name) is not None


def _want(orc, lutname, lut, mode, src_name, out_name, w, h, k, dist="natural", rng_src="tv", lut_depth=None, prelut=None):
    """(planar source codes, planar expected codes) of one frame, computed once per distinct case and shared (never modified)."""
    fin, fout = yuv_side(src_name), yuv_side(out_name)
    dl = lut_depth or fin.depth
    key = (lutname, mode, fin.depth, fout.depth, fout.csx, fout.csy, dist, w, h, k, rng_src, dl)
    if key not in _refs:
        src = frames.make_yuv(dist, w, h, fin.depth, 1, 0, k=k, full_range=(rng_src == "pc"))
        if fin.depth == 10:
            src = to_planar(to_v210(src, w), w)                    # the frame a v210 buffer really holds
        prologue = fin.depth != dl
        if (fout.csx, fout.csy) == (1, 0):
            kc = orc.yuv_constants("bt709", rng_src, "bt709", "tv", fin.depth, dl, fout.depth, 2, prologue=prologue)
            out = orc.apply_yuv(lut.table, lut.scale, mode, kc, fin.depth, dl, fout.depth, 1, 0, src, prelut=prelut)
        else:
            kc = twin.consts("bt709", rng_src, "bt709", "tv", fin.depth, dl, fout.depth, fout.csx, fout.csy, prologue=prologue)
            out = twin.apply(lut.table, lut.scale, mode, kc, dl, fout.depth, 1, 0, fout.csx, fout.csy, src, prelut=prelut)
        for p in list(src) + list(out):
            p.setflags(write=False)
        _refs[key] = (src, out)
    return _refs[key]


def _side(planes, name, w, stride=None):
    """Planar codes -> what `apply_yuv` takes for `name`: [one buffer of words] or the three planes."""
    return [to_v210(planes, w, stride)] if _is_v(name) else list(planes)


def _dev(planes, device):
    import torch
    view = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32}
    return [torch.from_numpy(np.array(p).view(view.get(p.dtype, p.dtype))).to(device) for p in planes]   # (copies)


def _host(tensors, name):
    tensors = [tensors] if hasattr(tensors, "shape") else tensors
    dt = np.uint32 if _is_v(name) else (np.uint16 if yuv_side(name).depth > 8 else np.uint8)
    return [t.cpu().numpy().view(dt) for t in tensors]


def _eq(got, want):
    return len(got) == len(want) and all(g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


class _variant:
    def __init__(self, engine, name):
        self.engine, self.name = engine, name

    def __enter__(self):
        self.engine.set_variant(self.name)

    def __exit__(self, *exc):
        self.engine.set_variant("auto")


def _has_vec(src_name, out_name):
    fin, fout = yuv_side(src_name), yuv_side(out_name)
    return fout.csx == 1 and (_is_v(src_name) or fin.depth > 8)


def _kernel_ok(name, variant, w, src_name, out_name, mode, dense=True):
    if variant == "generic" or not _has_vec(src_name, out_name) or mode not in VEC_MODES:
        return name == "k_yuv_v210_generic"
    planar = out_name if _is_v(src_name) else src_name         # (the side that is planes, if any)
    both = _is_v(src_name) and _is_v(out_name)
    bs = 2 if yuv_side(planar).depth > 8 else 1
    unit = 6 if both else (12 if bs == 2 else 24)
    # dense planes: the vector kernel wants row strides that are multiples of 4 bytes, luma and chroma
    if w < unit or (dense and not both and (w * bs % 4 or ((w + 1) // 2) * bs % 4)):
        return name == "k_yuv_v210_generic"
    return name.startswith("k_yuv_v210_vec<") and name.endswith(f",{MODES.index(mode)}>")


def _padded(tensors, cols=64):
    """Views of the planes' own columns inside rows of `cols` samples (aligned strides); a buffer of words stays as it is."""
    import torch
    out = []
    for t in tensors:
        if t.dtype == torch.int32:
            out.append(t)
            continue
        big = torch.zeros(t.shape[:-1] + (cols,), dtype=t.dtype, device=t.device)
        big[..., :t.shape[-1]] = t
        out.append(big[..., :t.shape[-1]])
    return out


def _run_pair(engine, orc, cube_dir, src_name, out_name, **kw):
    """One (source, destination) pair: 48 x 4 with three modes on vec_global (where the pair has a vector kernel) and five on
    generic; 50 x 6 and 7 x 5 on auto, dense; 50 x 6 again with the planes on padded rows, where the width is split between the
    vector kernel and the generic one."""
    okw = {k: v for k, v in kw.items() if k in ("lut_depth",)}
    rng = kw.get("range_src", "tv")
    lut = _lut(engine, cube_dir)
    cases = [(48, 4, "generic", m, True) for m in MODES] + [(50, 6, "auto", "tetrahedral", True), (7, 5, "auto", "tetrahedral", True)]
    if _has_vec(src_name, out_name):
        cases += [(48, 4, "vec_global", m, True) for m in VEC_MODES] + [(50, 6, "auto", "tetrahedral", False)]
    for w, h, variant, mode, dense in cases:
        src, out = _want(orc, LUT, lut, mode, src_name, out_name, w, h, 20 + w, rng_src=rng, **okw)
        want = _side(out, out_name, w)
        dev = _dev(_side(src, src_name, w), engine.device)
        dst = None
        if not dense:
            dev, dst = _padded(dev), _padded(_dev([np.zeros_like(p) for p in want], engine.device))
        with _variant(engine, variant):
            got = _host(engine.apply_yuv(dev, dst, pix_fmt=src_name, out_pix_fmt=out_name, interp=mode, width=w, **kw), out_name)
            name = engine.last_kernel
        assert _eq(got, want), (src_name, out_name, w, h, variant, mode, dense, name)
        assert _kernel_ok(name, variant, w, src_name, out_name, mode, dense), (src_name, out_name, w, variant, mode, dense, name)


# ------------------------------------------------------------------ sides, modes and routing
@pytest.mark.gpu
def test_v210_to_itself_and_in_place(engine, orc, cube_dir):
    _run_pair(engine, orc, cube_dir, "v210", "v210")
    lut = _lut(engine, cube_dir)
    for (w, h), variant in (((48, 4), "auto"), ((48, 4), "generic"), ((50, 6), "auto"), ((7, 5), "auto")):
        src, out = _want(orc, LUT, lut, "tetrahedral", "v210", "v210", w, h, 20 + w)
        dev = _dev(_side(src, "v210", w), engine.device)
        with _variant(engine, variant):
            res = engine.apply_yuv(dev, dev, pix_fmt="v210", width=w)
        assert res is dev and _eq(_host(dev, "v210"), _side(out, "v210", w)), (w, h, variant)
    t = _dev(_side(src, "v210", 7), engine.device)[0]                # a bare tensor in, the same bare tensor out
    assert engine.apply_yuv(t, t, pix_fmt="v210", width=7) is t and _eq(_host(t, "v210"), _side(out, "v210", 7))


@pytest.mark.gpu
@pytest.mark.parametrize("out_name", TO_PLANAR)
def test_v210_to_planar_422(engine, orc, cube_dir, out_name):
    _run_pair(engine, orc, cube_dir, "v210", out_name)


@pytest.mark.gpu
@pytest.mark.parametrize("src_name", FROM_PLANAR)
def test_planar_422_to_v210(engine, orc, cube_dir, src_name):
    _run_pair(engine, orc, cube_dir, src_name, "v210")


@pytest.mark.gpu
@pytest.mark.parametrize("out_name", XSUB)
def test_v210_to_planar_420_and_444(engine, orc, cube_dir, out_name):
    _run_pair(engine, orc, cube_dir, "v210", out_name)


@pytest.mark.gpu
def test_second_lut_and_uniform_content(engine, orc, cube_dir):
    """A lattice outside [0, 1] and one with a scaled domain, on uniform codes (every 10-bit value turns up)."""
    for lutname in ("random_9.cube", "domain_2.cube"):
        lut = _lut(engine, cube_dir, lutname)
        for src_name, out_name in (("v210", "v210"), ("v210", "yuv420p")):
            for variant in ("auto", "generic"):
                src, out = _want(orc, lutname, lut, "tetrahedral", src_name, out_name, 48, 4, 3, dist="uniform")
                with _variant(engine, variant):
                    got = engine.apply_yuv(_dev(_side(src, src_name, 48), engine.device), pix_fmt=src_name, out_pix_fmt=out_name, width=48)
                assert _eq(_host(got, out_name), _side(out, out_name, 48)), (lutname, src_name, out_name, variant)


@pytest.mark.gpu
def test_refusing_variants(engine, orc, cube_dir):
    lut = _lut(engine, cube_dir)
    src, _ = _want(orc, LUT, lut, "tetrahedral", "v210", "v210", 48, 4, 68)
    dev = _dev(_side(src, "v210", 48), engine.device)
    with _variant(engine, "vec_lds"):
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv(dev, pix_fmt="v210", width=48)
        assert e.value.code == _native.EINVAL
    src7, _ = _want(orc, LUT, lut, "tetrahedral", "v210", "v210", 7, 5, 27)
    src50, _ = _want(orc, LUT, lut, "tetrahedral", "v210", "v210", 50, 6, 70)
    src8 = frames.make_yuv("natural", 48, 4, 8, 1, 0, k=1)
    with _variant(engine, "vec_global"):
        engine.apply_yuv(dev, pix_fmt="v210", width=48)
        assert engine.last_kernel == "k_yuv_v210_vec<1,1,1,0,2>"
        engine.apply_yuv(dev, pix_fmt="v210", out_pix_fmt="yuv420p", width=48)
        assert engine.last_kernel == "k_yuv_v210_vec<0,1,0,1,2>"
        engine.apply_yuv(dev, pix_fmt="v210", out_pix_fmt="yuv422p10le", width=48, interp="nearest")
        assert engine.last_kernel == "k_yuv_v210_vec<1,1,0,0,0>"
        for args, kw in (((dev,), dict(pix_fmt="v210", width=48, interp="pyramid")),                     # no vector kernel for the mode
                         ((dev,), dict(pix_fmt="v210", width=48, out_pix_fmt="yuv444p10le")),            # nor for a 4:4:4 destination
                         ((_dev(_side(src50, "v210", 50), engine.device),), dict(pix_fmt="v210", width=50)),   # a partial unit
                         ((_dev(_side(src7, "v210", 7), engine.device),), dict(pix_fmt="v210", width=7)),
                         ((_dev(src8, engine.device),), dict(pix_fmt="yuv422p", out_pix_fmt="v210"))):   # nor for an 8-bit source
            with pytest.raises(_native.LutrError) as e:
                engine.apply_yuv(*args, **kw)
            assert e.value.code == _native.EINVAL, kw


# ------------------------------------------------------------------ the container's spare bits
@pytest.mark.gpu
def test_input_junk_is_ignored_and_output_slots_are_clean(engine, orc, cube_dir):
    """Random bits 30-31 in every word, random codes in the slots beyond the frame and random words in the row padding: the
    output is that of the clean buffer; bits 30-31 of the output are zero and the slots beyond the frame repeat the last real
    sample / pair (what `to_v210` writes)."""
    lut = _lut(engine, cube_dir)
    rng = np.random.default_rng(11)
    for w, h in ((50, 6), (7, 5), (48, 4)):
        src, out = _want(orc, LUT, lut, "tetrahedral", "v210", "v210", w, h, 20 + w)
        clean = to_v210(src, w)
        junk = rng.integers(0, 1 << 32, size=clean.shape, dtype=np.uint64).astype(np.uint32)
        # the mask of the bits that carry real samples: all-ones codes there, zeros in the other slots of the last group
        ones = [np.full(p.shape, 1023, np.uint16) for p in src]
        g6 = 6 * ((w + 5) // 6)
        wide = [np.concatenate([ones[0], np.zeros((h, g6 - w), np.uint16)], axis=1),
                np.concatenate([ones[1], np.zeros((h, g6 // 2 - ones[1].shape[1]), np.uint16)], axis=1),
                np.concatenate([ones[2], np.zeros((h, g6 // 2 - ones[2].shape[1]), np.uint16)], axis=1)]
        mask = to_v210(wide, g6)
        dirty = (clean & mask) | (junk & ~mask)
        assert (dirty != clean).any() and (dirty >> 30).any()
        assert _eq(to_planar(dirty, w), list(src))
        want = [to_v210(out, w)]
        want8 = _want(orc, LUT, lut, "tetrahedral", "v210", "yuv422p", w, h, 20 + w)[1]
        for variant in ("auto", "generic"):
            with _variant(engine, variant):
                got = _host(engine.apply_yuv(_dev([dirty], engine.device), pix_fmt="v210", width=w), "v210")
                got8 = _host(engine.apply_yuv(_dev([dirty], engine.device), pix_fmt="v210", out_pix_fmt="yuv422p", width=w), "yuv422p")
            assert _eq(got, want), (w, h, variant)
            assert not (got[0] >> 30).any(), (w, h, variant)
            assert _eq(got8, list(want8)), (w, h, variant)


@pytest.mark.gpu
def test_row_padding_is_never_written(engine, orc, cube_dir):
    """`dst` filled with a pattern first: every word past the last group of a row keeps it, on the default stride, on a custom
    stride with spare words and on the tightest one."""
    import torch
    lut = _lut(engine, cube_dir)
    for w, h in SHAPES:
        g4 = min_row_bytes(w) // 4
        for src_name in ("v210", "yuv422p10le"):
            src, out = _want(orc, LUT, lut, "tetrahedral", src_name, "v210", w, h, 20 + w)
            want = to_v210(out, w)[:, :g4]
            for words in (row_bytes(w) // 4, g4 + 4, g4):
                for variant in ("auto", "generic"):
                    dst = torch.full((h, words), 0x5a5a5a5a, dtype=torch.int32, device=engine.device)
                    with _variant(engine, variant):
                        engine.apply_yuv(_dev(_side(src, src_name, w), engine.device), [dst], pix_fmt=src_name, out_pix_fmt="v210", width=w)
                    got = dst.cpu().numpy().view(np.uint32)
                    assert np.array_equal(got[:, :g4], want), (w, h, src_name, words, variant)
                    assert (got[:, g4:] == 0x5a5a5a5a).all(), (w, h, src_name, words, variant, "wrote past the last group")


@pytest.mark.gpu
def test_three_frame_batch_with_a_padded_custom_stride(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir)
    nf, w, h = 3, 48, 4
    stride = row_bytes(w) + 64                                     # 16 spare words a row, and a spare row per frame
    for src_name, out_name in (("v210", "v210"), ("v210", "yuv422p10le"), ("yuv422p10le", "v210"), ("v210", "yuv420p")):
        refs = [_want(orc, LUT, lut, "tetrahedral", src_name, out_name, w, h, 30 + i) for i in range(nf)]

        def spaced(shape, dt):
            big = torch.zeros((shape[0], shape[1] + 1, shape[2] + (16 if dt == torch.int32 else 32)), dtype=dt, device=engine.device)
            return big[:, :shape[1], :shape[2]]

        dense = _dev([np.stack([_side(s, src_name, w)[i] for s, _ in refs]) for i in range(yuv_side(src_name).nplanes)], engine.device)
        src_v = []
        for t in dense:
            v = spaced(t.shape, t.dtype)
            v.copy_(t)
            src_v.append(v)
        fout = yuv_side(out_name)
        odt = torch.int32 if _is_v(out_name) else (torch.uint8 if fout.depth <= 8 else torch.int16)
        dst_v = [spaced((nf,) + fout.plane_shape(i, w, h), odt) for i in range(fout.nplanes)]
        if _is_v(src_name):
            assert src_v[0].stride(1) * 4 == stride
        engine.apply_yuv(src_v, dst_v, pix_fmt=src_name, out_pix_fmt=out_name, width=w)
        assert engine.last_kernel.startswith("k_yuv_v210_vec<"), engine.last_kernel
        want = [np.stack([_side(o, out_name, w)[i] for _, o in refs]) for i in range(fout.nplanes)]
        assert _eq(_host([d.contiguous() for d in dst_v], out_name), want), (src_name, out_name)


# ------------------------------------------------------------------ other layouts, through the C-ABI
def _abi(engine, src_name, out_name, w, h, nf, s, d, interp=2, row0=0, rows=None, flags=None, fmts=None):
    fin, fout = yuv_side(src_name), yuv_side(out_name)
    ci, co = fmts or (fin.code, fout.code)
    p = _native.YuvParams(ci, co, fin.depth, 0, 0, 0, 0, 0)
    vi, vo = flags if flags is not None else (int(_is_v(src_name)), int(_is_v(out_name)))
    with engine._lock:
        engine._bind_stream()
        return engine._lib.lutr_apply_yuv_v210(engine._ctx, C.byref(p), interp, vi, vo, w, h, nf, C.byref(s), C.byref(d), row0,
                                               h if rows is None else rows)


def _planes_desc(tensors, flip=False):
    st = _native.Planes()
    for i, t in enumerate(tensors):
        stride = t.stride(-2) * t.element_size()
        st.data[i] = t.data_ptr() + ((t.shape[-2] - 1) * stride if flip else 0)
        st.stride[i] = -stride if flip else stride
        st.frame_stride[i] = 0
    return st


@pytest.mark.gpu
def test_bottom_up_rows_and_a_base_offset_of_four_bytes(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir)
    w, h = 48, 4
    for src_name, out_name in (("v210", "v210"), ("v210", "yuv420p10le"), ("yuv422p10le", "v210")):
        src, out = _want(orc, LUT, lut, "tetrahedral", src_name, out_name, w, h, 20 + w)
        want = _side(out, out_name, w)
        # negative strides (a bottom-up surface): the generic kernel, the same picture
        dev = _dev([np.ascontiguousarray(p[::-1]) for p in _side(src, src_name, w)], engine.device)
        dst = _dev([np.zeros_like(p) for p in want], engine.device)
        assert _abi(engine, src_name, out_name, w, h, 1, _planes_desc(dev, flip=True), _planes_desc(dst, flip=True)) == 0
        torch.cuda.synchronize()
        assert engine.last_kernel == "k_yuv_v210_generic"
        assert _eq([g[::-1] for g in _host(dst, out_name)], want), (src_name, out_name)
        with _variant(engine, "vec_global"):
            assert _abi(engine, src_name, out_name, w, h, 1, _planes_desc(dev, flip=True), _planes_desc(dst, flip=True)) == _native.EINVAL
    # a v210 buffer 4 bytes off a 16-byte boundary
    src, out = _want(orc, LUT, lut, "tetrahedral", "v210", "v210", w, h, 20 + w)
    buf = _dev(_side(src, "v210", w), engine.device)[0]
    flat = torch.zeros(buf.numel() + 1, dtype=torch.int32, device=engine.device)
    off = flat[1:].view(buf.shape)
    off.copy_(buf)
    assert (off.data_ptr() - flat.data_ptr()) == 4 and off.data_ptr() % 16 == 4
    got = engine.apply_yuv(off, pix_fmt="v210", width=w)
    assert engine.last_kernel == "k_yuv_v210_generic"
    assert _eq(_host(got, "v210"), _side(out, "v210", w))
    with _variant(engine, "vec_global"):
        with pytest.raises(_native.LutrError) as e:
            engine.apply_yuv(off, pix_fmt="v210", width=w)
        assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_row_shard_leaves_the_rest_alone(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir)
    for src_name, out_name, w, h, r0, nr in (("v210", "v210", 48, 4, 1, 2), ("v210", "v210", 7, 5, 3, 2), ("v210", "yuv422p10le", 50, 6, 1, 3),
                                             ("yuv422p10le", "v210", 50, 6, 3, 3), ("v210", "yuv420p10le", 48, 4, 2, 2),
                                             ("v210", "yuv420p", 7, 5, 2, 3)):
        fout = yuv_side(out_name)
        src, out = _want(orc, LUT, lut, "tetrahedral", src_name, out_name, w, h, 20 + w)
        want = _side(out, out_name, w)
        g4 = min_row_bytes(w) // 4
        dev = _dev(_side(src, src_name, w), engine.device)
        for variant in ("auto", "generic"):
            dst = [torch.full(p.shape, 77, dtype=torch.int32 if _is_v(out_name) else (torch.uint8 if fout.depth <= 8 else torch.int16),
                              device=engine.device) for p in want]
            with _variant(engine, variant):
                engine.apply_yuv(dev, dst, pix_fmt=src_name, out_pix_fmt=out_name, width=w, row0=r0, rows=nr)
            for i, (g, wnt) in enumerate(zip(_host(dst, out_name), want)):
                a, b = (r0, r0 + nr) if i == 0 else (r0 >> fout.csy, (r0 + nr + fout.csy) >> fout.csy)
                cols = g4 if _is_v(out_name) else g.shape[1]
                assert np.array_equal(g[a:b, :cols], wnt[a:b, :cols]), (src_name, out_name, variant, i)
                assert (g[:a] == 77).all() and (g[b:] == 77).all(), (src_name, out_name, variant, i, "bytes outside the shard changed")
    src, _ = _want(orc, LUT, lut, "tetrahedral", "v210", "yuv420p10le", 48, 4, 68)
    with pytest.raises(_native.LutrError) as e:                  # a 4:2:0 destination takes even rows
        engine.apply_yuv(_dev(_side(src, "v210", 48), engine.device), pix_fmt="v210", out_pix_fmt="yuv420p10le", width=48, row0=1, rows=2)
    assert e.value.code == _native.EINVAL


# ------------------------------------------------------------------ everything lutr_yuv_params expresses
@pytest.mark.gpu
def test_full_range_prologue_and_lut_depth(engine, orc, cube_dir):
    _run_pair(engine, orc, cube_dir, "v210", "yuv422p", range_src="pc", lut_depth=8)
    _run_pair(engine, orc, cube_dir, "v210", "yuv420p", range_src="pc", lut_depth=8)
    _run_pair(engine, orc, cube_dir, "v210", "v210", range_src="pc", lut_depth=8)
    _run_pair(engine, orc, cube_dir, "yuv422p10le", "v210", range_src="pc", lut_depth=8)


@pytest.mark.gpu
def test_prelut(engine, orc, tmp_path):
    tab = cube.log709_lattice(17)
    shapers = [(np.array([0.0, 0.2, 0.5, 1.0]), np.array([0.0, 0.35, 0.7, 1.0]))] * 2 + \
              [(np.linspace(0.0, 1.0, 9), np.linspace(0.0, 1.0, 9) ** 0.7)]
    p = tmp_path / "shaped.csp"
    write_csp_with_prelut(p, 17, tab, shapers)
    lut = engine.load_cube(p)
    assert lut.prelut is not None
    pre = orc.parse_lut_file_ex(p)[3]
    for src_name, out_name in (("v210", "v210"), ("v210", "yuv422p"), ("v210", "yuv420p10le"), ("yuv422p10le", "v210")):
        for w, h in ((48, 4), (7, 5)):
            src, out = _want(orc, "shaped.csp", lut, "tetrahedral", src_name, out_name, w, h, 20 + w, prelut=pre)
            for variant in ("auto", "generic"):
                with _variant(engine, variant):
                    got = engine.apply_yuv(_dev(_side(src, src_name, w), engine.device), pix_fmt=src_name, out_pix_fmt=out_name, width=w)
                assert _eq(_host(got, out_name), _side(out, out_name, w)), (src_name, out_name, w, variant, engine.last_kernel)


@pytest.mark.gpu
def test_precisions_run_strict(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir)
    src, out = _want(orc, LUT, lut, "tetrahedral", "v210", "v210", 48, 4, 68)
    dev = _dev(_side(src, "v210", 48), engine.device)
    try:
        for prec in ("fast", "fma32"):
            engine.set_precision(prec)
            got = engine.apply_yuv(dev, pix_fmt="v210", width=48)
            assert engine.last_kernel == "k_yuv_v210_vec<1,1,1,0,2>", engine.last_kernel
            assert _eq(_host(got, "v210"), _side(out, "v210", 48)), prec
    finally:
        engine.set_precision("strict")
    with pytest.raises(ValueError, match="width"):
        engine.apply_yuv(dev, pix_fmt="v210")                      # v210 rows cannot tell the width
    with pytest.raises(ValueError):
        engine.apply_yuv(dev + dev, pix_fmt="v210", width=48)      # two buffers for a one-buffer format
    with pytest.raises(ValueError):
        engine.apply_yuv([dev[0][:, :28]], pix_fmt="v210", width=48)   # rows too short for eight groups
    with pytest.raises(ValueError):
        engine.apply_yuv([dev[0].view(torch.int16)], pix_fmt="v210", width=48)     # words are 32 bits
    planar = engine.apply_yuv(dev, pix_fmt="v210", out_pix_fmt="yuv422p10le", width=48)
    assert engine.apply_yuv(planar, pix_fmt="yuv422p10le", out_pix_fmt="v210")[0].shape == (4, 32)    # the planes tell the width


@pytest.mark.gpu
def test_abi_refusals(engine, orc, cube_dir):
    import torch
    lut = _lut(engine, cube_dir)
    w, h = 48, 4
    src, _ = _want(orc, LUT, lut, "tetrahedral", "v210", "v210", w, h, 68)
    buf = _dev(_side(src, "v210", w), engine.device)
    out = [torch.zeros_like(buf[0])]
    pl = _dev(src, engine.device)
    plo = [torch.zeros_like(t) for t in pl]
    sd, dd, ps, pd = _planes_desc(buf), _planes_desc(out), _planes_desc(pl), _planes_desc(plo)
    err = lambda: engine._lib.lutr_last_error()                    # noqa: E731
    F = _native.fmt_code
    v = F(10, 1, 0)
    assert _abi(engine, "v210", "v210", w, h, 1, ps, pd, flags=(0, 0)) == _native.EINVAL and b"neither side" in err()
    assert _abi(engine, "v210", "v210", w, h, 1, sd, dd, flags=(2, 1)) == _native.EINVAL and err()
    # a v210 side that is not 10-bit 4:2:2
    for fmts in ((F(8, 1, 0), v), (F(12, 1, 0), v), (F(10, 1, 1), v), (F(10, 0, 0), v), (v, F(16, 1, 0)), (v, F(10, 1, 1))):
        assert _abi(engine, "v210", "v210", w, h, 1, sd, dd, fmts=fmts) == _native.EINVAL, fmts
        assert b"10-bit 4:2:2" in err(), fmts
    # a v210 destination from a source that is not 4:2:2
    p420 = _dev(frames.natural_yuv(w, h, 10, 1, 1, k=7), engine.device)
    assert _abi(engine, "yuv420p10le", "v210", w, h, 1, _planes_desc(p420), dd) == _native.EINVAL and b"4:2:2 source" in err()
    # strides: below 16 * ceil(w / 6), not a multiple of 4; a base off a word
    for field, value, what in (("stride", 16 * 8 - 4, b"stride"), ("stride", 16 * 8 + 2, b"aligned"), ("data", buf[0].data_ptr() + 2, b"aligned")):
        for which in (0, 1):
            bad = _planes_desc(buf if which == 0 else out)
            getattr(bad, field)[0] = value
            assert _abi(engine, "v210", "v210", w, h, 1, bad if which == 0 else sd, bad if which == 1 else dd) == _native.EINVAL
            assert what in err(), (field, which, err())
    null = _planes_desc(buf)
    null.data[0] = None
    assert _abi(engine, "v210", "v210", w, h, 1, null, dd) == _native.EINVAL and b"null" in err()
    null = _planes_desc(plo)
    null.data[2] = None
    assert _abi(engine, "v210", "yuv422p10le", w, h, 1, sd, null) == _native.EINVAL and b"null" in err()
    # overlap: one row down inside the same buffer; the same bytes with another stride
    big = torch.zeros((h + 1, 32), dtype=torch.int32, device=engine.device)
    assert _abi(engine, "v210", "v210", w, h, 1, _planes_desc([big[:h]]), _planes_desc([big[1:]])) == _native.EINVAL and b"in place" in err()
    # row0 / rows off the chroma block of a 4:2:0 destination
    p420o = [torch.zeros_like(t) for t in p420]
    assert _abi(engine, "v210", "yuv420p10le", w, h, 1, sd, _planes_desc(p420o), row0=1, rows=2) == _native.EINVAL
    assert _abi(engine, "v210", "v210", w, h, 1, sd, dd, row0=2, rows=3) == _native.EINVAL
    assert _abi(engine, "v210", "v210", w, h, 1, sd, dd, interp=7) == _native.EINVAL
    # data[1] / data[2] of a v210 side may be NULL: that is what _planes_desc left there
    assert sd.data[1] is None and _abi(engine, "v210", "v210", w, h, 1, sd, dd) == 0
    torch.cuda.synchronize()
    assert engine.last_kernel.startswith("k_yuv_v210_vec<")


# ------------------------------------------------------------------ apply_lut, host pipeline, CLI, row-sharded group
@pytest.mark.gpu
def test_apply_lut(engine, orc, cube_dir):
    import torch
    from lut_renderer_amd.api import apply_lut
    lut = _lut(engine, cube_dir)
    for src_name, out_name, w, h in (("v210", None, 50, 6), ("v210", "yuv420p10le", 7, 5), ("yuv422p10le", "v210", 48, 4)):
        src, out = _want(orc, LUT, lut, "tetrahedral", src_name, out_name or "v210", w, h, 20 + w)
        planes = _dev(_side(src, src_name, w), engine.device)
        got, _ = apply_lut(planes[0] if _is_v(src_name) else planes, cube=lut, pix_fmt=src_name, out_pix_fmt=out_name, width=w,
                           colorspace="bt709", engine=engine)
        assert _eq(_host(got, out_name or "v210"), _side(out, out_name or "v210", w)), (src_name, out_name)
    # a full-range source: the 8-bit intermediate is planar yuv422p -- the bits of the planar call on the unpacked frame
    src, _ = _want(orc, LUT, lut, "tetrahedral", "v210", "yuv422p", 48, 4, 68, rng_src="pc", lut_depth=8)
    got, _ = apply_lut(_dev(_side(src, "v210", 48), engine.device), cube=lut, pix_fmt="v210", width=48, colorspace="bt709",
                       color_range="pc", engine=engine)
    ref, _ = apply_lut(_dev(src, engine.device), cube=lut, pix_fmt="yuv422p10le", colorspace="bt709", color_range="pc", engine=engine)
    assert len(got) == 3 and got[0].dtype == torch.uint8 and _eq(_host(got, "yuv422p"), _host(ref, "yuv422p"))


@pytest.mark.gpu
def test_host_pipeline(engine, orc, cube_dir):
    from lut_renderer_amd.stream import HostPipeline
    lut = _lut(engine, cube_dir)
    nf = 3
    for src_name, out_name, w, h in (("v210", "v210", 50, 6), ("v210", "yuv420p", 7, 5), ("yuv422p10le", "v210", 48, 4)):
        refs = [_want(orc, LUT, lut, "tetrahedral", src_name, out_name, w, h, 30 + i) for i in range(nf)]
        stream_in = b"".join(p.tobytes() for s, _ in refs for p in _side(s, src_name, w))
        want = b"".join(p.tobytes() for _, o in refs for p in _side(o, out_name, w))
        pipe = HostPipeline(engine, src_name, w, h, batch=2, out_pix_fmt=out_name)
        if _is_v(src_name):
            assert pipe.fin.frame_bytes == row_bytes(w) * h
        pos, chunks = {"i": 0}, []

        def fill(buf, max_frames):
            n = min(max_frames, nf - pos["i"])
            nb = n * pipe.fin.frame_bytes
            buf[:nb] = np.frombuffer(stream_in, np.uint8, nb, pos["i"] * pipe.fin.frame_bytes)
            pos["i"] += n
            return n

        assert pipe.run(fill, lambda buf, n: chunks.append(bytes(buf)), total_frames=nf) == nf
        assert b"".join(chunks) == want, (src_name, out_name)


@pytest.mark.gpu
def test_cli_round_trip_over_pipes(engine, orc, cube_dir):
    lut = _lut(engine, cube_dir)
    nf, w, h = 3, 50, 6
    refs = [_want(orc, LUT, lut, "tetrahedral", "v210", "v210", w, h, 30 + i) for i in range(nf)]
    cmd = [sys.executable, "-m", "lut_renderer_amd.cli", "-i", "-", "-o", "-", "--size", f"{w}x{h}", "--pix-fmt", "v210",
           "--cube", str(cube_dir / LUT), "--colorspace", "bt709", "--batch", "2", "--duration", f"{nf / 25.0:.3f}"]
    r = subprocess.run(cmd, input=b"".join(to_v210(s, w).tobytes() for s, _ in refs), capture_output=True, cwd=ROOT, timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == b"".join(to_v210(o, w).tobytes() for _, o in refs)


@pytest.mark.gpu
def test_group_passes_v210_frames_through(engine, orc, cube_dir, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    lut = _lut(engine, cube_dir)
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    for src_name, out_name, w, h, blocks in (("v210", "v210", 50, 6, [(0, 3), (3, 6)]), ("v210", "yuv420p", 48, 4, [(0, 2), (2, 4)]),
                                             ("yuv422p10le", "v210", 7, 5, None)):
        src, out = _want(orc, LUT, lut, "tetrahedral", src_name, out_name, w, h, 20 + w)
        with LutEngineGroup([0, 0]) as g:
            g.set_lut(lut)
            got = g.apply_yuv(_dev(_side(src, src_name, w), engine.device), pix_fmt=src_name, out_pix_fmt=out_name, width=w)
            assert g.last_remote == 1 and (blocks is None or g.last_blocks == blocks), g.last_blocks
            assert all(r0 % (1 << yuv_side(out_name).csy) == 0 for r0, _ in g.last_blocks)
            assert _eq(_host(got, out_name), _side(out, out_name, w)), (src_name, out_name)
