"""The stage stack on packed 4:2:2 / v210 frames (lutr_apply_yuv_stack_packed / lutr_apply_yuv_stack_v210) on
the GPU: for every call the entry accepts,

    apply_yuv_stack_packed(src in container A -> dst in container B) == hold_B(apply_yuv_stack(planar samples of src))

bit for bit on whole buffers.  The expected planes are tests/_stack_twin.py's composition on the planar samples, fed the product's
own host tables as tests/test_gpu_stack.py does, then put into the destination's container with `packedyuv.to_packed` /
`v210.to_v210`.  Shapes: those of tests/test_gpu_pkyuv.py / tests/test_gpu_v210.py -- 64 x 8 (packed) and 48 x 4 (v210) for the
vector kernels, 70 x 6 / 50 x 6 for a vector plus generic split, 33 x 5 / 7 x 5 odd -- each at 2 frames.
"""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from lut_renderer_amd import _native, v210
from lut_renderer_amd.formats import parse_stages, yuv_side
from tests import _gpu_stack_packed_worker as worker
from tests.test_gpu_stack import (GOLDEN, LAYOUTS, ROOT, _desc, _dev, _fmt, _host, _lds, _list, _src, _variant,  # noqa: F401
                                  _want, grade, l1ds, loaded, luts)

NF = 2
LAY = {v: k for k, v in LAYOUTS.items()}
CHILD_LIMIT_S = 120
PACKED = list(_native.PACKED_YUV_FORMATS)
VEC_MODES = ("nearest", "trilinear", "tetrahedral")
#: (vector shape, ragged shape, odd shape) of a call by the kind of its container
SHAPES = {"pk": ((64, 8), (70, 6), (33, 5)), "v210": ((48, 4), (50, 6), (7, 5))}


def _kind(a, b):
    return "v210" if "v210" in (a, b) else "pk"


def _generic(a, b):
    return "k_yuv_stack_v210_generic" if _kind(a, b) == "v210" else "k_yuv_stack_pk_generic"


def _lay(name):
    s = yuv_side(name)
    return s, LAY[(s.csx, s.csy)]


def _held(planar, name, w):
    return worker.held(planar, name, w)


def _np(got):
    """what the engine returned, as unsigned numpy buffers: a list of planes for a planar side, the one buffer of a packed 4:2:2 /
    v210 side (which the engine hands back bare or, like `apply_yuv`, in a one-element list)"""
    def one(t):
        a = t.cpu().numpy()
        return a.view(np.uint16) if a.dtype == np.int16 else a.view(np.uint32) if a.dtype == np.int32 else a
    if isinstance(got, (list, tuple)):
        return one(got[0]) if len(got) == 1 else [one(t) for t in got]
    return one(got)


def _same(got, want):
    if isinstance(want, list):
        return isinstance(got, list) and len(got) == len(want) and all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want))
    return not isinstance(got, list) and got.shape == want.shape and np.array_equal(got, want)


def _plane_fits(stride, rows, align, nf):
    """a dense plane of `stride` bytes a row (fresh allocations are aligned far beyond 16 bytes)"""
    return stride % align == 0 and (nf == 1 or (stride * rows) % align == 0)


def _vec(a, b, stages, lds=None):
    """the vector kernel of a pair of containers as `last_kernel` spells it, without the list"""
    fa, fb = yuv_side(a), yuv_side(b)
    tri = int(any(m == "trilinear" for _, m in parse_stages(stages)))
    lds = int(_lds(stages, fa.depth) if lds is None else lds)
    if _kind(a, b) == "v210":
        vi, vo = int(a == "v210"), int(b == "v210")
        wp = 1 if vi and vo else int((fb if vi else fa).depth > 8)
        return f"k_yuv_stack_v210_vec<{wp},{vi},{vo},{fb.csy},{tri},{lds}>"
    return f"k_yuv_stack_pk_vec<{int(fa.depth > 8)},{int(fb.depth > 8)},{int(fa.nplanes == 1)},{int(fb.nplanes == 1)},{fb.csy},{tri},{lds}>"


def _split(a, b, stages, lds=None):
    """what a ragged width on rows the vector kernel can take reports"""
    return _vec(a, b, stages, lds) + "+" + _generic(a, b) + _list(stages)


def _kernel(a, b, w, h, stages, variant="auto", lds=None, nf=NF):
    """This module's own statement of the kernel a call on DENSE tensors runs, as `last_kernel` spells it: the vector kernel on
    whole units of aligned rows, the generic kernel elsewhere, both for a ragged width on rows the vector kernel can take."""
    fa, fb = yuv_side(a), yuv_side(b)
    gen = _generic(a, b)
    st = parse_stages(stages)
    vec = _vec(a, b, stages, lds)
    modes_ok = all(m in VEC_MODES for _, m in st if m)
    bh = 1 << fb.csy
    ch = -(-h // bh)
    if _kind(a, b) == "v210":
        vi, vo = int(a == "v210"), int(b == "v210")
        wp = 1 if vi and vo else int((fb if vi else fa).depth > 8)
        pxt, ok = 6, fb.csx == 1 and (vi and vo or wp or vi)
        bs = 2 if wp else 1
        planes = []
        if not vi:
            planes += [(w * 2, h, 4), (-(-w // 2) * 2, h, 2)]
        if not vo:
            planes += [(w * bs, h, 2 * bs), (-(-w // 2) * bs, ch, bs)]
        planes += [(128 * -(-w // 48), h, 16)] * (vi + vo)
    else:
        pi, po = int(fa.nplanes == 1), int(fb.nplanes == 1)
        win, wout = int(fa.depth > 8), int(fb.depth > 8)
        ok = (win == wout or (win and not wout)) and fb.csx == 1
        pxt = 8 if win and not wout else 4 if win else 8
        planes = []
        for is_dst, packed, wide in ((False, pi, win), (True, po, wout)):
            bs = 2 if wide else 1
            if packed:
                planes.append((4 * -(-w // 2) * bs, h, min(16, 2 * pxt * bs)))
            else:
                planes += [(w * bs, h, pxt * bs), (-(-w // 2) * bs, ch if is_dst else h, (pxt // 2) * bs)]
    if variant == "generic":
        return gen + _list(stages)
    rows_ok = ok and modes_ok and h % bh == 0 and all(_plane_fits(s, r, al, nf) for s, r, al in planes)
    if rows_ok and w % pxt == 0:
        return vec + _list(stages)
    if rows_ok and w > pxt:
        return vec + "+" + gen + _list(stages)
    return gen + _list(stages)


def _expect(res, a, b, stages, cdl, planar, w, key, dl=None, **kw):
    """the twin's planes for the planar samples of a source `a`, in the container of `b`"""
    fa, la = _lay(a)
    fb, lb = _lay(b)
    # (the twin's results are cached by key: two containers of one depth share layouts and lists, so the key carries the shape)
    return _held(_want(res, stages, cdl, fa.depth, dl or fa.depth, fb.depth, la, lb, planar, (key, tuple(planar[0].shape)), **kw), b, w)


def _planar(a, dist, w, h, k=1, nf=NF, **kw):
    fa, la = _lay(a)
    return _src(dist, w, h, fa.depth, la, k=k, nf=nf, **kw)


def _run(eng, a, b, stages, cdl, planar, w, **kw):
    got = eng.apply_yuv_stack_packed(worker.to_device(_held(planar, a, w), eng.device), pix_fmt=a, out_pix_fmt=b, stages=stages, cdl=cdl,
                                     width=w, **kw)
    return _np(got)


def _own(eng, a, b, stages, cdl, planar, **kw):
    """the engine's own apply_yuv_stack on the planar samples, as numpy planes"""
    fa, la = _lay(a)
    fb, lb = _lay(b)
    own = eng.apply_yuv_stack(_dev(planar, eng.device), pix_fmt=_fmt(fa.depth, la), out_pix_fmt=_fmt(fb.depth, lb), stages=stages, cdl=cdl, **kw)
    return _host(own, fb.depth)


# ------------------------------------------------------------------ 1. every name onto itself
@pytest.mark.gpu
@pytest.mark.parametrize("stages", ["lut1d,cdl,lut3d", "lut3d,cdl,lut3d2"])
@pytest.mark.parametrize("name", PACKED + ["v210"])
def test_every_name_onto_itself(loaded, grade, name, stages):
    """Uniform content through nearest / trilinear / tetrahedral on the vector kernel (named exactly) and all five modes on the
    generic one; natural content through tetrahedral on both; then the ragged and the odd shape on dense rows, where the kernel is
    this module's own routing rule (the split of a ragged width is pinned on padded rows below).  The twin has pyramid / prism on
    lattices that are fed codes: in `lut3d,cdl,lut3d2` the first lattice takes the five modes and the one behind the CDL stays
    tetrahedral for those two; in `lut1d,cdl,lut3d`, whose only lattice is behind the CDL, pyramid / prism are checked against the
    planar stack's own bits."""
    kinds = stages.split(",")
    behind_cdl = {k for i, k in enumerate(kinds) if i and kinds[i - 1] == "cdl"}
    (w, h), ragged, odd = SHAPES[_kind(name, name)]

    def with_mode(m):
        keep = behind_cdl if m in ("pyramid", "prism") and any(k.startswith("lut3d") and k not in behind_cdl for k in kinds) else set()
        return ",".join(f"{k}:{'tetrahedral' if k in keep else m}" if k.startswith("lut3d") else k for k in kinds)

    def expected(st, m, planar, ww, key):
        if m in ("pyramid", "prism") and any(k.startswith("lut3d") and k in behind_cdl and f"{k}:{m}" in st for k in kinds):
            # the only lattice of the list is fed unit floats: the contract's own right-hand side, the planar stack on the same samples
            own = _own(loaded, name, name, st, grade, planar)
            assert loaded.last_kernel == "k_yuv_stack_generic" + _list(st), loaded.last_kernel
            return _held(own, name, ww)
        return _expect(loaded._res, name, name, st, grade, planar, ww, ("packed", key))

    for dist, variant, modes in (("uniform", "auto", VEC_MODES), ("natural", "auto", ("tetrahedral",)),
                                 ("uniform", "generic", VEC_MODES + ("pyramid", "prism")), ("natural", "generic", ("tetrahedral",))):
        planar = _planar(name, dist, w, h)
        for m in modes:
            st = with_mode(m)
            with _variant(loaded, variant):
                got = _run(loaded, name, name, st, grade, planar, w)
                assert loaded.last_kernel == _kernel(name, name, w, h, st, variant), loaded.last_kernel
                assert "_vec<" in loaded.last_kernel if variant == "auto" else "_generic[" in loaded.last_kernel
            assert _same(got, expected(st, m, planar, w, dist)), (name, st, dist, variant)
    st = with_mode("tetrahedral")
    for ww, hh in (ragged, odd):
        planar = _planar(name, "natural", ww, hh, k=3)
        got = _run(loaded, name, name, st, grade, planar, ww)
        assert loaded.last_kernel == _kernel(name, name, ww, hh, st), loaded.last_kernel
        assert _same(got, expected(st, "tetrahedral", planar, ww, (ww, hh))), (name, ww, hh)
        with _variant(loaded, "generic"):                              # the odd shape on the generic kernel alone, whatever auto chose
            got = _run(loaded, name, name, st, grade, planar, ww)
            assert loaded.last_kernel == _generic(name, name) + _list(st), loaded.last_kernel
        assert _same(got, expected(st, "tetrahedral", planar, ww, (ww, hh))), (name, ww, hh, "generic")


# ------------------------------------------------------------------ 2. container and layout mixes
PAIRS = [("v210", "yuv422p10le"), ("v210", "yuv420p"), ("v210", "yuv444p10le"), ("yuv422p10le", "v210"), ("yuv422p", "v210"),
         ("uyvy422", "yuv420p"), ("y210le", "yuv422p10le"), ("yuv422p", "yuyv422"), ("y216le", "y216le"), ("yvyu422", "uyvy422")]


@pytest.mark.gpu
@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_container_and_layout_mixes(loaded, grade, a, b):
    """Each pair, at its vector, ragged and odd shape, against the twin and against the engine's own apply_yuv_stack on the
    de-interleaved samples.  A 4:4:4 destination and an 8-bit source written as 16-bit words have a generic kernel only; y216le has
    16-bit tables, which never fit LDS."""
    stages = "lut1d,cdl,lut3d"
    fa, fb = yuv_side(a), yuv_side(b)
    for i, (w, h) in enumerate(SHAPES[_kind(a, b)]):
        planar = _planar(a, "natural", w, h, k=2 + i)
        got = _run(loaded, a, b, stages, grade, planar, w)
        assert loaded.last_kernel == _kernel(a, b, w, h, stages), loaded.last_kernel
        if i == 0:
            if fb.csx == 0 or (fa.depth <= 8 and fb.depth > 8):
                assert loaded.last_kernel == _generic(a, b) + _list(stages), loaded.last_kernel
            else:
                assert "_vec<" in loaded.last_kernel and "+" not in loaded.last_kernel, loaded.last_kernel
            if a == "y216le":
                assert loaded.last_kernel == "k_yuv_stack_pk_vec<1,1,1,1,0,0,0>" + _list(stages), loaded.last_kernel
        assert _same(got, _expect(loaded._res, a, b, stages, grade, planar, w, ("mix", w, h))), (a, b, w, h)
        own = _own(loaded, a, b, stages, grade, planar)
        assert loaded.last_kernel.startswith("k_yuv_stack_"), loaded.last_kernel
        assert _same(got, _held(own, b, w)), (a, b, w, h, "differs from apply_yuv_stack on the planar samples")


@pytest.mark.gpu
def test_a_packed_side_and_a_v210_side_are_refused_by_name(loaded):
    """The mix the pass leaves out, before any GPU work."""
    buf = worker.to_device(_held(_planar("uyvy422", "natural", 48, 4), "uyvy422", 48), loaded.device)
    with pytest.raises(ValueError, match=r"a packed 4:2:2 side together with a v210 side is not supported with a stage stack on "
                                         r"packed 4:2:2 / v210 frames \(packed_stages\) \('uyvy422' -> 'v210'\)"):
        loaded.apply_yuv_stack_packed(buf, pix_fmt="uyvy422", out_pix_fmt="v210", stages="lut3d")


# ------------------------------------------------------------------ 3. tied to k_yuv_pk_vec / k_yuv_v210_vec
@pytest.mark.gpu
@pytest.mark.parametrize("a,b", [("uyvy422", "uyvy422"), ("y210le", "y210le"), ("yuyv422", "yuv420p"), ("yuv422p10le", "y212le"),
                                 ("v210", "v210"), ("v210", "yuv422p10le"), ("v210", "yuv420p"), ("yuv422p10le", "v210")])
def test_one_lattice_gives_the_bits_of_apply_yuv(loaded, a, b):
    w, h = SHAPES[_kind(a, b)][0]
    w = 96 if _kind(a, b) == "v210" else w                            # (whole units of k_yuv_v210_vec too: 12 or 24 samples a thread)
    held = worker.to_device(_held(_planar(a, "natural", w, h, k=3), a, w), loaded.device)
    got = _np(loaded.apply_yuv_stack_packed(held, pix_fmt=a, out_pix_fmt=b, stages=("lut3d",), width=w))
    family = "k_yuv_stack_v210_vec<" if _kind(a, b) == "v210" else "k_yuv_stack_pk_vec<"
    assert loaded.last_kernel.startswith(family), loaded.last_kernel
    ref = _np(loaded.apply_yuv(held, pix_fmt=a, out_pix_fmt=b, interp="tetrahedral", width=w))
    assert loaded.last_kernel.startswith("k_yuv_v210_vec<" if _kind(a, b) == "v210" else "k_yuv_pk_vec<"), loaded.last_kernel
    assert _same(got, ref), (a, b)


# ------------------------------------------------------------------ 4. junk bits and padding
def _padded(eng, want, fill, align=16):
    """a destination for the buffers `want` ([nf, rows, cols]) whose rows carry spare elements and whose frames a spare row, all
    `fill`, with rows still a multiple of `align` bytes: (the storage, the views the call takes)"""
    import torch
    store, views = [], []
    for p in want if isinstance(want, list) else [want]:
        dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[p.dtype.itemsize]
        pad = align // p.dtype.itemsize
        cols = -(-(p.shape[-1] + 1) // pad) * pad
        t = torch.full((p.shape[0], p.shape[1] + 1, cols), fill, dtype=dt, device=eng.device)
        store.append(t)
        views.append(t[:, :p.shape[1], :p.shape[2]])
    return store, views


def _padded_src(eng, held):
    """the source buffers `held` (numpy) on the device in rows of a whole number of 16 bytes: the views the call takes"""
    hl = held if isinstance(held, list) else [held]
    store, views = _padded(eng, hl, 0)
    for v, p in zip(views, hl):
        v.copy_(worker.to_device(p, eng.device))
    return views if isinstance(held, list) else views[0]


def _padded_name(a, b, w, stages, variant):
    """the kernel of a call on rows padded to 16 bytes, for a pair that has a vector kernel: that kernel, with the generic one for
    what is left of a ragged width"""
    fa, fb = yuv_side(a), yuv_side(b)
    if variant == "generic":
        return _generic(a, b) + _list(stages)
    pxt = 6 if _kind(a, b) == "v210" else 8 if fa.depth > 8 and fb.depth == 8 else 4 if fa.depth > 8 else 8
    return _vec(a, b, stages) + _list(stages) if w % pxt == 0 else _split(a, b, stages)


def _untouched(store, want, fill, used=None):
    """every element of the storage outside the buffers `want` (and, with `used`, past their first `used` columns) is `fill`"""
    for t, p in zip(store, want if isinstance(want, list) else [want]):
        n = p.shape[2] if used is None else used
        if not ((t[:, :, n:] == fill).all() and (t[:, p.shape[1]:] == fill).all()):
            return False
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "generic"])
def test_junk_bits_and_padding(loaded, grade, variant):
    """Low bits under the shift, bits 30-31 of a v210 word and slots beyond the frame are ignored on input and zero / replicated on
    output; row bytes past the last group, row padding and a spare row keep their sentinel.  Both sides sit in rows padded to 16
    bytes, so the ragged and the odd width run the vector kernel up to the last whole unit and the generic kernel for the rest."""
    stages = "lut1d,cdl,lut3d"
    rng = np.random.default_rng(11)
    with _variant(loaded, variant):
        # y210le: random low six bits, at the vector, the ragged and the odd shape (whose last group's second luma slot is junk too)
        for w, h in SHAPES["pk"]:
            for a, b in (("y210le", "y210le"), ("y212le", "yuv422p12le")):
                fa = yuv_side(a)
                planar = _planar(a, "natural", w, h, k=4)
                clean = _held(planar, a, w)
                dirty = clean | rng.integers(0, 1 << fa.shift, size=clean.shape).astype(np.uint16)
                if w % 2:
                    slot = dirty.reshape(dirty.shape[:-1] + (-1, 4))[..., -1, 2]
                    slot[...] = rng.integers(0, 1 << 16, size=slot.shape).astype(np.uint16)
                assert (dirty != clean).any()
                want = _expect(loaded._res, a, b, stages, grade, planar, w, ("junk", w, h))
                fill = 0x5a5a
                store, views = _padded(loaded, want, fill)
                dst = views if isinstance(want, list) else views[0]
                loaded.apply_yuv_stack_packed(_padded_src(loaded, dirty), dst, pix_fmt=a, out_pix_fmt=b, stages=stages, cdl=grade, width=w)
                assert loaded.last_kernel == _padded_name(a, b, w, stages, variant), loaded.last_kernel
                got = _np(list(views)) if isinstance(want, list) else _np(views[0])
                assert _same(got, want), (a, b, w, h, variant)
                if not isinstance(want, list):
                    assert ((got & ((1 << yuv_side(b).shift) - 1)) == 0).all(), (a, b, "low bits set on output")
                assert _untouched(store, want, fill), (a, b, w, h, variant, "wrote outside the buffers")
        # v210: random bits 30-31 everywhere, random codes in every slot beyond the frame and in the words past the last group
        for w, h in SHAPES["v210"]:
            for a, b in (("v210", "v210"), ("v210", "yuv422p10le"), ("yuv422p10le", "v210")):
                planar = _planar(a, "natural", w, h, k=4)
                src = _held(planar, a, w)
                if a == "v210":
                    g = -(-w // 6)
                    slots, stride = (6 * g, 3 * g, 3 * g), src.shape[-1] * 4
                    junk = v210.to_v210([rng.integers(0, 1024, size=p.shape[:-1] + (n,)).astype(np.uint16)
                                         for p, n in zip(planar, slots)], 6 * g, stride=stride)
                    # the mask of the slots inside the frame: whole rows of groups with ones in the frame's own samples
                    ones = [np.zeros(p.shape[:-1] + (n,), np.uint16) for p, n in zip(planar, slots)]
                    for o, n in zip(ones, (w, (w + 1) // 2, (w + 1) // 2)):
                        o[..., :n] = 1023
                    mask = v210.to_v210(ones, 6 * g, stride=stride)
                    dirty = (src & mask) | (junk & ~mask & np.uint32(0x3fffffff))
                    dirty[..., 4 * g:] = rng.integers(0, 1 << 32, size=dirty[..., 4 * g:].shape, dtype=np.uint64).astype(np.uint32)
                    dirty |= rng.integers(0, 4, size=dirty.shape).astype(np.uint32) << np.uint32(30)
                    assert (dirty != src).any() and all(np.array_equal(x, y) for x, y in zip(v210.to_planar(dirty, w), planar))
                else:
                    dirty = src
                want = _expect(loaded._res, a, b, stages, grade, planar, w, ("junk210", w, h))
                fill = 0x5a5a5a5a if b == "v210" else 0x5a5a
                store, views = _padded(loaded, want, fill)
                dst = views if isinstance(want, list) else views[0]
                loaded.apply_yuv_stack_packed(_padded_src(loaded, dirty), dst, pix_fmt=a, out_pix_fmt=b, stages=stages, cdl=grade, width=w)
                assert loaded.last_kernel == _padded_name(a, b, w, stages, variant), loaded.last_kernel
                got = _np(list(views)) if isinstance(want, list) else _np(views[0])
                if b == "v210":
                    g4 = 4 * (-(-w // 6))
                    assert np.array_equal(got[..., :g4], want[..., :g4]), (a, b, w, h, variant)
                    assert (got[..., :g4] >> np.uint32(30) == 0).all(), "bits 30-31 set on output"
                    assert _untouched(store, want, fill, used=g4), (a, b, w, h, variant, "wrote past the last group")
                else:
                    assert _same(got, want), (a, b, w, h, variant)
                    assert _untouched(store, want, fill), (a, b, w, h, variant, "wrote outside the planes")


# ------------------------------------------------------------------ 5. row blocks
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "generic"])
def test_row_blocks_write_their_rows_only(loaded, grade, variant):
    import torch
    stages = "lut3d,cdl,lut3d2"
    for a, b, w, h in (("v210", "v210", 48, 12), ("uyvy422", "yuv420p", 64, 12), ("v210", "yuv420p10le", 48, 12)):
        fb = yuv_side(b)
        planar = _planar(a, "uniform", w, h, k=5)
        src = worker.to_device(_held(planar, a, w), loaded.device)
        whole = _expect(loaded._res, a, b, stages, grade, planar, w, ("rows", w, h))
        names = dict(pix_fmt=a, out_pix_fmt=b, stages=stages, cdl=grade, width=w)
        fill = 0x5a5a5a5a if b == "v210" else 0x5a5a if fb.depth > 8 else 0x5a
        wl = whole if isinstance(whole, list) else [whole]
        with _variant(loaded, variant):
            out = [torch.full(p.shape, fill, dtype={1: torch.uint8, 2: torch.int16, 4: torch.int32}[p.dtype.itemsize],
                              device=loaded.device) for p in wl]
            dst = out if isinstance(whole, list) else out[0]
            loaded.apply_yuv_stack_packed(src, dst, row0=4, rows=6, **names)
            used = 4 * (-(-w // 6)) if b == "v210" else None
            for i, (g, wh) in enumerate(zip([_np(t) for t in out], wl)):
                r0, r1 = (4, 10) if i == 0 or fb.csy == 0 else (2, 5)
                assert np.array_equal(g[:, r0:r1, :used], wh[:, r0:r1, :used]), (a, b, variant, i)
                assert (g[:, :r0] == fill).all() and (g[:, r1:] == fill).all(), (a, b, variant, i, "wrote outside the block")
            loaded.apply_yuv_stack_packed(src, dst, row0=0, rows=4, **names)
            loaded.apply_yuv_stack_packed(src, dst, row0=10, rows=h - 10, **names)
            assert all(np.array_equal(g[..., :used], wh[..., :used]) for g, wh in zip([_np(t) for t in out], wl)), (a, b, variant)
            if fb.csy:
                with pytest.raises(_native.LutrError, match="union") as e:
                    loaded.apply_yuv_stack_packed(src, dst, row0=1, rows=h - 1, **names)
                assert e.value.code == _native.EINVAL


# ------------------------------------------------------------------ 6. the full-range prologue
@pytest.mark.gpu
def test_full_range_prologue(loaded, grade):
    stages = "lut1d,cdl,lut3d"
    w, h = SHAPES["pk"][0]
    planar = _planar("uyvy422", "natural", w, h, k=6, full_range=True)
    got = _run(loaded, "uyvy422", "uyvy422", stages, grade, planar, w, range_src="pc", range_in="tv", lut_depth=8)
    assert loaded.last_kernel == _kernel("uyvy422", "uyvy422", w, h, stages), loaded.last_kernel
    assert _same(got, _expect(loaded._res, "uyvy422", "uyvy422", stages, grade, planar, w, "pc", dl=8, rin="tv", prologue=True))
    # v210 through the 8-bit LUT depth: the planar stack's own bits on the same samples, in the container
    w, h = SHAPES["v210"][0]
    planar = _planar("v210", "natural", w, h, k=6, full_range=True)
    kw = dict(range_src="pc", range_in="tv", lut_depth=8)
    for b in ("v210", "yuv422p"):
        got = _run(loaded, "v210", b, stages, grade, planar, w, **kw)
        assert loaded.last_kernel == _kernel("v210", b, w, h, stages, lds=_lds(stages, 8)), loaded.last_kernel
        assert _same(got, _held(_own(loaded, "v210", b, stages, grade, planar, **kw), b, w)), b


# ------------------------------------------------------------------ 7. table placement and grid-stride trips, in child processes
def _child(tmp, luts, ids, **env_add):
    env = {k: v for k, v in os.environ.items() if k not in ("LUTR_STACK_LDS", "LUTR_MAX_BLOCKS", "LUTR_DEBUG")}
    env.update(env_add)
    t0 = time.monotonic()
    try:
        p = subprocess.run([sys.executable, str(ROOT / "tests" / "_gpu_stack_packed_worker.py"), str(tmp), str(luts["log709_33"][0]),
                            str(GOLDEN / "lut1d" / "gamma1024.cube"), str(GOLDEN / "cdl" / "shot.cc")] + list(ids), env=env, cwd=str(ROOT),
                           capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the child ({env_add}) did not finish within {CHILD_LIMIT_S} s", pytrace=False)
    if p.returncode != 0:
        pytest.fail(f"the child ({env_add}) ended with {p.returncode} after {time.monotonic() - t0:.1f} s:\n{p.stderr[-3000:]}",
                    pytrace=False)
    debug, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"\[case (\S+)\]", line)
        if m:
            cur = m.group(1)
            debug[cur] = []
        elif cur and line.startswith("[lutr gs] "):
            debug[cur].append(line)
    out = {}
    for cid in ids:
        with np.load(tmp / f"{cid}.npz") as z:
            planes, kernel = [z[f"p{i}"] for i in range(len(z.files) - 1)], str(z["kernel"])
        planes = [p.view(np.uint16) if p.dtype == np.int16 else p.view(np.uint32) if p.dtype == np.int32 else p for p in planes]
        out[cid] = dict(planes=planes, kernel=kernel, debug=debug.get(cid, []))
    return out


def _child_want(res, grade, cid):
    a, b, w, h, nf = worker.CASES[cid]
    planar, _ = worker.source(a, w, h, nf)
    want = _expect(res, a, b, worker.STAGES, grade, planar, w, ("child", cid))
    return want if isinstance(want, list) else [want]


def _units(cid, kernel):
    """this module's own count of the units of the launch that carries the case's regime"""
    a, b, w, h, nf = worker.CASES[cid]
    fa, fb = yuv_side(a), yuv_side(b)
    if "_generic" in kernel:
        return -(-w // (6 if _kind(a, b) == "v210" else 2)) * -(-h // (1 << fb.csy)) * nf
    if _kind(a, b) == "v210":
        return (w // 6) * (h >> fb.csy) * nf
    pxt = 8 if fa.depth > 8 and fb.depth == 8 else (4 if fa.depth > 8 else 8)
    return (w // pxt) * (h >> fb.csy) * nf


@pytest.mark.gpu
def test_tables_in_global_memory_and_capped_grids_give_the_same_bits(loaded, luts, grade, tmp_path):
    """Two fresh children, one after the other, each under its own time limit; the second starts only if the first exited 0.
    LUTR_STACK_LDS=0: the tables read from global memory.  LUTR_MAX_BLOCKS=2 on six frames: every thread makes three trips or
    more, the last partial, consecutive trips in different frames; the `[lutr gs]` line is checked against the unit formula."""
    ids = list(worker.CASES)
    (tmp_path / "lds").mkdir()
    (tmp_path / "cap").mkdir()
    res = _child(tmp_path / "lds", luts, ids[:4], LUTR_STACK_LDS="0")
    for cid in ids[:4]:
        a, b, w, h, nf = worker.CASES[cid]
        assert res[cid]["kernel"] == _kernel(a, b, w, h, worker.STAGES, lds=False, nf=nf), res[cid]["kernel"]
        assert res[cid]["kernel"].endswith(",0>" + _list(worker.STAGES)), res[cid]["kernel"]
        assert _same(res[cid]["planes"], _child_want(loaded._res, grade, cid)), (cid, "LUTR_STACK_LDS=0")
    res = _child(tmp_path / "cap", luts, ids, LUTR_MAX_BLOCKS="2", LUTR_DEBUG="1")
    for cid in ids:
        a, b, w, h, nf = worker.CASES[cid]
        kernel = res[cid]["kernel"]
        small = cid.endswith("_small")
        assert kernel == _kernel(a, b, w, h, worker.STAGES, nf=nf), kernel
        assert kernel.startswith(_generic(a, b) + "[") if small else "_vec<" in kernel and "+" not in kernel, kernel
        family = kernel.split("[")[0].split("<")[0]
        lines = [re.fullmatch(r"\[lutr gs\] (\S+) units (\d+) blocks (\d+)", ln) for ln in res[cid]["debug"]]
        mine = [m for m in lines if m and m.group(1) == family]
        assert len(mine) == 1, res[cid]["debug"]
        units, blocks = int(mine[0].group(2)), int(mine[0].group(3))
        assert units == _units(cid, kernel) and blocks == 2, (cid, units, blocks)
        assert -(-units // 512) >= 3 and units % 512 != 0 and (units // nf) % 512 != 0, (cid, units)
        assert _same(res[cid]["planes"], _child_want(loaded._res, grade, cid)), (cid, "LUTR_MAX_BLOCKS=2")


# ------------------------------------------------------------------ 8. the ABI's refusals
def _abi(engine, entry, stages, cdl, fmt_in, fmt_out, sides, w, h, s, d):
    """lutr_apply_yuv_stack_packed (`sides`: two raw packings, None: a null pointer) or lutr_apply_yuv_stack_v210 (`sides`: two
    ints) with raw (kind, interp) pairs; returns (rc, message)."""
    p = _native.YuvParams(fmt_in, fmt_out, 10, 0, 0, 0, 0, 0)
    arr = (_native.StageStruct * max(len(stages), 1))()
    for i, (kind, interp) in enumerate(stages):
        arr[i].kind, arr[i].interp = kind, interp
    k = None if cdl is None else C.byref(_native.cdl_struct(cdl))
    if entry == "packed":
        sides = [None if y is None else C.byref(_native.YuvPacking(*y)) for y in sides]
        call = engine._lib.lutr_apply_yuv_stack_packed
    else:
        call = engine._lib.lutr_apply_yuv_stack_v210
    with engine._lock:
        engine._bind_stream()
        rc = call(engine._ctx, C.byref(p), arr, len(stages), k, *sides, w, h, 1, C.byref(s), C.byref(d), 0, h)
    return rc, engine._lib.lutr_last_error().decode()


@pytest.mark.gpu
def test_refusals_at_the_abi_leave_the_destination_untouched(loaded, grade):
    import torch
    w, h = 64, 8
    planar = _planar("y210le", "natural", w, h, nf=1)
    src = worker.to_device(_held(planar, "y210le", w), loaded.device)
    out = torch.full_like(src, 0x5a5a)
    s, d = _desc([src]), _desc([out])
    f422, f420, f444 = _native.fmt_code(10, 1, 0), _native.fmt_code(10, 1, 1), _native.fmt_code(10, 0, 0)
    pk = (1, 0, 6)
    L3, L1, CD, MX = 1, 3, 4, 5
    ok = [(L3, 2)]
    for args, message in (
            ((ok, None, f422, f422, (None, pk)), "stack: null packing"),
            ((ok, None, f422, f422, (pk, None)), "stack: null packing"),
            ((ok, None, f422, f422, (pk, (1, 0, 4))), "destination packing: shift is 6 (16 - depth) or 0 at 10 bit, not 4"),
            ((ok, None, f422, f422, ((1, 3, 6), pk)), "source packing: order is 0 (yuyv), 1 (uyvy) or 2 (yvyu), not 3"),
            ((ok, None, f422, f420, (pk, pk)), "destination packing: packed frames are 4:2:2"),
            ((ok, None, f420, f422, (pk, pk)), "a packed destination takes a 4:2:2 source (no subsampling change into a packed frame)"),
            ((ok, None, f444, f422, (pk, (0, 0, 0))), "the source of a packed call is 4:2:2"),
            (([(MX, 0), (L3, 2)], None, f422, f422, (pk, pk)),
             "stack: stage 0 is a matrix stage; a matrix is lutr_apply_yuv_stack_matrix's, and a strength or a matte together with a "
             "matrix is not supported")):
        rc, msg = _abi(loaded, "packed", *args, w, h, s, d)
        assert rc == _native.EINVAL and msg == message, (args, msg)
    with _variant(loaded, "vec_lds"):
        rc, msg = _abi(loaded, "packed", ok, None, f422, f422, (pk, pk), w, h, s, d)
        assert rc == _native.EINVAL and msg == "variant vec_lds: there is no LDS-window kernel for the stack pass", msg
    # the destination begins inside the source buffer
    big = torch.zeros(2 * src.numel(), dtype=torch.int16, device=loaded.device)
    inside = big[:src.numel()].view(src.shape)
    inside.copy_(src)
    over = big[src.numel() - 4:2 * src.numel() - 4].view(src.shape)
    rc, msg = _abi(loaded, "packed", ok, None, f422, f422, (pk, pk), w, h, _desc([inside]), _desc([over]))
    assert rc == _native.EINVAL and msg.startswith("the stack pass cannot run in place: the byte range of source plane 0 overlaps that "
                                                    "of destination plane 0"), msg
    with pytest.raises(ValueError, match="stack pass cannot run in place"):
        loaded.apply_yuv_stack_packed(src, src, pix_fmt="y210le", stages="lut3d")
    # the v210 entry
    w2, h2 = 48, 4
    vplanar = _planar("v210", "natural", w2, h2, nf=1)
    vsrc = worker.to_device(_held(vplanar, "v210", w2), loaded.device)
    vout = torch.full_like(vsrc, 0x5a5a5a5a)
    vs, vd = _desc([vsrc]), _desc([vout])
    p48 = _desc(_dev(_planar("yuv422p10le", "natural", w2, h2, nf=1), loaded.device))   # (4:2:2 planes: they hold a 4:2:0 frame too)
    for args, message in (
            ((ok, None, f422, f422, (2, 1)), "in_v210 and out_v210 are 0 or 1 (got 2, 1)"),
            ((ok, None, _native.fmt_code(12, 1, 0), f422, (1, 1)), "source: a v210 frame is 10-bit 4:2:2 (format 0x%x)" % _native.fmt_code(12, 1, 0)),
            (([(MX, 0)], None, f422, f422, (1, 1)),
             "stack: stage 0 is a matrix stage; a matrix is lutr_apply_yuv_stack_matrix's, and a strength or a matte together with a "
             "matrix is not supported")):
        rc, msg = _abi(loaded, "v210", *args, w2, h2, vs, vd)
        assert rc == _native.EINVAL and msg == message, (args, msg)
    rc, msg = _abi(loaded, "v210", ok, None, f420, f422, (0, 1), w2, h2, p48, vd)
    assert rc == _native.EINVAL and msg == "a v210 destination takes a 4:2:2 source (no subsampling change into a v210 frame)", msg
    with _variant(loaded, "vec_lds"):
        rc, msg = _abi(loaded, "v210", ok, None, f422, f422, (1, 1), w2, h2, vs, vd)
        assert rc == _native.EINVAL and msg == "variant vec_lds: there is no LDS-window kernel for the stack pass", msg
    rc, msg = _abi(loaded, "v210", ok, None, f422, f422, (1, 1), w2, h2, vs, vs)
    assert rc == _native.EINVAL and msg.startswith("the stack pass cannot run in place"), msg
    torch.cuda.synchronize()
    assert (out == 0x5a5a).all() and (vout == 0x5a5a5a5a).all(), "a refused call wrote to a destination"
    # both sides planar: lutr_apply_yuv_stack itself, from either entry
    pdev = _dev(planar, loaded.device)
    full = [(L1, 0), (CD, 0), (L3, 2)]
    for entry, sides in (("packed", ((0, 0, 0), (0, 0, 0))), ("v210", (0, 0))):
        pout = [torch.full_like(t, 0x5a5a) for t in pdev]
        rc, msg = _abi(loaded, entry, full, grade, f422, f422, sides, w, h, _desc(pdev), _desc(pout))
        assert rc == 0, msg
        assert loaded.last_kernel == "k_yuv_stack_vec<1,1,1,0,1,0,0,1>[lut1d,cdl,lut3d:2]", loaded.last_kernel
        assert _same(_host(pout, 10), _want(loaded._res, "lut1d,cdl,lut3d", grade, 10, 10, 10, "422", "422", planar, ("abi-planar", 64, 8)))
    rc, msg = _abi(loaded, "packed", full, grade, f422, f422, (pk, pk), w, h, s, d)
    assert rc == 0, msg
    assert loaded.last_kernel == "k_yuv_stack_pk_vec<1,1,1,1,0,0,1>[lut1d,cdl,lut3d:2]", loaded.last_kernel
    assert _same(_np(out), _expect(loaded._res, "y210le", "y210le", "lut1d,cdl,lut3d", grade, planar, w, "abi"))
    rc, msg = _abi(loaded, "v210", full, grade, f422, f422, (1, 1), w2, h2, vs, vd)
    assert rc == 0, msg
    assert loaded.last_kernel == "k_yuv_stack_v210_vec<1,1,1,0,0,1>[lut1d,cdl,lut3d:2]", loaded.last_kernel
    assert _same(_np(vout), _expect(loaded._res, "v210", "v210", "lut1d,cdl,lut3d", grade, vplanar, w2, "abi-v210"))


# ------------------------------------------------------------------ 9. the group
@pytest.mark.gpu
def test_group_shards_equal_the_single_engine_call(loaded, luts, l1ds, grade, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    stages = "lut1d,cdl,lut3d,lut3d2"
    for (w, h), a, b in (((48, 4), "v210", "v210"), ((64, 8), "uyvy422", "yuv420p"), ((50, 6), "v210", "yuv420p10le"),
                         ((33, 5), "yuv422p", "yuyv422")):
        fb = yuv_side(b)
        planar = _planar(a, "natural", w, h, k=9)
        single = _run(loaded, a, b, stages, grade, planar, w)
        with LutEngineGroup([0, 0]) as g:
            assert g.treat_as_remote
            g.set_lut(luts["log709_33"][1])
            g.set_lut2(luts["random_9"][1])
            g.set_lut1d(l1ds["gamma1024"], "cubic")
            got = g.apply_yuv_stack_packed(worker.to_device(_held(planar, a, w), loaded.device), pix_fmt=a, out_pix_fmt=b, stages=stages,
                                           cdl=grade, width=w)
            assert g.last_remote == 1 and all(r0 % (1 << fb.csy) == 0 for r0, _ in g.last_blocks), g.last_blocks
            assert all(k.startswith("k_yuv_stack_pk_") or k.startswith("k_yuv_stack_v210_") for k in g.last_kernels), g.last_kernels
            assert _same(_np(got), single), (w, h, a, b)
        assert _same(single, _expect(loaded._res, a, b, stages, grade, planar, w, ("group", w, h))), (w, h, a, b)
