"""A matte plane on the stage stack on the GPU: lutr_apply_yuv_stack_matte bit-exact, whole planes, against
tests/_matte_twin.py fed the product's own host tables, and against the strength calls where the matte is constant.  The base
size is tests/test_gpu_stack.py's: 136 x 36 -- at 8 samples per thread two full workgroups and a partial one.

The matte of every case is seeded noise with a hard-edged rectangle of Mm and one of 0 whose corners sit at odd x and y -- the
samples differ inside every kind of chroma block -- and moves from frame to frame: a sample read at the wrong row, column or
frame, or weighted behind the chroma mean, changes the planes."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, frames
from lut_renderer_amd.formats import parse_stages
from tests import _matte_twin as twin
from tests.test_gpu_stack import (LAYOUTS, H, W, _desc, _dev, _eq, _fmt, _host, _lds, _list, _src, _variant,  # noqa: F401
                                  _vec_name, grade, l1ds, loaded, luts)

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
MATTE_GENERIC = "k_yuv_stack_matte_generic"
STAGES = "lut1d,cdl,lut3d"
NAMES = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
_refs = {}           # mattes and expected planes, computed once per case and shared (never written to)


def _matte_name(din, dout, dm, a, b, stages, lds):
    head = f"k_yuv_stack_vec<{int(din > 8)},{int(dout > 8)},"
    return _vec_name(din, dout, a, b, stages, lds).replace(head, f"k_yuv_stack_matte_vec<{int(din > 8)},{int(dout > 8)},{int(dm > 8)},", 1)


def _matte(w, h, depth, nf=None, seed=0):
    """[h, w] (nf None) or [nf, h, w] codes of `depth` bits, uint8 at 8 bit, else uint16: noise, a rectangle of Mm and one of 0
    with odd corners, moved by two samples a frame."""
    rk = ("matte", w, h, depth, nf, seed)
    if rk not in _refs:
        mm = (1 << depth) - 1
        rng = np.random.default_rng(977 * depth + seed)
        out = []
        for f in range(nf or 1):
            m = rng.integers(0, mm + 1, size=(h, w))
            x0, x1, y0, y1 = 3 + 2 * f, (w // 2) | 1, 1 + 2 * f, (h // 2) | 1
            m[y0:y1, x0:x1] = mm
            m[y1:h - 3, x1 + 2 * f:w - 5] = 0
            out.append(m.astype(np.uint8 if depth == 8 else np.uint16))
        _refs[rk] = out[0] if nf is None else np.stack(out)
    return _refs[rk]


def _mdev(m, device):
    return _dev([m], device)[0]


def _want(res, stages, cdl, strength, matte, dm, invert, din, dl, dout, a, b, src, key):
    """The twin's planes for `src` and `matte` with the resources `res` (the `loaded` fixture's) and the product's own tables."""
    st = parse_stages(stages)
    rk = (id(res["lut"]), id(res["lut2"]), id(res["l1"][0]), res["l1"][1], st, None if cdl is None else (cdl.sop_text(), cdl.saturation),
          np.asarray(strength, dtype=np.float32).tobytes(), hash(np.ascontiguousarray(matte).tobytes()), matte.shape, dm, invert, din,
          dl, dout, a, b, key)
    if rk not in _refs:
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        k = twin.consts("bt709", "tv", "bt709", "tv", din, dl, dout, ocsx, ocsy)
        kinds = [s for s, _ in st]
        _refs[rk] = twin.apply(st, strength, matte, dm, invert, k, dl, dout, icsx, icsy, ocsx, ocsy, src, lut=res["lut"],
                               lut2=res["lut2"], prelut=res["prelut"], cdl=cdl,
                               l1d_tab=_native.lut1d_table(*res["l1"], dl) if "lut1d" in kinds else None,
                               cdl_tab=_native.cdl_table(cdl, dl) if "cdl" in kinds else None)
    return _refs[rk]


# ------------------------------------------------------------------ 1: layouts
@pytest.mark.gpu
@pytest.mark.parametrize("a", list(LAYOUTS))
@pytest.mark.parametrize("b", list(LAYOUTS))
def test_all_nine_layout_pairs_at_10_bit_with_a_10_bit_matte(loaded, grade, a, b):
    src = _src("natural", W, H, 10, a, nf=2)
    m = _matte(W, H, 10, nf=2)
    got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), stages=STAGES, cdl=grade,
                                 strength=0.8, matte=_mdev(m, loaded.device), matte_depth=10)
    assert loaded.last_kernel == _matte_name(10, 10, 10, a, b, STAGES, True), loaded.last_kernel
    assert _eq(_host(got, 10), _want(loaded._res, STAGES, grade, 0.8, m, 10, False, 10, 10, 10, a, b, src, "nine"))


# ------------------------------------------------------------------ 2: container triples
@pytest.mark.gpu
@pytest.mark.parametrize("din,dout,dm", [(8, 8, 8), (16, 16, 8), (16, 16, 10), (16, 16, 16), (16, 8, 8), (16, 8, 12), (8, 8, 16), (8, 16, 8)],
                         ids=lambda v: str(v))
def test_container_triples_on_420_to_422(loaded, grade, din, dout, dm):
    src = _src("uniform", W, H, din, "420", nf=2)
    m = _matte(W, H, dm, nf=2)
    got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(din, "420"), out_pix_fmt=_fmt(dout, "422"), stages=STAGES,
                                 cdl=grade, matte=_mdev(m, loaded.device), matte_depth=dm, matte_invert=dm == 12)
    # no vector kernel: an 8-bit source written as 16-bit words, and 16-bit matte words beside an 8-bit source
    generic = (din == 8 and dout > 8) or (din == 8 and dm > 8)
    name = MATTE_GENERIC + _list(STAGES) if generic else _matte_name(din, dout, dm, "420", "422", STAGES, _lds(STAGES, din))
    assert loaded.last_kernel == name, loaded.last_kernel
    assert _eq(_host(got, dout), _want(loaded._res, STAGES, grade, 1.0, m, dm, dm == 12, din, din, dout, "420", "422", src, "mix"))


# ------------------------------------------------------------------ 3: a trilinear stage
@pytest.mark.gpu
def test_a_trilinear_stage(loaded):
    stages = "lut3d:trilinear,lut3d2"
    src = _src("natural", W, H, 10, "420", nf=2)
    m = _matte(W, H, 8, nf=2)
    got = loaded.apply_yuv_stack(_dev(src, loaded.device), stages=stages, strength=0.9, matte=_mdev(m, loaded.device), **NAMES)
    assert loaded.last_kernel == _matte_name(10, 10, 8, "420", "422", stages, False) and ",1,0>" in loaded.last_kernel, loaded.last_kernel
    assert _eq(_host(got, 10), _want(loaded._res, stages, None, 0.9, m, 8, False, 10, 10, 10, "420", "422", src, "tri"))


# ------------------------------------------------------------------ 4: the identities
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "generic"])
def test_constant_mattes_are_the_strength_calls(loaded, grade, variant):
    import torch
    src = _src("natural", W, H, 10, "420", nf=2)
    dev = _dev(src, loaded.device)
    kw = dict(stages=STAGES, cdl=grade, **NAMES)
    full = lambda v, dt: torch.full((H, W), v, dtype=dt, device=loaded.device)                    # noqa: E731
    want = MATTE_GENERIC + _list(STAGES) if variant == "generic" else _matte_name(10, 10, 10, "420", "422", STAGES, True)
    with _variant(loaded, variant):
        mixed = _host(loaded.apply_yuv_stack(dev, strength=0.37, **kw), 10)
        zero = _host(loaded.apply_yuv_stack(dev, strength=0.0, **kw), 10)
        assert "_mix_" in loaded.last_kernel
        got = {}
        got["Mm"] = loaded.apply_yuv_stack(dev, strength=0.37, matte=full(1023, torch.int16), matte_depth=10, **kw)
        assert loaded.last_kernel == want, loaded.last_kernel          # the matte kernels with a constant matte as well
        got["0"] = loaded.apply_yuv_stack(dev, strength=0.37, matte=full(0, torch.int16), matte_depth=10, **kw)
        got["inv0"] = loaded.apply_yuv_stack(dev, strength=0.37, matte=full(0, torch.int16), matte_depth=10, matte_invert=True, **kw)
        got["above"] = loaded.apply_yuv_stack(dev, strength=0.37, matte=full(-1, torch.int16), matte_depth=10, **kw)   # 0xffff
        got["invabove"] = loaded.apply_yuv_stack(dev, strength=0.37, matte=full(-1, torch.int16), matte_depth=10, matte_invert=True, **kw)
        assert loaded.last_kernel == want, loaded.last_kernel
        got = {k: _host(v, 10) for k, v in got.items()}
    assert not _eq(mixed, zero)
    assert _eq(got["Mm"], mixed) and _eq(got["inv0"], mixed) and _eq(got["above"], mixed)
    assert _eq(got["0"], zero) and _eq(got["invabove"], zero)


# ------------------------------------------------------------------ 5: frames, shards, a group
@pytest.mark.gpu
@pytest.mark.parametrize("still", [False, True], ids=["per_frame", "still"])
def test_four_frames_whole_in_shards_and_on_a_group(loaded, luts, l1ds, grade, monkeypatch, still):
    import torch
    from lut_renderer_amd.multigpu import LutEngineGroup
    s = [0.0, 1.0, 0.37, 0.5]
    src = _src("natural", W, H, 10, "420", nf=4)
    dev = _dev(src, loaded.device)
    m = _matte(W, H, 10, seed=5) if still else _matte(W, H, 10, nf=4)
    md = _mdev(m, loaded.device)
    kw = dict(stages=STAGES, cdl=grade, strength=s, matte=md, matte_depth=10, **NAMES)
    want = _want(loaded._res, STAGES, grade, s, m, 10, False, 10, 10, 10, "420", "422", src, "frames")
    got = _host(loaded.apply_yuv_stack(dev, **kw), 10)
    assert loaded.last_kernel == _matte_name(10, 10, 10, "420", "422", STAGES, True)
    assert _eq(got, want)
    if still:                                                    # [1, H, W] is the same still
        assert _eq(_host(loaded.apply_yuv_stack(dev, **dict(kw, matte=md[None])), 10), want)
    # two row shards, on both kernels: a matte row taken from the shard's first row would move the matte
    for variant in ("auto", "generic"):
        with _variant(loaded, variant):
            out = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=loaded.device) for p in want]
            loaded.apply_yuv_stack(dev, out, row0=20, rows=H - 20, **kw)
            assert "k_yuv_stack_matte_" in loaded.last_kernel
            assert (out[0][:, :20] == 0x5a5a).all() and (out[1][:, :10] == 0x5a5a).all(), "wrote outside the shard"
            loaded.apply_yuv_stack(dev, out, row0=0, rows=20, **kw)
            assert (out[0][:, 20:].cpu().numpy().view(np.uint16) == want[0][:, 20:]).all(), "wrote outside the shard"
        assert _eq(_host(out, 10), want), variant
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    with LutEngineGroup([0, 0]) as g:
        g.set_lut(luts["log709_33"][1])
        g.set_lut1d(l1ds["gamma1024"], "cubic")
        got = g.apply_yuv_stack(dev, **kw)
        assert g.last_remote == 1 and all(k.startswith("k_yuv_stack_matte_") for k in g.last_kernels), g.last_kernels
        assert _eq(_host(got, 10), want)
    with pytest.raises(ValueError, match="matte has 3 frames for 4 frames"):
        loaded.apply_yuv_stack(dev, **dict(kw, matte=_mdev(_matte(W, H, 10, nf=4)[:3], loaded.device)))


# ------------------------------------------------------------------ 6: odd shapes and alignment
@pytest.mark.gpu
def test_a_ragged_width_tiny_frames_strides_and_the_generic_modes(loaded, grade):
    import torch
    pad = 160
    src = _src("natural", 134, H, 10, "420", k=4)
    m = _matte(134, H, 10, seed=2)
    sp = [torch.zeros((p.shape[0], pad), dtype=torch.int16, device=loaded.device) for p in list(src) + [m]]
    for t, p in zip(sp, _dev(list(src) + [m], loaded.device)):
        t[:, :p.shape[1]] = p
    src_v = [t[:, :p.shape[1]] for t, p in zip(sp, src)]
    oshape = [(H, 134)] + [frames.chroma_shape(134, H, 1, 0)] * 2
    dp = [torch.full((s[0], pad), -1, dtype=torch.int16, device=loaded.device) for s in oshape]
    dst_v = [t[:, :s[1]] for t, s in zip(dp, oshape)]
    loaded.apply_yuv_stack(src_v, dst_v, stages=STAGES, cdl=grade, strength=0.8, matte=sp[3][:, :134], matte_depth=10, **NAMES)
    assert loaded.last_kernel == _matte_name(10, 10, 10, "420", "422", STAGES, True).replace("[", "+" + MATTE_GENERIC + "[", 1), loaded.last_kernel
    assert _eq(_host(dst_v, 10), _want(loaded._res, STAGES, grade, 0.8, m, 10, False, 10, 10, 10, "420", "422", src, "ragged"))
    assert all((t[:, s[1]:] == -1).all() for t, s in zip(dp, oshape)), "wrote past the row"
    # 6 x 2 and an odd 7 x 3: the edge-pixel rule of the generic kernel, the matte read at the clamped position
    for (w, h), a, b in (((6, 2), "420", "422"), ((7, 3), "420", "422"), ((7, 3), "444", "420")):
        tiny = _src("natural", w, h, 10, a, k=5)
        tm = np.random.default_rng(w * h).integers(0, 256, size=(h, w)).astype(np.uint8)
        got = loaded.apply_yuv_stack(_dev(tiny, loaded.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), stages=STAGES, cdl=grade,
                                     strength=0.8, matte=_mdev(tm, loaded.device))
        assert loaded.last_kernel == MATTE_GENERIC + _list(STAGES), loaded.last_kernel
        assert _eq(_host(got, 10), _want(loaded._res, STAGES, grade, 0.8, tm, 8, False, 10, 10, 10, a, b, tiny, ("tiny", w, h))), (w, h, a, b)
    # a padded stride (a view into a wider tensor) keeps the vector kernel; a base off by one element runs the generic one
    src = _src("natural", W, H, 10, "420", nf=2)
    dev = _dev(src, loaded.device)
    m = _matte(W, H, 10, nf=2)
    want = _want(loaded._res, STAGES, grade, 0.8, m, 10, False, 10, 10, 10, "420", "422", src, "nine")
    wide = torch.zeros((2, H + 1, W + 24), dtype=torch.int16, device=loaded.device)
    for off, name in ((0, _matte_name(10, 10, 10, "420", "422", STAGES, True)), (1, MATTE_GENERIC + _list(STAGES))):
        view = wide[:, :H, off:off + W]
        view.copy_(_mdev(m, loaded.device))
        got = loaded.apply_yuv_stack(dev, stages=STAGES, cdl=grade, strength=0.8, matte=view, matte_depth=10, **NAMES)
        assert loaded.last_kernel == name, (off, loaded.last_kernel)
        assert _eq(_host(got, 10), want), off
    # a pyramid or prism stage runs on the generic kernel
    for st in ((("lut3d", "pyramid"), ("lut3d2", "nearest")), (("lut3d", "trilinear"), ("lut3d2", "prism"))):
        got = loaded.apply_yuv_stack(dev, stages=st, strength=0.8, matte=_mdev(m, loaded.device), matte_depth=10, **NAMES)
        assert loaded.last_kernel == MATTE_GENERIC + _list(st), loaded.last_kernel
        assert _eq(_host(got, 10), _want(loaded._res, st, None, 0.8, m, 10, False, 10, 10, 10, "420", "422", src, "modes")), st


# ------------------------------------------------------------------ 7: table placement
@pytest.mark.gpu
def test_lds_and_global_tables_give_the_same_bytes(luts):
    """LUTR_STACK_LDS unset / 0 in two child processes (the knob is read at launch): the same output bytes, and the placements that
    ran."""
    outs = []
    for knob, placed in ((None, b"1110"), ("0", b"0000")):
        env = {k: v for k, v in os.environ.items() if k != "LUTR_STACK_LDS"}
        if knob is not None:
            env["LUTR_STACK_LDS"] = knob
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "_gpu_matte_worker.py"), str(luts["log709_33"][0]),
                            str(GOLDEN / "lut1d" / "gamma1024.cube"), str(GOLDEN / "cdl" / "shot.cc")], capture_output=True, cwd=ROOT,
                           timeout=180, env=env)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        assert r.stderr.endswith(placed), r.stderr[-200:]
        outs.append(r.stdout)
    assert len(outs[0]) > 100000 and outs[0] == outs[1]


# ------------------------------------------------------------------ 8: the C entry
def _abi(engine, strength, matte, w, h, s, d, nf=1, stages=((3, 0), (4, 0), (1, 2)), cdl=None):
    """lutr_apply_yuv_stack_matte with raw (kind, interp) pairs at 10 bit, 4:2:0 in, 4:2:2 out; `matte` a MatteStruct or None;
    returns (rc, message)."""
    p = _native.YuvParams(_native.fmt_code(10, 1, 1), _native.fmt_code(10, 1, 0), 10, 0, 0, 0, 0, 0)
    arr = (_native.StageStruct * max(len(stages), 1))()
    for i, (kind, interp) in enumerate(stages):
        arr[i].kind, arr[i].interp = kind, interp
    k = None if cdl is None else C.byref(_native.cdl_struct(cdl))
    with engine._lock:
        engine._bind_stream()
        rc = engine._lib.lutr_apply_yuv_stack_matte(engine._ctx, C.byref(p), arr, len(stages), k, strength, None,
                                                    None if matte is None else C.byref(matte), w, h, nf, C.byref(s), C.byref(d), 0, h)
    return rc, engine._lib.lutr_last_error().decode()


def _mstruct(t, depth, invert=0, **over):
    m = _native.MatteStruct()
    m.data = t.data_ptr()
    m.stride = t.stride(-2) * t.element_size()
    m.frame_stride = t.stride(0) * t.element_size() if t.dim() == 3 else 0
    m.depth, m.invert = depth, invert
    for k, v in over.items():
        setattr(m, k, v)
    return m


@pytest.mark.gpu
def test_the_c_entry_refuses_and_runs(loaded, grade):
    import torch
    src = _src("natural", W, H, 10, "420", nf=2)
    dev = _dev(src, loaded.device)
    m = _matte(W, H, 10, nf=2)
    md = _mdev(m, loaded.device)
    m8 = _mdev(_matte(W, H, 8, nf=2), loaded.device)
    want = _want(loaded._res, STAGES, grade, 0.8, m, 10, True, 10, 10, 10, "420", "422", src, "abi")
    out = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=loaded.device) for p in want]
    s, d = _desc(dev), _desc(out)
    refusals = [
        (None, "null matte"),
        (_mstruct(md, 10, data=None), "null matte"),
        (_mstruct(md, 7), "depth 7 outside 8..16"),
        (_mstruct(md, 17), "depth 17 outside 8..16"),
        (_mstruct(md, 10, invert=2), "invert 2"),
        (_mstruct(md, 10, invert=-1), "invert -1"),
        (_mstruct(md, 10, stride=2 * W - 2), "shorter than a row"),
        (_mstruct(m8, 8, stride=W - 1), "shorter than a row"),
        (_mstruct(md, 10, data=md.data_ptr() + 1), "must be even"),
        (_mstruct(md, 10, stride=2 * W + 1), "must be even"),
        (_mstruct(md, 10, frame_stride=2 * W * H + 1), "must be even"),
        (_mstruct(md, 10, frame_stride=-2 * W * H), "negative"),
        (_mstruct(out[0], 10), "overlaps that of destination plane 0"),
        (_mstruct(m8, 8, data=out[2].data_ptr(), frame_stride=0), "overlaps that of destination plane 2"),
    ]
    for matte, text in refusals:
        rc, msg = _abi(loaded, 0.8, matte, W, H, s, d, nf=2, cdl=grade)
        assert rc == _native.EINVAL and "matte" in msg and text in msg, (text, rc, msg)
    # every refusal of lutr_apply_yuv_stack_mix is kept
    rc, msg = _abi(loaded, 1.5, _mstruct(md, 10), W, H, s, d, nf=2, cdl=grade)
    assert rc == _native.EINVAL and "strength" in msg and "[0, 1]" in msg, msg
    rc, msg = _abi(loaded, 0.8, _mstruct(md, 10), W, H, s, d, nf=2, stages=[(1, 2)], cdl=grade)
    assert rc == _native.EINVAL and "no cdl stage is listed" in msg, msg
    rc, msg = _abi(loaded, 0.8, _mstruct(md, 10), W, H, s, s, nf=2, cdl=grade)
    assert rc == _native.EINVAL and "cannot run in place" in msg, msg
    torch.cuda.synchronize()
    assert all((t == 0x5a5a).all() for t in out), "a refused call wrote to a destination"
    rc, msg = _abi(loaded, 0.8, _mstruct(md, 10, invert=1), W, H, s, d, nf=2, cdl=grade)
    assert rc == 0, msg
    assert loaded.last_kernel == "k_yuv_stack_matte_vec<1,1,1,1,1,1,0,0,1>[lut1d,cdl,lut3d:2]", loaded.last_kernel
    assert _eq(_host(out, 10), want)


# ------------------------------------------------------------------ 9: alpha
@pytest.mark.gpu
def test_a_yuva_frame_carries_its_alpha_past_the_matte(loaded, grade):
    src = _src("natural", W, H, 10, "420", k=11)
    alpha = np.random.default_rng(3).integers(0, 1024, size=(H, W)).astype(np.uint16)
    m = _matte(W, H, 10, seed=9)
    dev = _dev(list(src) + [alpha], loaded.device)
    kw = dict(stages=STAGES, cdl=grade, strength=0.8, matte=_mdev(m, loaded.device), matte_depth=10)
    got = _host(loaded.apply_yuv_stack(dev, pix_fmt="yuva420p10le", out_pix_fmt="yuva422p10le", **kw), 10)
    assert loaded.last_kernel.startswith(_matte_name(10, 10, 10, "420", "422", STAGES, True) + "+k_alpha_"), loaded.last_kernel
    assert len(got) == 4 and np.array_equal(got[3], alpha)
    assert _eq(got[:3], _want(loaded._res, STAGES, grade, 0.8, m, 10, False, 10, 10, 10, "420", "422", src, "yuva"))
    # the alpha plane as the key: passed as the matte, like any other plane
    keyed = _host(loaded.apply_yuv_stack(dev, pix_fmt="yuva420p10le", out_pix_fmt="yuva422p10le", **dict(kw, matte=dev[3])), 10)
    assert np.array_equal(keyed[3], alpha)
    assert _eq(keyed[:3], _want(loaded._res, STAGES, grade, 0.8, alpha, 10, False, 10, 10, 10, "420", "422", src, "yuva-key"))


# ------------------------------------------------------------------ 10: apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut_with_a_matte_and_no_stages(loaded, luts, grade):
    from lut_renderer_amd.api import apply_lut
    src = _src("natural", W, H, 10, "420", nf=2)
    m = _matte(W, H, 8, nf=2)
    got, tags = apply_lut(_dev(src, loaded.device), cube=luts["log709_33"][1], cdl=GOLDEN / "cdl" / "shot.cc", strength=0.5,
                          matte=_mdev(m, loaded.device), pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv",
                          out_pix_fmt="yuv422p10le", engine=loaded)
    assert loaded.last_kernel == _matte_name(10, 10, 8, "420", "422", "cdl,lut3d", True) and tags["colorspace"] == "bt709"
    assert _eq(_host(got, 10), _want(loaded._res, "cdl,lut3d", grade, 0.5, m, 8, False, 10, 10, 10, "420", "422", src, "api"))


def _cli(luts, tmp_path, src, matte, pix, extra=()):
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    path = tmp_path / "matte.raw"
    path.write_bytes(np.ascontiguousarray(matte).tobytes())
    nf = src[0].shape[0]
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le"), luts["log709_33"][0],
                         info, python_bin=sys.executable, cdl=GOLDEN / "cdl" / "shot.cc", strength=0.75, matte=path, matte_pix_fmt=pix,
                         matte_invert=bool(extra))
    tail = ["--strength", "0.75", "--matte", str(path), "--matte-pix-fmt", pix] + list(extra)
    assert cmd[-len(tail):] == tail, cmd
    r = subprocess.run(cmd + ["--batch", "2", "--duration", "0.200"], input=b"".join(p[f].tobytes() for f in range(nf) for p in src),
                       capture_output=True, cwd=ROOT, timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    return r.stdout


@pytest.mark.gpu
def test_cli_over_pipes_with_a_matte_per_frame(luts, l1ds, grade, tmp_path):
    """Five frames in batches of two: the matte file is read in lockstep with the input."""
    src = _src("natural", 64, 8, 10, "420", nf=5)
    res = dict(lut=luts["log709_33"][1], lut2=None, l1=(l1ds["gamma1024"], "linear"), prelut=None)
    m = _matte(64, 8, 10, nf=5)
    planes = _want(res, "cdl,lut3d", grade, 0.75, m, 10, False, 10, 10, 10, "420", "422", src, "cli")
    want = b"".join(p[f].tobytes() for f in range(5) for p in planes)
    out = _cli(luts, tmp_path, src, m, "gray10le")
    assert len(out) == len(want) and out == want


@pytest.mark.gpu
def test_cli_over_pipes_with_a_still_matte(luts, l1ds, grade, tmp_path):
    """A file of exactly one frame is a still for the whole stream; --matte-invert travels."""
    src = _src("natural", 64, 8, 10, "420", nf=5)
    res = dict(lut=luts["log709_33"][1], lut2=None, l1=(l1ds["gamma1024"], "linear"), prelut=None)
    m = _matte(64, 8, 8, seed=4)
    planes = _want(res, "cdl,lut3d", grade, 0.75, m, 8, True, 10, 10, 10, "420", "422", src, "cli-still")
    want = b"".join(p[f].tobytes() for f in range(5) for p in planes)
    out = _cli(luts, tmp_path, src, m, "gray", extra=("--matte-invert",))
    assert len(out) == len(want) and out == want


# ------------------------------------------------------------------ 11: the call without a matte is today's
@pytest.mark.gpu
def test_a_call_without_a_matte_after_one_with_it_is_todays(loaded, grade):
    from tests import _mix_twin
    src = _src("natural", W, H, 10, "420", nf=2)
    dev = _dev(src, loaded.device)
    kw = dict(stages=STAGES, cdl=grade, **NAMES)
    loaded.apply_yuv_stack(dev, strength=[0.2, 0.8], matte=_mdev(_matte(W, H, 10, nf=2), loaded.device), matte_depth=10, **kw)
    assert loaded.last_kernel.startswith("k_yuv_stack_matte_vec<")
    got = _host(loaded.apply_yuv_stack(dev, strength=[0.2, 0.8], **kw), 10)
    assert loaded.last_kernel == _vec_name(10, 10, "420", "422", STAGES, True).replace("k_yuv_stack_vec<", "k_yuv_stack_mix_vec<", 1)
    k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 1, 0)
    res = dict(lut=loaded._res["lut"], cdl=grade, l1d_tab=_native.lut1d_table(*loaded._res["l1"], 10), cdl_tab=_native.cdl_table(grade, 10))
    assert _eq(got, _mix_twin.apply(parse_stages(STAGES), [0.2, 0.8], k, 10, 10, 1, 1, 1, 0, src, **res))
    plain = _host(loaded.apply_yuv_stack(dev, **kw), 10)
    assert loaded.last_kernel == _vec_name(10, 10, "420", "422", STAGES, True), loaded.last_kernel
    one = _host(loaded.apply_yuv_stack(dev, strength=1.0, **kw), 10)
    assert _eq(plain, one)
