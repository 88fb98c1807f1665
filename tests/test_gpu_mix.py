"""LUT strength on the GPU: lutr_apply_yuv_stack_mix bit-exact, whole planes, against tests/_mix_twin.py fed the
product's own host tables, and against the existing calls at strength 1 and 0.  The base size is tests/test_gpu_stack.py's: 136 x
36 -- at 8 samples per thread two full workgroups and a partial one."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, frames
from lut_renderer_amd.cdl import Cdl
from lut_renderer_amd.formats import parse_stages
from tests import _mix_twin as twin
from tests.test_gpu_stack import (GENERIC, LAYOUTS, H, W, _desc, _dev, _eq, _fmt, _host, _lds, _list, _src, _variant,  # noqa: F401
                                  _vec_name, grade, l1ds, loaded, luts)

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
MIX_GENERIC = "k_yuv_stack_mix_generic"
_refs = {}           # expected planes, computed once per case and shared (never written to)


def _mix_name(din, dout, a, b, stages, lds):
    return _vec_name(din, dout, a, b, stages, lds).replace("k_yuv_stack_vec<", "k_yuv_stack_mix_vec<", 1)


def _want(res, stages, cdl, strength, din, dl, dout, a, b, src, key):
    """The twin's planes for `src` ([rows, cols] or [nf, rows, cols] planes) and `strength` (a scalar or one per frame), with the
    resources `res` (the `loaded` fixture's) and the product's own tables at dl."""
    st = parse_stages(stages)
    rk = (id(res["lut"]), id(res["lut2"]), id(res["l1"][0]), res["l1"][1], st, None if cdl is None else (cdl.sop_text(), cdl.saturation),
          np.asarray(strength, dtype=np.float32).tobytes(), din, dl, dout, a, b, key)
    if rk not in _refs:
        (icsx, icsy), (ocsx, ocsy) = LAYOUTS[a], LAYOUTS[b]
        k = twin.consts("bt709", "tv", "bt709", "tv", din, dl, dout, ocsx, ocsy)
        kinds = [s for s, _ in st]
        _refs[rk] = twin.apply(st, strength, k, dl, dout, icsx, icsy, ocsx, ocsy, src, lut=res["lut"], lut2=res["lut2"],
                               prelut=res["prelut"], cdl=cdl, l1d_tab=_native.lut1d_table(*res["l1"], dl) if "lut1d" in kinds else None,
                               cdl_tab=_native.cdl_table(cdl, dl) if "cdl" in kinds else None)
    return _refs[rk]


# ------------------------------------------------------------------ 1: layouts
@pytest.mark.gpu
@pytest.mark.parametrize("a", list(LAYOUTS))
@pytest.mark.parametrize("b", list(LAYOUTS))
def test_all_nine_layout_pairs_at_10_bit(loaded, grade, a, b):
    stages = "lut1d,cdl,lut3d"
    src = _src("natural", W, H, 10, a, nf=2)
    got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), stages=stages, cdl=grade,
                                 strength=0.6)
    assert loaded.last_kernel == _mix_name(10, 10, a, b, stages, True), loaded.last_kernel
    assert _eq(_host(got, 10), _want(loaded._res, stages, grade, 0.6, 10, 10, 10, a, b, src, "nine"))


# ------------------------------------------------------------------ 2: container mixes
@pytest.mark.gpu
@pytest.mark.parametrize("din,dout,stages", [(8, 8, "lut1d,cdl,lut3d"), (16, 16, "lut3d:trilinear,lut3d2"), (16, 8, "lut1d,cdl,lut3d"),
                                             (8, 16, "lut1d,cdl,lut3d")], ids=lambda v: str(v))
def test_container_mixes_on_420_to_422(loaded, grade, din, dout, stages):
    src = _src("uniform", W, H, din, "420", nf=2)
    c = grade if "cdl" in stages else None
    got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt=_fmt(din, "420"), out_pix_fmt=_fmt(dout, "422"), stages=stages, cdl=c,
                                 strength=0.6)
    # an 8-bit source written as 16-bit words has no vector kernel
    name = MIX_GENERIC + _list(stages) if din == 8 and dout > 8 else _mix_name(din, dout, "420", "422", stages, _lds(stages, din))
    assert loaded.last_kernel == name, loaded.last_kernel
    if "trilinear" in stages:
        assert ",1,0>" in loaded.last_kernel                   # tri = 1; no table of the stack: nothing staged
    assert _eq(_host(got, dout), _want(loaded._res, stages, c, 0.6, din, din, dout, "420", "422", src, "mix"))


# ------------------------------------------------------------------ 3: a strength per frame
@pytest.mark.gpu
def test_a_strength_per_frame_whole_in_shards_and_on_a_group(loaded, luts, l1ds, grade, monkeypatch):
    import torch
    from lut_renderer_amd.multigpu import LutEngineGroup
    stages, s = "lut1d,cdl,lut3d", [0.0, 1.0, 0.37, 0.5]
    src = _src("natural", W, H, 10, "420", nf=4)
    dev = _dev(src, loaded.device)
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
    want = _want(loaded._res, stages, grade, s, 10, 10, 10, "420", "422", src, "frames")
    got = _host(loaded.apply_yuv_stack(dev, stages=stages, cdl=grade, strength=s, **names), 10)
    assert loaded.last_kernel == _mix_name(10, 10, "420", "422", stages, True)
    assert _eq(got, want)
    # frame 0 (s = 0): the identity CDL alone, i.e. the two conversion stages; frame 1 (s = 1): the call without a strength
    ident = _host(loaded.apply_yuv_stack([t[0] for t in dev], stages="cdl", cdl=Cdl(), **names), 10)
    plain = _host(loaded.apply_yuv_stack([t[1] for t in dev], stages=stages, cdl=grade, **names), 10)
    assert _eq([g[0] for g in got], ident) and _eq([g[1] for g in got], plain)
    assert not _eq([g[2] for g in got], _host(loaded.apply_yuv_stack([t[2] for t in dev], stages=stages, cdl=grade, **names), 10))
    # two row shards, on both kernels: a frame index taken from the shard would move the strengths
    for variant in ("auto", "generic"):
        with _variant(loaded, variant):
            out = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=loaded.device) for p in want]
            loaded.apply_yuv_stack(dev, out, row0=20, rows=H - 20, stages=stages, cdl=grade, strength=s, **names)
            assert "k_yuv_stack_mix_" in loaded.last_kernel
            assert (out[0][:, :20] == 0x5a5a).all() and (out[1][:, :10] == 0x5a5a).all(), "wrote outside the shard"
            loaded.apply_yuv_stack(dev, out, row0=0, rows=20, stages=stages, cdl=grade, strength=np.asarray(s), **names)
        assert _eq(_host(out, 10), want), variant
    # a CPU tensor, and a group of two engines with the second taken as remote: one copy of the array per device
    assert _eq(_host(loaded.apply_yuv_stack(dev, stages=stages, cdl=grade, strength=torch.tensor(s), **names), 10), want)
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    with LutEngineGroup([0, 0]) as g:
        g.set_lut(luts["log709_33"][1])
        g.set_lut1d(l1ds["gamma1024"], "cubic")
        got = g.apply_yuv_stack(dev, stages=stages, cdl=grade, strength=s, **names)
        assert g.last_remote == 1 and all(k.startswith("k_yuv_stack_mix_") for k in g.last_kernels), g.last_kernels
        assert _eq(_host(got, 10), want)
    with pytest.raises(ValueError, match="strength has 3 entries for 4 frames"):
        loaded.apply_yuv_stack(dev, stages=stages, cdl=grade, strength=s[:3], **names)
    with pytest.raises(ValueError, match=r"strength\[2\] = 1\.5"):
        loaded.apply_yuv_stack(dev, stages=stages, cdl=grade, strength=[0.0, 1.0, 1.5, 0.5], **names)


# ------------------------------------------------------------------ 4: the two ends against the existing calls
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "generic"])
def test_strength_1_and_0_are_the_two_existing_calls(loaded, grade, variant):
    stages = "lut1d,cdl,lut3d"
    src = _src("natural", W, H, 10, "420", nf=2)
    dev = _dev(src, loaded.device)
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
    with _variant(loaded, variant):
        plain = _host(loaded.apply_yuv_stack(dev, stages=stages, cdl=grade, **names), 10)
        assert "_mix_" not in loaded.last_kernel
        ident = _host(loaded.apply_yuv_stack(dev, stages="cdl", cdl=Cdl(), **names), 10)
        one = _host(loaded.apply_yuv_stack(dev, stages=stages, cdl=grade, strength=1.0, **names), 10)
        want = MIX_GENERIC + _list(stages) if variant == "generic" else _mix_name(10, 10, "420", "422", stages, True)
        assert loaded.last_kernel == want, loaded.last_kernel              # the mix kernels at strength 1 as well
        zero = _host(loaded.apply_yuv_stack(dev, stages=stages, cdl=grade, strength=0.0, **names), 10)
    assert _eq(one, plain) and _eq(zero, ident) and not _eq(one, zero)


# ------------------------------------------------------------------ 5: shapes
@pytest.mark.gpu
def test_a_ragged_width_a_tiny_frame_and_the_generic_modes(loaded, grade):
    import torch
    stages, pad = "lut1d,cdl,lut3d", 160
    src = _src("natural", 134, H, 10, "420", k=4)
    sp = [torch.zeros((p.shape[0], pad), dtype=torch.int16, device=loaded.device) for p in src]
    for t, p in zip(sp, _dev(src, loaded.device)):
        t[:, :p.shape[1]] = p
    src_v = [t[:, :p.shape[1]] for t, p in zip(sp, src)]
    oshape = [(H, 134)] + [frames.chroma_shape(134, H, 1, 0)] * 2
    dp = [torch.full((s[0], pad), -1, dtype=torch.int16, device=loaded.device) for s in oshape]
    dst_v = [t[:, :s[1]] for t, s in zip(dp, oshape)]
    loaded.apply_yuv_stack(src_v, dst_v, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, cdl=grade, strength=0.6)
    assert loaded.last_kernel == _mix_name(10, 10, "420", "422", stages, True).replace("[", "+" + MIX_GENERIC + "[", 1), loaded.last_kernel
    assert _eq(_host(dst_v, 10), _want(loaded._res, stages, grade, 0.6, 10, 10, 10, "420", "422", src, "ragged"))
    assert all((t[:, s[1]:] == -1).all() for t, s in zip(dp, oshape)), "wrote past the row"
    # 6 x 2 and an odd 7 x 3: the edge-pixel rule of the generic kernel
    for (w, h), a, b in (((6, 2), "420", "422"), ((7, 3), "420", "422"), ((7, 3), "444", "420")):
        tiny = _src("natural", w, h, 10, a, k=5)
        got = loaded.apply_yuv_stack(_dev(tiny, loaded.device), pix_fmt=_fmt(10, a), out_pix_fmt=_fmt(10, b), stages=stages, cdl=grade,
                                     strength=0.6)
        assert loaded.last_kernel == MIX_GENERIC + _list(stages), loaded.last_kernel
        assert _eq(_host(got, 10), _want(loaded._res, stages, grade, 0.6, 10, 10, 10, a, b, tiny, ("tiny", w, h))), (w, h, a, b)
    # a pyramid or prism stage runs on the generic kernel
    src = _src("natural", W, H, 10, "420", nf=2)
    for st in ((("lut3d", "pyramid"), ("lut3d2", "nearest")), (("lut3d", "trilinear"), ("lut3d2", "prism"))):
        got = loaded.apply_yuv_stack(_dev(src, loaded.device), pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=st, strength=0.6)
        assert loaded.last_kernel == MIX_GENERIC + _list(st), loaded.last_kernel
        assert _eq(_host(got, 10), _want(loaded._res, st, None, 0.6, 10, 10, 10, "420", "422", src, "modes")), st


# ------------------------------------------------------------------ 6: table placement
@pytest.mark.gpu
def test_lds_and_global_tables_give_the_same_bytes(luts):
    """LUTR_STACK_LDS unset / 0 in two child processes (the knob is read at launch): the same output bytes, and the placements that
    ran."""
    outs = []
    for knob, placed in ((None, b"11110"), ("0", b"00000")):
        env = {k: v for k, v in os.environ.items() if k != "LUTR_STACK_LDS"}
        if knob is not None:
            env["LUTR_STACK_LDS"] = knob
        r = subprocess.run([sys.executable, str(ROOT / "tests" / "_gpu_mix_worker.py"), str(luts["log709_33"][0]),
                            str(GOLDEN / "lut1d" / "gamma1024.cube"), str(GOLDEN / "cdl" / "shot.cc")], capture_output=True, cwd=ROOT,
                           timeout=180, env=env)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        assert r.stderr.endswith(placed), r.stderr[-200:]
        outs.append(r.stdout)
    assert len(outs[0]) > 100000 and outs[0] == outs[1]


# ------------------------------------------------------------------ 7: the C entry
def _abi(engine, stages, cdl, strength, frame_strength, w, h, s, d, nf=1):
    """lutr_apply_yuv_stack_mix with raw (kind, interp) pairs at 10 bit, 4:2:0 in, 4:2:2 out; returns (rc, message)."""
    p = _native.YuvParams(_native.fmt_code(10, 1, 1), _native.fmt_code(10, 1, 0), 10, 0, 0, 0, 0, 0)
    arr = (_native.StageStruct * max(len(stages), 1))()
    for i, (kind, interp) in enumerate(stages):
        arr[i].kind, arr[i].interp = kind, interp
    k = None if cdl is None else C.byref(_native.cdl_struct(cdl))
    fs = None if frame_strength is None else C.c_void_p(frame_strength.data_ptr())
    with engine._lock:
        engine._bind_stream()
        rc = engine._lib.lutr_apply_yuv_stack_mix(engine._ctx, C.byref(p), arr, len(stages), k, strength, fs, w, h, nf, C.byref(s),
                                                  C.byref(d), 0, h)
    return rc, engine._lib.lutr_last_error().decode()


@pytest.mark.gpu
def test_the_c_entry_clamps_the_array_and_refuses_the_scalar(loaded, grade):
    import torch
    stages, raw = "lut1d,cdl,lut3d", [(3, 0), (4, 0), (1, 2)]
    src = _src("natural", W, H, 10, "420", nf=3)
    dev = _dev(src, loaded.device)
    want = _want(loaded._res, stages, grade, [1.0, 0.0, 0.0], 10, 10, 10, "420", "422", src, "clamp")
    out = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=loaded.device) for p in want]
    s, d = _desc(dev), _desc(out)
    # the scalar refusals first: nothing launched, the destination untouched
    for bad in (float("nan"), 1.5, -0.25, float("inf")):
        rc, msg = _abi(loaded, raw, grade, bad, None, W, H, s, d, nf=3)
        assert rc == _native.EINVAL and "strength" in msg and "[0, 1]" in msg, (bad, msg)
    rc, msg = _abi(loaded, [(1, 2)], grade, 0.5, None, W, H, s, d, nf=3)       # a refusal of lutr_apply_yuv_stack, kept
    assert rc == _native.EINVAL and "no cdl stage is listed" in msg, msg
    rc, msg = _abi(loaded, raw, grade, 0.5, None, W, H, s, s, nf=3)
    assert rc == _native.EINVAL and "cannot run in place" in msg, msg
    torch.cuda.synchronize()
    assert all((t == 0x5a5a).all() for t in out), "a refused call wrote to a destination"
    # with the array the scalar is not read (a NaN here), and the kernels clamp what the host could not see
    fs = torch.tensor([1.5, -1.0, float("nan")], dtype=torch.float32, device=loaded.device)
    rc, msg = _abi(loaded, raw, grade, float("nan"), fs, W, H, s, d, nf=3)
    assert rc == 0, msg
    assert loaded.last_kernel == "k_yuv_stack_mix_vec<1,1,1,1,1,0,0,1>[lut1d,cdl,lut3d:2]", loaded.last_kernel
    assert _eq(_host(out, 10), want)
    with _variant(loaded, "generic"):
        for t in out:
            t.fill_(0x5a5a)
        rc, msg = _abi(loaded, raw, grade, 0.0, fs, W, H, s, d, nf=3)
        assert rc == 0 and loaded.last_kernel == MIX_GENERIC + "[lut1d,cdl,lut3d:2]", (msg, loaded.last_kernel)
    assert _eq(_host(out, 10), want)


# ------------------------------------------------------------------ 8: alpha
@pytest.mark.gpu
def test_a_yuva_frame_carries_its_alpha_past_the_mix(loaded, grade):
    stages = "lut1d,cdl,lut3d"
    src = _src("natural", W, H, 10, "420", k=11)
    alpha = np.random.default_rng(3).integers(0, 1024, size=(H, W)).astype(np.uint16)
    names = dict(pix_fmt="yuva420p10le", out_pix_fmt="yuva422p10le", stages=stages, cdl=grade)
    dev = _dev(list(src) + [alpha], loaded.device)
    got = _host(loaded.apply_yuv_stack(dev, strength=0.6, **names), 10)
    assert loaded.last_kernel.startswith(_mix_name(10, 10, "420", "422", stages, True) + "+k_alpha_"), loaded.last_kernel
    three = _host(loaded.apply_yuv_stack(dev[:3], pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, cdl=grade, strength=0.6), 10)
    assert len(got) == 4 and _eq(got[:3], three)
    assert _eq(three, _want(loaded._res, stages, grade, 0.6, 10, 10, 10, "420", "422", src, "yuva"))
    plain = _host(loaded.apply_yuv_stack(dev, **names), 10)
    assert np.array_equal(got[3], plain[3]) and np.array_equal(got[3], alpha)


# ------------------------------------------------------------------ 9: apply_lut and the CLI
@pytest.mark.gpu
def test_apply_lut_with_a_strength_and_no_stages(loaded, luts, grade):
    from lut_renderer_amd.api import apply_lut
    src = _src("natural", W, H, 10, "420", nf=2)
    got, tags = apply_lut(_dev(src, loaded.device), cube=luts["log709_33"][1], cdl=GOLDEN / "cdl" / "shot.cc", strength=0.5,
                          pix_fmt="yuv420p10le", colorspace="bt709", color_range="tv", out_pix_fmt="yuv422p10le", engine=loaded)
    assert loaded.last_kernel == _mix_name(10, 10, "420", "422", "cdl,lut3d", True) and tags["colorspace"] == "bt709"
    assert _eq(_host(got, 10), _want(loaded._res, "cdl,lut3d", grade, 0.5, 10, 10, 10, "420", "422", src, "api"))
    # a plain LUT with a strength runs the stack's gather kernel (there is no tile kernel for the mix)
    got, _ = apply_lut(_dev(src, loaded.device), cube=luts["log709_33"][1], strength=[0.25, 0.75], pix_fmt="yuv420p10le",
                       colorspace="bt709", color_range="tv", out_pix_fmt="yuv422p10le", engine=loaded)
    assert loaded.last_kernel == _mix_name(10, 10, "420", "422", "lut3d", False), loaded.last_kernel
    assert _eq(_host(got, 10), _want(loaded._res, "lut3d", None, [0.25, 0.75], 10, 10, 10, "420", "422", src, "api"))


@pytest.mark.gpu
def test_cli_over_pipes_with_strength_keys(luts, l1ds, grade):
    """Five frames in batches of two: the keys are read at the frame's number in the stream, not in the batch."""
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    src = _src("natural", 64, 8, 10, "420", nf=5)
    res = dict(lut=luts["log709_33"][1], lut2=None, l1=(l1ds["gamma1024"], "linear"), prelut=None)
    s = np.array([0.0, 1.0 / 3.0, 2.0 / 3.0, 1.0, 1.0]).astype(np.float32)
    planes = _want(res, "cdl,lut3d", grade, s, 10, 10, 10, "420", "422", src, "cli")
    want = b"".join(p[f].tobytes() for f in range(5) for p in planes)
    info = VideoInfo(width=64, height=8, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709", fps=25.0)
    cmd = engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="prores_ks", pix_fmt="yuv422p10le"), luts["log709_33"][0],
                         info, python_bin=sys.executable, cdl=GOLDEN / "cdl" / "shot.cc", strength_keys="0:0,3:1")
    assert cmd[-2:] == ["--strength-keys", "0:0,3:1"]
    r = subprocess.run(cmd + ["--batch", "2", "--duration", "0.200"], input=b"".join(p[f].tobytes() for f in range(5) for p in src),
                       capture_output=True, cwd=ROOT, timeout=180)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert len(r.stdout) == len(want) and r.stdout == want


# ------------------------------------------------------------------ 10: the call without a strength is today's
@pytest.mark.gpu
def test_a_call_without_strength_after_one_with_it_is_todays(loaded, grade):
    from tests import _stack_twin
    stages = "lut1d,cdl,lut3d"
    src = _src("natural", W, H, 10, "420", nf=2)
    dev = _dev(src, loaded.device)
    names = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages, cdl=grade)
    loaded.apply_yuv_stack(dev, strength=[0.2, 0.8], **names)
    assert loaded.last_kernel.startswith("k_yuv_stack_mix_vec<")
    got = _host(loaded.apply_yuv_stack(dev, **names), 10)
    assert loaded.last_kernel == _vec_name(10, 10, "420", "422", stages, True), loaded.last_kernel
    k = twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 1, 0)
    kw = dict(lut=loaded._res["lut"], cdl=grade, l1d_tab=_native.lut1d_table(*loaded._res["l1"], 10), cdl_tab=_native.cdl_table(grade, 10))
    for f in range(2):
        want = _stack_twin.apply(parse_stages(stages), k, 10, 10, 1, 1, 1, 0, [p[f] for p in src], **kw)
        assert _eq([g[f] for g in got], want), f
    with _variant(loaded, "generic"):
        loaded.apply_yuv_stack(dev, strength=0.5, **names)
        assert loaded.last_kernel == MIX_GENERIC + _list(stages)
        again = _host(loaded.apply_yuv_stack(dev, **names), 10)
        assert loaded.last_kernel == GENERIC + _list(stages)
    assert _eq(again, got)
