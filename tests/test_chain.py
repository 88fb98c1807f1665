"""Two LUTs in one fused pass -- host side: the contract as a composition of oracle calls, the argument checks
that run before any GPU work, and the CLI / command-layer options.  GPU parity is tests/test_gpu_chain.py."""
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from lut_renderer_amd import _native, cube, frames
from lut_renderer_amd.engine import LutEngine, chain_side, check_chain_options
from lut_renderer_amd.params import ProcessingParams, VideoInfo
from oracle import lut3d_numpy as ref
from tests import _chain_twin as twin
from tests import _xsub_twin as xsub
from tests._csp_files import write_csp_with_prelut

ROOT = Path(__file__).resolve().parent.parent
W, H = 64, 8
VEC_MODES = ("nearest", "trilinear", "tetrahedral")


def _lut(table, scale=(1.0, 1.0, 1.0)):
    table = np.ascontiguousarray(table, dtype=np.float32)
    return cube.CubeLut(table.shape[0], np.array(scale, np.float32), table)


def _eq(got, want):
    return all(np.asarray(g).shape == np.asarray(w).shape and np.array_equal(g, w) for g, w in zip(got, want))


@pytest.fixture(scope="module")
def pairs(cube_dir, tmp_path_factory):
    """The LUT pairs of the GPU tests: name -> (A, B, A's oracle prelut or None).  A and B differ in size on purpose."""
    out = {name: (cube.read_lut(a), cube.read_lut(b), pre)
           for name, (a, b, pre) in twin.lut_pairs(cube_dir, tmp_path_factory.mktemp("chain_luts")).items()}
    assert float(out["wide_domain"][1].scale[0]) == 0.5 and out["csp_random"][0].prelut is not None
    return out


# ------------------------------------------------------------------ the contract
@pytest.mark.parametrize("depth", [8, 10])
@pytest.mark.parametrize("mode", VEC_MODES)
def test_the_c_oracle_composed_twice_is_the_numpy_oracle_composed_twice(pairs, depth, mode):
    k = twin.consts(din=depth, dl=depth, dout=depth, ocsx=1, ocsy=1)
    for dist in ("uniform", "natural"):
        src = frames.make_yuv(dist, W, H, depth, 1, 1, k=3)
        q0 = ref.yuv_to_rgb_codes(k, 1, 1, src)
        for name in ("log709_random", "wide_domain"):
            A, B, _ = pairs[name]
            q1 = ref.lut3d_codes(A.table, A.scale, depth, mode, *q0)
            q2 = ref.lut3d_codes(B.table, B.scale, depth, mode, *q1)
            assert _eq(twin.intermediate(A, mode, k, depth, 1, 1, src), q1), (name, dist, "intermediate")
            assert _eq(twin.apply(A, B, mode, mode, k, depth, depth, 1, 1, 1, 1, src), ref.rgb_codes_to_yuv(k, depth, 1, 1, q2)), \
                (name, dist)
        # the numpy oracle has no prelut: for the .csp pair the first stage is the C oracle's, the second stage is compared
        A, B, pre = pairs["csp_random"]
        q1 = twin.intermediate(A, mode, k, depth, 1, 1, src, pre)
        q2 = ref.lut3d_codes(B.table, B.scale, depth, mode, *[np.asarray(a).astype(np.int64) for a in q1])
        assert _eq(twin.apply(A, B, mode, mode, k, depth, depth, 1, 1, 1, 1, src, pre), ref.rgb_codes_to_yuv(k, depth, 1, 1, q2)), dist


@pytest.mark.parametrize("depth", [8, 10])
def test_known_answer_by_hand(depth):
    """A: every node (0.5, 0.25, 0.75).  Its output codes are (int)(0.5 M), (int)(0.25 M), (int)(0.75 M) = 127, 63, 191 at 8 bit and
    511, 255, 767 at 10 bit; over M they are 0.498, 0.247, 0.749 (0.4995, 0.2493, 0.7498), which nearest mode on N = 2 rounds to
    node (0, 0, 1) of B.  The frame is then one colour: the YUV code of that node."""
    m = (1 << depth) - 1
    A = _lut(np.broadcast_to(np.array([0.5, 0.25, 0.75], np.float32), (2, 2, 2, 3)))
    B = _lut(np.arange(24, dtype=np.float32).reshape(2, 2, 2, 3) / 32.0 + 0.125)        # eight distinct nodes
    node = B.table[0, 0, 1]
    k = twin.consts(din=depth, dl=depth, dout=depth, ocsx=1, ocsy=1)
    src = frames.uniform_yuv(16, 4, depth, 1, 1, k=1)
    q1 = twin.intermediate(A, "tetrahedral", k, depth, 1, 1, src)
    assert [int(np.unique(a)[0]) for a in q1 if len(np.unique(a)) == 1] == [int(0.5 * m), int(0.25 * m), int(0.75 * m)]
    codes = [np.full((4, 16), int(np.float32(v) * np.float32(m)), np.int64) for v in node]
    want = ref.rgb_codes_to_yuv(k, depth, 1, 1, codes)
    got = twin.apply(A, B, "tetrahedral", "nearest", k, depth, depth, 1, 1, 1, 1, src)
    assert _eq(got, want) and all(len(np.unique(p)) == 1 for p in got)
    # and not the code of any other node
    for other in ((0, 0, 0), (1, 1, 1), (1, 0, 1)):
        c2 = [np.full((4, 16), int(np.float32(v) * np.float32(m)), np.int64) for v in B.table[other]]
        assert not _eq(got, ref.rgb_codes_to_yuv(k, depth, 1, 1, c2))


def test_codes_that_enter_the_second_lut_are_clipped(pairs):
    A, B, _ = pairs["wide_domain"]
    assert A.table.min() == -0.25 and A.table.max() == 1.25
    k = twin.consts(din=10, dl=10, dout=10, ocsx=1, ocsy=1)
    src = frames.uniform_yuv(W, H, 10, 1, 1, k=5)
    q0 = ref.yuv_to_rgb_codes(k, 1, 1, src)
    q1 = twin.intermediate(A, "trilinear", k, 10, 1, 1, src)
    assert min(int(a.min()) for a in q0) == 0 and max(int(a.max()) for a in q0) == 1023        # the frame reaches both ends
    assert min(int(np.min(a)) for a in q1) == 0 and max(int(np.max(a)) for a in q1) == 1023    # -0.25 -> 0, 1.25 -> M
    # the unclipped value of the first LUT lies outside [0, M] there
    v = ref._interp(A.table, "trilinear", [np.clip((a.astype(np.float32) * np.float32(1 / 1023)) * np.float32(8), 0, 8).astype(np.float32)
                                           for a in q0])
    assert v.min() < 0 and v.max() > 1
    got = twin.apply(A, B, "trilinear", "trilinear", k, 10, 10, 1, 1, 1, 1, src)
    assert _eq(got, ref.rgb_codes_to_yuv(k, 10, 1, 1, twin.second_lut(B, "trilinear", 10, q1)))


def test_a_constant_second_lut_gives_its_single_lut_twin(pairs):
    A = pairs["log709_random"][0]
    B = _lut(np.broadcast_to(np.array([0.3, 0.6, 0.1], np.float32), (5, 5, 5, 3)))
    for a, b in (("420", "420"), ("420", "422"), ("444", "420")):
        (icsx, icsy), (ocsx, ocsy) = twin.LAYOUTS[a], twin.LAYOUTS[b]
        k = twin.consts(din=10, dl=10, dout=10, ocsx=ocsx, ocsy=ocsy)
        src = frames.natural_yuv(33, 7, 10, icsx, icsy, k=2)
        got = twin.apply(A, B, "tetrahedral", "trilinear", k, 10, 10, icsx, icsy, ocsx, ocsy, src)
        assert _eq(got, xsub.apply(B.table, B.scale, "trilinear", k, 10, 10, icsx, icsy, ocsx, ocsy, src)), (a, b)


# ------------------------------------------------------------------ the symbols
def test_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "lutr.h").read_text()
    assert "int  lutr_ctx_set_lut2(lutr_ctx *ctx, const float *rgb, int n, const float scale[3]);" in header
    assert "int lutr_apply_yuv_chain(lutr_ctx *ctx, const lutr_yuv_params *p, int interp, int interp2, int w, int h, int nframes," \
        in header
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    for sym in ("lutr_ctx_set_lut2", "lutr_apply_yuv_chain"):
        assert sym in _native.SYMBOLS and f" T {sym}\n" in nm
    lib = _native.load()
    assert len(lib.lutr_apply_yuv_chain.argtypes) == 11
    # no context, no planes: refused before anything touches a device
    assert lib.lutr_apply_yuv_chain(None, None, 2, 2, 16, 16, 1, None, None, 0, 16) == _native.EINVAL
    assert b"null" in lib.lutr_last_error()
    assert lib.lutr_ctx_set_lut2(None, None, 0, None) == _native.EINVAL


# ------------------------------------------------------------------ LutEngine, before the engine is touched
def _planes(depth, csx, csy, w=16, h=8):
    dt = torch.uint8 if depth <= 8 else torch.int16
    cs = ((h + (1 << csy) - 1) >> csy, (w + (1 << csx) - 1) >> csx)
    return [torch.zeros((h, w), dtype=dt), torch.zeros(cs, dtype=dt), torch.zeros(cs, dtype=dt)]


NAMES = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")


def test_a_second_lut_with_a_prelut_is_a_value_error(pairs):
    shaped = pairs["csp_random"][0]
    with pytest.raises(ValueError, match="second LUT carries a prelut"):
        LutEngine.set_lut2(object(), shaped)
    from lut_renderer_amd.multigpu import LutEngineGroup
    with pytest.raises(ValueError, match="second LUT carries a prelut"):
        LutEngineGroup.set_lut2(object(), shaped)
    from lut_renderer_amd.api import apply_lut
    with pytest.raises(ValueError, match="second LUT carries a prelut"):
        apply_lut(_planes(10, 1, 1), cube=None, cube2=shaped, pix_fmt="yuv420p10le", engine=object())


@pytest.mark.parametrize("side", ["pix_fmt", "out_pix_fmt"])
@pytest.mark.parametrize("name,word", [("yuva420p10le", "carries alpha"), ("nv12", "semi-planar"), ("p010le", "semi-planar"),
                                       ("uyvy422", "packed"), ("y210le", "packed"), ("vuyx", "packed"), ("v210", "v210"),
                                       ("gbrp10le", "an RGB format"), ("gbrap", "an RGB format"), ("rgb24", "an RGB format"),
                                       ("gbrpf32le", "a float RGB format")])
def test_a_side_that_is_not_planar_yuv_without_alpha_is_a_value_error(side, name, word):
    kw = {**NAMES, side: name}
    with pytest.raises(ValueError, match=f"planar YUV on both sides: {side} '{name}' (is|carries)"):
        LutEngine.apply_yuv_chain(object(), _planes(10, 1, 1), **kw)
    with pytest.raises(ValueError, match=word):
        check_chain_options(kw["pix_fmt"], kw["out_pix_fmt"])


def test_names_that_are_no_format_and_modes_lut3d_does_not_have():
    src = _planes(10, 1, 1)
    with pytest.raises(ValueError, match="unsupported pixel format 'yuv440p'"):
        LutEngine.apply_yuv_chain(object(), src, pix_fmt="yuv420p10le", out_pix_fmt="yuv440p")
    with pytest.raises(ValueError, match="no interpolation mode 'cubic'"):
        LutEngine.apply_yuv_chain(object(), src, **NAMES, interp2="cubic")
    with pytest.raises(ValueError, match="no interpolation mode 'bogus'"):
        LutEngine.apply_yuv_chain(object(), src, **NAMES, interp="bogus")
    assert chain_side("yuvj420p", "pix_fmt").name == "yuv420p"
    fin, fout = check_chain_options("yuv444p12le", None)
    assert (fout.name, fout.depth, fout.csx, fout.csy) == ("yuv444p12le", 12, 0, 0)


@pytest.mark.parametrize("key,value,message", [
    ("dither", "error_diffusion", "dither is not supported with a second LUT"),
    ("dither", "blue_noise", "apply_yuv_chain takes no 'dither'"),
    ("dither", "none", "apply_yuv_chain takes no 'dither'"),
    ("chroma_loc", "left", r"sited chroma resampling \(chroma_loc\) is not supported with a second LUT"),
    ("out_size", (8, 4), r"a resize \(out_size\) is not supported with a second LUT"),
    ("width", 16, r"a packed side \(width\) is not supported with a second LUT"),
    ("out2_pix_fmt", "yuv420p", r"a second output \(out2_pix_fmt\) is not supported with a second LUT"),
    ("dst2", None, r"a second output \(dst2\) is not supported with a second LUT"),
])
def test_options_of_apply_yuv_that_the_chain_does_not_take(key, value, message):
    with pytest.raises(ValueError, match=message):
        LutEngine.apply_yuv_chain(object(), _planes(10, 1, 1), **NAMES, **{key: value})
    with pytest.raises(TypeError, match="unexpected keyword argument 'bogus'"):
        LutEngine.apply_yuv_chain(object(), _planes(10, 1, 1), **NAMES, bogus=1)


def test_wrong_plane_shapes_and_dtypes():
    src = _planes(10, 1, 1)
    with pytest.raises(ValueError, match="expected three planes"):
        LutEngine.apply_yuv_chain(object(), src[:2], **NAMES)
    with pytest.raises(ValueError, match="source plane 1 is"):
        LutEngine.apply_yuv_chain(object(), _planes(10, 1, 0), **NAMES)
    with pytest.raises(ValueError, match="source plane 0: 'yuv420p10le' takes 16-bit integer samples"):
        LutEngine.apply_yuv_chain(object(), _planes(8, 1, 1), **NAMES)
    with pytest.raises(ValueError, match=r"destination plane 1 is \(4, 8\), 'yuv422p10le' at 16x8 needs \(8, 8\)"):
        LutEngine.apply_yuv_chain(object(), src, _planes(10, 1, 1), **NAMES)
    # everything in order: the first thing that fails is the engine itself (object() has no device)
    with pytest.raises(AttributeError):
        LutEngine.apply_yuv_chain(object(), src, _planes(10, 1, 0), **NAMES)


def test_the_group_checks_the_same_things_first():
    from lut_renderer_amd.multigpu import LutEngineGroup

    class _Lock:
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    class _Fake:
        _lock = _Lock()
    with pytest.raises(ValueError, match="the group owns the row partition"):
        LutEngineGroup.apply_yuv_chain(_Fake(), _planes(10, 1, 1), **NAMES, row0=0)
    with pytest.raises(ValueError, match="planar YUV on both sides"):
        LutEngineGroup.apply_yuv_chain(_Fake(), _planes(10, 1, 1), pix_fmt="yuv420p10le", out_pix_fmt="nv12")
    with pytest.raises(ValueError, match="not supported with a second LUT"):
        LutEngineGroup.apply_yuv_chain(_Fake(), _planes(10, 1, 1), **NAMES, chroma_loc="left")


# ------------------------------------------------------------------ apply_lut(cube2=)
def test_apply_lut_rejections_before_any_gpu_work():
    from lut_renderer_amd.api import apply_lut
    B = _lut(cube.identity_lattice(2))
    y, cb, cr = frames.natural_yuv(16, 8, 10, 1, 1)
    base = dict(cube=None, cube2=B, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", engine=object())
    for kw, message in ((dict(zscale_dither="error_diffusion"), "dither is not supported with a second LUT"),
                        (dict(engine_dither="blue_noise"), "dither is not supported with a second LUT"),
                        (dict(chroma_loc="left"), "chroma_loc.* is not supported with a second LUT"),
                        (dict(resolution="8x4"), "resize .* is not supported with a second LUT"),
                        (dict(second_pix_fmt="yuv420p"), "a second output is not supported with a second LUT"),
                        (dict(interp2="cubic"), "no interpolation mode 'cubic'")):
        with pytest.raises(ValueError, match=message):
            apply_lut((y, cb, cr), **base, **kw)
    with pytest.raises(ValueError, match="interp2 is the mode of the second LUT: it needs cube2"):
        apply_lut((y, cb, cr), cube=None, pix_fmt="yuv420p10le", interp2="nearest", engine=object())
    for name in ("yuva420p10le", "nv12", "uyvy422"):
        with pytest.raises(ValueError, match=name):          # (a container's own refusal may come first: it names the format too)
            apply_lut((y, cb, cr), **{**base, "out_pix_fmt": name})
    g, b, r = frames.natural_rgb(16, 8, 8, k=1)
    with pytest.raises(ValueError, match="pix_fmt 'gbrp' is an RGB format"):
        apply_lut((g, b, r), cube=None, cube2=B, pix_fmt="gbrp", out_pix_fmt="yuv420p", engine=object())
    with pytest.raises(ValueError, match="pix_fmt 'gbrpf32le' is a float RGB format"):
        apply_lut([np.zeros((8, 16), np.float32)] * 3, cube=None, cube2=B, pix_fmt="gbrpf32le", out_pix_fmt="yuv420p",
                  engine=object())


def test_chain_call_for_keeps_the_recorded_call_and_whitelists_the_second_mode():
    from lut_renderer_amd.api import chain_call_for, engine_call_for
    from lut_renderer_amd.plan import resolve_lut_plan
    info = VideoInfo(width=16, height=8, pix_fmt="yuvj420p", bit_depth=8, colorspace="bt709", color_range="pc")
    plan = resolve_lut_plan(ProcessingParams(), "look.cube", info)
    kw = engine_call_for(plan, "yuvj420p", "yuv422p10le")
    assert chain_call_for(dict(kw, dither="none")) == kw                                 # interp2 None: the first LUT's mode
    assert chain_call_for(dict(kw, dither="none"), "prism") == {**kw, "interp2": "prism"}
    assert chain_call_for(kw, "no-such-mode")["interp2"] == "tetrahedral"                # the fallback `interp` takes (plan.py)
    assert kw["range_src"] == "pc" and kw["lut_depth"] == 8                              # the full-range prologue travels unchanged


def test_apply_lut_uploads_a_second_lut_once_and_again_when_either_changes():
    """`apply_lut`'s shortcut on a stand-in engine: each LUT is uploaded when it is not the object uploaded last."""
    from lut_renderer_amd.api import apply_lut

    class _Lock:
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    class _Eng:
        _lock, precision, _applied_lut, _applied_lut2 = _Lock(), "strict", None, None

        def __init__(self): self.calls = []
        def set_lut(self, lut): self.calls.append(("A", lut)); self._applied_lut = None
        def set_lut2(self, lut): self.calls.append(("B", lut)); self._applied_lut2 = None
        def apply_yuv_chain(self, planes, out, **kw): self.calls.append(("apply", kw)); return out
        def apply_yuv(self, planes, out, **kw): self.calls.append(("plain", kw)); return out

    A, A2, B, B2 = (_lut(cube.identity_lattice(n)) for n in (2, 3, 4, 5))
    eng, y = _Eng(), frames.natural_yuv(16, 8, 10, 1, 1)
    kw = dict(pix_fmt="yuv420p10le", engine=eng)
    apply_lut(y, cube=A, cube2=B, interp2="nearest", **kw)
    assert [c[0] for c in eng.calls] == ["A", "B", "apply"] and eng.calls[2][1]["interp2"] == "nearest"
    assert eng.calls[2][1]["interp"] == "tetrahedral" and "dither" not in eng.calls[2][1]
    eng.calls.clear(); apply_lut(y, cube=A, cube2=B, **kw)
    assert [c[0] for c in eng.calls] == ["apply"] and "interp2" not in eng.calls[0][1]
    eng.calls.clear(); apply_lut(y, cube=A, cube2=B2, **kw)
    assert [c[:2] for c in eng.calls[:-1]] == [("B", B2)]
    eng.calls.clear(); apply_lut(y, cube=A2, cube2=B2, **kw)
    assert [c[:2] for c in eng.calls[:-1]] == [("A", A2)]
    eng.calls.clear(); apply_lut(y, cube=A2, **kw)                                       # without cube2 nothing changes
    assert [c[0] for c in eng.calls] == ["plain"] and eng.calls[0][1]["dither"] == "none"


# ------------------------------------------------------------------ the CLI
def _args(cube_path, *extra, pix_fmt="yuv420p10le"):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", pix_fmt, "--out-pix-fmt",
                                      "yuv422p10le", "--cube", str(cube_path), *extra])


def test_cli_flags(cube_dir):
    from lut_renderer_amd.cli import plan_from_args
    a = cube_dir / "log709_33.cube"
    plain = _args(a)
    assert plain.cube2 is None and plain.interp2 is None
    _, kw, w, h = plan_from_args(plain)
    assert "interp2" not in kw
    one = _args(a, "--cube2", "look.cube")
    _, kw1, _, _ = plan_from_args(one)
    assert one.cube2 == "look.cube" and kw1 == kw
    both = _args(a, "--cube2", "look.cube", "--interp2", "trilinear")
    _, kw2, _, _ = plan_from_args(both)
    assert kw2 == {**kw, "interp2": "trilinear"}
    with pytest.raises(ValueError, match="--interp2 is the mode of the second LUT: it needs --cube2"):
        plan_from_args(_args(a, "--interp2", "trilinear"))
    for extra, message in ((("--zscale-dither", "error_diffusion"), "dither is not supported with a second LUT"),
                           (("--engine-dither", "blue_noise"), "dither is not supported with a second LUT"),
                           (("--out-size", "8x4"), "resize .* is not supported with a second LUT"),
                           (("--second-output", "c.yuv", "--second-pix-fmt", "yuv420p"), "a second output is not supported"),
                           (("--interp2", "cubic"), "no interpolation mode 'cubic'")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args(a, "--cube2", "look.cube", *extra))
    with pytest.raises(ValueError, match="chroma_loc"):
        plan_from_args(_args(a, "--cube2", "look.cube", "--chroma-loc", "left", "--out-pix-fmt", "yuv420p10le"))
    for fmt, word in (("yuva420p10le", "carries alpha"), ("gbrp10le", "an RGB format"), ("uyvy422", "packed")):
        with pytest.raises(ValueError, match=word):
            plan_from_args(_args(a, "--cube2", "look.cube", pix_fmt=fmt))


def test_cli_refuses_before_it_opens_a_device(cube_dir, pairs, tmp_path):
    """The process contract on a bad option: `Error: ...` on stdout and exit code 1, no output file made."""
    src = tmp_path / "in.yuv"
    src.write_bytes(bytes(16 * 8 * 3))
    base = [sys.executable, "-m", "lut_renderer_amd.cli", "-i", str(src), "-o", str(tmp_path / "o.yuv"), "--size", "16x8",
            "--pix-fmt", "yuv420p10le", "--cube", str(cube_dir / "log709_33.cube")]
    r = subprocess.run(base + ["--interp2", "nearest"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 1 and "Error: --interp2 is the mode of the second LUT" in r.stdout
    assert not (tmp_path / "o.yuv").exists()


def test_cli_refuses_a_second_lut_with_a_prelut(cube_dir, tmp_path, capsys):
    from lut_renderer_amd import cli
    shapers = [(np.array([0.0, 0.5, 1.0]), np.array([0.0, 0.7, 1.0]))] * 3
    write_csp_with_prelut(tmp_path / "shaped.csp", 2, cube.identity_lattice(2), shapers)
    rc = cli.main(["-i", "a", "-o", str(tmp_path / "o.yuv"), "--size", "16x8", "--pix-fmt", "yuv420p10le", "--cube",
                   str(cube_dir / "log709_33.cube"), "--cube2", str(tmp_path / "shaped.csp")])
    assert rc == 1 and "Error: the second LUT carries a prelut" in capsys.readouterr().out
    assert not (tmp_path / "o.yuv").exists()


# ------------------------------------------------------------------ the command layer
def test_engine_command_and_pipe_render_the_flags_only_when_given():
    from lut_renderer_amd.command import engine_command
    from lut_renderer_amd.pipe import engine_stage_commands
    params = ProcessingParams(video_codec="libx265", pix_fmt="yuv420p10le")
    info = VideoInfo(width=1920, height=1080, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709",
                     fps=25.0, duration=4.0)
    plain = engine_command(Path("-"), Path("-"), params, Path("tech.cube"), info, python_bin="python3")
    assert "--cube2" not in plain and "--interp2" not in plain
    assert engine_command(Path("-"), Path("-"), params, Path("tech.cube"), info, python_bin="python3", cube2=None, interp2=None) == plain
    one = engine_command(Path("-"), Path("-"), params, Path("tech.cube"), info, python_bin="python3", cube2=Path("look.cube"))
    assert one == plain + ["--cube2", "look.cube"]
    two = engine_command(Path("-"), Path("-"), params, Path("tech.cube"), info, python_bin="python3", cube2=Path("look.cube"),
                         interp2="trilinear")
    assert two == plain + ["--cube2", "look.cube", "--interp2", "trilinear"]
    assert engine_command(Path("-"), Path("-"), params, Path("tech.cube"), info, python_bin="python3", cube2=Path("look.cube"),
                          interp2="no-such-mode")[-1] == "tetrahedral"
    # the CLI resolves what the command rendered
    from lut_renderer_amd.cli import build_parser, plan_from_args
    args = build_parser().parse_args(two[3:])
    assert (args.cube, args.cube2) == ("tech.cube", "look.cube") and plan_from_args(args)[1]["interp2"] == "trilinear"
    for kwargs, message in ((dict(interp2="nearest"), "it needs cube2"),
                            (dict(cube2=Path("l.cube"), chroma_loc="left"), "chroma_loc"),
                            (dict(cube2=Path("l.cube"), engine_dither="blue_noise"), "dither is not supported with a second LUT"),
                            (dict(cube2=Path("l.cube"), second_output=Path("d.yuv"), second_pix_fmt="yuv420p"), "a second output")):
        with pytest.raises(ValueError, match=message):
            engine_command(Path("-"), Path("-"), params, Path("tech.cube"), info, python_bin="python3", **kwargs)
    rgb = VideoInfo(width=64, height=32, bit_depth=8, pix_fmt="rgb24", fps=25.0)
    with pytest.raises(ValueError, match="pix_fmt 'rgb24' is an RGB format"):
        engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx264", pix_fmt="yuv420p"), Path("tech.cube"), rgb,
                       python_bin="python3", cube2=Path("l.cube"))
    # the three-process stage: only the engine's argv changes
    base = engine_stage_commands(Path("in.mov"), Path("out.mp4"), params, Path("tech.cube"), info, python_bin="python3")
    assert engine_stage_commands(Path("in.mov"), Path("out.mp4"), params, Path("tech.cube"), info, python_bin="python3", cube2=None,
                                 interp2=None) == base
    chain = engine_stage_commands(Path("in.mov"), Path("out.mp4"), params, Path("tech.cube"), info, python_bin="python3",
                                  cube2=Path("look.cube"), interp2="prism")
    assert (chain.decoder, chain.encoder) == (base.decoder, base.encoder)
    i = chain.engine.index("--cube2")
    assert chain.engine[i:i + 4] == ["--cube2", "look.cube", "--interp2", "prism"]
    assert chain.engine[:i] + chain.engine[i + 4:] == base.engine


def test_host_pipeline_checks_a_chain_before_it_allocates():
    from lut_renderer_amd.stream import HostPipeline
    for kw, message in ((dict(out_pix_fmt="nv12"), "semi-planar"), (dict(second_pix_fmt="yuv420p"), "a second output"),
                        (dict(out_size=(8, 4)), "resize"), (dict(dither="blue_noise"), "dither")):
        with pytest.raises(ValueError, match=message):
            HostPipeline(SimpleNamespace(), "yuv420p10le", 16, 8, chain=True, **kw)


def test_two_lut_side_and_option_refusals_keep_their_words():
    """Every refusal of `chain_side`, `check_chain_options` and `refuse_chain_keywords`, whole, and the order they fire in."""
    from lut_renderer_amd.engine import refuse_chain_keywords
    head = "the two-LUT pass takes planar YUV on both sides: out_pix_fmt"
    for name, tail in (("nv12", "is a semi-planar container"), ("uyvy422", "is a packed container"), ("vuya", "is a packed container"),
                       ("v210", "is a v210 container"), ("v410", "is a v210 container"), ("rgb24", "is an RGB format"),
                       ("gbrap10le", "is an RGB format"), ("gbrapf32le", "is a float RGB format"), ("yuva444p12le", "carries alpha")):
        with pytest.raises(ValueError) as e:
            chain_side(name, "out_pix_fmt")
        assert str(e.value) == f"{head} '{name}' {tail}"
    for name in (None, ""):
        with pytest.raises(ValueError) as e:
            chain_side(name, "out_pix_fmt")
        assert str(e.value) == "the two-LUT pass needs out_pix_fmt"
    assert chain_side("yuvj420p", "pix_fmt").name == "yuv420p"
    # a bad side goes before a bad option, and the options in the order dither, chroma_loc, out_size, second output
    with pytest.raises(ValueError, match="^the two-LUT pass takes planar YUV on both sides: pix_fmt 'nv12'"):
        check_chain_options("nv12", "yuva420p", "blue_noise", "left", (8, 4), "yuv420p")
    for args, text in ((("blue_noise", "left", (8, 4), "yuv420p"), "dither is not supported with a second LUT"),
                       (("none", "left", (8, 4), "yuv420p"), "sited chroma resampling (chroma_loc) is not supported with a second LUT"),
                       (("none", None, (8, 4), "yuv420p"), "a resize (out_size) is not supported with a second LUT"),
                       (("none", None, None, "yuv420p"), "a second output is not supported with a second LUT")):
        with pytest.raises(ValueError) as e:
            check_chain_options("yuv420p", "yuv422p10le", *args)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        refuse_chain_keywords(dict(dst2=None, out2_pix_fmt="yuv420p", width=16))
    assert str(e.value) == "a packed side (width) is not supported with a second LUT: apply_yuv_chain takes no 'width'"
    with pytest.raises(ValueError) as e:
        refuse_chain_keywords(dict(dst2=None, out2_pix_fmt="yuv420p"))
    assert str(e.value) == "a second output (out2_pix_fmt) is not supported with a second LUT: apply_yuv_chain takes no 'out2_pix_fmt'"
    with pytest.raises(ValueError) as e:
        refuse_chain_keywords(dict(dst2=None))
    assert str(e.value) == "a second output (dst2) is not supported with a second LUT: apply_yuv_chain takes no 'dst2'"
