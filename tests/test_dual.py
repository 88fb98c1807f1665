"""Two YUV outputs from one LUT pass -- host side: the argument checks that run before any GPU work, the CLI and
command-layer options, the exported symbol and the layout of the second output ring.  GPU parity is tests/test_gpu_dual.py."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from lut_renderer_amd import _native, frames
from lut_renderer_amd.engine import LutEngine, check_dual_options, dual_side
from lut_renderer_amd.params import ProcessingParams, VideoInfo

ROOT = Path(__file__).resolve().parent.parent


def _planes(fmt_depth, csx, csy, w=16, h=8, frames_=None):
    dt = torch.uint8 if fmt_depth <= 8 else torch.int16
    lead = () if frames_ is None else (frames_,)
    cs = ((h + (1 << csy) - 1) >> csy, (w + (1 << csx) - 1) >> csx)
    return [torch.zeros(lead + (h, w), dtype=dt), torch.zeros(lead + cs, dtype=dt), torch.zeros(lead + cs, dtype=dt)]


# ------------------------------------------------------------------ the symbol
def test_symbol_is_declared_exported_and_bound():
    header = (ROOT / "include" / "lutr.h").read_text()
    assert "int lutr_apply_yuv_dual(lutr_ctx *ctx, const lutr_yuv_params *p, int fmt_out2, int interp, int w, int h, int nframes," \
        in header
    assert "const lutr_planes *src, const lutr_planes *dst, const lutr_planes *dst2, int row0, int rows);" in header
    assert "lutr_apply_yuv_dual" in _native.SYMBOLS
    nm = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True).stdout
    assert " T lutr_apply_yuv_dual\n" in nm
    lib = _native.load()
    assert len(lib.lutr_apply_yuv_dual.argtypes) == 12
    # no context, no planes: refused before anything touches a device
    assert lib.lutr_apply_yuv_dual(None, None, _native.fmt_code(8, 1, 1), 2, 16, 16, 1, None, None, None, 0, 16) == _native.EINVAL
    assert b"null" in lib.lutr_last_error()


# ------------------------------------------------------------------ LutEngine.apply_yuv_dual, before the engine is touched
NAMES = dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", out2_pix_fmt="yuv420p")


@pytest.mark.parametrize("side", ["pix_fmt", "out_pix_fmt", "out2_pix_fmt"])
@pytest.mark.parametrize("name,word", [("gbrp10le", "RGB"), ("rgb24", "RGB"), ("gbrpf32le", "RGB"), ("nv12", "semi-planar or packed"),
                                       ("p010le", "semi-planar or packed"), ("uyvy422", "semi-planar or packed"),
                                       ("y210le", "semi-planar or packed"), ("vuyx", "semi-planar or packed")])
def test_a_side_that_is_not_planar_yuv_is_a_value_error(side, name, word):
    src = _planes(10, 1, 1)
    kw = {**NAMES, side: name}
    with pytest.raises(ValueError, match=f"planar YUV on every side: {side} '{name}' is an? {word}"):
        LutEngine.apply_yuv_dual(object(), src, **kw)
    with pytest.raises(ValueError, match="planar YUV on every side"):
        check_dual_options(kw["pix_fmt"], kw["out_pix_fmt"], kw["out2_pix_fmt"])


def test_names_that_are_no_format_and_a_missing_second_format():
    src = _planes(10, 1, 1)
    with pytest.raises(ValueError, match="unsupported pixel format 'yuv440p'"):
        LutEngine.apply_yuv_dual(object(), src, **{**NAMES, "out2_pix_fmt": "yuv440p"})
    with pytest.raises(ValueError, match="unsupported bit depth"):
        LutEngine.apply_yuv_dual(object(), src, **{**NAMES, "out2_pix_fmt": "yuv420p17le"})
    with pytest.raises(ValueError, match="needs out2_pix_fmt"):
        LutEngine.apply_yuv_dual(object(), src, **{**NAMES, "out2_pix_fmt": None})
    with pytest.raises(TypeError):
        LutEngine.apply_yuv_dual(object(), src, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le")
    assert dual_side("yuvj420p", "pix_fmt").name == "yuv420p"        # yuvj* is read as yuv*, as apply_lut hands it over
    fin, f1, f2 = check_dual_options("yuv420p10le", None, "yuv444p12le")
    assert (f1.name, f2.depth, f2.csx, f2.csy) == ("yuv420p10le", 12, 0, 0)


@pytest.mark.parametrize("key,value,message", [
    ("dither", "error_diffusion", "error-diffusion dither is not supported with a second output"),
    ("dither", "none", "apply_yuv_dual takes no 'dither'"),
    ("chroma_loc", "left", r"sited chroma resampling \(chroma_loc\) is not supported with a second output"),
    ("out_size", (8, 4), r"a resize \(out_size\) is not supported with a second output"),
])
def test_options_of_apply_yuv_that_the_dual_pass_does_not_take(key, value, message):
    with pytest.raises(ValueError, match=message):
        LutEngine.apply_yuv_dual(object(), _planes(10, 1, 1), **NAMES, **{key: value})
    with pytest.raises(TypeError, match="unexpected keyword argument 'bogus'"):
        LutEngine.apply_yuv_dual(object(), _planes(10, 1, 1), **NAMES, bogus=1)


def test_wrong_plane_shapes_and_dtypes():
    src = _planes(10, 1, 1)
    good1, good2 = _planes(10, 1, 0), _planes(8, 1, 1)
    with pytest.raises(ValueError, match="expected three planes"):
        LutEngine.apply_yuv_dual(object(), src[:2], **NAMES)
    with pytest.raises(ValueError, match="source plane 1 is"):
        LutEngine.apply_yuv_dual(object(), _planes(10, 1, 0), **NAMES)               # 4:2:2 planes named 4:2:0
    with pytest.raises(ValueError, match="source plane 0: 'yuv420p10le' takes 16-bit integer samples"):
        LutEngine.apply_yuv_dual(object(), _planes(8, 1, 1), **NAMES)
    with pytest.raises(ValueError, match=r"destination plane 1 is \(4, 8\), 'yuv422p10le' at 16x8 needs \(8, 8\)"):
        LutEngine.apply_yuv_dual(object(), src, _planes(10, 1, 1), good2, **NAMES)
    with pytest.raises(ValueError, match="second destination plane 0: 'yuv420p' takes 8-bit integer samples"):
        LutEngine.apply_yuv_dual(object(), src, good1, _planes(10, 1, 1), **NAMES)
    with pytest.raises(ValueError, match=r"second destination plane 1 is \(8, 8\), 'yuv420p' at 16x8 needs \(4, 8\)"):
        LutEngine.apply_yuv_dual(object(), src, good1, _planes(8, 1, 0), **NAMES)
    with pytest.raises(ValueError, match="second destination plane 0: 'yuv420p' takes 8-bit integer samples"):
        LutEngine.apply_yuv_dual(object(), src, None, [t.float() for t in good2], **NAMES)
    # everything in order: the first thing that fails is the engine itself (object() has no device)
    with pytest.raises(AttributeError):
        LutEngine.apply_yuv_dual(object(), src, good1, good2, **NAMES)


def test_the_group_checks_the_same_things_first():
    from lut_renderer_amd.multigpu import LutEngineGroup

    class _Lock:
        def __enter__(self): return self
        def __exit__(self, *exc): return False

    class _Fake:
        _lock = _Lock()
    with pytest.raises(ValueError, match="the group owns the row partition"):
        LutEngineGroup.apply_yuv_dual(_Fake(), _planes(10, 1, 1), **NAMES, row0=0)
    with pytest.raises(ValueError, match="planar YUV on every side"):
        LutEngineGroup.apply_yuv_dual(_Fake(), _planes(10, 1, 1), **{**NAMES, "out2_pix_fmt": "nv12"})
    with pytest.raises(ValueError, match="not supported with a second output"):
        LutEngineGroup.apply_yuv_dual(_Fake(), _planes(10, 1, 1), **NAMES, chroma_loc="left")


# ------------------------------------------------------------------ apply_lut(second_pix_fmt=)
def test_apply_lut_rejections_before_any_gpu_work():
    from lut_renderer_amd.api import apply_lut
    y, cb, cr = frames.natural_yuv(16, 8, 10, 1, 1)
    base = dict(cube=None, pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", engine=object())
    for kw, message in ((dict(second_pix_fmt="nv12"), "out2_pix_fmt 'nv12' is a semi-planar or packed"),
                        (dict(second_pix_fmt="uyvy422"), "out2_pix_fmt 'uyvy422' is a semi-planar or packed"),
                        (dict(second_pix_fmt="gbrp"), "out2_pix_fmt 'gbrp' is an RGB format"),
                        (dict(second_pix_fmt="yuv420p", zscale_dither="error_diffusion"), "dither is not supported with a second"),
                        (dict(second_pix_fmt="yuv420p", chroma_loc="left"), "chroma_loc.* is not supported with a second output"),
                        (dict(second_pix_fmt="yuv420p", resolution="8x4"), "resize .* is not supported with a second output")):
        with pytest.raises(ValueError, match=message):
            apply_lut((y, cb, cr), **base, **kw)
    g, b, r = frames.natural_rgb(16, 8, 8, k=1)
    with pytest.raises(ValueError, match="pix_fmt 'gbrp' is an RGB format"):
        apply_lut((g, b, r), cube=None, pix_fmt="gbrp", out_pix_fmt="yuv420p", second_pix_fmt="yuv422p", engine=object())
    with pytest.raises(ValueError, match="pix_fmt 'rgb24' is an RGB format"):
        apply_lut(np.zeros((8, 16, 3), np.uint8), cube=None, pix_fmt="rgb24", out_pix_fmt="yuv420p", second_pix_fmt="yuv422p",
                  engine=object())
    with pytest.raises(ValueError, match="pix_fmt 'gbrpf32le' is an RGB format"):
        apply_lut([np.zeros((8, 16), np.float32)] * 3, cube=None, pix_fmt="gbrpf32le", out_pix_fmt="yuv420p",
                  second_pix_fmt="yuv422p", engine=object())
    with pytest.raises(ValueError, match="pix_fmt 'nv12' is a semi-planar or packed"):
        apply_lut((y, cb), cube=None, pix_fmt="nv12", second_pix_fmt="yuv420p", engine=object())


def test_dual_call_for_keeps_the_recorded_call_and_adds_the_second_format():
    from lut_renderer_amd.api import dual_call_for, engine_call_for
    from lut_renderer_amd.plan import resolve_lut_plan
    info = VideoInfo(width=16, height=8, pix_fmt="yuvj420p", bit_depth=8, colorspace="bt709", color_range="pc")
    plan = resolve_lut_plan(ProcessingParams(), "look.cube", info)
    kw = engine_call_for(plan, "yuvj420p", "yuv422p10le")
    dual = dual_call_for(dict(kw, dither="none"), "yuvj420p")
    assert dual == {**kw, "out2_pix_fmt": "yuv420p"} and "dither" not in dual
    assert dual["range_src"] == "pc" and dual["lut_depth"] == 8          # the full-range prologue travels unchanged


# ------------------------------------------------------------------ the CLI
def _args(cube, *extra):
    from lut_renderer_amd.cli import build_parser
    return build_parser().parse_args(["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", "yuv420p10le", "--out-pix-fmt",
                                      "yuv422p10le", "--cube", str(cube), *extra])


def test_cli_flags(cube_dir):
    from lut_renderer_amd.cli import plan_from_args
    cube = cube_dir / "log709_33.cube"
    plain = _args(cube)
    assert plain.second_output is None and plain.second_pix_fmt is None
    _, kw, w, h = plan_from_args(plain)
    assert "out2_pix_fmt" not in kw and (kw["pix_fmt"], kw["out_pix_fmt"], w, h) == ("yuv420p10le", "yuv422p10le", 16, 8)
    both = _args(cube, "--second-output", "c.yuv", "--second-pix-fmt", "yuv420p")
    assert (both.second_output, both.second_pix_fmt) == ("c.yuv", "yuv420p")
    _, kw2, _, _ = plan_from_args(both)
    assert kw2 == {**kw, "out2_pix_fmt": "yuv420p"}
    for extra in (("--second-output", "c.yuv"), ("--second-pix-fmt", "yuv420p")):
        with pytest.raises(ValueError, match="--second-output and --second-pix-fmt go together"):
            plan_from_args(_args(cube, *extra))
    with pytest.raises(ValueError, match="--second-output is a file or FIFO, not '-'"):
        plan_from_args(_args(cube, "--second-output", "-", "--second-pix-fmt", "yuv420p"))
    for same in ("b", "./b", "sub/../b"):
        with pytest.raises(ValueError, match="--second-output names the same file as -o"):
            plan_from_args(_args(cube, "--second-output", same, "--second-pix-fmt", "yuv420p"))
    for extra, message in ((("--second-pix-fmt", "nv12"), "semi-planar or packed"),
                           (("--second-pix-fmt", "yuv420p", "--zscale-dither", "error_diffusion"), "dither is not supported"),
                           (("--second-pix-fmt", "yuv420p", "--out-size", "8x4"), "resize .* is not supported"),
                           (("--second-pix-fmt", "yuv420p10le", "--chroma-loc", "left"), "not")):
        with pytest.raises(ValueError, match=message):
            plan_from_args(_args(cube, "--second-output", "c.yuv", *extra))


def test_cli_refuses_before_it_opens_a_device(cube_dir, tmp_path):
    """The process contract on a bad option pair: `Error: ...` on stdout and exit code 1, no output file made."""
    import sys
    src = tmp_path / "in.yuv"
    src.write_bytes(bytes(16 * 8 * 3))
    r = subprocess.run([sys.executable, "-m", "lut_renderer_amd.cli", "-i", str(src), "-o", str(tmp_path / "o.yuv"), "--size", "16x8",
                        "--pix-fmt", "yuv420p10le", "--cube", str(cube_dir / "log709_33.cube"), "--second-output", "-",
                        "--second-pix-fmt", "yuv420p"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 1 and "Error: --second-output is a file or FIFO, not '-'" in r.stdout
    assert not (tmp_path / "o.yuv").exists()


# ------------------------------------------------------------------ the command layer
def test_engine_command_renders_the_flags_only_when_given():
    from lut_renderer_amd.command import _master_params, engine_command
    master = _master_params(ProcessingParams(video_codec="libx264", crf="18"))
    info = VideoInfo(width=1920, height=1080, bit_depth=10, pix_fmt="yuv420p10le", color_range="tv", colorspace="bt709",
                     fps=25.0, duration=4.0)
    plain = engine_command(Path("-"), Path("-"), master, Path("look.cube"), info, python_bin="python3")
    # the argv of the professional master stage as it has always been rendered
    assert plain == ["python3", "-m", "lut_renderer_amd.cli", "-y", "-i", "-", "-o", "-", "--size", "1920x1080", "--pix-fmt",
                     "yuv420p10le", "--out-pix-fmt", "yuv422p10le", "--cube", "look.cube", "--interp", "tetrahedral",
                     "--input-matrix", "auto", "--output-tags", "bt709", "--colorspace", "bt709", "--color-range", "tv",
                     "--fps", "25"]
    assert engine_command(Path("-"), Path("-"), master, Path("look.cube"), info, python_bin="python3", second_output=None,
                          second_pix_fmt=None) == plain
    dual = engine_command(Path("-"), Path("-"), master, Path("look.cube"), info, python_bin="python3",
                          second_output=Path("delivery.yuv"), second_pix_fmt="yuv420p")
    assert dual == plain + ["--second-output", "delivery.yuv", "--second-pix-fmt", "yuv420p"]
    # the CLI resolves what the command rendered
    from lut_renderer_amd.cli import build_parser, plan_from_args
    _, kw, _, _ = plan_from_args(build_parser().parse_args(dual[3:]))
    assert (kw["out_pix_fmt"], kw["out2_pix_fmt"]) == ("yuv422p10le", "yuv420p")
    for kwargs, message in ((dict(second_output=Path("d.yuv")), "go together"), (dict(second_pix_fmt="yuv420p"), "go together"),
                            (dict(second_output=Path("-"), second_pix_fmt="yuv420p"), "not '-'"),
                            (dict(second_output=Path("d.yuv"), second_pix_fmt="nv12"), "semi-planar or packed"),
                            (dict(second_output=Path("d.yuv"), second_pix_fmt="yuv420p", chroma_loc="left"), "chroma_loc")):
        with pytest.raises(ValueError, match=message):
            engine_command(Path("-"), Path("-"), master, Path("look.cube"), info, python_bin="python3", **kwargs)
    rgb = VideoInfo(width=64, height=32, bit_depth=8, pix_fmt="rgb24", fps=25.0)
    with pytest.raises(ValueError, match="pix_fmt 'rgb24' is an RGB format"):
        engine_command(Path("-"), Path("-"), ProcessingParams(video_codec="libx264", pix_fmt="yuv420p"), Path("look.cube"), rgb,
                       python_bin="python3", second_output=Path("d.yuv"), second_pix_fmt="yuv422p")


# ------------------------------------------------------------------ the second ring of HostPipeline
@pytest.mark.parametrize("w,h,master,delivery", [(7, 5, 7 * 5 * 2 + 2 * 4 * 5 * 2, 7 * 5 + 2 * 4 * 3),
                                                 (8, 6, 8 * 6 * 2 + 2 * 4 * 6 * 2, 8 * 6 + 2 * 4 * 3)])
def test_second_ring_layout(w, h, master, delivery):
    from lut_renderer_amd.stream import dual_layout, yuv_layout
    assert yuv_layout("yuv422p10le", w, h).frame_bytes == master
    second = dual_layout("yuv420p10le", "yuv422p10le", "yuv420p", w, h)
    assert second.frame_bytes == delivery and second.itemsize == 1
    assert second.plane_shapes == [(h, w), ((h + 1) // 2, (w + 1) // 2), ((h + 1) // 2, (w + 1) // 2)]
    views = second.plane_views(torch.zeros(3 * delivery, dtype=torch.uint8), 3)
    assert [tuple(v.shape) for v in views] == [(3,) + s for s in second.plane_shapes]
    assert views[2].storage_offset() == w * h + ((h + 1) // 2) * ((w + 1) // 2) and views[0].stride(0) == delivery
    assert dual_layout("yuv420p10le", "yuv422p10le", None, w, h) is None
    with pytest.raises(ValueError, match="semi-planar or packed"):
        dual_layout("yuv420p10le", "yuv422p10le", "nv12", w, h)
    with pytest.raises(ValueError, match="resize"):
        dual_layout("yuv420p10le", "yuv422p10le", "yuv420p", w, h, out_size=(4, 4))
    with pytest.raises(ValueError, match="dither"):
        dual_layout("yuv420p10le", "yuv422p10le", "yuv420p", w, h, apply_kw={"dither": "error_diffusion"})


def test_run_hands_both_outputs_of_a_batch_over_the_second_first():
    """`HostPipeline.run` on a stand-in that needs no device: per batch `drain2` then `drain`, the same frame counts; the drains go
    together (ValueError otherwise); when `drain` raises, `drain2` has taken that batch already."""
    from types import SimpleNamespace
    from lut_renderer_amd.stream import HostPipeline, yuv_layout

    class _Event:
        def synchronize(self): pass

    slots, batch = 2, 2
    fin, fout, fout2 = (yuv_layout(n, 8, 6) for n in ("yuv420p10le", "yuv422p10le", "yuv420p"))
    bufs = {k: [np.zeros(batch * f.frame_bytes, np.uint8) for _ in range(slots)] for k, f in (("i", fin), ("o", fout), ("o2", fout2))}
    fake = SimpleNamespace(slots=slots, batch=batch, fin=fin, fout=fout, fout2=fout2, e_out=[_Event() for _ in range(slots)],
                           host_in=lambda s: bufs["i"][s], host_out=lambda s: bufs["o"][s], host_out2=lambda s: bufs["o2"][s],
                           _submit=lambda slot, n: None)
    calls = []
    done = HostPipeline.run(fake, lambda buf, n: n, lambda buf, n: calls.append(("1", n, len(buf))), total_frames=5,
                            drain2=lambda buf, n: calls.append(("2", n, len(buf))))
    assert done == 5
    assert calls == [(k, n, n * f.frame_bytes) for n in (2, 2, 1) for k, f in (("2", fout2), ("1", fout))]
    with pytest.raises(ValueError, match="drain2 goes with second_pix_fmt"):
        HostPipeline.run(fake, lambda buf, n: n, lambda buf, n: None, total_frames=1)
    fake.fout2 = None
    with pytest.raises(ValueError, match="drain2 goes with second_pix_fmt"):
        HostPipeline.run(fake, lambda buf, n: n, lambda buf, n: None, total_frames=1, drain2=lambda buf, n: None)
    fake.fout2, seen = fout2, []

    def broken(buf, n):
        raise BrokenPipeError("the first output went away")
    with pytest.raises(BrokenPipeError):
        HostPipeline.run(fake, lambda buf, n: n, broken, total_frames=4, drain2=lambda buf, n: seen.append(n))
    assert seen == [2]


def test_two_output_side_and_option_refusals_keep_their_words():
    """Every refusal of `dual_side`, `check_dual_options` and `refuse_dual_keywords`, whole, and the order they fire in."""
    from lut_renderer_amd.engine import refuse_dual_keywords
    head = "the two-output pass takes planar YUV on every side: out2_pix_fmt"
    for name, tail in (("nv12", "is a semi-planar or packed container"), ("uyvy422", "is a semi-planar or packed container"),
                       ("vuya", "is a semi-planar or packed container"), ("v210", "is a v210 container"),
                       ("rgb24", "is an RGB format"), ("gbrap10le", "is an RGB format"), ("gbrpf32le", "is an RGB format")):
        with pytest.raises(ValueError) as e:
            dual_side(name, "out2_pix_fmt")
        assert str(e.value) == f"{head} '{name}' {tail}"
    for name in (None, ""):
        with pytest.raises(ValueError) as e:
            dual_side(name, "out2_pix_fmt")
        assert str(e.value) == "the two-output pass needs out2_pix_fmt"
    with pytest.raises(ValueError, match="unsupported pixel format 'v410'"):
        dual_side("v410", "pix_fmt")                              # (v210's relatives are no name at all here)
    assert dual_side("yuvj420p", "pix_fmt").name == "yuv420p" and dual_side("yuva444p12le", "pix_fmt").alpha
    # a bad side goes before a bad option, and the options in the order dither, chroma_loc, out_size
    with pytest.raises(ValueError, match="^the two-output pass takes planar YUV on every side: pix_fmt 'nv12'"):
        check_dual_options("nv12", "p010le", "rgb24", "error_diffusion", "left", (8, 4))
    with pytest.raises(ValueError, match="^the two-output pass takes planar YUV on every side: out_pix_fmt 'p010le'"):
        check_dual_options("yuv420p", "p010le", "rgb24", "error_diffusion", "left", (8, 4))
    for args, text in ((("blue_noise", "left", (8, 4)), "error-diffusion dither is not supported with a second output"),
                       (("none", "left", (8, 4)), "sited chroma resampling (chroma_loc) is not supported with a second output"),
                       (("none", None, (8, 4)), "a resize (out_size) is not supported with a second output")):
        with pytest.raises(ValueError) as e:
            check_dual_options("yuv420p", None, "yuv422p10le", *args)
        assert str(e.value) == text
    with pytest.raises(ValueError) as e:
        refuse_dual_keywords(dict(width=16, resize_chunk=2, out_size=None))
    assert str(e.value) == "a resize (out_size) is not supported with a second output: apply_yuv_dual takes no 'out_size'"
    with pytest.raises(ValueError) as e:
        refuse_dual_keywords(dict(width=16, resize_chunk=2))
    assert str(e.value) == "a resize (out_size) is not supported with a second output: apply_yuv_dual takes no 'resize_chunk'"
    with pytest.raises(ValueError) as e:
        refuse_dual_keywords(dict(width=16))
    assert str(e.value) == "a packed side (width) is not supported with a second output: apply_yuv_dual takes no 'width'"
    refuse_dual_keywords(dict(dst2=None, out2_pix_fmt="yuv420p", interp="nearest"))
