"""The case table, the sources and the destination layout shared by tests/_gpu_stride_worker.py (a child process that applies on
the GPU under LUTR_MAX_BLOCKS and computes no reference) and tests/test_gpu_stride_trips.py (the parent, which recomputes every
reference on the CPU) -- TEST INFRASTRUCTURE ONLY.  Plain numpy: nothing here touches torch or the GPU.

Sources come from the helpers of each family's own GPU test (`_src`, `_matte`, `_alpha_values`), so that the parent can hand the
same arrays to that test's `_want`."""
from __future__ import annotations

from pathlib import Path

import numpy as np

from lut_renderer_amd import cube, frames
from lut_renderer_amd.cdl import read_cdl
from lut_renderer_amd.v210 import to_planar as v210_to_planar, to_v210
from lut_renderer_amd.semiplanar import to_semi
from tests import _deep_content as dc
from tests import _rgbf_twin
from tests.test_gpu_alpha import _alpha_values
from tests.test_gpu_matte import _matte
from tests.test_gpu_stack import LAYOUTS, _src

F = np.float32
GOLDEN = Path(__file__).resolve().parent / "golden"
STAGES = "lut1d,cdl,lut3d"
#: columns of the padded rows of a ragged case, and the spare columns behind every other destination row
RAGGED_COLS, SPARE_COLS = 160, 8

_res = {}


def yuv_name(depth, lay, alpha=False):
    return f"yuv{'a' if alpha else ''}{lay}p" + ("" if depth == 8 else f"{depth}le")


def resources():
    """The lattice, the 1D LUT (with lut1d's mode) and the CDL every case uses, built once per process: dict(lut, l1, cdl)."""
    if not _res:
        _res.update(lut=dc.make_lut("u33", None)[0], l1=(cube.read_lut1d(GOLDEN / "lut1d" / "gamma1024.cube"), "cubic"),
                    cdl=read_cdl(GOLDEN / "cdl" / "shot.cc"))
    return _res


# ------------------------------------------------------------------ cases
# kind: which call the worker makes and which reference the parent builds; gs: the kernel family whose `[lutr gs]` line carries the
# case's regime (a column split prints a second line, for the generic tail); (w, h, nf): the frame and the batch; variant: the
# engine's set_variant; env: per-launch knobs set in the child around the call; pad: the rows of source and destination are
# RAGGED_COLS samples wide (aligned rows under a ragged width); kernel: what `last_kernel` must start with, and `both` a second
# name it must contain.
def _c(cid, kind, gs, w, h, nf, kernel, variant="auto", env=None, pad=False, both=None, **kw):
    return dict(id=cid, kind=kind, gs=gs, w=w, h=h, nf=nf, kernel=kernel, variant=variant, env=env or {}, pad=pad, both=both, **kw)


def _stack(cid, gs, w, h, nf, kernel, din=10, dout=10, a="420", b="422", stages=STAGES, strength=None, matte=None, **kw):
    """matte: None or (depth, still, invert)."""
    return _c(cid, "stack", gs, w, h, nf, kernel, din=din, dout=dout, a=a, b=b, stages=stages, strength=strength, matte=matte, **kw)


def _cases():
    V, X, M = "k_yuv_stack_vec", "k_yuv_stack_mix_vec", "k_yuv_stack_matte_vec"
    out = [
        # the stack family's vector kernels
        _stack("stack-lds", V, 136, 36, 3, V + "<1,1,1,1,1,0,0,1>"),
        _stack("stack-global", V, 136, 36, 3, V + "<1,1,1,1,1,0,0,0>", env={"LUTR_STACK_LDS": "0"}),
        _stack("stack-16to8", V, 136, 36, 4, V + "<1,0,1,1,1,0,0,0>", din=16, dout=8),
        _stack("stack-444to420-tri", V, 136, 36, 4, V + "<0,0,0,0,1,1,1,1>", din=8, dout=8, a="444", b="420",
               stages="lut1d,cdl,lut3d:trilinear"),
        _stack("stack-444", V, 136, 36, 2, V + "<1,1,0,0,0,0,0,1>", a="444", b="444"),
        _stack("mix-420to422", X, 136, 36, 3, X + "<1,1,1,1,1,0,0,1>", strength=[0.37, 0.0, 1.0]),
        _stack("mix-444", X, 136, 36, 3, X + "<1,1,0,0,0,0,0,1>", a="444", b="444", strength=[1.0, 0.37, 0.0]),
        _stack("matte-10", M, 136, 36, 3, M + "<1,1,1,1,1,1,0,0,1>", strength=[0.8, 0.0, 1.0], matte=(10, False, False)),
        _stack("matte-8-beside-16-inverted", M, 136, 36, 3, M + "<1,1,0,1,1,1,0,0,0>", din=16, dout=16, strength=[1.0, 0.6, 0.0],
               matte=(8, False, True)),
        _stack("matte-still", M, 136, 36, 3, M + "<1,1,1,1,1,1,0,0,1>", strength=[0.5, 1.0, 0.0], matte=(10, True, False)),
        # their generic forms
        _stack("stack-generic", "k_yuv_stack_generic", 67, 21, 3, "k_yuv_stack_generic[", variant="generic"),
        _stack("mix-generic", "k_yuv_stack_mix_generic", 67, 21, 3, "k_yuv_stack_mix_generic[", variant="generic",
               strength=[0.0, 1.0, 0.37]),
        _stack("matte-generic", "k_yuv_stack_matte_generic", 67, 21, 3, "k_yuv_stack_matte_generic[", variant="generic",
               strength=[0.8, 0.0, 1.0], matte=(10, False, False)),
        # a ragged width on padded rows, several frames: the vector kernel up to column 136, the generic one for three columns
        _stack("stack-ragged", V, 139, 36, 3, V + "<1,1,1,1,1,0,0,1>", pad=True, both="+k_yuv_stack_generic["),
        _stack("matte-ragged-8-beside-10", M, 139, 36, 3, M + "<1,1,0,1,1,1,0,0,1>", pad=True, both="+k_yuv_stack_matte_generic[",
               strength=[0.8, 0.0, 1.0], matte=(8, False, False)),
        # 1D LUT
        _c("l1d-lds", "lut1d", "k_yuv_l1d_vec", 136, 36, 3, "k_yuv_l1d_vec<1,1,1,1,1,0,2>", mode="tetrahedral"),
        _c("l1d-global", "lut1d", "k_yuv_l1d_vec", 136, 36, 3, "k_yuv_l1d_vec<1,1,1,1,1,0,2>", mode="tetrahedral",
           env={"LUTR_L1D_LDS": "0"}),
        _c("l1d-alone", "lut1d", "k_yuv_l1d_vec", 136, 36, 3, "k_yuv_l1d_vec<1,1,1,1,1,0,-1>", mode=None),
        _c("l1d-rgb", "rgb_l1d", "k_rgb_l1d", 136, 36, 2, "k_rgb_l1d<1>"),
        _c("l1d-rgb-ragged", "rgb_l1d", "k_rgb_l1d", 67, 21, 2, "k_rgb_l1d<1>+k_rgb_l1d_generic", pad=True),
        # alpha (apply_yuv on yuva* frames: the colour planes are checked as well)
        _c("alpha-copy", "alpha", "k_alpha_vec", 136, 36, 3, "+k_alpha_vec<1,1>", src_alpha=True, dout=10),
        _c("alpha-10to8", "alpha", "k_alpha_vec", 136, 36, 3, "+k_alpha_vec<1,0>", src_alpha=True, dout=8),
        _c("alpha-fill", "alpha", "k_alpha_fill", 136, 36, 3, "+k_alpha_fill", src_alpha=False, dout=10),
        _c("alpha-generic", "alpha", "k_alpha_generic", 67, 21, 2, "+k_alpha_generic", src_alpha=True, dout=10),
        # for_each_block generics: a row shard with row0 > 0, and pass 1 of error-diffusion dither (whole_frames)
        _c("yuv-generic-shard", "yuv", "k_yuv_generic", 67, 21, 6, "k_yuv_generic", variant="generic", shard=(4, 12)),
        _c("dither-pass1", "dither", "k_yuv_float", 67, 21, 3, "k_yuv_float+k_dither_ed"),
        # generics with a walk of their own
        _c("rgb-generic", "rgb", "k_rgb_generic", 67, 21, 2, "k_rgb_generic", variant="generic"),
        _c("packed-generic", "packed", "k_packed_generic", 67, 21, 2, "k_packed_generic", variant="generic", fmt="rgb24"),
        _c("rgbf-generic", "rgbf", "k_rgbf_generic", 67, 21, 2, "k_rgbf_generic", variant="generic"),
        _c("rgbaf-premul-generic", "rgbaf", "k_rgbaf_premul_generic", 67, 21, 2, "k_rgbaf_premul_generic", variant="generic"),
        _c("v210-generic", "v210", "k_yuv_v210_generic", 67, 21, 5, "k_yuv_v210_generic", variant="generic"),
        _c("semi-generic", "semi", "k_yuv_semi_generic", 67, 21, 3, "k_yuv_semi_generic", variant="generic", fmt="p010le"),
    ]
    return out


CASES = _cases()
BY_ID = {c["id"]: c for c in CASES}


# ------------------------------------------------------------------ sources
def _frames(per_frame):
    """[frame][plane] -> [plane] stacked over frames."""
    return [np.stack([f[i] for f in per_frame]) for i in range(len(per_frame[0]))]


def source(case):
    """The host arrays of a case, every one with a leading frame axis: dict(src=[planes], matte=array or None)."""
    w, h, nf, kind = case["w"], case["h"], case["nf"], case["kind"]
    matte = None
    if kind == "stack":
        src = _src("natural", w, h, case["din"], case["a"], k=3, nf=nf)
        if case["matte"]:
            depth, still, _ = case["matte"]
            matte = _matte(w, h, depth, seed=5) if still else _matte(w, h, depth, nf=nf)
    elif kind == "lut1d":
        src = _src("natural", w, h, 10, "420", k=3, nf=nf)
    elif kind == "rgb_l1d":
        src = _frames([frames.make_rgb("natural", w, h, 10, k=1 + i) for i in range(nf)])
    elif kind == "alpha":
        src = _frames([frames.natural_yuv(w, h, 10, 1, 1, k=3 + i) + ([_alpha_values(w, h, 10, k=i)] if case["src_alpha"] else [])
                       for i in range(nf)])
    elif kind in ("yuv", "dither"):
        src = _frames([frames.natural_yuv(w, h, 10, 1, 1, k=i) for i in range(nf)])
    elif kind == "rgb":
        src = _frames([frames.make_rgb("natural", w, h, 10, k=4 + i) for i in range(nf)])
    elif kind == "packed":
        img = np.random.default_rng(0xC0BE + w).integers(0, 256, size=(nf, h, w, 3), dtype=np.uint8)
        ramp = (np.add.outer(np.arange(h), np.arange(w)) * 255 // (h + w)).astype(np.uint8)
        img[:, :, : w // 2, :] = ramp[None, :, : w // 2, None] ^ (img[:, :, : w // 2, :] & 7)
        src = [img]
    elif kind in ("rgbf", "rgbaf"):
        per = [_rgbf_twin.make_float("hdr", w, h, k=1 + i) for i in range(nf)]
        if kind == "rgbaf":
            rng = np.random.default_rng(w)
            for i, f in enumerate(per):
                alpha = rng.uniform(-0.1, 1.2, size=(h, w)).astype(F)
                alpha.reshape(-1)[:4] = (0.0, 1.0, 0.5, 1e-3)
                per[i] = [(p * np.clip(alpha, 0, 1)).astype(F) for p in f] + [alpha]
        src = _frames(per)
    elif kind == "v210":                       # the planar codes a v210 buffer really holds (tests/test_gpu_v210.py's _want)
        src = _frames([v210_to_planar(to_v210(frames.make_yuv("natural", w, h, 10, 1, 0, k=30 + i), w), w) for i in range(nf)])
    elif kind == "semi":
        src = _frames([frames.make_yuv("natural", w, h, 10, 1, 1, k=20 + i) for i in range(nf)])
    else:
        raise ValueError(kind)
    return dict(src=src, matte=matte)


def container(case, planes):
    """Planar codes [plane][nf, rows, cols] -> the arrays the call takes or gives on a side that is no planar one."""
    if case["kind"] == "v210":
        return [np.stack([to_v210([p[i] for p in planes], case["w"]) for i in range(case["nf"])])]
    if case["kind"] == "semi":
        return _frames([to_semi([p[i] for p in planes], case["fmt"]) for i in range(case["nf"])])
    return list(planes)


# ------------------------------------------------------------------ destinations
def out_layout(case):
    """Per destination plane: (shape [nf, rows, cols(, C)], dtype)."""
    w, h, nf, kind = case["w"], case["h"], case["nf"], case["kind"]

    def yuv(depth, lay, alpha=False, semi=False):
        ch, cw = frames.chroma_shape(w, h, *LAYOUTS[lay])
        dt = np.uint16 if depth > 8 else np.uint8
        if semi:
            return [((nf, h, w), dt), ((nf, ch, 2 * cw), dt)]
        return [((nf, h, w), dt)] + [((nf, ch, cw), dt)] * 2 + ([((nf, h, w), dt)] if alpha else [])

    if kind == "stack":
        return yuv(case["dout"], case["b"])
    if kind == "lut1d":
        return yuv(10, "422")
    if kind == "alpha":
        return yuv(case["dout"], "420", alpha=True)
    if kind in ("yuv", "dither"):
        return yuv(10, "420")
    if kind == "v210":
        return yuv(10, "422")
    if kind == "semi":
        return yuv(10, "420", semi=True)
    if kind in ("rgb_l1d", "rgb"):
        return [((nf, h, w), np.uint16)] * 3
    if kind == "packed":
        return [((nf, h, w, 3), np.uint8)]
    if kind == "rgbf":
        return [((nf, h, w), F)] * 3
    if kind == "rgbaf":
        return [((nf, h, w), F)] * 4
    raise ValueError(kind)


SENTINEL = {np.dtype(np.uint8): 0xA5, np.dtype(np.uint16): 0xFFFF, np.dtype(F): 1234.5}


def spare_shape(case, shape):
    """The tensor a destination plane of `shape` is a view of: one spare row a frame, and spare columns -- rows of RAGGED_COLS
    samples for a `pad` case, SPARE_COLS more than the plane's otherwise.  All of it is saved; all but the view keeps the sentinel."""
    cols = RAGGED_COLS if case["pad"] else shape[2] + SPARE_COLS
    return (shape[0], shape[1] + 1, cols) + tuple(shape[3:])
