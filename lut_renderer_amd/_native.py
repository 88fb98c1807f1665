"""ctypes binding of liblutr.so (the C-ABI declared in include/lutr.h).

The product path has no CPU fallback: if the shared library is missing or cannot be
loaded this module raises, and every compute entry point needs a GPU context.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "lib" / "liblutr.so"

# error codes of include/lutr.h
OK, ENOENT, EIO, ENOMEM, EINVAL, EILSEQ = 0, -2, -5, -12, -22, -84

INTERP = {"nearest": 0, "trilinear": 1, "tetrahedral": 2, "pyramid": 3, "prism": 4}
#: enum lutr_interp1d: lut1d's modes
INTERP1D = {"nearest": 0, "linear": 1, "cosine": 2, "cubic": 3, "spline": 4}
#: enum lutr_stage_kind: the stage kinds of a stack
STAGE_KINDS = {"lut3d": 1, "lut3d2": 2, "lut1d": 3, "cdl": 4}
#: the stage kinds of lutr_apply_yuv_stack_matrix alone: LUTR_STAGE_MATRIX
MATRIX_STAGE_KINDS = {"matrix": 5}
MATRIX = {"bt709": 0, "smpte170m": 1, "bt470bg": 1, "bt601": 1, "bt2020nc": 2, "bt2020c": 2}
RANGE = {"tv": 0, "pc": 1}
DITHER = {"none": 0, "error_diffusion": 1, "blue_noise": 2}
#: LUTR_RGB_STACK_YUV: the dst_kind of lutr_apply_rgb_stack for a YUV destination (a gbrp destination's is its depth)
RGB_STACK_YUV = 0
#: LUTR_INTERP_NONE: lutr_apply_rgb_to_yuv without lut3d
INTERP_NONE = -1
VARIANT = {"auto": 0, "generic": 1, "vec_global": 2, "vec_lds": 3}
PRECISION = {"strict": 0, "fast": 1, "fma32": 2}
#: enum lutr_chroma_loc: ffprobe's chroma_location names (None = replicate, lutr_apply_yuv's contract)
CHROMA_LOC = {"left": 1, "center": 2, "topleft": 3}
CHROMA_REPLICATE = 0
BCAST_FORCE_PEER_COPY = 1
#: enum lutr_resize_family
RESIZE_FAMILY = {"yuv": 0, "gbr": 1}

#: every symbol include/lutr.h declares (tests check the library exports each one)
SYMBOLS = (
    "lutr_version", "lutr_last_error",
    "lutr_cube_parse", "lutr_cube_free", "lutr_lut_parse", "lutr_lut_parse_ex", "lutr_ctx_set_prelut",
    "lutr_ctx_create", "lutr_ctx_destroy", "lutr_ctx_set_stream", "lutr_ctx_sync",
    "lutr_ctx_set_lut", "lutr_ctx_lut_alloc", "lutr_ctx_lut_device", "lutr_ctx_lut_seal",
    "lutr_lattice_bytes", "lutr_lut_broadcast", "lutr_lut_broadcast_ex",
    "lutr_apply_planar_rgb", "lutr_apply_packed_rgb", "lutr_apply_yuv", "lutr_apply_yuv_dither",
    "lutr_apply_yuv_sited", "lutr_yuv_constants_sited", "lutr_apply_yuv_xsub", "lutr_yuv_constants_xsub",
    "lutr_apply_rgb_to_yuv", "lutr_yuv_constants_rgb2yuv", "lutr_apply_yuv_to_rgb", "lutr_yuv_constants_yuv2rgb",
    "lutr_apply_planar_rgb_f32", "lutr_apply_rgbf_to_yuv", "lutr_apply_yuv_semi", "lutr_apply_yuv_packed",
    "lutr_apply_yuv_dual", "lutr_apply_yuv_v210", "lutr_alpha_plane", "lutr_ctx_set_lut2", "lutr_apply_yuv_chain",
    "lutr_apply_yuv_premul", "lutr_apply_planar_rgb_f32_premul", "lutr_cdl_table", "lutr_apply_yuv_cdl",
    "lutr_lut1d_parse", "lutr_lut1d_table", "lutr_ctx_set_lut1d", "lutr_apply_yuv_lut1d", "lutr_apply_planar_rgb_lut1d",
    "lutr_apply_yuv_stack", "lutr_apply_yuv_stack_mix", "lutr_apply_yuv_stack_matte",
    "lutr_apply_yuv_stack_matrix", "lutr_apply_rgb_stack", "lutr_apply_yuv_stack_to_rgb", "lutr_apply_yuv_stack_semi",
    "lutr_apply_yuv_stack_packed", "lutr_apply_yuv_stack_v210",
    "lutr_resize_filter", "lutr_resize_planes", "lutr_resize_plan", "lutr_dither_mask",
    "lutr_ctx_set_variant", "lutr_ctx_set_precision", "lutr_ctx_last_kernel", "lutr_ctx_tile_stats", "lutr_yuv_constants",
    "lutr_max_waves_knob", "lutr_max_blocks_knob",
)


def fmt_code(depth: int, csx: int, csy: int) -> int:
    """LUTR_FMT(depth, csx, csy)"""
    return depth | (csx << 8) | (csy << 9)


class YuvParams(C.Structure):
    """struct lutr_yuv_params"""
    _fields_ = [(name, C.c_int32) for name in (
        "fmt_in", "fmt_out", "lut_depth", "matrix_in", "matrix_out", "range_src", "range_in", "range_out")]


class Planes(C.Structure):
    """struct lutr_planes"""
    _fields_ = [("data", C.c_void_p * 3), ("stride", C.c_ssize_t * 3), ("frame_stride", C.c_int64 * 3)]


class YuvLayout(C.Structure):
    """struct lutr_yuv_layout: the container of one side of lutr_apply_yuv_semi"""
    _fields_ = [("semi", C.c_int32), ("swap", C.c_int32), ("shift", C.c_int32)]


class YuvPacking(C.Structure):
    """struct lutr_yuv_packing: the container of one side of lutr_apply_yuv_packed"""
    _fields_ = [("packed", C.c_int32), ("order", C.c_int32), ("shift", C.c_int32)]


class Packed(C.Structure):
    """struct lutr_packed"""
    _fields_ = [("data", C.c_void_p), ("stride", C.c_ssize_t), ("frame_stride", C.c_int64)]


class AlphaSrc(C.Structure):
    """struct lutr_alpha_src: where the alpha samples of lutr_alpha_plane's source are"""
    _fields_ = [("kind", C.c_int32), ("depth", C.c_int32), ("data", C.c_void_p), ("stride", C.c_ssize_t),
                ("frame_stride", C.c_int64), ("step", C.c_int32), ("offset", C.c_int32)]


class CdlStruct(C.Structure):
    """struct lutr_cdl: an ASC CDL"""
    _fields_ = [("slope", C.c_float * 3), ("offset", C.c_float * 3), ("power", C.c_float * 3), ("saturation", C.c_float)]


class StageStruct(C.Structure):
    """struct lutr_stage: one stage of a stack"""
    _fields_ = [("kind", C.c_int32), ("interp", C.c_int32)]


class MatteStruct(C.Structure):
    """struct lutr_matte: the matte plane of lutr_apply_yuv_stack_matte"""
    _fields_ = [("data", C.c_void_p), ("stride", C.c_ssize_t), ("frame_stride", C.c_int64), ("depth", C.c_int32),
                ("invert", C.c_int32)]


class RgbMatrixStruct(C.Structure):
    """struct lutr_rgb_matrix: the matrix of lutr_apply_yuv_stack_matrix"""
    _fields_ = [("m", C.c_float * 9), ("offset", C.c_float * 3)]


def rgb_matrix_struct(mtx) -> RgbMatrixStruct:
    """struct lutr_rgb_matrix from an `rgbmatrix.RgbMatrix` (its numbers rounded to float32, as the C-ABI carries them)."""
    st = RgbMatrixStruct()
    for i in range(9):
        st.m[i] = mtx.m[i]
    for i in range(3):
        st.offset[i] = mtx.offset[i]
    return st


def stage_array(stages):
    """lutr_stage[] from parsed stages ((kind name, lut3d mode name or None), ...; `formats.parse_stages`)."""
    arr = (StageStruct * len(stages))()
    for i, (kind, mode) in enumerate(stages):
        arr[i].kind = MATRIX_STAGE_KINDS[kind] if kind in MATRIX_STAGE_KINDS else STAGE_KINDS[kind]
        arr[i].interp = 0 if mode is None else INTERP[mode]
    return arr


def cdl_struct(cdl) -> CdlStruct:
    """struct lutr_cdl from a `cdl.Cdl` (its numbers rounded to float32, as the C-ABI carries them)."""
    st = CdlStruct()
    for i in range(3):
        st.slope[i], st.offset[i], st.power[i] = cdl.slope[i], cdl.offset[i], cdl.power[i]
    st.saturation = cdl.saturation
    return st


#: enum lutr_alpha_kind
ALPHA_NONE, ALPHA_INT, ALPHA_FLOAT = 0, 1, 2


def packed_code(bits: int, ncomp: int, ro: int, go: int, bo: int) -> int:
    """LUTR_PACKED(bits, ncomp, ro, go, bo)"""
    return bits | (ncomp << 8) | (ro << 12) | (go << 16) | (bo << 20)


#: FFmpeg names of the packed RGB formats lut3d takes -> (bits, components, R, G, B component index)
PACKED_FORMATS = {
    "rgb24": (8, 3, 0, 1, 2), "bgr24": (8, 3, 2, 1, 0),
    "rgba": (8, 4, 0, 1, 2), "rgb0": (8, 4, 0, 1, 2), "bgra": (8, 4, 2, 1, 0), "bgr0": (8, 4, 2, 1, 0),
    "argb": (8, 4, 1, 2, 3), "0rgb": (8, 4, 1, 2, 3), "abgr": (8, 4, 3, 2, 1), "0bgr": (8, 4, 3, 2, 1),
    "rgb48le": (16, 3, 0, 1, 2), "bgr48le": (16, 3, 2, 1, 0),
    "rgba64le": (16, 4, 0, 1, 2), "bgra64le": (16, 4, 2, 1, 0),
}


#: the packed RGB names whose fourth component is a real alpha -> its component index; the pad byte of rgb0 / bgr0 /
#: 0rgb / 0bgr is not alpha
PACKED_ALPHA = {"rgba": 3, "bgra": 3, "argb": 0, "abgr": 0, "rgba64le": 3, "bgra64le": 3}


#: semi-planar YUV formats -> (depth, csx, csy, swap: Cr first, shift of the code inside its container)
SEMI_FORMATS = {
    "nv12": (8, 1, 1, 0, 0), "nv21": (8, 1, 1, 1, 0), "nv16": (8, 1, 0, 0, 0),
    "p010le": (10, 1, 1, 0, 6), "p012le": (12, 1, 1, 0, 4), "p016le": (16, 1, 1, 0, 0),
    "p210le": (10, 1, 0, 0, 6), "p212le": (12, 1, 0, 0, 4), "p216le": (16, 1, 0, 0, 0),
}


#: packed 4:2:2 YUV formats -> (depth, group order: 0 Y0 Cb Y1 Cr, 1 Cb Y0 Cr Y1, 2 Y0 Cr Y1 Cb, shift of the code
#: inside its container)
PACKED_YUV_FORMATS = {
    "yuyv422": (8, 0, 0), "uyvy422": (8, 1, 0), "yvyu422": (8, 2, 0),
    "y210le": (10, 0, 6), "y212le": (12, 0, 4), "y216le": (16, 0, 0),
}


#: v210: 10-bit 4:2:2, three codes per 32-bit word, six luma samples per group of four words -> (depth,)
V210_FORMATS = {"v210": (10,)}


#: planar float RGB sources -> planes per frame (G, B, R[, A])
FLOAT_FORMATS = {"gbrpf32le": 3, "gbrapf32le": 4}


class LutrError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"liblutr error {code}: {message}")
        self.code = code
        self.message = message


_lib = None


def load() -> C.CDLL:
    """Load liblutr.so once; raise loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    path = Path(os.environ.get("LUTR_LIBRARY", LIB_PATH))
    if not path.exists():
        raise ImportError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C lut_renderer_amd/csrc`. The LUT engine has no CPU fallback.")
    lib = C.CDLL(str(path))
    vp, ci, cp = C.c_void_p, C.c_int, C.c_char_p
    lib.lutr_version.restype = cp
    lib.lutr_last_error.restype = cp
    lib.lutr_cube_parse.argtypes = [cp, C.POINTER(C.POINTER(C.c_float)), C.POINTER(ci), C.POINTER(C.c_float)]
    lib.lutr_lut_parse.argtypes = lib.lutr_cube_parse.argtypes
    lib.lutr_lut_parse_ex.argtypes = list(lib.lutr_cube_parse.argtypes) + [C.POINTER(C.POINTER(C.c_float)), C.POINTER(ci),
                                                                           C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.lutr_ctx_set_prelut.argtypes = [vp, C.POINTER(C.c_float), ci, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.lutr_cube_free.argtypes = [C.POINTER(C.c_float)]
    lib.lutr_cube_free.restype = None
    lib.lutr_ctx_create.argtypes = [ci, C.POINTER(vp)]
    lib.lutr_ctx_destroy.argtypes = [vp]
    lib.lutr_ctx_destroy.restype = None
    lib.lutr_ctx_set_stream.argtypes = [vp, vp]
    lib.lutr_ctx_sync.argtypes = [vp]
    lib.lutr_ctx_set_lut.argtypes = [vp, C.POINTER(C.c_float), ci, C.POINTER(C.c_float)]
    lib.lutr_ctx_lut_alloc.argtypes = [vp, ci, C.POINTER(C.c_float)]
    lib.lutr_ctx_lut_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    lib.lutr_ctx_lut_seal.argtypes = [vp]
    lib.lutr_lut_broadcast.argtypes = [C.POINTER(vp), ci, ci]
    lib.lutr_lut_broadcast_ex.argtypes = [C.POINTER(vp), ci, ci, C.c_uint]
    lib.lutr_lattice_bytes.argtypes = [ci]
    lib.lutr_lattice_bytes.restype = C.c_size_t
    lib.lutr_apply_planar_rgb.argtypes = [vp, ci, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_packed_rgb.argtypes = [vp, ci, ci, ci, ci, ci, C.POINTER(Packed), C.POINTER(Packed), ci, ci]
    lib.lutr_apply_yuv.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes),
                                   ci, ci]
    lib.lutr_apply_yuv_dither.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, ci, C.POINTER(Planes),
                                          C.POINTER(Planes)]
    lib.lutr_apply_yuv_sited.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, ci, C.POINTER(Planes),
                                         C.POINTER(Planes), ci, ci]
    lib.lutr_yuv_constants_sited.argtypes = [C.POINTER(YuvParams), ci, C.POINTER(C.c_float)]
    lib.lutr_apply_yuv_xsub.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes),
                                        ci, ci]
    lib.lutr_yuv_constants_xsub.argtypes = [C.POINTER(YuvParams), C.POINTER(C.c_float)]
    lib.lutr_apply_rgb_to_yuv.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Packed),
                                          C.POINTER(Planes), ci, ci]
    lib.lutr_yuv_constants_rgb2yuv.argtypes = [C.POINTER(YuvParams), C.POINTER(C.c_float)]
    lib.lutr_apply_yuv_to_rgb.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes),
                                          C.POINTER(Packed), ci, ci]
    lib.lutr_yuv_constants_yuv2rgb.argtypes = [C.POINTER(YuvParams), C.POINTER(C.c_float)]
    lib.lutr_apply_planar_rgb_f32.argtypes = [vp, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_rgbf_to_yuv.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes),
                                           ci, ci]
    lib.lutr_apply_yuv_semi.argtypes = [vp, C.POINTER(YuvParams), ci, C.POINTER(YuvLayout), C.POINTER(YuvLayout), ci, ci, ci,
                                        C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_yuv_packed.argtypes = [vp, C.POINTER(YuvParams), ci, C.POINTER(YuvPacking), C.POINTER(YuvPacking), ci, ci, ci,
                                          C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_yuv_v210.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_yuv_dual.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes),
                                        C.POINTER(Planes), ci, ci]
    lib.lutr_ctx_set_lut2.argtypes = [vp, C.POINTER(C.c_float), ci, C.POINTER(C.c_float)]
    lib.lutr_apply_yuv_chain.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_alpha_plane.argtypes = [vp, C.POINTER(AlphaSrc), ci, vp, C.c_ssize_t, C.c_int64, ci, ci, ci, ci, ci]
    lib.lutr_apply_yuv_premul.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(AlphaSrc),
                                          C.POINTER(Planes), ci, ci]
    lib.lutr_apply_planar_rgb_f32_premul.argtypes = [vp, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(AlphaSrc), C.POINTER(Planes),
                                                     ci, ci]
    lib.lutr_cdl_table.argtypes = [C.POINTER(CdlStruct), ci, ci, C.POINTER(C.c_float)]
    lib.lutr_apply_yuv_cdl.argtypes = [vp, C.POINTER(YuvParams), ci, C.POINTER(CdlStruct), ci, ci, ci, C.POINTER(Planes),
                                       C.POINTER(Planes), ci, ci]
    lib.lutr_lut1d_parse.argtypes = lib.lutr_cube_parse.argtypes
    lib.lutr_lut1d_table.argtypes = [C.POINTER(C.c_float), ci, C.POINTER(C.c_float), ci, ci, ci, C.POINTER(C.c_uint16)]
    lib.lutr_ctx_set_lut1d.argtypes = [vp, C.POINTER(C.c_float), ci, C.POINTER(C.c_float), ci]
    lib.lutr_apply_yuv_lut1d.argtypes = [vp, C.POINTER(YuvParams), ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_planar_rgb_lut1d.argtypes = [vp, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_yuv_stack.argtypes = [vp, C.POINTER(YuvParams), C.POINTER(StageStruct), ci, C.POINTER(CdlStruct), ci, ci, ci,
                                         C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_yuv_stack_mix.argtypes = [vp, C.POINTER(YuvParams), C.POINTER(StageStruct), ci, C.POINTER(CdlStruct), C.c_float,
                                             vp, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_yuv_stack_matte.argtypes = [vp, C.POINTER(YuvParams), C.POINTER(StageStruct), ci, C.POINTER(CdlStruct), C.c_float,
                                               vp, C.POINTER(MatteStruct), ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_yuv_stack_matrix.argtypes = [vp, C.POINTER(YuvParams), C.POINTER(StageStruct), ci, C.POINTER(CdlStruct),
                                                C.POINTER(RgbMatrixStruct), ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_apply_rgb_stack.argtypes = [vp, C.POINTER(YuvParams), C.POINTER(StageStruct), ci, C.POINTER(CdlStruct),
                                         C.POINTER(RgbMatrixStruct), ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Packed), ci,
                                         C.POINTER(Planes), ci, ci]
    lib.lutr_apply_yuv_stack_to_rgb.argtypes = [vp, C.POINTER(YuvParams), C.POINTER(StageStruct), ci, C.POINTER(CdlStruct),
                                                C.POINTER(RgbMatrixStruct), ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes),
                                                C.POINTER(Packed), ci, ci]
    lib.lutr_apply_yuv_stack_semi.argtypes = [vp, C.POINTER(YuvParams), C.POINTER(StageStruct), ci, C.POINTER(CdlStruct),
                                              C.POINTER(YuvLayout), C.POINTER(YuvLayout), ci, ci, ci, C.POINTER(Planes),
                                              C.POINTER(Planes), ci, ci]
    lib.lutr_apply_yuv_stack_packed.argtypes = [vp, C.POINTER(YuvParams), C.POINTER(StageStruct), ci, C.POINTER(CdlStruct),
                                                C.POINTER(YuvPacking), C.POINTER(YuvPacking), ci, ci, ci, C.POINTER(Planes),
                                                C.POINTER(Planes), ci, ci]
    lib.lutr_apply_yuv_stack_v210.argtypes = [vp, C.POINTER(YuvParams), C.POINTER(StageStruct), ci, C.POINTER(CdlStruct), ci, ci,
                                              ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes), ci, ci]
    lib.lutr_dither_mask.argtypes = [C.POINTER(C.c_uint16)]
    lib.lutr_resize_filter.argtypes = [ci, ci, ci, ci, C.POINTER(ci), C.POINTER(C.c_int16), C.POINTER(ci)]
    lib.lutr_resize_planes.argtypes = [vp, ci, ci, ci, ci, ci, ci, ci, ci, ci, ci, C.POINTER(Planes), C.POINTER(Planes)]
    lib.lutr_resize_plan.argtypes = [ci, ci, ci, ci, ci, ci, ci, ci, ci, C.POINTER(ci)]
    lib.lutr_ctx_set_variant.argtypes = [vp, ci]
    lib.lutr_ctx_set_precision.argtypes = [vp, ci]
    lib.lutr_ctx_last_kernel.argtypes = [vp]
    lib.lutr_ctx_last_kernel.restype = cp
    lib.lutr_ctx_tile_stats.argtypes = [vp, ci, C.POINTER(C.c_uint64)]
    lib.lutr_yuv_constants.argtypes = [C.POINTER(YuvParams), C.POINTER(C.c_float)]
    lib.lutr_max_waves_knob.argtypes = [cp, ci, ci]
    lib.lutr_max_blocks_knob.argtypes = [cp, ci]
    _lib = lib
    return lib


def dither_mask():
    """lutr_dither_mask (host only): the 64 x 64 ranks of the blue-noise dither, uint16 [y, x]."""
    import numpy as np
    rank = np.zeros((64, 64), np.uint16)
    check(load().lutr_dither_mask(rank.ctypes.data_as(C.POINTER(C.c_uint16))))
    return rank


def cdl_table(cdl, depth: int):
    """lutr_cdl_table (host only): stage A of the CDL pass for the three channels, float32 [3, 2^depth] -- the
    value of every integer code after slope, offset, clamp and power."""
    import numpy as np
    st = cdl_struct(cdl)
    out = np.zeros((3, 1 << int(depth)), np.float32)
    for ch in range(3):
        check(load().lutr_cdl_table(C.byref(st), int(depth), ch, out[ch].ctypes.data_as(C.POINTER(C.c_float))))
    return out


def interp1d_code(name) -> int:
    """enum lutr_interp1d of a lut1d mode name; ValueError for an unknown one."""
    if name not in INTERP1D:
        raise ValueError(f"unknown interp1d '{name}' ({' | '.join(INTERP1D)})")
    return INTERP1D[name]


def lut1d_table(lut1d, interp1d: str, depth: int):
    """lutr_lut1d_table (host only): the per-code table of a `cube.Lut1D` for the three channels, uint16
    [3, 2^depth] -- the output code of every integer code."""
    import numpy as np
    mode = interp1d_code(interp1d)
    tab = np.ascontiguousarray(lut1d.table, dtype=np.float32)
    scale = (C.c_float * 3)(*[float(v) for v in lut1d.scale])
    out = np.zeros((3, 1 << int(depth)), np.uint16)
    for ch in range(3):
        check(load().lutr_lut1d_table(tab.ctypes.data_as(C.POINTER(C.c_float)), int(tab.shape[1]), scale, mode, int(depth), ch,
                                      out[ch].ctypes.data_as(C.POINTER(C.c_uint16))))
    return out


def max_waves_knob(text, waves_per_block: int, uncapped: int) -> int:
    """lutr_max_waves_knob (host only): what the tile launchers make of LUTR_MAX_WAVES = `text` (None = unset)."""
    return load().lutr_max_waves_knob(None if text is None else str(text).encode(), waves_per_block, uncapped)


def max_blocks_knob(text, cap: int) -> int:
    """lutr_max_blocks_knob (host only): the blocks a grid-stride launch capped at `cap` may get under LUTR_MAX_BLOCKS = `text`
    (None = unset)."""
    return load().lutr_max_blocks_knob(None if text is None else str(text).encode(), cap)


def resize_filter(src: int, dst: int, cs: int = 0, cosited: bool = False):
    """lutr_resize_filter (host only): (start [n_out] int32, weights [n_out, taps] int16) of one axis of one plane."""
    import numpy as np
    lib = load()
    taps = C.c_int()
    check(lib.lutr_resize_filter(src, dst, cs, int(cosited), None, None, C.byref(taps)))
    n_out = (dst + (1 << cs) - 1) >> cs
    start = np.zeros(n_out, np.int32)
    w = np.zeros((n_out, taps.value), np.int16)
    check(lib.lutr_resize_filter(src, dst, cs, int(cosited), start.ctypes.data_as(C.POINTER(C.c_int)),
                                 w.ctypes.data_as(C.POINTER(C.c_int16)), C.byref(taps)))
    return start, w


#: the words of lutr_resize_plan's out[8], in order
RESIZE_PLAN_FIELDS = ("th", "rows", "lds", "spx", "spy", "nx_max", "ny_max", "tiles_per_frame")


def resize_plan(family: str, depth: int, csx: int, csy: int, chroma_loc, sw: int, sh: int, dw: int, dh: int) -> dict:
    """lutr_resize_plan (host only): the launch plan of lutr_resize_planes for `family` ("yuv" | "gbr") frames of sw x sh resized to
    dw x dh, as a dict of RESIZE_PLAN_FIELDS.  `chroma_loc` is a CHROMA_LOC name or None."""
    out = (C.c_int * len(RESIZE_PLAN_FIELDS))()
    loc = CHROMA_REPLICATE if chroma_loc is None else CHROMA_LOC[chroma_loc]
    check(load().lutr_resize_plan(RESIZE_FAMILY[family], depth, csx, csy, loc, sw, sh, dw, dh, out))
    return dict(zip(RESIZE_PLAN_FIELDS, out))


def check(rc: int) -> None:
    if rc != 0:
        raise LutrError(rc, load().lutr_last_error().decode("utf-8", "replace"))
