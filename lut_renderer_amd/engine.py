"""Python host of the LUT engine: a thin wrapper over the C-ABI (include/lutr.h).

PyTorch is used only as plumbing: device memory (tensors), streams and
torch.distributed (RCCL) for the one collective this path has, the broadcast of the
lattice at LUT load.  All pixel work happens in liblutr's HIP kernels; nothing here
computes pixels, and nothing falls back to the CPU.

Replaces: the `ffmpeg` child process the reference starts per task
(`/root/reference/src/lut_renderer/task_manager.py:145-151`) for the filters built at
`/root/reference/src/lut_renderer/ffmpeg.py:195-247` and `:304-310`.
"""
from __future__ import annotations

import ctypes as C
import threading
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native
from .cdl import Cdl
from .cube import CubeLut, Lut1D, read_cube, read_lut, read_lut1d
from .rgbmatrix import RgbMatrix
# (the formats and the checks of names and options live in formats.py; the names callers have always imported from here stay)
from .formats import (_ALPHA_RESIZE, PackedYuvFmt, PixFmt, RgbSource, SemiFmt, V210Fmt, chain_interp, chain_side,  # noqa: F401
                      changes_subsampling, check_alpha_mode, check_cdl_options, check_chain_options, check_chroma_loc,
                      check_lut1d_options, check_matte, check_rgb_stack_options, check_stack_options, check_strength, check_yuv2rgb_options, check_yuv2rgb_stack_options,
                      check_container_options,
                      check_dual_options, check_lut2, check_packed_options, check_packed_stack_options, check_premul_options, check_semi_options,
                      check_semi_stack_options, chroma_loc_code, dual_side, has_prologue, held_resources, packed_frame_width, parse_packed_yuv_fmt, parse_pix_fmt,
                      parse_rgb_source, parse_semi_fmt, parse_size, parse_v210_fmt, refuse_alpha_resize, refuse_chain_keywords,
                      refuse_dual_keywords, source_bit_depth, v210_frame_width, yuv_side)

_NOT_TENSORS = "planes must be torch tensors resident on the engine's GPU"
#: what a planar side with the wrong number of planes is told
_PLANE_COUNT = {3: "expected three planes", 4: "'{}' takes four planes: the three colour planes and alpha"}


def _stack_front(eng, entry: str, check, allowed: Tuple[str, ...], pix_fmt, out_pix_fmt, stages, cdl, rgb_matrix, other: dict,
                 variant: bool = True, **told):
    """What the three stack entries (`entry`: the name of the one calling) do before they look at a plane: TypeError for a
    keyword of `other` that is not one of `allowed` -- the options the family's `check` refuses by name -- and for a `cdl` /
    `rgb_matrix` of the wrong type; then `check` with what `eng` holds (`held_resources`; its variant too unless `variant` is
    False), `other` and `told`.  Returns (parsed stages, source format, destination format, (the stage array, its length, the
    CDL's pointer | None, the matrix's pointer | None) as the C entries take them)."""
    for k in other:
        if k not in allowed:
            raise TypeError(f"{entry}() got an unexpected keyword argument '{k}'")
    if cdl is not None and not isinstance(cdl, Cdl):
        raise TypeError(f"cdl must be a lut_renderer_amd.cdl.Cdl, not {type(cdl).__name__}")
    if rgb_matrix is not None and not isinstance(rgb_matrix, RgbMatrix):
        raise TypeError(f"rgb_matrix must be a lut_renderer_amd.rgbmatrix.RgbMatrix, not {type(rgb_matrix).__name__}")
    st, fin, fout = check(pix_fmt, out_pix_fmt, stages=stages, cdl=cdl is not None, rgb_matrix=rgb_matrix is not None,
                          **held_resources(eng, variant), **other, **told)
    k = None if cdl is None else C.byref(_native.cdl_struct(cdl))
    m = None if rgb_matrix is None else C.byref(_native.rgb_matrix_struct(rgb_matrix))
    return st, fin, fout, (_native.stage_array(st), len(st), k, m)


def _source_frame(src, fin: PixFmt) -> Tuple[int, int]:
    """(w, h) of the planar source of a two-output or two-LUT call, its planes checked against `fin`."""
    if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
        raise ValueError(_PLANE_COUNT[fin.nplanes].format(fin.name))
    if not isinstance(src[0], torch.Tensor):
        raise TypeError(_NOT_TENSORS)
    h, w = src[0].shape[-2], src[0].shape[-1]
    _check_planes(src, fin, w, h, "source")
    return w, h


def dual_args(src, dst, dst2, pix_fmt, out_pix_fmt, out2_pix_fmt):
    """What `apply_yuv_dual` checks of its formats and planes before it touches the engine: the three formats, and the shapes
    and dtypes of the planes given.  Returns (fin, f1, f2, w, h)."""
    fin, f1, f2 = check_dual_options(pix_fmt, out_pix_fmt, out2_pix_fmt)
    w, h = _source_frame(src, fin)
    if dst is not None:
        _check_planes(dst, f1, w, h, "destination")
    if dst2 is not None:
        _check_planes(dst2, f2, w, h, "second destination")
    return fin, f1, f2, w, h


def chain_args(src, dst, pix_fmt, out_pix_fmt, interp, interp2):
    """What `apply_yuv_chain` checks of its formats, modes and planes before it touches the engine.  Returns (fin, fout, w, h,
    mode, mode2)."""
    fin, fout = check_chain_options(pix_fmt, out_pix_fmt)
    mode, mode2 = chain_interp(interp, interp2)
    w, h = _source_frame(src, fin)
    if dst is not None:
        _check_planes(dst, fout, w, h, "destination")
    return fin, fout, w, h, mode, mode2


#: frames per LUT launch when apply_yuv / apply_rgb resize (`out_size`): the LUT writes a chunk into the engine's scratch at the
#: source size and the resize reads it back while it is still in the Infinity Cache.  LUTR_RESIZE_CHUNK overrides.
RESIZE_CHUNK = 16


def resize_chunk_default() -> int:
    import os
    v = os.environ.get("LUTR_RESIZE_CHUNK")
    return max(1, int(v)) if v else RESIZE_CHUNK


def _alpha_src(t, depth: int, eng, nframes: int, slot: Optional[int] = None, premul: bool = False) -> _native.AlphaSrc:
    """struct lutr_alpha_src for the alpha source `t` of a call of `nframes` frames on the engine `eng`: a plane ([H,W] / [F,H,W],
    integer at `depth` bits or float32), a packed image whose component `slot` is alpha ([H,W,C] / [F,H,W,C]), or None
    (ALPHA_NONE: the destination is filled).  `premul`: the source travels beside the colour planes of a premultiplied call
    (DESIGN.md 3.18), which words two of the refusals its own way."""
    a = _native.AlphaSrc()
    a.kind, a.depth, a.step, a.offset = _native.ALPHA_NONE, 0, 1, 0
    if t is None:
        return a
    if not isinstance(t, torch.Tensor):
        raise TypeError(_NOT_TENSORS)
    if premul and t.device != eng.device:
        raise ValueError(f"the alpha plane is on {t.device}, engine is on {eng.device}")
    if t.stride(-1) != 1 or (slot is not None and t.stride(-2) != t.shape[-1]):
        raise ValueError("planes must be dense along the row")
    if t.device != eng.device:
        raise ValueError(_NOT_TENSORS)
    lead = t.dim() - (2 if slot is None else 3)
    a.kind = _native.ALPHA_FLOAT if t.dtype == torch.float32 else _native.ALPHA_INT
    a.depth = 0 if a.kind == _native.ALPHA_FLOAT else depth
    a.data = t.data_ptr()
    a.stride = t.stride(lead) * t.element_size()
    a.frame_stride = t.stride(0) * t.element_size() if lead else 0
    if slot is not None:
        a.step, a.offset = t.shape[-1], slot
    if (t.shape[0] if lead else 1) != nframes:
        raise ValueError("planes disagree on the number of frames" if premul else "src and dst disagree on the number of frames")
    return a


_PREMUL_IN_PLACE = ("the premultiplied-alpha pass cannot run in place: destination planes must not overlap the source planes or "
                    "the alpha source")


def _byte_range(t: torch.Tensor) -> Tuple[int, int]:
    lo = hi = t.data_ptr()
    for n, st in zip(t.shape, t.stride()):
        if st >= 0:
            hi += (n - 1) * st * t.element_size()
        else:
            lo += (n - 1) * st * t.element_size()
    return lo, hi + t.element_size()


_CDL_IN_PLACE = "the CDL pass cannot run in place: destination planes must not overlap the source planes"
_STACK_IN_PLACE = "the stack pass cannot run in place: destination planes must not overlap the source planes"
_LUT1D_IN_PLACE = "the lut1d pass cannot run in place: destination planes must not overlap the source planes"
_RESIZE_IN_PLACE = "a resize cannot run in place: destination planes must not overlap the source planes"
_RGB2YUV_IN_PLACE = "RGB -> YUV cannot run in place: destination planes must not overlap the source"
_YUV2RGB_IN_PLACE = "YUV -> RGB cannot run in place: the destination must not overlap the source planes"
_RGBSTACK_YUV_IN_PLACE = "the RGB stack pass cannot run in place into YUV: destination planes must not overlap the source"
_RGBSTACK_IN_PLACE = ("the RGB stack pass runs in place only on a planar source's own planes: any other destination must not "
                      "overlap the source")


def _check_not_in_place(src: Sequence[torch.Tensor], dst: Sequence[torch.Tensor], message: str) -> None:
    for a in src:
        alo, ahi = _byte_range(a)
        for b in dst:
            blo, bhi = _byte_range(b)
            if alo < bhi and blo < ahi:
                raise ValueError(message)


_ALPHA_OVERLAP = ("the alpha source overlaps {}: alpha may run in place only as the same plane at the same depth, and must not "
                  "share memory with any other destination plane")


def _check_alpha_overlap(a_src: Optional[torch.Tensor], din: int, dst: Sequence[torch.Tensor], dout: int) -> None:
    """What lutr_alpha_plane would refuse, found before the colour pass is launched: the alpha source (a plane,
    or the packed image that holds it; None = fill) against the alpha destination `dst[3]` -- the same plane at the same depth
    is the no-op, any other overlap of the byte ranges is refused -- and against the colour destinations `dst[:3]`, which the
    colour pass would overwrite before alpha is read."""
    if a_src is None:
        return
    alo, ahi = _byte_range(a_src)
    for i, d in enumerate(dst):
        blo, bhi = _byte_range(d)
        if not (alo < bhi and blo < ahi):
            continue
        same = (i == 3 and din == dout and a_src.dtype == d.dtype and a_src.data_ptr() == d.data_ptr() and a_src.shape == d.shape
                and a_src.stride() == d.stride())
        if not same:
            raise ValueError(_ALPHA_OVERLAP.format("the alpha destination" if i == 3 else f"destination plane {i}"))


def _frames3(planes: Sequence[torch.Tensor]) -> list:
    return [t if t.dim() == 3 else t.unsqueeze(0) for t in planes]



def _check_planes(planes: Sequence[torch.Tensor], fmt: PixFmt, w: int, h: int, what: str) -> None:
    """The C-ABI takes bare pointers and cannot know buffer sizes: every plane must have exactly the shape and the
    element size `fmt` implies for a w x h frame, or the kernels would read or write outside it."""
    if fmt.nplanes == 2:
        if isinstance(planes, torch.Tensor) or len(planes) != 2:
            raise ValueError(f"'{fmt.name}' takes two planes: luma and the interleaved chroma pairs")
    elif fmt.nplanes == 1:
        if isinstance(planes, torch.Tensor) or len(planes) != 1:
            raise ValueError(f"'{fmt.name}' takes one buffer of packed groups")
    elif len(planes) != fmt.nplanes:
        raise ValueError(_PLANE_COUNT[fmt.nplanes].format(fmt.name))
    esize = getattr(fmt, "itemsize", 1 if fmt.depth <= 8 else 2)
    for i, t in enumerate(planes):
        if not isinstance(t, torch.Tensor):
            raise TypeError(_NOT_TENSORS)
        if t.dim() not in (2, 3):
            raise ValueError("planes must be [H,W] or [F,H,W]")
        if t.is_floating_point() or t.element_size() != esize:
            raise ValueError(f"{what} plane {i}: '{fmt.name}' takes {8 * esize}-bit integer samples, got {t.dtype}")
        if i == 3 and t.stride(-1) != 1:                       # (the colour planes: _planes_struct; alpha goes its own way)
            raise ValueError("planes must be dense along the row")
        want = fmt.plane_shape(i, w, h)
        if isinstance(fmt, V210Fmt):                           # any row that holds the groups (FFmpeg's custom_stride)
            if t.shape[-2] != h or t.shape[-1] < 4 * fmt.groups(w):
                raise ValueError(f"{what} plane {i} is {tuple(t.shape[-2:])}, '{fmt.name}' at {w}x{h} needs {want} words "
                                 f"(at least {4 * fmt.groups(w)} a row)")
        elif tuple(t.shape[-2:]) != want:
            raise ValueError(f"{what} plane {i} is {tuple(t.shape[-2:])}, '{fmt.name}' at {w}x{h} needs {want}")


def _check_float_planes(planes: Sequence[torch.Tensor], fmt: RgbSource, w: int, h: int, what: str) -> None:
    """`_check_planes` for a float format: `fmt.nplanes` float32 planes of h x w (a three-plane list is taken for gbrapf32le too:
    the alpha plane never reaches the kernels)."""
    if isinstance(planes, torch.Tensor) or len(planes) not in (3, fmt.nplanes):
        raise ValueError(f"'{fmt.name}' takes {fmt.nplanes} planes (G, B, R{', A' if fmt.nplanes == 4 else ''})")
    for i, t in enumerate(planes):
        if not isinstance(t, torch.Tensor):
            raise TypeError(_NOT_TENSORS)
        if t.dim() not in (2, 3):
            raise ValueError("planes must be [H,W] or [F,H,W]")
        if t.dtype != torch.float32:
            raise ValueError(f"{what} plane {i}: '{fmt.name}' takes float32 samples, got {t.dtype}")
        if tuple(t.shape[-2:]) != (h, w):
            raise ValueError(f"{what} plane {i} is {tuple(t.shape[-2:])}, '{fmt.name}' at {w}x{h} needs {(h, w)}")
        if i == 3 and t.stride(-1) != 1:                       # (the colour planes: _planes_struct; alpha goes its own way)
            raise ValueError("planes must be dense along the row")


def _planes_struct(planes: Sequence[torch.Tensor], device: torch.device, nplanes: int = 3) -> Tuple[_native.Planes, int]:
    """Describe three [H,W] or [F,H,W] tensors as struct lutr_planes; returns (struct, nframes).  nplanes = 2: a semi-planar
    side (luma, chroma pairs); slot 2 stays NULL.  nplanes = 1: a packed 4:2:2 side; slots 1 and 2 stay NULL."""
    if len(planes) != nplanes:
        raise ValueError(f"expected {('one plane', 'two planes', 'three planes')[nplanes - 1]}")
    st = _native.Planes()
    nframes = None
    for i, t in enumerate(planes):
        if not isinstance(t, torch.Tensor):
            raise TypeError(_NOT_TENSORS)
        if t.device != device:
            raise ValueError(f"plane {i} is on {t.device}, engine is on {device}")
        if t.dim() == 2:
            f, fs = 1, 0
        elif t.dim() == 3:
            f, fs = t.shape[0], t.stride(0) * t.element_size()
        else:
            raise ValueError("planes must be [H,W] or [F,H,W]")
        if t.stride(-1) != 1:
            raise ValueError("planes must be dense along the row")
        if nframes is None:
            nframes = f
        elif nframes != f:
            raise ValueError("planes disagree on the number of frames")
        st.data[i] = t.data_ptr()
        st.stride[i] = t.stride(-2) * t.element_size()
        st.frame_stride[i] = fs
    return st, nframes


def _plane_pair(src: Sequence[torch.Tensor], dst: Sequence[torch.Tensor], device: torch.device):
    """(struct of src, struct of dst, nframes) for a source and a destination that must agree on the number of frames."""
    s, nf = _planes_struct(src, device)
    d, nfd = _planes_struct(dst, device)
    if nf != nfd:
        raise ValueError("src and dst disagree on the number of frames")
    return s, d, nf


def _packed_struct(t, name: str, nc: int, bits: int, device: torch.device, integers_only: bool) -> _native.Packed:
    """Describe one [H,W,C] or [F,H,W,C] packed image as struct lutr_packed.  integers_only: a floating-point tensor of the right
    element size is refused too (apply_packed has always taken one as raw bits)."""
    if not isinstance(t, torch.Tensor) or t.device != device:
        raise ValueError("packed images must be torch tensors resident on the engine's GPU")
    if (t.dim() not in (3, 4) or t.shape[-1] != nc or (integers_only and t.is_floating_point())
            or t.element_size() * 8 != bits):
        raise ValueError(f"'{name}' takes [H,W,{nc}] or [F,H,W,{nc}] tensors of {bits}-bit elements")
    if t.stride(-1) != 1 or t.stride(-2) != nc:
        raise ValueError("pixels must be dense along the row")
    st = _native.Packed()
    st.data = t.data_ptr()
    st.stride = t.stride(-3) * t.element_size()
    st.frame_stride = t.stride(0) * t.element_size() if t.dim() == 4 else 0
    return st


def _yuv_params(fmt_in: int, fmt_out: int, lut_depth: int, matrix_in: str, matrix_out: str, range_src: str, range_in: str,
                range_out: str) -> _native.YuvParams:
    p = _native.YuvParams()
    p.fmt_in, p.fmt_out, p.lut_depth = fmt_in, fmt_out, lut_depth
    p.matrix_in, p.matrix_out = _native.MATRIX[matrix_in], _native.MATRIX[matrix_out]
    p.range_src, p.range_in, p.range_out = _native.RANGE[range_src], _native.RANGE[range_in], _native.RANGE[range_out]
    return p


def _yuv_call_params(fin, fout, lut_depth: Optional[int], matrix_in: str, matrix_out: Optional[str], range_src: str,
                     range_in: Optional[str], range_out: str) -> _native.YuvParams:
    """`_yuv_params` from the keyword values of a YUV call: the LUT runs at the source's depth, the output keeps the input's
    matrix and the LUT sees the source's range unless the call says otherwise."""
    return _yuv_params(fin.code, fout.code, lut_depth if lut_depth is not None else fin.depth, matrix_in, matrix_out or matrix_in,
                       range_src, range_in or range_src, range_out)


def _yuv_out_dtype(depth: int, inherit: Optional[torch.dtype]) -> torch.dtype:
    """dtype of freshly allocated YUV output planes: uint8 up to 8 bit; deeper outputs inherit a 16-bit source dtype, else (a
    narrower source, or None: an RGB source) int16."""
    return torch.uint8 if depth <= 8 else inherit if inherit is not None and inherit.itemsize == 2 else torch.int16


def _new_planes(fmt, w: int, h: int, lead: tuple, dtype, device) -> list:
    """Fresh planes of one side: `fmt.nplanes` tensors of `lead + fmt.plane_shape(i, w, h)`."""
    return [torch.empty(lead + fmt.plane_shape(i, w, h), dtype=dtype, device=device) for i in range(fmt.nplanes)]


def _fresh_planes(fmt, w: int, h: int, like: torch.Tensor, device) -> list:
    """Fresh output planes of the YUV side `fmt` for a w x h call whose first source plane is `like`: its leading dimensions, and
    its dtype where a 16-bit output inherits one.  A v210 buffer is zeroed: the kernels never write the padding of a row."""
    lead = tuple(like.shape[:-2])
    if isinstance(fmt, V210Fmt):
        return [torch.zeros(lead + fmt.plane_shape(0, w, h), dtype=torch.int32, device=device)]
    return _new_planes(fmt, w, h, lead, _yuv_out_dtype(fmt.depth, like.dtype), device)


class LutEngine:
    """One GPU context: a device lattice plus the stream its kernels run on."""

    def __init__(self, device: int = 0, use_torch_stream: bool = True):
        if not torch.cuda.is_available():
            raise RuntimeError("LutEngine needs a HIP GPU; there is no CPU fallback")
        self._lib = _native.load()
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        handle = C.c_void_p()
        _native.check(self._lib.lutr_ctx_create(self.device_index, C.byref(handle)))
        self._ctx = handle
        self.n = 0
        self.scale = None
        self.use_torch_stream = use_torch_stream
        # One context = one stream, one lattice, one work queue (include/lutr.h: thread-safe per context, contexts are not
        # shared between threads).  The reference runs up to 16 tasks on a thread pool (task_manager.py:229-235) and ctypes
        # releases the GIL, so every call that touches the context takes this lock; `api.apply_lut` holds it across
        # set_lut + apply so that a cached engine cannot render one task with another task's lattice.
        self._lock = threading.RLock()
        self.precision = "strict"
        self._frame_strength = None       # the per-frame strengths of the last apply_yuv_stack(strength=[...])
        self._applied_lut = None          # the CubeLut object apply_lut uploaded last (its upload-skipping shortcut)
        self._applied_lut2 = None         # ... and the second LUT of apply_lut(cube2=)
        self.n2 = 0
        self._applied_lut1d = None        # ... and the (1D LUT, mode) of apply_lut(lut1d=)
        self.n1d = 0                      # rows of the 1D LUT set_lut1d holds (0: none)
        # grow-only plane caches of _scratch, (key, [3 planes]) per slot: "rz" = the source-size output of the LUT ahead of a
        # resize, "fr" = the 8-bit YUV frames between the two stages of a full-range RGB source
        self._scratch_slots = {}
        # (raw name of the last alpha kernel, the joined name `last_kernel` reports for it) after an alpha-carrying call, else None
        self._alpha_kernels = None
        self._has_prelut = False          # the lattice carries a .csp prelut (what a CDL in front of it refuses)

    # -- lifetime ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None):
            self._lib.lutr_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- lattice ----------------------------------------------------------
    def set_lut(self, lut: CubeLut) -> None:
        table = np.ascontiguousarray(lut.table, dtype=np.float32)
        scale = (C.c_float * 3)(*[float(v) for v in lut.scale])
        with self._lock:
            self._applied_lut = None      # any direct upload invalidates apply_lut's "same LUT as last time" shortcut
            _native.check(self._lib.lutr_ctx_set_lut(
                self._ctx, table.ctypes.data_as(C.POINTER(C.c_float)), int(lut.n), scale))
            self.n, self.scale = int(lut.n), np.array(lut.scale, dtype=np.float32)
            self.set_prelut(getattr(lut, "prelut", None))

    def set_prelut(self, pre) -> None:
        """lut3d's prelut (a cineSpace shaper, `cube.Prelut`) for the lattice just set, or None to remove it.  Uploading a
        lattice drops the prelut of the previous one."""
        self._has_prelut = pre is not None
        if pre is None:
            _native.check(self._lib.lutr_ctx_set_prelut(self._ctx, None, 0, None, None))
            return
        table = np.ascontiguousarray(pre.table, dtype=np.float32)
        pmin = (C.c_float * 3)(*[float(v) for v in pre.min])
        pscale = (C.c_float * 3)(*[float(v) for v in pre.scale])
        _native.check(self._lib.lutr_ctx_set_prelut(
            self._ctx, table.ctypes.data_as(C.POINTER(C.c_float)), int(table.shape[1]), pmin, pscale))

    def load_cube(self, path) -> CubeLut:
        lut = read_lut(path)
        self.set_lut(lut)
        return lut

    def set_lut2(self, lut: Optional[CubeLut]) -> None:
        """The SECOND LUT of `apply_yuv_chain`, or None to remove it.  It lives beside the first lattice: `set_lut`
        / `load_cube` leave it alone and no other call reads it.  A LUT that carries a prelut (a .csp shaper) is a ValueError."""
        check_lut2(lut)
        with self._lock:
            self._applied_lut2 = None     # any direct upload invalidates apply_lut's "same second LUT as last time" shortcut
            if lut is None:
                _native.check(self._lib.lutr_ctx_set_lut2(self._ctx, None, 0, None))
                self.n2 = 0
                return
            table = np.ascontiguousarray(lut.table, dtype=np.float32)
            scale = (C.c_float * 3)(*[float(v) for v in lut.scale])
            _native.check(self._lib.lutr_ctx_set_lut2(
                self._ctx, table.ctypes.data_as(C.POINTER(C.c_float)), int(lut.n), scale))
            self.n2 = int(lut.n)

    def load_cube2(self, path) -> CubeLut:
        lut = read_lut(path)
        self.set_lut2(lut)
        return lut

    def set_lut1d(self, lut1d: Optional[Lut1D], interp: str = "linear") -> None:
        """The 1D LUT of `apply_yuv_lut1d` / `apply_rgb_lut1d` (a `cube.Lut1D`) and lut1d's mode for it (nearest |
        linear | cosine | cubic | spline), or None to remove it.  It lives beside the lattices: `set_lut` / `load_cube` / `set_lut2`
        leave it alone and no other call reads it."""
        mode = _native.interp1d_code(interp)
        if lut1d is not None and not isinstance(lut1d, Lut1D):
            raise TypeError(f"lut1d must be a lut_renderer_amd.cube.Lut1D, not {type(lut1d).__name__}")
        with self._lock:
            self._applied_lut1d = None    # any direct upload invalidates apply_lut's "same 1D LUT as last time" shortcut
            if lut1d is None:
                _native.check(self._lib.lutr_ctx_set_lut1d(self._ctx, None, 0, None, mode))
                self.n1d = 0
                return
            table = np.ascontiguousarray(lut1d.table, dtype=np.float32)
            scale = (C.c_float * 3)(*[float(v) for v in lut1d.scale])
            _native.check(self._lib.lutr_ctx_set_lut1d(
                self._ctx, table.ctypes.data_as(C.POINTER(C.c_float)), int(table.shape[1]), scale, mode))
            self.n1d = int(table.shape[1])

    def load_lut1d(self, path, interp: str = "linear") -> Lut1D:
        lut1d = read_lut1d(path)
        self.set_lut1d(lut1d, interp)
        return lut1d

    def lattice_tensor(self) -> torch.Tensor:
        """The device lattice viewed as a float32 tensor [(n+1)^3 * 4] (no copy)."""
        ptr, size = C.c_void_p(), C.c_size_t()
        _native.check(self._lib.lutr_ctx_lut_device(self._ctx, C.byref(ptr), C.byref(size)))
        return _tensor_from_ptr(ptr.value, size.value // 4, self.device)

    def set_lut_distributed(self, lut: Optional[CubeLut], src: int = 0, group=None) -> None:
        """Rank `src` uploads the lattice; every other rank receives it with ONE broadcast
        (RCCL over xGMI on GPUs).  No other collective exists on this path."""
        import torch.distributed as dist
        self._applied_lut = None
        rank = dist.get_rank(group)
        meta = torch.zeros(4, dtype=torch.float32, device=self.device)
        if rank == src:
            if lut is None:
                raise ValueError("the source rank must pass the LUT")
            self.set_lut(lut)
            meta = torch.tensor([float(lut.n), *[float(v) for v in lut.scale]], dtype=torch.float32,
                                device=self.device)
        dist.broadcast(meta, src=src, group=group)
        if rank != src:
            n = int(meta[0].item())
            scale = (C.c_float * 3)(*[float(v) for v in meta[1:].tolist()])
            _native.check(self._lib.lutr_ctx_lut_alloc(self._ctx, n, scale))
            self.n, self.scale = n, np.array(list(scale), dtype=np.float32)
        dist.broadcast(self.lattice_tensor(), src=src, group=group)
        if rank != src:
            torch.cuda.current_stream(self.device).synchronize()
            _native.check(self._lib.lutr_ctx_lut_seal(self._ctx))      # finiteness + value range of what arrived
        # a cineSpace prelut travels with the lattice: its size first (0 = none), then table and ranges in one tensor
        pre = getattr(lut, "prelut", None) if rank == src else None
        size = torch.tensor([0 if pre is None else int(pre.table.shape[1])], dtype=torch.int32, device=self.device)
        dist.broadcast(size, src=src, group=group)
        nsz = int(size.item())
        if nsz:
            from .cube import Prelut
            if rank == src:
                flat = np.concatenate([pre.table.reshape(-1), pre.min, pre.scale]).astype(np.float32)
                buf = torch.from_numpy(flat).to(self.device)
            else:
                buf = torch.empty(3 * nsz + 6, dtype=torch.float32, device=self.device)
            dist.broadcast(buf, src=src, group=group)
            if rank != src:
                host = buf.cpu().numpy()
                self.set_prelut(Prelut(host[:3 * nsz].reshape(3, nsz), host[3 * nsz:3 * nsz + 3], host[3 * nsz + 3:]))

    # -- control ----------------------------------------------------------
    def set_variant(self, name: str) -> None:
        _native.check(self._lib.lutr_ctx_set_variant(self._ctx, _native.VARIANT[name]))
        self._variant_name = name

    def set_precision(self, name: str) -> None:
        """"strict" (default): bit-exact with FFmpeg's scalar C.  "fast": allow the tolerance-bounded tile kernels
        (<= 1 code from strict at 8 and 10 bit).  "fma32": strict's fp32 lattice with a fused multiply-add blend (<= 1 code
        from strict at every depth).  include/lutr.h lutr_ctx_set_precision."""
        if name not in _native.PRECISION:
            raise ValueError(f"unknown precision '{name}' ({' | '.join(_native.PRECISION)})")
        with self._lock:
            _native.check(self._lib.lutr_ctx_set_precision(self._ctx, _native.PRECISION[name]))
            self.precision = name

    @property
    def last_kernel(self) -> str:
        """The kernel of the last call; after an alpha-carrying call "<colour kernel>+<alpha kernel>" (DESIGN.md 3.16)."""
        name = self._lib.lutr_ctx_last_kernel(self._ctx).decode()
        joined = self._alpha_kernels
        return joined[1] if joined is not None and joined[0] == name else name

    def _alpha_plane(self, src, dst: torch.Tensor, din: int, dout: int, w: int, h: int, row0: int, rows: Optional[int],
                     slot: Optional[int] = None, after: Optional[str] = None) -> None:
        """The alpha plane of an alpha-carrying call (lutr_alpha_plane), launched on the engine's stream right
        after the colour pass: `src` is the source's alpha plane ([H,W] / [F,H,W], integer at `din` bits or float32), a packed
        image whose component `slot` is alpha ([H,W,C] / [F,H,W,C]), or None (no alpha on the source: `dst` is filled).
        `after`: what `last_kernel` read before this launch; it then reads "<after>+<alpha kernel>" (None: the alpha kernel)."""
        a = _alpha_src(src, din, self, dst.shape[0] if dst.dim() == 3 else 1, slot)
        if dst.device != self.device or dst.stride(-1) != 1:
            raise ValueError("planes must be dense along the row and resident on the engine's GPU")
        nf, dfs = (dst.shape[0], dst.stride(0) * dst.element_size()) if dst.dim() == 3 else (1, 0)
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_alpha_plane(
                self._ctx, C.byref(a), dout, C.c_void_p(dst.data_ptr()), dst.stride(-2) * dst.element_size(), dfs, w, h, nf,
                row0, rows))
            if after is not None and w and rows and nf:          # (an empty call launches nothing and names nothing)
                name = self._lib.lutr_ctx_last_kernel(self._ctx).decode()
                self._alpha_kernels = (name, f"{after}+{name}")

    def _alpha_tail(self, colour, outputs, a_src, din: int, w: int, h: int, row0: int, rows: Optional[int],
                    slot: Optional[int] = None):
        """An alpha-carrying call: `colour()` launches the colour planes, then every output of `outputs` --
        (its format, its planes) -- that carries alpha gets its fourth plane from `a_src` (`_alpha_plane`: a plane at `din` bits,
        a packed image with `slot`, or None), all under the lock.  Returns what `colour()` returned."""
        with self._lock:
            out = colour()
            for fmt, planes in outputs:
                if fmt.alpha:
                    self._alpha_plane(a_src, planes[3], din, fmt.depth, w, h, row0, rows, slot, after=self.last_kernel)
        return out

    def _yuva_call(self, colour, src, dst, fin: PixFmt, fout: PixFmt, prologue: bool, row0: int, rows: Optional[int]):
        """The yuva* path of an entry that takes planar YUV on both sides: the planes checked, the destination
        allocated when none is given, then `colour(src[:3], dst[:3], source name, output name)` -- the entry itself on the colour
        planes under their three-plane names -- and the alpha plane on the same stream (`_alpha_tail`).  Straight alpha goes past
        everything the colour call does; with `prologue` (the call has one) the output's alpha is filled.  Returns `dst`."""
        if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
            raise ValueError(_PLANE_COUNT[fin.nplanes].format(fin.name))
        h, w = src[0].shape[-2], src[0].shape[-1]
        _check_planes(src, fin, w, h, "source")
        if dst is None:
            dst = _fresh_planes(fout, w, h, src[0], self.device)
        _check_planes(dst, fout, w, h, "destination")
        a_src = src[3] if fin.alpha and not prologue else None
        if fout.alpha:
            _check_alpha_overlap(a_src, fin.depth, dst, fout.depth)
        self._alpha_tail(lambda: colour(src[:3], dst[:3], fin.colour.name, fout.colour.name), [(fout, dst)], a_src, fin.depth, w, h,
                         row0, rows)
        return dst

    def _upload_frame_strength(self, strength: np.ndarray) -> C.c_void_p:
        """One float per frame on the device, on the stream the kernel reads it from; the engine keeps it until the next one
        replaces it (torch's allocator hands the old one's memory out again in stream order; a context on a stream of its own is
        waited for first, so that the previous array is not recycled under a running kernel).  Called under the lock, after
        `_bind_stream`."""
        if not self.use_torch_stream and self._frame_strength is not None:
            self.sync()
        self._frame_strength = torch.from_numpy(strength).to(self.device)
        return C.c_void_p(self._frame_strength.data_ptr())

    def tile_stats(self, enable: bool = True) -> dict:
        """Counters of the LDS-window kernels since the previous call; (re)arms collection."""
        out = (C.c_uint64 * 8)()
        _native.check(self._lib.lutr_ctx_tile_stats(self._ctx, int(enable), out))
        return {"tiles": out[0], "misses": out[1], "global_tiles": out[2], "staged": out[3],
                "tube_tiles": out[6], "level2_tiles": out[7], "mixed_tiles": out[4]}

    def sync(self) -> None:
        _native.check(self._lib.lutr_ctx_sync(self._ctx))

    def _bind_stream(self) -> None:
        self._alpha_kernels = None        # (every launch binds first: a joined alpha name never outlives the call that made it)
        if self.use_torch_stream:
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _native.check(self._lib.lutr_ctx_set_stream(self._ctx, C.c_void_p(stream)))

    # -- apply ------------------------------------------------------------
    def apply_rgb(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *,
                  depth: int, interp: str = "tetrahedral", row0: int = 0, rows: Optional[int] = None,
                  out_size=None, resize_chunk: Optional[int] = None):
        """lut3d on planar RGB; planes in gbrp order (G, B, R), each [H,W] or [F,H,W].  A fourth plane (gbrap*'s alpha, DESIGN.md
        3.16) is copied to a fourth destination plane; no out_size then.
        out_size = (w, h) or "WxH" resizes the LUT's output to that size (whole frames, not in place)."""
        if not 8 <= int(depth) <= 16:
            raise ValueError(f"unsupported depth {depth}")
        h, w = src[0].shape[-2], src[0].shape[-1]
        if not isinstance(src, torch.Tensor) and len(src) == 4:      # gbrap*: the alpha plane is copied
            fmt = PixFmt(f"gbrap{depth}", "gbr", int(depth), 0, 0, True, True)
            if out_size is not None:
                raise ValueError(_ALPHA_RESIZE.format(fmt.name))
            if dst is None:
                dst = [torch.empty_like(t) for t in src]
            _check_planes(src, fmt, w, h, "source")
            _check_planes(dst, fmt, w, h, "destination")
            _check_alpha_overlap(src[3], int(depth), dst, int(depth))
            self._alpha_tail(lambda: self.apply_rgb(src[:3], dst[:3], depth=depth, interp=interp, row0=row0, rows=rows),
                             [(fmt, dst)], src[3], int(depth), w, h, row0, rows)
            return dst
        fmt = PixFmt(f"gbrp{depth}", "gbr", int(depth), 0, 0, True)
        if out_size is not None:
            return self._lut_then_resize(src, dst, fmt, fmt, w, h, out_size, row0, rows, resize_chunk, None,
                                         lambda s_, d_: self.apply_rgb(s_, d_, depth=depth, interp=interp))
        if dst is None:
            dst = [torch.empty_like(t) for t in src]
        _check_planes(src, fmt, w, h, "source")
        _check_planes(dst, fmt, w, h, "destination")
        s, d, nf = _plane_pair(src, dst, self.device)
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_planar_rgb(
                self._ctx, depth, _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(d), row0, rows))
        return dst

    def apply_rgb_float(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *,
                        interp: str = "tetrahedral", row0: int = 0, rows: Optional[int] = None, alpha_mode: str = "straight"):
        """lut3d on planar float RGB (gbrpf32le): float32 planes in gbrp order (G, B, R), each [H,W] or [F,H,W];
        float in, float out, nothing clipped.  Input NaN -> 0 and +-inf -> +-FLT_MAX; a .csp prelut is applied per pixel; always
        strict arithmetic.  `dst` may be `src` (in place).  A fourth plane (gbrapf32le's alpha) is copied through unchanged.
        alpha_mode="premultiplied" (four planes only) divides the colour by t = clamp(alpha, 0, 1) in front of
        lut3d and multiplies by it behind, in the same kernel; t == 1 gives the bits of the straight call."""
        premul = check_alpha_mode(alpha_mode)
        if premul and len(src) != 4:
            raise ValueError("alpha_mode='premultiplied' needs a source that carries alpha: 'gbrpf32le' has none")
        fmt = parse_rgb_source("gbrapf32le" if len(src) == 4 else "gbrpf32le")
        h, w = src[0].shape[-2], src[0].shape[-1]
        if dst is None:
            dst = [torch.empty_like(t) for t in src]
        _check_float_planes(src, fmt, w, h, "source")
        _check_float_planes(dst, fmt, w, h, "destination")
        if len(dst) != len(src):
            raise ValueError("src and dst disagree on the number of planes")
        s, d, nf = _plane_pair(src[:3], dst[:3], self.device)
        rows = h - row0 if rows is None else rows
        if premul:
            _check_alpha_overlap(src[3], 0, dst, 0)
            a = _alpha_src(src[3], 0, self, nf, premul=True)
        with self._lock:
            self._bind_stream()
            if premul:
                _native.check(self._lib.lutr_apply_planar_rgb_f32_premul(
                    self._ctx, _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(a), C.byref(d), row0, rows))
            else:
                _native.check(self._lib.lutr_apply_planar_rgb_f32(
                    self._ctx, _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(d), row0, rows))
            if len(src) == 4 and dst[3].data_ptr() != src[3].data_ptr():      # (torch's current stream is the one just bound)
                dst[3][..., row0:row0 + rows, :].copy_(src[3][..., row0:row0 + rows, :], non_blocking=True)
        return dst

    # -- resize -----------------------------------------------------------
    def resize(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, size,
               chroma_loc: Optional[str] = None):
        """Resize planar frames (Y, Cb, Cr or gbrp's G, B, R; each [H,W] or [F,H,W]) to `size` = (w, h) or "WxH" with the
        engine's separable bicubic (lutr_resize_planes).  `chroma_loc` sites the chroma samples (None =
        interstitial, the block centre).  Not in place; packed formats are a ValueError."""
        fmt = parse_pix_fmt(pix_fmt.replace("yuvj", "yuv"))
        loc = chroma_loc_code(chroma_loc)
        dw, dh = parse_size(size)
        sh, sw = src[0].shape[-2], src[0].shape[-1]
        if dst is None:
            dst = _new_planes(fmt, dw, dh, tuple(src[0].shape[:-2]), src[0].dtype, self.device)
        _check_planes(src, fmt, sw, sh, "source")
        _check_planes(dst, fmt, dw, dh, "destination")
        _check_not_in_place(src, dst, _RESIZE_IN_PLACE)
        s, d, nf = _plane_pair(src, dst, self.device)
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_resize_planes(
                self._ctx, _native.RESIZE_FAMILY[fmt.family], fmt.depth, fmt.csx, fmt.csy, loc, sw, sh, dw, dh, nf,
                C.byref(s), C.byref(d)))
        return dst

    def _scratch(self, slot: str, fmt: PixFmt, w: int, h: int, nframes: int, dtype) -> list:
        """Engine-owned planes of `nframes` frames at w x h in `fmt` (kept in `slot` for the next call of the same shape or smaller)."""
        key = (fmt.name, w, h, dtype)
        cur = self._scratch_slots.get(slot)
        if cur is None or cur[0] != key or cur[1][0].shape[0] < nframes:
            cur = self._scratch_slots[slot] = (key, _new_planes(fmt, w, h, (nframes,), dtype, self.device))
        return [t[:nframes] for t in cur[1]]

    def _lut_then_resize(self, src, dst, fin: Optional[PixFmt], fout: PixFmt, w: int, h: int, out_size, row0: int, rows, chunk,
                         chroma_loc, lut_call, src_frames=None):
        """The composition of DESIGN.md 3.7: the LUT into engine scratch at the source size, then the resize into dst, a chunk
        of frames at a time, both on the engine's stream with no host wait in between."""
        dw, dh = parse_size(out_size)
        if row0 != 0 or (rows is not None and rows != h):
            raise ValueError("a resize (out_size) takes whole frames: row0 / rows are not supported with it")
        if dst is None:
            lead = tuple(src_frames[0].shape[:1]) if src_frames is not None else tuple(src[0].shape[:-2])
            dst = _new_planes(fout, dw, dh, lead, _yuv_out_dtype(fout.depth, src[0].dtype), self.device)
        if src_frames is None:             # (a packed source comes checked, as a list of one [F,H,W,C] tensor, in src_frames)
            _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, dw, dh, "destination")
        _check_not_in_place(src, dst, _RESIZE_IN_PLACE)
        s3, d3 = (_frames3(src) if src_frames is None else src_frames), _frames3(dst)
        nf = s3[0].shape[0]
        if d3[0].shape[0] != nf:
            raise ValueError("src and dst disagree on the number of frames")
        chunk = resize_chunk_default() if chunk is None else max(1, int(chunk))
        with self._lock:
            tmp_all = self._scratch("rz", fout, w, h, min(chunk, nf), d3[0].dtype)
            for f0 in range(0, nf, chunk):
                n = min(chunk, nf - f0)
                tmp = [t[:n] for t in tmp_all]
                lut_call([t[f0:f0 + n] for t in s3], tmp)
                self.resize(tmp, [t[f0:f0 + n] for t in d3], pix_fmt=fout.name, size=(dw, dh), chroma_loc=chroma_loc)
        return dst

    def apply_packed(self, src: torch.Tensor, dst: Optional[torch.Tensor] = None, *, pix_fmt: str,
                     interp: str = "tetrahedral", row0: int = 0, rows: Optional[int] = None) -> torch.Tensor:
        """lut3d on packed RGB: `src` is [H,W,C] or [F,H,W,C] (C = 3 or 4, uint8, or int16/uint16 for the
        48/64-bit formats), `pix_fmt` an FFmpeg name from `_native.PACKED_FORMATS`.  The fourth component
        is carried over.  `dst` may be `src` (in place)."""
        if pix_fmt not in _native.PACKED_FORMATS:
            raise ValueError(f"unsupported packed pixel format '{pix_fmt}'")
        bits, nc, ro, go, bo = _native.PACKED_FORMATS[pix_fmt]
        if dst is None:
            dst = torch.empty_like(src)
        descs = [_packed_struct(t, pix_fmt, nc, bits, self.device, False) for t in (src, dst)]
        if src.shape != dst.shape:
            raise ValueError("src and dst shapes differ")
        h, w = src.shape[-3], src.shape[-2]
        nf = src.shape[0] if src.dim() == 4 else 1
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_packed_rgb(
                self._ctx, _native.packed_code(bits, nc, ro, go, bo), _native.INTERP[interp], w, h, nf,
                C.byref(descs[0]), C.byref(descs[1]), row0, rows))
        return dst

    def apply_yuv(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *,
                  pix_fmt: str, interp: str = "tetrahedral", matrix_in: str = "bt709",
                  matrix_out: Optional[str] = None, range_src: str = "tv", range_in: Optional[str] = None,
                  range_out: str = "tv", lut_depth: Optional[int] = None, out_pix_fmt: Optional[str] = None,
                  row0: int = 0, rows: Optional[int] = None, dither: str = "none", chroma_loc: Optional[str] = None,
                  out_size=None, resize_chunk: Optional[int] = None, width: Optional[int] = None,
                  alpha_mode: str = "straight", cdl: Optional[Cdl] = None):
        """Fused YUV -> RGB -> lut3d -> RGB -> YUV on planar frames (Y, Cb, Cr).
        `cdl` (a `cdl.Cdl`) applies an ASC CDL -- slope, offset, power per channel, then saturation -- to the
        integer RGB ahead of lut3d, in the same pass (lutr_apply_yuv_cdl): planar YUV on both sides (yuva* with straight alpha
        included), any layout pair at 8..16 bit, all five modes, the full-range prologue, row0 / rows on the union block, strict
        arithmetic, not in place.  The identity CDL gives the bits of the call without it.  Not with a LUT that carries a .csp
        prelut, dither, chroma_loc, out_size, alpha_mode="premultiplied" or a semi-planar / packed / v210 side.  None (the
        default) is every path described here, unchanged.
        `pix_fmt` / `out_pix_fmt` may each name an alpha-carrying format (yuva420p .. yuva444p16le): that side is
        FOUR planes, the last one alpha at the luma size and the format's depth.  The colour planes are this call on the first three
        under the three-plane names, bit for bit, with every option below; alpha never meets the LUT -- it is copied, converted to
        the output depth (nearest code), dropped when the output has none (the plane is still checked), or filled opaque when
        only the output has it or the call has a prologue (range_src != range_in, or lut_depth other than the source's depth: the
        reference's 8-bit intermediate has no alpha), and is treated as straight.  The alpha source must be dense along the row and
        may overlap the destination only as the same plane at the same depth.  Planar sides only; `out_size` with an alpha-carrying output is a
        ValueError.  `last_kernel` is then "<colour kernel>+<alpha kernel>".
        alpha_mode="premultiplied" (a yuva* source, planar YUV out with or without alpha) divides the integer RGB
        by the source's alpha in front of lut3d and multiplies by it behind, inside one kernel family of its own
        (lutr_apply_yuv_premul; any layout pair, row0 / rows on the union block, strict arithmetic, not in place); the output's
        alpha plane is written as for a straight call.  Opaque pixels give the straight call's bits.  Not with a prologue, dither,
        chroma_loc or out_size.  "straight" (the default) is every path described here, unchanged.
        `pix_fmt` / `out_pix_fmt` may each name a packed 4:2:2 format (yuyv422, uyvy422, yvyu422, y210le, y212le, y216le;
        DESIGN.md 3.12): that side is ONE tensor [..., h, 4 * ceil(w / 2)] (bare or in a one-element list), uint8, or int16 as for
        planar 16-bit; `width` names an odd frame width a packed source cannot tell.  The other side may be planar 4:2:2, and a
        planar destination also 4:2:0 or 4:4:4; no dither / chroma_loc / out_size, strict arithmetic, `dst` may be `src` when
        both sides are the same packed format.  The bits are those of the planar call on the de-interleaved samples.
        `pix_fmt` / `out_pix_fmt` may each name a semi-planar format instead (nv12, nv21, nv16, p010le .. p216le; DESIGN.md
        3.11): that side is a sequence of TWO tensors, y [..., h, w] and cbcr [..., ch, 2 * cw] (the pairs of a row side by side);
        same subsampling on both sides, no dither / chroma_loc / out_size, strict arithmetic, `dst` may be `src` when the two
        formats are the same.  The bits are those of the planar call on the same samples.
        dither="error_diffusion" (the reference's `zscale_dither`) dithers the final quantisation; whole frames only.
        dither="blue_noise" (an engine setting) quantises every output sample against a 64 x 64 void-and-cluster
        mask anchored to the frame, inside the LUT pass: any layout pair, row0 / rows as without dither, strict arithmetic.
        chroma_loc ("left" | "center" | "topleft", ffprobe's chroma_location names) resamples chroma bilinearly at that
        siting instead of replicating it (strict arithmetic, not in place, no dither).  None = replicate.
        `out_pix_fmt` may change the chroma subsampling (4:2:0 / 4:2:2 / 4:4:4 either way): input chroma is
        replicated over its input block, output chroma is the mean over its output block; strict arithmetic, no chroma_loc.
        out_size = (w, h) or "WxH" resizes the output planes to that size after everything else (the reference's `-s`,
        DESIGN.md 3.7): the LUT writes `resize_chunk` frames at a time (default RESIZE_CHUNK) into engine scratch at the source
        size and the resize reads them back; whole frames only, not in place.  The resize sites chroma by `chroma_loc`."""
        if dither not in _native.DITHER:
            raise ValueError(f"unknown dither mode '{dither}'")
        premul = check_alpha_mode(alpha_mode)
        if premul:
            check_premul_options(pix_fmt, out_pix_fmt, dither=dither, chroma_loc=chroma_loc, out_size=out_size, range_src=range_src,
                                 range_in=range_in, lut_depth=lut_depth)
        if cdl is not None:
            if not isinstance(cdl, Cdl):
                raise TypeError(f"cdl must be a lut_renderer_amd.cdl.Cdl, not {type(cdl).__name__}")
            check_cdl_options(pix_fmt, out_pix_fmt, dither=dither, chroma_loc=chroma_loc, out_size=out_size, alpha_mode=alpha_mode,
                              prelut=bool(getattr(self, "_has_prelut", False)))
        kind = check_container_options(pix_fmt, out_pix_fmt, dither, chroma_loc, out_size, width=width)
        if kind is not None:
            return self._apply_yuv_container(kind, src, dst, yuv_side(pix_fmt), yuv_side(out_pix_fmt or pix_fmt), interp, matrix_in,
                                             matrix_out, range_src, range_in, range_out, lut_depth, row0, rows, width)
        fin = parse_pix_fmt(pix_fmt)
        fout = parse_pix_fmt(out_pix_fmt or pix_fmt)
        if fin.family != "yuv" or fout.family != "yuv":
            raise ValueError("apply_yuv takes planar YUV formats")
        if fin.alpha or fout.alpha:
            # yuva*: the colour planes through this very call under their three-plane names, then the alpha plane on the same
            # stream
            if out_size is not None and fout.alpha:
                raise ValueError(_ALPHA_RESIZE.format(fout.name))
            check_chroma_loc(chroma_loc, dither, fin.colour.name, fout.colour.name)
            if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
                raise ValueError(_PLANE_COUNT[fin.nplanes].format(fin.name))
            h, w = src[0].shape[-2], src[0].shape[-1]
            _check_planes(src, fin, w, h, "source")
            if dst is None and out_size is None:
                dst = _fresh_planes(fout, w, h, src[0], self.device)
            if dst is not None and out_size is None:
                _check_planes(dst, fout, w, h, "destination")
            # a prologue call fills: the reference's 8-bit yuv4xxp intermediate has no alpha to carry
            a_src = src[3] if fin.alpha and not has_prologue(fin.depth, range_src, range_in, lut_depth) else None
            if fout.alpha and dst is not None:
                _check_alpha_overlap(a_src, fin.depth, dst, fout.depth)
            if premul:
                # the colour planes through lutr_apply_yuv_premul with the source's alpha beside them, then the alpha plane exactly
                # as for a straight call
                _check_alpha_overlap(a_src, fin.depth, dst[:3], fout.depth)
                _check_not_in_place(src, dst[:3], _PREMUL_IN_PLACE)
                s, d, nf = _plane_pair(src[:3], dst[:3], self.device)
                a = _alpha_src(src[3], fin.depth, self, nf, premul=True)
                p = _yuv_call_params(fin.colour, fout.colour, None, matrix_in, matrix_out, range_src, None, range_out)

                def colour():
                    self._bind_stream()
                    _native.check(self._lib.lutr_apply_yuv_premul(
                        self._ctx, C.byref(p), _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(a), C.byref(d), row0,
                        h - row0 if rows is None else rows))
            else:
                def colour():
                    return self.apply_yuv(src[:3], None if dst is None else dst[:3], pix_fmt=fin.colour.name, interp=interp,
                                          matrix_in=matrix_in, matrix_out=matrix_out, range_src=range_src, range_in=range_in,
                                          range_out=range_out, lut_depth=lut_depth, out_pix_fmt=fout.colour.name, row0=row0,
                                          rows=rows, dither=dither, chroma_loc=chroma_loc, out_size=out_size,
                                          resize_chunk=resize_chunk, cdl=cdl)
            out = self._alpha_tail(colour, [(fout, dst)], a_src, fin.depth, w, h, row0, rows)
            return out if dst is None else dst
        check_chroma_loc(chroma_loc, dither, fin.name, fout.name)
        xsub = (fin.csx, fin.csy) != (fout.csx, fout.csy)
        p = _yuv_call_params(fin, fout, lut_depth, matrix_in, matrix_out, range_src, range_in, range_out)
        h, w = src[0].shape[-2], src[0].shape[-1]
        if out_size is not None:
            kw = dict(pix_fmt=pix_fmt, interp=interp, matrix_in=matrix_in, matrix_out=matrix_out, range_src=range_src,
                      range_in=range_in, range_out=range_out, lut_depth=lut_depth, out_pix_fmt=out_pix_fmt, dither=dither,
                      chroma_loc=chroma_loc)
            return self._lut_then_resize(src, dst, fin, fout, w, h, out_size, row0, rows, resize_chunk, chroma_loc,
                                         lambda s_, d_: self.apply_yuv(s_, d_, **kw))
        if dst is None:
            dst = _fresh_planes(fout, w, h, src[0], self.device)
        _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, w, h, "destination")
        s, d, nf = _plane_pair(src, dst, self.device)
        rows = h - row0 if rows is None else rows
        if dither == "error_diffusion" and (row0 != 0 or rows != h):
            raise ValueError("error-diffusion dither couples the rows of a frame: whole frames only")
        if cdl is not None:
            _check_not_in_place(src, dst, _CDL_IN_PLACE)
            k = _native.cdl_struct(cdl)
        with self._lock:
            self._bind_stream()
            if cdl is not None:
                _native.check(self._lib.lutr_apply_yuv_cdl(
                    self._ctx, C.byref(p), _native.INTERP[interp], C.byref(k), w, h, nf, C.byref(s), C.byref(d), row0, rows))
            elif xsub or dither == "blue_noise":
                _native.check(self._lib.lutr_apply_yuv_xsub(
                    self._ctx, C.byref(p), _native.INTERP[interp], _native.DITHER[dither], w, h, nf, C.byref(s), C.byref(d),
                    row0, rows))
            elif chroma_loc is not None:
                _native.check(self._lib.lutr_apply_yuv_sited(
                    self._ctx, C.byref(p), _native.INTERP[interp], chroma_loc_code(chroma_loc), w, h, nf, C.byref(s), C.byref(d),
                    row0, rows))
            elif dither != "none":
                _native.check(self._lib.lutr_apply_yuv_dither(
                    self._ctx, C.byref(p), _native.INTERP[interp], _native.DITHER[dither], w, h, nf, C.byref(s), C.byref(d)))
            else:
                _native.check(self._lib.lutr_apply_yuv(
                    self._ctx, C.byref(p), _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(d), row0, rows))
        return dst

    def apply_yuv_lut1d(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                        out_pix_fmt: Optional[str] = None, interp: Optional[str] = "tetrahedral", matrix_in: str = "bt709",
                        matrix_out: Optional[str] = None, range_src: str = "tv", range_in: Optional[str] = None,
                        range_out: str = "tv", lut_depth: Optional[int] = None, row0: int = 0, rows: Optional[int] = None,
                        **other):
        """`apply_yuv` with the engine's 1D LUT (`set_lut1d`) on the integer RGB ahead of lut3d, in the same pass
        (lutr_apply_yuv_lut1d; ffmpeg's `lut1d=file=A,lut3d=file=B`): planar YUV on both sides (yuva* with straight alpha
        included), any layout pair at 8..16 bit, the full-range prologue, a .csp prelut on the 3D LUT, row0 / rows on the union
        block, strict arithmetic, not in place.  `interp` is lut3d's mode, or None for lut1d alone (no 3D LUT needed).  The
        identity 1D LUT gives the bits of `apply_yuv(out_pix_fmt=...)`.  No dither, chroma_loc, out_size, cdl, premultiplied alpha,
        second LUT or second output, and no RGB / float / semi-planar / packed / v210 side: each is a ValueError naming it."""
        for k in other:
            if k not in ("dither", "chroma_loc", "out_size", "alpha_mode", "cdl", "out2_pix_fmt", "cube2", "lut2"):
                raise TypeError(f"apply_yuv_lut1d() got an unexpected keyword argument '{k}'")
        lut2 = other.get("cube2") is not None or bool(other.get("lut2"))
        check_lut1d_options(pix_fmt, out_pix_fmt, dither=other.get("dither", "none"), chroma_loc=other.get("chroma_loc"),
                            out_size=other.get("out_size"), alpha_mode=other.get("alpha_mode", "straight"),
                            out2_pix_fmt=other.get("out2_pix_fmt"), lut2=lut2, cdl=other.get("cdl") is not None,
                            loaded=bool(getattr(self, "n1d", 0)))
        if interp is not None and interp not in _native.INTERP:
            raise ValueError(f"lut3d has no interpolation mode '{interp}'")
        mode = _native.INTERP_NONE if interp is None else _native.INTERP[interp]
        fin = parse_pix_fmt(pix_fmt.replace("yuvj", "yuv"))
        fout = parse_pix_fmt((out_pix_fmt or pix_fmt).replace("yuvj", "yuv"))
        if fin.alpha or fout.alpha:
            # yuva*: the colour planes through this very call under their three-plane names, then the alpha plane on the same
            # stream, exactly as the CDL call does
            return self._yuva_call(lambda s3, d3, name, out_name: self.apply_yuv_lut1d(
                s3, d3, pix_fmt=name, out_pix_fmt=out_name, interp=interp, matrix_in=matrix_in, matrix_out=matrix_out,
                range_src=range_src, range_in=range_in, range_out=range_out, lut_depth=lut_depth, row0=row0, rows=rows),
                src, dst, fin, fout, has_prologue(fin.depth, range_src, range_in, lut_depth), row0, rows)
        p = _yuv_call_params(fin, fout, lut_depth, matrix_in, matrix_out, range_src, range_in, range_out)
        h, w = src[0].shape[-2], src[0].shape[-1]
        if dst is None:
            dst = _fresh_planes(fout, w, h, src[0], self.device)
        _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, w, h, "destination")
        _check_not_in_place(src, dst, _LUT1D_IN_PLACE)
        s, d, nf = _plane_pair(src, dst, self.device)
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_yuv_lut1d(
                self._ctx, C.byref(p), mode, w, h, nf, C.byref(s), C.byref(d), row0, rows))
        return dst

    def apply_yuv_stack(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                        out_pix_fmt: Optional[str] = None, stages, cdl: Optional[Cdl] = None, matrix_in: str = "bt709",
                        matrix_out: Optional[str] = None, range_src: str = "tv", range_in: Optional[str] = None,
                        range_out: str = "tv", lut_depth: Optional[int] = None, row0: int = 0, rows: Optional[int] = None,
                        strength=None, matte: Optional[torch.Tensor] = None, matte_depth: Optional[int] = None,
                        matte_invert: bool = False, rgb_matrix: Optional[RgbMatrix] = None, **other):
        """`apply_yuv` with an ordered stack of 1..4 stages between its YUV -> RGB and RGB -> YUV stages, in one pass
        (lutr_apply_yuv_stack).  `stages` is a sequence of "lut3d" (`set_lut`), "lut3d2" (`set_lut2`), "lut1d"
        (`set_lut1d`), "cdl" (the `cdl` argument), each at most once; a lut3d stage may be a pair ("lut3d", "trilinear") -- the
        default mode is tetrahedral -- and a comma string "lut1d,cdl,lut3d:trilinear" is read the same way.  Planar YUV on both
        sides (yuva* with straight alpha included), any layout pair at 8..16 bit, the full-range prologue, row0 / rows on the union
        block, strict arithmetic, not in place.  ("lut3d",) gives the bits of `apply_yuv(out_pix_fmt=...)`, ("cdl", "lut3d") those
        of `apply_yuv(cdl=...)`, ("lut1d", "lut3d") those of `apply_yuv_lut1d`, ("lut3d", "lut3d2") those of `apply_yuv_chain`.  No
        dither, chroma_loc, out_size, premultiplied alpha or second output, and no RGB / float / semi-planar / packed / v210 side:
        each is a ValueError naming it (`formats.check_stack_options`).
        `strength`: None runs the pass above unchanged.  A number in [0, 1] mixes the graded pixel with the source
        behind the list, q = (int)((q0 + s * (q1 - q0)) + 0.5f) on the RGB codes, in the same pass (lutr_apply_yuv_stack_mix): 1
        gives the bits of the call without it, 0 those of the two conversion stages alone.  A sequence, NumPy array or CPU tensor
        of one number per frame gives every frame of the call its own strength (frame 0 = the first frame of `src`, whatever
        row0 / rows are): it is checked on the host (length, finite, in [0, 1]; a ValueError names the index and the value),
        uploaded on the engine's stream and held by the engine until the next such call replaces it.
        `matte`: None runs the passes above unchanged.  A tensor on the engine's device, [H,W] or [1,H,W] (a still:
        one matte for every frame) or [F,H,W], at the luma size of the frame, uint8 (`matte_depth` 8, the default) or int16 /
        uint16 (`matte_depth` 9..16, required; a code above 2^matte_depth - 1 acts as that), scales the strength per pixel in the
        same pass (lutr_apply_yuv_stack_matte): w = s * (a / Mm), or s * ((Mm - a) / Mm) with `matte_invert`, takes the place of s
        in the mix above, ahead of the chroma mean.  `strength` defaults to 1 with a matte.  A matte of Mm everywhere gives the
        bits of the call with the strength alone, 0 everywhere those of strength 0.  The matte is not processed in any way; the
        alpha plane of a yuva* source goes past it unchanged -- to key on it, pass it as `matte` (`formats.check_matte`).
        `rgb_matrix`: the `rgbmatrix.RgbMatrix` of a "matrix" stage, which may stand once anywhere in the list:
        o = clamp(M * u + offset, 0, 1) on unit RGB, u = q / (2^lut_depth - 1) where the pixel is a code.  A lattice behind it is
        fed unit floats as behind the CDL; lut1d, cdl and the end of the list round to codes first.  The call goes to
        lutr_apply_yuv_stack_matrix when a matrix stage is listed and only then; a matrix without its stage, a stage without its
        matrix and a strength or matte together with the stage are ValueErrors."""
        st, fin, fout, (arr, n, k, mtx) = _stack_front(
            self, "apply_yuv_stack", check_stack_options, ("dither", "chroma_loc", "out_size", "alpha_mode", "out2_pix_fmt"),
            pix_fmt, out_pix_fmt, stages, cdl, rgb_matrix, other, variant=False, strength=strength, matte=matte is not None)
        if fin.alpha or fout.alpha:
            # yuva*: the colour planes through this very call under their three-plane names, then the alpha plane on the same
            # stream, exactly as the CDL call does; straight alpha goes past the mix unchanged
            return self._yuva_call(lambda s3, d3, name, out_name: self.apply_yuv_stack(
                s3, d3, pix_fmt=name, out_pix_fmt=out_name, stages=st, cdl=cdl, matrix_in=matrix_in, matrix_out=matrix_out,
                range_src=range_src, range_in=range_in, range_out=range_out, lut_depth=lut_depth, row0=row0, rows=rows,
                strength=strength, matte=matte, matte_depth=matte_depth, matte_invert=matte_invert, rgb_matrix=rgb_matrix),
                src, dst, fin, fout, has_prologue(fin.depth, range_src, range_in, lut_depth), row0, rows)
        p = _yuv_call_params(fin, fout, lut_depth, matrix_in, matrix_out, range_src, range_in, range_out)
        h, w = src[0].shape[-2], src[0].shape[-1]
        if dst is None:
            dst = _fresh_planes(fout, w, h, src[0], self.device)
        _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, w, h, "destination")
        _check_not_in_place(src, dst, _STACK_IN_PLACE)
        s, d, nf = _plane_pair(src, dst, self.device)
        rows = h - row0 if rows is None else rows
        strength = check_strength(strength, nf)
        if matte is not None:
            matte, mdepth, minvert, still = check_matte(matte, matte_depth, matte_invert, w=w, h=h, nframes=nf, device=self.device)
            m = _native.MatteStruct()
            m.data = matte.data_ptr()
            m.stride = matte.stride(-2) * matte.element_size()
            m.frame_stride = 0 if still else matte.stride(0) * matte.element_size()
            m.depth, m.invert = mdepth, minvert
            if strength is None:
                strength = 1.0
        with self._lock:
            self._bind_stream()
            if rgb_matrix is not None:                            # a matrix stage is listed (check_stack_options)
                _native.check(self._lib.lutr_apply_yuv_stack_matrix(
                    self._ctx, C.byref(p), arr, n, k, mtx, w, h, nf, C.byref(s), C.byref(d), row0, rows))
            elif strength is None:                                # (a matte brings a strength of 1)
                _native.check(self._lib.lutr_apply_yuv_stack(
                    self._ctx, C.byref(p), arr, n, k, w, h, nf, C.byref(s), C.byref(d), row0, rows))
            else:
                # one number for the call, or 1.0 beside one float per frame
                frame = None if isinstance(strength, float) else self._upload_frame_strength(strength)
                mix = (strength if frame is None else 1.0, frame)
                if matte is not None:
                    _native.check(self._lib.lutr_apply_yuv_stack_matte(
                        self._ctx, C.byref(p), arr, n, k, *mix, C.byref(m), w, h, nf, C.byref(s), C.byref(d), row0, rows))
                else:
                    _native.check(self._lib.lutr_apply_yuv_stack_mix(
                        self._ctx, C.byref(p), arr, n, k, *mix, w, h, nf, C.byref(s), C.byref(d), row0, rows))
        return dst

    def apply_yuv_stack_semi(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                             out_pix_fmt: Optional[str] = None, stages, cdl: Optional[Cdl] = None, matrix_in: str = "bt709",
                             matrix_out: Optional[str] = None, range_src: str = "tv", range_in: Optional[str] = None,
                             range_out: str = "tv", lut_depth: Optional[int] = None, row0: int = 0, rows: Optional[int] = None,
                             **other):
        """`apply_yuv_stack` on frames whose source side, destination side or both are semi-planar, in one pass
        (lutr_apply_yuv_stack_semi): a hardware decoder's nv12 / p010le through `stages` into a planar master
        or back into nv12 / p010le, without a de-interleave pass ahead of the stack and an interleave pass behind it.  A
        semi-planar side is [y, cbcr], exactly as `apply_yuv(pix_fmt="nv12")` takes it; a planar side is three planes.  The
        result is bit for bit `semiplanar.to_semi(apply_yuv_stack(semiplanar.to_planar(src)))`.  A semi-planar side is 4:2:0 or
        4:2:2 (the names of `_native.SEMI_FORMATS`); the other side may be 4:2:0 / 4:2:2 / 4:4:4, planar or semi-planar, at 8..16
        bit -- the one call that changes the chroma subsampling of a semi-planar frame.  `stages`, `cdl`, the matrices, ranges,
        `lut_depth` and row0 / rows (on the union block) are `apply_yuv_stack`'s; strict arithmetic, not in place.  No matrix
        stage, strength, matte, dither, chroma_loc, out_size, premultiplied alpha or second output, no yuva* / RGB / float /
        packed / v210 side, and at least one semi-planar side: each is a ValueError naming it
        (`formats.check_semi_stack_options`)."""
        strength, matte, rgb_matrix = other.pop("strength", None), other.pop("matte", None), other.pop("rgb_matrix", None)
        st, fin, fout, (arr, n, k, _mtx) = _stack_front(
            self, "apply_yuv_stack_semi", check_semi_stack_options, ("dither", "chroma_loc", "out_size", "alpha_mode", "out2_pix_fmt"),
            pix_fmt, out_pix_fmt, stages, cdl, rgb_matrix, other, strength=strength, matte=matte)
        p = _yuv_call_params(fin, fout, lut_depth, matrix_in, matrix_out, range_src, range_in, range_out)
        if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
            raise ValueError(f"'{fin.name}' takes {fin.nplanes} planes")
        if not isinstance(src[0], torch.Tensor):
            raise TypeError(_NOT_TENSORS)
        h, w = src[0].shape[-2], src[0].shape[-1]
        if dst is None:
            dst = _fresh_planes(fout, w, h, src[0], self.device)
        if isinstance(dst, torch.Tensor) or len(dst) != fout.nplanes:
            raise ValueError(f"'{fout.name}' takes {fout.nplanes} planes")
        _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, w, h, "destination")
        _check_not_in_place(src, dst, _STACK_IN_PLACE)
        s, nf = _planes_struct(src, self.device, fin.nplanes)
        d, nfd = _planes_struct(dst, self.device, fout.nplanes)
        if nf != nfd:
            raise ValueError("src and dst disagree on the number of frames")
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_yuv_stack_semi(
                self._ctx, C.byref(p), arr, n, k, C.byref(fin.layout()), C.byref(fout.layout()), w, h, nf, C.byref(s), C.byref(d),
                row0, rows))
        return dst

    def apply_yuv_stack_packed(self, src, dst=None, *, pix_fmt: str, out_pix_fmt: Optional[str] = None, stages,
                               cdl: Optional[Cdl] = None, width: Optional[int] = None, matrix_in: str = "bt709",
                               matrix_out: Optional[str] = None, range_src: str = "tv", range_in: Optional[str] = None,
                               range_out: str = "tv", lut_depth: Optional[int] = None, row0: int = 0, rows: Optional[int] = None,
                               **other):
        """`apply_yuv_stack` on capture frames -- a source side, a destination side or both packed 4:2:2 (yuyv422, uyvy422, yvyu422,
        y210le, y212le, y216le) or v210 -- in one pass (lutr_apply_yuv_stack_packed / lutr_apply_yuv_stack_v210):
        a capture card's v210 / uyvy422 through `stages` into v210 / uyvy422 for a play-out card or into a planar master, without
        an unpacking pass ahead of the stack and a packing pass behind it.  The sides are what `apply_yuv` takes for these
        containers: a packed side ONE tensor [..., h, 4 * ceil(w / 2)], a v210 side ONE int32 tensor [..., h, 32 * ceil(w / 48)],
        bare or in a one-element list (`width` names a width the rows cannot tell); a planar side three planes.  The result is
        bit for bit `packedyuv.to_packed` / `v210.to_v210` of `apply_yuv_stack` on the planar samples of `src`.  A packed or v210
        source may go to planar 4:2:2, 4:2:0 or 4:4:4 at 8..16 bit; a packed or v210 destination takes a 4:2:2 source.  `stages`,
        `cdl`, the matrices, ranges, `lut_depth` and row0 / rows (on the destination's chroma block) are `apply_yuv_stack`'s;
        strict arithmetic, not in place.  No matrix stage, strength, matte, dither, chroma_loc, out_size, premultiplied alpha or
        second output, no yuva* / semi-planar / RGB / float side, no packed 4:2:2 side together with a v210 side, and at least one
        packed 4:2:2 or v210 side: each is a ValueError naming it (`formats.check_packed_stack_options`)."""
        strength, matte, rgb_matrix = other.pop("strength", None), other.pop("matte", None), other.pop("rgb_matrix", None)
        st, fin, fout, (arr, n, k, _mtx) = _stack_front(
            self, "apply_yuv_stack_packed", check_packed_stack_options,
            ("dither", "chroma_loc", "out_size", "alpha_mode", "out2_pix_fmt"), pix_fmt, out_pix_fmt, stages, cdl, rgb_matrix, other,
            strength=strength, matte=matte)
        p = _yuv_call_params(fin, fout, lut_depth, matrix_in, matrix_out, range_src, range_in, range_out)
        v210 = isinstance(fin, V210Fmt) or isinstance(fout, V210Fmt)
        bare = fout.nplanes == 1 and isinstance(dst, torch.Tensor)
        if fin.nplanes == 1 and isinstance(src, torch.Tensor):
            src = [src]
        if bare:
            dst = [dst]
        if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
            raise ValueError(f"'{fin.name}' takes {fin.nplanes} plane{'s' if fin.nplanes > 1 else ''}")
        if not isinstance(src[0], torch.Tensor):
            raise TypeError(_NOT_TENSORS)
        w = v210_frame_width(fin, fout, src, dst, width) if v210 else packed_frame_width(fin, src, width)
        h = src[0].shape[-2]
        if dst is None:
            dst = _fresh_planes(fout, w, h, src[0], self.device)
        _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, w, h, "destination")
        _check_not_in_place(src, dst, _STACK_IN_PLACE)
        s, nf = _planes_struct(src, self.device, fin.nplanes)
        d, nfd = _planes_struct(dst, self.device, fout.nplanes)
        if nf != nfd:
            raise ValueError("src and dst disagree on the number of frames")
        if v210:
            entry, sides = self._lib.lutr_apply_yuv_stack_v210, (int(isinstance(fin, V210Fmt)), int(isinstance(fout, V210Fmt)))
        else:
            entry, sides = self._lib.lutr_apply_yuv_stack_packed, (C.byref(fin.packing()), C.byref(fout.packing()))
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(entry(self._ctx, C.byref(p), arr, n, k, *sides, w, h, nf, C.byref(s), C.byref(d), row0, rows))
        return dst[0] if bare else dst

    def apply_rgb_lut1d(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, depth: int,
                        interp: Optional[str] = None, row0: int = 0, rows: Optional[int] = None):
        """The engine's 1D LUT (`set_lut1d`) on planar RGB; planes in gbrp order (G, B, R), each [H,W] or [F,H,W]:
        every sample through its channel's per-code table, a container value above 2^depth - 1 taken as that.  `dst` may be `src`
        (in place).  `interp` = a lut3d mode runs today's `apply_rgb` in place on `dst` behind it (ffmpeg's `lut1d,lut3d`): two
        launches on the engine's stream with no host wait in between."""
        if not 8 <= int(depth) <= 16:
            raise ValueError(f"unsupported depth {depth}")
        if interp is not None and interp not in _native.INTERP:
            raise ValueError(f"lut3d has no interpolation mode '{interp}'")
        if not getattr(self, "n1d", 0):
            raise ValueError("no 1D LUT is loaded: call set_lut1d / load_lut1d first, or pass lut1d")
        if isinstance(src, torch.Tensor) or len(src) != 3:
            raise ValueError("apply_rgb_lut1d takes three planes (G, B, R)")
        h, w = src[0].shape[-2], src[0].shape[-1]
        fmt = PixFmt(f"gbrp{depth}", "gbr", int(depth), 0, 0, True)
        if dst is None:
            dst = [torch.empty_like(t) for t in src]
        _check_planes(src, fmt, w, h, "source")
        _check_planes(dst, fmt, w, h, "destination")
        s, d, nf = _plane_pair(src, dst, self.device)
        n_rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_planar_rgb_lut1d(self._ctx, int(depth), w, h, nf, C.byref(s), C.byref(d), row0, n_rows))
            if interp is not None:
                self.apply_rgb(dst, dst, depth=depth, interp=interp, row0=row0, rows=rows)
        return dst

    def apply_yuv_dual(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None,
                       dst2: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, out_pix_fmt: Optional[str] = None,
                       out2_pix_fmt: str, interp: str = "tetrahedral", matrix_in: str = "bt709",
                       matrix_out: Optional[str] = None, range_src: str = "tv", range_in: Optional[str] = None,
                       range_out: str = "tv", lut_depth: Optional[int] = None, row0: int = 0, rows: Optional[int] = None,
                       **other):
        """`apply_yuv` with TWO planar YUV outputs from one pass (the reference's "pro" mode: a yuv422p10le
        master and the delivery format): the source is read once and lut3d evaluated once per pixel; `out_pix_fmt` and
        `out2_pix_fmt` may differ in depth and chroma subsampling and share `matrix_out` / `range_out`.  Each output has the bits
        of `apply_yuv(..., out_pix_fmt=<its format>)` alone.  Always strict arithmetic; no dither, chroma_loc or out_size;
        nothing may overlap (not in place).  row0 / rows are multiples of the union block height of the three layouts.
        Returns (planes, planes2)."""
        refuse_dual_keywords(other)
        if other:
            raise TypeError(f"apply_yuv_dual() got an unexpected keyword argument '{next(iter(other))}'")
        fin, f1, f2, w, h = dual_args(src, dst, dst2, pix_fmt, out_pix_fmt, out2_pix_fmt)
        if fin.alpha or f1.alpha or f2.alpha:
            # each output carries, fills or drops alpha on its own; the colour planes through this very call
            if dst is None:
                dst = _fresh_planes(f1, w, h, src[0], self.device)
            if dst2 is None:
                dst2 = _fresh_planes(f2, w, h, src[0], self.device)
            # (a prologue call fills, as in apply_yuv)
            a_src = src[3] if fin.alpha and not has_prologue(fin.depth, range_src, range_in, lut_depth) else None
            for f, d in ((f1, dst), (f2, dst2)):
                _check_alpha_overlap(a_src, fin.depth, list(d[:3]) + ([d[3]] if f.alpha else []), f.depth)
            if f1.alpha and f2.alpha:
                _check_not_in_place([dst[3]], list(dst2), "the two outputs' planes must not overlap")
                _check_not_in_place([dst2[3]], list(dst), "the two outputs' planes must not overlap")
            self._alpha_tail(lambda: self.apply_yuv_dual(
                src[:3], dst[:3], dst2[:3], pix_fmt=fin.colour.name, out_pix_fmt=f1.colour.name, out2_pix_fmt=f2.colour.name,
                interp=interp, matrix_in=matrix_in, matrix_out=matrix_out, range_src=range_src, range_in=range_in,
                range_out=range_out, lut_depth=lut_depth, row0=row0, rows=rows), [(f1, dst), (f2, dst2)], a_src, fin.depth, w, h,
                row0, rows)
            return dst, dst2
        p = _yuv_call_params(fin, f1, lut_depth, matrix_in, matrix_out, range_src, range_in, range_out)
        if dst is None:
            dst = _fresh_planes(f1, w, h, src[0], self.device)
        if dst2 is None:
            dst2 = _fresh_planes(f2, w, h, src[0], self.device)
        s, d, nf = _plane_pair(src, dst, self.device)
        d2, nf2 = _planes_struct(dst2, self.device)
        if nf != nf2:
            raise ValueError("src and dst2 disagree on the number of frames")
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_yuv_dual(
                self._ctx, C.byref(p), f2.code, _native.INTERP[interp], w, h, nf, C.byref(s), C.byref(d), C.byref(d2), row0, rows))
        return dst, dst2

    def apply_yuv_chain(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                        out_pix_fmt: Optional[str] = None, interp: str = "tetrahedral", interp2: Optional[str] = None,
                        matrix_in: str = "bt709", matrix_out: Optional[str] = None, range_src: str = "tv",
                        range_in: Optional[str] = None, range_out: str = "tv", lut_depth: Optional[int] = None, row0: int = 0,
                        rows: Optional[int] = None, **other):
        """`apply_yuv` with TWO LUTs in one pass (ffmpeg's `lut3d=A:interp=ia,lut3d=B:interp=ib,format=...`): the
        first LUT (`set_lut`, its prelut included) in mode `interp`, then the second (`set_lut2`) in mode `interp2` (None =
        `interp`) on the first one's integer RGB at the LUT depth, then RGB -> YUV once.  Planar YUV without alpha on both
        sides, any pair of 4:2:0 / 4:2:2 / 4:4:4 at 8..16 bit.  Always strict arithmetic; no dither, chroma_loc, out_size or
        second output; not in place.  row0 / rows are multiples of the union block height of the two layouts."""
        refuse_chain_keywords(other)
        if other:
            raise TypeError(f"apply_yuv_chain() got an unexpected keyword argument '{next(iter(other))}'")
        fin, fout, w, h, mode, mode2 = chain_args(src, dst, pix_fmt, out_pix_fmt, interp, interp2)
        p = _yuv_call_params(fin, fout, lut_depth, matrix_in, matrix_out, range_src, range_in, range_out)
        if dst is None:
            dst = _fresh_planes(fout, w, h, src[0], self.device)
        s, d, nf = _plane_pair(src, dst, self.device)
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_yuv_chain(
                self._ctx, C.byref(p), mode, mode2, w, h, nf, C.byref(s), C.byref(d), row0, rows))
        return dst

    def _apply_yuv_container(self, kind, src, dst, fin, fout, interp, matrix_in, matrix_out, range_src, range_in, range_out,
                             lut_depth, row0, rows, width):
        """apply_yuv with a side that is not three planes, `kind` as `check_container_options` told it after checking the options:
        "semi" (lutr_apply_yuv_semi), "packed" (lutr_apply_yuv_packed: a side may be a bare tensor, and `width` names an odd
        width) or "v210" (lutr_apply_yuv_v210, DESIGN.md 3.14: that side is ONE int32 tensor [..., h, words], bare or in a
        one-element list, 32 * ceil(w / 48) words a row by default; a planar side or `width` tells the width)."""
        p = _yuv_call_params(fin, fout, lut_depth, matrix_in, matrix_out, range_src, range_in, range_out)
        vi, vo = isinstance(fin, V210Fmt), isinstance(fout, V210Fmt)
        bare = (kind == "packed" or vo) and isinstance(dst, torch.Tensor)
        if (kind == "packed" or vi) and isinstance(src, torch.Tensor):
            src = [src]
        if bare:
            dst = [dst]
        if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
            raise ValueError(f"'{fin.name}' takes {fin.nplanes} plane{'s' if fin.nplanes > 1 else ''}")
        w = v210_frame_width(fin, fout, src, dst, width) if kind == "v210" else packed_frame_width(fin, src, width)
        h = src[0].shape[-2]
        if dst is None:
            dst = _fresh_planes(fout, w, h, src[0], self.device)
        _check_planes(src, fin, w, h, "source")
        _check_planes(dst, fout, w, h, "destination")
        s, nf = _planes_struct(src, self.device, fin.nplanes)
        d, nfd = _planes_struct(dst, self.device, fout.nplanes)
        if nf != nfd:
            raise ValueError("src and dst disagree on the number of frames")
        if kind == "v210":
            entry, sides = self._lib.lutr_apply_yuv_v210, (int(vi), int(vo))
        elif kind == "packed":
            entry, sides = self._lib.lutr_apply_yuv_packed, (C.byref(fin.packing()), C.byref(fout.packing()))
        else:
            entry, sides = self._lib.lutr_apply_yuv_semi, (C.byref(fin.layout()), C.byref(fout.layout()))
        rows = h - row0 if rows is None else rows
        with self._lock:
            self._bind_stream()
            _native.check(entry(self._ctx, C.byref(p), _native.INTERP[interp], *sides, w, h, nf, C.byref(s), C.byref(d), row0, rows))
        return dst[0] if bare else dst


    # -- RGB source, YUV output --------------------------------
    def _rgb_source(self, src, fmt: RgbSource):
        """Validate an RGB source; returns (planar struct | None, packed struct | None, w, h, nframes, lead shape)."""
        if fmt.floating:
            if isinstance(src, torch.Tensor) or len(src) not in (3, fmt.nplanes):
                raise ValueError(f"'{fmt.name}' takes {fmt.nplanes} planes (G, B, R{', A' if fmt.nplanes == 4 else ''})")
            h, w = src[0].shape[-2], src[0].shape[-1]
            _check_float_planes(src, fmt, w, h, "source")
            st, nf = _planes_struct(src[:3], self.device)          # (an alpha plane is dropped for a YUV output)
            return st, None, w, h, nf, tuple(src[0].shape[:-2])
        if not fmt.packed:
            if isinstance(src, torch.Tensor) or len(src) != fmt.nplanes:
                raise ValueError(f"'{fmt.name}' takes four planes (G, B, R, A)" if fmt.nplanes == 4 else
                                 f"'{fmt.name}' takes three planes (G, B, R)")
            h, w = src[0].shape[-2], src[0].shape[-1]
            _check_planes(src, PixFmt(fmt.name, "gbr", fmt.depth, 0, 0, True, fmt.nplanes == 4), w, h, "source")
            st, nf = _planes_struct(src[:3], self.device)          # (an alpha plane goes its own way: _alpha_plane)
            return st, None, w, h, nf, tuple(src[0].shape[:-2])
        t = src
        st = _packed_struct(t, fmt.name, fmt.ncomp, fmt.depth, self.device, True)
        return None, st, t.shape[-2], t.shape[-3], (t.shape[0] if t.dim() == 4 else 1), tuple(t.shape[:-3])

    def apply_rgb_to_yuv(self, src, dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, out_pix_fmt: str,
                         interp: str = "tetrahedral", matrix_out: str = "smpte170m", range_out: str = "tv", row0: int = 0,
                         rows: Optional[int] = None, dither: str = "none", out_size=None, resize_chunk: Optional[int] = None,
                         lut: bool = True, chroma_loc: Optional[str] = None, intermediate_pix_fmt: Optional[str] = None,
                         prologue_out_range: Optional[str] = None):
        """lut3d on an RGB source, then RGB -> YUV into planar `out_pix_fmt` (4:2:0 / 4:2:2 / 4:4:4, any depth), in one pass
        (DESIGN.md 3.9).  `src` is three gbrp-ordered planes (G, B, R; `pix_fmt` = gbrp, gbrp9le .. gbrp16le) or one [F,]H,W,C
        packed tensor (`pix_fmt` a name of `_native.PACKED_FORMATS`; a fourth component is dropped).  The LUT runs at the source's
        depth; always strict arithmetic.  `pix_fmt` = gbrpf32le | gbrapf32le takes float32 planes (lut3d's float
        path, its output quantised to 16-bit codes for the output stage; an alpha plane is dropped; no `out_size`).  A yuva*
        `out_pix_fmt` takes its alpha from the fourth plane of `gbrap*` / `gbrapf32le` or from the real A of a packed
        name (rgba, bgra, argb, abgr, rgba64le, bgra64le) at the output depth; any other source, and the full-range composition,
        fill it opaque; `gbrap*` with an output without alpha drops the plane.  lut=False leaves lut3d out.  dither / out_size as for `apply_yuv`.  Not in place.
        `intermediate_pix_fmt` / `prologue_out_range` (a LutPlan's fields for a source flagged full range) select the two-stage
        composition of `apply_rgb_full_range`, with `matrix_out` as the plan's matrix."""
        if dither not in _native.DITHER:
            raise ValueError(f"unknown dither mode '{dither}'")
        if chroma_loc is not None:
            raise ValueError("chroma siting (chroma_loc) is not defined for an RGB source: it has no chroma samples to site")
        fin = parse_rgb_source(pix_fmt)
        if fin is None:
            raise ValueError(f"apply_rgb_to_yuv takes gbrp*, gbrpf32le or packed RGB sources, not '{pix_fmt}'")
        fout = parse_pix_fmt((out_pix_fmt or "").replace("yuvj", "yuv"))
        if fin.floating and out_size is not None:
            raise ValueError("a resize (out_size) is not supported with a float source")
        if fout.family != "yuv":
            raise ValueError("apply_rgb_to_yuv writes planar YUV formats; use apply_rgb / apply_packed for RGB output")
        if fout.alpha:
            # a yuva* output: the colour planes through this very call, then alpha from gbrap*'s fourth plane, a
            # packed name's real A or gbrapf32le's fourth plane -- any other source, and the full-range prologue, fill it
            if out_size is not None:
                raise ValueError(_ALPHA_RESIZE.format(fout.name))
            _, _, w, h, _, lead = self._rgb_source(src, fin)
            if dst is None:
                dst = _new_planes(fout, w, h, lead, _yuv_out_dtype(fout.depth, None), self.device)
            _check_planes(dst, fout, w, h, "destination")
            a_src, slot = None, None
            if intermediate_pix_fmt is None:
                if fin.packed and fin.alpha_slot is not None:
                    a_src, slot = src, fin.alpha_slot
                elif not fin.packed and fin.nplanes == 4 and len(src) == 4:
                    a_src = src[3]
            _check_alpha_overlap(a_src, fin.depth, dst, fout.depth)
            self._alpha_tail(lambda: self.apply_rgb_to_yuv(
                src, dst[:3], pix_fmt=pix_fmt, out_pix_fmt=fout.colour.name, interp=interp, matrix_out=matrix_out,
                range_out=range_out, row0=row0, rows=rows, dither=dither, lut=lut, intermediate_pix_fmt=intermediate_pix_fmt,
                prologue_out_range=prologue_out_range), [(fout, dst)], a_src, fin.depth, w, h, row0, rows, slot)
            return dst
        if intermediate_pix_fmt is not None:
            return self.apply_rgb_full_range(src, dst, pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt,
                                             intermediate_pix_fmt=intermediate_pix_fmt, prologue_out_range=prologue_out_range,
                                             matrix=matrix_out, interp=interp, range_out=range_out, row0=row0, rows=rows,
                                             dither=dither, out_size=out_size, resize_chunk=resize_chunk)
        planar, packed, w, h, nf, lead = self._rgb_source(src, fin)
        if out_size is not None:
            kw = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, interp=interp, matrix_out=matrix_out, range_out=range_out,
                      dither=dither, lut=lut)
            if fin.packed:
                squeeze = src.dim() == 3
                s4 = src.unsqueeze(0) if squeeze else src
                d3 = dst if dst is None or not squeeze else [t.unsqueeze(0) for t in dst]
                out = self._lut_then_resize([s4], d3, None, fout, w, h, out_size, row0, rows, resize_chunk, None,
                                            lambda s_, d_: self.apply_rgb_to_yuv(s_[0], d_, **kw), src_frames=[s4])
                return dst if dst is not None else [t[0] for t in out] if squeeze else out
            return self._lut_then_resize(src, dst, PixFmt(fin.name, "gbr", fin.depth, 0, 0, True), fout, w, h, out_size, row0,
                                         rows, resize_chunk, None, lambda s_, d_: self.apply_rgb_to_yuv(s_, d_, **kw))
        if dst is None:
            dst = _new_planes(fout, w, h, lead, _yuv_out_dtype(fout.depth, None), self.device)      # (no dtype to inherit: int16)
        _check_planes(dst, fout, w, h, "destination")
        d, nfd = _planes_struct(dst, self.device)
        if nf != nfd:
            raise ValueError("src and dst disagree on the number of frames")
        rows = h - row0 if rows is None else rows
        if dither == "error_diffusion" and (row0 != 0 or rows != h):
            raise ValueError("error-diffusion dither couples the rows of a frame: whole frames only")
        _check_not_in_place([src] if fin.packed else src[:3], dst, _RGB2YUV_IN_PLACE)
        p = _yuv_params(_native.fmt_code(fin.depth, 0, 0), fout.code, fin.depth, matrix_out, matrix_out, range_out, range_out,
                        range_out)
        mode = _native.INTERP[interp] if lut else _native.INTERP_NONE
        with self._lock:
            self._bind_stream()
            if fin.floating:
                _native.check(self._lib.lutr_apply_rgbf_to_yuv(
                    self._ctx, C.byref(p), mode, _native.DITHER[dither], w, h, nf, C.byref(planar), C.byref(d), row0, rows))
                return dst
            _native.check(self._lib.lutr_apply_rgb_to_yuv(
                self._ctx, C.byref(p), mode, _native.DITHER[dither], fin.code, w, h, nf,
                C.byref(planar) if planar is not None else None, C.byref(packed) if packed is not None else None, C.byref(d),
                row0, rows))
        return dst

    # -- the stage stack on an RGB source -----------------------
    def apply_rgb_stack(self, src, dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                        out_pix_fmt: Optional[str] = None, stages, cdl: Optional[Cdl] = None,
                        rgb_matrix: Optional[RgbMatrix] = None, matrix_out: str = "smpte170m", range_out: str = "tv",
                        row0: int = 0, rows: Optional[int] = None, **other):
        """The ordered stack of `apply_yuv_stack` -- 1..4 stages out of "lut3d", "lut3d2", "lut1d", "cdl", "matrix", each at most
        once, in any order, every lut3d stage with its own mode -- on an RGB source, in one pass (lutr_apply_rgb_stack; DESIGN.md
        3.26).  `src` is `apply_rgb_to_yuv`'s: three gbrp-ordered planes (G, B, R; `pix_fmt` = gbrp, gbrp9le .. gbrp16le; gbrap*
        with its alpha plane) or one [F,]H,W,C packed tensor (a name of `_native.PACKED_FORMATS`).  Its codes enter the list as
        they are (a 16-bit word above 2^depth - 1 acts as that); the list runs at the source's depth.  `out_pix_fmt` is planar
        YUV (4:2:0 / 4:2:2 / 4:4:4 at 8..16 bit, through `apply_rgb_to_yuv`'s output stage with `matrix_out` / `range_out`; not in
        place), or gbrp* / gbrap* at the source's depth -- the default for a planar source -- where the final codes are stored as
        they are and `dst` may be `src`.  Alpha (gbrap*, a packed name's real A) goes past the list as in `apply_rgb_to_yuv`.
        ("lut3d",) gives the bits of `apply_rgb_to_yuv` / `apply_rgb`, ("lut1d",) into gbrp* those of `apply_rgb_lut1d`.  A float
        source, a packed destination, a gbrp destination of another depth, dither, out_size, chroma_loc, strength, matte,
        premultiplied alpha, a second output and the full-range composition are ValueErrors naming them
        (`formats.check_rgb_stack_options`)."""
        st, fin, fout, (arr, n, k, m) = _stack_front(
            self, "apply_rgb_stack", check_rgb_stack_options,
            ("dither", "chroma_loc", "out_size", "alpha_mode", "out2_pix_fmt", "strength", "matte", "intermediate_pix_fmt"),
            pix_fmt, out_pix_fmt, stages, cdl, rgb_matrix, other)
        to_rgb = fout.family == "gbr"
        planar, packed, w, h, nf, lead = self._rgb_source(src, fin)
        if dst is None:
            dtype = (torch.uint8 if fout.depth <= 8 else torch.int16) if fin.packed or not to_rgb else src[0].dtype
            dst = _new_planes(fout, w, h, lead, dtype if to_rgb else _yuv_out_dtype(fout.depth, None), self.device)
        _check_planes(dst, fout, w, h, "destination")
        if fout.alpha:
            # the colour planes through this very call under the three-plane name, then alpha from gbrap*'s fourth plane or a
            # packed name's real A on the same stream -- any other source fills it
            a_src, slot = None, None
            if fin.packed and fin.alpha_slot is not None:
                a_src, slot = src, fin.alpha_slot
            elif not fin.packed and fin.nplanes == 4:
                a_src = src[3]
            _check_alpha_overlap(a_src, fin.depth, dst, fout.depth)
            self._alpha_tail(lambda: self.apply_rgb_stack(
                src, dst[:3], pix_fmt=pix_fmt, out_pix_fmt=fout.colour.name, stages=st, cdl=cdl, rgb_matrix=rgb_matrix,
                matrix_out=matrix_out, range_out=range_out, row0=row0, rows=rows),
                [(fout, dst)], a_src, fin.depth, w, h, row0, rows, slot)
            return dst
        d, nfd = _planes_struct(dst, self.device)
        if nf != nfd:
            raise ValueError("src and dst disagree on the number of frames")
        rows = h - row0 if rows is None else rows
        colour_src = [src] if fin.packed else list(src[:3])
        in_place = (to_rgb and not fin.packed and all(
            a.data_ptr() == b.data_ptr() and a.stride() == b.stride() and a.shape == b.shape for a, b in zip(colour_src, dst)))
        if not in_place:
            _check_not_in_place(colour_src, dst, _RGBSTACK_IN_PLACE if to_rgb else _RGBSTACK_YUV_IN_PLACE)
        p = None
        if not to_rgb:
            p = C.byref(_yuv_params(_native.fmt_code(fin.depth, 0, 0), fout.code, fin.depth, matrix_out, matrix_out, range_out,
                                    range_out, range_out))
        with self._lock:
            self._bind_stream()
            _native.check(self._lib.lutr_apply_rgb_stack(
                self._ctx, p, arr, n, k, m, fin.code, w, h, nf, C.byref(planar) if planar is not None else None,
                C.byref(packed) if packed is not None else None, fin.depth if to_rgb else _native.RGB_STACK_YUV, C.byref(d),
                row0, rows))
        return dst

    # -- YUV source, RGB output --------------------------------
    def apply_yuv_to_rgb(self, src: Sequence[torch.Tensor], dst=None, *, pix_fmt: str, out_pix_fmt: str,
                         interp: str = "tetrahedral", matrix_in: str = "bt709", range_src: str = "tv",
                         range_in: Optional[str] = None, row0: int = 0, rows: Optional[int] = None, lut: bool = True, **refused):
        """Planar YUV frames (Y, Cb, Cr; `pix_fmt` 4:2:0 / 4:2:2 / 4:4:4 at 8..16 bit) -> integer RGB -> lut3d -> stored as RGB, in
        one pass (ffmpeg's `lut3d=...,format=<rgb fmt>`).  `out_pix_fmt` is gbrp .. gbrp16le (three planes G, B, R
        come back), gbrap* (four: alpha last) or a name of `_native.PACKED_FORMATS` (one [F,]H,W,C tensor; a fourth component is
        written opaque).  The LUT runs at the OUTPUT's depth; a source of another depth is converted inside the matrix constants
        (range_src == range_in), or by the full-range prologue (range_src="pc" with another range_in).  Source chroma is
        replicated over its block; always strict arithmetic; not in place.  `dst` is allocated when none is given: uint8 up to 8
        bit, int16 above.  A yuva* source carries its alpha into gbrap* (converted to the output depth; filled opaque for a
        yuv* source or a prologue call), drops it for a 3-component output, and is a ValueError for a 4-component packed one.
        lut=False leaves lut3d out.  chroma_loc, dither, out_size, alpha_mode="premultiplied", cdl, lut1d, stages, strength,
        matte, a second output, a second LUT and semi-planar / packed 4:2:2 / v210 sources are each a ValueError naming it."""
        fin, fout = check_yuv2rgb_options(pix_fmt, out_pix_fmt, **refused)
        if interp not in _native.INTERP:
            raise ValueError(f"lut3d has no interpolation mode '{interp}'")
        mode = _native.INTERP[interp] if lut else _native.INTERP_NONE

        def call(p, kind, w, h, nf, s, d_planar, d_packed, row0, nrows):
            return self._lib.lutr_apply_yuv_to_rgb(self._ctx, p, mode, kind, w, h, nf, s, d_planar, d_packed, row0, nrows)

        return self._yuv2rgb_run(call, src, dst, fin, fout, matrix_in, range_src, range_in, row0, rows)

    def _yuv2rgb_run(self, call, src, dst, fin, fout, matrix_in: str, range_src: str, range_in: Optional[str], row0: int,
                     rows: Optional[int]):
        """The host side `apply_yuv_to_rgb` and `apply_yuv_stack_to_rgb` share behind their option checks: the planes, the
        destination (allocated when none is given), the parameter block, `call(p, dst_kind, w, h, nframes, src, dst_planar,
        dst_packed, row0, rows)` -- the C entry -- and gbrap*'s alpha plane."""
        if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
            raise ValueError(_PLANE_COUNT[fin.nplanes].format(fin.name))
        if not isinstance(src[0], torch.Tensor):
            raise TypeError(_NOT_TENSORS)
        h, w = src[0].shape[-2], src[0].shape[-1]
        _check_planes(src, fin, w, h, "source")
        lead = tuple(src[0].shape[:-2])
        odt = torch.uint8 if fout.depth <= 8 else torch.int16
        packed = isinstance(fout, RgbSource)
        s, nf = _planes_struct(src[:3], self.device)
        if packed:
            if dst is None:
                dst = torch.empty(lead + (h, w, fout.ncomp), dtype=odt, device=self.device)
            d = _packed_struct(dst, fout.name, fout.ncomp, fout.depth, self.device, True)
            if tuple(dst.shape[-3:-1]) != (h, w):
                raise ValueError(f"the destination image is {tuple(dst.shape[-3:-1])}, the frame is {(h, w)}")
            nfd = dst.shape[0] if dst.dim() == 4 else 1
        else:
            if dst is None:
                dst = _new_planes(fout, w, h, lead, odt, self.device)
            _check_planes(dst, fout, w, h, "destination")
            d, nfd = _planes_struct(dst[:3], self.device)
        if nf != nfd:
            raise ValueError("src and dst disagree on the number of frames")
        _check_not_in_place(src[:3], [dst] if packed else dst[:3], _YUV2RGB_IN_PLACE)
        rin = range_in or range_src
        p = _yuv_params(fin.colour.code, _native.fmt_code(fout.depth, 0, 0), fout.depth, matrix_in, matrix_in, range_src, rin, rin)
        nrows = h - row0 if rows is None else rows

        def colour():
            self._bind_stream()
            _native.check(call(C.byref(p), fout.code if packed else 0, w, h, nf, C.byref(s), None if packed else C.byref(d),
                               C.byref(d) if packed else None, row0, nrows))

        if not packed and fout.alpha:
            # gbrap*: the colour planes, then the alpha plane on the same stream; a prologue call fills
            a_src = src[3] if fin.alpha and rin == range_src else None
            _check_alpha_overlap(a_src, fin.depth, dst, fout.depth)
            self._alpha_tail(colour, [(fout, dst)], a_src, fin.depth, w, h, row0, rows)
        else:
            with self._lock:
                colour()
        return dst

    # -- the stage stack from a YUV source into an RGB frame -----
    def apply_yuv_stack_to_rgb(self, src: Sequence[torch.Tensor], dst=None, *, pix_fmt: str, out_pix_fmt: str, stages,
                               cdl: Optional[Cdl] = None, rgb_matrix: Optional[RgbMatrix] = None, matrix_in: str = "bt709",
                               range_src: str = "tv", range_in: Optional[str] = None, row0: int = 0, rows: Optional[int] = None,
                               **other):
        """`apply_yuv_to_rgb` with the ordered stack of `apply_rgb_stack` in place of lut3d -- 1..4 stages out of "lut3d",
        "lut3d2", "lut1d", "cdl", "matrix", each at most once, in any order, every lut3d stage with its own mode -- in one pass
        (lutr_apply_yuv_stack_to_rgb).  `src`, `dst`, `pix_fmt`, `out_pix_fmt`, `matrix_in`, `range_src`,
        `range_in`, `row0` / `rows` and the alpha rules are `apply_yuv_to_rgb`'s: planar YUV (4:2:0 / 4:2:2 / 4:4:4 at 8..16 bit,
        yuva* too) converted to integer RGB codes at the OUTPUT's depth, where the list runs; its final codes are stored as they
        are into gbrp* / gbrap* planes or one packed image (a fourth component opaque).  Not in place.  ("lut3d",) gives the bits
        of `apply_yuv_to_rgb`; any list gives those of `apply_rgb_stack` from gbrp* into gbrp* on the output of
        `apply_yuv_to_rgb(lut=False)`.  Dither, out_size, chroma_loc, strength, matte, premultiplied alpha, a second output, a
        float destination, semi-planar / packed 4:2:2 / v210 sources and alpha into a 4-component packed destination are
        ValueErrors naming them (`formats.check_yuv2rgb_stack_options`)."""
        _st, fin, fout, stack = _stack_front(
            self, "apply_yuv_stack_to_rgb", check_yuv2rgb_stack_options,
            ("dither", "engine_dither", "chroma_loc", "out_size", "alpha_mode", "out2_pix_fmt", "strength", "matte"),
            pix_fmt, out_pix_fmt, stages, cdl, rgb_matrix, other)

        def call(p, kind, w, h, nf, s, d_planar, d_packed, row0, nrows):
            return self._lib.lutr_apply_yuv_stack_to_rgb(self._ctx, p, *stack, kind, w, h, nf, s, d_planar, d_packed, row0, nrows)

        return self._yuv2rgb_run(call, src, dst, fin, fout, matrix_in, range_src, range_in, row0, rows)

    def apply_rgb_full_range(self, src, dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, out_pix_fmt: str,
                             intermediate_pix_fmt: str, prologue_out_range: Optional[str], matrix: Optional[str],
                             interp: str = "tetrahedral", range_out: str = "tv", row0: int = 0, rows: Optional[int] = None,
                             dither: str = "none", out_size=None, resize_chunk: Optional[int] = None):
        """An RGB source flagged full range (DESIGN.md 3.9 point 6).  The reference puts `scale=in_range=pc:out_range=R,
        format=<8-bit yuv>` AHEAD of lut3d for it (ffmpeg.py:212-233), so the LUT runs on an 8-bit YUV frame.  Kept by
        composition, two launches on the engine's stream with no host wait: stage 0 is `apply_rgb_to_yuv` without the LUT into
        engine-owned scratch (`intermediate_pix_fmt` at 8 bit, range R = `prologue_out_range`, matrix `matrix` or smpte170m),
        then `apply_yuv` from that frame to `out_pix_fmt`.  The three plan fields are `LutPlan.intermediate_pix_fmt`,
        `.prologue_out_range` and `.matrix`."""
        fin = parse_rgb_source(pix_fmt)
        if fin is None:
            raise ValueError(f"apply_rgb_full_range takes gbrp*, gbrpf32le or packed RGB sources, not '{pix_fmt}'")
        mid = parse_pix_fmt(intermediate_pix_fmt)
        if mid.family != "yuv" or mid.depth != 8:
            raise ValueError(f"the full-range intermediate is an 8-bit planar YUV format, not '{intermediate_pix_fmt}'")
        rng = prologue_out_range or "pc"
        if rng not in _native.RANGE:
            raise ValueError(f"unknown range '{rng}'")
        m = matrix or "smpte170m"
        _, _, w, h, nf, lead = self._rgb_source(src, fin)
        with self._lock:
            tmp = self._scratch("fr", mid, w, h, nf, torch.uint8)
            if not lead:
                tmp = [t[0] for t in tmp]
            self.apply_rgb_to_yuv(src, tmp, pix_fmt=pix_fmt, out_pix_fmt=mid.name, lut=False, matrix_out=m, range_out=rng,
                                  row0=row0, rows=rows)
            return self.apply_yuv(tmp, dst, pix_fmt=mid.name, out_pix_fmt=out_pix_fmt, interp=interp, matrix_in=m, matrix_out=m,
                                  range_src=rng, range_in=rng, range_out=range_out, lut_depth=8, row0=row0, rows=rows,
                                  dither=dither, out_size=out_size, resize_chunk=resize_chunk)


def _yuv_constants(entry: str, *extra, **kw) -> np.ndarray:
    p = _native.YuvParams()
    for k, v in kw.items():
        setattr(p, k, v)
    out = (C.c_float * 32)()
    _native.check(getattr(_native.load(), entry)(C.byref(p), *extra, out))
    return np.array(list(out), dtype=np.float32)


def yuv_constants(**kw) -> np.ndarray:
    """The 32-float constant block liblutr derives for a lutr_yuv_params (host only, no GPU)."""
    return _yuv_constants("lutr_yuv_constants", **kw)


def yuv_constants_xsub(**kw) -> np.ndarray:
    """`yuv_constants` for a chroma subsampling change (lutr_yuv_constants_xsub): the block mean's n is the output block's."""
    return _yuv_constants("lutr_yuv_constants_xsub", **kw)


def yuv_constants_rgb2yuv(**kw) -> np.ndarray:
    """The constant block of `apply_rgb_to_yuv` (lutr_yuv_constants_rgb2yuv): fmt_out, lut_depth, matrix_out and range_out count."""
    return _yuv_constants("lutr_yuv_constants_rgb2yuv", **kw)


def yuv_constants_yuv2rgb(**kw) -> np.ndarray:
    """The constant block of `apply_yuv_to_rgb` (lutr_yuv_constants_yuv2rgb): fmt_in, lut_depth, matrix_in, range_src and range_in
    count."""
    return _yuv_constants("lutr_yuv_constants_yuv2rgb", **kw)


def yuv_constants_sited(chroma_loc: Optional[str], **kw) -> np.ndarray:
    """`yuv_constants` with the sited down-sampling's 1/n folded into cbr..crb (lutr_yuv_constants_sited)."""
    return _yuv_constants("lutr_yuv_constants_sited", chroma_loc_code(chroma_loc), **kw)


def _tensor_from_ptr(ptr: int, count: int, device: torch.device) -> torch.Tensor:
    """Wrap `count` device floats at `ptr` as a tensor without copying (__cuda_array_interface__)."""

    class _Holder:
        pass

    h = _Holder()
    h.__cuda_array_interface__ = {
        "shape": (count,), "typestr": "<f4", "data": (ptr, False), "version": 2, "strides": None}
    return torch.as_tensor(h, device=device)
