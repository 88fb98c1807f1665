"""Host-resident frame queue -> GPU -> host, overlapped (BASELINE.json config 5).

What the reference gets from ffmpeg's internal frame queue when it runs
`ffmpeg -i in -vf ...lut3d... out` (/root/reference/src/lut_renderer/task_manager.py:145-151),
rebuilt for frames that live in host memory: a ring of pinned host buffers, three HIP streams
(host->device, kernels, device->host) and events between them, so the PCIe copies of batch
i+1 / i-1 run under the LUT kernel of batch i (`hipMemcpyAsync` double buffering).  The LUT
kernel itself is ~60x faster than PCIe Gen5 x16 can feed it, so this pipeline is PCIe-bound by
construction; `bench.py --pipeline host` reports its rate beside (never as) the HBM-resident metric.

Frames are rawvideo-style: planes back to back (Y, Cb, Cr), frames back to back in a batch.
"""
from __future__ import annotations

import os
import stat
from dataclasses import dataclass
from typing import Callable, Iterable, Iterator, List, Optional

import numpy as np
import torch

from .engine import LutEngine
from .params import strength_keys
from .formats import (MATTE_PIX_FMTS, PACKED_STACK_TAIL, PACKED_STAGES_EXCLUSIVE, RGB_STACK_TAIL, SEMI_STACK_TAIL, SEMI_STAGES_EXCLUSIVE,
                      YUV2RGB_STACK_TAIL, RgbSource, check_packed_stack_options,
                      check_alpha_mode, check_cdl_options, check_chain_options, check_dual_options, check_lut1d_options,
                      check_premul_options, check_rgb_stack_options, check_semi_stack_options, check_stack_options, check_yuv2rgb_options, check_yuv2rgb_stack_options, held_resources, parse_rgb_out,
                      parse_rgb_source, parse_size, premul_to_yuv, refuse_alpha_resize, yuv_side, _YUV2RGB_NOT_TAKEN)


@dataclass
class FrameLayout:
    """Byte layout of one YUV (or gbrp) frame in a rawvideo stream: the planes of `fmt` back to back -- three for a planar
    format (four for yuva* / gbrap*, alpha last: ffmpeg's rawvideo order), luma then the chroma pairs for a semi-planar one, the one buffer of a packed 4:2:2 one (3.12) or of
    v210 (3.14: 32-bit words, rows of 128 * ceil(w / 48) bytes)."""
    fmt: object      # PixFmt | SemiFmt | PackedYuvFmt | V210Fmt
    width: int
    height: int

    @property
    def itemsize(self) -> int:
        return getattr(self.fmt, "itemsize", 1 if self.fmt.depth <= 8 else 2)

    @property
    def plane_shapes(self) -> List[tuple]:
        return [self.fmt.plane_shape(i, self.width, self.height) for i in range(self.fmt.nplanes)]

    @property
    def plane_bytes(self) -> List[int]:
        return [h * w * self.itemsize for h, w in self.plane_shapes]

    @property
    def frame_bytes(self) -> int:
        return sum(self.plane_bytes)

    def plane_views(self, buf: torch.Tensor, nframes: int) -> List[torch.Tensor]:
        """[F,H,W] views of the planes inside a flat uint8 buffer of `nframes` frames."""
        dt = {1: torch.uint8, 2: torch.int16, 4: torch.int32}[self.itemsize]
        typed = buf.view(dt)
        fe = self.frame_bytes // self.itemsize
        out, off = [], 0
        for (h, w), nbytes in zip(self.plane_shapes, self.plane_bytes):
            out.append(torch.as_strided(typed, (nframes, h, w), (fe, w, 1), off))
            off += nbytes // self.itemsize
        return out


def yuv_layout(pix_fmt: str, width: int, height: int) -> FrameLayout:
    """The `FrameLayout` of a planar, semi-planar, packed 4:2:2 or v210 YUV name (or gbrp)."""
    return FrameLayout(yuv_side(pix_fmt), width, height)


@dataclass
class PackedFrameLayout:
    """Byte layout of one packed RGB frame in a rawvideo stream: h x w pixels of `ncomp` components.  The input side of an RGB
    source, and the output side of a YUV source with an RGB output."""
    fmt: RgbSource
    width: int
    height: int

    @property
    def itemsize(self) -> int:
        return self.fmt.itemsize

    @property
    def frame_bytes(self) -> int:
        return self.height * self.width * self.fmt.ncomp * self.itemsize

    def image_view(self, buf: torch.Tensor, nframes: int) -> torch.Tensor:
        """The [F,H,W,C] view of `nframes` frames inside a flat uint8 buffer."""
        dt = torch.uint8 if self.itemsize == 1 else torch.int16
        n = nframes * self.frame_bytes // self.itemsize
        return buf.view(dt)[:n].view(nframes, self.height, self.width, self.fmt.ncomp)


@dataclass
class FloatFrameLayout:
    """Byte layout of one planar float RGB frame (gbrpf32le / gbrapf32le) in a rawvideo stream: `fmt.nplanes` planes of h x w
    32-bit floats, back to back (G, B, R[, A])."""
    fmt: RgbSource
    width: int
    height: int

    @property
    def itemsize(self) -> int:
        return 4

    @property
    def frame_bytes(self) -> int:
        return self.fmt.nplanes * self.height * self.width * 4

    def plane_views(self, buf: torch.Tensor, nframes: int) -> List[torch.Tensor]:
        """[F,H,W] float32 views of the planes inside a flat uint8 buffer of `nframes` frames."""
        h, w = self.height, self.width
        typed = buf.view(torch.float32)
        return [torch.as_strided(typed, (nframes, h, w), (self.fmt.nplanes * h * w, w, 1), i * h * w)
                for i in range(self.fmt.nplanes)]


def input_layout(pix_fmt: str, width: int, height: int):
    """The layout of a rawvideo input: `PackedFrameLayout` for a packed RGB name, `FloatFrameLayout` for a planar float one,
    else `FrameLayout` (planar, semi-planar or packed 4:2:2 YUV, or gbrp)."""
    rgb = parse_rgb_source(pix_fmt)
    if rgb is not None and rgb.packed:
        return PackedFrameLayout(rgb, width, height)
    if rgb is not None and rgb.floating:
        return FloatFrameLayout(rgb, width, height)
    return yuv_layout(pix_fmt, width, height)


def output_layout(pix_fmt: str, width: int, height: int):
    """The layout of a rawvideo RGB output: `PackedFrameLayout` for a packed name, `FrameLayout` for gbrp* /
    gbrap* (planes G, B, R[, A] back to back: ffmpeg's rawvideo order)."""
    fmt = parse_rgb_out(pix_fmt)
    return PackedFrameLayout(fmt, width, height) if isinstance(fmt, RgbSource) else FrameLayout(fmt, width, height)


def dual_layout(pix_fmt: str, out_pix_fmt: Optional[str], second_pix_fmt: Optional[str], width: int, height: int, out_size=None,
                apply_kw: Optional[dict] = None) -> Optional[FrameLayout]:
    """The layout of `HostPipeline`'s second output ring, or None without `second_pix_fmt`.  Planar YUV on
    every side, no dither, chroma_loc or out_size (ValueError, `formats.check_dual_options`)."""
    if second_pix_fmt is None:
        return None
    kw = apply_kw or {}
    _, _, f2 = check_dual_options(pix_fmt, out_pix_fmt, second_pix_fmt, kw.get("dither", "none"), kw.get("chroma_loc"), out_size)
    return FrameLayout(f2, width, height)


class MatteReader:
    """The matte of a stream: raw frames of `width` x `height` gray samples (`pix_fmt`: gray, or gray10le ..
    gray16le in little-endian 16-bit words), read in lockstep with the input batches.  A regular file that holds exactly one frame
    is a still: it is read once (`still`, [H, W]) and serves the whole stream.  Anything else is a stream of one matte per
    frame; `read(n)` gives the next n as [n, H, W] and raises a ValueError naming the frame number when the stream ends before
    the input does.  No device work: `HostPipeline` uploads what this reads."""

    def __init__(self, path, pix_fmt: str, width: int, height: int):
        if pix_fmt not in MATTE_PIX_FMTS:
            raise ValueError(f"unknown matte pixel format '{pix_fmt}' ({' | '.join(MATTE_PIX_FMTS)})")
        if str(path) == "-":
            raise ValueError("the matte is a file or FIFO, not '-': stdin carries the input")
        self.path, self.pix_fmt, self.depth = str(path), pix_fmt, MATTE_PIX_FMTS[pix_fmt]
        self.width, self.height = int(width), int(height)
        self.dtype = np.dtype(np.uint8) if self.depth == 8 else np.dtype("<u2")
        self.frame_bytes = self.width * self.height * self.dtype.itemsize
        self.frames_read = 0
        self.still = None
        st = os.stat(self.path)
        self._f = open(self.path, "rb")
        if stat.S_ISREG(st.st_mode) and st.st_size == self.frame_bytes:
            self.still = self.read(1)[0]
            self.close()

    def read(self, n: int) -> np.ndarray:
        """The mattes of the next `n` frames of the stream, [n, H, W]."""
        buf = bytearray(n * self.frame_bytes)
        view, got = memoryview(buf), 0
        while got < len(view):                               # a FIFO returns short reads: collect the whole batch (or EOF)
            k = self._f.readinto(view[got:])
            if not k:
                break
            got += k
        if got < len(view):
            raise ValueError(f"matte '{self.path}' ended at frame {self.frames_read + got // self.frame_bytes}: the input goes on "
                             f"(a matte has one frame for the whole stream or one for every frame)")
        self.frames_read += n
        return np.frombuffer(buf, dtype=self.dtype).reshape(n, self.height, self.width)

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None


class HostPipeline:
    """Apply the LUT to batches of host frames with copies overlapped against compute."""

    def __init__(self, engine: LutEngine, pix_fmt: str, width: int, height: int, batch: int = 8, slots: int = 3,
                 out_pix_fmt: Optional[str] = None, out_size=None, second_pix_fmt: Optional[str] = None, chain: bool = False, lut1d: bool = False,
                 rgb_out: Optional[str] = None, rgb_out_stages=None, **apply_kw):
        """Settles, once, which engine method every batch goes through (`entry`) and the layouts of its source and destination.
        `out_size` = (w, h) or "WxH": the engine resizes every frame to it and the output layout has that size.
        `second_pix_fmt`: a second planar YUV output from the same pass with a pinned output ring of its own
        (`fout2`); `run` then takes a second drain.
        `chain`: the engine holds a second LUT (`set_lut2`) and every batch goes through `apply_yuv_chain`;
        `apply_kw` may carry `interp2`.  Planar YUV without alpha on both sides, no dither, chroma_loc, out_size or second output.
        `lut1d`: the engine holds a 1D LUT (`set_lut1d`) and every batch goes through `apply_yuv_lut1d`;
        `apply_kw["interp"]` None is lut1d alone.
        `rgb_out`: a planar YUV source written as RGB -- gbrp* / gbrap* planes or a packed image -- through
        `apply_yuv_to_rgb`; the output ring has that layout (`output_layout`).  Not with `out_pix_fmt` or anything the pass refuses.
        `rgb_out_stages`: with `rgb_out`, every batch goes through `apply_yuv_stack_to_rgb` with the lattices and
        the 1D LUT the engine holds, `apply_kw["cdl"]` and `apply_kw["rgb_matrix"]`; the output ring is that of `rgb_out`.
        `apply_kw` travels to the engine with every batch.  Of its keywords:
        `stages`: every batch goes through `apply_yuv_stack` with the lattices and the 1D LUT the engine holds and
        `apply_kw["cdl"]`; `chain` / `lut1d` are not set then.
        `strength` (a number) or `strength_keys` ("F:S,..." or `params.strength_keys`' callable) mix the graded frame with the
        source: the keys are read at the frame's number in the stream, counted here across the batches.
        `matte` (a `MatteReader`) scales the strength per pixel: a still is uploaded once, a matte per frame is
        read and uploaded with every input batch; `matte_invert` travels to the engine.
        `rgb_matrix` (an `rgbmatrix.RgbMatrix`): the resource of a matrix stage of `stages`, which travels like the
        CDL; None is not passed on.
        `rgb_stages`: an RGB source through the stage stack -- every batch goes through `apply_rgb_stack` with
        the lattices and the 1D LUT the engine holds, `cdl` and `rgb_matrix`, into planar YUV or gbrp* / gbrap* at the source's
        depth (`out_pix_fmt` None: the latter, for a planar source).
        `semi_stages`: a call with a semi-planar side through the stage stack -- every batch goes through
        `apply_yuv_stack_semi` with the lattices and the 1D LUT the engine holds and `cdl`; the rings are laid out as the two names
        say.  Not with `stages`, `rgb_stages`, `rgb_out_stages` or `rgb_out`.
        `packed_stages`: a call with a packed 4:2:2 or v210 side through the stage stack -- every batch goes
        through `apply_yuv_stack_packed` the same way.  Not with another stage list or `rgb_out`.
        `alpha_mode` travels like `chroma_loc`, "straight" is not passed on; `cdl` (a `cdl.Cdl`)
        likewise, None is not passed on."""
        self.eng = engine
        self.batch, self.slots = int(batch), int(slots)
        self.frames_submitted = 0
        self.rgb_out_stack = rgb_out_stages is not None
        self.semi_stack = apply_kw.get("semi_stages") is not None
        self.packed_stack = apply_kw.get("packed_stages") is not None
        self.rgb_stack = not self.rgb_out_stack and not self.semi_stack and not self.packed_stack and \
            apply_kw.get("rgb_stages") is not None
        if self.rgb_out_stack or self.rgb_stack or self.semi_stack or self.packed_stack:
            # the four newer stack routes: what each refuses of its own, its family's check, then one tail
            if self.packed_stack:
                flag, tail, check = "packed_stages", PACKED_STACK_TAIL, check_packed_stack_options
                listed, out_name = apply_kw["packed_stages"], out_pix_fmt
                carried = ("matrix_in", "matrix_out", "range_src", "range_in", "range_out", "lut_depth")
                refusable = ("dither", "chroma_loc", "alpha_mode", "strength", "matte")
                if self.rgb_out_stack or self.semi_stack or apply_kw.get("stages") is not None or \
                        apply_kw.get("rgb_stages") is not None:
                    raise ValueError(PACKED_STAGES_EXCLUSIVE)
                if rgb_out is not None:
                    raise ValueError(f"rgb_out ('{rgb_out}') names the RGB output of a planar YUV source: with packed_stages the "
                                     f"output is out_pix_fmt")
                self.rgb_out_stack = False
            elif self.semi_stack:
                flag, tail, check = "semi_stages", SEMI_STACK_TAIL, check_semi_stack_options
                listed, out_name = apply_kw["semi_stages"], out_pix_fmt
                carried = ("matrix_in", "matrix_out", "range_src", "range_in", "range_out", "lut_depth")
                refusable = ("dither", "chroma_loc", "alpha_mode", "strength", "matte")
                if self.rgb_out_stack or apply_kw.get("stages") is not None or apply_kw.get("rgb_stages") is not None:
                    raise ValueError(SEMI_STAGES_EXCLUSIVE)
                if rgb_out is not None:
                    raise ValueError(f"rgb_out ('{rgb_out}') names the RGB output of a planar YUV source: with semi_stages the output "
                                     f"is out_pix_fmt")
                self.rgb_out_stack = False
            elif self.rgb_out_stack:
                flag, tail, check = "rgb_out_stages", YUV2RGB_STACK_TAIL, check_yuv2rgb_stack_options
                listed, out_name, carried = rgb_out_stages, rgb_out, ("matrix_in", "range_src", "range_in")
                refusable = ("dither", "engine_dither", "chroma_loc", "alpha_mode", "strength", "matte")
                if rgb_out is None:
                    raise ValueError("rgb_out_stages is the stage list of a YUV source written as RGB: it needs rgb_out")
                if apply_kw.get("stages") is not None or apply_kw.get("rgb_stages") is not None:
                    raise ValueError("rgb_out_stages and stages / rgb_stages are mutually exclusive")
                if out_pix_fmt:
                    raise ValueError(f"rgb_out ('{rgb_out}') and out_pix_fmt ('{out_pix_fmt}') are mutually exclusive")
            else:
                flag, tail, check = "rgb_stages", RGB_STACK_TAIL, check_rgb_stack_options
                listed, out_name, carried = apply_kw["rgb_stages"], out_pix_fmt, ("matrix_out", "range_out")
                refusable = ("dither", "chroma_loc", "alpha_mode", "strength", "matte", "intermediate_pix_fmt")
                if apply_kw.get("stages") is not None:
                    raise ValueError("stages and rgb_stages are mutually exclusive")
                if rgb_out is not None:
                    raise ValueError(f"rgb_out ('{rgb_out}') names the RGB output of a YUV source: with rgb_stages the output is out_pix_fmt")
            if chain or lut1d:
                raise ValueError(f"a stage stack names its lut3d2 / lut1d stages itself: chain / lut1d are not set with {flag}")
            st, _fin, fout = check(pix_fmt, out_name, stages=listed, cdl=apply_kw.get("cdl") is not None, **held_resources(engine),
                                   rgb_matrix=apply_kw.get("rgb_matrix") is not None, out_size=out_size, out2_pix_fmt=second_pix_fmt,
                                   **{k: apply_kw[k] for k in refusable if k in apply_kw})
            if apply_kw.get("strength_keys") is not None:
                raise ValueError(f"a LUT strength (strength_keys) is not supported with {tail}")
            self.stack = self.chain = self.lut1d = self.float_out = False
            self.rgb, self.rgb_out = self.rgb_stack, self.rgb_out_stack
            self.matte = self.strength_keys = self.fout2 = None
            self.fin = input_layout(pix_fmt, width, height)
            self.fout = output_layout(rgb_out, width, height) if self.rgb_out_stack else yuv_layout(fout.name, width, height)
            names = (self.fin.fmt.name, self.fout.fmt.name) if self.rgb_out_stack else (pix_fmt, fout.name)
            self.kw = dict({k: apply_kw[k] for k in ("cdl", "rgb_matrix") + carried if apply_kw.get(k) is not None}, stages=st,
                           pix_fmt=names[0], out_pix_fmt=names[1])
            if self.packed_stack:
                self.kw["width"] = width                       # (a packed row cannot tell an odd width, a v210 row none)
            self._settle("apply_yuv_stack_packed" if self.packed_stack else "apply_yuv_stack_semi" if self.semi_stack
                         else "apply_yuv_stack_to_rgb" if self.rgb_out_stack else "apply_rgb_stack", slots)
            return
        self.rgb_out = rgb_out is not None
        if self.rgb_out:
            if out_pix_fmt:
                raise ValueError(f"rgb_out ('{rgb_out}') and out_pix_fmt ('{out_pix_fmt}') are mutually exclusive")
            check_yuv2rgb_options(pix_fmt, rgb_out, out_size=out_size, out2_pix_fmt=second_pix_fmt, lut2=bool(chain),
                                  lut1d=True if lut1d else None,
                                  **{k: v for k, v in apply_kw.items() if k in _YUV2RGB_NOT_TAKEN and k not in ("out_size", "lut1d")})
            apply_kw = {k: v for k, v in apply_kw.items() if k not in _YUV2RGB_NOT_TAKEN}
        stages = apply_kw.get("stages")
        self.stack = stages is not None
        if apply_kw.get("rgb_matrix") is None:
            apply_kw.pop("rgb_matrix", None)
        elif not self.stack:
            raise ValueError("an RGB matrix is a stage of the stage stack: it needs stages")
        self.matte = apply_kw.pop("matte", None)
        if self.matte is None:
            apply_kw.pop("matte_invert", None)
        elif not self.stack:
            raise ValueError("a matte runs in the stage stack: it needs stages")
        elif (self.matte.width, self.matte.height) != (width, height):
            raise ValueError(f"the matte is {self.matte.width}x{self.matte.height}, the frames are {width}x{height}")
        keys = apply_kw.pop("strength_keys", None)
        if keys is not None and apply_kw.get("strength") is not None:
            raise ValueError("strength and strength_keys are mutually exclusive")
        self.strength_keys = strength_keys(keys) if isinstance(keys, str) else keys
        if apply_kw.get("strength") is None:
            apply_kw.pop("strength", None)
        mixed = keys is not None or "strength" in apply_kw
        if mixed and not self.stack:
            raise ValueError("strength runs in the stage stack: it needs stages")
        if self.stack:
            if chain or lut1d:
                raise ValueError("a stage stack names its lut3d2 / lut1d stages itself: chain / lut1d are not set with stages")
            check_stack_options(pix_fmt, out_pix_fmt, stages=stages, cdl=apply_kw.get("cdl") is not None, **held_resources(engine),
                                dither=apply_kw.get("dither", "none"), chroma_loc=apply_kw.get("chroma_loc"), out_size=out_size,
                                alpha_mode=apply_kw.get("alpha_mode", "straight"), out2_pix_fmt=second_pix_fmt,
                                strength=apply_kw.get("strength", 1.0 if mixed else None), matte=self.matte is not None,
                                rgb_matrix="rgb_matrix" in apply_kw)
            apply_kw = {k: v for k, v in apply_kw.items() if k not in ("dither", "alpha_mode", "interp") and
                        not (k == "cdl" and v is None)}
        self.chain, self.lut1d = bool(chain), bool(lut1d)
        if check_alpha_mode(apply_kw.get("alpha_mode", "straight")):
            check_premul_options(pix_fmt, out_pix_fmt, dither=apply_kw.get("dither", "none"), chroma_loc=apply_kw.get("chroma_loc"),
                                 out_size=out_size, range_src=apply_kw.get("range_src", "tv"), range_in=apply_kw.get("range_in"),
                                 lut_depth=apply_kw.get("lut_depth"), out2_pix_fmt=second_pix_fmt, lut2=self.chain,
                                 to_yuv=premul_to_yuv(pix_fmt, out_pix_fmt))
        else:
            apply_kw = {k: v for k, v in apply_kw.items() if k != "alpha_mode"}
        if self.stack:                                         # (checked above: the CDL is a stage of the stack)
            pass
        elif apply_kw.get("cdl") is not None:
            check_cdl_options(pix_fmt, out_pix_fmt, dither=apply_kw.get("dither", "none"), chroma_loc=apply_kw.get("chroma_loc"),
                              out_size=out_size, alpha_mode=apply_kw.get("alpha_mode", "straight"), out2_pix_fmt=second_pix_fmt,
                              lut2=self.chain, prelut=bool(getattr(engine, "_has_prelut", False)))
        else:
            apply_kw = {k: v for k, v in apply_kw.items() if k != "cdl"}
        if self.lut1d:
            check_lut1d_options(pix_fmt, out_pix_fmt, dither=apply_kw.get("dither", "none"), chroma_loc=apply_kw.get("chroma_loc"),
                                out_size=out_size, alpha_mode=apply_kw.get("alpha_mode", "straight"), out2_pix_fmt=second_pix_fmt,
                                lut2=self.chain, cdl=apply_kw.get("cdl") is not None, loaded=bool(getattr(engine, "n1d", 0)))
            apply_kw = {k: v for k, v in apply_kw.items() if k != "dither"}
        if self.chain:
            check_chain_options(pix_fmt, out_pix_fmt, apply_kw.get("dither", "none"), apply_kw.get("chroma_loc"), out_size,
                                second_pix_fmt)
            apply_kw = {k: v for k, v in apply_kw.items() if k != "dither"}
        self.fout2 = dual_layout(pix_fmt, out_pix_fmt, second_pix_fmt, width, height, out_size, apply_kw)
        self.fin = input_layout(pix_fmt, width, height)
        src_rgb = parse_rgb_source(pix_fmt)
        self.rgb = src_rgb is not None                         # an RGB source: apply_rgb_to_yuv
        # a float source without an output format, or with a float one, stays float: apply_rgb_float
        out_rgb = parse_rgb_source(out_pix_fmt) if out_pix_fmt else src_rgb
        self.float_out = self.rgb and src_rgb.floating and out_rgb is not None and out_rgb.floating
        if self.rgb and not out_pix_fmt and not self.float_out:
            raise ValueError("an RGB source needs out_pix_fmt (a planar YUV format)")
        ow, oh = (width, height) if out_size is None else parse_size(out_size)
        refuse_alpha_resize(out_pix_fmt or pix_fmt, out_size)
        if self.float_out:
            if out_size is not None or out_rgb.nplanes > src_rgb.nplanes:
                raise ValueError("a float output takes no out_size and cannot add an alpha plane")
            self.fout = FloatFrameLayout(out_rgb, ow, oh)
        elif self.rgb_out:
            self.fout = output_layout(rgb_out, ow, oh)
        else:
            self.fout = yuv_layout(out_pix_fmt or pix_fmt, ow, oh)
        self.kw = dict(apply_kw, pix_fmt=self.fin.fmt.name, out_pix_fmt=self.fout.fmt.name)
        if out_size is not None:
            self.kw["out_size"] = (ow, oh)
        if self.fin.fmt.nplanes == 1 or self.fout.fmt.nplanes == 1:
            self.kw["width"] = width                           # (a packed row cannot tell an odd width)
        self._settle("apply_yuv_to_rgb" if self.rgb_out else "apply_yuv_stack" if self.stack else "apply_yuv_lut1d" if self.lut1d
                     else "apply_yuv_chain" if self.chain else "apply_yuv_dual" if self.fout2 is not None
                     else "apply_rgb_float" if self.float_out else "apply_rgb_to_yuv" if self.rgb else "apply_yuv", slots)

    def _settle(self, entry: str, slots: int) -> None:
        """`entry`, the engine method every batch goes through, and how `_submit` calls it -- with the source and the destination
        viewed as their layouts say, planes or one packed image, and `kw`; the stack, the second output and the float planes each
        have a word of their own to add -- then the rings (`_allocate`)."""
        self.entry = entry
        self._launch = {"apply_yuv_stack": self._launch_stack, "apply_yuv_dual": self._launch_dual,
                        "apply_rgb_float": self._launch_float}.get(entry, self._launch_plain)
        self._allocate(self.eng, slots)

    def _launch_plain(self, src, dst, slot: int, nframes: int, matte) -> None:
        getattr(self.eng, self.entry)(src, dst, **self.kw)

    def _launch_stack(self, src, dst, slot: int, nframes: int, matte) -> None:
        self._run_stack(src, dst, nframes, matte)

    def _launch_dual(self, src, dst, slot: int, nframes: int, matte) -> None:
        self.eng.apply_yuv_dual(src, dst, self.fout2.plane_views(self.d_out2[slot], nframes), **self.kw)

    def _launch_float(self, src, dst, slot: int, nframes: int, matte) -> None:
        self.eng.apply_rgb_float(src[:self.fout.fmt.nplanes], dst, interp=self.kw.get("interp", "tetrahedral"),
                                 alpha_mode=self.kw.get("alpha_mode", "straight"))

    @staticmethod
    def _views(layout, buf: torch.Tensor, nframes: int):
        """`nframes` frames inside a flat buffer as `layout` says: one [F,H,W,C] image for a packed RGB side, else its planes."""
        return layout.image_view(buf, nframes) if isinstance(layout, PackedFrameLayout) else layout.plane_views(buf, nframes)

    def _allocate(self, engine: LutEngine, slots: int) -> None:
        """The pinned host rings, the device rings and the streams of the layouts `__init__` settled."""
        dev = engine.device
        self.h_in = [torch.empty(self.batch * self.fin.frame_bytes, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.h_out = [torch.empty(self.batch * self.fout.frame_bytes, dtype=torch.uint8).pin_memory() for _ in range(slots)]
        self.d_in = [torch.empty(self.batch * self.fin.frame_bytes, dtype=torch.uint8, device=dev) for _ in range(slots)]
        # (zeroed once: a v210 output's row padding is never written by the kernels and goes out with the frame)
        self.d_out = [torch.zeros(self.batch * self.fout.frame_bytes, dtype=torch.uint8, device=dev) for _ in range(slots)]
        if self.fout2 is not None:
            self.kw = {k: v for k, v in self.kw.items() if k != "dither"}
            self.kw["out2_pix_fmt"] = self.fout2.fmt.name
            self.h_out2 = [torch.empty(self.batch * self.fout2.frame_bytes, dtype=torch.uint8).pin_memory() for _ in range(slots)]
            self.d_out2 = [torch.empty(self.batch * self.fout2.frame_bytes, dtype=torch.uint8, device=dev) for _ in range(slots)]
        if self.matte is not None:
            self.kw["matte_depth"] = self.matte.depth
            if self.matte.still is not None:
                self.d_matte = self._matte_tensor(self.matte.still).to(dev)
            else:
                nb = self.batch * self.matte.frame_bytes
                self.h_matte = [torch.empty(nb, dtype=torch.uint8).pin_memory() for _ in range(slots)]
                self.d_matte = [torch.empty(nb, dtype=torch.uint8, device=dev) for _ in range(slots)]
        self.s_h2d, self.s_run, self.s_d2h = (torch.cuda.Stream(dev) for _ in range(3))
        self.e_in = [torch.cuda.Event() for _ in range(slots)]
        self.e_run = [torch.cuda.Event() for _ in range(slots)]
        self.e_out = [torch.cuda.Event() for _ in range(slots)]

    def host_in(self, slot: int) -> np.ndarray:
        return self.h_in[slot].numpy()

    def host_out(self, slot: int) -> np.ndarray:
        return self.h_out[slot].numpy()

    def host_out2(self, slot: int) -> np.ndarray:
        return self.h_out2[slot].numpy()

    @staticmethod
    def _matte_tensor(a: np.ndarray) -> torch.Tensor:
        """A host matte as the tensor the engine takes: uint8, or the 16-bit words as int16."""
        return torch.from_numpy(np.ascontiguousarray(a) if a.dtype == np.uint8 else np.ascontiguousarray(a).view(np.int16))

    def _load_matte(self, slot: int, nframes: int):
        """The matte of the batch in `slot`: the still, or the next `nframes` frames of the matte stream read into the slot's pinned
        buffer and copied on the input's stream (the caller waits for `e_in`).  None without a matte."""
        if self.matte is None:
            return None
        if self.matte.still is not None:
            return self.d_matte
        nb = nframes * self.matte.frame_bytes
        self.h_matte[slot].numpy()[:nb] = self.matte.read(nframes).reshape(-1).view(np.uint8)
        with torch.cuda.stream(self.s_h2d):
            self.d_matte[slot][:nb].copy_(self.h_matte[slot][:nb], non_blocking=True)
        typed = self.d_matte[slot][:nb] if self.matte.depth == 8 else self.d_matte[slot][:nb].view(torch.int16)
        return typed.view(nframes, self.matte.height, self.matte.width)

    def _run_stack(self, src, dst, nframes: int, matte=None) -> None:
        """One batch through the stage stack; with key frames every frame takes the strength of its number in the
        stream, counted here across the batches.  `matte`: the batch's matte on the device, or None."""
        kw = self.kw
        if matte is not None:
            kw = dict(kw, matte=matte)
        if self.strength_keys is not None:
            kw = dict(kw, strength=self.strength_keys(self.frames_submitted, nframes))
        self.frames_submitted += nframes
        self.eng.apply_yuv_stack(src, dst, **kw)

    def _submit(self, slot: int, nframes: int) -> None:
        nb_in, nb_out = nframes * self.fin.frame_bytes, nframes * self.fout.frame_bytes
        matte = self._load_matte(slot, nframes)
        with torch.cuda.stream(self.s_h2d):
            self.d_in[slot][:nb_in].copy_(self.h_in[slot][:nb_in], non_blocking=True)
            self.e_in[slot].record()
        with torch.cuda.stream(self.s_run):
            self.s_run.wait_event(self.e_in[slot])
            # (the engine launches on the current stream: s_run)
            self._launch(self._views(self.fin, self.d_in[slot], nframes), self._views(self.fout, self.d_out[slot], nframes), slot,
                         nframes, matte)
            self.e_run[slot].record()
        with torch.cuda.stream(self.s_d2h):
            self.s_d2h.wait_event(self.e_run[slot])
            self.h_out[slot][:nb_out].copy_(self.d_out[slot][:nb_out], non_blocking=True)
            if self.fout2 is not None:
                nb2 = nframes * self.fout2.frame_bytes
                self.h_out2[slot][:nb2].copy_(self.d_out2[slot][:nb2], non_blocking=True)
            self.e_out[slot].record()

    def run(self, fill: Callable[[np.ndarray, int], int], drain: Callable[[np.ndarray, int], None],
            total_frames: Optional[int] = None, stop: Optional[Callable[[], bool]] = None,
            drain2: Optional[Callable[[np.ndarray, int], None]] = None) -> int:
        """`fill(host_in_bytes, max_frames) -> frames written` (0 = end of stream) produces input,
        `drain(host_out_bytes, nframes)` consumes output, both on the calling thread.  With a second output
        (`second_pix_fmt`), `drain2(host_out2_bytes, nframes)` consumes it, called right before `drain` for the same
        batch: when neither drain raises, both have seen the same frames at every return (a stop included).  If `drain`
        raises (a closed pipe, say), `drain2` has already taken that batch and is one batch ahead.
        Returns the number of frames processed."""
        if (drain2 is not None) != (self.fout2 is not None):
            raise ValueError("drain2 goes with second_pix_fmt: give both or neither")

        def retire(s, n):               # hand a finished batch over: the second output first, `drain` counts progress
            self.e_out[s].synchronize()
            if drain2 is not None:
                drain2(self.host_out2(s)[: n * self.fout2.frame_bytes], n)
            drain(self.host_out(s)[: n * self.fout.frame_bytes], n)
            return n

        pending: List[tuple] = []       # (slot, nframes) in submission order
        done = 0
        i = 0
        while True:
            slot = i % self.slots
            if len(pending) == self.slots:                       # ring full: retire the oldest first
                done += retire(*pending.pop(0))
            if stop is not None and stop():
                break
            want = self.batch if total_frames is None else min(self.batch, total_frames - done - sum(n for _, n in pending))
            if want <= 0:
                break
            n = fill(self.host_in(slot)[: want * self.fin.frame_bytes], want)
            if n <= 0:
                break
            self._submit(slot, n)
            pending.append((slot, n))
            i += 1
        for s, n in pending:
            done += retire(s, n)
        return done
