"""One process, several GPUs: row-block sharding of every frame behind the drop-in API.

The reference is ONE GUI process whose tasks run on a thread pool
(`/root/reference/src/lut_renderer/task_manager.py:229-235`, spawn at `:145-151`); it cannot start
one rank per GPU.  `LutEngineGroup` is what `apply_lut(..., devices=[0..7])` uses instead: one
`LutEngine` (C-ABI context) per device, the lattice uploaded once and copied GPU to GPU over xGMI
(`lutr_lut_broadcast`), and the rows of every frame split with FFmpeg's own slice rule
(`shard.row_blocks`).  Block g is launched on device g's stream; nothing on the
host waits between the launches, so the devices run concurrently.

Frames usually live on ONE device (the caller's).  Row blocks owned by another device travel there
and back as peer copies (torch plumbing, asynchronous, ordered by torch's streams) -- 3.1 MB per
peer and UHD 10-bit frame each way, a few tens of microseconds of xGMI per link.  Callers that
keep frames sharded already (one tensor list per device) pass them as such and nothing is copied.

The one-rank-per-GPU path (`LutEngine.set_lut_distributed`, `bench.py --gpus N`) stays the way to
scale a batch job; this class exists so that the untouched caller of the reference can use every GPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _native
from .cube import CubeLut, read_lut, read_lut1d
from .engine import LutEngine, _fresh_planes, _new_planes, _yuv_out_dtype, chain_args, dual_args
from .formats import (RgbSource, check_alpha_mode, check_cdl_options, check_container_options, check_lut1d_options, check_lut2,
                      check_matte, check_packed_stack_options, check_premul_options, check_rgb_stack_options, check_semi_stack_options,
                      check_stack_options, check_strength, check_yuv2rgb_options, check_yuv2rgb_stack_options, held_resources, packed_frame_width, parse_pix_fmt,
                      parse_rgb_source, refuse_chain_keywords, refuse_dual_keywords, v210_frame_width, yuv_side)
from .shard import row_blocks


def _stack_opening(group, check, refusable, pix_fmt, out_pix_fmt, stages, cdl, rgb_matrix, kw: dict, variant: bool = True, **told):
    """How the group's three stack wrappers open, under its lock: the row partition is the group's; then the family's `check`
    with what the first engine holds -- the 1D LUT as the group's setter left it -- and the keywords of `kw` the check refuses
    by name (`refusable`).  Returns (parsed stages, source format, destination format)."""
    if "row0" in kw or "rows" in kw:
        raise ValueError("the group owns the row partition")
    return check(pix_fmt, out_pix_fmt, stages=stages, cdl=cdl is not None, rgb_matrix=rgb_matrix is not None,
                 **held_resources(group.engines[0], variant, lut1d_of=group), **{k: kw[k] for k in refusable if k in kw}, **told)


def _row_ranges(fmt, r0: int, r1: int) -> list:
    """The rows of every plane of side `fmt` that hold the luma rows [r0, r1): luma, chroma, chroma -- counted in the side's own
    layout -- and alpha with the luma rows.  A side of fewer planes reads the front of the list."""
    c0, c1 = r0 >> fmt.csy, (r1 + (1 << fmt.csy) - 1) >> fmt.csy
    return [(r0, r1), (c0, c1), (c0, c1)] + [(r0, r1)] * getattr(fmt, "alpha", False)


def _travel(planes, rng, device) -> list:
    """The rows `rng` of `planes`, copied to `device` (the peer copy: asynchronous, ordered by torch's streams)."""
    return [p[..., a:b, :].to(device, non_blocking=True, copy=True).contiguous() for p, (a, b) in zip(planes, rng)]


def _crop(full, fmt, s0: int, r0: int, r1: int):
    """(the rows [r0, r1) of the output planes `full` of a slice that began at luma row s0, their row ranges in the frame)."""
    rng = _row_ranges(fmt, r0, r1)
    return [o[..., a - sa:b - sa, :] for o, (a, b), (sa, _) in zip(full, rng, _row_ranges(fmt, s0, r1))], rng


def _bn_anchor(r0: int, ocsy: int) -> int:
    """The last luma row at or above `r0` where the blue-noise pattern of every output plane starts over: a
    multiple of the mask's 64 rows in luma and, with chroma rows subsampled by 2^ocsy, in chroma.  A slice of the frame that
    begins there and is processed as a frame of its own gets the pattern of the full frame."""
    period = 64 << ocsy
    return r0 // period * period


class LutEngineGroup:
    """Contexts on `devices` (repeats allowed: two contexts on one GPU split its frames in two launches)."""

    def __init__(self, devices: Sequence[int], treat_as_remote: Optional[bool] = None):
        if not devices:
            raise ValueError("at least one device")
        self.devices = tuple(int(d) for d in devices)
        # Test hook for boxes with one GPU: every engine after the first behaves as if it sat on ANOTHER device -- its row
        # block is sliced, copied (a same-device `.to(copy=True)` stands in for the peer copy), applied as a short frame of its
        # own and copied back, and `lutr_lut_broadcast` takes its hipMemcpyPeerAsync branch (a self-peer copy is legal).
        # LUTR_GROUP_FORCE_REMOTE=1 sets it from the environment.  Never set in production.
        self.treat_as_remote = bool(int(os.environ.get("LUTR_GROUP_FORCE_REMOTE", "0"))) if treat_as_remote is None \
            else bool(treat_as_remote)
        self._lock = threading.RLock()
        self._applied_lut = None
        self._applied_lut2 = None
        self._applied_lut1d = None
        self.precision = "strict"
        self.engines: List[LutEngine] = []
        try:
            for d in self.devices:
                self.engines.append(LutEngine(d))
        except Exception:
            self.close()
            raise
        self._lib = _native.load()
        self.last_blocks: List[tuple] = []

    # -- lifetime ---------------------------------------------------------
    def close(self) -> None:
        for e in self.engines:
            e.close()
        self.engines = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return len(self.engines)

    # -- lattice ----------------------------------------------------------
    def set_lut(self, lut: CubeLut) -> None:
        """Upload on the first device, then ONE broadcast call: every other context receives the lattice GPU to GPU."""
        with self._lock:
            self._applied_lut = None
            root = self.engines[0]
            root.set_lut(lut)
            if len(self.engines) > 1:
                for e in self.engines:
                    e._bind_stream()
                arr = (C.c_void_p * len(self.engines))(*[e._ctx for e in self.engines])
                flags = _native.BCAST_FORCE_PEER_COPY if self.treat_as_remote else 0
                _native.check(self._lib.lutr_lut_broadcast_ex(arr, len(self.engines), 0, flags))
                for e in self.engines[1:]:
                    e._applied_lut = None
                    e.n, e.scale = root.n, np.array(root.scale, dtype=np.float32)
                    e.set_prelut(getattr(lut, "prelut", None))     # host-side state: it does not travel with the lattice copy

    def load_cube(self, path) -> CubeLut:
        lut = read_lut(path)
        self.set_lut(lut)
        return lut

    def set_lut2(self, lut: Optional[CubeLut]) -> None:
        """The second LUT of `apply_yuv_chain`, uploaded from the host to every engine (None removes it)."""
        check_lut2(lut)
        with self._lock:
            self._applied_lut2 = None
            for e in self.engines:
                e.set_lut2(lut)

    def load_cube2(self, path) -> CubeLut:
        lut = read_lut(path)
        self.set_lut2(lut)
        return lut

    def set_variant(self, name: str) -> None:
        for e in self.engines:
            e.set_variant(name)

    def set_precision(self, name: str) -> None:
        for e in self.engines:
            e.set_precision(name)
        self.precision = name

    @property
    def _has_prelut(self) -> bool:
        return bool(self.engines) and self.engines[0]._has_prelut

    @property
    def last_kernels(self) -> List[str]:
        return [e.last_kernel for e in self.engines]

    def sync(self) -> None:
        for e in self.engines:
            e.sync()

    # -- apply ------------------------------------------------------------
    def _shard(self, h: int, align: int, home, local, remote) -> None:
        """The one loop over the group's row blocks (`shard.row_blocks`, on multiples of `align` rows; empty blocks are skipped).
        A block whose engine sits on `home`, the device of the caller's planes, is launched on those planes: `local(eng, r0, r1)`.
        A block of another GPU travels there (peer copy), is processed as a short frame of its own and comes back:
        `remote(eng, r0, r1)` runs with that GPU current and returns (destination planes, output planes, row ranges) per output;
        the copies back are queued after every launch was issued."""
        blocks = row_blocks(h, len(self.engines), align=align)
        self.last_blocks = blocks
        self.last_remote = 0                                       # row blocks that took the copy-there-and-back path
        pending = []
        for k, (eng, (r0, r1)) in enumerate(zip(self.engines, blocks)):
            if r1 <= r0:
                continue
            if eng.device == home and not (self.treat_as_remote and k > 0):
                local(eng, r0, r1)
                continue
            with torch.cuda.device(eng.device):
                pending += remote(eng, r0, r1)
            self.last_remote += 1
        for to, out, rng in pending:
            for d, o, (a, b) in zip(to, out, rng):
                d[..., a:b, :].copy_(o, non_blocking=True)

    def apply_yuv(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                  out_pix_fmt: Optional[str] = None, **kw):
        with self._lock:
            return self._apply_yuv(src, dst, pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, **kw)

    def _apply_yuv(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                   out_pix_fmt: Optional[str] = None, **kw):
        """`LutEngine.apply_yuv` with the rows of every frame split over the group's devices.
        `src` planes live on one device (any); `dst`, if given, on the same one."""
        if kw.get("dither", "none") == "error_diffusion":
            raise ValueError("error-diffusion dither couples the rows of a frame: it cannot be row-sharded")
        if "row0" in kw or "rows" in kw:
            raise ValueError("the group owns the row partition")
        # premultiplied alpha is passed on: shards fall on the union block, alpha rows go with the luma rows
        if check_alpha_mode(kw.get("alpha_mode", "straight")):
            check_premul_options(pix_fmt, out_pix_fmt, dither=kw.get("dither", "none"), chroma_loc=kw.get("chroma_loc"),
                                 out_size=kw.get("out_size"), range_src=kw.get("range_src", "tv"), range_in=kw.get("range_in"),
                                 lut_depth=kw.get("lut_depth"))
        # a CDL in front of the LUT is passed on too: per-pixel work, shards on the union block, no halo
        if kw.get("cdl") is not None:
            check_cdl_options(pix_fmt, out_pix_fmt, dither=kw.get("dither", "none"), chroma_loc=kw.get("chroma_loc"),
                              out_size=kw.get("out_size"), alpha_mode=kw.get("alpha_mode", "straight"),
                              prelut=bool(getattr(self, "_has_prelut", False)))
        # a semi-planar side is two planes, the second with the chroma plane's rows: the shard rule is unchanged.
        # A packed 4:2:2 side (3.12) is one buffer with the frame's rows -- any row for a 4:2:2 destination, even rows for a
        # planar 4:2:0 one, which is the union block rule below
        kind = check_container_options(pix_fmt, out_pix_fmt, kw.get("dither", "none"), kw.get("chroma_loc"), kw.get("out_size"))
        if kind is None:
            fin, fout = parse_pix_fmt(pix_fmt), parse_pix_fmt(out_pix_fmt or pix_fmt)
        else:
            fin, fout = yuv_side(pix_fmt), yuv_side(out_pix_fmt or pix_fmt)
        # (v210, 3.14, shards like a packed side; its words are int32 and its width is named or told by the planar side)
        bare = kind in ("packed", "v210") and isinstance(dst, torch.Tensor)
        if kind in ("packed", "v210"):
            src = [src] if isinstance(src, torch.Tensor) else src
            dst = [dst] if bare else dst
        if kind == "v210":
            h, w = src[0].shape[-2], v210_frame_width(fin, fout, src, dst, kw.get("width"))
            kw = dict(kw, width=w)
        else:
            h, w = src[0].shape[-2], packed_frame_width(fin, src, kw.get("width"))
        home = src[0].device
        if dst is None:
            dst = _fresh_planes(fout, w, h, src[0], home)
        names = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt)
        bh = 1 << max(fin.csy, fout.csy)                           # the union block: whole chroma rows on both sides

        def local(eng, r0, r1):
            eng.apply_yuv(src, dst, row0=r0, rows=r1 - r0, **names, **kw)

        def remote(eng, r0, r1):
            # the slice that travels is the luma rows [s0, s1) with the chroma rows of the source's own layout; the apply writes the
            # block's rows inside it (row0 = r0 - s0: 0 for a slice that is just the block)
            s0, s1 = r0, r1
            if kw.get("chroma_loc") is not None:
                # sited resampling reads one chroma row (one chroma block row of luma) above and below the block: the slice
                # carries that halo, clipped to the frame
                c0, c1 = _row_ranges(fin, r0, r1)[1]
                s0, s1 = max(c0 - 1, 0) * bh, min((c1 + 1) * bh, h)
            elif kw.get("dither", "none") == "blue_noise":
                # the mask is anchored to the frame's top: the slice starts at a row where the pattern of every
                # output plane starts over
                s0 = _bn_anchor(r0, fout.csy)
            full = eng.apply_yuv(_travel(src, _row_ranges(fin, s0, s1), eng.device), None, row0=r0 - s0, rows=r1 - r0, **names, **kw)
            return [(dst, *_crop(full, fout, s0, r0, r1))]

        self._shard(h, bh, home, local, remote)
        return dst[0] if bare else dst

    def apply_yuv_dual(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None,
                       dst2: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, out_pix_fmt: Optional[str] = None,
                       out2_pix_fmt: str, **kw):
        """`LutEngine.apply_yuv_dual` with the rows of every frame split over the group's devices: shards on
        multiples of the union block height of the three layouts, each side's chroma rows counted in its own layout, no halo."""
        with self._lock:
            if "row0" in kw or "rows" in kw:
                raise ValueError("the group owns the row partition")
            refuse_dual_keywords(kw)
            fin, f1, f2, w, h = dual_args(src, dst, dst2, pix_fmt, out_pix_fmt, out2_pix_fmt)
            home = src[0].device
            if dst is None:
                dst = _fresh_planes(f1, w, h, src[0], home)
            if dst2 is None:
                dst2 = _fresh_planes(f2, w, h, src[0], home)
            names = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, out2_pix_fmt=out2_pix_fmt)

            def local(eng, r0, r1):
                eng.apply_yuv_dual(src, dst, dst2, row0=r0, rows=r1 - r0, **names, **kw)

            def remote(eng, r0, r1):
                out, out2 = eng.apply_yuv_dual(_travel(src, _row_ranges(fin, r0, r1), eng.device), None, None, **names, **kw)
                return [(dst, out, _row_ranges(f1, r0, r1)), (dst2, out2, _row_ranges(f2, r0, r1))]

            self._shard(h, 1 << max(fin.csy, f1.csy, f2.csy), home, local, remote)
            return dst, dst2

    def apply_yuv_chain(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                        out_pix_fmt: Optional[str] = None, interp: str = "tetrahedral", interp2: Optional[str] = None, **kw):
        """`LutEngine.apply_yuv_chain` with the rows of every frame split over the group's devices: shards on
        multiples of the union block height of the two layouts, each side's chroma rows counted in its own layout, no halo."""
        with self._lock:
            if "row0" in kw or "rows" in kw:
                raise ValueError("the group owns the row partition")
            refuse_chain_keywords(kw)
            fin, fout, w, h, _, _ = chain_args(src, dst, pix_fmt, out_pix_fmt, interp, interp2)
            home = src[0].device
            if dst is None:
                dst = _fresh_planes(fout, w, h, src[0], home)
            names = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, interp=interp, interp2=interp2)

            def local(eng, r0, r1):
                eng.apply_yuv_chain(src, dst, row0=r0, rows=r1 - r0, **names, **kw)

            def remote(eng, r0, r1):
                out = eng.apply_yuv_chain(_travel(src, _row_ranges(fin, r0, r1), eng.device), None, **names, **kw)
                return [(dst, out, _row_ranges(fout, r0, r1))]

            self._shard(h, 1 << max(fin.csy, fout.csy), home, local, remote)
            return dst

    def set_lut1d(self, lut1d, interp: str = "linear") -> None:
        """The 1D LUT of `apply_yuv_lut1d` / `apply_rgb_lut1d`, set from the host on every engine (None removes
        it)."""
        with self._lock:
            self._applied_lut1d = None
            for e in self.engines:
                e.set_lut1d(lut1d, interp)

    def load_lut1d(self, path, interp: str = "linear"):
        lut1d = read_lut1d(path)
        self.set_lut1d(lut1d, interp)
        return lut1d

    @property
    def n1d(self) -> int:
        return self.engines[0].n1d if self.engines else 0

    def apply_yuv_lut1d(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                        out_pix_fmt: Optional[str] = None, **kw):
        """`LutEngine.apply_yuv_lut1d` with the rows of every frame split over the group's devices: shards on
        multiples of the union block height of the two layouts, as for a CDL; alpha rows go with the luma rows, no halo."""
        with self._lock:
            if "row0" in kw or "rows" in kw:
                raise ValueError("the group owns the row partition")
            lut2 = kw.get("cube2") is not None or bool(kw.get("lut2"))
            fin, fout = check_lut1d_options(pix_fmt, out_pix_fmt, dither=kw.get("dither", "none"), chroma_loc=kw.get("chroma_loc"),
                                            out_size=kw.get("out_size"), alpha_mode=kw.get("alpha_mode", "straight"),
                                            out2_pix_fmt=kw.get("out2_pix_fmt"), lut2=lut2, cdl=kw.get("cdl") is not None,
                                            loaded=bool(self.n1d))
            h, w = src[0].shape[-2], src[0].shape[-1]
            home = src[0].device
            if dst is None:
                dst = _fresh_planes(fout, w, h, src[0], home)
            names = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt)

            def local(eng, r0, r1):
                eng.apply_yuv_lut1d(src, dst, row0=r0, rows=r1 - r0, **names, **kw)

            def remote(eng, r0, r1):
                out = eng.apply_yuv_lut1d(_travel(src, _row_ranges(fin, r0, r1), eng.device), None, **names, **kw)
                return [(dst, out, _row_ranges(fout, r0, r1))]

            self._shard(h, 1 << max(fin.csy, fout.csy), home, local, remote)
            return dst

    def apply_yuv_stack(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                        out_pix_fmt: Optional[str] = None, stages, cdl=None, **kw):
        """`LutEngine.apply_yuv_stack` with the rows of every frame split over the group's devices: the lattices
        and the 1D LUT are on every engine through the group's setters, the CDL travels with the call; shards on multiples of the
        union block height of the two layouts, alpha rows go with the luma rows, no halo.  `strength` as the
        engine takes it: a per-frame array goes to every device once, and the shards give the bits of the whole call.  `matte`
         as the engine takes it, on the source's device: its rows travel with the source's luma rows, a still's
        once per device, and a pixel reads the sample of its own row and column on every shard.  `rgb_matrix`
        travels with the call like the CDL."""
        with self._lock:
            st, fin, fout = _stack_opening(
                self, check_stack_options, ("dither", "chroma_loc", "out_size", "alpha_mode", "out2_pix_fmt", "strength"),
                pix_fmt, out_pix_fmt, stages, cdl, kw.get("rgb_matrix"), kw, variant=False, matte=kw.get("matte") is not None)
            if kw.get("matte") is not None:
                check_matte(kw["matte"], kw.get("matte_depth"), kw.get("matte_invert", False), w=src[0].shape[-1], h=src[0].shape[-2],
                            nframes=src[0].shape[0] if len(src[0].shape) == 3 else 1, device=src[0].device)
            if kw.get("strength") is not None:
                # checked once for the whole call; every engine uploads its own copy of a per-frame array, and a shard's frame
                # 0 is the call's frame 0 (rows are split, frames are not)
                kw = dict(kw, strength=check_strength(kw["strength"], src[0].shape[0] if len(src[0].shape) == 3 else 1))
            h, w = src[0].shape[-2], src[0].shape[-1]
            home = src[0].device
            if dst is None:
                dst = _fresh_planes(fout, w, h, src[0], home)
            names = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, stages=st, cdl=cdl)

            def local(eng, r0, r1):
                eng.apply_yuv_stack(src, dst, row0=r0, rows=r1 - r0, **names, **kw)

            def remote(eng, r0, r1):
                there = kw if kw.get("matte") is None else dict(kw, matte=_travel([kw["matte"]], [(r0, r1)], eng.device)[0])
                out = eng.apply_yuv_stack(_travel(src, _row_ranges(fin, r0, r1), eng.device), None, **names, **there)
                return [(dst, out, _row_ranges(fout, r0, r1))]

            self._shard(h, 1 << max(fin.csy, fout.csy), home, local, remote)
            return dst

    def apply_yuv_stack_semi(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str,
                             out_pix_fmt: Optional[str] = None, stages, cdl=None, **kw):
        """`LutEngine.apply_yuv_stack_semi` with the rows of every frame split over the group's devices, by
        `apply_yuv_stack`'s rule: shards on multiples of the union block height of the two layouts, no halo.  A plane of pairs
        has the rows of a planar chroma plane, so it travels as one; the shards give the bits of the whole call."""
        with self._lock:
            st, fin, fout = _stack_opening(
                self, check_semi_stack_options,
                ("dither", "chroma_loc", "out_size", "alpha_mode", "out2_pix_fmt", "strength", "matte"),
                pix_fmt, out_pix_fmt, stages, cdl, kw.get("rgb_matrix"), kw)
            h, w = src[0].shape[-2], src[0].shape[-1]
            home = src[0].device
            if dst is None:
                dst = _fresh_planes(fout, w, h, src[0], home)
            names = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, stages=st, cdl=cdl)

            def local(eng, r0, r1):
                eng.apply_yuv_stack_semi(src, dst, row0=r0, rows=r1 - r0, **names, **kw)

            def remote(eng, r0, r1):
                out = eng.apply_yuv_stack_semi(_travel(src, _row_ranges(fin, r0, r1), eng.device), None, **names, **kw)
                return [(dst, out, _row_ranges(fout, r0, r1))]

            self._shard(h, 1 << max(fin.csy, fout.csy), home, local, remote)
            return dst

    def apply_yuv_stack_packed(self, src, dst=None, *, pix_fmt: str, out_pix_fmt: Optional[str] = None, stages, cdl=None, **kw):
        """`LutEngine.apply_yuv_stack_packed` with the rows of every frame split over the group's devices, by
        `apply_yuv_stack`'s rule: shards on multiples of the union block height of the two layouts (1 row, 2 with a 4:2:0
        destination), no halo.  A packed 4:2:2 or v210 side is one buffer with the frame's rows; the shards give the bits of the
        whole call."""
        with self._lock:
            st, fin, fout = _stack_opening(
                self, check_packed_stack_options,
                ("dither", "chroma_loc", "out_size", "alpha_mode", "out2_pix_fmt", "strength", "matte"),
                pix_fmt, out_pix_fmt, stages, cdl, kw.get("rgb_matrix"), kw)
            bare = fout.nplanes == 1 and isinstance(dst, torch.Tensor)
            src = [src] if isinstance(src, torch.Tensor) else src
            dst = [dst] if bare else dst
            if "v210" in (fin.name, fout.name):
                h, w = src[0].shape[-2], v210_frame_width(fin, fout, src, dst, kw.get("width"))
            else:
                h, w = src[0].shape[-2], packed_frame_width(fin, src, kw.get("width"))
            kw = dict(kw, width=w)
            home = src[0].device
            if dst is None:
                dst = _fresh_planes(fout, w, h, src[0], home)
            names = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, stages=st, cdl=cdl)

            def local(eng, r0, r1):
                eng.apply_yuv_stack_packed(src, dst, row0=r0, rows=r1 - r0, **names, **kw)

            def remote(eng, r0, r1):
                out = eng.apply_yuv_stack_packed(_travel(src, _row_ranges(fin, r0, r1), eng.device), None, **names, **kw)
                return [(dst, out, _row_ranges(fout, r0, r1))]

            self._shard(h, 1 << max(fin.csy, fout.csy), home, local, remote)
            return dst[0] if bare else dst

    def apply_rgb_lut1d(self, src: Sequence[torch.Tensor], dst: Optional[Sequence[torch.Tensor]] = None, *, depth: int,
                        interp: Optional[str] = None, **kw):
        """`LutEngine.apply_rgb_lut1d` with the rows of every frame split over the group's devices (any row)."""
        with self._lock:
            if "row0" in kw or "rows" in kw:
                raise ValueError("the group owns the row partition")
            if kw:
                raise TypeError(f"apply_rgb_lut1d() got an unexpected keyword argument '{next(iter(kw))}'")
            if not self.n1d:
                raise ValueError("no 1D LUT is loaded: call set_lut1d / load_lut1d first, or pass lut1d")
            h = src[0].shape[-2]
            home = src[0].device
            if dst is None:
                dst = [torch.empty_like(t) for t in src]

            def local(eng, r0, r1):
                eng.apply_rgb_lut1d(src, dst, depth=depth, interp=interp, row0=r0, rows=r1 - r0)

            def remote(eng, r0, r1):
                rng = [(r0, r1)] * 3
                out = eng.apply_rgb_lut1d(_travel(src, rng, eng.device), None, depth=depth, interp=interp)
                return [(dst, out, rng)]

            self._shard(h, 1, home, local, remote)
            return dst

    def apply_rgb_to_yuv(self, src, dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, out_pix_fmt: str, **kw):
        """`LutEngine.apply_rgb_to_yuv` with the rows of every frame split over the group's devices: shards on
        multiples of the output chroma block height, every source plane (or the packed image) counted in luma rows, no halo.
        Float sources (gbrpf32le / gbrapf32le) shard the same way."""
        with self._lock:
            if kw.get("dither", "none") == "error_diffusion":
                raise ValueError("error-diffusion dither couples the rows of a frame: it cannot be row-sharded")
            if "row0" in kw or "rows" in kw:
                raise ValueError("the group owns the row partition")
            if kw.get("out_size") is not None:
                raise ValueError("a resize (out_size) needs a single device")
            fin = parse_rgb_source(pix_fmt)
            if fin is None:
                raise ValueError(f"apply_rgb_to_yuv takes gbrp*, gbrpf32le or packed RGB sources, not '{pix_fmt}'")
            fout = parse_pix_fmt(out_pix_fmt.replace("yuvj", "yuv"))
            csy = fout.csy
            if kw.get("intermediate_pix_fmt"):                     # the full-range composition: its 8-bit frame has chroma rows too
                csy = max(csy, parse_pix_fmt(kw["intermediate_pix_fmt"]).csy)
            first = src if fin.packed else src[0]
            h, w = (first.shape[-3], first.shape[-2]) if fin.packed else (first.shape[-2], first.shape[-1])
            lead = tuple(first.shape[:-3]) if fin.packed else tuple(first.shape[:-2])
            home = first.device
            if dst is None:
                dst = _new_planes(fout, w, h, lead, _yuv_out_dtype(fout.depth, None), home)
            names = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt)

            def local(eng, r0, r1):
                eng.apply_rgb_to_yuv(src, dst, row0=r0, rows=r1 - r0, **names, **kw)

            def remote(eng, r0, r1):
                # (blue-noise dither: the slice starts where the pattern of every output plane starts over, as in _apply_yuv)
                s0 = _bn_anchor(r0, fout.csy) if kw.get("dither", "none") == "blue_noise" else r0
                if fin.packed:
                    part = src[..., s0:r1, :, :].to(eng.device, non_blocking=True, copy=True).contiguous()
                else:
                    part = _travel(src, [(s0, r1)] * len(src), eng.device)
                full = eng.apply_rgb_to_yuv(part, None, row0=r0 - s0, rows=r1 - r0, **names, **kw)
                return [(dst, *_crop(full, fout, s0, r0, r1))]

            self._shard(h, 1 << csy, home, local, remote)
            return dst

    def apply_rgb_stack(self, src, dst: Optional[Sequence[torch.Tensor]] = None, *, pix_fmt: str, out_pix_fmt: Optional[str] = None,
                        stages, cdl=None, rgb_matrix=None, **kw):
        """`LutEngine.apply_rgb_stack` with the rows of every frame split over the group's devices: the lattices
        and the 1D LUT are on every engine through the group's setters, the CDL and the matrix travel with the call; shards on
        multiples of the output chroma block height (any row for a gbrp destination), every source plane (or the packed image)
        and alpha counted in luma rows, no halo."""
        with self._lock:
            st, fin, fout = _stack_opening(
                self, check_rgb_stack_options,
                ("dither", "chroma_loc", "out_size", "alpha_mode", "out2_pix_fmt", "strength", "matte", "intermediate_pix_fmt"),
                pix_fmt, out_pix_fmt, stages, cdl, rgb_matrix, kw)
            first = src if fin.packed else src[0]
            h, w = (first.shape[-3], first.shape[-2]) if fin.packed else (first.shape[-2], first.shape[-1])
            lead = tuple(first.shape[:-3]) if fin.packed else tuple(first.shape[:-2])
            home = first.device
            if dst is None:
                dtype = first.dtype if fout.family == "gbr" and not fin.packed else _yuv_out_dtype(fout.depth, None)
                dst = _new_planes(fout, w, h, lead, dtype, home)
            names = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, stages=st, cdl=cdl, rgb_matrix=rgb_matrix)

            def local(eng, r0, r1):
                eng.apply_rgb_stack(src, dst, row0=r0, rows=r1 - r0, **names, **kw)

            def remote(eng, r0, r1):
                if fin.packed:
                    part = src[..., r0:r1, :, :].to(eng.device, non_blocking=True, copy=True).contiguous()
                else:
                    part = _travel(src, [(r0, r1)] * len(src), eng.device)
                out = eng.apply_rgb_stack(part, None, **names, **kw)
                return [(dst, out, _row_ranges(fout, r0, r1))]

            self._shard(h, 1 << fout.csy, home, local, remote)
            return dst

    def apply_yuv_to_rgb(self, src: Sequence[torch.Tensor], dst=None, *, pix_fmt: str, out_pix_fmt: str, **kw):
        """`LutEngine.apply_yuv_to_rgb` with the rows of every frame split over the group's devices: shards on
        multiples of the source's chroma block height, the source's chroma rows counted in its own layout, every destination
        plane (or the packed image) in luma rows, alpha rows with the luma rows; no halo."""
        with self._lock:
            if "row0" in kw or "rows" in kw:
                raise ValueError("the group owns the row partition")
            fin, fout = check_yuv2rgb_options(pix_fmt, out_pix_fmt, **{k: v for k, v in kw.items() if k not in (
                "interp", "matrix_in", "range_src", "range_in", "lut")})
            return self._yuv2rgb_shards("apply_yuv_to_rgb", src, dst, fin, fout, dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt), kw)

    def _yuv2rgb_shards(self, method: str, src, dst, fin, fout, names: dict, kw: dict):
        """The row shards of `apply_yuv_to_rgb` / `apply_yuv_stack_to_rgb` (`method`) behind their option checks."""
        if isinstance(src, torch.Tensor) or len(src) != fin.nplanes:
            raise ValueError(f"'{fin.name}' takes {fin.nplanes} planes")
        h, w = src[0].shape[-2], src[0].shape[-1]
        home = src[0].device
        lead = tuple(src[0].shape[:-2])
        packed = isinstance(fout, RgbSource)
        odt = torch.uint8 if fout.depth <= 8 else torch.int16
        if dst is None:
            dst = torch.empty(lead + (h, w, fout.ncomp), dtype=odt, device=home) if packed else \
                _new_planes(fout, w, h, lead, odt, home)

        def local(eng, r0, r1):
            getattr(eng, method)(src, dst, row0=r0, rows=r1 - r0, **names, **kw)

        def remote(eng, r0, r1):
            out = getattr(eng, method)(_travel(src, _row_ranges(fin, r0, r1), eng.device), None, **names, **kw)
            if packed:                                         # (rows of w * C components: a plane to the copy back)
                return [([dst.flatten(-2)], [out.flatten(-2)], [(r0, r1)])]
            return [(dst, out, _row_ranges(fout, r0, r1))]

        self._shard(h, 1 << fin.csy, home, local, remote)
        return dst

    def apply_yuv_stack_to_rgb(self, src: Sequence[torch.Tensor], dst=None, *, pix_fmt: str, out_pix_fmt: str, stages, cdl=None,
                               rgb_matrix=None, **kw):
        """`LutEngine.apply_yuv_stack_to_rgb` with the rows of every frame split over the group's devices, as
        `apply_yuv_to_rgb` splits them (shards on multiples of the source's chroma block height 2^icsy, no halo): the lattices
        and the 1D LUT are on every engine through the group's setters, the CDL and the matrix travel with the call."""
        with self._lock:
            st, fin, fout = _stack_opening(
                self, check_yuv2rgb_stack_options,
                ("dither", "engine_dither", "chroma_loc", "out_size", "alpha_mode", "out2_pix_fmt", "strength", "matte"),
                pix_fmt, out_pix_fmt, stages, cdl, rgb_matrix, kw)
            names = dict(pix_fmt=pix_fmt, out_pix_fmt=out_pix_fmt, stages=st, cdl=cdl, rgb_matrix=rgb_matrix)
            return self._yuv2rgb_shards("apply_yuv_stack_to_rgb", src, dst, fin, fout, names, kw)
