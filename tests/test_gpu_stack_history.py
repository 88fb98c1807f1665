"""The stage-stack passes against call history on ONE engine.  tests/test_engine_state.py pins the state that existed when it was
written (lattice copies, prelut tables and tube bound, resize tables, queue words); every GPU module of the newer families starts
from a freshly loaded engine and changes at most one resource.  This module changes the resources under a kept engine and checks
every apply, whole tensors, bit for bit, into sentinel-filled destinations, against the family's own reference computed from
scratch AFTER the step's state change (the `_want` helpers of test_gpu_cdl / lut1d / chain / stack / mix / matte / rgbmatrix /
rgbstack / y2rstack, fed `_native.cdl_table` / `_native.lut1d_table` of the resources current at that step), never against
another GPU run.  After each apply `last_kernel` is asserted too: family, stage list and, for the vector kernels, the LDS / global
placement flag computed from the table sizes.  A mismatch prints the step log.

What each section pins, and where that state lives:
  A  the CDL table: lutr_ctx.cdl_tab / cdl_cap / cdl_depth / cdl_key[9], `cdl_device_table` (lutr_api.cpp) -- one buffer for every
     depth, rebuilt on a depth or key change, reallocated for a deeper depth, refilled behind the previous kernel; saturation is
     an argument, not in the key.
  B  the 1D tables: lutr_ctx.l1d_tab[depth - 8] with their `gen`, l1d_gen, `l1d_device_table` and `lutr_ctx_set_lut1d`
     (lutr_api.cpp); `LutEngine.set_lut1d` / n1d (engine.py).
  C  the second lattice (lat2 / n2 / scale2, `lutr_ctx_set_lut2`) beside the first; the first lattice's per-depth prelut tables
     built by `fill_lut` at the depth the stack runs at; `LutEngine._has_prelut` and `formats.check_stage_list`'s "directly
     behind" refusal; the `unit` flag and the fast / fma32 lattice copies (lutr_api.cpp, engine.py); per call, `stack_in_lds`
     (lutr_launch.h).
  D  `LutEngine._frame_strength` and `_upload_frame_strength` (engine.py): the device array of the last per-frame strengths.
  E  all of it, on a seeded walk (its draw is replayed without a GPU in tests/test_stack_upload_markers.py).
  F  `_applied_lut` / `_applied_lut2` / `_applied_lut1d` on `LutEngine` and `LutEngineGroup` (engine.py, multigpu.py), read by
     `api._stack_upload`; the group's setters reaching both contexts.

The `_want` helpers memoise by `id()` of the resource objects; a freed object's id is handed out again, and the helper would then
return the reference of an earlier resource.  Every resource made here is therefore kept alive in `_KEEP` for the life of the
module, and every step passes a key of its own (tests/test_stack_upload_markers.py holds the CPU guard).

Proof that the cases can fail, done once by hand on a scratch copy of the library (nothing of it committed; both mutations leave
a stale table of the same size, so every read stays inside the allocation):
  - `cdl_device_table` without the memcmp of the key: of the 14 cases here, test_cdl_one_key_number_at_a_time,
    test_cdl_two_clips_back_to_back, test_seeded_stack_walk and the three test_apply_lut_on_kept_engines fail;
    test_cdl_depth_sequence and test_cdl_same_grade_another_depth_through_another_entry pass, as they must (one CDL, and the
    depth compare is intact), and so does every case without a CDL change.
  - `l1d_device_table` with `t.gen != c->l1d_gen` replaced by `!t.gen`: test_lut1d_tables_follow_the_generation,
    test_seeded_stack_walk and the three test_apply_lut_on_kept_engines fail, the other nine pass.
The families' own modules do NOT stay green under these mutations: 10 of the 40 tests of tests/test_gpu_cdl.py and 15 of the 40
of tests/test_gpu_lut1d.py fail, because their tests share the session's engine from one CDL / 1D LUT to the next (and
test_gpu_cdl.py has an a-b-a case).  So a stale table behind `apply_yuv(cdl=)` and `apply_yuv_lut1d` was already noticed, by that
sharing; what only this module catches is the same table reached through the three stack entries and `apply_lut`, whose modules
load one CDL and one 1D LUT and never change them, and every other history above.

Measured wall time of the module on the MI355X: 14 cases in 5.0 s (one pytest process; no case above 0.3 s)."""
import itertools
import os
import random
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native, cube
from lut_renderer_amd.cdl import Cdl, read_cdl
from lut_renderer_amd.rgbmatrix import RgbMatrix, read_rgb_matrix
from tests import _lut1d_twin, test_engine_state as ES, test_gpu_cdl as CD, test_gpu_chain as CH, test_gpu_lut1d as L1
from tests import test_gpu_matte as MT, test_gpu_mix as MIX, test_gpu_rgbmatrix as MX, test_gpu_rgbstack as RS
from tests import test_gpu_rgb2yuv as R2Y, test_gpu_stack as ST, test_gpu_y2rstack as Y2, test_gpu_yuv2rgb as Y2R
from tests._csp_files import write_csp_with_prelut
from tests._stride_cases import SENTINEL

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
F = np.float32
W, H = 136, 36               # the vector kernels: 612 threads a frame at 4:2:0
SW, SH = 67, 21              # the generic kernels
XS = np.linspace(0.0, 1.0, 9)
_KEEP = []                   # every resource object of the module: alive for its life, so that no id() is handed out twice
_STEP = itertools.count()    # a key of its own for every reference
_RGB = {}                    # planar RGB sources of apply_rgb_lut1d, by depth
I3 = RgbMatrix()
GAMUT = read_rgb_matrix(GOLDEN / "matrix" / "bt2020_to_709.spimtx")
OFFSET = RgbMatrix((0.9, 0.1, 0.0, 0.0, 1.05, -0.05, 0.02, 0.0, 0.95), (0.03, -0.02, 0.0))
SHOT = read_cdl(GOLDEN / "cdl" / "shot.cc")


def _keep(x):
    _KEEP.append(x)
    return x


def _cdl(c=SHOT, **kw):
    return Cdl(slope=kw.get("slope", c.slope), offset=kw.get("offset", c.offset), power=kw.get("power", c.power),
               saturation=kw.get("saturation", c.saturation))


def _one(t, i, v):
    t = list(t)
    t[i] = v
    return tuple(t)


def _sentinels(want, device):
    """Destinations of the reference's shapes and dtypes, pre-filled with the sentinel of tests/_stride_cases.py."""
    import torch

    def one(a):
        v = SENTINEL[a.dtype]
        return torch.full(a.shape, v - 0x10000 if a.dtype == np.uint16 else v, dtype=torch.int16 if a.dtype == np.uint16 else torch.uint8,
                          device=device)
    return one(want) if isinstance(want, np.ndarray) else [one(a) for a in want]


def _host(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _as_list(x):
    return [x] if isinstance(x, np.ndarray) or not isinstance(x, (list, tuple)) else list(x)


def _frames_of(src):
    return [src] if src[0].ndim == 2 else [[p[i] for p in src] for i in range(src[0].shape[0])]


def _restack(per, batch):
    return [np.stack([f[i] for f in per]) for i in range(len(per[0]))] if batch else list(per[0])


class _Pending:
    """One apply: the reference (computed before the launch, from the resources current then), the sentinel destinations, the
    launch and the kernel name it must report."""

    def __init__(self, hist, what, want, call, expect):
        self.h, self.what, self.want, self.call, self.expect = hist, what, want, call, expect
        self.dst = _sentinels(want, hist.eng.device)
        self.kernel = None

    def launch(self):
        self.call(self.dst)
        self.kernel = self.h.kernel()
        self.h.log.append(f"{self.what} -> {self.kernel}")
        return self

    def finish(self):
        ok = self.expect(self.kernel) if callable(self.expect) else self.kernel == self.expect
        assert ok, f"{self.what}: ran {self.kernel}, expected {self.expect}\n  " + "\n  ".join(self.h.log)
        ES._eq([_host(t) for t in _as_list(self.dst)], _as_list(self.want), self.what, self.h.log)


class Hist:
    """One engine, the resources it holds now, and the log of everything done to it."""

    def __init__(self, eng, orc):
        self.eng, self.orc, self.log = eng, orc, []
        self.res = dict(lut=None, lut2=None, l1=(None, None), prelut=None)
        self.variant, self.refusal = "auto", None

    def kernel(self):
        return self.eng.last_kernel

    # -- state changes
    def set_lut(self, path):
        lut = _keep(self.eng.load_cube(path))
        self.res = dict(self.res, lut=lut, prelut=_keep(self.orc.parse_lut_file_ex(path)[3]) if lut.prelut is not None else None)
        self.log.append(f"set_lut {Path(path).name} (n={lut.n}, prelut={lut.prelut is not None})")
        return lut

    def set_lut2(self, path):
        lut = None if path is None else _keep(cube.read_lut(path))
        self.eng.set_lut2(lut)
        self.res = dict(self.res, lut2=lut)
        self.log.append(f"set_lut2 {None if path is None else Path(path).name}")

    def set_lut1d(self, l1, mode="linear", name=""):
        self.eng.set_lut1d(l1, mode)
        self.res = dict(self.res, l1=(l1, mode) if l1 is not None else (None, None))
        self.log.append(f"set_lut1d {name or l1 is not None} {mode}")

    def set_variant(self, v):
        self.eng.set_variant(v)
        self.variant = v
        self.log.append(f"set_variant {v}")

    def set_precision(self, p):
        self.eng.set_precision(p)
        self.log.append(f"set_precision {p}")

    def refused(self, what, exc, match, fn):
        with pytest.raises(exc, match=match):
            fn()
        self.log.append(f"{what}: refused ({match})")

    def _no_vec(self, din, dout):
        return self.variant == "generic" or (din == 8 and dout > 8)

    def _go(self, what, want, call, expect, defer=False):
        """`want()` computes the reference -- after every state change so far, before the launch.  With `self.refusal` set (an
        exception type and a pattern) the call must be refused instead, before any GPU work."""
        if self.refusal is not None:
            return self.refused(what, *self.refusal, lambda: call(None))
        p = _Pending(self, what, want(), call, expect)
        return p if defer else p.launch().finish()

    # -- the entries
    def cdl(self, c, din, a, dout=None, b=None, size=(W, H, 2), defer=False):
        dout, b, (w, h, nf) = dout or din, b or a, size
        src = CD._src("natural", w, h, din, a, k=3, nf=nf)
        name = f"step{next(_STEP)}"
        want = lambda: CD._want({name: (None, self.res["lut"])}, name, c, "tetrahedral", din, din, dout, a, b, src, name)
        dev = CD._dev(src, self.eng.device)
        names = dict(pix_fmt=CD._fmt(din, a), out_pix_fmt=CD._fmt(dout, b))
        expect = CD.GENERIC if self._no_vec(din, dout) else CD._vec_name(din, dout, a, b, "tetrahedral")
        return self._go(f"apply_yuv(cdl={c.sop_text()} sat {c.saturation}) {names}", want,
                                 lambda d: self.eng.apply_yuv(dev, d, cdl=c, **names), expect, defer)

    def l1d(self, din, a, dout=None, b=None, mode="tetrahedral", size=(W, H, 2)):
        dout, b, (w, h, nf) = dout or din, b or a, size
        src = L1._src("natural", w, h, din, a, k=4, nf=nf)
        l1, m1 = self.res["l1"]
        want = lambda: L1._want(l1, m1, self.res["lut"], mode, din, din, dout, a, b, src, f"step{next(_STEP)}", prelut=self.res["prelut"])
        dev = L1._dev(src, self.eng.device)
        names = dict(pix_fmt=L1._fmt(din, a), out_pix_fmt=L1._fmt(dout, b), interp=mode)
        expect = L1.GENERIC if self._no_vec(din, dout) else L1._vec_name(din, dout, a, b, mode)
        return self._go(f"apply_yuv_lut1d {names}", want, lambda d: self.eng.apply_yuv_lut1d(dev, d, **names), expect, False)

    def rgb_l1d(self, depth):
        from lut_renderer_amd import frames
        if depth not in _RGB:
            fs = [frames.make_rgb("natural", W, H, depth, k=1 + i) for i in range(2)]
            _RGB[depth] = [np.stack([f[i] for f in fs]) for i in range(3)]
        src = _RGB[depth]
        want = lambda: _lut1d_twin.apply_rgb(_native.lut1d_table(*self.res["l1"], depth), depth, src)
        dev = L1._dev(src, self.eng.device)
        return self._go(f"apply_rgb_lut1d depth {depth}", want, lambda d: self.eng.apply_rgb_lut1d(dev, d, depth=depth),
                                 f"k_rgb_l1d<{int(depth > 8)}>", False)

    def chain(self, din, a, dout=None, b=None, size=(W, H, 2)):
        dout, b, (w, h, nf) = dout or din, b or a, size
        src = ST._src("natural", w, h, din, a, k=5, nf=nf)
        name = f"step{next(_STEP)}"
        pairs = {name: (None, None, self.res["lut"], self.res["lut2"], self.res["prelut"])}
        want = lambda: _restack([CH._want(pairs, name, "tetrahedral", "tetrahedral", din, din, dout, a, b, f, (name, i))   # noqa: E731
                                 for i, f in enumerate(_frames_of(src))], src[0].ndim == 3)
        dev = ST._dev(src, self.eng.device)
        names = dict(pix_fmt=ST._fmt(din, a), out_pix_fmt=ST._fmt(dout, b))
        expect = CH.GENERIC if self._no_vec(din, dout) else CH._vec_name(din, dout, a, b, "tetrahedral")
        return self._go(f"apply_yuv_chain {names}", want,
                                 lambda d: self.eng.apply_yuv_chain(dev, d, **names), expect, False)

    def stack(self, stages, din, a, dout=None, b=None, c=None, mtx=None, strength=None, matte=None, size=(W, H, 2), defer=False,
              stream=None):
        """matte: None or (depth, invert)."""
        dout, b, (w, h, nf) = dout or din, b or a, size
        src = ST._src("natural", w, h, din, a, k=6, nf=nf)
        key, lds = f"step{next(_STEP)}", ST._lds(stages, din)
        no_vec, tail = self._no_vec(din, dout), ST._list(stages)
        kw = dict(pix_fmt=ST._fmt(din, a), out_pix_fmt=ST._fmt(dout, b), stages=stages, cdl=c)
        if matte is not None:
            dm, inv = matte
            m = MT._matte(w, h, dm, nf=nf if nf > 1 else None)
            s = 1.0 if strength is None else strength
            want = lambda: MT._want(self.res, stages, c, s, m, dm, inv, din, din, dout, a, b, src, key)
            kw.update(strength=strength, matte=MT._mdev(m, self.eng.device), matte_depth=dm, matte_invert=inv)
            expect = MT.MATTE_GENERIC + tail if no_vec or (din == 8 and dm > 8) else MT._matte_name(din, dout, dm, a, b, stages, lds)
        elif strength is not None:
            want = lambda: MIX._want(self.res, stages, c, strength, din, din, dout, a, b, src, key)
            kw.update(strength=strength)
            expect = MIX.MIX_GENERIC + tail if no_vec else MIX._mix_name(din, dout, a, b, stages, lds)
        elif mtx is not None:
            want = lambda: MX._want(self.res, stages, c, mtx, din, din, dout, a, b, src, key)
            kw.update(rgb_matrix=mtx)
            expect = MX.GENERIC + tail if no_vec else MX._vec_name(din, dout, a, b, stages, lds)
        else:
            want = lambda: ST._want(self.res, stages, c, din, din, dout, a, b, src, key)
            expect = ST.GENERIC + tail if no_vec else ST._vec_name(din, dout, a, b, stages, lds)
        dev = ST._dev(src, self.eng.device)
        what = f"apply_yuv_stack {kw['pix_fmt']}->{kw['out_pix_fmt']} {stages} cdl={c and (c.sop_text(), c.saturation)} " \
               f"matrix={mtx and mtx.m} strength={strength} matte={matte} {nf} frames" + (" on a side stream" if stream else "")

        def call(d):
            if stream is None:
                return self.eng.apply_yuv_stack(dev, d, **kw)
            import torch
            cur = torch.cuda.current_stream()
            stream.wait_stream(cur)
            with torch.cuda.stream(stream):
                self.eng.apply_yuv_stack(dev, d, **kw)
            cur.wait_stream(stream)
        return self._go(what, want, call, expect, defer)

    def rgb_stack(self, stages, pix_fmt, out=None, c=None, mtx=None, size=(W, H, 2), matrix_out="smpte170m"):
        w, h, nf = size
        src = RS._src(pix_fmt, "natural", w, h, nf=nf, k=7)
        want = lambda: RS._want(self.res, stages, c, mtx, pix_fmt, out, src, f"step{next(_STEP)}", matrix_out=matrix_out)
        dl = RS.twin.source_depth(pix_fmt)
        dev = RS._dev(src, self.eng.device)
        kw = dict(pix_fmt=pix_fmt, out_pix_fmt=RS._out_name(pix_fmt, out), stages=stages, cdl=c, rgb_matrix=mtx, matrix_out=matrix_out)
        no_vec = self.variant == "generic" or (dl == 8 and out is not None and out[0] > 8)
        expect = RS.GENERIC + RS._list(stages) if no_vec else RS._vec_name(pix_fmt, out, stages)
        return self._go(f"apply_rgb_stack {pix_fmt}->{kw['out_pix_fmt']} {stages}", want,
                                 lambda d: self.eng.apply_rgb_stack(dev, d, **kw), expect, False)

    def y2r_stack(self, stages, pix_fmt, out_fmt, c=None, mtx=None, size=(W, H, 2)):
        w, h, nf = size
        src = Y2._src(pix_fmt, "natural", w, h, nf=nf, k=8)
        want = lambda: Y2._want(self.res, stages, c, mtx, pix_fmt, out_fmt, src, f"step{next(_STEP)}")
        dev = Y2._dev(src, self.eng.device)
        kw = dict(pix_fmt=pix_fmt, out_pix_fmt=out_fmt, stages=stages, cdl=c, rgb_matrix=mtx)
        no_vec = self.variant == "generic" or not Y2._has_vec(pix_fmt, out_fmt, stages)
        expect = Y2.GENERIC + Y2._list(stages) if no_vec else Y2._vec_name(pix_fmt, out_fmt, stages)
        return self._go(f"apply_yuv_stack_to_rgb {pix_fmt}->{out_fmt} {stages}", want,
                                 lambda d: self.eng.apply_yuv_stack_to_rgb(dev, d, **kw), expect, False)

    def to_rgb(self, pix_fmt, out_fmt, size=(W, H, 2)):
        """apply_yuv_to_rgb: the bits of the stack ("lut3d",) into an RGB frame, so that twin is its reference."""
        w, h, nf = size
        src = Y2._src(pix_fmt, "natural", w, h, nf=nf, k=8)
        want = lambda: Y2._want(self.res, "lut3d", None, None, pix_fmt, out_fmt, src, f"step{next(_STEP)}")
        dev = Y2._dev(src, self.eng.device)
        generic = self.variant == "generic" or not Y2._has_vec(pix_fmt, out_fmt, "lut3d")
        din, lay, _a = Y2._fmt(pix_fmt)
        expect = "k_yuv2rgb_generic" if generic else Y2R._vec_name(din, lay, out_fmt, "tetrahedral")
        return self._go(f"apply_yuv_to_rgb {pix_fmt}->{out_fmt}", want,
                                 lambda d: self.eng.apply_yuv_to_rgb(dev, d, pix_fmt=pix_fmt, out_pix_fmt=out_fmt), expect, False)

    def to_yuv(self, pix_fmt, out, size=(W, H, 2)):
        """apply_rgb_to_yuv: the bits of the RGB stack ("lut3d",) into a YUV frame, so that twin is its reference."""
        w, h, nf = size
        src = RS._src(pix_fmt, "natural", w, h, nf=nf, k=7)
        want = lambda: RS._want(self.res, "lut3d", None, None, pix_fmt, out, src, f"step{next(_STEP)}")
        dev = RS._dev(src, self.eng.device)
        dl = RS.twin.source_depth(pix_fmt)
        generic = self.variant == "generic" or (dl == 8 and out[0] > 8)
        expect = "k_rgb2yuv_generic" if generic else R2Y._vec_name(pix_fmt, out[0], out[1], "tetrahedral")
        return self._go(f"apply_rgb_to_yuv {pix_fmt}->{RS._yuv(*out)}", want,
                                 lambda d: self.eng.apply_rgb_to_yuv(dev, d, pix_fmt=pix_fmt, out_pix_fmt=RS._yuv(*out)), expect, False)


# ------------------------------------------------------------------ resources
@pytest.fixture(scope="module")
def files(cube_dir, tmp_path_factory):
    d = tmp_path_factory.mktemp("stack_history")
    rng = np.random.default_rng(23)
    out = dict(log709_33=cube_dir / "log709_33.cube", random_9=cube_dir / "random_9.cube")
    out["n2"] = cube.write_cube(d / "n2.cube", rng.uniform(0.0, 1.0, size=(2, 2, 2, 3)).astype(F))
    out["n17"] = cube.write_cube(d / "n17.cube", cube.log709_lattice(17))
    out["n33b"] = cube.write_cube(d / "n33b.cube", (0.5 * cube.log709_lattice(33) + 0.5 * cube.identity_lattice(33)).astype(F))
    out["domain"] = cube.write_cube(d / "domain.cube", cube.log709_lattice(17), domain_min=(0, 0, 0), domain_max=(1.25, 1.25, 1.25))
    out["csp"] = d / "shaped.csp"
    write_csp_with_prelut(out["csp"], 17, cube.log709_lattice(17), [(XS, XS ** 0.7), (XS, XS), (XS, XS + 0.3 * XS * (1.0 - XS))])
    for k in (1, 2):
        out[f"unit{k}"] = cube.write_cube(d / f"unit{k}.cube", ES._unit_lattice(33, 40 + k))
    return out


@pytest.fixture(scope="module")
def l1ds():
    return {n: _keep(cube.read_lut1d(GOLDEN / "lut1d" / f"{n}.cube")) for n in ("curve17", "gamma1024")}


@pytest.fixture()
def hist(orc, files, l1ds):
    """A fresh engine with log709_33, random_9 and gamma1024 (cubic): the families' `loaded` state, as a history's first step."""
    from lut_renderer_amd.engine import LutEngine
    with LutEngine(0) as eng:
        h = Hist(eng, orc)
        h.set_lut(files["log709_33"])
        h.set_lut2(files["random_9"])
        h.set_lut1d(l1ds["gamma1024"], "cubic", "gamma1024")
        yield h


def _yuv(depth, lay="420"):
    return ST._fmt(depth, lay)


def _gbrp(depth):
    return Y2._gbrp(depth)


def _cdl_entries(h, c, depth):
    """The four entries that read the CDL table, at LUT depth `depth`."""
    h.cdl(c, depth, "420")
    h.stack("cdl,lut3d", depth, "420", depth, "422", c=c)
    h.rgb_stack("cdl,lut3d", _gbrp(depth), None, c=c)
    h.y2r_stack("cdl,lut3d", _yuv(10 if depth == 8 else depth), _gbrp(depth), c=c)


# ------------------------------------------------------------------ A. the CDL table
@pytest.mark.gpu
def test_cdl_depth_sequence(hist):
    """10, 8 (a smaller table with another stride in the same buffer), 16 (the buffer grows), 10, 12; the 16- and 12-bit steps
    also flip the stack kernels from LDS to global tables."""
    for depth in (10, 8, 16, 10, 12):
        _cdl_entries(hist, SHOT, depth)
    assert ",1>[" in ST._vec_name(10, 10, "420", "422", "cdl,lut3d", ST._lds("cdl,lut3d", 10))
    assert not ST._lds("cdl,lut3d", 12) and not ST._lds("cdl,lut3d", 16)


@pytest.mark.gpu
def test_cdl_one_key_number_at_a_time(hist):
    """Slope G, offset B, power R, one per step; saturation alone (the key is unchanged); the first CDL again."""
    steps = [SHOT, _cdl(slope=_one(SHOT.slope, 1, SHOT.slope[1] + 0.07))]
    steps.append(_cdl(steps[-1], offset=_one(SHOT.offset, 2, SHOT.offset[2] - 0.03)))
    steps.append(_cdl(steps[-1], power=_one(SHOT.power, 0, SHOT.power[0] + 0.15)))
    steps.append(_cdl(steps[-1], saturation=SHOT.saturation + 0.35))
    steps.append(SHOT)
    for c in steps:
        _cdl_entries(hist, c, 10)


@pytest.mark.gpu
def test_cdl_same_grade_another_depth_through_another_entry(hist):
    hist.y2r_stack("cdl,lut3d", "yuv420p10le", "gbrp", c=SHOT)                     # the table at 8
    hist.stack("cdl,lut3d", 10, "420", 10, "422", c=SHOT)                          # ... and right after at 10
    hist.y2r_stack("lut1d,cdl", "yuv420p10le", "rgb24", c=SHOT)
    hist.cdl(SHOT, 10, "420")
    hist.set_variant("generic")                                                    # 67 x 21 on the generic kernels: 8, then 10
    small = (SW, SH, 1)
    hist.y2r_stack("cdl,lut3d", "yuv420p10le", "gbrp", c=SHOT, size=small)
    hist.cdl(SHOT, 10, "420", size=small)
    hist.rgb_stack("cdl,lut3d", "rgb24", (8, "420"), c=SHOT, size=small)
    hist.stack("cdl,lut3d", 10, "444", 10, "420", c=SHOT, size=small)


@pytest.mark.gpu
def test_cdl_two_clips_back_to_back(hist):
    """Two calls with two CDLs into two destinations, no host read and no sync() between them; then the same on two streams.
    The refill of the second call is queued behind the first call's kernel (the context's stream; a stream change waits for the
    context's `done` event): the expectations are deterministic, and this runs once."""
    import torch
    other = _keep(_cdl(slope=(0.9, 1.0, 1.2), offset=(-0.02, 0.0, 0.02), power=(1.2, 1.1, 0.9), saturation=1.4))
    a = hist.stack("cdl,lut3d", 10, "420", 10, "422", c=SHOT, defer=True)
    b = hist.stack("cdl,lut3d", 10, "420", 10, "422", c=other, defer=True)
    a.launch(), b.launch()
    a.finish(), b.finish()
    a, b = hist.cdl(SHOT, 10, "420", defer=True), hist.cdl(other, 10, "420", defer=True)
    a.launch(), b.launch()
    a.finish(), b.finish()
    s1, s2, cur = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.current_stream()
    a = hist.stack("cdl,lut3d", 10, "420", 10, "422", c=SHOT, defer=True)
    b = hist.stack("cdl,lut3d", 10, "420", 10, "422", c=other, defer=True)
    s1.wait_stream(cur), s2.wait_stream(cur)
    hist.log.append("two torch streams")
    with torch.cuda.stream(s1):
        a.launch()
    with torch.cuda.stream(s2):
        b.launch()
    cur.wait_stream(s1), cur.wait_stream(s2)
    torch.cuda.synchronize()
    a.finish(), b.finish()


# ------------------------------------------------------------------ B. the 1D tables
def _l1d_entries(h, depth, which):
    c = SHOT
    run = dict(yuv=lambda: h.l1d(depth, "420"), alone=lambda: h.l1d(depth, "420", mode=None), rgb=lambda: h.rgb_l1d(depth),
               stack=lambda: h.stack("lut1d,lut3d", depth, "420", depth, "422"),
               rgbs=lambda: h.rgb_stack("lut1d,cdl,lut3d", _gbrp(depth), None, c=c),
               y2r=lambda: h.y2r_stack("lut1d,lut3d", _yuv(10 if depth == 8 else depth), _gbrp(depth)))
    for name in which:
        run[name]()


@pytest.mark.gpu
def test_lut1d_tables_follow_the_generation(hist, l1ds):
    _l1d_entries(hist, 10, ("yuv", "stack", "rgb"))                                # gamma1024 cubic at 10, then 8
    _l1d_entries(hist, 8, ("rgbs", "y2r", "rgb"))
    hist.set_lut1d(l1ds["curve17"], "linear", "curve17")
    _l1d_entries(hist, 10, ("stack", "rgbs", "yuv"))                               # rebuilt
    assert ST._lds("lut1d,lut3d", 12) and 3 * (1 << 12) * 2 == 24 * 1024
    _l1d_entries(hist, 12, ("stack", "y2r", "alone"))                              # first build at 12: 24 KB exactly, in LDS
    _l1d_entries(hist, 8, ("yuv", "stack", "rgb"))                                 # this table is two generations old
    hist.set_lut1d(l1ds["curve17"], "cubic", "curve17")                            # the same object, another mode
    _l1d_entries(hist, 10, ("y2r", "rgb", "alone"))
    _l1d_entries(hist, 12, ("rgbs",))
    hist.set_lut1d(None)
    dev = ST._dev(ST._src("natural", W, H, 10, "420", k=6, nf=2), hist.eng.device)
    hist.refused("apply_yuv_lut1d", ValueError, "no 1D LUT is loaded", lambda: hist.eng.apply_yuv_lut1d(dev, pix_fmt="yuv420p10le"))
    hist.refused("apply_rgb_lut1d", ValueError, "no 1D LUT is loaded", lambda: hist.eng.apply_rgb_lut1d(dev, depth=10))
    for entry, kw in (("apply_yuv_stack", dict(pix_fmt="yuv420p10le")), ("apply_yuv_stack_to_rgb", dict(pix_fmt="yuv420p10le", out_pix_fmt="gbrp10le"))):
        hist.refused(entry, ValueError, "stage 'lut1d' is listed and no 1D LUT is loaded",
                     lambda: getattr(hist.eng, entry)(dev, stages="lut1d,lut3d", **kw))
    hist.stack("cdl,lut3d", 10, "420", 10, "422", c=SHOT)                          # a stack without the stage still runs
    hist.y2r_stack("lut3d,lut3d2", "yuv420p10le", "gbrp10le")
    hist.set_lut1d(l1ds["gamma1024"], "linear", "gamma1024")                       # set again: 8 and 10 with no explicit reset
    _l1d_entries(hist, 8, ("stack", "yuv"))
    _l1d_entries(hist, 10, ("rgb", "y2r", "stack"))
    hist.set_variant("generic")                                                    # 67 x 21 on the generic kernels
    hist.set_lut1d(l1ds["curve17"], "cosine", "curve17")
    small = (SW, SH, 1)
    hist.l1d(10, "420", size=small)
    hist.stack("lut1d,lut3d", 8, "420", 8, "422", size=small)
    hist.y2r_stack("lut1d,lut3d", "yuv420p10le", "rgb48le", size=small)


# ------------------------------------------------------------------ C. the lattices beside each other
@pytest.mark.gpu
def test_second_lattice_sizes_under_first_lattice_changes(hist, files):
    def both():
        hist.chain(10, "420")
        hist.stack("lut3d,lut3d2", 10, "420", 10, "422")

    both()                                                                         # log709_33, random_9
    hist.set_lut(files["n17"])                                                     # the second one's results do not move
    both()
    hist.set_lut2(files["n33b"])
    both()
    hist.set_lut(files["domain"])
    both()
    hist.set_lut2(files["n2"])
    both()
    hist.rgb_stack("lut3d2,lut3d", "gbrp10le", (10, "420"))
    hist.set_lut2(None)
    dev = ST._dev(ST._src("natural", W, H, 10, "420", k=5, nf=2), hist.eng.device)
    hist.refused("apply_yuv_chain", *REFUSED["lut2"], lambda: hist.eng.apply_yuv_chain(dev, pix_fmt="yuv420p10le"))
    hist.refused("apply_yuv_stack", ValueError, "stage 'lut3d2' is listed and no second LUT is loaded",
                 lambda: hist.eng.apply_yuv_stack(dev, pix_fmt="yuv420p10le", stages="lut3d,lut3d2"))
    hist.stack("lut1d,lut3d", 10, "420", 10, "422")
    hist.set_lut2(files["random_9"])
    both()
    hist.set_variant("generic")                                                    # 67 x 21 on the generic kernels
    hist.set_lut2(files["n2"])
    hist.chain(10, "420", size=(SW, SH, 1))
    hist.stack("lut3d,lut3d2", 10, "420", 10, "422", size=(SW, SH, 1))


@pytest.mark.gpu
def test_prelut_tables_and_the_refusals(hist, files):
    dev = ST._dev(ST._src("natural", W, H, 10, "420", k=6, nf=2), hist.eng.device)

    def refusals(expected):
        for stages, kw in (("cdl,lut3d", dict(cdl=SHOT)), ("matrix,lut3d", dict(rgb_matrix=I3))):
            if expected:
                hist.refused(f"[{stages}]", ValueError, "directly behind",
                             lambda: hist.eng.apply_yuv_stack(dev, pix_fmt="yuv420p10le", stages=stages, **kw))
                hist.refused(f"[{stages}] into RGB", ValueError, "directly behind",
                             lambda: hist.eng.apply_yuv_stack_to_rgb(dev, pix_fmt="yuv420p10le", out_pix_fmt="gbrp", stages=stages, **kw))
            else:
                hist.stack(stages, 10, "420", 10, "422", c=kw.get("cdl"), mtx=kw.get("rgb_matrix"))
                hist.y2r_stack(stages, "yuv420p10le", "gbrp", c=kw.get("cdl"), mtx=kw.get("rgb_matrix"))

    def runs():                                                                    # two depths through two entries: pre_tab at 10 and 8
        hist.stack("lut1d,lut3d", 10, "420", 10, "422")
        hist.y2r_stack("lut1d,lut3d", "yuv420p10le", "gbrp")
        hist.l1d(10, "420")
        hist.rgb_stack("cdl,lut1d,lut3d", "rgb24", (8, "420"), c=SHOT)

    for name in ("csp", "n17", "csp"):
        lut = hist.set_lut(files[name])
        assert (lut.prelut is not None) == (name == "csp") == hist.eng._has_prelut
        refusals(name == "csp")
        runs()


@pytest.mark.gpu
def test_precision_around_stack_calls(hist, files, orc):
    """The stack passes are strict whatever the precision; the tile route behind them must use the copy derived from the
    CURRENT lattice.  The reference of the plain call is the twin `last_kernel`'s tag names."""
    from lut_renderer_amd import frames
    k = orc.yuv_constants(din=10)
    src = frames.make_yuv("natural", 512, 128, 10, 1, 1, k=31)
    for prec, name in (("fast", "unit1"), ("fma32", "unit2"), ("strict", "log709_33"), ("fast", "unit2"), ("fma32", "unit1")):
        hist.set_precision(prec)
        hist.stack("lut1d,cdl,lut3d", 10, "420", 10, "422", c=SHOT)
        lut = hist.set_lut(files[name])
        hist.stack("lut3d,lut3d2", 10, "420", 10, "422")
        hist.y2r_stack("cdl,lut3d", "yuv420p10le", "gbrp10le", c=SHOT)
        got = ES._run_yuv(hist.eng, src, "yuv420p10le", 10)
        hist.log.append(f"apply_yuv -> {hist.kernel()}")
        # the LDS-window tile kernel of 16-bit words in and out at 4:2:0, tetrahedral; its tag names the precision that ran
        assert hist.kernel().startswith("k_yuv_tile2<11,11,2,") and ("," + prec in hist.kernel()) == (prec != "strict"), hist.log
        ES._eq(got, ES._yuv_ref(orc, hist.eng, lut, "tetrahedral", k, 10, 10, 10, src), f"apply_yuv under {prec} after {name}", hist.log)


# ------------------------------------------------------------------ D. strength and matte
@pytest.mark.gpu
@pytest.mark.parametrize("side_stream", [False, True], ids=["current_stream", "side_stream_between"])
def test_strength_and_matte_sequence(hist, side_stream):
    import torch
    st, run = "lut1d,cdl,lut3d", dict(din=10, a="420", dout=10, b="422", c=SHOT)
    hist.stack(st, strength=[0.0, 1.0, 0.37], size=(W, H, 3), **run)
    if side_stream:
        hist.stack(st, strength=0.45, size=(W, H, 3), stream=torch.cuda.Stream(), **run)
    hist.stack(st, strength=0.6, size=(W, H, 3), **run)
    hist.stack(st, strength=[0.25, 0.8], **run)
    if side_stream:
        hist.stack(st, strength=[0.5, 0.125], stream=torch.cuda.Stream(), **run)
        hist.stack(st, strength=[1.0, 0.3], **run)
    hist.stack(st, strength=[1.0, 0.5], matte=(10, False), **run)
    hist.stack(st, strength=0.8, matte=(8, True), **run)
    hist.stack(st, **run)
    hist.stack("lut1d,matrix,lut3d", 10, "420", 10, "422", mtx=OFFSET)
    hist.stack(st, strength=[0.7, 0.0], **run)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ E. a seeded walk
WALK_SEED, WALK_STEPS = 22833861, 60
#: the apply table: (entry, arguments); every YUV / RGB format of the issue's list occurs
APPLIES = (
    ("cdl", dict(din=10, a="420")),
    ("cdl", dict(din=8, a="420")),
    ("l1d", dict(din=10, a="444")),
    ("l1d", dict(din=16, a="422", mode=None)),
    ("chain", dict(din=10, a="420")),
    ("stack", dict(stages="lut1d,cdl,lut3d", din=10, a="420", dout=10, b="422")),
    ("stack", dict(stages="cdl,lut3d", din=10, a="420", strength=[0.3, 0.9])),
    ("stack", dict(stages="lut1d,lut3d", din=8, a="420", matte=(8, False))),
    ("stack", dict(stages="matrix,lut3d", din=10, a="444")),
    ("stack", dict(stages="lut1d,lut3d,lut3d2", din=16, a="422")),
    ("rgb_stack", dict(stages="lut1d,cdl,lut3d", pix_fmt="gbrp10le", out=None)),
    ("rgb_stack", dict(stages="cdl,lut3d", pix_fmt="rgb24", out=(8, "420"))),
    ("y2r_stack", dict(stages="lut1d,cdl,lut3d", pix_fmt="yuv420p10le", out_fmt="gbrp10le")),
    ("y2r_stack", dict(stages="lut3d,lut1d", pix_fmt="yuv420p", out_fmt="gbrp10le")),       # no vector kernel
    ("to_rgb", dict(pix_fmt="yuv444p10le", out_fmt="rgb24")),
    ("to_yuv", dict(pix_fmt="gbrp10le", out=(10, "420"))),
)
WALK_LUTS = [(n, kind) for n in (9, 17, 33) for kind in ("cube", "domain", "csp")]


def _refusal(entry, kw, prelut, lut2, variant):
    """Why the engine refuses this draw in this state (documented reasons only), or None."""
    kinds = kw.get("stages", "").split(",")
    behind = any(a in ("cdl", "matrix") and b == "lut3d" for a, b in zip(kinds, kinds[1:]))
    if prelut and (entry == "cdl" or behind):
        return "prelut"
    if not lut2 and (entry == "chain" or "lut3d2" in kinds):
        return "lut2"
    if variant == "vec_global" and entry == "y2r_stack" and kw["pix_fmt"] == "yuv420p" and kw["out_fmt"] == "gbrp10le":
        return "vec_global"
    return None


#: what the engine holds when the walk begins (the `hist` fixture, SHOT and GAMUT), in the words of the draws below
WALK_START = dict(lut=(33, "cube"), lut2="random_9", lut1d=("gamma1024", "cubic"), cdl=None, matrix="gamut", variant="auto",
                  precision="strict")
WALK_CHOICES = dict(
    lut=WALK_LUTS, lut2=("random_9", "n2", "n33b", None),
    lut1d=[(n, m) for n in ("curve17", "gamma1024") for m in ("linear", "cubic", "cosine")],
    cdl=[(sl, of, pw, sat) for sl in (0.9, 1.1, 1.3) for of in (-0.05, 0.0, 0.04) for pw in (0.8, 1.0, 1.25) for sat in (0.6, 1.0, 1.5)],
    matrix=("identity", "gamut", "offset"), variant=("auto", "vec_global", "generic"), precision=("strict", "fast", "fma32"))
NO_VECTOR_KERNEL = 13        # the entry of APPLIES that has none


def walk_plan(seed=WALK_SEED, steps=WALK_STEPS):
    """The draw, without a GPU: a list of dict(act=..., ...).  A state change carries `value`, always another one than the state
    current at that step (`was`); an apply carries the table `entry`, its `refusal` and the `variant` it runs under.  The seed is
    one whose draw meets the conditions tests/test_stack_upload_markers.py asserts: applies that run, and state changes."""
    rng = random.Random(seed)
    state, plan, deck = dict(WALK_START), [], []
    for _ in range(steps):
        act = rng.choice(tuple(WALK_CHOICES) + ("apply",) * 12)
        s = dict(act=act)
        if act != "apply":
            s["was"] = state[act]
            s["value"] = state[act] = rng.choice([v for v in WALK_CHOICES[act] if v != state[act]])
        else:
            if not deck:            # the table is dealt like a deck of cards: every entry comes up before one repeats
                deck = list(range(len(APPLIES)))
                rng.shuffle(deck)
            s["entry"], s["variant"] = deck.pop(), state["variant"]
            s["refusal"] = _refusal(*APPLIES[s["entry"]], state["lut"][1] == "csp", state["lut2"] is not None, state["variant"])
        plan.append(s)
    return plan


def _reads(entry, kw):
    """The kinds of state an apply of the table reads."""
    kinds = kw.get("stages", "").split(",")
    out = {"variant", "precision"}
    if entry in ("cdl", "chain", "to_rgb", "to_yuv") or "lut3d" in kinds or (entry == "l1d" and kw.get("mode", "") is not None):
        out.add("lut")
    if entry == "chain" or "lut3d2" in kinds:
        out.add("lut2")
    if entry == "l1d" or "lut1d" in kinds:
        out.add("lut1d")
    if entry == "cdl" or "cdl" in kinds:
        out.add("cdl")
    if "matrix" in kinds:
        out.add("matrix")
    return out


def walk_coverage(plan):
    """What a draw covers: dict(ran=applies that run, per_entry=[runs of each table entry], refusals={reasons}, changes={kind:
    [values drawn]}, same=[state changes that drew the current state], followed={kinds of change with a vector-kernel apply that
    reads that state behind one of them, before the next change of the kind}, lut_kinds={file kinds of the first lattices that
    were loaded and applied before the next one replaced them})."""
    ran = [s for s in plan if s["act"] == "apply" and s["refusal"] is None]
    changes = {k: [s["value"] for s in plan if s["act"] == k] for k in WALK_CHOICES}
    followed, fresh, lut, lut_kinds = set(), set(), None, set()
    for s in plan:
        if s["act"] != "apply":
            fresh.add(s["act"])
            lut = s["value"] if s["act"] == "lut" else lut
            continue
        if s["refusal"] is None and lut is not None and "lut" in _reads(*APPLIES[s["entry"]]):
            lut_kinds.add(lut[1])       # a first lattice of this file kind was loaded AND applied before the next one came
        if s["refusal"] is None and s["variant"] != "generic" and s["entry"] != NO_VECTOR_KERNEL:
            hit = fresh & _reads(*APPLIES[s["entry"]])
            followed |= hit
            fresh -= hit
    return dict(ran=len(ran), per_entry=[sum(1 for s in ran if s["entry"] == i) for i in range(len(APPLIES))],
                refusals={s["refusal"] for s in plan if s["act"] == "apply"} - {None}, changes=changes,
                same=[s for s in plan if s["act"] != "apply" and s["value"] == s["was"]], followed=followed, lut_kinds=lut_kinds)


REFUSED = dict(prelut=(ValueError, "\\.csp prelut"), lut2=((ValueError, _native.LutrError), "no second (LUT is loaded|lattice set)"),
               vec_global=(ValueError, "vec_global cannot take an 8-bit source"))


def _walk_lut(d, step, n, kind):
    tab = ES._unit_lattice(n, step) if step % 2 else cube.log709_lattice(n).astype(F)
    if kind == "csp":
        p = d / f"s{step}.csp"
        write_csp_with_prelut(p, n, tab, [(XS, XS ** 0.8), (XS, XS + 0.3 * XS * (1.0 - XS)), (XS, XS)])
        return p
    dom = dict(domain_min=(0, 0, 0), domain_max=(1.25, 1.25, 1.25)) if kind == "domain" else {}
    return cube.write_cube(d / f"s{step}.cube", tab, **dom)


@pytest.mark.gpu
def test_seeded_stack_walk(hist, files, l1ds, tmp_path):
    matrices = dict(identity=I3, gamut=GAMUT, offset=OFFSET)
    c, mtx = SHOT, GAMUT
    for i, s in enumerate(walk_plan()):
        act = s["act"]
        if act == "lut":
            hist.set_lut(_walk_lut(tmp_path, i, *s["value"]))
        elif act == "lut2":
            hist.set_lut2(None if s["value"] is None else files[s["value"]])
        elif act == "lut1d":
            hist.set_lut1d(l1ds[s["value"][0]], s["value"][1], s["value"][0])
        elif act == "cdl":
            sl, of, pw, sat = s["value"]
            c = _keep(Cdl(slope=(sl, 1.0, 2.2 - sl), offset=(of, 0.0, -of), power=(pw, 1.0, 1.0 / pw), saturation=sat))
            hist.log.append(f"cdl {c.sop_text()} sat {sat}")
        elif act == "matrix":
            mtx = matrices[s["value"]]
            hist.log.append(f"matrix {s['value']}")
        elif act == "variant":
            hist.set_variant(s["value"])
        elif act == "precision":
            hist.set_precision(s["value"])
        else:
            entry, kw = APPLIES[s["entry"]]
            kw = dict(kw)
            if entry == "cdl":
                kw["c"] = c
            elif "cdl" in kw.get("stages", ""):
                kw["c"] = c
            if "matrix" in kw.get("stages", ""):
                kw["mtx"] = mtx
            hist.refusal = None if s["refusal"] is None else REFUSED[s["refusal"]]
            getattr(hist, entry)(**kw)
            hist.refusal = None


# ------------------------------------------------------------------ F. apply_lut on kept engines
class _ApplyLut:
    """`api.apply_lut` through its three stage-list routes on one kept engine (a LutEngine, a LutEngineGroup, or None: the
    process's cached engine), each result against the family's reference of the files / objects passed to that call."""
    CALL = dict(colorspace="bt709", color_range="tv")
    STAGES = "lut1d,cdl,lut3d,lut3d2"

    def __init__(self, eng, orc, device):
        self.eng, self.orc, self.device, self.log = eng, orc, device, []

    def _res(self, A, B, l1, mode):
        return dict(lut=A, lut2=B, l1=(l1, mode), prelut=None)

    def case(self, route, res, c):
        """(the reference, the route's keywords, the device source, the kernel's full name: the vector kernel of the family with the
        stage list and the placement flag of 18 KB of tables) of one call."""
        stages, key = self.STAGES, f"step{next(_STEP)}"
        if route == "stages":
            src = ST._src("natural", W, H, 10, "420", k=6, nf=2)
            return (ST._want(res, stages, c, 10, 10, 10, "420", "422", src, key),
                    dict(pix_fmt="yuv420p10le", out_pix_fmt="yuv422p10le", stages=stages), ST._dev(src, self.device),
                    ST._vec_name(10, 10, "420", "422", stages, ST._lds(stages, 10)))
        if route == "rgb_stages":
            src = RS._src("gbrp10le", "natural", W, H, nf=2, k=7)
            return (RS._want(res, stages, c, None, "gbrp10le", (10, "420"), src, key, matrix_out="bt709"),
                    dict(pix_fmt="gbrp10le", out_pix_fmt="yuv420p10le", rgb_stages=stages), RS._dev(src, self.device),
                    RS._vec_name("gbrp10le", (10, "420"), stages))
        src = Y2._src("yuv420p10le", "natural", W, H, nf=2, k=8)
        return (Y2._want(res, stages, c, None, "yuv420p10le", "rgb48le", src, key),
                dict(pix_fmt="yuv420p10le", rgb_out="rgb48le", rgb_out_stages=stages), Y2._dev(src, self.device),
                Y2._vec_name("yuv420p10le", "rgb48le", stages))

    def run(self, route, A, B, l1, mode, c, what):
        """A, B: (path or CubeLut, parsed CubeLut); l1: (path or Lut1D, parsed Lut1D)."""
        from lut_renderer_amd import api
        import torch
        want, kw, dev, name = self.case(route, self._res(A[1], B[1], l1[1], mode), c)
        common = dict(cube=A[0], cube2=B[0], lut1d=l1[0], interp1d=mode, cdl=c, engine=self.eng, **self.CALL)
        dst = _sentinels(want, self.device)
        api.apply_lut(dev, out=dst, **kw, **common)
        eng = self.eng if self.eng is not None else api._cached_engine((0,))
        eng.sync()
        torch.cuda.synchronize()
        kernels = eng.last_kernels if hasattr(eng, "last_kernels") else [eng.last_kernel]
        self.log.append(f"apply_lut {route} {what} -> {kernels}")
        assert ST._lds(self.STAGES, 10) and all(k == name for k in kernels), (name, self.log)     # (every context of a group)
        if hasattr(eng, "last_kernels"):
            assert eng.last_remote == 1, self.log
        ES._eq([_host(t) for t in _as_list(dst)], _as_list(want), f"apply_lut {route} {what}", self.log)


def _kept_engine_history(al, files, l1ds, tmp_path):
    """Section F's history on the engine of `al`."""
    from lut_renderer_amd import api
    parsed = lambda p: (p, _keep(api._cached_cube(Path(p))))                        # noqa: E731
    A, A2 = (_keep(cube.read_lut(files["log709_33"])),) * 2, (_keep(cube.read_lut(files["n17"])),) * 2
    B, B2 = (_keep(cube.read_lut(files["random_9"])),) * 2, (_keep(cube.read_lut(files["n2"])),) * 2
    g, cv = (l1ds["gamma1024"],) * 2, (l1ds["curve17"],) * 2
    other = _keep(_cdl(saturation=1.3, slope=(1.0, 0.9, 1.2)))
    al.run("stages", A, B, g, "cubic", SHOT, "first call")
    al.run("rgb_stages", A, B, g, "cubic", other, "the same objects, another CDL")
    al.run("rgb_out_stages", A, B, g, "cubic", SHOT, "the same objects, third route")
    al.run("stages", A2, B2, cv, "linear", SHOT, "other objects")
    al.run("rgb_stages", A2, B2, cv, "cubic", SHOT, "the same 1D LUT object, another interp1d")
    al.run("rgb_out_stages", A, B2, cv, "cubic", other, "the first lattice back")
    eng = al.eng if al.eng is not None else api._cached_engine((0,))
    # the engine's own setters between two calls that pass the same objects: the markers clear, the next call uploads again
    eng.set_lut1d(g[1], "linear")
    eng.set_lut2(B[1])
    eng.set_lut(A2[1])
    al.log.append("set_lut1d / set_lut2 / set_lut directly")
    al.run("stages", A, B2, cv, "cubic", SHOT, "the same objects after direct setters")
    eng.set_lut2(None)
    eng.set_lut1d(None)
    al.log.append("set_lut2(None) / set_lut1d(None) directly")
    al.run("rgb_stages", A, B2, cv, "cubic", SHOT, "the same objects after their removal")
    # files rewritten in place with a moved mtime: a second-LUT file and a 1D file
    p2, p1 = tmp_path / "second.cube", tmp_path / "curve.cube"
    for i in range(2):
        cube.write_cube(p2, ES._unit_lattice(9 if i else 5, 70 + i))
        cube.write_lut1d(p1, np.stack([XS ** (0.6 + 0.5 * i), XS, 1.0 - (1.0 - XS) ** (1.5 - 0.4 * i)]))
        for p in (p1, p2):
            os.utime(p, (1_700_000_000 + i, 1_700_000_000 + i))
        l1 = (p1, _keep(api._cached_cube(p1, cube.read_lut1d)))
        for route in ("stages", "rgb_out_stages") if i else ("rgb_stages",):
            al.run(route, parsed(files["log709_33"]), parsed(p2), l1, "linear", SHOT, f"files, version {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["engine", "cached", "group"])
def test_apply_lut_on_kept_engines(orc, files, l1ds, tmp_path, kind):
    from lut_renderer_amd import api
    from lut_renderer_amd.engine import LutEngine
    from lut_renderer_amd.multigpu import LutEngineGroup
    if kind == "cached":
        try:
            _kept_engine_history(_ApplyLut(None, orc, "cuda:0"), files, l1ds, tmp_path)
        finally:
            api.close_cached_engines()
        return
    with (LutEngine(0) if kind == "engine" else LutEngineGroup((0, 0), treat_as_remote=True)) as eng:
        _kept_engine_history(_ApplyLut(eng, orc, "cuda:0"), files, l1ds, tmp_path)
