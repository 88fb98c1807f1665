"""The refusals of the fused YUV entry points at the C-ABI, in order.  The Python layer refuses most bad calls before they reach
liblutr, so these call engine._lib.lutr_apply_* themselves with ctypes structs and pin (return code, lutr_last_error()) -- the
texts are literals copied from lutr_api.cpp.  Where a call breaks two rules the first refusal in the source wins, and the pairs
below pin that order.  Every call here is refused or empty: no kernel of the library is launched, and every destination still
holds its fill afterwards.

Frame: 16 x 8, 2 frames, 10-bit 4:2:0 into 10-bit 4:2:2 where the entry takes a layout change (a 2-row union block), the entry's
own smallest legal layout otherwise.  A case is (mutations of the good call, message); message None = LUTR_OK."""
import ctypes as C
from pathlib import Path

import pytest

from lut_renderer_amd import _native, cube
from lut_renderer_amd.cdl import Cdl

GOLDEN = Path(__file__).resolve().parent / "golden"
W, H, NF = 16, 8, 2
FILL = 0x5a5a
F420, F422, F444 = _native.fmt_code(10, 1, 1), _native.fmt_code(10, 1, 0), _native.fmt_code(10, 0, 0)
RGB48 = _native.packed_code(16, 3, 0, 1, 2)

NULLARG = "null argument"
NULLP = "null yuv params"
INTERP = "unknown interpolation mode 7"
GEOM = "bad geometry w=16 h=8 nframes=2 row0=0 rows=9"
DEPTH7 = "unsupported bit depth (in 10, lut 7, out 10)"
UNION = "row0/rows must be multiples of the union chroma block height 2"
BLOCK = "row0/rows must be multiples of the chroma block height 2"
OBLOCK = "row0/rows must be multiples of the output chroma block height 2"
DITHER = "unknown dither mode 9"
ED_ROWS = "error-diffusion dither couples the rows of a frame: whole frames only (row0 = 0, rows = h)"
IMG_ALIGN = "16-bit packed formats need 2-byte aligned rows"


def _align(side, i):
    return f"{side} plane {i}: 16-bit planes need 2-byte aligned rows"


def _calign(side, i):
    return f"{side} plane {i}: 16-bit containers need 2-byte aligned rows"


def _inplace(what, src, j):
    return (f"{what} cannot run in place: the byte range of {src} overlaps that of destination plane {j} (bounding ranges over all "
            "rows and frames must be disjoint)")


def _lds(noun):
    return f"variant vec_lds: there is no LDS-window kernel for {noun}"


def _variant(engine, name):
    class _Ctx:
        def __enter__(self):
            engine.set_variant(name)

        def __exit__(self, *exc):
            engine.set_variant("auto")
    return _Ctx()


class _Bufs:
    """Sources (zeros) and destinations; every destination is a view of one pool filled with FILL."""

    def __init__(self, device):
        import torch
        self.pool = torch.full((8192,), FILL, dtype=torch.int16, device=device)
        self._used = 0

        def z(*shape, dtype=torch.int16):
            return torch.zeros(shape, dtype=dtype, device=device)
        y, c420, c422 = (NF, H, W), (NF, H // 2, W // 2), (NF, H, W // 2)
        self.s420 = [z(*y), z(*c420), z(*c420)]
        self.d420 = [self._dst(*y), self._dst(*c420), self._dst(*c420)]
        self.d420b = [self._dst(*y), self._dst(*c420), self._dst(*c420)]
        self.d422 = [self._dst(*y), self._dst(*c422), self._dst(*c422)]
        self.alpha, self.matte = z(*y), z(*y)
        self.ssemi = [z(*y), z(NF, H // 2, W)]                        # p010: Y, then CbCr interleaved
        self.dsemi = [self._dst(*y), self._dst(NF, H // 2, W)]
        self.sy210, self.dy210 = [z(NF, H, 2 * W)], [self._dst(NF, H, 2 * W)]
        self.sv210 = [z(NF, H, 12, dtype=torch.int32)]                # 48 bytes a row: three groups of six samples
        self.dv210 = [self._dst(NF, H, 24)]
        self.sgbrp = [z(*y), z(*y), z(*y)]
        self.dgbrp = [self._dst(*y), self._dst(*y), self._dst(*y)]
        self.srgb48, self.drgb48 = z(NF, H, 3 * W), self._dst(NF, H, 3 * W)

    def _dst(self, *shape):
        n = 1
        for s in shape:
            n *= s
        t = self.pool[self._used:self._used + n].view(shape)
        self._used += n
        assert self._used <= self.pool.numel()
        return t

    def untouched(self):
        return bool((self.pool == FILL).all().item())


@pytest.fixture(scope="module")
def loaded(engine, cube_dir):
    """The engine with a lattice, a second lattice and a 1D LUT (no prelut), and the buffers of this file."""
    engine.load_cube(cube_dir / "log709_33.cube")
    engine.load_cube2(cube_dir / "random_9.cube")
    engine.set_lut1d(cube.read_lut1d(GOLDEN / "lut1d" / "curve17.cube"), "linear")
    yield engine, _Bufs(engine.device)
    engine.set_lut2(None)
    engine.set_lut1d(None)


# ------------------------------------------------------------------ arguments under a case's mutations
def _p(m, fmt_in, fmt_out, depth=10):
    if m.get("null_p"):
        return None
    r = m.get("range", 0)
    return C.byref(_native.YuvParams(m.get("fmt_in", fmt_in), m.get("fmt_out", fmt_out), m.get("lut_depth", depth), 0, 0, r, r, 0))


def _sides(m, also=None, **sides):
    """struct lutr_planes pointers of the named sides (name -> tensors).  Mutations: null_<name> (no struct), <name>_null = i (null
    plane i), <name>_odd = i (base pointer + 1), <name>_stride = bytes (plane 0), <name>_at = other (plane 0 at the other side's
    plane 0; `also`: further names and their addresses), no_planes (every base pointer null)."""
    at = {k: t[0].data_ptr() for k, t in sides.items()}
    at.update(also or {})
    out = []
    for name, tensors in sides.items():
        if m.get("null_" + name):
            out.append(None)
            continue
        st = _native.Planes()
        for i, t in enumerate(tensors):
            st.data[i] = t.data_ptr()
            st.stride[i] = t.stride(-2) * t.element_size()
            st.frame_stride[i] = t.stride(0) * t.element_size()
        if name + "_at" in m:
            st.data[0] = at[m[name + "_at"]]
        if name + "_odd" in m:
            st.data[m[name + "_odd"]] += 1
        if name + "_stride" in m:
            st.stride[0] = m[name + "_stride"]
        if name + "_null" in m:
            st.data[m[name + "_null"]] = None
        if m.get("no_planes"):
            for i in range(3):
                st.data[i] = None
        out.append(C.byref(st))
    return out


def _image(m, t, at=None):
    """struct lutr_packed of t.  Mutations: img_null, img_odd, img_at (the image at address `at`)."""
    st = _native.Packed(t.data_ptr(), t.stride(-2) * t.element_size(), t.stride(0) * t.element_size())
    if m.get("img_at"):
        st.data = at
    if m.get("img_odd"):
        st.data += 1
    if m.get("img_null") or m.get("no_planes"):
        st.data = None
    return C.byref(st)


def _geom(m):
    return m.get("w", W), H, NF


def _rows(m):
    row0 = m.get("row0", 0)
    return row0, m.get("rows", H - row0)


def _stages(m):
    stages = m.get("stages", [(1, m.get("interp", 2))])
    arr = (_native.StageStruct * max(len(stages), 1))()
    for i, (kind, interp) in enumerate(stages):
        arr[i].kind, arr[i].interp = kind, interp
    cdl = C.byref(_native.cdl_struct(Cdl())) if m.get("cdl") else None
    return arr, len(stages), cdl


def _alpha(m, B, at):
    if m.get("null_alpha"):
        return None
    a = B.alpha
    st = _native.AlphaSrc(m.get("alpha_kind", _native.ALPHA_INT), 10, a.data_ptr(), a.stride(-2) * 2, a.stride(0) * 2, 1, 0)
    if m.get("alpha_at_dst"):
        st.data = at
    if m.get("alpha_null"):
        st.data = None
    return C.byref(st)


def _matte(m, B, at):
    if m.get("null_matte"):
        return None
    t = B.matte
    st = _native.MatteStruct(t.data_ptr(), m.get("matte_stride", t.stride(-2) * 2), t.stride(0) * 2, m.get("matte_depth", 10),
                             m.get("matte_invert", 0))
    if m.get("matte_at_dst"):
        st.data = at
    if m.get("matte_odd"):
        st.data += 1
    return C.byref(st)


# ------------------------------------------------------------------ the entries
def _yuv(lib, ctx, B, m):
    s, d = _sides(m, src=B.s420, dst=B.d420)
    return lib.lutr_apply_yuv(ctx, _p(m, F420, F420), m.get("interp", 2), *_geom(m), s, d, *_rows(m))


def _sited(lib, ctx, B, m):
    s, d = _sides(m, src=B.s420, dst=B.d420)
    return lib.lutr_apply_yuv_sited(ctx, _p(m, F420, F420), m.get("interp", 2), m.get("loc", 1), *_geom(m), s, d, *_rows(m))


def _xsub(dither):
    def call(lib, ctx, B, m):
        s, d = _sides(m, src=B.s420, dst=B.d422)
        return lib.lutr_apply_yuv_xsub(ctx, _p(m, F420, F422), m.get("interp", 2), m.get("dither", dither), *_geom(m), s, d, *_rows(m))
    return call


def _dual(lib, ctx, B, m):
    s, d, d2 = _sides(m, src=B.s420, dst=B.d422, dst2=B.d420b)
    return lib.lutr_apply_yuv_dual(ctx, _p(m, F420, F422), m.get("fmt_out2", F420), m.get("interp", 2), *_geom(m), s, d, d2, *_rows(m))


def _chain(lib, ctx, B, m):
    s, d = _sides(m, src=B.s420, dst=B.d422)
    return lib.lutr_apply_yuv_chain(ctx, _p(m, F420, F422), m.get("interp", 2), m.get("interp2", 2), *_geom(m), s, d, *_rows(m))


def _cdl(lib, ctx, B, m):
    s, d = _sides(m, src=B.s420, dst=B.d422)
    cdl = None if m.get("null_cdl") else C.byref(_native.cdl_struct(Cdl()))
    return lib.lutr_apply_yuv_cdl(ctx, _p(m, F420, F422), m.get("interp", 2), cdl, *_geom(m), s, d, *_rows(m))


def _lut1d(lib, ctx, B, m):
    s, d = _sides(m, src=B.s420, dst=B.d422)
    return lib.lutr_apply_yuv_lut1d(ctx, _p(m, F420, F422), m.get("interp", 2), *_geom(m), s, d, *_rows(m))


def _stack(lib, ctx, B, m):
    s, d = _sides(m, src=B.s420, dst=B.d422)
    return lib.lutr_apply_yuv_stack(ctx, _p(m, F420, F422), *_stages(m), *_geom(m), s, d, *_rows(m))


def _stack_mix(lib, ctx, B, m):
    s, d = _sides(m, src=B.s420, dst=B.d422)
    return lib.lutr_apply_yuv_stack_mix(ctx, _p(m, F420, F422), *_stages(m), m.get("strength", 0.5), None, *_geom(m), s, d, *_rows(m))


def _stack_matte(lib, ctx, B, m):
    s, d = _sides(m, src=B.s420, dst=B.d422)
    return lib.lutr_apply_yuv_stack_matte(ctx, _p(m, F420, F422), *_stages(m), m.get("strength", 0.5), None,
                                          _matte(m, B, B.d422[0].data_ptr()), *_geom(m), s, d, *_rows(m))


def _premul(lib, ctx, B, m):
    s, d = _sides(m, src=B.s420, dst=B.d422)
    return lib.lutr_apply_yuv_premul(ctx, _p(m, F420, F422), m.get("interp", 2), *_geom(m), s, _alpha(m, B, B.d422[0].data_ptr()), d,
                                     *_rows(m))


def _semi(lib, ctx, B, m):
    lin, lout = m.get("in", (1, 0, 6)), m.get("out", (1, 0, 6))
    s, d = _sides(m, src=B.ssemi, dst=B.dsemi)
    a, b = (None, None) if m.get("null_p") else (C.byref(_native.YuvLayout(*lin)), C.byref(_native.YuvLayout(*lout)))
    return lib.lutr_apply_yuv_semi(ctx, _p(m, F420, F420), m.get("interp", 2), a, b, *_geom(m), s, d, *_rows(m))


def _packed(lib, ctx, B, m):
    pin, pout = m.get("in", (1, 0, 6)), m.get("out", (0, 0, 0))
    s, d = _sides(m, src=B.sy210, dst=B.dy210 if pout[0] else B.d420)
    a, b = (None, None) if m.get("null_p") else (C.byref(_native.YuvPacking(*pin)), C.byref(_native.YuvPacking(*pout)))
    return lib.lutr_apply_yuv_packed(ctx, _p(m, F422, F420), m.get("interp", 2), a, b, *_geom(m), s, d, *_rows(m))


def _v210(lib, ctx, B, m):
    vin, vout = m.get("in", 1), m.get("out", 0)
    s, d = _sides(m, src=B.sv210, dst=B.dv210 if vout else B.d420)
    return lib.lutr_apply_yuv_v210(ctx, _p(m, F422, F420), m.get("interp", 2), vin, vout, *_geom(m), s, d, *_rows(m))


def _rgb2yuv(lib, ctx, B, m):
    s, d = _sides(m, src=B.sgbrp, dst=B.d420)
    return lib.lutr_apply_rgb_to_yuv(ctx, _p(m, F420, F420), m.get("interp", 2), m.get("dither", 0), 0, *_geom(m), s, None, d, *_rows(m))


def _rgb2yuv_packed(lib, ctx, B, m):
    (d,) = _sides(m, dict(src=B.srgb48.data_ptr()), dst=B.d420)
    img = None if m.get("null_src") else _image(m, B.srgb48)
    return lib.lutr_apply_rgb_to_yuv(ctx, _p(m, F420, F420, 16), m.get("interp", 2), m.get("dither", 0), m.get("kind", RGB48), *_geom(m),
                                     None, img, d, *_rows(m))


def _yuv2rgb(lib, ctx, B, m):
    s, d = _sides(m, src=B.s420, dst=B.dgbrp)
    return lib.lutr_apply_yuv_to_rgb(ctx, _p(m, F420, F420), m.get("interp", 2), 0, *_geom(m), s, d, None, *_rows(m))


def _yuv2rgb_packed(lib, ctx, B, m):
    (s,) = _sides(m, src=B.s420)
    img = None if m.get("null_dst") else _image(m, B.drgb48, B.s420[0].data_ptr())
    return lib.lutr_apply_yuv_to_rgb(ctx, _p(m, F420, F420, 16), m.get("interp", 2), m.get("kind", RGB48), *_geom(m), s, None, img,
                                     *_rows(m))


def _run(loaded, call, cases):
    engine, B = loaded
    for m, want in cases:
        with _variant(engine, "vec_lds" if m.get("lds") else "auto"):
            with engine._lock:
                engine._bind_stream()
                rc = call(engine._lib, engine._ctx, B, m)
            msg = engine._lib.lutr_last_error().decode()
        if want is None:
            assert rc == _native.OK, (m, msg)
        else:
            assert (rc, msg) == (_native.EINVAL, want), m
        assert B.untouched(), ("the call wrote to a destination", m)


# ------------------------------------------------------------------ the union-block family
def _union_cases(noun, lds_noun, null_src=NULLARG, interp=INTERP):
    """What every entry of the family refuses, and the order of its shared checks."""
    lds = _lds(lds_noun)
    return [
        (dict(null_p=1), NULLP),
        (dict(null_src=1), null_src),
        (dict(null_dst=1), null_src),
        (dict(interp=7), interp),
        (dict(rows=9), GEOM),
        (dict(lut_depth=7), DEPTH7),
        (dict(row0=1), UNION),
        (dict(lds=1), lds),
        (dict(src_null=1), "null plane 1"),
        (dict(dst_null=1), "null plane 1"),
        (dict(src_odd=0), _align("source", 0)),
        (dict(src_odd=2), _align("source", 2)),
        (dict(dst_odd=0), _align("destination", 0)),
        (dict(dst_at="src"), _inplace(noun, "source plane 0", 0)),
        # the first refusal in the source wins
        (dict(rows=9, null_p=1), GEOM),
        (dict(lut_depth=7, row0=1), DEPTH7),
        (dict(row0=1, lds=1), UNION),
        (dict(lds=1, src_null=1), lds),
        (dict(src_null=1, src_odd=0), "null plane 1"),
        (dict(dst_null=2, src_odd=0), "null plane 2"),
        (dict(src_odd=0, dst_at="src"), _align("source", 0)),
        (dict(dst_odd=1, dst_at="src"), _align("destination", 1)),
        # an empty call is refused for what comes before the plane checks and writes nothing
        (dict(w=0, no_planes=1), None),
        (dict(rows=0, row0=0, no_planes=1), None),
        (dict(w=0, lds=1), lds),
        (dict(w=0, row0=1, no_planes=1), UNION),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("dither", [0, 2], ids=["none", "blue_noise"])
def test_xsub(loaded, dither):
    """No variant, alignment or overlap rule of its own (it has an LDS-window kernel and is pixelwise per union block)."""
    _run(loaded, _xsub(dither), [
        (dict(dither=9), DITHER),
        (dict(null_p=1), NULLP),
        (dict(null_src=1), NULLARG),
        (dict(interp=7), INTERP),
        (dict(rows=9), GEOM),
        (dict(lut_depth=7), DEPTH7),
        (dict(row0=1), UNION),
        (dict(dither=1, row0=2), ED_ROWS),
        (dict(src_null=1), "null plane 1"),
        (dict(dst_null=1), "null plane 1"),
        (dict(dither=9, null_src=1), DITHER),
        (dict(rows=9, null_p=1), GEOM),
        (dict(lut_depth=7, row0=1), DEPTH7),
        (dict(row0=1, src_null=1), UNION),
        (dict(w=0, no_planes=1), None),
        (dict(w=0, row0=1, no_planes=1), UNION),
    ])


@pytest.mark.gpu
def test_dual(loaded):
    noun = "the two-output pass"
    _run(loaded, _dual, _union_cases(noun, "two outputs") + [
        (dict(null_dst2=1), NULLARG),
        (dict(fmt_out2=_native.fmt_code(10, 0, 1)),
         "bad fmt_out2 0x20a: the second output is planar 4:2:0 / 4:2:2 / 4:4:4 at a depth of 8 to 16 bit"),
        (dict(dst2_null=1), "null plane 1"),
        (dict(dst2_odd=0), _align("second destination", 0)),
        (dict(dst2_at="src"), _inplace(noun, "source plane 0", 0) + " (the second destination)"),
        (dict(dst2_at="dst"), "the two destinations overlap: their byte ranges over all rows and frames must be disjoint"),
        (dict(null_dst2=1, null_p=1), NULLARG),
        (dict(dst_null=1, dst2_null=2), "null plane 1"),
        (dict(dst2_null=2, src_odd=0), "null plane 2"),
        (dict(dst_odd=0, dst2_odd=1), _align("destination", 0)),
        (dict(dst2_odd=1, dst_at="src"), _align("second destination", 1)),
        (dict(dst_at="src", dst2_at="src"), _inplace(noun, "source plane 0", 0)),
        (dict(dst2_at="src", dst_odd=0), _align("destination", 0)),
    ])


@pytest.mark.gpu
def test_chain(loaded):
    second = "unknown interpolation mode 7 for the second LUT"
    _run(loaded, _chain, _union_cases("the two-LUT pass", "two LUTs in one pass") + [
        (dict(interp2=7), second),
        (dict(interp2=7, null_p=1), second),
        (dict(interp=7, interp2=7), INTERP),
        # the entry has no lut_depth check of its own: the constants refuse a depth outside 8..16 for it
        (dict(lut_depth=17), "unsupported bit depth (in 10, lut 17, out 10)"),
    ])


@pytest.mark.gpu
def test_cdl(loaded):
    _run(loaded, _cdl, _union_cases("the CDL pass", "the CDL pass") + [
        (dict(null_cdl=1), "null CDL"),
        (dict(null_cdl=1, null_p=1), "null CDL"),
        (dict(rows=9, null_cdl=1), GEOM),
    ])


@pytest.mark.gpu
def test_lut1d(loaded):
    _run(loaded, _lut1d, _union_cases("the lut1d pass", "the lut1d pass") + [
        (dict(interp=-2), "unknown interpolation mode -2"),
    ])


STACK_INTERP = "stack: unknown interpolation mode 7 on stage 0 (lut3d)"
TWICE = "stack: stage kind lut3d is listed twice; each kind may appear once"
STACK_CASES = [
    (dict(stages=[]), "stack: 0 stages; a stack has 1 to 4"),
    (dict(stages=[(1, 2), (1, 2)]), TWICE),
    (dict(cdl=1), "stack: a CDL is given and no cdl stage is listed"),
    (dict(stages=[(4, 0), (1, 2)]), "stack: a cdl stage is listed and the CDL is null"),
    (dict(stages=[(1, 2), (1, 2)], rows=9), TWICE),
    (dict(stages=[(1, 2), (1, 2)], null_src=1), NULLARG),
    (dict(cdl=1, null_p=1), "stack: a CDL is given and no cdl stage is listed"),
]
STRENGTH_CASES = [
    (dict(strength=1.5), "stack: strength 1.5 outside [0, 1]"),
    (dict(strength=-0.25), "stack: strength -0.25 outside [0, 1]"),
    (dict(strength=float("nan")), "stack: strength nan outside [0, 1]"),
    (dict(strength=1.5, null_src=1), "stack: strength 1.5 outside [0, 1]"),
    (dict(strength=1.5, stages=[]), "stack: strength 1.5 outside [0, 1]"),
]


def _stack_union():
    return _union_cases("the stack pass", "the stack pass", interp=STACK_INTERP)


@pytest.mark.gpu
def test_stack(loaded):
    _run(loaded, _stack, _stack_union() + STACK_CASES)


@pytest.mark.gpu
def test_stack_mix(loaded):
    _run(loaded, _stack_mix, _stack_union() + STACK_CASES + STRENGTH_CASES)


@pytest.mark.gpu
def test_stack_matte(loaded):
    short = "stack: matte stride 16 is shorter than a row of 16 samples of 2 byte(s)"
    _run(loaded, _stack_matte, _stack_union() + STACK_CASES + STRENGTH_CASES + [
        (dict(null_matte=1), "stack: null matte"),
        (dict(matte_depth=7), "stack: matte depth 7 outside 8..16"),
        (dict(matte_invert=2), "stack: matte invert 2 is neither 0 nor 1"),
        (dict(matte_stride=16), short),
        (dict(matte_odd=1), "stack: a matte of 10 bits is held in 16-bit words: base, stride and frame stride must be even"),
        (dict(matte_at_dst=1), "stack: the byte range of the matte overlaps that of destination plane 0"),
        (dict(strength=1.5, matte_depth=7), "stack: strength 1.5 outside [0, 1]"),
        (dict(matte_depth=7, stages=[(1, 2), (1, 2)]), "stack: matte depth 7 outside 8..16"),
        (dict(lds=1, matte_stride=16), _lds("the stack pass")),
        (dict(dst_at="src", matte_stride=16), _inplace("the stack pass", "source plane 0", 0)),
        (dict(matte_stride=16, matte_at_dst=1), short),
        (dict(w=0, no_planes=1, matte_stride=16), None),
    ])


@pytest.mark.gpu
def test_premul(loaded):
    kind = ("premultiplied alpha: the alpha source must be an integer plane (kind 1), got kind 2 -- premultiplied alpha is defined "
            "only for a source that carries alpha")
    _run(loaded, _premul, _union_cases("the premultiplied-alpha pass", "premultiplied alpha") + [
        (dict(null_alpha=1), "null alpha source"),
        (dict(range=1, lut_depth=12), "premultiplied alpha: a call with a prologue (range_src != range_in, or lut_depth 12 other than "
                                      "the source's depth 10) has no alpha to carry"),
        (dict(lut_depth=12), "a range/depth prologue is only defined for full-range (pc) sources"),
        (dict(alpha_kind=_native.ALPHA_FLOAT), kind),
        (dict(alpha_null=1), "premultiplied alpha: null alpha source plane"),
        (dict(alpha_at_dst=1), _inplace("the premultiplied-alpha pass", "source plane 3", 0)),
        (dict(null_p=1, null_alpha=1), NULLP),
        (dict(alpha_kind=_native.ALPHA_FLOAT, row0=1), kind),
        (dict(alpha_null=1, lds=1), "premultiplied alpha: null alpha source plane"),
        (dict(w=0, alpha_null=1), "premultiplied alpha: null alpha source plane"),
    ])


# ------------------------------------------------------------------ one layout on both sides
@pytest.mark.gpu
def test_yuv(loaded):
    """(vec_lds and unaligned planes are not refused here: the entry has an LDS-window kernel, and its generic kernel takes any
    address.)"""
    _run(loaded, _yuv, [
        (dict(null_p=1), NULLP),
        (dict(null_src=1), NULLARG),
        (dict(null_dst=1), NULLARG),
        (dict(interp=7), INTERP),
        (dict(rows=9), GEOM),
        (dict(lut_depth=7), DEPTH7),
        (dict(fmt_out=F422), "fmt_in and fmt_out must share chroma subsampling"),
        (dict(row0=1), BLOCK),
        (dict(src_null=1), "null plane 1"),
        (dict(dst_null=1), "null plane 1"),
        (dict(null_src=1, null_p=1), NULLARG),
        (dict(lut_depth=7, row0=1), DEPTH7),
        (dict(row0=1, dst_null=1), BLOCK),
        (dict(w=0, no_planes=1), None),
    ])


@pytest.mark.gpu
def test_sited(loaded):
    loc = "unknown chroma location 9"
    _run(loaded, _sited, [
        (dict(loc=9), loc),
        (dict(null_p=1), NULLP),
        (dict(null_src=1), NULLARG),
        (dict(interp=7), INTERP),
        (dict(rows=9), GEOM),
        (dict(lut_depth=7), DEPTH7),
        (dict(row0=1), BLOCK),
        (dict(src_null=1), "null plane 1"),
        (dict(dst_null=1), "null plane 1"),
        (dict(dst_at="src"), _inplace("sited chroma resampling", "source plane 0", 0)),
        (dict(loc=9, null_src=1), loc),
        (dict(lut_depth=7, row0=1), DEPTH7),
        (dict(row0=1, src_null=1), BLOCK),
        (dict(src_null=1, dst_at="src"), "null plane 1"),
        (dict(w=0, no_planes=1), None),
    ])


# ------------------------------------------------------------------ containers
@pytest.mark.gpu
def test_semi(loaded):
    shift = "source layout: shift is 6 (16 - depth) or 0 at 10 bit, not 3"
    _run(loaded, _semi, [
        (dict(null_p=1), "null yuv params or layout"),
        (dict(null_src=1), NULLARG),
        (dict(interp=7), INTERP),
        (dict(rows=9), GEOM),
        (dict(lut_depth=7), DEPTH7),
        (dict({"in": (2, 0, 6)}), "source layout: semi and swap are 0 or 1 (got 2, 0)"),
        (dict({"in": (0, 1, 0)}), "source layout: swap needs a semi-planar side"),
        (dict({"in": (1, 0, 3)}), shift),
        (dict(out=(1, 0, 3)), "destination layout: shift is 6 (16 - depth) or 0 at 10 bit, not 3"),
        (dict(fmt_in=F444, fmt_out=F444), "source layout: semi-planar frames are 4:2:0 or 4:2:2"),
        (dict(src_null=1), "null source plane 1"),
        (dict(dst_null=1), "null destination plane 1"),
        (dict(src_odd=0), _calign("source", 0)),
        (dict(dst_odd=1), _calign("destination", 1)),
        (dict(row0=1), BLOCK),
        (dict({"in": (1, 0, 3)}, lut_depth=7), DEPTH7),
        (dict({"in": (1, 0, 3)}, src_null=0), shift),
        (dict(src_odd=0, src_null=1), _calign("source", 0)),
        (dict(src_odd=1, src_null=0), "null source plane 0"),
        (dict(src_odd=1, dst_null=0), _calign("source", 1)),
        (dict(dst_null=1, row0=1), "null destination plane 1"),
        # the planes are looked at before the empty call returns
        (dict(w=0, no_planes=1), "null source plane 0"),
        (dict(w=0), None),
    ])


@pytest.mark.gpu
def test_packed(loaded):
    noun = "a packed 4:2:2 call between different buffers or containers"
    _run(loaded, _packed, [
        (dict(null_p=1), "null yuv params or packing"),
        (dict(null_src=1), NULLARG),
        (dict(interp=7), INTERP),
        (dict(rows=9), GEOM),
        (dict(lut_depth=7), DEPTH7),
        (dict(fmt_in=F420), "the source of a packed call is 4:2:2"),
        (dict(fmt_in=F420, fmt_out=F422, out=(1, 0, 6)),
         "a packed destination takes a 4:2:2 source (no subsampling change into a packed frame)"),
        (dict(fmt_out=_native.fmt_code(10, 0, 1)), "4:4:0 chroma layout is not supported"),
        (dict({"in": (2, 0, 6)}), "source packing: packed is 0 or 1 (got 2)"),
        (dict({"in": (1, 5, 6)}), "source packing: order is 0 (yuyv), 1 (uyvy) or 2 (yvyu), not 5"),
        (dict({"in": (1, 0, 3)}), "source packing: shift is 6 (16 - depth) or 0 at 10 bit, not 3"),
        (dict(out=(0, 1, 0)), "destination packing: a planar side takes order 0 and shift 0"),
        (dict(out=(1, 0, 6)), "destination packing: packed frames are 4:2:2"),
        (dict(src_null=0), "null source plane 0"),
        (dict(dst_null=1), "null destination plane 1"),
        (dict(src_odd=0), _calign("source", 0)),
        (dict(dst_odd=2), _calign("destination", 2)),
        (dict(row0=1), BLOCK),
        (dict(dst_at="src"), _inplace(noun, "source plane 0", 0)),
        # in place means the same container and the same bytes: the same bytes in another group order are an overlap
        (dict(fmt_out=F422, out=(1, 1, 6), dst_at="src"), _inplace(noun, "source plane 0", 0)),
        (dict(lut_depth=7, row0=1), DEPTH7),
        (dict({"in": (1, 0, 3)}, fmt_in=F420), "the source of a packed call is 4:2:2"),
        (dict({"in": (1, 0, 3)}, src_null=0), "source packing: shift is 6 (16 - depth) or 0 at 10 bit, not 3"),
        (dict(src_odd=0, dst_null=0), _calign("source", 0)),
        (dict(dst_null=1, row0=1), "null destination plane 1"),
        (dict(row0=1, dst_at="src"), BLOCK),
        (dict(w=0, no_planes=1), "null source plane 0"),
        (dict(w=0), None),
    ])


@pytest.mark.gpu
def test_v210(loaded):
    noun = "a v210 call between different buffers or containers"
    stride = "source: a v210 row of 16 samples takes 48 bytes, the stride is 32"
    _run(loaded, _v210, [
        (dict(null_p=1), NULLP),
        (dict(null_src=1), NULLARG),
        (dict(interp=7), INTERP),
        (dict(rows=9), GEOM),
        (dict({"in": 2}), "in_v210 and out_v210 are 0 or 1 (got 2, 0)"),
        (dict({"in": 0}), "neither side is v210: planar frames on both sides are lutr_apply_yuv / lutr_apply_yuv_xsub"),
        (dict(fmt_in=F420), "source: a v210 frame is 10-bit 4:2:2 (format 0x30a)"),
        (dict(src_null=0), "null source plane 0"),
        (dict(src_odd=0), "source: v210 rows are 32-bit words: base, stride and frame stride must be 4-byte aligned"),
        (dict(src_stride=32), stride),
        (dict(src_stride=-32), "source: a v210 row of 16 samples takes 48 bytes, the stride is -32"),
        (dict(out=1), "destination: a v210 frame is 10-bit 4:2:2 (format 0x30a)"),
        (dict(dst_null=1), "null destination plane 1"),
        (dict(dst_odd=0), _calign("destination", 0)),
        (dict(lut_depth=7), DEPTH7),
        (dict(fmt_out=_native.fmt_code(7, 1, 1)), "unsupported bit depth (in 10, lut 10, out 7)"),
        (dict(row0=1), BLOCK),
        (dict(dst_at="src"), _inplace(noun, "source plane 0", 0)),
        # the container's refusal comes before the constants'
        (dict(src_stride=32, fmt_out=_native.fmt_code(7, 1, 1)), stride),
        (dict(src_stride=32, lut_depth=7), stride),
        (dict(dst_null=1, lut_depth=7), "null destination plane 1"),
        (dict(null_p=1, **{"in": 2}), NULLP),
        (dict(src_null=0, src_stride=32), "null source plane 0"),
        (dict(lut_depth=7, row0=1), DEPTH7),
        (dict(row0=1, dst_at="src"), BLOCK),
        (dict(w=0, no_planes=1), "null source plane 0"),
        (dict(w=0), None),
    ])


# ------------------------------------------------------------------ RGB on one side
@pytest.mark.gpu
def test_rgb_to_yuv_planar(loaded):
    depth = "unsupported bit depth (in 7, lut 7, out 10)"
    over = _inplace("RGB -> YUV", "the source", 0)
    _run(loaded, _rgb2yuv, [
        (dict(dither=9), DITHER),
        (dict(null_p=1), NULLP),
        (dict(null_src=1), NULLARG),
        (dict(null_dst=1), NULLARG),
        (dict(interp=7), INTERP),
        (dict(rows=9), GEOM),
        (dict(lut_depth=7), depth),
        (dict(dither=1, row0=2), ED_ROWS),
        (dict(row0=1), OBLOCK),
        (dict(src_null=1), "null plane 1"),             # the gbrp plane's own number, whatever the R, G, B order of the streams
        (dict(src_null=2), "null plane 2"),
        (dict(dst_null=1), "null plane 1"),
        (dict(dst_at="src"), over),
        (dict(dither=9, null_src=1), DITHER),
        (dict(lut_depth=7, row0=1), depth),
        (dict(row0=1, src_null=1), OBLOCK),
        (dict(src_null=0, dst_null=1), "null plane 0"),
        (dict(dst_null=2, dst_at="src"), "null plane 2"),
        (dict(w=0, no_planes=1), None),
    ])


@pytest.mark.gpu
def test_rgb_to_yuv_packed(loaded):
    bits = "lut_depth 10 must be the packed source's depth 16"
    bad = _native.packed_code(12, 3, 0, 1, 2)
    _run(loaded, _rgb2yuv_packed, [
        (dict(null_p=1), NULLP),
        (dict(null_src=1), NULLARG),
        (dict(interp=7), INTERP),
        (dict(rows=9), GEOM),
        (dict(kind=bad), f"unsupported packed format 0x{bad:x}"),
        (dict(lut_depth=10), bits),
        (dict(row0=1), OBLOCK),
        (dict(img_null=1), "null image"),
        (dict(img_odd=1), IMG_ALIGN),
        (dict(dst_null=1), "null plane 1"),
        (dict(dst_at="src"), _inplace("RGB -> YUV", "the source", 0)),
        (dict(lut_depth=10, row0=1), bits),
        (dict(row0=1, img_null=1), OBLOCK),
        (dict(img_null=1, dst_null=1), "null image"),
        (dict(img_odd=1, dst_null=1), IMG_ALIGN),
        (dict(w=0, no_planes=1), None),
    ])


@pytest.mark.gpu
def test_yuv_to_rgb_planar(loaded):
    depth = "unsupported bit depth (in 7, lut 7, out 7)"
    _run(loaded, _yuv2rgb, [
        (dict(null_p=1), NULLP),
        (dict(null_src=1), NULLARG),
        (dict(null_dst=1), NULLARG),
        (dict(interp=7), INTERP),
        (dict(rows=9), GEOM),
        (dict(lut_depth=7), depth),
        (dict(row0=1), BLOCK),
        (dict(src_null=1), "null plane 1"),
        (dict(dst_null=1), "null plane 1"),             # the gbrp plane's own number
        (dict(dst_null=2), "null plane 2"),
        (dict(dst_at="src"), _inplace("YUV -> RGB", "source plane 0", 1)),      # gbrp plane 0 is G, stream 1 of R, G, B
        (dict(lut_depth=7, row0=1), depth),
        (dict(row0=1, src_null=1), BLOCK),
        (dict(src_null=1, dst_null=2), "null plane 1"),
        (dict(dst_null=1, dst_at="src"), "null plane 1"),
        (dict(w=0, no_planes=1), None),
    ])


@pytest.mark.gpu
def test_yuv_to_rgb_packed(loaded):
    bits = "lut_depth 10 must be the packed destination's depth 16"
    bad = _native.packed_code(16, 3, 0, 0, 2)
    _run(loaded, _yuv2rgb_packed, [
        (dict(null_p=1), NULLP),
        (dict(null_dst=1), NULLARG),
        (dict(interp=7), INTERP),
        (dict(rows=9), GEOM),
        (dict(kind=bad), f"unsupported packed format 0x{bad:x}"),
        (dict(lut_depth=10), bits),
        (dict(row0=1), BLOCK),
        (dict(src_null=1), "null plane 1"),
        (dict(img_null=1), "null image"),
        (dict(img_odd=1), IMG_ALIGN),
        (dict(img_at=1), _inplace("YUV -> RGB", "source plane 0", 0)),
        (dict(lut_depth=10, row0=1), bits),
        (dict(row0=1, img_null=1), BLOCK),
        (dict(src_null=1, img_null=1), "null plane 1"),
        (dict(img_odd=1, img_at=1), IMG_ALIGN),
        (dict(w=0, no_planes=1), None),
    ])
