"""The stage stack on semi-planar sides (lutr_apply_yuv_stack_semi) on the GPU: for every call the entry accepts,

    apply_yuv_stack_semi(src in container A -> dst in container B) == to_semi(apply_yuv_stack(to_planar(src, A)), B)

bit for bit on whole planes.  The expected planes are tests/_stack_twin.py's composition on the planar samples, fed the product's
own host tables as tests/test_gpu_stack.py does, then put into the destination's container with `semiplanar.to_semi`.
"""
import ctypes as C
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from lut_renderer_amd import _native, semiplanar
from lut_renderer_amd.formats import parse_stages, yuv_side
from tests import _gpu_stack_semi_worker as worker
from tests.test_gpu_stack import (GOLDEN, H, LAYOUTS, NF, ROOT, W, _desc, _dev, _eq, _fmt, _host, _lds, _list, _src, _variant,  # noqa: F401
                                  _vec_name, _want, grade, l1ds, loaded, luts)

GENERIC = "k_yuv_stack_semi_generic"
LAY = {v: k for k, v in LAYOUTS.items()}
CHILD_LIMIT_S = 120


def _side(name):
    """(the side, its layout key "420" | "422" | "444", whether it is semi-planar)"""
    s = yuv_side(name)
    return s, LAY[(s.csx, s.csy)], s.nplanes == 2


def _held(planar, name):
    """planar samples in the container `name`"""
    return semiplanar.to_semi(planar, name) if _side(name)[2] else list(planar)


def _semi_name(a, b, stages, lds=None):
    """The vector kernel's name for source `a` and destination `b` as `last_kernel` spells it."""
    fa, fb = yuv_side(a), yuv_side(b)
    lds = _lds(stages, fa.depth) if lds is None else lds
    tri = int(any(m == "trilinear" for _, m in parse_stages(stages)))
    return (f"k_yuv_stack_semi_vec<{int(fa.depth > 8)},{int(fb.depth > 8)},{fa.csx},{fa.csy},{fb.csx},{fb.csy},{tri},{int(lds)}>"
            + _list(stages))


def _expect(res, a, b, stages, cdl, planar, key, dl=None, **kw):
    """the twin's planes for the planar samples of a source `a`, in the container of `b`"""
    fa, la, _ = _side(a)
    fb, lb, _ = _side(b)
    return _held(_want(res, stages, cdl, fa.depth, dl or fa.depth, fb.depth, la, lb, planar, key, **kw), b)


def _run(eng, a, b, stages, cdl, planar, **kw):
    fb = yuv_side(b)
    got = eng.apply_yuv_stack_semi(_dev(_held(planar, a), eng.device), pix_fmt=a, out_pix_fmt=b, stages=stages, cdl=cdl, **kw)
    return _host(got, fb.depth)


# ------------------------------------------------------------------ 1. every semi-planar name onto itself
@pytest.mark.gpu
@pytest.mark.parametrize("stages", ["lut1d,cdl,lut3d", "lut3d,cdl,lut3d2"])
@pytest.mark.parametrize("name", list(_native.SEMI_FORMATS))
def test_every_name_onto_itself(loaded, grade, name, stages):
    """Uniform content through nearest / trilinear / tetrahedral on the vector kernel (named exactly) and all five modes on the
    generic one; natural content through tetrahedral on both.  The twin has pyramid / prism on lattices that are fed codes: in
    `lut3d,cdl,lut3d2` the first lattice takes the five modes and the one behind the CDL stays tetrahedral for those two; in
    `lut1d,cdl,lut3d`, whose only lattice is behind the CDL, pyramid / prism are checked against the planar stack's own bits."""
    fmt, lay, _ = _side(name)
    kinds = stages.split(",")
    behind_cdl = {k for i, k in enumerate(kinds) if i and kinds[i - 1] == "cdl"}

    def with_mode(m):
        # (the twin feeds pyramid / prism codes: behind the CDL it has the three vector modes, so a lattice there beside one that
        # is fed codes keeps tetrahedral)
        keep = behind_cdl if m in ("pyramid", "prism") and any(k.startswith("lut3d") and k not in behind_cdl for k in kinds) else set()
        return ",".join(f"{k}:{'tetrahedral' if k in keep else m}" if k.startswith("lut3d") else k for k in kinds)

    def expected(st, m, planar, dist):
        if m in ("pyramid", "prism") and any(k.startswith("lut3d") and k in behind_cdl and f"{k}:{m}" in st for k in kinds):
            # the only lattice of the list is fed unit floats: the contract's own right-hand side, the planar stack on the same samples
            own = loaded.apply_yuv_stack(_dev(planar, loaded.device), pix_fmt=_fmt(fmt.depth, lay), stages=st, cdl=grade)
            assert loaded.last_kernel == "k_yuv_stack_generic" + _list(st), loaded.last_kernel
            return _held(_host(own, fmt.depth), name)
        return _expect(loaded._res, name, name, st, grade, planar, ("semi", dist))

    for dist, variant, modes in (("uniform", "auto", ("nearest", "trilinear", "tetrahedral")), ("natural", "auto", ("tetrahedral",)),
                                 ("uniform", "generic", ("nearest", "trilinear", "tetrahedral", "pyramid", "prism")),
                                 ("natural", "generic", ("tetrahedral",))):
        planar = _src(dist, W, H, fmt.depth, lay, nf=NF)
        for m in modes:
            st = with_mode(m)
            with _variant(loaded, variant):
                got = _run(loaded, name, name, st, grade, planar)
                want_name = _semi_name(name, name, st) if variant == "auto" else GENERIC + _list(st)
                assert loaded.last_kernel == want_name, loaded.last_kernel
            assert _eq(got, expected(st, m, planar, dist)), (name, st, dist, variant)


# ------------------------------------------------------------------ 2. container and layout mixes
PAIRS = [("nv12", "yuv420p"), ("yuv420p", "nv12"), ("nv21", "nv12"), ("p010le", "nv12"), ("p010le", "yuv422p10le"),
         ("yuv444p10le", "p010le"), ("nv16", "nv12"), ("nv12", "nv16"), ("p210le", "yuv444p10le"), ("yuv420p10le", "p216le"),
         ("nv12", "p010le")]


@pytest.mark.gpu
@pytest.mark.parametrize("a,b", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_container_and_layout_mixes(loaded, grade, a, b):
    """Each pair against the twin and against the engine's own apply_yuv_stack on the de-interleaved samples; 8 -> 16 bit has a
    generic kernel only."""
    stages = "lut1d,cdl,lut3d"
    fa, la, _ = _side(a)
    fb, lb, _ = _side(b)
    planar = _src("natural", W, H, fa.depth, la, k=2, nf=NF)
    got = _run(loaded, a, b, stages, grade, planar)
    if fa.depth <= 8 and fb.depth > 8:
        assert loaded.last_kernel == GENERIC + _list(stages), loaded.last_kernel
    else:
        assert loaded.last_kernel == _semi_name(a, b, stages), loaded.last_kernel
    assert _eq(got, _expect(loaded._res, a, b, stages, grade, planar, "mix")), (a, b)
    own = loaded.apply_yuv_stack(_dev(planar, loaded.device), pix_fmt=_fmt(fa.depth, la), out_pix_fmt=_fmt(fb.depth, lb), stages=stages,
                                 cdl=grade)
    assert loaded.last_kernel.startswith("k_yuv_stack_"), loaded.last_kernel
    assert _eq(got, _held(_host(own, fb.depth), b)), (a, b, "differs from apply_yuv_stack on the planar samples")


# ------------------------------------------------------------------ 3. tied to k_yuv_semi_vec
@pytest.mark.gpu
@pytest.mark.parametrize("a,b", [("nv12", "nv12"), ("p010le", "p010le"), ("p210le", "yuv422p10le"), ("yuv420p", "nv21"), ("p010le", "nv12")])
def test_one_lattice_gives_the_bits_of_apply_yuv(loaded, a, b):
    fa, la, _ = _side(a)
    fb = yuv_side(b)
    held = _dev(_held(_src("natural", W, H, fa.depth, la, k=3, nf=NF), a), loaded.device)
    got = _host(loaded.apply_yuv_stack_semi(held, pix_fmt=a, out_pix_fmt=b, stages=("lut3d",)), fb.depth)
    assert loaded.last_kernel.startswith("k_yuv_stack_semi_vec<"), loaded.last_kernel
    ref = _host(loaded.apply_yuv(held, pix_fmt=a, out_pix_fmt=b, interp="tetrahedral"), fb.depth)
    assert loaded.last_kernel.startswith("k_yuv_semi_vec<"), loaded.last_kernel
    assert _eq(got, ref), (a, b)


# ------------------------------------------------------------------ 4. low bits
@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "generic"])
def test_low_bits_are_ignored_on_input_and_zero_on_output(loaded, grade, variant):
    stages = "lut1d,cdl,lut3d"
    rng = np.random.default_rng(11)
    with _variant(loaded, variant):
        for a, b in (("p010le", "p010le"), ("p210le", "p010le"), ("p010le", "yuv420p10le")):
            fa, la, _ = _side(a)
            planar = _src("natural", W, H, 10, la, k=4, nf=NF)
            clean = _held(planar, a)
            dirty = [p | rng.integers(0, 64, size=p.shape).astype(np.uint16) for p in clean]
            assert any((d != c).any() for d, c in zip(dirty, clean))
            got = _host(loaded.apply_yuv_stack_semi(_dev(dirty, loaded.device), pix_fmt=a, out_pix_fmt=b, stages=stages, cdl=grade), 10)
            assert _eq(got, _expect(loaded._res, a, b, stages, grade, planar, "low")), (a, b, variant)
            if _side(b)[2]:
                assert all(((p & 63) == 0).all() for p in got), (a, b, "low bits set on output")
        # shift 0 on a 16-bit container reads whole words: p016le codes with every bit in use
        planar = _src("natural", W, H, 16, "420", k=4, nf=NF)
        assert (planar[0] & 63).any()
        got = _run(loaded, "p016le", "p016le", stages, grade, planar)
        assert _eq(got, _expect(loaded._res, "p016le", "p016le", stages, grade, planar, "low16")), variant


# ------------------------------------------------------------------ 5. sizes and strides
def _padded(eng, planes, pad, fill):
    """device copies of `planes` ([rows, cols]) in rows of `pad` samples plus one spare row, filled with `fill`; returns (the
    storage, the views the call takes)"""
    import torch
    store, views = [], []
    for p in planes:
        dt = torch.uint8 if p.dtype == np.uint8 else torch.int16
        t = torch.full((p.shape[0] + 1, pad), fill, dtype=dt, device=eng.device)
        t[:p.shape[0], :p.shape[1]] = _dev([p], eng.device)[0]
        store.append(t)
        views.append(t[:p.shape[0], :p.shape[1]])
    return store, views


@pytest.mark.gpu
def test_ragged_width_on_padded_rows_and_untouched_padding(loaded, grade):
    """Width 138 on padded rows: the vector kernel up to column 136, the generic kernel for the last pair; the padding of every
    row and a spare row keep their sentinel."""
    import torch
    stages = "lut1d,cdl,lut3d"
    for a, b, fill in (("nv12", "nv12", 0x5a), ("p010le", "yuv422p10le", 0x5a5a), ("yuv444p10le", "p010le", 0x5a5a)):
        fa, la, _ = _side(a)
        fb, lb, _ = _side(b)
        w, h = 138, 36
        planar = _src("natural", w, h, fa.depth, la, k=6)
        _, src_v = _padded(loaded, _held(planar, a), 160, 0)
        want = _expect(loaded._res, a, b, stages, grade, planar, ("ragged", w, h))
        store, dst_v = _padded(loaded, [np.zeros_like(p) for p in want], 160, fill)
        for t, v in zip(store, dst_v):
            v.fill_(fill)
        loaded.apply_yuv_stack_semi(src_v, dst_v, pix_fmt=a, out_pix_fmt=b, stages=stages, cdl=grade)
        vec = _semi_name(a, b, stages)
        assert loaded.last_kernel == vec.replace("[", "+" + GENERIC + "[", 1), loaded.last_kernel
        assert _eq(_host(dst_v, fb.depth), want), (a, b)
        for t, p in zip(store, want):
            assert (t[:, p.shape[1]:] == fill).all() and (t[p.shape[0]:] == fill).all(), (a, b, "wrote outside the planes")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("a,b", [("nv12", "nv12"), ("p010le", "p010le"), ("nv16", "nv12"), ("p010le", "yuv444p10le"), ("yuv444p", "nv21")])
def test_odd_sizes_on_the_generic_kernel(loaded, grade, a, b):
    """137 x 35: edge replication, and the second element of the last pair."""
    stages = "lut1d,cdl,lut3d"
    fa, la, _ = _side(a)
    planar = _src("natural", 137, 35, fa.depth, la, k=7)
    got = _run(loaded, a, b, stages, grade, planar)
    assert loaded.last_kernel == GENERIC + _list(stages), loaded.last_kernel
    assert _eq(got, _expect(loaded._res, a, b, stages, grade, planar, ("odd", 137, 35))), (a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["auto", "generic"])
def test_row_blocks_write_their_rows_of_both_planes_only(loaded, grade, variant):
    import torch
    stages = "lut3d,cdl,lut3d2"
    a, b = "p010le", "p010le"
    planar = _src("uniform", W, H, 10, "420", nf=NF)
    dev = _dev(_held(planar, a), loaded.device)
    whole = _expect(loaded._res, a, b, stages, grade, planar, "rows")
    names = dict(pix_fmt=a, out_pix_fmt=b, stages=stages, cdl=grade)
    with _variant(loaded, variant):
        out = [torch.full(p.shape, 0x5a5a, dtype=torch.int16, device=loaded.device) for p in whole]
        loaded.apply_yuv_stack_semi(dev, out, row0=10, rows=14, **names)
        got = _host(out, 10)
        for i, (g, wh) in enumerate(zip(got, whole)):
            r0, r1 = (10, 24) if i == 0 else (5, 12)
            assert np.array_equal(g[:, r0:r1], wh[:, r0:r1]), (variant, i)
            assert (g[:, :r0] == 0x5a5a).all() and (g[:, r1:] == 0x5a5a).all(), (variant, i, "wrote outside the block")
        loaded.apply_yuv_stack_semi(dev, out, row0=0, rows=10, **names)
        loaded.apply_yuv_stack_semi(dev, out, row0=24, rows=H - 24, **names)
        assert _eq(_host(out, 10), whole), variant
        with pytest.raises(_native.LutrError, match="union") as e:
            loaded.apply_yuv_stack_semi(dev, out, row0=1, rows=H - 1, **names)
        assert e.value.code == _native.EINVAL


@pytest.mark.gpu
def test_a_misaligned_pair_plane(loaded, grade):
    """A pair plane at base + 4 bytes, 16 -> 16 bit (the vector kernel moves 8 bytes of it per access): the generic kernel under
    auto, LUTR_EINVAL under vec_global."""
    import torch
    stages = "lut1d,cdl,lut3d"
    a = "p010le"
    planar = _src("natural", W, H, 10, "420", k=8)
    y, pairs = _dev(_held(planar, a), loaded.device)
    store = torch.zeros(pairs.numel() + 2, dtype=torch.int16, device=loaded.device)
    off = store[2:].view(pairs.shape)
    off.copy_(pairs)
    assert off.data_ptr() % 8 == 4
    got = _host(loaded.apply_yuv_stack_semi([y, off], pix_fmt=a, out_pix_fmt=a, stages=stages, cdl=grade), 10)
    assert loaded.last_kernel == GENERIC + _list(stages), loaded.last_kernel
    assert _eq(got, _expect(loaded._res, a, a, stages, grade, planar, "misaligned"))
    with _variant(loaded, "vec_global"):
        with pytest.raises(_native.LutrError) as e:
            loaded.apply_yuv_stack_semi([y, off], pix_fmt=a, out_pix_fmt=a, stages=stages, cdl=grade)
        assert e.value.code == _native.EINVAL
        loaded.apply_yuv_stack_semi([y, pairs], pix_fmt=a, out_pix_fmt=a, stages=stages, cdl=grade)
        assert loaded.last_kernel == _semi_name(a, a, stages), loaded.last_kernel


# ------------------------------------------------------------------ 6. the full-range prologue
@pytest.mark.gpu
def test_full_range_prologue(loaded, grade):
    stages = "lut1d,cdl,lut3d"
    planar = _src("natural", W, H, 8, "420", k=6, nf=NF, full_range=True)
    got = _run(loaded, "nv12", "nv12", stages, grade, planar, range_src="pc", range_in="tv", lut_depth=8)
    assert loaded.last_kernel == _semi_name("nv12", "nv12", stages), loaded.last_kernel
    assert _eq(got, _expect(loaded._res, "nv12", "nv12", stages, grade, planar, "pc", dl=8, rin="tv", prologue=True))
    # p010le through the 8-bit LUT depth: the planar stack's own bits on the same samples, in the container
    planar = _src("natural", W, H, 10, "420", k=6, nf=NF, full_range=True)
    kw = dict(range_src="pc", range_in="tv", lut_depth=8)
    got = _run(loaded, "p010le", "p010le", stages, grade, planar, **kw)
    assert loaded.last_kernel == _semi_name("p010le", "p010le", stages, lds=_lds(stages, 8)), loaded.last_kernel
    own = loaded.apply_yuv_stack(_dev(planar, loaded.device), pix_fmt="yuv420p10le", stages=stages, cdl=grade, **kw)
    assert loaded.last_kernel == _vec_name(10, 10, "420", "420", stages, _lds(stages, 8)), loaded.last_kernel
    assert _eq(got, _held(_host(own, 10), "p010le"))


# ------------------------------------------------------------------ 7. table placement and grid-stride trips, in child processes
def _child(tmp, luts, ids, **env_add):
    env = {k: v for k, v in os.environ.items() if k not in ("LUTR_STACK_LDS", "LUTR_MAX_BLOCKS", "LUTR_DEBUG")}
    env.update(env_add)
    t0 = time.monotonic()
    try:
        p = subprocess.run([sys.executable, str(ROOT / "tests" / "_gpu_stack_semi_worker.py"), str(tmp), str(luts["log709_33"][0]),
                            str(GOLDEN / "lut1d" / "gamma1024.cube"), str(GOLDEN / "cdl" / "shot.cc")] + list(ids), env=env, cwd=str(ROOT),
                           capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        pytest.fail(f"the child ({env_add}) did not finish within {CHILD_LIMIT_S} s", pytrace=False)
    if p.returncode != 0:
        pytest.fail(f"the child ({env_add}) ended with {p.returncode} after {time.monotonic() - t0:.1f} s:\n{p.stderr[-3000:]}",
                    pytrace=False)
    debug, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"\[case (\S+)\]", line)
        if m:
            cur = m.group(1)
            debug[cur] = []
        elif cur and line.startswith("[lutr gs] "):
            debug[cur].append(line)
    out = {}
    for cid in ids:
        with np.load(tmp / f"{cid}.npz") as z:
            out[cid] = dict(planes=[z[f"p{i}"] for i in range(len(z.files) - 1)], kernel=str(z["kernel"]), debug=debug.get(cid, []))
    return out


def _child_want(res, grade, cid):
    a, b, w, h, nf = worker.CASES[cid]
    planar, _ = worker.source(a, w, h, nf)
    return _expect(res, a, b, worker.STAGES, grade, planar, ("child", cid))


def _units(cid, kernel):
    """this module's own count of the units of the launch that carries the case's regime"""
    a, b, w, h, nf = worker.CASES[cid]
    fa, fb = yuv_side(a), yuv_side(b)
    csy = max(fa.csy, fb.csy)
    if kernel.startswith(GENERIC):
        return -(-w // 2) * -(-h // (1 << csy)) * nf
    pxt = 8 if fa.depth > 8 and fb.depth == 8 else (4 if fa.depth > 8 else 8)
    return (w // pxt) * (h >> csy) * nf


@pytest.mark.gpu
def test_tables_in_global_memory_and_capped_grids_give_the_same_bits(loaded, luts, grade, tmp_path):
    """Two fresh children, one after the other, each under its own time limit; the second starts only if the first exited 0.
    LUTR_STACK_LDS=0: the tables read from global memory.  LUTR_MAX_BLOCKS=2 on six frames: every thread makes three trips or
    more, the last partial, consecutive trips in different frames; the `[lutr gs]` line is checked against the unit formula."""
    ids = list(worker.CASES)
    (tmp_path / "lds").mkdir()
    (tmp_path / "cap").mkdir()
    res = _child(tmp_path / "lds", luts, ids[:4], LUTR_STACK_LDS="0")
    for cid in ids[:4]:
        a, b = worker.CASES[cid][:2]
        assert res[cid]["kernel"] == _semi_name(a, b, worker.STAGES, lds=False), res[cid]["kernel"]
        got = [p.view(np.uint16) if p.dtype == np.int16 else p for p in res[cid]["planes"]]
        assert _eq(got, _child_want(loaded._res, grade, cid)), (cid, "LUTR_STACK_LDS=0")
    res = _child(tmp_path / "cap", luts, ids, LUTR_MAX_BLOCKS="2", LUTR_DEBUG="1")
    for cid in ids:
        a, b, w, h, nf = worker.CASES[cid]
        kernel = res[cid]["kernel"]
        small = cid.endswith("_small")
        assert kernel == (GENERIC + _list(worker.STAGES) if small else _semi_name(a, b, worker.STAGES)), kernel
        family = GENERIC if small else "k_yuv_stack_semi_vec"
        lines = [re.fullmatch(r"\[lutr gs\] (\S+) units (\d+) blocks (\d+)", ln) for ln in res[cid]["debug"]]
        mine = [m for m in lines if m and m.group(1) == family]
        assert len(mine) == 1, res[cid]["debug"]
        units, blocks = int(mine[0].group(2)), int(mine[0].group(3))
        assert units == _units(cid, kernel) and blocks == 2, (cid, units, blocks)
        assert -(-units // 512) >= 3 and units % 512 != 0 and (units // nf) % 512 != 0, (cid, units)
        got = [p.view(np.uint16) if p.dtype == np.int16 else p for p in res[cid]["planes"]]
        assert _eq(got, _child_want(loaded._res, grade, cid)), (cid, "LUTR_MAX_BLOCKS=2")


# ------------------------------------------------------------------ 8. the ABI's refusals
def _abi(engine, stages, cdl, fmt_in, fmt_out, lin, lout, w, h, s, d):
    """lutr_apply_yuv_stack_semi with raw (kind, interp) pairs and raw layouts (None: a null pointer); returns (rc, message)."""
    p = _native.YuvParams(fmt_in, fmt_out, 10, 0, 0, 0, 0, 0)
    arr = (_native.StageStruct * max(len(stages), 1))()
    for i, (kind, interp) in enumerate(stages):
        arr[i].kind, arr[i].interp = kind, interp
    k = None if cdl is None else C.byref(_native.cdl_struct(cdl))
    li = None if lin is None else C.byref(_native.YuvLayout(*lin))
    lo = None if lout is None else C.byref(_native.YuvLayout(*lout))
    with engine._lock:
        engine._bind_stream()
        rc = engine._lib.lutr_apply_yuv_stack_semi(engine._ctx, C.byref(p), arr, len(stages), k, li, lo, w, h, 1, C.byref(s), C.byref(d), 0, h)
    return rc, engine._lib.lutr_last_error().decode()


@pytest.mark.gpu
def test_refusals_at_the_abi_leave_the_destination_untouched(loaded, grade):
    import torch
    w, h = 64, 8
    planar = _src("natural", w, h, 10, "420")
    dev = _dev(_held(planar, "p010le"), loaded.device)
    out = [torch.full_like(t, 0x5a5a) for t in dev]
    s, d = _desc(dev), _desc(out)
    f420, f444 = _native.fmt_code(10, 1, 1), _native.fmt_code(10, 0, 0)
    semi = (1, 0, 6)
    L3, L1, CD, MX = 1, 3, 4, 5
    ok = [(L3, 2)]
    for args, message in (
            ((ok, None, f420, f420, None, semi), "stack: null layout"),
            ((ok, None, f420, f420, semi, None), "stack: null layout"),
            ((ok, None, f420, f420, (0, 1, 6), semi), "source layout: swap needs a semi-planar side"),
            ((ok, None, f420, f420, semi, (1, 0, 4)), "destination layout: shift is 6 (16 - depth) or 0 at 10 bit, not 4"),
            ((ok, None, f444, f420, semi, semi), "source layout: semi-planar frames are 4:2:0 or 4:2:2"),
            (([(MX, 0), (L3, 2)], None, f420, f420, semi, semi),
             "stack: stage 0 is a matrix stage; a matrix is lutr_apply_yuv_stack_matrix's, and a strength or a matte together with a "
             "matrix is not supported")):
        rc, msg = _abi(loaded, *args, w, h, s, d)
        assert rc == _native.EINVAL and msg == message, (args, msg)
    with _variant(loaded, "vec_lds"):
        rc, msg = _abi(loaded, ok, None, f420, f420, semi, semi, w, h, s, d)
        assert rc == _native.EINVAL and msg == "variant vec_lds: there is no LDS-window kernel for the stack pass", msg
    # the source's pair plane inside the destination's pair plane; then inside destination plane 0
    rc, msg = _abi(loaded, ok, None, f420, f420, semi, semi, w, h, s, _desc([out[0], dev[1]]))
    assert rc == _native.EINVAL and msg.startswith("the stack pass cannot run in place: the byte range of source plane 1 overlaps that "
                                                    "of destination plane 1"), msg
    # the last pair of a row: a plane of pairs spans 2 * ceil(w / 2) samples, so a plane that begins inside that pair overlaps
    big = torch.zeros(4096, dtype=torch.int16, device=loaded.device)
    pairs = big[:dev[1].numel()].view(dev[1].shape)
    pairs.copy_(dev[1])
    luma = big[pairs.numel() - 1:pairs.numel() - 1 + w * h].view(h, w)
    rc, msg = _abi(loaded, ok, None, f420, f420, semi, semi, w, h, _desc([dev[0], pairs]), _desc([luma, out[1]]))
    assert rc == _native.EINVAL and "source plane 1 overlaps that of destination plane 0" in msg, msg
    with pytest.raises(ValueError, match="stack pass cannot run in place"):
        loaded.apply_yuv_stack_semi(dev, dev, pix_fmt="p010le", stages="lut3d")
    torch.cuda.synchronize()
    assert all((t == 0x5a5a).all() for t in out), "a refused call wrote to a destination"
    # both layouts planar with shift 0: lutr_apply_yuv_stack itself
    pdev = _dev(planar, loaded.device)
    pout = [torch.full_like(t, 0x5a5a) for t in pdev]
    rc, msg = _abi(loaded, [(L1, 0), (CD, 0), (L3, 2)], grade, f420, f420, (0, 0, 0), (0, 0, 0), w, h, _desc(pdev), _desc(pout))
    assert rc == 0, msg
    assert loaded.last_kernel == "k_yuv_stack_vec<1,1,1,1,1,1,0,1>[lut1d,cdl,lut3d:2]", loaded.last_kernel
    assert _eq(_host(pout, 10), _want(loaded._res, "lut1d,cdl,lut3d", grade, 10, 10, 10, "420", "420", planar, "abi-planar"))
    rc, msg = _abi(loaded, [(L1, 0), (CD, 0), (L3, 2)], grade, f420, f420, semi, semi, w, h, s, d)
    assert rc == 0, msg
    assert loaded.last_kernel == "k_yuv_stack_semi_vec<1,1,1,1,1,1,0,1>[lut1d,cdl,lut3d:2]", loaded.last_kernel
    assert _eq(_host(out, 10), _expect(loaded._res, "p010le", "p010le", "lut1d,cdl,lut3d", grade, planar, "abi"))


# ------------------------------------------------------------------ 9. the group
@pytest.mark.gpu
def test_group_shards_equal_the_single_engine_call(loaded, luts, l1ds, grade, monkeypatch):
    from lut_renderer_amd.multigpu import LutEngineGroup
    monkeypatch.setenv("LUTR_GROUP_FORCE_REMOTE", "1")
    stages = "lut1d,cdl,lut3d,lut3d2"
    for (w, h), a, b in (((W, H), "p010le", "yuv422p10le"), ((W, H), "nv12", "nv12"), ((33, 7), "nv16", "nv12")):
        fa, la, _ = _side(a)
        fb = yuv_side(b)
        planar = _src("natural", w, h, fa.depth, la, k=9)
        single = _run(loaded, a, b, stages, grade, planar)
        with LutEngineGroup([0, 0]) as g:
            assert g.treat_as_remote
            g.set_lut(luts["log709_33"][1])
            g.set_lut2(luts["random_9"][1])
            g.set_lut1d(l1ds["gamma1024"], "cubic")
            got = g.apply_yuv_stack_semi(_dev(_held(planar, a), loaded.device), pix_fmt=a, out_pix_fmt=b, stages=stages, cdl=grade)
            assert g.last_remote == 1 and all(r0 % 2 == 0 for r0, _ in g.last_blocks), g.last_blocks
            assert all(k.startswith("k_yuv_stack_semi_") for k in g.last_kernels), g.last_kernels
            assert _eq(_host(got, fb.depth), single), (w, h, a, b)
        assert _eq(single, _expect(loaded._res, a, b, stages, grade, planar, ("group", w))), (w, h, a, b)
