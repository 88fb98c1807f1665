"""The grid-stride kernels several trips deep, on small frames.

The stack, 1D LUT and alpha kernels and every generic kernel walk their units with a grid stride under a capped grid, and a
production-size frame runs each thread for two trips, the second partial; the frames the other GPU tests use fit under every cap,
so that each thread there makes one trip.  Here a child process (tests/_gpu_stride_worker.py) runs with LUTR_MAX_BLOCKS=2, a
second one with 1: frames of 136 x 36 and 67 x 21, two to six of them, then take every kernel through three trips and more, the
last one partial, with consecutive trips of a thread in different frames -- the stride itself, the output words zeroed again, the
matte words and the per-trip frame and strength, the fences across trips, the LDS tables read on later trips, threads that leave
the loop while others of their wave go on.

Every (case, cap) is a test of its own: the reference is recomputed in this process with the twin (or the oracle) the family's own
GPU test uses, through that test's `_want`, and every plane is compared bit for bit, the spare row and columns around it included
(they keep the sentinel); the child's `[lutr gs]` line proves the regime against this module's own unit formulas, `last_kernel`
the kernel.  The same arithmetic is checked for the whole table on the CPU (the unmarked tests below).

Found by these cases: no defect -- every kernel is bit-exact under both caps.  That the cases can fail was checked once by hand:
the stack vector kernels built with the frame index of a thread's first trip kept for its later ones (an in-bounds read of the
wrong frame) failed `stack-lds`, `mix-420to422` and `matte-10` under both caps and passed tests/test_gpu_stack.py."""
import os
import re
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

from lut_renderer_amd import _native
from tests import _alpha_twin, _lut1d_twin, _premul_twin, _rgbf_twin
from tests import _stride_cases as sc
from tests.test_gpu_lut1d import _want as l1d_want
from tests.test_gpu_matte import _want as matte_want
from tests.test_gpu_mix import _want as mix_want
from tests.test_gpu_semi import _batch as semi_batch, _side as semi_side, _want as semi_want
from tests.test_gpu_stack import LAYOUTS, _list, _want as stack_want
from tests.test_gpu_v210 import _want as v210_want

ROOT = Path(__file__).resolve().parent.parent
WORKER = ROOT / "tests" / "_gpu_stride_worker.py"
CAPS = (2, 1)
CHILD_LIMIT_S = 180          # the limit of the stack and matte worker tests.  A limit, not a measurement: a child runs for seconds
_refs = {}                   # expected planes per case, computed once and shared by both caps (never written to)


# ================================================================== the knob's validation rule, on the CPU
def test_max_blocks_knob_validation():
    """The function every grid-stride launch judges LUTR_MAX_BLOCKS with (capped_blocks, lutr_launch.h), through the C ABI."""
    knob = _native.max_blocks_knob
    for cap in (2048, 16384):
        assert knob(None, cap) == cap                                                    # unset
        for ok in (1, 2, 3, 7, 100, cap - 1, cap):
            assert knob(str(ok), cap) == ok
        for above in (cap + 1, 10 * cap, 2 ** 31 - 1):                                   # min(its own cap, value)
            assert knob(str(above), cap) == cap
        for bad in ("0", "00", "-2", "-0", "+2", "", " 2", "2 ", "2x", "x2", "1e2", "0x10", "2.0", "two", "2147483648",
                    "99999999999999999999"):
            assert knob(bad, cap) == cap, (bad, cap)
    assert knob("2", 1) == 1 and knob("1", 1) == 1                                       # never above the site's own cap


# ================================================================== the regime of every case, on the CPU
def _ceil(n, d):
    return -(-n // d)


def _frame_units(case):
    """This module's own count of the units of ONE frame of the launch whose `[lutr gs]` line carries the case's regime."""
    w, h, kind, gs = case["w"], case["h"], case["kind"], case["gs"]
    if kind in ("stack", "lut1d"):
        din, dout = (case["din"], case["dout"]) if kind == "stack" else (10, 10)
        (icsx, icsy), (ocsx, ocsy) = (LAYOUTS[case["a"]], LAYOUTS[case["b"]]) if kind == "stack" else (LAYOUTS["420"], LAYOUTS["422"])
        csx, csy = max(icsx, ocsx), max(icsy, ocsy)
        if gs.endswith("_generic"):                            # one thread per union block
            return _ceil(w, 1 << csx) * _ceil(h, 1 << csy)
        pxt = 8 if din > 8 and dout == 8 else (4 if din > 8 else 8)     # 8 bytes of luma a row; 16 for 16 -> 8 bit
        return (w // pxt) * (h >> csy)
    if kind == "rgb_l1d":
        return (w // 2) * h                                    # a dword of two 16-bit samples
    if kind == "alpha":
        return w * h if gs == "k_alpha_generic" else (w // 8) * h       # 16 bytes on the wider side: 8 samples of 16 bits
    if kind == "yuv":
        return _ceil(w, 2) * _ceil(case["shard"][1], 2)
    if kind in ("dither", "semi"):
        return _ceil(w, 2) * _ceil(h, 2)
    if kind == "v210":
        return _ceil(w, 6) * h                                 # a group of six luma samples, 4:2:2 out
    return w * h                                               # rgb, packed, rgbf, rgbaf: one pixel


def _regime(case, cap, units):
    """What the issue asks of a launch of `units` under `cap` blocks."""
    per_trip = 256 * cap
    assert units == _frame_units(case) * case["nf"], (case["id"], units)
    if cap == 2:
        assert _ceil(units, per_trip) >= 3, (case["id"], units)                    # at least three trips
    assert units % per_trip != 0, (case["id"], units)                              # the last one partial
    assert case["nf"] >= 2 and _frame_units(case) % per_trip != 0, case["id"]      # a thread's trips change frames


def test_every_case_reaches_its_regime():
    for case in sc.CASES:
        for cap in CAPS:
            _regime(case, cap, _frame_units(case) * case["nf"])
        assert 2 <= case["nf"] <= 6 and (case["w"], case["h"]) in ((136, 36), (67, 21), (139, 36)), case["id"]
    assert len(sc.BY_ID) == len(sc.CASES)


def test_per_frame_strengths_differ_and_hold_both_ends():
    for case in sc.CASES:
        s = case.get("strength")
        if s is not None:
            assert len(s) == case["nf"] and len(set(s)) == len(s) and 0.0 in s and 1.0 in s, case["id"]


# ================================================================== the children
def _run_child(cap, out_dir):
    ids = [c["id"] for c in sc.CASES]
    env = dict(os.environ, LUTR_MAX_BLOCKS=str(cap), LUTR_DEBUG="1")
    for knob in ("LUTR_STACK_LDS", "LUTR_L1D_LDS"):
        env.pop(knob, None)
    t0 = time.monotonic()
    try:
        p = subprocess.run([sys.executable, str(WORKER), str(out_dir)] + ids, env=env, cwd=str(ROOT), capture_output=True, text=True,
                           timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode("utf-8", "replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"the LUTR_MAX_BLOCKS={cap} child did not finish within {CHILD_LIMIT_S} s; its last lines:\n{err[-3000:]}",
                    pytrace=False)
    wall = time.monotonic() - t0
    print(f"LUTR_MAX_BLOCKS={cap} child: {len(ids)} cases, exit {p.returncode}, wall {wall:.1f} s")
    if p.returncode != 0:
        pytest.fail(f"the LUTR_MAX_BLOCKS={cap} child ended with {p.returncode} after {wall:.1f} s; its last lines:\n{p.stderr[-3000:]}",
                    pytrace=False)
    debug, cur = {}, None
    for line in p.stderr.splitlines():
        m = re.match(r"\[case (\S+)\]", line)
        if m:
            cur = m.group(1)
            debug[cur] = []
        elif cur and line.startswith("[lutr gs] "):
            debug[cur].append(line)
    results = {}
    for cid in ids:
        with np.load(out_dir / f"{cid}.npz") as z:
            results[(cap, cid)] = dict(planes=[z[f"p{i}"] for i in range(len(z.files) - 1)], kernel=str(z["kernel"]),
                                       debug=debug.get(cid, []), wall=wall)
    return results


@pytest.fixture(scope="module")
def capped(tmp_path_factory):
    """Both children's results by (cap, case id).  The second child starts only if the first exited 0; a non-zero exit, a death
    by signal or the time limit fails this fixture for every case, and nothing is started after it -- no retry, and no case is
    lifted into this process."""
    results = {}
    for cap in CAPS:
        results.update(_run_child(cap, tmp_path_factory.mktemp(f"stride{cap}")))
    return results


# ================================================================== references, from scratch
def _first_diff(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: plane {i} {a.shape} {a.dtype} != {b.shape} {b.dtype}"
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        if not np.array_equal(a, b):
            bad = np.argwhere(a != b)
            raise AssertionError(f"{what}: plane {i} differs at {len(bad)} samples, first {bad[0].tolist()} got {a[tuple(bad[0])]} "
                                 f"want {b[tuple(bad[0])]}")


def _stacked(per_frame):
    """[frame][plane] -> [plane] stacked over frames."""
    return [np.stack([np.asarray(f[i]) for f in per_frame]) for i in range(len(per_frame[0]))]


def _planes(orc, case):
    """The planes the call must give, [nf, rows, cols] each, from the family's own reference."""
    r = sc.resources()
    lut, cid, nf, w, h = r["lut"], case["id"], case["nf"], case["w"], case["h"]
    host = sc.source(case)
    src, kind = host["src"], case["kind"]
    frames_ = [[p[i] for p in src] for i in range(nf)]
    if kind == "stack":
        res = dict(lut=lut, lut2=None, l1=r["l1"], prelut=None)
        din, dout, a, b = case["din"], case["dout"], case["a"], case["b"]
        if case["matte"]:
            depth, _, invert = case["matte"]
            return matte_want(res, case["stages"], r["cdl"], case["strength"], host["matte"], depth, invert, din, din, dout, a, b, src, cid)
        if case["strength"] is not None:
            return mix_want(res, case["stages"], r["cdl"], case["strength"], din, din, dout, a, b, src, cid)
        return stack_want(res, case["stages"], r["cdl"], din, din, dout, a, b, src, cid)
    if kind == "lut1d":
        return l1d_want(r["l1"][0], r["l1"][1], lut, case["mode"], 10, 10, 10, "420", "422", src, cid)
    if kind == "rgb_l1d":
        return _lut1d_twin.apply_rgb(_native.lut1d_table(*r["l1"], 10), 10, src)
    if kind == "alpha":
        dout = case["dout"]
        k = orc.yuv_constants("bt709", "tv", "bt709", "tv", 10, 10, dout, 4)
        colour = _stacked([orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, dout, 1, 1, f[:3]) for f in frames_])
        alpha = _alpha_twin.convert(src[3], 10, dout) if case["src_alpha"] else _alpha_twin.fill((nf, h, w), dout)
        return colour + [np.asarray(alpha).astype(colour[0].dtype)]
    if kind in ("yuv", "dither"):
        k = orc.yuv_constants(din=10, dl=10, dout=10, chroma_n=4)
        kw = dict(dither="error_diffusion") if kind == "dither" else {}
        return _stacked([orc.apply_yuv(lut.table, lut.scale, "tetrahedral", k, 10, 10, 10, 1, 1, f, **kw) for f in frames_])
    if kind == "rgb":
        return _stacked([orc.apply_rgb(lut.table, lut.scale, 10, "tetrahedral", f) for f in frames_])
    if kind == "packed":
        return [np.stack([orc.apply_packed(lut.table, lut.scale, case["fmt"], "tetrahedral", src[0][i]) for i in range(nf)])]
    if kind == "rgbf":
        return _stacked([_rgbf_twin.apply_float(lut.table, lut.scale, "tetrahedral", f) for f in frames_])
    if kind == "rgbaf":
        return _stacked([_premul_twin.apply_float(lut.table, lut.scale, "tetrahedral", f) for f in frames_])
    if kind == "v210":
        refs = [v210_want(orc, "stride-u33", lut, "tetrahedral", "v210", "yuv422p10le", w, h, 30 + i) for i in range(nf)]
    else:
        refs = [semi_want(orc, "stride-u33", lut, "tetrahedral", case["fmt"], case["fmt"], "natural", w, h, 20 + i) for i in range(nf)]
    for i, (s, _) in enumerate(refs):                          # the helper's source is the one the child was given
        assert all(np.array_equal(x, y) for x, y in zip(s, frames_[i])), (cid, i)
    if kind == "v210":
        return _stacked([o for _, o in refs])
    return semi_batch([semi_side(o, case["fmt"]) for _, o in refs])


def _reference(orc, case):
    """What the saved tensors must hold: the planes inside the sentinel of the spare row and columns (and, for a row shard, of the
    rows outside it)."""
    if case["id"] not in _refs:
        planes = _planes(orc, case)
        want = []
        for i, (p, (shape, dt)) in enumerate(zip(planes, sc.out_layout(case))):
            p = np.asarray(p)
            assert p.shape == tuple(shape) and p.dtype == np.dtype(dt), (case["id"], i, p.shape, p.dtype, shape, dt)
            big = np.full(sc.spare_shape(case, shape), sc.SENTINEL[np.dtype(dt)], dtype=dt)
            if case.get("shard"):
                r0, rows = case["shard"]
                r0, r1 = (r0, r0 + rows) if i == 0 else (r0 >> 1, (r0 + rows) >> 1)
                big[:, r0:r1, :shape[2]] = p[:, r0:r1]
            else:
                big[:, :shape[1], :shape[2]] = p
            big.setflags(write=False)
            want.append(big)
        _refs[case["id"]] = want
    return _refs[case["id"]]


# ================================================================== the claims of a case
def _check_regime(case, cap, res):
    lines = {}
    for line in res["debug"]:
        m = re.fullmatch(r"\[lutr gs\] (\S+) units (\d+) blocks (\d+)", line)
        assert m, line
        assert m.group(1) not in lines, res["debug"]
        lines[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    assert case["gs"] in lines, (case["gs"], res["debug"])
    units, blocks = lines[case["gs"]]
    assert blocks == cap, res["debug"]
    _regime(case, cap, units)
    if case["both"]:                                           # the tail of a column split: a launch of its own, under the cap as well
        tail = case["both"].strip("+[")
        assert tail in lines and lines[tail][1] <= cap, res["debug"]


def _check_names(case, kern):
    want = case["kernel"]
    assert kern.endswith(want) if want.startswith("+") else kern.startswith(want), (kern, want)
    if case["both"]:
        assert case["both"] in kern, (kern, case["both"])
    if case["kind"] == "stack":
        assert kern.endswith(_list(case["stages"])), kern


# ================================================================== one test per case and cap
@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("cid", [c["id"] for c in sc.CASES])
def test_stride_case(orc, capped, cid, cap):
    case, res = sc.BY_ID[cid], capped[(cap, cid)]
    print(f"{cid} cap {cap}: {res['kernel']}\n{res['debug']}\nchild wall {res['wall']:.1f} s")
    _check_regime(case, cap, res)
    _check_names(case, res["kernel"])
    _first_diff(res["planes"], _reference(orc, case), f"{cid} cap {cap}")


@pytest.mark.gpu
def test_the_cap_changes_no_bits(capped):
    """This process has no cap: a stack case run here gives the bytes both capped children gave (the comparison with the twin
    implies it; this pins it)."""
    from lut_renderer_amd.engine import LutEngine
    from tests import _gpu_stride_worker as worker
    assert "LUTR_MAX_BLOCKS" not in os.environ
    r = sc.resources()
    with LutEngine(0) as eng:
        eng.set_lut(r["lut"])
        eng.set_lut1d(*r["l1"])
        for cid in ("stack-lds", "matte-10"):
            planes, kern = worker.run_case(eng, sc.BY_ID[cid])
            for cap in CAPS:
                assert kern == capped[(cap, cid)]["kernel"], (cid, cap, kern)
                _first_diff(capped[(cap, cid)]["planes"], planes, f"{cid}: cap {cap} against no cap")
