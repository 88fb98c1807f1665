"""The upload markers of `apply_lut` on kept engines, without a GPU.  `api._stack_upload` is the one reader of `_applied_lut`,
`_applied_lut2` and `_applied_lut1d`; the setters of `LutEngine` and `LutEngineGroup` are the ones that clear them.  Both halves
run here as they are: the engines below are real `LutEngine` / `LutEngineGroup` objects whose native library is a recorder (every
`lutr_*` call returns 0 and is logged) and whose apply entries only note the call.  Each history of section F of
tests/test_gpu_stack_history.py is replayed and the exact list of setters that ran -- and so the ones that did not -- is asserted
after every step.  Also here: the guard against the `id()` trap of the GPU modules' memoised references, and the coverage
condition of the seeded walk, replayed without a GPU."""
import os
import threading
from pathlib import Path

import numpy as np

from lut_renderer_amd import api, cube, frames
from lut_renderer_amd.cdl import Cdl
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.multigpu import LutEngineGroup

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
F = np.float32
SETTERS = {"lutr_ctx_set_lut": "lut", "lutr_ctx_set_lut2": "lut2", "lutr_ctx_set_lut1d": "lut1d", "lutr_ctx_set_precision": "precision",
           "lutr_lut_broadcast_ex": "broadcast"}


class _Lib:
    """Stands in for liblutr: every entry returns 0; the four setters are logged as (engine tag, what)."""

    def __init__(self, log, tag):
        self._log, self._tag = log, tag

    def __getattr__(self, name):
        def call(*args):
            if name in SETTERS:
                what = SETTERS[name]
                if what in ("lut2", "lut1d") and args[1] is None:
                    what += "=None"
                self._log.append((self._tag, what))
            return 0
        return call


class _Engine(LutEngine):
    """A `LutEngine` with no context behind it: its setters are the product's, its apply entries record (entry, keywords).
    `LutEngine.__init__` needs a GPU, so the attributes are set here.  What the code under test reads: `_lib`, `_ctx`, `_lock`
    and the three markers (set_lut / set_lut2 / set_lut1d / set_precision), `_has_prelut` (set_prelut), `n` / `n2` / `n1d`
    (`formats.held_resources`), `precision` (`api._stack_upload`), `use_torch_stream` and `_alpha_kernels` (`_bind_stream`, from
    the group's set_lut).  The rest mirrors the constructor; an attribute added there belongs here too."""

    def __init__(self, log, tag="e"):
        self._lib, self._ctx, self.device = _Lib(log, tag), None, "cpu"
        self.n, self.scale, self.use_torch_stream, self._lock, self.precision = 0, None, False, threading.RLock(), "strict"
        self._frame_strength = self._applied_lut = self._applied_lut2 = self._applied_lut1d = self._alpha_kernels = None
        self.n2 = self.n1d = 0
        self._scratch_slots, self._has_prelut, self.calls = {}, False, []

    def close(self):
        pass

    def sync(self):
        pass

    def _note(entry):                                                  # noqa: N805
        def apply(self, planes, out=None, **kw):
            self.calls.append((entry, kw))
            return out
        return apply

    apply_yuv, apply_yuv_stack, apply_rgb_stack = _note("apply_yuv"), _note("apply_yuv_stack"), _note("apply_rgb_stack")
    apply_yuv_stack_to_rgb, apply_yuv_to_rgb = _note("apply_yuv_stack_to_rgb"), _note("apply_yuv_to_rgb")
    apply_yuv_lut1d, apply_yuv_chain = _note("apply_yuv_lut1d"), _note("apply_yuv_chain")


class _Group(LutEngineGroup):
    """A `LutEngineGroup` of two such engines: its setters are the product's, its apply entries record.  The setters read
    `engines`, `_lock`, `_lib`, `treat_as_remote`, `precision` and the three markers."""

    def __init__(self, log):
        self.devices, self.treat_as_remote, self._lock = (0, 0), True, threading.RLock()
        self._applied_lut = self._applied_lut2 = self._applied_lut1d = None
        self.precision, self.engines, self._lib = "strict", [_Engine(log, "g0"), _Engine(log, "g1")], _Lib(log, "g")
        self.last_blocks, self.calls = [], []

    def close(self):
        pass

    def sync(self):
        pass

    apply_yuv_stack, apply_rgb_stack = _Engine._note("apply_yuv_stack"), _Engine._note("apply_rgb_stack")
    apply_yuv_stack_to_rgb = _Engine._note("apply_yuv_stack_to_rgb")


def _lut(n, k=0):
    return cube.CubeLut(n, np.ones(3, F), (cube.identity_lattice(n) * (1.0 - 0.01 * k)).astype(F))


YUV = frames.natural_yuv(16, 8, 10, 1, 1)
RGB = frames.natural_rgb(16, 8, 10)
STAGES = "lut1d,cdl,lut3d,lut3d2"
ROUTES = {
    "stages": (YUV, dict(pix_fmt="yuv420p10le", stages=STAGES), "apply_yuv_stack"),
    "rgb_stages": (RGB, dict(pix_fmt="gbrp10le", rgb_stages=STAGES), "apply_rgb_stack"),
    "rgb_out_stages": (YUV, dict(pix_fmt="yuv420p10le", rgb_out="gbrp10le", rgb_out_stages=STAGES), "apply_yuv_stack_to_rgb"),
}


def _call(eng, route, A, B, l1, mode="linear", **more):
    planes, kw, entry = ROUTES[route]
    api.apply_lut(planes, cube=A, cube2=B, lut1d=l1, interp1d=mode, cdl=Cdl(saturation=0.7), engine=eng, **kw, **more)
    assert eng.calls[-1][0] == entry, eng.calls[-1]


def _per_engine(eng, what):
    """What one setter of the engine or of each engine of the group logs."""
    if not isinstance(eng, LutEngineGroup):
        return [("e", w) for w in what]
    out = []
    for w in what:      # the first lattice is uploaded to the first context and broadcast; everything else goes to each
        out += [("g0", "lut"), ("g", "broadcast")] if w == "lut" else [("g0", w), ("g1", w)]
    return out


def _history(eng, log):
    """The history of section F on `eng` (an engine or a group): after each step exactly the setters named ran."""
    A, A2, B, B2 = _lut(2), _lut(3, 1), _lut(2, 2), _lut(5, 3)
    l1, l2 = cube.Lut1D.identity(16), cube.Lut1D.identity(33)
    steps = []

    def step(what, want, fn):
        del log[:]
        fn()
        steps.append(f"{what}: {log}")
        assert log == _per_engine(eng, want), "\n".join(steps)

    step("first call: everything is uploaded", ["lut", "lut2", "lut1d"], lambda: _call(eng, "stages", A, B, l1))
    step("same objects, next route: nothing", [], lambda: _call(eng, "rgb_stages", A, B, l1))
    step("same objects, third route: nothing", [], lambda: _call(eng, "rgb_out_stages", A, B, l1))
    step("another first lattice alone", ["lut"], lambda: _call(eng, "stages", A2, B, l1))
    step("another second lattice alone", ["lut2"], lambda: _call(eng, "rgb_stages", A2, B2, l1))
    step("another 1D LUT alone", ["lut1d"], lambda: _call(eng, "rgb_out_stages", A2, B2, l2))
    step("the same 1D LUT in another mode", ["lut1d"], lambda: _call(eng, "stages", A2, B2, l2, "cubic"))
    step("... and that mode again: nothing", [], lambda: _call(eng, "rgb_stages", A2, B2, l2, "cubic"))
    step("back to the first objects", ["lut", "lut2", "lut1d"], lambda: _call(eng, "stages", A, B, l1))
    # the engine's own setters between two calls with the same objects: each clears its marker, the others stand
    step("set_lut1d directly", ["lut1d"], lambda: eng.set_lut1d(l2, "linear"))
    step("-> the 1D LUT is uploaded again", ["lut1d"], lambda: _call(eng, "rgb_out_stages", A, B, l1))
    step("set_lut2 directly", ["lut2"], lambda: eng.set_lut2(B2))
    step("-> the second lattice is uploaded again", ["lut2"], lambda: _call(eng, "stages", A, B, l1))
    step("set_lut directly", ["lut"], lambda: eng.set_lut(A2))
    step("-> the first lattice is uploaded again", ["lut"], lambda: _call(eng, "rgb_stages", A, B, l1))
    step("set_lut2(None), set_lut1d(None)", ["lut2=None", "lut1d=None"], lambda: (eng.set_lut2(None), eng.set_lut1d(None)))
    step("-> both come back", ["lut2", "lut1d"], lambda: _call(eng, "stages", A, B, l1))
    # a resource not passed is not touched, and its marker stands for the next call that passes it
    planes, kw, _ = ROUTES["stages"]
    step("a call that passes the first lattice only", [],
         lambda: api.apply_lut(planes, cube=A, engine=eng, **dict(kw, stages="lut3d")))
    step("-> the others still stand", [], lambda: _call(eng, "rgb_out_stages", A, B, l1))
    step("precision: set when it differs", ["precision"],
         lambda: api.apply_lut(planes, cube=A, engine=eng, precision="fma32", **dict(kw, stages="lut3d")))
    step("... and not when it is the engine's", [],
         lambda: api.apply_lut(planes, cube=A, engine=eng, precision="fma32", **dict(kw, stages="lut3d")))
    assert eng.precision == "fma32"
    step("back to strict", ["precision"], lambda: _call(eng, "stages", A, B, l1))


def test_marker_history_on_an_engine():
    log = []
    _history(_Engine(log), log)


def test_marker_history_on_a_group():
    """The group's setters reach both contexts, in order, after each change; its markers are its own (the engines' stay None)."""
    log = []
    grp = _Group(log)
    _history(grp, log)
    assert all(e._applied_lut is None and e._applied_lut2 is None and e._applied_lut1d is None for e in grp.engines)


def test_marker_history_on_the_cached_engine(monkeypatch, tmp_path):
    """engine=None: the engine `apply_lut` keeps per device tuple.  Files are parsed once per (path, mtime, size): the same path
    twice uploads once; a file rewritten in place with a moved mtime is another object and is uploaded again."""
    log = []
    eng = _Engine(log)
    monkeypatch.setattr(api, "_cached_engine", lambda devices: eng)
    a = cube.write_cube(tmp_path / "a.cube", cube.log709_lattice(9))
    b = tmp_path / "b.cube"
    l1 = tmp_path / "curve.cube"
    planes, kw, _ = ROUTES["stages"]

    def write(k):
        cube.write_cube(b, cube.identity_lattice(2 + k))
        cube.write_lut1d(l1, np.stack([np.linspace(0.0, 1.0, 5 + k) ** (1.0 + 0.1 * k)] * 3))
        for p in (b, l1):
            os.utime(p, (1_700_000_000 + k, 1_700_000_000 + k))

    def call(want):
        del log[:]
        api.apply_lut(planes, cube=a, cube2=b, lut1d=l1, cdl=Cdl(saturation=0.7), **kw)
        assert log == [("e", w) for w in want], log

    write(0)
    call(["lut", "lut2", "lut1d"])
    call([])
    write(1)
    call(["lut2", "lut1d"])
    call([])
    eng.set_lut(_lut(3))
    call(["lut"])


def test_a_memoised_reference_tells_two_live_1d_luts_apart():
    """The `_want` helpers of the GPU modules memoise by `id()` of the resources.  Two live objects have two ids, so the same
    key text gives two references; what a history test must not do is let a resource die while the module runs (a freed
    object's id is handed out again) -- tests/test_gpu_stack_history.py keeps every one in a module-level list."""
    from tests import test_gpu_lut1d as fam
    src = fam._src("natural", 16, 8, 10, "444", k=3)
    l1s = [cube.read_lut1d(GOLDEN / "lut1d" / f"{n}.cube") for n in ("curve17", "gamma1024")]
    lut = _lut(2)
    want = [fam._want(l1, "linear", lut, None, 10, 10, 10, "444", "444", src, "one key text") for l1 in l1s]
    assert id(l1s[0]) != id(l1s[1])
    assert not all(np.array_equal(a, b) for a, b in zip(*want))
    for l1, w in zip(l1s, want):        # ... and each is the reference of its own 1D LUT, from scratch
        tab = fam._native.lut1d_table(l1, "linear", 10)
        k = fam.twin.consts("bt709", "tv", "bt709", "tv", 10, 10, 10, 0, 0)
        assert all(np.array_equal(a, b) for a, b in zip(w, fam.twin.apply(tab, lut, None, k, 10, 10, 0, 0, 0, 0, src)))


def test_the_seeded_walk_covers_its_table():
    """The draw of test_seeded_stack_walk, replayed without a GPU.  Applies: at least 35 of the 60 steps are applies that run,
    every entry of the apply table runs at least twice, and each documented refusal occurs.  State changes: every kind of action
    occurs at least twice and every draw differs from the state current at that step; a plain cube, a domain-scaled cube and a
    .csp are each loaded and applied before the next first lattice replaces them; the second lattice changes its size (n = 2 or
    33); every variant and every precision is drawn; and behind a change of each kind there is an apply that reads that state on
    a vector kernel, before the next change of the kind."""
    from tests.test_gpu_stack_history import APPLIES, WALK_CHOICES, WALK_SEED, WALK_STEPS, walk_coverage, walk_plan
    plan = walk_plan(WALK_SEED, WALK_STEPS)
    assert len(plan) == WALK_STEPS == 60
    c = walk_coverage(plan)
    assert c["ran"] >= 35, c["ran"]
    assert len(c["per_entry"]) == len(APPLIES) and min(c["per_entry"]) >= 2, c["per_entry"]
    assert c["refusals"] == {"prelut", "vec_global", "lut2"}
    assert all(len(v) >= 2 for v in c["changes"].values()), {k: len(v) for k, v in c["changes"].items()}
    assert not c["same"], c["same"]
    assert c["lut_kinds"] == {"cube", "domain", "csp"}
    assert {"n2", "n33b"} & set(c["changes"]["lut2"]) and None in c["changes"]["lut2"]
    assert set(c["changes"]["variant"]) == set(WALK_CHOICES["variant"]) and set(c["changes"]["precision"]) == set(WALK_CHOICES["precision"])
    assert c["followed"] == set(WALK_CHOICES), c["followed"]
