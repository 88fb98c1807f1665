"""The argument layer of the YUV containers against a recording of what it did before it was gathered into one place
(tests/golden/container_options.json, written by tools/record_container_options.py): every refusal, its text and the order in
which refusals win, the arguments `engine_call_for` returns, and the rawvideo layouts.  No device needed."""
import json
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import record_container_options as rec  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    return json.loads((ROOT / "tests" / "golden" / "container_options.json").read_text())


def test_recording_covers_the_names_and_options(golden):
    assert golden["names"] == list(rec.NAMES)
    assert [tuple(o[:2]) + (tuple(o[2]) if o[2] else None,) for o in golden["options"]] == list(rec.OPTIONS)
    n = len(rec.NAMES)
    assert len(golden["checks"]) == n * n and len(golden["calls"]) == n * (n + 1)
    assert all(len(v) == len(rec.OPTIONS) for v in golden["checks"].values())


def test_option_checks_reproduce_the_recording(golden):
    from lut_renderer_amd.engine import check_container_options, check_packed_options, check_semi_options
    seen = set()
    for a in rec.NAMES:
        for b in rec.NAMES:
            for opt, (semi_ref, packed_ref) in zip(rec.OPTIONS, golden["checks"][f"{a}->{b}"]):
                semi, packed = golden["outcomes"][semi_ref], golden["outcomes"][packed_ref]
                assert rec.outcome(check_semi_options, a, b, *opt) == semi, (a, b, opt)
                assert rec.outcome(check_packed_options, a, b, *opt) == packed, (a, b, opt)
                # the one function is the callers' ladder: the packed check first, the semi-planar one when it found no packed
                # side, and the kind is the one the two booleans imply
                if "raise" in packed:
                    want = packed
                elif packed["return"]:
                    want = {"return": "packed"}
                elif "raise" in semi:
                    want = semi
                else:
                    want = {"return": "semi" if semi["return"] else None}
                assert rec.outcome(check_container_options, a, b, *opt) == want, (a, b, opt)
                seen.add(json.dumps(want))
    assert {json.dumps({"return": k}) for k in (None, "semi", "packed")} <= seen


def test_engine_call_for_reproduces_the_recording(golden):
    from lut_renderer_amd.api import engine_call_for
    for a in rec.NAMES:
        default, full = rec.plans(a)
        assert full.prologue and default.prologue == a.startswith("yuvj")
        for b in rec.NAMES + (None,):
            refs = golden["calls"][f"{a}->{b}"]
            for plan, r in zip((default, full), refs):
                assert rec.outcome(engine_call_for, plan, a, b) == golden["outcomes"][r], (a, b, plan.prologue)


@pytest.mark.parametrize("size", rec.LAYOUT_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_layouts_reproduce_the_recording(golden, size):
    names = rec.layout_names()
    assert {"nv12", "nv21", "p010le", "p216le", "yuyv422", "uyvy422", "y210le", "yuv420p", "yuv422p10le"} <= set(names)
    for name in names:
        want = golden["layouts"][f"{name}@{size[0]}x{size[1]}"]
        got = rec.layout_record(name, *size)
        assert got["frame_bytes"] == want["frame_bytes"], name
        assert got["planes"] == want["planes"], name
