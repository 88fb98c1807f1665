#!/usr/bin/env python3
"""tools/record_container_options.py [OUT.json]: records what the option checks of the YUV containers do (CPU only, no GPU).

For every ordered pair of NAMES, crossed with dither x chroma_loc x out_size, what `formats.check_semi_options` and
`formats.check_packed_options` return or raise; for every pair (and a source without an out_pix_fmt), what
`api.engine_call_for` returns or raises with a default plan and with a full-range plan; and, for every semi-planar and packed
name plus yuv420p / yuv422p10le at 7x5 and 8x6, `frame_bytes` and the shapes, strides and storage offsets of `plane_views`
over 2 frames of the stream layout.  tests/test_container_options.py replays all of it against the checked-in recording
(tests/golden/container_options.json), so a change to the argument layer that moves a refusal, its text or a layout shows.
"""
from __future__ import annotations

import itertools
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

NAMES = ("yuv420p", "yuv422p", "yuv444p", "yuvj420p", "yuv422p10le", "nv12", "nv21", "nv16", "p010le", "p210le", "yuyv422",
         "uyvy422", "yvyu422", "y210le", "y216le", "gbrp", "rgb24", "gbrpf32le", "vuya", "y210be")
#: (dither, chroma_loc, out_size)
OPTIONS = tuple(itertools.product(("none", "error_diffusion"), (None, "left"), (None, (64, 36))))
LAYOUT_SIZES = ((7, 5), (8, 6))


def outcome(fn, *args):
    """What a call does, as JSON: {"return": value} or {"raise": type name, "message": text}."""
    try:
        return {"return": fn(*args)}
    except Exception as exc:                                   # noqa: BLE001 -- the type and the text ARE the record
        return {"raise": type(exc).__name__, "message": str(exc)}


def plans(pix_fmt):
    """The default plan and the full-range plan of a source, resolved as `api.apply_lut` resolves them."""
    from lut_renderer_amd.params import ProcessingParams, VideoInfo
    from lut_renderer_amd.plan import resolve_lut_plan
    out = []
    for color_range in (None, "pc"):
        info = VideoInfo(width=64, height=36, pix_fmt=pix_fmt, bit_depth=None, colorspace=None, color_range=color_range)
        out.append(resolve_lut_plan(ProcessingParams(), "engine.cube", info))
    return out


def layout_names():
    from lut_renderer_amd import _native
    return tuple(_native.SEMI_FORMATS) + tuple(_native.PACKED_YUV_FORMATS) + ("yuv420p", "yuv422p10le")


def layout_record(name, w, h):
    import torch

    from lut_renderer_amd.stream import input_layout
    lay = input_layout(name, w, h)
    views = lay.plane_views(torch.zeros(2 * lay.frame_bytes, dtype=torch.uint8), 2)
    return {"frame_bytes": lay.frame_bytes,
            "planes": [[str(v.dtype), list(v.shape), list(v.stride()), v.storage_offset()] for v in views]}


def record() -> dict:
    """The whole recording.  Outcomes repeat a lot: they are stored once in "outcomes" and referred to by index."""
    from lut_renderer_amd.api import engine_call_for
    from lut_renderer_amd.engine import check_packed_options, check_semi_options
    table, index = [], {}

    def ref(o) -> int:
        key = json.dumps(o, sort_keys=True)
        if key not in index:
            index[key] = len(table)
            table.append(o)
        return index[key]

    checks, calls = {}, {}
    for a in NAMES:
        default, full = plans(a)
        for b in NAMES + (None,):
            key = f"{a}->{b}"
            calls[key] = [ref(outcome(engine_call_for, plan, a, b)) for plan in (default, full)]
            if b is not None:
                checks[key] = [[ref(outcome(fn, a, b, *opt)) for fn in (check_semi_options, check_packed_options)]
                               for opt in OPTIONS]
    layouts = {f"{n}@{w}x{h}": layout_record(n, w, h) for n in layout_names() for w, h in LAYOUT_SIZES}
    return {"names": list(NAMES), "options": [list(o[:2]) + [list(o[2]) if o[2] else None] for o in OPTIONS],
            "outcomes": table, "checks": checks, "calls": calls, "layouts": layouts}


def main(argv) -> int:
    out = Path(argv[1]) if len(argv) > 1 else ROOT / "tests" / "golden" / "container_options.json"
    out.write_text(json.dumps(record(), separators=(",", ":"), sort_keys=True) + "\n")
    print(f"{out}: {out.stat().st_size} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
