"""The full text of every refusal of the three stage-stack passes (DESIGN.md 3.21 .. 3.27), without a GPU.  The refusal tables of
`test_stack.py`, `test_rgbstack.py` and `test_y2rstack.py` match their messages by regular expression; here `str(exception)` of
every row -- and of rows that break several rules at once, which pin the order the refusals fire in -- is compared against
`tests/golden/stack_refusal_messages.json`, from the family's check and, for a handful of rows, through the engine entry,
`apply_lut`, `HostPipeline` and the CLI.  The file was written once by this module (`python -m tests.test_stack_messages`) and
is not regenerated: a changed wording fails here."""
import json
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from lut_renderer_amd import cube, frames
from lut_renderer_amd.cdl import Cdl
from lut_renderer_amd.engine import LutEngine
from lut_renderer_amd.formats import check_rgb_stack_options, check_stack_options, check_yuv2rgb_stack_options
from lut_renderer_amd.rgbmatrix import RgbMatrix
from tests import test_rgbstack, test_stack, test_y2rstack

GOLDEN = Path(__file__).resolve().parent / "golden"
PINNED = GOLDEN / "stack_refusal_messages.json"


def _together(base, singles):
    """Rows that break two neighbouring rules of `singles` at once, and one that breaks them all."""
    rows = [{**base, **a, **b} for a, b in zip(singles, singles[1:])]
    everything = dict(base)
    for s in singles:
        everything.update(s)
    return rows + [everything]


_FULL = test_stack.FULL
#: (what each family's table does not have) the wording with a strength, a matte and both; the matrix stage beside them; and
#: calls that break several rules, in the order `check_*_stack_options` answers them
_MORE = {
    "yuv": [dict(_FULL, dither="blue_noise", strength=0.5), dict(_FULL, dither="blue_noise", matte=True),
            dict(_FULL, dither="blue_noise", strength=0.5, matte=True), dict(_FULL, out_pix_fmt="nv12", strength=0.5),
            dict(_FULL, out_pix_fmt="nv12", matte=True), dict(_FULL, pix_fmt="gbrp10le", strength=0.5, matte=True),
            dict(_FULL, variant="vec_lds", strength=0.5), dict(_FULL, variant="vec_lds", matte=True),
            dict(_FULL, strength=0.5, precision="fast"), dict(_FULL, matte=True, precision="fma32"),
            dict(_FULL, strength=0.5, matte=True, precision="fast"), dict(_FULL, strength=1.5), dict(_FULL, strength=[0.5, 2.0]),
            dict(_FULL, strength="half"), dict(_FULL, strength=1.5, precision="fast"),
            dict(stages="matrix,lut3d"), dict(stages="lut3d", rgb_matrix=True),
            dict(stages="matrix,lut3d", rgb_matrix=True, prelut=True),
            dict(stages="matrix,lut3d", rgb_matrix=True, strength=0.5), dict(stages="matrix,lut3d", rgb_matrix=True, matte=True),
            dict(stages="matrix,lut3d", rgb_matrix=True, strength=0.5, matte=True),
            dict(stages="matrix,lut3d", rgb_matrix=True, strength=0.5, pix_fmt="nv12"),
            dict(stages="cdl,lut3d", pix_fmt="nv12", dither="blue_noise"), dict(_FULL, pix_fmt="nv12", out_pix_fmt="gbrp10le"),
            dict(stages="cdl,matrix,lut3d", cdl=True, rgb_matrix=True, prelut=True),
            dict(stages="matrix,cdl,lut3d", cdl=True, rgb_matrix=True, prelut=True)]
    + _together(_FULL, [dict(dither="error_diffusion"), dict(chroma_loc="left"), dict(out_size=(8, 4)),
                        dict(out2_pix_fmt="yuv420p"), dict(alpha_mode="premultiplied"), dict(variant="vec_lds"),
                        dict(strength=0.5, precision="fast")]),
    "rgb": [dict(stages="cdl,lut3d", pix_fmt="yuv420p10le", dither="blue_noise"),
            dict(stages="lut3d", out_pix_fmt="rgb48le", dither="blue_noise"),
            dict(stages="lut3d:pyramid", pix_fmt="rgb24", variant="vec_global")]
    + _together(dict(stages="lut3d"), [dict(intermediate_pix_fmt="yuv420p"), dict(dither="error_diffusion"), dict(out_size=(8, 8)),
                                       dict(chroma_loc="left"), dict(strength=0.5), dict(matte=True),
                                       dict(alpha_mode="premultiplied"), dict(out2_pix_fmt="yuv420p"), dict(variant="vec_lds")]),
    "y2r": [dict(stages="cdl,lut3d", pix_fmt="nv12", dither="error_diffusion"),
            dict(stages="lut3d", out_pix_fmt="gbrpf32le", chroma_loc="left"),
            dict(stages="lut3d:pyramid", pix_fmt="yuv420p", variant="vec_global")]
    + _together(dict(stages="lut3d"), [dict(chroma_loc="left"), dict(dither="error_diffusion"), dict(engine_dither="blue_noise"),
                                       dict(out_size=(8, 8)), dict(strength=0.5), dict(matte=True),
                                       dict(alpha_mode="premultiplied"), dict(out2_pix_fmt="yuv420p"), dict(variant="vec_lds")]),
}

#: a family: its table, the names its rows stand on, its check, its engine entry, and what the layers above call its list and output
FAMILIES = {
    "yuv": SimpleNamespace(table=test_stack.REFUSALS, names=test_stack.NAMES, check=check_stack_options, entry="apply_yuv_stack",
                           list_kw="stages", out_kw="out_pix_fmt", flag="--stages", out_flag="--out-pix-fmt"),
    "rgb": SimpleNamespace(table=test_rgbstack.REFUSALS, names=test_rgbstack.NAMES, check=check_rgb_stack_options,
                           entry="apply_rgb_stack", list_kw="rgb_stages", out_kw="out_pix_fmt", flag="--rgb-stages",
                           out_flag="--out-pix-fmt"),
    "y2r": SimpleNamespace(table=test_y2rstack.REFUSALS, names=test_y2rstack.NAMES, check=check_yuv2rgb_stack_options,
                           entry="apply_yuv_stack_to_rgb", list_kw="rgb_out_stages", out_kw="rgb_out", flag="--rgb-out-stages",
                           out_flag="--rgb-out"),
}

#: the fixed handful that also goes through the engine entry, `apply_lut`, `HostPipeline` and the CLI: one rule each, a strength
#: beside an option (the yuv family words its message for it; the others refuse it), and three rules at once
_LAYERED = [dict(stages="cdl,lut3d"), dict(stages="lut3d", dither="error_diffusion"), dict(stages="lut3d", chroma_loc="left"),
            dict(stages="lut3d", out_size=(8, 8)), dict(stages="lut3d", out2_pix_fmt="yuv420p"),
            dict(stages="lut3d", dither="error_diffusion", strength=0.5),
            dict(stages="lut3d", chroma_loc="left", out_size=(8, 8), out2_pix_fmt="yuv420p")]
LAYERED = {"yuv": _LAYERED + [dict(stages="lut3d", dither="blue_noise")], "rgb": _LAYERED + [dict(stages="lut3d", dither="blue_noise")],
           "y2r": _LAYERED + [dict(stages="lut3d", engine_dither="blue_noise")]}
LAYERS = ("engine", "apply_lut", "pipeline", "cli")


def _key(*parts, kw):
    return "/".join(parts) + ": " + ", ".join(f"{k}={v!r}" for k, v in sorted(kw.items()))


def _rows(family):
    return [kw for kw, _message in FAMILIES[family].table] + _MORE[family]


def _message(call, *args, **kw):
    try:
        call(*args, **kw)
    except (ValueError, TypeError) as exc:
        return f"{type(exc).__name__}: {exc}"
    return None


def from_the_check(family, kw):
    fam = FAMILIES[family]
    return _message(fam.check, **{**fam.names, **kw})


def _planes(pix_fmt):
    import torch
    if pix_fmt.startswith("gbr"):
        return [torch.from_numpy(p.view(np.int16)) for p in frames.natural_rgb(16, 8, 10)]
    return [torch.from_numpy(p.view(np.int16)) for p in frames.natural_yuv(16, 8, 10, 1, 1)]


def _lut():
    return cube.CubeLut(2, np.ones(3, np.float32), cube.identity_lattice(2).astype(np.float32))


def _kinds(stages):
    return [s.partition(":")[0] for s in stages.split(",")]


def through(layer, family, kw):
    """The message of row `kw` of `family` from `layer`, told the row in that layer's own words."""
    fam = FAMILIES[family]
    kw = {**fam.names, **kw}
    held = SimpleNamespace(n=33, n2=9, n1d=17, _has_prelut=False)
    grade, mtx = Cdl() if kw.get("cdl") else None, RgbMatrix() if kw.get("rgb_matrix") else None
    zscale = "error_diffusion" if kw.get("dither") == "error_diffusion" else "none"
    engine_dither = kw.get("engine_dither") or ("blue_noise" if kw.get("dither") == "blue_noise" else None)
    src = _planes(kw["pix_fmt"])
    if layer == "engine":
        call = {k: v for k, v in kw.items() if k not in ("cdl", "rgb_matrix")}
        return _message(getattr(LutEngine, fam.entry), held, src, cdl=grade, rgb_matrix=mtx, **call)
    if layer == "apply_lut":
        from lut_renderer_amd.api import apply_lut
        return _message(apply_lut, src, cube=_lut() if "lut3d" in _kinds(kw["stages"]) else None, pix_fmt=kw["pix_fmt"], cdl=grade,
                        rgb_matrix=mtx, engine=held, zscale_dither=zscale, engine_dither=engine_dither,
                        resolution="8x8" if kw.get("out_size") else None, chroma_loc=kw.get("chroma_loc"),
                        strength=kw.get("strength"), second_pix_fmt=kw.get("out2_pix_fmt"),
                        **{fam.list_kw: kw["stages"], fam.out_kw: kw["out_pix_fmt"]})
    if layer == "pipeline":
        from lut_renderer_amd.stream import HostPipeline
        extra = {k: kw[k] for k in ("dither", "engine_dither", "chroma_loc", "strength") if k in kw}
        return _message(HostPipeline, held, kw["pix_fmt"], 16, 8, cdl=grade, rgb_matrix=mtx,
                        out_size="8x8" if kw.get("out_size") else None, second_pix_fmt=kw.get("out2_pix_fmt"),
                        **{fam.list_kw: kw["stages"], fam.out_kw: kw["out_pix_fmt"]}, **extra)
    from lut_renderer_amd.cli import build_parser, plan_from_args
    argv = ["-i", "a", "-o", "b", "--size", "16x8", "--pix-fmt", kw["pix_fmt"], fam.out_flag, kw["out_pix_fmt"], fam.flag, kw["stages"]]
    argv += ["--cube", "x.cube"] if "lut3d" in _kinds(kw["stages"]) else []
    argv += ["--cdl-sat", "0.5"] if grade is not None else []
    argv += ["--zscale-dither", "error_diffusion"] if zscale != "none" else []
    argv += ["--engine-dither", engine_dither] if engine_dither else []
    argv += ["--out-size", "8x8"] if kw.get("out_size") else []
    argv += ["--chroma-loc", kw["chroma_loc"]] if kw.get("chroma_loc") else []
    argv += ["--strength", str(kw["strength"])] if kw.get("strength") is not None else []
    argv += ["--second-output", "c", "--second-pix-fmt", kw["out2_pix_fmt"]] if kw.get("out2_pix_fmt") else []
    return _message(lambda: plan_from_args(build_parser().parse_args(argv)))


def every_message():
    """What the pinned file holds: key -> "<exception type>: <message>"."""
    out = {}
    for family in FAMILIES:
        for kw in _rows(family):
            out[_key(family, "check", kw=kw)] = from_the_check(family, kw)
        for kw in LAYERED[family]:
            for layer in LAYERS:
                out[_key(family, layer, kw=kw)] = through(layer, family, kw)
    return out


def _pinned():
    return json.loads(PINNED.read_text(encoding="utf-8"))


_CHECK_ROWS = [(f, kw) for f in FAMILIES for kw in _rows(f)]
_LAYER_ROWS = [(f, layer, kw) for f in FAMILIES for kw in LAYERED[f] for layer in LAYERS]


@pytest.mark.parametrize("family,kw", _CHECK_ROWS, ids=[_key(f, kw=kw) for f, kw in _CHECK_ROWS])
def test_the_check_says_the_pinned_words(family, kw):
    want = _pinned()[_key(family, "check", kw=kw)]
    assert want is not None and want.startswith("ValueError: ")            # (every row is a refusal)
    assert from_the_check(family, kw) == want


@pytest.mark.parametrize("family,layer,kw", _LAYER_ROWS, ids=[_key(f, layer, kw=kw) for f, layer, kw in _LAYER_ROWS])
def test_every_layer_says_the_pinned_words(family, layer, kw):
    want = _pinned()[_key(family, layer, kw=kw)]
    assert want is not None and want.startswith("ValueError: ")
    assert through(layer, family, kw) == want


def test_the_pinned_file_holds_these_rows_and_no_others():
    assert sorted(_pinned()) == sorted(every_message())


if __name__ == "__main__":
    PINNED.write_text(json.dumps(every_message(), indent=1, sort_keys=True, ensure_ascii=False) + "\n", encoding="utf-8")
    print(f"wrote {len(every_message())} messages to {PINNED}")
