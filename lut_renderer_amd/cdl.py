"""ASC CDL (slope, offset, power, saturation; ASC CDL v1.2) in front of the LUT: the value type and the reader of the three file
kinds a colour decision travels in.  No torch, no GPU: the numbers only.

    .cc   one <ColorCorrection>
    .ccc  a <ColorCorrectionCollection> of them
    .cdl  a <ColorDecisionList> of <ColorDecision>s, each holding one <ColorCorrection>

A correction is  out = clamp(in * slope + offset, 0, 1) ^ power  per channel, then  luma + saturation * (out - luma)  with
Rec.709 luma weights.  `LutEngine.apply_yuv(..., cdl=)` applies it to the integer RGB the LUT would see, ahead of the LUT.
"""
from __future__ import annotations

import math
import xml.etree.ElementTree as ET
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Sequence, Tuple, Union

_Triple = Tuple[float, float, float]


def _triple(values, what: str) -> _Triple:
    try:
        out = tuple(float(v) for v in values)
    except (TypeError, ValueError):
        raise ValueError(f"CDL {what} must be three numbers, got {values!r}") from None
    if len(out) != 3:
        raise ValueError(f"CDL {what} must be three numbers, got {len(out)}")
    return out


@dataclass(frozen=True)
class Cdl:
    """One colour correction.  slope >= 0, power > 0, saturation >= 0, all ten numbers finite (ValueError otherwise)."""
    slope: _Triple = (1.0, 1.0, 1.0)
    offset: _Triple = (0.0, 0.0, 0.0)
    power: _Triple = (1.0, 1.0, 1.0)
    saturation: float = 1.0

    def __post_init__(self):
        for name in ("slope", "offset", "power"):
            object.__setattr__(self, name, _triple(getattr(self, name), name))
        try:
            object.__setattr__(self, "saturation", float(self.saturation))
        except (TypeError, ValueError):
            raise ValueError(f"CDL saturation must be a number, got {self.saturation!r}") from None
        for name in ("slope", "offset", "power"):
            for c, v in zip("RGB", getattr(self, name)):
                if not math.isfinite(v):
                    raise ValueError(f"CDL {name} of {c} is not finite ({v})")
        if not math.isfinite(self.saturation):
            raise ValueError(f"CDL saturation is not finite ({self.saturation})")
        for c, v in zip("RGB", self.slope):
            if v < 0:
                raise ValueError(f"CDL slope of {c} is negative ({v})")
        for c, v in zip("RGB", self.power):
            if not v > 0:
                raise ValueError(f"CDL power of {c} must be above 0 ({v})")
        if self.saturation < 0:
            raise ValueError(f"CDL saturation is negative ({self.saturation})")

    @classmethod
    def identity(cls) -> "Cdl":
        return cls()

    @property
    def is_identity(self) -> bool:
        return self == Cdl()

    def sop_text(self) -> str:
        """The nine slope / offset / power numbers as `--cdl-sop` takes them; repr round-trips a float exactly."""
        return " ".join(repr(v) for v in (*self.slope, *self.offset, *self.power))

    @classmethod
    def from_sop_text(cls, sop: Optional[str], saturation=None) -> "Cdl":
        """A Cdl from `--cdl-sop "s s s o o o p p p"` and `--cdl-sat X`; either may be None (identity)."""
        vals = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
        if sop is not None:
            parts = str(sop).replace(",", " ").split()
            if len(parts) != 9:
                raise ValueError(f"--cdl-sop takes nine numbers (slope R G B, offset R G B, power R G B), got {len(parts)}")
            try:
                vals = tuple(float(p) for p in parts)
            except ValueError:
                raise ValueError(f"--cdl-sop takes nine numbers, got {sop!r}") from None
        return cls(vals[0:3], vals[3:6], vals[6:9], 1.0 if saturation is None else saturation)


def as_cdl(cdl: Union[None, Cdl, str, Path], cc_id: Optional[str] = None) -> Optional[Cdl]:
    """What the public entry points make of their `cdl` argument: None, a Cdl, or the path of a .cc / .ccc / .cdl file."""
    if cdl is None or isinstance(cdl, Cdl):
        return cdl
    if isinstance(cdl, (str, Path)):
        return read_cdl(cdl, cc_id)
    raise TypeError(f"cdl must be a Cdl or the path of a .cc / .ccc / .cdl file, not {type(cdl).__name__}")


# ---------------------------------------------------------------- files
def _local(tag: str) -> str:
    return tag.rsplit("}", 1)[-1] if isinstance(tag, str) else ""


def _namespace_ok(tag: str) -> bool:
    """No namespace, or any urn:ASC:CDL:* one (v1.01, v1.2, ...)."""
    if not isinstance(tag, str) or not tag.startswith("{"):
        return True
    return tag[1:].split("}", 1)[0].startswith("urn:ASC:CDL:")


def _child(node, name: str):
    return [c for c in node if _local(c.tag) == name]


def _numbers(node, n: int, what: str, path) -> Sequence[float]:
    parts = (node.text or "").split()
    if len(parts) != n:
        raise ValueError(f"{path}: <{what}> holds {len(parts)} number{'s' if len(parts) != 1 else ''}, expected {n}")
    try:
        return [float(p) for p in parts]
    except ValueError:
        raise ValueError(f"{path}: <{what}> holds '{node.text.strip()}', not {n} number{'s' if n != 1 else ''}") from None


def _one(node, name: str, path, inside: str):
    found = _child(node, name)
    if len(found) > 1:
        raise ValueError(f"{path}: more than one <{name}> in <{inside}>")
    return found[0] if found else None


def _correction(cc, path) -> Cdl:
    slope, offset, power, sat = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1.0
    sop = _one(cc, "SOPNode", path, "ColorCorrection")
    if sop is not None:
        for name in ("Slope", "Offset", "Power"):
            node = _one(sop, name, path, "SOPNode")
            if node is None:
                continue
            vals = tuple(_numbers(node, 3, name, path))
            if name == "Slope":
                slope = vals
            elif name == "Offset":
                offset = vals
            else:
                power = vals
    satnode = _one(cc, "SatNode", path, "ColorCorrection")
    if satnode is not None:
        node = _one(satnode, "Saturation", path, "SatNode")
        if node is not None:
            sat = _numbers(node, 1, "Saturation", path)[0]
    try:
        return Cdl(slope, offset, power, sat)
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None


def read_cdl(path, cc_id: Optional[str] = None) -> Cdl:
    """The colour correction of a .cc, .ccc or .cdl file (told by the root element, not the suffix).  `cc_id` selects by the
    `id` attribute of <ColorCorrection>; None takes the only correction of the file and is an error when it holds several.
    Any urn:ASC:CDL:* namespace or none is accepted; <SOPNode> and <SatNode> are each optional and default to identity.
    ValueError names the file and what is wrong with it."""
    try:
        root = ET.parse(str(path)).getroot()
    except ET.ParseError as e:
        raise ValueError(f"{path}: not an XML file ({e})") from None
    except OSError as e:
        raise ValueError(f"{path}: cannot read ({e.strerror or e})") from None
    if not _namespace_ok(root.tag):
        raise ValueError(f"{path}: the root element's namespace is not an ASC CDL one (urn:ASC:CDL:*)")
    kind = _local(root.tag)
    if kind == "ColorCorrection":
        ccs = [root]
    elif kind == "ColorCorrectionCollection":
        ccs = _child(root, "ColorCorrection")
    elif kind == "ColorDecisionList":
        ccs = [cc for cd in _child(root, "ColorDecision") for cc in _child(cd, "ColorCorrection")]
    else:
        raise ValueError(f"{path}: the root element is <{kind}>, not ColorCorrection (.cc), ColorCorrectionCollection (.ccc) or "
                         f"ColorDecisionList (.cdl)")
    if not ccs:
        raise ValueError(f"{path}: no <ColorCorrection> in it")
    if cc_id is not None:
        match = [cc for cc in ccs if cc.get("id") == cc_id]
        if not match:
            ids = ", ".join(repr(cc.get("id")) for cc in ccs if cc.get("id") is not None) or "none"
            raise ValueError(f"{path}: no <ColorCorrection> with id '{cc_id}' (ids in the file: {ids})")
        if len(match) > 1:
            raise ValueError(f"{path}: {len(match)} corrections share the id '{cc_id}'")
        return _correction(match[0], path)
    if len(ccs) > 1:
        ids = ", ".join(repr(cc.get("id")) for cc in ccs)
        raise ValueError(f"{path}: {len(ccs)} corrections in the file ({ids}); name one with cc_id / --cdl-id")
    return _correction(ccs[0], path)
