"""The RGB matrix stage of the stage stack: the value type and the reader of the `.spimtx` file a matrix
travels in.  No torch, no GPU: the numbers only.

A matrix stage is  out = clamp(M * in + offset, 0, 1)  on unit RGB: row 0 of M gives R', row 1 G', row 2 B', from (R, G, B).
`LutEngine.apply_yuv_stack(..., stages="lut1d,matrix,lut3d", rgb_matrix=)` runs it where the list places it.

    .spimtx   twelve numbers, row-major 3 x 4: three rows of (m0 m1 m2 offset), the offset column in 16-bit codes (divided by
              65535 here, as OpenColorIO reads the format)
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from pathlib import Path
from typing import Optional, Tuple, Union

#: the largest magnitude of an entry: every sum of the stage stays finite in float32
MAX_ENTRY = 65536.0
_Nine = Tuple[float, float, float, float, float, float, float, float, float]
_Triple = Tuple[float, float, float]


def _numbers(values, n: int, what: str):
    try:
        if len(values) == 3 and n == 9 and all(hasattr(row, "__len__") and not isinstance(row, str) for row in values):
            values = [v for row in values for v in row]             # three rows of three
        out = tuple(float(v) for v in values)
    except (TypeError, ValueError):
        raise ValueError(f"RGB matrix {what} must be {n} numbers, got {values!r}") from None
    if len(out) != n:
        raise ValueError(f"RGB matrix {what} must be {n} numbers, got {len(out)}")
    return out


@dataclass(frozen=True)
class RgbMatrix:
    """A 3x3 matrix, row-major (nine numbers or three rows of three), and an offset in unit floats.  All twelve numbers finite and
    at most 65536 in magnitude (ValueError otherwise)."""
    m: _Nine = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    offset: _Triple = (0.0, 0.0, 0.0)

    def __post_init__(self):
        object.__setattr__(self, "m", _numbers(self.m, 9, "m"))
        object.__setattr__(self, "offset", _numbers(self.offset, 3, "offset"))
        for name, vals in (("m", self.m), ("offset", self.offset)):
            for i, v in enumerate(vals):
                if not math.isfinite(v):
                    raise ValueError(f"RGB matrix {name}[{i}] is not finite ({v})")
                if abs(v) > MAX_ENTRY:
                    raise ValueError(f"RGB matrix {name}[{i}] is above 65536 in magnitude ({v})")

    @classmethod
    def identity(cls) -> "RgbMatrix":
        return cls()

    @property
    def is_identity(self) -> bool:
        return self == RgbMatrix()

    def m_text(self) -> str:
        """The nine numbers as `--rgb-matrix` takes them; repr round-trips a float exactly."""
        return " ".join(repr(v) for v in self.m)

    def offset_text(self) -> str:
        """The three numbers as `--rgb-matrix-offset` takes them."""
        return " ".join(repr(v) for v in self.offset)

    @classmethod
    def from_text(cls, m: Optional[str], offset: Optional[str] = None) -> "RgbMatrix":
        """An RgbMatrix from `--rgb-matrix "9 numbers"` and `--rgb-matrix-offset "3 numbers"`; either may be None (identity / 0)."""
        out = []
        for text, n, flag, default in ((m, 9, "--rgb-matrix", RgbMatrix().m), (offset, 3, "--rgb-matrix-offset", (0.0, 0.0, 0.0))):
            if text is None:
                out.append(default)
                continue
            parts = str(text).replace(",", " ").split()
            if len(parts) != n:
                raise ValueError(f"{flag} takes {n} numbers, got {len(parts)}")
            try:
                out.append(tuple(float(p) for p in parts))
            except ValueError:
                raise ValueError(f"{flag} takes {n} numbers, got {text!r}") from None
        return cls(out[0], out[1])


def as_rgb_matrix(mtx: Union[None, RgbMatrix, str, Path]) -> Optional[RgbMatrix]:
    """What the public entry points make of their `rgb_matrix` argument: None, an RgbMatrix, or the path of a .spimtx file."""
    if mtx is None or isinstance(mtx, RgbMatrix):
        return mtx
    if isinstance(mtx, (str, Path)):
        return read_rgb_matrix(mtx)
    raise TypeError(f"rgb_matrix must be an RgbMatrix or the path of a .spimtx file, not {type(mtx).__name__}")


def read_rgb_matrix(path) -> RgbMatrix:
    """The matrix of a .spimtx file: twelve numbers separated by white space, row-major 3 x 4; the fourth column is the offset
    in 16-bit codes and is divided by 65535.  ValueError names the file and what is wrong with it."""
    try:
        text = Path(path).read_text()
    except UnicodeDecodeError:
        raise ValueError(f"{path}: not a text file") from None
    except OSError as e:
        raise ValueError(f"{path}: cannot read ({e.strerror or e})") from None
    parts = text.split()
    if len(parts) != 12:
        raise ValueError(f"{path}: holds {len(parts)} number{'s' if len(parts) != 1 else ''}, expected 12 (three rows of m0 m1 m2 offset)")
    vals = []
    for i, p in enumerate(parts):
        try:
            vals.append(float(p))
        except ValueError:
            raise ValueError(f"{path}: entry {i + 1} is '{p}', not a number") from None
    rows = [vals[0:4], vals[4:8], vals[8:12]]
    try:
        return RgbMatrix([v for row in rows for v in row[:3]], [row[3] / 65535.0 for row in rows])
    except ValueError as e:
        raise ValueError(f"{path}: {e}") from None
