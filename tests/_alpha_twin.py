"""The alpha plane's arithmetic restated in NumPy: the integer depth change in int64, the float quantiser in
float32, the fill.  Written from the contract, not from the kernels."""
import numpy as np

DEPTHS = (8, 9, 10, 12, 14, 16)


def convert(words, din: int, dout: int) -> np.ndarray:
    """a = min(word, Mi); a' = floor((2 a Mo + Mi) / (2 Mi)); the words themselves at equal depth."""
    w = np.asarray(words).astype(np.int64)
    if din == dout:
        return w
    mi, mo = (1 << din) - 1, (1 << dout) - 1
    a = np.minimum(w, mi)
    return (2 * a * mo + mi) // (2 * mi)


def convert_double(words, din: int, dout: int) -> np.ndarray:
    """floor(a * Mo / (double)Mi + 0.5)"""
    mi, mo = (1 << din) - 1, (1 << dout) - 1
    a = np.minimum(np.asarray(words).astype(np.int64), mi).astype(np.float64)
    return np.floor(a * np.float64(mo) / np.float64(mi) + 0.5).astype(np.int64)


def convert_fp32(words, din: int, dout: int) -> np.ndarray:
    """The same expression with every operation in fp32 -- what the contract rules out."""
    mi, mo = (1 << din) - 1, (1 << dout) - 1
    a = np.minimum(np.asarray(words).astype(np.int64), mi).astype(np.float32)
    return np.floor(a * np.float32(mo) / np.float32(mi) + np.float32(0.5)).astype(np.int64)


def quantise(a, dout: int) -> np.ndarray:
    """q = clip(rintf(a * (float)Mo), 0, Mo): one fp32 multiply, round half to even, NaN -> 0."""
    a = np.asarray(a, np.float32)
    mo = np.float32((1 << dout) - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.rint(np.where(np.isnan(a), np.float32(0), a) * mo)
    return np.clip(v, np.float32(0), mo).astype(np.int64)


def fill(shape, dout: int) -> np.ndarray:
    return np.full(shape, (1 << dout) - 1, np.int64)
