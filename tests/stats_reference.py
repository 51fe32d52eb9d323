"""numpy restatements of the whole-column reductions and of the quantile rule (include/gdf/gdf.h), shared by the CPU test that pins
the quantile rule to the reference's known answers and by the GPU tests of csrc/reduce.hip and csrc/quantile.hip."""
import math

import numpy as np

QUANTILE_METHODS = ("LINEAR", "LOWER", "HIGHER", "MIDPOINT", "NEAREST")


def _wrap(v, dtype):
    """a Python int wrapped into dtype's two's complement range"""
    bits = np.dtype(dtype).itemsize * 8
    v %= 1 << bits
    return v - (1 << bits) if v >= 1 << (bits - 1) else v


def _diff_sum(y0, y1):
    """y1 - y0 and y0 + y1 in the column type under C promotion (int8 / int16 -> int, int32 / int64 wrap, float32 stays float32)"""
    dt = np.dtype(type(y0))
    if dt.kind == "i":
        a, b = int(y0), int(y1)
        if dt.itemsize < 4:
            return float(b - a), float(a + b)
        return float(_wrap(b - a, dt)), float(_wrap(a + b, dt))
    with np.errstate(all="ignore"):
        return float(dt.type(y1) - dt.type(y0)), float(dt.type(y0) + dt.type(y1))


def quantile_rule(sorted_values, q, method=None):
    """The quantile of an ascending (NaN last) array: method None -> aprrox (an element, numpy scalar), else the exact
    method's double (method: name in QUANTILE_METHODS or its index)."""
    s = sorted_values
    n = len(s)
    if q >= 1.0 or n == 1:
        y = s[n - 1] if q >= 1.0 else s[0]
        return y if method is None else float(y)
    pos = q * float(n)
    k = int(math.floor(pos))
    x = pos - k
    if k > 0:
        k -= 1
    y0, y1 = s[k], s[k + 1]
    if method is None:
        return y0
    m = QUANTILE_METHODS[method] if isinstance(method, int) else method
    diff, tot = _diff_sum(y0, y1)
    if m == "LINEAR":
        return float(y0) + x * diff
    if m == "LOWER":
        return float(y0)
    if m == "HIGHER":
        return float(y1)
    if m == "MIDPOINT":
        return tot / 2.0
    return float(y0) if x < 0.5 else float(y1)


def same(a, b):
    """equal, or both NaN"""
    a, b = float(a), float(b)
    return a == b or (a != a and b != b)


def reduce_identity(op, dtype):
    dt = np.dtype(dtype)
    if op in ("sum", "sum_squared"):
        return dt.type(0)
    if op == "product":
        return dt.type(1)
    info = np.finfo(dt) if dt.kind == "f" else np.iinfo(dt)
    return dt.type(info.max) if op == "min" else dt.type(info.min)


def reduce_rule(op, values, valid=None):
    """The library's result for op over the valid elements of values (exact for integers and min / max; for float sums and
    products a value to compare with a tolerance)."""
    a = np.asarray(values)
    dt = a.dtype
    v = a if valid is None else a[np.asarray(valid, dtype=bool)]
    ident = reduce_identity(op, dt)
    with np.errstate(all="ignore"):
        if op in ("min", "max"):
            w = np.concatenate([v, np.array([ident], dtype=dt)])
            return (np.min if op == "min" else np.max)(w)
        if dt.kind == "i":
            x = v.astype(np.int64)
            tot = int(np.sum(x, dtype=np.int64)) if op == "sum" else int(np.prod(x, dtype=np.int64))
            return dt.type(_wrap(tot, dt))
        if op == "sum":
            return dt.type(np.sum(v.astype(np.float64)))
        if op == "sum_squared":
            return dt.type(np.sum(v.astype(np.float64) ** 2))
        return dt.type(np.prod(v.astype(np.float64)))
