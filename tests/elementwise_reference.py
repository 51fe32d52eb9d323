"""numpy restatements of the element-wise operators' rules (include/gdf/gdf.h), shared by the CPU test that pins the datetime and
cast rules to the reference's known answers and to numpy.datetime64, and by the GPU tests of csrc/elementwise.hip."""
import numpy as np

# gdf_dtype / gdf_time_unit values (include/gdf/gdf.h)
INT8, INT16, INT32, INT64, FLOAT32, FLOAT64, DATE32, DATE64, TIMESTAMP = 1, 2, 3, 4, 5, 6, 7, 8, 9
UNIT_NONE, UNIT_S, UNIT_MS, UNIT_US, UNIT_NS = 0, 1, 2, 3, 4
UNIT_NAMES = {"s": UNIT_S, "ms": UNIT_MS, "us": UNIT_US, "ns": UNIT_NS}
STORAGE = {INT8: np.int8, INT16: np.int16, INT32: np.int32, INT64: np.int64, FLOAT32: np.float32, FLOAT64: np.float64,
           DATE32: np.int32, DATE64: np.int64, TIMESTAMP: np.int64}
SUFFIX_DTYPE = dict(i8=INT8, i32=INT32, i64=INT64, f32=FLOAT32, f64=FLOAT64, date32=DATE32, date64=DATE64, timestamp=TIMESTAMP)
SUFFIX_NP = dict(i8=np.int8, i32=np.int32, i64=np.int64, f32=np.float32, f64=np.float64)

ARITH_OPS = ("add", "sub", "mul", "floordiv")
COMPARE_OPS = ("gt", "ge", "lt", "le", "eq", "ne")
BITWISE_OPS = ("bitwise_and", "bitwise_or", "bitwise_xor")
BINARY_SUFFIXES = {**{op: ("i32", "i64", "f32", "f64") for op in ARITH_OPS}, "div": ("f32", "f64"),
                   **{op: ("i8", "i32", "i64", "f32", "f64") for op in COMPARE_OPS},
                   **{op: ("i8", "i32", "i64") for op in BITWISE_OPS}}
MATH_OPS = ("sin", "cos", "tan", "asin", "acos", "atan", "exp", "log", "sqrt", "ceil", "floor")
EXACT_MATH_OPS = ("sqrt", "ceil", "floor")
MATH_NP = dict(sin=np.sin, cos=np.cos, tan=np.tan, asin=np.arcsin, acos=np.arccos, atan=np.arctan, exp=np.exp, log=np.log,
               sqrt=np.sqrt, ceil=np.ceil, floor=np.floor)
DATETIME_FIELDS = ("year", "month", "day", "hour", "minute", "second")
CAST_SOURCES = ("i8", "i32", "i64", "f32", "f64", "date32", "date64", "timestamp")
CAST_TARGETS = ("f32", "f64", "i8", "i32", "i64", "date32", "date64", "timestamp")


def binary(op, a, b):
    """The expected data of gdf_<op>_<type>(a, b) where it is specified (integer floordiv: rhs != 0 and not INT_MIN / -1)."""
    with np.errstate(all="ignore"):
        if op == "add":
            return a + b                              # numpy integer arrays wrap
        if op == "sub":
            return a - b
        if op == "mul":
            return a * b
        if op == "div":
            return a / b
        if op == "floordiv":
            if a.dtype.kind == "f":
                return np.floor(a / b)                # floor of the ROUNDED quotient, in the column type
            safe = np.where(b == 0, 1, b)
            return np.floor_divide(a, safe)           # exact floor division
        if op in COMPARE_OPS:
            f = dict(gt=np.greater, ge=np.greater_equal, lt=np.less, le=np.less_equal, eq=np.equal, ne=np.not_equal)[op]
            return f(a, b).astype(np.int8)
        return dict(bitwise_and=np.bitwise_and, bitwise_or=np.bitwise_or, bitwise_xor=np.bitwise_xor)[op](a, b)


def floordiv_specified(a, b):
    """rows of an integer floordiv whose value the interface specifies"""
    return (b != 0) & ~((a == np.iinfo(a.dtype).min) & (b == -1))


def ticks_per_day(dtype, unit):
    """ticks per day of a date / time type; 0: not one, or TIME_UNIT_NONE"""
    if dtype == DATE32:
        return 1
    if dtype == DATE64:
        return 86400 * 1000
    if dtype == TIMESTAMP:
        return {UNIT_S: 86400, UNIT_MS: 86400 * 10**3, UNIT_US: 86400 * 10**6, UNIT_NS: 86400 * 10**9}.get(unit, 0)
    return 0


def cast(values, from_dtype, from_unit, to_dtype, to_unit):
    """The expected data of a cast: between two date / time types of different resolution a wrapping multiplication (towards the
    finer one) or a floor division (towards the coarser one), otherwise the C conversion (float -> integer: in-range values)."""
    out = np.dtype(STORAGE[to_dtype])
    ft, tt = ticks_per_day(from_dtype, from_unit), ticks_per_day(to_dtype, to_unit)
    with np.errstate(all="ignore"):
        if ft and tt and ft != tt:
            v = values.astype(np.int64)
            r = v * np.int64(tt // ft) if tt > ft else np.floor_divide(v, np.int64(ft // tt))
            return r.astype(out)                      # int64 -> int32 truncates
        if values.dtype.kind == "f" and out.kind == "i":
            return np.trunc(values).astype(np.int64).astype(out) if out.itemsize < 8 else values.astype(out)
        return values.astype(out)


def float_to_int_specified(values, to_dtype):
    """rows of a float -> integer cast whose value the interface specifies: finite and inside the target's range after truncation"""
    info = np.iinfo(STORAGE[to_dtype])
    with np.errstate(all="ignore"):
        t = np.trunc(values.astype(np.float64))
        return np.isfinite(values) & (t >= float(info.min)) & (t < float(info.max) + 1.0)


def _civil(days):
    """(year, month, day) of day numbers since 1970-01-01, proleptic Gregorian, in Python / numpy integer arithmetic"""
    z = days.astype(np.int64) + 719468
    era = np.floor_divide(z, 146097)
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    d = doy - (153 * mp + 2) // 5 + 1
    m = np.where(mp < 10, mp + 3, mp - 9)
    return yoe + era * 400 + (m <= 2), m, d


def datetime_field(field, values, dtype, unit=UNIT_NONE):
    """The expected int16 data of gdf_extract_datetime_<field>: floor semantics on both sides of the epoch; TIME_UNIT_NONE counts
    as ms; the year is truncated to int16."""
    v = values.astype(np.int64)
    if dtype == DATE32:
        days, tps = v, None
    else:
        tps = {UNIT_S: 1, UNIT_US: 10**6, UNIT_NS: 10**9}.get(unit if dtype == TIMESTAMP else UNIT_MS, 10**3)
        days = np.floor_divide(v, 86400 * tps)
    if field in ("year", "month", "day"):
        y, m, d = _civil(days)
        return dict(year=y, month=m, day=d)[field].astype(np.int16)
    assert tps is not None, "DATE32 has no time of day"
    if field == "hour":
        return (np.mod(v, 86400 * tps) // (3600 * tps)).astype(np.int16)
    if field == "minute":
        return (np.mod(v, 3600 * tps) // (60 * tps)).astype(np.int16)
    return (np.mod(v, 60 * tps) // tps).astype(np.int16)


def datetime_field_numpy(field, values, np_unit):
    """The same field from numpy.datetime64 (np_unit 'D', 's', 'ms', 'us' or 'ns'): the independent yardstick."""
    t = values.astype(np.int64).astype(f"datetime64[{np_unit}]")
    if field == "year":
        return (t.astype("datetime64[Y]").astype(np.int64) + 1970).astype(np.int16)
    if field == "month":
        return (t.astype("datetime64[M]").astype(np.int64) % 12 + 1).astype(np.int16)
    if field == "day":
        return ((t.astype("datetime64[D]") - t.astype("datetime64[M]").astype("datetime64[D]")).astype(np.int64) + 1).astype(np.int16)
    coarse = dict(hour="h", minute="m", second="s")[field]
    per = dict(hour=24, minute=60, second=60)[field]
    return (t.astype(f"datetime64[{coarse}]").astype(np.int64) % per).astype(np.int16)
