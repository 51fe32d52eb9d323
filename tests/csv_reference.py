"""A pure Python restatement of the read_csv contract of include/gdf/gdf.h (written from that text, not from csrc/csv.hip): datetime for
the calendar, float() for the floats, a byte-range MurmurHash3 of its own.  read() returns, per column, what the library must
return: the data array (0 at a null), the mask bytes (LSB first, ceil(rows / 8) of them, spare bits 0) and the null count."""
import datetime
import math
import re

import numpy as np

DTYPE_OF = {"str": 10, "category": 10, "date": 8, "date64": 8, "date32": 7, "timestamp": 9, "float": 5, "float32": 5, "float64": 6,
            "double": 6, "short": 2, "int": 3, "int32": 3, "int64": 4, "long": 4}
NP_OF = {2: np.int16, 3: np.int32, 4: np.int64, 5: np.float32, 6: np.float64, 7: np.int32, 8: np.int64, 9: np.int64, 10: np.int32}
INT_RANGE = {2: (-2**15, 2**15 - 1), 3: (-2**31, 2**31 - 1), 4: (-2**63, 2**63 - 1), 9: (-2**63, 2**63 - 1)}
HASH_SEED = 33
FLOAT_ULP_BOUND = 7                     # gdf.h, floats: outside the fast domain

_INT = re.compile(rb"[+-]?[0-9]+(?:,[0-9]+)*")
_FLOAT = re.compile(rb"([+-]?)(?:([0-9]+(?:,[0-9]+)*)(?:\.([0-9]*))?|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?")
_DATE_YMD = re.compile(rb"([0-9]{4})([/-])([0-9]{1,2})(?:\2([0-9]{1,2}))?")
_DATE_XXY = re.compile(rb"([0-9]{1,2})([/-])([0-9]{1,2})\2([0-9]{4})")
_DATE_MY = re.compile(rb"([0-9]{1,2})([/-])([0-9]{4})")
_TIME = re.compile(rb"[T ]([0-9]{1,2}):([0-9]{1,2})(?::([0-9]{1,2}))?(?: ?([AaPp])[Mm])?")


def murmur3(data: bytes, seed: int) -> int:
    """MurmurHash3 x86_32 of the bytes, as an unsigned 32-bit value"""
    M = 0xffffffff
    rotl = lambda x, r: ((x << r) | (x >> (32 - r))) & M          # noqa: E731

    def scramble(k):
        return (rotl((k * 0xcc9e2d51) & M, 15) * 0x1b873593) & M

    h = seed & M
    body = len(data) // 4 * 4
    for i in range(0, body, 4):
        h ^= scramble(int.from_bytes(data[i:i + 4], "little"))
        h = (rotl(h, 13) * 5 + 0xe6546b64) & M
    if len(data) > body:
        h ^= scramble(int.from_bytes(data[body:], "little"))
    h ^= len(data) & M
    h ^= h >> 16
    h = (h * 0x85ebca6b) & M
    h ^= h >> 13
    h = (h * 0xc2b2ae35) & M
    return h ^ (h >> 16)


def parse_int(field: bytes, dtype: int):
    if not _INT.fullmatch(field):
        return None
    v = int(field.replace(b",", b""))
    lo, hi = INT_RANGE[dtype]
    return v if lo <= v <= hi else None


def float_parts(field: bytes):
    """(m, e) of gdf.h -- the first 19 significant digits and the decimal exponent -- or None when the field is no float literal"""
    g = _FLOAT.fullmatch(field)
    if not g:
        return None
    whole = (g.group(2) or b"").replace(b",", b"")
    frac = g.group(3) if g.group(2) is not None else g.group(4)
    frac = frac or b""
    digits = (whole + frac).lstrip(b"0")
    e = -len(frac) + int(g.group(5) or 0)
    if len(digits) > 19:
        e += len(digits) - 19
        digits = digits[:19]
    return int(digits or b"0"), e


def in_fast_domain(field: bytes) -> bool:
    m, e = float_parts(field)
    return m < 2**53 and abs(e) <= 22


def parse_float(field: bytes):
    if float_parts(field) is None:
        return None
    return float(field.replace(b",", b"").decode())              # correctly rounded; overflow gives inf, "-0" gives -0.0


def parse_date(field: bytes, dayfirst: bool, with_time: bool):
    """(days, milliseconds) since 1970-01-01, or None"""
    day = 1
    g = _DATE_YMD.match(field)
    if g:
        year, month = int(g.group(1)), int(g.group(3))
        if g.group(4) is not None:
            day = int(g.group(4))
    else:
        g = _DATE_XXY.match(field)
        if g:
            a, b, year = int(g.group(1)), int(g.group(3)), int(g.group(4))
            month, day = (b, a) if dayfirst else (a, b)
        else:
            g = _DATE_MY.match(field)
            if not g:
                return None
            month, year = int(g.group(1)), int(g.group(3))
    try:
        days = (datetime.date(year, month, day) - datetime.date(1970, 1, 1)).days            # year 1 .. 9999, the Gregorian rule
    except ValueError:
        return None
    rest = field[g.end():]
    seconds = 0
    if rest:
        t = _TIME.fullmatch(rest) if with_time else None
        if not t:
            return None
        hour, minute, second = int(t.group(1)), int(t.group(2)), int(t.group(3) or 0)
        if t.group(4) is not None:
            if not 1 <= hour <= 12:
                return None
            hour = hour % 12 + (12 if t.group(4) in b"Pp" else 0)
        if hour > 23 or minute > 59 or second > 59:
            return None
        seconds = hour * 3600 + minute * 60 + second
    return days, days * 86400000 + seconds * 1000


def parse_field(field, dtype: int, skipinitialspace=False, dayfirst=False):
    """the element of a field of a column of `dtype`, None for a null (a missing field is None already)"""
    if field is None:
        return None
    if dtype == 10:
        if skipinitialspace:
            field = field.lstrip(b" ")
        if not field:
            return None
        h = murmur3(field, HASH_SEED)
        return h - 2**32 if h >= 2**31 else h
    field = field.strip(b" ")
    if not field:
        return None
    if dtype in INT_RANGE:
        return parse_int(field, dtype)
    if dtype in (5, 6):
        return parse_float(field)
    d = parse_date(field, dayfirst, with_time=dtype == 8)
    return None if d is None else d[0 if dtype == 7 else 1]


def records(data: bytes, lineterminator=b"\n", skiprows=0, skipfooter=0):
    recs = data.split(lineterminator)
    if not recs[-1]:
        recs.pop()                                              # nothing behind the last terminator (or no bytes at all)
    if lineterminator == b"\n":
        recs = [r[:-1] if r.endswith(b"\r") else r for r in recs]
    return recs[skiprows:len(recs) - skipfooter] if len(recs) - skiprows - skipfooter > 0 else []


def read(data: bytes, dtypes, delimiter=b",", lineterminator=b"\n", delim_whitespace=False, skipinitialspace=False, skiprows=0,
         skipfooter=0, dayfirst=False):
    """[(data array, mask bytes as uint8 array, null_count)] per column"""
    codes = [DTYPE_OF[d] for d in dtypes]
    delim = b" " if delim_whitespace else delimiter
    recs = [r.split(delim) for r in records(data, lineterminator, skiprows, skipfooter)]
    out = []
    for c, dtype in enumerate(codes):
        vals = [parse_field(r[c] if c < len(r) else None, dtype, skipinitialspace, dayfirst) for r in recs]
        valid = np.array([v is not None for v in vals], dtype=bool)
        with np.errstate(over="ignore"):
            arr = np.array([0 if v is None else v for v in vals], dtype=np.float64 if dtype == 5 else NP_OF[dtype]).astype(NP_OF[dtype])
        out.append((arr, np.packbits(valid, bitorder="little"), int((~valid).sum())))
    return out


def ulps_apart(a: float, b: float) -> float:
    """|a - b| in ulps of b; 0 for two equal values (infinities and zeros of one sign included)"""
    if a == b and math.copysign(1, a) == math.copysign(1, b):
        return 0.0
    if math.isinf(a) or math.isinf(b):
        return math.inf
    return abs(a - b) / math.ulp(b)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
