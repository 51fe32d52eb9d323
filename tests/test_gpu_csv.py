"""-m gpu: read_csv (csrc/csv.hip) through the raw C ABI against the Python model of its contract (tests/csv_reference.py).  Integers,
categories, dates, masks (byte for byte), the data at null positions and null_count are compared exactly; floats bit for bit inside
the fast domain of include/gdf/gdf.h and within its stated ulp bound outside.

The bytes go in through gdf_amd_read_csv_device, 0 .. 15 bytes into a larger tensor whose surroundings are terminator and delimiter
bytes: a read outside the range changes the record count or a value instead of faulting.  Every case runs a second time with
GDF_CSV_NO_STAGE forced (every tile walks global memory instead of its LDS image) and must give the same bytes."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import csv_reference as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ["staged", "unstaged"]
GUARD = 48                                       # poison bytes on either side of the file's bytes


def noted(gdf, name):
    v = C.c_longlong(-1)
    assert gdf.libgdf.gdf_amd_debug_noted(name.encode(), C.byref(v)) == 0, name
    return v.value


def _poisoned(data: bytes, offset: int, term: bytes, delim: bytes):
    host = np.frombuffer((term + delim) * ((GUARD + 16 + len(data) + GUARD) // 2 + 1), dtype=np.uint8)[: GUARD + 16 + len(data) + GUARD].copy()
    host[GUARD + offset: GUARD + offset + len(data)] = np.frombuffer(data, dtype=np.uint8)
    return host


class Read:
    """one call through the raw C ABI: rc and, on success, host copies of every column as (data, mask bytes, null_count)"""

    def __init__(self, gdf, data: bytes, dtypes, offset=0, path=None, names=None, **opts):
        import torch
        from libgdf_amd import api
        names = [f"c{i}" for i in range(len(dtypes))] if names is None else names
        kw = {k: (v.decode("latin-1") if isinstance(v, bytes) else v) for k, v in opts.items()}
        a = api.csv_args(names, dtypes, path=path, **kw)
        C.memset(C.byref(a), 0xAB, 16)                                         # the three output fields
        poisoned = bytes(a)[:16]
        if path is None:
            term, delim = opts.get("lineterminator", b"\n"), b" " if opts.get("delim_whitespace") else opts.get("delimiter", b",")
            host = _poisoned(data, offset, term, delim)
            dev = torch.from_numpy(host).cuda()
            assert dev.data_ptr() % 16 == 0 and GUARD % 16 == 0
            self.rc = gdf.libgdf.raw("gdf_amd_read_csv_device")(dev.data_ptr() + GUARD + offset, len(data), C.byref(a))
            assert np.array_equal(dev.cpu().numpy(), host)                     # the input is not written
        else:
            self.rc = gdf.libgdf.raw("read_csv")(C.byref(a))
        if self.rc != 0:
            assert bytes(a)[:16] == poisoned
            return
        self.rows = int(a.num_rows_out)
        assert a.num_cols_out == len(dtypes) and a.data
        self.fields = []
        for c in range(len(dtypes)):
            col = a.data[c].contents
            self.fields.append((col.col_name.decode(), int(col.dtype), int(col.size), bool(col.data), bool(col.valid),
                                int(col.dtype_info.time_unit)))
        taken = api.take_csv_result(a)                                         # copies, then gdf_amd_read_csv_release
        assert (a.num_cols_out, a.num_rows_out, bool(a.data)) == (0, 0, False)
        assert list(taken) == list(names)
        self.cols = [(d.cpu().numpy(), m.cpu().numpy(), n) for d, m, n in taken.values()]

    def raw_bytes(self):
        return [(d.tobytes(), m.tobytes(), n) for d, m, n in self.cols]


def compare(got: Read, data: bytes, dtypes, **opts):
    """everything `got` returned against the model"""
    assert got.rc == 0
    want = ref.read(data, dtypes, **opts)
    rows = len(want[0][0])
    assert got.rows == rows
    delim = b" " if opts.get("delim_whitespace") else opts.get("delimiter", b",")
    recs = ref.records(data, opts.get("lineterminator", b"\n"), opts.get("skiprows", 0), opts.get("skipfooter", 0))
    for c, ((gd, gm, gn), (wd, wm, wn)) in enumerate(zip(got.cols, want)):
        name, dtype, size, has_data, has_valid, unit = got.fields[c]
        code = ref.DTYPE_OF[dtypes[c]]
        assert (dtype, size, has_data, has_valid, unit) == (code, rows, rows > 0, rows > 0, 0), (c, got.fields[c])
        assert gm.tobytes() == wm.tobytes(), f"mask of column {c}"
        assert gn == wn, f"null_count of column {c}"
        assert gd.dtype == wd.dtype and len(gd) == rows
        if code == 5:                                                          # FLOAT32: exactly (float) of the model's double
            bad = np.flatnonzero(ref.bits_of(gd) != ref.bits_of(wd))
            assert len(bad) == 0, f"column {c} rows {bad[:5]}: {gd[bad[:5]]!r}, (float) of float() gives {wd[bad[:5]]!r}"
            continue
        if code != 6:
            assert np.array_equal(gd, wd), f"column {c}"
            continue
        valid = np.unpackbits(wm, bitorder="little")[:rows].astype(bool)
        for r in np.flatnonzero(ref.bits_of(gd) != ref.bits_of(wd)):            # only the rows that differ need a reason
            assert valid[r], f"column {c} row {r}: data at a null"
            field = recs[r].split(delim)[c].strip(b" ")
            assert not ref.in_fast_domain(field), f"column {c} row {r}: {field!r} gave {gd[r]!r}, float() gives {wd[r]!r}"
            u = ref.ulps_apart(float(gd[r]), float(wd[r]))
            assert u <= ref.FLOAT_ULP_BOUND, f"column {c} row {r}: {field!r} is {u} ulp from float()"
    return got


def check(gdf, force_path, route, data, dtypes, offset=0, names=None, **opts):
    force_path("GDF_CSV_NO_STAGE", "1" if route == "unstaged" else None)
    got = compare(Read(gdf, data, dtypes, offset=offset, names=names, **opts), data, dtypes, **opts)
    tiles = -(-got.rows // noted(gdf, "csv.rows_per_tile"))
    if route == "unstaged":
        assert noted(gdf, "csv.unstaged_tiles") == tiles
    return got


def tile_rows(gdf):
    Read(gdf, b"1\n", ["int"])
    R = noted(gdf, "csv.rows_per_tile")
    assert R >= 64 and R % 64 == 0
    return R


def mixed_rows(rng, rows, delim=b","):
    """int64, float64, category, date, short: about one field in eight is empty or no literal"""
    out = []
    for r in range(rows):
        f = [str(rng.randint(-10**12, 10**12)), repr(round(rng.standard_normal() * 10.0 ** rng.randint(-5, 6), rng.randint(0, 9))),
             "".join(chr(rng.randint(97, 123)) for _ in range(rng.randint(1, 12))),
             f"{rng.randint(1900, 2100)}-{rng.randint(1, 13):02d}-{rng.randint(1, 29):02d}", str(rng.randint(-40000, 40000))]
        for i in range(5):
            k = rng.randint(0, 16)
            f[i] = "" if k == 0 else ("?" if k == 1 else f[i])
        out.append(delim.join(x.encode() for x in f))
    return out


MIXED = ["int64", "float64", "category", "date", "short"]


# ---- records -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_row_counts_on_every_tile_edge(gdf, force_path, route):
    rng = np.random.RandomState(1)
    R = tile_rows(gdf)
    for i, rows in enumerate(sorted({0, 1, 63, 64, 65, R - 1, R, R + 1, 2 * R + 1})):
        recs = mixed_rows(rng, rows)
        data = b"".join(r + b"\n" for r in recs)
        got = check(gdf, force_path, route, data, MIXED, offset=(5 * i + 3) % 16)
        assert got.rows == rows
        if route == "staged":
            assert noted(gdf, "csv.unstaged_tiles") == 0
        if rows:                                                               # the last record without its terminator: one row all the same
            assert check(gdf, force_path, route, data[:-1], MIXED, offset=(7 * i) % 16).raw_bytes() == got.raw_bytes()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("offset", range(16))
def test_every_alignment_of_the_first_byte(gdf, force_path, route, offset):
    """70 records (two waves, one of them partial) and a length that moves the last byte over every alignment as well"""
    rng = np.random.RandomState(100 + offset)
    data = b"\n".join(mixed_rows(rng, 70)) + b"\n" * (offset % 2)
    check(gdf, force_path, route, data, MIXED, offset=offset)
    check(gdf, force_path, route, data[: len(data) - offset], MIXED, offset=offset)


@pytest.mark.parametrize("route", ROUTES)
def test_records_of_zero_and_one_byte(gdf, force_path, route):
    for data in (b"\n", b"\n\n\n", b"7", b"7\n", b"\n7", b"7\n\n8\n,\n\n9", b"\r\n7\r\n\r\n", b"\r", b",", b"\n" * 300, b"5\n" * 257 + b"6",
                 b"\n" * 129 + b"1,2.5\n"):
        got = check(gdf, force_path, route, data, ["int", "float64"])
        assert got.rows == len(ref.records(data))
    check(gdf, force_path, route, b"7;;8;", ["int", "int"], lineterminator=b";")     # '\r' is only special in front of '\n'
    check(gdf, force_path, route, b"7\r;8\r\n;", ["int", "category"], lineterminator=b";")


@pytest.mark.parametrize("route", ROUTES)
def test_a_record_longer_than_the_staging_budget(gdf, force_path, route):
    """40000 bytes in one category field in the middle of short records: its tile, and only its tile, walks global memory"""
    rng = np.random.RandomState(2)
    R = tile_rows(gdf)
    recs = mixed_rows(rng, 2 * R + 5)
    data = b"".join(r + b"\n" for r in recs)
    check(gdf, force_path, route, data, MIXED, offset=9)
    if route == "staged":
        assert noted(gdf, "csv.unstaged_tiles") == 0
    long_field = bytes(rng.randint(97, 123, size=40000).astype(np.uint8))
    recs[R + 7] = b"12," + b"1.5," + long_field + b",2001-02-03,9"
    data = b"".join(r + b"\n" for r in recs)
    got = check(gdf, force_path, route, data, MIXED, offset=9)
    if route == "staged":
        assert noted(gdf, "csv.unstaged_tiles") == 1
    h = ref.murmur3(long_field, ref.HASH_SEED)
    assert got.cols[2][0][R + 7] == (h - 2**32 if h >= 2**31 else h)


@pytest.mark.parametrize("route", ROUTES)
def test_short_and_long_records(gdf, force_path, route):
    data = b"1,2,3\n4\n5,6\n7,8,9,10,11\n,,\n12,,13\n"
    got = check(gdf, force_path, route, data, ["int", "int", "int"])
    assert [c[2] for c in got.cols] == [1, 3, 3]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("skip", [(0, 0), (1, 0), (0, 1), (1, 1), (5, 0), (0, 5), (3, 2), (2, 4), (200, 0)])
def test_skiprows_and_skipfooter(gdf, force_path, route, skip):
    rng = np.random.RandomState(3)
    data = b"header,of,no,use,here\n" + b"\n".join(mixed_rows(rng, 4))           # five records, the last one unterminated
    got = check(gdf, force_path, route, data, MIXED, offset=4, skiprows=skip[0], skipfooter=skip[1])
    assert got.rows == max(0, 5 - sum(skip))
    R = tile_rows(gdf)
    data = b"".join(r + b"\n" for r in mixed_rows(rng, 2 * R + 3))
    check(gdf, force_path, route, data, MIXED, skiprows=skip[0] * 13, skipfooter=skip[1] * 7)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("delim", [b",", b"|", b"\t", b" "])
def test_delimiters(gdf, force_path, route, delim):
    rng = np.random.RandomState(4)
    opts = dict(delim_whitespace=True) if delim == b" " else dict(delimiter=delim)
    data = b"".join(r + b"\n" for r in mixed_rows(rng, 150, delim))
    check(gdf, force_path, route, data, MIXED, offset=1, **opts)
    thousands = b"1,234,567" if delim != b"," else b"1234567"
    data = delim.join([thousands, b"2.5", b"a b" if delim != b" " else b"a,b", b"", b"7"]) + b"\n" + delim * 2 + b"x\n"
    got = check(gdf, force_path, route, data, MIXED, **opts)
    assert got.cols[0][0][0] == 1234567 and [c[2] for c in got.cols] == [1, 1, 0, 2, 1]


@pytest.mark.parametrize("route", ROUTES)
def test_spaces(gdf, force_path, route):
    """numbers and dates are trimmed on both sides whatever skipinitialspace says; a category loses its leading spaces only with it"""
    data = b"  12 , 1.5  ,  ab , 2001-02-03 ,7\n , ,  , ,\n1 2, 1. 5,a, 2001-02- 03,+ 7\n"
    for flag in (False, True):
        got = check(gdf, force_path, route, data, MIXED, skipinitialspace=flag)
        assert [c[2] for c in got.cols] == [2, 2, 1 if flag else 0, 2, 2]


# ---- dtypes ------------------------------------------------------------------------------------------------------------------------
INT_LITERALS = [b"0", b"-0", b"+0", b"1", b"-1", b"+17", b"007", b"32767", b"32768", b"-32768", b"-32769", b"2147483647", b"2147483648",
                b"-2147483648", b"-2147483649", b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808",
                b"-9223372036854775809", b"18446744073709551616", b"99999999999999999999999999", b"1,000", b"1,0,0", b"1,,0", b",1", b"1,",
                b"-,1", b"--1", b"+-1", b"-", b"+", b"1.0", b"1e3", b"0x10", b"12a", b"a12", b"1 2", b" 42 ", b"4\t2", b"\xff", b"1-"]
FLOAT_LITERALS = [b"0", b"-0", b"0.0", b"-0.0e5", b"1", b"-1.5", b"+2.25", b"1.", b".5", b"-.5", b".", b"-.", b"1e5", b"1E5", b"1e+5", b"1e-5",
                  b"1e", b"1e+", b"e5", b".e5", b"1.e5", b"1,234.5", b"1,234,567.25e-3", b"1,.5", b"1.2,3", b"inf", b"-inf", b"nan", b"NaN",
                  b"infinity", b"0x1p3", b"0x10", b"1_0", b"1d5", b"1e5.5", b"1e400", b"-1e400", b"1e-400", b"1e-5000000000", b"1e5000000000",
                  b"0e5000000000", b"9007199254740991", b"9007199254740991e22", b"9007199254740991e-22", b"9007199254740993",
                  b"9007199254740993e22", b"123456789012345678", b"1234567890123456789", b"12345678901234567890123", b"0.1", b"0.3", b"1e22",
                  b"1e23", b"1e-22", b"1e-23", b"3.14159265358979323846264338327950288", b"2.2250738585072014e-308",
                  b"2.2250738585072011e-308", b"4.9406564584124654e-324", b"2.4703282292062327e-324", b"2e-324", b"1.797693134862315e308",
                  b"1.8e308", b"8.5e307", b"6.02214076e23", b"1.602176634e-19", b"123456.789e3", b"0.000001", b"000123.4500",
                  b"3.4028235e38", b"3.4028236e38", b"1e39", b"1.17549435e-38", b"1e-46", b"7e-46", b"8e-46", b"16777217", b"0.1e1", b"100000000000000000000",
                  b"-9.999999999999999e22", b"5e-1"]
DATE_LITERALS = [b"1970-01-01", b"1969-12-31", b"2018-06-01", b"2000-02-29", b"1900-03-01", b"0001-01-01", b"9999-12-31", b"2018-6-1", b"2018/06/01",
                 b"2018-06", b"2018/6", b"06/2018", b"6-2018", b"6/1/2018", b"06-01-2018", b"13/1/2018", b"1/13/2018", b"31/12/1999",
                 b"12/31/1999", b"2018-06-01T10:16:12", b"2018-06-01 10:16", b"2018-06-01T1:2:3", b"2018-06-01T10:16:12PM",
                 b"2018-06-01T10:16:12 pm", b"2018-06-01 12:00 AM", b"2018-06-01 12:00 PM", b"2018-06-01 12:59:59am", b"1/2/2018 1:00 PM",
                 b"6/2018 23:59:59", b"1969-12-31T23:59:59",
                 # every check of the contract on its own
                 b"2018-00-10", b"2018-13-01", b"2018-06-00", b"2018-06-31", b"2018-01-32", b"2018-02-30", b"2018-02-29", b"1900-02-29",
                 b"2100-02-29", b"2400-02-29", b"0000-01-01", b"2018-06-01T24:00", b"2018-06-01T23:60", b"2018-06-01T23:59:60",
                 b"2018-06-01T13:00PM", b"2018-06-01T0:30AM", b"2018-06-01T00:00:00",
                 # shapes that are none
                 b"2018", b"2018-", b"2018-06-", b"2018-06/01", b"18-06-01", b"1/2/18", b"20180601", b"2018-06-01T", b"2018-06-01T10",
                 b"2018-06-01T10:", b"2018-06-01 10:16:12.5", b"2018-06-01  10:16", b"2018-06-01T10:16 XM", b"2018-06-01T10:16PMX",
                 b"2018-06-01x", b"June 1 2018", b"12345-01-01", b"2018-123-01", b"2018-06-001", b"-2018-06-01"]


def column_of(literals, term=b"\n"):
    return b"".join(x + term for x in literals)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", ["short", "int", "int32", "int64", "long", "timestamp"])
def test_integers_alone(gdf, force_path, route, dtype):
    """range edges of every width and one past them, signs, thousands separators, everything that is no literal"""
    got = check(gdf, force_path, route, column_of(INT_LITERALS), [dtype], delimiter=b"|")
    valid = np.unpackbits(got.cols[0][1], bitorder="little")[: len(INT_LITERALS)].astype(bool)
    lo, hi = ref.INT_RANGE[ref.DTYPE_OF[dtype]]
    for text, ok in zip(INT_LITERALS, valid):
        if text in (str(lo).encode(), str(hi).encode()):
            assert ok, text
        if text in (str(lo - 1).encode(), str(hi + 1).encode()):
            assert not ok, text


def float_literals():
    """(all of them, the random ones inside the fast domain): the hand-picked list, then random ones of every kind"""
    rng = np.random.RandomState(6)
    fast = [("%d" % rng.randint(0, 2**53) + "e%d" % rng.randint(-22, 23)).encode() for _ in range(200)]
    fast += [("%.12g" % x).encode() for x in rng.standard_normal(200) * 1000]
    wide = [("%.17g" % (x * 10.0 ** e)).encode() for x, e in zip(rng.standard_normal(300), rng.randint(-300, 300, size=300))]
    narrow = [("%.17g" % (x * 10.0 ** e)).encode() for x, e in zip(rng.standard_normal(200), rng.randint(-46, 39, size=200))]    # float32's range
    long_ones = [("%d.%de%d" % (rng.randint(0, 10**18), rng.randint(0, 10**18), rng.randint(-330, 290))).encode() for _ in range(200)]
    assert all(ref.in_fast_domain(x) for x in fast)
    return FLOAT_LITERALS + fast + wide + narrow + long_ones, fast


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", ["float64", "double", "float32", "float"])
def test_floats_alone(gdf, force_path, route, dtype):
    """float64: bit for bit inside the fast domain, within the header's bound outside; float32: exactly (float) of the model's double"""
    literals, _ = float_literals()
    got = check(gdf, force_path, route, column_of(literals), [dtype], delimiter=b"|", offset=13)
    data = got.cols[0][0]
    at = {x: data[i] for i, x in enumerate(literals)}
    assert np.signbit(at[b"-0"]) and at[b"-0"] == 0 and np.signbit(at[b"-0.0e5"]) and not np.signbit(at[b"0"])
    assert at[b"1e400"] == np.inf and at[b"-1e400"] == -np.inf and at[b"1e5000000000"] == np.inf and at[b"1e-5000000000"] == 0
    assert got.cols[0][2] == sum(ref.parse_float(x) is None for x in literals)
    if dtype in ("float32", "float"):
        assert at[b"3.4028235e38"] == np.float32(3.4028235e38) and at[b"1e39"] == np.inf and at[b"16777217"] == np.float32(16777216.0)
        assert ref.bits_of(np.array([at[b"8e-46"], at[b"7e-46"], at[b"1e-46"]])).tolist() == [1, 0, 0]            # a float denormal is not flushed


@pytest.mark.parametrize("route", ROUTES)
def test_float32_is_the_cast_of_the_float64(gdf, force_path, route):
    """gdf.h: 'FLOAT32 is (float) of that double' -- the same literals read as both in one call, bit for bit, denormals and all"""
    literals, _ = float_literals()
    data = b"".join(x + b"|" + x + b"\n" for x in literals)
    got = check(gdf, force_path, route, data, ["float64", "float32"], delimiter=b"|", offset=5)
    (f64, m64, n64), (f32, m32, n32) = got.cols
    with np.errstate(over="ignore"):
        cast = f64.astype(np.float32)
    assert np.array_equal(ref.bits_of(cast), ref.bits_of(f32))
    assert m64.tobytes() == m32.tobytes() and n64 == n32


def test_next_to_the_overflow_threshold(gdf):
    """gdf.h: within the ulp bound of the largest finite double a literal may come out finite or as the infinity -- never null, never
    anything else; the bound holds again a few dozen ulp further down (FLOAT_LITERALS)"""
    top = 1.7976931348623157e308
    got = Read(gdf, b"1.7976931348623157e308\n-1.7976931348623157e308\n", ["float64"])
    assert got.rc == 0 and got.cols[0][2] == 0
    hi, lo = got.cols[0][0].tolist()
    assert (hi == np.inf or 0 <= (top - hi) / math.ulp(top) <= ref.FLOAT_ULP_BOUND) and lo == -hi


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dayfirst", [False, True])
@pytest.mark.parametrize("dtype", ["date", "date64", "date32"])
def test_dates_alone(gdf, force_path, route, dtype, dayfirst):
    """every date and time shape of the contract, every validation on its own, both orders of day and month"""
    got = check(gdf, force_path, route, column_of(DATE_LITERALS), [dtype], dayfirst=dayfirst, offset=6)
    at = dict(zip(DATE_LITERALS, zip(got.cols[0][0].tolist(), np.unpackbits(got.cols[0][1], bitorder="little").tolist())))
    unit = 1 if dtype == "date32" else 86400000
    assert at[b"1970-01-01"] == (0, 1) and at[b"1969-12-31"] == (-unit, 1) and at[b"2000-02-29"] == (11016 * unit, 1)
    assert at[b"13/1/2018"][1] == int(dayfirst) and at[b"1/13/2018"][1] == int(not dayfirst)
    for bad in (b"2018-06-00", b"2018-01-32", b"2018-02-30", b"2018-02-29", b"2018-13-01", b"2018-06-01T24:00", b"2018-06-01T23:59:60"):
        assert at[bad] == (0, 0), bad
    if dtype != "date32":
        assert at[b"2018-06-01 12:00 AM"][0] + 12 * 3600 * 1000 == at[b"2018-06-01 12:00 PM"][0] == at[b"2018-06-01"][0] + 12 * 3600 * 1000
    else:
        assert at[b"2018-06-01 12:00 PM"] == (0, 0)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("dtype", ["category", "str"])
def test_categories_alone(gdf, force_path, route, dtype):
    rng = np.random.RandomState(8)
    fields = [b"a", b"ab", b"abc", b"abcd", b"abcde", b"", b" ", b"  x", b"x  ", b'"quoted"', b"\xff\x00\x80"[:1] + b"\x80"]
    fields += [bytes(rng.randint(33, 127, size=n).astype(np.uint8)).replace(b"|", b"!") for n in range(1, 70)]
    data = column_of(fields)
    got = check(gdf, force_path, route, data, [dtype], delimiter=b"|")
    assert got.cols[0][0][2] == np.uint32(ref.murmur3(b"abc", 33)).astype(np.int32) and got.cols[0][2] == 1
    check(gdf, force_path, route, data, [dtype], delimiter=b"|", skipinitialspace=True)
    # the delimiter and the terminator are not hashed: the same fields give the same values wherever they stand
    two = b"".join(a + b"|" + b + b"\n" for a, b in zip(fields, fields[::-1]))
    both = check(gdf, force_path, route, two, [dtype, dtype], delimiter=b"|")
    assert np.array_equal(both.cols[0][0], got.cols[0][0]) and np.array_equal(both.cols[1][0], got.cols[0][0][::-1])


def mortgage_rows(rng, rows):
    day = lambda: f"{rng.randint(1, 13):02d}/{rng.randint(1, 29):02d}/{rng.randint(1999, 2020)}"       # noqa: E731
    money = lambda: "" if rng.randint(0, 4) else f"{rng.uniform(0, 50000):.2f}"                            # noqa: E731
    for r in range(rows):
        f = [str(100000000000 + rng.randint(0, 10**9)), day(), rng.choice(["", "OTHER", "BANK OF SOMEWHERE, N.A.", "X"]),
             f"{rng.uniform(2, 9):.3f}", money(), str(rng.randint(0, 360)), str(rng.randint(0, 360)), money(), f"{rng.randint(1, 13):02d}/{rng.randint(2020, 2050)}",
             str(rng.randint(10000, 50000)), rng.choice(["0", "1", "2", "X", ""]), rng.choice(["N", "Y"]), rng.choice(["", "01", "09"]),
             rng.choice(["", day()]), rng.choice(["", day()]), rng.choice(["", day()]), rng.choice(["", day()])]
        f += [money() for _ in range(11)] + [rng.choice(["", "Y", "N"]), money(), rng.choice(["", "Y", "N"])]
        yield "|".join(f).encode()


@pytest.mark.parametrize("route", ROUTES)
def test_mortgage_schema(gdf, force_path, route):
    """the 31 columns of the reference's pipeline test (names and dtype strings: tests/golden/mortgage_schema.json; the rows are invented)"""
    with open(os.path.join(ROOT, "tests", "golden", "mortgage_schema.json")) as f:
        schema = json.load(f)
    assert len(schema["names"]) == len(schema["dtypes"]) == 31
    R = tile_rows(gdf)
    data = b"".join(r + b"\n" for r in mortgage_rows(np.random.RandomState(9), 2 * R + 1))
    got = check(gdf, force_path, route, data, schema["dtypes"], names=schema["names"], delimiter=schema["delimiter"].encode(), offset=11)
    assert [f[0] for f in got.fields] == schema["names"] and got.rows == 2 * R + 1
    assert got.cols[0][2] == 0 and got.cols[4][2] > 0


# ---- calls -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES)
def test_two_calls_are_bit_identical(gdf, force_path, route):
    rng = np.random.RandomState(10)
    data = b"".join(r + b"\n" for r in mixed_rows(rng, 3 * tile_rows(gdf) + 17))
    a = check(gdf, force_path, route, data, MIXED, offset=2)
    b = check(gdf, force_path, route, data, MIXED, offset=2)
    assert a.raw_bytes() == b.raw_bytes()
    force_path("GDF_CSV_NO_STAGE", None if route == "unstaged" else "1")         # ... and the other route gives the same bytes
    assert Read(gdf, data, MIXED, offset=7).raw_bytes() == a.raw_bytes()


def test_read_csv_on_files(gdf, tmp_path):
    rng = np.random.RandomState(12)
    data = b"".join(r + b"\r\n" for r in mixed_rows(rng, 333))
    for name, content in (("plain.csv", data), ("unterminated.csv", data[:-2]), ("empty.csv", b""), ("one.csv", b"1,2.5,x,2001-01-01,3")):
        path = tmp_path / name
        path.write_bytes(content)
        from_file = compare(Read(gdf, content, MIXED, path=str(path)), content, MIXED)
        from_buffer = Read(gdf, content, MIXED, offset=3)
        assert from_file.raw_bytes() == from_buffer.raw_bytes() and from_file.fields == from_buffer.fields
    assert from_file.rows == 1
    assert Read(gdf, b"", MIXED, path=str(tmp_path / "missing.csv")).rc == 19                     # GDF_FILE_ERROR
    assert Read(gdf, b"", MIXED, path=str(tmp_path)).rc == 19
    assert Read(gdf, b"1\n", ["int8"]).rc == 2                                                    # GDF_UNSUPPORTED_DTYPE


def test_python_wrapper(gdf, tmp_path):
    import torch
    assert gdf.read_csv is gdf.api.read_csv
    path = tmp_path / "t.txt"
    content = b"skip me\n1|2.5|ab|13/2/2001\n|x||\n3|4||1/12/2001\nfooter"
    path.write_bytes(content)
    out = gdf.read_csv(str(path), ["n", "x", "s", "d"], ["int64", "float32", "str", "date32"], delimiter="|", skiprows=1, skipfooter=1,
                       dayfirst=True)
    want = ref.read(content, ["int64", "float32", "str", "date32"], delimiter=b"|", skiprows=1, skipfooter=1, dayfirst=True)
    assert list(out) == ["n", "x", "s", "d"]
    assert [out[k][0].dtype for k in out] == [torch.int64, torch.float32, torch.int32, torch.int32]
    for (data, mask, nulls), (wd, wm, wn) in zip(out.values(), want):
        assert data.is_cuda and mask.dtype == torch.uint8
        assert np.array_equal(data.cpu().numpy(), wd) and np.array_equal(mask.cpu().numpy(), wm) and nulls == wn
    assert out["n"][0].tolist() == [1, 0, 3] and out["d"][2] == 1
    with pytest.raises(gdf.GDFError, match="GDF_FILE_ERROR"):
        gdf.read_csv(str(tmp_path / "none"), ["a"], ["int"])
    with pytest.raises(gdf.GDFError, match="GDF_UNSUPPORTED_DTYPE"):
        gdf.read_csv(str(path), ["a"], ["int8"])


def test_release_gives_everything_back(gdf):
    """RMM's own count of outstanding allocations (the 'Current Allocs' column of its log, pool mode, this process only) is after
    gdf_amd_read_csv_release exactly what it was before the call; in between it is higher by one data and one mask block per column"""
    import torch
    from libgdf_amd import api
    from libgdf_amd._binding import rmmOptions_t
    data = b"".join(b"%d,%d.5,w%d\n" % (i, i, i) for i in range(20000))
    dev = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()

    def outstanding():
        size = gdf.librmm.rmmLogSize()
        buf = C.create_string_buffer(size + 1)
        gdf.librmm.rmmGetLog(buf, size + 1)
        events = buf.value.decode().strip().splitlines()[1:]                       # (the first line is the header)
        return int(events[-1].split(",")[7]) if events else 0

    def call():
        a = api.csv_args(["a", "b", "c"], ["int64", "float64", "category"])
        gdf.libgdf.gdf_amd_read_csv_device(dev.data_ptr(), len(data), C.byref(a))
        assert a.num_rows_out == 20000 and a.data[2].contents.null_count == 0
        return a

    gdf.librmm.rmmFinalize()
    gdf.librmm.rmmInitialize(C.byref(rmmOptions_t(1, 0, True)))                   # pool mode, logging on
    try:
        gdf.libgdf.gdf_amd_read_csv_release(C.byref(call()))
        before = outstanding()
        a = call()
        assert outstanding() == before + 2 * 3
        gdf.libgdf.gdf_amd_read_csv_release(C.byref(a))
        assert (a.num_cols_out, a.num_rows_out, bool(a.data)) == (0, 0, False)
        assert outstanding() == before
        gdf.libgdf.gdf_amd_read_csv_release(C.byref(a))                           # again: nothing to do
        assert outstanding() == before
        bad = api.csv_args(["a"], ["int8"])
        assert gdf.libgdf.raw("gdf_amd_read_csv_device")(dev.data_ptr(), len(data), C.byref(bad)) == 2
        big = api.csv_args(["a"], ["int64"], skiprows=-1)
        assert gdf.libgdf.raw("gdf_amd_read_csv_device")(dev.data_ptr(), len(data), C.byref(big)) == 8
        assert outstanding() == before
    finally:
        gdf.librmm.rmmFinalize()
        gdf.librmm.rmmInitialize(C.byref(rmmOptions_t(0, 0, False)))               # leave the session in default mode
