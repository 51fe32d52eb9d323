"""No-GPU checks that the Python model of the read_csv contract (tests/csv_reference.py) is itself right: a case written out by hand,
its byte-range MurmurHash3 against the fixed-width one of tests/hash_partition_cases.py, and pandas.read_csv on plain files."""
import datetime
import io

import numpy as np

import csv_reference as ref
from hash_partition_cases import murmur3_32


def _col(col):
    data, mask, nulls = col
    bits = np.unpackbits(mask, bitorder="little")[: len(data)].astype(bool)
    return data.tolist(), bits.tolist(), nulls


def test_a_case_written_by_hand():
    """every dtype; an empty field, an invalid literal, a short record (record 2), a long one (record 1), \\r\\n, a last record
    without terminator"""
    dtypes = ["int64", "short", "float64", "float32", "date32", "date", "category", "timestamp", "int"]
    data = (b"-12|7|1.5|-0|1970-01-02|1970-01-01T00:00:01|ab|1000|2147483647\r\n"
            b"1,234|32768|1e3|.25|12/31/1969|1/1/1970 12:00 PM|abcde|-5|2147483648|extra|fields\n"
            b"x||5\n"
            b"\n"
            b"+7| 8 |  -0.0  |nan|2000-02-29|02/2001| q|9223372036854775807|0x10")
    read = lambda d, **kw: ref.read(d, dtypes, delimiter=b"|", **kw)                               # noqa: E731
    cols = [_col(c) for c in read(data)]
    assert cols[0] == ([-12, 1234, 0, 0, 7], [True, True, False, False, True], 2)
    assert cols[1] == ([7, 0, 0, 0, 8], [True, False, False, False, True], 3)                    # 32768 is out of range
    assert cols[2][0][:2] == [1.5, 1000.0] and cols[2][0][2] == 5.0 and cols[2][1] == [True, True, True, False, True]
    assert np.signbit(cols[2][0][4]) and cols[2][0][4] == 0.0
    assert cols[3][0][:2] == [0.0, 0.25] and np.signbit(cols[3][0][0]) and cols[3][1] == [True, True, False, False, False]
    assert cols[4] == ([1, -1, 0, 0, 11016], [True, True, False, False, True], 2)
    assert datetime.date(1970, 1, 1) + datetime.timedelta(days=11016) == datetime.date(2000, 2, 29)
    feb2001 = (datetime.date(2001, 2, 1) - datetime.date(1970, 1, 1)).days * 86400000
    assert cols[5] == ([1000, 12 * 3600 * 1000, 0, 0, feb2001], [True, True, False, False, True], 2)
    h = lambda b: int(np.uint32(ref.murmur3(b, 33)).astype(np.int32))                             # noqa: E731
    assert cols[6] == ([h(b"ab"), h(b"abcde"), 0, 0, h(b" q")], [True, True, False, False, True], 2)
    assert cols[7] == ([1000, -5, 0, 0, 2**63 - 1], [True, True, False, False, True], 2)
    assert cols[8] == ([2**31 - 1, 0, 0, 0, 0], [True, False, False, False, False], 4)
    # the same bytes with a final terminator are the same five records; skipinitialspace reaches the category only
    again = read(data + b"\n", skipinitialspace=True)
    assert _col(again[6])[0][4] == h(b"q") and len(again[0][0]) == 5
    assert [len(c[0]) for c in read(data, skiprows=1, skipfooter=3)] == [1] * 9
    assert [len(c[0]) for c in read(data, skiprows=3, skipfooter=2)] == [0] * 9
    assert ref.read(b"", ["int"])[0][0].shape == (0,) and len(ref.read(b"\n", ["int"])[0][0]) == 1


def test_dates_times_and_their_validation():
    ms = lambda *a: int((datetime.datetime(*a) - datetime.datetime(1970, 1, 1)).total_seconds()) * 1000      # noqa: E731
    good = {b"2018-06-01T10:16:12PM": ms(2018, 6, 1, 22, 16, 12), b"2018/6/1 12:05 AM": ms(2018, 6, 1, 0, 5), b"6-1-2018": ms(2018, 6, 1),
            b"0001-01-01": ms(1, 1, 1), b"9999-12-31 23:59:59": ms(9999, 12, 31, 23, 59, 59), b"12/1969": ms(1969, 12, 1),
            b"1900-03-01": ms(1900, 3, 1), b"2000-02-29T12:00pm": ms(2000, 2, 29, 12)}
    for text, want in good.items():
        assert ref.parse_field(text, 8) == want, text
    assert ref.parse_field(b"3/4/2001", 7, dayfirst=True) == (datetime.date(2001, 4, 3) - datetime.date(1970, 1, 1)).days
    assert ref.parse_field(b"3/4/2001", 7) == (datetime.date(2001, 3, 4) - datetime.date(1970, 1, 1)).days
    for bad in (b"2001-00-10", b"2001-13-01", b"2001-01-00", b"2001-01-32", b"2001-02-30", b"1900-02-29", b"2001-02-29", b"0000-01-01",
                b"2001-01-01T24:00", b"2001-01-01T10:60", b"2001-01-01T10:00:60", b"2001-01-01T13:00PM", b"2001-01-01T0:00AM",
                b"2001-01-01X", b"2001-01/01", b"01-01-01", b"2001", b"2001-01-01T10", b"2001-01-01 10:00:00.5"):
        assert ref.parse_field(bad, 8) is None, bad
    assert ref.parse_field(b"2001-01-01T10:00", 7) is None                                      # DATE32 takes no time


def test_literals():
    assert [ref.parse_field(t, 3) for t in (b"1,000", b"1,,0", b",1", b"1,", b"--1", b"+", b"1 2", b"1.0", b"-0")] == \
        [1000, None, None, None, None, None, None, None, 0]
    assert [ref.parse_field(t, 4) for t in (b"-9223372036854775808", b"-9223372036854775809", b"9223372036854775808")] == \
        [-2**63, None, None]
    assert [ref.parse_field(t, 6) for t in (b"1.", b".5", b".", b"1e", b"1e+", b"e5", b"inf", b"NaN", b"0x1p3", b"1_0", b"1,234.5e-1",
                                            b"1e400", b"-1e400", b"1e-400")] == \
        [1.0, 0.5, None, None, None, None, None, None, None, None, 123.45, float("inf"), float("-inf"), 0.0]
    assert ref.float_parts(b"0.00123") == (123, -5) and ref.float_parts(b"123456789012345678901234.5") == (1234567890123456789, 5)
    assert ref.float_parts(b"1.2345678901234567890123") == (1234567890123456789, -18)
    assert ref.in_fast_domain(b"9007199254740991e22") and not ref.in_fast_domain(b"9007199254740992") \
        and not ref.in_fast_domain(b"1e23")


def test_byte_range_murmur_equals_the_fixed_width_one():
    rng = np.random.RandomState(3)
    for dt in (np.int32, np.int64):
        values = rng.randint(-2**31, 2**31 - 1, size=50).astype(dt) * (dt(2**31 + 12345) if dt is np.int64 else dt(1))
        want = murmur3_32(values)
        got = [ref.murmur3(v.tobytes(), 0) for v in values]
        assert got == want.tolist()
    # known answers of MurmurHash3 x86_32
    assert ref.murmur3(b"", 0) == 0 and ref.murmur3(b"", 1) == 0x514e28b7 and ref.murmur3(b"abc", 0) == 0xb3dd93fa
    assert ref.murmur3(b"Hello, world!", 1234) == 0xfaf6cdb3


def test_model_agrees_with_pandas_on_plain_files():
    import pandas as pd
    rng = np.random.RandomState(11)
    rows = 400
    ints = rng.randint(-2**62, 2**62, size=rows)
    small = rng.randint(-2**15, 2**15, size=rows)
    floats = [float(f"{x:.{rng.randint(1, 15)}g}") for x in rng.standard_normal(rows) * 10.0 ** rng.randint(-8, 9, size=rows)]
    days = rng.randint(-20000, 40000, size=rows)
    dates = [(datetime.date(1970, 1, 1) + datetime.timedelta(days=int(d))).isoformat() for d in days]
    for delim in (",", "|", "\t"):
        text = "".join(f"{i}{delim}{s}{delim}{f!r}{delim}{d}\n" for i, s, f, d in zip(ints, small, floats, dates)).encode()
        model = ref.read(text, ["int64", "short", "float64", "date"], delimiter=delim.encode())
        frame = pd.read_csv(io.BytesIO(text), sep=delim, header=None, names=list("abcd"), dtype={"a": np.int64, "b": np.int16, "c": np.float64},
                            parse_dates=["d"], float_precision="round_trip")
        assert all(c[2] == 0 and np.unpackbits(c[1], bitorder="little")[:rows].all() for c in model)
        assert np.array_equal(model[0][0], frame["a"].to_numpy()) and np.array_equal(model[1][0], frame["b"].to_numpy())
        assert np.array_equal(ref.bits_of(model[2][0]), ref.bits_of(frame["c"].to_numpy()))
        assert np.array_equal(model[3][0], frame["d"].to_numpy().astype("datetime64[ms]").astype(np.int64))
        assert np.array_equal(model[3][0], days.astype(np.int64) * 86400000)
