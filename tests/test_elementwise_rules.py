"""No-GPU checks of the numpy restatements the GPU tests of csrc/elementwise.hip compare against (elementwise_reference.py): the
datetime fields reproduce every known answer of the reference's datetime test (tests/golden/datetime_known_answers.json: its input
values and expected fields, copied as data) and agree with numpy.datetime64, also where this library deliberately differs from the
reference; the date / time casts are floor divisions and wrapping multiplications."""
import json
import os

import numpy as np
import pytest

import elementwise_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "datetime_known_answers.json")) as _f:
    KNOWN = json.load(_f)["vectors"]
DTYPES = dict(DATE32=ref.DATE32, DATE64=ref.DATE64, TIMESTAMP=ref.TIMESTAMP)


def test_known_answers_file_is_complete():
    assert len(KNOWN) == 48
    assert {v["field"] for v in KNOWN} == set(ref.DATETIME_FIELDS)
    assert {(v["dtype"], v["time_unit"]) for v in KNOWN} == {("DATE32", None), ("DATE64", None), ("TIMESTAMP", "s"), ("TIMESTAMP", "ms"),
                                                           ("TIMESTAMP", "us"), ("TIMESTAMP", "ns")}


@pytest.mark.parametrize("i", range(48))
def test_datetime_rule_reproduces_the_reference_known_answers(i):
    v = KNOWN[i]
    storage = ref.STORAGE[DTYPES[v["dtype"]]]
    got = ref.datetime_field(v["field"], np.array(v["input"], dtype=storage), DTYPES[v["dtype"]], ref.UNIT_NAMES.get(v["time_unit"], 0))
    assert got.tolist() == v["expected"], (v["source"], v["dtype"], v["time_unit"], v["field"])


def test_known_answers_avoid_the_deliberate_differences():
    """none of the negative inputs is an exact multiple of a minute in its unit, so hour 24 / minute 60 / second 60 of the reference
    (which this library answers with 0) cannot occur in the file"""
    negatives = 0
    for v in KNOWN:
        if v["dtype"] == "DATE32":
            continue
        tps = {"s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}[v["time_unit"] or "ms"]
        for x in v["input"]:
            if x < 0:
                negatives += 1
                assert x % (60 * tps) != 0
    assert negatives > 0


@pytest.mark.parametrize("unit,np_unit,dtype", [(ref.UNIT_S, "s", ref.TIMESTAMP), (ref.UNIT_MS, "ms", ref.TIMESTAMP), (ref.UNIT_US, "us", ref.TIMESTAMP),
                                                (ref.UNIT_NS, "ns", ref.TIMESTAMP), (ref.UNIT_NONE, "ms", ref.DATE64),
                                                (ref.UNIT_NONE, "ms", ref.TIMESTAMP)])
@pytest.mark.parametrize("field", ref.DATETIME_FIELDS)
def test_datetime_rule_is_numpy_datetime64(field, unit, np_unit, dtype):
    tps = {"s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}[np_unit]
    # +-300 years; ns: the int64 range (+-292 years) less two days, because numpy's datetime64[ns] -> [M] conversion is itself wrong
    # inside the first day of the range (1677-09-21)
    span = min(300 * 366 * 86400 * tps, 2**63 - 1 - 2 * 86400 * 10**9)
    rng = np.random.RandomState(7)
    x = rng.randint(-span, span, size=20000, dtype=np.int64)
    # ... and the exact multiples of a day / hour / minute on both sides of the epoch, where the reference says 24 / 60 / 60
    k = np.arange(-50, 51, dtype=np.int64)
    x = np.concatenate([x, k * 86400 * tps, k * 3600 * tps, k * 60 * tps, k * tps, k * 86400 * tps - 1, k * 86400 * tps + 1])
    got = ref.datetime_field(field, x, dtype, unit)
    assert np.array_equal(got, ref.datetime_field_numpy(field, x, np_unit))
    if field in ("hour", "minute", "second"):
        assert got.min() == 0 and got.max() == (23 if field == "hour" else 59)


@pytest.mark.parametrize("field", ("year", "month", "day"))
def test_date32_rule_is_numpy_datetime64(field):
    x = np.concatenate([np.random.RandomState(3).randint(-300 * 366, 300 * 366, size=20000), np.arange(-800, 800)]).astype(np.int32)
    assert np.array_equal(ref.datetime_field(field, x, ref.DATE32), ref.datetime_field_numpy(field, x, "D"))


def test_year_is_truncated_to_int16_from_a_64_bit_day_number():
    """seconds reach day numbers beyond 32 bits and years beyond int16: the year is that of the 64-bit day number (found here by
    stepping whole 400-year cycles of 146097 days into datetime.date's range), truncated to int16"""
    import datetime
    x = np.array([2**62, -2**62, 40000 * 366 * 86400], dtype=np.int64)
    y = ref.datetime_field("year", x, ref.TIMESTAMP, ref.UNIT_S)
    assert y.dtype == np.int16
    for xi, yi in zip(x.tolist(), y.tolist()):
        cycles, rest = divmod(xi // 86400, 146097)
        year = (datetime.date(1970, 1, 1) + datetime.timedelta(days=rest)).year + 400 * cycles
        assert yi == (year + 2**15) % 2**16 - 2**15


UNIT_NP = {ref.UNIT_S: "s", ref.UNIT_MS: "ms", ref.UNIT_US: "us", ref.UNIT_NS: "ns"}


@pytest.mark.parametrize("fu", UNIT_NP)
@pytest.mark.parametrize("tu", UNIT_NP)
def test_timestamp_unit_casts_are_numpy_datetime64_conversions(fu, tu):
    rng = np.random.RandomState(fu * 10 + tu)
    x = rng.randint(-2**40, 2**40, size=5000, dtype=np.int64)
    x = np.concatenate([x, np.arange(-3000, 3001, dtype=np.int64), np.arange(-5, 6, dtype=np.int64) * 10**9])
    got = ref.cast(x, ref.TIMESTAMP, fu, ref.TIMESTAMP, tu)
    want = x.astype(f"datetime64[{UNIT_NP[fu]}]").astype(f"datetime64[{UNIT_NP[tu]}]").astype(np.int64)
    assert np.array_equal(got, want)                                              # numpy floors towards the coarser unit too


def test_date_casts():
    d = np.array([-56374, -1, 0, 1, 17696], dtype=np.int32)
    assert ref.cast(d, ref.DATE32, 0, ref.DATE64, 0).tolist() == (d.astype(np.int64) * 86400000).tolist()
    ms = np.array([-86400001, -86400000, -1, 0, 86399999, 86400000], dtype=np.int64)
    assert ref.cast(ms, ref.DATE64, 0, ref.DATE32, 0).tolist() == [-2, -1, -1, 0, 0, 1]
    assert ref.cast(ms, ref.DATE64, 0, ref.TIMESTAMP, ref.UNIT_S).tolist() == [-86401, -86400, -1, 0, 86399, 86400]
    assert ref.cast(ms, ref.DATE64, 0, ref.TIMESTAMP, ref.UNIT_MS).tolist() == ms.tolist()            # the same thing
    assert ref.cast(ms, ref.DATE64, 0, ref.TIMESTAMP, ref.UNIT_NONE).tolist() == ms.tolist()          # no unit: a copy
    assert ref.cast(ms, ref.TIMESTAMP, ref.UNIT_NONE, ref.DATE32, 0).tolist() == ms.astype(np.int32).tolist()
    assert ref.cast(d, ref.DATE32, 0, ref.TIMESTAMP, ref.UNIT_NS).tolist() == (d.astype(np.int64) * 86400 * 10**9).tolist()
    big = np.array([2**62], dtype=np.int64)                                       # the multiplication wraps
    assert ref.cast(big, ref.TIMESTAMP, ref.UNIT_S, ref.TIMESTAMP, ref.UNIT_MS).tolist() == [(2**62 * 1000 + 2**63) % 2**64 - 2**63]
    assert ref.cast(ms, ref.DATE64, 0, ref.INT32, 0).tolist() == ms.astype(np.int32).tolist()         # not a date target: plain


def test_integer_floordiv_rule_is_exact():
    a = np.array([7, -7, 7, -7, 2**62 + 1, -(2**62) - 1, 0], dtype=np.int64)
    b = np.array([2, 2, -2, -2, 3, 3, 5], dtype=np.int64)
    assert ref.binary("floordiv", a, b).tolist() == [int(x) // int(y) for x, y in zip(a, b)]
    assert ref.floordiv_specified(np.array([1, np.iinfo(np.int64).min, 5]), np.array([0, -1, -1])).tolist() == [False, False, True]
