"""Datetime field extraction on the GPU (csrc/elementwise.hip) against numpy.datetime64 (elementwise_reference.datetime_field_numpy), 0
ulp: the six entry points on DATE32 / DATE64 / TIMESTAMP in all four units over +-300 years, the reference's known answers, the two
deliberate differences from the reference, sizes, misalignments, the mask copy, the guard bytes around the output, determinism."""
import json
import os

import numpy as np
import pytest

import elementwise_reference as er
from elementwise_common import BIG, SIZES, Buf, assert_same_bits, col, mask_tensor, offsets, ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(er.DATE32, 0, "D"), (er.DATE64, 0, "ms"), (er.TIMESTAMP, er.UNIT_S, "s"), (er.TIMESTAMP, er.UNIT_MS, "ms"),
         (er.TIMESTAMP, er.UNIT_US, "us"), (er.TIMESTAMP, er.UNIT_NS, "ns"), (er.TIMESTAMP, er.UNIT_NONE, "ms")]
TICKS = {"D": None, "s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}


def _values(np_unit, n, seed=0):
    rng = np.random.RandomState(seed + n % 1000)
    if np_unit == "D":
        return rng.randint(-300 * 366, 300 * 366, size=n).astype(np.int32)
    # ns: the int64 range (+-292 years) less two days -- numpy's own datetime64[ns] -> [M] conversion is wrong inside the first day of
    # the range (1677-09-21), where the restatement and the library agree with the calendar
    span = min(300 * 366 * 86400 * TICKS[np_unit], 2**63 - 1 - 2 * 86400 * 10**9)
    return rng.randint(-span, span, size=n, dtype=np.int64)


def _fields(dtype):
    return er.DATETIME_FIELDS[:3] if dtype == er.DATE32 else er.DATETIME_FIELDS


def _run(gdf, field, x, dtype, unit, offs=(0, 0), valid=None):
    import torch
    n = len(x)
    bi, bo = Buf(n, x.dtype, offs[0], x), Buf(n, np.int16, offs[1])
    mi = mask_tensor(valid)[0] if valid is not None else None
    mo = torch.full(((n + 7) // 8 + 5,), 0xEE, dtype=torch.uint8, device="cuda")
    co = col(bo, er.INT16, mo)
    getattr(gdf.libgdf, f"gdf_extract_datetime_{field}")(ref(col(bi, dtype, mi, unit)), ref(co))
    assert co.dtype == er.INT16
    assert np.array_equal(bi.read().view(np.uint8), x.view(np.uint8))
    return bo.read(), mo.cpu().numpy()


@pytest.mark.parametrize("field,dtype,unit,np_unit", [(f, d, u, nu) for d, u, nu in KINDS for f in _fields(d)])
def test_fields_against_numpy_datetime64(gdf, field, dtype, unit, np_unit):
    for n in SIZES:
        x = _values(np_unit, n)
        got, _ = _run(gdf, field, x, dtype, unit)
        assert_same_bits(got, er.datetime_field_numpy(field, x, np_unit))
        assert_same_bits(got, er.datetime_field(field, x, dtype, unit))


def test_the_reference_known_answers(gdf):
    with open(os.path.join(ROOT, "tests", "golden", "datetime_known_answers.json")) as f:
        known = json.load(f)["vectors"]
    assert len(known) == 48
    for v in known:
        dtype = dict(DATE32=er.DATE32, DATE64=er.DATE64, TIMESTAMP=er.TIMESTAMP)[v["dtype"]]
        x = np.array(v["input"], dtype=er.STORAGE[dtype])
        got, _ = _run(gdf, v["field"], x, dtype, er.UNIT_NAMES.get(v["time_unit"], 0))
        assert got.tolist() == v["expected"], (v["source"], v["dtype"], v["time_unit"], v["field"])


@pytest.mark.parametrize("dtype,unit,np_unit", KINDS[1:])
def test_negative_exact_multiples_give_zero_not_24_or_60(gdf, dtype, unit, np_unit):
    """the first deliberate difference from the reference"""
    t = TICKS[np_unit]
    k = np.arange(-2000, 2001, dtype=np.int64)
    for field, step in (("hour", 86400 * t), ("minute", 3600 * t), ("second", 60 * t)):
        x = np.concatenate([k * step, k * step - 1, k * step + 1])
        got, _ = _run(gdf, field, x, dtype, unit)
        assert_same_bits(got, er.datetime_field_numpy(field, x, np_unit))
        assert (got[: len(k)] == 0).all() and got.max() == (23 if field == "hour" else 59) and got.min() == 0


def test_day_numbers_beyond_32_bits(gdf):
    """the second deliberate difference: seconds reach day numbers the reference's 32-bit arithmetic cannot hold"""
    x = np.array([2**62, -2**62, 2**63 - 1, -2**63, 40000 * 366 * 86400, 10**15 + 12345], dtype=np.int64)
    for field in er.DATETIME_FIELDS:
        got, _ = _run(gdf, field, x, er.TIMESTAMP, er.UNIT_S)
        assert_same_bits(got, er.datetime_field(field, x, er.TIMESTAMP, er.UNIT_S))
    d = np.array([2**31 - 1, -2**31, 2**31 - 719468], dtype=np.int32)    # DATE32: the +719468 shift must not overflow
    for field in er.DATETIME_FIELDS[:3]:
        got, _ = _run(gdf, field, d, er.DATE32, 0)
        assert_same_bits(got, er.datetime_field(field, d, er.DATE32))


@pytest.mark.parametrize("dtype,unit,np_unit", [KINDS[0], KINDS[5]])
def test_every_misalignment_of_both_pointers(gdf, dtype, unit, np_unit):
    x = _values(np_unit, 555, 4)
    for field in ("year", "day") if dtype == er.DATE32 else ("year", "minute"):
        want = er.datetime_field_numpy(field, x, np_unit)
        for i in offsets(x.dtype.itemsize):
            for o in offsets(2):
                got, _ = _run(gdf, field, x, dtype, unit, offs=(i, o))
                assert_same_bits(got, want)


@pytest.mark.parametrize("n", [1, 8, 9, 65, 1000, 2**16 + 3])
def test_mask_copy(gdf, n):
    x = _values("us", n)
    valid = np.random.rand(n) < 0.5
    nb = (n + 7) // 8
    got, mo = _run(gdf, "month", x, er.TIMESTAMP, er.UNIT_US, valid=valid)
    assert np.array_equal(mo[:nb], mask_tensor(valid)[1]) and (mo[nb:] == 0xEE).all()
    assert_same_bits(got, er.datetime_field_numpy("month", x, "us"), valid)
    _, mo = _run(gdf, "month", x, er.TIMESTAMP, er.UNIT_US)
    assert (mo == 0xEE).all()


def test_a_large_column_and_determinism(gdf):
    x = _values("ns", BIG, 1)
    got, _ = _run(gdf, "year", x, er.TIMESTAMP, er.UNIT_NS, offs=(1, 3))
    assert_same_bits(got, er.datetime_field_numpy("year", x, "ns"))
    again, _ = _run(gdf, "year", x, er.TIMESTAMP, er.UNIT_NS, offs=(1, 3))
    assert np.array_equal(got, again)


def test_python_extract_datetime(gdf):
    from libgdf_amd.columns import column_from_numpy
    x = _values("ns", 1003)
    valid = np.random.rand(1003) < 0.8
    out = gdf.api.extract_datetime("hour", column_from_numpy(x, valid, dtype=er.TIMESTAMP, time_unit="ns"))
    assert out.c.dtype == er.INT16 and np.array_equal(out.valid_bits(), valid)
    assert_same_bits(out.to_numpy(), er.datetime_field_numpy("hour", x, "ns"), valid)
    out = gdf.api.extract_datetime("day", column_from_numpy(_values("D", 100), dtype=er.DATE32))
    assert_same_bits(out.to_numpy(), er.datetime_field_numpy("day", _values("D", 100), "D"))
    with pytest.raises(gdf.GDFError):
        gdf.api.extract_datetime("hour", column_from_numpy(_values("D", 100), dtype=er.DATE32))
