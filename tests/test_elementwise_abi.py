"""No-GPU checks of the element-wise operators (csrc/elementwise.hip): every argument check runs on the host before any device
work, through the C ABI with fake device pointers (include/gdf/gdf.h, "element-wise operators")."""
import ctypes as C
import os

import pytest

import elementwise_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libgdf_amd", "lib")

GDF_SUCCESS, GDF_UNSUPPORTED_DTYPE, GDF_COLUMN_SIZE_MISMATCH, GDF_INVALID_API_CALL, GDF_UNSUPPORTED_METHOD = 0, 2, 3, 8, 12
FAKE_DEV = 0x1000          # never dereferenced: every call below returns from its host-side checks
INT8, INT16, INT32, INT64, FLOAT32, FLOAT64, DATE32, DATE64, TIMESTAMP, CATEGORY, STRING = range(1, 12)
ALL_DTYPES = range(0, 12)


@pytest.fixture(scope="module")
def gdf():
    C.CDLL(os.path.join(LIBDIR, "libgdf_testhook.so"), mode=C.RTLD_GLOBAL)
    C.CDLL(os.path.join(LIBDIR, "librmm.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIBDIR, "libgdf.so"), mode=C.RTLD_GLOBAL)
    from libgdf_amd._binding import _PROTOTYPES, ELEMENTWISE_NAMES
    for names in ELEMENTWISE_NAMES.values():
        for name in names:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = C.c_int, _PROTOTYPES[name][1]
    return lib


def _col(dtype, size=4, unit=0):
    from libgdf_amd._binding import gdf_column
    c = gdf_column()
    c.data, c.size, c.dtype = FAKE_DEV if size else None, size, dtype
    c.dtype_info.time_unit = unit
    return c


def _binary_names():
    return [(op, sfx) for op, sfxs in ref.BINARY_SUFFIXES.items() for sfx in sfxs]


def _out_dtype(op, dtype):
    return INT8 if op in ref.COMPARE_OPS else dtype


def test_the_name_lists_cover_182_entry_points(gdf):
    from libgdf_amd._binding import ELEMENTWISE_NAMES
    names = [n for v in ELEMENTWISE_NAMES.values() for n in v]
    assert len(names) == len(set(names)) == 182
    assert len(ELEMENTWISE_NAMES["binary"]) == 23 + 36 + 12 and len(ELEMENTWISE_NAMES["unary_time_unit"]) == 9
    assert len(ELEMENTWISE_NAMES["unary"]) == 33 + 63 + 6


def test_null_column_pointers_everywhere(gdf):
    from libgdf_amd._binding import ELEMENTWISE_NAMES
    a = _col(FLOAT32)
    for name in ELEMENTWISE_NAMES["binary"]:
        for args in ((None, None, None), (C.byref(a), C.byref(a), None), (None, C.byref(a), C.byref(a)), (C.byref(a), None, C.byref(a))):
            assert getattr(gdf, name)(*args) == GDF_UNSUPPORTED_METHOD, name
    for name in ELEMENTWISE_NAMES["unary"]:
        for args in ((None, None), (C.byref(a), None), (None, C.byref(a))):
            assert getattr(gdf, name)(*args) == GDF_UNSUPPORTED_METHOD, name
    for name in ELEMENTWISE_NAMES["unary_time_unit"]:
        for args in ((None, None, 1), (C.byref(a), None, 1), (None, C.byref(a), 1)):
            assert getattr(gdf, name)(*args) == GDF_UNSUPPORTED_METHOD, name


@pytest.mark.parametrize("op,sfx", _binary_names())
def test_binary_checks(gdf, op, sfx):
    fn = getattr(gdf, f"gdf_{op}_{sfx}")
    dt = ref.SUFFIX_DTYPE[sfx]
    out_dt = _out_dtype(op, dt)
    # size 0 on either input: success before any other check (even a dtype mismatch), nothing touched
    for ls, rs in ((0, 4), (4, 0), (0, 0)):
        o = _col(STRING, 7)
        assert fn(C.byref(_col(dt, ls)), C.byref(_col(FLOAT64 if dt != FLOAT64 else INT8, rs)), C.byref(o)) == GDF_SUCCESS
        assert (o.dtype, o.size) == (STRING, 7)
    assert fn(C.byref(_col(dt, 4)), C.byref(_col(dt, 5)), C.byref(_col(out_dt, 4))) == GDF_COLUMN_SIZE_MISMATCH
    assert fn(C.byref(_col(dt, 4)), C.byref(_col(dt, 4)), C.byref(_col(out_dt, 5))) == GDF_COLUMN_SIZE_MISMATCH
    assert fn(C.byref(_col(dt, 4)), C.byref(_col(dt, 5)), C.byref(_col(STRING, 4))) == GDF_COLUMN_SIZE_MISMATCH      # size before dtype
    other = INT32 if dt != INT32 else INT64
    assert fn(C.byref(_col(dt, 4)), C.byref(_col(other, 4)), C.byref(_col(out_dt, 4))) == GDF_UNSUPPORTED_DTYPE
    wrong_out = INT16 if out_dt != INT16 else INT8
    assert fn(C.byref(_col(dt, 4)), C.byref(_col(dt, 4)), C.byref(_col(wrong_out, 4))) == GDF_UNSUPPORTED_DTYPE
    if op in ref.COMPARE_OPS and dt != INT8:
        assert fn(C.byref(_col(dt, 4)), C.byref(_col(dt, 4)), C.byref(_col(dt, 4))) == GDF_UNSUPPORTED_DTYPE         # comparisons write int8
    # a non-empty column without data
    bad = _col(dt, 4)
    bad.data = None
    assert fn(C.byref(bad), C.byref(_col(dt, 4)), C.byref(_col(out_dt, 4))) == GDF_INVALID_API_CALL


GENERIC_TABLES = {
    **{op: {INT32, INT64, FLOAT32, FLOAT64} for op in ref.ARITH_OPS},
    "div": {FLOAT32, FLOAT64},
    **{op: {INT8, INT32, INT64, FLOAT32, FLOAT64, DATE32, DATE64, TIMESTAMP} for op in ref.COMPARE_OPS},
    **{op: {INT8, INT32, INT64} for op in ref.BITWISE_OPS},
}


@pytest.mark.parametrize("op", list(GENERIC_TABLES))
def test_binary_generic_dispatch_table(gdf, op):
    """a dtype the table takes passes the dispatch and then fails on a size mismatch made for the purpose (3); any other dtype is
    refused by the dispatch (2)"""
    fn = getattr(gdf, f"gdf_{op}_generic")
    for dt in ALL_DTYPES:
        rc = fn(C.byref(_col(dt, 4)), C.byref(_col(dt, 4)), C.byref(_col(_out_dtype(op, dt), 5)))
        assert rc == (GDF_COLUMN_SIZE_MISMATCH if dt in GENERIC_TABLES[op] else GDF_UNSUPPORTED_DTYPE), (op, dt)
        assert fn(C.byref(_col(dt, 0)), C.byref(_col(dt, 0)), C.byref(_col(dt, 0))) == GDF_SUCCESS
    dt = sorted(GENERIC_TABLES[op])[-1]
    assert fn(C.byref(_col(dt, 4)), C.byref(_col(dt, 4)), C.byref(_col(INT16, 4))) == GDF_UNSUPPORTED_DTYPE


@pytest.mark.parametrize("op", ref.MATH_OPS)
def test_math_checks(gdf, op):
    for sfx, dt in (("f32", FLOAT32), ("f64", FLOAT64), ("generic", FLOAT32), ("generic", FLOAT64)):
        fn = getattr(gdf, f"gdf_{op}_{sfx}")
        assert fn(C.byref(_col(dt, 0)), C.byref(_col(dt, 3))) == GDF_SUCCESS
        assert fn(C.byref(_col(dt, 4)), C.byref(_col(dt, 3))) == GDF_COLUMN_SIZE_MISMATCH
        bad = _col(dt, 4)
        bad.data = None
        assert fn(C.byref(_col(dt, 4)), C.byref(bad)) == GDF_INVALID_API_CALL
    fn = getattr(gdf, f"gdf_{op}_generic")
    for dt in ALL_DTYPES:
        if dt not in (FLOAT32, FLOAT64):
            assert fn(C.byref(_col(dt, 4)), C.byref(_col(dt, 4))) == GDF_UNSUPPORTED_DTYPE, dt


def _cast_call(gdf, src, dst, i, o, unit=ref.UNIT_US):
    fn = getattr(gdf, f"gdf_cast_{src}_to_{dst}")
    return fn(C.byref(i), C.byref(o), unit) if dst == "timestamp" else fn(C.byref(i), C.byref(o))


@pytest.mark.parametrize("dst", ref.CAST_TARGETS)
@pytest.mark.parametrize("src", ref.CAST_SOURCES)
def test_cast_checks(gdf, src, dst):
    sdt, ddt = ref.SUFFIX_DTYPE[src], ref.SUFFIX_DTYPE[dst]
    # the source check: any other dtype is refused, and nothing of the output is written
    for dt in ALL_DTYPES:
        if dt != sdt:
            o = _col(STRING, 4, unit=ref.UNIT_S)
            assert _cast_call(gdf, src, dst, _col(dt, 4), o) == GDF_UNSUPPORTED_DTYPE
            assert (o.dtype, o.dtype_info.time_unit) == (STRING, ref.UNIT_S)
    o = _col(STRING, 5, unit=ref.UNIT_S)
    assert _cast_call(gdf, src, dst, _col(sdt, 4), o) == GDF_COLUMN_SIZE_MISMATCH
    assert (o.dtype, o.dtype_info.time_unit) == (STRING, ref.UNIT_S)
    assert _cast_call(gdf, src, dst, _col(sdt, 4), _col(STRING, 5)) == GDF_COLUMN_SIZE_MISMATCH
    # a size-0 cast succeeds and still types its output
    o = _col(STRING, 0, unit=ref.UNIT_S)
    assert _cast_call(gdf, src, dst, _col(sdt, 0), o) == GDF_SUCCESS
    assert o.dtype == ddt
    assert o.dtype_info.time_unit == (ref.UNIT_US if dst == "timestamp" else ref.UNIT_S)


@pytest.mark.parametrize("dst", ref.CAST_TARGETS)
def test_cast_generic_dispatch_table(gdf, dst):
    for dt in ALL_DTYPES:
        o = _col(STRING, 0)
        rc = _cast_call(gdf, "generic", dst, _col(dt, 0), o)
        if dt in (INT8, INT32, INT64, FLOAT32, FLOAT64, DATE32, DATE64, TIMESTAMP):
            assert rc == GDF_SUCCESS and o.dtype == ref.SUFFIX_DTYPE[dst], dt
        else:
            assert rc == GDF_UNSUPPORTED_DTYPE and o.dtype == STRING, dt            # INT16 too, as in the reference


@pytest.mark.parametrize("field", ref.DATETIME_FIELDS)
def test_datetime_checks(gdf, field):
    fn = getattr(gdf, f"gdf_extract_datetime_{field}")
    for dt in (DATE32, DATE64, TIMESTAMP):
        assert fn(C.byref(_col(dt, 4)), C.byref(_col(INT16, 5))) == GDF_COLUMN_SIZE_MISMATCH
        assert fn(C.byref(_col(dt, 4)), C.byref(_col(INT32, 4))) == GDF_UNSUPPORTED_DTYPE
        assert fn(C.byref(_col(dt, 4)), C.byref(_col(INT32, 5))) == GDF_COLUMN_SIZE_MISMATCH                         # size first, as the reference
    for dt in ALL_DTYPES:
        if dt not in (DATE32, DATE64, TIMESTAMP):
            assert fn(C.byref(_col(dt, 4)), C.byref(_col(INT16, 4))) == GDF_UNSUPPORTED_DTYPE, dt
    assert fn(C.byref(_col(DATE64, 0)), C.byref(_col(INT16, 0))) == GDF_SUCCESS
    assert fn(C.byref(_col(TIMESTAMP, 0, unit=ref.UNIT_NS)), C.byref(_col(INT16, 0))) == GDF_SUCCESS
    # DATE32 has a calendar date and no time of day
    want = GDF_SUCCESS if field in ("year", "month", "day") else GDF_UNSUPPORTED_DTYPE
    assert fn(C.byref(_col(DATE32, 0)), C.byref(_col(INT16, 0))) == want
    bad = _col(DATE64, 4)
    bad.data = None
    assert fn(C.byref(bad), C.byref(_col(INT16, 4))) == GDF_INVALID_API_CALL
