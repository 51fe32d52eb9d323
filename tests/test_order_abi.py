"""No-GPU checks of gdf_amd_order_by_ex and gdf_amd_gather (csrc/order.hip): both names are exported and declared in
include/gdf/gdf_amd_ext.h, and every argument error of their contracts comes back from the host-side checks -- the device pointers
below are fake and never dereferenced -- with the output structs untouched."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libgdf_amd", "lib")
HEADER = os.path.join(ROOT, "include", "gdf", "gdf_amd_ext.h")

(GDF_UNSUPPORTED_DTYPE, GDF_COLUMN_SIZE_MISMATCH, GDF_COLUMN_SIZE_TOO_BIG, GDF_DATASET_EMPTY, GDF_VALIDITY_UNSUPPORTED, GDF_INVALID_API_CALL,
 GDF_JOIN_TOO_MANY_COLUMNS) = 2, 3, 4, 5, 7, 8, 10
I8, I16, I32, I64, F32, F64, DATE32, DATE64, TIMESTAMP, CATEGORY, STRING = range(1, 12)
FAKE_DEV = 0x1000          # never dereferenced: every call below fails its host-side checks first
MAX_KEY_COLS = 16


@pytest.fixture(scope="module")
def gdf():
    C.CDLL(os.path.join(LIBDIR, "libgdf_testhook.so"), mode=C.RTLD_GLOBAL)
    C.CDLL(os.path.join(LIBDIR, "librmm.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIBDIR, "libgdf.so"), mode=C.RTLD_GLOBAL)
    from libgdf_amd._binding import _PROTOTYPES
    for name in ("gdf_amd_order_by_ex", "gdf_amd_gather", "gdf_error_get_name"):
        restype, argtypes = _PROTOTYPES[name]
        getattr(lib, name).restype = C.c_int if restype is None else restype
        getattr(lib, name).argtypes = argtypes
    return lib


def _col(dtype, size=4, data=FAKE_DEV, valid=None):
    from libgdf_amd._binding import gdf_column
    c = gdf_column()
    c.data, c.valid, c.size, c.dtype = data, valid, size, dtype
    return c


def _array(cols):
    from libgdf_amd._binding import gdf_column
    return (C.POINTER(gdf_column) * len(cols))(*[C.pointer(c) if c is not None else None for c in cols])


def _flags(values):
    return None if values is None else (C.c_uint8 * len(values))(*values)


def _snapshot(c):
    return bytes(C.string_at(C.addressof(c), C.sizeof(c)))


def test_both_names_are_exported_and_declared(gdf):
    with open(HEADER) as f:
        text = f.read()
    for name in ("gdf_amd_order_by_ex", "gdf_amd_gather"):
        assert hasattr(gdf, name)
        assert re.search(r"\bgdf_error\s+" + name + r"\s*\(", text), name
    assert re.search(r"#define\s+GDF_AMD_ORDER_DESC\s+1u", text) and re.search(r"#define\s+GDF_AMD_ORDER_NULLS_FIRST\s+2u", text)
    from libgdf_amd import api
    assert (api.ORDER_DESC, api.ORDER_NULLS_FIRST) == (1, 2)


def test_the_error_numbers_are_the_headers(gdf):
    names = {GDF_UNSUPPORTED_DTYPE: "GDF_UNSUPPORTED_DTYPE", GDF_COLUMN_SIZE_MISMATCH: "GDF_COLUMN_SIZE_MISMATCH",
             GDF_COLUMN_SIZE_TOO_BIG: "GDF_COLUMN_SIZE_TOO_BIG", GDF_DATASET_EMPTY: "GDF_DATASET_EMPTY",
             GDF_VALIDITY_UNSUPPORTED: "GDF_VALIDITY_UNSUPPORTED", GDF_INVALID_API_CALL: "GDF_INVALID_API_CALL",
             GDF_JOIN_TOO_MANY_COLUMNS: "GDF_JOIN_TOO_MANY_COLUMNS"}
    for code, name in names.items():
        assert gdf.gdf_error_get_name(code).decode() == name


# ---- gdf_amd_order_by_ex -------------------------------------------------------------------------------------------------------------
def _order_cases():
    key, out = (lambda **k: _col(I32, **k)), (lambda **k: _col(I32, **k))
    yield "cols NULL", None, 1, None, out(), GDF_DATASET_EMPTY
    yield "ncols 0", [key()], 0, None, out(), GDF_DATASET_EMPTY
    yield "ncols negative", [key()], -1, None, out(), GDF_DATASET_EMPTY
    yield "NULL element", [key(), None], 2, None, out(), GDF_DATASET_EMPTY
    yield "NULL first element", [None, key()], 2, None, out(), GDF_DATASET_EMPTY
    yield "17 columns", [key() for _ in range(MAX_KEY_COLS + 1)], MAX_KEY_COLS + 1, None, out(), GDF_JOIN_TOO_MANY_COLUMNS
    yield "sizes differ", [key(), key(size=5)], 2, None, out(), GDF_COLUMN_SIZE_MISMATCH
    for bad in (0, CATEGORY, STRING, 12, -1):
        yield f"key dtype {bad}", [key(), _col(bad)], 2, None, out(), GDF_UNSUPPORTED_DTYPE
    for bad in (4, 8, 0x80, 0xFF):
        yield f"flag byte {bad:#x}", [key(), key()], 2, [0, bad], out(), GDF_INVALID_API_CALL
    yield "flag byte 4 on the first column", [key(), key()], 2, [4, 3], out(), GDF_INVALID_API_CALL
    yield "out_indices NULL", [key()], 1, None, None, GDF_INVALID_API_CALL
    yield "out_indices INT64", [key()], 1, None, _col(I64), GDF_INVALID_API_CALL
    yield "out_indices DATE32", [key()], 1, None, _col(DATE32), GDF_INVALID_API_CALL
    yield "out_indices of another size", [key()], 1, None, out(size=3), GDF_INVALID_API_CALL
    yield "out_indices larger", [key()], 1, None, out(size=5), GDF_INVALID_API_CALL
    yield "out_indices without data", [key()], 1, None, out(data=None), GDF_INVALID_API_CALL
    yield "out_indices with a mask", [key()], 1, None, out(valid=FAKE_DEV), GDF_VALIDITY_UNSUPPORTED
    yield "rows == 2^31 - 1", [_col(I8, size=2**31 - 1)], 1, None, out(size=2**31 - 1), GDF_COLUMN_SIZE_TOO_BIG
    yield "rows == 2^33", [_col(I8, size=2**33)], 1, [3], out(size=2**33), GDF_COLUMN_SIZE_TOO_BIG
    # the order of the checks: the key columns before the flags before the output
    yield "bad dtype and bad flag", [_col(STRING)], 1, [4], out(), GDF_UNSUPPORTED_DTYPE
    yield "bad flag and bad output", [key()], 1, [4], _col(I64), GDF_INVALID_API_CALL
    yield "masked output of the wrong dtype", [key()], 1, None, _col(I64, valid=FAKE_DEV), GDF_INVALID_API_CALL


@pytest.mark.parametrize("case", list(_order_cases()), ids=lambda c: c[0])
def test_order_by_ex_host_side_errors_leave_the_output_untouched(gdf, case):
    _, cols, ncols, flags, out, want = case
    before = _snapshot(out) if out is not None else None
    arr = _array(cols) if cols is not None else None
    assert gdf.gdf_amd_order_by_ex(arr, ncols, _flags(flags), C.byref(out) if out is not None else None) == want
    if out is not None:
        assert _snapshot(out) == before


def test_order_by_ex_zero_rows_is_success(gdf):
    """rows == 0: nothing is written and no device work happens -- also with masks, flags and no data pointers at all"""
    for flags in (None, [0], [3]):
        out = _col(I32, size=0, data=None)
        before = _snapshot(out)
        key = _col(F64, size=0, data=None, valid=None)
        assert gdf.gdf_amd_order_by_ex(_array([key]), 1, _flags(flags), C.byref(out)) == 0
        assert _snapshot(out) == before
    out = _col(I32, size=0, data=None, valid=FAKE_DEV)
    assert gdf.gdf_amd_order_by_ex(_array([_col(I8, size=0, data=None)]), 1, None, C.byref(out)) == GDF_VALIDITY_UNSUPPORTED


def test_every_key_dtype_of_order_by_passes_the_dtype_check(gdf):
    """(INT8 ... TIMESTAMP reach the NEXT check: a flag error here, not GDF_UNSUPPORTED_DTYPE)"""
    for dtype in range(I8, TIMESTAMP + 1):
        out = _col(I32)
        assert gdf.gdf_amd_order_by_ex(_array([_col(dtype)]), 1, _flags([4]), C.byref(out)) == GDF_INVALID_API_CALL


# ---- gdf_amd_gather ------------------------------------------------------------------------------------------------------------------
def _gather_cases():
    idx, src = (lambda **k: _col(I32, **k)), (lambda **k: _col(F64, **k))
    yield "indices NULL", None, 1, [src()], True, GDF_DATASET_EMPTY
    yield "cols NULL", idx(), 1, None, True, GDF_DATASET_EMPTY
    yield "outs NULL", idx(), 1, [src()], False, GDF_DATASET_EMPTY
    yield "ncols 0", idx(), 0, [src()], True, GDF_DATASET_EMPTY
    yield "ncols negative", idx(), -2, [src()], True, GDF_DATASET_EMPTY
    yield "NULL source", idx(), 2, [src(), None], True, GDF_DATASET_EMPTY
    yield "indices without data", idx(data=None), 1, [src()], True, GDF_DATASET_EMPTY
    yield "source without data", idx(), 2, [src(), src(data=None)], True, GDF_DATASET_EMPTY
    yield "source sizes differ", idx(), 2, [src(), src(size=5)], True, GDF_COLUMN_SIZE_MISMATCH
    for bad in (0, I8, I16, F32, F64, DATE32, DATE64, TIMESTAMP, CATEGORY, 12):
        yield f"index dtype {bad}", _col(bad), 1, [src()], True, GDF_UNSUPPORTED_DTYPE
    for bad in (0, CATEGORY, STRING, 12, -1):
        yield f"source dtype {bad}", idx(), 2, [src(), _col(bad)], True, GDF_UNSUPPORTED_DTYPE
    yield "indices with a mask", idx(valid=FAKE_DEV), 1, [src()], True, GDF_VALIDITY_UNSUPPORTED
    yield "int64 indices with a mask", _col(I64, valid=FAKE_DEV), 1, [src()], True, GDF_VALIDITY_UNSUPPORTED


@pytest.mark.parametrize("case", list(_gather_cases()), ids=lambda c: c[0])
def test_gather_host_side_errors_leave_the_outputs_untouched(gdf, case):
    from libgdf_amd._binding import gdf_column
    _, indices, ncols, cols, with_outs, want = case
    n = len(cols) if cols is not None else 1
    outs = [gdf_column() for _ in range(n)]
    for o in outs:
        C.memset(C.byref(o), 0xAB, C.sizeof(o))
    before = [_snapshot(o) for o in outs]
    rc = gdf.gdf_amd_gather(C.byref(indices) if indices is not None else None, ncols, _array(cols) if cols is not None else None,
                            _array(outs) if with_outs else None)
    assert rc == want
    assert [_snapshot(o) for o in outs] == before


def test_gather_of_no_indices_allocates_nothing(gdf):
    """m == 0: size 0, data == valid == NULL, dtype and dtype_info of the source -- no device work, so it runs without a GPU"""
    from libgdf_amd._binding import gdf_column
    src = _col(TIMESTAMP, size=7)
    src.dtype_info.time_unit = 3
    out = gdf_column()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    for idx_dtype in (I32, I64):
        assert gdf.gdf_amd_gather(C.byref(_col(idx_dtype, size=0, data=None)), 1, _array([src]), _array([out])) == 0
        assert (out.data, out.valid, out.size, out.dtype, out.null_count, out.dtype_info.time_unit) == (None, None, 0, TIMESTAMP, 0, 3)
