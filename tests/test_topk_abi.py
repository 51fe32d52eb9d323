"""No-GPU checks of gdf_amd_top_k (csrc/topk.hip): the name is exported, declared in include/gdf/gdf_amd_ext.h and wrapped, and every
argument error of its contract comes back from the host-side checks -- the device pointers below are fake and never dereferenced --
in the order the contract gives, with out_indices untouched."""
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
FAKE_DEV = 0x1000          # never dereferenced: every call below ends in the host-side checks
MAX_KEY_COLS = 16
ROWS = 4                   # the key columns' size unless a case says otherwise


@pytest.fixture(scope="module")
def gdf():
    C.CDLL(os.path.join(LIBDIR, "libgdf_testhook.so"), mode=C.RTLD_GLOBAL)
    C.CDLL(os.path.join(LIBDIR, "librmm.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIBDIR, "libgdf.so"), mode=C.RTLD_GLOBAL)
    from libgdf_amd._binding import _PROTOTYPES
    restype, argtypes = _PROTOTYPES["gdf_amd_top_k"]
    lib.gdf_amd_top_k.restype = C.c_int if restype is None else restype
    lib.gdf_amd_top_k.argtypes = argtypes
    return lib


def _col(dtype, size=ROWS, data=FAKE_DEV, valid=None):
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


def _call(gdf, cols, ncols, flags, k, offset, out):
    before = _snapshot(out) if out is not None else None
    arr = _array(cols) if cols is not None else None
    rc = gdf.gdf_amd_top_k(arr, ncols, _flags(flags), k, offset, C.byref(out) if out is not None else None)
    if out is not None:
        assert _snapshot(out) == before
    return rc


def test_the_name_is_exported_declared_and_wrapped(gdf):
    with open(HEADER) as f:
        text = f.read()
    assert hasattr(gdf, "gdf_amd_top_k")
    assert re.search(r"\bgdf_error\s+gdf_amd_top_k\s*\(\s*gdf_column\s*\*\*\s*cols\s*,\s*int\s+ncols\s*,\s*const\s+uint8_t\s*\*\s*flags\s*,"
                     r"\s*int64_t\s+k\s*,\s*int64_t\s+offset\s*,\s*gdf_column\s*\*\s*out_indices\s*\)", text)
    from libgdf_amd import api
    assert callable(api.top_k)
    import inspect
    assert list(inspect.signature(api.top_k).parameters) == ["cols", "k", "descending", "nulls_first", "offset"]
    assert inspect.signature(api.top_k).parameters["offset"].default == 0


def _cases():
    key = lambda **kw: _col(I32, **kw)
    out = lambda size=2, **kw: _col(I32, size=size, **kw)          # k = 2, offset = 0 over 4 rows: m = 2
    # gdf_amd_order_by_ex's cases on cols and flags, with its codes
    yield "cols NULL", None, 1, None, 2, 0, out(), GDF_DATASET_EMPTY
    yield "ncols 0", [key()], 0, None, 2, 0, out(), GDF_DATASET_EMPTY
    yield "ncols negative", [key()], -1, None, 2, 0, out(), GDF_DATASET_EMPTY
    yield "NULL element", [key(), None], 2, None, 2, 0, out(), GDF_DATASET_EMPTY
    yield "NULL first element", [None, key()], 2, None, 2, 0, out(), GDF_DATASET_EMPTY
    yield "17 columns", [key() for _ in range(MAX_KEY_COLS + 1)], MAX_KEY_COLS + 1, None, 2, 0, out(), GDF_JOIN_TOO_MANY_COLUMNS
    yield "sizes differ", [key(), key(size=5)], 2, None, 2, 0, out(), GDF_COLUMN_SIZE_MISMATCH
    for bad in (0, CATEGORY, STRING, 12, -1):
        yield f"key dtype {bad}", [key(), _col(bad)], 2, None, 2, 0, out(), GDF_UNSUPPORTED_DTYPE
    for bad in (4, 8, 0x80, 0xFF):
        yield f"flag byte {bad:#x}", [key(), key()], 2, [0, bad], 2, 0, out(), GDF_INVALID_API_CALL
    yield "flag byte 4 on the first column", [key(), key()], 2, [4, 3], 2, 0, out(), GDF_INVALID_API_CALL
    # k and offset
    yield "k = -1", [key()], 1, None, -1, 0, out(size=0), GDF_INVALID_API_CALL
    yield "offset = -1", [key()], 1, None, 2, -1, out(), GDF_INVALID_API_CALL
    yield "k = INT64_MIN", [key()], 1, None, -2**63, 0, out(), GDF_INVALID_API_CALL
    # out_indices
    yield "out_indices NULL", [key()], 1, None, 2, 0, None, GDF_INVALID_API_CALL
    yield "out_indices INT64", [key()], 1, None, 2, 0, _col(I64, size=2), GDF_INVALID_API_CALL
    yield "out_indices DATE32", [key()], 1, None, 2, 0, _col(DATE32, size=2), GDF_INVALID_API_CALL
    yield "out_indices of size m - 1", [key()], 1, None, 2, 0, out(size=1), GDF_INVALID_API_CALL
    yield "out_indices of size m + 1", [key()], 1, None, 2, 0, out(size=3), GDF_INVALID_API_CALL
    yield "out_indices of size k where the table ends first", [key()], 1, None, 3, 2, out(size=3), GDF_INVALID_API_CALL
    yield "out_indices of size rows", [key()], 1, None, 2, 0, out(size=ROWS), GDF_INVALID_API_CALL
    yield "out_indices without data", [key()], 1, None, 2, 0, out(data=None), GDF_INVALID_API_CALL
    yield "out_indices with a mask", [key()], 1, None, 2, 0, out(valid=FAKE_DEV), GDF_VALIDITY_UNSUPPORTED
    yield "m == 0 and out_indices with a mask", [key()], 1, None, 0, 0, out(size=0, data=None, valid=FAKE_DEV), GDF_VALIDITY_UNSUPPORTED
    yield "rows == 2^31 - 1", [_col(I8, size=2**31 - 1)], 1, None, 2, 0, out(), GDF_COLUMN_SIZE_TOO_BIG
    yield "rows == 2^31 - 1, k = rows", [_col(I8, size=2**31 - 1)], 1, None, 2**31 - 1, 0, out(size=2**31 - 1), GDF_COLUMN_SIZE_TOO_BIG
    yield "rows == 2^33, m == 0", [_col(I8, size=2**33)], 1, [3], 0, 0, out(size=0), GDF_COLUMN_SIZE_TOO_BIG
    yield "a key column without data", [key(), key(data=None)], 2, None, 2, 0, out(), GDF_DATASET_EMPTY
    # the order of the checks: a bad dtype before a bad flag before a bad k before a bad output before the mask (before the row count,
    # before the data pointers)
    yield "bad dtype and bad flag", [_col(STRING)], 1, [4], -1, 0, _col(I64), GDF_UNSUPPORTED_DTYPE
    yield "bad flag and bad k", [key()], 1, [4], -1, 0, _col(I64), GDF_INVALID_API_CALL
    yield "bad k and a masked output", [key()], 1, None, -1, 0, out(size=0, valid=FAKE_DEV), GDF_INVALID_API_CALL
    yield "bad offset and a masked output", [key()], 1, None, 2, -5, out(valid=FAKE_DEV), GDF_INVALID_API_CALL
    yield "masked output of the wrong dtype", [key()], 1, None, 2, 0, _col(I64, size=2, valid=FAKE_DEV), GDF_INVALID_API_CALL
    yield "masked output of the wrong size", [key()], 1, None, 2, 0, out(size=3, valid=FAKE_DEV), GDF_INVALID_API_CALL
    yield "masked output and too many rows", [_col(I8, size=2**31 - 1)], 1, None, 2, 0, out(valid=FAKE_DEV), GDF_VALIDITY_UNSUPPORTED
    yield "too many rows and no data", [_col(I8, size=2**31 - 1, data=None)], 1, None, 2, 0, out(), GDF_COLUMN_SIZE_TOO_BIG
    yield "sizes differ and a bad k", [key(), key(size=5)], 2, None, -1, 0, out(), GDF_COLUMN_SIZE_MISMATCH


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_host_side_errors_leave_the_output_untouched(gdf, case):
    _, cols, ncols, flags, k, offset, out, want = case
    assert _call(gdf, cols, ncols, flags, k, offset, out) == want


def test_a_bad_k_without_a_mask_is_told_from_a_bad_output(gdf):
    """(k = -1 and offset = -1 come back as GDF_INVALID_API_CALL, the code of a bad output too: a masked output of the right shape
    tells them apart -- the mask check comes later and reports GDF_VALIDITY_UNSUPPORTED once k and offset are good)"""
    masked = _col(I32, size=2, valid=FAKE_DEV)
    assert _call(gdf, [_col(I32)], 1, None, 2, 0, masked) == GDF_VALIDITY_UNSUPPORTED
    assert _call(gdf, [_col(I32)], 1, None, -1, 0, masked) == GDF_INVALID_API_CALL
    assert _call(gdf, [_col(I32)], 1, None, 2, -1, masked) == GDF_INVALID_API_CALL


def test_m_zero_is_success_without_device_work(gdf):
    """k == 0, rows == 0 and offset >= rows: success from fake pointers (nothing is dereferenced: a fake pointer would fault), with
    masks, flags and no data pointers at all"""
    for flags in (None, [0], [3]):
        for key, k, offset in ((_col(F64, valid=FAKE_DEV), 0, 0), (_col(F64, valid=FAKE_DEV), 0, 3),
                               (_col(F64, size=0, data=None), 5, 0), (_col(F64, size=0, data=None), 0, 0),
                               (_col(F64), 5, ROWS), (_col(F64, data=None), 2**62, ROWS + 1), (_col(F64), 2**63 - 1, 2**63 - 1)):
            assert _call(gdf, [key], 1, flags, k, offset, _col(I32, size=0, data=None)) == 0
            assert _call(gdf, [key], 1, flags, k, offset, _col(I32, size=0, data=FAKE_DEV)) == 0
            assert _call(gdf, [key], 1, flags, k, offset, _col(I32, size=1)) == GDF_INVALID_API_CALL


def test_every_key_dtype_passes_the_dtype_check(gdf):
    """(INT8 ... TIMESTAMP reach the NEXT check: a flag error here, not GDF_UNSUPPORTED_DTYPE)"""
    for dtype in range(I8, TIMESTAMP + 1):
        assert _call(gdf, [_col(dtype)], 1, [4], 2, 0, _col(I32, size=2)) == GDF_INVALID_API_CALL
