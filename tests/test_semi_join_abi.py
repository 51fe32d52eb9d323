"""No-GPU checks of gdf_amd_semi_join (csrc/semijoin.hip): the name is exported, declared in include/gdf/gdf_amd_ext.h and wrapped, and
every argument error of its contract comes back from the host-side checks -- the device pointers below are fake and never
dereferenced -- in the order the contract gives, with out_indices untouched.  Each ordering case violates two conditions and must
report the earlier one."""
import ctypes as C
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libgdf_amd", "lib")
HEADER = os.path.join(ROOT, "include", "gdf", "gdf_amd_ext.h")

(GDF_UNSUPPORTED_DTYPE, GDF_COLUMN_SIZE_MISMATCH, GDF_COLUMN_SIZE_TOO_BIG, GDF_DATASET_EMPTY, GDF_INVALID_API_CALL, GDF_JOIN_DTYPE_MISMATCH,
 GDF_JOIN_TOO_MANY_COLUMNS) = 2, 3, 4, 5, 8, 9, 10
I8, I16, I32, I64, F32, F64, DATE32, DATE64, TIMESTAMP, CATEGORY, STRING = range(1, 12)
FAKE_DEV = 0x1000          # never dereferenced: every call below ends in the host-side checks
MAX_KEY_COLS = 16
ROWS = 4                   # the key columns' size unless a case says otherwise
ANTI, NULLS_EQUAL = 1, 2


@pytest.fixture(scope="module")
def gdf():
    C.CDLL(os.path.join(LIBDIR, "libgdf_testhook.so"), mode=C.RTLD_GLOBAL)
    C.CDLL(os.path.join(LIBDIR, "librmm.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIBDIR, "libgdf.so"), mode=C.RTLD_GLOBAL)
    from libgdf_amd._binding import _PROTOTYPES
    restype, argtypes = _PROTOTYPES["gdf_amd_semi_join"]
    lib.gdf_amd_semi_join.restype = C.c_int if restype is None else restype
    lib.gdf_amd_semi_join.argtypes = argtypes
    return lib


def _col(dtype, size=ROWS, data=FAKE_DEV, valid=None):
    from libgdf_amd._binding import gdf_column
    c = gdf_column()
    c.data, c.valid, c.size, c.dtype = data, valid, size, dtype
    return c


def _array(cols):
    from libgdf_amd._binding import gdf_column
    return (C.POINTER(gdf_column) * len(cols))(*[C.pointer(c) if c is not None else None for c in cols])


def _out():
    """an output struct with recognisable junk in it: an error must leave every byte"""
    return _col(F64, size=77, data=0xDEAD0, valid=0xBEEF0)


def _snapshot(c):
    return bytes(C.string_at(C.addressof(c), C.sizeof(c)))


def _call(gdf, left, right, ncols, flags, out="junk"):
    if out == "junk":
        out = _out()
    before = _snapshot(out) if out is not None else None
    la = _array(left) if left is not None else None
    ra = _array(right) if right is not None else None
    rc = gdf.gdf_amd_semi_join(la, ra, ncols, flags, C.byref(out) if out is not None else None)
    if out is not None and rc != 0:
        assert _snapshot(out) == before
    return rc, out


def test_the_name_is_exported_declared_and_wrapped(gdf):
    with open(HEADER) as f:
        text = f.read()
    assert hasattr(gdf, "gdf_amd_semi_join")
    assert re.search(r"\bgdf_error\s+gdf_amd_semi_join\s*\(\s*gdf_column\s*\*\*\s*left_cols\s*,\s*gdf_column\s*\*\*\s*right_cols\s*,\s*int\s+ncols\s*,"
                     r"\s*uint32_t\s+flags\s*,\s*gdf_column\s*\*\s*out_indices\s*\)", text)
    assert re.search(r"#define\s+GDF_AMD_SEMI_ANTI\s+1u", text) and re.search(r"#define\s+GDF_AMD_SEMI_NULLS_EQUAL\s+2u", text)
    from libgdf_amd import api
    assert callable(api.semi_join)
    params = inspect.signature(api.semi_join).parameters
    assert list(params) == ["left", "right", "anti", "nulls_equal"]
    assert params["anti"].default is False and params["nulls_equal"].default is False
    assert (api.SEMI_ANTI, api.SEMI_NULLS_EQUAL) == (ANTI, NULLS_EQUAL)


def _cases():
    key = lambda **kw: _col(I32, **kw)
    # each condition alone
    yield "left_cols NULL", None, [key()], 1, 0, "junk", GDF_DATASET_EMPTY
    yield "right_cols NULL", [key()], None, 1, 0, "junk", GDF_DATASET_EMPTY
    yield "out_indices NULL", [key()], [key()], 1, 0, None, GDF_DATASET_EMPTY
    yield "ncols 0", [key()], [key()], 0, 0, "junk", GDF_DATASET_EMPTY
    yield "ncols negative", [key()], [key()], -1, 0, "junk", GDF_DATASET_EMPTY
    yield "NULL left element", [key(), None], [key(), key()], 2, 0, "junk", GDF_DATASET_EMPTY
    yield "NULL right element", [key(), key()], [None, key()], 2, 0, "junk", GDF_DATASET_EMPTY
    yield "17 columns", [key() for _ in range(17)], [key() for _ in range(17)], 17, 0, "junk", GDF_JOIN_TOO_MANY_COLUMNS
    yield "left sizes differ", [key(), key(size=5)], [key(), key()], 2, 0, "junk", GDF_COLUMN_SIZE_MISMATCH
    yield "right sizes differ", [key(), key()], [key(size=9), key(size=8)], 2, 0, "junk", GDF_COLUMN_SIZE_MISMATCH
    for bad in (0, CATEGORY, STRING, 12, -1):
        yield f"left dtype {bad}", [key(), _col(bad)], [key(), key()], 2, 0, "junk", GDF_UNSUPPORTED_DTYPE
        yield f"right dtype {bad}", [key(), key()], [key(), _col(bad)], 2, 0, "junk", GDF_UNSUPPORTED_DTYPE
    yield "both sides STRING", [_col(STRING)], [_col(STRING)], 1, 0, "junk", GDF_UNSUPPORTED_DTYPE
    yield "INT32 against INT64", [key()], [_col(I64)], 1, 0, "junk", GDF_JOIN_DTYPE_MISMATCH
    yield "INT32 against DATE32", [key()], [_col(DATE32)], 1, 0, "junk", GDF_JOIN_DTYPE_MISMATCH
    yield "DATE64 against TIMESTAMP in the second column", [key(), _col(DATE64)], [key(), _col(TIMESTAMP)], 2, 0, "junk", GDF_JOIN_DTYPE_MISMATCH
    for bad in (4, 8, 0x80, 0x80000000, 0xFFFFFFFC, 7):
        yield f"flags {bad:#x}", [key()], [key()], 1, bad, "junk", GDF_INVALID_API_CALL
    yield "left rows == 2^31 - 1", [_col(I8, size=2**31 - 1)], [_col(I8)], 1, 0, "junk", GDF_COLUMN_SIZE_TOO_BIG
    yield "right rows == 2^31 - 1", [_col(I8)], [_col(I8, size=2**31 - 1)], 1, 0, "junk", GDF_COLUMN_SIZE_TOO_BIG
    yield "right rows == 2^33", [_col(I8)], [_col(I8, size=2**33)], 1, ANTI, "junk", GDF_COLUMN_SIZE_TOO_BIG
    yield "left column without data", [key(), key(data=None)], [key(), key()], 2, 0, "junk", GDF_DATASET_EMPTY
    yield "right column without data", [key(), key()], [key(data=None), key()], 2, 0, "junk", GDF_DATASET_EMPTY
    # the order: each call violates two conditions and reports the earlier one
    yield "NULL element and 17 columns", [None] + [key() for _ in range(16)], [key() for _ in range(17)], 17, 0, "junk", GDF_DATASET_EMPTY
    yield "out NULL and sizes differ", [key(), key(size=5)], [key(), key()], 2, 0, None, GDF_DATASET_EMPTY
    yield "17 columns and sizes differ", [key(size=i) for i in range(17)], [key() for _ in range(17)], 17, 0, "junk", GDF_JOIN_TOO_MANY_COLUMNS
    yield "sizes differ and a bad dtype", [key(), _col(STRING, size=5)], [key(), key()], 2, 0, "junk", GDF_COLUMN_SIZE_MISMATCH
    yield "bad dtype and a dtype mismatch", [_col(STRING), key()], [_col(STRING), _col(I64)], 2, 0, "junk", GDF_UNSUPPORTED_DTYPE
    yield "bad right dtype in column 1 and a mismatch in column 0", [key(), key()], [_col(I64), _col(STRING)], 2, 0, "junk", GDF_UNSUPPORTED_DTYPE
    yield "dtype mismatch and bad flags", [key()], [_col(I64)], 1, 4, "junk", GDF_JOIN_DTYPE_MISMATCH
    yield "bad flags and too many rows", [_col(I8, size=2**31 - 1)], [_col(I8)], 1, 4, "junk", GDF_INVALID_API_CALL
    yield "too many rows and no data", [_col(I8, size=2**31 - 1, data=None)], [_col(I8)], 1, 0, "junk", GDF_COLUMN_SIZE_TOO_BIG
    yield "too many right rows and no left data", [_col(I8, data=None)], [_col(I8, size=2**31 - 1)], 1, 0, "junk", GDF_COLUMN_SIZE_TOO_BIG
    yield "sizes differ and no data", [key(), key(size=5, data=None)], [key(), key()], 2, 0, "junk", GDF_COLUMN_SIZE_MISMATCH


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_host_side_errors_leave_the_output_untouched(gdf, case):
    _, left, right, ncols, flags, out, want = case
    rc, _ = _call(gdf, left, right, ncols, flags, out)
    assert rc == want


def test_every_key_dtype_passes_the_dtype_checks(gdf):
    """(INT8 ... TIMESTAMP on both sides reach the NEXT check: a flag error here)"""
    for dtype in range(I8, TIMESTAMP + 1):
        rc, _ = _call(gdf, [_col(dtype)], [_col(dtype)], 1, 4)
        assert rc == GDF_INVALID_API_CALL


@pytest.mark.parametrize("flags", [0, ANTI, NULLS_EQUAL, ANTI | NULLS_EQUAL])
def test_a_left_side_without_rows_is_success_without_device_work(gdf, flags):
    """no left rows: nothing qualifies under any flag; the output is filled in -- size 0, data NULL, no mask, GDF_INT32 -- from fake
    pointers that are never dereferenced, with or without right rows, data pointers and masks"""
    for left, right in (([_col(F64, size=0, data=None)], [_col(F64, valid=FAKE_DEV)]),
                        ([_col(F64, size=0)], [_col(F64, size=0, data=None)]),
                        ([_col(I8, size=0, data=None, valid=FAKE_DEV), _col(I64, size=0, data=None)], [_col(I8), _col(I64)])):
        rc, out = _call(gdf, left, right, len(left), flags)
        assert rc == 0
        assert (out.size, out.data, out.valid, out.dtype, out.null_count) == (0, None, None, I32, 0)


def test_a_right_column_without_data_is_fine_when_the_right_side_has_no_rows(gdf):
    """(the data check looks at the sides that have rows only: with left rows this call goes on to the device, so it is made with no
    left rows either)"""
    rc, out = _call(gdf, [_col(I32, size=0, data=None)], [_col(I32, size=0, data=None)], 1, ANTI)
    assert rc == 0 and out.size == 0 and out.data is None
