"""No-GPU checks of gdf_amd_group_by_agg (csrc/groupby_agg.hip): the name is exported and declared in include/gdf/gdf_amd_ext.h, and
every argument error of its contract comes back from the host-side checks -- the device pointers below are fake and never
dereferenced -- in the documented order, with the output structs untouched.  rows == 0 succeeds without device work."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libgdf_amd", "lib")
HEADER = os.path.join(ROOT, "include", "gdf", "gdf_amd_ext.h")

(GDF_UNSUPPORTED_DTYPE, GDF_COLUMN_SIZE_MISMATCH, GDF_COLUMN_SIZE_TOO_BIG, GDF_DATASET_EMPTY, GDF_INVALID_API_CALL,
 GDF_JOIN_TOO_MANY_COLUMNS, GDF_UNSUPPORTED_METHOD) = 2, 3, 4, 5, 8, 10, 12
I8, I16, I32, I64, F32, F64, DATE32, DATE64, TIMESTAMP, CATEGORY, STRING = range(1, 12)
SUM, MIN, MAX, AVG, COUNT, COUNT_DISTINCT = range(6)
FAKE_DEV = 0x1000          # never dereferenced: every call below either fails its host-side checks or has no rows
MAX_KEYS, MAX_VALUES, MAX_AGGS = 16, 64, 64


@pytest.fixture(scope="module")
def gdf():
    C.CDLL(os.path.join(LIBDIR, "libgdf_testhook.so"), mode=C.RTLD_GLOBAL)
    C.CDLL(os.path.join(LIBDIR, "librmm.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIBDIR, "libgdf.so"), mode=C.RTLD_GLOBAL)
    from libgdf_amd._binding import _PROTOTYPES
    for name in ("gdf_amd_group_by_agg", "gdf_error_get_name"):
        restype, argtypes = _PROTOTYPES[name]
        getattr(lib, name).restype = C.c_int if restype is None else restype
        getattr(lib, name).argtypes = argtypes
    return lib


def _col(dtype, size=4, data=FAKE_DEV, valid=None, time_unit=0):
    from libgdf_amd._binding import gdf_column
    c = gdf_column()
    c.data, c.valid, c.size, c.dtype = data, valid, size, dtype
    c.dtype_info.time_unit = time_unit
    return c


def _array(cols):
    from libgdf_amd._binding import gdf_column
    return (C.POINTER(gdf_column) * max(len(cols), 1))(*[C.pointer(c) if c is not None else None for c in cols])


def _aggs(reqs):
    from libgdf_amd._binding import gdf_amd_agg
    arr = (gdf_amd_agg * max(len(reqs), 1))()
    for r, (col, op) in zip(arr, reqs):
        r.column, r.op = col, op
    return arr


def _snapshot(c):
    return bytes(C.string_at(C.addressof(c), C.sizeof(c)))


def call(gdf, keys, values, reqs, nkeys=None, nvalues=None, naggs=None, null=(), null_out_key=None, null_out_agg=None):
    """-> (return code, out key structs, out aggregate structs, whether they are byte-identical to their 0xAB fill).
    null: which of the five pointer arguments to pass as NULL; null_out_key / null_out_agg: the index of a NULL element"""
    from libgdf_amd._binding import gdf_column
    nk = len(keys) if nkeys is None else nkeys
    nv = len(values) if nvalues is None else nvalues
    na = len(reqs) if naggs is None else naggs
    out_keys = [gdf_column() for _ in range(max(len(keys), nk, 1))]
    out_aggs = [gdf_column() for _ in range(max(len(reqs), na, 1))]
    for o in out_keys + out_aggs:
        C.memset(C.byref(o), 0xAB, C.sizeof(o))
    before = [_snapshot(o) for o in out_keys + out_aggs]
    ok_arr = _array([None if i == null_out_key else o for i, o in enumerate(out_keys)])
    oa_arr = _array([None if i == null_out_agg else o for i, o in enumerate(out_aggs)])
    rc = gdf.gdf_amd_group_by_agg(None if "keys" in null else _array(keys), nk,
                                  None if "values" in null else _array(values), nv,
                                  None if "aggs" in null else _aggs(reqs), na,
                                  None if "out_keys" in null else ok_arr, None if "out_aggs" in null else oa_arr)
    return rc, out_keys, out_aggs, [_snapshot(o) for o in out_keys + out_aggs] == before


def test_the_name_is_exported_declared_and_bound(gdf):
    from libgdf_amd import api
    from libgdf_amd._binding import gdf_amd_agg
    with open(HEADER) as f:
        text = f.read()
    assert hasattr(gdf, "gdf_amd_group_by_agg")
    assert re.search(r"\bgdf_error\s+gdf_amd_group_by_agg\s*\(", text)
    assert re.search(r"typedef\s+struct\s+gdf_amd_agg\s*\{\s*int32_t\s+column;\s*int32_t\s+op;\s*\}\s*gdf_amd_agg;", text)
    assert C.sizeof(gdf_amd_agg) == 8
    assert callable(api.group_by_agg)


def test_sizeof_the_request_struct_in_c(tmp_path):
    """the header's own struct, through the C compiler"""
    import subprocess
    src = tmp_path / "size.c"
    src.write_text('#include <gdf/gdf_amd_ext.h>\n_Static_assert(sizeof(gdf_amd_agg) == 8, "gdf_amd_agg");\n'
                   '_Static_assert(GDF_SUM == 0 && GDF_MIN == 1 && GDF_MAX == 2 && GDF_AVG == 3 && GDF_COUNT == 4 && GDF_COUNT_DISTINCT == 5, "ops");\n')
    subprocess.check_call(["gcc", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])


def test_the_error_numbers_are_the_headers(gdf):
    names = {GDF_UNSUPPORTED_DTYPE: "GDF_UNSUPPORTED_DTYPE", GDF_COLUMN_SIZE_MISMATCH: "GDF_COLUMN_SIZE_MISMATCH",
             GDF_COLUMN_SIZE_TOO_BIG: "GDF_COLUMN_SIZE_TOO_BIG", GDF_DATASET_EMPTY: "GDF_DATASET_EMPTY",
             GDF_INVALID_API_CALL: "GDF_INVALID_API_CALL", GDF_JOIN_TOO_MANY_COLUMNS: "GDF_JOIN_TOO_MANY_COLUMNS",
             GDF_UNSUPPORTED_METHOD: "GDF_UNSUPPORTED_METHOD"}
    for code, name in names.items():
        assert gdf.gdf_error_get_name(code).decode() == name


def _cases():
    key, val = (lambda **k: _col(I32, **k)), (lambda **k: _col(F64, **k))
    one = [(0, SUM)]
    # 1. GDF_DATASET_EMPTY
    yield "keys NULL", dict(keys=[key()], values=[val()], reqs=one, null=("keys",)), GDF_DATASET_EMPTY
    yield "nkeys 0", dict(keys=[key()], values=[val()], reqs=one, nkeys=0), GDF_DATASET_EMPTY
    yield "nkeys negative", dict(keys=[key()], values=[val()], reqs=one, nkeys=-1), GDF_DATASET_EMPTY
    yield "NULL key", dict(keys=[key(), None], values=[val()], reqs=one), GDF_DATASET_EMPTY
    yield "nvalues negative", dict(keys=[key()], values=[val()], reqs=[(-1, COUNT)], nvalues=-1), GDF_DATASET_EMPTY
    yield "values NULL with nvalues 1", dict(keys=[key()], values=[val()], reqs=one, null=("values",)), GDF_DATASET_EMPTY
    yield "NULL value", dict(keys=[key()], values=[val(), None], reqs=one), GDF_DATASET_EMPTY
    yield "aggs NULL", dict(keys=[key()], values=[val()], reqs=one, null=("aggs",)), GDF_DATASET_EMPTY
    yield "naggs 0", dict(keys=[key()], values=[val()], reqs=one, naggs=0), GDF_DATASET_EMPTY
    yield "naggs negative", dict(keys=[key()], values=[val()], reqs=one, naggs=-3), GDF_DATASET_EMPTY
    yield "out_keys NULL", dict(keys=[key()], values=[val()], reqs=one, null=("out_keys",)), GDF_DATASET_EMPTY
    yield "out_aggs NULL", dict(keys=[key()], values=[val()], reqs=one, null=("out_aggs",)), GDF_DATASET_EMPTY
    yield "NULL out key", dict(keys=[key(), key()], values=[val()], reqs=one, null_out_key=1), GDF_DATASET_EMPTY
    yield "NULL out aggregate", dict(keys=[key()], values=[val()], reqs=[(0, SUM), (0, MIN)], null_out_agg=1), GDF_DATASET_EMPTY
    # 2., 3. the limits
    yield "17 keys", dict(keys=[key() for _ in range(MAX_KEYS + 1)], values=[val()], reqs=one), GDF_JOIN_TOO_MANY_COLUMNS
    yield "65 values", dict(keys=[key()], values=[val() for _ in range(MAX_VALUES + 1)], reqs=one), GDF_INVALID_API_CALL
    yield "65 requests", dict(keys=[key()], values=[val()], reqs=one * (MAX_AGGS + 1)), GDF_INVALID_API_CALL
    # 4. sizes
    yield "key sizes differ", dict(keys=[key(), key(size=5)], values=[val()], reqs=one), GDF_COLUMN_SIZE_MISMATCH
    yield "value size differs", dict(keys=[key()], values=[val(), val(size=3)], reqs=one), GDF_COLUMN_SIZE_MISMATCH
    yield "unreferenced value size differs", dict(keys=[key()], values=[val(size=3)], reqs=[(-1, COUNT)]), GDF_COLUMN_SIZE_MISMATCH
    # 5. key dtypes
    for bad in (0, CATEGORY, STRING, 12, -1):
        yield f"key dtype {bad}", dict(keys=[key(), _col(bad)], values=[val()], reqs=one), GDF_UNSUPPORTED_DTYPE
    # 6. the requests
    for bad in (COUNT_DISTINCT, 6, -1, 100):
        yield f"op {bad}", dict(keys=[key()], values=[val()], reqs=[(0, SUM), (0, bad)]), GDF_UNSUPPORTED_METHOD
    yield "column == nvalues", dict(keys=[key()], values=[val()], reqs=[(1, SUM)]), GDF_INVALID_API_CALL
    yield "column -2", dict(keys=[key()], values=[val()], reqs=[(-2, COUNT)]), GDF_INVALID_API_CALL
    yield "column 0 without values", dict(keys=[key()], values=[], reqs=[(0, COUNT)], null=("values",)), GDF_INVALID_API_CALL
    for op in (SUM, MIN, MAX, AVG):
        yield f"column -1 with op {op}", dict(keys=[key()], values=[val()], reqs=[(-1, op)]), GDF_INVALID_API_CALL
    for op in (SUM, AVG):
        for bad in (DATE32, DATE64, TIMESTAMP, CATEGORY, STRING, 0):
            yield f"op {op} of dtype {bad}", dict(keys=[key()], values=[_col(bad)], reqs=[(0, op)]), GDF_UNSUPPORTED_DTYPE
    for op in (MIN, MAX, COUNT):
        for bad in (CATEGORY, STRING, 0, 12):
            yield f"op {op} of dtype {bad}", dict(keys=[key()], values=[_col(bad)], reqs=[(0, op)]), GDF_UNSUPPORTED_DTYPE
    # 7., 8.
    yield "rows == 2^31 - 1", dict(keys=[_col(I8, size=2**31 - 1)], values=[], reqs=[(-1, COUNT)]), GDF_COLUMN_SIZE_TOO_BIG
    yield "rows == 2^33", dict(keys=[_col(I8, size=2**33)], values=[_col(I8, size=2**33)], reqs=one), GDF_COLUMN_SIZE_TOO_BIG
    yield "key without data", dict(keys=[key(), key(data=None)], values=[val()], reqs=one), GDF_DATASET_EMPTY
    yield "referenced value without data", dict(keys=[key()], values=[val(), val(data=None)], reqs=[(0, SUM), (1, COUNT)]), GDF_DATASET_EMPTY
    # the ORDER of the checks
    yield "NULL out aggregate before 17 keys", dict(keys=[key() for _ in range(17)], values=[val()], reqs=one, null_out_agg=0), GDF_DATASET_EMPTY
    yield "17 keys before 65 requests", dict(keys=[key() for _ in range(17)], values=[val()], reqs=one * 65), GDF_JOIN_TOO_MANY_COLUMNS
    yield "65 requests before sizes", dict(keys=[key(), key(size=5)], values=[val()], reqs=one * 65), GDF_INVALID_API_CALL
    yield "sizes before a key dtype", dict(keys=[_col(STRING), key(size=5)], values=[val()], reqs=one), GDF_COLUMN_SIZE_MISMATCH
    yield "a key dtype before a bad request", dict(keys=[_col(STRING)], values=[val()], reqs=[(0, COUNT_DISTINCT)]), GDF_UNSUPPORTED_DTYPE
    yield "op before column", dict(keys=[key()], values=[val()], reqs=[(7, COUNT_DISTINCT)]), GDF_UNSUPPORTED_METHOD
    yield "column before value dtype", dict(keys=[key()], values=[_col(STRING)], reqs=[(0, SUM), (3, SUM)]), GDF_UNSUPPORTED_DTYPE
    yield "requests in array order", dict(keys=[key()], values=[_col(STRING)], reqs=[(3, SUM), (0, SUM)]), GDF_INVALID_API_CALL
    yield "a bad request before rows too big", dict(keys=[_col(I8, size=2**33)], values=[_col(I8, size=2**33)], reqs=[(0, 9)]), GDF_UNSUPPORTED_METHOD
    yield "rows too big before missing data", dict(keys=[_col(I8, size=2**33, data=None)], values=[], reqs=[(-1, COUNT)]), GDF_COLUMN_SIZE_TOO_BIG


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_host_side_errors_leave_the_outputs_untouched(gdf, case):
    _, kw, want = case
    rc, _, _, untouched = call(gdf, **kw)
    assert rc == want
    assert untouched


def test_an_unreferenced_value_column_needs_no_data(gdf):
    """check 8 looks at the key columns and at the value columns some request names: with rows == 0 nothing is looked at"""
    rc, _, _, _ = call(gdf, keys=[_col(I32, size=0, data=None)], values=[_col(F64, size=0, data=None)], reqs=[(0, SUM)])
    assert rc == 0


def test_every_allowed_value_dtype_passes_its_ops_check(gdf):
    """(with no rows the call then succeeds: no device work)"""
    for op, dtypes in ((SUM, range(I8, F64 + 1)), (AVG, range(I8, F64 + 1)), (MIN, range(I8, TIMESTAMP + 1)), (MAX, range(I8, TIMESTAMP + 1)),
                       (COUNT, range(I8, TIMESTAMP + 1))):
        for dtype in dtypes:
            rc, _, _, _ = call(gdf, keys=[_col(I64, size=0, data=None)], values=[_col(dtype, size=0, data=None)], reqs=[(0, op)])
            assert rc == 0, (op, dtype)
    for dtype in range(I8, TIMESTAMP + 1):                                          # ... and every key dtype
        rc, _, _, _ = call(gdf, keys=[_col(dtype, size=0, data=None)], values=[], reqs=[(-1, COUNT)], null=("values",))
        assert rc == 0, dtype


def test_zero_rows_gives_zero_size_outputs_with_the_right_dtypes(gdf):
    keys = [_col(TIMESTAMP, size=0, data=None, time_unit=2), _col(F32, size=0, data=None, valid=FAKE_DEV)]
    values = [_col(TIMESTAMP, size=0, data=None, time_unit=3), _col(I8, size=0, data=None), _col(F32, size=0, data=None), _col(DATE32, size=0, data=None)]
    reqs = [(0, MIN), (0, MAX), (0, COUNT), (1, SUM), (1, AVG), (1, MIN), (2, SUM), (2, MAX), (3, MIN), (-1, COUNT)]
    rc, out_keys, out_aggs, _ = call(gdf, keys=keys, values=values, reqs=reqs)
    assert rc == 0

    def fields(o):
        return (o.data, o.valid, o.size, o.dtype, o.null_count, o.dtype_info.time_unit)

    assert [fields(o) for o in out_keys] == [(None, None, 0, TIMESTAMP, 0, 2), (None, None, 0, F32, 0, 0)]
    want = [(TIMESTAMP, 3), (TIMESTAMP, 3), (I64, 0), (I64, 0), (F64, 0), (I8, 0), (F64, 0), (F32, 0), (DATE32, 0), (I64, 0)]
    assert [fields(o) for o in out_aggs] == [(None, None, 0, d, 0, u) for d, u in want]
