"""No-GPU checks of read_csv / gdf_amd_read_csv_device / gdf_amd_read_csv_release (csrc/csv.hip): the layout of csv_read_arg, every
argument error of the contract in include/gdf/gdf.h -- each returns before any device work and leaves the three output fields of a
poisoned csv_read_arg untouched -- and the empty file, which needs no device either.  The stub this replaces answered
GDF_UNSUPPORTED_METHOD (12) to every call."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libgdf_amd", "lib")

GDF_UNSUPPORTED_DTYPE, GDF_INVALID_API_CALL, GDF_FILE_ERROR = 2, 8, 19
DTYPE_STRINGS = ["str", "category", "date", "date64", "date32", "timestamp", "float", "float32", "float64", "double", "short", "int",
                 "int32", "int64", "long"]
FAKE_DEV = 0x1000          # never dereferenced: every call that gets it fails its host-side checks first

_LAYOUT_PROGRAM = r"""
#include <stdio.h>
#include <stddef.h>
#include <gdf/gdf.h>
#define F(f) printf("\"" #f "\": %zu, ", offsetof(csv_read_arg, f))
int main(void) {
  printf("{");
  F(num_cols_out); F(num_rows_out); F(data); F(file_path); F(lineterminator); F(delimiter); F(delim_whitespace); F(skipinitialspace);
  F(num_cols); F(names); F(dtype); F(skiprows); F(skipfooter); F(dayfirst);
  printf("\"sizeof\": %zu}\n", sizeof(csv_read_arg));
  return 0;
}
"""


@pytest.fixture(scope="module")
def gdf():
    C.CDLL(os.path.join(LIBDIR, "libgdf_testhook.so"), mode=C.RTLD_GLOBAL)
    C.CDLL(os.path.join(LIBDIR, "librmm.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIBDIR, "libgdf.so"), mode=C.RTLD_GLOBAL)
    from libgdf_amd._binding import _PROTOTYPES
    for name in ("read_csv", "gdf_amd_read_csv_device", "gdf_amd_read_csv_release"):
        restype, argtypes = _PROTOTYPES[name]
        getattr(lib, name).restype = C.c_int if restype is None else restype
        getattr(lib, name).argtypes = argtypes
    return lib


def _strings(values):
    return (C.c_char_p * len(values))(*[None if v is None else v.encode() for v in values])


def _args(names=("a", "b"), dtypes=("int", "float64"), path=None, num_cols=None, skiprows=0, skipfooter=0):
    """a csv_read_arg whose every byte is 0xAB except the input fields set here; returns it with what it points to"""
    from libgdf_amd._binding import csv_read_arg
    a = csv_read_arg()
    C.memset(C.byref(a), 0xAB, C.sizeof(a))
    keep = [None if names is None else _strings(names), None if dtypes is None else _strings(dtypes)]
    a.names = keep[0] if keep[0] is not None else C.POINTER(C.c_char_p)()
    a.dtype = keep[1] if keep[1] is not None else C.POINTER(C.c_char_p)()
    a.num_cols = len(names) if num_cols is None else num_cols
    a.file_path = None if path is None else os.fsencode(path)
    a.delimiter, a.lineterminator = b",", b"\n"
    a.delim_whitespace = a.skipinitialspace = a.dayfirst = False
    a.skiprows, a.skipfooter = skiprows, skipfooter
    return a, keep


def test_csv_read_arg_layout():
    """the ctypes mirror and gcc's table of include/gdf/gdf.h agree (the struct is the reference's io_types.h:26-60, whose prototype
    digest tests/test_abi.py pins)"""
    from libgdf_amd._binding import csv_read_arg
    mirror = {name: getattr(csv_read_arg, name).offset for name, _ in csv_read_arg._fields_}
    mirror["sizeof"] = C.sizeof(csv_read_arg)
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(_LAYOUT_PROGRAM)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", exe])
        ours = json.loads(subprocess.check_output([exe]).decode())
    assert ours == mirror
    assert (mirror["num_cols_out"], mirror["num_rows_out"], mirror["data"], mirror["sizeof"]) == (0, 4, 8, 64)


def _cases(tmp):
    missing = os.path.join(tmp, "no_such_file.csv")
    present = os.path.join(tmp, "present.csv")                     # (written by the test: a call that got this far would read it)
    yield "num_cols 0", dict(path=present, num_cols=0), GDF_INVALID_API_CALL
    yield "num_cols negative", dict(path=present, num_cols=-3), GDF_INVALID_API_CALL
    yield "names NULL", dict(path=present, names=None, num_cols=2), GDF_INVALID_API_CALL
    yield "dtype NULL", dict(path=present, dtypes=None), GDF_INVALID_API_CALL
    yield "a NULL name", dict(path=present, names=("a", None)), GDF_INVALID_API_CALL
    yield "a NULL dtype string", dict(path=present, dtypes=(None, "int")), GDF_INVALID_API_CALL
    yield "skiprows negative", dict(path=present, skiprows=-1), GDF_INVALID_API_CALL
    yield "skipfooter negative", dict(path=present, skipfooter=-1), GDF_INVALID_API_CALL
    yield "a NULL name before an unknown dtype", dict(path=present, names=("a", None), dtypes=("int", "int8")), GDF_INVALID_API_CALL
    for bad in ("int8", "INT64", "", "float16", "string", "int64 ", "bool", "datetime"):
        yield f"unknown dtype {bad!r}", dict(path=present, dtypes=("int", bad)), GDF_UNSUPPORTED_DTYPE
    yield "unknown dtype before a missing file", dict(path=missing, dtypes=("uint8", "int")), GDF_UNSUPPORTED_DTYPE
    yield "file_path NULL", dict(path=None), GDF_FILE_ERROR
    yield "a missing file", dict(path=missing), GDF_FILE_ERROR
    yield "a directory", dict(path=tmp), GDF_FILE_ERROR
    yield "every known dtype string, a missing file", dict(path=missing, names=DTYPE_STRINGS, dtypes=DTYPE_STRINGS), GDF_FILE_ERROR


CASE_NAMES = [name for name, _, _ in _cases("")]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_argument_errors_leave_the_outputs_untouched(gdf, tmp_path, name):
    (tmp_path / "present.csv").write_bytes(b"1,2.5\n")
    kw, want = {n: (k, w) for n, k, w in _cases(str(tmp_path))}[name]
    a, keep = _args(**kw)
    before = bytes(a)
    assert gdf.read_csv(C.byref(a)) == want
    assert bytes(a) == before
    # the device-buffer entry point makes the same checks of the same arguments (file_path is not one of them there)
    if want != GDF_FILE_ERROR:
        assert gdf.gdf_amd_read_csv_device(FAKE_DEV, 100, C.byref(a)) == want
        assert bytes(a) == before


def test_null_arguments(gdf):
    assert gdf.read_csv(None) == GDF_INVALID_API_CALL
    assert gdf.gdf_amd_read_csv_device(FAKE_DEV, 100, None) == GDF_INVALID_API_CALL
    assert gdf.gdf_amd_read_csv_release(None) == GDF_INVALID_API_CALL
    a, keep = _args()
    before = bytes(a)
    assert gdf.gdf_amd_read_csv_device(None, 100, C.byref(a)) == GDF_INVALID_API_CALL               # no bytes, but a length
    assert bytes(a) == before


@pytest.mark.parametrize("through", ["file", "buffer"])
def test_empty_input_is_zero_rows_and_release_frees_it(gdf, tmp_path, through):
    """no bytes: no record, so no device work -- the columns exist, named and typed, with size 0 and NULL buffers"""
    names, dtypes = ("loan_id", "when", "rate", "flag"), ("int64", "date", "float32", "category")
    path = tmp_path / "empty.csv"
    path.write_bytes(b"")
    a, keep = _args(names, dtypes, path=str(path), skiprows=2)
    rc = gdf.read_csv(C.byref(a)) if through == "file" else gdf.gdf_amd_read_csv_device(None, 0, C.byref(a))
    assert rc == 0
    assert (a.num_cols_out, a.num_rows_out) == (4, 0) and a.data
    for c, (name, code) in enumerate(zip(names, (4, 8, 5, 10))):
        col = a.data[c].contents
        assert (col.col_name, col.dtype, col.size, col.null_count, col.data, col.valid) == (name.encode(), code, 0, 0, None, None)
        assert col.dtype_info.time_unit == 0
    assert gdf.gdf_amd_read_csv_release(C.byref(a)) == 0
    assert (a.num_cols_out, a.num_rows_out, bool(a.data)) == (0, 0, False)
    assert gdf.gdf_amd_read_csv_release(C.byref(a)) == 0                                            # nothing left: nothing done
    assert a.num_cols == 4 and a.skiprows == 2                                                      # the inputs stay
