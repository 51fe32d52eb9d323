"""No-GPU checks of gdf_to_csr (csrc/csr.hip): the layout of csr_gdf, every argument error that returns before any device work, and
the numpy restatement of the contract (tests/csr_reference.py) on a case written out by hand.

Layout: csr_gdf is A@0 IA@8 JA@16 dtype@24 nnz@32 rows@40 cols@48, 56 bytes, and IA points at 8-byte elements -- gdf_size_type is
size_t in the reference's types.h:3 and in include/gdf/gdf.h (tests/test_abi.py pins sizeof(gdf_column) == 56 on the same typedef).
tests/golden/reference_csr_layout.json is the table the reference's own convert_types.h gives under gcc."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import csr_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libgdf_amd", "lib")
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_csr_layout.json")

GDF_UNSUPPORTED_DTYPE, GDF_COLUMN_SIZE_MISMATCH, GDF_COLUMN_SIZE_TOO_BIG, GDF_DATASET_EMPTY, GDF_INVALID_API_CALL = 2, 3, 4, 5, 8
FAKE_DEV = 0x1000          # never dereferenced: every call below fails its host-side checks first
FIELDS = ("A", "IA", "JA", "dtype", "nnz", "rows", "cols")

_LAYOUT_PROGRAM = r"""
#include <stdio.h>
#include <stddef.h>
#include <gdf/gdf.h>
int main(void) {
  printf("{\"sizeof\": %zu, \"A\": %zu, \"IA\": %zu, \"JA\": %zu, \"dtype\": %zu, \"nnz\": %zu, \"rows\": %zu, \"cols\": %zu, "
         "\"sizeof_IA_element\": %zu}\n", sizeof(csr_gdf), offsetof(csr_gdf, A), offsetof(csr_gdf, IA), offsetof(csr_gdf, JA),
         offsetof(csr_gdf, dtype), offsetof(csr_gdf, nnz), offsetof(csr_gdf, rows), offsetof(csr_gdf, cols),
         sizeof(*((csr_gdf *)0)->IA));
  return 0;
}
"""


@pytest.fixture(scope="module")
def gdf():
    C.CDLL(os.path.join(LIBDIR, "libgdf_testhook.so"), mode=C.RTLD_GLOBAL)
    C.CDLL(os.path.join(LIBDIR, "librmm.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIBDIR, "libgdf.so"), mode=C.RTLD_GLOBAL)
    from libgdf_amd._binding import _PROTOTYPES
    restype, argtypes = _PROTOTYPES["gdf_to_csr"]
    lib.gdf_to_csr.restype = C.c_int if restype is None else restype
    lib.gdf_to_csr.argtypes = argtypes
    return lib


def _col(dtype, size=4, data=FAKE_DEV, valid=None):
    from libgdf_amd._binding import gdf_column
    c = gdf_column()
    c.data, c.valid, c.size, c.dtype = data, valid, size, dtype
    return c


def _array(cols):
    from libgdf_amd._binding import gdf_column
    return (C.POINTER(gdf_column) * len(cols))(*[C.pointer(c) if c is not None else None for c in cols])


def _poisoned():
    from libgdf_amd._binding import csr_gdf
    csr = csr_gdf()
    C.memset(C.byref(csr), 0xAB, C.sizeof(csr))
    return csr, bytes(csr)


def test_csr_gdf_layout():
    """the ctypes mirror, gcc's table of include/gdf/gdf.h and the reference header's recorded table agree"""
    from libgdf_amd._binding import csr_gdf
    want = dict(sizeof=56, A=0, IA=8, JA=16, dtype=24, nnz=32, rows=40, cols=48, sizeof_IA_element=8)
    mirror = {f: getattr(csr_gdf, f).offset for f in FIELDS}
    mirror["sizeof"] = C.sizeof(csr_gdf)
    mirror["sizeof_IA_element"] = C.sizeof(C.c_size_t)
    assert mirror == want
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "t.c"), "w") as f:
            f.write(_LAYOUT_PROGRAM)
        exe = os.path.join(d, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", exe])
        ours = json.loads(subprocess.check_output([exe]).decode())
    assert ours == want
    with open(GOLDEN) as f:
        assert json.load(f) == want


def test_null_table_is_dataset_empty(gdf):
    """the stub answered GDF_UNSUPPORTED_METHOD (12) to every call"""
    csr, before = _poisoned()
    assert gdf.gdf_to_csr(None, 0, C.byref(csr)) == GDF_DATASET_EMPTY
    assert bytes(csr) == before


def _cases():
    i32, i32b, f64 = _col(3), _col(3), _col(6)
    yield "csrReturn NULL", [i32, f64], 2, False, GDF_INVALID_API_CALL
    yield "gdfData NULL", None, 2, True, GDF_DATASET_EMPTY
    yield "num_cols 0", [i32], 0, True, GDF_DATASET_EMPTY
    yield "num_cols negative", [i32], -1, True, GDF_DATASET_EMPTY
    yield "NULL element", [i32, None, f64], 3, True, GDF_DATASET_EMPTY
    yield "NULL first element", [None, f64], 2, True, GDF_DATASET_EMPTY
    yield "NULL data, rows > 0", [i32, _col(3, data=None)], 2, True, GDF_DATASET_EMPTY
    yield "sizes differ", [i32, _col(3, size=5)], 2, True, GDF_COLUMN_SIZE_MISMATCH
    yield "sizes differ, one empty", [_col(3, size=0, data=None), i32b], 2, True, GDF_COLUMN_SIZE_MISMATCH
    for bad in (0, 7, 8, 9, 10, 11, 12, -1):                      # GDF_invalid, DATE32, DATE64, TIMESTAMP, CATEGORY, STRING, beyond
        yield f"dtype {bad}", [i32, _col(bad)], 2, True, GDF_UNSUPPORTED_DTYPE
    yield "dtype 11 alone", [_col(11)], 1, True, GDF_UNSUPPORTED_DTYPE
    # without any mask nnz = rows * cols is known on the host
    yield "nnz > INT32_MAX, no masks", [_col(1, size=2**31), _col(1, size=2**31)], 2, True, GDF_COLUMN_SIZE_TOO_BIG
    yield "nnz == INT32_MAX + 1, one column", [_col(6, size=2**31)], 1, True, GDF_COLUMN_SIZE_TOO_BIG


@pytest.mark.parametrize("case", list(_cases()), ids=lambda c: c[0])
def test_host_side_errors_leave_the_result_untouched(gdf, case):
    _, cols, num_cols, with_result, want = case
    csr, before = _poisoned()
    arr = _array(cols) if cols is not None else None
    assert gdf.gdf_to_csr(arr, num_cols, C.byref(csr) if with_result else None) == want
    assert bytes(csr) == before


def test_reference_on_a_case_written_by_hand():
    """4 rows x 3 columns: int16, float32 (no mask), int64 -> FLOAT32 (the largest enumerator, not the widest type).
         row 0:  c0 valid    c1    c2 null
         row 1:  c0 null     c1    c2 valid
         row 2:  c0 null     c1    c2 null
         row 3:  c0 valid    c1    c2 valid      (mask bits 4 .. 7 are set too and must not count)"""
    c0 = np.array([7, -1, -2, -32768], dtype=np.int16)
    c1 = np.array([0.0, np.nan, -0.0, 1.5], dtype=np.float32)
    c2 = np.array([99, 2**24 + 1, 5, -3], dtype=np.int64)
    m0 = np.array([0b11111001], dtype=np.uint8)
    m2 = np.array([0b11111010], dtype=np.uint8)
    A, IA, JA, dtype = csr_reference.to_csr([(c0, m0), (c1, None), (c2, m2)])
    assert dtype == 5 and A.dtype == np.float32
    assert IA.tolist() == [0, 2, 4, 5, 8]
    assert JA.tolist() == [0, 1, 1, 2, 1, 0, 1, 2]
    want = np.array([7.0, 0.0, np.nan, 16777216.0, -0.0, -32768.0, 1.5, -3.0], dtype=np.float32)     # 2^24 + 1 rounds to even
    assert np.array_equal(csr_reference.bits_of(A), csr_reference.bits_of(want))
    # no entries at all
    A, IA, JA, dtype = csr_reference.to_csr([(c0, np.array([0xF0], dtype=np.uint8))])
    assert (len(A), IA.tolist(), len(JA), dtype) == (0, [0, 0, 0, 0, 0], 0, 2)
