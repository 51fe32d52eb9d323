"""No-GPU checks of the whole-column reductions and quantiles (csrc/reduce.hip, csrc/quantile.hip): every argument error returns
before any device work, and the numpy restatement of the quantile rule the GPU tests use reproduces the reference's known answers."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from stats_reference import QUANTILE_METHODS, quantile_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libgdf_amd", "lib")

GDF_UNSUPPORTED_DTYPE, GDF_DATASET_EMPTY, GDF_VALIDITY_UNSUPPORTED, GDF_INVALID_API_CALL = 2, 5, 7, 8
GDF_DTYPE_MISMATCH, GDF_UNSUPPORTED_METHOD = 11, 12
FAKE_DEV = 0x1000          # never dereferenced: every call below fails its host-side checks first


@pytest.fixture(scope="module")
def gdf():
    C.CDLL(os.path.join(LIBDIR, "libgdf_testhook.so"), mode=C.RTLD_GLOBAL)
    C.CDLL(os.path.join(LIBDIR, "librmm.so"), mode=C.RTLD_GLOBAL)
    lib = C.CDLL(os.path.join(LIBDIR, "libgdf.so"), mode=C.RTLD_GLOBAL)
    from libgdf_amd._binding import _PROTOTYPES
    for name, (restype, argtypes) in _PROTOTYPES.items():
        if name.startswith(("gdf_sum", "gdf_product", "gdf_min", "gdf_max", "gdf_quantile", "gdf_reduce")):
            fn = getattr(lib, name)
            fn.restype = C.c_int if restype is None else restype
            fn.argtypes = argtypes
    return lib


def _col(dtype, size=4, valid=None):
    from libgdf_amd._binding import gdf_column
    c = gdf_column()
    c.data, c.valid, c.size, c.dtype = FAKE_DEV if size else None, valid, size, dtype
    return c


def _ctx(sorted_=0, inplace=0):
    from libgdf_amd._binding import gdf_context
    x = gdf_context()
    x.flag_sorted, x.flag_sort_inplace = sorted_, inplace
    return x


def test_optimal_output_size_is_the_references(gdf):
    assert gdf.gdf_reduce_optimal_output_size() == 128


def test_reduction_argument_errors(gdf):
    i16, i32, f64 = _col(2), _col(3), _col(6)
    assert gdf.gdf_sum_generic(C.byref(i16), FAKE_DEV, 1) == GDF_UNSUPPORTED_DTYPE
    assert gdf.gdf_max_generic(C.byref(_col(7)), FAKE_DEV, 1) == GDF_UNSUPPORTED_DTYPE          # DATE32 through _generic
    assert gdf.gdf_sum_squared_generic(C.byref(i32), FAKE_DEV, 1) == GDF_UNSUPPORTED_DTYPE
    assert gdf.gdf_sum_generic(C.byref(i32), FAKE_DEV, 0) == GDF_INVALID_API_CALL
    assert gdf.gdf_min_i64(C.byref(f64), FAKE_DEV, 0) == GDF_INVALID_API_CALL
    assert gdf.gdf_sum_generic(None, FAKE_DEV, 1) == GDF_INVALID_API_CALL
    assert gdf.gdf_sum_generic(C.byref(i32), None, 1) == GDF_INVALID_API_CALL
    assert gdf.gdf_sum_i32(C.byref(f64), FAKE_DEV, 1) == GDF_DTYPE_MISMATCH
    assert gdf.gdf_product_i64(C.byref(i32), FAKE_DEV, 1) == GDF_DTYPE_MISMATCH
    assert gdf.gdf_sum_squared_f32(C.byref(f64), FAKE_DEV, 1) == GDF_DTYPE_MISMATCH
    assert gdf.gdf_max_i8(C.byref(i16), FAKE_DEV, 1) == GDF_DTYPE_MISMATCH


def test_quantile_argument_errors(gdf):
    res = C.c_double()
    ctx = _ctx()
    f64 = _col(6)
    masked = _col(6, valid=FAKE_DEV)
    assert gdf.gdf_quantile_exact(C.byref(masked), 0, 0.5, C.byref(res), C.byref(ctx)) == GDF_VALIDITY_UNSUPPORTED
    assert gdf.gdf_quantile_aprrox(C.byref(masked), 0.5, C.byref(res), C.byref(ctx)) == GDF_VALIDITY_UNSUPPORTED
    assert gdf.gdf_quantile_exact(C.byref(_col(6, size=0)), 0, 0.5, C.byref(res), C.byref(ctx)) == GDF_DATASET_EMPTY
    assert gdf.gdf_quantile_aprrox(C.byref(_col(3, size=0)), 0.5, C.byref(res), C.byref(ctx)) == GDF_DATASET_EMPTY
    assert gdf.gdf_quantile_exact(C.byref(f64), 7, 0.5, C.byref(res), C.byref(ctx)) == GDF_UNSUPPORTED_METHOD
    assert gdf.gdf_quantile_exact(C.byref(f64), -1, 0.5, C.byref(res), C.byref(ctx)) == GDF_UNSUPPORTED_METHOD
    assert gdf.gdf_quantile_exact(C.byref(f64), 0, -0.1, C.byref(res), C.byref(ctx)) == GDF_INVALID_API_CALL
    assert gdf.gdf_quantile_aprrox(C.byref(f64), math.nan, C.byref(res), C.byref(ctx)) == GDF_INVALID_API_CALL
    assert gdf.gdf_quantile_exact(C.byref(f64), 0, 0.5, None, C.byref(ctx)) == GDF_INVALID_API_CALL
    assert gdf.gdf_quantile_exact(C.byref(f64), 0, 0.5, C.byref(res), None) == GDF_INVALID_API_CALL
    assert gdf.gdf_quantile_exact(None, 0, 0.5, C.byref(res), C.byref(ctx)) == GDF_INVALID_API_CALL
    for bad in (7, 8, 9, 10):                                                   # DATE32, DATE64, TIMESTAMP, CATEGORY
        assert gdf.gdf_quantile_aprrox(C.byref(_col(bad)), 0.5, C.byref(res), C.byref(ctx)) == GDF_UNSUPPORTED_DTYPE


def test_double_argument_is_passed_as_a_double():
    """ctypes converts a Python float to int for an int parameter: q must be declared c_double"""
    from libgdf_amd._binding import _PROTOTYPES
    assert _PROTOTYPES["gdf_quantile_exact"][1][2] is C.c_double
    assert _PROTOTYPES["gdf_quantile_aprrox"][1][1] is C.c_double
    assert _PROTOTYPES["gdf_reduce_optimal_output_size"][0] is C.c_uint


def test_quantile_rule_reproduces_the_reference_known_answers():
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "quantile_known_answers.json")))
    assert tuple(g["methods"]) == QUANTILE_METHODS
    for case in g["cases"]:
        s = np.sort(np.array(case["values"], dtype=case["dtype"]))
        for qi, q in enumerate(g["q"]):
            assert abs(float(quantile_rule(s, q)) - case["approx"][qi]) < g["tolerance"], (case["name"], q)
            for mi, m in enumerate(g["methods"]):
                assert abs(quantile_rule(s, q, m) - case["exact"][qi][mi]) < g["tolerance"], (case["name"], q, m)


def test_quantile_rule_promotion_and_wrap():
    # int8 promotes to int: no wrap; int64 wraps in two's complement; float32 stays float32
    s8 = np.array([-128, 127], dtype=np.int8)
    assert quantile_rule(s8, 0.0, "LINEAR") == -128.0 and quantile_rule(s8, 0.0, "MIDPOINT") == -0.5
    s64 = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max], dtype=np.int64)
    assert quantile_rule(s64, 0.0, "MIDPOINT") == -0.5
    assert quantile_rule(s64, 0.0, "LINEAR") == float(np.iinfo(np.int64).min)   # x = 0: the wrapped difference is multiplied by 0
    assert quantile_rule(s64, 0.75, "LINEAR") == float(np.iinfo(np.int64).min) + 0.5 * -1.0
