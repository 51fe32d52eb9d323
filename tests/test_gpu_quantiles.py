"""gdf_quantile_exact / gdf_quantile_aprrox on the GPU (csrc/quantile.hip) through all three modes -- flag_sorted, flag_sort_inplace and
the radix selection (with and without its candidate buffer) -- against the numpy restatement of the rule in stats_reference.py."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from stats_reference import QUANTILE_METHODS, quantile_rule, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
METHODS = [None] + list(range(len(QUANTILE_METHODS)))


def _q_values(n):
    return [0.0, 1.0 / n, 0.25, 0.33, 0.5, 0.999999, 1.0, 1.5]


def _call(gdf, col, q, method, flag_sorted=0, inplace=0):
    from libgdf_amd.columns import GDF_TO_NP, new_context
    ctx = new_context(flag_sorted=flag_sorted, method=0, flag_sort_inplace=inplace)
    if method is None:
        res = np.zeros(1, dtype=GDF_TO_NP[int(col.c.dtype)])
        gdf.libgdf.gdf_quantile_aprrox(col.ptr, q, res.ctypes.data, C.byref(ctx))
        return res[0]
    res = C.c_double(0.0)
    gdf.libgdf.gdf_quantile_exact(col.ptr, method, q, C.addressof(res), C.byref(ctx))
    return res.value


def _check_all(gdf, col, s, qs, methods=METHODS, **mode):
    for q in qs:
        for m in methods:
            got, want = _call(gdf, col, q, m, **mode), quantile_rule(s, q, m)
            if m is None:
                assert np.asarray(got).dtype == s.dtype
            assert same(got, want), (s.dtype, len(s), q, m, mode, got, want)


def _random(dtype, n, rng):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.standard_normal(n) * 1e3).astype(dt)
    if dt == np.int64:
        return rng.integers(-(2**61), 2**61, size=n, dtype=np.int64)
    info = np.iinfo(dt)
    return rng.integers(info.min, int(info.max) + 1, size=n, dtype=np.int64).astype(dt)


def _all_modes(gdf, force_path, a, qs, methods=METHODS, sort_qs=None):
    """mode 3 (both routes; the column must come back byte-identical), mode 1 on np.sort(a), mode 2 on fresh copies"""
    import torch
    from libgdf_amd.columns import Column
    s = np.sort(a)
    t = torch.from_numpy(a).cuda()
    col = Column(t)
    _check_all(gdf, col, s, qs, methods)
    force_path("GDF_QT_NO_COMPACT")
    _check_all(gdf, col, s, qs, methods)
    force_path("GDF_QT_NO_COMPACT", None)
    assert torch.equal(t.view(torch.uint8), torch.from_numpy(a).cuda().view(torch.uint8)), "mode 3 modified the column"
    ts = torch.from_numpy(s).cuda()
    _check_all(gdf, Column(ts), s, qs, methods, flag_sorted=1)
    assert torch.equal(ts.view(torch.uint8), torch.from_numpy(s).cuda().view(torch.uint8)), "mode 1 modified the column"
    for q in (qs if sort_qs is None else sort_qs):
        for m in methods:
            tc = t.clone()
            got = _call(gdf, Column(tc), q, m, inplace=1)
            assert same(got, quantile_rule(s, q, m)), (a.dtype, len(a), q, m, "inplace", got)
            assert np.array_equal(tc.cpu().numpy(), s, equal_nan=a.dtype.kind == "f"), "mode 2 must leave the column sorted"


def test_known_answers_all_modes(gdf, force_path):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "quantile_known_answers.json")))
    import torch
    from libgdf_amd.columns import Column
    for case in g["cases"]:
        a = np.array(case["values"], dtype=case["dtype"])
        for mode in ({}, {"flag_sorted": 1}, {"inplace": 1}, {"compact": False}):
            for qi, q in enumerate(g["q"]):
                for mi in [None] + list(range(5)):
                    src = np.sort(a) if mode.get("flag_sorted") else a
                    col = Column(torch.from_numpy(src.copy()).cuda())
                    if mode.get("compact") is False:
                        force_path("GDF_QT_NO_COMPACT")
                    kw = {k: v for k, v in mode.items() if k != "compact"}
                    got = _call(gdf, col, q, mi, **kw)
                    force_path("GDF_QT_NO_COMPACT", None)
                    want = case["approx"][qi] if mi is None else case["exact"][qi][mi]
                    assert abs(float(got) - want) < g["tolerance"], (case["name"], mode, q, mi, got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n", [1, 2, 3, 9, 127, 10_000, 1_000_000])
def test_random_columns(gdf, force_path, dtype, n):
    rng = np.random.default_rng(n * 7 + np.dtype(dtype).itemsize)
    _all_modes(gdf, force_path, _random(dtype, n, rng), _q_values(n))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_random_columns_1e8(gdf, force_path, dtype):
    import torch
    n = 100_000_000
    rng = np.random.default_rng(11 + np.dtype(dtype).itemsize)
    _all_modes(gdf, force_path, _random(dtype, n, rng), _q_values(n), sort_qs=[0.5])
    torch.cuda.empty_cache()


def test_int64_extremes_pin_the_wrap_rule(gdf, force_path):
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    a = np.array([hi, lo, hi, lo, 0, hi - 1, lo + 1], dtype=np.int64)
    _all_modes(gdf, force_path, a, [0.0, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0])
    b = np.array([lo, hi], dtype=np.int64)
    _all_modes(gdf, force_path, b, [0.0, 0.5, 0.75])
    c = np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max] * 3, dtype=np.int32)
    _all_modes(gdf, force_path, c, [0.0, 0.25, 0.5, 0.6])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_floats_with_nan_inf_and_signed_zero(gdf, force_path, dtype):
    rng = np.random.default_rng(5)
    a = (rng.standard_normal(100_000) * 10).astype(dtype)
    a[rng.integers(0, len(a), 500)] = np.nan
    a[rng.integers(0, len(a), 300)] = np.inf
    a[rng.integers(0, len(a), 300)] = -np.inf
    a[rng.integers(0, len(a), 2000)] = 0.0
    a[rng.integers(0, len(a), 2000)] = -0.0
    _all_modes(gdf, force_path, a, [0.0, 0.001, 0.003, 0.25, 0.5, 0.996, 0.9999, 1.0])
    small = np.array([np.nan, 1.0, -np.inf, np.inf, -0.0, 0.0, np.nan], dtype=dtype)
    _all_modes(gdf, force_path, small, [0.0, 0.2, 0.4, 0.5, 0.7, 0.8, 0.9, 1.0])


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.float64], ids=lambda d: np.dtype(d).name)
def test_heavy_duplicates(gdf, force_path, dtype):
    rng = np.random.default_rng(3)
    n = 1_000_000
    qs = [0.0, 0.1, 0.5, 0.9, 0.95, 0.999999, 1.0]
    _all_modes(gdf, force_path, np.full(n, 42, dtype=dtype), qs)
    _all_modes(gdf, force_path, np.where(rng.random(n) < 0.5, -7, 9).astype(dtype), qs + [0.4999995, 0.5000005])
    a = np.where(rng.random(n) < 0.9, 5, rng.integers(-1000, 1000, n)).astype(dtype)
    _all_modes(gdf, force_path, a, qs)
    ten = rng.integers(-(2**62), 2**62, size=10, dtype=np.int64)
    _all_modes(gdf, force_path, ten[rng.integers(0, 10, n)].astype(dtype), qs)


def test_python_api(gdf):
    from libgdf_amd.columns import column_from_numpy
    a = np.array([7, 0, 3, 4, 2, 1, -1, 1, 6], dtype=np.int32)
    assert gdf.api.quantile(column_from_numpy(a), 0.5) == 1
    assert gdf.api.quantile(column_from_numpy(a), 0.5, method="linear") == 1.5
    col = column_from_numpy(a)
    assert gdf.api.quantile(col, 0.25, method="higher", sort_inplace=True) == 1.0
    assert np.array_equal(col.to_numpy(), np.sort(a))
    assert gdf.api.quantile(col, 0.5, method="midpoint", sorted=True) == 1.5
