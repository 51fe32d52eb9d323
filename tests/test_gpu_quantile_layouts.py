"""gdf_quantile_* on columns that are slices: the data pointer sits 1 .. 16/itemsize - 1 elements past a 16-byte boundary, so the
radix selection (csrc/quantile.hip qt_pass), the max reduction behind q >= 1 (csrc/reduce.hip column_max_element) and the in-place
sort (csrc/sort.hip sort_column_inplace) all see an unaligned head.  The slice lives inside a larger allocation between guard bytes
(tests/stats_common.py GuardedSlice): mode 2 must sort the slice and nothing else."""
import ctypes as C

import numpy as np
import pytest

import stats_common as sc
from stats_reference import QUANTILE_METHODS, quantile_rule, same

pytestmark = pytest.mark.gpu

METHODS = [None] + list(range(len(QUANTILE_METHODS)))
BACK = 37                             # elements of the allocation behind the slice (in front of it: the offset)


def _offsets(itemsize):
    """every element offset for 8- and 4-byte types; the odd ones and the last for 2- and 1-byte types (as the element-wise tests sample)"""
    v = 16 // itemsize
    if v <= 4:
        return list(range(1, v))
    return sorted(set(range(1, v, 2)) | {v - 1})


CASES = [(d, off) for d in sc.ALL_DTYPES for off in _offsets(np.dtype(d).itemsize)]
IDS = lambda v: np.dtype(v).name if isinstance(v, type) else str(v)          # noqa: E731


def _q_values(n):
    return [0.0, 1.0 / n, 0.25, 0.33, 0.5, 0.999999, 1.0, 1.5]


def _random(dtype, n, rng):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.standard_normal(n) * 1e3).astype(dt)
    if dt == np.int64:
        return rng.integers(-(2**61), 2**61, size=n, dtype=np.int64)
    info = np.iinfo(dt)
    return rng.integers(info.min, int(info.max) + 1, size=n, dtype=np.int64).astype(dt)


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


def _check(gdf, col, s, qs, methods=METHODS, **mode):
    for q in qs:
        for m in methods:
            got, want = _call(gdf, col, q, m, **mode), quantile_rule(s, q, m)
            assert same(got, want), (s.dtype, len(s), q, m, mode, got, want)


def _slice_all_modes(gdf, force_path, dtype, off, n, rng, sort_qs):
    dt = np.dtype(dtype)
    whole = _random(dtype, off + n + BACK, rng)
    a = whole[off: off + n]
    s = np.sort(a)
    qs = _q_values(n)
    # mode 3, both routes: nothing in the allocation changes
    g = sc.GuardedSlice(whole, off, n)
    assert g.col.c.data % 16 == off * dt.itemsize
    sc.clear_notes(gdf)
    _check(gdf, g.col, s, qs)
    if n > 1:
        assert sc.read_notes(gdf)["qt.column_passes"] >= 1
    force_path("GDF_QT_NO_COMPACT")
    _check(gdf, g.col, s, qs)
    force_path("GDF_QT_NO_COMPACT", None)
    assert np.array_equal(sc.bits_of(g.read()), sc.bits_of(whole)), "mode 3 modified the allocation"
    # mode 1 on a sorted slice
    sorted_whole = whole.copy()
    sorted_whole[off: off + n] = s
    g = sc.GuardedSlice(sorted_whole, off, n)
    _check(gdf, g.col, s, qs, flag_sorted=1)
    assert np.array_equal(sc.bits_of(g.read()), sc.bits_of(sorted_whole)), "mode 1 modified the allocation"
    # mode 2: the slice comes back sorted, the guard bytes and the elements in front of and behind the slice are untouched
    for q in sort_qs:
        for m in (None, 0):
            g = sc.GuardedSlice(whole, off, n)
            got = _call(gdf, g.col, q, m, inplace=1)
            assert same(got, quantile_rule(s, q, m)), (dt, n, off, q, m, "inplace", got)
            after = g.read()                                   # (asserts every guard byte)
            assert np.array_equal(sc.bits_of(after), sc.bits_of(sorted_whole)), "mode 2 must sort the slice and only the slice"


@pytest.mark.parametrize("n", [777, 2**16 + 9])
@pytest.mark.parametrize("dtype,off", CASES, ids=IDS)
def test_slices_all_modes(gdf, force_path, dtype, off, n):
    """head, body and tail: n = 777 is one workgroup's worth, 2^16 + 9 several"""
    rng = np.random.default_rng(1000 * off + n % 1000 + np.dtype(dtype).itemsize)
    _slice_all_modes(gdf, force_path, dtype, off, n, rng, sort_qs=[0.33, 1.0])


@pytest.mark.parametrize("dtype", sc.ALL_DTYPES, ids=IDS)
def test_tiny_slices(gdf, force_path, dtype):
    """n in {1, 2, V - 1, V, V + 1} at offset 1 (the head is V - 1 elements: it swallows the column or leaves no full vector, but for n = V + 1 of an 8-byte type) and at
    the largest offset V - 1 (a head of one element)"""
    v = 16 // np.dtype(dtype).itemsize
    for off in sorted({1, v - 1}):
        for n in sorted({1, 2, v - 1, v, v + 1}):
            rng = np.random.default_rng(n + v)
            _slice_all_modes(gdf, force_path, dtype, off, n, rng, sort_qs=[0.5, 1.0])
