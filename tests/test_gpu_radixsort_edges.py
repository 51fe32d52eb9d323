"""-m gpu: gdf_radixsort_* (csrc/sort.hip) where tests/util.gen_rand never goes: sizes on and around the tile edges of rs_count /
rs_scatter, float specials (NaNs with payloads, infinities, both zeros, denormals), keys where only stability decides the
answer, and the ten typed entry points.  Bit-exact against radixsort_common.expected."""
import numpy as np
import pytest

from radixsort_common import DTYPES, SUFFIX, check_sort, float_bit_patterns, float_specials, full_range_keys, low_cardinality, width

pytestmark = pytest.mark.gpu

_name = lambda d: np.dtype(d).name          # noqa: E731


def _rng(*seed):
    return np.random.default_rng(list(seed))


# rs_count / rs_scatter work on tiles of 4096 (key, row) pairs and the grid is rounded up to 8 tiles (32768 pairs)
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 32767, 32768, 32769])
@pytest.mark.parametrize("dtype", [np.int64, np.float32], ids=_name)
def test_sizes(gdf, dtype, n):
    key = full_range_keys(_rng(1, width(dtype), n), dtype, n)
    for descending in (False, True):
        check_sort(key, descending, 0, width(dtype))


@pytest.mark.parametrize("n", [11, 1000])
@pytest.mark.parametrize("make", [float_specials, float_bit_patterns], ids=["specials", "bit_patterns"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=_name)
def test_float_specials(gdf, dtype, make, n):
    """-0.0 and +0.0 tie, every NaN ties with every other NaN after +inf: ties keep the input order and every element comes back with
    the bits it went in with.  The partial range cuts through the exponent, where the canonical NaN image is all ones."""
    w = width(dtype)
    key = make(_rng(2, w, n), dtype, n)
    for descending in (False, True):
        check_sort(key, descending, 0, w)
        check_sort(key, descending, w - 12, w - 2)


def _stability_keys(kind, dtype, n):
    rng = _rng(3, width(dtype), int(np.dtype(dtype).kind == "f"))
    if kind == "three_values":
        return low_cardinality(rng, dtype, n)
    if kind == "all_equal":                                   # no bit varies: the sort returns before its first pass
        return low_cardinality(rng, dtype, 1)[[0] * n]
    key = full_range_keys(rng, dtype, n)
    if np.dtype(dtype).kind == "f":
        key = key[~np.isnan(key)]
    key = np.sort(key, kind="stable")                         # duplicates (int8 has only 256 values) stay: ties in sorted input
    return np.ascontiguousarray(key if kind == "sorted" else key[::-1])


@pytest.mark.parametrize("kind", ["three_values", "all_equal", "sorted", "reversed"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_stability(gdf, dtype, kind):
    key = _stability_keys(kind, dtype, 5000)
    w = width(dtype)
    for descending in (False, True):
        _, got_v = check_sort(key, descending, 0, w)
        if kind == "all_equal":
            np.testing.assert_array_equal(got_v, np.arange(len(key)))
        if kind == "three_values":
            check_sort(key, descending, 1, w - 1)


@pytest.mark.parametrize("segmented", [False, True], ids=["whole", "segmented"])
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_typed_entry_points(gdf, dtype, segmented):
    n, w = 1000, width(dtype)
    key = full_range_keys(_rng(4, w, int(segmented)), dtype, n)
    segments = [(10, 300), (300, 301), (450, 990)] if segmented else None
    check_sort(key, False, 0, w, segments, entry=SUFFIX[np.dtype(dtype)])
    check_sort(key, True, 2, w - 1, segments, entry=SUFFIX[np.dtype(dtype)])


def test_typed_entry_point_checks_the_key_width(gdf):
    """gdf_radixsort_i32 on a plan set up for 8-byte keys: GDF_COLUMN_SIZE_MISMATCH, nothing sorted."""
    import ctypes as C
    from libgdf_amd.columns import column_from_numpy
    from radixsort_common import api
    lib = api()
    key = full_range_keys(_rng(5), np.int32, 100)
    ck, cv = column_from_numpy(key), column_from_numpy(np.arange(100, dtype=np.int64))
    plan = lib.gdf_radixsort_plan(100, 0, 0, 32)
    assert lib.gdf_radixsort_plan_setup(plan, 8, 8) == 0
    assert lib.gdf_radixsort_i32(plan, C.addressof(ck.c), C.addressof(cv.c)) == 3
    assert lib.gdf_radixsort_plan_free(plan) == 0
    np.testing.assert_array_equal(ck.to_numpy(), key)
    np.testing.assert_array_equal(cv.to_numpy(), np.arange(100))
