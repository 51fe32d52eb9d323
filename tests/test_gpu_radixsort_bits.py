"""-m gpu: begin_bit / end_bit of gdf_radixsort_* and gdf_segmented_radixsort_* (csrc/sort.hip).  Keys whose every bit varies, so
that a pass which looks at a bit outside [begin_bit, end_bit) reorders rows that must keep their input order; the expectation is
radixsort_common.expected (a stable numpy sort on the masked image, pinned by test_radixsort_reference.py).  The LSD passes
work on 8- or 9-bit windows whatever the range: the ranges here end inside a window, at its edge, and past the key's width."""
import numpy as np
import pytest

from radixsort_common import DTYPES, check_sort, full_range_keys, run_sort, width, bits_of

pytestmark = pytest.mark.gpu

SIZES = (1000, 4097)                      # inside one 4096-pair tile of rs_count / rs_scatter, and one pair into the second


def ranges_of(dtype):
    w = width(dtype)
    r = [(0, w), (0, 4), (4, 8), (2, 6), (w - 1, w), (0, 1)]
    if w == 32:
        r += [(0, 20), (3, 17), (8, 24), (12, 32)]
    if w == 64:
        r += [(0, 40), (31, 33), (20, 64), (5, 59), (0, 61)]
    return r


def _cases(dtypes):
    return [pytest.param(dt, b0, b1, id=f"{np.dtype(dt).name}-{b0}_{b1}") for dt in dtypes for b0, b1 in ranges_of(dt)]


def _keys(dtype, n):
    return full_range_keys(np.random.default_rng([width(dtype), int(np.dtype(dtype).kind == "f"), n]), dtype, n)


@pytest.mark.parametrize("descending", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("dtype,begin_bit,end_bit", _cases(DTYPES))
def test_bit_range(gdf, dtype, begin_bit, end_bit, descending):
    for n in SIZES:
        check_sort(_keys(dtype, n), descending, begin_bit, end_bit)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_empty_range_is_identity(gdf, dtype):
    """begin_bit == end_bit, end_bit < begin_bit, and a range that is empty after clamping to the width: both columns unchanged."""
    w = width(dtype)
    key = _keys(dtype, 1000)
    for descending in (False, True):
        for b0, b1 in [(0, 0), (5, 5), (w, w), (6, 2), (w, 0), (w, w + 8), (w + 3, w + 8)]:
            got_k, got_v = run_sort(key, descending, b0, b1)
            np.testing.assert_array_equal(bits_of(got_k), bits_of(key), err_msg=f"[{b0},{b1})")
            np.testing.assert_array_equal(got_v, np.arange(len(key)), err_msg=f"[{b0},{b1})")
            got_k, got_v = run_sort(key, descending, b0, b1, segments=[(0, 400), (400, 1000)])
            np.testing.assert_array_equal(bits_of(got_k), bits_of(key), err_msg=f"segmented [{b0},{b1})")
            np.testing.assert_array_equal(got_v, np.arange(len(key)), err_msg=f"segmented [{b0},{b1})")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_end_bit_is_clamped_to_the_width(gdf, dtype):
    w = width(dtype)
    for n in SIZES:
        key = _keys(dtype, n)
        for descending in (False, True):
            for b0 in (0, 3):
                got_k, got_v = check_sort(key, descending, b0, w + 8)
                ref_k, ref_v = run_sort(key, descending, b0, w)
                np.testing.assert_array_equal(got_v, ref_v)
                np.testing.assert_array_equal(bits_of(got_k), bits_of(ref_k))


@pytest.mark.parametrize("dtype,begin_bit,end_bit", _cases([np.int8, np.float32, np.int64]))
def test_bit_range_segmented(gdf, dtype, begin_bit, end_bit):
    """The same ranges through the segmented entry: three segments with a gap, rows before the first and after the last."""
    for n in SIZES:
        key = _keys(dtype, n)
        segments = [(n // 50, n // 3), (n // 3, n // 2), (n // 2 + 7, n - n // 10)]
        for descending in (False, True):
            check_sort(key, descending, begin_bit, end_bit, segments)
