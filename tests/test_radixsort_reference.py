"""Pins tests/radixsort_common.py -- the reference the radix sort GPU tests compare against -- without a GPU: against numpy's own
stable sort where the two must agree, and against answers worked out by hand where the contract goes beyond numpy (bit ranges,
-0.0 / NaN canonicalisation, segments).  A reference that were wrong the way a kernel is wrong would pass nothing here."""
import numpy as np
import pytest

from radixsort_common import (DTYPES, bits_of, expected, float_bit_patterns, float_specials, full_range_ints, image, low_cardinality,
                              special_values, width)

INTS = [np.int8, np.int32, np.int64]
FLOATS = [np.float32, np.float64]
_name = lambda d: np.dtype(d).name          # noqa: E731


def _finite(dtype, n, seed):
    key = float_bit_patterns(np.random.default_rng(seed), dtype, n)
    return np.ascontiguousarray(key[np.isfinite(key)])


@pytest.mark.parametrize("dtype", INTS, ids=_name)
def test_full_range_integers_match_numpy(dtype):
    key = full_range_ints(np.random.default_rng(11), dtype, 3000)
    w = width(dtype)
    assert key.min() < 0 < key.max() and len(np.unique(key >> (w - 2))) == 4          # the top bits do vary
    k, v = expected(key, False, 0, w)
    idx = np.argsort(key, kind="stable")
    np.testing.assert_array_equal(v, idx)
    np.testing.assert_array_equal(k, key[idx])
    k, v = expected(key, True, 0, w)
    idx = np.argsort(~key, kind="stable")
    np.testing.assert_array_equal(v, idx)
    np.testing.assert_array_equal(k, key[idx])


@pytest.mark.parametrize("dtype", FLOATS, ids=_name)
def test_finite_floats_match_numpy(dtype):
    key = _finite(dtype, 3000, 12)
    key[::7] = key[3]                                    # ties, and both zeros
    key[5::50] = 0.0
    key[6::50] = -0.0
    w = width(dtype)
    for descending in (False, True):
        k, v = expected(key, descending, 0, w)
        idx = np.argsort(-key if descending else key, kind="stable")
        np.testing.assert_array_equal(v, idx)
        np.testing.assert_array_equal(bits_of(k), bits_of(key[idx]))


def test_int8_low_nibble_known_answer():
    key = np.array([0x13, -0x7E, 0x21, 0x03, -1, 0x12, 0x7F, 0x40], dtype=np.int8)
    # low nibbles (the sign flip does not reach them):  3, 2, 1, 3, F, 2, F, 0
    k, v = expected(key, False, 0, 4)
    np.testing.assert_array_equal(v, [7, 2, 1, 5, 0, 3, 4, 6])
    np.testing.assert_array_equal(k, np.array([0x40, 0x21, -0x7E, 0x12, 0x13, 0x03, -1, 0x7F], dtype=np.int8))
    # descending sorts on the complement's nibbles:      C, D, E, C, 0, D, 0, F -- ties still in input order
    k, v = expected(key, True, 0, 4)
    np.testing.assert_array_equal(v, [4, 6, 0, 3, 1, 5, 2, 7])
    np.testing.assert_array_equal(k, np.array([-1, 0x7F, 0x13, 0x03, -0x7E, 0x12, 0x21, 0x40], dtype=np.int8))
    # the high nibble of the image (sign flipped): 9, 0, A, 8, 7, 9, F, C
    k, v = expected(key, False, 4, 8)
    np.testing.assert_array_equal(v, [1, 4, 3, 0, 5, 2, 7, 6])


@pytest.mark.parametrize("dtype", FLOATS, ids=_name)
def test_specials_known_answer(dtype):
    key = special_values(dtype)     # 0:+0.0 1:-0.0 2:+inf 3:-inf 4:+NaN 5:-NaN 6:NaN(payload) 7:denormal 8:largest 9:+1 10:-1
    assert len(key) == 11 and np.isnan(key[[4, 5, 6]]).all() and np.signbit(key[[1, 3, 5, 10]]).all() and 0 < key[7] < np.finfo(dtype).tiny
    w = width(dtype)
    k, v = expected(key, False, 0, w)
    np.testing.assert_array_equal(v, [3, 10, 0, 1, 7, 9, 8, 2, 4, 5, 6])      # both zeros tie, the three NaNs tie after +inf
    np.testing.assert_array_equal(bits_of(k), bits_of(key)[v])
    k, v = expected(key, True, 0, w)
    np.testing.assert_array_equal(v, [4, 5, 6, 2, 8, 9, 7, 0, 1, 10, 3])
    np.testing.assert_array_equal(bits_of(k), bits_of(key)[v])
    # the sign bit of the image alone: set for everything that is not negative, -0.0 and -NaN included
    k, v = expected(key, False, w - 1, w)
    np.testing.assert_array_equal(v, [3, 10, 0, 1, 2, 4, 5, 6, 7, 8, 9])


def test_image_known_values():
    np.testing.assert_array_equal(image(np.array([-128, -1, 0, 127], dtype=np.int8), False), [0, 127, 128, 255])
    np.testing.assert_array_equal(image(np.array([-128, -1, 0, 127], dtype=np.int8), True), [255, 128, 127, 0])
    np.testing.assert_array_equal(image(np.array([-2 ** 31, 2 ** 31 - 1], dtype=np.int32), False), [0, 0xffffffff])
    np.testing.assert_array_equal(image(np.array([-2 ** 63, -1, 2 ** 63 - 1], dtype=np.int64), False),
                                  np.array([0, 0x7fffffffffffffff, 0xffffffffffffffff], dtype=np.uint64))
    f = special_values(np.float32)
    np.testing.assert_array_equal(image(f, False), [0x80000000, 0x80000000, 0xff800000, 0x007fffff, 0xffffffff, 0xffffffff, 0xffffffff,
                                                    0x80000001, 0xff7fffff, 0xbf800000, 0x407fffff])
    d = special_values(np.float64)[[1, 3, 5, 10]]
    np.testing.assert_array_equal(image(d, False), np.array([0x8000000000000000, 0x000fffffffffffff, 0xffffffffffffffff,
                                                             0x400fffffffffffff], dtype=np.uint64))
    for dtype in DTYPES:
        assert image(np.zeros(3, dtype=dtype), False).dtype.itemsize == np.dtype(dtype).itemsize


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_image_is_monotonic(dtype):
    """image(a) < image(b) exactly when a < b, for keys that numpy can compare (NaN aside)"""
    rng = np.random.default_rng(13)
    key = full_range_ints(rng, dtype, 2000) if np.dtype(dtype).kind == "i" else _finite(dtype, 2000, 13)
    a, b = key[:-1], key[1:]
    np.testing.assert_array_equal(image(a, False) < image(b, False), a < b)
    np.testing.assert_array_equal(image(a, True) < image(b, True), a > b)


def test_clamping_empty_range_and_segments():
    key = full_range_ints(np.random.default_rng(14), np.int32, 500)
    for a, b in zip(expected(key, False, 3, 40), expected(key, False, 3, 32)):
        np.testing.assert_array_equal(a, b)
    for b0, b1 in [(0, 0), (7, 7), (9, 2), (32, 40), (35, 40)]:
        k, v = expected(key, True, b0, b1)
        np.testing.assert_array_equal(k, key)
        np.testing.assert_array_equal(v, np.arange(500))
    small = np.array([5, 3, 9, 1, 7, 2], dtype=np.int8)
    k, v = expected(small, False, 0, 8, segments=[(4, 6), (2, 2), (1, 4)])
    np.testing.assert_array_equal(k, [5, 1, 3, 9, 2, 7])
    np.testing.assert_array_equal(v, [0, 3, 1, 2, 5, 4])
    k, v = expected(small, False, 0, 8, segments=[])
    np.testing.assert_array_equal(v, np.arange(6))
    k, v = expected(small[:0], False, 0, 8)
    assert len(k) == 0 and len(v) == 0


def test_generators():
    rng = np.random.default_rng(15)
    for dtype in FLOATS:
        s = float_specials(rng, dtype, 11)
        assert sorted(bits_of(s).tolist()) == sorted(bits_of(special_values(dtype)).tolist())          # n = 11: each value once
        assert len(np.unique(bits_of(float_specials(rng, dtype, 1000)))) == 11
    p = float_bit_patterns(rng, np.float32, 4000)
    assert np.isnan(p).any() and (np.isnan(p) & np.signbit(p)).any() and (np.abs(p[np.isfinite(p)]) < np.finfo(np.float32).tiny).any()
    for dtype in DTYPES:
        assert len(np.unique(bits_of(low_cardinality(rng, dtype, 500)))) == 3
