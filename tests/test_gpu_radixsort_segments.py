"""-m gpu: segment layouts of gdf_segmented_radixsort_* (csrc/sort.hip: radixsort_api turns the segments into regions, sorts every
row by its image -- rows outside all segments with image 0 -- and then, stably, by region number).  The reference's tests only
know adjacent segments that run to the last row; here are gaps, empty segments, untouched tails, segments listed backwards and
enough of them that the second sort takes two passes.  Bit-exact against radixsort_common.expected, which sorts one segment at
a time and leaves every other row in place.  Overlapping segments and offsets beyond n are undefined and not tried."""
import numpy as np
import pytest

from radixsort_common import bits_of, check_sort, full_range_keys, run_sort, width

pytestmark = pytest.mark.gpu

N = 10000


def _random_disjoint(n, count, seed):
    """`count` disjoint segments from 2 * count distinct cut points, shuffled: gaps of random length between them"""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(n + 1, size=2 * count, replace=False))
    segs = [(int(cuts[2 * i]), int(cuts[2 * i + 1])) for i in range(count)]
    return [segs[i] for i in rng.permutation(count)]


# name -> segments for n rows; the four that also make sense for n = 3 are listed in SMALL
LAYOUTS = {
    "gaps": lambda n: [(n // 100, n // 5), (n // 4, n // 2), (n // 2 + 3, n - n // 7)],
    "tail_untouched": lambda n: [(0, n // 4), (n // 4, n - 1 - n // 5)],
    "empty_segments": lambda n: [(0, 0), (0, n - n // 3), (n - n // 3, n - n // 3), (n - n // 3 + n // 50, n - n // 3 + n // 50),
                                 (n - n // 4, n), (n, n)],             # at row 0, at a segment's end, inside a gap, at row n
    "empty_inside_a_segment": lambda n: [(n // 10, n - n // 10), (n // 2, n // 2)],
    "descending_offsets": lambda n: [(n - n // 4, n - 1), (n // 2, n - n // 4), (n // 10, n // 3), (0, n // 10)],
    "no_segments": lambda n: [],
    "one_segment_all_rows": lambda n: [(0, n)],
    "length_one": lambda n: [(i, i + 1) for i in range(0, min(n, 600), 3)] + [(n - 1, n)],
    "straddles_row_4096": lambda n: [(4000, 4200), (4300, 4301)],
    "random_1000": lambda n: _random_disjoint(n, 1000, 7),      # 2000 boundary points: region numbers need 11 bits, two passes
    "adjacent": lambda n: [(0, n // 7), (n // 7, n // 2), (n // 2, n // 2 + 1), (n // 2 + 1, n)],
}
SMALL = ["tail_untouched", "empty_segments", "no_segments", "one_segment_all_rows"]


def _keys(dtype, n):
    return full_range_keys(np.random.default_rng([9, width(dtype), n]), dtype, n)


def _check_layout(dtype, n, layout):
    key = _keys(dtype, n)
    segments = LAYOUTS[layout](n)
    w = width(dtype)
    for descending in (False, True):
        got_k, got_v = check_sort(key, descending, 0, w, segments)
        covered = np.zeros(n, dtype=bool)
        for s, e in segments:
            covered[s:e] = True
        np.testing.assert_array_equal(got_v[~covered], np.arange(n)[~covered])        # said twice: rows outside every segment stay
        if layout == "one_segment_all_rows":
            ref_k, ref_v = run_sort(key, descending, 0, w)
            np.testing.assert_array_equal(got_v, ref_v)
            np.testing.assert_array_equal(bits_of(got_k), bits_of(ref_k))
        if layout == "no_segments":
            np.testing.assert_array_equal(got_v, np.arange(n))
            np.testing.assert_array_equal(bits_of(got_k), bits_of(key))


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("dtype", [np.int32, np.float64], ids=lambda d: np.dtype(d).name)
def test_segment_layout(gdf, dtype, layout):
    _check_layout(dtype, N, layout)


@pytest.mark.parametrize("layout", SMALL)
@pytest.mark.parametrize("dtype", [np.int32, np.float64], ids=lambda d: np.dtype(d).name)
def test_segment_layout_three_rows(gdf, dtype, layout):
    _check_layout(dtype, 3, layout)


def test_layouts_are_disjoint_and_in_bounds():
    """The layouts themselves: overlapping segments or offsets beyond n would make the tests above meaningless."""
    for n, names in ((N, list(LAYOUTS)), (3, SMALL)):
        for name in names:
            covered = np.zeros(n, dtype=np.int32)
            for s, e in LAYOUTS[name](n):
                assert 0 <= s <= e <= n, (name, s, e)
                covered[s:e] += 1
            assert covered.max(initial=0) <= 1, name
    assert len(LAYOUTS["random_1000"](N)) == 1000
