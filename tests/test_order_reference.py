"""No-GPU checks of tests/order_reference.py, the numpy restatement of gdf_amd_order_by_ex / gdf_amd_gather that the GPU tests compare
with: cases written out by hand with their expected permutation, the packed-image model (how the kernel computes the order) against
the lexsort statement of the contract, and -- so that the exact GPU comparison means something -- every mutation a wrong
implementation would make changes the permutation of the case designed to catch it."""
import numpy as np
import pytest

import order_reference as orf

I64 = np.iinfo(np.int64)
NAN2 = np.array([0x7FC00001], dtype=np.uint32).view(np.float32)[0]        # a NaN of another payload


def _b(bits):
    return np.array(bits, dtype=bool)


# name -> (columns, descending, nulls_first, expected permutation)
CASES = {
    # DESC with ties: equal rows keep their input order
    "desc_ties": ([(np.array([3, 1, 3, 2, 1], dtype=np.int32), None)], [True], [False], [0, 2, 3, 1, 4]),
    # nulls stand last whatever the direction ...
    "desc_nulls_last": ([(np.array([10, 77, 30, -77, 20], dtype=np.int16), _b([1, 0, 1, 0, 1]))], [True], [False], [2, 4, 0, 1, 3]),
    "asc_nulls_last": ([(np.array([10, 77, 30, -77, 20], dtype=np.int16), _b([1, 0, 1, 0, 1]))], [False], [False], [0, 4, 2, 1, 3]),
    # ... or first
    "desc_nulls_first": ([(np.array([10, 77, 30, -77, 20], dtype=np.int16), _b([1, 0, 1, 0, 1]))], [True], [True], [1, 3, 2, 4, 0]),
    "asc_nulls_first": ([(np.array([10, 77, 30, -77, 20], dtype=np.int16), _b([1, 0, 1, 0, 1]))], [False], [True], [1, 3, 0, 4, 2]),
    # the data under a null bit is not compared: the two nulls keep their input order
    "data_under_nulls": ([(np.array([5, I64.max, -7, I64.min, 0], dtype=np.int64), _b([1, 0, 1, 0, 1]))], [False], [False], [2, 4, 0, 1, 3]),
    # NaN is a value: behind +inf, in front of the nulls; all NaNs are equal
    "nan_and_null": ([(np.array([1.0, np.nan, np.inf, -np.inf, NAN2, 2.5], dtype=np.float32), _b([0, 1, 1, 1, 1, 1]))], [False], [False],
                     [3, 5, 2, 1, 4, 0]),
    "nan_and_null_desc": ([(np.array([1.0, np.nan, np.inf, -np.inf, NAN2, 2.5], dtype=np.float32), _b([0, 1, 1, 1, 1, 1]))], [True], [False],
                          [1, 4, 2, 5, 3, 0]),
    # -0.0 == +0.0
    "zeros": ([(np.array([0.0, -0.0, -1.0, -0.0, 0.0], dtype=np.float64), None)], [False], [False], [2, 0, 1, 3, 4]),
    "zeros_desc": ([(np.array([0.0, -0.0, -1.0, -0.0, 0.0], dtype=np.float64), None)], [True], [False], [0, 1, 3, 4, 2]),
    # the null bit is more significant than the value field (whose content is 0 under a null)
    "null_above_value": ([(np.array([5, 99, -3], dtype=np.int8), _b([1, 0, 1]))], [False], [False], [2, 0, 1]),
    # DESC reverses ITS column only
    "desc_then_asc": ([(np.array([1, 1, 2, 2], dtype=np.int8), None), (np.array([10, 20, 10, 20], dtype=np.int8), None)], [True, False],
                      [False, False], [2, 3, 0, 1]),
    # a NULLS_FIRST ascending column, then a descending float column with nulls last
    "mixed": ([(np.array([1, 1, 9, 2, -9, 2], dtype=np.int32), _b([1, 1, 0, 1, 0, 1])),
               (np.array([0.5, np.nan, 1.0, 7.0, -1.0, 3.0], dtype=np.float32), _b([1, 1, 1, 0, 1, 1]))], [False, True], [True, False],
              [2, 4, 1, 0, 5, 3]),
}

DESIGNED = {"desc_is_reversed_ascending": "desc_ties", "desc_flips_null_placement": "desc_nulls_last",
            "data_under_nulls_compared": "data_under_nulls", "nan_is_null": "nan_and_null", "negative_zero_first": "zeros",
            "null_bit_below_value": "null_above_value", "desc_complements_whole_word": "desc_then_asc"}


@pytest.mark.parametrize("name", list(CASES))
def test_cases_written_by_hand(name):
    cols, desc, first, want = CASES[name]
    assert orf.order_by_ex(cols, desc, first).tolist() == want
    assert orf.model_order(cols, desc, first).tolist() == want
    assert orf.order_by_ex(cols, desc, first).dtype == np.int32


def test_every_mutation_is_listed_with_its_case():
    assert sorted(DESIGNED) == sorted(orf.MUTATIONS)


@pytest.mark.parametrize("mutation", orf.MUTATIONS)
def test_the_designed_case_kills_the_mutation(mutation):
    cols, desc, first, want = CASES[DESIGNED[mutation]]
    assert orf.model_order(cols, desc, first, mutation).tolist() != want, mutation
    differing = [n for n, (c, d, f, w) in CASES.items() if orf.model_order(c, d, f, mutation).tolist() != w]
    assert DESIGNED[mutation] in differing


def test_default_flags_are_ascending_nulls_last():
    cols, _, _, want = CASES["asc_nulls_last"]
    assert orf.order_by_ex(cols).tolist() == want
    assert orf.order_by_ex(cols, False, False).tolist() == want


@pytest.mark.parametrize("seed", range(6))
def test_model_equals_the_lexsort_statement(seed):
    """random small tables, every dtype, many ties, all flag combinations: the packed image gives the lexsort permutation"""
    rng = np.random.default_rng(seed)
    n = 200
    cols, desc, first = [], [], []
    for dt in (np.int8, np.int16, np.int32, np.int64, np.float32, np.float64):
        if np.dtype(dt).kind == "f":
            data = rng.choice(np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan], dtype=dt), size=n)
        else:
            data = rng.integers(-3, 4, size=n).astype(dt)
            data[rng.integers(0, n, size=4)] = np.iinfo(dt).min
            data[rng.integers(0, n, size=4)] = np.iinfo(dt).max
        cols.append((data, rng.random(n) < 0.7 if rng.random() < 0.8 else None))
        desc.append(bool(rng.integers(0, 2)))
        first.append(bool(rng.integers(0, 2)))
    order = rng.permutation(len(cols))[:3]
    pick = lambda xs: [xs[i] for i in order]
    np.testing.assert_array_equal(orf.model_order(pick(cols), pick(desc), pick(first)), orf.order_by_ex(pick(cols), pick(desc), pick(first)))


def test_plain_ascending_is_a_stable_lexsort():
    rng = np.random.default_rng(9)
    a, b = rng.integers(-5, 5, size=500).astype(np.int32), rng.integers(0, 3, size=500).astype(np.int8)
    np.testing.assert_array_equal(orf.order_by_ex([(a, None), (b, None)]), np.lexsort((b, a)))


def test_gather_written_by_hand():
    data = np.array([1.5, -0.0, np.nan, 4.0], dtype=np.float64)
    valid = _b([1, 1, 0, 1])
    ints = np.array([7, 8, 9, 10], dtype=np.int16)
    idx = np.array([3, -1, 2, 0, 0, 1], dtype=np.int32)
    (d0, ok0, m0, n0), (d1, ok1, m1, n1) = orf.gather(idx, [(data, valid), (ints, None)])
    assert ok0.tolist() == [True, False, False, True, True, True] and n0 == 2
    assert np.array_equal(orf.bits_of(d0), orf.bits_of(np.array([4.0, 0.0, 0.0, 1.5, 1.5, -0.0])))
    assert m0.tolist() == [0b111001, 0, 0, 0, 0, 0, 0, 0]
    assert d1.tolist() == [10, 0, 9, 7, 7, 8] and ok1.tolist() == [True, False, True, True, True, True] and n1 == 1
    assert m1.tolist() == [0b111101, 0, 0, 0, 0, 0, 0, 0]
    (d, ok, m, nn), = orf.gather(np.zeros(0, dtype=np.int64), [(ints, None)])
    assert len(d) == 0 and len(m) == 0 and nn == 0
    assert len(orf.mask_words(np.ones(65, dtype=bool))) == 16 and orf.mask_words(np.ones(65, dtype=bool))[8:].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
