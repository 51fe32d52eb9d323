"""No-GPU checks of tests/semi_join_reference.py, the model tests/test_gpu_semi_join.py compares gdf_amd_semi_join against: tiny tables
whose expected row numbers are written out by hand, and for every mutation of the model a table on which it changes the answer."""
import numpy as np
import pytest

import semi_join_reference as sjr

NAN_A = np.array([0x7FF8000000000000], dtype=np.uint64).view(np.float64)[0]
NAN_B = np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]


def i32(*v):
    return np.array(v, dtype=np.int32)


def f64(*v):
    return np.array(v, dtype=np.float64)


def mask(*v):
    return np.array(v, dtype=bool)


def rows(*v):
    return np.array(v, dtype=np.int32)


def check(got, want):
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, want)


def test_one_integer_column():
    left = [(i32(5, 7, 5, 9, -1, 7), None)]
    right = [(i32(7, 7, 7, -1, 100), None)]
    check(sjr.semi_join(left, right), rows(1, 4, 5))
    check(sjr.semi_join(left, right, anti=True), rows(0, 2, 3))
    check(sjr.semi_join(left, right, nulls_equal=True), rows(1, 4, 5))
    check(sjr.semi_join(left, right, anti=True, nulls_equal=True), rows(0, 2, 3))


def test_two_columns_agree_in_every_column():
    left = [(i32(1, 1, 2, 2), None), (f64(0.5, 1.5, 0.5, 1.5), None)]
    right = [(i32(2, 1), None), (f64(0.5, 1.5), None)]
    check(sjr.semi_join(left, right), rows(1, 2))
    check(sjr.semi_join(left, right, anti=True), rows(0, 3))


def test_nulls_under_all_four_flag_combinations():
    #            row:  0     1      2     3      4
    left = [(i32(1, 1, 2, 2, 3), mask(1, 0, 1, 0, 1)), (i32(10, 10, 20, 20, 30), mask(1, 1, 0, 0, 1))]
    # right rows: (1, 10)  (null, 10)  (2, null)  (3, 31)
    right = [(i32(1, 9, 2, 3), mask(1, 0, 1, 1)), (i32(10, 10, 9, 31), mask(1, 1, 0, 1))]
    check(sjr.semi_join(left, right), rows(0))
    check(sjr.semi_join(left, right, anti=True), rows(1, 2, 3, 4))                  # NOT EXISTS keeps the rows with a null key
    check(sjr.semi_join(left, right, nulls_equal=True), rows(0, 1, 2))              # (null, null) has no partner on the right
    check(sjr.semi_join(left, right, anti=True, nulls_equal=True), rows(3, 4))


def test_floats_zeros_nans_and_infinities():
    left = [(f64(0.0, -0.0, NAN_A, NAN_B, np.inf, -np.inf, 1.0), None)]
    right = [(f64(-0.0, NAN_A, NAN_B, -np.inf), None)]
    for nulls_equal in (False, True):
        check(sjr.semi_join(left, right, nulls_equal=nulls_equal), rows(0, 1, 5))
        check(sjr.semi_join(left, right, anti=True, nulls_equal=nulls_equal), rows(2, 3, 4, 6))


def test_empty_sides():
    some = [(i32(4, 5), None)]
    none = [(i32(), None)]
    check(sjr.semi_join(some, none), rows())
    check(sjr.semi_join(some, none, anti=True), rows(0, 1))
    check(sjr.semi_join(none, some), rows())
    check(sjr.semi_join(none, some, anti=True), rows())
    check(sjr.semi_join(none, none, anti=True, nulls_equal=True), rows())


def test_data_under_a_null_is_not_compared():
    left = [(i32(7, 7), mask(1, 0))]
    right = [(i32(7, 8), mask(0, 1))]                                               # the right side's 7 is under a null
    check(sjr.semi_join(left, right), rows())
    check(sjr.semi_join(left, right, nulls_equal=True), rows(1))


# ---- every mutation changes some answer ---------------------------------------------------------------------------------------------------
def _mutation_cases():
    null_l = [(i32(1, 2), mask(1, 0))]
    null_r = [(i32(3, 4), mask(0, 1))]
    yield "null_matches_null_without_flag", null_l, null_r, dict(), rows(), rows(1)
    # with the flag a null must not meet the value the null's field holds in the image (0)
    yield "null_matches_value_with_flag", [(i32(0, 5), mask(1, 1))], [(i32(9, 5), mask(0, 1))], dict(nulls_equal=True), rows(1), rows(0, 1)
    yield "null_matches_value_with_flag", [(i32(9, 5), mask(0, 1))], [(i32(0, 6), mask(1, 1))], dict(nulls_equal=True), rows(), rows(0)
    yield "nan_matches_nan", [(f64(NAN_A, 1.0), None)], [(f64(NAN_A, NAN_B), None)], dict(), rows(), rows(0)
    yield "nan_matches_nan", [(f64(NAN_A, 1.0), None)], [(f64(NAN_A, NAN_B), None)], dict(anti=True), rows(0, 1), rows(1)
    yield "negative_zero_distinct", [(f64(-0.0, 0.0), None)], [(f64(0.0), None)], dict(), rows(0, 1), rows(1)
    yield "data_under_null_compared", [(i32(7, 8), mask(1, 1))], [(i32(7, 8), mask(0, 1))], dict(), rows(1), rows(0, 1)
    yield "data_under_null_compared", [(i32(7, 8), mask(0, 1))], [(i32(6, 1), mask(0, 1))], dict(nulls_equal=True), rows(0), rows()
    yield "anti_drops_null_rows", null_l, [(i32(1), None)], dict(anti=True), rows(1), rows()
    yield "result_not_ascending", [(i32(1, 2, 1), None)], [(i32(1), None)], dict(), rows(0, 2), rows(2, 0)
    yield "duplicates_emitted_per_partner", [(i32(1, 2), None)], [(i32(2, 2, 2), None)], dict(), rows(1), rows(1, 1, 1)
    ones = [(np.array([-1, 0], dtype=np.int64), None)]
    yield "reserved_image_lost", ones, ones, dict(), rows(0, 1), rows(1)
    yield "reserved_image_lost", ones, ones, dict(anti=True), rows(), rows(0)
    eight = [(np.array([-1, -1, 0], dtype=np.int8), None) for _ in range(8)]
    yield "reserved_image_lost", eight, eight, dict(), rows(0, 1, 2), rows(2)
    # sixteen left keys against one right key with a 1-bit tag: some left key shares the tag without being the key
    wide_l = [(np.arange(16, dtype=np.int64), None), (np.arange(16, dtype=np.int64), None)]
    wide_r = [(np.array([3], dtype=np.int64), None), (np.array([3], dtype=np.int64), None)]
    yield "tag_hit_taken_as_match", wide_l, wide_r, dict(tag_bits=1), rows(3), None


@pytest.mark.parametrize("case", list(_mutation_cases()), ids=lambda c: c[0])
def test_every_mutation_changes_an_answer(case):
    mutation, left, right, kw, want, mutated = case
    check(sjr.semi_join(left, right, **kw), want)
    got = sjr.semi_join(left, right, mutation=mutation, **kw)
    if mutated is None:                                                             # (which rows share the tag is the hash's business)
        assert len(got) > len(want) and set(want) <= set(got)
    else:
        np.testing.assert_array_equal(got, mutated)
    assert not np.array_equal(got, want)


def test_every_mutation_has_a_case():
    assert {c[0] for c in _mutation_cases()} == set(sjr.MUTATIONS)


def test_the_reserved_image_needs_exactly_64_bits_of_minus_one():
    assert sjr.image_is_reserved([np.int64], (-1,), False)
    assert sjr.image_is_reserved([np.int8] * 8, (-1,) * 8, False)
    assert not sjr.image_is_reserved([np.int32], (-1,), False)
    assert not sjr.image_is_reserved([np.int64], (-1,), True)
    assert not sjr.image_is_reserved([np.int32, np.int32], (-1, 0), False)
    assert not sjr.image_is_reserved([np.float64], (-1.0,), False)
