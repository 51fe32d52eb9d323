"""No-GPU checks of tests/groupby_agg_reference.py, the model of gdf_amd_group_by_agg's contract that the GPU tests compare with: every
case below is small enough that the expected groups and aggregates are written out by hand."""
import numpy as np

import groupby_agg_reference as gar
import order_reference as orf

NAN = float("nan")


def i32(*v):
    return np.array(v, dtype=np.int32)


def run(keys, values, aggs, **kw):
    return gar.group_by_agg(keys, values, aggs, **kw)


def expect(out, data, ok=None, dtype=None):
    ok = [True] * len(data) if ok is None else ok
    assert list(out.ok) == ok
    assert out.null_count == ok.count(False)
    assert [x for x, o in zip(out.data.tolist(), ok) if o] == [x for x, o in zip(data, ok) if o]
    assert all(x == 0 for x, o in zip(out.data.tolist(), ok) if not o)              # a null element has data 0
    np.testing.assert_array_equal(out.mask, orf.mask_words(ok))
    if dtype is not None:
        assert out.dtype == dtype


def test_plain_groups_come_out_ascending_with_sum_and_counts():
    keys = [(i32(3, 1, 3, 2, 1, 3), None)]
    vals = [(np.array([10, 20, 30, 40, 50, 60], dtype=np.int64), np.array([1, 1, 0, 1, 1, 1], dtype=bool))]
    (k,), (s, c, star) = run(keys, vals, [(0, "sum"), (0, "count"), (None, "count")])
    expect(k, [1, 2, 3], dtype=gar.INT32)
    expect(s, [70, 40, 70], dtype=gar.INT64)
    expect(c, [2, 1, 2], dtype=gar.INT64)                                            # COUNT(col): the valid values
    expect(star, [2, 1, 3], dtype=gar.INT64)                                         # COUNT(*): the rows


def test_null_keys_form_one_group_behind_the_values():
    keys = [(i32(5, 99, 4, 77, 5), np.array([1, 0, 1, 0, 1], dtype=bool))]           # the data under the null bits differs: not compared
    vals = [(np.array([1, 2, 4, 8, 16], dtype=np.int16), None)]
    (k,), (s,) = run(keys, vals, [(0, "sum")])
    expect(k, [4, 5, 0], ok=[True, True, False])
    expect(s, [4, 17, 10])


def test_three_way_null_split_over_two_columns():
    a = (i32(0, 0, 1, 0, 1), np.array([0, 0, 1, 0, 1], dtype=bool))                  # null, null, 1, null, 1
    b = (i32(1, 2, 0, 1, 0), np.array([1, 1, 0, 1, 0], dtype=bool))                  # 1,    2,    null, 1,  null
    (ka, kb), (star,) = run([a, b], [], [(None, "count")])
    # ascending, nulls last per column: (1, null) | (null, 1) | (null, 2)
    expect(ka, [1, 0, 0], ok=[True, False, False])
    expect(kb, [0, 1, 2], ok=[False, True, True])
    expect(star, [2, 2, 1])


def test_nan_keys_are_one_group_and_zeros_are_one_group():
    payload = np.array([0x7FF8000000000001], dtype=np.uint64).view(np.float64)[0]
    data = np.array([0.0, NAN, -0.0, payload, 1.5, -0.0], dtype=np.float64)
    (k,), (star,) = run([(data, None)], [], [(None, "count")])
    expect(star, [3, 1, 2])                                                          # {0.0, -0.0, -0.0}, {1.5}, {NaN, NaN'}
    # the key output is the bits of the group's FIRST input row: +0.0 (row 0) and the NaN of row 1, not its sibling's payload
    np.testing.assert_array_equal(orf.bits_of(k.data), orf.bits_of(np.array([0.0, 1.5, NAN], dtype=np.float64)))
    data2 = data[::-1].copy()                                                        # now -0.0 and the payload NaN come first
    (k2,), _ = run([(data2, None)], [], [(None, "count")])
    np.testing.assert_array_equal(orf.bits_of(k2.data), orf.bits_of(np.array([-0.0, 1.5, payload], dtype=np.float64)))


def test_min_and_max_with_nan():
    keys = [(i32(1, 1, 1, 2, 2, 3), None)]
    vals = [(np.array([2.0, NAN, -1.0, NAN, NAN, np.inf], dtype=np.float32), None)]
    _, (mn, mx) = run(keys, vals, [(0, "min"), (0, "max")])
    assert mn.dtype == mx.dtype == gar.FLOAT32 and mn.data.dtype == np.float32
    assert mn.data[0] == -1.0 and np.isnan(mx.data[0])                               # MAX is NaN if any valid value is
    assert np.isnan(mn.data[1]) and np.isnan(mx.data[1])                             # MIN only if all are
    assert mn.data[2] == np.inf and mx.data[2] == np.inf
    assert mn.null_count == mx.null_count == 0


def test_a_null_value_is_skipped_also_when_it_hides_a_nan():
    keys = [(i32(1, 1), None)]
    vals = [(np.array([NAN, 3.0]), np.array([0, 1], dtype=bool))]
    _, (mn, mx, s, a, c) = run(keys, vals, [(0, "min"), (0, "max"), (0, "sum"), (0, "avg"), (0, "count")])
    assert (mn.data[0], mx.data[0], s.data[0], a.data[0], c.data[0]) == (3.0, 3.0, 3.0, 3.0, 1)


def test_a_group_without_a_valid_value_is_null_except_its_counts():
    keys = [(i32(7, 8, 7), None)]
    vals = [(np.array([5, 6, 9], dtype=np.int8), np.array([0, 1, 0], dtype=bool))]
    _, (s, a, mn, mx, c, star) = run(keys, vals, [(0, "sum"), (0, "avg"), (0, "min"), (0, "max"), (0, "count"), (None, "count")])
    expect(s, [0, 6], ok=[False, True], dtype=gar.INT64)
    expect(a, [0.0, 6.0], ok=[False, True], dtype=gar.FLOAT64)
    expect(mn, [0, 6], ok=[False, True], dtype=gar.INT8)
    expect(mx, [0, 6], ok=[False, True], dtype=gar.INT8)
    expect(c, [0, 1])                                                                # never null
    expect(star, [2, 1])


def test_int64_sums_wrap_and_avg_divides_the_wrapped_sum():
    big = (1 << 62) + 5
    keys = [(i32(1, 1, 1, 2), None)]
    vals = [(np.array([big, big, big, -4], dtype=np.int64), None)]
    _, (s, a) = run(keys, vals, [(0, "sum"), (0, "avg")])
    wrapped = 3 * big - (1 << 64)
    expect(s, [wrapped, -4])
    assert a.data[0] == float(wrapped) / 3 and a.data[1] == -4.0


def test_int8_sums_widen():
    keys = [(i32(1, 1, 1), None)]
    vals = [(np.array([100, 100, 100], dtype=np.int8), None)]
    _, (s, a) = run(keys, vals, [(0, "sum"), (0, "avg")])
    expect(s, [300], dtype=gar.INT64)
    expect(a, [100.0], dtype=gar.FLOAT64)


def test_float32_sums_widen_before_the_first_add():
    keys = [(i32(1, 1, 1), None)]
    vals = [(np.array([16777216.0, 1.0, 1.0], dtype=np.float32), None)]              # 2^24 + 1 is no float32
    _, (s,) = run(keys, vals, [(0, "sum")])
    expect(s, [16777218.0], dtype=gar.FLOAT64)
    assert s.sum_abs[0] == 16777218.0 and s.count[0] == 3


def test_float_sums_are_exact():
    keys = [(i32(1, 1, 1), None)]
    vals = [(np.array([1e100, 1.0, -1e100]), None)]
    _, (s,) = run(keys, vals, [(0, "sum")])
    assert s.data[0] == 1.0


def test_min_max_keep_the_dtype_tag_and_signed_order():
    keys = [(i32(1, 1, 2), None)]
    vals = [(np.array([-5, 3, 9], dtype=np.int64), None)]
    (k,), (mn, mx) = run(keys, vals, [(0, "min"), (0, "max")], key_dtypes=[gar.DATE32], value_dtypes=[gar.TIMESTAMP])
    assert k.dtype == gar.DATE32
    expect(mn, [-5, 9], dtype=gar.TIMESTAMP)
    expect(mx, [3, 9], dtype=gar.TIMESTAMP)


def test_first_row_of_a_group_is_first_in_input_order():
    """the stable sort keeps a group's rows in input order, so the key bits are row 0's even when row 3 holds the other zero"""
    data = np.array([-0.0, 5.0, 0.0, 0.0], dtype=np.float32)
    (k,), _ = run([(data, None)], [], [(None, "count")])
    assert np.signbit(k.data[0]) and k.data[1] == 5.0


def test_no_rows():
    (k,), (s, c) = run([(np.zeros(0, dtype=np.int64), None)], [(np.zeros(0, dtype=np.float32), None)], [(0, "sum"), (None, "count")])
    assert len(k.data) == len(s.data) == len(c.data) == 0 and len(k.mask) == 0
    assert (k.dtype, s.dtype, c.dtype) == (gar.INT64, gar.FLOAT64, gar.INT64)


def test_mask_words_cover_whole_64_bit_words():
    n = 130
    keys = [(np.arange(n, dtype=np.int32), None)]
    vals = [(np.ones(n, dtype=np.int32), np.arange(n) % 2 == 0)]
    _, (s,) = run(keys, vals, [(0, "sum")])
    assert len(s.mask) == 24 and s.null_count == 65
    assert s.mask[16] == 0b01 and not s.mask[17:].any()                             # groups 128, 129; the bits beyond G are zero
