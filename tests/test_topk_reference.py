"""No-GPU checks of tests/topk_reference.py, the Python-integer model of gdf_amd_top_k's selection route: cases written out by hand
with the rows they owe, the model against the oracle slice order_reference.order_by_ex(...)[offset:offset + k], and -- so that the
exact GPU comparison means something -- every mutation a wrong kernel would make changes the result of the case designed for it."""
import numpy as np
import pytest

import order_reference as orf
import topk_reference as tkr

I64 = np.iinfo(np.int64)


def _b(bits):
    return np.array(bits, dtype=bool)


# name -> (columns, descending, nulls_first, k, offset, the rows owed)
CASES = {
    # +0.0 and -0.0 tie: the LOWER ROW makes the cut, not the smaller bit pattern
    "zeros_tie_at_the_cut": ([(np.array([-0.0, 0.0, 5.0], dtype=np.float64), None)], None, None, 1, 0, [0]),
    # three equal rows, two wanted: in row order
    "ties_in_row_order": ([(np.array([1, 1, 1, 5], dtype=np.int8), None)], None, None, 2, 0, [0, 1]),
    # a masked int64 is 65 bits: 3 and 2 share their 64-bit image, the dropped bit decides
    "dropped_bit_decides": ([(np.array([3, 2, 9], dtype=np.int64), _b([1, 1, 1]))], None, None, 1, 0, [1]),
    # ... and the straddling field gives its HIGH bits: -1 (0x7FF...F) before 0 (0x800...0)
    "straddle_keeps_high_bits": ([(np.array([0, -1], dtype=np.int64), _b([1, 1]))], None, None, 1, 0, [1]),
    # DESC complements its own eight bits only: the first column still decides
    "desc_second_column": ([(np.array([2, 1], dtype=np.int8), None), (np.array([5, 5], dtype=np.int8), None)], [False, True], None, 1, 0, [1]),
    # the null bit stands above the value field
    "null_above_value": ([(np.array([5, 99, -3], dtype=np.int8), _b([1, 0, 1]))], None, None, 1, 0, [2]),
    # the data under the null bits (INT64_MAX before INT64_MIN in row order) is not compared: the nulls keep their row order
    "data_under_nulls": ([(np.array([5, I64.max, -7, I64.min, 0], dtype=np.int64), _b([1, 0, 1, 0, 1]))], None, None, 4, 3, [1, 3]),
    # the OFFSET is taken from the K = offset + k smallest rows
    "offset_page": ([(np.array([4, 3, 2, 1, 0], dtype=np.int8), None)], None, None, 2, 2, [2, 1]),
    # the cut falls inside a run of equal rows: the (K + 1)-th smallest is no exclusive bound
    "cut_inside_a_run": ([(np.array([1, 1, 1, 5], dtype=np.int8), None)], None, None, 2, 0, [0, 1]),
    # DESC, NULLS FIRST and an offset together
    "desc_nulls_first_page": ([(np.array([10, 77, 30, -77, 20], dtype=np.int16), _b([1, 0, 1, 0, 1]))], [True], [True], 2, 1, [3, 2]),
    # NaN behind +inf, all NaNs equal; k beyond the table
    "nan_last_k_beyond": ([(np.array([np.nan, 1.0, np.inf, np.nan], dtype=np.float32), None)], None, None, 9, 2, [0, 3]),
}

DESIGNED = {"ties_cut_by_value_not_row": "zeros_tie_at_the_cut", "tie_block_not_in_row_order": "ties_in_row_order",
            "truncated_image_treated_as_complete": "dropped_bit_decides", "straddling_field_low_bits_kept": "straddle_keeps_high_bits",
            "desc_complements_beyond_field": "desc_second_column", "null_bit_below_value": "null_above_value",
            "data_under_null_compared": "data_under_nulls", "offset_applied_before_selection": "offset_page",
            "k_th_is_k_plus_one": "cut_inside_a_run"}


@pytest.mark.parametrize("name", list(CASES))
def test_cases_written_by_hand(name):
    cols, desc, first, k, offset, want = CASES[name]
    assert tkr.top_k(cols, k, offset, desc, first).tolist() == want
    assert tkr.model_top_k(cols, k, offset, desc, first).tolist() == want
    assert tkr.model_top_k(cols, k, offset, desc, first).dtype == np.int32
    assert tkr.model_top_k(cols, k, offset, desc, first, slack=tkr.SLACK).tolist() == want          # the select stopped early
    assert tkr.model_top_k(cols, k, offset, desc, first, slack=1).tolist() == want


def test_every_mutation_is_listed_with_its_case():
    assert sorted(DESIGNED) == sorted(tkr.MUTATIONS)


@pytest.mark.parametrize("mutation", tkr.MUTATIONS)
def test_the_designed_case_kills_the_mutation(mutation):
    cols, desc, first, k, offset, want = CASES[DESIGNED[mutation]]
    assert tkr.model_top_k(cols, k, offset, desc, first, mutation).tolist() != want, mutation


def test_complete_and_truncated_images():
    """which images are complete, and the candidate counts: exactly K for a complete image whatever the ties"""
    ties = [(np.array([1, 1, 1, 1, 5, 0], dtype=np.int8), None)]
    info = {}
    assert tkr.model_top_k(ties, 3, 0, info=info).tolist() == [5, 0, 1]
    assert info == dict(complete=True, exact=True, candidates=3, c_less=1, ties=2, passes=1)
    _, complete, low = tkr.leading_image([(np.zeros(2, dtype=np.int64), None)])
    assert complete and low == 0
    _, complete, low = tkr.leading_image([(np.zeros(2, dtype=np.int64), _b([1, 1]))])
    assert not complete and low == 0
    _, complete, low = tkr.leading_image([(np.zeros(2, dtype=np.int8), _b([1, 1]))] * 7)
    assert complete and low == 1
    _, complete, low = tkr.leading_image([(np.zeros(2, dtype=np.int8), _b([1, 1]))] * 8)          # the eighth gives its null bit only
    assert not complete and low == 0
    _, complete, low = tkr.leading_image([(np.zeros(2, dtype=np.int64), None), (np.zeros(2, dtype=np.int8), None)])
    assert not complete and low == 0
    # a truncated image keeps every tie on L among the candidates
    info = {}
    cols = [(np.array([7, 6, 7, 6, 100], dtype=np.int64), _b([1, 1, 1, 1, 1]))]
    assert tkr.model_top_k(cols, 1, 0, info=info).tolist() == [1]
    assert not info["complete"] and info["candidates"] == 4


def test_the_image_is_monotone_in_the_order():
    """a before b in the full order implies L(a) <= L(b); for a complete image equal L means equal rows"""
    rng = np.random.default_rng(3)
    n = 300
    for trial in range(8):
        cols, desc, first = [], [], []
        for dt in rng.permutation([np.int8, np.int16, np.int32, np.int64, np.float32, np.float64])[:3]:
            if np.dtype(dt).kind == "f":
                data = rng.choice(np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, 5e-324], dtype=dt), size=n)
            else:
                data = rng.integers(-3, 4, size=n).astype(dt)
                data[rng.integers(0, n, size=4)] = np.iinfo(dt).min
                data[rng.integers(0, n, size=4)] = np.iinfo(dt).max
            cols.append((data, rng.random(n) < 0.7 if rng.random() < 0.7 else None))
            desc.append(bool(rng.integers(0, 2)))
            first.append(bool(rng.integers(0, 2)))
        image, complete, _ = tkr.leading_image(cols, desc, first)
        perm = orf.order_by_ex(cols, desc, first)
        along = [image[i] for i in perm]
        assert all(a <= b for a, b in zip(along, along[1:]))
        for k, offset in ((1, 0), (7, 0), (7, 5), (n - 1, 0), (n, 0), (n + 5, 3), (1, n - 1)):
            for slack in (0, 5, 40, tkr.SLACK):
                np.testing.assert_array_equal(tkr.model_top_k(cols, k, offset, desc, first, slack=slack), tkr.top_k(cols, k, offset, desc, first),
                                              err_msg=f"trial {trial} k={k} offset={offset} complete={complete} slack={slack}")


def test_select_finds_every_rank():
    rng = np.random.default_rng(11)
    for low, span in ((0, 64), (40, 24), (56, 8), (63, 1)):
        image = [int(x) << low for x in rng.integers(0, 1 << min(span, 62), size=257)]
        image[:40] = [image[0]] * 40                                                             # a run of ties
        ordered = sorted(image)
        for K in (1, 2, 40, 41, 128, 256, 257):
            T, c_less, ties, passes, tshift = tkr.select(image, K, low)
            assert tshift == 0 and T == ordered[K - 1] and c_less == sum(x < T for x in image) and ties == image.count(T)
            assert passes <= (64 - low + tkr.DIGIT - 1) // tkr.DIGIT
            for slack in (1, 39, 40, 300):                                                       # an early stop: T on its decided bits
                T, c_less, ties, fewer, tshift = tkr.select(image, K, low, slack)
                assert T >> tshift == ordered[K - 1] >> tshift and fewer <= passes and (tshift == 0 or ties <= slack)
                assert c_less == sum(x >> tshift < T >> tshift for x in image) and ties == sum(x >> tshift == T >> tshift for x in image)
                assert c_less < K <= c_less + ties


@pytest.mark.parametrize("kind", ["float32", "float64", "masked_float32"])
def test_the_tied_float_table_kills_ties_cut_by_value(kind):
    """the table tests/test_gpu_topk.py::test_cut_inside_runs_of_zeros_and_nans runs: on every one of its cuts the model that cuts the
    ties by their raw bits gives other rows than the oracle, and the unmutated model gives the oracle's"""
    npt = np.float64 if kind == "float64" else np.float32
    col, cuts = tkr.tied_floats(npt, 1025, np.random.default_rng(70), kind.startswith("masked"))
    raw = orf.bits_of(col[0])
    assert len(set(raw[col[0] == 0].tolist())) == 2 and len(set(raw[np.isnan(col[0])].tolist())) == 2
    for desc in (False, True):
        for first in (False, True):
            for k, offset in cuts(desc, first):
                want = tkr.top_k([col], k, offset, [desc], [first]).tolist()
                info = {}
                assert tkr.model_top_k([col], k, offset, [desc], [first], info=info).tolist() == want
                assert info["complete"] and info["exact"] and info["candidates"] == offset + k
                assert tkr.model_top_k([col], k, offset, [desc], [first], "ties_cut_by_value_not_row").tolist() != want, (desc, first, k, offset)
