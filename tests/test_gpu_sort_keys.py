"""-m gpu: the KEY domain of csrc/sort.hip -- gdf_order_by and the SORT-method group-by on the key tables of tests/groupby_keys.py.

order_rows packs the key columns by rules of its own (SortGroup, group_image): (value - min) in bit_length(max - min) bits, a
constant column one bit, floats their full width with -0.0 folded and NaN behind +inf, groups of at most 64 bits and 8 columns formed
from the last column backwards, digits on which every key agrees skipped, 9-bit digits where they save a pass.  The sort is stable,
so the permutation must be IDENTICAL to groupby_keys.order_reference (np.lexsort over the canonical columns): every case of the
table at 70001 rows (plain LSD passes) and at 300000 rows with GDF_HS_MIN_ROWS=4096 (the hybrid sort where the shape allows it), each
again under GDF_SORT_NO_HYBRID.  The SORT-method group-by is compared with groupby_keys.reference: keys, order, COUNT, the wrapped int64
SUM and every group's last row."""
import functools

import numpy as np
import pytest

import groupby_keys as gk

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in gk.CASES]
LSD_ROWS, HYBRID_ROWS = 70001, 300_000


@functools.lru_cache(maxsize=2)
def _case(name, rows):
    lay = gk.layout(gk.CASE[name], "many", rows, np.random.default_rng(21))
    return lay, gk.order_reference(lay.keys)


def _order_by(gdf, keys):
    from libgdf_amd.columns import column_from_numpy
    got = {}
    prof = gk.profile_of(gdf, lambda: got.update(p=gdf.api.order_by([column_from_numpy(k) for k in keys]).cpu().numpy()))
    return got["p"], prof


@pytest.mark.parametrize("name", NAMES)
def test_order_by_lsd(gdf, force_path, name):
    """70001 rows: below the hybrid sort's floor, so every group takes plain LSD passes (rs_scatter, or none for a constant image)"""
    lay, want = _case(name, LSD_ROWS)
    perm, prof = _order_by(gdf, lay.keys)
    assert "rs_make_keys" in prof and "hs_local" not in prof, sorted(prof)
    assert prof["rs_make_keys"] == len(gk.CASE[name].sort_bits), (prof, gk.CASE[name].sort_bits)      # one image per column group
    np.testing.assert_array_equal(perm, want)
    force_path("GDF_SORT_NO_HYBRID")
    perm2, prof2 = _order_by(gdf, lay.keys)
    np.testing.assert_array_equal(perm2, perm)
    assert prof2.get("rs_scatter", 0) == prof.get("rs_scatter", 0)


@pytest.mark.parametrize("name", NAMES)
def test_order_by_hybrid(gdf, force_path, name):
    """300000 rows, GDF_HS_MIN_ROWS=4096: wide images take the hybrid sort (top bits by array passes, the rest in LDS), narrow ones stay
    with LSD; either way the permutation is the reference's, and GDF_SORT_NO_HYBRID gives the same one"""
    lay, want = _case(name, HYBRID_ROWS)
    force_path("GDF_HS_MIN_ROWS", 4096)
    perm, prof = _order_by(gdf, lay.keys)
    assert "rs_make_keys" in prof, sorted(prof)
    np.testing.assert_array_equal(perm, want)
    force_path("GDF_SORT_NO_HYBRID")
    perm2, prof2 = _order_by(gdf, lay.keys)
    assert "hs_local" not in prof2, sorted(prof2)
    np.testing.assert_array_equal(perm2, perm)


def test_hybrid_sort_is_reached(gdf, force_path):
    """(so that test_order_by_hybrid is not vacuous: a 63-bit image of uniform keys at 300000 rows takes hs_local)"""
    lay, want = _case("total_63", HYBRID_ROWS)
    force_path("GDF_HS_MIN_ROWS", 4096)
    perm, prof = _order_by(gdf, lay.keys)
    assert "hs_local" in prof, sorted(prof)
    np.testing.assert_array_equal(perm, want)


@pytest.mark.parametrize("name", [f"sort_width_{w}" for w in (9, 17, 18, 25, 26, 27)] + ["sort_skipped_digit", "const_middle", "total_62", "nine_cols",
                                                                                        "total_65_sort"])
def test_radix_pass_count(gdf, force_path, name):
    """the rule in the comment above radix_sort_pairs (sort.hip): the varying bits [lo, hi) of an image are covered by (span + 8) / 9
    windows of 8 or 9 bits -- 9, 17 / 18 and 25 .. 27 bits take one, two and three 9-bit digits -- and a window on which every key
    agrees is skipped.  The launch count of rs_scatter from the profile against that rule (groupby_keys.scatter_launches), summed over
    the column groups"""
    lay, want = _case(name, LSD_ROWS)
    force_path("GDF_SORT_NO_HYBRID")
    perm, prof = _order_by(gdf, lay.keys)
    np.testing.assert_array_equal(perm, want)
    expect = sum(gk.scatter_launches(img) for img in gk.sort_group_images(lay.keys))
    assert prof.get("rs_scatter", 0) == prof.get("rs_count", 0) == expect, (prof, expect)
    if name.startswith("sort_width_"):
        w = int(name.rsplit("_", 1)[1])
        assert expect == (w + 8) // 9
    if name == "sort_skipped_digit":
        assert expect == 2                                             # three windows, the middle one agrees on every key


# ---- SORT-method group-by ----------------------------------------------------------------------------------------------------------------
def _run_sort(gdf, op, lay):
    from libgdf_amd.columns import GDF_SORT, column_from_numpy, get_dtype
    k, a, i = gdf.api.group_by(op, [column_from_numpy(c) for c in lay.keys], column_from_numpy(lay.vals), out_dtype=get_dtype(np.int64),
                               method=GDF_SORT, with_indices=True)
    return [x.cpu().numpy() for x in k], a.cpu().numpy(), i.cpu().numpy()


@functools.lru_cache(maxsize=2)
def _groups(name, rows):
    lay, _ = _case(name, rows)
    return gk.reference(lay.keys, lay.vals)


# single integer group: sg_heads compares the sorted images; a float column or a second group: rows_equal
SORT_GROUP_BY = ["min_int8", "max_int64", "min_int64", "i64_full", "span_full_small", "const_middle", "total_63", "total_64_wide", "total_64_natural",
                 "reserved_8_x_i8", "total_65_sort", "nine_cols", "sixteen_cols", "float32_specials", "float64_specials", "float32_across_zero",
                 "float64_then_int", "int_then_float64", "float32_nan", "float64_nan"]


@pytest.mark.parametrize("name", SORT_GROUP_BY)
def test_sort_method_group_by(gdf, force_path, name):
    """method=GDF_SORT with out_col_indices, through the sort (GDF_SORT_NO_DIRECT keeps small ranges off the direct path): groups in
    ascending order (NaN rows behind +inf, each its own group), COUNT and SUM in int64, every group's LAST row"""
    case = gk.CASE[name]
    lay, _ = _case(name, LSD_ROWS)
    g = _groups(name, LSD_ROWS)
    force_path("GDF_SORT_NO_DIRECT")
    for op in ("count", "sum"):
        got = {}
        prof = gk.profile_of(gdf, lambda: got.update(r=_run_sort(gdf, op, lay)))
        keys, agg, idx = got["r"]
        assert "sg_heads" in prof and "rs_make_keys" in prof and "gb_direct_aggregate" not in prof, sorted(prof)
        assert prof["rs_make_keys"] == len(case.sort_bits)
        gk.assert_groups(keys, agg, None, g, op, False, in_order=not case.has_nan, what=f"{name} {op}")
        want = gk.expected(g, op, False)
        a, b = gk.match_order(keys, agg), gk.match_order(g.keys, want)
        np.testing.assert_array_equal(idx[a], g.last[b], err_msg=f"{name} {op}: last rows")
        if case.has_nan:                                               # the non-NaN groups ascend, the NaN rows follow their column's +inf
            first = keys[0]
            assert not np.isnan(first[:int((~np.isnan(first)).sum())]).any()


@pytest.mark.parametrize("name", ["min_int64", "span_2k_small", "direct_16x24x32"])
def test_sort_method_direct_shortcut(gdf, name):
    """small ranges: the SORT method is served by the direct path plus a last-row pass (gb_direct_last_rows); same contract"""
    lay, _ = _case(name, LSD_ROWS)
    g = _groups(name, LSD_ROWS)
    for op in ("count", "sum"):
        got = {}
        prof = gk.profile_of(gdf, lambda: got.update(r=_run_sort(gdf, op, lay)))
        keys, agg, idx = got["r"]
        assert "gb_direct_aggregate" in prof and "gb_direct_last_rows" in prof and "rs_scatter" not in prof, sorted(prof)
        gk.assert_groups(keys, agg, None, g, op, False, in_order=True, what=f"{name} {op}")
        np.testing.assert_array_equal(idx, g.last)
