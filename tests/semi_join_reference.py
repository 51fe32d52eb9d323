"""A plain Python / numpy model of gdf_amd_semi_join (include/gdf/gdf_amd_ext.h, csrc/semijoin.hip).  The reference project has no such
function; nothing here is derived from it, and nothing here is the code under test.

A key column is (data, valid): data a numpy array of a key dtype, valid a bool array or None (no mask = no nulls).

canonical      per row the tuple of its key elements: None for a null (NULLS_EQUAL only), the Python value otherwise, -0.0 == 0.0 as
               Python compares them.  A row that CANNOT MATCH has no tuple: a NaN in any column, or a null without NULLS_EQUAL.
semi_join      the contract: a left row qualifies when its tuple is (ANTI: is not) in the set of the right side's tuples; a row that
               cannot match never is.  The qualifying row numbers ascending, each once.
MUTATIONS      what a wrong kernel would do.  tests/test_semi_join_reference.py shows for each a hand-written table on which it changes
               the answer; tests/test_gpu_semi_join.py says which GPU case would catch which.
"""
import zlib

import numpy as np

MUTATIONS = ["null_matches_null_without_flag", "null_matches_value_with_flag", "nan_matches_nan", "negative_zero_distinct",
             "data_under_null_compared", "anti_drops_null_rows", "result_not_ascending", "duplicates_emitted_per_partner",
             "reserved_image_lost", "tag_hit_taken_as_match"]


def _bits(a):
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def canonical(cols, nulls_equal=False, mutation=None):
    """-> (list of per-row tuples, can_match bool array, has_null bool array)"""
    n = len(cols[0][0])
    can = np.ones(n, dtype=bool)
    has_null = np.zeros(n, dtype=bool)
    per_col = []
    for data, valid in cols:
        data = np.asarray(data)
        null = np.zeros(n, dtype=bool) if valid is None else ~np.asarray(valid, dtype=bool)
        has_null |= null
        compare_under_null = mutation == "data_under_null_compared"
        if data.dtype.kind == "f":
            nan = np.isnan(data) & (~null | compare_under_null)
            vals = _bits(data).tolist() if mutation == "negative_zero_distinct" else data.tolist()
            if mutation == "nan_matches_nan":
                vals = ["nan" if x else v for v, x in zip(vals, nan)]
            else:
                can &= ~nan
            zero = 0.0
        else:
            vals = data.tolist()
            zero = 0
        treat_as_equal = nulls_equal or mutation == "null_matches_null_without_flag"
        if compare_under_null:
            if treat_as_equal:
                vals = [(None, v) if nl else v for v, nl in zip(vals, null)]
            # (without the flag the mask is simply not looked at)
        elif not treat_as_equal:
            can &= ~null
        elif mutation == "null_matches_value_with_flag":
            vals = [zero if nl else v for v, nl in zip(vals, null)]             # the null bit forgotten: a null is the value field's 0
        else:
            vals = [None if nl else v for v, nl in zip(vals, null)]
        per_col.append(vals)
    return list(zip(*per_col)) if n else [], can, has_null


def image_is_reserved(cols_dtypes, tup, has_null_bits):
    """the EXACT image of csrc/semijoin.hip is all ones: 64 bits of integer columns, every element -1, no null bit anywhere"""
    if has_null_bits or any(np.dtype(d).kind == "f" for d in cols_dtypes):
        return False
    return sum(np.dtype(d).itemsize * 8 for d in cols_dtypes) == 64 and all(v == -1 for v in tup)


def _tag(tup, tag_bits):
    return zlib.crc32(repr(tup).encode()) & ((1 << tag_bits) - 1)


def semi_join(left, right, anti=False, nulls_equal=False, mutation=None, tag_bits=4):
    """the row numbers gdf_amd_semi_join owes (int32), optionally with one of MUTATIONS"""
    assert mutation is None or mutation in MUTATIONS
    assert len(left) == len(right)
    lt, lcan, lnull = canonical(left, nulls_equal, mutation)
    rt, rcan, _ = canonical(right, nulls_equal, mutation)
    partners = {}
    dtypes = [np.asarray(d).dtype for d, _ in left]
    null_bits = nulls_equal and any(v is not None for _, v in list(left) + list(right))
    for t, ok in zip(rt, rcan):
        if not ok:
            continue
        if mutation == "reserved_image_lost" and image_is_reserved(dtypes, t, null_bits):
            continue
        partners[t] = partners.get(t, 0) + 1
    tags = {_tag(t, tag_bits) for t in partners} if mutation == "tag_hit_taken_as_match" else set()
    hit = np.zeros(len(lt), dtype=bool)
    times = np.ones(len(lt), dtype=np.int64)
    for i, (t, ok) in enumerate(zip(lt, lcan)):
        if not ok:
            continue
        if t in partners:
            hit[i] = True
            times[i] = partners[t]
        elif tags and _tag(t, tag_bits) in tags:
            hit[i] = True
    take = ~hit if anti else hit
    if anti and mutation == "anti_drops_null_rows":
        take &= ~lnull
    rows = np.flatnonzero(take)
    if mutation == "duplicates_emitted_per_partner" and not anti:
        rows = np.repeat(rows, times[rows])
    if mutation == "result_not_ascending":
        rows = rows[::-1]
    return rows.astype(np.int32)
