"""Helpers shared by the group-by VALUE tests (test_groupby_value_cases, test_gpu_groupby_values, test_gpu_sort_values) and by
test_gpu_groupby: a table of value recipes per value dtype, a reference written from the documented arithmetic (not from the
oracle and not from the kernels), key layouts that carry the recipe table onto every aggregation path of csrc/groupby.hip, and
the comparison / profile helpers the GPU files share.

A RECIPE is one group's multiset of values.  Every recipe is decidable exactly -- integer sums wrap, float values lie on a grid
m * 2^e on which every partial sum in any order (and in the oracle's float32 row order) is representable -- so no test built on
this module uses a tolerance.

The arithmetic (aggregation_operations.cuh:30-86, groupby.cuh:102-109, 308-328 of the reference; cell_avg's comment in
oracle/gdf_oracle.c):
  SUM / MIN / MAX   live in the INPUT dtype; an integer sum wraps to the input width (two's complement).
  COUNT             lives in the OUTPUT dtype: the row count wrapped to that integer width, or converted to that float type.
  AVG               = (avg_type)(sum / (avg_type)count): the count is first cast to the OUTPUT dtype (an int8 count of 128..255 is
                    negative, of 256 is 0), the division is then done in the C++ common type of (sum type, avg type) -- int for
                    two integer types of at most 32 bits, int64 if either has 64, the float type if exactly one is a float,
                    double for (float, double) -- truncating toward zero for integers, and the quotient is cast to the avg type.
                    An integer avg type whose wrapped count is 0 stores 0 (the reference divides by zero there; oracle and library
                    both say 0).

NOT SPECIFIED by the reference, so neither generated here nor compared (DESIGN.md section 4 repeats this list):
  * MIN / MAX of a group that mixes NaN with numbers: `v < acc` depends on the row order.  The recipes `nan_pos_mixed` /
    `nan_neg_mixed` carry ops SUM / AVG / COUNT only; the GPU file checks MIN / MAX of exactly these inputs for membership
    (NaN, or the min / max of the non-NaN values).
  * float sums whose intermediate overflows while the total does not: order dependent in the reference, and the library adds in
    double.  No recipe mixes finfo.max with a value of the other sign under SUM / AVG (`extreme_winners` is MIN / MAX / COUNT only).
  * a float-to-integer AVG output outside the integer's range (inf and NaN included, hence also a float sum over an integer avg
    type whose wrapped count is 0): undefined behaviour in C++.  avg_defined() says which (recipe, in, out) triples these are.
  * an integer AVG whose wrapped sum is the minimum of the division type (int for <= 32-bit pairs, else int64) and whose
    wrapped count is -1: the quotient overflows, which traps on the host.  avg_defined() refuses such a pair; the table has none.
  * the sign of a zero result: compared with ==, under which -0.0 equals +0.0.
"""
import math
from fractions import Fraction

import numpy as np

INT_DTYPES = [np.int8, np.int16, np.int32, np.int64]
FLT_DTYPES = [np.float32, np.float64]
VALUE_DTYPES = INT_DTYPES + FLT_DTYPES
OPS = ["sum", "min", "max", "count", "avg"]
ALL_OPS = frozenset(OPS)

# float grids: |m| <= GRID_M, at most GRID_ROWS rows per group, exponents (0, large, the denormal grid)
GRID_M = {np.dtype(np.float32): 2 ** 7, np.dtype(np.float64): 2 ** 20}
GRID_ROWS = {np.dtype(np.float32): 2 ** 10, np.dtype(np.float64): 2 ** 16}
GRID_EXP = {np.dtype(np.float32): (0, 100, -149), np.dtype(np.float64): (0, 900, -1074)}


class Recipe:
    """name, the group's values (an array of the value dtype), the ops it is specified for, and -- for the masked tests -- which
    of the values are null (a bool array, True = null; None = none)"""

    def __init__(self, name, values, ops=ALL_OPS, nulls=None):
        self.name, self.values, self.ops = name, values, frozenset(ops)
        self.nulls = None if nulls is None else np.asarray(nulls, dtype=bool)

    def __repr__(self):
        return f"Recipe({self.name}, {len(self.values)} rows)"


def _int_recipes(dt):
    info = np.iinfo(dt)
    lo, hi = int(info.min), int(info.max)
    a = lambda xs: np.array(xs, dtype=dt)
    r = [Recipe("one_min", a([lo])), Recipe("one_max", a([hi])), Recipe("one_zero", a([0])), Recipe("one_minus1", a([-1])),
         Recipe("all_max", a([hi] * 5)),                       # int64: every image equals MIN's identity ~0
         Recipe("all_min", a([lo] * 5)),                       # int64: every image equals MAX's identity 0
         Recipe("min_max_mixed", a([lo, hi, lo, hi, hi]))]
    for k in (2, 3, 257):                                      # sums that wrap the input width once and many times
        r.append(Recipe(f"{k}_x_max", a([hi] * k)))
        r.append(Recipe(f"{k}_x_min", a([lo] * k)))
    r.append(Recipe("wraps_to_zero", a([hi, hi, 2])))          # 2 * max + 2 = 2^width
    if np.dtype(dt) == np.int64:
        r.append(Recipe("three_2p62_and_5", a([2 ** 62] * 3 + [5])))
        r.append(Recipe("min_min", a([lo, lo])))
    for n in (1, 127, 128, 255, 256, 257):                     # the int8 COUNT / AVG count wrap
        r.append(Recipe(f"ones_{n}", np.ones(n, dtype=dt)))
    for n in (32768, 65536):                                   # the int16 count wrap
        r.append(Recipe(f"ones_{n}", np.ones(n, dtype=dt)))
    r.append(Recipe("minus7_over_2", a([-3, -4])))             # truncation toward zero: -3, not -4
    r.append(Recipe("minus7_over_3", a([-5, -1, -1])))
    return r


def _grid(dt, e, rows, seed):
    rng = np.random.default_rng(seed)
    m = rng.integers(-GRID_M[np.dtype(dt)], GRID_M[np.dtype(dt)] + 1, size=rows)
    v = np.ldexp(m.astype(np.float64), e).astype(dt)
    assert np.array_equal(v.astype(np.float64), np.ldexp(m.astype(np.float64), e))          # the grid is representable
    return v


def _float_recipes(dt):
    dt = np.dtype(dt)
    fi = np.finfo(dt)
    a = lambda xs: np.array(xs, dtype=dt)
    nan_pos = np.array([np.nan], dtype=dt)
    nan_pos = np.abs(nan_pos)
    nan_neg = -nan_pos                                                               # sign bit set
    ones_payload = np.array([2 ** (dt.itemsize * 8 - 1) - 1], dtype=np.int64).astype(f"i{dt.itemsize}").view(dt)   # +NaN, all-ones payload
    e0, ebig, eden = GRID_EXP[dt]
    r = []
    for name, e in (("grid_e0", e0), ("grid_big", ebig), ("grid_denormal", eden)):
        r.append(Recipe(name, _grid(dt, e, 200, 2011 + e)))
        r.append(Recipe(name + "_negatives", -np.abs(_grid(dt, e, 37, 4012 + e)) - np.ldexp(1.0, e).astype(dt)))
    r.append(Recipe("grid_e0_many_rows", _grid(dt, e0, 1000, 5)))
    half = np.abs(_grid(dt, e0, 50, 6)) + 1
    r.append(Recipe("cancels_to_zero", np.concatenate([half, -half])))
    r.append(Recipe("zeros_both_signs", a([0.0, -0.0, 0.0, -0.0])))
    r.append(Recipe("neg_zero_only", a([-0.0, -0.0])))
    r.append(Recipe("plus_inf", a([np.inf])))
    r.append(Recipe("minus_inf", a([-np.inf])))
    r.append(Recipe("plus_inf_and_finite", a([1.0, np.inf, -2.0, 3.0])))
    r.append(Recipe("minus_inf_and_finite", a([1.0, -np.inf, -2.0, 3.0])))
    r.append(Recipe("both_infs", a([np.inf, 1.0, -np.inf])))                         # SUM / AVG: NaN
    r.append(Recipe("nan_pos_mixed", np.concatenate([a([1.0, -2.0]), nan_pos, a([3.0])]), ops=("sum", "avg", "count")))
    r.append(Recipe("nan_neg_mixed", np.concatenate([a([1.0, -2.0]), nan_neg, a([3.0])]), ops=("sum", "avg", "count")))
    r.append(Recipe("nan_only", np.concatenate([nan_pos, nan_pos, nan_pos])))
    r.append(Recipe("nan_only_negative", np.concatenate([nan_neg, nan_neg])))
    r.append(Recipe("nan_only_all_ones_payload", np.concatenate([ones_payload, ones_payload])))   # float64: the image is MIN's identity
    r.append(Recipe("one_finfo_max", a([fi.max])))
    r.append(Recipe("one_minus_finfo_max", a([-fi.max])))
    r.append(Recipe("one_finfo_tiny", a([fi.tiny])))
    r.append(Recipe("one_smallest_denormal", a([fi.smallest_subnormal])))
    r.append(Recipe("extreme_winners", a([1.0, fi.max, fi.tiny, -fi.max, -fi.tiny, 0.0]), ops=("min", "max", "count")))
    r.append(Recipe("tiny_winners", a([fi.tiny, fi.smallest_subnormal, 1.0]), ops=("min", "max", "count")))
    r.append(Recipe("overflow_to_inf", a([fi.max, fi.max])))
    r.append(Recipe("overflow_to_minus_inf", a([-fi.max, -fi.max, -fi.max])))
    for n in (1, 127, 128, 255, 256, 257):                     # the int8 AVG count wrap under float sums
        r.append(Recipe(f"ones_{n}", np.ones(n, dtype=dt)))
    for x in r:
        assert len(x.values) <= GRID_ROWS[dt]
    return r


_TABLES = {}


def recipes(dtype, op=None):
    """the recipe table of a value dtype; with op, only the recipes specified for that op (see the module docstring)"""
    dt = np.dtype(dtype)
    if dt not in _TABLES:
        _TABLES[dt] = _int_recipes(dt) if dt.kind == "i" else _float_recipes(dt)
    return [r for r in _TABLES[dt] if op is None or op in r.ops]


def masked_recipes(dtype, op=None):
    """the table for the masked tests: every recipe with a third of its values null (deterministically), and next to them the groups
    whose every VALID value is the type's extreme -- for int64 the accumulator's identity image under MIN (max) and MAX (min) --
    with nulls mixed in, and groups that are entirely null"""
    dt = np.dtype(dtype)
    lo, hi = (np.iinfo(dt).min, np.iinfo(dt).max) if dt.kind == "i" else (-np.inf, np.inf)
    out = []
    for r in recipes(dt, op):
        nulls = (np.arange(len(r.values)) % 3) == 1
        out.append(Recipe(r.name, r.values, r.ops, nulls))
    mix = np.array([False, True, False, False, True, False])
    out.append(Recipe("all_max_some_null", np.full(6, hi, dtype=dt), nulls=mix))
    out.append(Recipe("all_null_a", np.full(4, hi, dtype=dt), nulls=np.ones(4, dtype=bool)))
    out.append(Recipe("all_min_some_null", np.full(6, lo, dtype=dt), nulls=mix))
    out.append(Recipe("all_null_b", np.full(3, lo, dtype=dt), nulls=np.ones(3, dtype=bool)))
    return [r for r in out if op is None or op in r.ops]


# ---- the reference ------------------------------------------------------------------------------------------------------------------
def _wrap(v, dt):
    bits = np.dtype(dt).itemsize * 8
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _trunc_div(s, c):
    q = abs(s) // abs(c)
    return q if (s < 0) == (c < 0) else -q


def _float_sum(values, dt):
    """the exactly rounded sum of the values in dtype dt (IEEE rules for inf / NaN); on a grid the sum is representable and the
    rounding is no rounding"""
    vals = [float(v) for v in values]
    if any(math.isnan(v) for v in vals):
        return dt.type(np.nan)
    pinf, ninf = any(v == math.inf for v in vals), any(v == -math.inf for v in vals)
    if pinf or ninf:
        return dt.type(np.nan if pinf and ninf else (np.inf if pinf else -np.inf))
    total = sum((Fraction(v) for v in vals), Fraction(0))
    if abs(total) > Fraction(float(np.finfo(dt).max)):
        assert abs(total) >= Fraction(2) ** int(np.finfo(dt).maxexp), "rounds to inf or to finfo.max: not an exact recipe"
        return dt.type(np.inf if total > 0 else -np.inf)
    f = dt.type(float(total))
    assert Fraction(float(f)) == total, "the recipe's sum is not representable: not an exact recipe"
    return f


def _typed_sum(values, dt):
    if dt.kind == "i":
        return _wrap(sum(int(v) for v in values), dt)
    return _float_sum(values, dt)


def _division_type(in_dt, out_dt):
    return np.dtype(np.int64) if max(in_dt.itemsize, out_dt.itemsize) == 8 else np.dtype(np.int32)


def avg_defined(values, in_dtype, out_dtype):
    """False for the (values, sum type, avg type) triples the reference leaves undefined: see the module docstring"""
    in_dt, out_dt = np.dtype(in_dtype), np.dtype(out_dtype)
    n = len(values)
    s = _typed_sum(values, in_dt)
    if out_dt.kind == "f":
        return True
    c = _wrap(n, out_dt)
    if in_dt.kind == "i":
        return not (c == -1 and s == np.iinfo(_division_type(in_dt, out_dt)).min)
    if c == 0:
        return False
    with np.errstate(all="ignore"):
        q = float(in_dt.type(s) / in_dt.type(c))
    return math.isfinite(q) and np.iinfo(out_dt).min <= math.trunc(q) <= np.iinfo(out_dt).max


def reference(op, recipe, in_dtype, out_dtype=None):
    """the aggregate of one group as a numpy scalar of the result dtype.  `recipe` is a Recipe or an array of values (the nulls of
    a Recipe are skipped; a group without a valid value has no reference: None)."""
    in_dt = np.dtype(in_dtype)
    out_dt = in_dt if out_dtype is None else np.dtype(out_dtype)
    values = recipe.values if isinstance(recipe, Recipe) else np.asarray(recipe)
    if isinstance(recipe, Recipe) and recipe.nulls is not None:
        values = values[~recipe.nulls]
    assert values.dtype == in_dt
    n = len(values)
    if op == "count":
        return out_dt.type(_wrap(n, out_dt)) if out_dt.kind == "i" else out_dt.type(n)
    if n == 0:
        return None
    if op == "sum":
        return in_dt.type(_typed_sum(values, in_dt))
    if op in ("min", "max"):
        if in_dt.kind == "i":
            return in_dt.type(min(int(v) for v in values) if op == "min" else max(int(v) for v in values))
        nan = np.isnan(values)
        if nan.all():
            return in_dt.type(np.nan)
        assert not nan.any(), "MIN / MAX of NaN mixed with numbers is unspecified"
        return in_dt.type(min(float(v) for v in values) if op == "min" else max(float(v) for v in values))
    assert op == "avg"
    assert avg_defined(values, in_dt, out_dt), "unspecified AVG"
    s = _typed_sum(values, in_dt)
    with np.errstate(all="ignore"):
        if in_dt.kind == "i" and out_dt.kind == "i":
            c = _wrap(n, out_dt)
            return out_dt.type(0 if c == 0 else _wrap(_wrap(_trunc_div(s, c), _division_type(in_dt, out_dt)), out_dt))
        if in_dt.kind == "i":                                   # integer sum, float avg type: both converted to it
            return out_dt.type(out_dt.type(s) / out_dt.type(n))
        if out_dt.kind == "i":                                  # float sum, integer avg type: in the sum's float type, then truncated
            c = _wrap(n, out_dt)
            return out_dt.type(math.trunc(float(in_dt.type(s) / in_dt.type(c))))
        if in_dt == out_dt:
            return out_dt.type(in_dt.type(s) / in_dt.type(n))
        return out_dt.type(np.float64(s) / np.float64(out_dt.type(n)))       # (float, double) either way round: in double


# ---- key layouts --------------------------------------------------------------------------------------------------------------------
# path name -> how the existing tests of test_gpu_groupby.py reach it.  `rows`: the table is filled up to this many rows.
# `filler`: "single" = filler groups of ONE row each (they also supply the group count the path needs); "few" = a few thousand
# filler groups sharing the rows (the paths that hold every group in LDS); "hot" = half of the filler on keys inside the first
# window of 4096 ids, the other half on single-row keys beyond it.  `force`: the switches of csrc/lab.h the test sets.
# `kernel`: a kernel name only this path launches; `absent`: names that must NOT appear.
PATHS = {
    "direct":        dict(rows=4500, filler="single", key="i64", force={}, kernel="gb_direct_aggregate", absent=()),
    "dense":         dict(rows=4500, filler="single", key="i64", force={"GDF_GB_NO_DIRECT": "1"}, kernel="gb_dense_aggregate", absent=("gb_direct_aggregate",)),
    "lds_dict":      dict(rows=(1 << 22) + 77, filler="few", key="sparse", force={}, kernel="gb_ld_aggregate", absent=("gb_dense_aggregate",)),
    "lds_dict_off":  dict(rows=(1 << 22) + 77, filler="few", key="sparse", force={"GDF_GB_NO_LDS_DICT": "1"}, kernel="gb_dense_aggregate", absent=("gb_ld_aggregate",)),
    # (the statically typed and the type-switch scatter kernels are both profiled as "gbp_scatter": the switch, not the name, tells them apart)
    "part_fused":    dict(rows=(1 << 20) + 4321, filler="single", key="i64", force={}, kernel="gbp_scatter", absent=("gbp_scatter_hot", "gbp_sample_hist")),
    "part_dynamic":  dict(rows=(1 << 20) + 4321, filler="single", key="i64", force={"GDF_GBP_DYNAMIC": "1"}, kernel="gbp_scatter", absent=("gbp_scatter_hot", "gbp_sample_hist")),
    "hot_inside":    dict(rows=(1 << 22) + 77, filler="hot", key="i64", force={}, kernel="gbp_scatter_hot", absent=()),
    "hot_outside":   dict(rows=(1 << 22) + 77, filler="hot", key="i64", force={"GDF_GBP_HOT_WINDOW": "3"}, kernel="gbp_scatter_hot", absent=()),
    # the speculative layout lives inside the fused pass, whose own floor is 2^20 rows: that is the smallest row count that takes it
    "spec":          dict(rows=1 << 20, filler="single", key="i64", force={"GDF_GBP_SPEC_MIN_ROWS": "1"}, kernel="gbp_sample_hist", absent=("gbp_count",)),
    "spec_off":      dict(rows=1 << 20, filler="single", key="i64", force={"GDF_GBP_SPEC_MIN_ROWS": "1", "GDF_GBP_NO_SPEC": "1"}, kernel="gbp_count", absent=("gbp_sample_hist",)),
    "part_small":    dict(rows=300_000, filler="single", key="i64", force={}, kernel="gb_part_aggregate", absent=("gbp_scatter",)),
    "sorted":        dict(rows=300_000, filler="single", key="i64", force={"GDF_GB_NO_PART": "1"}, kernel="gb_sorted_reduce", absent=("gb_part_aggregate",)),
    "table":         dict(rows=300_000, filler="single", key="i64", force={"GDF_GB_NO_SORTED": "1"}, kernel="gb_aggregate_packed", absent=("gb_part_aggregate",)),
    "first_row":     dict(rows=30_000, filler="single", key="f64", force={"GDF_GB_NO_FLOAT_IMAGE": "1"}, kernel="gb_aggregate_rows", absent=("gb_aggregate_packed",)),
}
HOT_IDS = 4096            # csrc/groupby.hip GBP_HOT_IDS
FEW_FILLER_GROUPS = 3000


class Layout:
    """keys: list of key columns; vals; val_valid: bool array or None (True = valid); key_of_recipe[i]: the key of recipe i;
    filler_keys: the filler groups' keys; is_filler: which rows are filler; recipes: the table"""


def layout(path, recs, rng, rows=None, filler_groups=None):
    """place recipe g on key number g of a key layout that reaches `path`, fill the table up with filler groups holding small values
    until the path's preconditions hold (row count, group count, key sparsity), and shuffle the rows.  filler_groups: spread a
    "single" filler over that many groups instead of one group per row (the masked oracle walks the groups in Python)."""
    p = PATHS[path]
    dt = recs[0].values.dtype
    total = p["rows"] if rows is None else rows
    R = len(recs)
    g_of = np.concatenate([np.full(len(r.values), g, dtype=np.int64) for g, r in enumerate(recs)])
    vals = np.concatenate([r.values for r in recs])
    nulls = np.concatenate([r.nulls if r.nulls is not None else np.zeros(len(r.values), dtype=bool) for r in recs])
    nfill = max(total - len(vals), 16)
    if p["filler"] == "single" and filler_groups:
        fg = R + np.arange(nfill, dtype=np.int64) % filler_groups
    elif p["filler"] == "single":
        fg = R + np.arange(nfill, dtype=np.int64)
    elif p["filler"] == "few":
        fg = R + rng.integers(0, FEW_FILLER_GROUPS, size=nfill)
    else:
        assert R < HOT_IDS // 2
        fg = np.concatenate([rng.integers(R, HOT_IDS, size=nfill // 2),
                             HOT_IDS + np.arange(nfill - nfill // 2, dtype=np.int64) % (filler_groups or nfill)])
    fv = ((np.arange(nfill) % 5) - 2).astype(dt)                 # small values: -2 .. 2
    g_all = np.concatenate([g_of, fg])
    v_all = np.concatenate([vals, fv])
    n_all = np.concatenate([nulls, np.zeros(nfill, dtype=bool)])
    order = rng.permutation(len(g_all))
    g_all, v_all, n_all = g_all[order], v_all[order], n_all[order]
    if p["key"] == "sparse":
        lut = np.unique(rng.integers(-2 ** 62, 2 ** 62, size=R + FEW_FILLER_GROUPS + 64, dtype=np.int64))[:R + FEW_FILLER_GROUPS]
        lut[0] = -2 ** 63                                        # the library's reserved key pattern is a normal key
        assert len(lut) == R + FEW_FILLER_GROUPS
        conv = lambda g: lut[g]
    elif p["key"] == "f64":
        conv = lambda g: g.astype(np.float64)
    else:
        conv = lambda g: g
    out = Layout()
    out.path = path
    out.keys = [np.ascontiguousarray(conv(g_all))]
    out.vals = np.ascontiguousarray(v_all)
    out.val_valid = ~n_all if n_all.any() else None
    out.key_of_recipe = conv(np.arange(R, dtype=np.int64))
    out.filler_keys = conv(np.unique(fg))
    out.is_filler = g_all >= R
    out.recipes = recs
    return out


# ---- GPU-side helpers shared with test_gpu_groupby.py ------------------------------------------------------------------------------
def kernels_of(gdf, call):
    """names of the kernels one library call launched (the exported profile hooks of include/gdf/gdf_amd_ext.h)"""
    from bench import read_profile
    lib = gdf._binding._gdf_cdll
    lib.gdf_amd_profile_reset(); lib.gdf_amd_profile_enable(1)
    try:
        call()
    finally:
        lib.gdf_amd_profile_enable(0)
    return set(read_profile(gdf))


def zipf(rs, n, values):
    u = rs.random_sample(n)
    return np.clip(np.exp(u * np.log(values + 1.0)).astype(np.int64) - 1, 0, values - 1)      # p(rank) ~ 1 / rank, rank = value


def run_masked(gdf, op, keys, vals, key_valids, val_valid, out_dtype=None, sort_result=False):
    """the masked HASH group-by through the C ABI -> (keys, aggregate, aggregate-valid), rows in lexicographic key order"""
    from libgdf_amd.columns import column_from_numpy, get_dtype
    kc = [column_from_numpy(k, v) for k, v in zip(keys, key_valids)]
    vc = column_from_numpy(vals, val_valid)
    od = None if out_dtype is None else get_dtype(out_dtype)
    gk, ga, gok = gdf.api.group_by(op, kc, vc, out_dtype=od, sort_result=sort_result, with_masks=True)
    gk, ga, gok = [x.cpu().numpy() for x in gk], ga.cpu().numpy(), gok.numpy()
    if not (sort_result or op == "avg"):
        order = np.lexsort(tuple(reversed(gk)))
        gk, ga, gok = [k[order] for k in gk], ga[order], gok[order]
    return gk, ga, gok


def check_masked(gdf, op, keys, vals, key_valids, val_valid, out_dtype=None, sort_result=False, exact=False):
    """against oracle.group_by_masked: keys, valid bits, zeros in the null groups; float sums / averages within 1e-6 relative unless
    `exact` (the value tests' grids), everything else bit for bit"""
    from oracle import oracle
    gk, ga, gok = run_masked(gdf, op, keys, vals, key_valids, val_valid, out_dtype, sort_result)
    ek, ea, eok = oracle.group_by_masked(op, keys, vals, key_valids, val_valid, out_dtype)
    assert len(ga) == len(ea)
    for g, e in zip(gk, ek):
        np.testing.assert_array_equal(g, e)
    np.testing.assert_array_equal(gok, eok)
    assert (ga[~gok] == 0).all()
    if not exact and op in ("sum", "avg") and np.asarray(vals).dtype.kind == "f":
        np.testing.assert_allclose(ga[gok].astype(np.float64), ea[eok].astype(np.float64), rtol=1e-6, atol=1e-9)
    else:
        np.testing.assert_array_equal(ga[gok], ea[eok])
    return gk, ga, gok
