"""-m gpu: the KEY domain of gdf_group_by_* (HASH) on every key-packing path of csrc/groupby.hip.

The value tests (test_gpu_groupby_values.py) put one key column of group numbers under every path.  Here the key tables of
tests/groupby_keys.py -- columns at their dtype's minimum and maximum, spans of exactly 2^k - 1 and 2^k, totals that sit on every bit
budget the planner branches on, the reserved word 1 << 63 of the natural layout spelled in two, three and eight columns, float keys
with every special value -- go through the paths of groupby_values.PATHS.  Every call asserts the path from the kernel names of the
profile hook and compares keys (integers exactly, floats with == plus NaN membership), COUNT and SUM in int64 (a wrapped sum of
scrambled row numbers: a group that swapped one row for another shows), MIN under masks, AVG / sort_result on a subset (their output
must stand in the reference's order).  No tolerance anywhere.  The reference is groupby_keys.reference (plain numpy).

Budgets (groupby.hip): total > 63 declines the range plan (:1114); total + vbit + null_bit <= 64 keeps the sorted path (:3275);
total - 13 <= 13 selects the partitioned path (:3270); part_bits in 1 .. 11 and >= 2^20 rows the fused pass (:2835); the product of the
spans <= 12288 the direct path (:2570-2576).  The `<= 32` test of :3271 never decides anything: see DESIGN.md section 4."""
import functools

import numpy as np
import pytest

import groupby_keys as gk

pytestmark = pytest.mark.gpu
PATHS = gk.PATHS
FUSED_ROWS = PATHS["part_fused"]["rows"]
REGIME = {"single": "many", "few": "few", "hot": "hot"}


@functools.lru_cache(maxsize=2)
def _table(name, regime, rows):
    return gk.layout(gk.CASE[name], regime, rows, np.random.default_rng(7))


@functools.lru_cache(maxsize=2)
def _case(name, regime, rows, variant):
    """(layout, key valids, value valid, reference groups): computed once, shared by the paths that run on the same table"""
    lay = _table(name, regime, rows) if not name.startswith("guess:") else gk.guess_layout(name[6:], rows, np.random.default_rng(7))
    kv, vv = gk.masks(lay, variant, np.random.default_rng(8))
    return lay, kv, vv, gk.reference(lay.keys, lay.vals, kv, vv)


def _check(gdf, force_path, name, path, ops=("count", "sum"), variant="plain", regime=None, rows=None, kernel="path", absent="path",
           force="path", sort_result=False, launches=None):
    """one library call per op on the key table `name`, laid out for `path`: the path asserted from the kernel names, the groups
    exact against the reference.  kernel / absent / force default to the path's entry in groupby_values.PATHS."""
    p = PATHS[path]
    regime = regime or REGIME[p["filler"]]
    rows = rows or p["rows"]
    kernel = p["kernel"] if kernel == "path" else kernel
    absent = p["absent"] if absent == "path" else absent
    force = p["force"] if force == "path" else force
    lay, kv, vv, ref = _case(name, regime, rows, variant)
    masked = variant != "plain"
    for op in ops:
        for k, v in force.items():
            force_path(k, v)
        got = {}
        try:
            prof = gk.profile_of(gdf, lambda: got.update(r=gk.run_hash(gdf, op, lay.keys, lay.vals, kv, vv, sort_result and op != "avg")))
        finally:
            for k in force:
                force_path(k, None)
        what = f"{name} {path} {variant} {op}"
        assert kernel in prof and not (set(absent) & set(prof)), (what, sorted(prof))
        if launches:
            for k, v in launches.items():
                assert prof.get(k, 0) == v, (what, k, prof)
        keys, agg, ok = got["r"]
        gk.assert_groups(keys, agg, ok, ref, op, masked, in_order=sort_result or op == "avg", what=what)


EXTREMES = [f"{e}_{d}" for d in ("int8", "int16", "int32", "int64") for e in ("min", "max")] + ["int8_full", "i64_straddles_0", "i64_straddles_2p32"]
RESERVED = ["total_64_natural", "reserved_i16_i16_i32", "reserved_8_x_i8"]


# ---- direct index ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXTREMES + ["span_full_small", "span_2k_small", "const_first", "const_middle", "const_last",
                                             "direct_96x128", "direct_16x24x32"])
def test_direct_path(gdf, force_path, name):
    """4500 rows, the product of the spans at most 12288: gb_direct_aggregate; (value - lo) with lo at the dtype's minimum, hi at its
    maximum; AVG's output is the sorted one"""
    _check(gdf, force_path, name, "direct", ops=("count", "sum", "avg"), regime="few")


@pytest.mark.parametrize("name", ["direct_97x127", "i64_full", "span_full_large"])
def test_direct_path_declines(gdf, force_path, name):
    """12319 ids, a span of 2^64 - 1 (which reads as 0) and a 2^40 span: no gb_direct_aggregate, the dense dictionary"""
    _check(gdf, force_path, name, "direct", regime="few", kernel="gb_dense_aggregate", absent=("gb_direct_aggregate",))


@pytest.mark.parametrize("which", ["near_max", "near_min", "edge_inside"])
def test_direct_guessed_window(gdf, force_path, which):
    """one int64 column, 2^20 + 4321 rows: the window guessed from the first 65536 rows, widened to 12288 ids, saturates at INT64_MAX /
    INT64_MIN; rows exactly on the widened window's edges are inside it: ONE aggregation launch"""
    _check(gdf, force_path, "guess:" + which, "direct", rows=FUSED_ROWS, regime=which, launches={"gb_direct_aggregate": 1})


def test_direct_guessed_window_one_row_outside(gdf, force_path):
    """a row one below the widened window: the flag is raised and the call repeats with the exact range -- two launches, the
    reference's groups"""
    _check(gdf, force_path, "guess:edge_outside", "direct", rows=FUSED_ROWS, regime="edge_outside", launches={"gb_direct_aggregate": 2})


# ---- dense dictionary, LDS dictionary ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXTREMES + RESERVED + ["float32_specials", "float32_across_zero", "float64_across_zero", "total_62", "total_63",
                                                        "float32_then_int", "int_then_float64"])
def test_dense_dictionary(gdf, force_path, name):
    """GDF_GB_NO_DIRECT at 4500 rows: gb_dict_build / gb_dense_aggregate on the natural layout (the reserved word takes the dictionary's
    `special` slot) and on the range layout (62 and 63 bits; float images: -0.0 with +0.0, 32 image bits between the infinities)"""
    _check(gdf, force_path, name, "dense", regime="few")


@pytest.mark.parametrize("variant", ["vmask", "kmask"])
@pytest.mark.parametrize("name", ["min_int64", "total_64_natural", "float32_specials", "total_63"])
def test_dense_dictionary_masked(gdf, force_path, name, variant):
    _check(gdf, force_path, name, "dense", ops=("count", "sum", "min"), variant=variant, regime="few", force={})


@pytest.mark.parametrize("name", EXTREMES + RESERVED + ["float32_specials", "float64_across_zero", "total_62", "total_63"])
def test_lds_dictionary(gdf, force_path, name):
    """2^22 + 77 rows, about 3000 groups: gb_ld_encode / gb_ld_aggregate; GDF_GB_NO_LDS_DICT: the L2 dictionary on the same table"""
    for path in ("lds_dict", "lds_dict_off"):                                   # (the narrow int64 boxes would take the direct path)
        _check(gdf, force_path, name, path, force={**PATHS[path]["force"], "GDF_GB_NO_DIRECT": "1"})


@pytest.mark.parametrize("name", ["total_13", "total_14"])
def test_dense_dictionary_claims_the_smallest_totals(gdf, force_path, name):
    """2^20 + 4321 rows over every cell of a 13- / 14-bit box: at most 16384 groups, so the dictionary keeps them (total 14 has
    part_bits 1, but never reaches the fused pass: 15 is the lowest total that does).  GDF_GB_NO_DIRECT: 8192 ids are a direct range"""
    _check(gdf, force_path, name, "part_fused", kernel="gb_dense_aggregate", absent=("gbp_scatter", "gb_part_aggregate", "gb_direct_aggregate"),
           force={"GDF_GB_NO_DIRECT": "1"})


@pytest.mark.parametrize("variant", ["plain", "vmask"])
def test_total_14_is_fused_when_the_groups_are_counted(gdf, force_path, variant):
    """AVG and masked values keep a row count per group, and the dictionary then holds 12288 groups, not 16384: the same 14-bit table
    is declined there and takes the fused pass with part_bits 1 -- its lower end"""
    _check(gdf, force_path, "total_14", "part_fused", ops=("avg",) if variant == "plain" else ("sum", "min"), variant=variant,
           force={"GDF_GB_NO_DIRECT": "1"})


# ---- fused partition pass -----------------------------------------------------------------------------------------------------------------
FUSED = ["total_15", "total_24", "two_i32_static_20", "three_cols_18", "four_cols_20", "float32_band", "float64_band"]


@pytest.mark.parametrize("variant", ["plain", "vmask", "kmask"])
@pytest.mark.parametrize("name", FUSED)
def test_fused_partition_pass(gdf, force_path, name, variant):
    """2^20 + 4321 rows: both ends of the fused window (totals 15 and 24), the statically typed key signature (int64 + int32, two
    int32) and with GDF_GBP_DYNAMIC the type switch, three and four columns (the c >= 2 loop of gbp_pack32), float keys through
    gbp_load_col; with a value mask (vbit) and with a key mask (null_bit)"""
    ops = ("count", "sum") if variant == "plain" else ("sum", "min")
    _check(gdf, force_path, name, "part_fused", ops=ops, variant=variant)
    if name in ("total_15", "total_24", "two_i32_static_20"):
        _check(gdf, force_path, name, "part_dynamic", ops=ops[1:], variant=variant)


@pytest.mark.parametrize("path", ["hot_inside", "hot_outside"])
def test_hot_window(gdf, force_path, path):
    """the two-column static table at 2^22 + 77 rows, half of the filler below id 4096; the corners of the box lie inside (lo, lo) and
    outside (hi, hi) that window"""
    _check(gdf, force_path, "total_24", path, ops=("sum", "min"))


@pytest.mark.parametrize("path", ["spec", "spec_off"])
def test_speculative_layout(gdf, force_path, path):
    _check(gdf, force_path, "total_24", path, ops=("sum", "min"))


@pytest.mark.parametrize("rows", [PATHS["part_small"]["rows"], FUSED_ROWS])
@pytest.mark.parametrize("name", ["total_25", "total_26"])
def test_partitioned_not_fused(gdf, force_path, name, rows):
    """part_bits 12 and 13: past GBP_MAX_PART_BITS, so pair build + radix sort + gb_part_aggregate even at 2^20 + 4321 rows"""
    _check(gdf, force_path, name, "part_small", rows=rows)


# ---- sorted, table, first row ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["total_25", "three_cols_18", "float32_band", "nine_cols"])
def test_sorted_path_forced(gdf, force_path, name):
    _check(gdf, force_path, name, "sorted")


@pytest.mark.parametrize("name", ["total_27", "total_30", "total_31", "total_32", "total_62", "total_63", "sixteen_cols", "span_2k_large"])
def test_sorted_path_by_budget(gdf, force_path, name):
    """27 bits is the first total past GB_PART_MAX_BITS: no force, gb_sorted_reduce and no partition kernel"""
    _check(gdf, force_path, name, "sorted", force={}, absent=("gb_part_aggregate", "gbp_scatter"))


def test_63_bits_and_the_mask_bits(gdf, force_path):
    """63 + vbit = 64 stays sorted; 63 + vbit + null_bit = 65 goes to the table on packed keys"""
    _check(gdf, force_path, "total_63", "sorted", ops=("sum", "min"), variant="vmask", force={})
    _check(gdf, force_path, "total_63", "sorted", ops=("sum", "min"), variant="kmask", force={})
    _check(gdf, force_path, "total_63", "sorted", ops=("sum", "min"), variant="bothmask", force={}, kernel="gb_aggregate_packed",
           absent=("gb_sorted_reduce",))


def test_natural_64_bits_two_int32(gdf, force_path):
    """two full-range int32 columns: no range plan, the natural layout (unordered) on the sorted path -- sort_result re-sorts the
    result rows; with a value mask 64 + vbit does not fit and the table takes it, the reserved word live in slot T"""
    _check(gdf, force_path, "total_64_natural", "sorted", force={})
    _check(gdf, force_path, "total_64_natural", "sorted", ops=("sum", "avg"), force={}, sort_result=True)
    _check(gdf, force_path, "total_64_natural", "sorted", ops=("sum", "min"), variant="vmask", force={}, kernel="gb_aggregate_packed",
           absent=("gb_sorted_reduce",))


@pytest.mark.parametrize("name", RESERVED + ["total_63", "i64_full"])
def test_table_on_packed_keys(gdf, force_path, name):
    _check(gdf, force_path, name, "table")


@pytest.mark.parametrize("name", ["total_64_wide", "total_65_sort", "float64_specials", "float32_nan", "float64_nan"])
def test_first_row_table(gdf, force_path, name):
    """64 bits in 12 bytes, float64 with both infinities (a 64-bit image span), NaN keys (every NaN row its own group): the plan declines
    by itself and the row-comparing table takes the rows"""
    _check(gdf, force_path, name, "first_row", force={}, regime="few" if "float" in name else "many")


# ---- the order of sorted output ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,path,kw", [
    ("min_int64", "direct", dict(regime="few")),
    ("float32_specials", "dense", dict(regime="few")),
    ("float64_across_zero", "dense", dict(regime="few")),
    ("total_62", "lds_dict", {}),
    ("three_cols_18", "part_fused", {}),
    ("total_25", "part_small", {}),
    ("total_63", "sorted", dict(force={})),
    ("reserved_i16_i16_i32", "table", {}),
    ("float64_specials", "first_row", dict(force={}, regime="few")),
    ("total_64_wide", "first_row", dict(force={})),
], ids=lambda x: x if isinstance(x, str) else "")
def test_sorted_output(gdf, force_path, name, path, kw):
    """sort_result=True (and AVG, whose output is always sorted): the rows stand in the reference's order -- negatives before positives in
    every column, -inf < ... < -0.0 == +0.0 < ... < +inf"""
    _check(gdf, force_path, name, path, ops=("sum", "avg"), sort_result=True, **kw)


def test_17_key_columns(gdf):
    """one column more than MAX_KEY_COLS: make_key_table's error code, and no output column written"""
    import ctypes as C
    import torch
    from libgdf_amd import GDFError, libgdf, new_context
    from libgdf_amd.columns import GDF_HASH, Column, column_array, column_from_numpy
    n = 5000
    keys = [column_from_numpy((np.arange(n) % (3 + c)).astype(np.int8)) for c in range(gk.MAX_KEY_COLS + 1)]
    vals = column_from_numpy(gk.scramble(n))
    out_keys = [Column(torch.full((n,), 77, dtype=torch.int8, device="cuda"), None, k.c.dtype, size=n) for k in keys]
    out_agg = Column(torch.full((n,), 77, dtype=torch.int64, device="cuda"), None, vals.c.dtype, size=n)
    ctx = new_context(method=GDF_HASH)
    with pytest.raises(GDFError, match="GDF_JOIN_TOO_MANY_COLUMNS"):
        libgdf.gdf_group_by_sum(len(keys), column_array(keys), vals.ptr, None, column_array(out_keys), out_agg.ptr, C.byref(ctx))
    assert all(bool((k.data == 77).all()) for k in out_keys) and bool((out_agg.data == 77).all())
    with pytest.raises(GDFError, match="GDF_JOIN_TOO_MANY_COLUMNS"):
        gdf.api.order_by(keys)
    k16, a16 = gdf.api.group_by("sum", keys[:16], vals)                          # sixteen columns are fine
    assert len(a16) == len(np.unique(np.stack([(np.arange(n) % (3 + c)) for c in range(16)]), axis=1).T)
