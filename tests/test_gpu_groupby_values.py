"""-m gpu: the VALUE domain of gdf_group_by_* (HASH) on every aggregation path of csrc/groupby.hip.

The path tests of test_gpu_groupby.py feed every path values from [-1000, 1000] or U[0, 1).  Here the whole recipe table of
tests/groupby_values.py -- type extremes (for int64 the accumulators' identity images), sums that wrap, counts that wrap the AVG /
COUNT type, float grids at 2^0, 2^100 / 2^900 and on the denormals, infinities, NaN, finfo.max / tiny -- goes through every path
in ONE call per (path, op, value dtype): recipe g sits on key number g of a key layout that reaches the path, filler groups bring
the row and group counts the path needs.  Every comparison is exact (np.testing.assert_array_equal against the CPU oracle, NaN equal
to NaN); the one exception is MIN / MAX of a group mixing NaN with numbers, which the reference leaves to the row order: there the
answer must be NaN or the min / max of the numbers.  Every test asserts the path it meant from the kernel names of the profile hook.

Reference semantics: aggregation_operations.cuh:30-86, groupby.cuh:102-109, 308-328; masks as in DESIGN.md section 4."""
import functools

import numpy as np
import pytest

import groupby_values as gv
from oracle import oracle
from util import sort_groups

pytestmark = pytest.mark.gpu
IDS = lambda d: np.dtype(d).name
EIGHT_BYTE = [np.int64, np.float64]
# the three layouts of >= 2^22 rows: int16 and int32 share the loader switch with int8 there (acc_image / the FASTVAL == 4 branch is
# reached by float32), so they run int8, int64, float32, float64
BIG_DTYPES = [np.int8, np.int64, np.float32, np.float64]
MIXED_NAN = ("nan_pos_mixed", "nan_neg_mixed")


def _out(op, dt):
    """COUNT in int64; AVG in the value dtype (integer AVG: the count wraps in that type); the typing matrices vary it"""
    return np.int64 if op == "count" else (dt if op == "avg" else None)


def _table_for(op, dt, out):
    recs = [r for r in gv.recipes(dt, op) if op != "avg" or gv.avg_defined(r.values, dt, out)]
    if op in ("min", "max") and np.dtype(dt).kind == "f":
        recs = recs + [r for r in gv.recipes(dt) if r.name in MIXED_NAN]           # membership check only
    return recs


@functools.lru_cache(maxsize=2)
def _case(shape, op, dtname, outname):
    """(layout, oracle keys, oracle aggregate) of one (key layout, op, value dtype, output dtype): computed once, shared by the
    variants of a path that run on the same table"""
    dt = np.dtype(dtname).type
    out = None if outname is None else np.dtype(outname).type
    lay = gv.layout(shape, _table_for(op, dt, out), np.random.default_rng(7))
    ek, ea = oracle.group_by(op, lay.keys, lay.vals, out)
    return lay, ek, ea


def _run(gdf, op, lay, out):
    from libgdf_amd.columns import column_from_numpy, get_dtype
    od = None if out is None else get_dtype(out)
    k, a = gdf.api.group_by(op, [column_from_numpy(c) for c in lay.keys], column_from_numpy(lay.vals), out_dtype=od)
    return sort_groups([x.cpu().numpy() for x in k], a.cpu().numpy())


def _check_path(gdf, force_path, path, op, dt, out="default", shape=None):
    """the recipe table of (op, dt) through `path`: exact against the oracle, the path asserted from the kernel names"""
    out = _out(op, dt) if out == "default" else out
    p = gv.PATHS[path]
    lay, ek, ea = _case(shape or path, op, np.dtype(dt).name, None if out is None else np.dtype(out).name)
    for name, value in p["force"].items():
        force_path(name, value)
    got = {}
    try:
        names = gv.kernels_of(gdf, lambda: got.update(r=_run(gdf, op, lay, out)))
    finally:
        for name in p["force"]:
            force_path(name, None)
    gk, ga = got["r"]
    assert p["kernel"] in names and not (set(p["absent"]) & names), (path, sorted(names))
    want_dtype = np.dtype(out if op in ("count", "avg") else dt)
    assert ga.dtype == ea.dtype == want_dtype
    np.testing.assert_array_equal(gk[0], ek[0])
    mixed = np.zeros(len(ea), dtype=bool)
    for r, key in zip(lay.recipes, lay.key_of_recipe):
        if r.name in MIXED_NAN and op in ("min", "max"):
            i = int(np.searchsorted(ek[0], key))
            mixed[i] = True
            nums = r.values[~np.isnan(r.values)]
            assert np.isnan(ga[i]) or ga[i] == (nums.min() if op == "min" else nums.max()), (r.name, ga[i])
    np.testing.assert_array_equal(ga[~mixed], ea[~mixed], err_msg=f"{path} {op} {np.dtype(dt).name}: recipes " + ", ".join(
        r.name for r, key in zip(lay.recipes, lay.key_of_recipe) if not _same(ga, ea, int(np.searchsorted(ek[0], key)))))


def _same(ga, ea, i):
    return ga[i] == ea[i] or (ga[i] != ga[i] and ea[i] != ea[i])


# ---- B: every recipe on every path ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", gv.VALUE_DTYPES, ids=IDS)
@pytest.mark.parametrize("path", ["direct", "dense"])
def test_small_key_range(gdf, force_path, path, op, dt):
    """direct index (gb_direct_aggregate: FASTVAL 8 / 4 / acc_image) and, with GDF_GB_NO_DIRECT, the dense dictionary
    (gb_dense_aggregate) on the same table"""
    _check_path(gdf, force_path, path, op, dt, shape="direct")


@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", BIG_DTYPES, ids=IDS)
def test_lds_dictionary(gdf, force_path, op, dt):
    """2^22 + 77 rows, sparse int64 keys, 3000 filler groups: gb_ld_encode / gb_ld_aggregate; GDF_GB_NO_LDS_DICT: the L2 dictionary and
    gb_dense_aggregate with its FASTVAL branch"""
    _check_path(gdf, force_path, "lds_dict", op, dt, shape="lds_dict")
    _check_path(gdf, force_path, "lds_dict_off", op, dt, shape="lds_dict")


@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", gv.VALUE_DTYPES, ids=IDS)
def test_fused_partition_pass(gdf, force_path, op, dt):
    """2^20 + 4321 rows, one int64 key column, a million single-row filler groups: the fused partition pass.  8-byte values take the
    statically typed scatter kernels (gbp_scatter_static) and, with GDF_GBP_DYNAMIC, the kernels with the type switch (gbp_scatter),
    which 1- / 2- / 4-byte values and COUNT take anyway"""
    _check_path(gdf, force_path, "part_fused", op, dt, shape="part_fused")
    if np.dtype(dt).itemsize == 8 and op != "count":
        _check_path(gdf, force_path, "part_dynamic", op, dt, shape="part_fused")


@pytest.mark.parametrize("op", ["sum", "min", "max", "avg"])
@pytest.mark.parametrize("dt", EIGHT_BYTE, ids=IDS)
def test_hot_window(gdf, force_path, op, dt):
    """2^22 + 77 rows, half of them on keys below 4096: the scatter kernel aggregates that window in LDS (gbp_scatter_hot; only the
    statically typed kernels have it: 8-byte values, no COUNT).  The recipes sit on keys 0 .. R-1, INSIDE the window the sample picks;
    with the window forced elsewhere (GDF_GBP_HOT_WINDOW=3) the same recipes travel as cold records"""
    _check_path(gdf, force_path, "hot_inside", op, dt, shape="hot_inside")
    _check_path(gdf, force_path, "hot_outside", op, dt, shape="hot_inside")


@pytest.mark.parametrize("op", ["sum", "min", "max", "avg"])
@pytest.mark.parametrize("dt", EIGHT_BYTE, ids=IDS)
def test_speculative_layout(gdf, force_path, op, dt):
    """GDF_GBP_SPEC_MIN_ROWS=1 at 2^20 rows -- the floor of the fused pass the layout lives in, so the smallest table that takes it:
    gbp_sample_hist and no gbp_count; with GDF_GBP_NO_SPEC the count pass is back"""
    _check_path(gdf, force_path, "spec", op, dt, shape="spec")
    _check_path(gdf, force_path, "spec_off", op, dt, shape="spec")


@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", gv.VALUE_DTYPES, ids=IDS)
def test_many_groups_below_2p20_rows(gdf, force_path, op, dt):
    """3e5 rows, more groups than LDS accumulators hold: pair build + radix sort of the high key bits + gb_part_aggregate; the whole
    key sorted (GDF_GB_NO_PART: gb_sorted_reduce); the global table on packed keys (GDF_GB_NO_SORTED: gb_aggregate_packed)"""
    for path in ("part_small", "sorted", "table"):
        _check_path(gdf, force_path, path, op, dt, shape="part_small")


@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", gv.VALUE_DTYPES, ids=IDS)
def test_first_row_table(gdf, force_path, op, dt):
    """a float64 key column kept off its integer image (GDF_GB_NO_FLOAT_IMAGE): the row-comparing table, gb_aggregate_rows"""
    _check_path(gdf, force_path, "first_row", op, dt)


# ---- C: typing matrices ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out", gv.VALUE_DTYPES, ids=IDS)
@pytest.mark.parametrize("dt", gv.VALUE_DTYPES, ids=IDS)
@pytest.mark.parametrize("path", ["direct", "part_small"])
def test_avg_typing_matrix(gdf, force_path, path, dt, out):
    """all 36 (sum type, avg type) pairs of store_avg over the recipe table (without the triples C++ leaves undefined:
    groupby_values.avg_defined), on the direct path and on the partitioned one"""
    _check_path(gdf, force_path, path, "avg", dt, out=out)


@pytest.mark.parametrize("out", gv.VALUE_DTYPES, ids=IDS)
@pytest.mark.parametrize("path", ["direct", "part_small"])
def test_count_typing(gdf, force_path, path, out):
    """COUNT in all six output dtypes over groups of 1 .. 65536 rows (int8 wraps from 128, int16 from 32768; float32 stays far below
    2^24 rows per group, where the oracle's += 1.0f is exact)"""
    _check_path(gdf, force_path, path, "count", np.int32, out=out)


# ---- D: masks with poison under the nulls ----------------------------------------------------------------------------------------------
MASKED_PATHS = {
    # a request with a mask never takes the direct path or the LDS dictionary: the small key range lands on the dense dictionary
    "dense": dict(shape="dense", kernel="gb_dense_aggregate", force={}),
    "part_fused": dict(shape="part_fused", kernel="gbp_scatter", force={}),
    "part_dynamic": dict(shape="part_fused", kernel="gbp_scatter", force={"GDF_GBP_DYNAMIC": "1"}),
    "hot_inside": dict(shape="hot_inside", kernel="gbp_scatter_hot", force={}),
    "sorted": dict(shape="part_small", kernel="gb_sorted_reduce", force={"GDF_GB_NO_PART": "1"}),
    "table": dict(shape="part_small", kernel="gb_aggregate_packed", force={"GDF_GB_NO_SORTED": "1"}),
    # a float64 key column on its integer image: whichever packed path the image's range selects (kernel None: only the EQUALITY of the
    # kernel names with in-range and with NaN / far-away words under the null keys is asserted -- a NaN there must not cost the image)
    "float_keys": dict(shape="first_row", kernel=None, force={}),
}


def _poison(dt):
    dt = np.dtype(dt)
    if dt.kind == "i":
        return np.array([np.iinfo(dt).min, np.iinfo(dt).max, -1], dtype=dt)
    fi = np.finfo(dt)
    return np.array([np.nan, np.inf, -np.inf, fi.max, -fi.max, -np.nan], dtype=dt)


def _check_masked_path(gdf, force_path, path, op, dt):
    m = MASKED_PATHS[path]
    out = _out(op, dt)
    recs = [r for r in gv.masked_recipes(dt, op) if op != "avg" or r.nulls.all() or gv.avg_defined(r.values[~r.nulls], dt, out)]
    rng = np.random.default_rng(9)
    lay = gv.layout(m["shape"], recs, rng, filler_groups=40_000 if gv.PATHS[m["shape"]]["rows"] > 100_000 else None)
    n = len(lay.vals)
    v_ok = lay.val_valid & ~(lay.is_filler & (rng.random(n) < 0.3))          # a third of the filler is null as well
    zeros, poison = lay.vals.copy(), lay.vals.copy()
    zeros[~v_ok] = 0
    poison[~v_ok] = _poison(dt)[np.arange(int((~v_ok).sum())) % len(_poison(dt))]      # every poison under the nulls of every larger group
    k_ok = rng.random(n) > 0.03
    k_in, k_far = lay.keys[0].copy(), lay.keys[0].copy()
    k_in[~k_ok] = lay.keys[0][0]
    far = np.array([np.nan, 1e300, -1e300]) if k_far.dtype.kind == "f" else np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, 1 << 40], dtype=np.int64)
    k_far[~k_ok] = far[np.arange(int((~k_ok).sum())) % 3]
    for name, value in m["force"].items():
        force_path(name, value)
    res = {}
    # null VALUES: zeros under the nulls against the oracle, every poison under them against that answer
    names_z = gv.kernels_of(gdf, lambda: res.update(z=gv.check_masked(gdf, op, lay.keys, zeros, [None], v_ok, out, exact=True)))
    names_p = gv.kernels_of(gdf, lambda: res.update(p=gv.run_masked(gdf, op, lay.keys, poison, [None], v_ok, out)))
    # null KEYS: in-range words under them against the oracle, far-away words against that answer -- same plan, same path, same result
    names_i = gv.kernels_of(gdf, lambda: res.update(i=gv.check_masked(gdf, op, [k_in], poison, [k_ok], v_ok, out, exact=True)))
    names_f = gv.kernels_of(gdf, lambda: res.update(f=gv.run_masked(gdf, op, [k_far], poison, [k_ok], v_ok, out)))
    for name in m["force"]:
        force_path(name, None)
    assert (m["kernel"] is None or m["kernel"] in names_z) and names_z == names_p and names_z, (sorted(names_z), sorted(names_p))
    assert (m["kernel"] is None or m["kernel"] in names_i) and names_i == names_f and names_i, (sorted(names_i), sorted(names_f))
    if m["kernel"] is None:
        assert "gb_aggregate_rows" not in names_i, sorted(names_i)                   # the image was kept: no row-comparing table
    for a, b in (("z", "p"), ("i", "f")):
        (ak, aa, aok), (bk, ba, bok) = res[a], res[b]
        np.testing.assert_array_equal(ak[0], bk[0])
        np.testing.assert_array_equal(aok, bok)
        np.testing.assert_array_equal(aa, ba)
    # the groups whose every valid value is the type's extreme come out valid with it; the groups without a valid value come out null with 0
    gk, ga, gok = res["p"]
    by = {r.name: int(np.searchsorted(gk[0], key)) for r, key in zip(recs, lay.key_of_recipe)}
    if op in ("min", "max"):
        for name in ("all_max_some_null", "all_min_some_null"):
            r = recs[[x.name for x in recs].index(name)]
            assert gok[by[name]] and ga[by[name]] == r.values[0], (name, ga[by[name]])
    if op != "count":
        for name in ("all_null_a", "all_null_b"):
            assert not gok[by[name]] and ga[by[name]] == 0, (name, ga[by[name]])


@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", gv.VALUE_DTYPES, ids=IDS)
@pytest.mark.parametrize("path", ["dense", "sorted", "table"])
def test_masks_with_poison_under_the_nulls(gdf, force_path, path, op, dt):
    _check_masked_path(gdf, force_path, path, op, dt)


@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", [np.int8, np.int64, np.float32, np.float64], ids=IDS)
@pytest.mark.parametrize("path", ["part_fused", "part_dynamic"])
def test_masks_with_poison_fused_partition_pass(gdf, force_path, path, op, dt):
    """(the statically typed kernels take 8-byte values only; int16 / int32 share the type switch's loader with int8)"""
    _check_masked_path(gdf, force_path, path, op, dt)


@pytest.mark.parametrize("op", ["sum", "min", "max", "avg"])
@pytest.mark.parametrize("dt", EIGHT_BYTE, ids=IDS)
def test_masks_with_poison_hot_window(gdf, force_path, op, dt):
    _check_masked_path(gdf, force_path, "hot_inside", op, dt)


@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", EIGHT_BYTE, ids=IDS)
def test_masks_with_poison_float_keys(gdf, force_path, op, dt):
    """a float64 key column: NaN and +-1e300 as the key words under null keys change neither the kernels nor the answer"""
    _check_masked_path(gdf, force_path, "float_keys", op, dt)
