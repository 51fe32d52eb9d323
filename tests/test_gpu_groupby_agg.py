"""-m gpu: gdf_amd_group_by_agg (csrc/groupby_agg.hip) through api.group_by_agg against tests/groupby_agg_reference.py -- data, mask
words, null counts, dtypes compared exactly; only a float SUM / AVG over general values gets a (derived) bound.

The reduce kernel gba_reduce folds tiles of T = GBA_TILE sorted positions (libgdf_amd/csrc/groupby_agg.hip), one position per lane, 64 per
wave: the sizes and segment layouts below sit on the wave and tile edges.  Inputs are built as run lengths in SORTED order and the rows
are then shuffled with a seeded permutation, so that the gather through the sort's permutation is a real one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import groupby_agg_reference as gar
import order_reference as orf

pytestmark = pytest.mark.gpu

T = 1024                       # GBA_TILE
N3 = 3 * T + 17
SIZES = [1, 2, 63, 64, 65, T - 1, T, T + 1, N3]
NP_OF_GDF = {1: np.int8, 2: np.int16, 3: np.int32, 4: np.int64, 5: np.float32, 6: np.float64, 7: np.int32, 8: np.int64, 9: np.int64}


def test_T_is_the_kernels_tile():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libgdf_amd", "csrc", "groupby_agg.hip")) as f:
        assert int(re.search(r"constexpr int GBA_TILE = (\d+);", f.read()).group(1)) == T


# ---- building inputs ---------------------------------------------------------------------------------------------------------------------
def keys_of_runs(runs, dtype=np.int32):
    """one ascending key per run, in sorted order"""
    return np.repeat(np.arange(len(runs)), runs).astype(dtype)


def shuffled(rng, n, *cols):
    """the same seeded row permutation applied to every (data, valid) column"""
    p = rng.permutation(n)
    return [(d[p], None if v is None else v[p]) for d, v in cols]


def int_values(rng, n, npt=np.int64, lo=-1000, hi=1000):
    return rng.integers(lo, hi, size=n).astype(npt)


def exact_floats(rng, n, npt):
    """integers of magnitude below 2^20: every double sum of them is exact in every association order"""
    return rng.integers(-(1 << 20) + 1, 1 << 20, size=n).astype(npt)


# ---- running and comparing -----------------------------------------------------------------------------------------------------------------
def run(gdf, keys, values, aggs, key_dtypes=None, value_dtypes=None, key_units=None, value_units=None):
    kc = [orf.device_column(d, v, key_dtypes and key_dtypes[i], key_units and key_units[i]) for i, (d, v) in enumerate(keys)]
    vc = [orf.device_column(d, v, value_dtypes and value_dtypes[i], value_units and value_units[i]) for i, (d, v) in enumerate(values)]
    return gdf.api.group_by_agg(kc, vc, aggs)


def compare_common(o, want, G, what):
    assert o.size == G, (what, o.size, G)
    assert int(o.c.dtype) == want.dtype, (what, int(o.c.dtype), want.dtype)
    got_mask = o.valid.cpu().numpy()
    assert len(got_mask) == (G + 63) // 64 * 8, what
    np.testing.assert_array_equal(got_mask, want.mask, err_msg=f"{what}: mask")                   # the bits beyond G are zero
    assert int(o.c.null_count) == want.null_count, (what, int(o.c.null_count), want.null_count)
    got = o.data.cpu().numpy()
    assert got.dtype == NP_OF_GDF[want.dtype], what
    assert not orf.bits_of(got)[~want.ok].any(), f"{what}: a null element has data 0"
    return got


def check(gdf, keys, values, aggs, float_sums="exact", what="", **kw):
    """float_sums: 'exact' -- SUM / AVG of floats compared with == -- or 'bound': |got - fsum| <= (n_g - 1) * 2^-52 * sum|x| per group,
    twice the first-order bound of ANY summation order; AVG the same divided by the count, plus one ulp for the division"""
    outs_k, outs_a = run(gdf, keys, values, aggs, **kw)
    want_k, want_a = gar.group_by_agg(keys, values, aggs, kw.get("key_dtypes"), kw.get("value_dtypes"))
    G = len(want_k[0].data)
    assert len(outs_k) == len(keys) and len(outs_a) == len(aggs)
    for c, (o, w) in enumerate(zip(outs_k, want_k)):
        got = compare_common(o, w, G, f"{what} key {c}")
        np.testing.assert_array_equal(orf.bits_of(got), orf.bits_of(w.data), err_msg=f"{what}: key {c}")       # the FIRST row's bits
    for a, (o, w, (col, op)) in enumerate(zip(outs_a, want_a, aggs)):
        label = f"{what} request {a} = {op}({col})"
        got = compare_common(o, w, G, label)
        if got.dtype.kind != "f":
            np.testing.assert_array_equal(got, w.data, err_msg=label)
        elif op in ("min", "max"):                                                                # either zero, any NaN
            np.testing.assert_array_equal(orf.value_image(got)[0][w.ok], orf.value_image(w.data)[0][w.ok], err_msg=label)
        elif float_sums == "exact" or w.sum_abs is None:
            np.testing.assert_array_equal(got, w.data, err_msg=label)
        else:
            bound = np.maximum(w.count - 1, 0) * 2.0 ** -52 * w.sum_abs
            if op == "avg":
                bound = bound / np.maximum(w.count, 1) + np.spacing(np.abs(w.data))
            err = np.abs(got - w.data)
            assert (err <= bound).all(), (label, float(err.max()), int(np.argmax(err - bound)))
    return outs_k, outs_a


MIXED_AGGS = [(0, "sum"), (0, "avg"), (1, "min"), (1, "max"), (2, "count"), (None, "count"), (2, "sum"), (0, "min")]


def mixed_values(rng, n):
    """an int64 column with 50 % nulls, a float64 one without a mask, an int8 one with 10 % nulls"""
    return [(int_values(rng, n), rng.random(n) < 0.5), (exact_floats(rng, n, np.float64), None),
            (int_values(rng, n, np.int8, -128, 128), rng.random(n) < 0.9)]


def check_runs(gdf, runs, seed, what):
    rng = np.random.default_rng(seed)
    n = int(np.sum(runs))
    cols = shuffled(rng, n, (keys_of_runs(runs), None), *mixed_values(rng, n))
    return check(gdf, cols[:1], cols[1:], MIXED_AGGS, what=what)


# ---- sizes and segment layouts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_one_group(gdf, n):
    check_runs(gdf, [n], n, f"one group of {n}")


@pytest.mark.parametrize("n", SIZES)
def test_all_distinct(gdf, n):
    check_runs(gdf, [1] * n, n + 1, f"{n} groups of one")


def _layouts():
    yield "one group over everything", [N3]
    yield "every row its own group", [1] * N3
    yield "groups of 64 on the waves", [64] * (N3 // 64) + [N3 % 64]
    yield "groups of 64 shifted by one", [1] + [64] * ((N3 - 1) // 64) + [(N3 - 1) % 64]
    yield "two rows on T-1, T", [T - 1, 2, N3 - T - 1]
    yield "from the last position of a tile through two more", [T - 1, 2 * T + 1, 17]
    yield "1 and 129 alternating", ([1, 129] * (N3 // 130 + 1))[:2 * (N3 // 130)] + [N3 % 130]
    yield "one row, then all the rest", [1, N3 - 1]
    yield "tile-sized groups", [T, T, T, 17]
    yield "ends on a tile edge behind a tile without a head", [10, 2 * T - 10, T, 17]
    yield "a group over two tile edges between singles", [1] * (T - 3) + [T + 6] + [1] * (N3 - 2 * T - 3)


@pytest.mark.parametrize("layout", list(_layouts()), ids=lambda l: l[0])
def test_segment_layouts(gdf, layout):
    name, runs = layout
    runs = [r for r in runs if r > 0]
    assert sum(runs) == N3
    check_runs(gdf, runs, len(name), name)


def test_a_group_over_a_hundred_tiles(gdf):
    """2^17 rows: 5 short groups, one of 100 * T + 3 rows (its carry records are folded in tile order), then groups of 300"""
    n = 1 << 17
    rest = n - (5 * 7 + 100 * T + 3)
    runs = [7] * 5 + [100 * T + 3] + [300] * (rest // 300) + [rest % 300]
    rng = np.random.default_rng(17)
    cols = shuffled(rng, n, (keys_of_runs(runs), None), (int_values(rng, n), rng.random(n) < 0.5), (exact_floats(rng, n, np.float32), None))
    check(gdf, cols[:1], cols[1:], [(0, "sum"), (1, "sum"), (1, "avg"), (1, "min"), (0, "max"), (None, "count")], what="100 tiles")


@pytest.mark.parametrize("tiles", [64, 65, 66])
def test_a_group_that_ends_around_a_step_of_the_fix_up(gdf, tiles):
    """gba_fixup walks a group's carry records 64 tiles at a time: the group begins on position 5 and ends with the LAST position of
    tile `tiles` - 1, and the next tile begins with a head"""
    runs = [5, tiles * T - 5, 40]
    n = sum(runs)
    rng = np.random.default_rng(tiles)
    cols = shuffled(rng, n, (keys_of_runs(runs), None), (int_values(rng, n), rng.random(n) < 0.5), (exact_floats(rng, n, np.float64), None))
    check(gdf, cols[:1], cols[1:], [(0, "sum"), (1, "sum"), (1, "avg"), (1, "min"), (0, "max"), (0, "count")], what=f"{tiles} tiles")


# ---- ops x value dtypes --------------------------------------------------------------------------------------------------------------------
VALUE_DTYPES = [("int8", np.int8, 1), ("int16", np.int16, 2), ("int32", np.int32, 3), ("int64", np.int64, 4), ("float32", np.float32, 5),
                ("float64", np.float64, 6), ("date32", np.int32, 7), ("date64", np.int64, 8), ("timestamp", np.int64, 9)]
RUNS_MIX = [1, 5, 64, 70, 1, 1, 300, T + 3, 2, 129, 16, 16, 63, 65]


@pytest.mark.parametrize("nulls", [0.0, 0.5, 1.0], ids=["0%", "50%", "100%"])
@pytest.mark.parametrize("vt", VALUE_DTYPES, ids=lambda v: v[0])
def test_every_op_on_every_value_dtype(gdf, vt, nulls):
    """every op the dtype allows in one call; group 2 (and group 6, a single row) has no valid value unless there are no nulls at all"""
    name, npt, gdf_dtype = vt
    rng = np.random.default_rng(gdf_dtype * 10 + int(nulls * 2))
    n = sum(RUNS_MIX)
    k = keys_of_runs(RUNS_MIX)
    if np.dtype(npt).kind == "f":
        v = exact_floats(rng, n, npt)
    else:
        info = np.iinfo(npt)
        v = rng.integers(max(info.min, -(1 << 40)), min(info.max, 1 << 40), size=n, dtype=np.int64, endpoint=True).astype(npt)
    valid = None if nulls == 0.0 else rng.random(n) >= nulls
    if nulls == 0.5:
        valid[(k == 2) | (k == 6)] = False
    ops = ["min", "max", "count"] + (["sum", "avg"] if gdf_dtype <= 6 else [])
    kcol, vcol = shuffled(rng, n, (k, None), (v, valid))
    check(gdf, [kcol], [vcol], [(0, op) for op in ops], value_dtypes=[gdf_dtype], value_units=["ms" if gdf_dtype == 9 else None],
          what=f"{name} {nulls}")


def test_requests_that_share_a_column_and_repeat(gdf):
    """SUM / AVG in both orders, AVG alone on a column (divided in place), the same request twice, MIN twice"""
    rng = np.random.default_rng(5)
    n = sum(RUNS_MIX)
    cols = shuffled(rng, n, (keys_of_runs(RUNS_MIX), None), (int_values(rng, n), rng.random(n) < 0.5), (exact_floats(rng, n, np.float64), rng.random(n) < 0.8),
                    (exact_floats(rng, n, np.float32), None))
    aggs = [(0, "avg"), (0, "sum"), (0, "avg"), (0, "sum"), (1, "avg"), (1, "avg"), (2, "sum"), (2, "avg"), (1, "min"), (1, "min"), (1, "max"),
            (0, "count"), (0, "count"), (None, "count"), (None, "count")]
    check(gdf, cols[:1], cols[1:], aggs, what="shared")


def test_64_requests_over_64_value_columns(gdf):
    rng = np.random.default_rng(64)
    runs = [3, 64, 1, 200, T, 5]
    n = sum(runs)
    npts = [np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
    vals = []
    for c in range(64):
        npt = npts[c % 6]
        v = exact_floats(rng, n, npt) if np.dtype(npt).kind == "f" else int_values(rng, n, npt, -100, 100)
        vals.append((v, rng.random(n) < 0.7 if c % 3 else None))
    cols = shuffled(rng, n, (keys_of_runs(runs), None), *vals)
    ops = ["sum", "min", "max", "avg", "count"]
    check(gdf, cols[:1], cols[1:], [(c, ops[c % 5]) for c in range(64)], what="64 x 64")
    check(gdf, cols[:1], cols[1:3], [(c % 2, ops[c % 5]) for c in range(63)] + [(None, "count")], what="64 requests on two columns")


def test_count_star_alone_without_value_columns(gdf):
    rng = np.random.default_rng(8)
    runs = [5, 1, 70, T + 1]
    (kcol,) = shuffled(rng, sum(runs), (keys_of_runs(runs), None))
    _, (star,) = check(gdf, [kcol], [], [(None, "count")], what="COUNT(*)")
    assert star.data.cpu().tolist() == runs


# ---- keys ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys", [1, 2, 3, 16])
def test_key_column_counts(gdf, nkeys):
    """few distinct values per column, 20 % nulls in every second column: groups of every size, null groups among them"""
    rng = np.random.default_rng(nkeys)
    n = N3
    keys = []
    for c in range(nkeys):
        npt = [np.int32, np.int8, np.int64, np.float32, np.int16, np.float64][c % 6]
        keys.append((rng.integers(0, 3 if nkeys > 3 else 12, size=n).astype(npt), rng.random(n) < 0.8 if c % 2 else None))
    check(gdf, keys, mixed_values(rng, n), MIXED_AGGS, what=f"{nkeys} keys")


@pytest.mark.parametrize("kt", VALUE_DTYPES, ids=lambda v: v[0])
def test_every_key_dtype(gdf, kt):
    name, npt, gdf_dtype = kt
    rng = np.random.default_rng(100 + gdf_dtype)
    n = 2 * T + 5
    if np.dtype(npt).kind == "f":
        k = rng.integers(-20, 20, size=n).astype(npt) / npt(4)
    else:
        info = np.iinfo(npt)
        k = rng.choice(np.array([info.min, info.max, -1, 0, 1, 7, info.min + 1], dtype=npt), size=n)
    outs_k, _ = check(gdf, [(k, rng.random(n) < 0.9)], mixed_values(rng, n), MIXED_AGGS, key_dtypes=[gdf_dtype],
                      key_units=["us" if gdf_dtype == 9 else None], what=name)
    assert int(outs_k[0].c.dtype_info.time_unit) == (3 if gdf_dtype == 9 else 0)


def test_masked_full_range_int64_key(gdf):
    """65 image bits: gdf_amd_order_by_ex splits the unit over two column groups"""
    rng = np.random.default_rng(65)
    n = 2 * T + 100
    pool = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, size=300, dtype=np.int64, endpoint=True)
    pool[:2] = [np.iinfo(np.int64).min, np.iinfo(np.int64).max]
    k = rng.choice(pool, size=n)
    check(gdf, [(k, rng.random(n) < 0.7)], mixed_values(rng, n), MIXED_AGGS, what="int64 full range")


@pytest.mark.parametrize("npt", [np.float32, np.float64], ids=["float32", "float64"])
def test_float_keys_with_zeros_nans_and_infinities(gdf, npt):
    """-0.0 / +0.0 are one group and so are the two NaN payloads; the output key shows the bits of the group's first input row"""
    rng = np.random.default_rng(9)
    n = T + 77
    u = np.uint32 if npt == np.float32 else np.uint64
    nan_a, nan_b = (np.array([0x7FC00001, 0xFFC00123], dtype=u) if npt == np.float32 else
                    np.array([0x7FF8000000000001, 0xFFF8000000000123], dtype=u)).view(npt)
    pool = np.array([-0.0, 0.0, nan_a, nan_b, np.inf, -np.inf, 1.5, -1.5], dtype=npt)
    for first_zero, first_nan in ((0, 2), (1, 3)):
        k = pool[rng.integers(0, len(pool), size=n)]
        k[0], k[1] = pool[first_zero], pool[first_nan]                       # which zero and which payload come first in input order
        outs_k, outs_a = check(gdf, [(k, None)], mixed_values(rng, n), MIXED_AGGS, what=f"float keys {first_zero}")
        got = outs_k[0].data.cpu().numpy()
        assert len(got) == 6                                                 # -inf, -1.5, 0, 1.5, +inf, NaN
        assert orf.bits_of(got)[2] == orf.bits_of(pool[first_zero:first_zero + 1])[0]
        assert orf.bits_of(got)[5] == orf.bits_of(pool[first_nan:first_nan + 1])[0]


def test_constant_key_column(gdf):
    rng = np.random.default_rng(10)
    n = T + 5
    keys = [(np.full(n, 42, dtype=np.int64), None), (rng.integers(0, 4, size=n).astype(np.int8), None), (np.full(n, -1.0, dtype=np.float32), None)]
    check(gdf, keys, mixed_values(rng, n), MIXED_AGGS, what="constant keys")
    check(gdf, keys[:1], mixed_values(rng, n), MIXED_AGGS, what="one constant key")


@pytest.mark.parametrize("nulls", [0.01, 0.5, 1.0], ids=["1%", "50%", "100%"])
def test_null_keys(gdf, nulls):
    """the data under the null bits is random: it must not split the null group"""
    rng = np.random.default_rng(int(nulls * 100))
    n = 2 * T + 9
    valid = rng.random(n) >= nulls
    k = np.where(valid, rng.integers(0, 40, size=n), rng.integers(-(1 << 30), 1 << 30, size=n)).astype(np.int32)
    outs_k, _ = check(gdf, [(k, valid)], mixed_values(rng, n), MIXED_AGGS, what=f"null keys {nulls}")
    assert int(outs_k[0].c.null_count) == 1                                  # ONE null group, the last


def test_three_way_null_split(gdf):
    rng = np.random.default_rng(11)
    rows = [((0, False), (1, True)), ((0, False), (2, True)), ((1, True), (0, False)), ((1, True), (1, True)), ((0, False), (0, False))]
    pick = rng.integers(0, len(rows), size=T + 30)
    a = (np.array([rows[p][0][0] for p in pick], dtype=np.int32) + np.where([rows[p][0][1] for p in pick], 0, rng.integers(5, 99, size=len(pick))).astype(np.int32),
         np.array([rows[p][0][1] for p in pick]))
    b = (np.array([rows[p][1][0] for p in pick], dtype=np.int64) + np.where([rows[p][1][1] for p in pick], 0, rng.integers(5, 99, size=len(pick))),
         np.array([rows[p][1][1] for p in pick]))
    outs_k, (star,) = check(gdf, [a, b], [], [(None, "count")], what="three-way")
    # (1, 1) | (1, null) | (null, 1) | (null, 2) | (null, null)
    assert outs_k[0].valid_bits().tolist() == [True, True, False, False, False]
    assert outs_k[1].valid_bits().tolist() == [True, False, True, True, False]
    assert star.data.cpu().tolist() == [int((pick == i).sum()) for i in (3, 2, 0, 1, 4)]


# ---- values ----------------------------------------------------------------------------------------------------------------------------------
def test_exact_floats(gdf):
    """integers below 2^20: FLOAT32 groups of at most 16 rows and FLOAT64 groups of any length are exact in every association order"""
    rng = np.random.default_rng(12)
    runs32 = [int(r) for r in rng.integers(1, 17, size=400)]
    n = sum(runs32)
    cols = shuffled(rng, n, (keys_of_runs(runs32), None), (exact_floats(rng, n, np.float32), rng.random(n) < 0.8))
    check(gdf, cols[:1], cols[1:], [(0, "sum"), (0, "avg")], what="float32, groups <= 16")
    runs64 = [N3 - 500, 1, 499]
    cols = shuffled(rng, N3, (keys_of_runs(runs64), None), (exact_floats(rng, N3, np.float64), rng.random(N3) < 0.8))
    check(gdf, cols[:1], cols[1:], [(0, "sum"), (0, "avg")], what="float64, long groups")


def general_float_case():
    rng = np.random.default_rng(13)
    runs = [N3] + [int(r) for r in rng.integers(1, 40, size=300)]
    n = sum(runs)
    return shuffled(rng, n, (keys_of_runs(runs), None), (rng.standard_normal(n) * 1e3, None), (rng.standard_normal(n), rng.random(n) < 0.5))


def test_general_floats_within_the_derived_bound(gdf):
    cols = general_float_case()
    check(gdf, cols[:1], cols[1:], [(0, "sum"), (0, "avg"), (1, "sum"), (1, "avg")], float_sums="bound", what="normal floats")


def test_a_second_call_is_bit_identical(gdf):
    import torch
    cols = general_float_case()
    aggs = [(0, "sum"), (0, "avg"), (1, "sum"), (1, "avg"), (1, "min"), (0, "max"), (None, "count")]
    a, b = run(gdf, cols[:1], cols[1:], aggs), run(gdf, cols[:1], cols[1:], aggs)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert x.size == y.size and int(x.c.null_count) == int(y.c.null_count)
        assert torch.equal(x.data.view(torch.uint8), y.data.view(torch.uint8)) and torch.equal(x.valid, y.valid)


def test_int8_sums_widen_and_int64_sums_wrap(gdf):
    rng = np.random.default_rng(14)
    runs = [200, 3, T + 1]
    n = sum(runs)
    small = np.full(n, 127, dtype=np.int8)
    big = rng.integers((1 << 62) - 1000, 1 << 62, size=n).astype(np.int64)
    cols = shuffled(rng, n, (keys_of_runs(runs), None), (small, None), (big, None))
    _, (s8, a8, s64, a64) = check(gdf, cols[:1], cols[1:], [(0, "sum"), (0, "avg"), (1, "sum"), (1, "avg")], what="widen / wrap")
    assert s8.data.cpu().tolist() == [127 * r for r in runs]
    true_sum = sum(int(x) for x in big[:200])                                 # (group 0: rows 0 .. 199 before the shuffle)
    assert true_sum >= 1 << 63 and s64.data.cpu().tolist()[0] == gar._wrap64(true_sum)


def test_min_max_nan_rule_and_signed_zeros(gdf):
    nan = np.nan
    runs = [3, 2, 1, 4, 2]
    v = np.array([2.0, nan, -1.0,   nan, nan,   np.inf,   -0.0, 0.0, -0.0, 0.0,   -np.inf, nan], dtype=np.float64)
    for npt in (np.float32, np.float64):
        rng = np.random.default_rng(15)
        cols = shuffled(rng, len(v), (keys_of_runs(runs), None), (v.astype(npt), None))
        _, (mn, mx) = check(gdf, cols[:1], cols[1:], [(0, "min"), (0, "max")], what="NaN rule")
        mn, mx = mn.data.cpu().numpy(), mx.data.cpu().numpy()
        assert mn[0] == -1.0 and np.isnan(mx[0])                             # MAX is NaN if any valid value is
        assert np.isnan(mn[1]) and np.isnan(mx[1])                           # MIN only if all are
        assert mn[2] == np.inf and mx[2] == np.inf
        assert mn[3] == 0.0 and mx[3] == 0.0                                 # either zero
        assert mn[4] == -np.inf and np.isnan(mx[4])


def test_timestamp_min_keeps_the_time_unit(gdf):
    rng = np.random.default_rng(16)
    n = 500
    stamps = rng.integers(-(1 << 50), 1 << 50, size=n, dtype=np.int64)
    k = rng.integers(0, 9, size=n).astype(np.int32)
    _, (mn, mx, c) = check(gdf, [(k, None)], [(stamps, rng.random(n) < 0.6)], [(0, "min"), (0, "max"), (0, "count")], value_dtypes=[9],
                           value_units=["ns"], what="timestamp")
    assert [int(o.c.dtype) for o in (mn, mx, c)] == [9, 9, 4]
    assert [int(o.c.dtype_info.time_unit) for o in (mn, mx, c)] == [4, 4, 0]


# ---- against what exists, and what must not change ---------------------------------------------------------------------------------------------
def test_agrees_with_group_by_sum(gdf):
    """unmasked int32 keys and int64 values: gdf_group_by_sum with sorted results gives the same keys and sums"""
    from libgdf_amd.columns import column_from_numpy
    rng = np.random.default_rng(18)
    n = 50_000
    k = rng.integers(-500, 500, size=n).astype(np.int32)
    v = rng.integers(-(1 << 40), 1 << 40, size=n).astype(np.int64)
    old_k, old_s = gdf.api.group_by("sum", [column_from_numpy(k)], column_from_numpy(v), sort_result=True)
    (new_k,), (new_s,) = gdf.api.group_by_agg([column_from_numpy(k)], [column_from_numpy(v)], [(0, "sum")])
    assert new_k.size == old_k[0].numel() and int(new_k.c.null_count) == int(new_s.c.null_count) == 0
    np.testing.assert_array_equal(new_k.to_numpy(), old_k[0].cpu().numpy())
    np.testing.assert_array_equal(new_s.to_numpy(), old_s.cpu().numpy())


def test_inputs_are_untouched(gdf):
    import torch
    rng = np.random.default_rng(19)
    n = 2 * T + 1
    keys = [(rng.integers(0, 30, size=n).astype(np.int64), rng.random(n) < 0.8), (rng.integers(0, 3, size=n).astype(np.float32), None)]
    vals = mixed_values(rng, n)
    kc = [orf.device_column(d, v) for d, v in keys]
    vc = [orf.device_column(d, v) for d, v in vals]
    buffers = [t for c in kc + vc for t in (c.data, c.valid) if t is not None]
    before = [t.clone() for t in buffers]
    gdf.api.group_by_agg(kc, vc, MIXED_AGGS)
    for t, b in zip(buffers, before):
        assert torch.equal(t, b)


def test_raw_c_abi(gdf):
    """the entry point itself: library-allocated outputs, released with gdf_column_free; a failing call leaves the structs untouched"""
    from libgdf_amd import gdf_column
    from libgdf_amd._binding import gdf_amd_agg
    from libgdf_amd.columns import column_array
    rng = np.random.default_rng(20)
    runs = [3, T, 70]
    n = sum(runs)
    (kd, _), (vd, vv) = shuffled(rng, n, (keys_of_runs(runs, np.int64), None), (int_values(rng, n, np.int32), rng.random(n) < 0.5))
    kc, vc = [orf.device_column(kd)], [orf.device_column(vd, vv)]
    reqs = (gdf_amd_agg * 2)()
    (reqs[0].column, reqs[0].op), (reqs[1].column, reqs[1].op) = (0, 0), (-1, 4)
    outs = [gdf_column() for _ in range(3)]
    for o in outs:
        C.memset(C.byref(o), 0xAB, C.sizeof(o))
    ka = (C.POINTER(gdf_column) * 1)(C.pointer(outs[0]))
    aa = (C.POINTER(gdf_column) * 2)(C.pointer(outs[1]), C.pointer(outs[2]))
    fn = gdf.libgdf.raw("gdf_amd_group_by_agg")
    before = [bytes(C.string_at(C.addressof(o), C.sizeof(o))) for o in outs]
    reqs[1].op = 5                                                            # GDF_COUNT_DISTINCT
    assert fn(column_array(kc), 1, column_array(vc), 1, reqs, 2, ka, aa) == 12
    assert [bytes(C.string_at(C.addressof(o), C.sizeof(o))) for o in outs] == before
    reqs[1].op = 4
    assert fn(column_array(kc), 1, column_array(vc), 1, reqs, 2, ka, aa) == 0
    _, want = gar.group_by_agg([(kd, None)], [(vd, vv)], [(0, "sum"), (None, "count")])
    assert [(int(o.size), int(o.dtype)) for o in outs] == [(3, 4)] * 3
    assert [int(o.null_count) for o in outs] == [0, want[0].null_count, 0]
    assert all(o.data and o.valid for o in outs)
    taken = [gdf.api._take_masked_column(o) for o in outs]                    # (copies, then gdf_column_free)
    assert taken[0].to_numpy().tolist() == [0, 1, 2]
    np.testing.assert_array_equal(taken[1].to_numpy(), want[0].data)
    assert taken[2].to_numpy().tolist() == runs
    for t, w in zip(taken[1:], want):
        np.testing.assert_array_equal(t.valid.cpu().numpy(), w.mask)
