"""No GPU: the recipe table of tests/groupby_values.py and its independent reference.

  * the CPU oracle (group_by, group_by_masked, group_by_sort) equals reference() on every recipe, for every op and every (value
    dtype, output dtype) pair the GPU value tests use -- two statements of the same arithmetic, written apart;
  * every float grid is exact: its sum in the value dtype is the same bits forward, backward and shuffled;
  * layout() keeps its promises: every recipe is there once, under its own key, and no filler row shares a key with a recipe."""
import numpy as np
import pytest

import groupby_values as gv
from oracle import oracle

IDS = lambda d: np.dtype(d).name


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    np.testing.assert_array_equal(got, want, err_msg=str(what))          # NaN equals NaN, -0.0 equals 0.0


def _pairs(op, dt):
    """the (op, output dtype) combinations of the GPU tests, HASH method"""
    if op == "count":
        return gv.VALUE_DTYPES
    if op == "avg":
        return gv.VALUE_DTYPES
    return [None]


@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", gv.VALUE_DTYPES, ids=IDS)
def test_oracle_equals_reference(op, dt):
    for out in _pairs(op, dt):
        recs = [r for r in gv.recipes(dt, op) if op != "avg" or gv.avg_defined(r.values, dt, out)]
        lay = gv.layout("direct", recs, np.random.default_rng(1))
        ek, ea = oracle.group_by(op, lay.keys, lay.vals, out)
        pos = np.searchsorted(ek[0], lay.key_of_recipe)
        np.testing.assert_array_equal(ek[0][pos], lay.key_of_recipe)
        want = np.array([gv.reference(op, r, dt, out) for r in recs])
        _same(ea[pos], want, (op, np.dtype(dt).name, out, [r.name for r in recs]))


@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", gv.VALUE_DTYPES, ids=IDS)
def test_masked_oracle_equals_reference(op, dt):
    out = np.int64 if op == "count" else None
    recs = [r for r in gv.masked_recipes(dt, op) if op != "avg" or r.nulls.all() or gv.avg_defined(r.values[~r.nulls], dt, dt)]
    lay = gv.layout("dense", recs, np.random.default_rng(2))
    ek, ea, eok = oracle.group_by_masked(op, lay.keys, lay.vals, [None], lay.val_valid, out)
    pos = np.searchsorted(ek[0], lay.key_of_recipe)
    for r, i in zip(recs, pos):
        want = gv.reference(op, r, dt, out)
        assert bool(eok[i]) == (want is not None), r.name
        if want is None:
            assert ea[i] == 0, r.name
        else:
            _same(ea[i], want, (op, r.name))
    named = {r.name: i for r, i in zip(recs, pos)}
    if op in ("min", "max", "sum"):
        hi, lo = recs[named_index(recs, "all_max_some_null")].values[0], recs[named_index(recs, "all_min_some_null")].values[0]
        if op != "sum":
            assert ea[named["all_max_some_null"]] == hi and eok[named["all_max_some_null"]]
            assert ea[named["all_min_some_null"]] == lo and eok[named["all_min_some_null"]]
        assert ea[named["all_null_a"]] == 0 and not eok[named["all_null_a"]]
        assert ea[named["all_null_b"]] == 0 and not eok[named["all_null_b"]]


def named_index(recs, name):
    return [r.name for r in recs].index(name)


@pytest.mark.parametrize("op", gv.OPS)
@pytest.mark.parametrize("dt", gv.VALUE_DTYPES, ids=IDS)
def test_sort_oracle_equals_reference(op, dt):
    """the SORT method: SUM / MIN / MAX / AVG in the input dtype, COUNT in every output dtype, every group's LAST row as its index"""
    for out in (gv.VALUE_DTYPES if op == "count" else [None]):
        recs = [r for r in gv.recipes(dt, op) if op != "avg" or gv.avg_defined(r.values, dt, dt)]
        lay = gv.layout("direct", recs, np.random.default_rng(3))
        ek, ea, idx = oracle.group_by_sort(op, lay.keys, lay.vals, out)
        pos = np.searchsorted(ek[0], lay.key_of_recipe)
        want = np.array([gv.reference(op, r, dt, dt if out is None else out) for r in recs])
        _same(ea[pos], want, (op, np.dtype(dt).name, out))
        last = np.array([np.flatnonzero(lay.keys[0] == k)[-1] for k in lay.key_of_recipe])
        np.testing.assert_array_equal(idx[pos], last)


@pytest.mark.parametrize("dt", gv.FLT_DTYPES, ids=IDS)
def test_float_grids_are_exact(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(4)
    seen = 0
    for r in gv.recipes(dt, "sum"):
        v = r.values
        if not np.isfinite(v).all():
            continue
        with np.errstate(over="ignore"):
            sums = [np.cumsum(o, dtype=dt)[-1] + dt.type(0) for o in (v, v[::-1], v[rng.permutation(len(v))], np.sort(v))]
        bits = {s.tobytes() for s in sums}
        assert len(bits) == 1, (r.name, sums)
        _same(sums[0], gv.reference("sum", r, dt), r.name)
        seen += 1
    assert seen >= 15
    # the grids reach what they are meant to reach: denormal sums, sums beyond 2^100 / 2^900
    by = {r.name: r for r in gv.recipes(dt)}
    assert 0 < abs(float(gv.reference("max", by["grid_denormal"], dt))) < float(np.finfo(dt).tiny)
    assert abs(float(gv.reference("min", by["grid_big_negatives"], dt))) >= 2.0 ** gv.GRID_EXP[dt][1]
    for r in gv.recipes(dt):
        assert len(r.values) <= gv.GRID_ROWS[dt]


@pytest.mark.parametrize("dt", gv.INT_DTYPES, ids=IDS)
def test_integer_recipes_reach_the_wraps(dt):
    by = {r.name: r for r in gv.recipes(dt)}
    info = np.iinfo(dt)
    assert gv.reference("sum", by["wraps_to_zero"], dt) == 0 and gv.reference("sum", by["2_x_min"], dt) == 0
    assert gv.reference("sum", by["2_x_max"], dt) == -2 and gv.reference("sum", by["257_x_max"], dt) == gv._wrap(257 * int(info.max), dt)
    assert gv.reference("count", by["ones_128"], dt, np.int8) == -128 and gv.reference("count", by["ones_256"], dt, np.int8) == 0
    assert gv.reference("count", by["ones_32768"], dt, np.int16) == -32768 and gv.reference("count", by["ones_65536"], dt, np.int16) == 0
    assert gv.reference("avg", by["minus7_over_2"], dt, dt) == -3 and gv.reference("avg", by["minus7_over_3"], dt, np.int64) == -2
    assert gv.reference("avg", by["ones_256"], dt, np.int8) == 0                       # wrapped count 0 stores 0
    assert gv.reference("avg", by["ones_128"], dt, np.int8) == (1 if dt == np.int8 else -1)   # int8 sums: -128 / -128; wider: 128 / -128
    assert gv.reference("avg", by["ones_255"], dt, np.int8) == (1 if dt == np.int8 else -255 + 256)   # -1 / -1; 255 / -1 = -255 -> int8 1
    for out in gv.INT_DTYPES:                                                           # no pair that traps on the host
        for r in gv.recipes(dt, "avg"):
            assert gv.avg_defined(r.values, dt, out), (r.name, out)


@pytest.mark.parametrize("path", ["direct", "dense", "part_small", "first_row", "part_fused", "lds_dict", "hot_inside"])
def test_layout_keeps_its_promises(path):
    recs = gv.masked_recipes(np.int16) if path == "dense" else gv.recipes(np.float32 if path == "first_row" else np.int64)
    lay = gv.layout(path, recs, np.random.default_rng(5))
    k = lay.keys[0]
    assert len(k) == len(lay.vals) >= gv.PATHS[path]["rows"]
    assert len(np.unique(lay.key_of_recipe)) == len(recs)
    assert not np.isin(lay.filler_keys, lay.key_of_recipe).any()
    order = np.argsort(k, kind="stable")
    ks, vs = k[order], lay.vals[order]
    lo, hi = np.searchsorted(ks, lay.key_of_recipe, "left"), np.searchsorted(ks, lay.key_of_recipe, "right")
    for r, a, b in zip(recs, lo, hi):
        got = vs[a:b]
        assert len(got) == len(r.values), r.name
        np.testing.assert_array_equal(np.sort(got.view(f"u{got.dtype.itemsize}")), np.sort(r.values.view(f"u{got.dtype.itemsize}")), err_msg=r.name)
        if r.nulls is not None:
            assert int((~lay.val_valid[order][a:b]).sum()) == int(r.nulls.sum()), r.name
    assert int(hi.sum() - lo.sum()) + int(np.isin(k, lay.filler_keys).sum()) == len(k)
    filler = lay.vals[np.isin(k, lay.filler_keys)]
    assert np.abs(filler.astype(np.float64)).max() <= 2
    if gv.PATHS[path]["filler"] == "single":
        assert len(lay.filler_keys) == len(filler)                 # one row per filler group
    # the same seed gives the same table
    again = gv.layout(path, recs, np.random.default_rng(5))
    np.testing.assert_array_equal(again.keys[0], k)
