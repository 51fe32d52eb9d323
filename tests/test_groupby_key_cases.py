"""No GPU: the key tables of tests/groupby_keys.py, their independent reference and the model of the two planning rules.

  * every case's recorded budget is what the plan model computes from the generated data, under the group-by rule and the sort rule;
  * the reference agrees with the CPU oracle (group_by, group_by_sort, order_by) on every case at a reduced row count;
  * the un-mutated model of pack / unpack reproduces the reference wherever the rule packs, and NO mutation of it survives the
    table: for each of groupby_keys.MUTATIONS at least one case gives another grouping or order than the reference.  That is the
    evidence that the table would catch these errors in a kernel; no wrong kernel is ever run.

Excluded by name, because the reference semantics leave it open (groupby_keys' docstring):
  * the NaN tables against oracle.group_by / group_by_sort: where the single-row NaN groups stand among the groups is
    unspecified, so they are compared as matched tables (groupby_keys.match_order), not position by position;
  * which of -0.0 / +0.0 names a group: == on both sides."""
import functools

import numpy as np
import pytest

import groupby_keys as gk
from oracle import oracle

ROWS = 6000
NAMES = [c.name for c in gk.CASES]


@functools.lru_cache(maxsize=None)
def _lay(name, regime="many", rows=ROWS):
    return gk.layout(gk.CASE[name], regime, rows, np.random.default_rng(11))


@functools.lru_cache(maxsize=None)
def _ref(name):
    lay = _lay(name)
    return gk.reference(lay.keys, lay.vals)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("regime", ["few", "many"])
def test_recorded_budgets(name, regime):
    case = gk.CASE[name]
    lay = _lay(name, regime, 4000)
    p = gk.gb_plan(lay.keys)
    assert p.total == case.gb_bits, (name, p.bits)
    if case.gb_bits is not None:
        assert p.packed == (case.gb_bits <= 63)
    assert case.natural == (all(k.dtype.kind == "i" for k in lay.keys) and sum(k.dtype.itemsize for k in lay.keys) <= 8)
    width, groups = gk.sort_plan(lay.keys)
    assert tuple(sum(width[c] for c in g) for g in groups) == case.sort_bits, (name, width, groups)
    assert all(len(g) <= 8 for g in groups) and len(lay.keys) <= gk.MAX_KEY_COLS


def test_the_table_sits_on_the_budgets():
    """the totals the library branches on are all there (groupby.hip: GB_PART_ID_BITS 13, GBP_MAX_PART_BITS 11, GB_PART_MAX_BITS 13,
    the 32-bit record, 63 / 64; GB_DIRECT_MAX_IDS) and so are the column counts"""
    totals = {c.gb_bits for c in gk.CASES}
    assert {13, 14, 15, 24, 25, 26, 27, 30, 31, 32, 62, 63, 64} <= totals
    assert {len(c.cols) for c in gk.CASES} >= {1, 2, 3, 8, 9, 16}
    prod = lambda c: int(np.prod([col.hi - col.lo + 1 for col in c.cols], dtype=object))
    assert prod(gk.CASE["direct_96x128"]) == prod(gk.CASE["direct_16x24x32"]) == gk.GB_DIRECT_MAX_IDS < prod(gk.CASE["direct_97x127"])
    assert {c.sort_bits for c in gk.CASES} >= {(w,) for w in (9, 17, 18, 25, 26, 27)} | {(64,), (32, 33), (24, 3), (24, 24)}


@pytest.mark.parametrize("name", ["total_64_natural", "reserved_i16_i16_i32", "reserved_8_x_i8"])
def test_reserved_word_rows_are_there(name):
    """the natural layout (column 0 in the low bits) of the explicit rows: 1 << 63, its neighbours, 0 and all-ones"""
    lay = _lay(name)
    word = np.zeros(len(lay.vals), dtype=np.uint64)
    shift = 0
    for k in lay.keys:
        word |= k.view(f"u{k.dtype.itemsize}").astype(np.uint64) << np.uint64(shift)
        shift += k.dtype.itemsize * 8
    assert shift == 64
    for w in (1 << 63, (1 << 63) - 1, (1 << 63) + 1, 0, (1 << 64) - 1):
        assert (word == np.uint64(w)).any(), hex(w)


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_oracle_group_by(name):
    lay, g = _lay(name), _ref(name)
    for op in ("count", "sum", "min"):
        ek, ea = oracle.group_by(op, lay.keys, lay.vals, np.int64)
        gk.assert_groups(ek, ea, None, g, op, False, in_order=not gk.CASE[name].has_nan, what=f"{name} {op}")


@pytest.mark.parametrize("name", NAMES)
def test_reference_equals_oracle_group_by_sort(name):
    lay, g = _lay(name), _ref(name)
    ek, ea, idx = oracle.group_by_sort("sum", lay.keys, lay.vals)
    in_order = not gk.CASE[name].has_nan
    gk.assert_groups(ek, ea, None, g, "sum", False, in_order=in_order, what=name)
    a, b = gk.match_order(ek, ea), gk.match_order(g.keys, g.sum)
    np.testing.assert_array_equal(idx[a], g.last[b])


@pytest.mark.parametrize("name", NAMES)
def test_order_reference_equals_oracle_order_by(name):
    lay = _lay(name)
    want = gk.order_reference(lay.keys)
    np.testing.assert_array_equal(oracle.order_by(lay.keys), want)
    np.testing.assert_array_equal(gk.model_order_by(lay.keys), want)          # the un-mutated sort model is right


@pytest.mark.parametrize("variant", ["vmask", "kmask", "bothmask"])
@pytest.mark.parametrize("name", ["total_15", "three_cols_18", "float32_across_zero", "total_63"])
def test_masked_reference_equals_masked_oracle(name, variant):
    """rows with a null key dropped, null values skipped, a group without a valid value 0 and invalid"""
    lay = _lay(name, "few", 3000)
    kv, vv = gk.masks(lay, variant, np.random.default_rng(5))
    g = gk.reference(lay.keys, lay.vals, kv, vv)
    for op in ("count", "sum", "min"):
        ek, ea, eok = oracle.group_by_masked(op, lay.keys, lay.vals, kv, vv, np.int64 if op == "count" else None)
        gk.assert_groups(ek, ea, eok, g, op, True, in_order=True, what=f"{name} {variant} {op}")
    assert (~g.ok).any() or variant == "kmask"                                  # some group lost every value


def _model_differs(name, mutation):
    lay, g = _lay(name), _ref(name)
    m = gk.model_group_by(lay.keys, mutation)
    if m is None:                                   # the rule declines: the row-comparing table, which is the reference
        return False
    mk, mc = m
    if len(mc) != len(g.rows) or not np.array_equal(mc, g.rows):
        return True
    for a, b in zip(mk, g.keys):
        if not np.array_equal(a, b):                # (no NaN reaches here; == semantics hold: -0.0 equals +0.0 under array_equal)
            return True
    return False


@pytest.mark.parametrize("name", NAMES)
def test_unmutated_model_is_the_reference(name):
    assert not _model_differs(name, None)
    case = gk.CASE[name]
    assert (gk.model_group_by(_lay(name).keys) is None) == (case.gb_bits is None or case.gb_bits > 63)


@pytest.mark.parametrize("mutation", gk.GB_MUTATIONS)
def test_no_group_by_mutation_survives_the_table(mutation):
    killers = [n for n in NAMES if _model_differs(n, mutation)]
    assert killers, f"the mutation {mutation} gives the reference's answer on every case of the table"


@pytest.mark.parametrize("mutation", gk.SORT_MUTATIONS)
def test_no_sort_mutation_survives_the_table(mutation):
    killers = []
    for n in NAMES:
        lay = _lay(n)
        if not np.array_equal(gk.model_order_by(lay.keys, mutation), gk.order_reference(lay.keys)):
            killers.append(n)
    assert killers, f"the mutation {mutation} gives the reference's order on every case of the table"


def test_the_expected_cases_kill_the_mutations():
    """(documentation as a test: the case each mutation was designed to be caught by)"""
    designed = {"width_one_bit_short": "span_full_small", "bias_plus_one": "span_full_small", "bias_ignored": "span_full_small",
                "span_signed_64": "i64_full", "shift_off_by_one": "span_full_large", "columns_reversed": "total_15",
                "no_zero_fold": "float32_across_zero", "no_sign_flip": "float32_across_zero", "budget_gt_64": "total_64_wide"}
    for mutation, name in designed.items():
        assert _model_differs(name, mutation), (mutation, name)
    for mutation, name in {"sort_constant_0_bits": "const_middle", "sort_cap_9_columns": "nine_cols"}.items():
        lay = _lay(name)
        assert not np.array_equal(gk.model_order_by(lay.keys, mutation), gk.order_reference(lay.keys)), (mutation, name)


@pytest.mark.parametrize("mutation", ["width_one_bit_short", "bias_plus_one", "shift_off_by_one", "columns_reversed", "no_zero_fold", "no_sign_flip"])
def test_the_comparison_rejects_a_mutated_answer(mutation):
    """assert_groups -- what the GPU files compare with -- fails on the groups a mutated model reports: on the keys, on COUNT, or, for
    sort_result / AVG output, on the order alone"""
    name = {"no_zero_fold": "float32_across_zero", "no_sign_flip": "float32_across_zero", "columns_reversed": "total_15"}.get(mutation, "span_full_small")
    lay, g = _lay(name), _ref(name)
    mk, mc = gk.model_group_by(lay.keys, mutation)
    with pytest.raises(AssertionError):
        gk.assert_groups(mk, mc, None, g, "count", False, in_order=mutation in ("columns_reversed", "no_sign_flip"), what=mutation)
    mk, mc = gk.model_group_by(lay.keys)
    gk.assert_groups(mk, mc, None, g, "count", False, in_order=True, what="unmutated")
    swapped = g.sum.copy()
    swapped[[0, 1]] = swapped[[1, 0]]                               # two groups that traded their rows: COUNT may agree, SUM does not
    with pytest.raises(AssertionError):
        gk.assert_groups(g.keys, swapped, None, g, "sum", False, what="swapped sums")


def test_pack_unpack_round_trip():
    for name in NAMES:
        lay = _lay(name)
        p = gk.gb_plan(lay.keys)
        if p.total is None or not p.packed:
            continue
        back = gk.unpack(gk.pack(gk.images(lay.keys), p), p, [k.dtype for k in lay.keys])
        for a, b in zip(back, lay.keys):
            assert (a == b).all(), name
        assert int(gk.pack(gk.images(lay.keys), p).max()) < (1 << p.total) if p.total else True


@pytest.mark.parametrize("which", ["near_max", "near_min", "edge_inside", "edge_outside"])
def test_guess_layouts(which):
    """the direct path's guessed window: what the first 65536 rows show, and where the later rows lie relative to the widened window"""
    lay = gk.guess_layout(which, (1 << 20) + 4321, np.random.default_rng(3))
    k = lay.keys[0]
    lo, hi = int(k[:1 << 16].min()), int(k[:1 << 16].max())
    room = (gk.GB_DIRECT_MAX_IDS - (hi - lo + 1)) // 2
    wlo, whi = max(lo - room, gk.IMIN[gk.I64]), min(hi + room, gk.IMAX[gk.I64])
    inside = (int(k.min()) >= wlo) and (int(k.max()) <= whi)
    assert inside == (which != "edge_outside")
    assert int(k.max()) - int(k.min()) + 1 <= gk.GB_DIRECT_MAX_IDS              # the exact range is a direct one in every case
    if which == "near_max":
        assert whi == gk.IMAX[gk.I64] and int(k.max()) == whi
    if which == "near_min":
        assert wlo == gk.IMIN[gk.I64] and int(k.min()) == wlo
    if which == "edge_inside":
        assert int(k.min()) == wlo and int(k.max()) == whi
    if which == "edge_outside":
        assert int(k.min()) == wlo - 1


def test_hot_regime_fills_the_first_window():
    case = gk.CASE["total_24"]
    lay = gk.layout(case, "hot", 40000, np.random.default_rng(2))
    p = gk.gb_plan(lay.keys)
    ids = gk.pack(gk.images(lay.keys), p)
    assert p.total == 24 and 0.45 < (ids < gk.HOT_IDS).mean() < 0.6
    des = gk.designated(case)
    dids = gk.pack(gk.images(des), p)
    assert (dids < gk.HOT_IDS).any() and (dids >= gk.HOT_IDS).any()            # corners inside and outside the window
