"""-m gpu: gdf_amd_order_by_ex (csrc/order.hip) against tests/order_reference.py.  The sort is stable, so the permutation is unique and
every comparison is EXACT.  Masks sit at an odd byte offset inside a buffer filled with 0xFF and have their tail bits set (a mask
needs no alignment; bits beyond size are ignored)."""
import functools

import numpy as np
import pytest

import groupby_keys as gk
import order_reference as orf

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
ROW_COUNTS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 100_000]        # one rs_scatter tile is 4096 pairs
MASKS = ["no_nulls", "all_nulls", "one_valid", "last_null", "half"]
GDF_VALIDITY_UNSUPPORTED = 7
FLAG_COMBOS = [(False, False), (True, False), (False, True), (True, True)]


def make_valid(kind, rows, rng):
    v = np.ones(rows, dtype=bool)
    if kind == "all_nulls":
        v[:] = False
    elif kind == "one_valid":
        v[:] = False
        if rows:
            v[rows // 2] = True
    elif kind == "last_null":
        if rows:
            v[-1] = False
    elif kind == "half":
        v = rng.random(rows) < 0.5
    return v


def run(gdf, cols, desc=None, first=None, dtypes=None):
    """cols: [(data, valid or None)] -> the library's permutation as numpy int32"""
    cs = [orf.device_column(d, v, None if dtypes is None else dtypes[i]) for i, (d, v) in enumerate(cols)]
    out = gdf.api.order_by_ex(cs, desc, first)
    assert str(out.dtype) == "torch.int32" and out.numel() == len(cols[0][0])
    return out.cpu().numpy()


def check(gdf, cols, desc=None, first=None, dtypes=None, what=""):
    got = run(gdf, cols, desc, first, dtypes)
    np.testing.assert_array_equal(got, orf.order_by_ex(cols, desc, first), err_msg=f"{what} desc={desc} nulls_first={first}")
    return got


# ---- row counts x masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_row_counts_and_masks(gdf, rows, mask):
    """two masked columns with many ties (the second decides among equal firsts, the input order among equal rows), DESC on the first"""
    rng = np.random.default_rng(rows * 7 + len(mask))
    a = rng.integers(-3, 4, size=rows).astype(np.int32)
    b = rng.choice(np.array([-1.5, 0.0, -0.0, 2.25, np.nan], dtype=np.float32), size=rows)
    cols = [(a, make_valid(mask, rows, rng)), (b, make_valid(mask, rows, rng))]
    got = check(gdf, cols, [True, False], [False, True], what=f"{rows} rows, {mask}")
    np.testing.assert_array_equal(run(gdf, cols, [True, False], [False, True]), got)             # a second call: bit-identical
    check(gdf, cols[:1], what=f"{rows} rows, {mask}, one column, default flags")


# ---- dtypes and flags ------------------------------------------------------------------------------------------------------------------
KEY_DTYPES = [("int8", np.int8, 1), ("int16", np.int16, 2), ("int32", np.int32, 3), ("int64", np.int64, 4), ("float32", np.float32, 5),
              ("float64", np.float64, 6), ("date32", np.int32, 7), ("date64", np.int64, 8), ("timestamp", np.int64, 9)]


def _draw(npt, rows, rng, wide=True):
    if np.dtype(npt).kind == "f":
        x = (rng.standard_normal(rows) * 1e3).astype(npt)
        x[rng.integers(0, rows, size=rows // 8)] = npt(7.5)                                      # ties
        return x
    info = np.iinfo(npt)
    x = rng.integers(info.min, info.max, size=rows, dtype=npt, endpoint=True) if wide else rng.integers(-2, 2, size=rows).astype(npt)
    x[rng.integers(0, rows, size=rows // 8)] = npt(-1)
    return x


@pytest.mark.parametrize("name,npt,gdf_dtype", KEY_DTYPES, ids=[k[0] for k in KEY_DTYPES])
def test_every_key_dtype_alone_under_all_four_flag_combinations(gdf, name, npt, gdf_dtype):
    rng = np.random.default_rng(gdf_dtype)
    rows = 4097
    data, valid = _draw(npt, rows, rng), rng.random(rows) < 0.7
    for desc, first in FLAG_COMBOS:
        check(gdf, [(data, valid)], [desc], [first], dtypes=[gdf_dtype], what=name)
        check(gdf, [(data, None)], [desc], [first], dtypes=[gdf_dtype], what=name + " without a mask")


def test_sixteen_masked_int8_columns(gdf):
    """MAX_KEY_COLS columns of two values each plus nulls: 16 x (1 + 1) bits, two groups of eight columns; full range: 16 x 9 bits in
    groups of 7 + 7 + 2 columns"""
    rng = np.random.default_rng(16)
    rows = 4097
    for wide in (False, True):
        cols = [(_draw(np.int8, rows, rng, wide) if wide else rng.integers(0, 2, size=rows).astype(np.int8), rng.random(rows) < 0.8)
                for _ in range(16)]
        desc = [bool(c % 2) for c in range(16)]
        first = [bool((c // 2) % 2) for c in range(16)]
        got = {}
        prof = gk.profile_of(gdf, lambda: got.update(p=check(gdf, cols, desc, first, what=f"16 columns, wide={wide}")))
        assert prof.get("ob_make_keys") == (3 if wide else 2), prof


def _sixty_five(kind, rows, rng):
    if kind == "float64":
        x = rng.standard_normal(rows) * 1e100
        x[:6] = [np.inf, -np.inf, np.nan, 0.0, -0.0, 5e-324]
    else:
        x = rng.integers(I64.min, I64.max, size=rows, dtype=np.int64, endpoint=True)
        x[:2] = [I64.min, I64.max]
    valid = rng.random(rows) < 0.75
    valid[:6] = True
    order = rng.permutation(rows)
    return x[order], valid[order]


@pytest.mark.parametrize("place", ["alone", "first_of_three", "last_of_three"])
@pytest.mark.parametrize("kind", ["float64", "int64_full_range"])
def test_sixty_five_bit_column(gdf, kind, place):
    """a masked float64 / full-range int64 column: 64 value bits + the null bit -- the null bit goes to the next column group (alone
    in it when the column is the first key: nothing more significant is left to share it)"""
    rng = np.random.default_rng(65)
    rows = 4097
    wide = _sixty_five(kind, rows, rng)
    small = [(rng.integers(0, 3, size=rows).astype(np.int16), rng.random(rows) < 0.9), (rng.integers(0, 3, size=rows).astype(np.int8), None)]
    if place != "alone":                                                                        # ties in the wide column too
        wide[0][rows // 2:] = wide[0][:rows - rows // 2]
        if kind != "float64":                                                                   # (still the full range, on valid rows)
            wide[0][:2], wide[1][:2] = [I64.min, I64.max], True
    cols = {"alone": [wide], "first_of_three": [wide] + small, "last_of_three": small + [wide]}[place]
    for desc, first in FLAG_COMBOS:
        d = [desc] + [not desc] * (len(cols) - 1)
        f = [first] * len(cols)
        got = {}
        prof = gk.profile_of(gdf, lambda: got.update(p=check(gdf, cols, d, f, what=f"{kind} {place}")))
        assert prof.get("ob_make_keys") == (3 if place == "first_of_three" else 2), prof


def test_flags_mixed_across_columns(gdf):
    rng = np.random.default_rng(4)
    rows = 4097
    cols = [(rng.integers(0, 4, size=rows).astype(np.int8), rng.random(rows) < 0.8) for _ in range(4)]
    for bits in range(256):
        if bits % 5:                                                                            # every fifth of the 256 assignments
            continue
        desc = [bool(bits >> c & 1) for c in range(4)]
        first = [bool(bits >> (4 + c) & 1) for c in range(4)]
        check(gdf, cols, desc, first, what="mixed flags")


# ---- the value domain ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npt", [np.float32, np.float64], ids=["float32", "float64"])
def test_float_specials(gdf, npt):
    """both zeros, NaNs of several payloads and signs, both infinities, denormals -- ascending and descending, with and without nulls"""
    if npt == np.float32:
        nans = np.array([0x7FC00000, 0x7FC00001, 0xFFC00000, 0x7F800001, 0xFFFFFFFF], dtype=np.uint32).view(npt)
    else:
        nans = np.array([0x7FF8000000000000, 0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF],
                        dtype=np.uint64).view(npt)
    assert np.isnan(nans).all()
    tiny = np.finfo(npt).tiny
    base = np.concatenate([nans, np.array([0.0, -0.0, np.inf, -np.inf, tiny / 2, -tiny / 2, 1.0, -1.0, np.finfo(npt).max, np.finfo(npt).min],
                                          dtype=npt)])
    rng = np.random.default_rng(3)
    data = base[rng.integers(0, len(base), size=4097)]
    valid = rng.random(len(data)) < 0.8
    for desc, first in FLAG_COMBOS:
        got = check(gdf, [(data, None)], [desc], [first], what="specials")
        head = data[got[:8]]
        assert np.isnan(head).all() if desc else (head == -np.inf).all()                         # NaN first among descending values
        check(gdf, [(data, valid)], [desc], [first], what="specials with nulls")


def test_data_under_nulls_is_not_compared(gdf):
    """INT64_MIN / INT64_MAX / NaN patterns under the null bits: the permutation is the one with zeros there, and the integer range
    the image is built from stays that of the valid rows (a 3-bit value field: one pass, not eight)"""
    rng = np.random.default_rng(8)
    rows = 100_000
    valid = rng.random(rows) < 0.6
    ints = rng.integers(-3, 4, size=rows).astype(np.int64)
    flts = rng.choice(np.array([-2.0, 0.5, 3.0], dtype=np.float64), size=rows)
    dirty_i, dirty_f = ints.copy(), flts.copy()
    dirty_i[~valid] = rng.choice(np.array([I64.min, I64.max, -1, 1 << 62], dtype=np.int64), size=int((~valid).sum()))
    dirty_f[~valid] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float64), size=int((~valid).sum()))
    clean_i, clean_f = np.where(valid, ints, 0), np.where(valid, flts, 0.0)
    for desc, first in FLAG_COMBOS:
        got = {}
        prof = gk.profile_of(gdf, lambda: got.update(p=check(gdf, [(dirty_i, valid)], [desc], [first], what="dirty int64")))
        assert prof.get("rs_scatter", 0) <= 1, prof
        np.testing.assert_array_equal(run(gdf, [(clean_i, valid)], [desc], [first]), got["p"])
        dirty = check(gdf, [(dirty_f, valid), (dirty_i, valid)], [desc, not desc], [first, first], what="dirty float64 + int64")
        np.testing.assert_array_equal(run(gdf, [(clean_f, valid), (clean_i, valid)], [desc, not desc], [first, first]), dirty)


def test_descending_sort_is_stable(gdf):
    """one key column with 3 distinct values, DESC, 100000 rows: inside each value the row numbers ascend"""
    rng = np.random.default_rng(5)
    data = rng.integers(10, 13, size=100_000).astype(np.int32)
    got = check(gdf, [(data, None)], [True], what="stability")
    keys = data[got]
    assert (np.diff(keys.astype(np.int64)) <= 0).all()
    same = keys[1:] == keys[:-1]
    assert (np.diff(got.astype(np.int64))[same] > 0).all()


# ---- compatibility with gdf_order_by -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _layout(name):
    return gk.layout(gk.CASE[name], "many", 20_001, np.random.default_rng(21))


@pytest.mark.parametrize("name", [c.name for c in gk.CASES])
def test_no_masks_and_zero_flags_is_gdf_order_by(gdf, name):
    """every key layout of tests/groupby_keys.py: the permutation is gdf_order_by's element for element -- through the wrapper
    (a flag byte of 0 per column) and with flags == NULL through the raw entry"""
    import torch
    from libgdf_amd.columns import Column, column_array, column_from_numpy
    lay = _layout(name)
    want = gdf.api.order_by([column_from_numpy(k) for k in lay.keys]).cpu().numpy()
    got = run(gdf, [(k, None) for k in lay.keys])
    np.testing.assert_array_equal(got.astype(np.int64), want)
    cs = [column_from_numpy(k) for k in lay.keys]
    out = Column(torch.empty(len(want), dtype=torch.int32, device="cuda"))
    gdf.libgdf.gdf_amd_order_by_ex(column_array(cs), len(cs), None, out.ptr)
    np.testing.assert_array_equal(out.data.cpu().numpy().astype(np.int64), want)


# ---- passes ------------------------------------------------------------------------------------------------------------------------------
def test_nulls_cost_a_bit_not_a_pass(gdf, force_path):
    """three masked full-range int8 columns: 3 x (8 + 1) = 27 image bits in ONE group -- at most ceil(27 / 8) = 4 rs_scatter launches"""
    rng = np.random.default_rng(27)
    rows = 100_000
    cols = []
    for _ in range(3):
        x = rng.integers(-128, 128, size=rows).astype(np.int8)
        x[:2] = [-128, 127]
        v = rng.random(rows) < 0.9
        v[:2] = True
        cols.append((x, v))
    force_path("GDF_SORT_NO_HYBRID")
    got = {}
    prof = gk.profile_of(gdf, lambda: got.update(p=check(gdf, cols, [False, True, False], [False, False, True], what="27 bits")))
    assert prof.get("ob_make_keys") == 1, prof
    assert 1 <= prof.get("rs_scatter", 0) <= 4 and prof["rs_scatter"] == prof["rs_count"], prof
    # a mask without nulls: its bit never varies and costs nothing -- the launches of the same columns without masks
    no_nulls = [(x, np.ones(rows, dtype=bool)) for x, _ in cols]
    prof_masked = gk.profile_of(gdf, lambda: check(gdf, no_nulls, what="masks without nulls"))
    prof_plain = gk.profile_of(gdf, lambda: check(gdf, [(x, None) for x, _ in cols], what="no masks"))
    assert prof_masked.get("rs_scatter") == prof_plain.get("rs_scatter"), (prof_masked, prof_plain)


# ---- the hybrid path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nulls", ["no_nulls", "half"])
def test_hybrid_path(gdf, force_path, nulls):
    """a 62-bit masked key at 300000 rows with GDF_HS_MIN_ROWS=4096.  Without nulls the image takes hs_local; with 50 % nulls all
    of them share the top bucket, the sample sees it and the LSD passes run instead.  Right both times, and as GDF_SORT_NO_HYBRID"""
    rng = np.random.default_rng(62)
    rows = 300_000
    data = rng.integers(0, 1 << 62, size=rows, dtype=np.int64)
    valid = make_valid(nulls, rows, rng)
    force_path("GDF_HS_MIN_ROWS", 4096)
    for desc, first in ((True, False), (False, True)):
        got = {}
        prof = gk.profile_of(gdf, lambda: got.update(p=check(gdf, [(data, valid)], [desc], [first], what=f"hybrid {nulls}")))
        assert "hs_sample" in prof, sorted(prof)
        assert ("hs_local" in prof) == (nulls == "no_nulls"), sorted(prof)
        force_path("GDF_SORT_NO_HYBRID")
        prof2 = gk.profile_of(gdf, lambda: np.testing.assert_array_equal(run(gdf, [(data, valid)], [desc], [first]), got["p"]))
        assert "hs_sample" not in prof2 and "hs_local" not in prof2, sorted(prof2)
        force_path("GDF_SORT_NO_HYBRID", None)


# ---- gdf_order_by itself ---------------------------------------------------------------------------------------------------------------
def test_gdf_order_by_is_unchanged(gdf):
    """it still refuses a mask, and one plain call launches the sort kernels it launched before, under their names"""
    from libgdf_amd import GDFError
    from libgdf_amd.columns import column_from_numpy
    rng = np.random.default_rng(1)
    data = rng.integers(-(1 << 40), 1 << 40, size=70_001, dtype=np.int64)
    with pytest.raises(GDFError) as e:
        gdf.api.order_by([column_from_numpy(data, np.ones(len(data), dtype=bool))])
    assert e.value.errcode == GDF_VALIDITY_UNSUPPORTED
    got = {}
    prof = gk.profile_of(gdf, lambda: got.update(p=gdf.api.order_by([column_from_numpy(data)]).cpu().numpy()))
    np.testing.assert_array_equal(got["p"], np.argsort(data, kind="stable"))
    sort_names = {n for n in prof if n.split("_")[0] in ("rs", "hs", "ob", "ga")}
    assert sort_names == {"rs_minmax", "rs_make_keys", "rs_count", "rs_scatter", "rs_widen"}, sorted(prof)
    assert prof["rs_make_keys"] == 1 and prof["rs_scatter"] == prof["rs_count"] == (41 + 8) // 9
    # ... and the new entry runs the same passes over an image of its own making
    prof_ex = gk.profile_of(gdf, lambda: np.testing.assert_array_equal(run(gdf, [(data, None)]), got["p"]))
    assert {n for n in prof_ex if n.split("_")[0] in ("rs", "hs", "ob", "ga")} == {"rs_minmax", "ob_make_keys", "rs_count", "rs_scatter"}
    assert prof_ex["rs_scatter"] == prof["rs_scatter"]
