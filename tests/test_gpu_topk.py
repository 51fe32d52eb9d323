"""-m gpu: gdf_amd_top_k (csrc/topk.hip) against tests/order_reference.py::order_by_ex(cols, desc, first)[offset:offset + k] -- numpy,
not the code under test.  The order is total and stable, so the rows are unique and every comparison is EXACT.  Masks sit at an odd
byte offset inside a buffer filled with 0xFF and have their tail bits set.  The output buffer carries 64 sentinel elements behind m
that must stay; every call is made twice and the second result must be bit-identical.

The select stops as soon as at most TK_SLACK (32768) images share T's decided bits, which at the row counts here is after its first
pass; force_path("GDF_TK_SLACK", 0) makes it run to the last digit, and the cases that are about the digits run both ways.

Which case would catch which mutation of tests/topk_reference.py (each changes the rows, so the exact comparison fails):
    ties_cut_by_value_not_row            test_cut_inside_runs_of_zeros_and_nans (complete float images; tests/test_topk_reference.py
                                         shows on the same table that the mutation changes every one of its cuts)
    tie_block_not_in_row_order           test_cut_inside_a_run, test_all_rows_equal
    truncated_image_treated_as_complete  test_truncated_images (pairs that differ in the dropped bit only), test_every_bit (float64, b = 0)
    straddling_field_low_bits_kept       test_truncated_images (full-range int64), test_every_bit (masked float64, every b >= 1)
    desc_complements_beyond_field        test_row_counts_and_masks (DESC on the second column), test_truncated_images (sixteen columns)
    null_bit_below_value                 test_row_counts_and_masks ("half", "last_null"), test_every_key_dtype with a mask
    data_under_null_compared             test_data_under_nulls
    offset_applied_before_selection      test_row_counts_and_masks (offset in {1, k, rows - 1}), test_cut_inside_a_run
    k_th_is_k_plus_one                   test_cut_inside_a_run, test_every_bit (K = the size of the lower half - 1)
"""
import ctypes as C

import numpy as np
import pytest

import groupby_keys as gk
import order_reference as orf
import topk_reference as tkr

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
TILE = 512                                   # TK_TILE of csrc/topk.hip: the rows one wave of tk_pass / tk_count / tk_emit owns
TK_CAND_CAP = 10_000_000 + (1 << 15)         # the shipped candidate cap (csrc/topk.hip)
ROW_COUNTS = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 100_000]
MASKS = ["no_nulls", "all_nulls", "one_valid", "last_null", "half"]
FLAG_COMBOS = [(False, False), (True, False), (False, True), (True, True)]
SENTINEL, GUARD = -7, 64
ROUTE_SELECT, ROUTE_K, ROUTE_CAP = 0, 1, 2


def make_valid(kind, rows, rng):
    v = np.ones(rows, dtype=bool)
    if kind == "all_nulls":
        v[:] = False
    elif kind == "one_valid":
        v[:] = False
        v[rows // 2] = True
    elif kind == "last_null":
        v[-1] = False
    elif kind == "half":
        v = rng.random(rows) < 0.5
    return v


def note(gdf, name):
    v = C.c_longlong(-1)
    assert gdf.libgdf.gdf_amd_debug_noted(name.encode(), C.byref(v)) == 0, name
    return int(v.value)


class Table:
    """key columns uploaded once, their oracle permutation computed once"""

    def __init__(self, cols, desc=None, first=None, dtypes=None):
        self.cols, self.desc, self.first = cols, desc, first
        self.rows = len(cols[0][0])
        self.dev = [orf.device_column(d, v, None if dtypes is None else dtypes[i]) for i, (d, v) in enumerate(cols)]
        self.want = orf.order_by_ex(cols, desc, first)
        n = len(cols)
        d, f = orf._flags(desc, n), orf._flags(first, n)
        self.flags = (C.c_uint8 * n)(*[(1 if a else 0) | (2 if b else 0) for a, b in zip(d, f)])

    def call(self, gdf, k, offset):
        import torch
        from libgdf_amd.columns import Column, column_array
        m = max(0, min(k, self.rows - offset))
        buf = torch.full((m + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
        out = Column(buf, None, 3, size=m)
        gdf.libgdf.gdf_amd_top_k(column_array(self.dev), len(self.dev), self.flags, k, offset, out.ptr)
        got = buf.cpu().numpy()
        assert (got[m:] == SENTINEL).all(), "written behind m"
        return got[:m]

    def check(self, gdf, k, offset=0, what=""):
        got = self.call(gdf, k, offset)
        np.testing.assert_array_equal(got, self.want[offset:offset + k], err_msg=f"{what} rows={self.rows} k={k} offset={offset} "
                                      f"desc={self.desc} nulls_first={self.first}")
        np.testing.assert_array_equal(self.call(gdf, k, offset), got, err_msg="the second call differs")
        return got


# ---- row counts x masks ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("rows", ROW_COUNTS)
def test_row_counts_and_masks(gdf, rows, mask):
    """two masked columns with many ties (the second decides among equal firsts, the row number among equal rows), DESC on the second;
    every k of {1, 2, 64, rows - 1, rows, rows + 1} and every offset of {0, 1, k, rows - 1} at every row count"""
    rng = np.random.default_rng(rows * 7 + len(mask))
    a = rng.integers(-3, 4, size=rows).astype(np.int32)
    b = rng.choice(np.array([-1.5, 0.0, -0.0, 2.25, np.nan], dtype=np.float32), size=rows)
    t = Table([(a, make_valid(mask, rows, rng)), (b, make_valid(mask, rows, rng))], [False, True], [False, True])
    ks = [1, 2, 64, rows - 1, rows, rows + 1]
    for i, k in enumerate(ks):
        offsets = [0, 1, k, rows - 1]
        t.check(gdf, k, offsets[i % 4], what=mask)
        t.check(gdf, k, offsets[(i + 1) % 4], what=mask)
    t1 = Table(t.cols[:1])
    t1.check(gdf, 64, 1, what=mask + ", one column, default flags")


# ---- dtypes and flags ------------------------------------------------------------------------------------------------------------------
KEY_DTYPES = [("int8", np.int8, 1), ("int16", np.int16, 2), ("int32", np.int32, 3), ("int64", np.int64, 4), ("float32", np.float32, 5),
              ("float64", np.float64, 6), ("date32", np.int32, 7), ("date64", np.int64, 8), ("timestamp", np.int64, 9)]


def _draw(npt, rows, rng):
    if np.dtype(npt).kind == "f":
        x = (rng.standard_normal(rows) * 1e3).astype(npt)
        nan2 = np.array([0x7FC00001], dtype=np.uint32).view(np.float32)[0] if npt == np.float32 else \
            np.array([0xFFF8000000000001], dtype=np.uint64).view(np.float64)[0]
        specials = np.array([np.nan, nan2, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324], dtype=npt)
        where = rng.permutation(rows)[:len(specials) * 6]
        x[where] = np.tile(specials, 6)
        return x
    info = np.iinfo(npt)
    x = rng.integers(info.min, info.max, size=rows, dtype=npt, endpoint=True)
    x[rng.integers(0, rows, size=rows // 8)] = npt(-1)
    x[:2] = [info.min, info.max]
    return x


@pytest.mark.parametrize("name,npt,gdf_dtype", KEY_DTYPES, ids=[k[0] for k in KEY_DTYPES])
def test_every_key_dtype_alone_under_all_four_flag_combinations(gdf, force_path, name, npt, gdf_dtype):
    """4097 rows, with and without a mask.  Floats: NaNs of two payloads, both infinities, both zeros and the smallest denormals (six
    rows of each): k = 30 takes in all twelve NaNs (DESC) / the six -inf (ASC), k = 2100 passes the zeros and the denormals in both
    directions.  No cut here falls INSIDE a run of rows that tie on the image: test_cut_inside_runs_of_zeros_and_nans does that"""
    rng = np.random.default_rng(gdf_dtype)
    rows = 4097
    data, valid = _draw(npt, rows, rng), rng.random(rows) < 0.7
    for desc, first in FLAG_COMBOS:
        for v in (valid, None):
            t = Table([(data, v)], [desc], [first], dtypes=[gdf_dtype])
            t.check(gdf, 30, 0, what=name)
            t.check(gdf, 2100, 5, what=name)
            force_path("GDF_TK_SLACK", 0)                                                        # ... and with T decided to its last bit
            t.check(gdf, 30, 0, what=name + ", no slack")
            t.check(gdf, 2100, 5, what=name + ", no slack")
            assert note(gdf, "tk.exact") == 1
            force_path("GDF_TK_SLACK", None)
            if v is not None and first:                                                          # the nulls, then the first values
                t.check(gdf, 30, int((~valid).sum()) - 3, what=name)


def test_data_under_nulls(gdf):
    """INT64_MIN / INT64_MAX / NaN patterns under the null bits: the rows are those of the table with zeros there"""
    rng = np.random.default_rng(8)
    rows = 20_000
    valid = rng.random(rows) < 0.6
    ints = rng.integers(-3, 4, size=rows).astype(np.int64)
    flts = rng.choice(np.array([-2.0, 0.5, 3.0], dtype=np.float64), size=rows)
    dirty_i, dirty_f = ints.copy(), flts.copy()
    dirty_i[~valid] = rng.choice(np.array([I64.min, I64.max, -1, 1 << 62], dtype=np.int64), size=int((~valid).sum()))
    dirty_f[~valid] = rng.choice(np.array([np.nan, np.inf, -np.inf, -0.0], dtype=np.float64), size=int((~valid).sum()))
    nvalid = int(valid.sum())
    for desc, first in FLAG_COMBOS:
        for cols in ([(dirty_i, valid)], [(dirty_f, valid), (dirty_i, valid)]):
            t = Table(cols, [desc] * len(cols), [first] * len(cols))
            t.check(gdf, 100, 0 if first else nvalid - 50, what="dirty")                         # the page holds nulls and values
            t.check(gdf, 100, rows - nvalid - 50 if first else 0, what="dirty")


# ---- the cut inside a run of equal rows --------------------------------------------------------------------------------------------------
def test_cut_inside_a_run(gdf):
    """one int8 column of three values plus nulls, 100000 rows: a complete image with massive ties.  The selection route, one column
    pass of the select, and exactly K candidates"""
    rng = np.random.default_rng(5)
    rows = 100_000
    data = rng.integers(10, 13, size=rows).astype(np.int8)
    valid = rng.random(rows) < 0.9
    for desc, first in FLAG_COMBOS:
        t = Table([(data, valid)], [desc], [first])
        run0 = int((~valid).sum()) if first else int((valid & (data == (12 if desc else 10))).sum())
        for k, offset in ((10, 0), (run0 - 1, 0), (run0, 0), (run0 + 1, 0), (10, run0 - 5), (run0, 7)):
            gdf.libgdf.gdf_amd_debug_noted(None, None)
            prof = gk.profile_of(gdf, lambda: t.check(gdf, k, offset, what="run"))
            assert note(gdf, "tk.route") == ROUTE_SELECT and note(gdf, "tk.complete") == 1
            assert note(gdf, "tk.candidates") == offset + k
            assert {"tk_pass", "tk_select", "tk_count", "tk_emit", "tk_write"} <= set(prof), sorted(prof)
        got = t.check(gdf, run0 + 1000, 0, what="run")
        keys = np.where(valid[got], data[got], -1)
        assert (np.diff(got.astype(np.int64))[keys[1:] == keys[:-1]] > 0).all()                 # inside a run the row numbers ascend


@pytest.mark.parametrize("kind", ["float32", "float64", "masked_float32"])
def test_cut_inside_runs_of_zeros_and_nans(gdf, force_path, kind):
    """complete float images (32, 64 and 33 bits) whose rows are mostly +0.0 / -0.0 and NaNs of two payloads in shuffled row order:
    K = offset + k falls inside the run of zeros and inside the run of NaNs, so rows that tie on the image but differ in their raw
    bits stand on both sides of the cut -- it goes to the lower row number.  Each run is longer than TK_SLACK, so T is exact and
    exactly K rows are candidates both as shipped and with GDF_TK_SLACK = 0"""
    npt = np.float64 if kind == "float64" else np.float32
    col, cuts = tkr.tied_floats(npt, 100_000, np.random.default_rng(70), kind.startswith("masked"))
    for desc, first in FLAG_COMBOS:
        t = Table([col], [desc], [first])
        for slack in (None, 0):
            force_path("GDF_TK_SLACK", slack)
            for k, offset in cuts(desc, first):
                gdf.libgdf.gdf_amd_debug_noted(None, None)
                got = t.check(gdf, k, offset, what=f"{kind}, slack {slack}")
                assert note(gdf, "tk.route") == ROUTE_SELECT and note(gdf, "tk.complete") == 1 and note(gdf, "tk.exact") == 1
                assert note(gdf, "tk.candidates") == offset + k
                tail = col[0][got[-2:]]                                                          # the last rows of the page tie with the next
                assert (tail == 0).all() or np.isnan(tail).all()


# ---- every bit of the image decides once -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["int64", "masked_float64"])
def test_every_bit_of_the_image_decides(gdf, force_path, kind):
    """for b in 0 .. 63 a column whose two shuffled halves differ in bit b only; K = the size of the lower half and +- 1.  The masked
    float64 is 65 bits: its bit 0 is the dropped one, which the finish has to resolve"""
    rng = np.random.default_rng(64)
    rows = 4097
    for b in range(64):
        upper = rng.random(rows) < 0.5
        if kind == "int64":
            base = np.uint64(0x1234_5678_9ABC_DEF0) & ~np.uint64(1 << b)
            data = np.where(upper, base | np.uint64(1 << b), base).astype(np.uint64).view(np.int64)
            valid = None
        else:
            base = np.uint64(0x3FE8_0000_0000_0000) & ~np.uint64(1 << b)                         # 0.75: no bit makes it a NaN
            data = np.where(upper, base | np.uint64(1 << b), base).astype(np.uint64).view(np.float64)
            assert np.isfinite(data).all()
            valid = rng.random(rows) < 0.9
        desc = bool(b % 2)
        t = Table([(data, valid)], [desc], [False])
        first_value = data[t.want[0]]
        lower = int(((data == first_value) & (valid if valid is not None else True)).sum())      # the run the order starts with
        force_path("GDF_TK_SLACK", 0)                                                            # every digit down to bit b
        for K in (lower - 1, lower, lower + 1):
            t.check(gdf, K, 0, what=f"{kind} bit {b}")
        assert note(gdf, "tk.exact") == 1
        if kind == "int64":                          # the digits down to the one that holds bit b, and the pass that finds all equal
            assert note(gdf, "tk.column_passes") == min(6, (63 - b) // 11 + 2)
        force_path("GDF_TK_SLACK", None)
        t.check(gdf, lower, 0, what=f"{kind} bit {b}, the shipped slack")
        t.check(gdf, 3, lower - 1, what=f"{kind} bit {b}, the shipped slack")


# ---- truncated images --------------------------------------------------------------------------------------------------------------------
def _pairs_in_the_low_bit(rows, rng):
    """full-range int64 whose second half repeats the first with bit 0 flipped: pairs that share every image bit but the dropped one"""
    x = rng.integers(I64.min, I64.max, size=rows, dtype=np.int64, endpoint=True)
    x[:2] = [I64.min, I64.max]
    half = rows // 2
    x[half:2 * half] = x[:half] ^ 1
    order = rng.permutation(rows)
    valid = rng.random(rows) < 0.8
    valid[:2] = True
    return x[order], valid[order]


@pytest.mark.parametrize("shape", ["alone", "first_of_three", "last_of_three", "two_int64", "sixteen_int8"])
def test_truncated_images(gdf, force_path, shape):
    """keys wider than 64 bits, with ties on L that only the dropped bits resolve, and DESC on the straddling column"""
    rng = np.random.default_rng(65)
    rows = 4097
    small = [(rng.integers(0, 3, size=rows).astype(np.int16), rng.random(rows) < 0.9), (rng.integers(0, 3, size=rows).astype(np.int8), None)]
    if shape == "two_int64":                                                                     # the second column is not in L at all
        cols = [(rng.integers(-2, 3, size=rows).astype(np.int64), None), (rng.integers(I64.min, I64.max, size=rows, dtype=np.int64), None)]
        straddle = 1
    elif shape == "sixteen_int8":                                                                # 16 x 9 = 144 bits; L ends in column 8's null bit
        proto = rng.integers(-128, 128, size=(40, 8)).astype(np.int8)
        pick = rng.integers(0, 40, size=rows)
        cols = [(proto[pick, c].copy(), rng.random(rows) < 0.95) for c in range(8)]
        cols += [(rng.integers(-128, 128, size=rows).astype(np.int8), rng.random(rows) < 0.8) for _ in range(8)]
        straddle = 7
    else:
        wide = _pairs_in_the_low_bit(rows, rng)
        cols = {"alone": [wide], "first_of_three": [wide] + small, "last_of_three": small + [wide]}[shape]
        straddle = {"alone": 0, "first_of_three": 0, "last_of_three": 2}[shape]
    for desc, first in FLAG_COMBOS:
        d = [not desc] * len(cols)
        d[straddle] = desc
        t = Table(cols, d, [first] * len(cols))
        for slack in (None, 0):
            force_path("GDF_TK_SLACK", slack)
            for k, offset in ((1, 0), (2, 0), (100, 0), (100, 37), (1000, 1000)):
                gdf.libgdf.gdf_amd_debug_noted(None, None)
                t.check(gdf, k, offset, what=f"{shape}, slack {slack}")
                assert note(gdf, "tk.route") == ROUTE_SELECT and note(gdf, "tk.complete") == 0
                assert note(gdf, "tk.candidates") >= offset + k
                assert slack is None or note(gdf, "tk.exact") == 1


# ---- all rows equal ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("image", ["complete", "truncated"])
def test_all_rows_equal(gdf, image):
    """L identical everywhere, k in the middle: the rows come in row order.  Complete: K candidates; truncated: every row is one"""
    rows = 4097
    cols = [(np.full(rows, -5, dtype=np.int32), np.ones(rows, dtype=bool))] if image == "complete" else \
        [(np.full(rows, I64.min, dtype=np.int64), np.ones(rows, dtype=bool)), (np.full(rows, 1.5, dtype=np.float32), None)]
    for desc, first in FLAG_COMBOS:
        t = Table(cols, [desc] * len(cols), [first] * len(cols))
        gdf.libgdf.gdf_amd_debug_noted(None, None)
        got = t.check(gdf, 2000, 7, what=image)
        np.testing.assert_array_equal(got, np.arange(7, 2007, dtype=np.int32))
        assert note(gdf, "tk.route") == ROUTE_SELECT and note(gdf, "tk.column_passes") == 1
        assert note(gdf, "tk.candidates") == (2007 if image == "complete" else rows)


# ---- both fallbacks ----------------------------------------------------------------------------------------------------------------------
def test_both_fallbacks_give_the_selection_routes_answers(gdf, force_path):
    """4097 rows: GDF_TK_MAX_K below K sends the call to the whole sort at once, GDF_TK_CAND_CAP below the ties of a truncated image
    sends it there after the select; the rows are those of the selection route"""
    rng = np.random.default_rng(7)
    rows = 4097
    t = Table([_pairs_in_the_low_bit(rows, rng), (rng.integers(0, 3, size=rows).astype(np.int8), None)], [True, False], [False, True])
    tied = Table([(np.full(rows, 3, dtype=np.int64), rng.random(rows) < 0.9), (rng.integers(0, 50, size=rows).astype(np.int16), None)])
    for tab, k, offset in ((t, 100, 20), (tied, 100, 20), (tied, 3000, 0)):
        gdf.libgdf.gdf_amd_debug_noted(None, None)
        prof = gk.profile_of(gdf, lambda: tab.check(gdf, k, offset, what="selection"))
        assert note(gdf, "tk.route") == ROUTE_SELECT and "tk_emit" in prof, sorted(prof)
        selected = tab.call(gdf, k, offset)
        force_path("GDF_TK_MAX_K", offset + k - 1)
        gdf.libgdf.gdf_amd_debug_noted(None, None)
        prof = gk.profile_of(gdf, lambda: np.testing.assert_array_equal(tab.check(gdf, k, offset, what="K fallback"), selected))
        assert note(gdf, "tk.route") == ROUTE_K and not any(name.startswith("tk_") for name in prof), sorted(prof)
        force_path("GDF_TK_MAX_K", offset + k)                                                   # K == the limit still selects
        tab.check(gdf, k, offset, what="at the limit")
        assert note(gdf, "tk.route") == ROUTE_SELECT
        force_path("GDF_TK_MAX_K", None)
    # the candidate cap: `tied` has ~3700 rows that share L (the constant first column; the second is not in L)
    ties = int(tied.cols[0][1].sum())
    force_path("GDF_TK_CAND_CAP", ties - 1)
    gdf.libgdf.gdf_amd_debug_noted(None, None)
    prof = gk.profile_of(gdf, lambda: tied.check(gdf, 100, 20, what="cap fallback"))
    assert note(gdf, "tk.route") == ROUTE_CAP and note(gdf, "tk.candidates") == ties
    assert "tk_pass" in prof and "tk_emit" not in prof, sorted(prof)
    force_path("GDF_TK_CAND_CAP", ties)                                                          # exactly the cap still selects
    tied.check(gdf, 100, 20, what="at the cap")
    assert note(gdf, "tk.route") == ROUTE_SELECT
    # a complete image never has more than K candidates: the cap does not apply
    force_path("GDF_TK_CAND_CAP", 1)
    Table([(np.full(rows, 3, dtype=np.int32), None)]).check(gdf, 100, 20, what="complete under a cap of 1")
    assert note(gdf, "tk.route") == ROUTE_SELECT
    # k beyond the table is the whole sort whatever the limits say
    force_path("GDF_TK_CAND_CAP", None)
    tied.check(gdf, rows, 1, what="k beyond the table")
    assert note(gdf, "tk.route") == ROUTE_K


def test_the_shipped_cap_without_an_override(gdf):
    """the smallest row count that exceeds the shipped cap with a truncated all-equal image: every row is a candidate, so the call
    takes the whole sort -- and gives the rows in row order"""
    rows = TK_CAND_CAP + 1
    t = Table([(np.full(rows, 3, dtype=np.int64), np.ones(rows, dtype=bool))])
    gdf.libgdf.gdf_amd_debug_noted(None, None)
    got = t.check(gdf, 100, 5, what="beyond the shipped cap")
    np.testing.assert_array_equal(got, np.arange(5, 105, dtype=np.int32))
    assert note(gdf, "tk.route") == ROUTE_CAP and note(gdf, "tk.candidates") == rows


def test_the_select_with_and_without_its_slack(gdf, force_path):
    """100000 full-range int64 keys: as shipped the select stops after one pass with ~50 rows sharing T's first eleven bits (all of
    them candidates); without slack it runs until T is exact and the candidates are exactly K.  The same rows both ways"""
    rng = np.random.default_rng(17)
    rows = 100_000
    t = Table([(rng.integers(I64.min, I64.max, size=rows, dtype=np.int64, endpoint=True), None)], [True])
    for k, offset in ((1, 0), (1000, 0), (50, 99_900), (40_000, 7)):
        gdf.libgdf.gdf_amd_debug_noted(None, None)
        shipped = t.check(gdf, k, offset, what="shipped slack")
        assert note(gdf, "tk.route") == ROUTE_SELECT and note(gdf, "tk.exact") == 0 and note(gdf, "tk.column_passes") == 1
        assert offset + k <= note(gdf, "tk.candidates") < offset + k + (1 << 15)
        force_path("GDF_TK_SLACK", 0)
        np.testing.assert_array_equal(t.check(gdf, k, offset, what="no slack"), shipped)
        assert note(gdf, "tk.exact") == 1 and note(gdf, "tk.column_passes") >= 2 and note(gdf, "tk.candidates") == offset + k
        force_path("GDF_TK_SLACK", None)


# ---- parity with the library itself ------------------------------------------------------------------------------------------------------
def test_parity_with_order_by_ex_and_gather(gdf):
    """api.top_k(...) == api.order_by_ex(...)[offset:offset + k], and api.gather of it gives the expected rows and masks"""
    rng = np.random.default_rng(12)
    rows = 100_000
    cases = [([(rng.integers(0, 1 << 62, size=rows, dtype=np.int64), None)], [False], [False], 100, 0),
             ([_pairs_in_the_low_bit(rows, rng)], [True], [False], 1000, 50),
             ([(rng.integers(-3, 4, size=rows).astype(np.int8), rng.random(rows) < 0.8),
               (rng.standard_normal(rows).astype(np.float32), rng.random(rows) < 0.8)], [True, False], [True, False], 64, rows - 100)]
    for cols, desc, first, k, offset in cases:
        cs = [orf.device_column(d, v) for d, v in cols]
        got = gdf.api.top_k(cs, k, desc, first, offset=offset)
        assert str(got.dtype) == "torch.int32" and got.numel() == min(k, rows - offset)
        np.testing.assert_array_equal(got.cpu().numpy(), gdf.api.order_by_ex(cs, desc, first)[offset:offset + k].cpu().numpy())
        np.testing.assert_array_equal(got.cpu().numpy(), orf.order_by_ex(cols, desc, first)[offset:offset + k])
    payload = [(rng.standard_normal(rows), rng.random(rows) < 0.7), (rng.integers(-9, 9, size=rows).astype(np.int16), None)]
    outs = gdf.api.gather(got, cs + [orf.device_column(d, v) for d, v in payload])
    want = orf.gather(orf.order_by_ex(cols, desc, first)[offset:offset + k], cols + payload)
    for o, (data, ok, mask, nulls) in zip(outs, want):
        np.testing.assert_array_equal(orf.bits_of(o.to_numpy()), orf.bits_of(data))
        np.testing.assert_array_equal(o.valid.cpu().numpy(), mask)
        assert int(o.c.null_count) == nulls
    assert gdf.api.top_k(cs, 0).numel() == 0 and gdf.api.top_k(cs, 5, offset=rows).numel() == 0
