"""-m gpu: gdf_amd_semi_join (csrc/semijoin.hip) against tests/semi_join_reference.py::semi_join -- Python sets, not the code under test.
The result is a list of distinct ascending row numbers, so every comparison is EXACT.  Masks sit at an odd byte offset inside a buffer
filled with 0xFF and have their tail bits set.  A row with a null carries, in ALL its columns, the data of some row of the other side:
were the mask not looked at, it would match.  Every call is made twice and the second result must be bit-identical.  Every case outside
the deliberate extremes (one row, an empty side, a side of nulls) first asserts 0 < m < left rows from the model, so that "nothing" and
"everything" cannot pass.  A test loops over its cases itself; the failure message names the case.

Which case would catch which mutation of tests/semi_join_reference.py (each changes the rows, so the exact comparison fails):
    null_matches_null_without_flag   test_mask_kinds_on_either_side ("half" / "last_null" on both sides, flags without NULLS_EQUAL),
                                     test_left_row_counts
    null_matches_value_with_flag     test_a_null_never_meets_the_value_zero
    nan_matches_nan                  test_floats_zeros_nans_infinities (NaNs of two payloads on both sides), test_every_key_dtype (floats)
    negative_zero_distinct           test_floats_zeros_nans_infinities (-0.0 only on the left, +0.0 only on the right)
    data_under_null_compared         every masked case: the data under the nulls is another row's that would match
    anti_drops_null_rows             test_left_row_counts, test_mask_kinds_on_either_side (ANTI without NULLS_EQUAL over "half")
    result_not_ascending             every case (exact comparison of the order); test_against_the_inner_join sorts nothing of ours
    duplicates_emitted_per_partner   test_right_distinct_counts (every key 16 times), test_against_the_inner_join
    reserved_image_lost              test_the_reserved_image (eight int8 columns / one int64 column of -1), test_int64_extremes
    tag_hit_taken_as_match           test_wide_keys_that_differ_in_the_last_column_only with GDF_SJ_TAG_BITS = 4
"""
import ctypes as C

import numpy as np
import pytest

import groupby_keys as gk
import order_reference as orf
import semi_join_reference as sjr

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
TILE = 512                                   # SJ_TILE of csrc/semijoin.hip: the rows one wave probes and emits
LDS_C = 8192                                 # SJ_LDS_C: distinct keys up to which the LDS route is taken (SJ_LDS_MAX_SLOTS / 2)
LDS_MAX = 8192                               # what one workgroup's LDS holds at half load: a forced LDS route goes no further
ROW_COUNTS = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 100_000]
MASKS = ["no_nulls", "all_nulls", "one_valid", "last_null", "half"]
EXTREME_MASKS = ("all_nulls", "one_valid")
FLAG_COMBOS = [(False, False), (True, False), (False, True), (True, True)]          # (anti, nulls_equal)
ROUTE_NONE, ROUTE_LDS, ROUTE_GLOBAL, ROUTE_WIDE = 0, 1, 2, 3


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


def _with_other_sides_data_under_nulls(mine, other, rng):
    """every row of `mine` with a null gets, in all its columns, the data of a random row of `other`; the masks stay"""
    n, rows_other = len(mine[0][0]), len(other[0][0])
    has_null = np.zeros(n, dtype=bool)
    for _, v in mine:
        if v is not None:
            has_null |= ~np.asarray(v, dtype=bool)
    if not has_null.any() or rows_other == 0:
        return mine
    src = rng.integers(0, rows_other, size=int(has_null.sum()))
    out = []
    for (d, v), (od, _) in zip(mine, other):
        d = np.array(d, copy=True)
        d[has_null] = np.asarray(od)[src]
        out.append((d, v))
    return out


class Pair:
    """both sides uploaded once; the model's answer computed once per flag combination"""

    def __init__(self, left, right, dtypes=None, seed=0):
        rng = np.random.default_rng(seed)
        self.left = _with_other_sides_data_under_nulls(left, right, rng)
        self.right = _with_other_sides_data_under_nulls(right, left, rng)
        self.rows = len(left[0][0])
        self.ldev = [orf.device_column(d, v, None if dtypes is None else dtypes[i]) for i, (d, v) in enumerate(self.left)]
        self.rdev = [orf.device_column(d, v, None if dtypes is None else dtypes[i]) for i, (d, v) in enumerate(self.right)]
        self._want = {}

    def want(self, anti, nulls_equal):
        key = (bool(anti), bool(nulls_equal))
        if key not in self._want:
            self._want[key] = sjr.semi_join(self.left, self.right, anti, nulls_equal)
        return self._want[key]

    def call(self, gdf, anti, nulls_equal):
        got = gdf.api.semi_join(self.ldev, self.rdev, anti=anti, nulls_equal=nulls_equal)
        assert str(got.dtype) == "torch.int32"
        return got.cpu().numpy()

    def check(self, gdf, anti=False, nulls_equal=False, what="", extreme=False):
        want = self.want(anti, nulls_equal)
        if not extreme:
            assert 0 < len(want) < self.rows, f"{what}: the model gives {len(want)} of {self.rows} rows -- the case shows nothing"
        got = self.call(gdf, anti, nulls_equal)
        np.testing.assert_array_equal(got, want, err_msg=f"{what} rows={self.rows} anti={anti} nulls_equal={nulls_equal}")
        np.testing.assert_array_equal(self.call(gdf, anti, nulls_equal), got, err_msg="the second call differs")
        return got

    def check_all_flags(self, gdf, what="", extreme=False):
        for anti, nulls_equal in FLAG_COMBOS:
            self.check(gdf, anti, nulls_equal, what, extreme)


def _half_hitting(distinct, left_rows, rng, npt=np.int64, repeat=1):
    """right: `distinct` unique keys out of [0, 2 * distinct), each `repeat` times, shuffled; left: draws from that range"""
    right = rng.permutation(2 * distinct)[:distinct].astype(npt)
    right = rng.permutation(np.repeat(right, repeat))
    left = rng.integers(0, 2 * distinct, size=left_rows).astype(npt)
    return left, right


# ---- left row counts ---------------------------------------------------------------------------------------------------------------------
def _left_row_count(gdf, rows):
    """a masked int32 and an unmasked int16 column, 60 right rows; every flag combination at every row count around the emit tile"""
    rng = np.random.default_rng(rows)
    la, lb = rng.integers(0, 8, size=rows).astype(np.int32), rng.integers(0, 4, size=rows).astype(np.int16)
    ra, rb = rng.integers(0, 8, size=60).astype(np.int32), rng.integers(0, 4, size=60).astype(np.int16)
    keep = (ra * 4 + rb) % 3 != 0                                                    # a third of the 32 combinations never occur
    p = Pair([(la, rng.random(rows) < 0.8), (lb, None)], [(ra[keep], rng.random(int(keep.sum())) < 0.8), (rb[keep], None)], seed=rows)
    p.check_all_flags(gdf, what="row counts", extreme=rows == 1)
    if rows == 1:                                                                    # the one row once with and once without a partner
        for value, hits in ((5, True), (6, False)):
            q = Pair([(np.array([value], dtype=np.int32), None)], [(np.array([1, 5, 5], dtype=np.int32), None)])
            for anti, nulls_equal in FLAG_COMBOS:
                got = q.check(gdf, anti, nulls_equal, what="one row", extreme=True)
                assert len(got) == int(hits != anti)


def test_left_row_counts(gdf):
    for rows in ROW_COUNTS:
        _left_row_count(gdf, rows)


# ---- right distinct counts and the routes ------------------------------------------------------------------------------------------------
def _right_distinct_count(gdf, distinct, repeat):
    """int64 keys, 20000 left rows, half of them hitting; up to SJ_LDS_C distinct keys the LDS route, beyond it the global route --
    also when every key stands 16 times, where the count of distinct keys is measured after the build and the table rebuilt small"""
    if distinct == 100_000 and repeat == 16:
        distinct = 20_000                                                            # (320000 right rows; enough beyond the bound)
    rng = np.random.default_rng(distinct * 31 + repeat)
    left, right = _half_hitting(distinct, 20_000, rng, repeat=repeat)
    p = Pair([(left, None)], [(right, None)])
    for anti, nulls_equal in FLAG_COMBOS:
        gdf.libgdf.gdf_amd_debug_noted(None, None)
        prof = gk.profile_of(gdf, lambda: p.check(gdf, anti, nulls_equal, what=f"{distinct} distinct x {repeat}"))
        assert note(gdf, "sj_exact") == 1
        if distinct <= LDS_C:
            assert note(gdf, "sj_route") == ROUTE_LDS and "sj_probe_lds" in prof and "sj_probe" not in prof, sorted(prof)
            assert ("sj_compact" in prof) == (distinct * repeat > LDS_C), sorted(prof)
        else:
            assert note(gdf, "sj_route") == ROUTE_GLOBAL and "sj_probe" in prof and "sj_probe_lds" not in prof, sorted(prof)
        if distinct * repeat > LDS_C:
            assert note(gdf, "sj_distinct") == distinct
        assert {"sj_build", "sj_count", "sj_emit"} <= set(prof), sorted(prof)


def test_right_distinct_counts(gdf):
    for distinct in (1, LDS_C - 1, LDS_C, LDS_C + 1, 100_000):
        for repeat in (1, 16):
            _right_distinct_count(gdf, distinct, repeat)


def test_each_route_forced_gives_the_same_rows(gdf, force_path):
    """GDF_SJ_ROUTE = 1 / 2 / 3 sends one request through the LDS, the global and the WIDE route; the note says which was taken.
    GDF_SJ_LDS_C moves the LDS route's bound: below the count of distinct keys it sends the shipped call to the global route"""
    rng = np.random.default_rng(3)
    for distinct, repeat in ((300, 1), (LDS_C - 1, 4), (LDS_MAX * 2, 1)):      # (a tenth of the right rows is null; the null is a key too)
        left, right = _half_hitting(distinct, 30_000, rng, npt=np.int32, repeat=repeat)   # (33 bits with the null bit: EXACT)
        valid_l, valid_r = rng.random(len(left)) < 0.9, rng.random(len(right)) < 0.9
        p = Pair([(left, valid_l)], [(right, valid_r)], seed=distinct)
        for anti, nulls_equal in FLAG_COMBOS:
            shipped = p.check(gdf, anti, nulls_equal, what="shipped")
            assert note(gdf, "sj_route") == (ROUTE_LDS if distinct <= LDS_C else ROUTE_GLOBAL)
            if distinct == 300:
                force_path("GDF_SJ_LDS_C", 200)
                np.testing.assert_array_equal(p.check(gdf, anti, nulls_equal, what="bound 200"), shipped)
                assert note(gdf, "sj_route") == ROUTE_GLOBAL
                force_path("GDF_SJ_LDS_C", None)
            for forced, name in ((ROUTE_LDS, "sj_probe_lds"), (ROUTE_GLOBAL, "sj_probe"), (ROUTE_WIDE, "sj_probe_wide")):
                force_path("GDF_SJ_ROUTE", forced)
                gdf.libgdf.gdf_amd_debug_noted(None, None)
                prof = gk.profile_of(gdf, lambda: np.testing.assert_array_equal(p.check(gdf, anti, nulls_equal, what=f"route {forced}"), shipped))
                # (more distinct keys than one workgroup's LDS holds: the forced LDS route cannot be taken)
                taken = ROUTE_GLOBAL if forced == ROUTE_LDS and distinct > LDS_MAX else forced
                assert note(gdf, "sj_route") == taken
                assert (name if taken == forced else "sj_probe") in prof, sorted(prof)
                force_path("GDF_SJ_ROUTE", None)


# ---- dtypes ------------------------------------------------------------------------------------------------------------------------------
KEY_DTYPES = [("int8", np.int8, 1), ("int16", np.int16, 2), ("int32", np.int32, 3), ("int64", np.int64, 4), ("float32", np.float32, 5),
              ("float64", np.float64, 6), ("date32", np.int32, 7), ("date64", np.int64, 8), ("timestamp", np.int64, 9)]


def _nans(npt):
    if np.dtype(npt) == np.float32:
        return np.array([0x7FC00000, 0xFFC00001], dtype=np.uint32).view(np.float32)
    return np.array([0x7FF8000000000000, 0xFFF8000000000001], dtype=np.uint64).view(np.float64)


def _draw_pool(npt, rng):
    """200 distinct values of the dtype with its extremes among them"""
    if np.dtype(npt).kind == "f":
        pool = np.unique((rng.standard_normal(300) * 1e3).astype(npt))[:192]
        return np.concatenate([pool, np.array([np.inf, -np.inf, 0.0, 5e-324, -5e-324, np.finfo(npt).max, np.finfo(npt).min, 1.0], dtype=npt)])
    info = np.iinfo(npt)
    if info.bits == 8:
        return rng.permutation(np.arange(-128, 128)).astype(npt)[:200]
    pool = np.unique(rng.integers(info.min, info.max, size=300, dtype=npt, endpoint=True))[:196]
    return np.unique(np.concatenate([pool, np.array([info.min, info.max, -1, 0], dtype=npt)]))


def _key_dtype_with_and_without_masks(gdf, name, npt, gdf_dtype):
    """4097 left rows drawn from a pool of about 200 values with the dtype's extremes, half of the pool on the right side; floats with
    NaNs of two payloads on both sides"""
    rng = np.random.default_rng(gdf_dtype)
    pool = rng.permutation(_draw_pool(npt, rng))
    right = np.repeat(pool[:len(pool) // 2], 3)
    left = pool[rng.integers(0, len(pool), size=4097)]
    if np.dtype(npt).kind == "f":
        left[rng.integers(0, 4097, size=40)] = np.tile(_nans(npt), 20)
        right = np.concatenate([right, _nans(npt)])
    right = rng.permutation(right)
    for masked in (False, True):
        lv = rng.random(len(left)) < 0.7 if masked else None
        rv = rng.random(len(right)) < 0.7 if masked else None
        Pair([(left, lv)], [(right, rv)], dtypes=[gdf_dtype], seed=gdf_dtype).check_all_flags(gdf, what=f"{name}, masked {masked}")


def test_every_key_dtype_with_and_without_masks(gdf):
    for name, npt, gdf_dtype in KEY_DTYPES:
        _key_dtype_with_and_without_masks(gdf, name, npt, gdf_dtype)


def test_int64_extremes(gdf):
    """keys among {INT64_MIN, -1, 0, INT64_MAX}: every subset of them as the right side.  -1 is the image the table's empty marker has"""
    values = np.array([I64.min, -1, 0, I64.max], dtype=np.int64)
    rng = np.random.default_rng(11)
    left = values[rng.integers(0, 4, size=1000)]
    for subset in range(1, 15):
        right = np.repeat(values[[i for i in range(4) if subset >> i & 1]], 2)
        for masked in (False, True):
            lv = rng.random(1000) < 0.8 if masked else None
            rv = np.arange(len(right)) % 2 == 0 if masked else None                  # every value once valid, once null
            Pair([(left, lv)], [(right, rv)], seed=subset).check_all_flags(gdf, what=f"subset {subset:04b}, masked {masked}")


def _reserved_image(gdf, force_path, shape):
    """64-bit EXACT keys whose every element is -1 (the image that marks an empty slot) or 0, next to others: with -1 on the right
    side only, with 0 only, with both, with neither -- on the LDS and on the global route"""
    ncols, npt = {"eight_int8": (8, np.int8), "one_int64": (1, np.int64), "two_int32": (2, np.int32)}[shape]
    rng = np.random.default_rng(ncols)
    kinds = rng.integers(0, 4, size=3000)                                            # all -1, all 0, mixed -1 / 0, a constant 7
    mixed = np.array([-1, 0] * 4, dtype=npt)[:ncols] if ncols > 1 else np.array([1], dtype=npt)
    protos = np.stack([np.full(ncols, -1, dtype=npt), np.zeros(ncols, dtype=npt), mixed, np.full(ncols, 7, dtype=npt)])
    left = [(protos[kinds, c].copy(), None) for c in range(ncols)]
    for present in ([0], [1], [0, 1], [2], [0, 2, 3], [1, 2]):
        right = [(np.repeat(protos[present, c], 2), None) for c in range(ncols)]
        p = Pair(left, right)
        for forced in (None, ROUTE_GLOBAL):
            force_path("GDF_SJ_ROUTE", forced)
            for anti, nulls_equal in FLAG_COMBOS:
                got = p.check(gdf, anti, nulls_equal, what=f"{shape}, right holds {present}")
                assert note(gdf, "sj_exact") == 1
                assert set(np.unique(kinds[got])) == ({0, 1, 2, 3} - set(present) if anti else set(present))
        force_path("GDF_SJ_ROUTE", None)


def test_the_reserved_image(gdf, force_path):
    for shape in ("eight_int8", "one_int64", "two_int32"):
        _reserved_image(gdf, force_path, shape)


def _floats_zeros_nans_infinities(gdf, npt):
    """-0.0 only on the left and +0.0 only on the right (they match); NaNs of two payloads on both sides (they never do); +inf on both
    sides, -inf on the left only"""
    nan_a, nan_b = _nans(npt)
    rng = np.random.default_rng(5)
    pool = np.array([-0.0, nan_a, nan_b, np.inf, -np.inf, 1.5, -2.5, 3.0], dtype=npt)
    left = pool[rng.integers(0, len(pool), size=5000)]
    right = np.array([0.0, nan_a, nan_b, nan_a, np.inf, 1.5, 99.0], dtype=npt)
    assert not np.signbit(right[0]) and np.signbit(left[left == 0]).all()
    for masked in (False, True):
        lv = rng.random(5000) < 0.8 if masked else None
        p = Pair([(left, lv)], [(right, None)])
        for anti, nulls_equal in FLAG_COMBOS:
            got = p.check(gdf, anti, nulls_equal, what=f"masked {masked}")
            ok = np.ones(len(got), dtype=bool) if lv is None else lv[got]
            vals = left[got][ok]
            if anti:
                assert np.isnan(vals).any() and (vals == -np.inf).any() and not (vals == 0).any() and not (vals == np.inf).any()
            else:
                assert not np.isnan(vals).any() and (vals == 0).any() and (vals == np.inf).any() and (vals == 1.5).any()
    # the same as the second column of a two-column key (an int8 in front: 40 / 72 bits, EXACT and WIDE)
    front_l, front_r = rng.integers(0, 2, size=5000).astype(np.int8), np.zeros(len(right), dtype=np.int8)
    Pair([(front_l, None), (left, None)], [(front_r, None), (right, None)]).check_all_flags(gdf, what="two columns")


def test_floats_zeros_nans_infinities(gdf):
    for npt in (np.float32, np.float64):
        _floats_zeros_nans_infinities(gdf, npt)


def test_a_null_never_meets_the_value_zero(gdf):
    """under NULLS_EQUAL the null's value field is 0 in the image: nulls on one side against the value 0 on the other must not match,
    nulls against nulls must"""
    rng = np.random.default_rng(9)
    left = rng.integers(0, 3, size=3000).astype(np.int32)
    lv = rng.random(3000) < 0.6
    for right, rv in ((np.array([0, 0, 2], dtype=np.int32), None),                   # the value 0, no null
                      (np.array([5, 2], dtype=np.int32), np.array([False, True])),     # a null, no 0
                      (np.array([0, 7, 2], dtype=np.int32), np.array([True, False, True]))):
        p = Pair([(left, lv), (left, None)], [(right, rv), (right, None)])
        p.check_all_flags(gdf, what="null against 0")
        q = Pair([(left, None)], [(right, rv)])                                       # (the mask on the right side only)
        q.check_all_flags(gdf, what="null against 0, unmasked left")


# ---- WIDE keys ---------------------------------------------------------------------------------------------------------------------------
def _wide_keys_that_differ_in_the_last_column_only(gdf, force_path, shape, tag_bits):
    """keys beyond 64 bits whose rows agree in every column but the last: only the verification against the columns tells them apart.
    With a 4-bit tag nearly every left row meets foreign keys with its tag on its way through the table"""
    rng = np.random.default_rng(16)
    if shape == "three_columns":                                                     # int64, float64, int32: 160 bits
        last_l, last_r = _half_hitting(50_000, 100_000, rng, npt=np.int32)
        n_l, n_r = len(last_l), len(last_r)
        left = [(np.full(n_l, I64.min, dtype=np.int64), None), (np.full(n_l, -0.0), None), (last_l, rng.random(n_l) < 0.9)]
        right = [(np.full(n_r, I64.min, dtype=np.int64), None), (np.zeros(n_r), None), (last_r, rng.random(n_r) < 0.9)]
    else:                                                                            # sixteen int8: 128 bits, 256 possible keys
        last_r = np.repeat(rng.permutation(np.arange(-128, 128))[:100].astype(np.int8), 5)
        last_l = rng.integers(-128, 128, size=20_000).astype(np.int8)
        left = [(np.full(len(last_l), -1, dtype=np.int8), None) for _ in range(15)] + [(last_l, rng.random(len(last_l)) < 0.9)]
        right = [(np.full(len(last_r), -1, dtype=np.int8), None) for _ in range(15)] + [(last_r, None)]
    p = Pair(left, right)
    force_path("GDF_SJ_TAG_BITS", tag_bits)
    for anti, nulls_equal in FLAG_COMBOS:
        gdf.libgdf.gdf_amd_debug_noted(None, None)
        prof = gk.profile_of(gdf, lambda: p.check(gdf, anti, nulls_equal, what=f"{shape}, tag bits {tag_bits}"))
        assert note(gdf, "sj_route") == ROUTE_WIDE and note(gdf, "sj_exact") == 0
        assert {"sj_build_wide", "sj_probe_wide"} <= set(prof) and "sj_build" not in prof, sorted(prof)


def test_wide_keys_that_differ_in_the_last_column_only(gdf, force_path):
    for shape in ("three_columns", "sixteen_columns"):
        for tag_bits in (4, None):
            _wide_keys_that_differ_in_the_last_column_only(gdf, force_path, shape, tag_bits)


# ---- mask kinds on either side -----------------------------------------------------------------------------------------------------------
def _mask_kinds(gdf, left_mask, right_mask):
    """two columns (int16, float32 -- 48 bits, 50 with both null bits), 1001 left and 301 right rows, the first column masked on either
    side independently, the second "half" masked on both"""
    rng = np.random.default_rng(len(left_mask) * 16 + len(right_mask))
    nl, nr = 1001, 301
    la, ra = rng.integers(0, 6, size=nl).astype(np.int16), rng.integers(0, 4, size=nr).astype(np.int16)
    lb, rb = rng.integers(0, 3, size=nl).astype(np.float32), rng.integers(0, 2, size=nr).astype(np.float32)
    extreme = left_mask in EXTREME_MASKS or right_mask in EXTREME_MASKS
    for second_masked in (False, True):
        lv2 = rng.random(nl) < 0.5 if second_masked else None
        rv2 = rng.random(nr) < 0.5 if second_masked else None
        p = Pair([(la, make_valid(left_mask, nl, rng)), (lb, lv2)], [(ra, make_valid(right_mask, nr, rng)), (rb, rv2)], seed=nl)
        p.check_all_flags(gdf, what=f"{left_mask} x {right_mask}", extreme=extreme)


def test_mask_kinds_on_either_side(gdf):
    for left_mask in MASKS:
        for right_mask in MASKS:
            _mask_kinds(gdf, left_mask, right_mask)


# ---- empty sides -------------------------------------------------------------------------------------------------------------------------
def test_empty_sides(gdf):
    some = (np.arange(700, dtype=np.int32), np.arange(700) % 3 != 0)
    none = (np.zeros(0, dtype=np.int32), None)
    for anti, nulls_equal in FLAG_COMBOS:
        got = Pair([some], [none]).check(gdf, anti, nulls_equal, what="no right rows", extreme=True)
        np.testing.assert_array_equal(got, np.arange(700, dtype=np.int32) if anti else np.zeros(0, dtype=np.int32))
        assert note(gdf, "sj_route") == ROUTE_NONE
        assert len(Pair([none], [some]).check(gdf, anti, nulls_equal, what="no left rows", extreme=True)) == 0
        assert len(Pair([none], [none]).check(gdf, anti, nulls_equal, what="no rows", extreme=True)) == 0


# ---- the second oracle: the library's own inner join -------------------------------------------------------------------------------------
def test_against_the_inner_join(gdf):
    """flags == 0: the rows are unique(left indices of gdf_inner_join) on the same columns, ANTI their complement; and gather of the
    result is the filtered table in input order"""
    import torch
    rng = np.random.default_rng(21)
    rows = 100_000
    for ncols in (1, 2):
        la, ra = _half_hitting(5_000, rows, rng, npt=np.int32, repeat=4)
        left = [(la, rng.random(rows) < 0.9)]
        right = [(ra, rng.random(len(ra)) < 0.9)]
        if ncols == 2:
            left.append((rng.integers(0, 2, size=rows).astype(np.float64), rng.random(rows) < 0.9))
            right.append((rng.integers(0, 2, size=len(ra)).astype(np.float64), None))
        p = Pair(left, right, seed=ncols)
        semi, anti = p.check(gdf, False, False, what="semi"), p.check(gdf, True, False, what="anti")
        li, _ = gdf.api.join(p.ldev, p.rdev, how="inner")
        assert li.numel() > len(semi)                                                 # (the join emits a pair per partner)
        joined = torch.unique(li).cpu().numpy()
        np.testing.assert_array_equal(semi, joined)
        np.testing.assert_array_equal(anti, np.setdiff1d(np.arange(rows, dtype=np.int32), joined))
    payload = [(rng.standard_normal(rows), rng.random(rows) < 0.7)]
    idx = gdf.api.semi_join(p.ldev, p.rdev)
    outs = gdf.api.gather(idx, p.ldev + [orf.device_column(d, v) for d, v in payload])
    want = orf.gather(semi, p.left + payload)
    for o, (data, ok, mask, nulls) in zip(outs, want):
        np.testing.assert_array_equal(o.valid.cpu().numpy(), mask)
        np.testing.assert_array_equal(orf.bits_of(o.to_numpy())[ok], orf.bits_of(data)[ok])
        assert int(o.c.null_count) == nulls
