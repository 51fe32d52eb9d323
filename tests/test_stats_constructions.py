"""The constructions of tests/stats_common.py checked without a GPU (as test_radixsort_reference.py does for the sort tests): the
key image, the columns that part ranks k and k + 1 at a chosen digit, the columns that fill chosen regions of the candidate buffer,
the host model of the selection, and the note channel of the test-hook library.  No kernel runs here: a GPU test that believes it
forces a route is only as good as the input it builds."""
import ctypes as C
import os

import numpy as np
import pytest

import stats_common as sc
from stats_reference import quantile_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "libgdf_amd", "lib")
IDS = lambda d: np.dtype(d).name            # noqa: E731
LEVELS = [(d, l) for d in sc.ALL_DTYPES for l in range(1, len(sc.digit_plan(np.dtype(d).itemsize * 8)) + 1)]


def _edge_values(dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(dt.itemsize)
    if dt.kind == "i":
        info = np.iinfo(dt)
        a = np.concatenate([np.array([info.min, info.min + 1, -1, 0, 1, info.max - 1, info.max], dtype=dt),
                            rng.integers(info.min, int(info.max) + 1, size=2000, dtype=np.int64).astype(dt)])
    else:
        fi = np.finfo(dt)
        tiny = np.nextafter(dt.type(0), dt.type(1))
        a = np.concatenate([np.array([-np.inf, fi.min, -1.0, -fi.tiny, -tiny, -0.0, 0.0, tiny, fi.tiny, 1.0, fi.max, np.inf], dtype=dt),
                            (rng.standard_normal(2000) * 1e3).astype(dt), (rng.standard_normal(200) * 1e-40).astype(dt)])
    return a


@pytest.mark.parametrize("dtype", sc.ALL_DTYPES, ids=IDS)
def test_key_image_is_strictly_monotone_and_invertible(dtype):
    dt = np.dtype(dtype)
    a = _edge_values(dtype)
    # distinct as BIT PATTERNS, sorted by value with -0.0 before +0.0
    bits = np.unique(sc.bits_of(a))
    a = bits.view(dt)
    s = a[np.lexsort((~np.signbit(a), a))] if dt.kind == "f" else np.sort(a)
    k = sc.key_image(s)
    assert k.dtype == np.uint64 and int(k.max()) < 1 << (dt.itemsize * 8)
    assert np.all(k[1:] > k[:-1]), "the image must be strictly increasing on distinct sorted values"
    back = sc.from_key_image(k, dt)
    assert back.dtype == dt and np.array_equal(sc.bits_of(back), sc.bits_of(s)), "from_key_image must invert key_image bit for bit"
    if dt.kind == "f":
        z = sc.key_image(np.array([-0.0, 0.0], dtype=dt))
        assert z[0] + 1 == z[1], "-0.0 sits right below +0.0"
        inf = sc.key_image(np.array([np.inf], dtype=dt))[0]
        assert inf < (1 << (dt.itemsize * 8)) - 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=IDS)
def test_every_nan_pattern_maps_to_the_all_ones_key(dtype):
    dt = np.dtype(dtype)
    nans = sc.nan_values(dt)
    assert len(nans) == 8 and np.isnan(nans).all()
    assert len(set(sc.bits_of(nans).tolist())) == 8, "the patterns must survive the trip into the float type"
    assert np.count_nonzero(np.signbit(nans)) == 4
    ones = (1 << (dt.itemsize * 8)) - 1
    assert (sc.key_image(nans) == np.uint64(ones)).all()
    assert np.isnan(sc.from_key_image(np.array([ones], dtype=np.uint64), dt)[0])
    # ... and above +inf, which is the largest other key
    assert sc.key_image(np.array([np.inf], dtype=dt))[0] < ones


def test_digit_plan():
    assert sc.digit_plan(64) == [(53, 11), (42, 11), (31, 11), (20, 11), (9, 11), (0, 9)]
    assert sc.digit_plan(32) == [(21, 11), (10, 11), (0, 10)]
    assert sc.digit_plan(16) == [(5, 11), (0, 5)]
    assert sc.digit_plan(8) == [(0, 8)]


def _parting_facts(dtype, level, values, q):
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    n = len(values)
    s = np.sort(values)
    keys = sc.key_image(s)
    assert np.all(keys[1:] >= keys[:-1])
    d = sc.digits(keys, bits)
    k = sc.rank_of_q(n, q)
    return s, keys, d, k


@pytest.mark.parametrize("dtype,level", LEVELS, ids=lambda v: np.dtype(v).name if isinstance(v, type) else str(v))
def test_parting_column_has_its_stated_properties(dtype, level):
    dt = np.dtype(dtype)
    n = 4096
    values, q = sc.parting_column(dtype, level, n, np.random.default_rng(100 * dt.itemsize + level))
    assert values.dtype == dt and len(values) == n
    assert not np.array_equal(values, np.sort(values)), "the column is shuffled"
    s, keys, d, k = _parting_facts(dtype, level, values, q)
    plan = sc.digit_plan(dt.itemsize * 8)
    shift = plan[level - 1][0]
    last = level == len(plan)
    assert q == (k + 1.5) / n and q * n - np.floor(q * n) == 0.5
    L = level - 1
    assert np.array_equal(d[k, :L], d[k + 1, :L]), "ranks k and k + 1 share every digit above the level"
    assert d[k + 1, L] >= d[k, L] + 2, "they differ at the level, with an empty bucket in between"
    inA = (d[:, :L + 1] == d[k, :L + 1]).all(axis=1)
    inB = (d[:, :L + 1] == d[k + 1, :L + 1]).all(axis=1)
    between = (d[:, :L] == d[k, :L]).all(axis=1) & (d[:, L] > d[k, L]) & (d[:, L] < d[k + 1, L])
    assert not between.any()
    assert keys[k] == keys[inA].max() and np.flatnonzero(inA).max() == k, "rank k is the largest key of its bucket"
    assert keys[k + 1] == keys[inB].min() and np.flatnonzero(inB).min() == k + 1
    if last:
        assert np.count_nonzero(inB) >= 3
    else:
        assert len(np.unique(keys[inB])) >= 3 and keys[k + 2] > keys[k + 1]
    low = np.uint64((1 << shift) - 1)
    if level >= 2:
        same_digit = d[:, L] == d[k + 1, L]
        other_prefix = ~(d[:, :L] == d[k + 1, :L]).all(axis=1)
        smaller_low = (keys & low) < (keys[k + 1] & low) if not last else np.ones(n, dtype=bool)
        decoy = same_digit & other_prefix & smaller_low
        assert decoy.any(), "a decoy with rank k + 1's digit, another prefix and smaller low bits"
        assert (decoy & (keys < keys[k + 1])).any() and (decoy & (keys > keys[k + 1])).any(), "decoys on both sides"
    top = d[:, 0] == d[k, 0]
    assert np.count_nonzero(top) * 2 <= n, "at most half of the column shares rank k's top digit: compaction is attempted"
    # the rule reads both ranks: every exact method gives another value than it would for a neighbouring pair
    assert quantile_rule(s, q, "LOWER") == float(s[k]) and quantile_rule(s, q, "HIGHER") == float(s[k + 1])
    assert s[k] != s[k + 1]


@pytest.mark.parametrize("dtype,level", LEVELS, ids=lambda v: np.dtype(v).name if isinstance(v, type) else str(v))
def test_selection_model_agrees_with_sorting_on_parting_columns(dtype, level):
    """the host model of DESIGN §11's search finds ranks k and k + 1 of every parting column, on both routes; with the candidate
    buffer allowed and level >= 3 it ends on the candidates"""
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    values, q = sc.parting_column(dtype, level, 4096, np.random.default_rng(100 * dt.itemsize + level))
    s, keys, d, k = _parting_facts(dtype, level, values, q)
    unsorted = sc.key_image(values)
    for allow in (True, False):
        m = sc.select_model(unsorted, bits, k, allow_compact=allow)
        assert m["ok"] and m["key0"] == int(keys[k]) and m["key1"] == int(keys[k + 1]), (allow, m)
        if allow and level >= 3:
            assert m["src"] == 1
        if not allow:
            assert m["src"] == 0 and m["column_passes"] >= min(level + 1, len(sc.digit_plan(bits)))
    m = sc.select_model(unsorted, bits, k, one=True)
    assert m["ok"] and m["key0"] == int(keys[k])


@pytest.mark.parametrize("dtype,level", [(d, l) for d, l in LEVELS if l >= 2],
                         ids=lambda v: np.dtype(v).name if isinstance(v, type) else str(v))
def test_decoys_catch_a_mask_that_forgets_the_higher_digits(dtype, level):
    """D3's check of itself: rank k + 1 is the smallest key matching prefix_b in the bits >= hi_b.  A search whose mask compares
    only the digit at hi_b (the higher bits forgotten) still answers correctly on a column WITHOUT decoys that has no other key
    with that digit -- and answers with a decoy on the column parting_column builds.  At the last level the digit alone decides
    rank k + 1 (no min pass), so the wrong mask is never consulted there."""
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    plan = sc.digit_plan(bits)
    digit_only = lambda hi_b, width: ((1 << width) - 1) << hi_b           # noqa: E731
    seed = 100 * dt.itemsize + level
    values, q = sc.parting_column(dtype, level, 4096, np.random.default_rng(seed))
    s, keys, d, k = _parting_facts(dtype, level, values, q)
    uk = sc.key_image(values)
    L = level - 1
    # (level 2 with the candidate buffer: the buffer holds rank k's top-digit bucket only, the decoys of level 2 differ in the top
    # digit and are not in it -- there the forced column route is the one that meets them; D3 runs both routes)
    for allow in ((False,) if level == 2 else (True, False)):
        good = sc.select_model(uk, bits, k, allow_compact=allow)
        bad = sc.select_model(uk, bits, k, allow_compact=allow, mb_mask=digit_only)
        assert good["key1"] == int(keys[k + 1]) and bad["key0"] == int(keys[k])
        if level == len(plan):
            assert bad["key1"] == good["key1"]
            continue
        assert bad["key1"] != good["key1"], "the wrong mask must change rank k + 1"
        wrong = np.flatnonzero(keys == np.uint64(bad["key1"]))
        assert len(wrong) and d[wrong[0], L] == d[k + 1, L] and not np.array_equal(d[wrong[0], :L], d[k + 1, :L]), "... to a decoy"
    if level == len(plan):
        return
    # the same column with every key of that digit outside rank k + 1's bucket removed (replaced by copies of the smallest key):
    # the wrong mask goes unnoticed
    ud = sc.digits(uk, bits)
    stray = (ud[:, L] == d[k + 1, L]) & ~(ud[:, :L] == d[k + 1, :L]).all(axis=1)
    assert stray.any()
    uk2 = uk.copy()
    uk2[stray] = uk.min()
    s2 = np.sort(uk2)
    k2 = int(np.searchsorted(s2, keys[k], side="right")) - 1
    blind = sc.select_model(uk2, bits, k2, allow_compact=False, mb_mask=digit_only)
    assert blind["key0"] == int(s2[k2]) and blind["key1"] == int(s2[k2 + 1]), "without decoys the wrong mask is invisible"


OVERFLOW_CASES = [(np.int32, 1 << 23), (np.int64, (1 << 22) + (1 << 20)), (np.float64, (1 << 22) + (1 << 20))]


def _layout_counts(dtype, values, D):
    dt = np.dtype(dtype)
    shift = sc.digit_plan(dt.itemsize * 8)[0][0]
    keys = sc.key_image(values)
    target = (keys >> np.uint64(shift)) == np.uint64(D)
    V = 16 // dt.itemsize
    pos = np.flatnonzero(target)
    n = len(values)
    nvec = n // V
    region = np.where(pos < nvec * V, (pos // V) % 256, (pos - nvec * V) % 256)        # from positions alone
    return keys, target, np.bincount(region, minlength=256)


@pytest.mark.parametrize("dtype,n", OVERFLOW_CASES, ids=lambda v: np.dtype(v).name if isinstance(v, type) else str(v))
def test_region_layout_overflow_case(dtype, n):
    """D1's input: region 0 is filled with keys of one top-digit bucket and holds more than rs of them; the model then leaves the
    candidate buffer (src 0, compaction withdrawn, one more column pass than the shuffled control, which ends on candidates).
    With the overflow branch disabled the model continues on a buffer that lost keys: the notes change for certain (src 1), the
    answers as well where half of the bucket is lost (int32)."""
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    rs = sc.region_size(n)
    assert rs == 16384 == -(-min(n, 1 << 22) // 256)
    rng = np.random.default_rng(n % 1000 + dt.itemsize)
    values, q, D = sc.region_layout(dtype, n, n // 256, [0], rng)
    assert len(values) == n and values.dtype == dt
    keys, target, counts = _layout_counts(dtype, values, D)
    assert counts[0] == n // 256 > rs and not counts[1:].any()
    assert len(np.unique(keys[target])) == n // 256, "the bucket's keys are distinct"
    assert np.count_nonzero(target) * 2 <= 256 * rs, "the bucket fills at most half the buffer: compaction is attempted"
    s = np.sort(keys)
    k = sc.rank_of_q(n, q)
    lo, hi = np.searchsorted(s, keys[target].min()), np.searchsorted(s, keys[target].max())
    assert lo + 100 < k < hi - 100, "rank k sits inside the bucket, away from its ends"
    m = sc.select_model(keys, bits, k)
    assert m["ok"] and (m["key0"], m["key1"]) == (int(s[k]), int(s[k + 1]))
    assert m["src"] == 0 and m["allow_compact"] == 0
    shuffled = rng.permutation(keys)
    c = sc.select_model(shuffled, bits, k)
    assert c["ok"] and (c["key0"], c["key1"]) == (int(s[k]), int(s[k + 1])) and c["src"] == 1 and c["allow_compact"] == 1
    assert m["column_passes"] > c["column_passes"]
    broken = sc.select_model(keys, bits, k, overflow_branch=False)
    assert broken["src"] == 1, "the disabled branch goes on with the candidates"
    if n // 256 >= 2 * rs:
        # half of the bucket's keys are lost: about 16 keys share rank k's second digit and half of them are gone
        assert not broken["ok"] or (broken["key0"], broken["key1"]) != (int(s[k]), int(s[k + 1]))
    # (the 64-bit cases lose 4096 of 20480 keys and decide the ranks among the ~10 keys that share the second digit: the answers
    # survive whenever none of the lost keys is one of those below rank k + 1, so there only the notes are certain to change)


def test_region_layout_boundary_cases():
    """D2's inputs: exactly rs keys in region 0 (no overflow: ends on candidates), rs + 1 (overflow), and rs in region 0 with
    rs + 1 in region 255 (the last lane of the overflow check)"""
    n, dt, bits = 1 << 23, np.dtype(np.int32), 32
    rs = sc.region_size(n)
    for per, regions, src in ((rs, [0], 1), (rs + 1, [0], 0), ([rs, rs + 1], [0, 255], 0), ([rs, rs], [0, 255], 1)):
        rng = np.random.default_rng(7)
        values, q, D = sc.region_layout(dt, n, per, regions, rng)
        keys, target, counts = _layout_counts(dt, values, D)
        want = np.zeros(256, dtype=np.int64)
        want[regions] = per
        assert np.array_equal(counts, want)
        assert np.count_nonzero(target) * 2 <= 256 * rs
        s = np.sort(keys)
        k = sc.rank_of_q(n, q)
        m = sc.select_model(keys, bits, k)
        assert m["ok"] and (m["key0"], m["key1"]) == (int(s[k]), int(s[k + 1])) and m["src"] == src, (per, regions, m)
        assert m["allow_compact"] == src


def test_region_of_positions_with_a_head():
    # int32 column whose first aligned element is element 3: elements 0..2 are loose (regions 0..2), element 3 starts vector 0
    reg = sc.region_of_positions(3 + 4 * 300 + 2, 4, head=3)
    assert list(reg[:3]) == [0, 1, 2] and list(reg[3:7]) == [0] * 4 and list(reg[7:11]) == [1] * 4
    assert list(reg[3 + 4 * 256: 3 + 4 * 257]) == [0] * 4
    assert list(reg[-2:]) == [3, 4], "tail elements continue the loose numbering behind the head"


@pytest.fixture(scope="module")
def hook():
    lib = C.CDLL(os.path.join(LIBDIR, "libgdf_testhook.so"), mode=C.RTLD_GLOBAL)
    lib.gdf_amd_debug_noted.restype = C.c_int
    lib.gdf_amd_debug_noted.argtypes = [C.c_char_p, C.POINTER(C.c_longlong)]
    lib.gdf_amd_testhook_note.restype = None
    lib.gdf_amd_testhook_note.argtypes = [C.c_char_p, C.c_longlong]
    lib.gdf_amd_debug_force.restype = C.c_int
    lib.gdf_amd_debug_force.argtypes = [C.c_char_p, C.c_char_p]
    return lib


def test_note_channel(hook):
    v = C.c_longlong(-5)
    assert hook.gdf_amd_debug_noted(None, None) == 0                              # clear
    assert hook.gdf_amd_debug_noted(b"qt.never_noted", C.byref(v)) == 8          # GDF_INVALID_API_CALL
    assert v.value == -5
    assert hook.gdf_amd_debug_noted(None, C.byref(v)) == 8
    hook.gdf_amd_testhook_note(b"qt.src", 1)
    hook.gdf_amd_testhook_note(b"qt.column_passes", 2)
    hook.gdf_amd_testhook_note(b"qt.column_passes", 6)                             # the last value per name
    assert hook.gdf_amd_debug_noted(b"qt.column_passes", C.byref(v)) == 0 and v.value == 6
    assert hook.gdf_amd_debug_noted(b"qt.src", C.byref(v)) == 0 and v.value == 1
    # forcing a path leaves the notes alone
    assert hook.gdf_amd_debug_force(b"GDF_QT_NO_COMPACT", b"1") == 0
    assert hook.gdf_amd_debug_force(b"GDF_QT_NO_COMPACT", None) == 0
    assert hook.gdf_amd_debug_noted(b"qt.src", C.byref(v)) == 0 and v.value == 1
    hook.gdf_amd_testhook_note(None, 9)                                            # ignored
    assert hook.gdf_amd_debug_noted(None, None) == 0
    assert hook.gdf_amd_debug_noted(b"qt.src", C.byref(v)) == 8


def test_binding_routes_the_note_reader_to_the_hook_library():
    """libgdf_amd._binding: gdf_amd_debug_noted, like gdf_amd_debug_force, lives in libgdf_testhook.so (conftest.py asks for it)"""
    import libgdf_amd
    v = C.c_longlong(0)
    assert libgdf_amd.libgdf.gdf_amd_debug_noted(b"qt.no_such_note", C.byref(v)) == 8
    with pytest.raises(AttributeError):
        libgdf_amd.libgdf.raw("gdf_amd_debug_noted")                               # not an export of libgdf.so
