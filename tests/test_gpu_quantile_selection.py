"""The radix selection of csrc/quantile.hip on inputs built to take one route each (tests/stats_common.py; the constructions are
checked without a GPU in test_stats_constructions.py): a candidate-buffer region that overflows, the boundary of that, ranks k and
k + 1 parting at every digit with decoys, one deep bucket, and every flavour of NaN.  Expected values come from
stats_reference.quantile_rule on np.sort(a) only; which route a search took is read from the note channel of the test-hook library
(qt.column_passes, qt.src, qt.allow_compact), so a test that no longer reaches its route fails instead of passing quietly."""
import ctypes as C

import numpy as np
import pytest

import stats_common as sc
from stats_reference import QUANTILE_METHODS, quantile_rule, same

pytestmark = pytest.mark.gpu

METHODS = [None] + list(range(len(QUANTILE_METHODS)))
IDS = lambda v: np.dtype(v).name if isinstance(v, type) else str(v)          # noqa: E731
LEVELS = [(d, l) for d in sc.ALL_DTYPES for l in range(1, len(sc.digit_plan(np.dtype(d).itemsize * 8)) + 1)]


def _call(gdf, col, q, method, flag_sorted=0, inplace=0):
    from libgdf_amd.columns import GDF_TO_NP, new_context
    ctx = new_context(flag_sorted=flag_sorted, method=0, flag_sort_inplace=inplace)
    if method is None:
        res = np.zeros(1, dtype=GDF_TO_NP[int(col.c.dtype)])
        gdf.libgdf.gdf_quantile_aprrox(col.ptr, q, res.ctypes.data, C.byref(ctx))
        return res[0]
    res = C.c_double(0.0)
    gdf.libgdf.gdf_quantile_exact(col.ptr, method, q, C.addressof(res), C.byref(ctx))
    return res.value


def _select(gdf, a, s, qs):
    """aprrox and the five exact methods by the radix selection at every q, against the rule on s = np.sort(a); the column must be
    byte-identical afterwards.  Returns the notes of every call: [(q, method, notes)]."""
    import torch
    from libgdf_amd.columns import Column
    t = torch.from_numpy(a).cuda()
    keep = t.clone()
    col = Column(t)
    out = []
    for q in qs:
        for m in METHODS:
            sc.clear_notes(gdf)
            got, want = _call(gdf, col, q, m), quantile_rule(s, q, m)
            if m is None:
                assert np.asarray(got).dtype == s.dtype
            assert same(got, want), (s.dtype, len(s), q, m, got, want)
            if q < 1.0 and len(a) > 1:                       # (q >= 1 is the max reduction: no selection, no notes)
                out.append((q, m, sc.read_notes(gdf)))
    assert torch.equal(t.view(torch.uint8), keep.view(torch.uint8)), "the selection modified the column"
    return out


def _each(notes, name):
    return [nt[name] for _, _, nt in notes]


def _assert_route_as_modelled(a, notes, allow_compact):
    """the notes of every call equal what the host model of DESIGN §11 (stats_common.select_model) predicts for the column"""
    bits = a.dtype.itemsize * 8
    keys = sc.key_image(a)
    cache = {}
    for q, m, nt in notes:
        key = (q, m is None)
        if key not in cache:
            r = sc.select_model(keys, bits, sc.rank_of_q(len(a), q), one=m is None, allow_compact=allow_compact)
            cache[key] = {"qt.column_passes": r["column_passes"], "qt.src": r["src"], "qt.allow_compact": r["allow_compact"]}
        assert nt == cache[key], (a.dtype, q, m, nt, cache[key])


# ---------------------------------------------------------------------------------------------------------------------------------
# D1 / D2: a region of the candidate buffer overflows -- or just does not

# the smallest sizes at which a region can overflow at all: rs = 2^22 / 256 = 16384 keys, a region receives n / 256
OVERFLOW_CASES = [(np.int32, 1 << 23), (np.int64, (1 << 22) + (1 << 20)), (np.float64, (1 << 22) + (1 << 20))]


@pytest.mark.parametrize("dtype,n", OVERFLOW_CASES, ids=IDS)
def test_region_overflow_falls_back_to_column_passes(gdf, dtype, n):
    """region 0 receives n / 256 keys of rank k's bucket (32768 for int32, 20480 for the 64-bit types; rs = 16384): the search must
    withdraw the compaction and go on with filtered column passes.  Control: the same values shuffled end on the candidates."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(n % 1000 + dt.itemsize)
    a, q, _ = sc.region_layout(dtype, n, n // 256, [0], rng)
    assert n // 256 > sc.region_size(n) == 16384
    s = np.sort(a)
    over = _select(gdf, a, s, [q])
    print("overflow", dt.name, n, over[0][2], over[-1][2])
    assert _each(over, "qt.src") == [0] * len(METHODS), "the search must not finish on an incomplete candidate buffer"
    assert _each(over, "qt.allow_compact") == [0] * len(METHODS), "compaction was allowed at the start and must have been withdrawn"
    control = _select(gdf, rng.permutation(a), s, [q])
    print("control", dt.name, n, control[0][2], control[-1][2])
    assert _each(control, "qt.src") == [1] * len(METHODS)
    assert _each(control, "qt.allow_compact") == [1] * len(METHODS)
    for o, c in zip(_each(over, "qt.column_passes"), _each(control, "qt.column_passes")):
        assert o > c, (o, c)


@pytest.mark.parametrize("per,regions,src", [("rs", [0], 1), ("rs+1", [0], 0), (["rs", "rs+1"], [0, 255], 0)], ids=str)
def test_region_boundary(gdf, per, regions, src):
    """exactly rs keys in a region is no overflow (the search ends on the candidates), rs + 1 is; region 255 is the last lane of the
    overflow check"""
    n = 1 << 23
    rs = sc.region_size(n)
    count = {"rs": rs, "rs+1": rs + 1}
    per = count[per] if isinstance(per, str) else [count[p] for p in per]
    a, q, _ = sc.region_layout(np.int32, n, per, regions, np.random.default_rng(7))
    notes = _select(gdf, a, np.sort(a), [q])
    print("boundary", per, regions, notes[0][2], notes[-1][2])
    assert _each(notes, "qt.src") == [src] * len(METHODS)
    assert _each(notes, "qt.allow_compact") == [src] * len(METHODS)


# ---------------------------------------------------------------------------------------------------------------------------------
# D3: ranks k and k + 1 part at every digit

@pytest.mark.parametrize("dtype,level", LEVELS, ids=IDS)
def test_parting_at_every_digit(gdf, force_path, dtype, level):
    dt = np.dtype(dtype)
    a, q = sc.parting_column(dtype, level, 4096, np.random.default_rng(100 * dt.itemsize + level))
    s = np.sort(a)
    notes = _select(gdf, a, s, [q])
    print("parting", dt.name, level, notes[0][2], notes[-1][2])
    _assert_route_as_modelled(a, notes, True)
    assert _each(notes, "qt.allow_compact") == [1] * len(METHODS)
    if level >= 3:
        assert _each(notes, "qt.src") == [1] * len(METHODS), "rank k + 1 must have been found as a min over the candidate buffer"
    force_path("GDF_QT_NO_COMPACT")
    notes = _select(gdf, a, s, [q])
    force_path("GDF_QT_NO_COMPACT", None)
    _assert_route_as_modelled(a, notes, False)
    assert _each(notes, "qt.src") == [0] * len(METHODS) and _each(notes, "qt.allow_compact") == [0] * len(METHODS)


def _both_routes(gdf, force_path, a, qs):
    s = np.sort(a)
    notes = _select(gdf, a, s, qs)
    force_path("GDF_QT_NO_COMPACT")
    forced = _select(gdf, a, s, qs)
    force_path("GDF_QT_NO_COMPACT", None)
    assert _each(forced, "qt.src") == [0] * len(forced)
    _assert_route_as_modelled(a, notes, True)
    _assert_route_as_modelled(a, forced, False)
    return notes, forced


def _q_for_rank(n, k):
    return (k + 1.5) / n


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=IDS)
def test_parting_at_float_specials(gdf, force_path, dtype):
    dt = np.dtype(dtype)
    rng = np.random.default_rng(17)
    n = 4096
    body = (rng.standard_normal(n) * 100).astype(dt)
    # rank k on the last +inf, rank k + 1 a NaN
    a = body.copy()
    a[:40] = np.inf
    a[40:100] = np.nan
    a = rng.permutation(a)
    s = np.sort(a)
    k = n - 60 - 1
    assert np.isinf(s[k]) and np.isnan(s[k + 1])
    _both_routes(gdf, force_path, a, [_q_for_rank(n, k), _q_for_rank(n, k - 40), _q_for_rank(n, k + 1)])
    # rank k on -0.0, rank k + 1 on +0.0 (np.sort is stable about neither: the expected values ignore the sign of a zero, the keys
    # do not -- so the column holds ONE zero of each sign, and negative / positive values around them)
    a = np.abs(body) + dt.type(1)
    a[: n // 2] *= -1
    a[0], a[n - 1] = -0.0, 0.0
    k = n // 2 - 1                       # sorted: n/2 - 1 negatives, then -0.0 at rank n/2 - 1 ... see the assertion
    a = rng.permutation(a)
    s = np.sort(a)
    assert s[k] == 0 and s[k + 1] == 0 and s[k - 1] < 0 < s[k + 2]
    _both_routes(gdf, force_path, a, [_q_for_rank(n, k - 1), _q_for_rank(n, k), _q_for_rank(n, k + 1)])
    import torch
    from libgdf_amd.columns import Column
    col = Column(torch.from_numpy(a).cuda())
    lower, upper = _call(gdf, col, _q_for_rank(n, k), None), _call(gdf, col, _q_for_rank(n, k + 1), None)
    assert lower == 0 and np.signbit(lower) and upper == 0 and not np.signbit(upper), "-0.0 sorts right below +0.0"
    # rank k on the most negative finite value, rank k - 1 on -inf
    a = body.copy()
    a[:30] = -np.inf
    a[30] = np.finfo(dt).min
    a = rng.permutation(a)
    s = np.sort(a)
    k = 30
    assert np.isinf(s[k - 1]) and s[k] == np.finfo(dt).min
    _both_routes(gdf, force_path, a, [_q_for_rank(n, k - 1), _q_for_rank(n, k)])


def test_parting_at_the_int64_sign(gdf, force_path):
    """rank k = -1, rank k + 1 = 0: the sign flip of the key image puts them into different top digits"""
    rng = np.random.default_rng(23)
    n = 4096
    a = rng.integers(-(2**62), 2**62, size=n, dtype=np.int64)
    a[np.abs(a) < 2**40] = 2**40
    a[0], a[1] = -1, 0
    a = rng.permutation(a)
    s = np.sort(a)
    k = int(np.searchsorted(s, -1))
    assert s[k] == -1 and s[k + 1] == 0
    d = sc.digits(sc.key_image(s[k: k + 2]), 64)
    assert d[0, 0] + 1 == d[1, 0]
    _both_routes(gdf, force_path, a, [_q_for_rank(n, k - 1), _q_for_rank(n, k), _q_for_rank(n, k + 1)])


# ---------------------------------------------------------------------------------------------------------------------------------
# D4: one bucket, deep

def _deep_column(dtype, chain):
    dt = np.dtype(dtype)
    n = 4096
    if dt.kind == "i":
        base = {4: 0x12345000, 8: 0x1234567890ABC000}[dt.itemsize] * (1 if chain == "up" else -1)
        return (base + np.arange(n, dtype=np.int64)).astype(dt)
    start = dt.type(1.0 if chain == "up" else -1.0)
    u = {4: np.uint32, 8: np.uint64}[dt.itemsize]
    return (np.array([start], dtype=dt).view(u)[0] + np.arange(n, dtype=u)).view(dt)      # a nextafter chain away from zero


@pytest.mark.parametrize("chain", ["up", "down"])
@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.float32, np.float64], ids=IDS)
def test_one_deep_bucket_reads_the_column_in_every_pass(gdf, force_path, dtype, chain):
    """4096 consecutive keys share every digit but the last two: the bucket's count equals n until then, the candidate buffer is
    never eligible before the last pass, and every pass reads the column"""
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    a = _deep_column(dtype, chain)
    d = sc.digits(sc.key_image(a), bits)
    levels = d.shape[1]
    assert (d[:, : levels - 2] == d[0, : levels - 2]).all() and len(np.unique(d[:, levels - 2])) <= 8
    assert len(np.unique(a)) == len(a) and (dt.kind == "i" or (np.abs(a[1:]) > np.abs(a[:-1])).all())
    a = np.random.default_rng(3).permutation(a)
    n = len(a)
    notes, forced = _both_routes(gdf, force_path, a, [0.0, _q_for_rank(n, 511), 0.5, _q_for_rank(n, n - 2)])
    print("deep", dt.name, chain, notes[0][2], notes[-1][2])
    assert _each(notes, "qt.column_passes") == [levels] * len(notes)
    assert _each(forced, "qt.column_passes") == [levels] * len(forced)


@pytest.mark.parametrize("where", ["below", "above"])
@pytest.mark.parametrize("far", [False, True], ids=["neighbour", "far"])
@pytest.mark.parametrize("dtype", sc.ALL_DTYPES, ids=IDS)
def test_one_value_repeated_with_a_single_other_element(gdf, force_path, dtype, where, far):
    """min == max of the matching keys ends the search -- which must not happen while the one other element is still in the bucket:
    q puts ranks k and k + 1 on either side of it"""
    dt = np.dtype(dtype)
    n = 4096
    rng = np.random.default_rng(dt.itemsize + (where == "below"))
    v = dt.type(100)
    if dt.kind == "i":
        e = dt.type(-100 if where == "below" else 120) if far else dt.type(v - 1 if where == "below" else v + 1)
    else:
        e = dt.type(-3e5 if where == "below" else 3e5) if far else np.nextafter(v, dt.type(-np.inf if where == "below" else np.inf))
    a = np.full(n, v, dtype=dt)
    a[int(rng.integers(0, n))] = e
    ks = [0, 1] if where == "below" else [n - 3, n - 2]
    s = np.sort(a)
    assert (s[0] == e and s[1] == v) if where == "below" else (s[n - 1] == e and s[n - 2] == v)
    _both_routes(gdf, force_path, a, [_q_for_rank(n, k) for k in ks] + [0.5])


# ---------------------------------------------------------------------------------------------------------------------------------
# D5: every flavour of NaN, all three modes

@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=IDS)
def test_nan_flavours_all_modes(gdf, force_path, dtype):
    import torch
    from libgdf_amd.columns import Column
    dt = np.dtype(dtype)
    rng = np.random.default_rng(29)
    n = 10_000
    a = (rng.standard_normal(n) * 10).astype(dt)
    nans = sc.nan_values(dt)
    where = rng.choice(n, size=250, replace=False)
    a[where[:200]] = nans[np.arange(200) % len(nans)]                # 2 % NaNs, 25 of every pattern
    a[where[200:215]] = np.inf
    a[where[215:230]] = -np.inf
    a[where[230:240]] = 0.0
    a[where[240:250]] = -0.0
    ub = sc.bits_of(a)
    for pattern in sc.NAN_BITS[dt]:
        assert np.count_nonzero(ub == pattern) == 25, "every pattern must reach the column bit for bit"
    s = np.sort(a)
    nn, ninf = 200, 15
    assert np.isnan(s[n - nn:]).all() and np.isinf(s[n - nn - ninf: n - nn]).all() and np.isfinite(s[n - nn - ninf - 1])
    ranks = [n - nn - ninf - 1, n - nn - ninf - 2, n - nn - 1, n - nn - 2, n - nn // 2, n - 2, 0, 14, 15]
    qs = [_q_for_rank(n, k) for k in ranks] + [0.0, 0.5, 1.0]
    for q, k in zip(qs, ranks):
        assert sc.rank_of_q(n, q) == k
    # mode 3, both routes
    _both_routes(gdf, force_path, a, qs)
    # mode 1 on np.sort(a)
    ts = torch.from_numpy(s).cuda()
    cs = Column(ts)
    for q in qs:
        for m in METHODS:
            assert same(_call(gdf, cs, q, m, flag_sorted=1), quantile_rule(s, q, m)), (dt, q, m, "sorted")
    assert np.array_equal(sc.bits_of(ts.cpu().numpy()), sc.bits_of(s))
    # mode 2 on copies
    t = torch.from_numpy(a).cuda()
    m_finite = n - nn
    for q in qs:
        for m in (None, 0, 3):
            tc = t.clone()
            assert same(_call(gdf, Column(tc), q, m, inplace=1), quantile_rule(s, q, m)), (dt, q, m, "inplace")
            got = tc.cpu().numpy()
            assert np.array_equal(got, s, equal_nan=True), "mode 2 must leave the column sorted, NaN last"
            assert np.array_equal(sc.bits_of(sc.zeros_unsigned(got[:m_finite])), sc.bits_of(sc.zeros_unsigned(s[:m_finite])))
            assert np.isnan(got[m_finite:]).all()
