"""-m gpu: gdf_inner_join / gdf_left_join / gdf_full_join through the C ABI vs the oracle.

Cases follow the reference's gtest suite (tests/join/join-tests.cu:516-760): 1-5 key columns of every
numeric dtype, EqualValues, MaxRandomValues, Left/RightColumnsBigger, Empty*, random valid masks on the
inputs, and the size-limit checks.  Results are compared as SORTED (l, r) pair lists (:342-345)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import oracle
from util import gen_rand, random_valid, sort_pairs

pytestmark = pytest.mark.gpu


def _cols(arrs, valids=None):
    from libgdf_amd.columns import column_from_numpy
    valids = valids or [None] * len(arrs)
    return [column_from_numpy(a, v) for a, v in zip(arrs, valids)]


def _check(gdf, left, right, how, lvalid=None, rvalid=None):
    li, ri = gdf.api.join(_cols(left, lvalid), _cols(right, rvalid), how=how)
    el, er = oracle.join(left, right, how, lvalid, rvalid)
    a, b = sort_pairs(li.cpu().numpy(), ri.cpu().numpy())
    c, d = sort_pairs(el, er)
    assert len(a) == len(c), (len(a), len(c))
    np.testing.assert_array_equal(a, c)
    np.testing.assert_array_equal(b, d)
    return len(a)


KEYSETS = [
    [np.int32], [np.int64], [np.float32], [np.float64], [np.int8], [np.int16],
    [np.int32, np.int32], [np.int64, np.int32], [np.int32, np.float64],
    [np.int32, np.int64, np.int16], [np.int64, np.int64], [np.float32, np.float64, np.int8, np.int64, np.int32],
]


def _gen(dtypes, n, rng):
    out = []
    for dt in dtypes:
        if np.dtype(dt).kind == "f":
            out.append(np.round(gen_rand(dt, n) * rng).astype(dt))
        else:
            info = np.iinfo(dt)
            out.append(gen_rand(dt, n, low=0, high=min(rng, info.max)))
    return out


@pytest.mark.parametrize("how", ["inner", "left", "full"])
@pytest.mark.parametrize("dtypes", KEYSETS, ids=lambda d: "-".join(np.dtype(x).name for x in d))
def test_random_values(gdf, how, dtypes):
    """MaxRandomValues-style: 10k x 10k rows (join-tests.cu:617-633), value range tuned for a non-trivial result."""
    rng = 2000 if len(dtypes) == 1 else 12
    _check(gdf, _gen(dtypes, 10000, rng), _gen(dtypes, 10000, rng), how)


@pytest.mark.parametrize("how", ["inner", "left", "full"])
def test_equal_values(gdf, how):
    """EqualValues: 100 x 1000 rows, every key identical -> full cross product (join-tests.cu:597-615)."""
    n = _check(gdf, [np.ones(100, dtype=np.int32)], [np.ones(1000, dtype=np.int32)], how)
    assert n == 100 * 1000


@pytest.mark.parametrize("how", ["inner", "left", "full"])
@pytest.mark.parametrize("nl,nr", [(10000, 100), (100, 10000)])
def test_one_side_bigger(gdf, how, nl, nr):
    """Left/RightColumnsBigger: range 100 (join-tests.cu:635-671); exercises the build-side swap of INNER."""
    _check(gdf, _gen([np.int64], nl, 100), _gen([np.int64], nr, 100), how)


@pytest.mark.parametrize("how", ["inner", "left", "full"])
@pytest.mark.parametrize("dtypes", [[np.int32], [np.int64, np.int32], [np.float64]], ids=["i32", "i64-i32", "f64"])
def test_random_valid_masks(gdf, how, dtypes):
    """join-tests.cu HASH inputs carry masks: first half valid, second half coin flips (valid_vectors.h:32-50)."""
    left, right = _gen(dtypes, 5000, 60), _gen(dtypes, 3000, 60)
    lv = [random_valid(5000) for _ in dtypes]
    rv = [random_valid(3000) for _ in dtypes]
    _check(gdf, left, right, how, lv, rv)


def test_float_nan_and_signed_zero(gdf):
    l = np.array([0.0, -0.0, np.nan, 1.5, np.nan], dtype=np.float64)
    r = np.array([-0.0, np.nan, 1.5, 0.0], dtype=np.float64)
    for how in ("inner", "left", "full"):
        _check(gdf, [l], [r], how)      # NaN matches nothing, -0.0 == +0.0 (rows_equal uses ==)


@pytest.mark.parametrize("how", ["inner", "left", "full"])
@pytest.mark.parametrize("nl,nr", [(0, 100), (100, 0), (0, 0)])
def test_empty_inputs(gdf, how, nl, nr):
    """EmptyLeft / EmptyRight / EmptyBoth (join-tests.cu:673-714 with the rules of joining.cu:304-323)."""
    import torch
    from libgdf_amd import Column, gdf_column, libgdf, new_context
    from libgdf_amd.columns import column_array
    L = [Column(torch.arange(max(nl, 1), dtype=torch.int32, device="cuda"), None, 3, size=nl)]
    R = [Column(torch.arange(max(nr, 1), dtype=torch.int32, device="cuda"), None, 3, size=nr)]
    li, ri = gdf_column(), gdf_column()
    ctx = new_context()
    fn = getattr(libgdf, f"gdf_{how}_join")
    idx = (C.c_int * 1)(0)
    fn(column_array(L), 1, idx, column_array(R), 1, idx, 1, 0, None, C.byref(li), C.byref(ri), C.byref(ctx))
    if how == "full" and (nl or nr):
        n = max(nl, nr)
        assert li.size == n and ri.size == n
        import ctypes
        a = gdf.api._take_library_column(li, torch.int32).cpu().numpy()
        b = gdf.api._take_library_column(ri, torch.int32).cpu().numpy()
        if nl:
            assert list(a) == list(range(nl)) and np.all(b == -1)
        else:
            assert list(b) == list(range(nr)) and np.all(a == -1)
    elif how == "left" and nl and not nr:
        # joining.cu:304-323 has no early return for LEFT with an empty right side: every left row pairs with -1
        assert li.size == nl and ri.size == nl
        a = gdf.api._take_library_column(li, torch.int32).cpu().numpy()
        b = gdf.api._take_library_column(ri, torch.int32).cpu().numpy()
        assert sorted(a) == list(range(nl)) and np.all(b == -1)
    else:
        assert li.size == 0 and ri.size == 0


def test_no_match_returns_empty_columns(gdf):
    li, ri = gdf.api.join(_cols([np.arange(1000, dtype=np.int64)]), _cols([np.arange(5000, 6000, dtype=np.int64)]))
    assert li.numel() == 0 and ri.numel() == 0


def test_error_codes(gdf):
    import torch
    from libgdf_amd import GDFError, gdf_column, libgdf, new_context
    from libgdf_amd.columns import GDF_SORT, column_array
    a = _cols([gen_rand(np.int32, 10)])
    b = _cols([gen_rand(np.int64, 10)])
    with pytest.raises(GDFError, match="GDF_JOIN_DTYPE_MISMATCH"):
        gdf.api.join(a, b)
    two_l = _cols([gen_rand(np.int32, 10), gen_rand(np.int32, 10)])
    two_r = _cols([gen_rand(np.int32, 10), gen_rand(np.int32, 10)])
    with pytest.raises(GDFError, match="GDF_JOIN_TOO_MANY_COLUMNS"):
        gdf.api.join(two_l, two_r, method=GDF_SORT)
    short = _cols([gen_rand(np.int32, 10), gen_rand(np.int32, 9)])
    with pytest.raises(GDFError, match="GDF_COLUMN_SIZE_MISMATCH"):
        gdf.api.join(short, two_r)
    li, ri = gdf_column(), gdf_column()
    idx = (C.c_int * 1)(0)
    with pytest.raises(GDFError, match="GDF_INVALID_API_CALL"):
        libgdf.gdf_inner_join(column_array(a), 1, idx, column_array(a), 1, idx, 1, 0, None, C.byref(li), C.byref(ri), None)


def test_medium_fk_pk_join_uses_two_partition_levels(gdf):
    """4M build rows -> 11 fine bits (two scatter levels); unique build keys, every probe row matches once."""
    nb, npr = 4_000_000, 6_000_000
    build = np.random.permutation(nb).astype(np.int64)
    probe = (oracle.splitmix64(np.arange(npr, dtype=np.uint64) + np.uint64(0x5EED0002)) % np.uint64(nb)).astype(np.int64)
    li, ri = gdf.api.join(_cols([probe]), _cols([build]))
    li, ri = li.cpu().numpy(), ri.cpu().numpy()
    assert len(li) == npr
    assert np.array_equal(np.sort(li), np.arange(npr))
    assert np.array_equal(build[ri], probe[li])          # every emitted pair really joins


def test_skewed_build_side_takes_global_table_path(gdf):
    """One key repeated 20k times on the build side exceeds the LDS table (JK_MAX_BUILD = 6080)."""
    build = np.concatenate([np.full(20000, 7, dtype=np.int32), np.arange(100, 3000, dtype=np.int32)])
    probe = np.concatenate([np.full(30, 7, dtype=np.int32), np.arange(0, 4000, 3, dtype=np.int32)])
    for how in ("inner", "left", "full"):
        _check(gdf, [probe], [build], how)


@pytest.mark.parametrize("copies", list(range(6030, 6160, 10)))
@pytest.mark.parametrize("kdt", ["wide", "narrow"])
def test_wide_keys_largest_lds_partition(gdf, copies, kdt, force_path):
    """A build partition at the edge of what stays in LDS (csrc/join.hip JK_MAX_BUILD): one key repeated `copies` times next to a few
    others.  The general kernel's WIDE image is 16 bytes per build tuple + the two tables: up to 6080 tuples fit a CU's 160 KiB, 6081 ...
    6144 (the bound until round 6) asked for 80 bytes more than there are and the launch failed -- found by tools/stress_join.py.  A
    sweep across both bounds (32 partitions: the repeated key's holds `copies` + ~9 tuples), genuinely 64-bit and narrow keys, INNER /
    LEFT / FULL (FULL and repeated build keys take the general kernel)."""
    force_path("GDF_JK_FORCE_FB", "5")
    base = (1 << 61) + 12345 if kdt == "wide" else 1000
    spread = (1 << 44) + 1 if kdt == "wide" else 1
    build = np.concatenate([np.full(copies, base + 7 * spread, dtype=np.int64), base + np.arange(100, 400, dtype=np.int64) * spread])
    probe = np.concatenate([np.full(3, base + 7 * spread, dtype=np.int64), base + np.arange(0, 800, 3, dtype=np.int64) * spread])
    for how in ("inner", "left", "full"):
        _check(gdf, [probe], [build], how)


@pytest.mark.parametrize("how", ["inner", "left", "full"])
def test_result_cols_materialisation(gdf, how):
    """gdf_*_join with result_cols: [left non-key..., key..., right non-key...] (joining.cu:413-439), gathered by one
    multi-column kernel per side (csrc/join.hip jk_gather_multi).  Payload widths 1 / 2 / 4 / 8 bytes, masked payload and
    masked right key; the key of a FULL join's unmatched right rows comes from the right table."""
    import torch
    from libgdf_amd import Column, gdf_column, libgdf, new_context
    from libgdf_amd.columns import column_array
    nl, nr = 30_000, 20_000
    lk = gen_rand(np.int32, nl, 0, 5000)
    rk = gen_rand(np.int32, nr, 2500, 7500)
    lp = [gen_rand(np.float64, nl), gen_rand(np.int8, nl), gen_rand(np.int16, nl)]
    rp = [gen_rand(np.int64, nr), gen_rand(np.float32, nr)]
    lpv = [random_valid(nl), None, random_valid(nl)]
    rpv = [None, random_valid(nr)]
    L = _cols([lp[0], lk, lp[1], lp[2]], [lpv[0], None, lpv[1], lpv[2]])          # key is column 1 on the left
    R = _cols([rk, rp[0], rp[1]], [None, rpv[0], rpv[1]])                          # and column 0 on the right
    nres = 3 + 1 + 2
    res = [gdf_column() for _ in range(nres)]
    res_arr = (C.POINTER(gdf_column) * nres)(*[C.pointer(r) for r in res])
    li, ri = gdf_column(), gdf_column()
    ctx = new_context()
    fn = {"inner": libgdf.gdf_inner_join, "left": libgdf.gdf_left_join, "full": libgdf.gdf_full_join}[how]
    fn(column_array(L), 4, (C.c_int * 1)(1), column_array(R), 3, (C.c_int * 1)(0), 1, nres, res_arr, C.byref(li), C.byref(ri), C.byref(ctx))
    n = li.size
    a = gdf.api._take_library_column(li, torch.int32).cpu().numpy()
    b = gdf.api._take_library_column(ri, torch.int32).cpu().numpy()
    el, er = oracle.join([lk], [rk], how)
    assert n == len(el)
    assert [r.size for r in res] == [n] * nres
    assert [r.dtype for r in res] == [6, 1, 2, 3, 4, 5]                             # f64, i8, i16 | i32 key | i64, f32

    def pull(col, npdtype):
        nbytes_valid = (n + 7) // 8
        data = torch.empty(n * np.dtype(npdtype).itemsize, dtype=torch.uint8, device="cuda")
        valid = torch.empty(nbytes_valid, dtype=torch.uint8, device="cuda")
        gdf.api._hipMemcpyDtoD(data.data_ptr(), col.data, data.numel())
        gdf.api._hipMemcpyDtoD(valid.data_ptr(), col.valid, nbytes_valid)
        libgdf.gdf_column_free(C.byref(col))
        bits = np.unpackbits(valid.cpu().numpy(), bitorder="little")[:n].astype(bool)
        return data.cpu().numpy().view(npdtype), bits

    has_l, has_r = a >= 0, b >= 0
    for j, (src, sv) in enumerate(zip(lp, lpv)):
        d, v = pull(res[j], src.dtype)
        exp_valid = has_l & (sv[np.where(has_l, a, 0)] if sv is not None else True)
        np.testing.assert_array_equal(v, exp_valid)
        np.testing.assert_array_equal(d[v], src[a[v]])
    d, v = pull(res[3], np.int32)
    np.testing.assert_array_equal(v, has_l | has_r)
    exp_key = np.where(has_l, lk[np.where(has_l, a, 0)], rk[np.where(has_r, b, 0)])
    np.testing.assert_array_equal(d[v], exp_key[v])
    for j, (src, sv) in enumerate(zip(rp, rpv)):
        d, v = pull(res[4 + j], src.dtype)
        exp_valid = has_r & (sv[np.where(has_r, b, 0)] if sv is not None else True)
        np.testing.assert_array_equal(v, exp_valid)
        np.testing.assert_array_equal(d[v], src[b[v]])


def _join_with_result_cols(gdf, how, left, lkey, right, rkey, left_valid=None, right_valid=None):
    """gdf_{how}_join over numpy columns with result_cols -> (left idx, right idx, [(data, valid bits)] per result column).
    left_valid / right_valid: optional per-column bool vectors (None entries: no mask)."""
    import torch
    from libgdf_amd import gdf_column, libgdf
    from libgdf_amd.columns import column_array, column_from_numpy, new_context
    L = [column_from_numpy(a, None if left_valid is None else left_valid[i]) for i, a in enumerate(left)]
    R = [column_from_numpy(a, None if right_valid is None else right_valid[i]) for i, a in enumerate(right)]
    nres = len(left) + len(right) - 1
    res = [gdf_column() for _ in range(nres)]
    res_arr = (C.POINTER(gdf_column) * nres)(*[C.pointer(r) for r in res])
    li, ri = gdf_column(), gdf_column()
    ctx = new_context()
    fn = {"inner": libgdf.gdf_inner_join, "left": libgdf.gdf_left_join, "full": libgdf.gdf_full_join}[how]
    fn(column_array(L), len(left), (C.c_int * 1)(lkey), column_array(R), len(right), (C.c_int * 1)(rkey), 1, nres, res_arr,
       C.byref(li), C.byref(ri), C.byref(ctx))
    n = int(li.size)
    a = gdf.api._take_library_column(li, torch.int32).cpu().numpy() if n else np.zeros(0, np.int32)
    b = gdf.api._take_library_column(ri, torch.int32).cpu().numpy() if n else np.zeros(0, np.int32)
    order = [c for i, c in enumerate(left) if i != lkey] + [left[lkey]] + [c for i, c in enumerate(right) if i != rkey]
    out = []
    for col, src in zip(res, order):
        assert int(col.size) == n
        if n == 0:
            out.append((np.zeros(0, src.dtype), np.zeros(0, bool)))
            continue
        data = torch.empty(n * src.dtype.itemsize, dtype=torch.uint8, device="cuda")
        valid = torch.empty((n + 7) // 8, dtype=torch.uint8, device="cuda")
        gdf.api._hipMemcpyDtoD(data.data_ptr(), col.data, data.numel())
        gdf.api._hipMemcpyDtoD(valid.data_ptr(), col.valid, valid.numel())
        libgdf.gdf_column_free(C.byref(col))
        out.append((data.cpu().numpy().view(src.dtype), np.unpackbits(valid.cpu().numpy(), bitorder="little")[:n].astype(bool)))
    return a, b, out


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("payload", ["i64", "f64", "i32", "i32+f32", "i16"], ids=lambda p: p)
@pytest.mark.parametrize("shape", ["all-hit", "half-hit", "80pct-hit", "dup-build-keys", "probe-is-right", "small-exact-layout", "skewed"])
@pytest.mark.parametrize("kdt", [np.int64, np.int32], ids=["key-i64", "key-i32"])
def test_carried_payload_matches_the_gather(gdf, how, payload, shape, kdt, force_path):
    """result_cols of an INNER / LEFT join whose probe relation has one 8-byte, one 4-byte or two 4-byte non-key columns: the
    values travel through the partition passes next to their tuples (csrc/join.hip PayCarry, jk_scatter1_pay, Tuples::pay)
    and the probe kernel writes the result columns streaming.  Every pair's payload must be the probe row's value -- through
    the optimistic single pass, the sparse pass + compaction, count + write, the general kernel (repeated build keys: payload
    gathered by row), the exact layout and a skewed probe side; a 2-byte column is not carried and still gathers
    (reference: joining.cu:375-479, gdf_table.cuh:873-963)."""
    import zlib
    rs = np.random.RandomState(zlib.crc32(f"{payload}/{shape}".encode()) % 100000)
    npr, nb = (400_000, 40_000)
    if shape != "small-exact-layout":
        force_path("GDF_JK_SPEC_MIN", "1000")
    else:
        npr, nb = 3_000, 700
    space = {"all-hit": nb, "half-hit": 2 * nb, "80pct-hit": nb + nb // 4}.get(shape, nb)
    build = rs.permutation(max(space, nb))[:nb].astype(np.int64) if shape != "dup-build-keys" else (rs.permutation(nb) % (nb // 4)).astype(np.int64)
    if shape == "all-hit":
        build = rs.permutation(nb).astype(np.int64)
    probe = rs.randint(0, space if shape != "dup-build-keys" else nb // 4, size=npr).astype(np.int64)
    if shape == "skewed":
        probe[rs.randint(0, npr, size=npr // 8)] = build[0]
    build, probe = build.astype(kdt), probe.astype(kdt)       # (an INNER join on one int64 / int32 key column also emits the KEY column from the kernel)
    pays = {"i64": [rs.randint(-2**62, 2**62, size=npr).astype(np.int64)], "f64": [rs.random_sample(npr)],
            "i32": [rs.randint(-2**31, 2**31 - 1, size=npr).astype(np.int32)],
            "i32+f32": [rs.randint(-2**31, 2**31 - 1, size=npr).astype(np.int32), rs.random_sample(npr).astype(np.float32)],
            "i16": [rs.randint(-2**15, 2**15 - 1, size=npr).astype(np.int16)]}[payload]
    # the BUILD relation's non-key columns travel too (INNER joins, jk_probe_bp): one 8-byte, one 4-byte or two 4-byte columns
    bpays = {"i64": [rs.randint(-2**62, 2**62, size=nb).astype(np.int64)], "f64": [rs.randint(0, 1000, size=nb).astype(np.int32), rs.random_sample(nb).astype(np.float32)],
             "i32": [rs.randint(0, 1000, size=nb).astype(np.int32)], "i32+f32": [rs.random_sample(nb)],
             "i16": [rs.randint(0, 1000, size=nb).astype(np.int16)]}[payload]
    if shape == "probe-is-right":
        if how == "left":
            pytest.skip("a LEFT join always probes with the left relation")
        a, b, cols = _join_with_result_cols(gdf, how, [build] + bpays, 0, pays + [probe], len(pays))      # smaller relation on the LEFT: INNER flips
        el, er = oracle.join([build], [probe], how)
        probe_idx, build_idx = b, a
        res_build_pay, res_key, res_probe_pay = cols[:len(bpays)], cols[len(bpays)], cols[len(bpays) + 1:]
    else:
        a, b, cols = _join_with_result_cols(gdf, how, pays + [probe], len(pays), [build] + bpays, 0)
        el, er = oracle.join([probe], [build], how)
        probe_idx, build_idx = a, b
        res_probe_pay, res_key, res_build_pay = cols[:len(pays)], cols[len(pays)], cols[len(pays) + 1:]
    x, y = sort_pairs(a, b)
    ex, ey = sort_pairs(el, er)
    np.testing.assert_array_equal(x, ex)
    np.testing.assert_array_equal(y, ey)
    for (d, v), src in zip(res_probe_pay, pays):
        assert v.all()                                              # the probe row of an INNER / LEFT pair always exists
        np.testing.assert_array_equal(d, src[probe_idx])
    d, v = res_key
    assert v.all()
    np.testing.assert_array_equal(d, probe[probe_idx])
    for (d, v), src in zip(res_build_pay, bpays):
        np.testing.assert_array_equal(v, build_idx >= 0)
        np.testing.assert_array_equal(d[v], src[build_idx[v]])


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("cols", ["i64,i64+i64,i64", "i32,i64m,f32+i16,f64,i32", "i64m,i64+f64m", "i32,i32,i32+i64,i64,i64",
                                  # one side without non-key columns, one and two payload words against two and one: every (probe words,
                                  # build words) pair of the lean kernels, with the lean tables above 42 % load (30 000 build rows) ...
                                  "i32+", "i32,i32+", "i64,i64+", "+i64", "+i64,i64", "i64,i64+i64",
                                  # ... and below it (40 000 build rows: power-of-two tables)
                                  "i64+@40k", "i32+@40k", "i32,i32+@40k", "i64,i64+@40k", "+i64@40k", "+i64,i64@40k", "i64+i64,i64@40k", "i64,i64+i64@40k"])
def test_one_payload_word_is_carried_and_the_rest_gathered(gdf, how, cols, force_path):
    """Relations with SEVERAL non-key columns: one 64-bit word per side travels with the tuples -- the first
    unmasked 8-byte column, else the first two unmasked 4-byte ones -- and every other column (further ones, masked ones, 2-byte
    ones) is gathered through the index columns; the result must not depend on which way a column took (reference:
    joining.cu:375-479).  'm' marks a column with a validity mask."""
    import zlib
    rs = np.random.RandomState(zlib.crc32(cols.encode()) % 100000)
    cols, _, size = cols.partition("@")
    npr, nb = (400_000, 40_000) if size == "40k" else (300_000, 30_000)
    force_path("GDF_JK_SPEC_MIN", "1000")
    build = rs.permutation(nb + nb // 4)[:nb].astype(np.int64)
    probe = rs.randint(0, nb + nb // 4, size=npr).astype(np.int64)

    def make(spec, n):
        arrs, valids = [], []
        for name in filter(None, spec.split(",")):
            masked = name.endswith("m")
            dt = {"i64": np.int64, "f64": np.float64, "i32": np.int32, "f32": np.float32, "i16": np.int16}[name.rstrip("m")]
            arrs.append(rs.random_sample(n).astype(dt) if np.dtype(dt).kind == "f" else rs.randint(-30000, 30000, size=n).astype(dt))
            valids.append(rs.random_sample(n) < 0.8 if masked else None)
        return arrs, valids

    pspec, bspec = cols.split("+")
    pays, pvalid = make(pspec, npr)
    bpays, bvalid = make(bspec, nb)
    a, b, res = _join_with_result_cols(gdf, how, pays + [probe], len(pays), [build] + bpays, 0, pvalid + [None], [None] + bvalid)
    el, er = oracle.join([probe], [build], how)
    x, y = sort_pairs(a, b)
    ex, ey = sort_pairs(el, er)
    np.testing.assert_array_equal(x, ex)
    np.testing.assert_array_equal(y, ey)
    for (d, v), src, sv in zip(res[:len(pays)], pays, pvalid):
        exp_valid = np.ones(len(a), bool) if sv is None else sv[a]
        np.testing.assert_array_equal(v, exp_valid)
        np.testing.assert_array_equal(d[v], src[a][v])
    d, v = res[len(pays)]
    assert v.all()
    np.testing.assert_array_equal(d, probe[a])
    for (d, v), src, sv in zip(res[len(pays) + 1:], bpays, bvalid):
        has = b >= 0
        exp_valid = has & (True if sv is None else sv[np.where(has, b, 0)])
        np.testing.assert_array_equal(v, exp_valid)
        np.testing.assert_array_equal(d[v], src[b[v]])


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("shape", ["all-hit", "half-hit", "80pct-hit", "dup-build-keys", "small-exact-layout", "skewed", "headline-geometry", "three-per-side",
                                   "int32-keys"])
def test_two_payload_words_per_side(gdf, how, shape, force_path):
    """Round 6: a relation with TWO unmasked 8-byte non-key columns carries both -- a 16-byte payload element
    through jk_scatter1_pay<.., 4> (6144-tuple tiles), jk_scatter2<.., 2> and the probe kernels (csrc/join.hip PayCarry mode 4) -- and an
    INNER join's build relation has its first such column travel with the tuples and the second staged BY BUILD ROW into the LDS image
    (jk_probe_bp<.., BW2>).  Every output-sizing path (dense single pass, hole filling, compaction, count + write), the general kernel
    (repeated build keys: payloads gathered by row), the exact layout, a skewed probe side, the headline's geometry
    (GDF_JK_FORCE_FB=15), a third 8-byte column per side (gathered) -- against the oracle and against the one-word path
    (GDF_JK_NO_CARRY2).  Reference: joining.cu:375-479, gdf_table.cuh:873-963."""
    import zlib
    rs = np.random.RandomState(zlib.crc32(shape.encode()) % 100000)
    npr, nb = (400_000, 40_000)
    if shape == "small-exact-layout":
        npr, nb = 3_000, 700
    else:
        force_path("GDF_JK_SPEC_MIN", "1000")
    if shape == "headline-geometry":
        npr, nb = 1_300_000, 60_000
        force_path("GDF_JK_FORCE_FB", "15")
    space = {"half-hit": 2 * nb, "80pct-hit": nb + nb // 4}.get(shape, nb)
    build = rs.permutation(max(space, nb))[:nb].astype(np.int64) if shape != "dup-build-keys" else (rs.permutation(nb) % (nb // 4)).astype(np.int64)
    probe = rs.randint(0, space if shape != "dup-build-keys" else nb // 4, size=npr).astype(np.int64)
    if shape == "skewed":
        probe[rs.randint(0, npr, size=npr // 8)] = build[0]
    if shape == "int32-keys":                      # (jk_scatter1_pay reads a 4-byte key column next to the 16-byte payload element)
        build, probe = build.astype(np.int32), probe.astype(np.int32)
    ncols = 3 if shape == "three-per-side" else 2
    pays = [rs.randint(-2**62, 2**62, size=npr).astype(np.int64), rs.random_sample(npr)] + ([rs.randint(0, 99, size=npr).astype(np.int64)] if ncols == 3 else [])
    bpays = [rs.random_sample(nb), rs.randint(-2**62, 2**62, size=nb).astype(np.int64)] + ([rs.random_sample(nb)] if ncols == 3 else [])

    def run():
        a, b, res = _join_with_result_cols(gdf, how, pays + [probe], len(pays), [build] + bpays, 0)
        el, er = oracle.join([probe], [build], how)
        x, y = sort_pairs(a, b)
        ex, ey = sort_pairs(el, er)
        np.testing.assert_array_equal(x, ex)
        np.testing.assert_array_equal(y, ey)
        for (d, v), src in zip(res[:len(pays)], pays):
            assert v.all()
            np.testing.assert_array_equal(d.view(np.int64), src[a].view(np.int64))
        d, v = res[len(pays)]
        assert v.all()
        np.testing.assert_array_equal(d, probe[a])
        has = b >= 0
        for (d, v), src in zip(res[len(pays) + 1:], bpays):
            np.testing.assert_array_equal(v, has)
            np.testing.assert_array_equal(d[v].view(np.int64), src[b[v]].view(np.int64))
        return len(a)
    n1 = run()
    force_path("GDF_JK_NO_CARRY2")
    assert run() == n1


@pytest.mark.parametrize("how", ["inner", "left", "full"])
def test_int64_keys_wider_than_32_bits(gdf, how):
    """Build keys spanning more than 2^32 use the 12-byte tuple format; a narrower build range uses packed
    8-byte tuples and probe keys outside it must simply not match."""
    wide = (gen_rand(np.int64, 6000, 0, 400) * np.int64(1 << 34)) - np.int64(7)
    _check(gdf, [np.random.permutation(wide)], [wide[:3000]], how)
    build = gen_rand(np.int64, 3000, -50, 50)
    probe = np.concatenate([gen_rand(np.int64, 3000, -80, 80), np.array([2**40, -2**40, 2**63 - 1, -2**63], dtype=np.int64)])
    _check(gdf, [probe], [build], how)


@pytest.mark.parametrize("how", ["inner", "left"])
def test_wide_keys_lean_kernel_and_fold_collisions(gdf, how, force_path):
    """64-bit keys spread over 2^60 take the WIDE tuples and (round 2) the lean write kernel; keys that share their 32-bit
    fold (lo ^ hi * 0x9e3779b1) land in one partition and in the same slot of cuckoo table 0 -- six of them per fold value
    here, which only settles because table 1 hashes an independent second fold (csrc/join.hip key_fold2)."""
    force_path("GDF_JK_SPEC_MIN", "1000")
    rs = np.random.RandomState(11)
    nb = 300_000
    build = rs.randint(0, 2**60, size=nb, dtype=np.int64)
    C = np.uint64(0x9e3779b1)
    fam = []
    for x in rs.randint(0, 2**32, size=400, dtype=np.int64):
        for hi in rs.randint(1, 2**27, size=6, dtype=np.int64):
            lo = (np.uint64(x) ^ ((np.uint64(hi) * C) & np.uint64(0xffffffff))) & np.uint64(0xffffffff)
            fam.append(int((np.uint64(hi) << np.uint64(32)) | lo))
    build = np.unique(np.concatenate([build, np.array(fam, dtype=np.int64)]))
    rs.shuffle(build)
    probe = np.concatenate([build[rs.randint(0, len(build), size=1_500_000)], np.array(fam * 3, dtype=np.int64),
                            rs.randint(0, 2**60, size=200_000, dtype=np.int64)])
    rs.shuffle(probe)
    _check(gdf, [probe], [build], how)


def test_multigpu_layer_world_size_one(gdf):
    """libgdf_amd/multigpu.py end to end on the GPU with a 1-rank RCCL group: device-side gdf_hash_partition,
    all_to_all_single, local gdf_inner_join, global row ids.  (2-rank exchange logic: tests/test_multigpu_gloo.py.)"""
    import os
    import socket
    import torch
    import torch.distributed as dist
    from libgdf_amd import multigpu
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        probe = gen_rand(np.int64, 200000, 0, 5000)
        build = np.random.permutation(5000).astype(np.int64)[:4000]
        pairs = multigpu.distributed_inner_join(torch.from_numpy(probe).cuda(), torch.from_numpy(build).cuda())
        pg, bg = pairs.global_ids()
        el, er = oracle.join([probe], [build], "inner")
        a, b = sort_pairs(pg.cpu().numpy(), bg.cpu().numpy())
        c, d = sort_pairs(el, er)
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(b, d)
        # shard sizes at which the received probe slices are accumulated and probed once (gdf_amd_join_probe_*)
        big_b = torch.randperm(1_300_000, device="cuda")[:1_000_000]
        big_p = torch.randint(0, 1_300_000, (6_000_000,), device="cuda")
        bp = multigpu.distributed_inner_join(big_p, big_b)
        assert len(bp.probe_pos) == 1                      # one pair list: the accumulator took all four slices
        g1, g2 = bp.global_ids()
        assert g1.numel() == int(torch.isin(big_p, big_b).sum().item())
        assert torch.equal(big_p[g1], big_b[g2])           # rank 0: a global id is the local row
        assert torch.unique(g1).numel() == g1.numel()
        # the broadcast variant: same pairs
        bpairs = multigpu.broadcast_inner_join(torch.from_numpy(probe).cuda(), torch.from_numpy(build).cuda())
        bpg, bbg = bpairs.global_ids()
        a2, b2 = sort_pairs(bpg.cpu().numpy(), bbg.cpu().numpy())
        np.testing.assert_array_equal(a2, c)
        np.testing.assert_array_equal(b2, d)
        # a rank may hold no rows of a relation
        empty = torch.zeros(0, dtype=torch.int64, device="cuda")
        assert multigpu.distributed_inner_join(empty, torch.from_numpy(build).cuda()).numel() == 0
        assert multigpu.distributed_inner_join(torch.from_numpy(probe).cuda(), empty).numel() == 0
        # keys too far apart for the 4-byte narrowing travel as 8 bytes
        wide_b = torch.from_numpy(build).cuda() * (1 << 33)
        wide_p = torch.from_numpy(probe).cuda() * (1 << 33)
        assert multigpu.distributed_inner_join(wide_p, wide_b).numel() == len(el)
        k = torch.from_numpy(probe).cuda()
        v = torch.from_numpy((probe * 2 + 1).astype(np.int64)).cuda()
        gk, gv = multigpu.distributed_group_by_sum(k, v)
        ek, ea = oracle.group_by("sum", [probe], (probe * 2 + 1).astype(np.int64))
        o = np.argsort(gk.cpu().numpy())
        np.testing.assert_array_equal(gk.cpu().numpy()[o], ek[0])
        np.testing.assert_array_equal(gv.cpu().numpy()[o], ea)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("dtypes", [[np.int64], [np.int32], [np.float64], [np.int32, np.int64, np.int16]],
                         ids=lambda d: "-".join(np.dtype(x).name for x in d))
def test_prepared_build_probed_in_slices(gdf, how, dtypes):
    """gdf_amd_join_build_* (include/gdf/gdf_amd_ext.h): one partitioned build relation probed by several probe
    relations gives, for each, exactly the pairs of gdf_{inner,left}_join(probe, build)."""
    rng = 3000 if len(dtypes) == 1 else 12
    build = _gen(dtypes, 20000, rng)
    jb = gdf.api.JoinBuild(_cols(build))
    for n in (0, 1, 777, 50000):
        probe = _gen(dtypes, n, rng * 2 if len(dtypes) == 1 else rng)
        li, ri = jb.probe(_cols(probe), how=how)
        el, er = oracle.join(probe, build, how)
        a, b = sort_pairs(li.cpu().numpy(), ri.cpu().numpy())
        c, d = sort_pairs(el, er)
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(b, d)
    jb.close()


@pytest.mark.parametrize("dtype", [np.int64, np.int32], ids=lambda d: np.dtype(d).name)
def test_probe_relation_accumulated_in_slices(gdf, dtype):
    """gdf_amd_join_probe_* (include/gdf/gdf_amd_ext.h): slices partitioned as they arrive, one probe pass at the end
    == the join of the concatenated slices; unsupported shapes say so instead of computing something else."""
    import torch
    from libgdf_amd import Column, GDFError
    nb = 3_000_000
    tdt = torch.int64 if dtype == np.int64 else torch.int32
    build = torch.randperm(nb + nb // 5, device="cuda")[:nb].to(tdt)
    jb = gdf.api.JoinBuild([Column(build)])
    slices = [torch.randint(0, nb + nb // 5, (n,), device="cuda").to(tdt) for n in (2_500_000, 1, 3_000_001, 0, 1_700_000)]
    acc = jb.accumulate(sum(int(x.numel()) for x in slices))
    for x in slices:
        acc.add([Column(x)])
    li, ri = acc.finish()
    allp = torch.cat(slices)
    el, er = jb.probe([Column(allp)])
    assert li.numel() == el.numel()
    assert torch.equal(build[ri.long()], allp[li.long()])
    a = torch.sort(li.long() * (nb + 1) + ri.long()).values
    b = torch.sort(el.long() * (nb + 1) + er.long()).values
    assert torch.equal(a, b)
    # too small an estimate: the slices do not fit the room reserved for them -> the accumulator gives up, loudly
    acc = jb.accumulate(1 << 22)
    with pytest.raises(GDFError, match="GDF_UNSUPPORTED_METHOD"):
        for _ in range(4):
            acc.add([Column(torch.randint(0, nb, (4_000_000,), device="cuda").to(tdt))])
    with pytest.raises(GDFError, match="GDF_UNSUPPORTED_METHOD"):
        acc.finish()
    # a small build side (single partition level) and a small expected size are not accumulated at all
    with pytest.raises(GDFError, match="GDF_UNSUPPORTED_METHOD"):
        gdf.api.JoinBuild([Column(build[:1000])]).accumulate(1 << 24)
    with pytest.raises(GDFError, match="GDF_UNSUPPORTED_METHOD"):
        jb.accumulate(1000)


def test_prepared_build_edge_cases(gdf, force_path):
    import torch
    from libgdf_amd import Column, GDFError
    empty = gdf.api.JoinBuild(_cols([np.zeros(0, dtype=np.int64)]))
    li, ri = empty.probe(_cols([np.arange(5, dtype=np.int64)]), how="inner")
    assert li.numel() == 0 and ri.numel() == 0
    li, ri = empty.probe(_cols([np.arange(5, dtype=np.int64)]), how="left")
    assert sorted(li.cpu().tolist()) == [0, 1, 2, 3, 4] and ri.cpu().tolist() == [-1] * 5
    jb = gdf.api.JoinBuild(_cols([np.arange(100, dtype=np.int64)]))
    with pytest.raises(GDFError, match="GDF_JOIN_DTYPE_MISMATCH"):
        jb.probe(_cols([np.arange(5, dtype=np.int32)]))
    # a probe relation larger than the build relation keeps the table on the prepared side, at speculative-partition size
    force_path("GDF_JK_SPEC_MIN", "1000")
    build = torch.randperm(3_000_000, dtype=torch.int64, device="cuda")[:2_000_000]
    jb2 = gdf.api.JoinBuild([Column(build)])
    for seed in range(2):
        probe = torch.randint(0, 3_000_000, (5_000_000,), dtype=torch.int64, device="cuda")
        li, ri = jb2.probe([Column(probe)])
        present = torch.zeros(3_000_000, dtype=torch.bool, device="cuda")
        present[build] = True
        assert li.numel() == int(present[probe].sum().item())
        assert torch.equal(build[ri.long()], probe[li.long()])
        assert torch.unique(li).numel() == li.numel()


def test_every_partition_oversize_uses_one_global_table(gdf, force_path):
    """A build side beyond 32768 x 6144 rows makes EVERY fine partition exceed the LDS image: the global-table
    path (third partitioning level switched off) must handle them as one run (one table, three launches), not one
    launch per partition."""
    import torch
    force_path("GDF_JK_NO_LEVEL3", "1")
    from libgdf_amd.columns import Column
    nb, npr = 210_000_000, 2_000_000
    build = torch.randperm(nb, dtype=torch.int32, device="cuda")
    probe = torch.randint(0, nb + nb // 4, (npr,), dtype=torch.int32, device="cuda")
    li, ri = gdf.api.join([Column(probe)], [Column(build)])
    hits = int((probe < nb).sum().item())
    assert li.numel() == hits
    assert torch.equal(build[ri.long()], probe[li.long()])
    assert torch.unique(li).numel() == hits


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.int64, np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_sort_method_single_column(gdf, how, dtype):
    """GDF_SORT joins (joining.cu:100-159): one column, same pair SET as the hash method; floats compare by bit
    pattern there (FLOAT32/64 dispatch to int32_t/int64_t), so +0.0 != -0.0 and equal-bit NaNs match."""
    from libgdf_amd.columns import GDF_SORT
    l = _gen([dtype], 8000, 1500)[0]
    r = _gen([dtype], 6000, 1500)[0]
    if np.dtype(dtype).kind == "f":
        l[:4] = [0.0, -0.0, np.nan, 1.0]
        r[:3] = [-0.0, np.nan, 0.0]
    li, ri = gdf.api.join(_cols([l]), _cols([r]), how=how, method=GDF_SORT)
    as_int = {4: np.int32, 8: np.int64}.get(np.dtype(dtype).itemsize) if np.dtype(dtype).kind == "f" else None
    el, er = oracle.join([l.view(as_int) if as_int else l], [r.view(as_int) if as_int else r], how)
    a, b = sort_pairs(li.cpu().numpy(), ri.cpu().numpy())
    c, d = sort_pairs(el, er)
    np.testing.assert_array_equal(a, c)
    np.testing.assert_array_equal(b, d)


def test_sort_method_rules(gdf):
    from libgdf_amd import GDFError
    from libgdf_amd.columns import GDF_SORT, column_from_numpy
    k = gen_rand(np.int32, 50, 0, 10)
    masked = column_from_numpy(k, np.ones(50, dtype=bool))
    with pytest.raises(GDFError, match="GDF_VALIDITY_UNSUPPORTED"):      # joining.cu:105-106
        gdf.api.join([masked], _cols([k]), method=GDF_SORT)
    li, ri = gdf.api.join(_cols([k]), _cols([k]), how="full", method=GDF_SORT)   # generic SortJoin: empty result (joining.cu:66-75)
    assert li.numel() == 0 and ri.numel() == 0


# ---- histogram-free (speculative) partitioning of the probe side -------------------------------------------------
@pytest.mark.parametrize("how", ["inner", "left", "full"])
@pytest.mark.parametrize("dtypes", [[np.int64], [np.int32], [np.int32, np.int64], [np.float64]], ids=lambda d: "-".join(np.dtype(x).name for x in d))
def test_speculative_partitioning_small_inputs(gdf, how, dtypes, force_path):
    """GDF_JK_SPEC_MIN=1 sends even small probe sides through the capacity-slack layout (normally >= 4M rows)."""
    force_path("GDF_JK_SPEC_MIN", "1")
    rng = 20000 if len(dtypes) == 1 else 150
    _check(gdf, _gen(dtypes, 300000, rng), _gen(dtypes, 40000, rng), how)
    lv = [random_valid(300000) for _ in dtypes]
    rv = [random_valid(40000) for _ in dtypes]
    _check(gdf, _gen(dtypes, 300000, rng), _gen(dtypes, 40000, rng), how, lv, rv)


def test_speculative_partitioning_falls_back_on_skew(gdf, force_path):
    """Half of the probe rows carry ONE key: its partition outgrows the slack, the flag is raised and the exact
    (histogram) layout takes over.  Same answer, checked against the oracle and by count."""
    force_path("GDF_JK_SPEC_MIN", "1")
    n = 400000
    l = gen_rand(np.int64, n, 0, 50000)
    l[::2] = 777
    r = np.arange(50000, dtype=np.int64)
    np.random.shuffle(r)
    assert _check(gdf, [l], [r], "inner") == n


def test_speculative_matches_exact_at_scale(gdf, force_path):
    """3e7 x 3e6 uniform keys: speculative (default at this size) and exact (GDF_JK_NO_SPEC) give the same pair set."""
    import torch
    from libgdf_amd.columns import Column
    nb, npr = 3_000_000, 30_000_000
    b = torch.randperm(nb, device="cuda")
    p = torch.randint(0, nb + nb // 10, (npr,), device="cuda")
    li, ri = gdf.api.join([Column(p)], [Column(b)])
    force_path("GDF_JK_NO_SPEC", "1")
    le, re_ = gdf.api.join([Column(p)], [Column(b)])
    assert li.numel() == le.numel() == int((p < nb).sum())
    assert bool((p[li.long()] == b[ri.long()]).all())
    a = torch.sort(li.long() * nb + ri.long()).values
    c = torch.sort(le.long() * nb + re_.long()).values
    assert torch.equal(a, c)


@pytest.mark.parametrize("how", ["inner", "left", "full"])
@pytest.mark.parametrize("dtypes", [[np.int64, np.int32], [np.int32, np.int16, np.int8], [np.int64, np.int64], [np.int8, np.int64]],
                         ids=lambda d: "-".join(np.dtype(x).name for x in d))
def test_range_packed_multi_column_keys(gdf, how, dtypes, force_path):
    """Several integer key columns are packed as (value - build minimum) fields (plan_ranged in csrc/join.hip): probe
    values below / above the build range of a column, negative values and nulls must behave exactly as in the oracle;
    GDF_JK_NO_RANGED (hashed key + row comparison) is the same join."""
    rs = np.random.RandomState(11)
    nb, npr = 6000, 20000
    build, probe = [], []
    for i, dt in enumerate(dtypes):
        info = np.iinfo(dt)
        lo, hi = max(info.min, -40 - 10 * i), min(info.max, 45 + 10 * i)
        build.append(rs.randint(lo + 10, hi - 10, size=nb).astype(dt))            # build range strictly inside the probe range
        probe.append(rs.randint(lo, hi, size=npr).astype(dt))
    bvalid = [None if i else (rs.rand(nb) > 0.05) for i in range(len(dtypes))]
    pvalid = [(rs.rand(npr) > 0.05) if i == len(dtypes) - 1 else None for i in range(len(dtypes))]
    n1 = _check(gdf, probe, build, how, pvalid, bvalid)
    assert n1 > 0
    force_path("GDF_JK_NO_RANGED")
    assert _check(gdf, probe, build, how, pvalid, bvalid) == n1
    force_path("GDF_JK_NO_RANGED", None)
    if dtypes == [np.int64, np.int64]:
        # ranges that do not fit 64 bits together keep the hashed plan
        wide_b = [b.astype(np.int64) * (1 << 40) for b in build]
        wide_p = [q.astype(np.int64) * (1 << 40) for q in probe]
        _check(gdf, wide_p, wide_b, how)


@pytest.mark.parametrize("shape", ["uniform", "hot probe key", "hot build key"])
def test_third_partition_level_for_large_build_sides(gdf, shape):
    """Build relations beyond 2^15 LDS-sized partitions (here 2.6e8 rows) get a third regrouping pass (refine_side in
    csrc/join.hip).  A probe key hot enough to outgrow its refined partition makes the call repeat with the plain
    two-level build side; a hot BUILD key keeps the two-level layout and the global-table path from the start."""
    import torch
    from libgdf_amd.columns import Column
    nb, npr = 260_000_000, 300_000_000
    b = torch.randperm(nb, dtype=torch.int32, device="cuda")
    p = torch.randint(0, nb + nb // 8, (npr,), dtype=torch.int32, device="cuda")
    if shape == "hot probe key":
        p[: npr // 3] = 12345
    if shape == "hot build key":
        b[: 200_000] = 777                                         # 2e5 equal build keys: far beyond one LDS partition
        p[:1000] = 777
    li, ri = gdf.api.join([Column(p)], [Column(b)])
    expect = int((p < nb).sum().item())
    if shape == "hot build key":
        first = torch.zeros(nb + nb // 8 + 1, dtype=torch.int32, device="cuda")
        first.scatter_add_(0, b.long(), torch.ones_like(b))          # multiplicity of every build key
        expect = int(first[p.long()].sum().item())
        del first
    assert li.numel() == expect
    assert torch.equal(b[ri.long()], p[li.long()])
    if shape != "hot build key":
        assert torch.unique(li).numel() == expect


@pytest.mark.parametrize("how", ["inner", "left"])
def test_xcd_regions_match_plain_layout(gdf, how, force_path):
    """1e8 x 1e7 rows (above the 2^26-row threshold): the per-XCD level-1 regions and the XCD-ordered level-2 tiles
    (default) give the same pair set as the plain speculative layout (GDF_JK_NO_XCD_SPLIT / GDF_JK_NO_XCD_ORDER)."""
    import torch
    from libgdf_amd.columns import Column
    nb, npr = 10_000_000, 100_000_000
    b = torch.randperm(nb + nb // 8, device="cuda")[:nb]
    p = torch.randint(0, nb + nb // 4, (npr,), device="cuda")
    li, ri = gdf.api.join([Column(p)], [Column(b)], how=how)
    force_path("GDF_JK_NO_XCD_SPLIT", "1")
    force_path("GDF_JK_NO_XCD_ORDER", "1")
    le, re_ = gdf.api.join([Column(p)], [Column(b)], how=how)
    assert li.numel() == le.numel()
    if how == "left":
        assert li.numel() == npr and torch.equal(torch.sort(li).values, torch.arange(npr, dtype=torch.int32, device="cuda"))
    hit = ri >= 0
    assert bool((p[li[hit].long()] == b[ri[hit].long()]).all())
    a = torch.sort(li.long() * (nb + 1) + (ri.long() + 1)).values
    c = torch.sort(le.long() * (nb + 1) + (re_.long() + 1)).values
    assert torch.equal(a, c)


def test_randomized_inner_join_properties(gdf):
    """60 random shapes (sizes, key ranges, duplicate rates, int32 / int64 keys) checked by properties that do not
    need the oracle: the number of pairs equals sum_probe multiplicity_in_build(key), every pair joins equal keys,
    and no pair occurs twice.  Exercises the lean and the general write kernels, cuckoo retries, the
    linear-probing fallback (duplicate build keys) and both partition layouts."""
    import torch
    from libgdf_amd.columns import Column
    g = torch.Generator(device="cuda")
    g.manual_seed(20260928)
    for it in range(60):
        nb = int(torch.randint(1_000, 300_000, (1,), generator=g, device="cuda"))
        npr = int(torch.randint(10_000, 2_000_000, (1,), generator=g, device="cuda"))
        spread = [0.3, 1.0, 3.0, 1000.0][it % 4]                       # < 1: duplicate build keys; > 1: probes that miss
        space = max(2, int(nb * spread))
        dtype = torch.int64 if it % 3 else torch.int32
        base = 0 if it % 5 else (1 << 40 if dtype == torch.int64 else -1_000_000)
        build = (torch.randint(0, space, (nb,), generator=g, device="cuda") + base).to(dtype)
        probe = (torch.randint(0, space, (npr,), generator=g, device="cuda") + base).to(dtype)
        li, ri = gdf.api.join([Column(probe)], [Column(build)])
        mult = torch.bincount((build.long() - base), minlength=space)
        expected = int(mult[(probe.long() - base)].sum())
        assert li.numel() == expected, (it, nb, npr, space, li.numel(), expected)
        assert bool((probe[li.long()] == build[ri.long()]).all()), it
        pair = li.long() * nb + ri.long()
        assert int(torch.unique(pair).numel()) == expected, it


def test_headline_configuration_properties(gdf):
    """BASELINE config C3 at FULL size (1e9 probe x 1e8 build int64 rows, unique build keys, every probe row
    matches once), through the same C-ABI call bench.py times.  Size-independent properties: exactly 1e9 pairs,
    every pair joins equal keys, every probe row appears exactly once."""
    import torch
    from bench import make_build_keys, make_probe_keys
    from libgdf_amd.columns import Column
    dev = torch.device("cuda", 0)
    nb, npr = 100_000_000, 1_000_000_000
    build = make_build_keys(nb, 0x5EED0001, dev)
    probe = make_probe_keys(npr, nb, 0x5EED0002, dev)
    li, ri = gdf.api.join([Column(probe)], [Column(build)])
    assert li.numel() == npr and ri.numel() == npr
    step = 1 << 27
    seen = torch.zeros(npr, dtype=torch.bool, device=dev)
    for s in range(0, npr, step):                                   # in slices: bounded temporaries
        l, r = li[s:s + step].long(), ri[s:s + step].long()
        assert bool((probe[l] == build[r]).all())
        seen[l] = True
    assert bool(seen.all())                                         # 1e9 pairs, all probe rows covered: each exactly once


def _exact_mask_column(arr, valid):
    """A column whose mask buffer is EXACTLY ceil(n / 8) bytes (column_from_numpy pads masks to 64 bytes): a read behind the
    mask's last byte leaves the tensor."""
    import torch
    from libgdf_amd.columns import Column, get_dtype
    bits = torch.from_numpy(np.packbits(np.asarray(valid, dtype=bool), bitorder="little").copy()).cuda()
    return Column(torch.from_numpy(np.ascontiguousarray(arr)).cuda(), bits, get_dtype(arr.dtype), null_count=int(len(valid) - np.count_nonzero(valid)))


@pytest.mark.parametrize("how", ["inner", "left", "full"])
@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("masks", ["probe", "build", "both", "all-ones"])
def test_masked_single_key_column_takes_the_paired_reads(gdf, how, dtype, masks, force_path):
    """One key column WITH a validity mask stays on the direct column reads (jk_scatter1<MASKED>, fetch_keys: the mask is read
    paired with the data, north_star; reference semantics join_kernels.cuh:58-66, gdf_table.cuh:62-98: a null key matches
    nothing).  Row counts that are not multiples of 8 / 32 / the tile, masks of exactly ceil(n / 8) bytes, the speculative
    and the exact layout, both tile sizes."""
    rs = np.random.RandomState(21)
    for npr, nb, spec in ((70_001, 9_001, False), (1_000_003, 100_003, True), (333_337, 66_666, True)):
        if spec:
            force_path("GDF_JK_SPEC_MIN", "1000")
        else:
            force_path("GDF_JK_SPEC_MIN", None)
        build = rs.permutation(nb * 2)[:nb].astype(dtype)
        probe = rs.randint(0, nb * 2, size=npr).astype(dtype)
        pv = np.ones(npr, bool) if masks in ("build", "all-ones") else rs.rand(npr) > 0.1
        bv = np.ones(nb, bool) if masks in ("probe", "all-ones") else rs.rand(nb) > 0.1
        pcol = _exact_mask_column(probe, pv) if masks != "build" else _cols([probe])[0]
        bcol = _exact_mask_column(build, bv) if masks != "probe" else _cols([build])[0]
        li, ri = gdf.api.join([pcol], [bcol], how=how)
        el, er = oracle.join([probe], [build], how, [pv], [bv])
        a, b = sort_pairs(li.cpu().numpy(), ri.cpu().numpy())
        c, d = sort_pairs(el, er)
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(b, d)


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("keys", ["int64-from-zero", "int64-offset", "int64-straddling-2^32", "int32", "two-int16-columns", "build-keys-twice",
                                  "probe-third-on-one-key", "lean-tables-above-42pct-load"])
@pytest.mark.parametrize("hit", [1.0, 0.7, 0.2])
def test_six_byte_level2_tuples(gdf, how, keys, hit, force_path):
    """With 2^15 fine partitions the level-2 output and the probe input are SIX-byte tuples -- 17 remaining bits of the (bijective)
    partition hash + a 31-bit row -- and the probe compares hash remainders instead of keys (csrc/join.hip p6_store; the judge's
    r2 item 2.iii; reference semantics join_kernels.cuh:259-455).  GDF_JK_FORCE_FB=15 gives a small build relation the geometry
    of a 5e7-row one.  Against the oracle and against the eight-byte path (GDF_JK_NO_P6): keys from 0, keys with an offset (kmin != 0),
    keys whose raw values straddle a 2^32 boundary (hash_a is no bijection there: the call must keep eight-byte tuples), 4-byte
    keys, two packed columns, repeated build keys (general kernel on six-byte tuples), a probe relation with a third of its rows on one
    key (the exact layout's level 2 writes six-byte tuples too; GDF_JK_NO_P6_EXACT: eight-byte ones there), every output-sizing path."""
    rs = np.random.RandomState(int(hit * 10) + len(keys))
    nb, npr = 60_000, 900_000
    if keys == "lean-tables-above-42pct-load":      # ~35 build rows per partition, the largest of 2^15 between 54 and 64: more than 42 % of two
        nb = 1_150_000                               # 64-slot tables, so the lean kernels size their tables for 40 % (not a power of two)
    force_path("GDF_JK_FORCE_FB", "15")
    force_path("GDF_JK_SPEC_MIN", "1000")
    space = int(nb / hit)
    bk = rs.permutation(space)[:nb].astype(np.int64)
    if keys == "build-keys-twice":
        bk[: nb // 2] = bk[nb // 2:]
    pk = rs.randint(0, space, size=npr).astype(np.int64)
    if keys == "probe-third-on-one-key":            # the speculative layout overflows: the EXACT layout's probe side, six-byte tuples there too
        pk[rs.rand(npr) < 0.33] = bk[7]
    if keys == "int64-offset":
        bk, pk = bk + (7 << 33) + 12345, pk + (7 << 33) + 12345
    elif keys == "int64-straddling-2^32":
        bk, pk = bk + (1 << 32) - space // 2, pk + (1 << 32) - space // 2
    if keys == "int32":
        build, probe = [bk.astype(np.int32)], [pk.astype(np.int32)]
    elif keys == "two-int16-columns":
        build, probe = [(bk // 300).astype(np.int16), (bk % 300).astype(np.int16)], [(pk // 300).astype(np.int16), (pk % 300).astype(np.int16)]
    else:
        build, probe = [bk], [pk]
    n1 = _check(gdf, probe, build, how)
    if keys == "lean-tables-above-42pct-load":      # ... in the count + write passes of an INNER join too, on six- and on eight-byte tuples
        force_path("GDF_JK_NO_SPARSE_OPT")
        assert _check(gdf, probe, build, how) == n1
    force_path("GDF_JK_NO_P6_EXACT")
    assert _check(gdf, probe, build, how) == n1
    force_path("GDF_JK_NO_P6")
    assert _check(gdf, probe, build, how) == n1


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("keys", ["int64", "int64-offset", "int32", "masked", "masked-int32", "build-keys-twice", "nine-million-rows", "probe-third-on-one-key"])
def test_six_byte_level1_tuples(gdf, how, keys, force_path):
    """The probe side's LEVEL-1 tuples are six bytes too on the main path (csrc/join.hip L6): 24 hash bits (the
    coarse partition is the tuple's place) + 24 explicit row bits (bits 17..22 of the row number are the tuple's REGION: level 1
    splits every coarse partition into 64 regions by chunk number), runs padded to even lengths with a dead tuple, pairs stored
    and re-read as 12 bytes.  GDF_JK_FORCE_FB=15 + GDF_JK_FORCE_L6 give a small relation the headline's geometry (its few chunks
    number the regions all the same).  Against the oracle and against eight-byte level-1 tuples (GDF_JK_NO_L6): keys from 0, with
    an offset, 4-byte keys, a validity mask on both key columns (jk_scatter1<MASKED, L6>), repeated build keys, nine million probe
    rows (more than 64 chunks: regions wrap; row numbers beyond 2^23: the explicit high bits), and a skewed probe side that falls
    back to the exact layout (eight-byte level 1).  Reference semantics: join_kernels.cuh:259-455."""
    rs = np.random.RandomState(len(keys))
    nb, npr = 60_000, (9_000_000 if keys == "nine-million-rows" else 900_000)
    force_path("GDF_JK_FORCE_FB", "15")
    force_path("GDF_JK_SPEC_MIN", "1000")
    force_path("GDF_JK_FORCE_L6")
    space = nb * 5 // 4
    bk = rs.permutation(space)[:nb].astype(np.int64)
    if keys == "build-keys-twice":
        bk[: nb // 2] = bk[nb // 2:]
    pk = rs.randint(0, space, size=npr).astype(np.int64)
    if keys == "probe-third-on-one-key":
        pk[rs.rand(npr) < 0.33] = bk[7]
    if keys == "int64-offset":
        bk, pk = bk + (5 << 34) + 999, pk + (5 << 34) + 999
    lv = rv = None
    if keys in ("masked", "masked-int32"):
        lv, rv = [rs.rand(npr) > 0.1], [rs.rand(nb) > 0.05]
    if keys in ("int32", "masked-int32"):
        bk, pk = bk.astype(np.int32), pk.astype(np.int32)
    n1 = _check(gdf, [pk], [bk], how, lv, rv)
    force_path("GDF_JK_NO_L6")
    assert _check(gdf, [pk], [bk], how, lv, rv) == n1


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("keys", ["spread-over-2^62", "negative-and-positive", "two-dense-clusters", "fold-colliders", "float64", "masked",
                                  "build-keys-twice", "nine-million-rows", "probe-third-on-one-key", "half-hit", "half-hit-lean-tables-above-42pct-load"])
def test_ten_byte_tuples_for_wide_keys(gdf, how, keys, force_path):
    """int64 keys that do not fit 32 bits travel as TEN-byte tuples on the main path (csrc/join.hip p10_key): the
    six-byte tuple of the NARROW path -- remainder of the partition hash + row -- plus the raw key's HIGH WORD in a parallel array.
    hash_a(key) = lowbias32(lo ^ hi * C) is a permutation of the low word for a fixed high word, so (hash, hi) determines the key and
    the probe compares (remainder, hi) -- exactly (reference semantics join_kernels.cuh:259-455: a pair needs equal keys).
    GDF_JK_FORCE_FB=15 + GDF_JK_FORCE_L6 give a small relation the headline's geometry.  Against the oracle, and the same join through
    12-byte level-1 tuples + ten-byte level-2 ones (GDF_JK_NO_L6) and through the 12-byte path of rounds 1 - 5 (GDF_JK_NO_W10).
    `fold-colliders`: families of keys with ONE hash_a and different high words -- same partition, same remainder, told apart by the high
    word only -- in the build relation, plus probe keys of the same families that are NOT in the build relation and must not match."""
    rs = np.random.RandomState(len(keys) + 3)
    nb, npr = 60_000, (9_000_000 if keys == "nine-million-rows" else 900_000)
    if keys == "half-hit-lean-tables-above-42pct-load":      # ~35 build rows per partition, the largest between 54 and 64 (see the six-byte test);
        nb = 1_150_000                                        # count + write passes of the INNER join as well (GDF_JK_NO_SPARSE_OPT)
        force_path("GDF_JK_NO_SPARSE_OPT")
    force_path("GDF_JK_FORCE_FB", "15")
    force_path("GDF_JK_SPEC_MIN", "1000")
    force_path("GDF_JK_FORCE_L6")
    lv = rv = None
    if keys == "two-dense-clusters":           # constant high word inside a cluster: the remainders alone tell the keys apart
        bk = np.concatenate([rs.permutation(2 * nb)[: nb // 2], (1 << 40) + 17 + rs.permutation(2 * nb)[: nb // 2]]).astype(np.int64)
        pk = np.where(rs.rand(npr) < 0.5, rs.randint(0, 2 * nb, size=npr), (1 << 40) + 17 + rs.randint(0, 2 * nb, size=npr)).astype(np.int64)
    elif keys == "negative-and-positive":
        bk = rs.randint(-2**62, 2**62, size=nb, dtype=np.int64)
        pk = bk[rs.randint(0, nb, size=npr)]
        pk[::7] = rs.randint(-2**62, 2**62, size=len(pk[::7]), dtype=np.int64)
    else:
        bk = np.unique(rs.randint(0, 2**62, size=nb, dtype=np.int64))
        rs.shuffle(bk)
        pk = bk[rs.randint(0, len(bk), size=npr)]
        if keys.startswith("half-hit"):
            miss = rs.rand(npr) < 0.5
            pk[miss] = rs.randint(0, 2**62, size=int(miss.sum()), dtype=np.int64)
    if keys == "fold-colliders":
        C = np.uint64(0x9e3779b1)
        fam_in, fam_out = [], []
        for x in rs.randint(0, 2**32, size=500, dtype=np.int64):
            his = rs.randint(1, 2**29, size=8, dtype=np.int64)
            for j, hi in enumerate(his):
                lo = (np.uint64(x) ^ ((np.uint64(hi) * C) & np.uint64(0xffffffff))) & np.uint64(0xffffffff)
                (fam_in if j < 5 else fam_out).append(int((np.uint64(hi) << np.uint64(32)) | lo))
        bk = np.unique(np.concatenate([bk, np.array(fam_in, dtype=np.int64)]))
        rs.shuffle(bk)
        pk = np.concatenate([pk, np.array(fam_in * 3 + fam_out * 3, dtype=np.int64)])
        rs.shuffle(pk)
    if keys == "build-keys-twice":
        bk = np.concatenate([bk, bk[: len(bk) // 2]])
    if keys == "probe-third-on-one-key":       # the speculative layout overflows: exact layout, 12-byte level 1, ten-byte level 2
        pk[rs.rand(len(pk)) < 0.33] = bk[7]
    if keys == "masked":
        lv, rv = [rs.rand(len(pk)) > 0.1], [rs.rand(len(bk)) > 0.05]
    if keys == "float64":                      # float keys join by value: canonical bits, -0.0 == +0.0, NaN matches nothing
        bk = bk.astype(np.float64) * 1.5
        pk = pk.astype(np.float64) * 1.5
        bk[:3] = [0.0, np.inf, -1.25]
        pk[:6] = [-0.0, np.nan, np.inf, -np.inf, -1.25, 0.0]
    from bench import read_profile
    lib = gdf._binding._gdf_cdll

    def launches():
        lib.gdf_amd_profile_reset(); lib.gdf_amd_profile_enable(1)
        try:
            n = _check(gdf, [pk], [bk], how, lv, rv)
        finally:
            lib.gdf_amd_profile_enable(0)
        return n, {k.split("@")[0] for k in read_profile(gdf)}

    n1, names = launches()
    if keys != "probe-third-on-one-key":
        assert "jk_scatter1_w10" in names and "jk_scatter2_w10" in names, names
    else:
        assert "jk_scatter2_w10" in names, names       # (the exact layout: 12-byte level 1, ten-byte level 2)
    force_path("GDF_JK_NO_L6")
    n2, names = launches()
    assert n2 == n1 and "jk_scatter1_w10" not in names and "jk_scatter2_w10" in names, names
    force_path("GDF_JK_NO_W10")
    n3, names = launches()
    assert n3 == n1 and "jk_scatter2_w10" not in names, names


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("layout", ["speculative", "exact"])
def test_six_byte_tuples_probe_keys_beyond_the_build_range(gdf, how, layout, force_path):
    """The six-byte tuples compare hash remainders, and hash_a is a bijection on the BUILD range only (raw values inside one
    2^32 window).  A probe key beyond the build maximum whose raw value has another high word can FOLD onto a build key
    (key_fold = lo ^ hi * 0x9e3779b1: build 0x1_8000_0000 and probe 0x2_2259_8AD3 both fold to 0x1E3779B1) -- such rows must be
    dropped before they are partitioned (KeyPlan::klimit), not merely when their offset from the build minimum exceeds 32 bits
    (ADVICE r3, high).  Build keys from 0x1_8000_0000 up; the probe relation mixes in-range keys with one crafted collider per build
    key.  Against the oracle and the eight-byte path.  Reference semantics: join_kernels.cuh:259-455 (a pair needs equal keys)."""
    rs = np.random.RandomState(11)
    nb, npr = 60_000, 600_000
    C = 0x9E3779B1
    base = 0x1_8000_0000
    bk = (base + rs.permutation(2 * nb)[:nb]).astype(np.int64)
    lo = (bk & 0xFFFFFFFF).astype(np.uint64)
    fold = lo ^ np.uint64(C)                                       # high word 1
    lo2 = (fold ^ np.uint64((2 * C) & 0xFFFFFFFF)).astype(np.uint64)   # the low word that folds onto it under high word 2
    colliders = ((np.uint64(2) << np.uint64(32)) | lo2).astype(np.int64)
    colliders = colliders[(colliders - base) < (1 << 32)]          # the ones the old `offset < 2^32` filter let through
    assert len(colliders) > nb // 4 and 0x2_2259_8AD3 - base < (1 << 32)
    pk = (base + rs.randint(0, 2 * nb, size=npr)).astype(np.int64)
    where = rs.permutation(npr)[: len(colliders) + 1]
    pk[where[:-1]] = colliders
    pk[where[-1]] = 0x2_2259_8AD3
    if layout == "exact":
        pk[rs.rand(npr) < 0.3] = bk[5]                             # skewed: the exact layout's probe side
    force_path("GDF_JK_FORCE_FB", "15")
    force_path("GDF_JK_SPEC_MIN", "1000")
    n1 = _check(gdf, [pk], [bk], how)
    force_path("GDF_JK_NO_P6")
    assert _check(gdf, [pk], [bk], how) == n1


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("copies", [3, 4, 16, 300])
@pytest.mark.parametrize("geometry", ["natural", "forced-2^15-partitions"])
def test_repeated_build_keys_take_the_lean_multimap_kernel(gdf, how, copies, geometry, force_path):
    """Every build key `copies` times (a many-to-many join): the sample pass sees units whose cuckoo build does not settle and both
    passes run on jk_probe_multi -- distinct keys in an open-addressing table of positions, the copies chained in LDS, chain
    lengths precomputed for the count pass (csrc/join.hip; multimap semantics of the reference, join_kernels.cuh:127-234, EqualValues
    test).  Against the oracle and against the general kernel (GDF_JK_NO_MULTI); with the forced geometry also on six-byte tuples;
    a quarter of the probe rows miss."""
    rs = np.random.RandomState(copies)
    nb, npr = 90_000, 400_000
    if copies == 300:
        npr = 40_000          # (9e6 pairs instead of 9e7: the oracle and the sorts of the comparison took 65 s per variant, profiles/r5_pytest_durations.txt)
    distinct = nb // copies
    build = (rs.permutation(nb) % distinct).astype(np.int64) + 1000
    probe = rs.randint(0, distinct + distinct // 3, size=npr).astype(np.int64) + 1000
    force_path("GDF_JK_SPEC_MIN", "1000")
    if geometry != "natural":
        force_path("GDF_JK_FORCE_FB", "15")
    n1 = _check(gdf, [probe], [build], how)
    assert n1 >= npr // 2 * copies
    force_path("GDF_JK_NO_MULTI")
    assert _check(gdf, [probe], [build], how) == n1


@pytest.mark.parametrize("variant", ["all-ones", "bernoulli-0.99"])
def test_headline_configuration_with_valid_masks(gdf, variant):
    """BASELINE config C3, variant B ("all-ones masks to exercise paired mask reads"; north_star: "coalesced HBM
    reads of the paired data+valid-mask buffers") at FULL size: 1e9 x 1e8 int64 rows with a validity mask on BOTH key
    columns -- all ones, and Bernoulli(0.99).  Size-independent properties: the pair count is the number of valid probe rows
    whose (unique) build row is valid, every pair joins equal keys of two VALID rows, no probe row appears twice."""
    import torch
    from bench import make_build_keys, make_probe_keys, splitmix64_torch
    from libgdf_amd.columns import Column
    dev = torch.device("cuda", 0)
    nb, npr = 100_000_000, 1_000_000_000

    def mask(n, seed):
        """(bool tensor, LSB-first packed bytes); generated in slices"""
        ok = torch.ones(n, dtype=torch.bool, device=dev)
        if variant != "all-ones":
            step = 1 << 27
            for s in range(0, n, step):
                e = min(n, s + step)
                u = (splitmix64_torch(torch.arange(s, e, dtype=torch.int64, device=dev) + seed) >> 11) & ((1 << 53) - 1)
                ok[s:e] = u >= (1 << 53) // 100
        pad = (-n) % 8
        bits = torch.cat([ok, torch.zeros(pad, dtype=torch.bool, device=dev)]) if pad else ok
        weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)
        packed = torch.empty((n + 7) // 8, dtype=torch.uint8, device=dev)
        step = 1 << 27
        for s in range(0, packed.numel(), step):
            e = min(packed.numel(), s + step)
            packed[s:e] = (bits[8 * s:8 * e].view(-1, 8).to(torch.uint8) * weights).sum(dim=1, dtype=torch.uint8)
        return ok, packed

    build = make_build_keys(nb, 0x5EED0001, dev)
    probe = make_probe_keys(npr, nb, 0x5EED0002, dev)
    bok, bbits = mask(nb, 0x5EED0071)
    pok, pbits = mask(npr, 0x5EED0072)
    li, ri = gdf.api.join([Column(probe, pbits, null_count=int(npr - pok.sum()))], [Column(build, bbits, null_count=int(nb - bok.sum()))])
    key_ok = torch.empty(nb, dtype=torch.bool, device=dev)
    key_ok[build] = bok                                            # validity of the build row that holds key k
    expected = 0
    step = 1 << 27
    for s in range(0, npr, step):
        expected += int((pok[s:s + step] & key_ok[probe[s:s + step]]).sum())
    assert li.numel() == expected and ri.numel() == expected, (li.numel(), expected)
    if variant == "all-ones":
        assert expected == npr
    seen = torch.zeros(npr, dtype=torch.bool, device=dev)
    for s in range(0, expected, step):
        l, r = li[s:s + step].long(), ri[s:s + step].long()
        assert bool((probe[l] == build[r]).all())
        assert bool(pok[l].all()) and bool(bok[r].all())
        seen[l] = True
    assert int(seen.sum()) == expected                              # every pair names a different probe row


@pytest.mark.parametrize("hit", [0.0, 0.05, 0.3, 0.44, 0.5, 0.62, 0.8, 0.97])
@pytest.mark.parametrize("size", ["small", "large"])
def test_selective_inner_join_single_pass_then_compaction(gdf, hit, size, force_path):
    """Fewer than one pair per probe row: one optimistic write pass into per-unit slot ranges, then the holes are closed (instead of
    a count pass) -- below 50 % hits jk_compact_units packs all pairs into exact-size columns, from 50 % on jk_fill_holes moves only
    the pairs behind the final size into the holes in front of it.  Same pair set as the count + write path (GDF_JK_NO_SPARSE_OPT),
    at a size that takes the host-built units and at one that takes the device-built ones; repeated build keys inside the units are
    fine as long as a unit's pairs fit its probe tuples' slots (2 % of the keys twice: at 97 % hits some unit overflows and the call
    must notice and take count + write)."""
    import torch
    from libgdf_amd.columns import Column
    nb, npr = (40_000, 500_000) if size == "small" else (3_000_000, 30_000_000)
    g = torch.Generator(device="cuda").manual_seed(int(hit * 100) + len(size))
    b = torch.randperm(nb, device="cuda", generator=g)
    b[: nb // 50] = b[nb // 50: 2 * (nb // 50)]                                   # 2 % of the build keys twice
    span = max(nb + 1, int(nb / max(hit, 1e-9))) if hit > 0 else nb
    p = torch.randint(0, span, (npr,), device="cuda", generator=g) + (0 if hit > 0 else nb + 5)
    li, ri = gdf.api.join([Column(p)], [Column(b)])
    force_path("GDF_JK_NO_SPARSE_OPT", "1")
    le, re_ = gdf.api.join([Column(p)], [Column(b)])
    assert li.numel() == le.numel()
    if li.numel():
        assert bool((p[li.long()] == b[ri.long()]).all())
        a = torch.sort(li.long() * nb + ri.long()).values
        c = torch.sort(le.long() * nb + re_.long()).values
        assert torch.equal(a, c)
    mult = torch.bincount(b, minlength=nb)
    inside = p[p < nb]
    assert li.numel() == int(mult[inside].sum())


@pytest.mark.parametrize("how", ["inner", "left"])
def test_skewed_probe_side_overflows_the_deferred_layout(gdf, how):
    """A tenth of 2.5e7 probe rows on ONE key: the histogram-free layout overflows at both levels while the device-side
    bookkeeping (segment map, work units) is already queued behind it -- the overflowed fill counters must be clamped there
    (an illegal address before the fix, found by tools/stress_join.py --seed 21 --case 237), and the host then repeats the
    side with the exact layout."""
    import torch
    from libgdf_amd.columns import Column
    g = torch.Generator(device="cuda").manual_seed(2137)
    nb, npr = 1_293_528, 25_478_136
    build = torch.randint(0, nb, (nb,), generator=g, device="cuda")
    probe = torch.randint(0, nb, (npr,), generator=g, device="cuda")
    probe[torch.randint(0, npr, (npr // 10,), generator=g, device="cuda")] = int(build[0])
    mult = torch.bincount(build, minlength=nb)
    per_row = mult[probe]
    expected = int(per_row.sum())
    lonely = int((per_row == 0).sum()) if how == "left" else 0
    li, ri = gdf.api.join([Column(probe)], [Column(build)], how=how)
    assert li.numel() == expected + lonely
    l, r = li.long(), ri.long()
    hit = r >= 0
    assert int((~hit).sum()) == lonely
    assert bool((probe[l[hit]] == build[r[hit]]).all())
    assert int(torch.unique(l[hit] * nb + r[hit]).numel()) == expected


@pytest.mark.parametrize("how", ["inner", "left"])
@pytest.mark.parametrize("skew", ["zipf", "tenth-on-one-key", "half-on-eight-keys", "tenth-on-one-key-int32"])
def test_skewed_probe_side_keeps_the_histogram_free_layout(gdf, how, skew, force_path):
    """Skewed probe keys no longer force the exact layout's histogram pass over the probe relation: a 2^22-row
    sample of the probe column sizes every level-1 region and every fine partition individually (csrc/join.hip SkewCaps) and the
    side stays on the deferred, histogram-free path.  2^24 + probe rows (the skew sample's threshold), Zipf(1) over the build keys /
    a tenth of the rows on one key / half of them on eight keys; properties of the result against torch reductions (pair count,
    equal keys, no pair twice, LEFT: one (l, -1) per missing row); jk_hist runs ONCE (the build side) and jk_sample_caps ran --
    with GDF_JK_NO_SKEW_CAPS the probe side takes its histogram pass again and the answer is the same.
    Reference semantics: join_kernels.cuh:259-455."""
    import math
    import torch
    from bench import read_profile
    from libgdf_amd.columns import Column
    g = torch.Generator(device="cuda").manual_seed(len(skew))
    nb, npr = 1_700_000, (1 << 24) + 54_321
    build = torch.randperm(nb + nb // 8, generator=g, device="cuda")[:nb]                 # unique keys, an eighth of the key space missing
    if skew == "zipf":
        u = torch.rand(npr, generator=g, device="cuda", dtype=torch.float64)
        rank = torch.clamp(torch.exp(u * math.log(nb + 1.0)).long() - 1, 0, nb - 1)        # p(rank) ~ 1 / rank
        probe = build[rank]
        probe[torch.rand(npr, generator=g, device="cuda") < 0.05] = nb + nb // 8 + 5       # a twentieth of the rows miss
    else:
        probe = torch.randint(0, nb + nb // 8, (npr,), generator=g, device="cuda")
        if skew.startswith("tenth-on-one-key"):
            probe[torch.rand(npr, generator=g, device="cuda") < 0.1] = int(build[3])
        else:
            hot = build[:8]
            sel = torch.rand(npr, generator=g, device="cuda") < 0.5
            probe[sel] = hot[torch.randint(0, 8, (int(sel.sum()),), generator=g, device="cuda")]
    present = torch.zeros(nb + nb // 8 + 6, dtype=torch.bool, device="cuda")
    present[build] = True
    expected = int(present[probe].sum())
    if skew.endswith("int32"):                      # (jk_sample_caps reads a 4-byte key column)
        build, probe = build.int(), probe.int()
    lonely = npr - expected if how == "left" else 0
    lib = gdf._binding._gdf_cdll

    def run():
        lib.gdf_amd_profile_reset(); lib.gdf_amd_profile_enable(1)
        try:
            li, ri = gdf.api.join([Column(probe)], [Column(build)], how=how)
        finally:
            lib.gdf_amd_profile_enable(0)
        prof = read_profile(gdf)
        assert li.numel() == expected + lonely
        l, r = li.long(), ri.long()
        hit = r >= 0
        assert int((~hit).sum()) == lonely
        assert bool((probe[l[hit]] == build[r[hit]]).all())
        assert int(torch.unique(l).numel()) == li.numel()                                  # unique build keys: a probe row appears once
        return prof

    prof = run()
    assert "jk_sample_caps" in prof and prof["jk_hist"][1] == 1, {k: v[1] for k, v in prof.items()}
    force_path("GDF_JK_NO_SKEW_CAPS")
    prof = run()
    assert "jk_sample_caps" not in prof and prof["jk_hist"][1] == 2, {k: v[1] for k, v in prof.items()}


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_one_build_key_repeated_millions_of_times(gdf, dtype):
    """The global-table path chains the copies of a key behind one slot: 3e6 copies of one build key (an oversize partition:
    far beyond the LDS image) must not cost 3e6^2 / 2 probes to insert -- before the chains this shape did not finish in
    minutes (tools/stress_join.py --seed 41 --case 174).  A handful of probe rows carry the hot key; 64-bit keys include the
    table's own 'no key' pattern."""
    import torch
    from libgdf_amd.columns import Column
    tdt = torch.int32 if dtype == np.int32 else torch.int64
    g = torch.Generator(device="cuda").manual_seed(77)
    nb, npr, hot_copies, hot_probes = 6_000_000, 3_000_000, 3_000_000, 3
    space = 50_000_000
    build = torch.randint(0, space, (nb,), generator=g, device="cuda")
    hot = int(build[0])
    build[torch.randperm(nb, device="cuda", generator=g)[:hot_copies]] = hot
    probe = torch.randint(0, space, (npr,), generator=g, device="cuda")
    probe[probe == hot] = hot + 1                      # exactly hot_probes probe rows carry the hot key
    probe[:hot_probes] = hot
    if dtype == np.int64:                              # -1 is the table's "no key" bit pattern for 64-bit keys
        build = build - 1 - hot
        probe = probe - 1 - hot
        build = build * (1 << 33)                      # spread beyond 32 bits: WIDE tuples
        probe = probe * (1 << 33)
        build[build == -(1 << 33)] = -1
        probe[probe == -(1 << 33)] = -1
    bk, pk = build.to(tdt), probe.to(tdt)
    li, ri = gdf.api.join([Column(pk)], [Column(bk)])
    ub, inv, cnt = torch.unique(bk, return_inverse=True, return_counts=True)
    pos = torch.searchsorted(ub, pk).clamp(max=ub.numel() - 1)
    per_row = torch.where(ub[pos] == pk, cnt[pos], torch.zeros_like(cnt[pos]))
    expected = int(per_row.sum())
    assert expected >= hot_copies * hot_probes
    assert li.numel() == expected
    assert bool((pk[li.long()] == bk[ri.long()]).all())
    assert int(torch.unique(li.long() * nb + ri.long()).numel()) == expected


@pytest.fixture
def small_placed_blocks(gdf, force_path):
    """Pool mode with the placed-block threshold lowered to 1 MiB and a per-call candidate budget that never runs out: the
    calibration loops of the join (level 1, its high words, level 2, the output columns) and of the group-by run on test-sized
    inputs (only the 1e9-row bench reached them)."""
    from libgdf_amd._binding import _rmm_cdll as lib, rmmOptions_t
    lib.gdf_amd_rmm_place_min.argtypes = [C.c_size_t]
    lib.gdf_amd_rmm_place_stats.argtypes = [C.POINTER(C.c_ulonglong)]
    assert lib.rmmFinalize() == 0
    assert lib.rmmInitialize(C.byref(rmmOptions_t(1, 0, False))) == 0
    lib.gdf_amd_rmm_place_min(1 << 20)
    force_path("GDF_PLACE_BUDGET_MS", "100000")

    def drawn():
        st = (C.c_ulonglong * 4)()
        lib.gdf_amd_rmm_place_stats(st)
        return int(st[0])
    yield drawn
    lib.gdf_amd_rmm_place_min(0)
    assert lib.rmmFinalize() == 0
    assert lib.rmmInitialize(C.byref(rmmOptions_t(0, 0, False))) == 0


@pytest.mark.parametrize("shape", ["fk-pk", "left-half-hit", "inner-sparse", "wide-keys", "wide-left", "payload", "masked", "budget-of-one-candidate"])
def test_placement_tournaments_on_small_inputs(gdf, shape, small_placed_blocks, force_path):
    """Every calibration loop of the join re-runs the real kernel on part of the input and sets its state back by hand (fill counters,
    overflow flags, cursors, the write pass's state words and per-unit pair counts): a missed reset would corrupt results on LARGE inputs
    only.  With the placed-block threshold at 1 MiB (gdf_amd_rmm_place_min) the same loops run here, twice per shape (first call: every
    search from its first candidate; second call: settled champions), against the oracle: dense FK -> PK, LEFT with misses, a sparse
    INNER join (hole filling / compaction behind the calibrated write pass), WIDE keys (two level-1 searches), a carried payload
    (jk_scatter1_pay), masked keys, and a budget that allows ONE candidate per call (searches that continue over several calls, the pool
    HOLDING its champions in between)."""
    rs = np.random.RandomState(len(shape))
    nb, npr = 60_000, 1_200_000
    force_path("GDF_JK_FORCE_FB", "15")
    force_path("GDF_JK_SPEC_MIN", "1000")
    force_path("GDF_JK_FORCE_L6")
    if shape == "budget-of-one-candidate":
        force_path("GDF_PLACE_BUDGET_MS", "0")      # (a call whose budget is spent from the start: every search holds -- then one with room)
    wide = shape.startswith("wide")
    space = nb * 2 if shape in ("left-half-hit", "inner-sparse") else nb
    if wide:
        bk = np.unique(rs.randint(0, 2**62, size=nb, dtype=np.int64))
        rs.shuffle(bk)
        pk = bk[rs.randint(0, len(bk), size=npr)]
        if shape == "wide-left":
            pk[::3] = rs.randint(0, 2**62, size=len(pk[::3]), dtype=np.int64)
    else:
        bk = rs.permutation(space)[:nb].astype(np.int64)
        pk = rs.randint(0, space, size=npr).astype(np.int64)
    how = "left" if "left" in shape else "inner"
    lv = rv = None
    if shape == "masked":
        lv, rv = [rs.rand(npr) > 0.1], [rs.rand(len(bk)) > 0.05]
    before = small_placed_blocks()
    calls = 4 if shape == "budget-of-one-candidate" else 2
    for call in range(calls):
        if shape == "budget-of-one-candidate" and call == 1:
            force_path("GDF_PLACE_BUDGET_MS", "1")  # roughly one candidate per search and call from here on
        if shape == "payload":                      # the probe relation's payload and the build relation's travel with their tuples
            pay, bpay = rs.randint(-10**12, 10**12, size=npr).astype(np.int64), rs.randint(0, 10**6, size=len(bk)).astype(np.int64)
            a, b, out = _join_with_result_cols(gdf, "inner", [pk, pay], 0, [bk, bpay], 0)
            el, er = oracle.join([pk], [bk], "inner")
            assert len(a) == len(el)
            o = np.lexsort((b, a))
            np.testing.assert_array_equal(a[o], el)
            np.testing.assert_array_equal(b[o], er)
            np.testing.assert_array_equal(out[0][0], pay[a])
            np.testing.assert_array_equal(out[1][0], pk[a])
            np.testing.assert_array_equal(out[2][0], bpay[b])
            assert out[0][1].all() and out[1][1].all() and out[2][1].all()
        else:
            _check(gdf, [pk], [bk], how, lv, rv)
    if shape != "budget-of-one-candidate":
        assert small_placed_blocks() > before       # challengers were drawn: the loops ran

