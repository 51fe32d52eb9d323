"""Pins the CPU oracle before anything is compared against it (no GPU needed):
  * Murmur3_32 / hash_combine / IdentityHash against golden vectors captured from the reference's own
    header (tests/golden/murmur3_32.json and murmur3_32_sampled.json, made by tests/golden/make_golden.py), and
    -- where oracle/_ref/libref_hash.so was built -- against the reference functors live;
  * group-by and filter semantics against the known-answer vectors of the reference's sqls tests
    (tests/golden/sqls_known_answers.json);
  * the numpy expectations against the statements in the reference's python tests."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from oracle import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
NP = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLD, "murmur3_32.json")) as f:
        return json.load(f)


def test_murmur3_golden(golden):
    n = 0
    for name, entries in golden["murmur3_32"].items():
        for e in entries:
            v = np.frombuffer(bytes.fromhex(e["bytes"]), dtype=NP[name])
            assert oracle.murmur3_32(v) == e["hash"], (name, e)
            n += 1
    assert n >= 180


def test_survey_table_values():
    # SURVEY.md 8c table (captured from the reference header during the survey)
    assert oracle.murmur3_32(np.int32(0)) == 593689054
    assert oracle.murmur3_32(np.int32(1)) == 4226891818
    assert oracle.murmur3_32(np.int32(-1)) == 1982413648
    assert oracle.murmur3_32(np.int64(0)) == 1669671676
    assert oracle.murmur3_32(np.int64(1)) == 1392991556
    assert oracle.murmur3_32(np.int64(-1)) == 1651860712
    assert oracle.murmur3_32(np.int64(123456789012345)) == 3825968124
    assert oracle.murmur3_32(np.float64(1.5)) == 4034560987
    assert oracle.murmur3_32(np.float32(1.5)) == 376679366
    assert oracle.murmur3_32(np.int8(7)) == 1753412482
    assert oracle.murmur3_32(np.int16(300)) == 3578234270
    assert oracle.hash_combine(oracle.murmur3_32(np.int32(1)), oracle.murmur3_32(np.int32(2))) == 3787935720
    assert oracle.identity_hash(np.int64(0x1FFFFFFFF)) == 4294967295


def test_hash_combine_and_identity_golden(golden):
    for e in golden["hash_combine"]:
        assert oracle.hash_combine(e["l"], e["r"]) == e["out"]
    for e in golden["identity"]["i64"]:
        assert oracle.identity_hash(np.int64(e["v"])) == e["out"]
    for e in golden["identity"]["i32"]:
        assert oracle.identity_hash(np.int32(e["v"])) == e["out"]


def sampled_hash_inputs():
    """The seeded inputs of test_against_live_reference_header: 500 values of every dtype made of random bytes, then 500 hash_combine
    pairs (tests/golden/make_golden.py records the reference functors' answers on exactly these)."""
    rng = np.random.RandomState(7)
    vals = {}
    for name, dt in NP.items():
        raw = rng.randint(0, 256, size=(500, np.dtype(dt).itemsize), dtype=np.uint8)
        vals[name] = raw.view(dt).reshape(-1)
    pairs = rng.randint(0, 2**32, size=(500, 2), dtype=np.int64)
    return vals, pairs


def test_against_live_reference_header():
    """The oracle against the reference's own functors on 3,500 seeded inputs: their answers as recorded from the reference header
    (tests/golden/murmur3_32_sampled.json), and live as well where oracle/_ref/libref_hash.so was built."""
    vals, pairs = sampled_hash_inputs()
    with open(os.path.join(GOLD, "murmur3_32_sampled.json")) as f:
        rec = json.load(f)
    for name, v in vals.items():
        assert [oracle.murmur3_32(v[i:i + 1]) for i in range(len(v))] == rec["murmur3_32"][name], name
    assert [oracle.hash_combine(int(l), int(r)) for l, r in pairs] == rec["hash_combine"]
    path = os.path.join(HERE, "..", "oracle", "_ref", "libref_hash.so")
    if not os.path.exists(path):
        return
    ref = C.CDLL(path)
    for name, dt in NP.items():
        fn = getattr(ref, "ref_murmur_" + name)
        fn.restype = C.c_uint32
        fn.argtypes = [C.c_void_p]
        v = vals[name]
        for i in range(len(v)):
            assert oracle.murmur3_32(v[i:i + 1]) == fn(v[i:i + 1].ctypes.data)
    ref.ref_hash_combine.restype = C.c_uint32
    ref.ref_hash_combine.argtypes = [C.c_uint32, C.c_uint32]
    for l, r in pairs:
        assert oracle.hash_combine(int(l), int(r)) == ref.ref_hash_combine(int(l), int(r))


def test_row_hash_folds_columns_left_to_right():
    a = np.array([1, 5, 1], dtype=np.int32)
    b = np.array([2, 6, 2], dtype=np.int32)
    h = oracle.hash_rows([a, b])
    assert h[0] == 3787935720 and h[0] == h[2] and h[0] != h[1]
    assert oracle.hash_rows([a])[0] == 4226891818          # first column is not combined (gdf_table.cuh:730-733)


@pytest.fixture(scope="module")
def sqls():
    with open(os.path.join(GOLD, "sqls_known_answers.json")) as f:
        return json.load(f)


def test_group_by_known_answers(sqls):
    g = sqls["group_by"]
    keys = [np.array(g["keys"][c]["values"], dtype=g["keys"][c]["dtype"]) for c in ("c0", "c1", "c2")]
    for case in g["cases"]:
        vals = np.array(case["agg"]["values"], dtype=case["agg"]["dtype"])
        out_keys, agg = oracle.group_by(case["op"], keys, vals, out_dtype=case["out_dtype"])
        for c, name in zip(out_keys, ("c0", "c1", "c2")):
            assert list(c) == g["expected_keys"][name], case["ref"]
        assert list(agg) == case["expected"], case["ref"]


def test_sort_method_known_answers(sqls):
    """GDF_SORT restatement (oracle.group_by_sort / order_by) vs the reference's own vectors, INCLUDING the row
    index per group (sqls_g_tester.cu:250-256) and the order-by permutation (sqls_tests_new_api.dat:1-2)."""
    g = sqls["group_by"]
    keys = [np.array(g["keys"][c]["values"], dtype=g["keys"][c]["dtype"]) for c in ("c0", "c1", "c2")]
    for case in g["cases"]:
        vals = np.array(case["agg"]["values"], dtype=case["agg"]["dtype"])
        out_keys, agg, idx = oracle.group_by_sort(case["op"], keys, vals, out_dtype=case["out_dtype"])
        for c, name in zip(out_keys, ("c0", "c1", "c2")):
            assert list(c) == g["expected_keys"][name], case["ref"]
        assert list(agg) == case["expected"], case["ref"]
        assert list(idx) == g["expected_first_rows"], case["ref"]
    ob = sqls["order_by"]
    cols = [np.array(ob["cols"]["c0"], dtype=np.int32), np.array(ob["cols"]["c1"], dtype=np.int32),
            np.array(ob["cols"]["c2"], dtype=np.float64)]
    assert list(oracle.order_by(cols)) == ob["expected_permutation"]


def test_sort_and_hash_restatements_agree():
    keys = [np.random.randint(0, 7, 500).astype(np.int32), np.random.randint(-3, 3, 500).astype(np.int8)]
    for op, dt, od in (("sum", np.int64, None), ("min", np.float32, None), ("max", np.int16, None), ("count", np.int32, np.int64)):
        vals = (np.random.random(500) * 200 - 100).astype(dt)
        hk, ha = oracle.group_by(op, keys, vals, od)
        sk, sa, _ = oracle.group_by_sort(op, keys, vals, od)
        for a, b in zip(hk, sk):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(ha, sa)


def test_filter_known_answer(sqls):
    f = sqls["filter"]
    cols = [np.array(f["cols"][c]["values"], dtype=f["cols"][c]["dtype"]) for c in ("c0", "c1", "c2")]
    idx = oracle.filter_rows(cols, f["tuple"])
    assert len(idx) == f["expected_size"] and list(idx) == f["expected_indices"]


def test_comparison_conversions_known_answers():
    """oracle.comparison on answers derived by hand from C's usual arithmetic conversions (the GPU tests compare the kernels with it on
    exactly these values, so it must not be right only by agreeing with them).  Operators in enum order: ==, !=, <, <=, >, >=."""
    def cmp(l, r):
        return [int(oracle.comparison(np.array([l]), np.array([r]), op)[0]) for op in range(6)]

    EQUAL, LESS, GREATER, UNORDERED = [1, 0, 0, 1, 0, 1], [0, 1, 1, 1, 0, 0], [0, 1, 0, 0, 1, 1], [0, 1, 0, 0, 0, 0]
    # (int32, float32) compares in float32: 2^24 + 1 lies half way between 2^24 and 2^24 + 2 and rounds to the even mantissa, 2^24
    assert cmp(np.int32(2**24 + 1), np.float32(2**24)) == EQUAL
    assert cmp(np.float32(2**24), np.int32(2**24 + 1)) == EQUAL
    assert cmp(np.int32(2**24 + 2), np.float32(2**24)) == GREATER          # (2^24 + 2 is a float32)
    # (int64, float64) compares in float64: 2^53 + 1 rounds to 2^53
    assert cmp(np.int64(2**53 + 1), np.float64(2**53)) == EQUAL
    assert cmp(np.int64(2**53 + 2), np.float64(2**53)) == GREATER
    # (int64, float32) compares in float32 -- numpy's own promotion would be float64, where 2^24 + 1 is exact and greater
    assert cmp(np.int64(2**24 + 1), np.float32(2**24)) == EQUAL
    assert cmp(np.float32(2**24), np.int64(2**24 + 1)) == EQUAL
    assert cmp(np.int64(2**24 + 1), np.float64(2**24)) == GREATER
    # ... and to nearest EVEN: 2^24 + 3 lies half way between 2^24 + 2 (odd mantissa) and 2^24 + 4 (even) and goes up
    assert cmp(np.int64(2**24 + 3), np.float32(2**24 + 4)) == EQUAL
    assert cmp(np.int64(2**24 + 3), np.float32(2**24 + 2)) == GREATER
    assert cmp(np.int64(2**63 - 1), np.float32(2.0**63)) == EQUAL           # the int64 maximum rounds up to 2^63
    # integers of two widths compare by value (sign extension)
    assert cmp(np.int8(-128), np.int64(-128)) == EQUAL
    assert cmp(np.int8(-1), np.int32(2**31 - 1)) == LESS
    assert cmp(np.int64(-(2**63)), np.int8(-128)) == LESS
    # NaN is unordered: only != holds, whichever side holds it and whatever the other type
    for nan in (np.float32(np.nan), np.float64(np.nan)):
        for other in (np.int8(0), np.int64(2**62), np.float32(np.inf), np.float64(-0.0), nan):
            assert cmp(nan, other) == UNORDERED and cmp(other, nan) == UNORDERED
    # the two zeros are equal
    for f in (np.float32, np.float64):
        assert cmp(f(-0.0), f(0.0)) == EQUAL and cmp(f(0.0), f(-0.0)) == EQUAL
        assert cmp(f(-0.0), np.int32(0)) == EQUAL
    # a scalar right-hand side converts like a column
    assert list(oracle.comparison(np.array([2**24 + 1, 2**24 + 3], dtype=np.int64), np.float32(2**24), 0)) == [1, 0]


def test_prefixsum_matches_numpy_statement():
    for dt in (np.int8, np.int32, np.int64):
        for n in (1, 2, 13, 64, 100, 1000):           # python/tests/test_prefixsum.py:16-62
            a = np.random.randint(-100, 100, size=n).astype(dt)
            np.testing.assert_array_equal(oracle.prefixsum(a, True), np.cumsum(a, dtype=dt))
            ex = oracle.prefixsum(a, False)
            assert ex[0] == 0 and np.array_equal(ex[1:], np.cumsum(a, dtype=dt)[:-1])


def test_int8_sum_wraps_in_input_dtype():
    keys = [np.zeros(4, dtype=np.int32)]
    vals = np.array([100, 100, 100, 27], dtype=np.int8)          # 327 -> 71 (mod 256)
    _, agg = oracle.group_by("sum", keys, vals)
    assert agg.dtype == np.int8 and agg[0] == np.int8(71)
    _, avg = oracle.group_by("avg", keys, vals, out_dtype=np.float64)
    assert avg[0] == 71 / 4.0                                      # sum wraps BEFORE the division (groupby.cuh:308-328)
    _, avgi = oracle.group_by("avg", keys, vals, out_dtype=np.int32)
    assert avgi[0] == 71 // 4


def test_fnv1a_restatement_against_published_vectors():
    """gpu_hash_columns is FNV-1a 64 (hashops.cu:40-75).  The reference source cannot be compiled here (thrust +
    CUDA runtime headers), so the restatement is pinned on the PUBLISHED FNV-1a test vectors (Fowler/Noll/Vo, isthe.com
    test suite): "" -> cbf29ce484222325, "a" -> af63dc4c8601ec8c, "foobar" -> 85944171f73967e8; each character is
    one int8 column, which is exactly how the reference folds columns."""
    def h(text):
        cols = [np.array([ord(ch)], dtype=np.int8) for ch in text] or [np.zeros((1, 0), dtype=np.int8).reshape(1, 0)[:, :0].ravel()]
        return int(oracle.fnv1a_rows(cols)[0]) if text else 14695981039346656037
    assert h("") == 0xcbf29ce484222325
    assert h("a") == 0xaf63dc4c8601ec8c
    assert h("foobar") == 0x85944171f73967e8
    # one int32 column holding "foob" little-endian hashes like the four characters
    word = np.array([int.from_bytes(b"foob", "little")], dtype=np.int32)
    assert int(oracle.fnv1a_rows([word])[0]) == h("foob")
    # the reference's signed-char quirk: a byte >= 0x80 is sign-extended before the XOR
    x = np.array([-1], dtype=np.int8)
    exp = ((14695981039346656037 ^ 0xFFFFFFFFFFFFFFFF) * 1099511628211) % (1 << 64)
    assert int(oracle.fnv1a_rows([x])[0]) == exp
