"""CPU: the numpy reference of hash_partition_cases.py against the oracle and the golden Murmur3 vectors, the route model against
the recorded notes of every case and boundary, and the verifier against corrupted outputs built from a correct one."""
import json
import os

import numpy as np
import pytest

import hash_partition_cases as hp
from oracle import oracle

DTYPES = [np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
_NP_OF = {"i8": np.int8, "i16": np.int16, "i32": np.int32, "i64": np.int64, "f32": np.float32, "f64": np.float64}


def _golden():
    with open(os.path.join(os.path.dirname(__file__), "golden", "murmur3_32.json")) as f:
        return json.load(f)


def test_reference_equals_golden_vectors():
    g = _golden()
    for name, rows in g["murmur3_32"].items():
        raw = np.frombuffer(bytes.fromhex("".join(r["bytes"] for r in rows)), dtype=_NP_OF[name])
        np.testing.assert_array_equal(hp.murmur3_32(raw), np.array([r["hash"] for r in rows], dtype=np.uint32))
    hc = g["hash_combine"]
    np.testing.assert_array_equal(hp.hash_combine([r["l"] for r in hc], [r["r"] for r in hc]), np.array([r["out"] for r in hc], dtype=np.uint32))
    for name, rows in g["identity"].items():
        vals = np.array([r["v"] for r in rows], dtype=_NP_OF[name])
        np.testing.assert_array_equal(hp.identity_hash(vals), np.array([r["out"] for r in rows], dtype=np.uint32))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("hash_func", [hp.MURMUR3, hp.IDENTITY])
def test_reference_equals_oracle_on_every_recipe(dtype, hash_func):
    ident = hash_func == hp.IDENTITY
    arrays = [hp.specials(dtype, ident), hp.fill(dtype, 5003, 3, ident)] + [hp.skewed(dtype, 2001, s, 5, ident) for s in hp.SKEWS]
    for a in arrays:
        np.testing.assert_array_equal(hp.hash_rows([a], hash_func), oracle.hash_rows([a], identity=ident))
        for P in (1, 2, 3, 7, 16, 100, 1024, 1025, 16384):
            np.testing.assert_array_equal(hp.partition_ids([a], P, hash_func), oracle.partition_ids([a], P, ident))


def test_recipes_hold_what_they_promise():
    for dt in (np.float32, np.float64):
        s = hp.specials(dt, True)
        bits = hp.raw_bits(s)
        assert np.isnan(s).sum() >= 6 and len(np.unique(bits[np.isnan(s)])) >= 6                # NaN payloads are kept apart
        assert np.isinf(s).sum() == 2 and (s == 0).sum() == 2 and np.signbit(s[s == 0]).sum() == 1
        tiny = np.finfo(dt).tiny
        assert ((np.abs(s) < tiny) & (s != 0)).sum() >= 4 and np.finfo(dt).max in s and tiny in s
        assert (s >= 2.0 ** 32).sum() >= 3 and (s < 0).sum() >= 5
        h = hp.identity_hash(s)
        assert h[np.isnan(s)].max() == 0 and h[s < 0].max() == 0 and h[s >= 2.0 ** 32].min() == 0xffffffff
    assert hp.identity_hash(np.array([4294967295.5, 4294967294.999, 0.9999, 65535.5]))[:].tolist() == [4294967295, 4294967294, 0, 65535]
    assert hp.identity_hash(np.array([-1, -128], dtype=np.int8)).tolist() == [0xffffffff, 0xffffff80]
    assert hp.identity_hash(np.array([-1, 1 << 32, (1 << 32) + 5, -(1 << 33) - 2], dtype=np.int64)).tolist() == [0xffffffff, 0, 5, 0xfffffffe]
    hi = hp.raw_bits(hp.specials(np.int64)) >> np.uint64(32)
    assert len(np.unique(hi)) >= 10                                                             # varied high words
    for dt in DTYPES:
        a = hp.fill(dt, 4001, 9)
        assert set(hp.raw_bits(hp.specials(dt)).tolist()) <= set(hp.raw_bits(a).tolist())
        assert len(np.unique(hp.raw_bits(hp.skewed(dt, 999, "one", 1)))) == 1
        assert len(np.unique(hp.raw_bits(hp.skewed(dt, 999, "sparse", 1)))) <= 5
        third = hp.raw_bits(hp.skewed(dt, 9000, "third", 1))
        assert 2500 < np.bincount(np.unique(third, return_inverse=True)[1]).max()


def test_reference_equals_oracle_on_multi_column_keys():
    n = 4001
    cols = [hp.fill(dt, n, 11 + i) for i, dt in enumerate(DTYPES)]
    for pick in ([0, 1], [5, 3, 0], [2, 4], list(range(6)), [3, 3]):
        key = [cols[i] for i in pick]
        np.testing.assert_array_equal(hp.hash_rows(key), oracle.hash_rows(key))
        np.testing.assert_array_equal(hp.partition_ids(key, 300), oracle.partition_ids(key, 300))
    icols = [hp.fill(dt, n, 21 + i, True) for i, dt in enumerate(DTYPES)]
    for pick in ([0, 3], [4, 5], [5, 2, 1], list(range(6))):
        key = [icols[i] for i in pick]
        np.testing.assert_array_equal(hp.hash_rows(key, hp.IDENTITY), oracle.hash_rows(key, identity=True))
        np.testing.assert_array_equal(hp.partition_ids(key, 1000, hp.IDENTITY), oracle.partition_ids(key, 1000, True))


def test_case_ids_are_unique_and_tables_have_row_ids():
    ids = [c.id for c in hp.ALL_CASES]
    assert len(ids) == len(set(ids))
    for c in hp.ALL_CASES:
        assert c.rowid is not None or len(c.cols) == 1, c.id
        assert c.hashed and all(0 <= h < len(c.cols) for h in c.hashed)


@pytest.mark.parametrize("case", hp.ALL_CASES, ids=repr)
def test_route_model_gives_the_recorded_notes(case):
    assert case.model() == case.expect
    if hasattr(case, "free_nchunks"):                   # the same request without the selector: only the chunk count changes, and on two levels the pieces
        free = case.model({})
        assert free["hp.route"] == case.expect["hp.route"] and free["hp.nchunks"] == case.free_nchunks


@pytest.mark.parametrize("args,notes", hp.MODEL_BOUNDARIES, ids=lambda v: None)
def test_route_model_at_the_dispatch_boundaries(args, notes):
    dtypes, im, om, hashed, hf, P, n, forced = args
    assert hp.route_model(dtypes, set(im), set(om), hashed, hf, P, n, forced) == notes


def test_chunk_layouts_of_the_selector():
    """GDF_HP_MAX_CHUNKS = 16: 15 chunks of 24576 / 32768 rows and a last chunk of one row; in tiles of every regrouping kernel"""
    assert hp.chunking(hp.N3, hp.SEL) == (24576, 16) and hp.N3 - 15 * 24576 == 1
    assert hp.chunking(hp.N4, hp.SEL) == (32768, 16) and hp.N4 - 15 * 32768 == 1
    assert 24576 == 3 * hp.PAIRS_TILE == 2 * hp.TILE_FAST == 4 * hp.TILE_GENERIC and 24576 * 2 == 3 * hp.COLS8_TILE
    assert 32768 == 4 * hp.PAIRS_TILE == 2 * hp.COLS8_TILE and 2 * hp.TILE_FAST < 32768 < 3 * hp.TILE_FAST and 5 * hp.TILE_GENERIC < 32768
    assert hp.chunking(hp.N3) == (2048, 181) and hp.chunking(hp.N4) == (2048, 241)


# ---------------------------------------------------------------------------------------------------------------------------------
# the verifier

def _correct(cols, masks, hashed, P, hash_func=hp.MURMUR3, seed=0):
    """a correct output: a stable sort by partition, then a random permutation inside every partition"""
    pid = hp.partition_ids([cols[c] for c in hashed], P, hash_func)
    rs = np.random.RandomState(seed)
    perm = np.lexsort((rs.rand(len(pid)), pid))
    got = [c[perm].copy() for c in cols]
    gm = [None if m is None else m[perm].copy() for m in masks]
    return got, gm, hp.reference_offsets(pid, P)


def _table(n=3001, seed=2):
    cols = [hp.fill(np.int64, n, seed), np.arange(n, dtype=np.int64), hp.fill(np.int8, n, seed + 1), hp.fill(np.int16, n, seed + 2),
            hp.fill(np.float32, n, seed + 3), hp.fill(np.float64, n, seed + 4)]
    masks = [np.random.RandomState(seed).rand(n) > 0.4, None, np.random.RandomState(seed + 1).rand(n) > 0.4, None, None, None]
    return cols, masks


@pytest.mark.parametrize("rowid", [1, None])
def test_verifier_accepts_any_order_inside_a_partition(rowid):
    cols, masks = _table()
    for seed in range(3):
        got, gm, off = _correct(cols, masks, [0], 7, seed=seed)
        hp.check_partition(cols, masks, got, gm, off, [0], 7, rowid=rowid)
    got, gm, off = _correct(cols, masks, [0, 3], 300)
    hp.check_partition(cols, masks, got, gm, off, [0, 3], 300, rowid=rowid)
    got, gm, off = _correct(cols, masks, [2], 5, hp.IDENTITY)
    hp.check_partition(cols, masks, got, gm, off, [2], 5, hp.IDENTITY, rowid=rowid)


def _corruptions():
    def swap_across(cols, got, gm, off, P):
        a, b = int(off[3]) - 1, int(off[3])                 # last row of partition 2, first of partition 3
        for g in got:
            g[[a, b]] = g[[b, a]]
        for m in gm:
            if m is not None:
                m[[a, b]] = m[[b, a]]

    def shift_offset(cols, got, gm, off, P):
        off[4] += 1

    def clear_high_byte(c):
        def f(cols, got, gm, off, P):
            u = hp.raw_bits(got[c])
            w = u.dtype.itemsize
            top = np.flatnonzero(u >> u.dtype.type(8 * (w - 1)))
            u[top[len(top) // 2]] &= u.dtype.type((1 << (8 * (w - 1))) - 1)
        return f

    def move_validity_bit(cols, got, gm, off, P):
        m = gm[2]
        i = int(np.flatnonzero(m[:-1] & ~m[1:])[5])
        m[i], m[i + 1] = False, True

    def duplicate_row(cols, got, gm, off, P):
        a = int(off[2])                                     # two rows of one partition: positions and offsets stay right
        for g in got:
            g[a + 1] = g[a]
        for m in gm:
            if m is not None:
                m[a + 1] = m[a]

    def negative_zero(cols, got, gm, off, P):
        for c in (4, 5):
            z = np.flatnonzero((got[c] == 0) & np.signbit(got[c]))
            assert len(z)
            got[c][z[0]] = 0.0

    out = [("two rows swapped across a partition boundary", swap_across), ("one offset shifted by one", shift_offset),
           ("one validity bit moved to the neighbouring row", move_validity_bit), ("one row duplicated over another", duplicate_row),
           ("-0.0 replaced by 0.0", negative_zero)]
    out += [(f"high byte of one {w}-byte payload element cleared", clear_high_byte(c)) for w, c in ((1, 2), (2, 3), (4, 4), (8, 5))]
    return out


@pytest.mark.parametrize("rowid", [1, None])
@pytest.mark.parametrize("name,corrupt", _corruptions(), ids=lambda v: v if isinstance(v, str) else None)
def test_verifier_rejects_a_corrupted_output(name, corrupt, rowid):
    cols, masks = _table()
    P = 7
    got, gm, off = _correct(cols, masks, [0], P)
    hp.check_partition(cols, masks, got, gm, off, [0], P, rowid=rowid)
    corrupt(cols, got, gm, off, P)
    with pytest.raises(AssertionError):
        hp.check_partition(cols, masks, got, gm, off, [0], P, rowid=rowid)
