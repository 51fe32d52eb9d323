"""prefixsum_cases.py on the CPU: the reference against oracle.prefixsum, what the value recipes promise, the dispatch model against rows
worked out by hand from csrc/scan.hip, and every entry of the size tables against the geometry it is named for."""
import numpy as np
import pytest

import prefixsum_cases as pc
from oracle import oracle

T = pc.LB_TILE


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_reference_is_the_oracle(dtype):
    rng = np.random.default_rng(5)
    for n in (1, 2, 1000):
        a = pc.RECIPES["full"](dtype, n, rng)
        for inc in (True, False):
            got = pc.reference(a, inc)
            assert got.dtype == np.dtype(dtype) and np.array_equal(got, oracle.prefixsum(a, inc))
    a, inc = pc.values_and_scan("full", dtype, 5000)
    assert np.array_equal(inc[:777], pc.reference(a[:777], True))          # a prefix of the scan is the scan of the prefix
    assert not a.flags.writeable and not inc.flags.writeable
    assert pc.values_and_scan("full", dtype, 5000)[0] is a


def test_constants_are_the_sources():
    """the model's constants are READ from csrc/scan.hip: a changed tile or threshold has to be changed here too"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libgdf_amd", "csrc", "scan.hip")).read()

    def const(name):
        return re.search(r"constexpr \w+ " + name + r" = ([^;]+);", src).group(1).strip()

    assert const("SCAN_THREADS") == "256" and const("LB_THREADS") == "256" and pc.THREADS == 256
    assert const("LB_ITEMS") == "16" and const("LB_TILE") == "LB_THREADS * LB_ITEMS" and pc.LB_TILE == 256 * 16
    assert const("SCAN_MAX_CHUNKS") == "2048" and pc.MAX_CHUNKS == 2048
    assert const("SCAN_ROUNDS_MIN") == "(size_t)1 << 22" and pc.ROUNDS_MIN == 1 << 22
    assert "constexpr int ITEMS = 16 / sizeof(ELEM) >= 4 ? 8 : 4;" in src
    assert [pc.elementwise_tile(d) for d in pc.DTYPES] == [2048, 2048, 1024]
    assert [pc.vec(d) for d in pc.DTYPES] == [16, 4, 2]
    assert "grid > (size_t)4 * LB_THREADS" in src and pc.MAX_GRID == 1024
    assert "page += PT * LB_THREADS" in src and "constexpr int PT = 2;" in src and pc.POLL_PAGE == 512
    for name in pc.NOTE_NAMES:
        assert f'"{name}"' in src
    for name in pc.SWITCH_NAMES:
        assert f'"{name}"' in src


# --- recipes ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_full_wraps_within_the_smallest_tables(dtype):
    a, inc = pc.values_and_scan("full", dtype, 3 * T)
    ii = np.iinfo(dtype)
    assert a.dtype == np.dtype(dtype) and a.min() < ii.min // 2 and a.max() > ii.max // 2
    assert pc.wraps(a[:pc.THREADS - 1], inc[:pc.THREADS - 1]) > 0          # already inside the smallest multi-element sizes
    for t in range(3):                                                    # and inside every tile
        s = slice(t * T, (t + 1) * T)
        assert pc.wraps(a[s], np.cumsum(a[s], dtype=a.dtype)) > T // 8
    if np.dtype(dtype) == np.int64:                                       # arbitrary high words in the tile aggregates
        hi = (inc[T - 1::T].view(np.uint64) >> np.uint64(32)).astype(np.uint32)
        assert all(h not in (0, 0xffffffff) for h in hi)


def test_half_word_carries_out_of_the_low_word():
    n = 1025 * T + 7
    a, inc = pc.values_and_scan("half-word", np.int64, n)
    assert set(np.unique(a)) == set(pc.HALF_WORD_VALUES)
    assert pc.low_word_carries(a, inc) > n // 8                            # (half the values have a low word near 2^32, prefix uniform)
    # the tiles' aggregates: added to the running prefix they carry at about every second tile, and every tile carries inside
    m = np.uint64(0xffffffff)
    agg = np.add.reduceat(a[:1025 * T].view(np.uint64), np.arange(0, 1025 * T, T))
    before = np.concatenate([[np.uint64(0)], np.cumsum(agg)[:-1]])
    carried = np.count_nonzero((before & m) + (agg & m) > m)
    assert carried > 1025 // 3, carried
    for t in (0, 1, 512, 1024):
        s = slice(t * T, (t + 1) * T)
        assert pc.low_word_carries(a[s], inc[s]) > T // 8
    hi = (agg >> np.uint64(32)).astype(np.uint32)
    assert np.count_nonzero((hi != 0) & (hi != 0xffffffff)) > 1000


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_constant_recipes(dtype):
    ii = np.iinfo(dtype)
    rng = np.random.default_rng(1)
    n = 1000
    a = pc.RECIPES["minus-one"](dtype, n, rng)
    assert np.array_equal(pc.reference(a, True), (-np.arange(1, n + 1)).astype(dtype))
    a = pc.RECIPES["type-min"](dtype, n, rng)
    inc = pc.reference(a, True)
    assert (inc[1::2] == 0).all() and (inc[0::2] == ii.min).all()
    a = pc.RECIPES["ones"](dtype, n, rng)
    assert np.array_equal(pc.reference(a, False), np.arange(n).astype(dtype))
    a = pc.RECIPES["small"](dtype, n, rng)
    assert a.min() >= -100 and a.max() < 100 and a.dtype == np.dtype(dtype)
    assert ("half-word" in pc.recipes_for(dtype)) == (np.dtype(dtype) == np.int64)
    assert len(pc.recipes_for(dtype)) == (6 if np.dtype(dtype) == np.int64 else 5)


# --- the model -------------------------------------------------------------------------------------------------------------------

def _m(route, chunks=0, chunk=0, bailed=0):
    return {"scan.route": route, "scan.bailed": bailed, "scan.chunks": chunks, "scan.chunk_elems": chunk}


LB0, LB1, LB2, LB3 = ({"GDF_SCAN_LOOKBACK": str(i)} for i in range(4))
BLOCKED, BAIL = {"GDF_SCAN_BLOCKED": "1"}, {"GDF_SCAN_FORCE_BAIL": "1"}

HAND_ROWS = [
    # dtype, n, in_off, out_off, in_place, forced -> notes; worked out from device_scan by hand
    (np.int32, 1, 0, 0, False, {}, _m(pc.COALESCED, 1, 4096)),
    (np.int32, 4097, 0, 0, False, {}, _m(pc.COALESCED, 2, 4096)),
    (np.int64, 2048 * 4096, 0, 0, False, LB0, _m(pc.COALESCED, 2048, 4096)),
    (np.int64, 2048 * 4096 + 1, 0, 0, False, LB0, _m(pc.COALESCED, 1025, 8192)),
    (np.int8, 2048 * 4096 + 4096 + 5, 0, 0, False, {}, _m(pc.COALESCED, 1025, 8192)),        # 2050 tiles, two per chunk
    (np.int8, 3 * 2048 * 4096, 0, 0, False, {}, _m(pc.COALESCED, 2048, 12288)),
    (np.int32, (1 << 22) - 1, 0, 0, False, {}, _m(pc.COALESCED, 1024, 4096)),
    (np.int32, 1 << 22, 0, 0, False, {}, _m(pc.ROUNDS)),
    (np.int64, 1 << 22, 0, 0, False, {}, _m(pc.ROUNDS)),
    (np.int8, 1 << 22, 0, 0, False, {}, _m(pc.COALESCED, 1024, 4096)),                       # one-byte types keep the three launches
    (np.int8, 1 << 22, 0, 0, False, LB3, _m(pc.ROUNDS)),
    (np.int32, 1 << 22, 0, 0, True, {}, _m(pc.COALESCED, 1024, 4096)),                       # in place: never the rounds
    (np.int32, 1 << 22, 0, 0, True, LB3, _m(pc.COALESCED, 1024, 4096)),
    (np.int32, 1 << 22, 0, 0, True, LB1, _m(pc.LOOKBACK)),
    (np.int32, 1 << 22, 0, 0, False, BAIL, _m(pc.COALESCED, 1024, 4096, bailed=1)),
    (np.int32, 5000, 0, 0, False, {**LB3, **BAIL}, _m(pc.COALESCED, 2, 4096, bailed=1)),
    (np.int32, 5000, 0, 0, False, {**LB1, **BAIL}, _m(pc.LOOKBACK)),                         # the bail-out switch is the rounds' alone
    (np.int64, 5000, 0, 0, False, LB2, _m(pc.SPINE)),
    (np.int32, 4097, 0, 0, False, BLOCKED, _m(pc.ELEMENTWISE, 3, 2048)),
    (np.int64, 4097, 0, 0, False, BLOCKED, _m(pc.ELEMENTWISE, 5, 1024)),
    (np.int64, 2048 * 1024 + 1, 0, 0, False, BLOCKED, _m(pc.ELEMENTWISE, 1025, 2048)),
    (np.int32, 4097, 0, 0, False, {**BLOCKED, **LB3}, _m(pc.ELEMENTWISE, 3, 2048)),
    (np.int32, 4097, 1, 0, False, {}, _m(pc.ELEMENTWISE, 3, 2048)),                          # `in` off
    (np.int32, 4097, 0, 3, False, LB3, _m(pc.ELEMENTWISE, 3, 2048)),                         # `out` off, whatever is forced
    (np.int32, 4097, 4, 0, False, {}, _m(pc.COALESCED, 2, 4096)),                            # four int32 = 16 bytes: aligned again
    (np.int64, 1 << 22, 1, 1, True, {}, _m(pc.ELEMENTWISE, 2048, 2048)),
    (np.int64, 1 << 22, 2, 0, False, {}, _m(pc.ROUNDS)),
    (np.int8, 2049, 15, 0, False, LB1, _m(pc.ELEMENTWISE, 2, 2048)),
    (np.int8, 2049, 16, 16, True, LB2, _m(pc.SPINE)),
]


@pytest.mark.parametrize("row", HAND_ROWS, ids=lambda r: f"{np.dtype(r[0]).name}-{r[1]}-{r[2]}{r[3]}{'ip' if r[4] else ''}-" + "".join(sorted(r[5])))
def test_model_against_hand_computed_rows(row):
    dtype, n, in_off, out_off, in_place, forced, want = row
    assert pc.model(dtype, n, in_off, out_off, in_place, forced) == want


def test_chunking_by_hand():
    assert pc.chunking(1, 4096) == (1, 4096)
    assert pc.chunking(4096, 4096) == (1, 4096)
    assert pc.chunking(256 * 4096 + 1, 4096) == (257, 4096)
    assert pc.chunking(2048 * 4096 + 1, 4096) == (1025, 8192)
    assert pc.chunking(10**9, 4096) == (2035, 120 * 4096)
    assert pc.chunking(2048 * 1024 + 1024 + 5, 1024) == (1025, 2048)


# --- the size tables -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_coalesced_table_lands_on_its_geometry(dtype):
    s = pc.coalesced_sizes(dtype)
    V = pc.vec(dtype)
    for name, n in s.items():
        m = pc.model(dtype, n, forced=pc.family_forced("coalesced", dtype, n))
        assert m["scan.route"] == pc.COALESCED and m["scan.bailed"] == 0, name
    geo = {name: pc.chunking(n, T) for name, n in s.items()}
    assert s["one"] == 1 and s["vec"] == V and s["vec+1"] == V + 1 and (V == 2 or s["vec-1"] == V - 1)
    assert all(geo[k] == (1, T) for k in ("one", "vec", "vec+1", "tile-1", "tile")) and geo["tile+1"] == (2, T)
    # the second chunk: one whole vector (nvec == 1) and one element behind it for thread 0
    n = s["subvector-tail"]
    assert geo["subvector-tail"] == (2, T) and (n - T) // V == 1 and (n - T) % V == 1
    assert geo["spine-one-batch"] == (pc.SPINE_BATCH, T) and geo["spine-second-batch"] == (pc.SPINE_BATCH + 1, T)
    assert geo["max-chunks"] == (2048, T)
    # two tiles per chunk; a last chunk of one element; a last chunk of a full tile (prefetched: full, !next_full) and a partial one
    assert geo["two-tiles-per-chunk"] == (1025, 2 * T) and s["two-tiles-per-chunk"] - 1024 * 2 * T == 1
    assert geo["full-then-partial"] == (1025, 2 * T) and s["full-then-partial"] - 1024 * 2 * T == T + 5
    assert s["full-then-partial"] == pc.value_domain_size("coalesced", dtype)
    # below the rounds' threshold the family is the default dispatch, from it on GDF_SCAN_LOOKBACK=0
    assert pc.family_forced("coalesced", dtype, s["tile"]) == {}
    assert pc.family_forced("coalesced", dtype, s["max-chunks"]) == ({} if V == 16 else {"GDF_SCAN_LOOKBACK": "0"})
    # three tiles per chunk: the carry inside a chunk has to advance after its second tile too
    assert geo["three-tiles-per-chunk"] == (1366, 3 * T) and max(s.values()) == s["three-tiles-per-chunk"] == 2 * 2048 * T + 1


@pytest.mark.parametrize("dtype", pc.DTYPES)
def test_elementwise_table_lands_on_its_geometry(dtype):
    s = pc.elementwise_sizes(dtype)
    E = pc.elementwise_tile(dtype)
    for name, n in s.items():
        assert pc.model(dtype, n, forced=pc.FAMILY_SWITCHES["elementwise"]) == _m(pc.ELEMENTWISE, *pc.chunking(n, E)), name
    assert [s[k] for k in ("one", "block-1", "block", "block+1")] == [1, 255, 256, 257]
    assert (s["tile-1"], s["tile"], s["tile+1"]) == (E - 1, E, E + 1)
    # scan_reduce's unrolled loop runs while i + 7 * 256 < end: its first whole trip for thread 0 is at 8 * 256 - 255 elements, for
    # every thread at 8 * 256; these sizes are inside one chunk only where the tile is 2048
    assert {2047, 2048, 2049} <= set(s.values())
    if E == 2048:                                                         # (the same sizes as the tile's edge: listed once)
        assert "unroll" not in s
    else:
        assert (s["unroll-1"], s["unroll"], s["unroll+1"]) == (2047, 2048, 2049)
    assert pc.chunking(s["spine-second-batch"], E) == (257, E)
    assert pc.chunking(s["two-tiles-per-chunk"], E) == (1025, 2 * E)
    assert pc.chunking(pc.value_domain_size("elementwise", dtype), E) == (1025, 2 * E)
    assert pc.chunking(s["three-tiles-per-chunk"], E) == (1366, 3 * E)


def test_single_pass_table():
    s = pc.single_pass_sizes()
    assert list(s.values()) == [1, 4096, 4097, 257 * 4096 + 1, 1025 * 4096 + 7, 10_000_019]
    for fam in ("lookback", "spine"):
        for dtype in pc.DTYPES:
            for n in s.values():
                assert pc.model(dtype, n, forced=pc.FAMILY_SWITCHES[fam]) == _m(pc.FAMILY_ROUTE[fam])
        assert pc.value_domain_size(fam, np.int64) == 1025 * 4096 + 7
    assert -(-s["window+1"] // T) == pc.LOOKBACK_WINDOW + 2 and -(-s["spine-round+1"] // T) == pc.SPINE_ROUND + 2


@pytest.mark.parametrize("G", [3, 256, 512, 513, 768, 1024])
def test_rounds_table_lands_on_its_geometry(G):
    s = pc.rounds_sizes(G)
    geo = {name: pc.rounds_of(n, G) for name, n in s.items()}
    for name, n in s.items():
        assert pc.model(np.int64, n, forced=pc.FAMILY_SWITCHES["rounds"]) == _m(pc.ROUNDS), name
    if G > 2:
        assert geo["tile-1"] == (1, 1, 1) and geo["tile"] == (1, 1, 1) and geo["two-tiles+1"] == (3, 1, 3)
        assert geo["G-1"] == (G - 1, 1, G - 1)
    assert geo["G"] == (G, 1, G)                                          # one full round
    assert geo["G+1elem"] == (G + 1, 2, 1)                                # a last round of one publisher, a partial tile
    assert geo["2G+4095"] == (2 * G + 1, 3, 1)
    assert (513 * T in s.values()) == (G > 512)
    if G > 513:
        assert geo["second-poll-page"] == (513, 1, 513)                   # one publisher on the second poll page
    # round 4 publishes into slot set 4 & 3 == 0 again, round 5 into set 1
    assert geo["slot-set-0-again"] == (4 * G + 1, 5, 1) and (5 - 1) & 3 == 0
    assert geo["slot-set-1-again"] == (5 * G + 2, 6, 2) and (6 - 1) & 3 == 1
    assert max(s.values()) <= 5121 * 4096 + 17
    assert "slot-set-1-again" not in pc.rounds_sizes(G, np.int8) and "slot-set-0-again" in pc.rounds_sizes(G, np.int8)
    assert pc.rounds_of(pc.value_domain_size("rounds", np.int32, G), G) == (2 * G + 1, 3, 1)


def test_alignment_offsets():
    assert [len(pc.alignment_offsets(d)) for d in pc.DTYPES] == [16, 4, 2]
    for d in pc.DTYPES:
        for i in pc.alignment_offsets(d):
            for o in pc.alignment_offsets(d):
                want = pc.COALESCED if (i, o) == (0, 0) else pc.ELEMENTWISE
                assert pc.model(d, pc.elementwise_tile(d) + 1, i, o)["scan.route"] == want
                assert pc.model(d, pc.elementwise_tile(d) + 1, i, o, forced=LB3)["scan.route"] == (pc.ROUNDS if (i, o) == (0, 0) else pc.ELEMENTWISE)
