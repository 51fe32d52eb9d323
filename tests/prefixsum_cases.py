"""gdf_prefixsum_*: the reference, value recipes, a model of device_scan's dispatch and chunk geometry, and the size tables the GPU
tests run (test_gpu_prefixsum.py).  Nothing here needs a GPU; test_prefixsum_cases.py checks all of it on the CPU.

The reference is np.cumsum in the column's own dtype (it wraps), shifted by one for an exclusive scan -- oracle.prefixsum.  Integers
are compared exactly everywhere.

The model is written from the conditions of device_scan / device_scan_coalesced / device_scan_lookback_impl in csrc/scan.hip; the
library leaves the same facts in the note channel (scan.route, scan.bailed, scan.grid, scan.chunks, scan.chunk_elems; DESIGN
section 5d).  The size tables are BUILT from the model's constants, so a change of a tile size moves the tables with it, and the CPU
test holds every entry to the geometry it is named for."""
import functools

import numpy as np

# scan.route
ELEMENTWISE, COALESCED, LOOKBACK, SPINE, ROUNDS = range(5)
ROUTE_NAMES = ("elementwise", "coalesced", "lookback", "spine", "rounds")
NOTE_NAMES = ("scan.route", "scan.bailed", "scan.grid", "scan.chunks", "scan.chunk_elems")

DTYPES = (np.int8, np.int32, np.int64)

# csrc/scan.hip
THREADS = 256                    # SCAN_THREADS == LB_THREADS
LB_TILE = 4096                   # LB_THREADS * LB_ITEMS: the tile of the coalesced and the single-pass kernels, every dtype
MAX_CHUNKS = 2048                # SCAN_MAX_CHUNKS
ROUNDS_MIN = 1 << 22             # SCAN_ROUNDS_MIN: the rounds are the default from here on (4- and 8-byte types, not in place)
SPINE_BATCH = THREADS            # chunk sums scan_spine takes per iteration
REDUCE_UNROLL = 8                # loads per thread of scan_reduce's / scan_reduce_v's unrolled loop
LOOKBACK_WINDOW = THREADS        # predecessors one look-back step examines
SPINE_ROUND = 4 * THREADS        # tile aggregates the spine workgroup takes per round
MAX_GRID = 4 * THREADS           # slots one poll of the rounds covers: G <= 1024
POLL_PAGE = 2 * THREADS          # slots per poll page of the rounds

# the forced-switch sets that select a family (conftest.force_path); "coalesced" names GDF_SCAN_LOOKBACK=0 ("never a single pass"),
# without which 4- and 8-byte columns of 2^22 elements and more take the rounds
FAMILY_SWITCHES = {
    "elementwise": {"GDF_SCAN_BLOCKED": "1"},
    "coalesced": {"GDF_SCAN_LOOKBACK": "0"},
    "lookback": {"GDF_SCAN_LOOKBACK": "1"},
    "spine": {"GDF_SCAN_LOOKBACK": "2"},
    "rounds": {"GDF_SCAN_LOOKBACK": "3"},
}
FAMILIES = tuple(FAMILY_SWITCHES)
FAMILY_ROUTE = dict(zip(FAMILIES, range(5)))
SWITCH_NAMES = ("GDF_SCAN_BLOCKED", "GDF_SCAN_LOOKBACK", "GDF_SCAN_FORCE_BAIL")


def itemsize(dtype):
    return np.dtype(dtype).itemsize


def vec(dtype):
    """elements per 16-byte vector"""
    return 16 // itemsize(dtype)


def elementwise_tile(dtype):
    """SCAN_THREADS * ITEMS, ITEMS = 8 when a vector holds four elements or more, else 4"""
    return THREADS * (8 if vec(dtype) >= 4 else 4)


def family_tile(family, dtype):
    return elementwise_tile(dtype) if family == "elementwise" else LB_TILE


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference

def reference(a, inclusive):
    """oracle.prefixsum's statement: np.cumsum in the column's dtype; exclusive = the same shifted by one, 0 in front"""
    inc = np.cumsum(a, dtype=a.dtype)
    return inc if inclusive else exclusive_of(inc)


def exclusive_of(inc):
    out = np.empty_like(inc)
    out[0:1] = 0
    out[1:] = inc[:-1]
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# value recipes: f(dtype, n, rng) -> array

def _small(dtype, n, rng):
    return rng.integers(-100, 100, size=n).astype(dtype)


def _full(dtype, n, rng):
    ii = np.iinfo(dtype)
    return rng.integers(ii.min, ii.max, size=n, dtype=dtype, endpoint=True)


def _minus_one(dtype, n, rng):
    return np.full(n, -1, dtype=dtype)


def _type_min(dtype, n, rng):
    return np.full(n, np.iinfo(dtype).min, dtype=dtype)


def _ones(dtype, n, rng):
    return np.ones(n, dtype=dtype)


HALF_WORD_VALUES = (2**31 - 1, 2**32 - 1, 2**32, -2**32)


def _half_word(dtype, n, rng):
    assert np.dtype(dtype) == np.int64
    return np.array(HALF_WORD_VALUES, dtype=np.int64)[rng.integers(0, len(HALF_WORD_VALUES), size=n)]


RECIPES = {"small": _small, "full": _full, "minus-one": _minus_one, "type-min": _type_min, "ones": _ones, "half-word": _half_word}


def recipes_for(dtype):
    return tuple(r for r in RECIPES if r != "half-word" or np.dtype(dtype) == np.int64)


@functools.lru_cache(maxsize=4)
def values_and_scan(recipe, dtype, n):
    """(values, inclusive scan) of n elements, read-only and cached: the scan of a PREFIX of the values is the prefix of the scan, so
    one pair at a table's largest size serves every size of the table"""
    dt = np.dtype(dtype)
    rng = np.random.default_rng([sorted(RECIPES).index(recipe), dt.itemsize, 0x5ca9])
    a = RECIPES[recipe](dt.type, n, rng)
    inc = np.cumsum(a, dtype=dt)
    a.setflags(write=False)
    inc.setflags(write=False)
    return a, inc


def wraps(a, inc):
    """how many additions of the running sum overflowed the signed dtype"""
    prev, cur, s = inc[:-1], a[1:], inc[1:]
    return int(np.count_nonzero(((s ^ prev) & (s ^ cur)) < 0))


def low_word_carries(a, inc):
    """int64: how many additions of the running sum carried out of the low 32-bit word"""
    m = np.uint64(0xffffffff)
    prev = inc[:-1].view(np.uint64) & m
    cur = a[1:].view(np.uint64) & m
    return int(np.count_nonzero(prev + cur > m))


# ---------------------------------------------------------------------------------------------------------------------------------
# the model of device_scan

def chunking(n, tile):
    """(chunks, chunk_elems) of a three-launch family: whole tiles per chunk, at most MAX_CHUNKS chunks"""
    tiles = -(-n // tile)
    tiles_per_chunk = -(-tiles // MAX_CHUNKS)
    chunk = tiles_per_chunk * tile
    return -(-n // chunk), chunk


def model(dtype, n, in_off=0, out_off=0, in_place=False, forced=None):
    """The notes device_scan leaves for a column of n elements that starts in_off / out_off ELEMENTS past a 16-byte boundary.
    forced: {switch: value}.  scan.grid depends on the device and is not modelled (test_gpu_prefixsum.py reads G from it)."""
    forced = forced or {}
    assert n > 0 and set(forced) <= set(SWITCH_NAMES)
    assert not in_place or in_off == out_off
    w = itemsize(dtype)
    mode = int(forced.get("GDF_SCAN_LOOKBACK", -1))
    if mode < 0:
        mode = 3 if (n >= ROUNDS_MIN and w >= 4) else 0
    if mode == 3 and in_place:
        mode = 0
    aligned = (in_off * w) % 16 == 0 and (out_off * w) % 16 == 0
    if "GDF_SCAN_BLOCKED" in forced or not aligned:
        chunks, chunk = chunking(n, elementwise_tile(dtype))
        return {"scan.route": ELEMENTWISE, "scan.bailed": 0, "scan.chunks": chunks, "scan.chunk_elems": chunk}
    bail = mode == 3 and "GDF_SCAN_FORCE_BAIL" in forced
    if mode > 0 and not bail:
        return {"scan.route": {1: LOOKBACK, 2: SPINE, 3: ROUNDS}[mode], "scan.bailed": 0, "scan.chunks": 0, "scan.chunk_elems": 0}
    chunks, chunk = chunking(n, LB_TILE)
    return {"scan.route": COALESCED, "scan.bailed": 1 if bail else 0, "scan.chunks": chunks, "scan.chunk_elems": chunk}


# ---------------------------------------------------------------------------------------------------------------------------------
# size tables: {name: n}, named for the geometry each size is there for

def _dedupe(table):
    seen, out = set(), {}
    for name, n in table.items():
        if n > 0 and n not in seen:
            seen.add(n)
            out[name] = n
    return out


def coalesced_sizes(dtype):
    V, T = vec(dtype), LB_TILE
    return _dedupe({
        "one": 1, "vec-1": V - 1, "vec": V, "vec+1": V + 1,
        "tile-1": T - 1, "tile": T, "tile+1": T + 1,
        "subvector-tail": T + V + 1,                                      # second chunk: one whole vector and thread 0's tail
        "spine-one-batch": SPINE_BATCH * T, "spine-second-batch": SPINE_BATCH * T + 1,
        "max-chunks": MAX_CHUNKS * T, "two-tiles-per-chunk": MAX_CHUNKS * T + 1, "full-then-partial": MAX_CHUNKS * T + T + 5,
        # (not in the first plan: with two tiles per chunk a carry that stops advancing after a chunk's FIRST tile changes nothing)
        "three-tiles-per-chunk": 2 * MAX_CHUNKS * T + 1,
    })


def elementwise_sizes(dtype):
    T = elementwise_tile(dtype)
    U = REDUCE_UNROLL * THREADS
    return _dedupe({
        "one": 1, "block-1": THREADS - 1, "block": THREADS, "block+1": THREADS + 1,
        "tile-1": T - 1, "tile": T, "tile+1": T + 1,
        "unroll-1": U - 1, "unroll": U, "unroll+1": U + 1,
        "spine-second-batch": SPINE_BATCH * T + 1, "two-tiles-per-chunk": MAX_CHUNKS * T + 1,
        "three-tiles-per-chunk": 2 * MAX_CHUNKS * T + 1,
    })


def single_pass_sizes(dtype=None):
    T = LB_TILE
    return _dedupe({
        "one": 1, "tile": T, "tile+1": T + 1,
        "window+1": (LOOKBACK_WINDOW + 1) * T + 1,
        "spine-round+1": (SPINE_ROUND + 1) * T + 7,
        "ten-million": 10_000_019,
    })


def rounds_tiles(G):
    """(name, whole tiles, remainder) as a function of the resident grid G"""
    rows = [("tile-1", 1, -1), ("tile", 1, 0), ("two-tiles+1", 2, 1)]
    if G > 1:
        rows.append(("G-1", G - 1, 0))
    rows += [("G", G, 0), ("G+1elem", G, 1), ("2G+4095", 2 * G, LB_TILE - 1)]
    if G > POLL_PAGE:
        rows.append(("second-poll-page", POLL_PAGE + 1, 0))
    rows += [("slot-set-0-again", 4 * G + 1, 0), ("slot-set-1-again", 5 * G + 1, 17)]
    return rows


def rounds_sizes(G, dtype=None):
    """int8 stops at 4G + 1 tiles (its rounds are a forced route only)"""
    assert 1 <= G <= MAX_GRID
    rows = rounds_tiles(G)
    if dtype is not None and itemsize(dtype) == 1:
        rows = rows[:-1]
    return _dedupe({name: tiles * LB_TILE + rem for name, tiles, rem in rows})


def family_sizes(family, dtype, G=None):
    if family == "elementwise":
        return elementwise_sizes(dtype)
    if family == "coalesced":
        return coalesced_sizes(dtype)
    if family in ("lookback", "spine"):
        return single_pass_sizes(dtype)
    return rounds_sizes(G, dtype)


def value_domain_size(family, dtype, G=None):
    """one multi-tile, multi-chunk size per family"""
    if family in ("elementwise", "coalesced"):
        T = family_tile(family, dtype)
        return MAX_CHUNKS * T + T + 5
    if family in ("lookback", "spine"):
        return (SPINE_ROUND + 1) * LB_TILE + 7
    return 2 * G * LB_TILE + LB_TILE - 1


def rounds_of(n, G):
    """(tiles, rounds, publishers of the last round) of a rounds launch"""
    tiles = -(-n // LB_TILE)
    g = min(G, tiles)
    rounds = -(-tiles // g)
    return tiles, rounds, tiles - (rounds - 1) * g


def family_forced(family, dtype, n):
    """the switches a family's case is run with: the coalesced family below the rounds' threshold is the DEFAULT dispatch"""
    if family == "coalesced" and model(dtype, n)["scan.route"] == COALESCED:
        return {}
    return dict(FAMILY_SWITCHES[family])


def alignment_offsets(dtype):
    """every element misalignment against 16 bytes (int8: every byte offset)"""
    return range(vec(dtype))
