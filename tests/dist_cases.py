"""The case tables of the one-process tests of csrc/dist_ops.hip (tests/dist_world.py is the harness): which worlds, which shard
sizes per rank, which dtypes, keys and values.  Pure numpy, shared by the CPU tests (test_dist_world_cpu.py: the model reproduces
the oracle on every entry; the properties the tables promise) and the GPU tests (test_gpu_dist_*.py).

Every float value is a multiple of 1/4 of magnitude at most 32 and a world holds fewer than 2^15.5 rows, so every sum of every
subset, in any order, is a multiple of 1/4 below 2^22.5 / 4: representable in float32 and float64.  SUM and AVG are compared bit for
bit; no test here has a tolerance.
"""
import zlib

import numpy as np

from dist_world import NP_OF, owner_of

# (rows per rank, the rank whose rows all belong to ONE owner, the group layout).  Every size of dist_world.SHARD_SIZES occurs; every
# world has a rank without rows and (W > 1) a one-owner rank with hundreds of rows of several groups and a small rank next to a large
# one: the agreed block exceeds what the small one sends.  Layouts: "mixed" = a pool of keys, one of them on every sender;
# "one_group"; "distinct" = no key twice anywhere.
SHAPES = {
    1: [((0,), None, "mixed"), ((65,), None, "one_group"), ((2049,), None, "distinct")],
    2: [((0, 2049), None, "mixed"), ((8, 255), 1, "mixed"), ((20011, 7), None, "distinct")],
    3: [((1, 20011, 0), None, "mixed"), ((63, 64, 256), 2, "mixed")],
    5: [((9, 0, 2049, 257, 1), 3, "mixed"), ((65, 7, 20011, 0, 64), None, "one_group")],
    8: [((1, 0, 8, 2049, 63, 255, 256, 9), 3, "mixed")],
}
KEY_DTYPES = ("int64", "int32", "date32", "timestamp")
VAL_DTYPES = ("int8", "int16", "int32", "int64", "float32", "float64")
FLOAT_UNIT, FLOAT_MAX_UNITS = 0.25, 128


# (op, key dtype, value dtype) of the single-key group-by: every op x value dtype on int64 keys (partials of every width cross a rank
# boundary, every dg_widen instantiation), and every op on the 4-byte key branch (INT32, DATE32) and an 8-byte date type
VAL_FOR_KEY_CASES = {"sum": "int16", "min": "int8", "max": "float32", "count": "float64", "avg": "int16"}
GROUP_BY_CASES = ([(op, "int64", val) for op in ("sum", "min", "max", "count", "avg") for val in VAL_DTYPES]
                  + [(op, key, VAL_FOR_KEY_CASES[op]) for key in KEY_DTYPES[1:] for op in ("sum", "min", "max", "count", "avg")])


def rng_of(*what):
    return np.random.default_rng(zlib.crc32("|".join(str(w) for w in what).encode()))


def values(rng, name, n):
    dt = np.dtype(NP_OF[name])
    if dt.kind == "f":
        return (rng.integers(-FLOAT_MAX_UNITS, FLOAT_MAX_UNITS + 1, size=n) * FLOAT_UNIT).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, size=n, endpoint=True, dtype=np.int64).astype(dt)


def key_pool(name):
    """keys at both ends of the dtype, negative, dense; pool[0] is the group every sender has"""
    dt = np.dtype(NP_OF[name])
    info = np.iinfo(dt)
    far = [-(2 ** 40) - 7, 2 ** 33 + 5, -(2 ** 62)] if dt.itemsize == 8 else [-(2 ** 30) - 7, 2 ** 30 + 5, -(2 ** 31) + 9]
    return np.array([info.min, info.max, info.min + 1, info.max - 1, -1, -2, -77] + list(range(0, 24)) + far, dtype=dt)


def group_by_shards(world, shape, key_name, val_name):
    """[(keys, values)] per rank for shape number `shape` of the world"""
    sizes, one, layout = SHAPES[world][shape]
    rng = rng_of("gb", world, shape, key_name, val_name)
    pool = key_pool(key_name)
    kd = pool.dtype
    owners = owner_of([pool], world)
    shards, base = [], 0
    for r, n in enumerate(sizes):
        if layout == "one_group":
            keys = np.full(n, pool[4], dtype=kd)
        elif layout == "distinct":
            keys = (np.iinfo(kd).min + base + rng.permutation(n)).astype(kd)          # dense from the dtype's minimum, no key twice anywhere
        else:
            mine = pool[owners == owners[0]] if r == one else pool
            keys = mine[rng.integers(0, len(mine), size=n)]
            keys[:1] = pool[0]                                                        # the group every sender has
        base += n
        shards.append((np.ascontiguousarray(keys), values(rng, val_name, n)))
    return shards


def wrap_twice_shards(world):
    """int8: three rows of 127 in one group on every rank.  The partial sum 381 wraps to 125 on its sender, the owner's sum of W >= 2
    such partials wraps again; int64: the AVG's sum passes 2^53 (and wraps) on the way"""
    return ([(np.full(3, -9, dtype=np.int64), np.full(3, 127, dtype=np.int8)) for _ in range(world)],
            [(np.full(3, -9, dtype=np.int64), np.full(3, 2 ** 62 + 12345, dtype=np.int64)) for _ in range(world)])


SPECIAL_WORLDS = (2, 3, 5)


def special_float_shards(world, dtype):
    """MIN / MAX of what tests/groupby_values.py pins, split ACROSS senders: key 3 is NaN only on every rank, key 11 NaN only on
    the last rank alone, key 1 holds +0.0 on even ranks and -0.0 on odd ones, key 2 only -0.0, key 7 has +inf on rank 0 and finite
    values elsewhere, key -5 has -inf on the last rank, key 9 plain numbers.  No group mixes NaN with numbers (unspecified)."""
    dt = np.dtype(dtype)
    shards = []
    for r in range(world):
        z = 0.0 if r % 2 == 0 else -0.0
        rows = [(3, np.nan), (3, np.nan), (1, z), (1, z), (2, -0.0), (7, np.inf if r == 0 else 1.5 * r), (7, -2.0),
                (-5, -np.inf if r == world - 1 else -0.25 * r), (-5, 4.0), (9, r + 0.5), (9, -r - 0.5)]
        if r == world - 1:
            rows += [(11, np.nan)]
        shards.append((np.array([k for k, _ in rows], dtype=np.int64), np.array([v for _, v in rows], dtype=dt)))
    return shards


# ---- gdf_amd_dist_group_by_multi ----
# (op, key dtypes, which key columns are masked, values masked, value dtype)
MULTI_CASES = [
    ("sum", ("int64",), (False,), True, "int32"),
    ("min", ("int32", "float64"), (True, False), True, "float64"),
    ("max", ("int32", "float64"), (False, True), True, "int16"),
    ("count", ("int32", "float64"), (True, True), True, "int8"),
    ("count", ("int64",), (False,), False, "float32"),
    ("avg", ("int16", "float64", "int64"), (True, False, True), True, "int64"),
    ("avg", ("int32", "float64"), (False, False), True, "float32"),
    ("sum", ("int16", "float64", "int64"), (False, True, False), False, "float64"),
    ("avg", ("float64",), (True,), True, "int8"),
    ("max", ("int64",), (True,), False, "float32"),
    ("sum", ("int32", "float64"), (True, True), True, "int8"),
    ("min", ("float64",), (False,), True, "int64"),
]
MULTI_KEY_RANGE = (6, 5, 3)        # values per key column: at most 90 groups


def multi_shards(world, shape, case):
    """[(keys, key_valids, values, value_valid)] per rank.  The groups with key column 0 == 1 have no valid value on any rank, those
    with key column 0 == 2 valid values on the first rank with rows only."""
    op, kds, kmask, vmask, vd = case
    sizes, one, _ = SHAPES[world][shape]
    rng = rng_of("multi", world, shape, *case)
    first = next((r for r, n in enumerate(sizes) if n), 0)
    shards = []
    for r, n in enumerate(sizes):
        keys = []
        for c, name in enumerate(kds):
            k = rng.integers(0, MULTI_KEY_RANGE[c], size=n) - (1 if c else 0)
            if r == one:
                k[:] = 3 if c == 0 else 0                                           # one group: one owner
            keys.append(k.astype(NP_OF[name]))
        kvs = [rng.random(n) < 0.85 if m else None for m in kmask]
        vv = None
        if vmask:
            vv = rng.random(n) < 0.7
            vv[keys[0] == 1] = False
            vv[keys[0] == 2] = r == first
        shards.append((keys, kvs, values(rng, vd, n), vv))
    return shards


OWNER_ROWS = (1, 7, 8, 9, 63, 64, 65)                # the mask bytes and the padded tail of dg_mask_from_counts
OWNER_ROWS_WORLDS = (2, 3, 5, 8)


def owner_rows_shards(world, real, rows):
    """one int64 key column, masked int32 values: exactly `rows` partial rows reach rank `real` -- every group it owns lives on one sender"""
    rng = rng_of("owner_rows", world, real, rows)
    cand = np.arange(-600, 600, dtype=np.int64)
    own = owner_of([cand], world)
    mine, other = cand[own == real][:rows], cand[own != real][:40]
    assert len(mine) == rows
    shards = []
    for r in range(world):
        keys = np.concatenate([mine[r::world], other[r::world]])
        keys = np.repeat(keys, 3)
        n = len(keys)
        vv = rng.random(n) < 0.5
        shards.append(([keys], [None], values(rng, "int32", n), vv))
    return shards


# ---- the joins ----
JOIN_KEYS = ("int32", "int64")
JOIN_HOWS = ("inner", "left", "full")


def join_pool(name, size, rng):
    dt = np.dtype(NP_OF[name])
    info = np.iinfo(dt)
    base = rng.choice(np.arange(-size, size), size=size, replace=False).astype(np.int64)
    if dt.itemsize == 8:
        base[::3] = base[::3] * (2 ** 33) + 12345                                  # beyond 2^32, both signs
    pool = base.astype(dt)
    pool[:2] = [info.min, info.max]
    return pool


def join_shards(world, shape, key_name, empty=None, real=None):
    """[(probe keys, build keys)] per rank: many-to-many duplicates.  empty = "build" / "probe" / "both": no row of that relation is
    owned by rank `real`."""
    sizes, one, _ = SHAPES[world][shape]
    rng = rng_of("join", world, shape, key_name, empty, real)
    total = sum(sizes)
    pool = join_pool(key_name, max(total // 4, 8), rng)
    own = owner_of([pool], world)
    ppool = pool[own != real] if empty in ("probe", "both") else pool
    bpool = pool[own != real] if empty in ("build", "both") else pool
    shards = []
    draw = lambda p, n: p[rng.integers(0, len(p), size=n)] if len(p) else p[:0]
    for r, n in enumerate(sizes):
        nb = sizes[::-1][r] // 2 if world > 1 else n // 2
        if r == one and empty is None:                      # the rank whose rows, of both relations, all belong to one owner
            mine = pool[own == own[2]]
            shards.append((draw(mine, n), draw(mine, max(nb, 40))))
        else:
            shards.append((draw(ppool, n), draw(bpool, nb)))
    return shards


EMPTY_SIDE_SHAPES = ((3, 1), (5, 0), (8, 0))          # (world, shape) of the tests in which a rank receives nothing of a relation
BIG_SENDER_WORLDS = (2, 5)


def big_sender_shards(world=2):
    """a sender with more than 2^16 rows of either relation: local row numbers above 65535 inside sender << 40 | row.  The big
    sender is the first rank and -- in a world of more than two -- the last as well, so that the real rank is one and receives from one."""
    rng = rng_of("big sender", world)
    pool = join_pool("int64", 40000, rng)
    sizes = [(70001, 66000), (300, 200), (0, 9), (65, 0), (66001, 67000)]
    sizes = sizes[:2] if world == 2 else sizes
    assert len(sizes) == world
    return [(pool[rng.integers(0, len(pool), size=p)], pool[rng.integers(0, len(pool), size=b)]) for p, b in sizes]


# ---- the gather ----
GATHER_DTYPES = ("int8", "int16", "int32", "date32", "float32", "int64", "timestamp", "float64")
ID_SIZES = (1, 7, 8, 9, 63, 64, 65, 2049)
# (column dtypes, which of them carry a mask) per gather call: one column of every width with and without a mask, 16 columns at once
GATHER_CASES = ([((name,), (m,)) for name in GATHER_DTYPES for m in (False, True)]
                + [(GATHER_DTYPES * 2, (False,) * 8 + (True,) * 8)])
# (ids per rank, shard rows per rank, the rank nobody asks anything of)
GATHER_SHAPES = {
    1: [((2049,), (257,), None), ((7,), (9,), None)],
    2: [((8, 0), (65, 7), None), ((63, 2049), (1, 2049), None)],
    3: [((9, 64, 0), (64, 255, 8), 1), ((65, 1, 2049), (9, 63, 20011), 0)],
    5: [((1, 7, 0, 2049, 65), (256, 0, 65, 9, 257), 1)],
    8: [((64, 8, 0, 9, 63, 1, 7, 2049), (7, 64, 0, 2049, 1, 255, 9, 63), 2)],
}


def gather_shards(world, shape, col_names, masked):
    """[(ids, columns, valids)] per rank.  Row 1 % rows of every masked column is null; every rank that asks anything asks for row 0,
    the last row and that row of every rank that may be asked, then random rows with repeats and -1, in random order."""
    nids, rows, lonely = GATHER_SHAPES[world][shape]
    rng = rng_of("gather", world, shape, *col_names, *masked)
    askable = [r for r in range(world) if rows[r] and r != lonely]
    shards = []
    for r in range(world):
        cols = [values(rng, name, rows[r]) for name in col_names]
        valids = []
        for m in masked:
            v = None
            if m:
                v = rng.random(rows[r]) < 0.6
                v[1 % max(rows[r], 1):1 % max(rows[r], 1) + 1] = False
            valids.append(v)
        must = np.array([(o << 40) | x for o in askable for x in (0, rows[o] - 1, 1 % rows[o])] + [-1], dtype=np.int64)
        if askable:
            own = rng.choice(askable, size=nids[r])
            rnd = (own.astype(np.int64) << 40) | (rng.random(nids[r]) * np.array(rows)[own]).astype(np.int64)
            rnd[rng.random(nids[r]) < 0.1] = -1
        else:
            rnd = np.full(nids[r], -1, dtype=np.int64)
        if nids[r] >= len(must):
            ids = np.concatenate([must, rnd[len(must):]])               # the rows that must be asked, then random ones
        else:
            ids = rng.permutation(must)[:nids[r]]                       # fewer ids than that: some of them
        ids = rng.permutation(ids)
        shards.append((np.ascontiguousarray(ids), cols, valids))
    return shards
