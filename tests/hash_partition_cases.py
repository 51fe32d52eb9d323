"""gdf_hash / gdf_hash_partition: a numpy reference, value and skew recipes, a model of the dispatcher's route, a verifier and the
tables of cases the GPU tests run (test_gpu_hash_partition_routes.py, _masks.py, test_gpu_hash_values.py).  Nothing here needs a GPU;
test_hash_partition_cases.py checks all of it on the CPU.

The reference is written from the statements in csrc/hash.cuh and SURVEY (Murmur3_x86_32 with seed 0 over the element's raw bytes,
columns folded with the Boost-style combine and the first column not combined, IdentityHash = static_cast<uint32_t>(value), the
partition rule `& (P - 1)` for powers of two and `% P` otherwise), in vectorised uint32 / uint64 numpy -- independently of
oracle/gdf_oracle.c, against which the CPU test then holds it.

The route model is written from the conditions of gdf_hash_partition / hash_partition_two_level in csrc/hashing.hip; the library
leaves the same facts in the note channel (hp.route, hp.fastw, hp.murmur, hp.nchunks, hp.map_launches and, on two levels,
hp.kshift, hp.pieces)."""
import functools

import numpy as np

MURMUR3, IDENTITY = 0, 1

# hp.route
DIRECT_GENERIC, DIRECT_FAST, TILE, PAIRS, COLS8, TWO_LEVEL = range(6)
ROUTE_NAMES = ("direct-generic", "direct-fast", "tile", "pairs", "cols8", "two-level")
NOTE_NAMES = ("hp.route", "hp.fastw", "hp.murmur", "hp.nchunks", "hp.map_launches", "hp.kshift", "hp.pieces")

U32 = np.uint32
_UBITS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def mask_bytes(n):
    return (n + 7) // 8


def raw_bits(a):
    """the element's bytes as an unsigned integer of the same width: NaN payloads and -0.0 are data"""
    a = np.ascontiguousarray(a)
    return a.view(_UBITS[a.dtype.itemsize])


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference

def _rotl(x, r):
    return (x << U32(r)) | (x >> U32(32 - r))


def _fmix(h):
    h = h ^ (h >> U32(16))
    h = h * U32(0x85ebca6b)
    h = h ^ (h >> U32(13))
    h = h * U32(0xc2b2ae35)
    return h ^ (h >> U32(16))


def _scramble(k):
    return _rotl(k * U32(0xcc9e2d51), 15) * U32(0x1b873593)


def _block(h, k):
    h = _rotl(h ^ _scramble(k), 13)
    return h * U32(5) + U32(0xe6546b64)


def murmur3_32(a):
    """Murmur3_x86_32, seed 0, over the itemsize raw bytes of every element -> uint32 array"""
    bits = raw_bits(np.atleast_1d(a))
    w = bits.dtype.itemsize
    h = np.zeros(len(bits), dtype=U32)
    if w == 8:
        h = _block(h, (bits & np.uint64(0xffffffff)).astype(U32))
        h = _block(h, (bits >> np.uint64(32)).astype(U32))
    elif w == 4:
        h = _block(h, bits.astype(U32))
    else:                                   # 1 or 2 tail bytes, no body block
        h = h ^ _scramble(bits.astype(U32))
    return _fmix(h ^ U32(w))


def hash_combine(l, r):
    l, r = np.asarray(l, dtype=U32), np.asarray(r, dtype=U32)
    return l ^ (r + U32(0x9e3779b9) + (l << U32(6)) + (l >> U32(2)))


def identity_hash(a):
    """static_cast<uint32_t>(value): integers wrap; floats truncate towards zero and saturate, NaN and negatives give 0"""
    a = np.atleast_1d(np.ascontiguousarray(a))
    if a.dtype.kind == "f":
        with np.errstate(invalid="ignore"):                        # (a signalling NaN is data here)
            x = a.astype(np.float64)                               # exact for float32
        x = np.where(np.isnan(x), 0.0, x)
        x = np.minimum(np.maximum(x, 0.0), 4294967295.0)           # (2^32 - 1 is exact in float64; truncation comes next)
        return np.trunc(x).astype(np.uint64).astype(U32)
    return (a.astype(np.int64).view(np.uint64) & np.uint64(0xffffffff)).astype(U32)


def hash_rows(cols, hash_func=MURMUR3):
    one = murmur3_32 if hash_func == MURMUR3 else identity_hash
    h = one(cols[0])
    for c in cols[1:]:
        h = hash_combine(h, one(c))
    return h


def partition_ids(cols, P, hash_func=MURMUR3):
    h = hash_rows(cols, hash_func)
    return (h & U32(P - 1)) if P & (P - 1) == 0 else (h % U32(P))


def reference_offsets(pid, P):
    counts = np.bincount(pid, minlength=P)
    return np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# value recipes (keys and payloads) and skew recipes

def _from_bits(dtype, bits):
    dtype = np.dtype(dtype)
    return np.array(bits, dtype=np.uint64).astype(_UBITS[dtype.itemsize]).view(dtype)


def specials(dtype, identity=False):
    """the values of a dtype at which a hash, a conversion or a narrowing store goes wrong first"""
    dtype = np.dtype(dtype)
    w = dtype.itemsize
    full = (1 << (8 * w)) - 1
    if dtype.kind == "i":
        bits = [0, full, 1, 1 << (8 * w - 1), (1 << (8 * w - 1)) - 1,                   # 0, -1, 1, min, max
                0x5555555555555555 & full, 0xaaaaaaaaaaaaaaaa & full, 0x0f0f0f0f0f0f0f0f & full, 0x8000000000000001 & full | (1 << (8 * w - 1)),
                0xfe & full, (full ^ 0xff) & full]
        if w == 8:                                                                     # varied high words
            bits += [0x0000000100000000, 0x00000001ffffffff, 0xffffffff00000001, 0x7fffffff00000000, 0x123456789abcdef0,
                     0xfedcba9876543210, 0x00000000ffffffff, 0xffffffff00000000, 0x0000000080000000, 0xdeadbeef00c0ffee]
        return _from_bits(dtype, bits)
    if w == 4:
        bits = [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0x7fc12345, 0xffc00001, 0x7f800001, 0x7fa5a5a5, 0xff812345,
                0x00000001, 0x007fffff, 0x80000001, 0x807fffff, 0x7f7fffff, 0xff7fffff, 0x00800000, 0x80800000,
                0x3f800000, 0xbf800000, 0x3f000000, 0x3fc00000, 0x34000000]
        out = _from_bits(dtype, bits)
        ident = np.array([4294967296.0, 4294967040.0, 2147483648.0, 2147483520.0, 8589934592.0, 1e10, 3e38, 0.99999994, 1.9999999,
                          123456.79, 16777216.0, 16777217.0, -1.5, -0.25, -1e10, -4294967296.0, 65535.5, 255.99], dtype=np.float32)
    else:
        bits = [0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000, 0x7ff8123456789abc,
                0xfff8000000000001, 0x7ff0000000000001, 0x7ff5a5a5a5a5a5a5, 0xfff0123400005678,
                0x0000000000000001, 0x000fffffffffffff, 0x8000000000000001, 0x800fffffffffffff, 0x7fefffffffffffff, 0xffefffffffffffff,
                0x0010000000000000, 0x8010000000000000, 0x3ff0000000000000, 0xbff0000000000000, 0x3fe0000000000000, 0x3ff8000000000000,
                0x3cb0000000000000, 0x0000000100000000, 0x3ff00000ffffffff]
        out = _from_bits(dtype, bits)
        ident = np.array([4294967296.0, 4294967295.0, 4294967295.5, 4294967294.999, 2147483648.0, 2147483647.5, 8589934592.0, 1e10, 1e300,
                          0.9999999999, 1.9999999999, 123456.789, 2.0 ** 53, -1.5, -0.25, -1e10, -4294967296.0, -1e300, 65535.5,
                          4294967296.5], dtype=np.float64)
    return np.concatenate([out, ident]) if identity else out


def fill(dtype, n, seed, identity=False):
    """n values: the specials first (as many as fit), then random bit patterns over the whole width -- for the identity hash of
    floats half of the rest are finite values on both sides of 0 and of 2^32 -- shuffled"""
    dtype = np.dtype(dtype)
    rs = np.random.RandomState(seed)
    w = dtype.itemsize
    bits = rs.randint(0, 1 << 32, size=n, dtype=np.uint64)
    if w == 8:
        bits = bits | (rs.randint(0, 1 << 32, size=n, dtype=np.uint64) << np.uint64(32))
    out = bits.astype(_UBITS[w]).view(dtype).copy()
    if identity and dtype.kind == "f":
        m = rs.rand(n) < 0.5
        out[m] = (rs.rand(int(m.sum())) * 2.0 ** 33 - 2.0 ** 30).astype(dtype)
    sp = specials(dtype, identity)[:n]
    raw_bits(out)[:len(sp)] = raw_bits(sp)
    perm = rs.permutation(n)
    return raw_bits(out)[perm].view(dtype)


SKEWS = ("uniform", "one", "third", "sparse")


def skewed(dtype, n, skew, seed, identity=False):
    """key columns: uniform (fill), ONE key on every row (one partition gets everything and a rank reaches the tile size), one key
    on a third of the rows, or five distinct keys (most partitions stay empty)"""
    dtype = np.dtype(dtype)
    sp = specials(dtype, identity)
    rs = np.random.RandomState(seed + 7919)
    if skew == "uniform":
        return fill(dtype, n, seed, identity)
    if skew == "one":
        return raw_bits(sp)[np.full(n, 5 % len(sp))].view(dtype)
    if skew == "third":
        out = fill(dtype, n, seed, identity)
        raw_bits(out)[rs.rand(n) < 1.0 / 3] = raw_bits(sp)[6 % len(sp)]
        return out
    assert skew == "sparse"
    return raw_bits(sp)[rs.randint(0, min(5, len(sp)), size=n)].view(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# the route model (csrc/hashing.hip: gdf_hash_partition, hash_partition_two_level)

HP_MAX_CHUNKS, HP_MAX_PAYLOAD_COLS, HPT_BIG_PARTS, HP_MAX_LDS_PARTS = 1024, 32, 1024, 16384
PAIRS_MAX_PARTS, COLS8_MAX_PARTS, COLS8_MAX_COLS = 64, 256, 4
PAIRS_TILE, COLS8_TILE, TILE_FAST, TILE_GENERIC = 8192, 16384, 12288, 6144


def chunking(n, forced=None):
    maxc = min(max(int((forced or {}).get("GDF_HP_MAX_CHUNKS", HP_MAX_CHUNKS)), 1), HP_MAX_CHUNKS)
    chunk = -(-n // maxc)
    chunk = -(-chunk // 2048) * 2048
    return chunk, -(-n // chunk)


def route_model(dtypes, in_masked, out_masked, hashed, hash_func, P, n, forced=None):
    """the notes gdf_hash_partition must leave for a valid request of n > 0 rows: dtypes per column, the sets of columns that carry
    a mask on the input and on the output side, the hashed columns in order, the hash function, P, n and the forced selectors"""
    forced = forced or {}
    widths = [np.dtype(d).itemsize for d in dtypes]
    ncols = len(widths)
    murmur = hash_func == MURMUR3
    kw = widths[hashed[0]]
    fastw = kw if murmur and len(hashed) == 1 and kw in (4, 8) else 0
    chunk, nchunks = chunking(n, forced)
    notes = {"hp.fastw": fastw, "hp.murmur": int(murmur), "hp.nchunks": nchunks, "hp.map_launches": 0}
    if P > HPT_BIG_PARTS and ncols <= HP_MAX_PAYLOAD_COLS and n >= 1 << 18 and "GDF_HP_ONE_LEVEL" not in forced:
        kshift = 0
        while ((P + (1 << kshift) - 1) >> kshift) > HPT_BIG_PARTS:
            kshift += 1
        while kshift < 8 and (1 << (2 * kshift)) < P:
            kshift += 1
        S = (P + (1 << kshift) - 1) >> kshift
        piece = int(forced.get("GDF_HP_PIECE", 49152))
        group = int(max(1.0, min(float(nchunks), piece / max(chunk / S, 1.0))))
        notes.update({"hp.route": TWO_LEVEL, "hp.kshift": kshift, "hp.pieces": -(-nchunks // group)})
        return notes
    moved = [i in in_masked and i in out_masked for i in range(ncols)]
    plain8 = all(w == 8 for w in widths) and not any(moved)
    big = n >= 1 << 16 and fastw == 8 and P > 16 and plain8
    pairs = big and ncols <= 2 and P <= PAIRS_MAX_PARTS and "GDF_HP_NO_PAIRS" not in forced
    cols8 = big and not pairs and ncols <= COLS8_MAX_COLS and P <= COLS8_MAX_PARTS and "GDF_HP_NO_COLS8" not in forced
    if pairs or cols8:
        notes["hp.route"] = PAIRS if pairs else COLS8
        return notes
    notes["hp.route"] = TILE if 16 < P <= HPT_BIG_PARTS else (DIRECT_FAST if fastw else DIRECT_GENERIC)
    notes["hp.map_launches"] = -(-ncols // HP_MAX_PAYLOAD_COLS) - 1
    return notes


def notes_of(route, fastw, murmur, nchunks, map_launches=0, kshift=None, pieces=None):
    d = {"hp.route": route, "hp.fastw": fastw, "hp.murmur": murmur, "hp.nchunks": nchunks, "hp.map_launches": map_launches}
    if kshift is not None:
        d.update({"hp.kshift": kshift, "hp.pieces": pieces})
    return d


# ---------------------------------------------------------------------------------------------------------------------------------
# the verifier

def check_partition(inputs, input_masks, got_columns, got_masks, got_offsets, hashed, P, hash_func=MURMUR3, rowid=None):
    """Exact: the offsets are the reference's; every output row sits in the range of the partition the reference assigns to its
    key; the rows are preserved as a multiset with every column compared as raw bits, and validity bits where a mask travels
    (input_masks[c] and got_masks[c] both given: bool arrays).  rowid: a column whose input holds distinct values -- the
    permutation is recovered from it in O(n); without one the rows of both sides are sorted."""
    n = len(inputs[0])
    assert all(len(c) == n for c in inputs) and all(len(c) == n for c in got_columns), "column lengths"
    assert all(g.dtype == c.dtype for g, c in zip(got_columns, inputs)), "column dtypes"
    pid = partition_ids([inputs[c] for c in hashed], P, hash_func)
    exp_off = reference_offsets(pid, P)
    got_offsets = np.asarray(got_offsets, dtype=np.int64)
    assert got_offsets.shape == (P,) and np.array_equal(got_offsets, exp_off), "partition offsets differ from the reference's"
    bounds = np.concatenate([exp_off, [n]])
    where = np.repeat(np.arange(P, dtype=np.int64), np.diff(bounds))            # the partition every output position belongs to
    got_pid = partition_ids([got_columns[c] for c in hashed], P, hash_func)
    assert np.array_equal(got_pid, where), "a row sits outside its partition's range"
    travelling = [c for c in range(len(inputs)) if input_masks[c] is not None and got_masks[c] is not None]
    if rowid is not None:
        src = raw_bits(inputs[rowid]).astype(np.int64)
        if not np.array_equal(src, np.arange(n)):                             # any distinct values: look the row up
            order = np.argsort(src, kind="stable")
            assert np.all(np.diff(src[order]) != 0), "rowid column is not distinct"
            pos = np.searchsorted(src[order], raw_bits(got_columns[rowid]).astype(np.int64))
            rid = order[np.minimum(pos, n - 1)]
        else:
            rid = raw_bits(got_columns[rowid]).astype(np.int64)
        assert rid.min(initial=0) >= 0 and rid.max(initial=0) < n, "a row id that the input does not hold"
        assert np.all(np.bincount(rid, minlength=n) == 1), "a row was lost or duplicated"
        for c in range(len(inputs)):
            assert np.array_equal(raw_bits(inputs[c])[rid], raw_bits(got_columns[c])), f"column {c}: bits changed on the way"
        for c in travelling:
            assert np.array_equal(np.asarray(input_masks[c], bool)[rid], np.asarray(got_masks[c], bool)), f"column {c}: validity bits"
        return
    exp_keys = [pid.astype(np.int64)] + [raw_bits(c) for c in inputs] + [np.asarray(input_masks[c], bool) for c in travelling]
    got_keys = [where] + [raw_bits(c) for c in got_columns] + [np.asarray(got_masks[c], bool) for c in travelling]
    eo, go = np.lexsort(exp_keys[::-1]), np.lexsort(got_keys[::-1])
    for k, (e, g) in enumerate(zip(exp_keys, got_keys)):
        assert np.array_equal(e[eo], g[go]), f"rows differ as a multiset (sort key {k})"


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases

class Case:
    """One gdf_hash_partition request.  cols: one spec per column -- "key:<dtype>" (filled by the skew recipe, hashed unless
    `hashed` says otherwise), "val:<dtype>" (value recipe), "rid" (int64 row number) or "rid32".  hashed: column indices, default
    every key column in order.  in_masks / out_masks: columns with a mask on that side.  base_off: every column (both sides)
    starts this many elements into its allocation.  expect: the notes the library must leave, recorded by hand."""

    def __init__(self, cid, cols, P, n, expect, hash_func=MURMUR3, hashed=None, skew="uniform", in_masks=(), out_masks=(), forced=None,
                 base_off=0, seed=1):
        self.id, self.cols, self.P, self.n, self.expect, self.hash_func = cid, tuple(cols), P, n, expect, hash_func
        self.hashed = list(hashed) if hashed is not None else [i for i, s in enumerate(cols) if s.startswith("key:")]
        self.skew, self.in_masks, self.out_masks = skew, frozenset(in_masks), frozenset(out_masks)
        self.forced, self.base_off, self.seed = dict(forced or {}), base_off, seed

    def __repr__(self):
        return self.id

    @property
    def dtypes(self):
        return [np.dtype({"rid": "int64", "rid32": "int32"}.get(s, s.split(":")[-1])) for s in self.cols]

    @property
    def rowid(self):
        for i, s in enumerate(self.cols):
            if s.startswith("rid"):
                return i
        return None

    def model(self, forced=None):
        return route_model(self.dtypes, self.in_masks, self.out_masks, self.hashed, self.hash_func, self.P, self.n,
                           self.forced if forced is None else forced)

    def with_(self, cid_suffix, **kw):
        d = dict(cols=self.cols, P=self.P, n=self.n, expect=self.expect, hash_func=self.hash_func, hashed=self.hashed, skew=self.skew,
                 in_masks=self.in_masks, out_masks=self.out_masks, forced=self.forced, base_off=self.base_off, seed=self.seed)
        d.update(kw)
        return Case(self.id + cid_suffix, **d)


@functools.lru_cache(maxsize=8)
def _table(cols, n, skew, identity, seed, mask_cols):
    out, masks = [], []
    for i, s in enumerate(cols):
        if s.startswith("rid"):
            a = np.arange(n, dtype=np.int64 if s == "rid" else np.int32)
        elif s.startswith("key:"):
            a = skewed(s[4:], n, skew, seed + 31 * i, identity)
        else:
            a = fill(s[4:], n, seed + 31 * i, identity)
        a.setflags(write=False)
        out.append(a)
        m = None
        if i in mask_cols:
            m = np.random.RandomState(seed + 1000 + i).rand(n) > 0.3
            m.setflags(write=False)
        masks.append(m)
    return out, masks


def build_table(case):
    """(columns, input masks) of a case: read-only arrays, shared between the tests that ask for the same table"""
    return _table(case.cols, case.n, case.skew, case.hash_func == IDENTITY, case.seed, case.in_masks)


N3, N4 = 368641, 491521            # with GDF_HP_MAX_CHUNKS = 16: 15 chunks of 24576 / 32768 rows and a last chunk of ONE row
SEL = {"GDF_HP_MAX_CHUNKS": "16"}
NB = 100003                        # 49 chunks of 2048 rows, an odd count, not a multiple of 8
I64, F64, I32, F32, I16, I8 = "int64", "float64", "int32", "float32", "int16", "int8"


def _multi_tile_cases():
    """D1: several tiles per chunk at one level (the carry between tiles, the hist reset, the prefetch, a full tile then a partial
    one).  Every case runs under the selector (16 chunks) and again without it (181 / 241 chunks): same offsets."""
    out = []
    for n, free in ((N3, 181), (N4, 241)):
        for skew in ("uniform", "one"):
            tag = f"n{n}-{skew}"
            for P in (17, 64):
                e = notes_of(PAIRS, 8, 1, 16)
                out += [Case(f"pairs-kv-P{P}-{tag}", ["key:int64", "rid"], P, n, e, skew=skew, forced=SEL),
                        Case(f"pairs-vk-P{P}-{tag}", ["rid", "key:float64"], P, n, e, skew=skew, forced=SEL),
                        Case(f"pairs-k-P{P}-{tag}", ["key:int64"], P, n, e, skew=skew, forced=SEL)]
            for P in (65, 256):
                e = notes_of(COLS8, 8, 1, 16)
                out += [Case(f"cols8-1-P{P}-{tag}", ["key:int64"], P, n, e, skew=skew, forced=SEL),
                        Case(f"cols8-3first-P{P}-{tag}", ["key:int64", "rid", "val:float64"], P, n, e, skew=skew, forced=SEL),
                        Case(f"cols8-3mid-P{P}-{tag}", ["val:int64", "key:float64", "rid"], P, n, e, skew=skew, forced=SEL),
                        Case(f"cols8-4last-P{P}-{tag}", ["rid", "val:float64", "val:int64", "key:int64"], P, n, e, skew=skew, forced=SEL)]
            out.append(Case(f"tile-k4-P17-{tag}", ["key:int32", "rid"], 17, n, notes_of(TILE, 4, 1, 16), skew=skew, forced=SEL))
            for P in (257, 1024):
                out += [Case(f"tile-k8-P{P}-{tag}", ["key:int64", "rid", "val:int16"], P, n, notes_of(TILE, 8, 1, 16), skew=skew, forced=SEL),
                        Case(f"tile-generic-P{P}-{tag}", ["key:int64", "rid", "key:int16"], P, n, notes_of(TILE, 0, 1, 16), skew=skew,
                             forced=SEL),
                        Case(f"tile-identity-P{P}-{tag}", ["key:int64", "rid"], P, n, notes_of(TILE, 0, 0, 16), hash_func=IDENTITY,
                             skew=skew, forced=SEL)]
    for c in out:
        c.free_nchunks = 181 if c.n == N3 else 241
    # level A of the two-level route with several tiles per chunk: kshift 6 (K = 64, S = 17), 16 chunks in one piece per super-partition
    two = Case(f"two-level-P1025-n{N3}", ["key:int64", "rid", "val:int32"], 1025, N3, notes_of(TWO_LEVEL, 8, 1, 16, 0, 6, 1), forced=SEL)
    two.free_nchunks = 181
    return out + [two]


WIDTH_COLS = ["key:int64", "val:int8", "val:int16", "val:float32", "val:float64", "rid"]


def _width_cases():
    """D2: 1-, 2-, 4- and 8-byte payloads on every route that takes them; pairs and cols8 must decline this table"""
    k16 = ["key:int16"] + WIDTH_COLS[1:]
    return [Case("widths-direct-fast-P8", WIDTH_COLS, 8, NB, notes_of(DIRECT_FAST, 8, 1, 49)),
            Case("widths-direct-generic-P8", k16, 8, NB, notes_of(DIRECT_GENERIC, 0, 1, 49)),
            Case("widths-tile-P300", WIDTH_COLS, 300, NB, notes_of(TILE, 8, 1, 49)),
            Case("widths-two-level-P3000", WIDTH_COLS, 3000, 1 << 18, notes_of(TWO_LEVEL, 8, 1, 128, 0, 6, 1)),
            Case("widths-not-pairs-P32", WIDTH_COLS, 32, 1 << 16, notes_of(TILE, 8, 1, 32)),
            Case("widths-not-cols8-P128", WIDTH_COLS, 128, 1 << 16, notes_of(TILE, 8, 1, 32))]


def wide_cols(ncols, key, key_at=0):
    cyc = [I8, F64, I16, I32, F32, I64]
    cols = ["val:" + cyc[i % 6] for i in range(ncols)]
    cols[key_at] = "key:" + key
    cols[1 if key_at != 1 else 2] = "rid"
    return cols


NW = 20011


def _wide_cases():
    """D3: more than 32 columns: dst_map recorded by the first launch, then part_apply_map_kernel once per further 32 columns"""
    out = []
    for ncols, maps in ((33, 1), (65, 2)):
        masks = (0, 5, 31, 32, ncols - 1)
        for name, key, P, route, fastw in (("direct-fast", I64, 8, DIRECT_FAST, 8), ("direct-generic", I16, 8, DIRECT_GENERIC, 0),
                                           ("tile", I64, 300, TILE, 8)):
            c = Case(f"wide{ncols}-{name}", wide_cols(ncols, key), P, NW, notes_of(route, fastw, 1, 10, maps))
            out += [c, c.with_("-masks", in_masks=masks, out_masks=masks)]
    c = Case("wide40-key-at-33-tile4", wide_cols(40, I32, 33), 100, NW, notes_of(TILE, 4, 1, 10, 1))
    out += [c, c.with_("-masks", in_masks=(1, 33, 39), out_masks=(1, 33, 39))]
    # beyond 1024 partitions and beyond 32 columns: one level
    c = Case("wide33-P2000-one-level", wide_cols(33, I64), 2000, 1 << 18, notes_of(DIRECT_FAST, 8, 1, 128, 1))
    return out + [c, c.with_("-masks", in_masks=(0, 31, 32), out_masks=(0, 31, 32))]


def _identity_cases():
    """D4: the identity hash at one level: hist<false>, scatter<false>, tile<false, 0>; negatives wrap, floats saturate"""
    out = []
    for key in (I8, I16, I32, I64, F32, F64, "2col"):
        cols = ["key:int32", "rid", "key:float64"] if key == "2col" else ["key:" + key, "rid", "val:int16"]
        for P, n, route in ((7, NB, DIRECT_GENERIC), (16, NB, DIRECT_GENERIC), (100, NB, TILE), (1024, NB, TILE), (5000, 200003, DIRECT_GENERIC)):
            out.append(Case(f"identity-{key}-P{P}", cols, P, n, notes_of(route, 0, 0, -(-n // 2048)), hash_func=IDENTITY))
    return out


def _fast4_cases():
    """D5: the 4-byte fast key on every route it can take, and P <= 2 with a fast key (wave_aggregated_inc)"""
    out = []
    for key in (I32, F32):
        for P, n, e in ((1, NB, notes_of(DIRECT_FAST, 4, 1, 49)), (2, NB, notes_of(DIRECT_FAST, 4, 1, 49)), (3, NB, notes_of(DIRECT_FAST, 4, 1, 49)),
                        (16, NB, notes_of(DIRECT_FAST, 4, 1, 49)), (700, NB, notes_of(TILE, 4, 1, 49)),
                        (4096, 1 << 18, notes_of(TWO_LEVEL, 4, 1, 128, 0, 6, 1))):
            out.append(Case(f"fast4-{key}-P{P}", ["key:" + key, "rid", "val:int8"], P, n, e))
    for key in (I64, F64):
        for P in (1, 2):
            out.append(Case(f"fast8-{key}-P{P}", ["key:" + key, "rid"], P, NB, notes_of(DIRECT_FAST, 8, 1, 49)))
    return out


KV = ["key:int64", "rid"]


def _boundary_cases():
    """D6: the row counts and partition counts at which the dispatcher changes route"""
    return [Case("bound-P32-n65535", KV, 32, 65535, notes_of(TILE, 8, 1, 32)),
            Case("bound-P32-n65536", KV, 32, 65536, notes_of(PAIRS, 8, 1, 32)),
            Case("bound-P128-n65535", KV, 128, 65535, notes_of(TILE, 8, 1, 32)),
            Case("bound-P128-n65536", KV, 128, 65536, notes_of(COLS8, 8, 1, 32)),
            Case("bound-P1025-n262143", KV, 1025, (1 << 18) - 1, notes_of(DIRECT_FAST, 8, 1, 128)),
            Case("bound-P1025-n262144", KV, 1025, 1 << 18, notes_of(TWO_LEVEL, 8, 1, 128, 0, 6, 1)),
            Case("bound-P16384-two-level", KV, 16384, 1 << 18, notes_of(TWO_LEVEL, 8, 1, 128, 0, 7, 1)),
            Case("bound-P16384-direct", KV, 16384, NB, notes_of(DIRECT_FAST, 8, 1, 49)),
            Case("bound-P16384-direct-generic", ["key:int16", "rid"], 16384, NB, notes_of(DIRECT_GENERIC, 0, 1, 49)),
            Case("bound-P16-n65536", KV, 16, 65536, notes_of(DIRECT_FAST, 8, 1, 32)),
            Case("bound-P17-n65536", KV, 17, 65536, notes_of(PAIRS, 8, 1, 32)),
            Case("bound-P64-n65536", KV, 64, 65536, notes_of(PAIRS, 8, 1, 32)),
            Case("bound-P65-n65536", KV, 65, 65536, notes_of(COLS8, 8, 1, 32)),
            Case("bound-P256-n65536", KV, 256, 65536, notes_of(COLS8, 8, 1, 32)),
            Case("bound-P257-n65536", KV, 257, 65536, notes_of(TILE, 8, 1, 32)),
            Case("bound-P1024-n262144", KV, 1024, 1 << 18, notes_of(TILE, 8, 1, 128)),
            Case("bound-3cols-P32", KV + ["val:float64"], 32, 65536, notes_of(COLS8, 8, 1, 32)),
            Case("bound-4cols-P256", KV + ["val:float64", "val:int64"], 256, 65536, notes_of(COLS8, 8, 1, 32)),
            Case("bound-5cols-P256", KV + ["val:float64", "val:int64", "val:int64"], 256, 65536, notes_of(TILE, 8, 1, 32))]


MASK_COLS = ["key:int64", "rid", "val:int32", "val:int8", "val:float64"]       # masks: key and int32 both sides, int8 input only, float64 output only
MASK_IN, MASK_OUT = (0, 2, 3), (0, 2, 4)


def _mask_cases():
    """D7: masks on every route that moves them, row counts that are no multiple of 8 or 32, a column masked on one side only"""
    k16 = ["key:int16"] + MASK_COLS[1:]
    out = []
    for n in (1000, NB):
        ch = -(-n // 2048)
        out += [Case(f"masks-direct-generic-n{n}", k16, 8, n, notes_of(DIRECT_GENERIC, 0, 1, ch), in_masks=MASK_IN, out_masks=MASK_OUT),
                Case(f"masks-direct-fast-n{n}", MASK_COLS, 8, n, notes_of(DIRECT_FAST, 8, 1, ch), in_masks=MASK_IN, out_masks=MASK_OUT),
                Case(f"masks-direct-fast4-n{n}", ["key:float32"] + MASK_COLS[1:], 2, n, notes_of(DIRECT_FAST, 4, 1, ch), in_masks=MASK_IN,
                     out_masks=MASK_OUT),
                Case(f"masks-tile-n{n}", MASK_COLS, 300, n, notes_of(TILE, 8, 1, ch), in_masks=MASK_IN, out_masks=MASK_OUT),
                Case(f"masks-tile-generic-n{n}", k16, 300, n, notes_of(TILE, 0, 1, ch), in_masks=MASK_IN, out_masks=MASK_OUT),
                Case(f"masks-apply-map-n{n}", wide_cols(34, I64), 8, n, notes_of(DIRECT_FAST, 8, 1, ch, 1), in_masks=(0, 2, 32, 33),
                     out_masks=(0, 2, 31, 33)),
                Case(f"masks-apply-map-tile-n{n}", wide_cols(34, I64), 300, n, notes_of(TILE, 8, 1, ch, 1), in_masks=(0, 2, 32, 33),
                     out_masks=(0, 2, 31, 33))]
    n = (1 << 18) + 5
    out += [Case("masks-two-level-fast", MASK_COLS, 2000, n, notes_of(TWO_LEVEL, 8, 1, 129, 0, 6, 1), in_masks=MASK_IN, out_masks=MASK_OUT),
            Case("masks-two-level-generic", k16, 2000, n, notes_of(TWO_LEVEL, 0, 1, 129, 0, 6, 1), in_masks=MASK_IN, out_masks=MASK_OUT),
            Case("masks-two-level-identity", ["key:int32"] + MASK_COLS[1:], 2000, n, notes_of(TWO_LEVEL, 0, 0, 129, 0, 6, 1), hash_func=IDENTITY,
                 in_masks=MASK_IN, out_masks=MASK_OUT),
            # a mask on one side only moves nothing: the 8-byte kernels still take the table
            Case("masks-input-only-pairs", KV, 32, 70001, notes_of(PAIRS, 8, 1, 35), in_masks=(0, 1)),
            Case("masks-output-only-pairs", KV, 32, 70001, notes_of(PAIRS, 8, 1, 35), out_masks=(0, 1)),
            Case("masks-one-side-cols8", KV + ["val:float64"], 128, 70001, notes_of(COLS8, 8, 1, 35), in_masks=(0, 2), out_masks=(1,)),
            Case("masks-both-sides-not-pairs", KV, 32, 70001, notes_of(TILE, 8, 1, 35), in_masks=(1,), out_masks=(1,)),
            Case("masks-both-sides-not-cols8", KV + ["val:float64"], 128, 70001, notes_of(TILE, 8, 1, 35), in_masks=(0,), out_masks=(0,))]
    return out


def _unaligned_cases():
    """D8: columns that start one element into their allocation: 8-byte but not 16-byte aligned on pairs and cols8, a 1-byte column
    at an odd address on the tile and the direct routes"""
    b = ["key:int64", "rid", "val:int8"]
    return [Case("unaligned-pairs", KV, 32, 70001, notes_of(PAIRS, 8, 1, 35), base_off=1),
            Case("unaligned-pairs-vk", ["rid", "key:float64"], 64, 70001, notes_of(PAIRS, 8, 1, 35), base_off=1),
            Case("unaligned-cols8", ["val:float64", "key:int64", "rid"], 128, 70001, notes_of(COLS8, 8, 1, 35), base_off=1),
            Case("unaligned-byte-tile", b, 300, NB, notes_of(TILE, 8, 1, 49), base_off=1),
            Case("unaligned-byte-direct-fast", b, 8, NB, notes_of(DIRECT_FAST, 8, 1, 49), base_off=1),
            Case("unaligned-byte-direct-generic", ["key:int8", "rid", "val:int8"], 8, NB, notes_of(DIRECT_GENERIC, 0, 1, 49), base_off=1)]


MULTI_TILE_CASES = _multi_tile_cases()
WIDTH_CASES = _width_cases()
WIDE_CASES = _wide_cases()
IDENTITY_CASES = _identity_cases()
FAST4_CASES = _fast4_cases()
BOUNDARY_CASES = _boundary_cases()
MASK_CASES = _mask_cases()
UNALIGNED_CASES = _unaligned_cases()
ALL_CASES = MULTI_TILE_CASES + WIDTH_CASES + WIDE_CASES + IDENTITY_CASES + FAST4_CASES + BOUNDARY_CASES + MASK_CASES + UNALIGNED_CASES

# further boundaries of the dispatcher that need no GPU run of their own: (dtypes, in masks, out masks, hashed, hash, P, n, forced) -> notes
MODEL_BOUNDARIES = [
    (([I64, I64], (), (), [0], MURMUR3, 2, NB, None), notes_of(DIRECT_FAST, 8, 1, 49)),
    (([I64, I64], (), (), [0], MURMUR3, 3, NB, None), notes_of(DIRECT_FAST, 8, 1, 49)),
    (([I64, I64], (), (), [0], MURMUR3, 16, 1 << 20, None), notes_of(DIRECT_FAST, 8, 1, 512)),
    (([I64, I64], (), (), [0], MURMUR3, 17, 1 << 20, None), notes_of(PAIRS, 8, 1, 512)),
    (([I64, I64], (), (), [0], MURMUR3, 17, 1 << 20, {"GDF_HP_NO_PAIRS": "1"}), notes_of(COLS8, 8, 1, 512)),
    (([I64, I64], (), (), [0], MURMUR3, 17, 1 << 20, {"GDF_HP_NO_PAIRS": "1", "GDF_HP_NO_COLS8": "1"}), notes_of(TILE, 8, 1, 512)),
    (([I64, I64], (), (), [0], IDENTITY, 32, 1 << 20, None), notes_of(TILE, 0, 0, 512)),
    (([I64, I32], (), (), [0], MURMUR3, 32, 1 << 20, None), notes_of(TILE, 8, 1, 512)),
    (([I64, I64], (), (), [0, 1], MURMUR3, 32, 1 << 20, None), notes_of(TILE, 0, 1, 512)),
    (([I64] * 32, (), (), [0], MURMUR3, 1025, 1 << 18, None), notes_of(TWO_LEVEL, 8, 1, 128, 0, 6, 1)),
    (([I64] * 33, (), (), [0], MURMUR3, 1025, 1 << 18, None), notes_of(DIRECT_FAST, 8, 1, 128, 1)),
    (([I64] * 65, (), (), [0], MURMUR3, 1025, 1 << 18, None), notes_of(DIRECT_FAST, 8, 1, 128, 2)),
    (([I64] * 64, (), (), [0], MURMUR3, 300, 1 << 18, None), notes_of(TILE, 8, 1, 128, 1)),
    (([I64, I64], (), (), [0], MURMUR3, 16384, 1 << 18, {"GDF_HP_ONE_LEVEL": "1"}), notes_of(DIRECT_FAST, 8, 1, 128)),
    (([I64, I64], (), (), [0], MURMUR3, 2048, 1 << 18, None), notes_of(TWO_LEVEL, 8, 1, 128, 0, 6, 1)),
    (([I64, I64], (), (), [0], MURMUR3, 4097, 1 << 18, None), notes_of(TWO_LEVEL, 8, 1, 128, 0, 7, 1)),
    # chunk rule: 2048-row chunks up to 2^21 rows, then ceil(n / 1024) rounded up to 2048; the selector; the piece rule
    (([I64, I64], (), (), [0], MURMUR3, 8, 1 << 21, None), notes_of(DIRECT_FAST, 8, 1, 1024)),
    (([I64, I64], (), (), [0], MURMUR3, 8, (1 << 21) + 1, None), notes_of(DIRECT_FAST, 8, 1, 513)),
    (([I64, I64], (), (), [0], MURMUR3, 8, N3, {"GDF_HP_MAX_CHUNKS": "0"}), notes_of(DIRECT_FAST, 8, 1, 1)),
    (([I64, I64], (), (), [0], MURMUR3, 8, N3, {"GDF_HP_MAX_CHUNKS": "5000"}), notes_of(DIRECT_FAST, 8, 1, 181)),
    (([I64, I32], (), (), [0], MURMUR3, 1025, 2_000_003, {"GDF_HP_PIECE": "150"}), notes_of(TWO_LEVEL, 8, 1, 977, 0, 6, 977)),
    (([I64, I32], (), (), [0], MURMUR3, 1025, 2_000_003, {"GDF_HP_PIECE": "3000"}), notes_of(TWO_LEVEL, 8, 1, 977, 0, 6, 41)),
]
