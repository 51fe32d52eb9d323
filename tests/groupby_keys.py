"""Helpers shared by the group-by / sort KEY tests (test_groupby_key_cases, test_gpu_groupby_keys, test_gpu_sort_keys): a table of
key tables that sit on the bit budgets csrc/groupby.hip and csrc/sort.hip branch on, a reference written from the documented
semantics (plain numpy: nothing from oracle/, nothing from the kernels' packing), a layout builder that carries every key table
onto the aggregation paths of groupby_values.PATHS, and a small Python MODEL of the two planning rules with a list of mutations
(the CPU file shows that the table tells every mutated model from the reference).

A CASE is a named list of key columns.  A column is an integer box `(dtype, lo, hi)` (inclusive), a float box given in IMAGE
space (`fbox`: the float values whose signed integer image lies in [lo, hi]; image -1 is -0.0, which the fold maps onto image 0),
or an explicit list of float values (`fvals`).  Every case records the budgets it was designed for:

  gb_bits    group-by rule (gb_plan_range, groupby.hip:1081-1122): a column takes bit_length(max - min) bits of its integer
             value / float image, a constant column 0 bits, column 0 on top; the plan packs iff the total is <= 63 and no NaN
             is present.  None: a NaN table (the plan declines).
  natural    all-integer keys of at most 8 bytes: gb_plan_keys packs the raw element bits, column 0 in the LOW bits, and the
             range plan is consulted by the sorted path only.
  sort_bits  sort rule (order_rows, sort.hip:715-759): a constant integer column owns 1 bit, a float column 32 / 64 bits; groups
             are formed from the LAST column backwards, at most 64 bits and at most 8 columns each.  Recorded as the tuple of
             group widths, last group first.

DESIGNATED ROWS of a case: the cartesian product of {lo, lo + 1, middle, hi - 1, hi} (every listed value of an `fvals` column) over
the case's corner columns (at most three), the other columns at a fixed value; for every other column two AXIS rows at its lo and
hi (so that the generated data has exactly the recorded ranges); and the case's explicit rows (the reserved word 1 << 63 of the
natural layout and its neighbours).  Designated row g occurs 1 + g % 3 times.  Filler rows come from the same box.

VALUES: one int64 per row, row number * an odd constant + an offset (mod 2^64): two different row sets have different wrapped
sums for all practical purposes, so a group that gained or lost a row shows in SUM even where COUNT agrees.

NOT SPECIFIED, so not compared (DESIGN.md section 4 repeats this):
  * where the NaN groups stand in sorted group-by output (every NaN row is a group of its own; they are matched by their
    aggregate);
  * which of -0.0 / +0.0 names a zero group: keys are compared with ==;
  * the sign and payload of a NaN key in the output: NaN membership only.
"""
import itertools

import numpy as np

from groupby_values import PATHS, HOT_IDS  # noqa: F401  (the row counts and forces of every path: imported, not copied)

I8, I16, I32, I64, F32, F64 = (np.dtype(x) for x in (np.int8, np.int16, np.int32, np.int64, np.float32, np.float64))
IMIN = {d: int(np.iinfo(d).min) for d in (I8, I16, I32, I64)}
IMAX = {d: int(np.iinfo(d).max) for d in (I8, I16, I32, I64)}
MAX_KEY_COLS = 16                 # csrc/common.h
GB_DIRECT_MAX_IDS = 12288         # csrc/groupby.hip
FEW_POOL = 3000
EMPTY_WORD = 1 << 63              # GB_EMPTY_KEY


# ---- float images (the model's statement of f32_image / f64_image: order like the values, equal iff ==) ------------------------------
def _int_of(dt):
    return np.dtype(f"i{np.dtype(dt).itemsize}")


def float_image(a, fold=True, flip=True):
    """signed integer image of a float array (int64): -0.0 folded onto +0.0, the magnitude bits of negatives flipped"""
    a = np.ascontiguousarray(a)
    it = _int_of(a.dtype)
    s = a.view(it).astype(np.int64)
    mag = np.int64(np.iinfo(it).max)
    if fold:
        s = np.where((s & mag) == 0, np.int64(0), s)
    if flip:
        s = np.where(s < 0, s ^ mag, s)
    return s


def float_of_image(img, dt):
    """the float whose image is img (image -1: -0.0)"""
    dt = np.dtype(dt)
    it = _int_of(dt)
    s = np.asarray(img, dtype=np.int64)
    s = np.where(s < 0, s ^ np.int64(np.iinfo(it).max), s)
    return s.astype(it).view(dt)


def _bits_float(dt, bits):
    return np.array([bits], dtype=f"u{np.dtype(dt).itemsize}").view(dt)[0]


def nan_values(dt):
    """+NaN, -NaN and +NaN with an all-ones payload"""
    dt = np.dtype(dt)
    w = dt.itemsize * 8
    quiet = (0x7fc << 20) if w == 32 else (0x7ff8 << 48)
    return [_bits_float(dt, quiet), _bits_float(dt, quiet | (1 << (w - 1))), _bits_float(dt, (1 << (w - 1)) - 1)]


# ---- columns and cases ---------------------------------------------------------------------------------------------------------------
class Col:
    """kind "int": integer box [lo, hi]; "fbox": float box in image space [lo, hi]; "fvals": explicit values (floats; for the sort's
    skipped digit also integers)"""

    def __init__(self, kind, dtype, lo=None, hi=None, values=None):
        self.kind, self.dtype, self.lo, self.hi = kind, np.dtype(dtype), lo, hi
        self.values = None if values is None else np.array(values, dtype=self.dtype)
        if kind == "int":
            assert IMIN[self.dtype] <= lo <= hi <= IMAX[self.dtype]

    def _conv(self, ints):
        a = np.asarray(ints, dtype=np.int64)
        return a.astype(self.dtype) if self.kind == "int" else float_of_image(a, self.dtype)

    def points(self):
        """the corner values of the column"""
        if self.kind == "fvals":
            return self.values
        lo, hi = self.lo, self.hi
        mid = lo + (hi - lo) // 2
        return self._conv(sorted({lo, min(lo + 1, hi), mid, max(hi - 1, lo), hi}))

    def ends(self):
        return self.values if self.kind == "fvals" else self._conv([self.lo, self.hi])

    def fixed(self):
        return self.values[0] if self.kind == "fvals" else self._conv([self.lo + (self.hi - self.lo) // 2])[0]

    def draw(self, rng, n):
        if self.kind == "fvals":
            return self.values[rng.integers(0, len(self.values), size=n)]
        return self._conv(rng.integers(self.lo, self.hi, size=n, endpoint=True, dtype=np.int64))


def ibox(dtype, lo, hi):
    return Col("int", dtype, lo, hi)


def ispan(dtype, lo, bits):
    """an integer column whose field of `bits` bits is FULL: span 2^bits - 1"""
    return Col("int", dtype, lo, lo + (1 << bits) - 1)


def fbox(dtype, lo_img, hi_img):
    return Col("fbox", dtype, lo_img, hi_img)


def fvals(dtype, values):
    return Col("fvals", dtype, values=values)


class Case:
    def __init__(self, name, cols, gb_bits, sort_bits, corners=None, rows=(), note=""):
        self.name, self.cols, self.gb_bits, self.sort_bits, self.note = name, cols, gb_bits, tuple(sort_bits), note
        self.corners = tuple(range(min(3, len(cols)))) if corners is None else tuple(corners)
        self.rows = [tuple(r) for r in rows]
        self.all_int = all(c.dtype.kind == "i" for c in cols)
        self.natural = self.all_int and sum(c.dtype.itemsize for c in cols) <= 8
        self.has_nan = any(c.kind == "fvals" and c.dtype.kind == "f" and np.isnan(c.values).any() for c in cols)
        assert len(self.corners) <= 3

    def __repr__(self):
        return f"Case({self.name})"


def _specials(dt):
    fi = np.finfo(dt)
    v = [0.0, fi.smallest_subnormal, fi.tiny, 1.5, fi.max, np.inf]
    return [s * x for x in v for s in (1.0, -1.0)]


def _cases():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))
    # -- dtype extremes: a box that starts at iinfo.min, one that ends at iinfo.max (span 12: 4 bits)
    for dt in (I8, I16, I32, I64):
        add(f"min_{dt.name}", [ibox(dt, IMIN[dt], IMIN[dt] + 12)], 4, (4,))
        add(f"max_{dt.name}", [ibox(dt, IMAX[dt] - 12, IMAX[dt])], 4, (4,))
    add("int8_full", [ibox(I8, -128, 127)], 8, (8,))
    add("i64_straddles_0", [ibox(I64, -7, 8)], 4, (4,))
    add("i64_straddles_2p32", [ibox(I64, (1 << 32) - 5, (1 << 32) + 6)], 4, (4,))
    add("i64_full", [ibox(I64, IMIN[I64], IMAX[I64])], 64, (64,), note="span 2^64 - 1: no range plan; the natural layout holds it")
    # -- span edges: the field is full (span 2^k - 1) / one more bit with only the top bit set at hi (span 2^k)
    add("span_full_small", [ispan(I32, 100, 3), ispan(I32, -50, 3)], 6, (6,))
    add("span_2k_small", [ibox(I32, 100, 108), ibox(I32, -50, -42)], 8, (8,))
    add("span_full_large", [ispan(I64, -(1 << 40), 40), ispan(I16, 0, 10)], 50, (50,))
    add("span_2k_large", [ibox(I64, 5, 5 + (1 << 40)), ibox(I16, -512, 512)], 52, (52,))
    # -- a constant column first / in the middle / last (0 bits in the group-by rule, 1 never-varying bit in the sort rule); its value
    #    0x55 has bits where the neighbouring fields vary
    add("const_first", [ibox(I32, 0x55, 0x55), ispan(I16, 0, 3), ispan(I8, -4, 3)], 6, (7,))
    add("const_middle", [ispan(I16, 0, 3), ibox(I32, 0x55, 0x55), ispan(I8, -4, 3)], 6, (7,))
    add("const_last", [ispan(I16, 0, 3), ispan(I8, -4, 3), ibox(I64, 0x55, 0x55)], 6, (7,))
    # -- budget edges: (int64, int32) is the statically typed signature of the fused pass; 12 bytes, so the range plan is THE plan
    two = lambda a, b, la=-1000, lb=7: [ispan(I64, la, a), ispan(I32, lb, b)]
    add("total_13", two(7, 6), 13, (13,), note="8192 ids: the dense dictionary (at most 16384 groups)")
    add("total_14", two(8, 6), 14, (14,), note="part_bits 1, but at most 16384 groups exist: the dense dictionary claims it unless it counts rows (AVG, masked values: 12288)")
    add("total_15", two(9, 6), 15, (15,), note="the lowest total that reaches the fused pass under every op (32768 groups)")
    add("total_24", two(17, 7, la=IMIN[I64]), 24, (24,), note="part_bits 11: the last total of the fused pass")
    add("total_25", [ispan(I32, IMAX[I32] - (1 << 13) + 1, 13), ispan(I64, -5, 12)], 25, (25,), note="part_bits 12: partitioned, not fused")
    add("total_26", [ispan(I64, 1 << 40, 20), ispan(I16, -4, 3), ispan(I8, 120, 3)], 26, (26,), note="part_bits 13 = GB_PART_MAX_BITS")
    add("total_27", two(19, 8), 27, (27,), note="the first total past GB_PART_MAX_BITS: sorted")
    add("total_30", two(22, 8), 30, (30,))
    add("total_31", two(23, 8), 31, (31,))
    add("total_32", two(24, 8), 32, (32,))
    add("total_62", two(40, 22, la=IMIN[I64], lb=IMIN[I32]), 62, (62,))
    add("total_63", two(40, 23, la=IMAX[I64] - (1 << 40) + 1, lb=IMAX[I32] - (1 << 23) + 1), 63, (63,))
    add("total_64_wide", [ibox(I64, -3, -3 + (1 << 40)), ispan(I32, 7, 23)], 64, (64,),
        note="64 bits in 12 bytes: no packed plan, the first-row table; (hi, lo) would pack to the reserved word")
    add("total_64_natural", [ibox(I32, IMIN[I32], IMAX[I32]), ibox(I32, IMIN[I32], IMAX[I32])], 64, (64,),
        rows=[(0, IMIN[I32]), (-1, IMAX[I32]), (1, IMIN[I32]), (0, 0), (-1, -1)],
        note="the natural layout, unordered; column 0 in the LOW bits: (0, INT32_MIN) is the reserved word 1 << 63")
    add("total_65_sort", [ispan(I64, -9, 33), ibox(I32, IMIN[I32], IMAX[I32])], 65, (32, 33), note="sort: two groups from the width")
    # -- the fused pass beyond the static signature: three and four columns of mixed widths (the c >= 2 loop of gbp_pack32)
    add("three_cols_18", [ispan(I8, -16, 5), ispan(I16, 1000, 6), ispan(I32, -64, 7)], 18, (18,))
    add("four_cols_20", [ispan(I16, -8, 4), ispan(I8, 0, 4), ispan(I32, 1 << 20, 6), ispan(I64, -(1 << 50), 6)], 20, (20,), corners=(0, 2, 3))
    add("two_i32_static_20", [ispan(I32, IMIN[I32], 10), ispan(I32, IMAX[I32] - 1023, 10)], 20, (20,))
    # -- the reserved word of the natural layout in several columns, with (1 << 63) - 1, (1 << 63) + 1, 0 and all-ones
    add("reserved_i16_i16_i32", [ibox(I16, IMIN[I16], IMAX[I16]), ibox(I16, IMIN[I16], IMAX[I16]), ibox(I32, IMIN[I32], IMAX[I32])], 64, (64,),
        rows=[(0, 0, IMIN[I32]), (-1, -1, IMAX[I32]), (1, 0, IMIN[I32]), (0, 0, 0), (-1, -1, -1)])
    add("reserved_8_x_i8", [ibox(I8, -128, 127) for _ in range(8)], 64, (64,), corners=(0, 3, 7),
        rows=[(0,) * 7 + (-128,), (-1,) * 7 + (127,), (1,) + (0,) * 6 + (-128,), (0,) * 8, (-1,) * 8])
    # -- direct-path ids: the product of the spans at, just above and (three columns) at GB_DIRECT_MAX_IDS
    add("direct_96x128", [ibox(I64, IMIN[I64], IMIN[I64] + 95), ibox(I64, IMAX[I64] - 127, IMAX[I64])], 14, (14,))
    add("direct_97x127", [ibox(I64, IMIN[I64], IMIN[I64] + 96), ibox(I64, IMAX[I64] - 126, IMAX[I64])], 14, (14,), note="12319 ids: not direct")
    add("direct_16x24x32", [ibox(I8, -128, -113), ibox(I16, IMAX[I16] - 23, IMAX[I16]), ibox(I32, -16, 15)], 14, (14,))
    # -- column counts: 9 and 16 narrow columns stay far below 64 bits, so only sort's 8-column cap splits the group
    add("nine_cols", [ispan(I8 if k % 2 else I16, -4 + k, 3) for k in range(9)], 27, (24, 3), corners=(0, 4, 8))
    add("sixteen_cols", [ispan((I8, I16, I32, I64)[k % 4], 10 * k - 80, 3) for k in range(16)], 48, (24, 24), corners=(0, 7, 15))
    # -- sort image widths that take 9-bit digits: spans of 9, 17, 18, 25, 26, 27 bits
    for w in (9, 17, 18, 25, 26, 27):
        add(f"sort_width_{w}", [ispan(I64, -(1 << (w - 1)), w)], w, (w,))
    # bits 0 .. 7 and bit 26 vary, bits 8 .. 25 agree: the middle one of the three 9-bit windows is skipped
    add("sort_skipped_digit", [fvals(I64, list(range(200)) + [1 << 26, (1 << 26) + 255])], 27, (27,))
    # -- float keys
    for dt in (F32, F64):
        n, w = dt.name, dt.itemsize * 8
        one = int(float_image(np.array([1.0], dtype=dt))[0])
        # +-inf: image span 2 * image(inf) + 1 -- 32 bits for float32 (0xff000001), 64 bits for float64, which leaves the packed paths
        add(f"{n}_specials", [fvals(dt, _specials(dt))], w, (w,))
        if dt == F32:
            add(f"{n}_band", [fbox(dt, one, one + (1 << 23) - 1)], 23, (32,), note="[1, 2): 2^23 images")
        else:
            add(f"{n}_band", [fbox(dt, one, one + (1 << 22))], 23, (64,), note="[1, 1 + 2^-30]: 2^22 + 1 images")
        add(f"{n}_across_zero", [fbox(dt, -201, 200)], 9, (w,), note="200 negative denormals (flipped images), -0.0, +0.0, 200 positive denormals")
        add(f"{n}_then_int", [fbox(dt, one, one + 1023), ispan(I32, -8, 4)], 14, (w + 4,) if w + 4 <= 64 else (4, w))
        add(f"int_then_{n}", [ispan(I32, -8, 4), fbox(dt, -8, 7)], 8, (w + 4,) if w + 4 <= 64 else (w, 4))
        add(f"{n}_nan", [fvals(dt, [1.0, -2.0, 0.0, -0.0] + nan_values(dt)), ispan(I16, 0, 2)], None, (w + 2,) if w + 2 <= 64 else (2, w),
            note="+NaN, -NaN, all-ones payload among ordinary keys: every NaN row its own group, the plan declines")
    # (a float column in the last group and in the first: float64_then_int / int_then_float64 split into two groups)
    names = [x.name for x in c]
    assert len(set(names)) == len(names)
    return c


CASES = _cases()
CASE = {c.name: c for c in CASES}


# ---- designated rows, fillers, layouts -------------------------------------------------------------------------------------------------
def designated(case):
    """the designated rows of a case as a list of column arrays (see the module docstring)"""
    cols = case.cols
    fixed = [c.fixed() for c in cols]
    rows = []
    for combo in itertools.product(*[cols[k].points() for k in case.corners]):
        r = list(fixed)
        for k, v in zip(case.corners, combo):
            r[k] = v
        rows.append(r)
    for k, col in enumerate(cols):
        if k in case.corners:
            continue
        for v in col.ends():
            r = list(fixed)
            r[k] = v
            rows.append(r)
    for r in case.rows:
        rows.append([np.array([v]).astype(col.dtype)[0] for v, col in zip(r, cols)])
    reps = 1 + np.arange(len(rows)) % 3
    return [np.repeat(np.array([r[k] for r in rows], dtype=cols[k].dtype), reps) for k in range(len(cols))]


def scramble(n, offset=0):
    """the value of row i: (i + offset) * an odd constant + 12345 (mod 2^64) as int64"""
    with np.errstate(over="ignore"):
        return ((np.arange(n, dtype=np.uint64) + np.uint64(offset)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)).view(np.int64)


def _hot_ids(case, rng, n):
    """n rows whose packed id (group-by rule, column 0 on top) is below HOT_IDS: integer columns only"""
    assert all(c.kind == "int" for c in case.cols)
    ids = rng.integers(0, HOT_IDS, size=n, dtype=np.int64)
    out = [None] * len(case.cols)
    for k in range(len(case.cols) - 1, -1, -1):
        col = case.cols[k]
        bits = (col.hi - col.lo).bit_length()
        out[k] = (col.lo + (ids & ((1 << bits) - 1))).astype(col.dtype)
        assert int(out[k].max()) <= col.hi
        ids = ids >> bits
    return out


class Layout:
    """keys: the key columns; vals: int64; n_designated: how many rows are designated ones (before the shuffle)"""


def layout(case, regime, rows, rng):
    """the designated rows of the case plus filler drawn from its box, shuffled.  regime "few": filler from a fixed pool of about
    3000 box points (dictionary, LDS dictionary, direct); "many": uniform over the box (partitioned, sorted, table); "hot": half of
    the filler inside the first 4096 ids"""
    des = designated(case)
    nfill = max(rows - len(des[0]), 16)
    if regime == "few":
        pool = [c.draw(rng, FEW_POOL) for c in case.cols]
        pick = rng.integers(0, FEW_POOL, size=nfill)
        fill = [p[pick] for p in pool]
    elif regime == "many":
        fill = [c.draw(rng, nfill) for c in case.cols]
    else:
        assert regime == "hot"
        hot = _hot_ids(case, rng, nfill // 2)
        cold = [c.draw(rng, nfill - nfill // 2) for c in case.cols]
        fill = [np.concatenate([h, x]) for h, x in zip(hot, cold)]
    order = rng.permutation(len(des[0]) + nfill)
    out = Layout()
    out.case, out.regime = case, regime
    out.keys = [np.ascontiguousarray(np.concatenate([d, f])[order]) for d, f in zip(des, fill)]
    out.vals = scramble(len(order))
    out.n_designated = len(des[0])
    return out


def guess_layout(which, rows, rng):
    """one int64 key column for the direct path's GUESSED window (more than 2^20 rows; the window comes from the first 65536 rows and
    is widened by room = (12288 - span) / 2 on both sides, saturating at the int64 limits):
      near_max / near_min   keys within 100 of INT64_MAX / INT64_MIN: the saturating branches
      edge_inside           the first 65536 rows span 10 values, later rows lie exactly at lo - room and hi + room
      edge_outside          ... and one row at lo - room - 1 (hi side: hi + room - 5, so that the exact range still fits 12288 ids):
                            the guess is violated and the call repeats with the exact range"""
    assert rows > (1 << 20)
    if which in ("near_max", "near_min"):
        lo = IMAX[I64] - 100 if which == "near_max" else IMIN[I64]
        k = rng.integers(lo, lo + 100, size=rows, endpoint=True, dtype=np.int64)
        k[:101] = np.arange(lo, lo + 101, dtype=np.int64)                     # the whole box inside the sampled prefix
    else:
        lo, hi = 1_000_000, 1_000_009
        room = (GB_DIRECT_MAX_IDS - 10) // 2
        k = rng.integers(lo, hi, size=rows, endpoint=True, dtype=np.int64)
        k[:10] = np.arange(lo, hi + 1)
        tail = rng.integers(lo - room + 1, hi + room - 6, size=rows - (1 << 16), endpoint=True, dtype=np.int64)
        k[1 << 16:] = tail
        if which == "edge_inside":
            k[-3:] = [lo - room, hi + room, lo - room]
        else:
            assert which == "edge_outside"
            k[-3:] = [lo - room - 1, hi + room - 5, lo - room]
    out = Layout()
    out.case, out.regime = None, which
    out.keys = [np.ascontiguousarray(k)]
    out.vals = scramble(rows)
    out.n_designated = 0
    return out


def masks(lay, variant, rng):
    """(key valids per column, value valid) of a variant: "plain" none; "vmask" a quarter of the values null (sets vbit); "kmask" 3 % of
    column 0's elements null (sets null_bit); "bothmask" both"""
    n = len(lay.vals)
    kv = [None] * len(lay.keys)
    vv = None
    if variant in ("vmask", "bothmask"):
        vv = rng.random(n) >= 0.25
    if variant in ("kmask", "bothmask"):
        kv[0] = rng.random(n) >= 0.03
    assert variant in ("plain", "vmask", "kmask", "bothmask")
    return kv, vv


# ---- the reference ---------------------------------------------------------------------------------------------------------------------
def _canonical(keys):
    """per float column: -0.0 -> +0.0, NaN -> 0 with the row flagged; returns (columns, nan row flags)"""
    cols, nan = [], np.zeros(len(keys[0]), dtype=bool)
    for k in keys:
        if k.dtype.kind == "f":
            isn = np.isnan(k)
            nan |= isn
            k = np.where(isn, k.dtype.type(0), k) + k.dtype.type(0)            # x + 0.0: -0.0 becomes +0.0
        cols.append(k)
    return cols, nan


class Groups:
    """keys (per column, one row per group), rows (int64 row count), count (valid values), sum (wrapped int64 over the valid values),
    min (over the valid values; 0 where there is none), ok (the group has a valid value), last (the group's last row in input order);
    groups in lexicographic typed order, NaN groups somewhere"""


def reference(keys, vals, key_valids=None, val_valid=None):
    n = len(vals)
    keep = np.ones(n, dtype=bool)
    for v in (key_valids or []):
        if v is not None:
            keep &= v
    rows = np.flatnonzero(keep)
    ks = [k[rows] for k in keys]
    cols, nan = _canonical(ks)
    tag = np.where(nan, rows + 1, 0)                                            # every NaN row is a group of its own
    order = np.lexsort((tag,) + tuple(reversed(cols)))
    head = np.ones(len(rows), dtype=bool)
    if len(rows) > 1:
        same = tag[order][1:] == tag[order][:-1]
        for c in cols:
            cs = c[order]
            same &= cs[1:] == cs[:-1]
        head[1:] = ~same
    starts = np.flatnonzero(head)
    g = Groups()
    g.keys = [k[order][starts] for k in ks]
    g.rows = np.diff(np.append(starts, len(rows))).astype(np.int64)
    v = vals[rows][order]
    ok = np.ones(len(rows), dtype=bool) if val_valid is None else val_valid[rows][order]
    with np.errstate(over="ignore"):
        if len(rows):
            g.count = np.add.reduceat(ok.astype(np.int64), starts)
            g.sum = np.add.reduceat(np.where(ok, v, 0), starts)
            g.min = np.minimum.reduceat(np.where(ok, v, np.int64(IMAX[I64])), starts)
            g.last = np.maximum.reduceat(rows[order], starts)
        else:
            g.count = g.sum = g.min = g.last = np.zeros(0, dtype=np.int64)
    g.ok = g.count > 0
    g.min = np.where(g.ok, g.min, 0)
    g.nan = np.zeros(len(starts), dtype=bool)
    for k in g.keys:
        if k.dtype.kind == "f":
            g.nan |= np.isnan(k)
    return g


def expected(g, op, masked):
    """the aggregate column of a HASH group-by over int64 values: COUNT in int64 (the valid values), SUM / MIN in int64, AVG in int64
    (C++ division of the wrapped sum by the count, truncating toward zero); a group without a valid value reports 0"""
    if op == "count":
        return g.count if masked else g.rows
    if op == "sum":
        return g.sum
    if op == "min":
        return g.min
    assert op == "avg"
    c = np.where(g.count != 0, g.count, 1)
    q = g.sum // c
    q = q + ((g.sum - q * c != 0) & (g.sum < 0))
    return np.where(g.count != 0, q, 0)


def order_reference(keys):
    """the stable permutation gdf_order_by owes: lexicographic, -0.0 == +0.0, every NaN behind +inf and onto one value"""
    seq = []
    for k in keys:
        if k.dtype.kind == "f":
            isn = np.isnan(k)
            seq += [isn, np.where(isn, k.dtype.type(0), k)]
        else:
            seq.append(k)
    return np.lexsort(tuple(reversed(seq))).astype(np.int64)


def match_order(keys, agg):
    """an order that lines two group tables up whatever order they came in: by canonical key, NaN flags, then the aggregate (which
    tells the single-row NaN groups apart)"""
    seq = []
    for k in keys:
        if k.dtype.kind == "f":
            isn = np.isnan(k)
            seq += [isn, np.where(isn, k.dtype.type(0), k)]
        else:
            seq.append(k)
    return np.lexsort((agg,) + tuple(reversed(seq)))


def assert_groups(got_keys, got_agg, got_ok, g, op, masked, in_order=False, what=""):
    """a group-by result against the reference: integer keys exactly, float keys with == plus NaN membership, the aggregate in int64
    exactly; in_order: the rows must stand in the reference's order as they are (no NaN case)"""
    want = expected(g, op, masked)
    assert len(got_agg) == len(want), (what, len(got_agg), len(want))
    assert got_agg.dtype == np.int64, (what, got_agg.dtype)
    if in_order:
        assert not g.nan.any()
        a = b = slice(None)
    else:
        a, b = match_order(got_keys, got_agg), match_order(g.keys, want)
    for c, (gk, ek) in enumerate(zip(got_keys, g.keys)):
        assert gk.dtype == ek.dtype, (what, c)
        gk, ek = gk[a], ek[b]
        if gk.dtype.kind == "f":
            np.testing.assert_array_equal(np.isnan(gk), np.isnan(ek), err_msg=f"{what}: NaN membership, column {c}")
            ok = ~np.isnan(ek)
            assert (gk[ok] == ek[ok]).all(), f"{what}: key column {c}"
        else:
            np.testing.assert_array_equal(gk, ek, err_msg=f"{what}: key column {c}")
    np.testing.assert_array_equal(got_agg[a], want[b], err_msg=f"{what}: {op}")
    if got_ok is not None:
        want_ok = np.ones(len(want), dtype=bool) if op == "count" else g.ok
        np.testing.assert_array_equal(got_ok[a], want_ok[b], err_msg=f"{what}: valid bits")


# ---- the model of the planning rules, and its mutations --------------------------------------------------------------------------------
MUTATIONS = ["width_one_bit_short", "bias_plus_one", "bias_ignored", "span_signed_64", "shift_off_by_one", "columns_reversed",
             "no_zero_fold", "no_sign_flip", "budget_gt_64", "sort_constant_0_bits", "sort_cap_9_columns"]
GB_MUTATIONS = MUTATIONS[:9]
SORT_MUTATIONS = MUTATIONS[9:]


def _wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def images(keys, mutation=None):
    """every key column as the int64 array the packing works on: integers their value, floats their image"""
    return [float_image(k, fold=mutation != "no_zero_fold", flip=mutation != "no_sign_flip") if k.dtype.kind == "f" else k.astype(np.int64)
            for k in keys]


class Plan:
    """packed, total, bits[c], bias[c], shift[c] (the GbKeyPlan of the range layout)"""


def gb_plan(keys, key_valids=None, mutation=None):
    """the group-by rule (gb_plan_range): bits = bit_length(max - min) over the valid elements, column 0 on top, packs iff the total is at
    most 63 bits and no NaN was seen"""
    p = Plan()
    p.packed, p.bits, p.bias, p.shift = False, [], [], []
    for k in keys:
        if k.dtype.kind == "f" and np.isnan(k).any():
            p.total = None
            return p
    kv = key_valids or [None] * len(keys)
    for img, v in zip(images(keys, mutation), kv):
        img = img if v is None else img[v]
        lo, hi = (int(img.min()), int(img.max())) if len(img) else (0, 0)
        span = hi - lo
        if mutation == "span_signed_64":
            span = max(_wrap64(span), 0)                       # a negative span reads as "no valid element": a constant column
        bits = span.bit_length()
        if mutation == "width_one_bit_short":
            bits = max(bits - 1, 0)
        p.bits.append(bits)
        p.bias.append(0 if mutation == "bias_ignored" else lo + (mutation == "bias_plus_one"))
    p.total = sum(p.bits)
    p.packed = p.total <= (64 if mutation == "budget_gt_64" else 63)
    below = p.total
    order = range(len(keys)) if mutation != "columns_reversed" else range(len(keys) - 1, -1, -1)
    p.shift = [0] * len(keys)
    for c in order:
        below -= p.bits[c]
        p.shift[c] = below
    if mutation == "shift_off_by_one":
        p.shift = [max(s - 1, 0) for s in p.shift]
    return p


def _mask(bits):
    return np.uint64((1 << bits) - 1) if bits < 64 else np.uint64((1 << 64) - 1)


def pack(imgs, p):
    """gb_pack over whole columns: OR of ((image - bias) & low_mask(bits)) << shift"""
    word = np.zeros(len(imgs[0]), dtype=np.uint64)
    with np.errstate(over="ignore"):
        for img, bits, bias, shift in zip(imgs, p.bits, p.bias, p.shift):
            if bits == 0:
                continue
            field = (img - np.int64(_wrap64(bias))).view(np.uint64) & _mask(bits)
            word |= field << np.uint64(shift)
    return word


def unpack(word, p, dtypes, mutation=None):
    """gb_unpack_store over whole columns: ((word >> shift) & low_mask(bits)) + bias, floats back through the image"""
    out = []
    with np.errstate(over="ignore"):
        for bits, bias, shift, dt in zip(p.bits, p.bias, p.shift, dtypes):
            f = (word >> np.uint64(shift)) & _mask(bits) if bits else np.zeros(len(word), dtype=np.uint64)
            img = (f + np.uint64(bias & ((1 << 64) - 1))).view(np.int64)
            if np.dtype(dt).kind == "f":
                out.append(float_of_image(img, dt) if mutation != "no_sign_flip" else img.astype(_int_of(dt)).view(dt))
            else:
                out.append(img.astype(dt))
    return out


def model_group_by(keys, mutation=None):
    """(key columns, row counts) of the groups the packed paths would report under the (mutated) rule, in the order of the packed
    word -- which the range plan promises to be the lexicographic typed order; None: the rule does not pack (the first-row table takes
    the rows, which compares rows and is the reference itself).  The range plan also promises that the word 1 << 63 cannot occur
    (groupby.hip:1117): the model treats it as the empty marker it is, so a row that packs to it is lost."""
    p = gb_plan(keys, mutation=mutation)
    if p.total is None or not p.packed:
        return None
    word = pack(images(keys, mutation), p)
    word = word[word != np.uint64(EMPTY_WORD)] if p.total == 64 else word
    u, counts = np.unique(word, return_counts=True)
    return unpack(u, p, [k.dtype for k in keys], mutation), counts.astype(np.int64)


def sort_plan(keys, mutation=None):
    """the sort rule (order_rows): per-column widths (constant integer column 1 bit, floats full width) and the groups as lists of
    column numbers, last group first: at most 64 bits and at most 8 columns each"""
    width = []
    for k in keys:
        if k.dtype.kind == "f":
            width.append(k.dtype.itemsize * 8)
        else:
            w = (int(k.max()) - int(k.min())).bit_length() if len(k) else 0
            width.append(w if w or mutation == "sort_constant_0_bits" else 1)
    cap = 9 if mutation == "sort_cap_9_columns" else 8
    groups, c = [], len(keys) - 1
    while c >= 0:
        bits, first = 0, c
        while first >= 0 and bits + width[first] <= 64 and c - first < cap:
            bits += width[first]
            first -= 1
        groups.append(list(range(first + 1, c + 1)))
        c = first
    return width, groups


def _sort_float_image(k):
    """ordered_float_bits: unsigned, -0.0 folded, NaN all ones"""
    w = k.dtype.itemsize * 8
    u = k.view(f"u{k.dtype.itemsize}").astype(np.uint64)
    top = np.uint64(1 << (w - 1))
    full = np.uint64((1 << w) - 1)
    u = np.where((u & (full >> np.uint64(1))) == 0, np.uint64(0), u)
    img = np.where((u & top) != 0, ~u & full, u | top)
    return np.where(np.isnan(k), full, img)


def sort_group_images(keys, mutation=None):
    """the 64-bit image of every column group under the (mutated) sort rule, last group first.  A SortGroup has 8 column slots: under
    the 9-column cap the ninth column of a group is not stored, so it is not sorted on; a field of 0 bits is read as a float field
    (that is what bits == 0 means in SortGroup), here the integer's raw 64-bit ordered image OR-ed in at the field's shift"""
    width, groups = sort_plan(keys, mutation)
    out = []
    with np.errstate(over="ignore"):
        for grp in groups:
            image = np.zeros(len(keys[0]), dtype=np.uint64)
            shift = sum(width[c] for c in grp)
            for slot, c in enumerate(grp):
                shift -= width[c]
                if slot >= 8:
                    continue
                k = keys[c]
                if k.dtype.kind == "f":
                    f = _sort_float_image(k)
                elif width[c] == 0:
                    f = k.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)
                else:
                    f = (k.astype(np.int64) - np.int64(int(k.min()))).view(np.uint64) & _mask(width[c])
                image |= f << np.uint64(shift)
            out.append(image)
    return out


def model_order_by(keys, mutation=None):
    """the permutation the (mutated) sort rule gives: stable sorts by the group images, from the last group to the first"""
    perm = np.arange(len(keys[0]), dtype=np.int64)
    for image in sort_group_images(keys, mutation):
        perm = perm[np.argsort(image[perm], kind="stable")]
    return perm


def scatter_launches(image):
    """how many radix passes one group image costs, from the comment above radix_sort_pairs (sort.hip): the varying bits [lo, hi) are
    covered by (span + 8) / 9 windows of 8 or 9 bits, and a window on which every key agrees is skipped"""
    varying = int(np.bitwise_or.reduce(image ^ image[0]))
    if varying == 0:
        return 0
    lo, hi = (varying & -varying).bit_length() - 1, varying.bit_length()
    span = hi - lo
    passes = (span + 8) // 9
    bpp = (span + passes - 1) // passes
    bits = 9 if bpp > 8 else 8
    return sum(1 for p in range(passes) if (varying >> (lo + p * bpp)) & ((1 << bits) - 1))


# ---- GPU-side helpers ------------------------------------------------------------------------------------------------------------------
def profile_of(gdf, call):
    """{kernel name: launches} of one library call (the exported profile hooks of include/gdf/gdf_amd_ext.h)"""
    from bench import read_profile
    lib = gdf._binding._gdf_cdll
    lib.gdf_amd_profile_reset(); lib.gdf_amd_profile_enable(1)
    try:
        call()
    finally:
        lib.gdf_amd_profile_enable(0)
    return {name: launches for name, (ms, launches) in read_profile(gdf).items()}


def run_hash(gdf, op, keys, vals, key_valids=None, val_valid=None, sort_result=False):
    """the HASH group-by through the C ABI -> (key arrays, aggregate, aggregate-valid bools or None), rows as the library left them.
    COUNT comes out in int64, everything else in the value dtype (int64)"""
    from libgdf_amd.columns import column_from_numpy, get_dtype
    kv = key_valids or [None] * len(keys)
    masked = val_valid is not None or any(v is not None for v in kv)
    kc = [column_from_numpy(k, v) for k, v in zip(keys, kv)]
    vc = column_from_numpy(vals, val_valid)
    res = gdf.api.group_by(op, kc, vc, out_dtype=get_dtype(np.int64), sort_result=sort_result, with_masks=masked)
    gk, ga = [x.cpu().numpy() for x in res[0]], res[1].cpu().numpy()
    return gk, ga, (res[2].numpy() if masked else None)
