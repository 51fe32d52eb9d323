"""Helpers of the tests of csrc/quantile.hip and csrc/reduce.hip that construct their inputs on purpose: the
order-preserving key image and its 11-bit digits, columns whose ranks k and k + 1 part at a chosen digit, columns that put one
bucket's keys into chosen regions of the candidate buffer, a host model of the selection's state machine, the NaN bit patterns, and
slices of a guarded device buffer.  Importing this module needs no GPU; tests/test_stats_constructions.py checks every construction
here without one."""
import ctypes as C

import numpy as np

from elementwise_common import Buf

QT_DIGIT = 11
QT_NSUB = 256                       # regions of the candidate buffer
QT_CAND_CAP = 1 << 22               # candidate keys
ALL_DTYPES = [np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]

# NaN bit patterns: positive quiet, signalling, all-ones payload, minimum payload; then each with the sign bit set
NAN_BITS = {
    np.dtype(np.float32): [0x7FC00000, 0x7FA00000, 0x7FFFFFFF, 0x7F800001, 0xFFC00000, 0xFFA00000, 0xFFFFFFFF, 0xFF800001],
    np.dtype(np.float64): [0x7FF8000000000000, 0x7FF4000000000000, 0x7FFFFFFFFFFFFFFF, 0x7FF0000000000001,
                           0xFFF8000000000000, 0xFFF4000000000000, 0xFFFFFFFFFFFFFFFF, 0xFFF0000000000001],
}
_UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def nan_values(dtype):
    """one NaN of every pattern of NAN_BITS, as dtype (built from bits: no arithmetic touches them)"""
    dt = np.dtype(dtype)
    return np.array(NAN_BITS[dt], dtype=_UINT[dt.itemsize]).view(dt)


# ---------------------------------------------------------------------------------------------------------------------------------
# key images and digits (sign flip for integers; the usual float flip, every NaN -> the all-ones key; 11-bit digits
# from the top)

def key_image(values):
    """uint64 array: the order-preserving unsigned image of every element, in the low 8 * itemsize bits"""
    a = np.ascontiguousarray(values)
    dt = a.dtype
    bits = dt.itemsize * 8
    u = a.view(_UINT[dt.itemsize]).astype(np.uint64)
    sign = np.uint64(1 << (bits - 1))
    ones = np.uint64((1 << bits) - 1)
    if dt.kind == "i":
        return u ^ sign
    negative = (u & sign) != 0
    k = np.where(negative, ~u & ones, u | sign)
    return np.where(np.isnan(a), ones, k)


def from_key_image(keys, dtype):
    """the inverse of key_image (the all-ones key of a float type gives the quiet NaN)"""
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    k = np.asarray(keys, dtype=np.uint64)
    sign = np.uint64(1 << (bits - 1))
    ones = np.uint64((1 << bits) - 1)
    if dt.kind == "i":
        return (k ^ sign).astype(_UINT[dt.itemsize]).view(dt)
    u = np.where((k & sign) != 0, k & ~sign & ones, ~k & ones)
    out = u.astype(_UINT[dt.itemsize]).view(dt).copy()
    out[k == ones] = np.nan
    return out


def digit_plan(bits):
    """[(shift, width)] of the digits, level 1 (the top) first: 11 bits each, the last one takes what is left"""
    plan, hi = [], bits
    while hi > 0:
        lo = max(hi - QT_DIGIT, 0)
        plan.append((lo, hi - lo))
        hi = lo
    return plan


def digits(keys, bits):
    """(n, levels) array of the digits of every key"""
    k = np.asarray(keys, dtype=np.uint64)
    return np.stack([(k >> np.uint64(s)) & np.uint64((1 << w) - 1) for s, w in digit_plan(bits)], axis=1).astype(np.int64)


def rank_of_q(n, q):
    """k of stats_reference.quantile_rule for q < 1 and n > 1"""
    k = int(np.floor(q * float(n)))
    return k - 1 if k > 0 else k


# ---------------------------------------------------------------------------------------------------------------------------------
# ranks k and k + 1 part at a chosen digit

def _digit_range(dt, level, width):
    """allowed values of the digit at `level`: a float's top digit stays clear of the exponents of inf and NaN on both signs"""
    if dt.kind == "f" and level == 1:
        return 8, (1 << width) - 9
    return 0, (1 << width) - 1


def _rand_bits(rng, width, size):
    if width == 0:
        return np.zeros(size, dtype=np.uint64)
    return rng.integers(0, 1 << width, size=size, dtype=np.uint64)


def parting_column(dtype, level, n, rng, decoys=True):
    """(values, q): a shuffled column of n elements whose sorted ranks k and k + 1 (k = the rule's rank for q) share every 11-bit
    digit above `level` and differ at `level` (levels count from the top).  Rank k is the largest key of its bucket; rank k + 1 is
    the smallest of at least three distinct keys of its bucket (at the last level a bucket IS one key: three copies of it); at
    least one empty bucket lies between the two.  For level >= 2 there are decoys: keys with rank k + 1's digit at `level`, another
    digit above it (one smaller, one larger) and smaller bits below it (at the last level there are no bits below).  At most half
    of the column shares rank k's top digit.  q = (k + 1.5) / n, so x = 0.5 and every exact method reads both ranks.
    decoys=False leaves the decoys out (the construction test shows that they are what catches a wrong mask)."""
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    plan = digit_plan(bits)
    assert 1 <= level <= len(plan)
    shift, width = plan[level - 1]
    last = level == len(plan)

    def key_of(ds, low=0):
        """digits ds for levels 1 .. len(ds), `low` in the bits below them"""
        k = 0
        for (s, _), d in zip(plan, ds):
            k |= int(d) << s
        return k | int(low)

    # the shared digits above `level`: never the smallest or largest allowed value, so that a neighbour exists on both sides
    P = []
    for j in range(1, level):
        lo, hi = _digit_range(dt, j, plan[j - 1][1])
        P.append(int(rng.integers(lo + 1, hi)))
    lo, hi = _digit_range(dt, level, width)
    gap = int(rng.integers(2, 4))                              # one or two empty buckets in between
    dA = int(rng.integers(lo + 1, hi - gap - 1))
    dB = dA + gap
    keys = []
    if last:
        keys += [key_of(P + [dA])] * 3 + [key_of(P + [dB])] * 3
        lowB = 0
    else:
        lowsA = rng.choice(1 << min(shift, 20), size=5, replace=False)
        lowsB = 2 + rng.choice((1 << min(shift, 20)) - 2, size=4, replace=False)
        keys += [key_of(P + [dA], l) for l in lowsA] + [key_of(P + [dB], l) for l in lowsB]
        lowB = int(lowsB.min())
    if decoys and level >= 2:
        variants = [P[:-1] + [P[-1] - 1], P[:-1] + [P[-1] + 1]]
        if level >= 3:
            variants.append([P[0] - 1] + P[1:])
        for i, Pd in enumerate(variants):
            keys.append(key_of(Pd + [dB], 0 if last else (lowB - 1 - i) % lowB))
    fill = max(n // 16, 1)
    # the parent bucket's other keys: every digit above `level` shared, the digit at `level` outside [dA, dB]
    outside = np.array([d for d in range(lo, hi + 1) if d < dA or d > dB])
    base = key_of(P)
    keys += list(np.uint64(base) | (rng.choice(outside, size=fill).astype(np.uint64) << np.uint64(shift)) | _rand_bits(rng, shift, fill))
    # keys that leave the shared prefix at digit j, 2 <= j < level
    for j in range(2, level):
        s, w = plan[j - 1]
        l, h = _digit_range(dt, j, w)
        other = np.array([d for d in range(l, h + 1) if d != P[j - 1]])
        keys += list(np.uint64(key_of(P[:j - 1])) | (rng.choice(other, size=fill).astype(np.uint64) << np.uint64(s)) | _rand_bits(rng, s, fill))
    # the rest: other top digits (level 1: outside [dA, dB])
    s, w = plan[0]
    l, h = _digit_range(dt, 1, w)
    if level == 1:
        other = outside
    else:
        other = np.array([d for d in range(l, h + 1) if d != P[0]])
    rest = n - len(keys)
    assert rest > n // 2
    keys += list((rng.choice(other, size=rest).astype(np.uint64) << np.uint64(s)) | _rand_bits(rng, s, rest))
    keys = np.array(keys, dtype=np.uint64)
    assert len(keys) == n
    srt = np.sort(keys)
    k = int(np.searchsorted(srt, np.uint64(key_of(P + [dA], (1 << shift) - 1)), side="right")) - 1
    values = from_key_image(rng.permutation(keys), dt)
    assert not (dt.kind == "f" and np.isnan(values).any())
    return values, (k + 1.5) / n


# ---------------------------------------------------------------------------------------------------------------------------------
# which region of the candidate buffer an element's key is appended to

def region_of_positions(n, itemsize, head=0):
    """region (0 .. 255) of every element position of a column whose first 16-byte aligned element is element `head`: 16-byte
    vector j -- counted from that element -- goes to region j % 256 (a thread's region is its index % 256 and the grid stride is
    a multiple of 256), loose head / tail element t to region t % 256"""
    V = 16 // itemsize
    head = min(head, n)
    nvec = (n - head) // V
    i = np.arange(n, dtype=np.int64)
    reg = ((i - head) // V) % QT_NSUB
    tail0 = head + nvec * V
    reg[:head] = i[:head] % QT_NSUB
    reg[tail0:] = (head + (i[tail0:] - tail0)) % QT_NSUB
    return reg


def region_size(n):
    """rs: keys per region"""
    return (min(n, QT_CAND_CAP) + QT_NSUB - 1) // QT_NSUB


def region_layout(dtype, n, per_region, regions, rng):
    """(values, q, top_digit): a column of n elements for a 16-byte aligned buffer.  The keys of ONE top-digit bucket, all distinct,
    occupy exactly per_region element positions (an int, or one count per region) in each of `regions`; every other position holds
    a key of another top-digit bucket.  Rank k of q falls into the middle of that bucket."""
    dt = np.dtype(dtype)
    bits = dt.itemsize * 8
    shift, width = digit_plan(bits)[0]
    lo, hi = _digit_range(dt, 1, width)
    counts = [per_region] * len(regions) if np.isscalar(per_region) else list(per_region)
    assert len(counts) == len(regions) and shift >= 21
    reg = region_of_positions(n, dt.itemsize)
    D = int(rng.integers(lo + 2, hi - 1))
    other = np.array([d for d in range(lo, hi + 1) if d != D], dtype=np.uint64)
    keys = (rng.choice(other, size=n) << np.uint64(shift)) | _rand_bits(rng, shift, n)
    total = int(sum(counts))
    # distinct low bits: distinct 21-bit numbers in the highest bits below the digit, random bits under them
    lows = rng.choice(1 << 21, size=total, replace=False).astype(np.uint64) << np.uint64(shift - 21)
    lows |= _rand_bits(rng, shift - 21, total)
    at = 0
    for r, c in zip(regions, counts):
        pos = np.flatnonzero(reg == r)
        assert c <= len(pos), (r, c, len(pos))
        pos = rng.choice(pos, size=c, replace=False)
        keys[pos] = (np.uint64(D) << np.uint64(shift)) | lows[at: at + c]
        at += c
    below = int(np.count_nonzero((keys >> np.uint64(shift)) < np.uint64(D)))
    k = below + total // 2
    values = from_key_image(keys, dt)
    assert not (dt.kind == "f" and np.isnan(values).any())
    return values, (k + 1.5) / n, D


# ---------------------------------------------------------------------------------------------------------------------------------
# a host model of the selection, to predict the route and to show what a test would see if a rule were broken

def select_model(keys, bits, k, one=False, allow_compact=True, region=None, overflow_branch=True, mb_mask=None):
    """Ranks k and k + 1 of `keys` by the digit-by-digit search of DESIGN §11, with the candidate buffer.  Returns a dict with
    key0, key1, column_passes, src, allow_compact -- or ok=False when a pass finds the rank outside every bucket (a search over an
    incomplete candidate buffer).  overflow_branch=False continues on the candidates although a region overflowed (the buffer then
    holds the first rs keys of each region).  mb_mask(hi_b, width) replaces the mask that selects rank k + 1's bucket."""
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    plan = digit_plan(bits)
    rs = region_size(n)
    if region is None:
        region = region_of_positions(n, bits // 8)

    def hi_mask(hi):
        return np.uint64(0) if hi >= 64 else np.uint64((~0 << hi) & 0xFFFFFFFFFFFFFFFF)

    prefix, rank, done = np.uint64(0), k, False
    y1_state, y1 = ("unwanted" if one else "follows"), None
    prefix_b, hi_b, width_b = np.uint64(0), 64, 0
    src, compact, column_passes, cand = 0, False, 0, None
    level = 0
    for _ in plan:
        want_b = y1_state == "min_of_b"
        if done and not want_b:
            break
        shift, width = plan[level]
        pool = keys if src == 0 else cand
        ma = hi_mask(shift + width)
        overflow, new_cand = False, None
        if not done:
            sel = (pool & ma) == (prefix & ma)
            match = pool[sel]
            hist = np.bincount(((match >> np.uint64(shift)) & np.uint64((1 << width) - 1)).astype(np.int64), minlength=1 << width)
            if compact and src == 0:
                r = region[sel]
                order = np.argsort(r, kind="stable")
                rsorted = r[order]
                start = np.searchsorted(rsorted, np.arange(QT_NSUB))
                within = np.arange(len(rsorted)) - start[rsorted]
                overflow = bool((within >= rs).any())
                new_cand = match[order][within < rs]
        if want_b:
            mb = hi_mask(hi_b) if mb_mask is None else np.uint64(mb_mask(hi_b, width_b))
            inb = pool[(pool & mb) == (prefix_b & mb)]
            y1 = int(inb.min()) if len(inb) else (1 << 64) - 1
            y1_state = "known"
        if not done:
            cum = np.cumsum(hist)
            if len(match) == 0 or rank >= cum[-1]:
                return dict(ok=False, column_passes=column_passes, src=src, allow_compact=int(allow_compact))
            b = int(np.searchsorted(cum, rank, side="right"))
            r_in = rank - (int(cum[b - 1]) if b else 0)
            cnt = int(hist[b])
            later = np.flatnonzero(hist[b + 1:])
            prefix = (prefix & ma) | np.uint64(b << shift)
            if y1_state == "follows" and r_in + 1 >= cnt and len(later):
                pb = (prefix & ma) | np.uint64((b + 1 + int(later[0])) << shift)
                if shift == 0:
                    y1, y1_state = int(pb), "known"
                else:
                    prefix_b, hi_b, width_b, y1_state = pb, shift, width, "min_of_b"
            was_compacting = compact and src == 0
            rank = r_in
            if match.min() == match.max():
                prefix, done = match.min(), True
            elif shift == 0:
                done = True
            else:
                level += 1
            if done and y1_state == "follows":
                y1, y1_state = int(prefix), "known"
            if src == 0:
                column_passes += 1
            if was_compacting:
                compact = False
                if overflow and overflow_branch:
                    allow_compact = False
                else:
                    src, cand = 1, new_cand
            elif src == 0 and allow_compact and cnt * 2 <= QT_NSUB * rs:
                compact = True
    ok = done and (one or y1_state == "known")
    return dict(ok=ok, key0=int(prefix), key1=int(prefix) if one else y1, column_passes=column_passes, src=src,
                allow_compact=int(allow_compact))


# ---------------------------------------------------------------------------------------------------------------------------------
# the note channel (libgdf_testhook.so): which route the last radix selection took

NOTE_NAMES = ("qt.column_passes", "qt.src", "qt.allow_compact")


def clear_notes(gdf):
    assert gdf.libgdf.gdf_amd_debug_noted(None, None) == 0


def read_notes(gdf):
    """{name: value} of the selection's notes; a missing note is an assertion (the call did not come through the radix selection)"""
    out = {}
    for name in NOTE_NAMES:
        v = C.c_longlong(-1)
        rc = gdf.libgdf.gdf_amd_debug_noted(name.encode(), C.byref(v))
        assert rc == 0, (name, rc)
        out[name] = int(v.value)
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# slices of a guarded device buffer

class GuardedSlice:
    """elements [off, off + n) of `whole`, uploaded between guard bytes (elementwise_common.Buf): .col is a Column over the slice,
    whose address is off elements past a 16-byte boundary; .read() returns the whole allocation's elements after checking that
    every guard byte is intact."""

    def __init__(self, whole, off, n):
        import torch
        from libgdf_amd.columns import Column
        whole = np.ascontiguousarray(whole)
        assert off + n <= len(whole)
        self.buf = Buf(len(whole), whole.dtype, 0, whole)
        self.off, self.n = off, n
        tdt = getattr(torch, whole.dtype.name)
        self.typed = self.buf.t[self.buf.start: self.buf.start + self.buf.nbytes].view(tdt)
        self.col = Column(self.typed[off: off + n])
        assert self.col.c.data == self.buf.ptr + off * whole.dtype.itemsize

    def read(self):
        return self.buf.read()


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(_UINT[a.dtype.itemsize])


def zeros_unsigned(a):
    """a float array with every -0.0 replaced by +0.0 (the in-place sort's image does not tell them apart)"""
    a = a.copy()
    a[a == 0] = 0.0
    return a
