"""numpy restatement of the contracts of gdf_amd_order_by_ex and gdf_amd_gather (include/gdf/gdf_amd_ext.h, csrc/order.hip).  The
reference project has neither function; nothing here is derived from it.

A key column is (data, valid): data a numpy array of a key dtype, valid a bool array or None (no mask = no nulls).

order_by_ex    the contract, as a stable np.lexsort over per-column (null rank, value image): the value image is the order-preserving
               unsigned image of the element in its own width (integers: sign bit flipped; floats: IEEE total order with -0.0 folded
               onto +0.0 and every NaN onto the all-ones image, i.e. behind +inf), complemented within that width under DESC and zero
               under a null; the null rank puts the nulls of a column behind (or, NULLS_FIRST, in front of) all its values whatever
               the direction.
model_order    the same order computed the way the kernel does it -- ONE packed image per row, per column [null bit][value field of
               bit_length(max - min) bits, ranges over valid rows only] -- in Python integers of any width, with the mutations a wrong
               implementation would make (MUTATIONS).  tests/test_order_reference.py shows that each mutation changes the permutation
               of some case written out by hand there, so the GPU comparison against order_by_ex can tell them apart.
gather         outs[c][i] = cols[c][indices[i]], null (data 0) where indices[i] == -1 or the source row is null.
"""
import numpy as np

DESC, NULLS_FIRST = 1, 2

MUTATIONS = ["desc_is_reversed_ascending", "desc_flips_null_placement", "data_under_nulls_compared", "nan_is_null", "negative_zero_first",
             "null_bit_below_value", "desc_complements_whole_word"]


def float_image(a, fold=True):
    """(order-preserving unsigned image as uint64, width in bits) of a float array"""
    u = a.view(np.uint32 if a.dtype == np.float32 else np.uint64).astype(np.uint64)
    w = a.dtype.itemsize * 8
    sign, full = np.uint64(1 << (w - 1)), np.uint64((1 << w) - 1)
    if fold:
        u = np.where(u == sign, np.uint64(0), u)                     # -0.0 == +0.0
    img = np.where(u & sign != 0, ~u & full, u | sign)
    return np.where(np.isnan(a), full, img), w                       # every NaN: one value behind +inf


def value_image(a, fold=True):
    """(image, width): ascending order of the elements == ascending order of the unsigned images"""
    if a.dtype.kind == "f":
        return float_image(a, fold)
    w = a.dtype.itemsize * 8
    return (a.astype(np.int64).view(np.uint64) + np.uint64(1 << (w - 1))) & np.uint64((1 << w) - 1 if w < 64 else ~np.uint64(0)), w


def _flags(value, n):
    if value is None:
        return [False] * n
    if isinstance(value, (bool, np.bool_)):
        return [bool(value)] * n
    assert len(value) == n
    return [bool(v) for v in value]


def order_by_ex(cols, descending=None, nulls_first=None):
    """the stable permutation (int32) gdf_amd_order_by_ex owes"""
    n = len(cols[0][0])
    desc, first = _flags(descending, len(cols)), _flags(nulls_first, len(cols))
    seq = []                                                          # most significant first
    for (data, valid), d, f in zip(cols, desc, first):
        null = np.zeros(n, dtype=bool) if valid is None else ~np.asarray(valid, dtype=bool)
        img, w = value_image(np.asarray(data))
        if d:
            img = np.uint64((1 << w) - 1 if w < 64 else 0xFFFFFFFFFFFFFFFF) - img
        seq += [null != f, np.where(null, np.uint64(0), img)]
    return np.lexsort(tuple(reversed(seq))).astype(np.int32)


def model_order(cols, descending=None, nulls_first=None, mutation=None):
    """the permutation from ONE packed image per row (Python integers), optionally with one of MUTATIONS"""
    assert mutation is None or mutation in MUTATIONS
    n = len(cols[0][0])
    desc, first = _flags(descending, len(cols)), _flags(nulls_first, len(cols))
    image = [0] * n
    total = 0
    whole_word_complements = 0
    for (data, valid), d, f in zip(cols, desc, first):
        data = np.asarray(data)
        null = np.zeros(n, dtype=bool) if valid is None else ~np.asarray(valid, dtype=bool)
        if mutation == "nan_is_null" and data.dtype.kind == "f":
            null = null | np.isnan(data)
            valid = ~null
        img, w = value_image(data, fold=mutation != "negative_zero_first")
        img = [int(x) for x in img]
        if data.dtype.kind != "f":                                    # (v - min) in bit_length(max - min) bits, valid rows only
            seen = [x for x, nl in zip(img, null) if not nl or mutation == "data_under_nulls_compared"]
            lo, hi = (min(seen), max(seen)) if seen else (0, 0)
            w = max((hi - lo).bit_length(), 1)
            img = [x - lo for x in img]
        full = (1 << w) - 1
        field_desc = d and mutation not in ("desc_is_reversed_ascending", "desc_complements_whole_word")
        if d and mutation == "desc_complements_whole_word":
            whole_word_complements += 1
        place_first = f != (d and mutation == "desc_flips_null_placement")
        has_mask = valid is not None
        for i in range(n):
            v = img[i] & full if (not null[i] or mutation == "data_under_nulls_compared") else None
            if v is None:
                v = 0
            elif field_desc:
                v = full - v
            bit = int(bool(null[i]) != place_first)
            if not has_mask:
                unit, uw = v, w
            elif mutation == "null_bit_below_value":
                unit, uw = (v << 1) | bit, w + 1
            else:
                unit, uw = (bit << w) | v, w + 1
            image[i] = (image[i] << uw) | unit
        total += w + (1 if has_mask else 0)
    if whole_word_complements % 2:
        image = [((1 << total) - 1) - x for x in image]
    perm = sorted(range(n), key=lambda i: image[i])                   # (sorted is stable)
    if mutation == "desc_is_reversed_ascending" and desc[0]:
        perm = perm[::-1]
    return np.asarray(perm, dtype=np.int32)


def mask_words(ok):
    """the output mask of gather: ceil(m / 64) * 8 bytes, LSB first, bits beyond m zero"""
    ok = np.asarray(ok, dtype=bool)
    out = np.zeros((len(ok) + 63) // 64 * 8, dtype=np.uint8)
    packed = np.packbits(ok, bitorder="little")
    out[:len(packed)] = packed
    return out


def gather(indices, cols):
    """-> [(data, ok bools, mask bytes, null_count)] per source column (data, valid)"""
    idx = np.asarray(indices).astype(np.int64)
    res = []
    for data, valid in cols:
        data = np.asarray(data)
        rows = len(data)
        assert ((idx >= -1) & (idx < rows)).all()
        safe = np.where(idx >= 0, idx, 0)
        if rows == 0:
            ok = np.zeros(len(idx), dtype=bool)
            out = np.zeros(len(idx), dtype=data.dtype)
        else:
            ok = (idx >= 0) & (np.ones(rows, dtype=bool) if valid is None else np.asarray(valid, dtype=bool))[safe]
            out = np.where(ok, data[safe], data.dtype.type(0))
        res.append((out, ok, mask_words(ok), int(len(idx) - ok.sum())))
    return res


def bits_of(a):
    """the storage bits of an array (NaN payloads and the sign of zero compare exactly)"""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ---- GPU-side helpers ------------------------------------------------------------------------------------------------------------------
def device_mask(valid):
    """the packed mask at byte offset 1 of a 0xFF-filled device buffer, with the bits beyond len(valid) set: a mask needs no alignment
    and its tail is ignored"""
    import torch
    rows = len(valid)
    packed = np.packbits(np.asarray(valid, dtype=bool), bitorder="little")
    if rows % 8:
        packed[-1] |= (0xFF << (rows % 8)) & 0xFF
    buf = np.full(len(packed) + 16, 0xFF, dtype=np.uint8)
    buf[1:1 + len(packed)] = packed
    t = torch.from_numpy(buf).cuda()[1:]
    assert t.data_ptr() % 2 == 1
    return t


def device_column(data, valid=None, dtype=None, time_unit=None):
    """a libgdf_amd Column over an upload of (data, valid bools or None)"""
    import torch
    from libgdf_amd.columns import Column
    return Column(torch.from_numpy(np.ascontiguousarray(data)).cuda(), None if valid is None else device_mask(valid), dtype, time_unit=time_unit)
