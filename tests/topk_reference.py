"""A Python-integer model of gdf_amd_top_k's selection route (csrc/topk.hip), next to the statement of its contract.

top_k          the contract: order_reference.order_by_ex(cols, desc, first)[offset:offset + k].  numpy, not the code under test.
model_top_k    the same rows computed the way the kernels do it:
                 leading_image  L(row), 64 bits, most significant first, per column [null bit, only with a mask][value image in the
                                element's own width, complemented within it under DESC, 0 under a null]; the field that straddles bit
                                64 gives its high bits, later fields are dropped; complete = every field fits whole
                 select         T = the K-th smallest L (K = offset + k) digit by digit, 11 bits at a time, among the images that
                                match the decided prefix, with c_less = #{L < T}; all matching images equal ends the search, and so
                                does a bucket of at most `slack` images (SLACK in the library): T then stays undecided below that
                                digit and "L < T", "L == T" compare the decided bits only
                 candidates     the rows with L < T in row order, then the rows with L == T in row order -- a complete image and an
                                exact T: only the first K - c_less of them; otherwise all
                 finish         the candidates' rows sorted by the full key (stable), element offset + i of that is output i
               with the mutations a wrong kernel would make (MUTATIONS).  tests/test_topk_reference.py shows that each changes the
               result of a case written out by hand there; tests/test_gpu_topk.py says which GPU case would catch which.
"""
import numpy as np

import order_reference as orf

MUTATIONS = ["ties_cut_by_value_not_row", "tie_block_not_in_row_order", "truncated_image_treated_as_complete",
             "straddling_field_low_bits_kept", "desc_complements_beyond_field", "null_bit_below_value", "data_under_null_compared",
             "offset_applied_before_selection", "k_th_is_k_plus_one"]
DIGIT = 11
SLACK = 1 << 15                              # TK_SLACK of csrc/topk.hip
FULL = (1 << 64) - 1


def top_k(cols, k, offset=0, descending=None, nulls_first=None):
    """the rows gdf_amd_top_k owes (int32)"""
    return orf.order_by_ex(cols, descending, nulls_first)[offset:offset + k]


def leading_image(cols, descending=None, nulls_first=None, mutation=None):
    """-> ([L(row) as Python integers], complete, low): low = the number of unused bits at the bottom of L"""
    n = len(cols[0][0])
    desc, first = orf._flags(descending, len(cols)), orf._flags(nulls_first, len(cols))
    image = [0] * n
    pos, complete = 64, True
    for (data, valid), d, f in zip(cols, desc, first):
        if pos == 0:
            complete = False
            break
        data = np.asarray(data)
        null = np.zeros(n, dtype=bool) if valid is None else ~np.asarray(valid, dtype=bool)
        img, w = orf.value_image(data)
        img = [int(x) for x in img]
        wmask = (1 << w) - 1
        nshift = None
        if valid is not None and mutation != "null_bit_below_value":
            pos -= 1
            nshift = pos
        keep = min(w, pos)
        if keep < w:
            complete = False
        drop = w - keep
        pos -= keep
        vshift = pos
        if valid is not None and mutation == "null_bit_below_value":
            if pos > 0:
                pos -= 1
                nshift = pos
            else:
                complete = False
        for i in range(n):
            k = 0
            if nshift is not None:
                k |= int(bool(null[i]) != f) << nshift
            if keep and (not null[i] or mutation == "data_under_null_compared"):
                v = img[i]
                if d:
                    v = (FULL - v) if mutation == "desc_complements_beyond_field" else (wmask - v)
                if mutation == "straddling_field_low_bits_kept":
                    v &= (1 << keep) - 1
                else:
                    v >>= drop
                k |= (v << vshift) & FULL
            image[i] |= k
    return image, complete, pos


def select(image, K, low, slack=0):
    """(T, c_less, ties, column passes, tshift): T = the K-th smallest image (K >= 1) on its bits >= tshift, c_less / ties = the images
    below / equal to it on those bits; tshift == 0: T is exact.  The control flow of tk_select."""
    prefix, rank, count, c_less = 0, K - 1, len(image), 0
    shift = max(64 - DIGIT, low)
    dbits = 64 - shift
    passes = 0
    while True:
        hi = shift + dbits
        ma = (FULL >> hi << hi) if hi < 64 else 0
        match = [x for x in image if (x & ma) == (prefix & ma)]
        assert len(match) == count and 0 <= rank < count
        passes += 1
        if min(match) == max(match):
            return match[0], c_less, count, passes, 0
        hist = [0] * (1 << dbits)
        for x in match:
            hist[(x >> shift) & ((1 << dbits) - 1)] += 1
        before = 0
        for b, c in enumerate(hist):
            if rank < before + c:
                break
            before += c
        prefix = (prefix & ma) | (b << shift)
        c_less, rank, count = c_less + before, rank - before, hist[b]
        if shift <= low:
            return prefix, c_less, count, passes, 0
        if count <= slack:
            return prefix, c_less, count, passes, shift
        ns = max(shift - DIGIT, low)
        shift, dbits = ns, shift - ns


def _take(cols, rows):
    rows = np.asarray(rows, dtype=np.int64)
    return [(np.asarray(d)[rows], None if v is None else np.asarray(v, dtype=bool)[rows]) for d, v in cols]


def model_top_k(cols, k, offset=0, descending=None, nulls_first=None, mutation=None, info=None, slack=0):
    """the selection route in Python integers, optionally with one of MUTATIONS; 0 < offset + k <= rows.  A row the mutated route
    cannot deliver comes back as -1.  info (a dict) receives complete, exact, candidates, c_less, ties and passes.  slack = 0: the
    select runs until T is exact (the mutations are stated for that)."""
    assert mutation is None or mutation in MUTATIONS
    n = len(cols[0][0])
    m = max(0, min(k, n - offset))
    K = offset + m
    assert 0 < K <= n
    image, complete, low = leading_image(cols, descending, nulls_first, mutation)
    if mutation == "truncated_image_treated_as_complete":
        complete = True
    target = m if mutation == "offset_applied_before_selection" else K
    if mutation == "k_th_is_k_plus_one" and target < n:
        # the (K + 1)-th smallest taken as an exclusive bound: "the rows strictly below it are the K smallest" -- not with ties at the cut
        T, _, _, passes, tshift = select(image, target + 1, low, slack)
        less = [i for i in range(n) if image[i] >> tshift < T >> tshift]
        equal = []
        c_less = len(less)
    else:
        T, c_less, ties, passes, tshift = select(image, target, low, slack)
        less = [i for i in range(n) if image[i] >> tshift < T >> tshift]
        equal = [i for i in range(n) if image[i] >> tshift == T >> tshift]
        assert len(less) == c_less and len(equal) == ties and c_less < target <= c_less + ties
        if mutation == "ties_cut_by_value_not_row":                   # the cut among the ties by the raw element, not the row number
            raw = orf.bits_of(np.asarray(cols[-1][0]))
            equal = sorted(equal, key=lambda i: int(raw[i]))
        if complete and tshift == 0:
            equal = equal[:target - c_less]
        if mutation == "tie_block_not_in_row_order":
            equal = equal[::-1]
    cand = less + equal
    if info is not None:
        info.update(complete=complete, exact=tshift == 0, candidates=len(cand), c_less=c_less, ties=len(equal), passes=passes)
    perm = orf.order_by_ex(_take(cols, cand), descending, nulls_first) if cand else np.zeros(0, dtype=np.int32)
    out = [cand[perm[offset + i]] if offset + i < len(cand) else -1 for i in range(m)]
    return np.asarray(out, dtype=np.int32)


def tied_floats(npt, rows, rng, masked):
    """a float column that is mostly +0.0 / -0.0 and NaNs of two payloads in shuffled row order, with a few other values: rows that
    tie on the image but differ in their raw bits.  -> ((data, valid or None), cuts): cuts(desc, first) gives the (k, offset) pairs
    whose K = offset + k falls inside the run of zeros and inside the run of NaNs"""
    if np.dtype(npt) == np.float32:
        nan_a, nan_b = np.array([0x7FC00000, 0xFFC00001], dtype=np.uint32).view(np.float32)
    else:
        nan_a, nan_b = np.array([0x7FF8000000000000, 0xFFF8000000000001], dtype=np.uint64).view(np.float64)
    pool = np.array([0.0, -0.0, nan_a, nan_b, -1.0, 1.0], dtype=npt)
    data = pool[rng.choice(6, size=rows, p=[0.22, 0.22, 0.22, 0.22, 0.06, 0.06])]
    valid = (rng.random(rows) < 0.85) if masked else None

    def cuts(desc, first):
        perm = orf.order_by_ex([(data, valid)], [desc], [first])
        ok = np.ones(rows, dtype=bool) if valid is None else valid[perm]
        along = data[perm]
        out = []
        for run in (ok & (along == 0), ok & np.isnan(along)):
            at = np.flatnonzero(run)
            K = int(at[0] + len(at) // 2)                       # rows K - 1 and K both lie in the run
            assert run[K - 1] and run[K]
            out += [(K, 0), (7, K - 7), (K - int(at[0]), int(at[0]))]
        return out

    return (data, valid), cuts
