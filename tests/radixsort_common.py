"""Helpers shared by the radix sort ABI tests (test_gpu_radixsort*, test_radixsort_reference): the ctypes prototypes of
gdf_radixsort_* / gdf_segmented_radixsort_*, a numpy reference written from the documented contract (not from the kernels),
and seeded key generators.

The contract (csrc/sort.hip above RadixPlan): rows are ordered, stably, by bits [begin_bit, end_bit) of the key's
order-preserving IMAGE; both bounds are clamped to the key's width and an empty range leaves both columns as they are.  Everything
is bit-exact: key outputs are compared as raw bits (bits_of), the int64 value column 0..n-1 exactly."""
import ctypes as C

import numpy as np

UNSIGNED = {1: np.uint8, 4: np.uint32, 8: np.uint64}
DTYPES = [np.int8, np.int32, np.int64, np.float32, np.float64]
SUFFIX = {np.dtype(np.int8): "i8", np.dtype(np.int32): "i32", np.dtype(np.int64): "i64", np.dtype(np.float32): "f32",
          np.dtype(np.float64): "f64"}


def api():
    from libgdf_amd._binding import _gdf_cdll as lib
    lib.gdf_radixsort_plan.restype = C.c_void_p
    lib.gdf_radixsort_plan.argtypes = [C.c_size_t, C.c_int, C.c_uint, C.c_uint]
    lib.gdf_segmented_radixsort_plan.restype = C.c_void_p
    lib.gdf_segmented_radixsort_plan.argtypes = [C.c_size_t, C.c_int, C.c_uint, C.c_uint]
    for n in ("gdf_radixsort_plan_setup", "gdf_segmented_radixsort_plan_setup"):
        getattr(lib, n).argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
    for n in ("gdf_radixsort_plan_free", "gdf_segmented_radixsort_plan_free"):
        getattr(lib, n).argtypes = [C.c_void_p]
    for s in ("generic",) + tuple(SUFFIX.values()):
        getattr(lib, "gdf_radixsort_" + s).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(lib, "gdf_segmented_radixsort_" + s).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p]
    return lib


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(UNSIGNED[a.dtype.itemsize])


def width(dtype):
    return np.dtype(dtype).itemsize * 8


def image(key, descending):
    """The order-preserving unsigned image of `key`, in the key's width.  Integers: two's complement with the sign bit flipped.
    Floats: -0.0 counts as +0.0, any NaN is all ones (after +inf), otherwise negatives have all bits flipped and non-negatives the
    sign bit set.  Descending: the complement within the width."""
    key = np.ascontiguousarray(key)
    U = UNSIGNED[key.dtype.itemsize]
    bits = key.view(U)
    top = U(1 << (width(key.dtype) - 1))
    if np.issubdtype(key.dtype, np.integer):
        img = bits ^ top
    else:
        bits = np.where(key == 0, U(0), bits)                    # -0.0 == 0 is true: both zeros become +0.0
        img = np.where(np.signbit(key) & (key != 0), ~bits, bits | top)
        img = np.where(np.isnan(key), U(~U(0)), img)
    img = img.astype(U)
    return ~img if descending else img


def expected(key, descending, begin_bit, end_bit, segments=None):
    """(sorted key, sorted value column 0..n-1) of a stable sort on bits [begin_bit, end_bit) of image(key); `segments` (a list of
    (begin, end) row ranges, disjoint) restricts the sort to those rows, every other row stays where it is."""
    key = np.ascontiguousarray(key)
    n, w = len(key), width(key.dtype)
    U = UNSIGNED[key.dtype.itemsize]
    b0, b1 = min(int(begin_bit), w), min(int(end_bit), w)
    perm = np.arange(n, dtype=np.int64)
    if b1 > b0 and n:
        digit = (image(key, descending) >> U(b0)) & U((1 << (b1 - b0)) - 1)
        for s, e in ([(0, n)] if segments is None else segments):
            s, e = int(s), int(e)
            if e > s:
                perm[s:e] = s + np.argsort(digit[s:e], kind="stable")
    return key[perm], perm


# ---------------------------------------------------------------------------
# key generators (rng: a seeded np.random.default_rng)
# ---------------------------------------------------------------------------
def full_range_ints(rng, dtype, n):
    """Every bit of the width varies, the sign bit included (util.gen_rand stays within +-10000)."""
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=n, dtype=dtype, endpoint=True)


def float_bit_patterns(rng, dtype, n):
    """Floats from uniformly random BITS: NaNs of both signs with payloads (one float32 in 256, one float64 in 2048), denormals,
    and exponents over the whole range."""
    dtype = np.dtype(dtype)
    return rng.integers(0, 256, size=n * dtype.itemsize, dtype=np.uint8).view(dtype)


def full_range_keys(rng, dtype, n):
    return full_range_ints(rng, dtype, n) if np.issubdtype(np.dtype(dtype), np.integer) else float_bit_patterns(rng, dtype, n)


SPECIAL_BITS = {
    # +0.0, -0.0, +inf, -inf, +NaN, -NaN, a NaN with a payload, the smallest denormal, the largest finite value, +1, -1
    np.dtype(np.float32): [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fc12345, 0x00000001,
                           0x7f7fffff, 0x3f800000, 0xbf800000],
    np.dtype(np.float64): [0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000, 0x7ff8000000000000,
                           0xfff8000000000000, 0x7ff8000012345678, 0x0000000000000001, 0x7fefffffffffffff, 0x3ff0000000000000,
                           0xbff0000000000000],
}


def special_values(dtype):
    dtype = np.dtype(dtype)
    return np.array(SPECIAL_BITS[dtype], dtype=UNSIGNED[dtype.itemsize]).view(dtype)


def float_specials(rng, dtype, n):
    """The eleven special values tiled to length n and shuffled (n = 11: each of them once)."""
    sp = special_values(dtype)
    return bits_of(np.resize(sp, n))[rng.permutation(n)].view(sp.dtype)


def low_cardinality(rng, dtype, n):
    """Only 3 distinct values: the order inside each run of equal keys is what the test checks."""
    dtype = np.dtype(dtype)
    if np.issubdtype(dtype, np.integer):
        vals = np.array([np.iinfo(dtype).min + 5, -1, np.iinfo(dtype).max - 3], dtype=dtype)
    else:
        vals = np.array([-2.5, 0.75, 3e10], dtype=dtype)
    return vals[rng.integers(0, 3, size=n)]


# ---------------------------------------------------------------------------
# one call of the library
# ---------------------------------------------------------------------------
def run_sort(key, descending, begin_bit, end_bit, segments=None, entry="generic"):
    """Sorts a copy of `key` with the value column 0..n-1 through gdf_radixsort_<entry> (segments None) or
    gdf_segmented_radixsort_<entry>; returns the two columns as numpy arrays.  An empty column has a null data pointer."""
    import torch
    from libgdf_amd.columns import column_from_numpy
    lib = api()
    n, isz = len(key), key.dtype.itemsize
    ck, cv = column_from_numpy(key), column_from_numpy(np.arange(n, dtype=np.int64))
    seg = "" if segments is None else "segmented_"
    plan = getattr(lib, f"gdf_{seg}radixsort_plan")(n, int(descending), begin_bit, end_bit)
    assert plan
    assert getattr(lib, f"gdf_{seg}radixsort_plan_setup")(plan, isz, 8) == 0
    if segments is None:
        err = getattr(lib, "gdf_radixsort_" + entry)(plan, C.addressof(ck.c), C.addressof(cv.c))
    else:
        sb = np.array([s for s, _ in segments], dtype=np.uint32)
        se = np.array([e for _, e in segments], dtype=np.uint32)
        db, de = torch.from_numpy(sb.view(np.int32)).cuda(), torch.from_numpy(se.view(np.int32)).cuda()
        err = getattr(lib, "gdf_segmented_radixsort_" + entry)(plan, C.addressof(ck.c), C.addressof(cv.c), len(segments),
                                                               db.data_ptr() if len(segments) else None,
                                                               de.data_ptr() if len(segments) else None)
    assert err == 0, err
    assert getattr(lib, f"gdf_{seg}radixsort_plan_free")(plan) == 0
    return ck.to_numpy(), cv.to_numpy()


def check_sort(key, descending, begin_bit, end_bit, segments=None, entry="generic"):
    """run_sort against expected(): keys as raw bits (-0.0 and NaN payloads come through unchanged and in stable order), values exactly."""
    got_k, got_v = run_sort(key, descending, begin_bit, end_bit, segments, entry)
    exp_k, exp_v = expected(key, descending, begin_bit, end_bit, segments)
    what = f"{key.dtype} n={len(key)} desc={descending} bits=[{begin_bit},{end_bit})"
    np.testing.assert_array_equal(got_v, exp_v, err_msg="values, " + what)
    np.testing.assert_array_equal(bits_of(got_k), bits_of(exp_k), err_msg="keys, " + what)
    return got_k, got_v
