"""-m gpu: gpu_comparison / gpu_comparison_static_* (csrc/filter.hip) on edge VALUES, at the edges of the 16-byte-vector kernel, and the
three branches of comparison_mask().  Every expectation is oracle.comparison (pinned by hand in test_oracle_pinning.py) or a plain numpy
expression on the validity vectors; every assertion is exact."""
import functools

import numpy as np
import pytest

from filter_common import device_slice, garbage_mask, unaligned_offset
from oracle import oracle
from util import ALL_DTYPES, INT_DTYPES

pytestmark = pytest.mark.gpu

OPS = range(6)                   # GDF_EQUALS, _NOT_EQUALS, _LESS_THAN, _LESS_THAN_OR_EQUALS, _GREATER_THAN, _GREATER_THAN_OR_EQUALS
SUFFIX = {np.dtype(np.int8): "i8", np.dtype(np.int16): "i16", np.dtype(np.int32): "i32", np.dtype(np.int64): "i64",
          np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}
_ids = dict(ids=lambda d: np.dtype(d).name)


# ---- the value tables -------------------------------------------------------------------------------------------------------------
def int_table(dtype):
    """min, min + 1, -1, 0, 1, max - 1, max; from 32 bits on the integers around float32's 2^24, for int64 those around float64's 2^53
    and one that float64 cannot hold either."""
    dtype = np.dtype(dtype)
    i = np.iinfo(dtype)
    v = [i.min, i.min + 1, -1, 0, 1, i.max - 1, i.max]
    if dtype.itemsize >= 4:
        v += [2**24, 2**24 + 1, -(2**24 + 1)]
    if dtype.itemsize == 8:
        v += [2**53, 2**53 + 1, 2**62 + 1]
    return np.array(v, dtype=dtype)


@functools.lru_cache(maxsize=None)
def table(dtype):
    """The edge values of one dtype (read-only, shared).  Floats: NaN, +-inf, +-0.0, the smallest subnormal, the largest finite,
    +-2^24, +-2^53 (float64) and the float nearest every integer edge value of every integer dtype; distinct BIT patterns are kept, so
    0.0 and -0.0 both stay."""
    dtype = np.dtype(dtype)
    if dtype.kind == "i":
        t = int_table(dtype)
    else:
        f = np.finfo(dtype)
        v = [np.nan, np.inf, -np.inf, 0.0, -0.0, np.nextafter(dtype.type(0), dtype.type(1)), f.max, 2.0**24, -(2.0**24)]
        if dtype.itemsize == 8:
            v += [2.0**53, -(2.0**53)]
        t = np.concatenate([np.array(v, dtype=dtype)] + [int_table(i).astype(dtype) for i in INT_DTYPES])
        u = np.dtype(f"u{dtype.itemsize}")
        t = np.unique(t.view(u)).view(dtype)
    t.setflags(write=False)
    return t


def _col(a, v=None):
    from libgdf_amd.columns import column_from_numpy
    return column_from_numpy(np.array(a), v)           # (a copy: the shared tables are read-only)


@pytest.mark.parametrize("ldt", ALL_DTYPES, **_ids)
@pytest.mark.parametrize("rdt", ALL_DTYPES, **_ids)
def test_edge_values_all_against_all(gdf, ldt, rdt):
    """Every edge value of the left dtype against every edge value of the right one (the cross product as two columns), six operators:
    NaN (only != holds), -0.0 == 0.0, the subnormal against zero, the extremes of one width against those of another (sign extension),
    and the integers that the common float type cannot hold -- C compares (int, float32) in float32 and converts int64 to nearest-even,
    where numpy alone would pick float64."""
    lt, rt = table(ldt), table(rdt)
    l, r = np.repeat(lt, len(rt)), np.tile(rt, len(lt))
    cl, cr = _col(l), _col(r)
    for op in OPS:
        out = gdf.api.comparison(cl, cr, op)
        np.testing.assert_array_equal(out.to_numpy(), oracle.comparison(l, r, op), err_msg=f"op {op}")
        assert out.valid_bits().all() and out.c.null_count == 0


@pytest.mark.parametrize("cdt", ALL_DTYPES, **_ids)
@pytest.mark.parametrize("sdt", ALL_DTYPES, **_ids)
def test_edge_values_against_a_scalar(gdf, cdt, sdt):
    """gpu_comparison_static_<sdt>: the column holds every edge value of its dtype, the scalar walks the whole table of ITS dtype (NaN,
    -0.0 and the integer extremes among them)."""
    l = table(cdt)
    cl = _col(l)
    for s in table(sdt):
        for op in OPS:
            out = gdf.api.comparison(cl, s, op)
            np.testing.assert_array_equal(out.to_numpy(), oracle.comparison(l, s, op), err_msg=f"scalar {s!r} op {op}")


# ---- the vector kernel's edges ------------------------------------------------------------------------------------------------------
def vector_sizes(width):
    """launch_compare takes compare_vec_kernel when all pointers are 16-byte aligned and n / EPV >= 1024 (EPV = 16 / width), the
    element-wise kernel for the n % EPV rows after it and for everything else.  Just below and at the threshold; tails of 1 and of
    EPV - 1 rows; 1025, 2047 and 4096 vectors, none a multiple of the 1024-vector tile except the last (the loads of the last
    tile's missing vectors are clamped to nvec - 1)."""
    e = 16 // width
    return [1024 * e - 1, 1024 * e, 1024 * e + 1, 1024 * e + e - 1, 2047 * e + 1, 4096 * e + 3]


def _small_values(rng, dtype, n):
    return rng.integers(-3, 4, size=n).astype(dtype)             # (integer-valued floats: every operator has both outcomes)


def _run_into_slice(gdf, call, n, out_off, expected, tag):
    """Run `call(out_column)` with an int8 output that starts out_off bytes into an allocation filled with 0x55; the bytes on either side
    of the n results must still be 0x55 afterwards."""
    import torch
    from libgdf_amd.columns import Column
    buf = torch.full((out_off + n + 32,), 0x55, dtype=torch.int8, device="cuda")
    valid = torch.zeros(((n + 7) // 8 + 63) // 64 * 64, dtype=torch.uint8, device="cuda")
    out = Column(buf[out_off:out_off + n], valid, 1)
    assert (out.data.data_ptr() % 16 != 0) == (out_off != 0)
    call(out)
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[out_off:out_off + n], expected, err_msg=str(tag))
    assert (got[:out_off] == 0x55).all() and (got[out_off + n:] == 0x55).all(), tag
    assert out.valid_bits().all() and out.c.null_count == 0, tag


ALIGNMENTS = {"all-aligned": (False, False, False), "lhs-unaligned": (True, False, False), "rhs-unaligned": (False, True, False),
              "out-unaligned": (False, False, True)}


@pytest.mark.parametrize("ldt,rdt", [(np.int8, np.int8), (np.int16, np.int16), (np.int32, np.int32), (np.float32, np.int32),
                                     (np.int64, np.int64), (np.int64, np.float64)],
                         ids=lambda d: np.dtype(d).name)
def test_vector_kernel_edges_two_columns(gdf, ldt, rdt):
    """Same-width pairs (the only column pairs that take the vector kernel) at vector_sizes(width); all three pointers aligned (vector
    body + element-wise tail), and lhs, rhs and output misaligned one at a time (element-wise throughout).  A third of the rows are
    equal pairs."""
    from libgdf_amd import libgdf
    from libgdf_amd.columns import Column
    width = np.dtype(ldt).itemsize
    rng = np.random.default_rng([41, width, np.dtype(rdt).kind == "f"])
    for n in vector_sizes(width):
        l, r = _small_values(rng, ldt, n), _small_values(rng, rdt, n)
        r[::3] = l[::3].astype(rdt)
        expected = [oracle.comparison(l, r, op) for op in OPS]
        for name, (lu, ru, ou) in ALIGNMENTS.items():
            cl = Column(device_slice(l, unaligned_offset(ldt) if lu else 0))
            cr = Column(device_slice(r, unaligned_offset(rdt) if ru else 0))
            assert (cl.data.data_ptr() % 16 != 0) == lu and (cr.data.data_ptr() % 16 != 0) == ru
            for op in OPS:
                _run_into_slice(gdf, lambda out: libgdf.gpu_comparison(cl.ptr, cr.ptr, out.ptr, op), n, 3 if ou else 0, expected[op],
                                (n, name, op))


@pytest.mark.parametrize("cdt,sdt", [(np.int8, np.int8), (np.int8, np.float64), (np.int16, np.int16), (np.int16, np.int64),
                                     (np.float32, np.float32), (np.int32, np.int8), (np.int64, np.int64), (np.float64, np.float32)],
                         ids=lambda d: np.dtype(d).name)
def test_vector_kernel_edges_scalar(gdf, cdt, sdt):
    """A scalar of any dtype takes the vector kernel (there is no right column to load): every column width with a scalar of its own
    dtype and with one of another width, at vector_sizes(width); all aligned, then the column and the output misaligned in turn."""
    from libgdf_amd import libgdf
    from libgdf_amd.columns import Column
    width = np.dtype(cdt).itemsize
    rng = np.random.default_rng([43, width, np.dtype(sdt).itemsize])
    fn = getattr(libgdf, "gpu_comparison_static_" + SUFFIX[np.dtype(sdt)])
    for n in vector_sizes(width):
        l = _small_values(rng, cdt, n)
        s = np.dtype(sdt).type(1)
        expected = [oracle.comparison(l, s, op) for op in OPS]
        for name, (lu, _, ou) in ALIGNMENTS.items():
            if name == "rhs-unaligned":
                continue
            cl = Column(device_slice(l, unaligned_offset(cdt) if lu else 0))
            assert (cl.data.data_ptr() % 16 != 0) == lu
            for op in OPS:
                _run_into_slice(gdf, lambda out: fn(cl.ptr, s.item(), out.ptr, op), n, 3 if ou else 0, expected[op], (n, name, op))


# ---- comparison_mask ---------------------------------------------------------------------------------------------------------------
MASK_SIZES = [1, 8, 9, 1003, 70001]


def _masked(gdf, data, valid, garbage, null_count=None):
    """A column whose mask buffer holds `valid` (bits beyond n clear, or all set when `garbage`) and whose null_count is the mask's zero
    bits among the first n unless given."""
    import torch
    from libgdf_amd.columns import Column, mask_from_bools
    m = garbage_mask(valid) if garbage else mask_from_bools(valid)
    nulls = int(len(valid) - np.count_nonzero(valid)) if null_count is None else null_count
    return Column(torch.from_numpy(np.ascontiguousarray(data)).cuda(), torch.from_numpy(m).cuda(), null_count=nulls)


@pytest.mark.parametrize("garbage", [False, True], ids=["zero-padded", "bits-beyond-n-set"])
@pytest.mark.parametrize("n", MASK_SIZES)
def test_comparison_masks_by_branch(gdf, n, garbage):
    """comparison_mask(): `both null counts zero` fills ones; `vl == vr` copies (one column on both sides, and every scalar variant);
    everything else is mask_and_kernel, which counts the zero bits among the first n rows only -- input masks whose bits beyond n are
    all set must not lower null_count."""
    rng = np.random.default_rng([47, n, int(garbage)])
    l, r = rng.integers(-3, 4, size=n).astype(np.int32), rng.integers(-3, 4, size=n).astype(np.int64)
    lv, rv = rng.random(n) < 0.7, rng.random(n) < 0.6
    lv[0], rv[0] = False, False                  # (at least one null each, also at n = 1: the count is what selects the branch)
    ones = np.ones(n, dtype=bool)

    def check(out, bits, tag):
        np.testing.assert_array_equal(out.valid_bits(), bits, err_msg=tag)
        assert out.c.null_count == n - int(bits.sum()), (tag, out.c.null_count)
        return out

    # mask_and_kernel: left only, right only (the other pointer is null = all ones), both
    check(gdf.api.comparison(_masked(gdf, l, lv, garbage), _col(r), 0), lv, "left only")
    check(gdf.api.comparison(_col(l), _masked(gdf, r, rv, garbage), 0), rv, "right only")
    out = check(gdf.api.comparison(_masked(gdf, l, lv, garbage), _masked(gdf, r, rv, garbage), 2), lv & rv, "both")
    np.testing.assert_array_equal(out.to_numpy(), oracle.comparison(l, r, 2))          # (the data do not depend on the masks)
    # ... one side's mask present but without nulls, the other with nulls: still the AND
    check(gdf.api.comparison(_masked(gdf, l, ones, garbage), _masked(gdf, r, rv, garbage), 0), rv, "left mask all ones")
    # the copy branch: one column on both sides shares one mask pointer
    c = _masked(gdf, l, lv, garbage)
    out = check(gdf.api.comparison(c, c, 0), lv, "same column")
    assert out.to_numpy().all()
    # masks present, both null counts zero: the counts are trusted (as the reference does), the output is all ones
    check(gdf.api.comparison(_masked(gdf, l, lv, garbage, null_count=0), _masked(gdf, r, rv, garbage, null_count=0), 0), ones,
          "null counts zero")
    # the scalar variants: the column's mask is copied
    for s in (np.int8(1), np.int16(1), np.int32(1), np.int64(1), np.float32(1), np.float64(1)):
        out = check(gdf.api.comparison(_masked(gdf, l, lv, garbage), s, 4), lv, f"scalar {s.dtype}")
        np.testing.assert_array_equal(out.to_numpy(), oracle.comparison(l, s, 4))
    check(gdf.api.comparison(_masked(gdf, l, lv, garbage, null_count=0), np.int32(0), 1), ones, "scalar, null count zero")
