"""-m gpu: gdf_filter over every column dtype, size edge and match rate; gdf_validity_and, gdf_count_nonzero_mask, gdf_column_concat and
gpu_concat (csrc/filter.hip: compact<RowEqualsPred>, mask_and_kernel, mask_popcount_kernel, mask_concat_kernel) against numpy."""
import ctypes as C

import numpy as np
import pytest

from filter_common import garbage_mask
from oracle import oracle

pytestmark = pytest.mark.gpu

GDF = dict(int8=1, int16=2, int32=3, int64=4, float32=5, float64=6, date32=7, date64=8, timestamp=9)
STORAGE = dict(int8=np.int8, int16=np.int16, int32=np.int32, int64=np.int64, float32=np.float32, float64=np.float64, date32=np.int32,
               date64=np.int64, timestamp=np.int64)
# the scalar of each column: negative, fractional, and beyond 32 bits where the storage allows it
SCALAR = dict(int8=-7, int16=-300, int32=70001, int64=2**40 + 3, float32=1.5, float64=-2.25, date32=-12345, date64=2**41 + 5,
              timestamp=-(2**45) - 9)
COLUMN_SETS = [("int8",), ("int16", "float32"), ("int32", "int64", "float64"), ("date32", "date64", "timestamp", "int8")]
TILE = 4096
FILTER_SIZES = [0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1]
FILTER_BIG = 2048 * TILE + 300             # chunk = ceil(n / 2048) = 4097 rows rounded up to 8192; the last chunk holds 300 rows


def _filter_inputs(rng, names, n, mode):
    """Host columns + scalars.  The rows of `match` hold the scalar in EVERY column; every other row holds scalar + d, d in {-1, 0, 1},
    per column, and d = 1 in the column (row % ncols) -- so most rows agree with the scalars in some columns but never in all."""
    match = {"none": np.zeros(n, dtype=bool), "all": np.ones(n, dtype=bool), "one-percent": rng.random(n) < 0.01}[mode]
    rows = np.arange(n)
    cols = []
    for c, name in enumerate(names):
        d = rng.integers(-1, 2, size=n)
        d[rows % len(names) == c] = 1
        d[match] = 0
        cols.append((np.asarray(SCALAR[name], dtype=STORAGE[name]) + d.astype(STORAGE[name])).astype(STORAGE[name]))
    return cols, [SCALAR[name] for name in names], int(match.sum())


def _run_filter(gdf, names, cols, vals):
    from libgdf_amd.columns import column_from_numpy
    idx = gdf.api.filter_rows([column_from_numpy(c, dtype=GDF[name]) for c, name in zip(cols, names)], vals)
    return idx.cpu().numpy().astype(np.uint64)


@pytest.mark.parametrize("mode", ["none", "all", "one-percent"])
@pytest.mark.parametrize("names", COLUMN_SETS, ids=lambda s: "-".join(s))
def test_filter_dtypes_sizes_and_match_rates(gdf, names, mode):
    """One to four columns covering int8 ... float64 and the three date types (integer storage, the date dtype on the column), at 0, 1,
    one 256-row ballot tile +- 1 and one chunk +- 1 rows; no row, every row and about 1 % of the rows matching.  gdf_filter always takes
    compact_count_kernel + compact_write_kernel<RowEqualsPred, 0>; the indices come back ascending and new_sz is their number."""
    rng = np.random.default_rng([53, len(names), len(mode)])
    for n in FILTER_SIZES:
        cols, vals, nmatch = _filter_inputs(rng, names, n, mode)
        exp = oracle.filter_rows(cols, vals)
        assert len(exp) == nmatch                       # (the generator and the oracle agree on what matches)
        got = _run_filter(gdf, names, cols, vals)
        assert len(got) == len(exp), (n, len(got), len(exp))
        np.testing.assert_array_equal(got, exp, err_msg=str(n))


@pytest.mark.parametrize("names,mode", [(COLUMN_SETS[0], "none"), (COLUMN_SETS[0], "all"), (COLUMN_SETS[0], "one-percent"),
                                        (COLUMN_SETS[1], "one-percent"), (COLUMN_SETS[2], "one-percent"), (COLUMN_SETS[3], "one-percent")],
                         ids=lambda s: s if isinstance(s, str) else "-".join(s))
def test_filter_two_tiles_of_chunks(gdf, names, mode):
    """n = 2048 * 4096 + 300: 1025 chunks of 8192 rows, 32 ballot tiles each with the running base carried from tile to tile, and a
    last chunk of 300 rows.  Every column set at 1 % matching; the one-column set also with no and with every row matching."""
    rng = np.random.default_rng([59, len(names), len(mode)])
    cols, vals, nmatch = _filter_inputs(rng, names, FILTER_BIG, mode)
    exp = oracle.filter_rows(cols, vals)
    assert len(exp) == nmatch
    got = _run_filter(gdf, names, cols, vals)
    assert len(got) == len(exp)
    np.testing.assert_array_equal(got, exp)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_filter_nan_and_signed_zero(gdf, dtype):
    """Equality is the IEEE one: a NaN scalar matches no row (not even the NaN rows), -0.0 matches the rows holding 0.0 and -0.0."""
    n = 3 * 256 + 5
    a = np.array([np.nan, 0.0, -0.0, 1.0], dtype=dtype)[np.random.default_rng(61).integers(0, 4, size=n)]
    got = _run_filter(gdf, ("float32",) if dtype == np.float32 else ("float64",), [a], [float("nan")])
    assert len(got) == 0 and len(oracle.filter_rows([a], [np.nan])) == 0
    got = _run_filter(gdf, ("float32",) if dtype == np.float32 else ("float64",), [a], [-0.0])
    np.testing.assert_array_equal(got, np.nonzero(a == 0)[0].astype(np.uint64))
    np.testing.assert_array_equal(got, oracle.filter_rows([a], [-0.0]))
    # ... and next to a second column that always matches
    b = np.full(n, 4, dtype=np.int16)
    got = _run_filter(gdf, ("int16", "float32" if dtype == np.float32 else "float64"), [b, a], [4, -0.0])
    np.testing.assert_array_equal(got, oracle.filter_rows([b, a], [4, -0.0]))


# ---- gdf_validity_and ---------------------------------------------------------------------------------------------------------------
def _mask_column(n, valid, garbage=True):
    """An int8 column of n rows; valid None = no mask."""
    import torch
    from libgdf_amd.columns import Column
    tv, nulls = None, 0
    if valid is not None:
        tv = torch.from_numpy(garbage_mask(valid) if garbage else np.zeros_like(garbage_mask(valid))).cuda()
        nulls = int(n - np.count_nonzero(valid))
    return Column(torch.zeros(max(n, 1), dtype=torch.int8, device="cuda"), tv, 1, size=n, null_count=nulls)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 1001, 2**20 + 5])
def test_validity_and_missing_masks_and_garbage(gdf, n):
    """out = lhs & rhs with a missing mask counting as all ones, on either side and on both; the input masks carry set bits beyond n
    and null_count is the zero bits among the first n.  2^20 + 5 rows are 131073 mask bytes: 33 workgroups of 256 threads, 16 bytes
    per thread in a grid-stride loop, and a last byte with 5 live bits."""
    from libgdf_amd import libgdf
    rng = np.random.default_rng([67, n])
    a, b = rng.random(n) < 0.7, rng.random(n) < 0.5
    ones = np.ones(n, dtype=bool)
    for va, vb, tag in ((a, b, "both"), (None, b, "left missing"), (a, None, "right missing"), (None, None, "both missing")):
        ca, cb, out = _mask_column(n, va), _mask_column(n, vb), _mask_column(n, np.zeros(n, dtype=bool), garbage=False)
        out.c.null_count = -1
        libgdf.gdf_validity_and(ca.ptr, cb.ptr, out.ptr)
        exp = (ones if va is None else va) & (ones if vb is None else vb)
        np.testing.assert_array_equal(out.valid_bits(), exp, err_msg=tag)
        assert out.c.null_count == n - int(exp.sum()), (tag, out.c.null_count)


def test_validity_and_error_returns(gdf):
    from libgdf_amd import GDFError, libgdf
    v = np.ones(11, dtype=bool)
    c9, c10, d10, c11, bare10 = (_mask_column(9, v[:9]), _mask_column(10, v[:10]), _mask_column(10, v[:10]), _mask_column(11, v),
                                 _mask_column(10, None))
    with pytest.raises(GDFError, match="GDF_VALIDITY_MISSING"):                  # an output without a mask
        libgdf.gdf_validity_and(c10.ptr, d10.ptr, bare10.ptr)
    with pytest.raises(GDFError, match="GDF_COLUMN_SIZE_MISMATCH"):
        libgdf.gdf_validity_and(c10.ptr, c9.ptr, d10.ptr)
    with pytest.raises(GDFError, match="GDF_COLUMN_SIZE_MISMATCH"):
        libgdf.gdf_validity_and(c10.ptr, d10.ptr, c11.ptr)


# ---- gdf_count_nonzero_mask -----------------------------------------------------------------------------------------------------------
def test_count_nonzero_mask_many_workgroups(gdf):
    """2^24 + 5 rows = 2 MiB of mask: 512 workgroups, every wave adding its count to the one counter; the bits beyond n are set."""
    import torch
    from libgdf_amd import libgdf
    n = 2**24 + 5
    v = np.random.default_rng(71).random(n) < 0.37
    d = torch.from_numpy(garbage_mask(v)).cuda()
    cnt = C.c_int(0)
    libgdf.gdf_count_nonzero_mask(d.data_ptr(), n, C.byref(cnt))
    assert cnt.value == int(v.sum())


# ---- gdf_column_concat / gpu_concat ---------------------------------------------------------------------------------------------------
def _concat_parts(rng, dtype, lengths, unmasked_every=4):
    """Host parts + validity (None for every `unmasked_every`-th part: no mask = all valid)."""
    from filter_common import random_bits
    parts = [random_bits(rng, dtype, n) for n in lengths]
    valids = [None if i % unmasked_every == 2 else rng.random(n) < 0.6 for i, n in enumerate(lengths)]
    return parts, valids


def _concat_check(gdf, dtype, parts, valids, call):
    import torch
    from filter_common import bits_of
    from libgdf_amd.columns import Column, column_from_numpy, get_dtype
    cols = [column_from_numpy(p, v) for p, v in zip(parts, valids)]
    total = sum(len(p) for p in parts)
    out = Column(torch.empty(max(total, 1), dtype=getattr(torch, np.dtype(dtype).name), device="cuda"),
                 torch.zeros(((total + 7) // 8 + 63) // 64 * 64 or 64, dtype=torch.uint8, device="cuda"), get_dtype(dtype), size=total)
    out.c.null_count = -1
    call(out, cols)
    np.testing.assert_array_equal(bits_of(out.to_numpy()), bits_of(np.concatenate(parts)))
    exp_valid = np.concatenate([np.ones(len(p), dtype=bool) if v is None else v for p, v in zip(parts, valids)])
    np.testing.assert_array_equal(out.valid_bits(), exp_valid)
    assert out.c.null_count == sum(c.c.null_count for c in cols) == total - int(exp_valid.sum())


ALL_WIDTHS = [np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]


@pytest.mark.parametrize("dtype", ALL_WIDTHS, ids=lambda d: np.dtype(d).name)
def test_column_concat_many_short_columns(gdf, dtype):
    """37 columns of 0, 1, 3, 7, 8, 9, 64 or 1000 rows: several columns inside one output mask byte, zero-length columns first, last and
    between non-empty ones (also two in a row), every fourth column without a mask, and a source table long enough for
    mask_concat_kernel's binary search to take several steps."""
    from libgdf_amd import libgdf
    from libgdf_amd.columns import column_array
    rng = np.random.default_rng([73, np.dtype(dtype).itemsize, np.dtype(dtype).kind == "f"])
    lengths = [int(x) for x in rng.permutation(np.resize([0, 1, 3, 7, 8, 9, 64, 1000], 37))]
    lengths[0] = lengths[36] = lengths[5] = lengths[6] = lengths[20] = 0
    lengths[1:5] = [1, 3, 1, 1]                        # four columns (one without a mask) inside the first output byte
    lengths[19], lengths[21] = 7, 9
    assert set(lengths) == {0, 1, 3, 7, 8, 9, 64, 1000}
    parts, valids = _concat_parts(rng, dtype, lengths)
    _concat_check(gdf, dtype, parts, valids, lambda out, cols: libgdf.gdf_column_concat(out.ptr, column_array(cols), len(cols)))


@pytest.mark.parametrize("dtype", ALL_WIDTHS, ids=lambda d: np.dtype(d).name)
def test_column_concat_two_long_columns(gdf, dtype):
    """2^20 + 3 and 2^20 + 5 rows: 262145 output mask bytes (256 workgroups of mask_concat_kernel) and the boundary between the two
    columns three bits into a byte."""
    from libgdf_amd import libgdf
    from libgdf_amd.columns import column_array
    rng = np.random.default_rng([79, np.dtype(dtype).itemsize])
    parts, valids = _concat_parts(rng, dtype, [2**20 + 3, 2**20 + 5], unmasked_every=99)
    _concat_check(gdf, dtype, parts, valids, lambda out, cols: libgdf.gdf_column_concat(out.ptr, column_array(cols), len(cols)))


def test_gpu_concat_two_long_columns(gdf):
    from libgdf_amd import libgdf
    rng = np.random.default_rng(83)
    parts, valids = _concat_parts(rng, np.int32, [2**20 + 3, 2**20 + 5], unmasked_every=99)
    _concat_check(gdf, np.int32, parts, valids, lambda out, cols: libgdf.gpu_concat(cols[0].ptr, cols[1].ptr, out.ptr))


def test_concat_error_returns_in_order(gdf):
    """gdf_column_concat walks the array once and returns at the FIRST column it objects to: a null entry (GDF_DATASET_EMPTY) before a
    dtype mismatch behind it, a dtype mismatch (GDF_DTYPE_MISMATCH) before the total size is looked at, the size mismatch
    (GDF_COLUMN_SIZE_MISMATCH) last.  gpu_concat answers a dtype mismatch with GDF_VALIDITY_MISSING, as the reference does."""
    import torch
    from libgdf_amd import GDFError, libgdf
    from libgdf_amd._binding import gdf_column
    from libgdf_amd.columns import Column, column_from_numpy
    i32 = [column_from_numpy(np.arange(5, dtype=np.int32)) for _ in range(4)]
    i64 = column_from_numpy(np.arange(5, dtype=np.int64))

    def out(n, dtype=torch.int32):
        return Column(torch.empty(n, dtype=dtype, device="cuda"), torch.zeros(64, dtype=torch.uint8, device="cuda"))

    def array(entries):
        return (C.POINTER(gdf_column) * len(entries))(*[e.ptr if e is not None else C.POINTER(gdf_column)() for e in entries])

    wrong, wide20, out10, wide10, good = out(21), out(20, torch.int64), out(10), out(10, torch.int64), out(20)
    with pytest.raises(GDFError, match="GDF_DATASET_EMPTY"):
        libgdf.gdf_column_concat(wrong.ptr, array([i32[0], i32[1], None, i64]), 4)
    with pytest.raises(GDFError, match="GDF_DTYPE_MISMATCH"):
        libgdf.gdf_column_concat(wrong.ptr, array([i32[0], i64, i32[1], i32[2]]), 4)
    with pytest.raises(GDFError, match="GDF_DTYPE_MISMATCH"):                    # the output's dtype against the first column's
        libgdf.gdf_column_concat(wide20.ptr, array(i32), 4)
    with pytest.raises(GDFError, match="GDF_COLUMN_SIZE_MISMATCH"):
        libgdf.gdf_column_concat(wrong.ptr, array(i32), 4)
    with pytest.raises(GDFError, match="GDF_VALIDITY_MISSING"):
        libgdf.gpu_concat(i32[0].ptr, i64.ptr, out10.ptr)
    with pytest.raises(GDFError, match="GDF_VALIDITY_MISSING"):
        libgdf.gpu_concat(i32[0].ptr, i32[1].ptr, wide10.ptr)
    libgdf.gdf_column_concat(good.ptr, array(i32), 4)
    np.testing.assert_array_equal(good.to_numpy(), np.tile(np.arange(5, dtype=np.int32), 4))
