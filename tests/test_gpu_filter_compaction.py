"""-m gpu: gpu_apply_stencil, one case per combination of count and write kernel that compact() (csrc/filter.hip) can pick.

compact() decides by the 16-byte alignment of the stencil and of the data column and, once the count is known, by the share of kept
rows.  Stencil and data are slices of larger device tensors with INDEPENDENT element offsets; every test asserts the alignment it
means to have.  Below 2^22 rows (and for the data widths below 8 bytes at any size) the request takes the two passes:

    stencil    data       kept     count kernel            write kernel
    aligned    aligned    any      stencil_count_kernel    stencil_stage_write_kernel
    aligned    unaligned  < n/3    stencil_count_kernel    stencil_write_kernel      (<= 4 per 16-row group: the __ffs loop;
                                                                                      more: the `mine > 4` branch)
    aligned    unaligned  >= n/3   stencil_count_kernel    compact_write_kernel
    unaligned  either     any      compact_count_kernel    compact_write_kernel

Which kernel ran cannot be observed from here (the profile labels `compact_count` / `compact_write` are shared); the mapping is
derived from compact()'s conditions and kept in the docstrings.  The expectation is oracle.apply_stencil; the data are random BITS
and compared as bits, the non-zero stencil bytes come from {1, 2, -1, -128, 64} (the contract is `!= 0`), and a stencil validity mask
has every bit from n to the end of its buffer set.
"""
import functools

import numpy as np
import pytest

from filter_common import bits_of, device_slice, garbage_mask, random_bits, unaligned_offset
from oracle import oracle

pytestmark = pytest.mark.gpu

WIDTH_DTYPES = [np.int8, np.int16, np.float32, np.int64]          # 1, 2, 4 and 8 bytes
NONZERO = np.array([1, 2, -1, -128, 64], dtype=np.int8)
TILE = 4096                                                      # rows per tile of the vector write kernels (FLS_ROWS)
SIZES = [0, 1, 15, 16, 17, TILE - 1, TILE, TILE + 1, 3 * TILE + 1234]
BIG = 2048 * TILE + 3 * TILE + 77                                # chunk = 2 tiles: ceil(BIG / 2048) = 4103 rows, rounded up to 8192
_ids = dict(ids=lambda d: np.dtype(d).name)


def keep_pattern(kind, n, rng):
    """bool[n]: mixed ~40 % / dense ~60 % at random; sparse: ~19 %, at most 4 per aligned 16-row group; clustered: one run of 16 kept
    rows in every 96 (17 %), starting anywhere in the first 16 rows of the 96 -- groups with 16, or with s and 16 - s, kept rows."""
    if kind == "mixed":
        return rng.random(n) < 0.4
    if kind == "dense":
        return rng.random(n) < 0.6
    if kind == "sparse":
        groups = -(-n // 16)
        k = rng.random((groups, 16)) < 0.2
        k &= np.cumsum(k, axis=1) <= 4
        return k.ravel()[:n]
    assert kind == "clustered"
    k = np.zeros(n + 112, dtype=bool)
    starts = np.arange(0, n, 96)
    starts = starts + rng.integers(0, 16, size=len(starts))
    k[(starts[:, None] + np.arange(16)).ravel()] = True
    return k[:n]


def stencil_bytes(keep, rng):
    return np.where(keep, NONZERO[rng.integers(0, len(NONZERO), size=len(keep))], np.int8(0)).astype(np.int8)


def run_and_check(gdf, data, stencil, valid, st_off, data_unaligned, tag):
    """One gpu_apply_stencil request, checked as test_gpu_filter.test_apply_stencil does: the kept elements in input order, out.size,
    null_count == 0 and an output mask of `kept` ones followed by zeros up to bit n."""
    import torch
    from libgdf_amd.columns import Column
    n = len(data)
    d_off = unaligned_offset(data.dtype) if data_unaligned else 0
    td, ts = device_slice(data, d_off), device_slice(stencil, st_off)
    if n:
        assert (td.data_ptr() % 16 != 0) == data_unaligned and (ts.data_ptr() % 16 != 0) == (st_off != 0), tag
    tv, nulls = None, 0
    if valid is not None:
        tv = torch.from_numpy(garbage_mask(valid)).cuda()
        nulls = int(n - np.count_nonzero(valid))
    out = gdf.api.apply_stencil(Column(td), Column(ts, tv, 1, null_count=nulls))
    exp = oracle.apply_stencil(data, stencil, valid)
    assert out.size == len(exp), (tag, out.size, len(exp))
    np.testing.assert_array_equal(bits_of(out.to_numpy()), bits_of(exp), err_msg=str(tag))
    assert out.c.null_count == 0, tag
    bits = out.valid_bits(n)
    assert bits[: len(exp)].all() and not bits[len(exp):].any(), tag
    return len(exp)


def sweep(gdf, dtype, st_off, data_unaligned, kind, kept_check):
    """Every size of SIZES, without and with a stencil validity mask.  kept_check(kept, n) states the share of kept rows that the table
    row needs; it is asserted on the INPUT from one tile on (below that the patterns cannot hold a share)."""
    rng = np.random.default_rng([17, np.dtype(dtype).itemsize, st_off, int(data_unaligned), len(kind)])
    for n in SIZES:
        for masked in (False, True):
            keep = keep_pattern(kind, n, rng)
            valid = rng.random(n) < 0.85 if masked else None
            kept = run_and_check(gdf, random_bits(rng, dtype, n), stencil_bytes(keep, rng), valid, st_off, data_unaligned,
                                 (np.dtype(dtype).name, kind, n, masked))
            if n >= TILE - 1:
                assert kept_check(kept, n), (kind, n, masked, kept)


@pytest.mark.parametrize("dtype", WIDTH_DTYPES, **_ids)
def test_aligned_stencil_aligned_data(gdf, dtype):
    """stencil offset 0, data offset 0, ~40 % kept: stencil_count_kernel + stencil_stage_write_kernel<width> (both pointers 16-byte
    aligned, chunk a multiple of 4096).  n = 4095 is one ragged tile (element-wise loads), 4096 one whole tile (vector loads), 4097
    and 3 * 4096 + 1234 whole tiles and a ragged one in the next chunks; below 16 rows only the single-bit tail runs."""
    sweep(gdf, dtype, 0, False, "mixed", lambda kept, n: True)


@pytest.mark.parametrize("dtype", WIDTH_DTYPES, **_ids)
def test_aligned_stencil_unaligned_data_sparse(gdf, dtype):
    """stencil offset 0, data offset 1 element (3 for int8), fewer than a third kept and at most 4 per 16-row group:
    stencil_count_kernel + stencil_write_kernel<width>, every thread in the `__ffs` loop."""
    sweep(gdf, dtype, 0, True, "sparse", lambda kept, n: kept * 3 < n)


@pytest.mark.parametrize("dtype", WIDTH_DTYPES, **_ids)
def test_aligned_stencil_unaligned_data_clustered(gdf, dtype):
    """stencil offset 0, data offset 1 element (3 for int8), fewer than a third kept in runs of 16 rows with gaps of 80:
    stencil_count_kernel + stencil_write_kernel<width>, the threads that own a run in the `mine > 4` branch (16 independent loads, then
    the stores), their neighbours with nothing to write."""
    sweep(gdf, dtype, 0, True, "clustered", lambda kept, n: 0 < kept * 3 < n)


@pytest.mark.parametrize("dtype", WIDTH_DTYPES, **_ids)
def test_aligned_stencil_unaligned_data_dense(gdf, dtype):
    """stencil offset 0, data offset 1 element (3 for int8), at least a third kept (60 %, 51 % under the mask): the vector count
    followed by the ballot write, stencil_count_kernel + compact_write_kernel<StencilPred, width>."""
    sweep(gdf, dtype, 0, True, "dense", lambda kept, n: kept * 3 >= n)


@pytest.mark.parametrize("data_unaligned", [False, True], ids=["data-aligned", "data-unaligned"])
@pytest.mark.parametrize("dtype", WIDTH_DTYPES, **_ids)
def test_unaligned_stencil(gdf, dtype, data_unaligned):
    """stencil offset 3, data offset 0 or 1 element (3 for int8), ~40 % kept: compact_count_kernel<StencilPred> +
    compact_write_kernel<StencilPred, width>, whatever the data's alignment."""
    sweep(gdf, dtype, 3, data_unaligned, "mixed", lambda kept, n: True)


@functools.lru_cache(maxsize=None)
def _big_inputs(kind):
    """(stencil bytes, validity) of the BIG request for one keep pattern -- made once, shared by the dtypes, never modified."""
    rng = np.random.default_rng([29, len(kind)])
    st = stencil_bytes(keep_pattern(kind, BIG, rng), rng)
    valid = rng.random(BIG) < 0.85
    st.setflags(write=False)
    valid.setflags(write=False)
    return st, valid


@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "mask"])
@pytest.mark.parametrize("kind,data_unaligned", [("mixed", False), ("sparse", True), ("clustered", True)],
                         ids=["aligned-aligned", "aligned-unaligned-sparse", "aligned-unaligned-clustered"])
@pytest.mark.parametrize("dtype", [np.int8, np.int64], **_ids)
def test_two_tiles_per_chunk(gdf, force_path, dtype, kind, data_unaligned, masked):
    """n = 2048 * 4096 + 3 * 4096 + 77: ceil(n / 2048) = 4103 rows round up to a chunk of 8192, so every workgroup of the write kernel
    walks TWO 4096-row tiles and the second one starts at `base += total` of the first -- the carry of stencil_stage_write_kernel
    (aligned / aligned) and of stencil_write_kernel (aligned stencil, unaligned data, fewer than a third kept; both of its branches).
    The last chunk ends in a ragged tile.  The aligned int64 request would take the lockstep rounds from 2^22 rows on (they are tested in
    test_gpu_filter.py); GDF_FL_NO_ROUNDS sends it through the two passes."""
    if not data_unaligned and np.dtype(dtype).itemsize == 8:
        force_path("GDF_FL_NO_ROUNDS")
    st, valid = _big_inputs(kind)
    rng = np.random.default_rng([31, np.dtype(dtype).itemsize])
    kept = run_and_check(gdf, random_bits(rng, dtype, BIG), st, valid if masked else None, 0, data_unaligned,
                         (np.dtype(dtype).name, kind, BIG, masked))
    assert kind == "mixed" or 0 < kept * 3 < BIG


@pytest.mark.parametrize("data_unaligned", [False, True], ids=["data-aligned", "data-unaligned"])
@pytest.mark.parametrize("st_off", [0, 3], ids=["stencil-aligned", "stencil-unaligned"])
@pytest.mark.parametrize("dtype", WIDTH_DTYPES, **_ids)
def test_no_keeper_and_all_keeper(gdf, dtype, st_off, data_unaligned):
    """n = 4097 at the extremes, for the four alignment combinations.  Nothing kept (all stencil bytes zero; or all non-zero under an
    all-zero validity mask) is `kept < n / 3`: with an aligned stencil and unaligned data it is stencil_write_kernel with nothing to
    write.  Everything kept (without a mask, and under an all-ones mask whose bits beyond n are set as well) is `kept >= n / 3`: there
    it is compact_write_kernel.  Aligned / aligned stays with stencil_stage_write_kernel, an unaligned stencil with the ballot pair."""
    n = TILE + 1
    rng = np.random.default_rng([37, np.dtype(dtype).itemsize, st_off, int(data_unaligned)])
    data = random_bits(rng, dtype, n)
    nonzero = stencil_bytes(np.ones(n, dtype=bool), rng)
    tag = (np.dtype(dtype).name, st_off, data_unaligned)
    assert run_and_check(gdf, data, np.zeros(n, dtype=np.int8), None, st_off, data_unaligned, tag + ("zero stencil",)) == 0
    assert run_and_check(gdf, data, nonzero, np.zeros(n, dtype=bool), st_off, data_unaligned, tag + ("zero mask",)) == 0
    assert run_and_check(gdf, data, nonzero, None, st_off, data_unaligned, tag + ("all kept",)) == n
    assert run_and_check(gdf, data, nonzero, np.ones(n, dtype=bool), st_off, data_unaligned, tag + ("all kept, mask",)) == n
