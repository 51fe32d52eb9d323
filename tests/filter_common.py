"""Helpers shared by the filter-family GPU tests (test_gpu_filter_compaction / _compare / _rows_masks)."""
import numpy as np

UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def garbage_mask(valid):
    """LSB-first mask bytes of `valid` (a 64-byte multiple, as columns.mask_from_bools pads) with EVERY bit from len(valid) to the end of
    the buffer set: a kernel that reads a bit past the last row sees a valid row that does not exist."""
    from libgdf_amd.columns import mask_from_bools
    valid = np.asarray(valid, dtype=bool)
    n = len(valid)
    m = mask_from_bools(valid)
    m[(n + 7) // 8:] = 0xFF
    if n % 8:
        m[n // 8] |= np.uint8((0xFF << (n % 8)) & 0xFF)
    return m


def device_slice(host, off):
    """`host` uploaded `off` ELEMENTS into a larger device allocation: the returned tensor starts off * itemsize bytes past a 16-byte
    boundary (the allocator hands out 256-byte multiples; the callers assert the alignment they mean to have)."""
    import torch
    host = np.ascontiguousarray(host)
    if not host.flags.writeable:
        host = host.copy()                         # (torch refuses to wrap a read-only array quietly)
    n = len(host)
    buf = torch.empty(off + n + 16, dtype=getattr(torch, host.dtype.name), device="cuda")
    buf[off:off + n] = torch.from_numpy(host)
    return buf[off:off + n]


def unaligned_offset(dtype):
    """The element offset the tests use to break a column's 16-byte alignment: 1 element for widths 2, 4 and 8, 3 elements for width 1."""
    return 3 if np.dtype(dtype).itemsize == 1 else 1


def random_bits(rng, dtype, n):
    """n elements of random BITS (floats: NaN payloads, infinities and subnormals included); compare through bits_of()."""
    dtype = np.dtype(dtype)
    return rng.integers(0, 256, size=n * dtype.itemsize, dtype=np.uint8).view(dtype)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(UNSIGNED[a.dtype.itemsize])
