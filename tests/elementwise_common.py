"""Device-buffer helpers of the GPU tests of csrc/elementwise.hip: columns at a chosen element misalignment against 16 bytes, inside
a buffer whose other bytes hold a guard pattern that must survive every call."""
import ctypes as C

import numpy as np

GUARD = 0xA5
PAD = 64                      # guard bytes in front of and behind the column
SIZES = [1, 2, 15, 16, 17, 63, 64, 65, 1000, 2**20 + 3]
BIG = 2**26 + 5


class Buf:
    """n elements of np_dtype at byte offset PAD + off * itemsize of a 16-byte aligned device buffer"""

    def __init__(self, n, np_dtype, off=0, values=None):
        import torch
        self.dtype = np.dtype(np_dtype)
        self.n = n
        self.start = PAD + off * self.dtype.itemsize
        self.nbytes = n * self.dtype.itemsize
        host = np.full(self.start + self.nbytes + PAD, GUARD, dtype=np.uint8)
        if values is not None:
            assert len(values) == n and values.dtype == self.dtype
            host[self.start: self.start + self.nbytes] = np.ascontiguousarray(values).view(np.uint8)
        self.t = torch.from_numpy(host).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + self.start

    def read(self):
        """the column's elements, after checking that no byte outside it changed"""
        host = self.t.cpu().numpy()
        assert (host[: self.start] == GUARD).all(), "bytes in front of the column were written"
        assert (host[self.start + self.nbytes:] == GUARD).all(), "bytes beyond the column were written"
        return host[self.start: self.start + self.nbytes].view(self.dtype).copy()


def mask_tensor(valid_bools):
    """(device tensor, host bytes) of an LSB-first mask"""
    import torch
    packed = np.packbits(np.asarray(valid_bools, dtype=bool), bitorder="little")
    return torch.from_numpy(packed.copy()).cuda(), packed


def col(buf, gdf_dtype, valid=None, unit=0, null_count=0):
    from libgdf_amd._binding import gdf_column
    c = gdf_column()
    c.data, c.size, c.dtype, c.null_count = buf.ptr, buf.n, gdf_dtype, null_count
    c.valid = valid.data_ptr() if valid is not None else None
    c.dtype_info.time_unit = unit
    return c


def ref(c):
    return C.byref(c)


def offsets(itemsize):
    """every element misalignment against 16 bytes"""
    return range(16 // itemsize)


def assert_same_bits(got, want, where=None):
    """equal as bit patterns (NaN payloads aside: a NaN matches a NaN), on the rows `where` selects"""
    if where is not None:
        got, want = got[where], want[where]
    if got.dtype.kind == "f":
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan)
        ui = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
        assert np.array_equal(got[~nan].view(ui), want[~nan].view(ui))
    else:
        assert got.dtype == want.dtype and np.array_equal(got, want)
