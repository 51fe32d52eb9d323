"""Reductions and the radix selection on columns whose data pointer is not even element-aligned (one byte past a 16-byte boundary):
both kernels then treat every element as loose (head = n, no 16-byte vector) and only do element-wise loads.  The columns are raw
gdf_column views of a uint8 buffer with guard bytes around them; answers come from the numpy rules on the same bytes.
Run this file in a pytest process of its own, after the other statistics tests: it is the one branch here that no aligned test
shares code with."""
import ctypes as C

import numpy as np
import pytest

from elementwise_common import GUARD, PAD
from stats_reference import QUANTILE_METHODS, quantile_rule, reduce_rule, same

pytestmark = pytest.mark.gpu

N = 1000


def _misaligned(values):
    """(device tensor, gdf_column) with the column's bytes one byte past a 16-byte boundary, guard bytes on both sides"""
    import torch
    from libgdf_amd._binding import gdf_column
    from libgdf_amd.columns import get_dtype
    raw = np.ascontiguousarray(values).view(np.uint8)
    start = PAD + 1
    host = np.full(start + len(raw) + PAD, GUARD, dtype=np.uint8)
    host[start: start + len(raw)] = raw
    t = torch.from_numpy(host).cuda()
    assert t.data_ptr() % 16 == 0
    c = gdf_column()
    c.data, c.size, c.dtype, c.null_count = t.data_ptr() + start, len(values), get_dtype(values.dtype), 0
    c.valid = None
    assert c.data % values.dtype.itemsize == 1
    return t, c, host


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.float64], ids=lambda d: np.dtype(d).name)
def test_byte_misaligned_column(gdf, dtype):
    import torch
    from libgdf_amd.columns import new_context
    dt = np.dtype(dtype)
    rng = np.random.default_rng(61 + dt.itemsize)
    if dt.kind == "f":
        a = rng.integers(-1024, 1025, size=N).astype(dt) / 4          # multiples of 1/4: the sum is exact
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, int(info.max) + 1, size=N, dtype=np.int64).astype(dt) if dt != np.int64 else \
            rng.integers(-(2**62), 2**62, size=N, dtype=np.int64)
    t, c, host = _misaligned(a)
    out = torch.zeros(16, dtype=torch.uint8, device="cuda")
    for op in ("sum", "max"):
        getattr(gdf.libgdf, f"gdf_{op}_generic")(C.byref(c), out.data_ptr(), 1)
        got = out[: dt.itemsize].cpu().numpy().view(dt)[0]
        assert got == reduce_rule(op, a), (op, got, reduce_rule(op, a))
    s = np.sort(a)
    ctx = new_context(flag_sorted=0, method=0, flag_sort_inplace=0)
    res = np.zeros(1, dtype=dt)
    gdf.libgdf.gdf_quantile_aprrox(C.byref(c), 0.5, res.ctypes.data, C.byref(ctx))
    assert same(res[0], quantile_rule(s, 0.5, None)), (res[0], quantile_rule(s, 0.5, None))
    for m in range(len(QUANTILE_METHODS)):
        r = C.c_double(0.0)
        gdf.libgdf.gdf_quantile_exact(C.byref(c), m, 0.5, C.addressof(r), C.byref(ctx))
        assert same(r.value, quantile_rule(s, 0.5, m)), (m, r.value, quantile_rule(s, 0.5, m))
    assert np.array_equal(t.cpu().numpy(), host), "the buffer, guard bytes included, must be unchanged"
