"""Whole-column reductions (csrc/reduce.hip) on inputs whose result is EXACT in every combine order, so a float result can be compared
bit for bit and one dropped or doubled element cannot hide in a tolerance: sums of integer-valued floats, products of powers of two,
a single 1 among zeros at every boundary of the element -> thread map, mask padding bits, and every flavour of NaN."""
import numpy as np
import pytest

import stats_common as sc
from stats_reference import reduce_identity, reduce_rule

pytestmark = pytest.mark.gpu

DTYPES = [np.int8, np.int32, np.int64, np.float32, np.float64]
FLOATS = [np.float32, np.float64]
OPS = ["sum", "product", "min", "max", "sum_squared"]
IDS = lambda d: np.dtype(d).name            # noqa: E731
THREADS, UNROLL = 256, 4                    # rd_column: 256 lanes, four 16-byte vectors per lane in flight


def _ops_for(dtype):
    return OPS if np.dtype(dtype).kind == "f" else OPS[:4]


def _ncu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tile(dtype):
    return THREADS * UNROLL * (16 // np.dtype(dtype).itemsize)        # one workgroup's elements per trip


def _run(gdf, op, col, dtype):
    import torch
    dt = np.dtype(dtype)
    out = torch.zeros(dt.itemsize, dtype=torch.uint8, device="cuda")
    getattr(gdf.libgdf, f"gdf_{op}_generic")(col.ptr, out.data_ptr(), 1)
    return out.cpu().numpy().view(dt)[0]


def _same_bits(got, want):
    return np.asarray(got).tobytes() == np.asarray(want).tobytes()


def _exact(op, a, valid=None):
    """sum / sum_squared of integer-valued floats as a Python int, rounded once to the column type"""
    v = a if valid is None else a[valid]
    x = v.astype(np.int64)
    tot = int(np.sum(x)) if op == "sum" else int(np.sum(x * x))
    assert abs(tot) < 2**53
    return a.dtype.type(tot)


def _integer_valued(dtype, n, rng):
    return rng.integers(-1024, 1025, size=n).astype(dtype)


# ---------------------------------------------------------------------------------------------------------------------------------
# F1: exact float sums

@pytest.mark.parametrize("dtype", FLOATS, ids=IDS)
def test_exact_sums_at_tile_and_grid_boundaries(gdf, dtype):
    """integers in [-1024, 1024]: |sum| <= 2^33 and sum of squares <= 2^43 at these sizes, exact in f64 in every order; the f32
    result is that integer rounded once"""
    from libgdf_amd.columns import column_from_numpy
    v = 16 // np.dtype(dtype).itemsize
    tile = _tile(dtype)
    ncu = 256
    sizes = [v - 1, v, v + 1, tile - 1, tile, tile + 1, 2 * tile + 7, ncu * 4 * tile - 1, ncu * 4 * tile, ncu * 4 * tile + 1,
             ncu * 4 * tile * 2 + 5]
    rng = np.random.default_rng(41)
    for n in sizes:
        a = _integer_valued(dtype, n, rng)
        valid = rng.random(n) < 0.9
        for op in ("sum", "sum_squared"):
            got = _run(gdf, op, column_from_numpy(a), dtype)
            assert _same_bits(got, _exact(op, a)), (op, n, got, _exact(op, a))
            got = _run(gdf, op, column_from_numpy(a, valid), dtype)
            assert _same_bits(got, _exact(op, a, valid)), (op, n, "masked", got, _exact(op, a, valid))


@pytest.mark.parametrize("dtype", FLOATS, ids=IDS)
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_exact_sums_on_unaligned_slices(gdf, dtype, offset):
    import torch
    from libgdf_amd.columns import Column, mask_from_bools
    n = 100003
    rng = np.random.default_rng(43 + offset)
    a = _integer_valued(dtype, n + offset, rng)
    t = torch.from_numpy(a).cuda()
    view = a[offset:]
    valid = rng.random(n) < 0.7
    for op in ("sum", "sum_squared"):
        col = Column(t[offset:], torch.from_numpy(mask_from_bools(valid)).cuda(), null_count=int(n - valid.sum()))
        assert _same_bits(_run(gdf, op, col, dtype), _exact(op, view, valid)), (op, offset, "masked")
        assert _same_bits(_run(gdf, op, Column(t[offset:]), dtype), _exact(op, view)), (op, offset)


# ---------------------------------------------------------------------------------------------------------------------------------
# F2: exact float products

@pytest.mark.parametrize("dtype", FLOATS, ids=IDS)
def test_exact_products(gdf, dtype):
    """factors +-1 with at most 100 factors of 2 and 100 of 0.5 (signs kept): every partial product of every subset lies within
    2^+-100, so the product is exact in any tree, in f32 as well -- bit equality, sign included"""
    from libgdf_amd.columns import column_from_numpy
    dt = np.dtype(dtype)
    tile = _tile(dtype)
    rng = np.random.default_rng(47)
    for n in (tile - 1, tile + 1, _ncu() * 4 * tile + 1):
        a = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(dt)
        where = rng.choice(n, size=min(200, n), replace=False)
        twos, halves = where[: int(rng.integers(50, 101))], where[100: 100 + int(rng.integers(50, 101))]
        a[twos] *= 2
        a[halves] *= 0.5
        for valid in (None, rng.random(n) < 0.9):
            v = a if valid is None else a[valid]
            exp = int(np.count_nonzero(np.abs(v) == 2)) - int(np.count_nonzero(np.abs(v) == 0.5))
            sign = -1.0 if np.count_nonzero(v < 0) % 2 else 1.0
            want = dt.type(sign * 2.0 ** exp)
            got = _run(gdf, "product", column_from_numpy(a, valid), dtype)
            assert _same_bits(got, want), (n, valid is not None, got, want)


# ---------------------------------------------------------------------------------------------------------------------------------
# F3: a single 1 among zeros, at every boundary of the element -> thread map

def _boundary_indices(n, itemsize, off, ncu):
    """element indices where the map of rd_column changes hands, for a column whose data pointer is `off` elements past a 16-byte
    boundary: elements [0, head) and [head + nvec * V, n) go one per thread; vector j (elements head + j*V ...) belongs to thread
    j % (grid * 256), the grid being ceil(nvec / 1024) workgroups, at most 4 per CU"""
    V = 16 // itemsize
    head = min((V - off) % V, n)
    nvec = (n - head) // V
    grid = max(1, min(-(-nvec // (THREADS * UNROLL)), ncu * 4))
    stride = grid * THREADS
    last_lane = stride - 1
    assert nvec > last_lane
    j_last = last_lane + ((nvec - 1 - last_lane) // stride) * stride
    idx = {0, head - 1, head, head + nvec * V - 1, head + nvec * V, n - 1, head + last_lane * V, head + j_last * V + V - 1}
    return sorted(i for i in idx if 0 <= i < n), head, nvec


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("off", [0, 1])
def test_single_element_sensitivity(gdf, dtype, off):
    import torch
    from libgdf_amd.columns import Column
    dt = np.dtype(dtype)
    ncu = _ncu()
    n = ncu * 4 * _tile(dtype) + 1
    tdt = getattr(torch, dt.name)
    t = torch.zeros(n + off, dtype=tdt, device="cuda")
    assert t.data_ptr() % 16 == 0
    view = t[off:]
    idx, head, nvec = _boundary_indices(n, dt.itemsize, off, ncu)
    assert len(idx) >= 4 and head == ((16 // dt.itemsize - off) % (16 // dt.itemsize))
    mask = torch.full(((n + 7) // 8 + 64,), 0xFF, dtype=torch.uint8, device="cuda")
    plain = Column(view)
    masked = Column(view, mask, null_count=1)
    one, zero = dt.type(1), dt.type(0)
    for i in idx:
        view[i] = 1
        for op in ("sum", "max"):
            got = _run(gdf, op, plain, dtype)
            assert _same_bits(got, one), (op, i, got)
        mask[i >> 3] = 0xFF ^ (1 << (i & 7))
        for op in ("sum", "max"):
            got = _run(gdf, op, masked, dtype)
            assert _same_bits(got, zero), (op, i, "masked", got)
        mask[i >> 3] = 0xFF
        view[i] = 0


# ---------------------------------------------------------------------------------------------------------------------------------
# F4: the padding bits of the mask are not rows

@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_mask_padding_bits_are_ignored(gdf, dtype):
    """every row null, n not a multiple of 8, the padding bits of the last mask byte and the byte behind the mask all ones"""
    import torch
    from libgdf_amd.columns import Column
    dt = np.dtype(dtype)
    rng = np.random.default_rng(53)
    for n in (13, 1003, 2 * _tile(dtype) + 5):
        assert n % 8
        a = (rng.integers(2, 100, size=n)).astype(dt)
        mbytes = (n + 7) // 8
        m = np.zeros(mbytes + 1, dtype=np.uint8)
        m[mbytes - 1] = (0xFF << (n % 8)) & 0xFF
        m[mbytes] = 0xFF
        col = Column(torch.from_numpy(a).cuda(), torch.from_numpy(m).cuda(), null_count=n)
        for op in _ops_for(dtype):
            got = _run(gdf, op, col, dtype)
            assert _same_bits(got, reduce_identity(op, dt)), (op, n, got)


# ---------------------------------------------------------------------------------------------------------------------------------
# F5: every flavour of NaN

@pytest.mark.parametrize("dtype", FLOATS, ids=IDS)
def test_nan_flavours(gdf, dtype):
    """one NaN of any sign and payload makes every reduction NaN; masked out, the result is the rule's (exact here: integer-valued
    data for sum / min / max / sum_squared, powers of two for product)"""
    from libgdf_amd.columns import column_from_numpy
    dt = np.dtype(dtype)
    rng = np.random.default_rng(59)
    n = 5003
    ints = _integer_valued(dtype, n, rng)
    pows = np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(dt)
    pows[rng.choice(n, 60, replace=False)] *= 2
    for nan, bits in zip(sc.nan_values(dt), sc.NAN_BITS[dt]):
        at = int(rng.integers(0, n))
        valid = np.ones(n, dtype=bool)
        valid[at] = False
        for op in OPS:
            a = (pows if op == "product" else ints).copy()
            sc.bits_of(a)[at] = bits                           # (through the bits: no float move may quieten the pattern)
            assert np.isnan(a[at]) and np.isnan(nan) and int(sc.bits_of(a)[at]) == bits
            got = _run(gdf, op, column_from_numpy(a), dtype)
            assert np.isnan(got), (op, hex(bits), got)
            got = _run(gdf, op, column_from_numpy(a, valid), dtype)
            if op in ("sum", "sum_squared"):
                want = _exact(op, np.where(valid, a, 0).astype(dt), None)
            elif op == "product":
                v = a[valid]
                want = dt.type((-1.0 if np.count_nonzero(v < 0) % 2 else 1.0) * 2.0 ** int(np.count_nonzero(np.abs(v) == 2)))
            else:
                want = reduce_rule(op, a, valid)
            assert _same_bits(got, want), (op, hex(bits), "masked", got, want)
