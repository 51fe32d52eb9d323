"""Whole-column reductions on the GPU (csrc/reduce.hip) against the numpy restatement in stats_reference.py.  Replays the reference's
python/tests/test_reductions.py (5 dtypes x sizes, masked sums) and adds masks on every op, identities, wrap-around, NaN / inf,
unaligned slices, tile and grid boundaries, determinism and the one-element result contract."""
import numpy as np
import pytest

from stats_reference import reduce_identity, reduce_rule

pytestmark = pytest.mark.gpu

DTYPES = [np.int8, np.int32, np.int64, np.float32, np.float64]
OPS = ["sum", "product", "min", "max", "sum_squared"]
SFX = {np.dtype(np.int8): "i8", np.dtype(np.int32): "i32", np.dtype(np.int64): "i64", np.dtype(np.float32): "f32",
       np.dtype(np.float64): "f64"}


def _ops_for(dtype):
    return OPS if np.dtype(dtype).kind == "f" else OPS[:4]


def _values(op, dtype, n):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        if op == "product":
            return np.random.uniform(0.99, 1.01, n).astype(dt)
        return (np.random.random(n) * 2 - 1).astype(dt)
    info = np.iinfo(dt)
    return np.random.randint(info.min, int(info.max) + 1, size=n, dtype=np.int64).astype(dt)


def _run(gdf, op, col, dtype, typed=False, size=1, out=None):
    import torch
    dt = np.dtype(dtype)
    if out is None:
        out = torch.zeros(max(size, 1) * dt.itemsize, dtype=torch.uint8, device="cuda")
    name = f"gdf_{op}_{SFX[dt] if typed else 'generic'}"
    getattr(gdf.libgdf, name)(col.ptr, out.data_ptr(), size)
    return out[: dt.itemsize].cpu().numpy().view(dt)[0]


def _check(op, got, want, values, valid=None):
    dt = values.dtype
    if dt.kind == "i" or op in ("min", "max"):
        assert (got == want) or (np.isnan(got) and np.isnan(want)), (op, got, want)
        return
    v = values if valid is None else values[valid]
    scale = float(np.sum(np.abs(v.astype(np.float64)) ** (2 if op == "sum_squared" else 1))) + 1.0
    if op == "product":              # accumulated in the input type, in another order than numpy's: relative error ~ n * eps
        tol = (1e-3 if dt == np.float32 else 1e-10) * (abs(float(want)) + 1e-30)
    elif dt == np.float32:
        # the kernel accumulates in f64 and rounds once, as the reference value does: both f64 sums are within n * 2^-53 * scale of
        # the true sum, so within n * 2^-52 * scale of each other, and each rounding to f32 adds half an ulp of the result
        tol = float(np.spacing(np.float32(abs(float(want))))) + len(v) * 2.0 ** -52 * (scale - 1.0)
    else:
        tol = 1e-12 * scale
    assert abs(float(got) - float(want)) <= tol, (op, got, want)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n", [1, 2, 3, 127, 128, 129, 200, 10000])
def test_reductions_replay(gdf, dtype, n):
    from libgdf_amd.columns import column_from_numpy
    for op in _ops_for(dtype):
        a = _values(op, dtype, n)
        col = column_from_numpy(a)
        _check(op, _run(gdf, op, col, dtype), reduce_rule(op, a), a)
        _check(op, _run(gdf, op, col, dtype, typed=True), reduce_rule(op, a), a)
        valid = np.random.random(n) < 0.5
        mcol = column_from_numpy(a, valid)
        _check(op, _run(gdf, op, mcol, dtype), reduce_rule(op, a, valid), a, valid)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_empty_and_all_null_give_the_identity(gdf, dtype):
    import torch
    from libgdf_amd.columns import Column, column_from_numpy
    dt = np.dtype(dtype)
    for op in _ops_for(dtype):
        empty = Column(torch.zeros(0, dtype=getattr(torch, {"int8": "int8", "int32": "int32", "int64": "int64", "float32": "float32",
                                                            "float64": "float64"}[dt.name]), device="cuda"))
        got = _run(gdf, op, empty, dtype)
        assert got.tobytes() == reduce_identity(op, dt).tobytes(), (op, got)
        a = _values(op, dtype, 1000)
        nulls = column_from_numpy(a, np.zeros(1000, dtype=bool))
        got = _run(gdf, op, nulls, dtype)
        assert got.tobytes() == reduce_identity(op, dt).tobytes(), (op, got)


def test_integer_wrap_around(gdf):
    from libgdf_amd.columns import column_from_numpy
    assert _run(gdf, "sum", column_from_numpy(np.array([100, 100], dtype=np.int8)), np.int8) == np.int8(-56)
    assert _run(gdf, "sum", column_from_numpy(np.full(1000, 127, dtype=np.int8)), np.int8) == np.int8((127 * 1000 + 128) % 256 - 128)
    assert _run(gdf, "product", column_from_numpy(np.array([65536, 65536, 3], dtype=np.int32)), np.int32) == 0
    assert _run(gdf, "product", column_from_numpy(np.array([2**31 - 1, 2], dtype=np.int32)), np.int32) == np.int32(-2)
    big = np.full(5, np.iinfo(np.int64).max, dtype=np.int64)
    assert _run(gdf, "sum", column_from_numpy(big), np.int64) == reduce_rule("sum", big)
    a = np.random.randint(-128, 128, 100000).astype(np.int8)
    for op in ("sum", "product"):
        assert _run(gdf, op, column_from_numpy(a), np.int8) == reduce_rule(op, a)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_nan_and_inf(gdf, dtype):
    from libgdf_amd.columns import column_from_numpy
    dt = np.dtype(dtype)
    a = np.random.random(5000).astype(dt)
    a[1234] = np.nan
    col = column_from_numpy(a)
    for op in ("min", "max", "sum", "product", "sum_squared"):
        assert np.isnan(_run(gdf, op, col, dtype)), op
    valid = np.ones(5000, dtype=bool)
    valid[1234] = False                       # a null NaN does not count
    mcol = column_from_numpy(a, valid)
    assert _run(gdf, "min", mcol, dtype) == reduce_rule("min", a, valid)
    assert _run(gdf, "max", mcol, dtype) == reduce_rule("max", a, valid)
    b = np.array([1.0, np.inf, 2.0], dtype=dt)
    assert _run(gdf, "sum", column_from_numpy(b), dtype) == np.inf
    assert _run(gdf, "max", column_from_numpy(b), dtype) == np.inf
    c = np.array([np.inf, -np.inf], dtype=dt)
    assert np.isnan(_run(gdf, "sum", column_from_numpy(c), dtype))
    # the identities are +-FLT_MAX / +-DBL_MAX and take part: min of +inf alone is the identity
    assert _run(gdf, "min", column_from_numpy(np.array([np.inf], dtype=dt)), dtype) == np.finfo(dt).max
    assert _run(gdf, "max", column_from_numpy(np.array([-np.inf], dtype=dt)), dtype) == np.finfo(dt).min


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("offset", [1, 2, 3])
def test_unaligned_slices(gdf, dtype, offset):
    import torch
    from libgdf_amd.columns import Column, mask_from_bools
    n = 100003
    for op in _ops_for(dtype):
        a = _values(op, dtype, n + offset)
        t = torch.from_numpy(a).cuda()
        view = a[offset:]
        valid = np.random.random(n) < 0.7
        col = Column(t[offset:], torch.from_numpy(mask_from_bools(valid)).cuda(), null_count=int(n - valid.sum()))
        _check(op, _run(gdf, op, col, dtype), reduce_rule(op, view, valid), view, valid)
        col = Column(t[offset:])
        _check(op, _run(gdf, op, col, dtype), reduce_rule(op, view), view)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_tile_and_grid_boundaries(gdf, dtype):
    from libgdf_amd.columns import column_from_numpy
    v = 16 // np.dtype(dtype).itemsize
    tile = 256 * 4 * v                                      # one workgroup's 16-B vectors per trip
    ncu = 256
    sizes = [v - 1, v, v + 1, tile - 1, tile, tile + 1, 2 * tile + 7, ncu * 4 * tile - 1, ncu * 4 * tile, ncu * 4 * tile + 1,
             ncu * 4 * tile * 2 + 5]
    for n in sizes:
        a = _values("sum", dtype, n)
        valid = np.random.random(n) < 0.9
        for op in ("sum", "max"):
            _check(op, _run(gdf, op, column_from_numpy(a), dtype), reduce_rule(op, a), a)
            _check(op, _run(gdf, op, column_from_numpy(a, valid), dtype), reduce_rule(op, a, valid), a, valid)


def test_bit_identical_results(gdf):
    import torch
    from libgdf_amd.columns import column_from_numpy
    for dtype in (np.float32, np.float64):
        a = (np.random.standard_normal(3_000_001) * 1e3).astype(dtype)
        col = column_from_numpy(a)
        for op in ("sum", "sum_squared", "product"):
            seen = set()
            for size in (1, 128, 1000, 1, 128, 1000, 1, 128, 1000):
                out = torch.zeros(max(size, 1) * 8, dtype=torch.uint8, device="cuda")
                seen.add(_run(gdf, op, col, dtype, size=size, out=out).tobytes())
            assert len(seen) == 1, (dtype, op, seen)


def test_only_the_first_element_of_dev_result_is_written(gdf):
    import torch
    from libgdf_amd.columns import column_from_numpy
    for dtype in DTYPES:
        dt = np.dtype(dtype)
        a = _values("sum", dtype, 1_000_000)
        col = column_from_numpy(a)
        for op in _ops_for(dtype):
            out = torch.full((128 * dt.itemsize,), 0xA5, dtype=torch.uint8, device="cuda")
            _run(gdf, op, col, dtype, size=128, out=out)
            assert bool((out[dt.itemsize:] == 0xA5).all()), (dt, op)


def test_python_api(gdf):
    from libgdf_amd.columns import column_from_numpy
    a = np.arange(1, 11, dtype=np.int64)
    col = column_from_numpy(a)
    assert gdf.api.reduce("sum", col) == 55 and gdf.api.reduce("product", col) == 3628800
    assert gdf.api.reduce("min", col) == 1 and gdf.api.reduce("max", col) == 10
    r = gdf.api.reduce("sum_squared", column_from_numpy(a.astype(np.float32)))
    assert r == np.float32(385) and r.dtype == np.float32


def test_billion_row_int64_sum(gdf):
    import torch
    from libgdf_amd.columns import Column
    n = 1_000_000_000
    t = torch.arange(n, dtype=torch.int64, device="cuda")
    assert _run(gdf, "sum", Column(t), np.int64) == n * (n - 1) // 2
    del t
    torch.cuda.empty_cache()
