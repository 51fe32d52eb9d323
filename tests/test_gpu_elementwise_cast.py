"""The casts on the GPU (csrc/elementwise.hip) against numpy (elementwise_reference.py), 0 ulp: all 72 entry points, sizes across the
run boundaries, every misalignment of both pointers, the fused mask copy, every date / timestamp unit pair with negative values,
out-of-range float -> integer conversions next to valid neighbours, the guard bytes around the output, and determinism."""
import numpy as np
import pytest

import elementwise_reference as er
from elementwise_common import BIG, SIZES, Buf, assert_same_bits, col, mask_tensor, offsets, ref

pytestmark = pytest.mark.gpu

UNITS = (er.UNIT_NONE, er.UNIT_S, er.UNIT_MS, er.UNIT_US, er.UNIT_NS)


def _values(src, n, seed=0):
    rng = np.random.RandomState(seed + n % 1000)
    npt = np.dtype(er.STORAGE[er.SUFFIX_DTYPE[src]])
    if npt.kind == "f":
        return ((rng.random_sample(n) * 2 - 1) * 10.0 ** rng.randint(-2, 3, n)).astype(npt)      # |x| < 100: inside int8
    if src in ("date64", "timestamp"):
        return rng.randint(-2**44, 2**44, size=n, dtype=np.int64)        # negative and positive instants, some days, some decades
    if src == "date32":
        return rng.randint(-110000, 110000, size=n).astype(np.int32)
    info = np.iinfo(npt)
    return rng.randint(info.min, int(info.max) + 1, size=n, dtype=np.int64).astype(npt)


def _run(gdf, src, dst, x, generic=False, from_unit=0, to_unit=0, offs=(0, 0), valid=None, out_valid=True, inplace=False):
    """-> (output elements, output column struct, output mask bytes or None)"""
    import torch
    sdt, ddt = er.SUFFIX_DTYPE[src], er.SUFFIX_DTYPE[dst]
    n = len(x)
    bi = Buf(n, er.STORAGE[sdt], offs[0], x)
    bo = bi if inplace else Buf(n, er.STORAGE[ddt], offs[1])
    mi = mask_tensor(valid)[0] if valid is not None else None
    mo = torch.full(((n + 7) // 8 + 5,), 0xEE, dtype=torch.uint8, device="cuda") if out_valid else None
    ci, co = col(bi, sdt, mi, from_unit), col(bo, er.INT16, mo, er.UNIT_S)
    fn = getattr(gdf.libgdf, f"gdf_cast_{'generic' if generic else src}_to_{dst}")
    fn(ref(ci), ref(co), to_unit) if dst == "timestamp" else fn(ref(ci), ref(co))
    assert co.dtype == ddt and co.dtype_info.time_unit == (to_unit if dst == "timestamp" else er.UNIT_S)
    if not inplace:
        assert np.array_equal(bi.read().view(np.uint8), x.view(np.uint8))
    return bo.read().view(er.STORAGE[ddt]), co, (mo.cpu().numpy() if mo is not None else None)


def _specified(x, dst):
    if x.dtype.kind == "f" and np.dtype(er.STORAGE[er.SUFFIX_DTYPE[dst]]).kind == "i":
        return er.float_to_int_specified(x, er.SUFFIX_DTYPE[dst])
    return None


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("dst", er.CAST_TARGETS)
@pytest.mark.parametrize("src", er.CAST_SOURCES)
def test_every_entry_point_and_size(gdf, src, dst, generic):
    fu = er.UNIT_US if src == "timestamp" else 0
    tu = er.UNIT_MS if dst == "timestamp" else 0
    for n in SIZES:
        x = _values(src, n)
        got, _, _ = _run(gdf, src, dst, x, generic, fu, tu)
        assert_same_bits(got, er.cast(x, er.SUFFIX_DTYPE[src], fu, er.SUFFIX_DTYPE[dst], tu), _specified(x, dst))


def _unit_cases():
    cases = [("date32", 0, "date64", 0), ("date64", 0, "date32", 0)]
    for u in UNITS:
        cases += [("date32", 0, "timestamp", u), ("timestamp", u, "date32", 0), ("date64", 0, "timestamp", u), ("timestamp", u, "date64", 0)]
        cases += [("timestamp", u, "timestamp", v) for v in UNITS]
        cases += [("timestamp", u, "i64", 0), ("i64", 0, "timestamp", u), ("timestamp", u, "f64", 0)]
    return cases


@pytest.mark.parametrize("src,fu,dst,tu", _unit_cases())
def test_every_unit_pair_with_negative_values(gdf, src, fu, dst, tu):
    factor = 86400 * 10**9
    edge = np.array([0, -1, 1, -999, -1000, -1001, 999, 1000, -86400, -86399, -86401, -86400000, -86400001, -factor, -factor - 1, -factor + 1,
                     factor, -10**9, -10**9 - 1, -10**6, -10**6 + 1, 2**62, -2**62], dtype=np.int64)
    x = np.concatenate([_values(src, 5000, 3), edge.astype(er.STORAGE[er.SUFFIX_DTYPE[src]])])
    assert (x < 0).sum() > 2000
    got, _, _ = _run(gdf, src, dst, x, False, fu, tu, offs=(1, 1))
    assert_same_bits(got, er.cast(x, er.SUFFIX_DTYPE[src], fu, er.SUFFIX_DTYPE[dst], tu))


@pytest.mark.parametrize("src,dst", [("i8", "i64"), ("i64", "i8"), ("f64", "i8"), ("i32", "f64"), ("f32", "i32"), ("i64", "f32"), ("i8", "i8"),
                                     ("f64", "f32"), ("date64", "date32"), ("date32", "date64"), ("i32", "i32")])
def test_every_misalignment_of_both_pointers(gdf, src, dst):
    n = 555
    x = _values(src, n, 9)
    want = er.cast(x, er.SUFFIX_DTYPE[src], 0, er.SUFFIX_DTYPE[dst], 0)
    for i in offsets(x.dtype.itemsize):
        for o in offsets(want.dtype.itemsize):
            got, _, _ = _run(gdf, src, dst, x, offs=(i, o))
            assert_same_bits(got, want, _specified(x, dst))


@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 65, 1000, 2**16 + 3])
def test_mask_copy(gdf, n):
    x = _values("i32", n)
    valid = np.random.rand(n) < 0.5
    nb = (n + 7) // 8
    got, co, mo = _run(gdf, "i32", "f64", x, valid=valid)
    assert np.array_equal(mo[:nb], mask_tensor(valid)[1]) and (mo[nb:] == 0xEE).all()      # ceil(n / 8) bytes and no more
    assert_same_bits(got, x.astype(np.float64), valid)
    assert co.null_count == 0                                                             # not the library's to set
    _, _, mo = _run(gdf, "i32", "f64", x, valid=None)                                      # no input mask: the output's is left alone
    assert (mo == 0xEE).all()
    _run(gdf, "i32", "f64", x, valid=valid, out_valid=False)                               # no output mask: nothing to copy into


@pytest.mark.parametrize("src", ["f32", "f64"])
@pytest.mark.parametrize("dst", ["i8", "i32", "i64", "date32", "timestamp"])
def test_out_of_range_floats_return_and_neighbours_are_right(gdf, src, dst):
    x = _values(src, 4096, 5)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 3e9, -3e9, 1e19, 300.0, -300.0], dtype=x.dtype)
    x[::7][: len(bad)] = bad
    got, _, _ = _run(gdf, src, dst, x, to_unit=er.UNIT_S)
    spec = _specified(x, dst)
    assert (~spec).sum() >= 6
    assert_same_bits(got, er.cast(x, er.SUFFIX_DTYPE[src], 0, er.SUFFIX_DTYPE[dst], er.UNIT_S), spec)


@pytest.mark.parametrize("src,dst", [("i64", "f64"), ("f32", "i32"), ("timestamp", "date64"), ("i8", "i8")])
def test_in_place_between_equal_widths(gdf, src, dst):
    for n, off in ((1, 0), (65, 1), (2**20 + 3, 1)):
        x = _values(src, n, 2)
        got, _, _ = _run(gdf, src, dst, x, from_unit=er.UNIT_NS, offs=(off, 0), inplace=True)
        assert_same_bits(got, er.cast(x, er.SUFFIX_DTYPE[src], er.UNIT_NS, er.SUFFIX_DTYPE[dst], 0), _specified(x, dst))


def test_a_large_column_and_determinism(gdf):
    x = _values("i64", BIG, 1)
    got, _, _ = _run(gdf, "i64", "f32", x, offs=(1, 3))
    assert_same_bits(got, x.astype(np.float32))
    x = _values("f64", 2**20 + 3, 1)
    a, _, _ = _run(gdf, "f64", "i8", x, offs=(1, 5))
    b, _, _ = _run(gdf, "f64", "i8", x, offs=(1, 5))
    assert np.array_equal(a, b)


def test_python_cast(gdf):
    from libgdf_amd.columns import column_from_numpy
    x = _values("timestamp", 1003)
    valid = np.random.rand(1003) < 0.8
    c = column_from_numpy(x, valid, dtype=er.TIMESTAMP, time_unit="ms")
    assert c.c.dtype_info.time_unit == er.UNIT_MS
    out = gdf.api.cast(c, "timestamp", time_unit="s")
    assert out.c.dtype == er.TIMESTAMP and out.c.dtype_info.time_unit == er.UNIT_S
    assert np.array_equal(out.valid_bits(), valid) and out.c.null_count == 1003 - valid.sum()
    assert_same_bits(out.to_numpy(), x // 1000, valid)
    out = gdf.api.cast(column_from_numpy(x.astype(np.int32)), "f32")
    assert out.valid is None and out.c.dtype == er.FLOAT32
    assert_same_bits(out.to_numpy(), x.astype(np.int32).astype(np.float32))
    assert column_from_numpy(x).c.dtype_info.time_unit == 0                               # the default is unchanged
