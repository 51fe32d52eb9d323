"""-m gpu: gdf_amd_gather (csrc/order.hip) against tests/order_reference.py -- data, mask words, null counts compared exactly -- and
the chain the entry exists for: read_csv -> gdf_amd_order_by_ex -> gdf_amd_gather, and the index columns of gdf_left_join."""
import ctypes as C

import numpy as np
import pytest

import order_reference as orf

pytestmark = pytest.mark.gpu

GDF_INVALID_API_CALL = 8
M_VALUES = [0, 1, 63, 64, 65, 1000]
PATTERNS = ["identity", "reverse", "repeats", "all_minus_one", "minus_one_around_64"]
WIDTHS = [("int8", np.int8, 1), ("int16", np.int16, 2), ("int32", np.int32, 3), ("float32", np.float32, 5), ("int64", np.int64, 4),
          ("float64", np.float64, 6)]


def make_indices(pattern, m, rows, rng, dtype):
    if pattern == "identity":
        idx = np.arange(m) % rows
    elif pattern == "reverse":
        idx = (rows - 1 - np.arange(m)) % rows
    elif pattern == "repeats":
        idx = rng.integers(0, min(rows, 5), size=m)
    elif pattern == "all_minus_one":
        idx = np.full(m, -1)
    else:
        idx = rng.integers(0, rows, size=m)
        for k in range(0, m + 64, 64):                         # -1 at every 64th position plus or minus 1
            for p in (k - 1, k, k + 1):
                if 0 <= p < m:
                    idx[p] = -1
    return idx.astype(dtype)


def sources(rows, rng):
    """one column per width class with a mask, one without; NaN / -0.0 / extremes among the values"""
    cols = []
    for name, npt, _ in WIDTHS:
        if np.dtype(npt).kind == "f":
            x = rng.standard_normal(rows).astype(npt)
            x[:4] = [np.nan, -0.0, np.inf, np.finfo(npt).max]
        else:
            info = np.iinfo(npt)
            x = rng.integers(info.min, info.max, size=rows, dtype=npt, endpoint=True)
            x[:2] = [info.min, info.max]
        cols.append((x, rng.random(rows) < 0.7))
        cols.append((x[::-1].copy(), None))
    return cols


def run(gdf, idx, cols, dtypes=None, time_units=None):
    import torch
    cs = [orf.device_column(d, v, None if dtypes is None else dtypes[i], None if time_units is None else time_units[i])
          for i, (d, v) in enumerate(cols)]
    return gdf.api.gather(torch.from_numpy(idx).cuda(), cs)


def check(gdf, idx, cols, what=""):
    outs = run(gdf, idx, cols)
    want = orf.gather(idx, cols)
    m = len(idx)
    assert len(outs) == len(cols)
    for c, (o, (data, ok, mask, nulls), (src, _)) in enumerate(zip(outs, want, cols)):
        assert o.size == m and int(o.c.null_count) == nulls, (what, c, int(o.c.null_count), nulls)
        got = o.data.cpu().numpy()
        assert got.dtype == src.dtype
        np.testing.assert_array_equal(orf.bits_of(got), orf.bits_of(data), err_msg=f"{what}: data of column {c}")        # 0 at null rows
        got_mask = o.valid.cpu().numpy()
        assert len(got_mask) == (m + 63) // 64 * 8
        np.testing.assert_array_equal(got_mask, mask, err_msg=f"{what}: mask of column {c}")                            # tail bits zero
    return outs


@pytest.mark.parametrize("idx_dtype", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("m", M_VALUES)
def test_indices(gdf, m, pattern, idx_dtype):
    """twelve source columns (every width, with and without a mask: three batches of the kernel) by every index pattern"""
    rng = np.random.default_rng(m * 11 + len(pattern))
    rows = 777
    check(gdf, make_indices(pattern, m, rows, rng, idx_dtype), sources(rows, rng), what=f"m={m} {pattern}")


def test_more_outputs_than_sources_and_no_source_rows(gdf):
    rng = np.random.default_rng(2)
    check(gdf, make_indices("repeats", 5000, 4, rng, np.int32), sources(4, rng)[:3], what="four source rows")
    check(gdf, make_indices("minus_one_around_64", 100_000, 300, rng, np.int64), sources(300, rng)[4:6], what="100000 from 300")
    empty = [(np.zeros(0, dtype=np.int64), np.zeros(0, dtype=bool)), (np.zeros(0, dtype=np.int8), None)]
    check(gdf, np.full(70, -1, dtype=np.int32), empty, what="no source rows, all -1")


def test_dtype_and_time_unit_are_carried_over(gdf):
    rng = np.random.default_rng(3)
    rows = 100
    stamps = rng.integers(0, 1 << 50, size=rows, dtype=np.int64)
    days = rng.integers(0, 20000, size=rows).astype(np.int32)
    idx = make_indices("minus_one_around_64", 130, rows, rng, np.int32)
    outs = run(gdf, idx, [(stamps, rng.random(rows) < 0.5), (days, None), (stamps, None)], dtypes=[9, 7, 8], time_units=["us", None, None])
    assert [int(o.c.dtype) for o in outs] == [9, 7, 8]
    assert [int(o.c.dtype_info.time_unit) for o in outs] == [3, 0, 0]
    for m in (0,):                                               # ... also when nothing is gathered
        outs = run(gdf, np.zeros(m, dtype=np.int64), [(stamps, None)], dtypes=[9], time_units=["ns"])
        assert (int(outs[0].c.dtype), int(outs[0].c.dtype_info.time_unit), outs[0].size) == (9, 4, 0)


@pytest.mark.parametrize("bad", ["rows", -2, "int64 beyond 2^32"])
def test_bad_indices(gdf, bad):
    """an index of `rows`, one of -2 (and an int64 one whose low half is a valid row): GDF_INVALID_API_CALL, found on the device;
    the output structs are untouched and nothing stays allocated"""
    import torch
    from libgdf_amd import GDFError, gdf_column
    from libgdf_amd.columns import Column, column_array
    rng = np.random.default_rng(4)
    rows, m = 500, 1000
    idx = rng.integers(-1, rows, size=m).astype(np.int64 if isinstance(bad, str) and "int64" in bad else np.int32)
    idx[m // 2 + 1] = rows if bad == "rows" else (-2 if bad == -2 else (1 << 32) + 5)
    srcs = [orf.device_column(d, v) for d, v in sources(rows, rng)]
    ic = Column(torch.from_numpy(idx).cuda())

    def free_bytes():
        free, total = C.c_size_t(), C.c_size_t()
        gdf.librmm.rmmGetInfo(C.byref(free), C.byref(total), None)
        return free.value

    def call():
        outs = [gdf_column() for _ in srcs]
        for o in outs:
            C.memset(C.byref(o), 0xAB, C.sizeof(o))
        before = [bytes(C.string_at(C.addressof(o), C.sizeof(o))) for o in outs]
        arr = (C.POINTER(gdf_column) * len(outs))(*[C.pointer(o) for o in outs])
        rc = gdf.libgdf.raw("gdf_amd_gather")(ic.ptr, len(srcs), column_array(srcs), arr)
        assert [bytes(C.string_at(C.addressof(o), C.sizeof(o))) for o in outs] == before
        return rc

    assert call() == GDF_INVALID_API_CALL
    before = free_bytes()
    assert call() == GDF_INVALID_API_CALL
    assert free_bytes() >= before
    with pytest.raises(GDFError):
        gdf.api.gather(ic, srcs)
    idx[m // 2 + 1] = -1                                          # the same call with the index mended succeeds
    check(gdf, idx, sources(rows, np.random.default_rng(4))[:2], what="mended")


def test_gather_is_deterministic(gdf):
    import torch
    rng = np.random.default_rng(6)
    idx = make_indices("minus_one_around_64", 100_000, 5000, rng, np.int32)
    cols = sources(5000, rng)[:4]
    a, b = run(gdf, idx, cols), run(gdf, idx, cols)
    for x, y in zip(a, b):
        assert (x.data.view(torch.uint8) == y.data.view(torch.uint8)).all() and (x.valid == y.valid).all()
        assert int(x.c.null_count) == int(y.c.null_count)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_read_csv_order_by_ex_gather(gdf):
    """CSV bytes -> gdf_amd_read_csv_device (every column comes back with a mask) -> ORDER BY a DESC NULLS LAST, b -> gather: the
    sorted table equals the parsed columns taken in order_reference's order"""
    import torch
    from libgdf_amd import api
    from libgdf_amd.columns import Column
    rng = np.random.default_rng(7)
    n = 5000
    a = rng.integers(-50, 50, size=n)
    b = np.round(rng.standard_normal(n) * 100) / 4
    null_a, null_b = rng.random(n) < 0.1, rng.random(n) < 0.1
    text = "".join(f"{'' if null_a[i] else a[i]},{'' if null_b[i] else b[i]},{i}\n" for i in range(n)).encode()
    dev = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    args = api.csv_args(["a", "b", "row"], ["int32", "float64", "int64"])
    gdf.libgdf.gdf_amd_read_csv_device(dev.data_ptr(), len(text), C.byref(args))
    parsed = api.take_csv_result(args)
    cols, host = [], []
    for name in ("a", "b", "row"):
        data, mask, nulls = parsed[name]
        assert mask.numel() == (n + 7) // 8                      # read_csv: valid is never NULL when rows > 0
        cols.append(Column(data, mask, null_count=nulls))
        host.append((data.cpu().numpy(), np.unpackbits(mask.cpu().numpy(), bitorder="little")[:n].astype(bool)))
    assert (host[0][1] == ~null_a).all() and (host[1][1] == ~null_b).all() and host[2][1].all()
    perm = api.order_by_ex(cols[:2], descending=[True, False])
    want_perm = orf.order_by_ex(host[:2], [True, False])
    np.testing.assert_array_equal(perm.cpu().numpy(), want_perm)
    outs = api.gather(perm, cols)
    for o, (data, ok, mask, nulls) in zip(outs, orf.gather(want_perm, host)):
        np.testing.assert_array_equal(orf.bits_of(o.data.cpu().numpy()), orf.bits_of(data))
        np.testing.assert_array_equal(o.valid.cpu().numpy(), mask)
        assert int(o.c.null_count) == nulls
    np.testing.assert_array_equal(outs[2].data.cpu().numpy(), want_perm)                      # the row column IS the permutation
    sa, va = outs[0].data.cpu().numpy(), outs[0].valid_bits()
    assert (np.diff(sa[va].astype(np.int64)) <= 0).all() and not va[int(va.sum()):].any()       # descending, nulls last


def test_gather_over_left_join_indices_equals_result_cols(gdf):
    """gdf_left_join with result_cols materialises [left non-key, key, right non-key]; gathering the same columns by the join's two
    index columns (-1: no partner) gives the same data where valid, the same masks and null counts"""
    import torch
    from test_gpu_join import _join_with_result_cols
    rng = np.random.default_rng(8)
    nl, nr = 3000, 400
    lkey = rng.integers(0, 800, size=nl).astype(np.int64)
    lpay = rng.standard_normal(nl)
    rkey = rng.permutation(800)[:nr].astype(np.int64)
    rpay = rng.integers(-1000, 1000, size=nr).astype(np.int32)
    lvalid, rvalid = [rng.random(nl) < 0.9, None], [None, rng.random(nr) < 0.8]
    li, ri, res = _join_with_result_cols(gdf, "left", [lpay, lkey], 1, [rkey, rpay], 1 - 1, lvalid, rvalid)
    assert (ri == -1).any() and (ri >= 0).any()
    from_left = run(gdf, li, [(lpay, lvalid[0]), (lkey, None)])
    from_right = run(gdf, ri, [(rpay, rvalid[1])])
    for o, (data, bits) in zip(from_left + from_right, res):
        ok = o.valid_bits()
        np.testing.assert_array_equal(ok, bits)
        np.testing.assert_array_equal(orf.bits_of(o.data.cpu().numpy()[ok]), orf.bits_of(data[ok]))
        assert int(o.c.null_count) == int((~bits).sum())
