"""Binary arithmetic, comparisons and bit operations on the GPU (csrc/elementwise.hip) against numpy (elementwise_reference.py): every
entry point typed and _generic, sizes across the run / tile boundaries, every misalignment of each of the three pointers, masks, in-place
output, wrap-around, NaN / inf / signed zeros, division by zero, the guard bytes around the output, and determinism.  Everything here
compares with 0 ulp."""
import numpy as np
import pytest

import elementwise_reference as er
from elementwise_common import BIG, SIZES, Buf, assert_same_bits, col, mask_tensor, offsets, ref

pytestmark = pytest.mark.gpu

NAMES = [(op, sfx) for op, sfxs in er.BINARY_SUFFIXES.items() for sfx in sfxs]


def _values(np_dtype, n, op, seed=0):
    rng = np.random.RandomState(seed + n % 1000)
    dt = np.dtype(np_dtype)
    if dt.kind == "f":
        x = ((rng.random_sample(n) * 2 - 1) * 10.0 ** rng.randint(-3, 4, n)).astype(dt)
        if op in er.COMPARE_OPS:
            x = np.round(x, 1).astype(dt)                                # ties happen
        return x
    info = np.iinfo(dt)
    if op in er.COMPARE_OPS:
        return rng.randint(-3, 4, n).astype(dt)
    return rng.randint(info.min, int(info.max) + 1, size=n, dtype=np.int64).astype(dt)      # full range: add / sub / mul wrap


def _run(gdf, op, sfx, a, b, generic=False, offs=(0, 0, 0), va=None, vb=None, inplace=None):
    """-> (output elements, rows that are valid in both inputs)"""
    np_in = er.SUFFIX_NP[sfx]
    dt = er.SUFFIX_DTYPE[sfx]
    np_out, out_dt = (np.int8, er.INT8) if op in er.COMPARE_OPS else (np_in, dt)
    n = len(a)
    ba, bb = Buf(n, np_in, offs[0], a), Buf(n, np_in, offs[1], b)
    bo = {None: None, "lhs": ba, "rhs": bb}[inplace] or Buf(n, np_out, offs[2])
    ma = mask_tensor(va)[0] if va is not None else None
    mb = mask_tensor(vb)[0] if vb is not None else None
    ca, cb, co = col(ba, dt, ma), col(bb, dt, mb), col(bo, out_dt)
    getattr(gdf.libgdf, f"gdf_{op}_{'generic' if generic else sfx}")(ref(ca), ref(cb), ref(co))
    assert co.valid is None and co.null_count == 0                       # the library leaves both alone
    both = np.ones(n, dtype=bool)
    for v in (va, vb):
        if v is not None:
            both &= v
    got = bo.read()
    if inplace != "lhs":
        assert np.array_equal(ba.read().view(np.uint8), a.view(np.uint8))
    if inplace != "rhs":
        assert np.array_equal(bb.read().view(np.uint8), b.view(np.uint8))
    return got, both


def _specified(op, a, b):
    if op == "floordiv" and a.dtype.kind == "i":
        return er.floordiv_specified(a, b)
    return np.ones(len(a), dtype=bool)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("op,sfx", NAMES)
def test_every_entry_point_and_size(gdf, op, sfx, generic):
    for n in SIZES:
        a, b = _values(er.SUFFIX_NP[sfx], n, op, 1), _values(er.SUFFIX_NP[sfx], n, op, 2)
        got, _ = _run(gdf, op, sfx, a, b, generic)
        assert_same_bits(got, er.binary(op, a, b), _specified(op, a, b))


@pytest.mark.parametrize("op", ["gt", "eq"])
@pytest.mark.parametrize("dtype", [er.DATE32, er.DATE64, er.TIMESTAMP])
def test_generic_comparisons_take_dates(gdf, op, dtype):
    npt = er.STORAGE[dtype]
    n = 1000
    a, b = _values(npt, n, op, 1), _values(npt, n, op, 2)
    ba, bb, bo = Buf(n, npt, 0, a), Buf(n, npt, 0, b), Buf(n, np.int8)
    getattr(gdf.libgdf, f"gdf_{op}_generic")(ref(col(ba, dtype)), ref(col(bb, dtype)), ref(col(bo, er.INT8)))
    assert_same_bits(bo.read(), er.binary(op, a, b))


@pytest.mark.parametrize("op,sfx", [("add", "f64"), ("sub", "i32"), ("mul", "i64"), ("lt", "i64"), ("ne", "f32"), ("ge", "i8"),
                                    ("bitwise_xor", "i8"), ("bitwise_and", "i32"), ("floordiv", "f32"), ("div", "f64"), ("le", "f64"),
                                    ("eq", "i32")])
def test_every_misalignment_of_each_pointer(gdf, op, sfx):
    """lhs, rhs and the output move independently over every element offset against 16 bytes, at a size with head, body and tail"""
    np_in = np.dtype(er.SUFFIX_NP[sfx])
    np_out = np.dtype(np.int8) if op in er.COMPARE_OPS else np_in
    n = 777
    a, b = _values(np_in, n, op, 1), _values(np_in, n, op, 2)
    want = er.binary(op, a, b)
    # all triples would be up to 16^3 launches: every pair with the third at 0 and at an odd offset, plus the full diagonal
    in_offs, out_offs = list(offsets(np_in.itemsize)), list(offsets(np_out.itemsize))
    triples = {(x, y, z) for x in in_offs for y in in_offs for z in (0, out_offs[-1])}
    triples |= {(x, 0, z) for x in in_offs for z in out_offs} | {(0, y, z) for y in in_offs for z in out_offs}
    triples |= {(x, in_offs[-1 - i % len(in_offs)], z) for i, x in enumerate(in_offs) for z in out_offs}
    for t in sorted(triples):
        got, _ = _run(gdf, op, sfx, a, b, offs=t)
        assert_same_bits(got, want)


@pytest.mark.parametrize("masks", ["neither", "lhs", "rhs", "both"])
@pytest.mark.parametrize("op,sfx", [("add", "i32"), ("mul", "f64"), ("lt", "i64"), ("bitwise_or", "i8"), ("floordiv", "i64")])
def test_masks_only_valid_rows_are_compared(gdf, op, sfx, masks):
    for n in (17, 1000, 2**16 + 9):
        a, b = _values(er.SUFFIX_NP[sfx], n, op, 3), _values(er.SUFFIX_NP[sfx], n, op, 4)
        va = np.random.RandomState(5).rand(n) < 0.7 if masks in ("lhs", "both") else None
        vb = np.random.RandomState(6).rand(n) < 0.7 if masks in ("rhs", "both") else None
        got, both = _run(gdf, op, sfx, a, b, generic=True, va=va, vb=vb)
        assert_same_bits(got, er.binary(op, a, b), both & _specified(op, a, b))


@pytest.mark.parametrize("inplace", ["lhs", "rhs"])
@pytest.mark.parametrize("op,sfx", [("add", "f64"), ("sub", "i64"), ("mul", "i32"), ("eq", "i8"), ("bitwise_and", "i64"), ("div", "f32")])
def test_in_place_output(gdf, op, sfx, inplace):
    for n, off in ((1, 0), (65, 1), (1000, 0), (2**20 + 3, 1)):
        a, b = _values(er.SUFFIX_NP[sfx], n, op, 7), _values(er.SUFFIX_NP[sfx], n, op, 8)
        got, _ = _run(gdf, op, sfx, a, b, offs=(off, 0, 0) if inplace == "lhs" else (0, off, 0), inplace=inplace)
        assert_same_bits(got, er.binary(op, a, b))


@pytest.mark.parametrize("sfx", ["i32", "i64"])
def test_integers_wrap(gdf, sfx):
    dt = er.SUFFIX_NP[sfx]
    info = np.iinfo(dt)
    a = np.array([info.max, info.min, info.max, info.min, -1, info.max // 2 + 1] * 11, dtype=dt)
    b = np.array([1, -1, info.max, info.min, info.min, 2] * 11, dtype=dt)
    for op in ("add", "sub", "mul"):
        got, _ = _run(gdf, op, sfx, a, b)
        want = [((int(x) + int(y) if op == "add" else int(x) - int(y) if op == "sub" else int(x) * int(y)) + 2**(info.bits - 1))
                % 2**info.bits - 2**(info.bits - 1) for x, y in zip(a, b)]
        assert got.tolist() == want


@pytest.mark.parametrize("sfx", ["i32", "i64"])
def test_integer_floordiv_is_exact_and_never_faults(gdf, sfx):
    dt = er.SUFFIX_NP[sfx]
    info = np.iinfo(dt)
    rng = np.random.RandomState(11)
    a = np.concatenate([np.array([7, -7, 7, -7, info.min, info.min, info.max, 5, 0, info.max - 1, info.min + 1], dtype=dt),
                        rng.randint(info.min, int(info.max) + 1, size=5000, dtype=np.int64).astype(dt)])
    b = np.concatenate([np.array([2, 2, -2, -2, -1, 0, 0, 0, 0, 3, -3], dtype=dt),
                        rng.randint(-50, 50, size=5000).astype(dt)])
    got, _ = _run(gdf, "floordiv", sfx, a, b)
    spec = er.floordiv_specified(a, b)
    assert (~spec).sum() >= 5                                            # rhs == 0 and INT_MIN / -1 are in there: the call returned
    assert got[spec].tolist() == [int(x) // int(y) for x, y in zip(a[spec], b[spec])]      # exact also beyond 2^53


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_float_specials(gdf, sfx):
    dt = er.SUFFIX_NP[sfx]
    tiny = np.finfo(dt).tiny
    s = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, tiny, -tiny / 4, np.finfo(dt).max, 1e-3, 3.0], dtype=dt)
    a, b = np.repeat(s, len(s)), np.tile(s, len(s))
    for op in ("add", "sub", "mul", "div", "floordiv") + er.COMPARE_OPS:
        got, _ = _run(gdf, op, sfx, a, b)
        want = er.binary(op, a, b)
        assert_same_bits(got, want)                                      # signed zeros and subnormals bit for bit
        if op in er.COMPARE_OPS:
            nan = np.isnan(a) | np.isnan(b)
            assert (got[nan] == (1 if op == "ne" else 0)).all()


def test_a_large_column(gdf):
    n = BIG
    a, b = _values(np.int8, n, "bitwise_xor", 1), _values(np.int8, n, "bitwise_xor", 2)
    got, _ = _run(gdf, "bitwise_xor", "i8", a, b, offs=(3, 3, 3))
    assert_same_bits(got, a ^ b)
    a, b = a.astype(np.int32) * 1000003, b.astype(np.int32) * 77
    got, _ = _run(gdf, "lt", "i32", a, b, offs=(1, 2, 5))
    assert_same_bits(got, (a < b).astype(np.int8))


@pytest.mark.parametrize("op,sfx", [("add", "f32"), ("div", "f64"), ("lt", "i64"), ("mul", "i32")])
def test_a_second_call_is_bit_identical(gdf, op, sfx):
    n = 2**20 + 3
    a, b = _values(er.SUFFIX_NP[sfx], n, op, 1), _values(er.SUFFIX_NP[sfx], n, op, 2)
    first, _ = _run(gdf, op, sfx, a, b, offs=(1, 0, 1))
    second, _ = _run(gdf, op, sfx, a, b, offs=(1, 0, 1))
    assert np.array_equal(first.view(np.uint8), second.view(np.uint8))


def test_python_binary_op(gdf):
    from libgdf_amd.columns import column_from_numpy
    n = 1003
    a, b = _values(np.float64, n, "add", 1), _values(np.float64, n, "add", 2)
    va, vb = np.random.rand(n) < 0.8, np.random.rand(n) < 0.8
    out = gdf.api.binary_op("add", column_from_numpy(a, va), column_from_numpy(b, vb))
    assert np.array_equal(out.valid_bits(), va & vb) and out.c.null_count == n - (va & vb).sum()
    assert_same_bits(out.to_numpy(), a + b, va & vb)
    out = gdf.api.binary_op("le", column_from_numpy(a), column_from_numpy(b))
    assert out.valid is None and out.c.dtype == er.INT8
    assert_same_bits(out.to_numpy(), (a <= b).astype(np.int8))
    with pytest.raises(ValueError):
        gdf.api.binary_op("pow", column_from_numpy(a), column_from_numpy(b))
