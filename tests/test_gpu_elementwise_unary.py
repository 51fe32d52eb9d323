"""The math functions on the GPU (csrc/elementwise.hip) against numpy.  sqrt, ceil and floor compare with 0 ulp.  The nine
transcendental functions are held to the reference's own bounds (python/tests/test_unaryops.py: 3 ulp for f64, 4 ulp for f32, with
np.testing.assert_array_max_ulp) on inputs drawn as that test draws them -- U(-1, 1), U(0, 1) for log -- and, where DESIGN.md
section 12 records that the device math library keeps the bound there too, on |x| <= 100."""
import numpy as np
import pytest

import elementwise_reference as er
from elementwise_common import BIG, SIZES, Buf, assert_same_bits, col, mask_tensor, offsets, ref
from util import gen_rand

pytestmark = pytest.mark.gpu

ULP = {"f32": 4, "f64": 3}
POSITIVE = ("log", "sqrt")
# |x| <= 100 (DESIGN.md section 12 has the measured maxima); asin / acos have no values outside [-1, 1], log takes (0, 100]
WIDE_OPS = ("sin", "cos", "tan", "atan", "exp", "log")


def _run(gdf, op, sfx, x, generic=False, offs=(0, 0), valid=None, inplace=False):
    npt, dt = er.SUFFIX_NP[sfx], er.SUFFIX_DTYPE[sfx]
    bi = Buf(len(x), npt, offs[0], x)
    bo = bi if inplace else Buf(len(x), npt, offs[1])
    m = mask_tensor(valid)[0] if valid is not None else None
    co = col(bo, dt)
    getattr(gdf.libgdf, f"gdf_{op}_{'generic' if generic else sfx}")(ref(col(bi, dt, m)), ref(co))
    assert co.valid is None
    if not inplace:
        assert np.array_equal(bi.read().view(np.uint8), x.view(np.uint8))
    return bo.read()


def _check(op, sfx, got, x, where=None):
    with np.errstate(all="ignore"):
        want = er.MATH_NP[op](x)
    assert want.dtype == x.dtype
    if where is not None:
        got, want = got[where], want[where]
    if op in er.EXACT_MATH_OPS:
        assert_same_bits(got, want)
    else:
        print(op, sfx, "max ulp", np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)))
        np.testing.assert_array_max_ulp(want, got, maxulp=ULP[sfx])


def _reference_draw(op, sfx, n):
    x = gen_rand(er.SUFFIX_NP[sfx], n, positive_only=op in POSITIVE)
    if op in ("ceil", "floor"):
        x = (x * 100).astype(x.dtype)
    return x


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("op", er.MATH_OPS)
def test_every_entry_point_on_the_reference_range(gdf, op, sfx, generic):
    for n in [128] + SIZES:
        x = _reference_draw(op, sfx, n)
        _check(op, sfx, _run(gdf, op, sfx, x, generic), x)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("op", WIDE_OPS + er.EXACT_MATH_OPS)
def test_wider_range(gdf, op, sfx):
    n = 2**18
    x = ((np.random.random(n) * 2 - 1) * 100).astype(er.SUFFIX_NP[sfx])
    if op in POSITIVE:
        x = np.abs(x) + np.finfo(x.dtype).tiny
    _check(op, sfx, _run(gdf, op, sfx, x), x)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("op", ["sin", "exp", "sqrt", "floor"])
def test_every_misalignment(gdf, op, sfx):
    n = 333
    x = _reference_draw(op, sfx, n)
    for i in offsets(x.dtype.itemsize):
        for o in offsets(x.dtype.itemsize):
            _check(op, sfx, _run(gdf, op, sfx, x, offs=(i, o)), x)
    for i in offsets(x.dtype.itemsize):
        _check(op, sfx, _run(gdf, op, sfx, x, offs=(i, 0), inplace=True), x)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("op", ["cos", "log", "ceil"])
def test_masked_input_only_valid_rows_are_compared(gdf, op, sfx):
    n = 2**16 + 9
    x = _reference_draw(op, sfx, n)
    valid = np.random.rand(n) < 0.6
    x[~valid] = np.nan                                                   # whatever sits at a null row must not matter
    _check(op, sfx, _run(gdf, op, sfx, x, generic=True, valid=valid), x, valid)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_specials(gdf, sfx):
    dt = er.SUFFIX_NP[sfx]
    x = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 2.5, -2.5, np.finfo(dt).tiny / 2, 4.0, 1e30], dtype=dt)
    for op in er.MATH_OPS:
        got = _run(gdf, op, sfx, x)
        with np.errstate(all="ignore"):
            want = er.MATH_NP[op](x)
        assert np.array_equal(np.isnan(got), np.isnan(want)), op
        assert np.array_equal(np.isinf(got), np.isinf(want)), op
        if op in er.EXACT_MATH_OPS:
            assert_same_bits(got, want)                                  # -0.0 stays -0.0, sqrt(-0.0) is -0.0
        else:
            fin = np.isfinite(want) & (np.abs(x) <= 100)
            np.testing.assert_array_max_ulp(want[fin], got[fin], maxulp=ULP[sfx])


def test_a_large_column_and_determinism(gdf):
    x = np.abs(_reference_draw("sqrt", "f32", BIG)) * 1e6
    first = _run(gdf, "sqrt", "f32", x, offs=(1, 3))
    assert_same_bits(first, np.sqrt(x))
    x = _reference_draw("sin", "f64", 2**20 + 3)
    a, b = _run(gdf, "sin", "f64", x, offs=(1, 0)), _run(gdf, "sin", "f64", x, offs=(1, 0))
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_python_unary_op(gdf):
    from libgdf_amd.columns import column_from_numpy
    x = _reference_draw("exp", "f64", 1003)
    valid = np.random.rand(1003) < 0.8
    out = gdf.api.unary_op("exp", column_from_numpy(x, valid))
    assert np.array_equal(out.valid_bits(), valid) and out.c.null_count == 1003 - valid.sum()
    np.testing.assert_array_max_ulp(np.exp(x)[valid], out.to_numpy()[valid], maxulp=3)
    with pytest.raises(gdf.GDFError):
        gdf.api.unary_op("sin", column_from_numpy(np.arange(4, dtype=np.int32)))
