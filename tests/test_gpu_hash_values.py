"""-m gpu: gdf_hash over the whole value domain, bit-exact against the numpy reference of hash_partition_cases.py: every dtype's
recipes (type extremes, 64-bit values with varied high words, +-0.0, +-inf, quiet and signalling NaN with payload bits, denormals)
under Murmur3, the integer and float recipes under the identity hash (the hardware conversion truncates, saturates and sends NaN
and negatives to 0), a five-column mixed key; n = 1, 63, 64, 65 and one size beyond a grid stride."""
import numpy as np
import pytest

import hash_partition_cases as hp

pytestmark = pytest.mark.gpu

DTYPES = [np.int8, np.int16, np.int32, np.int64, np.float32, np.float64]
BEYOND_GRID = 256 * 8 * 2048 + 4099           # csrc/common.h stream_grid: at most 2048 blocks of 256 threads x 8 rows


def _hash(gdf, cols, hash_func):
    from libgdf_amd.columns import column_from_numpy
    return gdf.api.hash_rows([column_from_numpy(c) for c in cols], hash_func=hash_func).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("hash_func", [hp.MURMUR3, hp.IDENTITY], ids=["murmur3", "identity"])
def test_hash_value_recipes(gdf, dtype, hash_func):
    ident = hash_func == hp.IDENTITY
    sp = hp.specials(dtype, ident)
    np.testing.assert_array_equal(_hash(gdf, [sp], hash_func), hp.hash_rows([sp], hash_func))
    for n in (1, 63, 64, 65, 100003):
        a = hp.fill(dtype, n, n, ident)
        np.testing.assert_array_equal(_hash(gdf, [a], hash_func), hp.hash_rows([a], hash_func))


@pytest.mark.parametrize("hash_func", [hp.MURMUR3, hp.IDENTITY], ids=["murmur3", "identity"])
def test_hash_five_column_mixed_key_and_grid_stride(gdf, hash_func):
    ident = hash_func == hp.IDENTITY
    for n in (1, 63, 64, 65, BEYOND_GRID):
        cols = [hp.fill(dt, n, 40 + i, ident) for i, dt in enumerate((np.int32, np.float64, np.int8, np.float32, np.int64))]
        np.testing.assert_array_equal(_hash(gdf, cols, hash_func), hp.hash_rows(cols, hash_func))
    a = hp.fill(np.int16, BEYOND_GRID, 3, ident)
    np.testing.assert_array_equal(_hash(gdf, [a], hash_func), hp.hash_rows([a], hash_func))
