"""-m gpu: the VALUE domain of the GDF_SORT group-by (csrc/sort.hip group_by_sort, and its direct-path shortcut in
csrc/groupby.hip group_by_single).

The recipe table of tests/groupby_values.py (type extremes, sums and counts that wrap, exact float grids from the denormals to
2^900, infinities, NaN) through method=GDF_SORT, once served by the direct path and once by the sort (GDF_SORT_NO_DIRECT), exact
against oracle.group_by_sort: ascending keys, the aggregate, and out_col_indices (every group's last row).  SUM / MIN / MAX / AVG
live in the input dtype (sqls_rtti_comp.hpp:487-662), COUNT in every output dtype (sqls_ops.cu:272-400).  MIN / MAX of a group
mixing NaN with numbers is left to the row order by the reference: NaN or the min / max of the numbers."""
import numpy as np
import pytest

import groupby_values as gv
from oracle import oracle

pytestmark = pytest.mark.gpu
IDS = lambda d: np.dtype(d).name
MIXED_NAN = ("nan_pos_mixed", "nan_neg_mixed")


def _run(gdf, op, lay, out):
    from libgdf_amd.columns import GDF_SORT, column_from_numpy, get_dtype
    od = None if out is None else get_dtype(out)
    k, a, i = gdf.api.group_by(op, [column_from_numpy(c) for c in lay.keys], column_from_numpy(lay.vals), out_dtype=od, method=GDF_SORT,
                               with_indices=True)
    return [x.cpu().numpy() for x in k], a.cpu().numpy(), i.cpu().numpy()


def _check_sort(gdf, force_path, op, dt, out=None):
    recs = [r for r in gv.recipes(dt, op) if op != "avg" or gv.avg_defined(r.values, dt, dt)]
    if op in ("min", "max") and np.dtype(dt).kind == "f":
        recs = recs + [r for r in gv.recipes(dt) if r.name in MIXED_NAN]           # membership check only
    lay = gv.layout("direct", recs, np.random.default_rng(8))
    ek, ea, ei = oracle.group_by_sort(op, lay.keys, lay.vals, out)
    mixed = np.zeros(len(ea), dtype=bool)
    for r, key in zip(recs, lay.key_of_recipe):
        if r.name in MIXED_NAN and op in ("min", "max"):
            mixed[int(np.searchsorted(ek[0], key))] = True
    for direct in (True, False):
        force_path("GDF_SORT_NO_DIRECT", None if direct else "1")
        got = {}
        names = gv.kernels_of(gdf, lambda: got.update(r=_run(gdf, op, lay, out)))
        gk, ga, gi = got["r"]
        assert ("gb_direct_aggregate" in names) == direct and ("gb_direct_last_rows" in names) == direct and names, sorted(names)
        assert ga.dtype == ea.dtype == np.dtype(dt if out is None else out)
        np.testing.assert_array_equal(gk[0], ek[0])                                     # ascending, no sorting here
        np.testing.assert_array_equal(gi, ei)
        np.testing.assert_array_equal(ga[~mixed], ea[~mixed], err_msg=f"{op} {np.dtype(dt).name} direct={direct}")
        for r, key in zip(recs, lay.key_of_recipe):
            i = int(np.searchsorted(ek[0], key))
            if mixed[i]:
                nums = r.values[~np.isnan(r.values)]
                assert np.isnan(ga[i]) or ga[i] == (nums.min() if op == "min" else nums.max()), (r.name, ga[i])
    force_path("GDF_SORT_NO_DIRECT", None)


@pytest.mark.parametrize("op", ["sum", "min", "max", "avg"])
@pytest.mark.parametrize("dt", gv.VALUE_DTYPES, ids=IDS)
def test_sort_method_recipe_table(gdf, force_path, op, dt):
    _check_sort(gdf, force_path, op, dt)


@pytest.mark.parametrize("out", gv.VALUE_DTYPES, ids=IDS)
def test_sort_method_count_typing(gdf, force_path, out):
    """COUNT in all six output dtypes over groups of 1 .. 65536 rows (int8 wraps from 128, int16 from 32768)"""
    _check_sort(gdf, force_path, "count", np.int32, out)
