"""gdf_amd_dist_group_by_multi with ONE real rank among scripted numpy peers (tests/dist_world.py): one to three key columns of mixed
dtypes (one of them float64), masks on any subset of the key columns and on the values, groups without a valid value on any rank,
groups valid on one sender only, COUNT with masks, AVG over int and float values; worlds of 1, 2, 3, 5 and 8 ranks, both exchange
layouts.  The reference is oracle.group_by_masked over the concatenated shards; Device.group_by_multi also checks null_count, that
the aggregate is 0 under a cleared bit and that the mask bits behind the last group are 0."""
import numpy as np
import pytest

import dist_cases as dc
import dist_world as dw
from dist_world import Device, GroupByMultiModel, positions, run_owner_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rank(gdf):
    return Device(gdf)


@pytest.mark.parametrize("case", dc.MULTI_CASES, ids=lambda c: "-".join([c[0], *c[1], c[4]]))
def test_keys_masks_and_values(rank, case):
    for world in dw.WORLDS:
        for shape in range(len(dc.SHAPES[world])):
            shards = dc.multi_shards(world, shape, case)
            model = GroupByMultiModel(case[0], [dw.NP_OF[k] for k in case[1]], dw.NP_OF[case[4]])
            sends = [model.send(s, world) for s in shards]
            for real in positions(world):
                for with_v in (False, True):
                    run_owner_call(model, shards, sends, world, real, with_v, rank, lambda m, sh, tr: rank.group_by_multi(m, sh, tr, key_gdfs=case[1]))


@pytest.mark.parametrize("rows", dc.OWNER_ROWS)
@pytest.mark.parametrize("op", ["sum", "avg"])
def test_rows_at_the_owner_around_the_mask_bytes(rank, rows, op):
    """exactly 1, 7, 8, 9, 63, 64 and 65 partial rows reach the real rank: the bytes and the padded tail of dg_mask_from_counts"""
    for world in dc.OWNER_ROWS_WORLDS:
        for real in positions(world):
            shards = dc.owner_rows_shards(world, real, rows)
            model = GroupByMultiModel(op, [np.int64], np.int32)
            sends = [model.send(s, world) for s in shards]
            assert sum(len(sends[s][real][0]) for s in range(world)) == rows
            for with_v in (False, True):
                w = run_owner_call(model, shards, sends, world, real, with_v, rank, rank.group_by_multi)
                x = w.done[0]
                assert int(x.real_counts[real]) + sum(len(x.to_real[s][0]) for s in x.to_real) == rows
