"""gdf_amd_dist_gather with ONE real rank among scripted numpy peers (tests/dist_world.py): columns of every width (int8, int16,
int32, DATE32, float32, int64, TIMESTAMP, float64) with and without masks, 16 columns in one call, ids in random order with
repeats, -1 and ids of every owner, a rank that asks for nothing and a rank nobody asks anything of; ids->size of 1, 7, 8, 9, 63,
64, 65 and 2049 (the bytes and words of dg_pack).  Per call: (a) the requests sent to every owner and -- in the order the peers
asked, flag by flag and value by value -- the answers sent back, row 0, the last row and a masked row included; (b, c) the rows the
ids name.  Device.gather checks that every output carries a mask, its null_count and that the bits behind the last row are 0."""
import pytest

import dist_cases as dc
import dist_world as dw
from dist_world import Device, GatherModel, positions, run_gather

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rank(gdf):
    return Device(gdf)


def sweep(rank, names, masked, worlds=dw.WORLDS):
    model = GatherModel([dw.NP_OF[n] for n in names])
    for world in worlds:
        for shape in range(len(dc.GATHER_SHAPES[world])):
            shards = dc.gather_shards(world, shape, names, masked)
            for real in positions(world):
                for with_v in (False, True):
                    run_gather(model, shards, world, real, with_v, rank, lambda m, sh, tr: rank.gather(m, sh, tr, col_gdfs=names))


@pytest.mark.parametrize("names, masked", dc.GATHER_CASES, ids=lambda v: "-".join(str(x) for x in v) if len(v) < 3 else f"{len(v)}cols")
def test_every_column_width_with_and_without_masks(rank, names, masked):
    """one column of every width, plain and masked, and 16 columns in one call"""
    sweep(rank, names, masked)
