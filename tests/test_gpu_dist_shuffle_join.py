"""gdf_amd_dist_shuffle_join, _left_join and _full_join with ONE real rank among scripted numpy peers (tests/dist_world.py): int32
and int64 keys (negative, beyond 2^32, the ends of the range, many-to-many duplicates), worlds of 1, 2, 3, 5 and 8 ranks, both
exchange layouts.  Per call: (a) the (key, local row) tuples sent to every owner, build side then probe side, (b) the pairs of
global ids (sender << 40 | row, -1 for the missing side) for what the rank received, (c) the world's pairs against oracle.join of
the concatenated shards -- every pair, and every unmatched row of a LEFT / FULL join, exactly once."""
import numpy as np
import pytest

import dist_cases as dc
import dist_world as dw
from dist_world import Device, JoinModel, positions, run_join

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rank(gdf):
    return Device(gdf)


def sends_of(model, shards, world):
    return [model.send_side(s[1], world) for s in shards], [model.send_side(s[0], world) for s in shards]


@pytest.mark.parametrize("key", dc.JOIN_KEYS)
@pytest.mark.parametrize("how", dc.JOIN_HOWS)
def test_every_world(rank, how, key):
    model = JoinModel(how, dw.NP_OF[key])
    for world in dw.WORLDS:
        for shape in range(len(dc.SHAPES[world])):
            shards = dc.join_shards(world, shape, key)
            sends = sends_of(model, shards, world)
            for real in positions(world):
                for with_v in (False, True):
                    run_join(model, shards, world, real, with_v, rank, lambda m, sh, tr: rank.join(m, sh, tr, key_gdf=key), sends)


@pytest.mark.parametrize("empty", ["build", "probe", "both"])
@pytest.mark.parametrize("how", dc.JOIN_HOWS)
def test_a_rank_that_receives_nothing_of_a_relation(rank, how, empty):
    """no build rows, no probe rows, neither: LEFT keeps the probe rows, FULL both sides' rows, each with -1 for the missing side"""
    model = JoinModel(how, np.int64)
    for world, shape in dc.EMPTY_SIDE_SHAPES:
        for real in positions(world):
            shards = dc.join_shards(world, shape, "int64", empty, real)
            for with_v in (False, True):
                w, got = run_join(model, shards, world, real, with_v, rank, rank.join)
                xb, xp = w.done[0], w.done[1]
                nb = int(xb.real_counts[real]) + sum(len(p[0]) for p in xb.to_real.values())
                np_ = int(xp.real_counts[real]) + sum(len(p[0]) for p in xp.to_real.values())
                assert (nb == 0) == (empty in ("build", "both")) and (np_ == 0) == (empty in ("probe", "both"))
                if empty == "build" and how != "inner":
                    assert len(got[0]) == np_ and (got[1] == -1).all()
                if empty == "probe" and how == "full":
                    assert len(got[0]) == nb and (got[0] == -1).all()
                if empty == "both" or (how == "inner") or (how == "left" and empty == "probe"):
                    assert len(got[0]) == 0


@pytest.mark.parametrize("how", ["inner", "full"])
def test_a_sender_with_more_than_65536_rows(rank, how):
    """local row numbers above 2^16 inside sender << 40 | row, from the real rank's own rows and from a peer's"""
    model = JoinModel(how, np.int64)
    for world in dc.BIG_SENDER_WORLDS:
        shards = dc.big_sender_shards(world)
        sends = sends_of(model, shards, world)
        for real in positions(world):
            for with_v in (False, True):
                w, got = run_join(model, shards, world, real, with_v, rank, rank.join, sends)
                assert ((got[0] & ((1 << 40) - 1))[got[0] >= 0] > 65536).any() and (got[0] >> 40).max() == world - 1
