"""gdf_amd_dist_group_by and its five typed wrappers with ONE real rank among scripted numpy peers (tests/dist_world.py): every op,
value dtype and key dtype of csrc/dist_ops.hip's single-key path, in worlds of 1, 2, 3, 5 and 8 ranks, in both exchange layouts
(equal blocks through the typed wrappers, all_to_all_v through the generic entry), the real rank first and last (everywhere for
W <= 3).  Per call: (a) the partial aggregates it sent to every owner, (b) its result for what it received, (c) the world's groups
against the oracle over the concatenated shards.  Integer sums wrap; float sums are exact by construction (tests/dist_cases.py), so
everything is compared bit for bit."""
import numpy as np
import pytest

import dist_cases as dc
import dist_world as dw
from dist_world import Device, GroupByModel, positions, run_owner_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rank(gdf):
    return Device(gdf)


def sweep(rank, op, key, val, worlds=dw.WORLDS):
    for world in worlds:
        for shape in range(len(dc.SHAPES[world])):
            shards = dc.group_by_shards(world, shape, key, val)
            model = GroupByModel(op, dw.NP_OF[key], dw.NP_OF[val])
            sends = [model.send(s, world) for s in shards]
            for real in positions(world):
                for with_v in (False, True):
                    run_owner_call(model, shards, sends, world, real, with_v, rank,
                                   lambda m, sh, tr: rank.group_by(m, sh, tr, typed=not with_v, key_gdf=key))


@pytest.mark.parametrize("op, key, val", dc.GROUP_BY_CASES)
def test_every_op_value_dtype_and_key_dtype(rank, op, key, val):
    """partials in the value dtype cross rank boundaries (int8 ... float64), COUNT travels as int64, AVG as widened sum and count;
    the 4-byte key branch (INT32, DATE32) and an 8-byte date type, keys at both ends of their range, negative, dense"""
    sweep(rank, op, key, val)


@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_sums_wrap_on_the_sender_and_again_at_the_owner(rank, world):
    """int8: 3 x 127 wraps to 125 on every sender and the owner's sum of the partials wraps again; int64 AVG: the sum passes 2^53 and
    wraps -- the reference is the wrapped sum, converted once, over the count"""
    for shards, ops, vd in zip(dc.wrap_twice_shards(world), (("sum",), ("sum", "avg")), (np.int8, np.int64)):
        for op in ops:
            model = GroupByModel(op, np.int64, vd)
            sends = [model.send(s, world) for s in shards]
            for real in positions(world):
                for with_v in (False, True):
                    run_owner_call(model, shards, sends, world, real, with_v, rank, lambda m, sh, tr: rank.group_by(m, sh, tr, typed=with_v))


@pytest.mark.parametrize("op", ["min", "max"])
@pytest.mark.parametrize("val", ["float32", "float64"])
def test_nan_groups_infinities_and_signed_zeros_across_senders(rank, gdf, op, val):
    """what tests/groupby_values.py pins for MIN / MAX, with every group SPLIT across senders: a NaN-only group stays NaN at the owner,
    +0.0 from one sender and -0.0 from another compare equal, an infinity from one sender wins.  (a) the partials sent, (b) the
    owner's combine of what it received, (c) the world's union against the SINGLE-GPU call on the concatenated shards; == throughout."""
    from libgdf_amd.columns import column_from_numpy
    for world in dc.SPECIAL_WORLDS:
        shards = dc.special_float_shards(world, dw.NP_OF[val])
        keys, vals = np.concatenate([s[0] for s in shards]), np.concatenate([s[1] for s in shards])
        gk, ga = gdf.api.group_by(op, [column_from_numpy(keys)], column_from_numpy(vals), sort_result=True)
        reference = [gk[0].cpu().numpy(), ga.cpu().numpy()]
        model = dw.MinMaxSpecialsModel(op, np.int64, dw.NP_OF[val])
        dw.assert_same_groups(model.whole(shards), reference, "the numpy model against the single-GPU call")
        sends = [model.send(s, world) for s in shards]
        for real in range(world):
            for with_v in (False, True):
                dw.run_specials(model, shards, sends, world, real, with_v, rank, lambda m, sh, tr: rank.group_by(m, sh, tr, typed=with_v), reference)
