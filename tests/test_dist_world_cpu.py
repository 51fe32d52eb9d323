"""CPU tests of the one-process harness for csrc/dist_ops.hip (tests/dist_world.py, tests/dist_cases.py): nothing here needs a GPU.

1. The peer model with ALL W ranks in numpy reproduces the oracle over the concatenated shards on every entry of the case tables --
   what makes checks (b) and (c) of the GPU tests trustworthy.
2. The harness's state machine, driven by StandIn (a numpy real rank that makes the library's callback sequence over host buffers):
   it accepts the right sequence in both exchange layouts and refuses each wrong one.
3. The properties the case tables promise: exact float sums, every listed shape, every kernel instantiation reached.
"""
import numpy as np
import pytest

import dist_cases as dc
import dist_world as dw
from dist_world import Exchange, GatherModel, GroupByModel, GroupByMultiModel, JoinModel, StandIn, World, owner_of, positions, same_rows

ALL_SHAPES = [(w, s) for w in dw.WORLDS for s in range(len(dc.SHAPES[w]))]


def all_numpy(model, shards, world):
    sends = [model.send(sh, world) for sh in shards]
    results = [model.finish([sends[s][r] for s in range(world)]) for r in range(world)]
    for r, res in enumerate(results):
        assert (model.owner(res, world) == r).all()
    return [np.concatenate([res[c] for res in results]) for c in range(len(results[0]))]


# ---- 1. the model is the oracle ----
@pytest.mark.parametrize("op, key, val", dc.GROUP_BY_CASES)
def test_group_by_model_reproduces_the_oracle(op, key, val):
    """the (op, key dtype, value dtype) triples the GPU file runs, in every world and shape"""
    for world, shape in ALL_SHAPES:
        shards = dc.group_by_shards(world, shape, key, val)
        model = GroupByModel(op, shards[0][0].dtype, shards[0][1].dtype)
        assert same_rows(all_numpy(model, shards, world), model.whole(shards)), (world, shape)


@pytest.mark.parametrize("op", ["min", "max"])
@pytest.mark.parametrize("val", ["float32", "float64"])
def test_special_float_model_reproduces_what_groupby_values_pins(op, val):
    """NaN-only groups, infinities and zeros of both signs split across senders: the numpy model with all ranks, against
    tests/groupby_values.py's reference of every group over the concatenated shards"""
    import groupby_values as gv
    dt = np.dtype(dw.NP_OF[val])
    for world in dc.SPECIAL_WORLDS:
        shards = dc.special_float_shards(world, dt)
        keys, vals = np.concatenate([s[0] for s in shards]), np.concatenate([s[1] for s in shards])
        uk = np.unique(keys)
        want = [uk, np.array([gv.reference(op, vals[keys == k], dt) for k in uk], dtype=dt)]
        model = dw.MinMaxSpecialsModel(op, np.int64, dt)
        dw.assert_same_groups(all_numpy(model, shards, world), want, "all ranks in numpy")
        dw.assert_same_groups(model.whole(shards), want, "the model over the concatenation")
        assert np.isnan(want[1][uk == 3]).all() and np.isnan(want[1][uk == 11]).all()
        # the groups really are split: NaN partials from every sender, zeros of both signs from different senders
        sends = [model.send(s, world) for s in shards]
        parts = [p for s in sends for p in s if len(p[0])]
        assert sum(int((p[0] == 3).sum()) for p in parts) == world
        zeros = np.concatenate([p[1][p[0] == 1] for p in parts])
        assert len(zeros) == world and np.signbit(zeros).any() and not np.signbit(zeros).all()
        for rank in StandIn(),:
            for real in range(world):
                for with_v in (False, True):
                    dw.run_specials(model, shards, sends, world, real, with_v, rank, rank.group_by, want)


@pytest.mark.parametrize("names, masked", dc.GATHER_CASES, ids=lambda v: "-".join(str(x) for x in v) if len(v) < 3 else f"{len(v)}cols")
def test_gather_model_reproduces_the_rows_the_ids_name(names, masked):
    """all ranks in numpy: requests split by owner, the owners' answers in arrival order, placed at the positions kept -- against a
    row-by-row lookup of every id in its owner's shard, written here without the model"""
    model = GatherModel([dw.NP_OF[n] for n in names])
    for world in dw.WORLDS:
        for shape in range(len(dc.GATHER_SHAPES[world])):
            shards = dc.gather_shards(world, shape, names, masked)
            reqs = [model.requests(shards[r][0], r, world) for r in range(world)]
            for r in range(world):
                ids = shards[r][0]
                parts, owner = reqs[r]
                answers = [model.serve(parts[o][0], shards[o][1], shards[o][2]) for o in range(world)]
                where = [np.flatnonzero(owner == o) for o in range(world)]
                whole = model.whole(shards, r)
                for c in range(len(names)):
                    vals, ok = np.zeros(len(ids), dtype=model.cds[c]), np.zeros(len(ids), dtype=bool)
                    for o in range(world):
                        vals[where[o]], ok[where[o]] = answers[o][2 * c], answers[o][2 * c + 1] != 0
                    for i, g in enumerate(ids.tolist()):
                        if g == -1:
                            assert not ok[i] and not whole[c][1][i]
                            continue
                        o, row = g >> 40, g & ((1 << 40) - 1)
                        valid = shards[o][2][c] is None or bool(shards[o][2][c][row])
                        assert ok[i] == valid == whole[c][1][i]
                        if valid:
                            assert vals[i] == shards[o][1][c][row] == whole[c][0][i]


@pytest.mark.parametrize("case", dc.MULTI_CASES, ids=lambda c: "-".join([c[0], *c[1], c[4]]))
def test_multi_key_model_reproduces_the_oracle(case):
    for world, shape in ALL_SHAPES:
        shards = dc.multi_shards(world, shape, case)
        model = GroupByMultiModel(case[0], [dw.NP_OF[k] for k in case[1]], dw.NP_OF[case[4]])
        assert same_rows(all_numpy(model, shards, world), model.whole(shards)), (world, shape)


@pytest.mark.parametrize("rows", dc.OWNER_ROWS)
def test_owner_row_counts_are_what_the_table_says(rows):
    for world in dc.OWNER_ROWS_WORLDS:
        for real in positions(world):
            shards = dc.owner_rows_shards(world, real, rows)
            model = GroupByMultiModel("sum", [np.int64], np.int32)
            sends = [model.send(sh, world) for sh in shards]
            assert sum(len(sends[s][real][0]) for s in range(world)) == rows
            assert same_rows(all_numpy(model, shards, world), model.whole(shards))


@pytest.mark.parametrize("how", dc.JOIN_HOWS)
@pytest.mark.parametrize("key", dc.JOIN_KEYS)
def test_join_model_reproduces_the_oracle(how, key):
    model = JoinModel(how, dw.NP_OF[key])
    tables = [(w, dc.join_shards(w, s, key)) for w, s in ALL_SHAPES]
    tables += [(w, dc.join_shards(w, s, key, empty, real)) for w, s in dc.EMPTY_SIDE_SHAPES for empty in ("build", "probe", "both")
               for real in positions(w)]
    if key == "int64":
        tables += [(w, dc.big_sender_shards(w)) for w in dc.BIG_SENDER_WORLDS]
    for world, shards in tables:
        bs, ps = [model.send_side(s[1], world) for s in shards], [model.send_side(s[0], world) for s in shards]
        results = [model.finish([bs[s][r] for s in range(world)], [ps[s][r] for s in range(world)]) for r in range(world)]
        union = [np.concatenate([res[c] for res in results]) for c in range(2)]
        want = model.whole(shards)
        assert same_rows(union, want)
        if how != "inner":                   # every probe row comes out, unmatched ones exactly once
            assert len(np.unique(union[0][union[1] == -1])) == (union[1] == -1).sum()
        if how == "full":
            assert len(np.unique(union[1][union[0] == -1])) == (union[0] == -1).sum()


def test_the_empty_side_shapes_are_empty():
    for world, shape in dc.EMPTY_SIDE_SHAPES:
        for empty in ("build", "probe", "both"):
            for real in positions(world):
                shards = dc.join_shards(world, shape, "int64", empty, real)
                for side, name in ((1, "build"), (0, "probe")):
                    n = sum(int((owner_of([s[side]], world) == real).sum()) for s in shards)
                    assert (n == 0) == (empty in (name, "both")), (world, empty, real, name, n)


def test_a_big_sender_is_first_and_last():
    for world in dc.BIG_SENDER_WORLDS:
        shards = dc.big_sender_shards(world)
        assert len(shards[0][0]) > 65536 and len(shards[0][1]) > 65536 and (world == 2 or len(shards[-1][0]) > 65536)


# ---- 2. the state machine, driven by the numpy stand-in ----
@pytest.mark.parametrize("with_v", [False, True], ids=["blocks", "a2av"])
@pytest.mark.parametrize("world", dw.WORLDS)
def test_harness_accepts_the_protocol(world, with_v):
    rank = StandIn()
    for shape in range(len(dc.SHAPES[world])):
        for op, val in (("sum", "int8"), ("avg", "float32"), ("count", "int16")):
            shards = dc.group_by_shards(world, shape, "int32", val)
            model = GroupByModel(op, np.int32, dw.NP_OF[val])
            sends = [model.send(s, world) for s in shards]
            for real in positions(world):
                dw.run_owner_call(model, shards, sends, world, real, with_v, rank, rank.group_by)
        case = dc.MULTI_CASES[5]
        shards = dc.multi_shards(world, shape, case)
        model = GroupByMultiModel(case[0], [dw.NP_OF[k] for k in case[1]], dw.NP_OF[case[4]])
        sends = [model.send(s, world) for s in shards]
        for real in positions(world):
            dw.run_owner_call(model, shards, sends, world, real, with_v, rank, rank.group_by_multi)
            shards_j = dc.join_shards(world, shape, "int64")
            dw.run_join(JoinModel("full", np.int64), shards_j, world, real, with_v, rank, rank.join)
    names = ("int16", "float64", "int8")
    for shape in range(len(dc.GATHER_SHAPES[world])):
        shards = dc.gather_shards(world, shape, names, (True, False, True))
        for real in positions(world):
            dw.run_gather(GatherModel([dw.NP_OF[n] for n in names]), shards, world, real, with_v, rank, rank.gather)


def _one_exchange(world, real, with_v, bug, peer_fail=None, fail_at=None):
    shards = dc.group_by_shards(world, 0, "int64", "int32")          # (1, 20011, 0) rows, keys of every owner
    model = GroupByModel("sum", np.int64, np.int32)
    sends = [model.send(s, world) for s in shards]
    x = Exchange(model.dtypes, {s: sends[s][real] for s in range(world) if s != real},
                 max(len(sends[s][r][0]) for s in range(world) if s != real for r in range(world)), expect_sent=sends[real], peer_fail=peer_fail)
    w = World(world, real, with_v, [x], fail_at=fail_at)
    err, got = StandIn(bug).group_by(model, shards[real], w.transport)
    return w, err, got


@pytest.mark.parametrize("bug, with_v, says", [
    ("skip_first_agreement", False, "the first agreement carries 2 values"),        # wrong order
    ("skip_first_agreement", True, "the first agreement carries 2 values"),
    ("skip_third_agreement", True, "all_to_all_v where it is not due"),
    ("wrong_block", False, "agreed were"),                                          # wrong block size
    ("wrong_counts", False, "disagree with the largest partition"),                 # counts that disagree with the data
    ("wrong_counts", True, "disagree with the largest partition"),
    ("wrong_offsets", True, "send offsets"),
    ("extra_exchange", False, "an extra exchange"),
])
def test_harness_refuses_a_wrong_sequence(bug, with_v, says):
    w, err, _ = _one_exchange(3, 1, with_v, bug)
    assert w.violation is not None and says in w.violation, w.violation
    with pytest.raises(AssertionError):
        w.finish()


def test_harness_refuses_rows_the_model_does_not_send():
    w, err, got = _one_exchange(3, 1, False, None)
    w.finish()
    w.check_sent()
    x = w.done[0]
    x.sent[0][1][:1] += 1                  # one value of one row
    with pytest.raises(AssertionError):
        w.check_sent()
    x.sent[0][1][:1] -= 1
    x.sent[0] = [c[::-1].copy() for c in x.sent[0]]     # order inside a partition is free
    w.check_sent()
    x.sent[0][0] = x.sent[0][0][::-1].copy()            # ... but the columns stay aligned
    with pytest.raises(AssertionError):
        w.check_sent()


@pytest.mark.parametrize("with_v", [False, True], ids=["blocks", "a2av"])
def test_harness_poisons_the_padding_and_never_waits(with_v):
    """the padding behind a peer's short block is 0xA5; a peer's failure at each agreement ends the sequence there; a failing
    callback at each position ends it too"""
    w, err, got = _one_exchange(3, 0, with_v, None)
    w.finish()
    assert err == "GDF_SUCCESS"
    n = w.ncalls
    for k in (1, 2, 3) if with_v else (1, 2):
        w, err, _ = _one_exchange(3, 0, with_v, None, peer_fail=k)
        w.finish(complete=False)
        assert err == "GDF_C_ERROR" and w.stage == "aborted" and w.log[-1][0] == "all_reduce"
        assert sum(e[0] == "all_reduce" for e in w.log) == k
    for i in range(n):
        w, err, _ = _one_exchange(3, 0, with_v, None, fail_at=i)
        w.finish(complete=False)
        assert err == "GDF_C_ERROR" and w.injected
    if not with_v:
        seen = {}
        class Spy(dw.Host):
            @staticmethod
            def write(ptr, data):
                seen.setdefault("blocks", []).append(np.array(data))
                dw.Host.write(ptr, data)
        shards = dc.group_by_shards(3, 0, "int64", "int32")      # (1, 20011, 0) rows: rank 2 sends nothing into blocks of thousands
        model = GroupByModel("sum", np.int64, np.int32)
        sends = [model.send(s, 3) for s in shards]
        x = Exchange(model.dtypes, {1: sends[1][0], 2: sends[2][0]}, max(len(sends[1][r][0]) for r in range(3)), expect_sent=sends[0])
        w = World(3, 0, False, [x], backend=Spy)
        StandIn().group_by(model, shards[0], w.transport)
        w.finish()
        block = seen["blocks"][1].reshape(3, -1)
        assert (block[2] == dw.POISON).all() and w.blk > 1


# ---- 3. what the tables promise ----
def test_every_float_case_has_exact_sums():
    """|value| <= 32 in steps of 1/4 and fewer than 2^15.5 rows in a world: the sum of ANY subset in ANY order is a multiple of 1/4
    below 2^24 / 4, exact in float32 and float64 -- so the float SUM / AVG tests need no tolerance"""
    tables = [dc.group_by_shards(w, s, "int64", v) for w, s in ALL_SHAPES for v in ("float32", "float64")]
    tables += [[(None, sh[2]) for sh in dc.multi_shards(w, s, c)] for w, s in ALL_SHAPES for c in dc.MULTI_CASES if c[4].startswith("float")]
    for shards in tables:
        vals = np.concatenate([s[1] for s in shards]).astype(np.float64)
        units = vals / dc.FLOAT_UNIT
        assert np.array_equal(units, np.round(units)) and np.abs(units).sum() < 2 ** 24


def test_every_listed_shape_is_there():
    sizes = {n for w in dw.WORLDS for shape, _, _ in dc.SHAPES[w] for n in shape}
    assert sizes == set(dw.SHARD_SIZES)
    for w in dw.WORLDS:
        assert any(0 in shape for shape, _, _ in dc.SHAPES[w]), "a rank without rows"
        one_owner = 0
        for s, (shape, one, layout) in enumerate(dc.SHAPES[w]):
            if one is None:
                continue
            # a rank of hundreds of rows and several groups whose partials -- and whose rows of both join relations -- go to ONE owner
            assert layout == "mixed" and shape[one] >= 255 and w > 1
            sends = sends_of(w, s)
            assert sum(len(p[0]) > 0 for p in sends[one]) == 1 and max(len(p[0]) for p in sends[one]) > 1
            for key in dc.JOIN_KEYS:
                probe, build = dc.join_shards(w, s, key)[one]
                assert len(probe) == shape[one] and len(build) >= 40
                assert len(set(owner_of([probe], w).tolist()) | set(owner_of([build], w).tolist())) == 1 and len(np.unique(probe)) > 1
            one_owner += 1
        assert one_owner > 0 or w == 1, "a rank whose rows belong to one owner"
        assert {layout for _, _, layout in dc.SHAPES[w]} >= {"mixed"}
        if w > 1:                                # the agreed block exceeds what a real rank at the first or last position sends
            assert any(max(len(p[0]) for s in range(w) if s != real for p in sends_of(w, sh)[s]) > max(len(p[0]) for p in sends_of(w, sh)[real])
                       for sh in range(len(dc.SHAPES[w])) for real in (0, w - 1))
    got_ids = {n for w in dw.WORLDS for ids, _, _ in dc.GATHER_SHAPES[w] for r, n in enumerate(ids) if r in positions(w)}
    assert set(dc.ID_SIZES) <= got_ids and 0 in got_ids
    for w in (3, 5, 8):
        assert any(lonely is not None for _, _, lonely in dc.GATHER_SHAPES[w])
    assert {layout for w in dw.WORLDS for _, _, layout in dc.SHAPES[w]} == {"mixed", "one_group", "distinct"}


def sends_of(world, shape):
    shards = dc.group_by_shards(world, shape, "int64", "int8")
    model = GroupByModel("sum", np.int64, np.int8)
    return [model.send(sh, world) for sh in shards]


def test_int8_sums_wrap_on_the_sender_and_at_the_owner_and_int64_averages_pass_2_53():
    for world in (2, 3, 5, 8):
        i8, i64 = dc.wrap_twice_shards(world)
        partial = sum(int(v) for v in i8[0][1])
        assert partial > 127 and abs(world * int(np.int64(partial).astype(np.int8))) > 127
        model = GroupByModel("sum", np.int64, np.int8)
        assert same_rows(all_numpy(model, i8, world), model.whole(i8))
        assert int(model.whole(i8)[1][0]) == int(np.int64(world * partial).astype(np.int8))
        model = GroupByModel("avg", np.int64, np.int64)
        total = world * 3 * (2 ** 62 + 12345)
        assert total > 2 ** 53
        wrapped = (total + 2 ** 63) % 2 ** 64 - 2 ** 63
        assert same_rows(all_numpy(model, i64, world), model.whole(i64))
        assert model.whole(i64)[1][0] == np.float64(wrapped) / np.float64(3 * world)


# kernel instantiation of csrc/dist_ops.hip, keyed by dtype width and op -> the GPU test function that reaches it and one entry of the
# table that test is parametrised with
KERNELS = {
    ("dg_widen<int8_t, long long>", 1, "avg"): ("test_gpu_dist_group_by", "test_every_op_value_dtype_and_key_dtype", ("avg", "int64", "int8")),
    ("dg_widen<int16_t, long long>", 2, "avg"): ("test_gpu_dist_group_by", "test_every_op_value_dtype_and_key_dtype", ("avg", "int64", "int16")),
    ("dg_widen<int16_t, long long> under 4-byte keys", 2, "avg"): ("test_gpu_dist_group_by", "test_every_op_value_dtype_and_key_dtype", ("avg", "date32", "int16")),
    ("dg_widen<int32_t, long long>", 4, "avg"): ("test_gpu_dist_group_by", "test_every_op_value_dtype_and_key_dtype", ("avg", "int64", "int32")),
    ("dg_widen<long long, long long>", 8, "avg"): ("test_gpu_dist_group_by", "test_every_op_value_dtype_and_key_dtype", ("avg", "int64", "int64")),
    ("dg_widen<float, double>", 4, "avg"): ("test_gpu_dist_group_by", "test_every_op_value_dtype_and_key_dtype", ("avg", "int64", "float32")),
    ("dg_widen<double, double>", 8, "avg"): ("test_gpu_dist_group_by", "test_every_op_value_dtype_and_key_dtype", ("avg", "int64", "float64")),
    ("dg_divide<long long>", 2, "avg"): ("test_gpu_dist_group_by", "test_every_op_value_dtype_and_key_dtype", ("avg", "int32", "int16")),
    ("dg_divide<double>", 4, "avg"): ("test_gpu_dist_group_by", "test_every_op_value_dtype_and_key_dtype", ("avg", "int64", "float32")),
    ("dg_mask_from_counts", 4, "sum"): ("test_gpu_dist_group_by_multi", "test_keys_masks_and_values", ("sum", ("int64",), (False,), True, "int32")),
    ("dg_mask_from_counts", 8, "min"): ("test_gpu_dist_group_by_multi", "test_keys_masks_and_values", ("min", ("int32", "float64"), (True, False), True, "float64")),
    ("dg_mask_from_counts", 2, "max"): ("test_gpu_dist_group_by_multi", "test_keys_masks_and_values", ("max", ("int32", "float64"), (False, True), True, "int16")),
    ("dg_divide_masked<long long>", 8, "avg"): ("test_gpu_dist_group_by_multi", "test_keys_masks_and_values",
                                                ("avg", ("int16", "float64", "int64"), (True, False, True), True, "int64")),
    ("dg_divide_masked<double>", 4, "avg"): ("test_gpu_dist_group_by_multi", "test_keys_masks_and_values", ("avg", ("int32", "float64"), (False, False), True, "float32")),
    ("dg_gids, dg_resolve", 4, "inner"): ("test_gpu_dist_shuffle_join", "test_every_world", ("inner", "int32")),
    ("dg_gids, dg_resolve", 8, "full"): ("test_gpu_dist_shuffle_join", "test_every_world", ("full", "int64")),
    ("dg_requests, dg_serve<uint8_t>, dg_place<uint8_t>", 1, "gather"): ("test_gpu_dist_gather", "test_every_column_width_with_and_without_masks", (("int8",), (False,))),
    ("dg_serve<uint16_t>, dg_place<uint16_t>", 2, "gather"): ("test_gpu_dist_gather", "test_every_column_width_with_and_without_masks", (("int16",), (False,))),
    ("dg_serve<uint32_t>, dg_place<uint32_t>", 4, "gather"): ("test_gpu_dist_gather", "test_every_column_width_with_and_without_masks", (("date32",), (False,))),
    ("dg_serve<uint64_t>, dg_place<uint64_t>", 8, "gather"): ("test_gpu_dist_gather", "test_every_column_width_with_and_without_masks", (("timestamp",), (True,))),
    ("dg_serve reading a mask, dg_pack with null rows", 2, "gather"): ("test_gpu_dist_gather", "test_every_column_width_with_and_without_masks", (("int16",), (True,))),
    ("dg_pack, 16 columns", 8, "gather"): ("test_gpu_dist_gather", "test_every_column_width_with_and_without_masks", dc.GATHER_CASES[-1]),
}


def parametrised_with(module, function):
    """the argument tuples the GPU test function is parametrised with (the product of its parametrize marks)"""
    import importlib
    import itertools
    marks = [m for m in getattr(importlib.import_module(module), function).pytestmark if m.name == "parametrize"]
    lists = [[v if isinstance(v, (tuple, list)) and "," in m.args[0] else (v,) for v in m.args[1]] for m in marks]
    return {sum((tuple(x) for x in combo), ()) for combo in itertools.product(*lists)}


def test_every_kernel_instantiation_is_reached():
    """every entry of KERNELS is one of the argument tuples its GPU test function is really parametrised with, its width is that
    of the dtype it names, and the GPU tests sweep every world, position and layout for it"""
    for (kernel, width, op), (module, function, entry) in KERNELS.items():
        cases = parametrised_with(module, function)
        assert tuple(entry) in cases or (tuple(entry),) in cases, (kernel, entry)      # (one argument name: the case is the argument)
        assert op in entry or op == "gather", (kernel, op)
        names = entry[0] if op == "gather" else [entry[-1]]
        assert width in {np.dtype(dw.NP_OF[n]).itemsize for n in names}, (kernel, width)
    ops = {(op, np.dtype(dw.NP_OF[val]).itemsize) for op, _, val in dc.GROUP_BY_CASES}
    assert {op for op, _ in ops} == set(dw.OPS) and {w for _, w in ops} == {1, 2, 4, 8}
    assert {np.dtype(dw.NP_OF[n[0]]).itemsize for n, m in dc.GATHER_CASES[:-1]} == {1, 2, 4, 8}
    assert {m[0] for n, m in dc.GATHER_CASES[:-1]} == {False, True} and len(dc.GATHER_CASES[-1][0]) == 16


def test_the_multi_key_tables_hold_null_groups_and_groups_valid_on_one_sender():
    for case in dc.MULTI_CASES:
        op, kds, kmask, vmask, vd = case
        if not vmask:
            continue
        null_groups = one_sender = 0
        for world, shape in ALL_SHAPES:
            shards = dc.multi_shards(world, shape, case)
            model = GroupByMultiModel("sum", [dw.NP_OF[k] for k in kds], dw.NP_OF[vd])
            null_groups += int((~model.whole(shards)[-1]).sum())
            senders = 0
            for keys, kvs, vals, vv in shards:
                live = vv & (keys[0] == 2)
                for v in kvs:
                    live = live & (v if v is not None else True)
                senders += bool(live.any())
            one_sender += senders == 1 and world > 1
        assert null_groups > 0 and one_sender > 0, case
