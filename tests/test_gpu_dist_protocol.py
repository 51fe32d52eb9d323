"""The agreement and error protocol of csrc/dist_ops.hip ("nobody is left waiting in a collective"), with ONE real rank among
scripted numpy peers (tests/dist_world.py).  Host-level return codes and the exact sequence of transport callbacks only: nothing
here faults the device, and nothing waits -- a call the protocol does not allow is refused by the harness and fails the test.

  * a local argument error is carried INTO the first agreement (failure flag set), no block is posted, the rank returns its code;
  * a peer's failure at the first, second or (all_to_all_v) third agreement makes the real rank leave with GDF_C_ERROR there;
  * a bad gather id is reported at the first agreement, a bad row asked by a peer at the answer exchange's agreement;
  * a transport callback that returns non-zero, at every position of the sequence in turn, gives GDF_C_ERROR and leaves no
    state behind: the next call on a fresh transport is right;
  * a malformed transport struct is GDF_INVALID_API_CALL before any callback runs."""
import ctypes as C

import numpy as np
import pytest

import dist_cases as dc
import dist_world as dw
from dist_world import Device, Exchange, Final, GatherModel, GroupByModel, JoinModel, World, run_gather, run_join, run_owner_call

pytestmark = pytest.mark.gpu
LAYOUTS = pytest.mark.parametrize("with_v", [False, True], ids=["blocks", "a2av"])
FLAGGED = [("all_reduce", 2, 1, (0, 1))]          # the first agreement, attended with the failure flag set; nothing else


@pytest.fixture(scope="module")
def rank(gdf):
    return Device(gdf)


def lone_world(world, real, with_v, rank, dtypes, n_exchanges=1, **kw):
    """peers without rows (they agree on blocks of up to 5 rows)"""
    empty = [np.zeros(0, d) for d in dtypes]
    script = [Exchange(dtypes, {s: empty for s in range(world) if s != real}, 5, **kw) for _ in range(n_exchanges)]
    return World(world, real, with_v, script, rank)


@LAYOUTS
@pytest.mark.parametrize("what, code", [
    ("key_mask", "GDF_VALIDITY_UNSUPPORTED"), ("key_dtype", "GDF_UNSUPPORTED_DTYPE"), ("value_dtype", "GDF_UNSUPPORTED_DTYPE"),
    ("sizes", "GDF_COLUMN_SIZE_MISMATCH")])
def test_group_by_argument_errors_travel_into_the_first_agreement(rank, what, code, with_v):
    keys, vals = np.arange(9, dtype=np.int64), np.arange(9, dtype=np.int32)
    kc = {"key_mask": lambda: rank.column(keys, None, np.ones(9, dtype=bool)), "key_dtype": lambda: rank.column(keys.astype(np.float64))}.get(
        what, lambda: rank.column(keys))()
    vc = {"value_dtype": lambda: rank.column(vals, "date32"), "sizes": lambda: rank.column(vals[:8])}.get(what, lambda: rank.column(vals))()
    for op in ("sum", "avg"):
        model = GroupByModel(op, np.int64, np.int32)
        for real in (0, 2):
            w = lone_world(3, real, with_v, rank, model.dtypes)
            err, _ = rank.group_by(model, None, w.ptr, typed=with_v, cols=(kc, vc))
            w.finish(complete=False)
            assert err == code and w.log == FLAGGED


@LAYOUTS
def test_join_and_gather_argument_errors_travel_into_the_first_agreement(rank, with_v):
    k64, k32 = np.arange(9, dtype=np.int64), np.arange(9, dtype=np.int32)
    for how in dc.JOIN_HOWS:
        model = JoinModel(how, np.int64)
        w = lone_world(2, 1, with_v, rank, model.dtypes, 2)
        err, _ = rank.join(model, None, w.ptr, cols=(rank.column(k64), rank.column(k32)))
        w.finish(complete=False)
        assert err == "GDF_JOIN_DTYPE_MISMATCH" and w.log == FLAGGED
    model = GatherModel([np.int32, np.int8])
    cols = [rank.column(k32), rank.column(k32.astype(np.int8))]
    ids = (np.int64(1) << 40) | k64
    for ids_col, use, code in ((rank.column(ids.astype(np.int32)), cols, "GDF_UNSUPPORTED_DTYPE"),
                               (rank.column(ids, None, np.ones(9, dtype=bool)), cols, "GDF_VALIDITY_UNSUPPORTED"),
                               (rank.column(ids), [cols[0], rank.column(k32[:5].astype(np.int8))], "GDF_COLUMN_SIZE_MISMATCH"),
                               (rank.column(np.array([5, 2 << 40, -1], dtype=np.int64)), cols, "GDF_INVALID_API_CALL"),      # names no rank
                               (rank.column(np.array([5, -2], dtype=np.int64)), cols, "GDF_INVALID_API_CALL")):
        w = lone_world(2, 1, with_v, rank, [np.int32], 1)
        err, _ = rank.gather(model, (None, None, None), w.ptr, cols=use, ids_col=ids_col)
        w.finish(complete=False)
        assert err == code and w.log == FLAGGED, (code, err, w.log)


def _group_by_world(rank, real, with_v, **kw):
    shards = dc.group_by_shards(3, 1, "int64", "int32")
    model = GroupByModel("avg", np.int64, np.int32)
    sends = [model.send(s, 3) for s in shards]
    x = Exchange(model.dtypes, {s: sends[s][real] for s in range(3) if s != real}, 40, expect_sent=sends[real], peer_fail=kw.pop("peer_fail", None))
    return model, shards, sends, World(3, real, with_v, [x], rank, **kw)


@LAYOUTS
def test_a_peer_reports_failure_at_each_agreement(rank, with_v):
    for k in (1, 2, 3) if with_v else (1, 2):
        for real in (0, 2):
            model, shards, _, w = _group_by_world(rank, real, with_v, peer_fail=k)
            err, _ = rank.group_by(model, shards[real], w.ptr)
            w.finish(complete=False)
            assert err == "GDF_C_ERROR" and w.stage == "aborted" and w.log[-1][0] == "all_reduce"       # nothing posted behind it
            assert sum(e[0] == "all_reduce" for e in w.log) == k
        # ... in the join's second exchange, and in its last agreement
        jm = JoinModel("left", np.int64)
        js = dc.join_shards(3, 1, "int64")
        bs, ps = [jm.send_side(s[1], 3) for s in js], [jm.send_side(s[0], 3) for s in js]
        mk = lambda snd, fail: Exchange(jm.dtypes, {s: snd[s][0] for s in (1, 2)}, 400, expect_sent=snd[0], peer_fail=fail)
        w = World(3, 0, with_v, [mk(bs, None), mk(ps, k), Final()], rank)
        err, _ = rank.join(jm, js[0], w.ptr)
        w.finish(complete=False)
        assert err == "GDF_C_ERROR" and w.stage == "aborted" and w.done[0].complete and not w.done[1].complete
    w = World(3, 0, with_v, [mk(bs, None), mk(ps, None), Final((0, 1))], rank)
    err, _ = rank.join(jm, js[0], w.ptr)
    w.finish()
    assert err == "GDF_C_ERROR" and w.log[-1][:3] == ("all_reduce", 2, 1)


@LAYOUTS
def test_a_row_beyond_the_shard_asked_by_a_peer(rank, with_v):
    """dg_serve finds it; the failure travels into the answer exchange's first agreement and the rank returns GDF_INVALID_API_CALL"""
    model = GatherModel([np.int16])
    col = np.arange(10, dtype=np.int16)
    for bad_row, code in ((10, "GDF_INVALID_API_CALL"), (9, "GDF_SUCCESS")):
        asks = np.array([0, bad_row, 3], dtype=np.int32)
        x1 = Exchange([np.int32], {1: [asks]}, 3, name="requests")
        x2 = Exchange(model.resp_dtypes, {1: [np.zeros(0, np.int16), np.zeros(0, np.int8)]}, 0, name="answers")
        w = World(2, 0, with_v, [x1, x2], rank)
        err, got = rank.gather(model, (np.zeros(0, np.int64), [col], [None]), w.ptr)
        w.finish(complete=code == "GDF_SUCCESS")
        assert err == code and x1.complete
        if code == "GDF_SUCCESS":
            assert np.array_equal(x2.sent[1][0], col[asks]) and x2.sent[1][1].all()
        else:
            assert w.log[-1] == ("all_reduce", 2, 1, (0, 1)) and not x2.complete


@LAYOUTS
def test_a_failing_transport_call_at_every_position(rank, with_v):
    """GDF_C_ERROR at once (tickets already handed out may still be waited for, nothing else follows), and the next call is right"""
    model, shards, sends, w = _group_by_world(rank, 1, with_v)
    err, _ = rank.group_by(model, shards[1], w.ptr)
    w.finish()
    n = w.ncalls
    assert err == "GDF_SUCCESS" and n >= 8
    for i in range(n):
        model, shards, sends, w = _group_by_world(rank, 1, with_v, fail_at=i)
        err, _ = rank.group_by(model, shards[1], w.ptr)
        w.finish(complete=False)
        assert err == "GDF_C_ERROR" and w.injected, (i, err)
        run_owner_call(model, shards, sends, 3, 1, with_v, rank, rank.group_by)
    jm = JoinModel("full", np.int64)
    js = dc.join_shards(2, 1, "int64")
    gm = GatherModel([np.int16, np.float64])
    gs = dc.gather_shards(2, 1, ("int16", "float64"), (True, False))
    for run, model, shards, call in ((run_join, jm, js, rank.join), (run_gather, gm, gs, rank.gather)):
        w = run(model, shards, 2, 0, with_v, rank, call)
        n = (w[0] if isinstance(w, tuple) else w).ncalls
        for i in range(n):
            assert run(model, shards, 2, 0, with_v, rank, call, fail_at=i).log[-1][0] in ("failed", "wait")
            run(model, shards, 2, 0, with_v, rank, call)


def test_a_malformed_transport_is_refused_before_any_callback(rank):
    model = GroupByModel("sum", np.int64, np.int32)
    shard = (np.arange(5, dtype=np.int64), np.arange(5, dtype=np.int32))
    jm, gm = JoinModel("inner", np.int64), GatherModel([np.int32])
    for spoil in ("all_to_all", "wait", "all_reduce_i64", "rank", "negative_rank", "world"):
        w = lone_world(2, 0, True, rank, model.dtypes)
        t = w.transport
        if spoil == "rank":
            t.rank = 2
        elif spoil == "negative_rank":
            t.rank = -1
        elif spoil == "world":
            t.world = 0
        else:
            setattr(t, spoil, C.cast(None, dict(dw.Transport._fields_)[spoil]))
        assert rank.group_by(model, shard, w.ptr)[0] == "GDF_INVALID_API_CALL"
        assert rank.group_by(model, shard, w.ptr, typed=True)[0] == "GDF_INVALID_API_CALL"
        assert rank.join(jm, (shard[0], shard[0]), w.ptr)[0] == "GDF_INVALID_API_CALL"
        assert rank.gather(gm, (shard[0], [shard[1]], [None]), w.ptr)[0] == "GDF_INVALID_API_CALL"
        assert w.log == [] and w.ncalls == 0
