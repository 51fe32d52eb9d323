"""A virtual world with ONE real rank for the distributed entry points of csrc/dist_ops.hip (gdf_amd_dist_group_by*,
gdf_amd_dist_group_by_multi, gdf_amd_dist_shuffle_*join, gdf_amd_dist_gather).

A gdf_amd_transport is four function pointers plus an optional fifth, so a test can BE the other W - 1 ranks: World builds the
struct from ctypes callbacks (as libgdf_amd.api.CallbackTransport does) and answers every collective at once from numpy PEERS --
models of a rank that compute, with numpy and oracle/oracle.py, what a rank sends and what it makes of what it receives.  Nothing
here blocks, waits or starts a process; a call the protocol does not allow at that point makes the callback return 1 and is
recorded (World.violation), so the order of the collectives that all ranks must share is pinned and no state of the harness can
hang a test.

The wire (include/gdf/gdf_amd_ext.h, exchange_blocks in csrc/dist_ops.hip), per exchange of `ncols` columns:
    all_reduce_i64 max {largest partition anywhere, a rank has failed}       -> blk = max(largest, 1)
    all_reduce_i64 max {a rank has failed}                                   (the wire buffers / the count buffers exist)
    all_to_all of 8 bytes per rank: the int64 row counts
  equal blocks (no fifth function):
    one all_to_all of width * blk bytes per rank and column, then one wait per ticket
  all_to_all_v (fifth function present):
    wait, all_reduce_i64 max {a rank has failed} (the result columns exist), one all_to_all_v per column with exact byte
    offsets, then the waits.
An agreement that says "a rank has failed" ends the call on every rank.  The join adds a last all_reduce_i64 max {received too
many rows, a rank has failed} behind its two exchanges.

Three checks per call (run_* below): (a) what the real rank SENT to every peer is, as a multiset of row tuples, what a numpy
peer in its place would have sent; (b) what it RETURNED is the model's result for what it received; (c) the union of its result
and the peers' modelled results is the oracle over the concatenated shards.

Device memory is touched through two functions only, `read` and `write` of a backend: Device (gdf_amd_copy) or Host (ctypes
memmove).  StandIn is a numpy real rank that makes the same callback sequence over host buffers, so the CPU tests drive this same
harness without a GPU.
"""
import ctypes as C

import numpy as np

from oracle import oracle

POISON = 0xA5
GDF = dict(int8=1, int16=2, int32=3, int64=4, float32=5, float64=6, date32=7, date64=8, timestamp=9)
NP_OF = dict(int8=np.int8, int16=np.int16, int32=np.int32, int64=np.int64, float32=np.float32, float64=np.float64,
             date32=np.int32, date64=np.int64, timestamp=np.int64)
OPS = ("sum", "min", "max", "count", "avg")
AGG_OP = {"sum": 0, "min": 1, "max": 2, "avg": 3, "count": 4}            # gdf_agg_op
WORLDS = (1, 2, 3, 5, 8)
SHARD_SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2049, 20011)

_A2A = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p))
_WAIT = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)
_ALLRED = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_int, C.c_int)
_DESTROY = C.CFUNCTYPE(None, C.c_void_p)
_A2AV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_void_p))


class Transport(C.Structure):
    """gdf_amd_transport (include/gdf/gdf_amd_ext.h)"""
    _fields_ = [("ctx", C.c_void_p), ("rank", C.c_int), ("world", C.c_int), ("all_to_all", _A2A), ("wait", _WAIT),
                ("all_reduce_i64", _ALLRED), ("destroy", _DESTROY), ("all_to_all_v", _A2AV)]


def positions(world):
    """where the real rank sits: everywhere in a small world, first and last in a larger one"""
    return list(range(world)) if world <= 3 else [0, world - 1]


# ---- the two memory backends ---------------------------------------------------------------------------------------------------------
class Host:
    """`device` pointers are host pointers (the CPU tests)"""

    @staticmethod
    def read(ptr, nbytes):
        return np.frombuffer(C.string_at(ptr, nbytes), dtype=np.uint8).copy() if nbytes else np.zeros(0, np.uint8)

    @staticmethod
    def write(ptr, data):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.size:
            C.memmove(ptr, data.ctypes.data, data.size)


# ---- rows as bytes -------------------------------------------------------------------------------------------------------------------
def row_bytes(cols):
    """[n, sum of widths] uint8: the row tuples of equally long columns, bit for bit"""
    n = len(cols[0])
    return np.concatenate([np.ascontiguousarray(c).view(np.uint8).reshape(n, c.dtype.itemsize) for c in cols], axis=1)


def sorted_rows(cols):
    m = row_bytes(cols)
    return m[np.lexsort(m.T[::-1])] if len(m) else m


def same_rows(a, b, ordered=False):
    if [c.dtype for c in a] != [c.dtype for c in b] or len(a[0]) != len(b[0]):
        return False
    return np.array_equal(row_bytes(a), row_bytes(b)) if ordered else np.array_equal(sorted_rows(a), sorted_rows(b))


# ---- the script of one call ----------------------------------------------------------------------------------------------------------
class Exchange:
    """One exchange_blocks as the peers see it.  dtypes: the wire columns; to_real[s]: the columns peer s sends to the real rank;
    peer_max: the largest partition any peer sends to anybody; expect_sent[r]: the columns the model says the real rank sends to
    rank r (check a; `ordered`: in that order too), or check(exchange): a check of its own; peer_fail: the agreement (1, 2, 3)
    at which a peer reports a failure.  The harness fills real_agree, real_counts and sent[r]."""

    def __init__(self, dtypes, to_real, peer_max, expect_sent=None, ordered=False, check=None, peer_fail=None, name="exchange"):
        self.dtypes = [np.dtype(d) for d in dtypes]
        self.to_real, self.peer_max, self.expect_sent, self.ordered, self.check, self.peer_fail, self.name = (
            to_real, int(peer_max), expect_sent, ordered, check, peer_fail, name)
        self.real_agree = self.real_counts = self.sent = None
        self.complete = False


class Final:
    """the join's last agreement: all_reduce_i64 max over two values"""

    def __init__(self, peer_values=(0, 0)):
        self.peer_values = list(peer_values)
        self.real_values = None


class Violation(Exception):
    pass


class World:
    """W ranks, one of them real.  script: Exchange / Final objects, or callables (world) -> Exchange evaluated when the exchange
    opens (a response depends on what the real rank asked).  with_v: the transport has the fifth function.  fail_at: the index
    of the callback invocation that returns non-zero without doing anything (a failing transport)."""

    def __init__(self, world, real, with_v, script, backend=Host, fail_at=None):
        self.world, self.real, self.with_v, self.script, self.backend, self.fail_at = world, real, with_v, list(script), backend, fail_at
        self.log, self.violation, self.injected, self.ncalls = [], None, False, 0
        self.done = []                      # the script items that were opened, evaluated
        self.tickets, self.next_ticket = set(), 1
        self.stage, self.cur, self.col, self.blk = None, None, 0, 0
        self._advance()
        self._cbs = (_A2A(self._guard(self._all_to_all)), _WAIT(self._guard(self._wait)), _ALLRED(self._guard(self._all_reduce)),
                     _A2AV(self._guard(self._all_to_all_v)))          # kept alive with the world
        self.transport = Transport(None, real, world, self._cbs[0], self._cbs[1], self._cbs[2], C.cast(None, _DESTROY),
                                   self._cbs[3] if with_v else C.cast(None, _A2AV))

    @property
    def ptr(self):
        return C.addressof(self.transport)

    # -- the state machine --
    def _advance(self):
        if not self.script:
            self.stage, self.cur = "done", None
            return
        item = self.script.pop(0)
        self.cur = item                      # (a callable is evaluated when its first agreement arrives)
        self.stage = "final" if isinstance(item, Final) else "agree1"

    def _guard(self, fn):
        def cb(*args):
            try:
                i, self.ncalls = self.ncalls, self.ncalls + 1
                if self.violation:
                    return 1
                if self.fail_at == i:
                    self.injected = True
                    self.log.append(("failed", fn.__name__.lstrip("_")))
                    return 1
                if self.injected and fn.__name__ != "_wait":
                    raise Violation(f"{fn.__name__}: a collective after a transport call failed")
                return fn(*args)
            except Violation as e:
                self.violation = f"call {self.ncalls - 1}, stage {self.stage}: {e}"
                return 1
            except Exception as e:           # noqa: BLE001 -- a callback must not raise into C
                self.violation = f"call {self.ncalls - 1}, stage {self.stage}: harness error {e!r}"
                return 1
        return cb

    def _all_reduce(self, ctx, values, count, op):
        vals = [int(values[i]) for i in range(count)]
        self.log.append(("all_reduce", count, op, tuple(vals)))
        if self.tickets:
            raise Violation("all_reduce_i64 while an exchange has not been waited for")
        if op != 1:
            raise Violation(f"all_reduce_i64 with op {op}: every agreement of the protocol is a max")
        if self.stage == "final":
            if count != 2:
                raise Violation(f"the last agreement carries 2 values, not {count}")
            self.cur.real_values = vals
            res = [max(a, b) for a, b in zip(vals, self.cur.peer_values)]
            self.done.append(self.cur)
            self._advance()
        elif self.stage == "agree1":
            if count != 2:
                raise Violation(f"the first agreement carries 2 values, not {count}")
            if callable(self.cur):
                self.cur = self.cur(self)
            x = self.cur
            self.done.append(x)
            x.real_agree = vals
            res = [max(vals[0], x.peer_max), max(vals[1], 1 if x.peer_fail == 1 else 0)]
            self.blk = max(res[0], 1)
            self.stage = "aborted" if res[1] else "agree2"
        elif self.stage in ("agree2", "agree3"):
            if count != 1:
                raise Violation(f"the agreement carries 1 value, not {count}")
            res = [max(vals[0], 1 if self.cur.peer_fail == int(self.stage[-1]) else 0)]
            self.stage = "aborted" if res[0] else ("counts" if self.stage == "agree2" else "cols")
        elif self.stage == "aborted":
            raise Violation("a collective after an agreement said that a rank has failed")
        elif self.stage == "done":
            raise Violation("an extra agreement: the call's collectives are over")
        else:
            raise Violation("all_reduce_i64 where a block is due")
        for i, v in enumerate(res):
            values[i] = v
        return 0

    def _ticket(self, ticket):
        t, self.next_ticket = self.next_ticket, self.next_ticket + 1
        self.tickets.add(t)
        ticket[0] = t

    def _recv_counts(self):
        x = self.cur
        return [int(x.real_counts[s]) if s == self.real else len(x.to_real[s][0]) for s in range(self.world)]

    def _all_to_all(self, ctx, send, recv, nbytes, ticket):
        self.log.append(("all_to_all", int(nbytes)))
        x, W = self.cur, self.world
        if self.stage == "counts":
            if nbytes != 8:
                raise Violation(f"the counts travel as 8 bytes per rank, not {nbytes}")
            counts = self.backend.read(send, 8 * W).view(np.int64)
            if (counts < 0).any() or (not x.real_agree[1] and int(counts.max()) != x.real_agree[0]):
                raise Violation(f"counts {counts.tolist()} disagree with the largest partition {x.real_agree[0]} the rank agreed on")
            x.real_counts = counts.copy()
            x.sent = [[] for _ in range(W)]
            self.backend.write(recv, np.array(self._recv_counts(), dtype=np.int64).view(np.uint8))
            self._ticket(ticket)
            self.stage = "agree3" if self.with_v else "cols"
            self.col = 0
            return 0
        if self.stage != "cols":
            raise Violation({"done": "an extra exchange: the call's collectives are over",
                             "aborted": "a block posted after an agreement said that a rank has failed"}.get(self.stage, "all_to_all where an agreement is due"))
        if self.with_v:
            raise Violation("all_to_all for a column of a transport that has all_to_all_v")
        w = x.dtypes[self.col].itemsize
        if nbytes != w * self.blk:
            raise Violation(f"column {self.col}: a block of {nbytes} bytes, agreed were {self.blk} rows of {w} bytes")
        data = self.backend.read(send, nbytes * W).reshape(W, nbytes)
        out = np.full((W, nbytes), POISON, dtype=np.uint8)          # the padding behind a short block is poisoned
        for r in range(W):
            x.sent[r].append(data[r, :w * int(x.real_counts[r])].copy().view(x.dtypes[self.col]))
        for s in range(W):
            rows = x.sent[s][self.col] if s == self.real else np.ascontiguousarray(x.to_real[s][self.col], dtype=x.dtypes[self.col])
            if len(rows) > self.blk:
                raise Violation("harness: a peer's partition exceeds the agreed block")
            out[s, :w * len(rows)] = rows.view(np.uint8)
        self.backend.write(recv, out.reshape(-1))
        self._ticket(ticket)
        self._column_done()
        return 0

    def _all_to_all_v(self, ctx, send, send_off, recv, recv_off, ticket):
        self.log.append(("all_to_all_v",))
        x, W = self.cur, self.world
        if self.stage != "cols" or not self.with_v:
            raise Violation({"done": "an extra exchange: the call's collectives are over"}.get(self.stage, "all_to_all_v where it is not due"))
        w = x.dtypes[self.col].itemsize
        so = [int(send_off[i]) for i in range(W + 1)]
        ro = [int(recv_off[i]) for i in range(W + 1)]
        want_s = np.concatenate([[0], np.cumsum(w * x.real_counts)]).tolist()
        want_r = np.concatenate([[0], np.cumsum(w * np.array(self._recv_counts(), dtype=np.int64))]).tolist()
        if so != want_s:
            raise Violation(f"column {self.col}: send offsets {so} disagree with the counts {x.real_counts.tolist()} of {w}-byte rows")
        if ro != want_r:
            raise Violation(f"column {self.col}: receive offsets {ro} disagree with the counts received {self._recv_counts()}")
        data = self.backend.read(send, so[-1]) if so[-1] else np.zeros(0, np.uint8)
        for r in range(W):
            x.sent[r].append(data[so[r]:so[r + 1]].copy().view(x.dtypes[self.col]))
        parts = [x.sent[s][self.col] if s == self.real else np.ascontiguousarray(x.to_real[s][self.col], dtype=x.dtypes[self.col])
                 for s in range(W)]
        if ro[-1]:
            self.backend.write(recv, np.concatenate([p.view(np.uint8) for p in parts]))
        self._ticket(ticket)
        self._column_done()
        return 0

    def _column_done(self):
        self.col += 1
        if self.col == len(self.cur.dtypes):
            self.cur.complete = True
            self._advance()

    def _wait(self, ctx, ticket):
        self.log.append(("wait",))
        t = int(ticket or 0)
        if t not in self.tickets:
            raise Violation(f"wait for ticket {t}, which names no exchange that is under way")
        self.tickets.discard(t)
        return 0

    # -- after the call --
    def finish(self, complete=True):
        """the protocol was followed; with `complete`, to its end"""
        assert self.violation is None, self.violation
        assert not self.tickets or self.injected, f"{len(self.tickets)} exchanges were never waited for"
        if complete:
            assert self.stage == "done", f"the call stopped at stage {self.stage} with {len(self.script)} steps of the script left"

    def check_sent(self):
        """check (a): per destination, the rows the real rank sent are the rows the model sends"""
        for x in self.done:
            if isinstance(x, Final) or not x.complete:
                continue
            if x.check is not None:
                x.check(x)
            if x.expect_sent is None:
                continue
            for r in range(self.world):
                assert same_rows(x.sent[r], x.expect_sent[r], x.ordered), (
                    f"{x.name}: the real rank {self.real} sent rank {r} {len(x.sent[r][0])} rows, the model {len(x.expect_sent[r][0])}"
                    f" -- or other rows")


def shape_log(log):
    """the log without the values of the agreements: the sequence of the collectives"""
    return [e[:3] if e[0] == "all_reduce" else e for e in log]


def exchange_shape(ncols, with_v):
    """the callbacks of one complete exchange_blocks"""
    a2, a1 = ("all_reduce", 2, 1), ("all_reduce", 1, 1)
    if with_v:
        return [a2, a1, ("all_to_all", 8), ("wait",), a1] + [("all_to_all_v",)] * ncols + [("wait",)] * ncols
    return [a2, a1, ("all_to_all", 8)] + [None] * ncols + [("wait",)] * (ncols + 1)      # None: an all_to_all of width * blk bytes


def assert_shape(log, shapes):
    got, want = shape_log(log), [s for shape in shapes for s in shape]
    assert len(got) == len(want), (got, want)
    for g, w in zip(got, want):
        assert g[0] == "all_to_all" if w is None else g == w, (got, want)      # (the state machine checked the size)


# ---- numpy models of a rank ----------------------------------------------------------------------------------------------------------
def owner_of(key_cols, world):
    n = len(key_cols[0])
    return oracle.partition_ids(key_cols, world).astype(np.int64) if n else np.zeros(0, np.int64)


def split(cols, owner, world):
    return [[np.ascontiguousarray(c[owner == r]) for c in cols] for r in range(world)]


def concat(parts):
    """parts[s] = the columns from sender s -> the columns, sender by sender"""
    return [np.concatenate([p[c] for p in parts]) for c in range(len(parts[0]))]


def widen(v):
    return v.astype(np.float64 if v.dtype.kind == "f" else np.int64)


def group(op, keys, vals, out_dtype=None):
    if len(vals) == 0:
        return [k[:0].copy() for k in keys], np.zeros(0, dtype=out_dtype or vals.dtype)
    gk, ga = oracle.group_by(op, keys, vals, out_dtype)
    return [np.array(k) for k in gk], np.array(ga)


def group_masked(op, keys, vals, key_valids, val_valid, out_dtype=None):
    if len(vals) == 0:
        return [k[:0].copy() for k in keys], np.zeros(0, dtype=out_dtype or vals.dtype), np.zeros(0, dtype=bool)
    kv = np.ones(len(vals), dtype=bool)
    for v in key_valids or []:
        if v is not None:
            kv &= v
    if not kv.any():
        return [k[:0].copy() for k in keys], np.zeros(0, dtype=out_dtype or vals.dtype), np.zeros(0, dtype=bool)
    if val_valid is not None and not (kv & val_valid).any():                # no valid value anywhere: every group is null
        gk, _ = oracle.group_by("count", [k[kv] for k in keys], vals[kv], np.int64)
        g = len(gk[0])
        return [np.array(k) for k in gk], np.zeros(g, dtype=out_dtype or vals.dtype), np.full(g, op == "count")
    gk, ga, ok = oracle.group_by_masked(op, keys, vals, key_valids, val_valid, out_dtype)
    return [np.array(k) for k in gk], np.array(ga), np.array(ok)


class GroupByModel:
    """gdf_amd_dist_group_by: (key, partial) -- AVG: (key, widened partial sum, partial count) -- travel to Murmur3(key) % world"""

    def __init__(self, op, key_dtype, val_dtype):
        self.op, self.kd, self.vd = op, np.dtype(key_dtype), np.dtype(val_dtype)
        acc = np.dtype(np.float64 if self.vd.kind == "f" else np.int64)
        self.dtypes = {"avg": [self.kd, acc, np.dtype(np.int64)], "count": [self.kd, np.dtype(np.int64)]}.get(op, [self.kd, self.vd])
        self.out_dtype = {"avg": np.dtype(np.float64), "count": np.dtype(np.int64)}.get(op, self.vd)

    def send(self, shard, world):
        keys, vals = shard
        if self.op == "avg":
            gk, s = group("sum", [keys], widen(vals))
            _, c = group("count", [keys], widen(vals), np.int64)
            cols = [gk[0], s, c]
        elif self.op == "count":
            gk, c = group("count", [keys], vals, np.int64)
            cols = [gk[0], c]
        else:
            gk, a = group(self.op, [keys], vals)
            cols = [gk[0], a]
        return split(cols, owner_of([cols[0]], world), world)

    def finish(self, parts):
        cols = concat(parts)
        if self.op == "avg":
            gk, s = group("sum", [cols[0]], cols[1])
            _, c = group("sum", [cols[0]], cols[2])
            return [gk[0], s.astype(np.float64) / c.astype(np.float64)]
        gk, a = group("sum" if self.op == "count" else self.op, [cols[0]], cols[1])
        return [gk[0], a]

    def whole(self, shards):
        """the oracle over the concatenated shards.  AVG: the wrapped int64 (float64) sum, converted once, over the count."""
        keys, vals = np.concatenate([s[0] for s in shards]), np.concatenate([s[1] for s in shards])
        if self.op == "avg":
            gk, s = group("sum", [keys], widen(vals))
            _, c = group("count", [keys], vals, np.int64)
            return [gk[0], s.astype(np.float64) / c.astype(np.float64)]
        gk, a = group(self.op, [keys], vals, np.int64 if self.op == "count" else None)
        return [gk[0], a]

    def owner(self, result, world):
        return owner_of([result[0]], world)


class MinMaxSpecialsModel(GroupByModel):
    """MIN / MAX of float groups that are NaN only, hold infinities or zeros of both signs -- in plain numpy, whose min / max hand
    a NaN on (no group mixes NaN with numbers: that is unspecified).  Such results are compared with ==, under which NaN equals NaN
    here and -0.0 equals +0.0 (tests/groupby_values.py), never bit for bit."""

    def _reduce(self, keys, vals):
        uk = np.unique(keys)
        f = np.min if self.op == "min" else np.max
        return [uk, np.array([f(vals[keys == k]) for k in uk], dtype=vals.dtype)]

    def send(self, shard, world):
        cols = self._reduce(*shard)
        return split(cols, owner_of([cols[0]], world), world)

    def finish(self, parts):
        return self._reduce(*concat(parts))

    def whole(self, shards):
        return self._reduce(np.concatenate([s[0] for s in shards]), np.concatenate([s[1] for s in shards]))


def assert_same_groups(got, want, what):
    """(keys, aggregate) with one row per key, in any order: the same keys and ==-equal aggregates (NaN == NaN, -0.0 == 0.0)"""
    assert len(got[0]) == len(want[0]) and got[1].dtype == want[1].dtype, what
    og, ow = np.argsort(got[0], kind="stable"), np.argsort(want[0], kind="stable")
    np.testing.assert_array_equal(got[0][og], want[0][ow], what)
    np.testing.assert_array_equal(got[1][og], want[1][ow], what)


class GroupByMultiModel:
    """gdf_amd_dist_group_by_multi: (key columns, S, C) travel to the owner of the row hash; shard = (keys, key_valids, vals, val_valid)"""

    def __init__(self, op, key_dtypes, val_dtype):
        self.op, self.kds, self.vd = op, [np.dtype(d) for d in key_dtypes], np.dtype(val_dtype)
        self.nk = len(self.kds)
        self.sop = "sum" if op == "avg" else op
        self.sd = np.dtype((np.float64 if self.vd.kind == "f" else np.int64) if op == "avg" else self.vd)
        self.dtypes = self.kds + ([] if op == "count" else [self.sd]) + [np.dtype(np.int64)]
        self.out_dtype = {"avg": np.dtype(np.float64), "count": np.dtype(np.int64)}.get(op, self.vd)

    def send(self, shard, world):
        keys, kvs, vals, vv = shard
        gk, c, _ = group_masked("count", keys, vals, kvs, vv, np.int64)
        cols = list(gk)
        if self.op != "count":
            gk2, s, ok = group_masked(self.sop, keys, widen(vals) if self.op == "avg" else vals, kvs, vv)
            assert all(np.array_equal(a, b) for a, b in zip(gk, gk2)) and not s[~ok].any()
            cols.append(s.astype(self.sd))
        cols.append(c)
        return split(cols, owner_of(cols[:self.nk], world), world)

    def finish(self, parts):
        cols = concat(parts)
        keys, c = cols[:self.nk], cols[-1]
        gk, fc = group("sum", keys, c)
        if self.op == "count":
            return list(gk) + [fc, np.ones(len(fc), dtype=bool)]
        _, fs, ok = group_masked(self.sop, keys, cols[self.nk], None, c > 0)
        if self.op == "avg":
            with np.errstate(all="ignore"):
                fs = np.where(fc > 0, fs.astype(np.float64) / fc.astype(np.float64), 0.0)
        return list(gk) + [fs, ok]

    def whole(self, shards):
        keys = [np.concatenate([s[0][c] for s in shards]) for c in range(self.nk)]
        kvs = [None if shards[0][1][c] is None else np.concatenate([s[1][c] for s in shards]) for c in range(self.nk)]
        vals = np.concatenate([s[2] for s in shards])
        vv = None if shards[0][3] is None else np.concatenate([s[3] for s in shards])
        if self.op == "avg":                                                  # sums in the accumulator type, one division
            gk, s, ok = group_masked("sum", keys, widen(vals), kvs, vv)
            _, c, _ = group_masked("count", keys, vals, kvs, vv, np.int64)
            with np.errstate(all="ignore"):
                return list(gk) + [np.where(c > 0, s.astype(np.float64) / c.astype(np.float64), 0.0), ok]
        gk, a, ok = group_masked(self.op, keys, vals, kvs, vv, np.int64 if self.op == "count" else None)
        return list(gk) + [a, ok]

    def owner(self, result, world):
        return owner_of(result[:self.nk], world)


def np_join(pk, bk, how):
    """oracle.join with empty relations answered here; (probe index, build index), -1 = the missing side"""
    if len(pk) == 0 or len(bk) == 0:
        e = np.zeros(0, np.int32)
        if how == "inner" or (len(pk) == 0 and how == "left") or (len(pk) == 0 and len(bk) == 0):
            return e, e
        if len(bk) == 0:
            return np.arange(len(pk), dtype=np.int32), np.full(len(pk), -1, np.int32)
        return np.full(len(bk), -1, np.int32), np.arange(len(bk), dtype=np.int32)
    return oracle.join([pk], [bk], how)


class JoinModel:
    """gdf_amd_dist_shuffle_*join: (key, local row) of the build relation, then of the probe relation, travel to Murmur3(key) % world;
    shard = (probe keys, build keys)"""

    def __init__(self, how, key_dtype):
        self.how, self.kd = how, np.dtype(key_dtype)
        self.dtypes = [self.kd, np.dtype(np.int32)]

    def send_side(self, keys, world):
        return split([keys, np.arange(len(keys), dtype=np.int32)], owner_of([keys], world), world)

    @staticmethod
    def gids(parts):
        return np.concatenate([(np.int64(s) << 40) | p[1].astype(np.int64) for s, p in enumerate(parts)])

    def finish(self, build_parts, probe_parts):
        bk, pk = concat(build_parts)[0], concat(probe_parts)[0]
        bg, pg = self.gids(build_parts), self.gids(probe_parts)
        l, r = np_join(pk, bk, self.how)
        return [np.where(l >= 0, pg[np.maximum(l, 0)] if len(pg) else -1, -1).astype(np.int64),
                np.where(r >= 0, bg[np.maximum(r, 0)] if len(bg) else -1, -1).astype(np.int64)]

    def whole(self, shards):
        pk, bk = np.concatenate([s[0] for s in shards]), np.concatenate([s[1] for s in shards])
        pg = np.concatenate([(np.int64(r) << 40) | np.arange(len(s[0]), dtype=np.int64) for r, s in enumerate(shards)])
        bg = np.concatenate([(np.int64(r) << 40) | np.arange(len(s[1]), dtype=np.int64) for r, s in enumerate(shards)])
        l, r = np_join(pk, bk, self.how)
        return [np.where(l >= 0, pg[np.maximum(l, 0)] if len(pg) else -1, -1).astype(np.int64),
                np.where(r >= 0, bg[np.maximum(r, 0)] if len(bg) else -1, -1).astype(np.int64)]


class GatherModel:
    """gdf_amd_dist_gather: the local rows travel to their owners, (values, valid flag) per column travel back in arrival order;
    shard = (ids, columns, valids)"""
    ROW = (1 << 40) - 1

    def __init__(self, col_dtypes):
        self.cds = [np.dtype(d) for d in col_dtypes]
        self.resp_dtypes = [d for cd in self.cds for d in (cd, np.dtype(np.int8))]

    def requests(self, ids, rank, world):
        owner, row = ids >> 40, ids & self.ROW
        owner, row = np.where(ids == -1, rank, owner), np.where(ids == -1, -1, row)
        return split([row.astype(np.int32)], owner, world), owner

    @staticmethod
    def serve(rows, cols, valids):
        ok = rows >= 0
        out = []
        for c, v in zip(cols, valids):
            vals = np.zeros(len(rows), dtype=c.dtype)
            vals[ok] = c[rows[ok]]
            f = ok.astype(np.int8)
            if v is not None:
                f[ok] = v[rows[ok]]
            out += [vals, f]
        return out

    def whole(self, shards, rank):
        """what rank `rank` must get: per column (values, valid), straight from the shards the ids name"""
        ids = shards[rank][0]
        owner, row = ids >> 40, ids & self.ROW
        res = []
        for c in range(len(self.cds)):
            vals, ok = np.zeros(len(ids), dtype=self.cds[c]), np.zeros(len(ids), dtype=bool)
            for o in np.unique(owner[ids >= 0]).tolist():
                sel = (owner == o) & (ids >= 0)
                col, valid = shards[o][1][c], shards[o][2][c]
                vals[sel] = col[row[sel]]
                ok[sel] = True if valid is None else valid[row[sel]]
            res.append((vals, ok))
        return res


# ---- the real rank in numpy: the same callbacks over host buffers (the CPU tests) ----------------------------------------------------
class StandIn:
    """A numpy rank that speaks the wire through the transport's function pointers as exchange_blocks does.  `bug` makes one wrong
    move so that the CPU tests can watch the harness refuse it."""
    backend = Host
    name = "stand-in"

    def __init__(self, bug=None):
        self.bug = bug

    def exchange(self, tr, dtypes, parts, hard=None):
        """-> (error name or None, parts received per sender)"""
        W, bug = tr.world, self.bug
        counts = np.array([len(p[0]) for p in parts], dtype=np.int64)
        agree = (C.c_int64 * 2)(0 if hard else int(counts.max()), 1 if hard else 0)
        if bug == "skip_first_agreement":
            agree[0] = max(int(counts.max()), 1 << 20)
        elif tr.all_reduce_i64(tr.ctx, agree, 2, 1):
            return "GDF_C_ERROR", None
        if agree[1]:
            return hard or "GDF_C_ERROR", None
        blk = max(int(agree[0]), 1)
        flag = (C.c_int64 * 1)(0)
        if tr.all_reduce_i64(tr.ctx, flag, 1, 1):
            return "GDF_C_ERROR", None
        if flag[0]:
            return "GDF_C_ERROR", None
        scnt = counts.copy()
        if bug == "wrong_counts":
            scnt[int(counts.argmax())] += 1
        rcnt = np.zeros(W, dtype=np.int64)
        tickets = []

        def post(fn, *args):
            t = C.c_void_p()
            if fn(tr.ctx, *args, C.byref(t)):
                return False
            tickets.append(t)
            return True

        def settle():
            bad = [tr.wait(tr.ctx, t) for t in tickets]
            tickets.clear()
            return not any(bad)

        if not post(tr.all_to_all, scnt.ctypes.data, rcnt.ctypes.data, 8):
            return "GDF_C_ERROR", None
        if tr.all_to_all_v:
            if not settle():
                return "GDF_C_ERROR", None
            if bug != "skip_third_agreement":
                if tr.all_reduce_i64(tr.ctx, flag, 1, 1):
                    return "GDF_C_ERROR", None
                if flag[0]:
                    return "GDF_C_ERROR", None
            outs = []
            for c, dt in enumerate(dtypes):
                w = dt.itemsize
                send = np.concatenate([np.ascontiguousarray(p[c], dtype=dt) for p in parts]) if counts.sum() else np.zeros(1, dtype=dt)
                out = np.zeros(max(int(rcnt.sum()), 1), dtype=dt)
                so = (C.c_size_t * (W + 1))(*np.concatenate([[0], np.cumsum(w * counts)]).tolist())
                if bug == "wrong_offsets":
                    so[W] += w
                ro = (C.c_size_t * (W + 1))(*np.concatenate([[0], np.cumsum(w * rcnt)]).tolist())
                if not post(tr.all_to_all_v, send.ctypes.data, so, out.ctypes.data, ro):
                    settle()
                    return "GDF_C_ERROR", None
                outs.append(out[:int(rcnt.sum())])
            if not settle():
                return "GDF_C_ERROR", None
            cuts = np.cumsum(rcnt)[:-1]
            return None, [list(cols) for cols in zip(*[np.split(o, cuts) for o in outs])]
        sends, recvs = [], []
        for c, dt in enumerate(dtypes):
            w = dt.itemsize
            rows = blk + (1 if bug == "wrong_block" else 0)
            send = np.full((W, rows * w), 0x5A, dtype=np.uint8)
            for r, p in enumerate(parts):
                send[r, :w * len(p[c])] = np.ascontiguousarray(p[c], dtype=dt).view(np.uint8)
            recv = np.zeros((W, rows * w), dtype=np.uint8)
            sends.append(send)
            recvs.append(recv)
            if not post(tr.all_to_all, send.ctypes.data, recv.ctypes.data, rows * w):
                settle()
                return "GDF_C_ERROR", None
        if not settle():
            return "GDF_C_ERROR", None
        got = [[recvs[c][s, :dt.itemsize * int(rcnt[s])].copy().view(dt) for c, dt in enumerate(dtypes)] for s in range(W)]
        if bug == "extra_exchange":
            t = C.c_void_p()
            tr.all_to_all(tr.ctx, scnt.ctypes.data, rcnt.ctypes.data, 8, C.byref(t))
        return None, got

    # -- the entry points: model.send, the wire, model.finish --
    def group_by(self, model, shard, tr, hard=None):
        err, got = self.exchange(tr, model.dtypes, model.send(shard, tr.world) if not hard else [[np.zeros(0, d) for d in model.dtypes]] * tr.world, hard)
        return (err, None) if err else ("GDF_SUCCESS", model.finish(got))

    group_by_multi = group_by

    def join(self, model, shard, tr, hard=None):
        empty = [[np.zeros(0, d) for d in model.dtypes]] * tr.world
        err, bgot = self.exchange(tr, model.dtypes, empty if hard else model.send_side(shard[1], tr.world), hard)
        if err:
            return err, None
        err, pgot = self.exchange(tr, model.dtypes, model.send_side(shard[0], tr.world))
        if err:
            return err, None
        last = (C.c_int64 * 2)(0, 0)
        if tr.all_reduce_i64(tr.ctx, last, 2, 1) or last[1]:
            return "GDF_C_ERROR", None
        return "GDF_SUCCESS", model.finish(bgot, pgot)

    def gather(self, model, shard, tr, hard=None):
        ids, cols, valids = shard
        W, rank = tr.world, tr.rank
        if hard is None and ((ids < -1) | ((ids >> 40) >= W)).any():
            hard = "GDF_INVALID_API_CALL"
        n = 0 if hard else len(ids)
        owner, row = ids[:n] >> 40, ids[:n] & GatherModel.ROW
        owner, row = np.where(ids[:n] == -1, rank, owner), np.where(ids[:n] == -1, -1, row).astype(np.int32)
        order = np.argsort(owner, kind="stable")
        err, asked = self.exchange(tr, [np.dtype(np.int32)], split([row], owner, W), hard)
        if err:
            return err, None
        rows = [a[0] for a in asked]
        bad = any(((r >= len(cols[0])) & (r >= 0)).any() for r in rows)
        resp = [model.serve(np.where(r < len(cols[0]), r, -1), cols, valids) for r in rows]
        err, back = self.exchange(tr, model.resp_dtypes, resp, "GDF_INVALID_API_CALL" if bad else None)
        if err:
            return err, None
        back = concat(back)
        res = []
        for c, cd in enumerate(model.cds):
            vals, ok = np.zeros(n, dtype=cd), np.zeros(n, dtype=bool)
            vals[order], ok[order] = back[2 * c], back[2 * c + 1] != 0
            res.append((vals, ok))
        return "GDF_SUCCESS", res


# ---- the real rank on the device: the library through its C ABI ----------------------------------------------------------------------
class Device:
    """The entry points of libgdf.so, unchecked (the return code is part of what is tested); device bytes through gdf_amd_copy."""
    name = "device"

    def __init__(self, gdf):
        self.gdf = gdf
        self.cdll = gdf._binding._gdf_cdll
        self.backend = self

    # the two functions through which the harness touches device memory
    def read(self, ptr, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        if nbytes:
            self.gdf.libgdf.gdf_amd_copy(out.ctypes.data, ptr, nbytes, 0)
        return out

    def write(self, ptr, data):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if data.size:
            self.gdf.libgdf.gdf_amd_copy(ptr, data.ctypes.data, data.size, 1)

    def fn(self, name, argtypes):
        f = getattr(self.cdll, name)
        f.restype, f.argtypes = C.c_int, argtypes
        return f

    def error_name(self, rc):
        return self.cdll.gdf_error_get_name(rc).decode()

    def column(self, arr, gdf_dtype=None, valid=None):
        from libgdf_amd.columns import column_from_numpy
        return column_from_numpy(np.ascontiguousarray(arr), valid, GDF[gdf_dtype] if isinstance(gdf_dtype, str) else gdf_dtype)

    def take(self, col, dtype=None):
        """a library-allocated column -> (values, valid bits or None, the mask's bits behind the last row, null_count, gdf dtype); frees it"""
        n = int(col.size)
        dt = np.dtype(self.gdf.columns.GDF_TO_NP[int(col.dtype)] if dtype is None else dtype)
        vals = self.read(col.data, n * dt.itemsize).view(dt) if n else np.zeros(0, dt)
        valid = tail = None
        if col.valid:
            nb = (n + 7) // 8
            bits = np.unpackbits(self.read(col.valid, nb), bitorder="little") if nb else np.zeros(0, np.uint8)
            valid, tail = bits[:n].astype(bool), bits[n:]
        info = (vals, valid, tail, int(col.null_count), int(col.dtype))
        if col.data:
            self.gdf.libgdf.gdf_column_free(C.byref(col))
        return info

    def group_by(self, model, shard, tr, typed=False, key_gdf=None, cols=None):
        from libgdf_amd._binding import gdf_column
        P = C.POINTER(gdf_column)
        kc, vc = cols if cols else (self.column(shard[0], key_gdf), self.column(shard[1]))
        ok, oa = gdf_column(), gdf_column()
        if typed:
            rc = self.fn(f"gdf_amd_dist_group_by_{model.op}", [P, P, C.c_void_p, P, P])(kc.ptr, vc.ptr, tr, C.byref(ok), C.byref(oa))
        else:
            rc = self.fn("gdf_amd_dist_group_by", [C.c_int, P, P, C.c_void_p, P, P])(AGG_OP[model.op], kc.ptr, vc.ptr, tr, C.byref(ok), C.byref(oa))
        if rc:
            assert not ok.data and not oa.data
            return self.error_name(rc), None
        k, a = self.take(ok), self.take(oa)
        assert k[4] == kc.c.dtype and k[1] is None and a[1] is None
        assert a[4] == {"avg": GDF["float64"], "count": GDF["int64"]}.get(model.op, vc.c.dtype), "the aggregate's dtype"
        return "GDF_SUCCESS", [k[0], a[0]]

    def group_by_multi(self, model, shard, tr, key_gdfs=None):
        from libgdf_amd._binding import gdf_column
        from libgdf_amd.columns import column_array
        P = C.POINTER(gdf_column)
        keys, kvs, vals, vv = shard
        kcs = [self.column(k, key_gdfs[i] if key_gdfs else None, kvs[i]) for i, k in enumerate(keys)]
        vc = self.column(vals, None, vv)
        oks, oa = [gdf_column() for _ in keys], gdf_column()
        oks_arr = (P * len(keys))(*[C.pointer(k) for k in oks])
        rc = self.fn("gdf_amd_dist_group_by_multi", [C.c_int, C.c_int, C.POINTER(P), P, C.c_void_p, C.POINTER(P), P])(
            AGG_OP[model.op], len(keys), column_array(kcs), vc.ptr, tr, oks_arr, C.byref(oa))
        if rc:
            return self.error_name(rc), None
        ks = [self.take(k) for k in oks]
        for k, kc in zip(ks, kcs):
            assert k[4] == kc.c.dtype
        a = self.take(oa)
        g = len(a[0])
        assert a[4] == {"avg": GDF["float64"], "count": GDF["int64"]}.get(model.op, vc.c.dtype), "the aggregate's dtype"
        if model.op == "count":
            assert a[1] is None and a[3] == 0
            ok = np.ones(g, dtype=bool)
        else:
            ok = a[1]
            assert ok is not None and a[3] == g - int(ok.sum()), "null_count"
            assert not a[2].any(), "mask bits behind the last group"
            assert not a[0][~ok].any(), "the aggregate under a cleared bit is 0"
        return "GDF_SUCCESS", [k[0] for k in ks] + [a[0], ok]

    def join(self, model, shard, tr, key_gdf=None, cols=None):
        from libgdf_amd._binding import gdf_column
        P = C.POINTER(gdf_column)
        pc, bc = cols if cols else (self.column(shard[0], key_gdf), self.column(shard[1], key_gdf))
        op, ob = gdf_column(), gdf_column()
        name = {"inner": "gdf_amd_dist_shuffle_join", "left": "gdf_amd_dist_shuffle_left_join", "full": "gdf_amd_dist_shuffle_full_join"}[model.how]
        rc = self.fn(name, [P, P, C.c_void_p, P, P])(pc.ptr, bc.ptr, tr, C.byref(op), C.byref(ob))
        if rc:
            return self.error_name(rc), None
        p, b = self.take(op, np.int64), self.take(ob, np.int64)
        assert p[4] == GDF["int64"] and b[4] == GDF["int64"]
        return "GDF_SUCCESS", [p[0], b[0]]

    def gather(self, model, shard, tr, col_gdfs=None, cols=None, ids_col=None):
        from libgdf_amd._binding import gdf_column
        from libgdf_amd.columns import column_array
        P = C.POINTER(gdf_column)
        ids, data, valids = shard
        idc = ids_col if ids_col is not None else self.column(ids)
        ccs = cols if cols else [self.column(d, col_gdfs[i] if col_gdfs else None, valids[i]) for i, d in enumerate(data)]
        outs = [gdf_column() for _ in ccs]
        outs_arr = (P * len(ccs))(*[C.pointer(o) for o in outs])
        rc = self.fn("gdf_amd_dist_gather", [P, C.c_int, C.POINTER(P), C.c_void_p, C.POINTER(P)])(idc.ptr, len(ccs), column_array(ccs), tr, outs_arr)
        if rc:
            return self.error_name(rc), None
        res = []
        for o, cc in zip(outs, ccs):
            vals, ok, tail, nulls, dt = self.take(o)
            assert dt == cc.c.dtype
            assert ok is not None, "a gathered column always carries a mask"
            assert nulls == len(vals) - int(ok.sum()), "null_count"
            assert not tail.any(), "mask bits behind the last row"
            res.append((vals, ok))
        return "GDF_SUCCESS", res


# ---- one call in a virtual world, with the three checks ------------------------------------------------------------------------------
def assert_result(got, want, what):
    assert len(got) == len(want), what
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g.view(np.uint8) if g.dtype.kind == "f" else g,
                                                                            w.view(np.uint8) if w.dtype.kind == "f" else w), what


def failed_transport(w, err):
    """a transport call returned non-zero: GDF_C_ERROR at once, no further collective (tickets handed out may still be waited for)"""
    w.finish(complete=False)
    assert w.injected and err == "GDF_C_ERROR", (err, w.log)
    return w


def run_owner_call(model, shards, sends, world, real, with_v, rank, call, fail_at=None):
    """group-by entries: one exchange to the owner.  sends[s] = model.send(shards[s], world), computed once per world by the caller."""
    x = Exchange(model.dtypes, {s: sends[s][real] for s in range(world) if s != real},
                 max([len(sends[s][r][0]) for s in range(world) if s != real for r in range(world)], default=0), expect_sent=sends[real])
    w = World(world, real, with_v, [x], rank.backend, fail_at)
    err, got = call(model, shards[real], w.ptr if isinstance(rank, Device) else w.transport)
    if fail_at is not None:
        return failed_transport(w, err)
    w.finish()
    assert err == "GDF_SUCCESS", err
    assert_shape(w.log, [exchange_shape(len(model.dtypes), with_v)])
    w.check_sent()                                                                                   # (a)
    received = lambda r: [x.sent[r] if s == real else sends[s][r] for s in range(world)]
    nk = len(got) - (2 if isinstance(model, GroupByMultiModel) else 1)
    assert_result(got, model.finish(received(real)), "(b) the real rank's result for what it received")
    assert np.array_equal(np.lexsort(tuple(got[:nk][::-1])), np.arange(len(got[0]))), "the groups are not in ascending key order"
    assert (model.owner(got, world) == real).all(), "a group on a rank that does not own it"
    results = [got if r == real else model.finish(received(r)) for r in range(world)]
    union = [np.concatenate([res[c] for res in results]) for c in range(len(got))]
    assert same_rows(union, model.whole(shards)), "(c) the world's groups are not the oracle's over the concatenated shards"
    return w


def run_specials(model, shards, sends, world, real, with_v, rank, call, reference):
    """run_owner_call for MinMaxSpecialsModel: the same three checks with == in place of bits.  reference: (keys, aggregate) of the
    concatenated shards from an independent source (the single-GPU call; tests/groupby_values.py on the CPU)."""
    def check(x):                                                                                    # (a)
        for r in range(world):
            assert_same_groups(x.sent[r], sends[real][r], f"the partials sent to rank {r}")
    x = Exchange(model.dtypes, {s: sends[s][real] for s in range(world) if s != real},
                 max([len(sends[s][r][0]) for s in range(world) if s != real for r in range(world)], default=0), check=check)
    w = World(world, real, with_v, [x], rank.backend)
    err, got = call(model, shards[real], w.ptr if isinstance(rank, Device) else w.transport)
    w.finish()
    assert err == "GDF_SUCCESS", err
    w.check_sent()
    received = lambda r: [x.sent[r] if s == real else sends[s][r] for s in range(world)]
    assert_same_groups(got, model.finish(received(real)), "(b) the real rank's result for what it received")
    assert np.array_equal(np.sort(got[0]), got[0]) and (owner_of([got[0]], world) == real).all()
    results = [got if r == real else model.finish(received(r)) for r in range(world)]
    union = [np.concatenate([res[c] for res in results]) for c in range(2)]
    assert_same_groups(union, reference, "(c) the world's groups against the reference over the concatenated shards")
    return w


def run_join(model, shards, world, real, with_v, rank, call, sends=None, fail_at=None):
    bs, ps = sends if sends else ([model.send_side(s[1], world) for s in shards], [model.send_side(s[0], world) for s in shards])
    others = [s for s in range(world) if s != real]
    mk = lambda snd, name: Exchange(model.dtypes, {s: snd[s][real] for s in others},
                                    max([len(snd[s][r][0]) for s in others for r in range(world)], default=0), expect_sent=snd[real], name=name)
    xb, xp = mk(bs, "build side"), mk(ps, "probe side")
    w = World(world, real, with_v, [xb, xp, Final()], rank.backend, fail_at)
    err, got = call(model, shards[real], w.ptr if isinstance(rank, Device) else w.transport)
    if fail_at is not None:
        return failed_transport(w, err)
    w.finish()
    assert err == "GDF_SUCCESS", err
    assert_shape(w.log, [exchange_shape(2, with_v)] * 2 + [[("all_reduce", 2, 1)]])
    w.check_sent()                                                                                   # (a)
    recv = lambda x, snd, r: [x.sent[r] if s == real else snd[s][r] for s in range(world)]
    want = model.finish(recv(xb, bs, real), recv(xp, ps, real))
    assert same_rows(got, want), "(b) the real rank's pairs for what it received"
    results = [got if r == real else model.finish(recv(xb, bs, r), recv(xp, ps, r)) for r in range(world)]
    union = [np.concatenate([res[c] for res in results]) for c in range(2)]
    assert same_rows(union, model.whole(shards)), "(c) the world's pairs are not the oracle's join of the concatenated shards"
    return w, got


def run_gather(model, shards, world, real, with_v, rank, call, fail_at=None):
    """shards[r] = (ids, columns, valids).  The peers' answers are modelled from the requests the real rank really sent, in their order."""
    others = [s for s in range(world) if s != real]
    reqs = {s: model.requests(shards[s][0], s, world)[0] for s in range(world)}
    x1 = Exchange([np.int32], {s: reqs[s][real] for s in others}, max([len(reqs[s][r][0]) for s in others for r in range(world)], default=0),
                  expect_sent=reqs[real], name="requests")

    def answers(w):
        def check(x):                          # (a) for the answers: in the order the requests came, flag by flag, value by value
            for r in others:
                want = model.serve(reqs[r][real][0], shards[real][1], shards[real][2])
                for c in range(len(model.cds)):
                    f = want[2 * c + 1]
                    assert np.array_equal(x.sent[r][2 * c + 1], f), f"answer to rank {r}, column {c}: valid flags"
                    assert np.array_equal(x.sent[r][2 * c][f != 0], want[2 * c][f != 0]), f"answer to rank {r}, column {c}: values"
        to_real = {s: model.serve(x1.sent[s][0], shards[s][1], shards[s][2]) for s in others}
        # a peer answers every rank what that rank asked: its largest answer is its largest request received
        pmax = max([len(reqs[q][s][0]) for s in others for q in others] + [int(x1.real_counts[s]) for s in others], default=0)
        return Exchange(model.resp_dtypes, to_real, pmax, check=check, name="answers")

    w = World(world, real, with_v, [x1, answers], rank.backend, fail_at)
    err, got = call(model, shards[real], w.ptr if isinstance(rank, Device) else w.transport)
    if fail_at is not None:
        return failed_transport(w, err)
    w.finish()
    assert err == "GDF_SUCCESS", err
    assert_shape(w.log, [exchange_shape(1, with_v), exchange_shape(2 * len(model.cds), with_v)])
    w.check_sent()
    want = model.whole(shards, real)                                                                 # (b) and (c): the rows the ids name
    for c, ((gv, gok), (wv, wok)) in enumerate(zip(got, want)):
        assert np.array_equal(gok, wok), f"column {c}: valid bits"
        assert gv.dtype == wv.dtype and np.array_equal(gv[wok].view(np.uint8), wv[wok].view(np.uint8)), f"column {c}: values"
    return w
