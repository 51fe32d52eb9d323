"""numpy / Python restatement of the contract of gdf_amd_group_by_agg (include/gdf/gdf_amd_ext.h, csrc/groupby_agg.hip).  The reference
project has no such function; nothing here is derived from it.

A column is (data, valid): data a numpy array, valid a bool array or None (no mask = no nulls).  A request is (index into values or
None, "sum" | "min" | "max" | "avg" | "count"); (None, "count") is COUNT(*).

group_by_agg   groups by the stable lexicographic order of tests/order_reference.py (ascending, a column's nulls behind its values):
               two rows of that order that follow each other belong to one group when in every key column both are null, or both are
               valid with equal value images (-0.0 == +0.0, every NaN equals every NaN).  Float sums are math.fsum, i.e. exact.
               -> (key outputs, aggregate outputs), each an Out.
"""
import math
from collections import namedtuple

import numpy as np

import order_reference as ref

# data: one element per group (0 under a null); ok: bool per group; mask: the ceil(G / 64) * 8 mask bytes; dtype: gdf_dtype of the
# output; count / sum_abs: per group the number of valid values and the exact sum of their magnitudes (float SUM / AVG only, else None)
Out = namedtuple("Out", "data ok mask null_count dtype count sum_abs")

OPS = {"sum": 0, "min": 1, "max": 2, "avg": 3, "count": 4}                       # gdf_agg_op
INT8, INT16, INT32, INT64, FLOAT32, FLOAT64, DATE32, DATE64, TIMESTAMP = range(1, 10)
_GDF_OF_NP = {np.dtype(np.int8): INT8, np.dtype(np.int16): INT16, np.dtype(np.int32): INT32, np.dtype(np.int64): INT64,
              np.dtype(np.float32): FLOAT32, np.dtype(np.float64): FLOAT64}


def _null(col, n):
    return np.zeros(n, dtype=bool) if col[1] is None else ~np.asarray(col[1], dtype=bool)


def group_bounds(keys):
    """(perm, starts): the sorted row order and the positions in it at which a group begins"""
    n = len(keys[0][0])
    perm = ref.order_by_ex(keys).astype(np.int64)
    if n == 0:
        return perm, np.zeros(0, dtype=np.int64)
    head = np.zeros(n, dtype=bool)
    head[0] = True
    for col in keys:
        null = _null(col, n)[perm]
        img = ref.value_image(np.asarray(col[0]))[0][perm]
        differ = (null[1:] != null[:-1]) | (~null[1:] & ~null[:-1] & (img[1:] != img[:-1]))      # the data under a null bit is not compared
        head[1:] |= differ
    return perm, np.flatnonzero(head)


def _wrap64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def _out(data, ok, dtype, count=None, sum_abs=None):
    ok = np.asarray(ok, dtype=bool)
    data = np.where(ok, data, np.zeros(1, dtype=data.dtype)) if len(ok) else data
    return Out(data, ok, ref.mask_words(ok), int(len(ok) - ok.sum()), dtype, count, sum_abs)


def group_by_agg(keys, values, aggs, key_dtypes=None, value_dtypes=None):
    """key_dtypes / value_dtypes: gdf_dtype per column where it is not the numpy dtype's (DATE32, DATE64, TIMESTAMP)"""
    n = len(keys[0][0])
    perm, starts = group_bounds(keys)
    ends = np.append(starts[1:], n)
    G = len(starts)
    key_dtypes = key_dtypes or [None] * len(keys)
    value_dtypes = value_dtypes or [None] * len(values)

    key_outs = []
    for (data, valid), kd in zip(keys, key_dtypes):
        data = np.asarray(data)
        first = perm[starts]                                                    # the sort is stable: the group's first row in input order
        ok = np.ones(G, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)[first]
        key_outs.append(_out(data[first], ok, kd or _GDF_OF_NP[data.dtype]))

    agg_outs = []
    for col, op in aggs:
        assert op in OPS and (col is not None or op == "count")
        if col is None:
            agg_outs.append(_out((ends - starts).astype(np.int64), np.ones(G, dtype=bool), INT64))
            continue
        data, valid = values[col]
        data = np.asarray(data)
        vd = value_dtypes[col] or _GDF_OF_NP[data.dtype]
        ok_rows = ~_null((data, valid), n)
        is_float = data.dtype.kind == "f"
        if op in ("sum", "avg"):
            assert vd <= FLOAT64, "SUM and AVG take INT8 ... FLOAT64"
        res, cnt, sabs = [], np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.float64)
        for g in range(G):
            rows = perm[starts[g]:ends[g]]
            rows = rows[ok_rows[rows]]
            cnt[g] = len(rows)
            v = data[rows]
            if op == "count":
                res.append(len(rows))
            elif len(rows) == 0:
                res.append(0)
            elif op in ("sum", "avg"):
                if is_float:
                    s = math.fsum(float(x) for x in v)                          # float32 widens exactly
                    sabs[g] = math.fsum(abs(float(x)) for x in v)
                else:
                    s = _wrap64(sum(int(x) for x in v))                         # wraps modulo 2^64
                res.append(s if op == "sum" else float(s) / len(rows))
            else:                                                               # gdf_order_by's order: NaN above +inf
                img = ref.value_image(v)[0]
                res.append(v[np.argmin(img) if op == "min" else np.argmax(img)])
        if op == "count":
            agg_outs.append(_out(np.asarray(res, dtype=np.int64), np.ones(G, dtype=bool), INT64))
        elif op == "avg" or (op == "sum" and is_float):
            agg_outs.append(_out(np.asarray(res, dtype=np.float64), cnt > 0, FLOAT64, cnt, sabs if is_float else None))
        elif op == "sum":
            agg_outs.append(_out(np.asarray(res, dtype=np.int64), cnt > 0, INT64))
        else:
            agg_outs.append(_out(np.asarray(res, dtype=data.dtype), cnt > 0, vd))
    return key_outs, agg_outs
