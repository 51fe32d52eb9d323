"""gdf_amd_group_by_agg (csrc/groupby_agg.hip): one JSON line per configuration, appended to profiles/groupby_agg_bench.jsonl (--out).

    python tools/bench_groupby_agg.py [--rows 100000000] [--reps 5] [--groups 10000,1600000] [--out profiles/groupby_agg_bench.jsonl]

The query:  SELECT k1, k2, SUM(a), AVG(a), MIN(b), MAX(b), COUNT(c), SUM(c) ... GROUP BY k1, k2  over two int32 key columns (uniform,
g1 x g2 = the group count, no null keys), a: int64, b: float64, c: float32 with a 50 % null mask.

  yardstick   the way the parent commit answers it: six gdf_group_by_<op> calls, GDF_HASH, every output with a mask and preallocated
              at `rows` elements (the group count is not known beforehand), flag_sort_result = 1 -- without it the six results cannot
              be laid side by side.  Allocation is outside the timed region.
  new         one gdf_amd_group_by_agg call; its outputs are released outside the timed region.

The timed calls of the two alternate in one process; ms is the median of --reps after one warm-up call each, with min and max.  Before
timing, the integer aggregates (the keys, SUM(a), COUNT(c)) of the two are checked equal.  kernels_ms: per-call time of every kernel
from the library's gdf_amd_profile_* events, taken on one extra call.  must_move_bytes: every input element and mask read once, every
output written once.  No ratio is promised: the line says which side wins.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUM, MIN, MAX, AVG, COUNT = 0, 1, 2, 3, 4


def factor(groups):
    """g1 x g2 = groups with g1 >= g2 as close as they come"""
    g2 = int(groups ** 0.5)
    while groups % g2:
        g2 -= 1
    return groups // g2, g2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--groups", default="10000,1600000")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "groupby_agg_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import libgdf_amd as gdf
    from bench import read_profile
    from libgdf_amd._binding import gdf_amd_agg, gdf_column, rmmOptions_t
    from libgdf_amd.api import _hipMemcpyDtoD
    from libgdf_amd.columns import GDF_HASH, Column, column_array, new_context
    gdf.librmm.rmmInitialize(C.byref(rmmOptions_t(1, 0, False)))
    lib = gdf._binding._gdf_cdll
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0x6B0A)
    n = a.rows
    torch_of = {3: torch.int32, 4: torch.int64, 5: torch.float32, 6: torch.float64}

    def emit(line):
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def kernels_of(call):
        lib.gdf_amd_profile_reset()
        lib.gdf_amd_profile_enable(1)
        call()
        torch.cuda.synchronize()
        lib.gdf_amd_profile_enable(0)
        return {k: round(v[0], 3) for k, v in read_profile(gdf).items()}

    def stats(times):
        return {"ms": round(statistics.median(times), 3), "ms_min": round(min(times), 3), "ms_max": round(max(times), 3),
                "ms_all": [round(t, 3) for t in times]}

    def mask_bytes(rows):
        return torch.zeros(((rows + 7) // 8 + 63) // 64 * 64, dtype=torch.uint8, device=dev)

    va = Column(torch.randint(-2**40, 2**40, (n,), dtype=torch.int64, device=dev, generator=g))
    vb = Column(torch.randn(n, dtype=torch.float64, device=dev, generator=g))
    bits = torch.rand(((n + 7) // 8, 8), device=dev, generator=g) < 0.5
    c_mask = (bits.to(torch.int32) << torch.arange(8, device=dev, dtype=torch.int32)).sum(dim=1).to(torch.uint8)
    c_nulls = n - int(bits.reshape(-1)[:n].sum().item())
    del bits
    vc = Column(torch.randn(n, dtype=torch.float32, device=dev, generator=g), c_mask, size=n, null_count=c_nulls)
    values = [va, vb, vc]
    requests = [(0, SUM), (0, AVG), (1, MIN), (1, MAX), (2, COUNT), (2, SUM)]
    names = ["SUM(a)", "AVG(a)", "MIN(b)", "MAX(b)", "COUNT(c)", "SUM(c)"]
    # the yardstick's six calls: (entry point, value column, output dtype as the parent's api.group_by callers choose it)
    old_calls = [("gdf_group_by_sum", va, 4), ("gdf_group_by_avg", va, 6), ("gdf_group_by_min", vb, 6), ("gdf_group_by_max", vb, 6),
                 ("gdf_group_by_count", vc, 4), ("gdf_group_by_sum", vc, 5)]

    for groups in [int(x) for x in a.groups.split(",")]:
        g1, g2 = factor(groups)
        keys = [Column(torch.randint(0, g1, (n,), dtype=torch.int32, device=dev, generator=g)),
                Column(torch.randint(0, g2, (n,), dtype=torch.int32, device=dev, generator=g))]
        ka, va_arr = column_array(keys), column_array(values)

        # ---- the yardstick
        ctx = new_context(method=GDF_HASH, flag_sort_result=1)
        old_outs = []
        for _, _, out_dtype in old_calls:
            ok = [Column(torch.empty(n, dtype=torch.int32, device=dev), mask_bytes(n), 3, size=n) for _ in keys]
            oa = Column(torch.empty(n, dtype=torch_of[out_dtype], device=dev), mask_bytes(n), out_dtype, size=n)
            old_outs.append((ok, column_array(ok), oa))

        def old():
            for (fn, vcol, _), (_, ok_arr, oa) in zip(old_calls, old_outs):
                getattr(gdf.libgdf, fn)(len(keys), ka, vcol.ptr, None, ok_arr, oa.ptr, C.byref(ctx))

        # ---- the new entry
        reqs = (gdf_amd_agg * len(requests))()
        for r, (col, op) in zip(reqs, requests):
            r.column, r.op = col, op
        new_k, new_a = [gdf_column() for _ in keys], [gdf_column() for _ in requests]
        nk_arr = (C.POINTER(gdf_column) * len(keys))(*[C.pointer(o) for o in new_k])
        na_arr = (C.POINTER(gdf_column) * len(requests))(*[C.pointer(o) for o in new_a])

        def new():
            gdf.libgdf.gdf_amd_group_by_agg(ka, len(keys), va_arr, len(values), reqs, len(requests), nk_arr, na_arr)

        def release():
            for o in new_k + new_a:
                gdf.libgdf.gdf_column_free(C.byref(o))

        def fetch(o, dtype):
            t = torch.empty(int(o.size), dtype=dtype, device=dev)
            _hipMemcpyDtoD(t.data_ptr(), o.data, t.numel() * t.element_size())
            return t

        # warm-up and the equality of the integer aggregates
        old(), new()
        G = int(new_k[0].size)
        assert all(int(oa.size) == G for _, _, oa in old_outs), "group counts differ"
        for c in range(len(keys)):
            got = fetch(new_k[c], torch.int32)
            assert all(torch.equal(got, ok[c].data[:G]) for ok, _, _ in old_outs), f"key column {c} differs"
        assert torch.equal(fetch(new_a[0], torch.int64), old_outs[0][2].data[:G]), "SUM(a) differs"
        assert torch.equal(fetch(new_a[4], torch.int64), old_outs[4][2].data[:G]), "COUNT(c) differs"
        assert all(int(o.null_count) == 0 for o in new_k)
        release()

        t_old, t_new = [], []
        for _ in range(a.reps):
            t_old.append(timed(old))
            t_new.append(timed(new))
            release()
        prof_old = kernels_of(old)
        prof_new = kernels_of(new)
        release()
        must = n * (4 + 4) + n * (8 + 8 + 4) + (n + 7) // 8 + G * (4 + 4 + 6 * 8) + 8 * ((G + 63) // 64 * 8)
        shape = {"rows": n, "groups": G, "keys": "2 x int32", "values": "int64, float64, float32 (50 % null)", "requests": names}
        emit({"case": "yardstick: six gdf_group_by_<op> calls, GDF_HASH, masks, sort_result", **shape, **stats(t_old), "kernels_ms": prof_old})
        m_old, m_new = statistics.median(t_old), statistics.median(t_new)
        emit({"case": "gdf_amd_group_by_agg: one call", **shape, **stats(t_new), "yardstick_ms": round(m_old, 3),
              "ratio_to_yardstick": round(m_new / m_old, 4), "faster": "gdf_amd_group_by_agg" if m_new < m_old else "six gdf_group_by_<op> calls",
              "must_move_bytes": int(must), "must_move_gb_per_s": round(must / m_new / 1e6, 1), "kernels_ms": prof_new})
        del keys, old_outs, ka
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
