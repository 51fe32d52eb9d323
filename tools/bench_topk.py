"""gdf_amd_top_k (csrc/topk.hip): one JSON line per configuration, appended to profiles/top_k_bench.jsonl (--out).

    python tools/bench_topk.py [--rows 100000000] [--reps 5] [--out profiles/top_k_bench.jsonl] [--only a,b,b65,t,s,e] [--slack N]

The yardstick is the parent commit's own path to the same rows: gdf_amd_order_by_ex over the whole table plus a device copy of
[offset, offset + k).  It is timed in the same process, its calls alternating with gdf_amd_top_k's, after one warm-up call of each;
ms is the median of --reps calls, every call ending with its result written.  The first call of both is compared element for element.
kernels_ms is the per-call time of each kernel from the library's gdf_amd_profile_* events, taken on one extra call; route,
candidates and select_passes are what that call noted through the test hook (this tool loads it: LIBGDF_AMD_TESTHOOK=1).
column_passes = the select passes that read the columns + tk_count; tk_emit reads again only the 512-row tiles that hold a candidate.
must_move_bytes = the key columns and their masks once, the output once.

  a    one int64 column (uniform in [0, 2^62)), no mask, k = 100
  b    the same column with a 10 % null mask, DESC
  b65  a FULL-RANGE int64 column with a 10 % null mask, DESC: 65 image bits, the 64-bit image is truncated
  t    one int8 column of 16 values: massive ties, a complete image
  s    (a) with K = k in {1e2, 1e4, 1e6, 1e7, 5e7}, each twice: the selection route forced (GDF_TK_MAX_K and GDF_TK_CAND_CAP lifted
       through the hook) and the library as shipped.  TK_MAX_K is the largest swept K at which the forced selection's median still
       lies under the yardstick's minimum; above it the shipped call takes the whole sort and must lie within the yardstick's min..max.
  e    top_k + gather of four int64 payload columns against order_by_ex + gather of the first k rows
  --slack N  forces GDF_TK_SLACK = N through the hook for every line (0: the select runs until T is exact) and says so in each line's
       "slack" field; without it the library's own TK_SLACK holds and the field is null.
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
os.environ["LIBGDF_AMD_TESTHOOK"] = "1"      # the route notes and the forced sweep need the hook library in front of libgdf.so


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "top_k_bench.jsonl"))
    ap.add_argument("--only", default="a,b,b65,t,s,e")
    ap.add_argument("--slack", type=int, default=None, help="force GDF_TK_SLACK through the test hook (0: an exact T)")
    a = ap.parse_args()
    only = set(a.only.split(","))
    import torch
    import libgdf_amd as gdf
    from bench import read_profile
    from libgdf_amd._binding import gdf_column, rmmOptions_t
    from libgdf_amd.api import _hipMemcpyDtoD
    from libgdf_amd.columns import Column, column_array
    gdf.librmm.rmmInitialize(C.byref(rmmOptions_t(1, 0, False)))
    lib = gdf._binding._gdf_cdll
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0x70B)
    n = a.rows

    def emit(line):
        line["slack"] = a.slack
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

    def noted(name):
        v = C.c_longlong(-1)
        return int(v.value) if gdf.libgdf.gdf_amd_debug_noted(name.encode(), C.byref(v)) == 0 else None

    def force(name, value):
        gdf.libgdf.gdf_amd_debug_force(name.encode(), None if value is None else str(value).encode())

    if a.slack is not None:
        force("GDF_TK_SLACK", a.slack)

    def kernels_of(call):
        lib.gdf_amd_profile_reset()
        lib.gdf_amd_profile_enable(1)
        call()
        torch.cuda.synchronize()
        lib.gdf_amd_profile_enable(0)
        return {k: round(v[0], 3) for k, v in read_profile(gdf).items()}

    def random_mask(valid_frac):
        bits = torch.rand(((n + 7) // 8, 8), device=dev, generator=g) < valid_frac
        return (bits.to(torch.int32) << torch.arange(8, device=dev, dtype=torch.int32)).sum(dim=1).to(torch.uint8)

    def calls(col, flag, k, offset=0):
        """(top_k call, its output tensor, yardstick call, its slice tensor)"""
        arr = column_array([col])
        flags = (C.c_uint8 * 1)(flag)
        m = max(0, min(k, n - offset))
        out = Column(torch.empty(max(m, 1), dtype=torch.int32, device=dev), None, 3, size=m)
        full = Column(torch.empty(n, dtype=torch.int32, device=dev))
        part = torch.empty(max(m, 1), dtype=torch.int32, device=dev)

        def new():
            gdf.libgdf.gdf_amd_top_k(arr, 1, flags, k, offset, out.ptr)

        def old():
            gdf.libgdf.gdf_amd_order_by_ex(arr, 1, flags, full.ptr)
            _hipMemcpyDtoD(part.data_ptr(), full.data.data_ptr() + 4 * offset, 4 * m)

        new.keep = old.keep = (arr, flags, col)
        return new, out.data[:m], old, part[:m]

    def measure(case, col, flag, k, width, masked, extra=None):
        new, got, old, want = calls(col, flag, k)
        gdf.libgdf.gdf_amd_debug_noted(None, None)
        old(), new()
        torch.cuda.synchronize()
        assert torch.equal(got, want), case + ": gdf_amd_top_k differs from gdf_amd_order_by_ex's slice"
        t_old, t_new = [], []
        for _ in range(a.reps):
            t_old.append(timed(old))
            t_new.append(timed(new))
        ms = statistics.median(t_new)
        prof = kernels_of(new)
        route, passes = noted("tk.route"), noted("tk.column_passes")
        line = {"case": case, "rows": n, "k": k, "offset": 0, "ms": round(ms, 3), "ms_all": [round(t, 3) for t in t_new],
                "yardstick_ms": round(statistics.median(t_old), 3), "yardstick_min_ms": round(min(t_old), 3), "yardstick_max_ms": round(max(t_old), 3),
                "below_yardstick_min": bool(ms < min(t_old)), "within_yardstick_spread": bool(min(t_old) <= ms <= max(t_old)),
                "ratio_to_yardstick": round(ms / statistics.median(t_old), 4),
                "must_move_bytes": int(n * width + (((n + 7) // 8) if masked else 0) + 4 * min(k, n)),
                "route": route, "select_passes": passes if route != 1 else 0, "column_passes": (passes + 1) if route == 0 else None,
                "candidates": noted("tk.candidates") if route != 1 else None, "kernels_ms": prof}
        if extra:
            line.update(extra)
        emit(line)
        return line

    if only & {"a", "b", "s", "e"}:
        keys = torch.randint(0, 2**62, (n,), dtype=torch.int64, device=dev, generator=g)
        plain = Column(keys)
        if "a" in only:
            measure("a: int64 in [0, 2^62), no mask, k = 100", plain, 0, 100, 8, False)
        if "b" in only:
            masked = Column(keys, random_mask(0.9), size=n)
            measure("b: the same column, 10 % nulls, DESC, k = 100", masked, 1, 100, 8, True)
            del masked
        if "s" in only:
            for K in (100, 10_000, 1_000_000, 10_000_000, 50_000_000):
                if K >= n:
                    continue
                force("GDF_TK_MAX_K", 2**62)
                force("GDF_TK_CAND_CAP", 2**62)
                measure(f"s: (a) with K = {K:.0e}, the selection route forced", plain, 0, K, 8, False, {"forced_selection": True})
                force("GDF_TK_MAX_K", None)
                force("GDF_TK_CAND_CAP", None)
                measure(f"s: (a) with K = {K:.0e}, as shipped", plain, 0, K, 8, False, {"forced_selection": False})
                torch.cuda.empty_cache()
        if "e" in only:
            k = 100
            payload = [Column(torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g)) for _ in range(4)]
            parr = column_array(payload)
            new, got, old, want = calls(plain, 0, k)
            outs = [gdf_column() for _ in payload]
            outs_arr = (C.POINTER(gdf_column) * 4)(*[C.pointer(o) for o in outs])
            idx_new, idx_old = Column(got), Column(want)

            def release():
                for o in outs:
                    gdf.libgdf.gdf_column_free(C.byref(o))

            def run(first, idx, check=None):
                first()
                gdf.libgdf.gdf_amd_gather(idx.ptr, 4, parr, outs_arr)
                if check is not None:
                    rows = torch.empty(k, dtype=torch.int64, device=dev)
                    _hipMemcpyDtoD(rows.data_ptr(), outs[3].data, k * 8)
                    check.append(rows)
                release()

            seen = []
            run(old, idx_old, seen), run(new, idx_new, seen)
            assert torch.equal(seen[0], seen[1]), "e: the gathered rows differ"
            t_old, t_new = [], []
            for _ in range(a.reps):
                t_old.append(timed(lambda: run(old, idx_old)))
                t_new.append(timed(lambda: run(new, idx_new)))
            ms = statistics.median(t_new)
            emit({"case": "e: top_k + gather of 4 x int64 against order_by_ex + gather of the first k rows, (a)'s key, k = 100", "rows": n, "k": k, "offset": 0,
                  "ms": round(ms, 3), "ms_all": [round(t, 3) for t in t_new], "yardstick_ms": round(statistics.median(t_old), 3),
                  "yardstick_min_ms": round(min(t_old), 3), "yardstick_max_ms": round(max(t_old), 3), "below_yardstick_min": bool(ms < min(t_old)),
                  "must_move_bytes": int(n * 8 + 4 * k + 4 * k * (8 + 8) + 4 * 8), "kernels_ms": kernels_of(lambda: run(new, idx_new)),
                  "route": noted("tk.route"), "select_passes": noted("tk.column_passes"),
                  "column_passes": (noted("tk.column_passes") + 1) if noted("tk.route") == 0 else None, "candidates": noted("tk.candidates")})
            del payload, parr
        del keys, plain
        torch.cuda.empty_cache()
    if "b65" in only:
        keys = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g)
        masked = Column(keys, random_mask(0.9), size=n)
        measure("b65: FULL-RANGE int64, 10 % nulls, DESC, k = 100 (65 image bits: a truncated image)", masked, 1, 100, 8, True)
        del masked, keys
        torch.cuda.empty_cache()
    if "t" in only:
        keys = torch.randint(0, 16, (n,), dtype=torch.int8, device=dev, generator=g)
        measure("t: one int8 column of 16 values, no mask, k = 100 (ties)", Column(keys), 0, 100, 1, False)
        del keys


if __name__ == "__main__":
    main()
