"""gdf_amd_semi_join (csrc/semijoin.hip): one JSON line per shape, appended to profiles/semi_join_bench.jsonl (--out).

    python tools/bench_semi_join.py [--rows 100000000] [--reps 5] [--out profiles/semi_join_bench.jsonl] [--only a,b,c,d,l,g] [--limit 300]

The yardstick is the parent commit's only route to the same rows: gdf_inner_join alone on the same columns (the caller's
de-duplication of its left index column is NOT counted, which favours the yardstick).  It is timed in the same process, its calls
alternating with gdf_amd_semi_join's, after one warm-up call of each; every call ends with its result written and released.  The line
carries both sides' minimum, median and maximum over --reps calls; the condition is that the semi join's MEDIAN is not above the
yardstick's MINIMUM ("met").  kernels_ms is the per-call time of each kernel from the library's gdf_amd_profile_* events, taken on one
extra call; route and distinct are what that call noted through the test hook (this tool loads it: LIBGDF_AMD_TESTHOOK=1).
Each shape runs in a child process of its own under a time limit of --limit seconds; the first shape that fails or runs out of time
ends the run.

  a  --rows int64 left rows, about half of them hitting; right = 2 000 unique keys
  b  the same; right = 1e6 unique keys
  c  the same; right = 1e7 rows, every key 8 times
  d  a masked (int32, float64) key pair (10 % nulls per column, 96 bits: the WIDE route), 1e7 left x 1e6 right rows
  l  the LDS route's bound: (a)'s left side against 500 ... 8192 unique keys, the LDS and the global route forced in turn (no yardstick)
  g  the global route beyond the caches: (a)'s left side against 1e5 ... 4e7 unique keys (no yardstick); table_bytes = slots * 8
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["LIBGDF_AMD_TESTHOOK"] = "1"      # the route notes and the forced routes need the hook library in front of libgdf.so

ROUTES = {0: "none", 1: "lds", 2: "global", 3: "wide"}


def parent(a):
    for shape in a.only.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--only", shape, "--rows", str(a.rows), "--reps", str(a.reps), "--out", a.out]
        try:
            rc = subprocess.run(cmd, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"shape {shape}: no result within {a.limit} s; stopping", flush=True)
            return 124
        if rc != 0:
            print(f"shape {shape}: exit status {rc}; stopping", flush=True)
            return rc
    return 0


def child(a):
    shape = a.only
    import torch
    import libgdf_amd as gdf
    from bench import read_profile
    from libgdf_amd._binding import gdf_column, rmmOptions_t
    from libgdf_amd.columns import Column, column_array
    gdf.librmm.rmmInitialize(C.byref(rmmOptions_t(1, 0, False)))
    lib = gdf._binding._gdf_cdll
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0x5E31)
    n = a.rows

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

    def noted(name):
        v = C.c_longlong(-1)
        return int(v.value) if gdf.libgdf.gdf_amd_debug_noted(name.encode(), C.byref(v)) == 0 else None

    def force(name, value):
        gdf.libgdf.gdf_amd_debug_force(name.encode(), None if value is None else str(value).encode())

    def kernels_of(call):
        lib.gdf_amd_profile_reset()
        lib.gdf_amd_profile_enable(1)
        call()
        torch.cuda.synchronize()
        lib.gdf_amd_profile_enable(0)
        return {k: round(v[0], 3) for k, v in read_profile(gdf).items()}

    def random_mask(rows, valid_frac):
        bits = torch.rand(((rows + 7) // 8, 8), device=dev, generator=g) < valid_frac
        return (bits.to(torch.int32) << torch.arange(8, device=dev, dtype=torch.int32)).sum(dim=1).to(torch.uint8)

    def unique_keys(distinct, repeat=1):
        """`distinct` unique int64 keys out of [0, 2 * distinct), each `repeat` times, shuffled"""
        keys = torch.randperm(2 * distinct, device=dev, generator=g)[:distinct]
        if repeat > 1:
            keys = keys.repeat_interleave(repeat)[torch.randperm(distinct * repeat, device=dev, generator=g)]
        return keys.contiguous()

    def stats(ts, prefix):
        return {prefix + "min_ms": round(min(ts), 3), prefix + "ms": round(statistics.median(ts), 3), prefix + "max_ms": round(max(ts), 3)}

    def semi_call(left, right):
        la, ra = column_array(left), column_array(right)
        sizes = []

        def call():
            out = gdf_column()
            gdf.libgdf.gdf_amd_semi_join(la, ra, len(left), 0, C.byref(out))
            sizes.append(int(out.size))
            gdf.libgdf.gdf_column_free(C.byref(out))

        call.keep = (la, ra, left, right)
        return call, sizes

    def measure(case, left, right, want_m, must_move, yardstick=True, extra=None):
        new, sizes = semi_call(left, right)

        def old():
            li, ri = gdf.api.join(left, right, how="inner", copy=False)
            pairs.append(li.numel())
            del li, ri

        pairs = []
        gdf.libgdf.gdf_amd_debug_noted(None, None)
        new()
        assert sizes[-1] == want_m, f"{case}: {sizes[-1]} rows, expected {want_m}"
        t_old, t_new = [], []
        if yardstick:
            old()
        for _ in range(a.reps):
            if yardstick:
                t_old.append(timed(old))
            t_new.append(timed(new))
        prof = kernels_of(new)
        line = {"case": case, "left_rows": int(left[0].size), "right_rows": int(right[0].size), "result_rows": want_m, "reps": a.reps}
        line.update(stats(t_new, ""))
        line["ms_all"] = [round(t, 3) for t in t_new]
        if yardstick:
            line.update(stats(t_old, "yardstick_"))
            line["yardstick_ms_all"] = [round(t, 3) for t in t_old]
            line["yardstick_pairs"] = pairs[-1]
            line["met"] = bool(statistics.median(t_new) <= min(t_old))
            line["ratio_to_yardstick_min"] = round(statistics.median(t_new) / min(t_old), 4)
        line.update({"must_move_bytes": int(must_move), "route": ROUTES.get(noted("sj_route")), "distinct": noted("sj_distinct"), "kernels_ms": prof})
        if extra:
            line.update(extra)
        emit(line)

    if shape in ("a", "b", "c", "l", "g"):
        configs = {"a": [(2_000, 1, None)], "b": [(1_000_000, 1, None)], "c": [(1_250_000, 8, None)],
                   "l": [(d, 1, r) for d in (500, 2_000, 4_096, 8_192) for r in (1, 2)],
                   "g": [(d, 1, None) for d in (100_000, 1_000_000, 10_000_000, 40_000_000)]}[shape]
        for distinct, repeat, forced in configs:
            right_keys = unique_keys(distinct, repeat)
            left_keys = torch.randint(0, 2 * distinct, (n,), dtype=torch.int64, device=dev, generator=g)
            present = torch.zeros(2 * distinct, dtype=torch.bool, device=dev)
            present[right_keys] = True
            want_m = int(present[left_keys].sum())
            del present
            force("GDF_SJ_ROUTE", forced)
            slots = 64
            while slots < 2 * distinct * repeat:
                slots *= 2
            name = {"a": "a: int64, right = 2 000 unique keys", "b": "b: int64, right = 1e6 unique keys", "c": "c: int64, right = 1e7 rows, every key 8 times",
                    "l": f"l: int64, right = {distinct} unique keys, route {ROUTES.get(forced)} forced",
                    "g": f"g: int64, right = {distinct:.0e} unique keys"}[shape]
            measure(name, [Column(left_keys)], [Column(right_keys)], want_m, 8 * n + 8 * distinct * repeat + 4 * want_m,
                    yardstick=shape in ("a", "b", "c"), extra={"forced_route": ROUTES.get(forced), "build_table_bytes": slots * 8})
            force("GDF_SJ_ROUTE", None)
            del left_keys, right_keys
            torch.cuda.empty_cache()
    elif shape == "d":
        nl, nr = min(n, 10_000_000), 1_000_000
        ids_r = torch.randperm(2 * nr, device=dev, generator=g)[:nr]
        ids_l = torch.randint(0, 2 * nr, (nl,), dtype=torch.int64, device=dev, generator=g)
        cols = lambda ids, rows: [Column((ids // 1000).to(torch.int32), random_mask(rows, 0.9), size=rows),
                                  Column((ids % 1000).to(torch.float64), random_mask(rows, 0.9), size=rows)]
        left, right = cols(ids_l, nl), cols(ids_r, nr)
        li, _ = gdf.api.join(left, right, how="inner")
        want_m = int(torch.unique(li).numel())
        del li
        measure("d: masked (int32, float64) pair, 1e7 x 1e6 rows", left, right, want_m, nl * 12 + nr * 12 + 2 * ((nl + 7) // 8 + (nr + 7) // 8) + 4 * want_m)
    else:
        raise SystemExit(f"unknown shape {shape}")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semi_join_bench.jsonl"))
    ap.add_argument("--only", default="a,b,c,d,l,g")
    ap.add_argument("--limit", type=int, default=300, help="seconds one shape's child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    sys.exit(child(a) if a.child else parent(a))


if __name__ == "__main__":
    main()
