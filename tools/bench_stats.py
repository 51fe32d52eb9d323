"""Whole-column reductions (csrc/reduce.hip) and quantiles (csrc/quantile.hip) at 1e9 rows: one JSON line per case.

    python tools/bench_stats.py [--rows 1000000000] [--reps 5] [--cases reduce,select,sort]

ms is the median of --reps timed calls after one warm-up call; algorithmic bytes are one read of the column (plus its validity
mask), the least any implementation must move; frac_of_8TBps = algorithmic bytes / ms / 8 TB/s; kernels_ms is the per-call time of
each kernel from the library's gdf_amd_profile_* events, taken on one extra call.  The sort-route medians (flag_sort_inplace) sort
a fresh copy of the column each call; the copy is not timed.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="reduce,select,sort")
    a = ap.parse_args()
    import numpy as np
    import torch
    import libgdf_amd as gdf
    from bench import read_profile
    from libgdf_amd._binding import rmmOptions_t
    from libgdf_amd.columns import Column, new_context
    gdf.librmm.rmmInitialize(C.byref(rmmOptions_t(1, 0, False)))
    lib = gdf._binding._gdf_cdll
    dev = torch.device("cuda", 0)
    n = a.rows
    cases = a.cases.split(",")
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED57A7)

    def timed(name, fn, alg_bytes, setup=None, extra=None):
        if setup:
            setup()
        fn()
        times = []
        for _ in range(a.reps):
            if setup:
                setup()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        if setup:
            setup()
        lib.gdf_amd_profile_reset()
        lib.gdf_amd_profile_enable(1)
        fn()
        torch.cuda.synchronize()
        lib.gdf_amd_profile_enable(0)
        prof = read_profile(gdf)
        dt = statistics.median(times)
        out = {"case": name, "rows": n, "ms": round(dt * 1e3, 3), "ms_all": [round(t * 1e3, 3) for t in times],
               "algorithmic_bytes": int(alg_bytes), "frac_of_8TBps": round(alg_bytes / dt / 8e12, 3),
               "kernels_ms": {k: round(v[0], 3) for k, v in prof.items()}}
        if extra:
            out.update(extra)
        print(json.dumps(out), flush=True)

    res = torch.zeros(16, dtype=torch.uint8, device=dev)
    if "reduce" in cases:
        x = torch.randint(-(2**62), 2**62, (n,), dtype=torch.int64, device=dev, generator=g)
        c = Column(x)
        timed("gdf_sum_generic int64", lambda: gdf.libgdf.gdf_sum_generic(c.ptr, res.data_ptr(), 1), 8.0 * n)
        del c, x
        x = torch.rand(n, dtype=torch.float64, device=dev, generator=g)
        mask = torch.randint(0, 256, ((n + 7) // 8,), dtype=torch.uint8, device=dev, generator=g)      # ~50 % valid
        c = Column(x, mask)
        timed("gdf_sum_generic float64, 50% null mask", lambda: gdf.libgdf.gdf_sum_generic(c.ptr, res.data_ptr(), 1), 8.0 * n + n / 8)
        del c, x, mask
        x = torch.rand(n, dtype=torch.float32, device=dev, generator=g)
        c = Column(x)
        timed("gdf_min_generic float32", lambda: gdf.libgdf.gdf_min_generic(c.ptr, res.data_ptr(), 1), 4.0 * n)
        del c, x
        x = torch.randint(-128, 128, (n,), dtype=torch.int8, device=dev, generator=g)
        c = Column(x)
        timed("gdf_sum_generic int8", lambda: gdf.libgdf.gdf_sum_generic(c.ptr, res.data_ptr(), 1), 1.0 * n)
        del c, x
        torch.cuda.empty_cache()

    def median(col, inplace):
        ctx = new_context(flag_sorted=0, method=0, flag_sort_inplace=1 if inplace else 0)
        r = C.c_double()
        gdf.libgdf.gdf_quantile_exact(col.ptr, 0, 0.5, C.addressof(r), C.byref(ctx))
        return r.value

    columns = [("int64 uniform over 2^62", lambda: torch.randint(-(2**61), 2**61, (n,), dtype=torch.int64, device=dev, generator=g)),
               ("float64 uniform", lambda: torch.rand(n, dtype=torch.float64, device=dev, generator=g)),
               ("int64, 10 distinct values",
                lambda: torch.randint(-(2**62), 2**62, (10,), dtype=torch.int64, device=dev, generator=g)[
                    torch.randint(0, 10, (n,), device=dev, generator=g)])]
    for label, make in columns:
        x = make()
        want = None
        if "select" in cases:
            c = Column(x)
            want = median(c, False)
            timed(f"gdf_quantile_exact LINEAR median, {label} (radix select)", lambda: median(c, False), 8.0 * n,
                  extra={"value": want})
        if "sort" in cases:
            y = torch.empty_like(x)
            cy = Column(y)
            timed(f"gdf_quantile_exact LINEAR median, {label} (flag_sort_inplace)", lambda: median(cy, True), 8.0 * n,
                  setup=lambda: y.copy_(x), extra={"value": median(cy, True) if want is None else want,
                                                   "same_as_select": None if want is None else bool(median(Column(y.copy_(x)), True) == want)})
            del cy, y
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
