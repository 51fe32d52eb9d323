"""Element-wise operators (csrc/elementwise.hip) at 1e9 rows: one JSON line per case, and the accuracy of the device math library.

    python tools/bench_elementwise.py [--rows 1000000000] [--reps 5] [--cases time,ulp] [--out profiles/elementwise_bench.jsonl]

Timing method of tools/bench_stats.py: ms is the median of --reps timed calls (host clock around the call and a device
synchronisation) after one warm-up call, ms_all has every repeat (its min and max are the run-to-run spread).  bytes is what the
call must move by contract: inputs + output (+ masks; these cases carry none).  frac_of_8TBps / frac_of_copy_ceiling are
bytes / ms against the 8 TB/s specification and the 6.29 TB/s device-to-device copy ceiling.  torch_ms is torch's own kernel for
the same operation on the same buffers in the same process, timed the same way (null where torch has none).
The ulp cases compare the nine transcendental functions with numpy on |x| <= 100 (asin / acos: [-1, 1]; log: (0, 100]) and on
the reference test's own draw U(-1, 1): the largest error in ulp and the input that has it.
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
    ap.add_argument("--cases", default="time,ulp")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import libgdf_amd as gdf
    from libgdf_amd.columns import GDF_DTYPES, Column, column_from_numpy
    dev = torch.device("cuda", 0)
    n = a.rows
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED57A7)
    sink = open(a.out, "w") if a.out else None

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def clock(fn):
        fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return statistics.median(times), [round(t * 1e3, 3) for t in times]

    def timed(name, fn, nbytes, torch_fn=None, note=None):
        dt, all_ms = clock(fn)
        row = {"case": name, "rows": n, "ms": round(dt * 1e3, 3), "ms_all": all_ms, "bytes": int(nbytes),
               "frac_of_8TBps": round(nbytes / dt / 8e12, 3), "frac_of_copy_ceiling": round(nbytes / dt / 6.29e12, 3),
               "torch_ms": None, "torch_ms_all": None}
        if torch_fn is not None:
            tdt, tall = clock(torch_fn)
            row.update(torch_ms=round(tdt * 1e3, 3), torch_ms_all=tall, vs_torch=round(dt / tdt, 3))
        if note:
            row["note"] = note
        emit(row)

    def rand_int(dtype, lo, hi):
        return torch.randint(lo, hi, (n,), dtype=dtype, device=dev, generator=g)

    if "time" in a.cases.split(","):
        lib = gdf.libgdf
        # add_f64, add_i32
        for name, make, width in (("gdf_add_f64", lambda: torch.rand(n, dtype=torch.float64, device=dev, generator=g), 8),
                                  ("gdf_add_i32", lambda: rand_int(torch.int32, -2**31, 2**31 - 1), 4)):
            x, y = make(), make()
            o = torch.empty_like(x)
            cx, cy, co = Column(x), Column(y), Column(o)
            timed(name, lambda: getattr(lib, name)(cx.ptr, cy.ptr, co.ptr), 3 * width * n, lambda: torch.add(x, y, out=o))
            del x, y, o, cx, cy, co
            torch.cuda.empty_cache()
        # lt_i64 -> int8 (torch writes bool, one byte too)
        x, y = rand_int(torch.int64, -2**40, 2**40), rand_int(torch.int64, -2**40, 2**40)
        o, ob = torch.empty(n, dtype=torch.int8, device=dev), torch.empty(n, dtype=torch.bool, device=dev)
        cx, cy, co = Column(x), Column(y), Column(o)
        timed("gdf_lt_i64", lambda: lib.gdf_lt_i64(cx.ptr, cy.ptr, co.ptr), 17 * n, lambda: torch.lt(x, y, out=ob))
        # cast_i64_to_f32 on the same input
        of = torch.empty(n, dtype=torch.float32, device=dev)
        cf = Column(of)
        timed("gdf_cast_i64_to_f32", lambda: lib.gdf_cast_i64_to_f32(cx.ptr, cf.ptr), 12 * n, lambda: of.copy_(x))
        # extract_datetime_year on TIMESTAMP(ns): torch has no such kernel
        x.copy_(rand_int(torch.int64, -2**62, 2**62))
        ct = Column(x, dtype=GDF_DTYPES["GDF_TIMESTAMP"], time_unit="ns")
        oy = torch.empty(n, dtype=torch.int16, device=dev)
        cyr = Column(oy)
        timed("gdf_extract_datetime_year TIMESTAMP(ns)", lambda: lib.gdf_extract_datetime_year(ct.ptr, cyr.ptr), 10 * n)
        del x, y, o, ob, of, oy, cx, cy, co, cf, ct, cyr
        torch.cuda.empty_cache()
        # bitwise_and_i8
        x, y = rand_int(torch.int8, -128, 128), rand_int(torch.int8, -128, 128)
        o = torch.empty_like(x)
        cx, cy, co = Column(x), Column(y), Column(o)
        timed("gdf_bitwise_and_i8", lambda: lib.gdf_bitwise_and_i8(cx.ptr, cy.ptr, co.ptr), 3 * n, lambda: torch.bitwise_and(x, y, out=o))
        del x, y, cx, cy
        # cast_f64_to_i8 into the same int8 output
        x = (torch.rand(n, dtype=torch.float64, device=dev, generator=g) - 0.5) * 200
        cx = Column(x)
        timed("gdf_cast_f64_to_i8", lambda: lib.gdf_cast_f64_to_i8(cx.ptr, co.ptr), 9 * n, lambda: o.copy_(x))
        del o, co
        # sin_f64 on the same input
        o = torch.empty_like(x)
        co = Column(o)
        timed("gdf_sin_f64", lambda: lib.gdf_sin_f64(cx.ptr, co.ptr), 16 * n, lambda: torch.sin(x, out=o),
              note="compute-bound: not in the memory-bound group")
        del x, o, cx, co
        torch.cuda.empty_cache()
        # sqrt_f32, sin_f32
        x = torch.rand(n, dtype=torch.float32, device=dev, generator=g) * 100
        o = torch.empty_like(x)
        cx, co = Column(x), Column(o)
        timed("gdf_sqrt_f32", lambda: lib.gdf_sqrt_f32(cx.ptr, co.ptr), 8 * n, lambda: torch.sqrt(x, out=o))
        timed("gdf_sin_f32", lambda: lib.gdf_sin_f32(cx.ptr, co.ptr), 8 * n, lambda: torch.sin(x, out=o))
        del x, o, cx, co
        torch.cuda.empty_cache()

    if "ulp" in a.cases.split(","):
        np_fn = dict(sin=np.sin, cos=np.cos, tan=np.tan, asin=np.arcsin, acos=np.arccos, atan=np.arctan, exp=np.exp, log=np.log)
        rng = np.random.RandomState(0xabcdef)
        m = 1 << 22
        for op in ("sin", "cos", "tan", "asin", "acos", "atan", "exp", "log"):
            for sfx, npt, bound in (("f32", np.float32, 4), ("f64", np.float64, 3)):
                for label, scale in (("reference draw U(-1,1)", 1.0), ("|x| <= 100", 100.0)):
                    if scale > 1 and op in ("asin", "acos"):
                        continue
                    x = ((rng.random_sample(m) * 2 - 1) * scale).astype(npt)
                    if op == "log":
                        x = np.abs(x) + np.finfo(npt).tiny
                    out = gdf.api.unary_op(op, column_from_numpy(x)).to_numpy()
                    with np.errstate(all="ignore"):
                        want = np_fn[op](x)
                    err = np.abs(out.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
                    err[~np.isfinite(err)] = 0
                    w = int(np.argmax(err))
                    emit({"case": f"ulp gdf_{op}_{sfx}", "range": label, "samples": m, "bound_ulp": bound, "max_ulp": round(float(err[w]), 3),
                          "within_bound": bool(err[w] <= bound), "over_bound": int((err > bound).sum()), "worst_input": float(x[w]),
                          "got": float(out[w]), "numpy": float(want[w])})


if __name__ == "__main__":
    main()
