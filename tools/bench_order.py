"""gdf_amd_order_by_ex and gdf_amd_gather (csrc/order.hip): one JSON line per configuration, appended to
profiles/order_by_ex_bench.jsonl (--out).

    python tools/bench_order.py [--rows 100000000] [--reps 5] [--out profiles/order_by_ex_bench.jsonl] [--only a,b,b65,c] [--no-yardstick]

ms is the median of --reps timed calls after one warm-up call; every call ends with its result written (the entries synchronise);
kernels_ms is the per-call time of each kernel from the library's gdf_amd_profile_* events, taken on one extra call.

  a    one int64 column (uniform in [0, 2^62)), no mask, flags 0: gdf_order_by -- the parent commit's code, the yardstick -- and
       gdf_amd_order_by_ex in the same process, their timed calls alternating.  The new entry's line says whether its median lies
       within the yardstick's own min .. max over its repeats (within_yardstick_spread) or under the minimum (below_yardstick_min:
       the new entry writes 4-byte row numbers where gdf_order_by writes size_t).
  b    the same column with a 10 % null mask and DESC: ratio_to_a against the new entry's median of (a).  One more image bit (63
       instead of 62) and one mask read.
  b65  (b) over a FULL-RANGE int64 column: 64 value bits + the null bit = 65, so the null bit is sorted as a column group of its own
       (one more image, gathered through the permutation, and one more pass) -- the price of the 65-bit rule, DESIGN section 15.
  c    gdf_amd_gather of four int64 columns (no masks) by an int32 index column, once a random permutation and once the identity.
       must_move_bytes: the indices and the source elements once, the outputs and their masks once; memcpy_half_ms is a device-to-
       device hipMemcpy of HALF as many bytes (a copy reads and writes, so its traffic equals must_move_bytes), frac_of_memcpy_half =
       memcpy_half_ms / ms.  No target: random 8-byte gathers are latency-bound.
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
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "order_by_ex_bench.jsonl"))
    ap.add_argument("--only", default="a,b,b65,c")
    ap.add_argument("--no-yardstick", action="store_true", help="(a) without gdf_order_by: the new entry alone, for a counter run")
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
    g.manual_seed(0x0DE2)
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

    def order_by_call(col):
        arr = (gdf_column * 1)(col.c)
        d_cols = torch.empty(1, dtype=torch.int64, device=dev)
        d_types = torch.empty(1, dtype=torch.int32, device=dev)
        d_indx = torch.empty(n, dtype=torch.int64, device=dev)
        return (lambda: gdf.libgdf.gdf_order_by(n, arr, 1, d_cols.data_ptr(), d_types.data_ptr(), d_indx.data_ptr())), d_indx

    def order_by_ex_call(col, flag):
        arr = column_array([col])
        flags = (C.c_uint8 * 1)(flag)
        out = Column(torch.empty(n, dtype=torch.int32, device=dev))
        return (lambda: gdf.libgdf.gdf_amd_order_by_ex(arr, 1, flags, out.ptr)), out

    def stats(times):
        return {"ms": round(statistics.median(times), 3), "ms_all": [round(t, 3) for t in times]}

    ex_a_ms = None
    if only & {"a", "b"}:
        keys = torch.randint(0, 2**62, (n,), dtype=torch.int64, device=dev, generator=g)
        plain = Column(keys)
        if "a" in only and a.no_yardstick:
            new, new_out = order_by_ex_call(plain, 0)
            new()
            times = [timed(new) for _ in range(a.reps)]
            ex_a_ms = statistics.median(times)
            emit({"case": "a: gdf_amd_order_by_ex, int64 in [0, 2^62), no mask, flags 0 (alone)", "rows": n, **stats(times), "kernels_ms": kernels_of(new)})
            del new, new_out
        elif "a" in only:
            old, old_out = order_by_call(plain)
            new, new_out = order_by_ex_call(plain, 0)
            old(), new()
            assert torch.equal(old_out.to(torch.int32), new_out.data), "gdf_amd_order_by_ex differs from gdf_order_by"
            t_old, t_new = [], []
            for _ in range(a.reps):
                t_old.append(timed(old))
                t_new.append(timed(new))
            ex_a_ms = statistics.median(t_new)
            emit({"case": "a: gdf_order_by, int64 in [0, 2^62), no mask (the yardstick)", "rows": n, **stats(t_old), "kernels_ms": kernels_of(old)})
            emit({"case": "a: gdf_amd_order_by_ex, same column, no mask, flags 0", "rows": n, **stats(t_new),
                  "yardstick_min_ms": round(min(t_old), 3), "yardstick_max_ms": round(max(t_old), 3),
                  "within_yardstick_spread": bool(min(t_old) <= ex_a_ms <= max(t_old)), "below_yardstick_min": bool(ex_a_ms < min(t_old)),
                  "ratio_to_yardstick": round(ex_a_ms / statistics.median(t_old), 4), "kernels_ms": kernels_of(new)})
            del old, new, old_out, new_out
        if "b" in only:
            masked = Column(keys, random_mask(0.9), size=n)
            new, new_out = order_by_ex_call(masked, 1)
            new()
            times = [timed(new) for _ in range(a.reps)]
            line = {"case": "b: gdf_amd_order_by_ex, same column, 10 % nulls, DESC", "rows": n, **stats(times)}
            if ex_a_ms is not None:
                line["ratio_to_a"] = round(statistics.median(times) / ex_a_ms, 4)
            emit({**line, "kernels_ms": kernels_of(new)})
            del new, new_out, masked
        del keys, plain
        torch.cuda.empty_cache()
    if "b65" in only:
        keys = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g)
        masked = Column(keys, random_mask(0.9), size=n)
        new, new_out = order_by_ex_call(masked, 1)
        new()
        times = [timed(new) for _ in range(a.reps)]
        line = {"case": "b65: gdf_amd_order_by_ex, FULL-RANGE int64, 10 % nulls, DESC (65 image bits: two column groups)", "rows": n, **stats(times)}
        if ex_a_ms is not None:
            line["ratio_to_a"] = round(statistics.median(times) / ex_a_ms, 4)
        emit({**line, "kernels_ms": kernels_of(new)})
        del new, new_out, masked, keys
        torch.cuda.empty_cache()
    if "c" in only:
        cols = [Column(torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev, generator=g)) for _ in range(4)]
        arr = column_array(cols)
        must = n * 4 + 4 * (n * 8 + n * 8 + (n + 63) // 64 * 8)

        def memcpy_ms(nbytes):
            src = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            dst = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            return statistics.median([timed(lambda: _hipMemcpyDtoD(dst.data_ptr(), src.data_ptr(), nbytes)) for _ in range(a.reps + 1)][1:])

        for name, idx in (("a random permutation", torch.randperm(n, device=dev, generator=g).to(torch.int32)),
                          ("the identity", torch.arange(n, dtype=torch.int32, device=dev))):
            ic = Column(idx)
            outs = [gdf_column() for _ in cols]
            outs_arr = (C.POINTER(gdf_column) * 4)(*[C.pointer(o) for o in outs])

            def call(check=False):
                gdf.libgdf.gdf_amd_gather(ic.ptr, 4, arr, outs_arr)
                if check:
                    got = torch.empty(n, dtype=torch.int64, device=dev)
                    _hipMemcpyDtoD(got.data_ptr(), outs[3].data, n * 8)
                    assert torch.equal(got, cols[3].data[idx.long()]) and int(outs[3].null_count) == 0
                for o in outs:
                    gdf.libgdf.gdf_column_free(C.byref(o))

            call(check=True)
            times = []
            for _ in range(a.reps):                                   # (the outputs are released outside the timed region)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gdf.libgdf.gdf_amd_gather(ic.ptr, 4, arr, outs_arr)
                times.append((time.perf_counter() - t0) * 1e3)
                for o in outs:
                    gdf.libgdf.gdf_column_free(C.byref(o))
            prof = kernels_of(call)
            half = memcpy_ms(must // 2)
            ms = statistics.median(times)
            emit({"case": f"c: gdf_amd_gather, 4 x int64 by {name} (int32 indices)", "rows": n, **stats(times), "must_move_bytes": int(must),
                  "memcpy_half_ms": round(half, 3), "frac_of_memcpy_half": round(half / ms, 3),
                  "must_move_gb_per_s": round(must / ms / 1e6, 1), "kernels_ms": prof})
            del ic, idx
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
