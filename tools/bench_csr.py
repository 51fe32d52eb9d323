"""gdf_to_csr (csrc/csr.hip): one JSON line per configuration, appended to profiles/csr_bench.jsonl (--out).

    python tools/bench_csr.py [--rows 100000000] [--wide-rows 1000000] [--reps 5] [--out profiles/csr_bench.jsonl]

ms is the median of --reps timed calls after one warm-up call (the call includes its allocations and the host round trip for nnz;
the returned buffers are released outside the timed region).  must_move_bytes is what any implementation has to move: the column
data and the masks once, plus A, JA and IA once.  memcpy_ms is a hipMemcpy device-to-device of must_move_bytes measured in the same
run (median of --reps), frac_of_memcpy = memcpy_ms / ms.  Such a copy reads AND writes that many bytes, twice the traffic of the
conversion; memcpy_half_ms is the copy of half as many bytes, whose traffic equals must_move_bytes.  kernels_ms is the per-call time
of each kernel from the library's gdf_amd_profile_* events, taken on one extra call.
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
    ap.add_argument("--wide-rows", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csr_bench.jsonl"))
    a = ap.parse_args()
    import torch
    import libgdf_amd as gdf
    from bench import read_profile
    from libgdf_amd._binding import csr_gdf, rmmOptions_t
    from libgdf_amd.api import _hipMemcpyDtoD
    from libgdf_amd.columns import Column, column_array
    gdf.librmm.rmmInitialize(C.byref(rmmOptions_t(1, 0, False)))
    lib = gdf._binding._gdf_cdll
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(0xC5A0)
    width = {torch.int32: 4, torch.float32: 4, torch.float64: 8}

    def make(rows, dtype, valid_frac):
        if dtype.is_floating_point:
            x = torch.rand(rows, dtype=dtype, device=dev, generator=g)
        else:
            x = torch.randint(-(2**31), 2**31 - 1, (rows,), dtype=dtype, device=dev, generator=g)
        mask = None
        if valid_frac is not None:
            bits = torch.rand(((rows + 7) // 8, 8), device=dev, generator=g) < valid_frac
            mask = (bits.to(torch.int32) << torch.arange(8, device=dev, dtype=torch.int32)).sum(dim=1).to(torch.uint8)
            del bits
        return Column(x, mask, size=rows)

    def memcpy_ms(nbytes):
        src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        src.zero_()
        dst.zero_()
        times = []
        for i in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _hipMemcpyDtoD(dst.data_ptr(), src.data_ptr(), nbytes)
            torch.cuda.synchronize()
            if i:
                times.append(time.perf_counter() - t0)
        return statistics.median(times) * 1e3

    def run(name, rows, dtypes, valid_frac):
        cols = [make(rows, dt, valid_frac) for dt in dtypes]
        arr = column_array(cols)
        csr = csr_gdf()

        def call(keep=False):
            gdf.libgdf.gdf_to_csr(arr, len(cols), C.byref(csr))
            info = (int(csr.nnz), int(csr.dtype))
            for p in (csr.A, csr.IA, csr.JA):
                if p and not keep:
                    gdf.librmm.rmmFree(p, None)
            return info

        call()
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            gdf.libgdf.gdf_to_csr(arr, len(cols), C.byref(csr))
            times.append(time.perf_counter() - t0)
            for p in (csr.A, csr.IA, csr.JA):
                if p:
                    gdf.librmm.rmmFree(p, None)
        lib.gdf_amd_profile_reset()
        lib.gdf_amd_profile_enable(1)
        nnz, out_dtype = call()
        torch.cuda.synchronize()
        lib.gdf_amd_profile_enable(0)
        prof = read_profile(gdf)
        out_w = {3: 4, 5: 4, 6: 8}[out_dtype]
        must = sum(rows * width[dt] for dt in dtypes) + (len(dtypes) * ((rows + 7) // 8) if valid_frac is not None else 0)
        must += nnz * out_w + nnz * 8 + (rows + 1) * 8
        del cols, arr
        torch.cuda.empty_cache()
        dt = statistics.median(times) * 1e3
        copy, half = memcpy_ms(must), memcpy_ms(must // 2)
        line = {"case": name, "rows": rows, "cols": len(dtypes), "nnz": nnz, "ms": round(dt, 3), "ms_all": [round(t * 1e3, 3) for t in times],
                "must_move_bytes": int(must), "memcpy_ms": round(copy, 3), "frac_of_memcpy": round(copy / dt, 3),
                "memcpy_half_ms": round(half, 3), "frac_of_memcpy_half": round(half / dt, 3),
                "kernels_ms": {k: round(v[0], 3) for k, v in prof.items()}}
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
        torch.cuda.empty_cache()

    n = a.rows
    run("8 x float32, no masks", n, [torch.float32] * 8, None)
    run("8 x float64, 50% valid", n, [torch.float64] * 8, 0.5)
    run("4 x int32 + 4 x float64, 90% valid", n, [torch.int32, torch.float64] * 4, 0.9)
    run("512 x float32, 50% valid (chunked route)", a.wide_rows, [torch.float32] * 512, 0.5)


if __name__ == "__main__":
    main()
