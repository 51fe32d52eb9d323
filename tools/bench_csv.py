"""read_csv (csrc/csv.hip): one JSON line per file size, appended to profiles/csv_bench.jsonl (--out).

    python tools/bench_csv.py [--rows 100000 1000000 4000000] [--reps 5] [--out profiles/csv_bench.jsonl]

Writes a synthetic '|'-separated file in the 31-column mortgage performance schema (tests/golden/mortgage_schema.json; the rows are
invented) at every size and times, as the median of --reps calls after one warm-up call:
  read_csv_ms      read_csv on the file: open + mmap + one upload + the device work; the result is released outside the timed region
  upload_ms        the file's bytes host -> device alone (gdf_amd_copy from pageable memory), so that the upload is visible on its own
  device_ms        gdf_amd_read_csv_device on bytes that already sit in device memory
  pandas_ms / pyarrow_ms   pandas.read_csv (C engine) and pyarrow.csv.read_csv (16 threads) on the same file, same machine (the second
                   of two calls; pandas leaves the MM/YYYY column a string)
kernels_ms is the per-call time of each kernel from the library's gdf_amd_profile_* events on one extra call, and roofline the fraction
of the HBM rate (--hbm-tbs, 6.3 TB/s achievable) each kernel reaches by the byte accounting of DESIGN.md section 14:
  csv_count     reads the file's bytes
  csv_offsets   reads the file's bytes, writes 8 bytes per record
  csv_convert   reads the file's bytes and 8 bytes per record, writes the columns' elements and one mask bit per element
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WIDTH = {"int64": 8, "date": 8, "float64": 8, "category": 4}
BLOCK = 100_000


def write_file(path, total_rows, seed=1):
    """rows of the mortgage shape: a block of up to BLOCK invented rows, built column by column with numpy and written as often as
    it takes (building millions of distinct rows would take minutes; what the reader does per byte does not depend on it)"""
    rng = np.random.RandomState(seed)
    rows = min(total_rows, BLOCK)
    as_str = lambda a: a.astype(str)                                                           # noqa: E731

    def day():
        return np.char.add(np.char.add(np.char.zfill(as_str(rng.randint(1, 13, rows)), 2), "/"),
                           np.char.add(np.char.add(np.char.zfill(as_str(rng.randint(1, 29, rows)), 2), "/"), as_str(rng.randint(1999, 2020, rows))))

    def money():
        return np.where(rng.randint(0, 4, rows) == 0, np.char.mod("%.2f", rng.uniform(0, 50000, rows)), "")

    def pick(values):
        return np.array(values)[rng.randint(0, len(values), rows)]

    cols = [as_str(100000000000 + rng.randint(0, 10**9, rows)), day(), pick(["", "OTHER", "BANK OF SOMEWHERE, N.A.", "X"]),
            np.char.mod("%.3f", rng.uniform(2, 9, rows)), money(), as_str(rng.randint(0, 360, rows)), as_str(rng.randint(0, 360, rows)),
            money(), np.char.add(np.char.add(np.char.zfill(as_str(rng.randint(1, 13, rows)), 2), "/"), as_str(rng.randint(2020, 2050, rows))),
            as_str(rng.randint(10000, 50000, rows)), pick(["0", "1", "2", "X", ""]), pick(["N", "Y"]), pick(["", "01", "09"])]
    cols += [np.where(rng.randint(0, 8, rows) == 0, day(), "") for _ in range(4)]
    cols += [money() for _ in range(11)] + [pick(["", "Y", "N"]), money(), pick(["", "Y", "N"])]
    line = cols[0]
    for c in cols[1:]:
        line = np.char.add(np.char.add(line, "|"), c)
    line = line.tolist()
    with open(path, "w") as f:
        for start in range(0, total_rows, rows):
            f.write("\n".join(line[: min(rows, total_rows - start)]) + "\n")
    return os.path.getsize(path)


def median_ms(fn, reps, after=lambda r: None):
    times = []
    for i in range(reps + 1):
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        after(r)
        if i:
            times.append(dt * 1e3)
    return round(statistics.median(times), 3), [round(t, 3) for t in times]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[100_000, 1_000_000, 4_000_000])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=6.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csv_bench.jsonl"))
    ap.add_argument("--no-cpu", action="store_true", help="skip pandas and pyarrow")
    a = ap.parse_args()
    import torch
    import libgdf_amd as gdf
    from bench import read_profile
    from libgdf_amd import api
    from libgdf_amd._binding import rmmOptions_t
    gdf.librmm.rmmInitialize(C.byref(rmmOptions_t(1, 0, False)))
    lib = gdf._binding._gdf_cdll
    with open(os.path.join(ROOT, "tests", "golden", "mortgage_schema.json")) as f:
        schema = json.load(f)
    names, dtypes = schema["names"], schema["dtypes"]
    release = lambda args: gdf.libgdf.gdf_amd_read_csv_release(C.byref(args))                  # noqa: E731

    for rows in a.rows:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "performance.txt")
            nbytes = write_file(path, rows)

            def from_file():
                args = api.csv_args(names, dtypes, path, delimiter="|")
                gdf.libgdf.read_csv(C.byref(args))
                return args

            read_ms, read_all = median_ms(from_file, a.reps, release)
            host = np.fromfile(path, dtype=np.uint8)
            dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

            def upload():
                gdf.libgdf.gdf_amd_copy(dev.data_ptr(), host.ctypes.data, nbytes, 1)

            upload_ms, _ = median_ms(upload, a.reps)

            def from_buffer():
                args = api.csv_args(names, dtypes, delimiter="|")
                gdf.libgdf.gdf_amd_read_csv_device(dev.data_ptr(), nbytes, C.byref(args))
                return args

            device_ms, device_all = median_ms(from_buffer, a.reps, release)
            lib.gdf_amd_profile_reset()
            lib.gdf_amd_profile_enable(1)
            args = from_buffer()
            torch.cuda.synchronize()
            lib.gdf_amd_profile_enable(0)
            out_rows = int(args.num_rows_out)
            nulls = sum(int(args.data[c].contents.null_count) for c in range(len(names)))
            release(args)
            prof = {k: v[0] for k, v in read_profile(gdf).items() if k.startswith("csv_")}
            out_bytes = sum(WIDTH[d] for d in dtypes) * out_rows + len(dtypes) * ((out_rows + 63) // 64) * 8
            moved = {"csv_count": nbytes, "csv_offsets": nbytes + 8 * out_rows, "csv_convert": nbytes + 8 * out_rows + out_bytes}
            line = {"rows": out_rows, "cols": len(names), "file_bytes": nbytes, "output_bytes": out_bytes, "null_elements": nulls,
                    "read_csv_ms": read_ms, "read_csv_ms_all": read_all, "upload_ms": upload_ms, "device_ms": device_ms,
                    "device_ms_all": device_all, "file_gb_per_s_device": round(nbytes / device_ms / 1e6, 2),
                    "file_gb_per_s_read_csv": round(nbytes / read_ms / 1e6, 2),
                    "kernels_ms": {k: round(v, 4) for k, v in prof.items()}, "bytes_moved": moved,
                    "roofline": {k: round(moved[k] / (prof[k] * 1e-3) / (a.hbm_tbs * 1e12), 4) for k in moved if prof.get(k)},
                    "hbm_tbs": a.hbm_tbs}
            if not a.no_cpu:
                import pandas as pd
                import pyarrow as pa
                import pyarrow.csv as pacsv
                pa.set_cpu_count(16)
                pd_types = {n: ("float64" if d == "float64" else "int64" if d == "int64" else "str") for n, d in zip(names, dtypes)}
                dates = [n for n, d in zip(names, dtypes) if d == "date" and n != "maturity_date"]       # (that one is MM/YYYY)
                for n in dates:
                    del pd_types[n]
                pd_types["maturity_date"] = "str"
                line["pandas_ms"], _ = median_ms(lambda: pd.read_csv(path, sep="|", header=None, names=names, dtype=pd_types,
                                                                      parse_dates=dates, date_format="%m/%d/%Y"), 1)
                line["pyarrow_ms"], _ = median_ms(lambda: pacsv.read_csv(path, read_options=pacsv.ReadOptions(column_names=names),
                                                                          parse_options=pacsv.ParseOptions(delimiter="|")), 1)
                line["cpu_threads"] = pa.cpu_count()
            print(json.dumps(line), flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del dev
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
