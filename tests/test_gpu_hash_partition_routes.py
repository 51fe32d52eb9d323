"""-m gpu: gdf_hash_partition on every scatter route, at the shapes no other test reaches -- several tiles per chunk at one level
(GDF_HP_MAX_CHUNKS), 1- and 2-byte payloads, tables wider than 32 columns, the identity hash at one level, the 4-byte fast key,
P <= 2, the dispatch boundaries, unaligned bases and the error codes.  Every call asserts the notes the library left against the
case's recorded expectation and the route model, compares exactly against the numpy reference (hash_partition_cases.py) and
checks the sentinels around its outputs (hash_partition_gpu.py)."""
import ctypes as C

import numpy as np
import pytest

import hash_partition_cases as hp
from hash_partition_gpu import clear_notes, read_notes, run_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", hp.MULTI_TILE_CASES, ids=repr)
def test_several_tiles_per_chunk(gdf, force_path, case):
    """16 chunks of 24576 / 32768 rows: 3 / 4 pair tiles, 1.5 / 2 cols8 tiles, 2 / 2.67 fast and 4 / 5.33 generic tile-kernel tiles
    per chunk, and a last chunk of one row -- the cursor carried from tile to tile, the hist reset, the prefetch of the next tile, a
    full tile followed by a partial one.  The same call without the selector (2048-row chunks) must give the same offsets."""
    off16 = run_case(gdf, force_path, case)
    free = dict(case.expect)
    free["hp.nchunks"] = case.free_nchunks
    off = run_case(gdf, force_path, case, forced={}, expect=free)
    assert np.array_equal(off16, off)


@pytest.mark.parametrize("case", hp.WIDTH_CASES + hp.WIDE_CASES + hp.IDENTITY_CASES + hp.FAST4_CASES + hp.BOUNDARY_CASES + hp.UNALIGNED_CASES,
                         ids=repr)
def test_route(gdf, force_path, case):
    run_case(gdf, force_path, case)


def test_one_level_and_two_levels_agree_on_every_width(gdf, force_path):
    case = next(c for c in hp.WIDTH_CASES if c.id == "widths-two-level-P3000")
    two = run_case(gdf, force_path, case)
    one = run_case(gdf, force_path, case, forced={"GDF_HP_ONE_LEVEL": "1"}, expect=hp.notes_of(hp.DIRECT_FAST, 8, 1, 128))
    assert np.array_equal(one, two)


# gdf_error values (include/gdf/gdf.h)
GDF_SUCCESS, GDF_DATASET_EMPTY, GDF_INVALID_API_CALL, GDF_JOIN_TOO_MANY_COLUMNS, GDF_PARTITION_DTYPE_MISMATCH = 0, 5, 8, 10, 15


def test_error_codes_in_the_dispatcher_s_order(gdf):
    """The argument checks of gdf_hash_partition, in their order; no error leaves a note, and none writes the offsets."""
    import torch
    from libgdf_amd.columns import Column, column_array
    names = {v: gdf._binding._gdf_cdll.gdf_error_get_name(v).decode() for v in (5, 8, 10, 15)}
    assert names == {5: "GDF_DATASET_EMPTY", 8: "GDF_INVALID_API_CALL", 10: "GDF_JOIN_TOO_MANY_COLUMNS", 15: "GDF_PARTITION_DTYPE_MISMATCH"}
    fn = gdf.libgdf.raw("gdf_hash_partition")
    n = 100

    def cols(count, dtype=torch.int64, rows=n):
        return [Column(torch.arange(rows, dtype=dtype, device="cuda")) for _ in range(count)]

    def call(ins, outs, hashed, P, hash_func=0):
        offsets = (C.c_int * max(P, 1))(*([-7] * max(P, 1)))
        clear_notes(gdf)
        rc = fn(len(ins), column_array(ins), (C.c_int * len(hashed))(*hashed), len(hashed), P, column_array(outs), offsets, hash_func)
        if rc != GDF_SUCCESS:
            assert read_notes(gdf) == {} and all(o == -7 for o in offsets)
        return rc, list(offsets)

    ins, outs = cols(2), cols(2)
    assert call(ins, outs, [0], 16385)[0] == GDF_INVALID_API_CALL
    assert call(ins, outs, [0], 0)[0] == GDF_INVALID_API_CALL
    assert call(ins, outs, [0], -1)[0] == GDF_INVALID_API_CALL
    assert call(ins, outs, [-1], 4)[0] == GDF_INVALID_API_CALL
    assert call(ins, outs, [2], 4)[0] == GDF_INVALID_API_CALL
    assert call(ins, outs, [0, 2], 4)[0] == GDF_INVALID_API_CALL
    assert call(ins, cols(1) + cols(1, torch.float64), [0], 4)[0] == GDF_PARTITION_DTYPE_MISMATCH
    null_data = cols(2)
    null_data[1].c.data = None
    assert call(null_data, outs, [0], 4)[0] == GDF_DATASET_EMPTY
    assert call(ins, null_data, [0], 4)[0] == GDF_DATASET_EMPTY
    # a null data pointer is met before a dtype mismatch in a LATER column, a dtype mismatch before an unknown hash function
    assert call(null_data, cols(1, torch.float64) + cols(1), [0], 4)[0] == GDF_PARTITION_DTYPE_MISMATCH
    assert call(ins, cols(1) + cols(1, torch.float64), [0], 4, hash_func=9)[0] == GDF_PARTITION_DTYPE_MISMATCH
    # no rows: success, the offsets untouched, nothing noted (even P beyond the limit is not looked at)
    rc, offsets = call(cols(2, rows=0), cols(2, rows=0), [0], 4)
    assert rc == GDF_SUCCESS and offsets == [-7] * 4 and read_notes(gdf) == {}
    assert call(cols(2, rows=0), cols(2, rows=0), [0], 16385)[0] == GDF_SUCCESS
    # more key columns than a key table holds (MAX_KEY_COLS = 16, csrc/common.h; make_key_table): 16 pass, 17 do not
    ins, outs = cols(17, torch.int8), cols(17, torch.int8)
    assert call(ins, outs, list(range(17)), 4)[0] == GDF_JOIN_TOO_MANY_COLUMNS
    rc, offsets = call(ins, outs, list(range(16)), 4)
    assert rc == GDF_SUCCESS and offsets[0] == 0 and read_notes(gdf)["hp.route"] == hp.DIRECT_GENERIC
