"""Runs one case of hash_partition_cases.py through libgdf.gdf_hash_partition on the GPU and checks everything about the call:
the notes against the recorded expectation and the route model, the outputs with check_partition, the sentinels around every output
column, output mask and the offsets array, the mask-clearing contract and null_count.  Output columns and masks are SLICES of larger
buffers filled with a sentinel; output masks start as 0xff, so a library that forgot to clear them fails."""
import ctypes as C

import numpy as np

import hash_partition_cases as hp

GUARD = 64                    # bytes in front of and behind every output slice
DATA_SENTINEL, MASK_SENTINEL, OFFSET_SENTINEL, NULLS_SENTINEL = 0xA5, 0xFF, -7, 987654321


def clear_notes(gdf):
    assert gdf.libgdf.gdf_amd_debug_noted(None, None) == 0


def read_notes(gdf):
    """{name: value} of every hp.* note that is set"""
    out = {}
    for name in hp.NOTE_NAMES:
        v = C.c_longlong(-1)
        if gdf.libgdf.gdf_amd_debug_noted(name.encode(), C.byref(v)) == 0:
            out[name] = int(v.value)
    return out


def _torch_dtype(dt):
    import torch
    return getattr(torch, np.dtype(dt).name)


class OutSlice:
    """n elements of `dtype`, `off` elements past GUARD bytes into a sentinel-filled allocation"""

    def __init__(self, dtype, n, off):
        import torch
        self.w = np.dtype(dtype).itemsize
        self.lo = GUARD + off * self.w
        self.hi = self.lo + n * self.w
        self.buf = torch.full((self.hi + GUARD,), DATA_SENTINEL, dtype=torch.uint8, device="cuda")
        self.view = self.buf[self.lo:self.hi].view(_torch_dtype(dtype))

    def read(self, dtype):
        raw = self.buf.cpu().numpy()
        assert np.all(raw[:self.lo] == DATA_SENTINEL) and np.all(raw[self.hi:] == DATA_SENTINEL), "bytes outside the output column changed"
        return raw[self.lo:self.hi].view(dtype)


class OutMask:
    """mask_bytes(n) bytes (padded to 64 like an Arrow buffer), GUARD bytes into an allocation of 0xff bytes"""

    def __init__(self, n):
        import torch
        self.n, self.nbytes = n, hp.mask_bytes(n)
        self.padded = -(-self.nbytes // 64) * 64
        self.buf = torch.full((GUARD + self.padded + GUARD,), MASK_SENTINEL, dtype=torch.uint8, device="cuda")
        self.view = self.buf[GUARD:GUARD + self.padded]

    def read(self, written):
        """bool[n].  written: the mask travels -- bits from n on are 0, the bytes up to the next multiple of 4 may have been
        cleared, nothing beyond changed; otherwise every byte is unchanged"""
        raw = self.buf.cpu().numpy()
        if not written:
            assert np.all(raw == MASK_SENTINEL), "an output mask that does not travel was written"
            return None
        word_end = GUARD + -(-self.nbytes // 4) * 4
        assert np.all(raw[:GUARD] == MASK_SENTINEL), "bytes in front of the output mask changed"
        assert np.all(raw[word_end:] == MASK_SENTINEL), "bytes beyond the output mask's last word changed"
        pad = raw[GUARD + self.nbytes:word_end]
        assert np.all((pad == 0) | (pad == MASK_SENTINEL)), "padding bytes of the last mask word hold neither 0 nor their old value"
        bits = np.unpackbits(raw[GUARD:GUARD + self.nbytes], bitorder="little")
        assert not bits[self.n:].any(), "mask bits from n on are set"
        return bits[:self.n].astype(bool)


def upload(arr, off):
    """device tensor holding arr, starting `off` elements into its allocation"""
    import torch
    t = torch.empty(len(arr) + off, dtype=_torch_dtype(arr.dtype), device="cuda")
    t[off:].copy_(torch.from_numpy(np.array(arr)))
    return t[off:]


def call_partition(gdf, cols, masks, hashed, P, hash_func, out_masks, base_off=0):
    """gdf_hash_partition on sentinel-guarded outputs -> (got columns, got masks, offsets, output Column objects, input Columns)"""
    import torch
    from libgdf_amd.columns import Column, column_array, mask_from_bools
    n = len(cols[0])
    ins, outs, oslices, omasks = [], [], [], []
    for i, a in enumerate(cols):
        v, nulls = None, 0
        if masks[i] is not None:
            v = torch.from_numpy(mask_from_bools(masks[i])).cuda()
            nulls = int(n - np.count_nonzero(masks[i]))
        ins.append(Column(upload(a, base_off), v, null_count=nulls))
        s = OutSlice(a.dtype, n, base_off)
        m = OutMask(n) if i in out_masks else None
        oslices.append(s)
        omasks.append(m)
        outs.append(Column(s.view, m.view if m else None, null_count=NULLS_SENTINEL))
    offsets = (C.c_int * (P + 2))(*([OFFSET_SENTINEL] * (P + 2)))
    optr = C.cast(C.addressof(offsets) + C.sizeof(C.c_int), C.POINTER(C.c_int))
    hashed_arr = (C.c_int * len(hashed))(*hashed)
    gdf.libgdf.gdf_hash_partition(len(cols), column_array(ins), hashed_arr, len(hashed), P, column_array(outs), optr, hash_func)
    off = np.frombuffer(offsets, dtype=np.int32)
    assert off[0] == OFFSET_SENTINEL and off[-1] == OFFSET_SENTINEL, "the offsets array was written outside its P entries"
    got = [s.read(a.dtype) for s, a in zip(oslices, cols)]
    got_masks = [m.read(masks[i] is not None) if m is not None else None for i, m in enumerate(omasks)]
    for i, (ci, co) in enumerate(zip(ins, outs)):
        travels = masks[i] is not None and omasks[i] is not None
        assert co.c.null_count == (ci.c.null_count if travels else NULLS_SENTINEL), f"column {i}: null_count"
    return got, got_masks, off[1:-1].copy()


def run_case(gdf, force_path, case, forced=None, expect=None):
    """one call of the case (forced / expect override the case's own) -> offsets; everything else is asserted here"""
    forced = case.forced if forced is None else forced
    expect = case.expect if expect is None else expect
    cols, masks = hp.build_table(case)
    for k in ("GDF_HP_MAX_CHUNKS", "GDF_HP_ONE_LEVEL", "GDF_HP_NO_PAIRS", "GDF_HP_NO_COLS8", "GDF_HP_PIECE"):
        force_path(k, forced.get(k))
    clear_notes(gdf)
    got, got_masks, offsets = call_partition(gdf, cols, masks, case.hashed, case.P, case.hash_func, case.out_masks, case.base_off)
    notes = read_notes(gdf)
    assert notes == expect, (case.id, notes, expect)
    assert notes == case.model(forced), (case.id, "the model disagrees")
    if case.base_off:
        w = [d.itemsize for d in case.dtypes]
        assert any((case.base_off * x) % 16 for x in w)
    hp.check_partition(cols, masks, got, got_masks, offsets, case.hashed, case.P, case.hash_func, rowid=case.rowid)
    return offsets
