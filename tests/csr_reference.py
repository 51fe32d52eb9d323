"""numpy restatement of the gdf_to_csr contract (the comment block above the prototype in include/gdf/gdf.h), written from that text
and not from csrc/csr.hip.  Pinned on a hand-written case by tests/test_csr_abi.py and used by the GPU tests of csrc/csr.hip."""
import numpy as np

# gdf_dtype enumerators INT8 .. FLOAT64 (include/gdf/gdf.h): the result dtype is the LARGEST enumerator among the columns
NP_TO_GDF = {np.dtype(np.int8): 1, np.dtype(np.int16): 2, np.dtype(np.int32): 3, np.dtype(np.int64): 4,
             np.dtype(np.float32): 5, np.dtype(np.float64): 6}
GDF_TO_NP = {v: k for k, v in NP_TO_GDF.items()}


def mask_bits(mask, rows):
    """Validity bits 0 .. rows - 1 of an LSB-first byte mask (None: all valid); bits of the last byte beyond `rows` do not count."""
    if mask is None:
        return np.ones(rows, dtype=bool)
    mask = np.asarray(mask, dtype=np.uint8)
    assert len(mask) >= (rows + 7) // 8
    return np.unpackbits(mask[: (rows + 7) // 8], bitorder="little")[:rows].astype(bool)


def to_csr(columns):
    """columns: list of (array, mask bytes or None), all arrays of one length = rows.  Returns (A, IA, JA, dtype): A in the result
    dtype (numpy array), IA int64[rows + 1], JA int64[nnz], dtype the gdf_dtype value.  Entry (r, c) exists exactly when bit r of
    column c's mask is set; rows are emitted in order, the columns of a row ascending; every value is converted with a plain cast
    (numpy astype, the C static_cast) to the result dtype -- a valid 0 or NaN is an entry like any other."""
    assert len(columns) > 0
    rows = len(columns[0][0])
    assert all(len(a) == rows for a, _ in columns)
    dtype = max(NP_TO_GDF[np.asarray(a).dtype] for a, _ in columns)
    out_np = GDF_TO_NP[dtype]
    valid = np.stack([mask_bits(m, rows) for _, m in columns], axis=1) if rows else np.zeros((0, len(columns)), dtype=bool)
    values = (np.stack([np.asarray(a).astype(out_np) for a, _ in columns], axis=1) if rows
              else np.zeros((0, len(columns)), dtype=out_np))
    A = values[valid]                                        # boolean indexing walks row-major: row by row, columns ascending
    JA = np.nonzero(valid)[1].astype(np.int64)
    IA = np.concatenate([[0], np.cumsum(valid.sum(axis=1))]).astype(np.int64)
    return np.ascontiguousarray(A), IA, JA, dtype


def bits_of(a):
    """The bit patterns of an array as unsigned integers: == on these tells NaN payloads and -0.0 apart."""
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
