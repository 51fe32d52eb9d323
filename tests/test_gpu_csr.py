"""-m gpu: gdf_to_csr (csrc/csr.hip) against the numpy restatement of its contract (tests/csr_reference.py), exactly: A is compared
by bit pattern, so NaN payloads and -0.0 count.  Rows around every tile edge (R is read back from the route note), both emit routes,
every mask shape on its own, every dtype and mixed pair, and the call-level promises (determinism, inputs untouched, the nnz limit)."""
import ctypes as C

import numpy as np
import pytest

import csr_reference

pytestmark = pytest.mark.gpu

GDF_COLUMN_SIZE_TOO_BIG = 4
ROUTES = {"default": None, "chunk1": 1, "chunk2": 2}


class Csr:
    """one gdf_to_csr call through the raw C ABI: the error code and, on success, host copies of everything it returned"""

    def __init__(self, gdf, columns, mask_offset=0, rows=None):
        import torch
        from libgdf_amd._binding import csr_gdf, gdf_column
        from libgdf_amd.api import _hipMemcpyDtoD
        rows = len(columns[0][0]) if rows is None else rows
        self.keep, self.cols = [], []
        for arr, mask in columns:
            arr = np.ascontiguousarray(arr)
            data = torch.from_numpy(arr.copy()).cuda() if len(arr) else None
            c = gdf_column()
            c.data, c.size, c.dtype = (data.data_ptr() if data is not None else None), rows, csr_reference.NP_TO_GDF[arr.dtype]
            mbuf = None
            if mask is not None:
                # the mask bytes sit mask_offset bytes into an allocation, and 0xFF surrounds them: a read outside them counts wrong
                host = np.full(mask_offset + len(mask) + 16, 0xFF, dtype=np.uint8)
                host[mask_offset:mask_offset + len(mask)] = mask
                mbuf = torch.from_numpy(host).cuda()
                c.valid = mbuf.data_ptr() + mask_offset
            self.keep.append((data, mbuf))
            self.cols.append(c)
        arr_t = (C.POINTER(gdf_column) * len(self.cols))(*[C.pointer(c) for c in self.cols])
        csr = csr_gdf()
        C.memset(C.byref(csr), 0xAB, C.sizeof(csr))
        poisoned = bytes(csr)
        self.rc = gdf.libgdf.raw("gdf_to_csr")(arr_t, len(self.cols), C.byref(csr))
        if self.rc != 0:
            assert bytes(csr) == poisoned                                  # untouched on an error
            return
        self.nnz, self.rows, self.ncols, self.dtype = int(csr.nnz), int(csr.rows), int(csr.cols), int(csr.dtype)
        self.null_A, self.null_JA = not csr.A, not csr.JA
        npt = csr_reference.GDF_TO_NP[self.dtype]
        A = torch.empty(self.nnz, dtype=getattr(torch, npt.name), device="cuda")
        IA = torch.empty(self.rows + 1, dtype=torch.int64, device="cuda")
        JA = torch.empty(self.nnz, dtype=torch.int64, device="cuda")
        assert csr.IA
        _hipMemcpyDtoD(IA.data_ptr(), csr.IA, 8 * (self.rows + 1))
        if self.nnz:
            _hipMemcpyDtoD(A.data_ptr(), csr.A, self.nnz * A.element_size())
            _hipMemcpyDtoD(JA.data_ptr(), csr.JA, 8 * self.nnz)
        for p in (csr.A, csr.IA, csr.JA):
            if p:
                gdf.librmm.rmmFree(p, None)
        self.A, self.IA, self.JA = A.cpu().numpy(), IA.cpu().numpy(), JA.cpu().numpy()

    def inputs(self):
        return [(None if d is None else d.cpu().numpy(), None if m is None else m.cpu().numpy()) for d, m in self.keep]


def noted(gdf, name):
    v = C.c_longlong(-1)
    assert gdf.libgdf.gdf_amd_debug_noted(name.encode(), C.byref(v)) == 0, name
    return v.value


def check(gdf, columns, route="default", mask_offset=0, chunked_expected=None):
    """runs the call and compares everything with the reference; returns the Csr"""
    got = Csr(gdf, columns, mask_offset=mask_offset)
    assert got.rc == 0
    A, IA, JA, dtype = csr_reference.to_csr(columns)
    assert (got.rows, got.ncols, got.dtype, got.nnz) == (len(columns[0][0]), len(columns), dtype, len(JA))
    assert np.array_equal(got.IA, IA)
    assert got.IA[0] == 0 and got.IA[-1] == got.nnz == len(got.JA) and np.all(np.diff(got.IA) >= 0)
    assert np.array_equal(got.JA, JA)
    assert got.A.dtype == A.dtype and np.array_equal(csr_reference.bits_of(got.A), csr_reference.bits_of(A))
    assert (got.null_A, got.null_JA) == (got.nnz == 0, got.nnz == 0)
    if chunked_expected is not None:
        assert noted(gdf, "csr.route") == (1 if chunked_expected else 0)
    return got


def select(force_path, route):
    if ROUTES[route] is not None:
        force_path("GDF_CSR_CHUNKED", "1")
        force_path("GDF_CSR_CHUNK", ROUTES[route])


def random_mask(rng, rows, p):
    return np.packbits(rng.random_sample(rows) < p, bitorder="little")


def random_columns(rng, rows, ncols, dtypes=(np.float64,), p=0.5):
    cols = []
    for c in range(ncols):
        dt = np.dtype(dtypes[c % len(dtypes)])
        a = rng.randint(-100, 100, size=rows).astype(dt)
        cols.append((a, random_mask(rng, rows, p)))
    return cols


def tile_rows(gdf, ncols, dtype):
    """R of the route a call with this many columns of this dtype takes (a one-row call; the plan depends on cols and dtype only)"""
    Csr(gdf, [(np.zeros(1, dtype=dtype), None)] * ncols)
    return noted(gdf, "csr.rows_per_tile"), noted(gdf, "csr.route")


def edge_rows(R):
    return sorted({1, 7, 8, 9, 63, 64, 65, R - 1, R, R + 1, 3 * R + 5})


# ---- rows x cols ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [1, 2, 3, 17])
def test_rows_on_every_tile_edge(gdf, ncols):
    rng = np.random.RandomState(ncols)
    R, route = tile_rows(gdf, ncols, np.float64)
    assert route == 0 and R in (64, 128, 256)
    for rows in edge_rows(R):
        check(gdf, random_columns(rng, rows, ncols, (np.float64, np.int32)), chunked_expected=False)
        assert noted(gdf, "csr.rows_per_tile") == R


def test_wide_matrix_takes_the_chunked_route_on_its_own(gdf):
    """90 float64 columns: an image of 64 rows would need 64 * 90 * 12 bytes, more than the budget; several chunks per row"""
    rng = np.random.RandomState(90)
    R, route = tile_rows(gdf, 90, np.float64)
    assert route == 1 and R >= 64
    C_ = noted(gdf, "csr.chunk")
    assert 1 <= C_ < 90
    for rows in sorted({1, 65, R - 1, R, R + 1, 3 * R + 5}):
        check(gdf, random_columns(rng, rows, 90), chunked_expected=True)
    unmasked = [(a, None) for a, _ in random_columns(rng, R + 3, 90)]
    check(gdf, unmasked, chunked_expected=True)


@pytest.mark.parametrize("width", [1, 2])
@pytest.mark.parametrize("ncols", [3, 17])
def test_chunked_route_forced_equals_the_default_route(gdf, force_path, ncols, width):
    rng = np.random.RandomState(100 * ncols + width)
    R_default, _ = tile_rows(gdf, ncols, np.float64)
    force_path("GDF_CSR_CHUNKED", "1")
    force_path("GDF_CSR_CHUNK", width)
    R, route = tile_rows(gdf, ncols, np.float64)
    assert route == 1 and noted(gdf, "csr.chunk") == width
    for rows in sorted(set(edge_rows(R)) | {3 * R_default + 5}):
        cols = random_columns(rng, rows, ncols, (np.float64, np.int16))
        force_path("GDF_CSR_CHUNKED", None)
        a = check(gdf, cols, chunked_expected=False)
        force_path("GDF_CSR_CHUNKED", "1")
        b = check(gdf, cols, chunked_expected=True)
        assert np.array_equal(a.IA, b.IA) and np.array_equal(a.JA, b.JA)
        assert np.array_equal(csr_reference.bits_of(a.A), csr_reference.bits_of(b.A))


# ---- masks, each on its own ---------------------------------------------------------------------------------------------------------
def _mask_cases(rng, rows, R):
    full = lambda v: np.full((rows + 7) // 8, v, dtype=np.uint8)                 # noqa: E731
    yield "none", [None, None, None], 0
    yield "all set", [full(0xFF)] * 3, 0
    yield "all clear", [full(0x00)] * 3, 0
    yield "random 50 %", [random_mask(rng, rows, 0.5) for _ in range(3)], 0
    yield "random 3 %", [random_mask(rng, rows, 0.03) for _ in range(3)], 0
    yield "one unmasked column among masked ones", [random_mask(rng, rows, 0.5), None, random_mask(rng, rows, 0.5)], 0
    bits = rng.random_sample((3, rows)) < 0.7
    bits[:, R // 2 + 3] = False                                                   # a whole row clear in the middle of a tile
    bits[:, R + 1] = False
    bits[:, rows - 1] = False                                                     # ... and the last row
    yield "whole rows clear", [np.packbits(b, bitorder="little") for b in bits], 0
    tail = [random_mask(rng, rows, 0.5) for _ in range(3)]
    assert rows % 8 != 0
    for m in tail:
        m[-1] |= (0xFF << (rows % 8)) & 0xFF                                      # every bit beyond `rows` set
    yield "tail bits beyond rows set", tail, 0
    yield "mask pointer offset by 1", [random_mask(rng, rows, 0.5) for _ in range(3)], 1
    yield "mask pointer offset by 3", [random_mask(rng, rows, 0.5) for _ in range(3)], 3


MASK_CASE_NAMES = ["none", "all set", "all clear", "random 50 %", "random 3 %", "one unmasked column among masked ones",
                   "whole rows clear", "tail bits beyond rows set", "mask pointer offset by 1", "mask pointer offset by 3"]


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", MASK_CASE_NAMES)
def test_mask_shapes(gdf, force_path, name, route):
    select(force_path, route)
    R, _ = tile_rows(gdf, 3, np.int32)
    rows = 2 * R + 37
    rng = np.random.RandomState(7)
    cases = {n: (m, off) for n, m, off in _mask_cases(rng, rows, R)}
    assert list(cases) == MASK_CASE_NAMES
    masks, offset = cases[name]
    data = [rng.randint(-2**31, 2**31 - 1, size=rows).astype(np.int32) for _ in range(3)]
    got = check(gdf, list(zip(data, masks)), mask_offset=offset, chunked_expected=route != "default")
    if name == "all clear":
        assert got.nnz == 0 and got.null_A and got.null_JA and not got.IA.any() and len(got.IA) == rows + 1
    if name in ("none", "all set"):
        assert got.nnz == 3 * rows and np.array_equal(got.IA, 3 * np.arange(rows + 1))


def test_no_rows(gdf):
    got = Csr(gdf, [(np.zeros(0, dtype=np.int32), None), (np.zeros(0, dtype=np.float32), None)])
    assert got.rc == 0 and (got.rows, got.ncols, got.nnz, got.dtype) == (0, 2, 0, 5)
    assert got.null_A and got.null_JA and got.IA.tolist() == [0]


# ---- dtypes -------------------------------------------------------------------------------------------------------------------------
I8, I16, I32, I64, F32, F64 = np.int8, np.int16, np.int32, np.int64, np.float32, np.float64
F32_SPECIALS = np.array([np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1.1754942e-38, 3.4028235e38], dtype=np.float32)


def _with_specials(rng, rows, dtype, specials):
    """a column whose first len(specials) rows hold `specials`, all valid; the rest random at 50 %"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        a = (rng.random_sample(rows) * 2000 - 1000).astype(dtype)
    else:
        info = np.iinfo(dtype)
        a = rng.randint(info.min, info.max, size=rows, dtype=np.int64).astype(dtype)
    a[: len(specials)] = np.asarray(specials, dtype=dtype)
    valid = rng.random_sample(rows) < 0.5
    valid[: len(specials)] = True
    return a, np.packbits(valid, bitorder="little")


DTYPE_CASES = {
    "i8": [(I8, [-128, 127, 0, -1])],
    "i16": [(I16, [-32768, 32767, 0])],
    "i32": [(I32, [-2**31, 2**31 - 1, 0])],
    "i64": [(I64, [-2**63, 2**63 - 1, 0])],
    "f32": [(F32, F32_SPECIALS)],
    "f64": [(F64, [np.nan, np.inf, -np.inf, -0.0, 0.0, 5e-324, 1.7976931348623157e308])],
    "i8+i64": [(I8, [-128, 127]), (I64, [-2**63, 2**63 - 1])],
    "i16+i32": [(I16, [-32768, 32767]), (I32, [-2**31, 2**31 - 1])],
    "i32+f32": [(I32, [2**24 + 1, -(2**24) - 3, 2**31 - 1, -2**31, 2**25 + 2]), (F32, F32_SPECIALS)],      # |v| > 2^24: rounds
    "i64+f64": [(I64, [2**53 + 1, -(2**53) - 3, 2**63 - 1, -2**63, 2**54 + 2]), (F64, [np.nan, -0.0])],     # |v| > 2^53: rounds
    "i64+f32": [(I64, [2**24 + 1, 2**53 + 1, 2**63 - 1, -2**63, -(2**40) - 1]), (F32, F32_SPECIALS)],
    "f32+f64": [(F32, F32_SPECIALS), (F64, [np.nan, -0.0, 5e-324])],
    "all six": [(I8, [-128]), (I16, [-32768]), (I32, [2**31 - 1]), (I64, [2**63 - 1]), (F32, F32_SPECIALS), (F64, [np.nan])],
}
DTYPE_RESULT = {"i8": 1, "i16": 2, "i32": 3, "i64": 4, "f32": 5, "f64": 6, "i8+i64": 4, "i16+i32": 3, "i32+f32": 5, "i64+f64": 6,
                "i64+f32": 5, "f32+f64": 6, "all six": 6}


@pytest.mark.parametrize("route", ["default", "chunk2"])
@pytest.mark.parametrize("name", list(DTYPE_CASES))
def test_dtypes_and_widening(gdf, force_path, name, route):
    select(force_path, route)
    rng = np.random.RandomState(len(name))
    rows = 77
    cols = [_with_specials(rng, rows, dt, sp) for dt, sp in DTYPE_CASES[name]]
    with np.errstate(all="ignore"):
        got = check(gdf, cols, chunked_expected=route != "default")
    assert got.dtype == DTYPE_RESULT[name]


def test_a_valid_nan_and_a_valid_zero_are_entries(gdf):
    a = np.array([0.0, np.nan, -0.0, 0.0, 3.0], dtype=np.float64)
    z = np.zeros(5, dtype=np.int32)
    got = check(gdf, [(a, np.array([0b00010111], dtype=np.uint8)), (z, np.array([0b00011111], dtype=np.uint8))])
    assert got.nnz == 9 and got.IA.tolist() == [0, 2, 4, 6, 7, 9]
    assert np.isnan(got.A[2]) and np.signbit(got.A[4]) and got.A[0] == 0.0


# ---- calls --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["default", "chunk2"])
def test_two_calls_are_bit_identical_and_leave_the_inputs_alone(gdf, force_path, route):
    select(force_path, route)
    rng = np.random.RandomState(5)
    R, _ = tile_rows(gdf, 5, np.float64)
    cols = random_columns(rng, 3 * R + 5, 5, (np.float32, np.float64, np.int8))
    a = check(gdf, cols)
    for (d, m), (arr, mask) in zip(a.inputs(), cols):
        assert np.array_equal(csr_reference.bits_of(d), csr_reference.bits_of(arr))
        assert np.array_equal(m[: len(mask)], mask) and np.all(m[len(mask):] == 0xFF)
    b = check(gdf, cols)
    assert a.IA.tobytes() == b.IA.tobytes() and a.JA.tobytes() == b.JA.tobytes() and a.A.tobytes() == b.A.tobytes()


def test_nnz_limit(gdf, force_path):
    """GDF_CSR_MAX_NNZ forced to 10: 11 entries are refused after the count pass, with and without masks; nothing stays allocated
    (the pool's free figure does not sink from one refused call to the next) and the next, smaller call succeeds"""
    force_path("GDF_CSR_MAX_NNZ", 10)
    bits = np.zeros((2, 20), dtype=bool)
    bits[0, :6] = True
    bits[1, 3:8] = True                                                            # 11 entries
    data = [np.arange(20, dtype=np.int32), np.arange(20, dtype=np.float32)]
    eleven = [(d, np.packbits(b, bitorder="little")) for d, b in zip(data, bits)]

    def free_bytes():
        free, total = C.c_size_t(), C.c_size_t()
        gdf.librmm.rmmGetInfo(C.byref(free), C.byref(total), None)
        return free.value

    assert Csr(gdf, eleven).rc == GDF_COLUMN_SIZE_TOO_BIG
    before = free_bytes()
    assert Csr(gdf, eleven).rc == GDF_COLUMN_SIZE_TOO_BIG
    assert free_bytes() >= before
    assert Csr(gdf, [(np.zeros(11, dtype=np.int8), None)]).rc == GDF_COLUMN_SIZE_TOO_BIG       # no mask: known on the host
    bits[1, 7] = False                                                             # 10 entries
    ten = [(d, np.packbits(b, bitorder="little")) for d, b in zip(data, bits)]
    assert check(gdf, ten).nnz == 10
    check(gdf, [(np.arange(10, dtype=np.int8), None)])


# ---- the Python wrapper -----------------------------------------------------------------------------------------------------------
def test_api_to_csr_round_trip(gdf):
    """scattering A by (row from IA, JA) into a dense matrix reproduces the valid entries of the columns"""
    import torch
    from libgdf_amd.columns import column_from_numpy
    rng = np.random.RandomState(11)
    rows, ncols = 300, 6
    arrays = [rng.randint(-1000, 1000, size=rows).astype(dt) for dt in (I8, I16, I32, I64, F32, F64)]
    valids = [rng.random_sample(rows) < 0.6 for _ in range(ncols)]
    valids[2] = None
    cols = [column_from_numpy(a, v) for a, v in zip(arrays, valids)]
    A, IA, JA = gdf.to_csr(cols)
    assert gdf.api.to_csr is gdf.to_csr
    assert (A.dtype, IA.dtype, JA.dtype) == (torch.float64, torch.int32, torch.int64)
    A, IA, JA = A.cpu().numpy(), IA.cpu().numpy(), JA.cpu().numpy()
    assert len(IA) == rows + 1 and IA[0] == 0 and IA[-1] == len(A) == len(JA)
    dense = np.full((rows, ncols), np.nan)
    present = np.zeros((rows, ncols), dtype=bool)
    row_of = np.repeat(np.arange(rows), np.diff(IA))
    dense[row_of, JA] = A
    present[row_of, JA] = True
    for c in range(ncols):
        v = np.ones(rows, dtype=bool) if valids[c] is None else valids[c]
        assert np.array_equal(present[:, c], v)
        assert np.array_equal(dense[v, c], arrays[c][v].astype(np.float64))
