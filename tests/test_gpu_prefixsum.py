"""-m gpu: every kernel family of csrc/scan.hip through the raw C ABI (gdf_prefixsum_i8 / _i32 / _i64 / _generic) against np.cumsum
in the column's dtype, exactly.  The sizes, value recipes and the dispatch model are prefixsum_cases.py's (checked on the CPU by
test_prefixsum_cases.py).

Every call here
  * scans a column that sits at a chosen element offset inside a buffer of 0xA5 bytes, into such a buffer: the guard bytes in front
    of and behind `out` must survive, and `in` must be unchanged unless the scan is in place;
  * asserts the notes the library left (scan.route, scan.bailed, scan.chunks, scan.chunk_elems) against the model, so a case that is
    named for a kernel family has run that family; scan.grid, which depends on the device, is read once per dtype (G, the resident grid
    of the rounds) and then held to min(G, tiles).
Values and expected scans live on the device; a comparison is one torch.equal, and only a failure is copied back to say where."""
import ctypes as C
import warnings

import numpy as np
import pytest

import prefixsum_cases as pc
from elementwise_common import col

pytestmark = pytest.mark.gpu

GUARD, PAD = 0xA5, 64
MODES = (("inclusive", True), ("exclusive", False))
TYPED = {np.dtype(np.int8): "gdf_prefixsum_i8", np.dtype(np.int32): "gdf_prefixsum_i32", np.dtype(np.int64): "gdf_prefixsum_i64"}


def _name(dtype):
    return np.dtype(dtype).name


def _tdtype(dtype):
    import torch
    return getattr(torch, _name(dtype))


class Slab:
    """n elements of dtype, `off` elements past PAD guard bytes into a 16-byte aligned device buffer filled with GUARD"""

    def __init__(self, dtype, n, off=0, payload=None):
        import torch
        self.dtype, self.n = np.dtype(dtype), n
        self.lo = PAD + off * self.dtype.itemsize
        self.hi = self.lo + n * self.dtype.itemsize
        self.t = torch.full((self.hi + PAD,), GUARD, dtype=torch.uint8, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        if payload is not None:
            assert payload.numel() == n
            self.t[self.lo:self.hi].copy_(payload.view(torch.uint8))
        self.ptr = self.t.data_ptr() + self.lo

    def elements(self):
        return self.t[self.lo:self.hi].view(_tdtype(self.dtype)) if self.dtype.kind == "i" else self.t[self.lo:self.hi]

    def guards_intact(self):
        return bool((self.t[:self.lo] == GUARD).all()) and bool((self.t[self.hi:] == GUARD).all())

    def untouched(self):
        return bool((self.t == GUARD).all())


class Device:
    """values and their inclusive scan on the device, at a table's largest size; a case takes prefixes"""

    def __init__(self, recipe, dtype, nmax):
        import torch
        self.dtype = np.dtype(dtype)
        a, inc = pc.values_and_scan(recipe, self.dtype.type, nmax)
        with warnings.catch_warnings():                  # (the cached arrays are read-only on purpose; they are only copied from)
            warnings.simplefilter("ignore", UserWarning)
            self.vals = torch.from_numpy(a).cuda()
            self.inc = torch.from_numpy(inc).cuda()

    def expected(self, n, inclusive):
        import torch
        if inclusive:
            return self.inc[:n]
        return torch.cat([torch.zeros(1, dtype=self.inc.dtype, device="cuda"), self.inc[:n - 1]])


def set_switches(force_path, forced):
    for name in pc.SWITCH_NAMES:
        force_path(name, forced.get(name))


def read_notes(gdf):
    out = {}
    for name in pc.NOTE_NAMES:
        v = C.c_longlong(-1)
        if gdf.libgdf.gdf_amd_debug_noted(name.encode(), C.byref(v)) == 0:
            out[name] = int(v.value)
    return out


def _where(got, want):
    g, w = got.cpu().numpy(), want.cpu().numpy()
    bad = np.flatnonzero(g != w)
    return f"{len(bad)} of {len(g)} elements differ, the first at {bad[0]}: {g[bad[0]]} for {w[bad[0]]}"


def scan(gdf, force_path, dev, n, inclusive, in_off=0, out_off=0, in_place=False, forced=None, entry=None, G=None):
    """one call, everything about it asserted -> the notes"""
    from libgdf_amd.columns import NP_TO_GDF
    forced = forced or {}
    dtype = dev.dtype
    what = (_name(dtype), n, "inclusive" if inclusive else "exclusive", in_off, out_off, in_place, forced)
    src = Slab(dtype, n, in_off, dev.vals[:n])
    dst = src if in_place else Slab(dtype, n, out_off)
    cin, cout = col(src, NP_TO_GDF[dtype]), col(dst, NP_TO_GDF[dtype])
    set_switches(force_path, forced)
    assert gdf.libgdf.gdf_amd_debug_noted(None, None) == 0
    rc = gdf.libgdf.raw(entry or TYPED[dtype])(C.byref(cin), C.byref(cin if in_place else cout), 1 if inclusive else 0)
    assert rc == 0, what
    notes = read_notes(gdf)
    want_notes = pc.model(dtype, n, in_off, out_off, in_place, forced)
    assert {k: notes.get(k) for k in want_notes} == want_notes, what
    tiles = -(-n // pc.LB_TILE)
    if notes["scan.route"] in (pc.ELEMENTWISE, pc.COALESCED) and not notes["scan.bailed"]:
        assert notes["scan.grid"] == 0, what
    elif notes["scan.route"] == pc.ROUNDS or notes["scan.bailed"]:
        assert 1 <= notes["scan.grid"] <= min(pc.MAX_GRID, tiles), what
        assert G is None or notes["scan.grid"] == min(G, tiles), (what, notes, G)
    else:
        assert 1 <= notes["scan.grid"] <= tiles + (notes["scan.route"] == pc.SPINE), what
    want = dev.expected(n, inclusive)
    got = dst.elements()
    import torch
    assert torch.equal(got, want), (what, _where(got, want))
    assert dst.guards_intact(), (what, "bytes outside out[0, n) were written")
    if not in_place:
        assert torch.equal(src.elements(), dev.vals[:n]) and src.guards_intact(), (what, "`in` changed")
    return notes


_G = {}


def resident_grid(gdf, force_path, dtype):
    """G of the rounds for this dtype on this device: scan.grid of a forced-rounds call over 1024 tiles (G <= 1024)"""
    key = np.dtype(dtype)
    if key not in _G:
        dev = Device("full", dtype, pc.ROUNDS_MIN)
        notes = scan(gdf, force_path, dev, pc.ROUNDS_MIN, True, forced=pc.FAMILY_SWITCHES["rounds"])
        assert notes["scan.route"] == pc.ROUNDS and notes["scan.bailed"] == 0
        _G[key] = notes["scan.grid"]
        assert 1 <= _G[key] <= pc.MAX_GRID
    return _G[key]


def _grid_for(gdf, force_path, family, dtype):
    return resident_grid(gdf, force_path, dtype) if family == "rounds" else None


# ---------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,dtype,mode", [pytest.param(f, d, m, id=f"{f}-{_name(d)}-{m[0]}")
                                               for f in pc.FAMILIES for d in pc.DTYPES for m in MODES])
def test_family_sizes(gdf, force_path, family, dtype, mode):
    """The family's size table -- every tile, chunk, batch, window and round edge of its kernels -- with values drawn from the whole
    dtype: every running sum wraps, 64-bit aggregates have arbitrary high words."""
    G = _grid_for(gdf, force_path, family, dtype)
    sizes = pc.family_sizes(family, dtype, G)
    dev = Device("full", dtype, max(sizes.values()))
    for name, n in sizes.items():
        notes = scan(gdf, force_path, dev, n, mode[1], forced=pc.family_forced(family, dtype, n), G=G)
        assert notes["scan.route"] == pc.FAMILY_ROUTE[family] and notes["scan.bailed"] == 0, (name, notes)


@pytest.mark.parametrize("family,dtype,recipe", [pytest.param(f, d, r, id=f"{f}-{_name(d)}-{r}")
                                                 for f in pc.FAMILIES for d in pc.DTYPES for r in pc.recipes_for(d)])
def test_value_domains(gdf, force_path, family, dtype, recipe):
    """Every value recipe through every family at one multi-tile, multi-chunk size, both modes: all-ones words and borrows across both
    halves of a 64-bit publication (minus-one), sums that return to 0 (type-min), the index itself (ones), low-word sums that carry
    into the high word at every tile (half-word)."""
    G = _grid_for(gdf, force_path, family, dtype)
    n = pc.value_domain_size(family, dtype, G)
    dev = Device(recipe, dtype, n)
    for _, inclusive in MODES:
        notes = scan(gdf, force_path, dev, n, inclusive, forced=pc.family_forced(family, dtype, n), G=G)
        assert notes["scan.route"] == pc.FAMILY_ROUTE[family] and notes["scan.bailed"] == 0, notes


@pytest.mark.parametrize("dtype,lookback", [pytest.param(d, lb, id=f"{_name(d)}-lookback-{lb}")
                                            for d in pc.DTYPES for lb in (None, "0", "1", "2", "3")])
def test_alignment(gdf, force_path, dtype, lookback):
    """Every pair of `in` and `out` misalignment against 16 bytes (int8: every byte offset).  Only (0, 0) may take 16-byte accesses: it
    goes to the coalesced kernels (unforced: to the rounds where the model says so), to the forced single pass otherwise; every other
    pair runs the element-wise kernels whatever is forced, inside intact guards."""
    E = pc.elementwise_tile(dtype)
    forced = {} if lookback is None else {"GDF_SCAN_LOOKBACK": lookback}
    G = resident_grid(gdf, force_path, dtype) if lookback in (None, "3") else None
    dev = Device("full", dtype, pc.MAX_CHUNKS * E + 1)
    for n in (E + 1, pc.MAX_CHUNKS * E + 1):
        for i in pc.alignment_offsets(dtype):
            for o in pc.alignment_offsets(dtype):
                for _, inclusive in MODES:
                    notes = scan(gdf, force_path, dev, n, inclusive, in_off=i, out_off=o, forced=forced, G=G)
                    if (i, o) != (0, 0):
                        assert notes["scan.route"] == pc.ELEMENTWISE, (i, o, notes)
                    elif lookback in ("1", "2", "3"):
                        assert notes["scan.route"] == {"1": pc.LOOKBACK, "2": pc.SPINE, "3": pc.ROUNDS}[lookback], notes
                    elif lookback == "0" or n < pc.ROUNDS_MIN or np.dtype(dtype).itemsize == 1:
                        assert notes["scan.route"] == pc.COALESCED, notes
                    else:
                        assert notes["scan.route"] == pc.ROUNDS and notes["scan.bailed"] == 0, notes


IN_PLACE = {
    # variant: (family whose sizes are used, forced switches, element offset of the column, expected route)
    "elementwise-forced": ("elementwise", {"GDF_SCAN_BLOCKED": "1"}, 0, pc.ELEMENTWISE),
    "elementwise-misaligned": ("elementwise", {}, 1, pc.ELEMENTWISE),
    "coalesced": ("coalesced", {}, 0, pc.COALESCED),                       # (the default dispatch: in place it never takes the rounds)
    "lookback": ("lookback", {"GDF_SCAN_LOOKBACK": "1"}, 0, pc.LOOKBACK),
    "spine": ("spine", {"GDF_SCAN_LOOKBACK": "2"}, 0, pc.SPINE),
    "rounds-forced": ("coalesced", {"GDF_SCAN_LOOKBACK": "3"}, 0, pc.COALESCED),
}


@pytest.mark.parametrize("variant,dtype", [pytest.param(v, d, id=f"{v}-{_name(d)}") for v in IN_PLACE for d in pc.DTYPES])
def test_in_place(gdf, force_path, variant, dtype):
    """in == out on every family that accepts it, at a multi-chunk size and at 4097; the rounds do not (a bail-out would have destroyed
    the input): forced or by default from 2^22 elements on, an in-place scan is noted as the coalesced kernels'."""
    family, forced, off, route = IN_PLACE[variant]
    big = pc.value_domain_size(family, dtype)
    sizes = [big, 4097] + ([pc.ROUNDS_MIN] if variant in ("coalesced", "rounds-forced") else [])
    dev = Device("full", dtype, max(sizes))
    for n in sizes:
        for _, inclusive in MODES:
            notes = scan(gdf, force_path, dev, n, inclusive, in_off=off, out_off=off, in_place=True, forced=forced)
            assert notes["scan.route"] == route and notes["scan.bailed"] == 0, (n, notes)
            if n == big and route in (pc.ELEMENTWISE, pc.COALESCED):
                assert notes["scan.chunks"] == 1025, notes


@pytest.mark.parametrize("dtype", [np.int32, np.int64], ids=_name)
def test_rounds_bail_out(gdf, force_path, dtype):
    """GDF_SCAN_FORCE_BAIL sets the bail-out flag before the rounds launch: every workgroup leaves, and the three coalesced launches
    start over from `in` and write all of an `out` that holds nothing but the guard byte."""
    G = resident_grid(gdf, force_path, dtype)
    sizes = [G * pc.LB_TILE + 1, (4 * G + 1) * pc.LB_TILE]
    dev = Device("full", dtype, max(sizes))
    for n in sizes:
        for _, inclusive in MODES:
            notes = scan(gdf, force_path, dev, n, inclusive, forced={"GDF_SCAN_LOOKBACK": "3", "GDF_SCAN_FORCE_BAIL": "1"}, G=G)
            assert notes["scan.bailed"] == 1 and notes["scan.route"] == pc.COALESCED, notes
            assert notes["scan.grid"] == G
            # and the same column without the switch is the rounds' work
            notes = scan(gdf, force_path, dev, n, inclusive, forced={"GDF_SCAN_LOOKBACK": "3"}, G=G)
            assert notes["scan.bailed"] == 0 and notes["scan.route"] == pc.ROUNDS, notes


def test_generic_dispatch(gdf, force_path):
    """gdf_prefixsum_generic switches on the dtype like the reference's (src/scan.cu:66-76): int8 / int32 / int64 go to the typed entry
    points, every other dtype SUCCEEDS and writes nothing; an empty column succeeds on every entry point."""
    import torch
    from libgdf_amd.columns import GDF_DTYPES, NP_TO_GDF
    generic = gdf.libgdf.raw("gdf_prefixsum_generic")
    set_switches(force_path, {})
    for np_dtype, name in ((np.float64, "GDF_FLOAT64"), (np.int16, "GDF_INT16")):
        n = 5000
        w = np.dtype(np_dtype).itemsize
        payload = torch.from_numpy(np.random.default_rng(7).integers(0, 255, size=n * w, dtype=np.uint8)).cuda()
        src = Slab(np.uint8, n * w, 0, payload)
        dst = Slab(np.uint8, n * w, 0)
        src.n = dst.n = n
        cin, cout = col(src, GDF_DTYPES[name]), col(dst, GDF_DTYPES[name])
        for inclusive in (1, 0):
            assert gdf.libgdf.gdf_amd_debug_noted(None, None) == 0
            assert generic(C.byref(cin), C.byref(cout), inclusive) == 0
            assert read_notes(gdf) == {}, name
            assert dst.untouched(), name
            assert torch.equal(src.t[src.lo:src.hi], payload) and src.guards_intact(), name
    for dtype in pc.DTYPES:
        empty_in, empty_out = Slab(dtype, 0), Slab(dtype, 0)
        for entry in (TYPED[np.dtype(dtype)], "gdf_prefixsum_generic"):
            cin, cout = col(empty_in, NP_TO_GDF[np.dtype(dtype)]), col(empty_out, NP_TO_GDF[np.dtype(dtype)])
            for inclusive in (1, 0):
                assert gdf.libgdf.raw(entry)(C.byref(cin), C.byref(cout), inclusive) == 0
                assert empty_in.untouched() and empty_out.untouched()
        # the typed entry points and the generic one: the same answer (each held to the reference) and the same route
        dev = Device("full", dtype, 3 * pc.LB_TILE + 5)
        for n in (1, 3 * pc.LB_TILE + 5):
            for _, inclusive in MODES:
                a = scan(gdf, force_path, dev, n, inclusive)
                b = scan(gdf, force_path, dev, n, inclusive, entry="gdf_prefixsum_generic")
                assert a == b
