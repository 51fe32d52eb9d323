// semijoin.hip -- gdf_amd_semi_join: the left rows with (EXISTS) or without (NOT EXISTS, GDF_AMD_SEMI_ANTI) a partner among the right
// rows, as ascending row numbers (include/gdf/gdf_amd_ext.h has the contract, DESIGN.md section 18 the routes and the measurements).
// No counterpart in the reference; csrc/join.hip is not involved.
//
//   image     per row, from the key columns: per column [value field in the element's own width: the integer's bits, the float's bits
//             with -0.0 folded onto +0.0][null bit, only under NULLS_EQUAL and when either side's column has a mask; the value field of
//             a null is 0 and its data is not loaded].  A row that CANNOT MATCH -- a null without NULLS_EQUAL, a NaN -- has no image: it
//             is never inserted and never looked up.  EXACT: the fields fit 64 bits whole, the image is the key.  WIDE: they do not; a
//             64-bit hash of the fields stands in, and a hit is verified against the columns.
//   build     an open-addressing set of the right side's distinct keys, linear probing, at most half full.
//             EXACT  slot = image; SJ_EMPTY (all ones) marks a free slot, so the image that equals it is kept as one flag (SjCtl).
//             WIDE   slot = (tag << 32) | representative right row, tag = the hash's high bits, the slot number its low bits; claimed by
//                    one compare-and-swap, so no reader sees half a slot.  A tag hit is verified (sj_rows_agree), a mismatch probes on.
//             Every probing loop is bounded by the table's capacity; a loop that runs out sets SjCtl::overflow -> GDF_CUDA_ERROR.
//   probe     LDS route     EXACT and at most SJ_LDS_C (8192) distinct keys: the table (rebuilt small by sj_compact when the right side has more
//                           ROWS than that) is copied into each persistent workgroup's LDS once, the left rows stream past it.
//             global route  EXACT otherwise: the same lookups against the table in device memory.
//             WIDE route    the tag table in device memory, verification against the right columns.
//             A wave's 64 verdicts leave as one 64-bit ballot word, written by one lane.
//   emit      ordered compaction of the verdict bitmap (complemented and tail-masked under ANTI): sj_count popcounts per 512-row tile,
//             scan_u32, sj_emit writes the row numbers ascending.
// HOST READ-BACKS: one for the number of result rows (with the control words); one more, only when the right side has more than
// SJ_LDS_C rows and an EXACT key, for the count of distinct keys that picks the route.
#include "internal.h"
#include "launch.h"

#include <gdf/gdf_amd_ext.h>

#include <algorithm>

namespace gdf_amd {

constexpr int SJ_THREADS = 256;
constexpr int SJ_LDS_THREADS = 1024;
constexpr int SJ_PER_LANE = 8;
constexpr int SJ_TILE = WAVE * SJ_PER_LANE;       // 512 rows: one wave's tile, lane l owns rows base + j * 64 + l; 8 verdict words
constexpr uint64_t SJ_EMPTY = ~0ULL;
constexpr long long SJ_MIN_SLOTS = 64;
// The route constants (tools/bench_semi_join.py -> profiles/semi_join_bench.jsonl):
//   SJ_LDS_MAX_SLOTS  16384 slots are 128 KiB of the CU's 160 KiB: the largest power of two one workgroup can hold.
//   SJ_LDS_C          distinct keys up to which the LDS route is taken: all that fit at half load.  Lines "l: ... route lds / global
//                     forced", 1e8 left rows: the LDS route is ahead at every swept size, 500 (1.35 against 2.03 ms), 2000 (1.30 / 1.66),
//                     4096 (1.51 / 1.91) and 8192 keys (1.47 / 2.03) -- also where the 128 KiB table leaves one workgroup per CU.
constexpr long long SJ_LDS_MAX_SLOTS = 16384;
constexpr long long SJ_LDS_C = SJ_LDS_MAX_SLOTS / 2;
enum : int { SJ_ROUTE_NONE = 0, SJ_ROUTE_LDS = 1, SJ_ROUTE_GLOBAL = 2, SJ_ROUTE_WIDE = 3 };

struct SjCol {
  const void *data;
  const uint8_t *valid;      // may be null
  int kind;
  int wbits;                 // the element's width in bits
  int shift;                 // EXACT: position of the value field in the image
  int nshift;                // EXACT: position of the null bit, < 0: none
};
struct SjSide {
  int ncols;
  int nulls_equal;
  SjCol c[MAX_KEY_COLS];
};
struct SjCtl {               // device memory, zeroed before the build
  uint32_t reserved;         // EXACT: some right row's image is SJ_EMPTY
  uint32_t distinct;         // slots claimed by the build
  uint32_t overflow;         // a probing loop ran through the whole table (cannot happen at half load)
  uint32_t pad;
};

// the row's EXACT image (EXACT_KEY) or the 64-bit hash of its fields -> *out; false: the row cannot match
template <bool EXACT_KEY>
__device__ __forceinline__ bool sj_image(const SjSide &s, int64_t row, uint64_t *out) {
  uint64_t k = EXACT_KEY ? 0ULL : 0x9E3779B97F4A7C15ULL;
  for (int c = 0; c < s.ncols; ++c) {
    const SjCol &f = s.c[c];
    const bool null = f.valid && !bit_is_set(f.valid, row);
    uint64_t v = 0;
    if (null) {
      if (!s.nulls_equal) return false;
    } else if (f.kind == K_F32) {                                       // (the data under a null bit is not loaded)
      uint32_t b = ((const uint32_t *)f.data)[row];
      if ((b & 0x7fffffffu) > 0x7f800000u) return false;
      if ((b << 1) == 0) b = 0;
      v = b;
    } else if (f.kind == K_F64) {
      uint64_t b = ((const uint64_t *)f.data)[row];
      if ((b & 0x7fffffffffffffffULL) > 0x7ff0000000000000ULL) return false;
      if ((b << 1) == 0) b = 0;
      v = b;
    } else {
      v = ob_load_int(f.data, f.kind, row);
      if (f.wbits < 64) v &= (1ULL << f.wbits) - 1ULL;
    }
    if (EXACT_KEY) {
      k |= v << f.shift;
      if (f.nshift >= 0) k |= (uint64_t)null << f.nshift;
    } else {
      k = mix64(k ^ v) + (null ? 0xD6E8FEB86659FD93ULL : 0ULL);
    }
  }
  *out = k;
  return true;
}

// row i of a against row j of b, column by column: both null (NULLS_EQUAL only), or both valid and equal as gdf_inner_join compares
__device__ __forceinline__ bool sj_rows_agree(const SjSide &a, int64_t i, const SjSide &b, int64_t j) {
  for (int c = 0; c < a.ncols; ++c) {
    const SjCol &fa = a.c[c], &fb = b.c[c];
    const bool na = fa.valid && !bit_is_set(fa.valid, i), nb = fb.valid && !bit_is_set(fb.valid, j);
    if (na || nb) {
      if (!(a.nulls_equal && na && nb)) return false;
      continue;
    }
    if (fa.kind == K_F32) {
      if (!(((const float *)fa.data)[i] == ((const float *)fb.data)[j])) return false;
    } else if (fa.kind == K_F64) {
      if (!(((const double *)fa.data)[i] == ((const double *)fb.data)[j])) return false;
    } else if (ob_load_int(fa.data, fa.kind, i) != ob_load_int(fb.data, fb.kind, j)) {
      return false;
    }
  }
  return true;
}

__device__ __forceinline__ uint64_t sj_slot_of(uint64_t key, uint64_t mask) { return mix64(key) & mask; }

// insert `key` (never SJ_EMPTY) into the EXACT table; true: this call claimed a slot
__device__ __forceinline__ bool sj_insert(unsigned long long *tab, uint64_t mask, uint64_t key, SjCtl *ctl) {
  uint64_t slot = sj_slot_of(key, mask);
  for (uint64_t step = 0; step <= mask; ++step) {
    const unsigned long long old = atomicCAS(&tab[slot], (unsigned long long)SJ_EMPTY, (unsigned long long)key);
    if (old == SJ_EMPTY) return true;
    if (old == key) return false;
    slot = (slot + 1) & mask;
  }
  ctl->overflow = 1;
  return false;
}

__device__ __forceinline__ void sj_add_distinct(uint32_t claimed, SjCtl *ctl) {
  claimed = wave_reduce_add(claimed);
  if (lane_id() == 0 && claimed) atomicAdd(&ctl->distinct, claimed);
}

__global__ __launch_bounds__(SJ_THREADS) void sj_build(SjSide r, uint32_t n, unsigned long long *tab, uint64_t mask, SjCtl *ctl) {
  uint32_t claimed = 0;
  for (uint64_t row = (uint64_t)blockIdx.x * SJ_THREADS + threadIdx.x; row < n; row += (uint64_t)gridDim.x * SJ_THREADS) {
    uint64_t key;
    if (!sj_image<true>(r, (int64_t)row, &key)) continue;
    if (key == SJ_EMPTY) ctl->reserved = 1;
    else claimed += sj_insert(tab, mask, key, ctl) ? 1u : 0u;
  }
  sj_add_distinct(claimed, ctl);
}

// the occupied slots of a large EXACT table into a small one (the right side has many rows and few distinct keys)
__global__ __launch_bounds__(SJ_THREADS) void sj_compact(const unsigned long long *big, uint64_t big_slots, unsigned long long *tab, uint64_t mask,
                                                         SjCtl *ctl) {
  for (uint64_t i = (uint64_t)blockIdx.x * SJ_THREADS + threadIdx.x; i < big_slots; i += (uint64_t)gridDim.x * SJ_THREADS) {
    const uint64_t key = big[i];
    if (key != SJ_EMPTY) sj_insert(tab, mask, key, ctl);
  }
}

__global__ __launch_bounds__(SJ_THREADS) void sj_build_wide(SjSide r, uint32_t n, unsigned long long *tab, uint64_t mask, uint32_t tagmask, SjCtl *ctl) {
  uint32_t claimed = 0;
  for (uint64_t row = (uint64_t)blockIdx.x * SJ_THREADS + threadIdx.x; row < n; row += (uint64_t)gridDim.x * SJ_THREADS) {
    uint64_t h;
    if (!sj_image<false>(r, (int64_t)row, &h)) continue;
    const uint32_t tag = (uint32_t)(h >> 32) & tagmask;
    const unsigned long long mine = ((unsigned long long)tag << 32) | (unsigned long long)row;
    uint64_t slot = h & mask;
    bool placed = false;
    for (uint64_t step = 0; step <= mask && !placed; ++step) {
      const unsigned long long old = atomicCAS(&tab[slot], (unsigned long long)SJ_EMPTY, mine);
      if (old == SJ_EMPTY) {
        placed = true;
        claimed++;
      } else if ((uint32_t)(old >> 32) == tag && sj_rows_agree(r, (int64_t)row, r, (int64_t)(uint32_t)old)) {
        placed = true;                                                  // the key is in the set already
      } else {
        slot = (slot + 1) & mask;
      }
    }
    if (!placed) ctl->overflow = 1;
  }
  sj_add_distinct(claimed, ctl);
}

// `s` is the content of `slot`; probes on from there
__device__ __forceinline__ bool sj_find(const uint64_t *tab, uint64_t mask, uint64_t slot, uint64_t s, uint64_t key) {
  for (uint64_t step = 0; step <= mask; ++step) {
    if (s == key) return true;
    if (s == SJ_EMPTY) return false;
    slot = (slot + 1) & mask;
    s = tab[slot];
  }
  return false;
}

// EXACT probe.  LDS: persistent workgroups with the whole table in dynamic LDS ((mask + 1) * 8 bytes); otherwise the table is read in
// device memory.  verdict: 8 words per tile, bit l of word tile * 8 + j = row tile * 512 + j * 64 + l has a partner; 0 beyond n.
template <bool LDS>
__global__ __launch_bounds__(LDS ? SJ_LDS_THREADS : SJ_THREADS) void sj_probe(SjSide l, uint32_t n, uint32_t ntiles, const uint64_t *gtab, uint64_t mask,
                                                                              const SjCtl *ctl, uint64_t *__restrict__ verdict) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sj_smem[];
  const uint64_t *tab = gtab;
  if (LDS) {
    uint64_t *lt = reinterpret_cast<uint64_t *>(sj_smem);
    for (uint64_t i = threadIdx.x; i <= mask; i += blockDim.x) lt[i] = gtab[i];
    block_sync();
    tab = lt;
  }
  const bool reserved = ctl->reserved != 0;
  const int lane = lane_id();
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) / WAVE, nwaves = gridDim.x * (blockDim.x / WAVE);
  for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t base = (int64_t)tile * SJ_TILE + lane;
    uint64_t key[SJ_PER_LANE], slot[SJ_PER_LANE], first[SJ_PER_LANE];
    bool ok[SJ_PER_LANE];
#pragma unroll
    for (int j = 0; j < SJ_PER_LANE; ++j) {
      const int64_t row = base + j * WAVE;
      key[j] = 0;
      ok[j] = row < (int64_t)n && sj_image<true>(l, row, &key[j]);
      slot[j] = sj_slot_of(key[j], mask);
    }
#pragma unroll
    for (int j = 0; j < SJ_PER_LANE; ++j) first[j] = ok[j] ? tab[slot[j]] : SJ_EMPTY;      // the eight first probes are in flight together
    if (LDS) {
      // the eight lookups advance in LOCKSTEP: every round resolves what it can and issues the next probes of all open lookups together
      // (profiles/semi_join_bench.jsonl: sj_probe_lds 1.01 - 1.28 ms against 1.11 - 1.34 ms with one lookup after the other)
      bool hit[SJ_PER_LANE], open[SJ_PER_LANE];
#pragma unroll
      for (int j = 0; j < SJ_PER_LANE; ++j) {
        const bool is_marker = key[j] == SJ_EMPTY;
        hit[j] = ok[j] && is_marker && reserved;
        open[j] = ok[j] && !is_marker;
      }
      for (uint64_t step = 0; step <= mask; ++step) {                   // bounded by the table's capacity
        bool more = false;
#pragma unroll
        for (int j = 0; j < SJ_PER_LANE; ++j) {
          if (!open[j]) continue;
          if (first[j] == key[j]) {
            hit[j] = true;
            open[j] = false;
          } else if (first[j] == SJ_EMPTY) {
            open[j] = false;
          } else {
            slot[j] = (slot[j] + 1) & mask;
            more = true;
          }
        }
        if (__ballot(more) == 0) break;
#pragma unroll
        for (int j = 0; j < SJ_PER_LANE; ++j)
          if (open[j]) first[j] = tab[slot[j]];
      }
#pragma unroll
      for (int j = 0; j < SJ_PER_LANE; ++j) {
        const unsigned long long word = __ballot(hit[j]);
        if (lane == 0) verdict[(size_t)tile * SJ_PER_LANE + j] = word;
      }
    } else {
      // in device memory one lookup after the other is the faster form once the table leaves the L2 (the same file: sj_probe 2.39 /
      // 2.64 / 2.73 ms at 1e6 / 1e7 / 4e7 keys against 2.70 / 2.82 / 2.91 ms in lockstep; no difference below 1e5 keys)
#pragma unroll
      for (int j = 0; j < SJ_PER_LANE; ++j) {
        bool hit = false;
        if (ok[j]) hit = key[j] == SJ_EMPTY ? reserved : sj_find(tab, mask, slot[j], first[j], key[j]);
        const unsigned long long word = __ballot(hit);
        if (lane == 0) verdict[(size_t)tile * SJ_PER_LANE + j] = word;
      }
    }
  }
}

__global__ __launch_bounds__(SJ_THREADS) void sj_probe_wide(SjSide l, SjSide r, uint32_t n, uint32_t ntiles, const uint64_t *__restrict__ tab, uint64_t mask,
                                                            uint32_t tagmask, uint64_t *__restrict__ verdict) {
  const int lane = lane_id();
  const uint32_t wave = (blockIdx.x * SJ_THREADS + threadIdx.x) / WAVE, nwaves = gridDim.x * (SJ_THREADS / WAVE);
  for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t base = (int64_t)tile * SJ_TILE + lane;
    uint64_t h[SJ_PER_LANE], first[SJ_PER_LANE];
    bool ok[SJ_PER_LANE];
#pragma unroll
    for (int j = 0; j < SJ_PER_LANE; ++j) {
      const int64_t row = base + j * WAVE;
      h[j] = 0;
      ok[j] = row < (int64_t)n && sj_image<false>(l, row, &h[j]);
    }
#pragma unroll
    for (int j = 0; j < SJ_PER_LANE; ++j) first[j] = ok[j] ? tab[h[j] & mask] : SJ_EMPTY;
#pragma unroll
    for (int j = 0; j < SJ_PER_LANE; ++j) {
      bool hit = false;
      if (ok[j]) {
        const int64_t row = base + j * WAVE;
        const uint32_t tag = (uint32_t)(h[j] >> 32) & tagmask;
        uint64_t slot = h[j] & mask, s = first[j];
        for (uint64_t step = 0; step <= mask; ++step) {
          if (s == SJ_EMPTY) break;
          if ((uint32_t)(s >> 32) == tag && sj_rows_agree(l, row, r, (int64_t)(uint32_t)s)) { hit = true; break; }
          slot = (slot + 1) & mask;
          s = tab[slot];
        }
      }
      const unsigned long long word = __ballot(hit);
      if (lane == 0) verdict[(size_t)tile * SJ_PER_LANE + j] = word;
    }
  }
}

// word w of the bitmap as the emit sees it: complemented under ANTI, the bits of the rows beyond n cleared
__device__ __forceinline__ uint64_t sj_word(const uint64_t *verdict, uint64_t w, uint32_t n, int anti) {
  uint64_t v = verdict[w];
  if (anti) v = ~v;
  const uint64_t first = w * WAVE;
  if (first >= n) return 0;
  const uint64_t live = (uint64_t)n - first;
  return live >= WAVE ? v : v & ((1ULL << live) - 1ULL);
}

// cnt[tile] = qualifying rows of the tile, cnt[ntiles] = 0 (the exclusive scan leaves the total there)
__global__ __launch_bounds__(SJ_THREADS) void sj_count(const uint64_t *__restrict__ verdict, uint32_t n, uint32_t ntiles, int anti, uint32_t *__restrict__ cnt) {
  for (uint64_t tile = (uint64_t)blockIdx.x * SJ_THREADS + threadIdx.x; tile <= ntiles; tile += (uint64_t)gridDim.x * SJ_THREADS) {
    uint32_t c = 0;
    if (tile < ntiles) {
#pragma unroll
      for (int j = 0; j < SJ_PER_LANE; ++j) c += (uint32_t)__popcll(sj_word(verdict, tile * SJ_PER_LANE + j, n, anti));
    }
    cnt[tile] = c;
  }
}

// off: the exclusive scan of cnt.  out[off[tile] ...] = the tile's qualifying row numbers, ascending.  No position >= m is written.
__global__ __launch_bounds__(SJ_THREADS) void sj_emit(const uint64_t *__restrict__ verdict, uint32_t n, uint32_t ntiles, int anti,
                                                      const uint32_t *__restrict__ off, int32_t *__restrict__ out, uint32_t m) {
  const int lane = lane_id();
  const uint32_t wave = (blockIdx.x * SJ_THREADS + threadIdx.x) / WAVE, nwaves = gridDim.x * (SJ_THREADS / WAVE);
  for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {
    uint32_t at = off[tile];
    if (off[tile + 1] == at) continue;
#pragma unroll
    for (int j = 0; j < SJ_PER_LANE; ++j) {
      const uint64_t w = sj_word(verdict, (uint64_t)tile * SJ_PER_LANE + j, n, anti);
      if ((w >> lane) & 1ULL) {
        const uint32_t pos = at + (uint32_t)mask_rank(w);
        if (pos < m) out[pos] = (int32_t)((uint64_t)tile * SJ_TILE + (uint64_t)j * WAVE + (uint64_t)lane);
      }
      at += (uint32_t)__popcll(w);
    }
  }
}

// the image plan, shared by both sides: which bits of the image each column gets; -> the fields fit 64 bits whole (EXACT)
static bool sj_plan(gdf_column **left, gdf_column **right, int ncols, bool nulls_equal, SjSide *l, SjSide *r) {
  *l = SjSide{};
  *r = SjSide{};
  l->ncols = r->ncols = ncols;
  l->nulls_equal = r->nulls_equal = nulls_equal ? 1 : 0;
  int pos = 0;
  for (int c = 0; c < ncols; ++c) {
    const ElemKind k = elem_kind(left[c]->dtype);
    SjCol f{};
    f.kind = (int)k;
    f.wbits = kind_width(k) * 8;
    f.shift = pos < 64 ? pos : 0;
    pos += f.wbits;
    f.nshift = -1;
    if (nulls_equal && (left[c]->valid || right[c]->valid)) {
      f.nshift = pos < 64 ? pos : 0;
      pos++;
    }
    f.data = left[c]->data;
    f.valid = left[c]->valid;
    l->c[c] = f;
    f.data = right[c]->data;
    f.valid = right[c]->valid;
    r->c[c] = f;
  }
  return pos <= 64;
}

static uint64_t sj_slots_for(uint64_t keys) {
  uint64_t s = (uint64_t)SJ_MIN_SLOTS;
  while (s < 2 * keys) s <<= 1;
  return s;
}

static gdf_error sj_new_table(DevBuf *tab, uint64_t slots) {
  RMM_TRY(tab->alloc(sizeof(uint64_t) * (size_t)slots));
  HIP_TRY(hipMemsetAsync(tab->p, 0xFF, sizeof(uint64_t) * (size_t)slots, stream0()));
  return GDF_SUCCESS;
}

static gdf_error semi_join(gdf_column **left, gdf_column **right, int ncols, uint32_t flags, gdf_column *out) {
  GDF_REQUIRE(left != nullptr && right != nullptr && out != nullptr && ncols > 0, GDF_DATASET_EMPTY);
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(left[c] != nullptr && right[c] != nullptr, GDF_DATASET_EMPTY);
  GDF_REQUIRE(ncols <= MAX_KEY_COLS, GDF_JOIN_TOO_MANY_COLUMNS);
  const gdf_size_type lrows = left[0]->size, rrows = right[0]->size;
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(left[c]->size == lrows && right[c]->size == rrows, GDF_COLUMN_SIZE_MISMATCH);
  for (int c = 0; c < ncols; ++c)
    GDF_REQUIRE(elem_kind(left[c]->dtype) != K_BAD && elem_kind(right[c]->dtype) != K_BAD, GDF_UNSUPPORTED_DTYPE);
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(left[c]->dtype == right[c]->dtype, GDF_JOIN_DTYPE_MISMATCH);
  GDF_REQUIRE((flags & ~(uint32_t)(GDF_AMD_SEMI_ANTI | GDF_AMD_SEMI_NULLS_EQUAL)) == 0, GDF_INVALID_API_CALL);
  GDF_REQUIRE(lrows >= 0 && rrows >= 0 && lrows < (gdf_size_type)0x7fffffff && rrows < (gdf_size_type)0x7fffffff, GDF_COLUMN_SIZE_TOO_BIG);
  for (int c = 0; c < ncols; ++c)
    GDF_REQUIRE((lrows == 0 || left[c]->data != nullptr) && (rrows == 0 || right[c]->data != nullptr), GDF_DATASET_EMPTY);

  const int anti = (flags & GDF_AMD_SEMI_ANTI) ? 1 : 0;
  const bool nulls_equal = (flags & GDF_AMD_SEMI_NULLS_EQUAL) != 0;
  const uint32_t nl = (uint32_t)lrows, nr = (uint32_t)rrows;
  gdf_column result{};
  result.dtype = GDF_INT32;
  if (nl == 0) {
    lab::note("sj_route", SJ_ROUTE_NONE);
    *out = result;
    return GDF_SUCCESS;
  }

  SjSide l, r;
  const bool exact = sj_plan(left, right, ncols, nulls_equal, &l, &r);
  lab::note("sj_exact", exact ? 1 : 0);

  const uint32_t ntiles = (uint32_t)(((size_t)nl + SJ_TILE - 1) / SJ_TILE);
  const size_t nwords = (size_t)ntiles * SJ_PER_LANE;
  // verdict words | cnt[ntiles + 1] | SjCtl: the total and the control words come back in one copy
  const size_t cnt_off = sizeof(uint64_t) * nwords, ctl_off = cnt_off + sizeof(uint32_t) * ((size_t)ntiles + 1);
  DevBuf scratch;
  RMM_TRY(scratch.alloc(ctl_off + sizeof(SjCtl)));
  uint64_t *verdict = scratch.as<uint64_t>();
  uint32_t *cnt = reinterpret_cast<uint32_t *>(scratch.as<unsigned char>() + cnt_off);
  SjCtl *ctl = reinterpret_cast<SjCtl *>(scratch.as<unsigned char>() + ctl_off);
  HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(SjCtl), stream0()));

  const int tiles_per_block = SJ_THREADS / WAVE;
  const int grid = stream_grid(ntiles, tiles_per_block);
  DevBuf table, small;
  int route = SJ_ROUTE_NONE;
  if (nr == 0) {
    HIP_TRY(hipMemsetAsync(verdict, 0, sizeof(uint64_t) * nwords, stream0()));
  } else {
    const long long forced = lab::path_int("GDF_SJ_ROUTE", 0);
    const int build_grid = stream_grid(nr, SJ_THREADS * 4);
    if (!exact || forced == SJ_ROUTE_WIDE) {
      route = SJ_ROUTE_WIDE;
      const long long tag_bits = std::min<long long>(std::max<long long>(lab::path_int("GDF_SJ_TAG_BITS", 32), 0), 32);
      const uint32_t tagmask = tag_bits >= 32 ? 0xffffffffu : ((1u << tag_bits) - 1u);
      const uint64_t slots = sj_slots_for(nr);
      GDF_TRY(sj_new_table(&table, slots));
      GDF_LAUNCH("sj_build_wide", sj_build_wide, dim3(build_grid), dim3(SJ_THREADS), 0, stream0(), r, nr, table.as<unsigned long long>(), slots - 1,
                 tagmask, ctl);
      GDF_LAUNCH("sj_probe_wide", sj_probe_wide, dim3(grid), dim3(SJ_THREADS), 0, stream0(), l, r, nl, ntiles, (const uint64_t *)table.as<uint64_t>(),
                 slots - 1, tagmask, verdict);
      HIP_CHECK_LAST();
    } else {
      // the LDS route's bound on the distinct keys (GDF_SJ_LDS_C lowers it; forcing the route takes it wherever the table fits)
      long long bound = std::min<long long>(std::max<long long>(lab::path_int("GDF_SJ_LDS_C", SJ_LDS_C), 0), SJ_LDS_MAX_SLOTS / 2);
      if (forced == SJ_ROUTE_LDS) bound = SJ_LDS_MAX_SLOTS / 2;
      if (forced == SJ_ROUTE_GLOBAL) bound = -1;
      uint64_t slots = sj_slots_for(nr);
      GDF_TRY(sj_new_table(&table, slots));
      GDF_LAUNCH("sj_build", sj_build, dim3(build_grid), dim3(SJ_THREADS), 0, stream0(), r, nr, table.as<unsigned long long>(), slots - 1, ctl);
      HIP_CHECK_LAST();
      bool lds = (long long)nr <= bound;
      if (!lds && bound >= 0) {                  // many right rows: are they few distinct keys?
        SjCtl seen;
        HIP_TRY(read_back(&seen, ctl, sizeof(seen)));
        lab::note("sj_distinct", seen.distinct);
        if ((long long)seen.distinct <= bound) {
          const uint64_t small_slots = sj_slots_for(seen.distinct);
          GDF_TRY(sj_new_table(&small, small_slots));
          GDF_LAUNCH("sj_compact", sj_compact, dim3(stream_grid((size_t)slots, SJ_THREADS * 4)), dim3(SJ_THREADS), 0, stream0(),
                     (const unsigned long long *)table.as<unsigned long long>(), slots, small.as<unsigned long long>(), small_slots - 1, ctl);
          HIP_CHECK_LAST();
          slots = small_slots;
          lds = true;
        }
      }
      const uint64_t *tab = (small.p ? small : table).as<uint64_t>();
      if (lds) {
        route = SJ_ROUTE_LDS;
        const size_t lds_bytes = sizeof(uint64_t) * (size_t)slots;
        const int per_cu = lds_bytes <= 64 * 1024 ? 2 : 1;              // (1024 threads each: two fill the CU's wave slots)
        const int lds_grid = stream_grid(ntiles, SJ_LDS_THREADS / WAVE, device_cu_count() * per_cu);
        GDF_TRY(launch_lds("sj_probe_lds", sj_probe<true>, dim3(lds_grid), dim3(SJ_LDS_THREADS), lds_bytes, l, nl, ntiles, tab, slots - 1,
                           (const SjCtl *)ctl, verdict));
      } else {
        route = SJ_ROUTE_GLOBAL;
        GDF_LAUNCH("sj_probe", sj_probe<false>, dim3(grid), dim3(SJ_THREADS), 0, stream0(), l, nl, ntiles, tab, slots - 1, (const SjCtl *)ctl, verdict);
      }
      HIP_CHECK_LAST();
    }
  }
  lab::note("sj_route", route);

  GDF_LAUNCH("sj_count", sj_count, dim3(stream_grid((size_t)ntiles + 1, SJ_THREADS)), dim3(SJ_THREADS), 0, stream0(), (const uint64_t *)verdict, nl, ntiles,
             anti, cnt);
  HIP_CHECK_LAST();
  GDF_TRY(scan_u32(cnt, cnt, (size_t)ntiles + 1, false));
  struct { uint32_t total; SjCtl c; } tail;
  static_assert(sizeof(tail) == sizeof(uint32_t) + sizeof(SjCtl), "the total sits in front of the control words");
  HIP_TRY(read_back(&tail, cnt + ntiles, sizeof(tail)));
  if (tail.c.overflow || tail.total > nl) return GDF_CUDA_ERROR;
  const uint32_t m = tail.total;
  if (m) {
    DevBuf rows;
    RMM_TRY(rows.alloc(sizeof(int32_t) * (size_t)m));
    GDF_LAUNCH("sj_emit", sj_emit, dim3(grid), dim3(SJ_THREADS), 0, stream0(), (const uint64_t *)verdict, nl, ntiles, anti, (const uint32_t *)cnt,
               rows.as<int32_t>(), m);
    HIP_CHECK_LAST();
    HIP_TRY(hipStreamSynchronize(stream0()));
    result.data = rows.release();
  }
  result.size = (gdf_size_type)m;
  *out = result;
  return GDF_SUCCESS;
}

}  // namespace gdf_amd

extern "C" {

gdf_error gdf_amd_semi_join(gdf_column **left_cols, gdf_column **right_cols, int ncols, uint32_t flags, gdf_column *out_indices) {
  return gdf_amd::guarded([&]() -> gdf_error { return gdf_amd::semi_join(left_cols, right_cols, ncols, flags, out_indices); });
}

}  // extern "C"
