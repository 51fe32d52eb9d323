// order.hip -- gdf_amd_order_by_ex (null-aware ORDER BY with a direction per column) and gdf_amd_gather (rows by an index
// column); include/gdf/gdf_amd_ext.h has both contracts.  No counterpart in the reference: its gdf_order_by refuses masks and
// sorts ascending only (src/sqls_ops.cu:1373-1392), and so does ours (sort.hip).
//
//   order_by_ex   order_rows' scheme (sort.hip) with two more things in the image.  The key columns are folded, last column group
//                 first, into 64-bit order-preserving images and the (image, row) pairs go through the same stable passes
//                 (hybrid_sort_pairs / radix_sort_pairs_u32: rs_count, rs_scatter, hs_*).  Per column, most significant first:
//                     [ null bit ]  only when the column has a mask: nulls last -> 1 for a null, NULLS_FIRST -> 1 for a value
//                     [ value    ]  integers (v - min) in bit_length(max - min) bits, floats their full-width total-order image;
//                                   DESC: (max - v) / ~image WITHIN the field; a null row: 0
//                 DESC therefore changes the images, not the passes: equal rows keep their input order.  min / max come from
//                 key_ranges, which skips null rows, so the data under a null bit neither widens a field nor is compared.  A unit
//                 that does not fit 64 bits (a masked full-range int64 / float64: 65) is split between two column groups, the null
//                 bit going to the more significant one -- LSD over groups, as for any key wider than 64 bits.
//   ga_gather     one wave owns 64 consecutive output rows: the index is loaded once, up to GA_BATCH columns are gathered from it
//                 (all loads of the batch issued before the first store), the ballot of "this row has a value" IS the output
//                 mask word (one 8-byte store by lane 0) and its complement's popcount the wave's share of null_count.
#include "internal.h"

#include <gdf/gdf_amd_ext.h>

#include <vector>

namespace gdf_amd {

// ---------------------------------------------------------------------------
// order_by_ex
// ---------------------------------------------------------------------------
// one key column's share of a column group's image
struct OrdField {
  const void *data;
  const uint8_t *valid;      // may be null
  long long bias;            // integers: the column minimum, or the maximum under DESC
  int kind;
  int bits;                  // value field: > 0 an integer of that many bits, 0 a float (full width), < 0 none in this group
  int shift;
  int nshift;                // position of the null bit, < 0: none in this group
  int desc, nulls_first;
};
struct OrdGroup {
  int nf;
  OrdField f[8];
};

// (ob_float_image / ob_load_int: internal.h -- groupby_agg.hip compares and folds with the same images)
__device__ __forceinline__ uint64_t ob_image(const OrdGroup &g, int64_t row) {
  uint64_t k = 0;
  for (int c = 0; c < g.nf; ++c) {
    const OrdField &f = g.f[c];
    const bool null = f.valid && !bit_is_set(f.valid, row);
    if (f.nshift >= 0) k |= (uint64_t)(null != (f.nulls_first != 0)) << f.nshift;
    if (f.bits < 0 || null) continue;                       // the data under a null bit is not even loaded
    uint64_t v;
    if (f.bits > 0) {
      const uint64_t x = ob_load_int(f.data, f.kind, row);
      v = (f.desc ? (uint64_t)f.bias - x : x - (uint64_t)f.bias) & (f.bits >= 64 ? ~0ULL : ((1ULL << f.bits) - 1ULL));
    } else {
      v = ob_float_image(f.data, f.kind, row);
      if (f.desc) v = ~v & (f.kind == K_F32 ? 0xffffffffULL : ~0ULL);
    }
    k |= v << f.shift;
  }
  return k;
}

// rs_make_keys of sort.hip over an OrdGroup.  perm may alias vals; *varying collects the bits on which some image differs from
// image 0, so that a digit on which all agree (a null bit of a column without nulls, say) costs no pass.
__global__ __launch_bounds__(256) void ob_make_keys(OrdGroup g, const uint32_t *perm, uint64_t *__restrict__ keys, uint32_t *vals, uint32_t n,
                                                    unsigned long long *__restrict__ varying) {
  const uint64_t k0 = ob_image(g, perm ? perm[0] : 0);
  uint64_t diff = 0;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t row = perm ? perm[i] : i;
    const uint64_t k = ob_image(g, row);
    keys[i] = k;
    vals[i] = row;
    diff |= k ^ k0;
  }
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const uint32_t lo = __shfl_xor((uint32_t)diff, d), hi = __shfl_xor((uint32_t)(diff >> 32), d);
    diff |= ((uint64_t)hi << 32) | lo;
  }
  if (lane_id() == 0 && diff) atomicOr(varying, (unsigned long long)diff);
}

static int ob_bit_length(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }

// The stable permutation of rows [0, n) under (cols, flags) -> dst (n x uint32, device).  The arguments are the CHECKED ones of
// gdf_amd_order_by_ex (1 <= ncols <= 16, equal sizes, key dtypes, data pointers, 0 < n < 2^31 - 1); flags may be null.  Returns after
// dst is written.  groupby_agg.hip groups on this order; it passes sorted_images, which receives the n sorted 64-bit images when ONE
// column group holds the whole key: two rows are then equal on every key column (both null, or equal values) exactly when their images
// are, so the group boundaries need no gather.  With more than one column group sorted_images stays empty.
gdf_error order_rows_ex(gdf_column **cols, int ncols, const uint8_t *flags, uint32_t n, uint32_t *dst, DevBuf *sorted_images) {
  KeyTable t;
  GDF_TRY(make_key_table(cols, ncols, &t));
  std::vector<long long> lo_hi(2 * (size_t)ncols);
  bool any_int = false;
  for (int c = 0; c < ncols; ++c) any_int |= !(t.col[c].kind == K_F32 || t.col[c].kind == K_F64);
  if (any_int) GDF_TRY(key_ranges(t, lo_hi.data()));                   // over the valid rows only

  // the atoms of the image, most significant first: per column its null bit (if it has a mask), then its value field
  struct Atom { int col; bool null_bit; int width; };
  std::vector<Atom> atoms;
  for (int c = 0; c < ncols; ++c) {
    const bool f = (t.col[c].kind == K_F32 || t.col[c].kind == K_F64);
    int w = t.col[c].width * 8;
    if (!f) {
      if (lo_hi[2 * c] > lo_hi[2 * c + 1]) lo_hi[2 * c] = lo_hi[2 * c + 1] = 0;      // no valid row at all
      w = ob_bit_length((uint64_t)lo_hi[2 * c + 1] - (uint64_t)lo_hi[2 * c]);
      if (w == 0) w = 1;                                                             // a constant column still owns one (never varying) bit
    }
    if (t.col[c].valid) atoms.push_back(Atom{c, true, 1});
    atoms.push_back(Atom{c, false, w});
  }
  // column groups of <= 64 image bits and <= 8 columns, last atoms first (LSD over groups)
  std::vector<OrdGroup> groups;
  for (int last = (int)atoms.size() - 1; last >= 0;) {
    int bits = 0, first = last, ncol = 0;
    while (first >= 0 && bits + atoms[first].width <= 64) {
      const bool new_col = first == last || atoms[first].col != atoms[first + 1].col;
      if (new_col && ncol == 8) break;
      ncol += new_col ? 1 : 0;
      bits += atoms[first].width;
      --first;
    }
    ++first;
    OrdGroup g{};
    int shift = bits;
    for (int k = first; k <= last; ++k) {
      const Atom &a = atoms[k];
      shift -= a.width;
      if (k == first || atoms[k - 1].col != a.col) {
        const bool f = (t.col[a.col].kind == K_F32 || t.col[a.col].kind == K_F64);
        const int fl = flags ? flags[a.col] : 0;
        OrdField &of = g.f[g.nf++];
        of.data = t.col[a.col].data;
        of.valid = t.col[a.col].valid;
        of.kind = t.col[a.col].kind;
        of.desc = (fl & GDF_AMD_ORDER_DESC) ? 1 : 0;
        of.nulls_first = (fl & GDF_AMD_ORDER_NULLS_FIRST) ? 1 : 0;
        of.bias = f ? 0 : lo_hi[2 * a.col + (of.desc ? 1 : 0)];
        of.bits = -1;
        of.shift = 0;
        of.nshift = -1;
      }
      OrdField &of = g.f[g.nf - 1];
      if (a.null_bit) {
        of.nshift = shift;
      } else {
        of.bits = (of.kind == K_F32 || of.kind == K_F64) ? 0 : a.width;
        of.shift = shift;
      }
    }
    groups.push_back(g);
    last = first - 1;
  }

  // the caller's column is one of the two row-number buffers: the result is copied only when it ends up in the other one
  DevBuf ka, kb, vb, vary;
  RMM_TRY(ka.alloc(sizeof(uint64_t) * (size_t)n));
  RMM_TRY(kb.alloc(sizeof(uint64_t) * (size_t)n));
  RMM_TRY(vb.alloc(sizeof(uint32_t) * (size_t)n));
  RMM_TRY(vary.alloc(sizeof(unsigned long long)));
  uint64_t *kin = ka.as<uint64_t>(), *kout = kb.as<uint64_t>();
  uint32_t *vin = vb.as<uint32_t>(), *vout = dst;
  const int sgrid = stream_grid(n, 256 * 8);
  bool have_perm = false, written = false;
  const bool want_images = sorted_images != nullptr && groups.size() == 1;
  for (size_t gi = 0; gi < groups.size(); ++gi) {
    const bool last_group = gi + 1 == groups.size();
    HIP_TRY(hipMemsetAsync(vary.p, 0, sizeof(unsigned long long), stream0()));
    GDF_LAUNCH("ob_make_keys", ob_make_keys, dim3(sgrid), dim3(256), 0, stream0(), groups[gi],
               have_perm ? (const uint32_t *)vin : (const uint32_t *)nullptr, kin, vin, n, vary.as<unsigned long long>());
    have_perm = true;
    unsigned long long varying = 0;
    HIP_TRY(hipMemcpyAsync(&varying, vary.p, sizeof(varying), hipMemcpyDeviceToHost, stream0()));
    HIP_TRY(hipStreamSynchronize(stream0()));
    bool hybrid = false;
    // (the last group's hs_local writes the row numbers straight into the caller's column unless that column is its input)
    GDF_TRY(hybrid_sort_pairs(kin, kout, vin, vout, n, varying, want_images, nullptr, &written, &hybrid, last_group ? dst : nullptr));
    if (!hybrid) GDF_TRY(radix_sort_pairs_u32(kin, kout, vin, vout, n, varying));
  }
  HIP_CHECK_LAST();
  if (!written && vin != dst) HIP_TRY(hipMemcpyAsync(dst, vin, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToDevice, stream0()));
  HIP_TRY(hipStreamSynchronize(stream0()));
  if (want_images) {
    sorted_images->reset();
    sorted_images->p = (kin == ka.as<uint64_t>() ? ka : kb).release();
  }
  return GDF_SUCCESS;
}

static gdf_error order_by_ex(gdf_column **cols, int ncols, const uint8_t *flags, gdf_column *out) {
  GDF_REQUIRE(cols != nullptr && ncols > 0, GDF_DATASET_EMPTY);
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(cols[c] != nullptr, GDF_DATASET_EMPTY);
  GDF_REQUIRE(ncols <= MAX_KEY_COLS, GDF_JOIN_TOO_MANY_COLUMNS);
  const gdf_size_type rows = cols[0]->size;
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(cols[c]->size == rows, GDF_COLUMN_SIZE_MISMATCH);
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(elem_kind(cols[c]->dtype) != K_BAD, GDF_UNSUPPORTED_DTYPE);
  const uint8_t known = GDF_AMD_ORDER_DESC | GDF_AMD_ORDER_NULLS_FIRST;
  for (int c = 0; flags && c < ncols; ++c) GDF_REQUIRE((flags[c] & ~known) == 0, GDF_INVALID_API_CALL);
  GDF_REQUIRE(out != nullptr && out->dtype == GDF_INT32 && out->size == rows, GDF_INVALID_API_CALL);
  GDF_REQUIRE(rows == 0 || out->data != nullptr, GDF_INVALID_API_CALL);
  GDF_REQUIRE(out->valid == nullptr, GDF_VALIDITY_UNSUPPORTED);
  GDF_REQUIRE(rows < (gdf_size_type)0x7fffffff, GDF_COLUMN_SIZE_TOO_BIG);
  if (rows == 0) return GDF_SUCCESS;
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(cols[c]->data != nullptr, GDF_DATASET_EMPTY);
  return order_rows_ex(cols, ncols, flags, (uint32_t)rows, static_cast<uint32_t *>(out->data), nullptr);
}

// ---------------------------------------------------------------------------
// gather
// ---------------------------------------------------------------------------
constexpr int GA_BATCH = 4;            // columns gathered from one load of the index (8 spill the kernel arguments out of the SGPRs)
constexpr int GA_THREADS = 256;

struct GatherBatch {
  int n;
  int width[GA_BATCH];
  const void *src[GA_BATCH];
  const uint8_t *valid[GA_BATCH];    // may be null
  void *dst[GA_BATCH];
  unsigned long long *mask[GA_BATCH];
  unsigned long long *nulls[GA_BATCH];
};

__device__ __forceinline__ uint64_t ga_load(const void *p, int width, int64_t i) {
  switch (width) {
    case 1: return ((const uint8_t *)p)[i];
    case 2: return ((const uint16_t *)p)[i];
    case 4: return ((const uint32_t *)p)[i];
    default: return ((const uint64_t *)p)[i];
  }
}
__device__ __forceinline__ void ga_store(void *p, int width, int64_t i, uint64_t v) {
  switch (width) {
    case 1: ((uint8_t *)p)[i] = (uint8_t)v; break;
    case 2: ((uint16_t *)p)[i] = (uint16_t)v; break;
    case 4: ((uint32_t *)p)[i] = (uint32_t)v; break;
    default: ((uint64_t *)p)[i] = v; break;
  }
}

// out row i = source row idx[i]; null (data 0, mask bit 0) where idx[i] is -1 or the source row is null.  An index outside
// [-1, rows) raises *bad and is treated as -1: no address is formed from it.  nwords = ceil(m / 64) mask words, one per wave trip.
template <class I>
__global__ __launch_bounds__(GA_THREADS) void ga_gather(const I *__restrict__ idx, int64_t m, int64_t rows, int64_t nwords, GatherBatch g,
                                                        uint32_t *__restrict__ bad) {
  const int lane = lane_id();
  const int64_t wave = ((int64_t)blockIdx.x * GA_THREADS + threadIdx.x) / WAVE, nwaves = (int64_t)gridDim.x * (GA_THREADS / WAVE);
  uint32_t nulls[GA_BATCH];
#pragma unroll
  for (int c = 0; c < GA_BATCH; ++c) nulls[c] = 0;
  bool any_bad = false;
  for (int64_t w = wave; w < nwords; w += nwaves) {
    const int64_t i = w * WAVE + lane;
    const bool live = i < m;
    long long ix = live ? (long long)idx[i] : -1;
    if (ix < -1 || ix >= rows) { any_bad = true; ix = -1; }
    const unsigned long long live_mask = __ballot(live);
    uint64_t v[GA_BATCH];
    bool ok[GA_BATCH];
#pragma unroll
    for (int c = 0; c < GA_BATCH; ++c) {
      ok[c] = false;
      v[c] = 0;
      if (c < g.n) {
        ok[c] = ix >= 0 && (!g.valid[c] || bit_is_set(g.valid[c], ix));
        if (ok[c]) v[c] = ga_load(g.src[c], g.width[c], ix);
      }
    }
#pragma unroll
    for (int c = 0; c < GA_BATCH; ++c) {
      if (c < g.n) {
        if (live) ga_store(g.dst[c], g.width[c], i, v[c]);
        const unsigned long long word = __ballot(ok[c]);
        if (lane == 0) {
          g.mask[c][w] = word;
          nulls[c] += (uint32_t)__popcll(live_mask & ~word);
        }
      }
    }
  }
  if (__ballot(any_bad) != 0ULL && lane == 0) *bad = 1u;               // (a plain store: every writer writes the same value)
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < GA_BATCH; ++c)
      if (c < g.n && nulls[c]) atomicAdd(g.nulls[c], (unsigned long long)nulls[c]);
  }
}

gdf_error gather_columns(gdf_column *indices, int ncols, gdf_column **cols, gdf_column **outs) {
  GDF_REQUIRE(indices != nullptr && cols != nullptr && outs != nullptr && ncols > 0, GDF_DATASET_EMPTY);
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(cols[c] != nullptr && outs[c] != nullptr, GDF_DATASET_EMPTY);
  const gdf_size_type rows_u = cols[0]->size;
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(cols[c]->size == rows_u, GDF_COLUMN_SIZE_MISMATCH);
  GDF_REQUIRE(indices->dtype == GDF_INT32 || indices->dtype == GDF_INT64, GDF_UNSUPPORTED_DTYPE);
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(dtype_width(cols[c]->dtype) > 0, GDF_UNSUPPORTED_DTYPE);
  GDF_REQUIRE(indices->valid == nullptr, GDF_VALIDITY_UNSUPPORTED);
  GDF_REQUIRE(rows_u <= (gdf_size_type)INT64_MAX / 16 && indices->size <= (gdf_size_type)INT64_MAX / 16, GDF_COLUMN_SIZE_TOO_BIG);
  const int64_t rows = (int64_t)rows_u, m = (int64_t)indices->size;
  GDF_REQUIRE(m == 0 || indices->data != nullptr, GDF_DATASET_EMPTY);
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(rows == 0 || cols[c]->data != nullptr, GDF_DATASET_EMPTY);

  const int64_t nwords = (m + 63) / 64;
  std::vector<DevBuf> data((size_t)ncols), mask((size_t)ncols);
  std::vector<unsigned long long> counts((size_t)ncols + 1, 0ULL);     // [ncols]: the "bad index" flag
  if (m > 0) {
    DevBuf d_counts;
    RMM_TRY(d_counts.alloc(sizeof(unsigned long long) * counts.size()));
    HIP_TRY(hipMemsetAsync(d_counts.p, 0, sizeof(unsigned long long) * counts.size(), stream0()));
    for (int c = 0; c < ncols; ++c) {
      RMM_TRY(data[c].alloc((size_t)m * (size_t)dtype_width(cols[c]->dtype)));
      RMM_TRY(mask[c].alloc((size_t)nwords * 8));
    }
    const dim3 grid(stream_grid((size_t)nwords, GA_THREADS / WAVE * 4));
    for (int c0 = 0; c0 < ncols; c0 += GA_BATCH) {
      GatherBatch g{};
      g.n = ncols - c0 < GA_BATCH ? ncols - c0 : GA_BATCH;
      for (int k = 0; k < g.n; ++k) {
        g.width[k] = dtype_width(cols[c0 + k]->dtype);
        g.src[k] = cols[c0 + k]->data;
        g.valid[k] = (const uint8_t *)cols[c0 + k]->valid;
        g.dst[k] = data[c0 + k].p;
        g.mask[k] = mask[c0 + k].as<unsigned long long>();
        g.nulls[k] = d_counts.as<unsigned long long>() + c0 + k;
      }
      uint32_t *bad = reinterpret_cast<uint32_t *>(d_counts.as<unsigned long long>() + ncols);
      if (indices->dtype == GDF_INT32)
        GDF_LAUNCH("ga_gather", ga_gather<int32_t>, grid, dim3(GA_THREADS), 0, stream0(), (const int32_t *)indices->data, m, rows, nwords, g, bad);
      else
        GDF_LAUNCH("ga_gather", ga_gather<long long>, grid, dim3(GA_THREADS), 0, stream0(), (const long long *)indices->data, m, rows, nwords, g, bad);
    }
    HIP_CHECK_LAST();
    HIP_TRY(read_back(counts.data(), d_counts.p, sizeof(unsigned long long) * counts.size()));
    GDF_REQUIRE(counts[ncols] == 0, GDF_INVALID_API_CALL);             // (the buffers go with their DevBufs)
  }
  for (int c = 0; c < ncols; ++c) {
    gdf_column *o = outs[c];
    o->data = m ? data[c].release() : nullptr;
    o->valid = m ? static_cast<gdf_valid_type *>(mask[c].release()) : nullptr;
    o->size = (gdf_size_type)m;
    o->dtype = cols[c]->dtype;
    o->null_count = (gdf_size_type)counts[c];
    o->dtype_info = cols[c]->dtype_info;
  }
  return GDF_SUCCESS;
}

}  // namespace gdf_amd

extern "C" {

gdf_error gdf_amd_order_by_ex(gdf_column **cols, int ncols, const uint8_t *flags, gdf_column *out_indices) {
  return gdf_amd::guarded([&]() -> gdf_error { return gdf_amd::order_by_ex(cols, ncols, flags, out_indices); });
}

gdf_error gdf_amd_gather(gdf_column *indices, int ncols, gdf_column **cols, gdf_column **outs) {
  return gdf_amd::guarded([&]() -> gdf_error { return gdf_amd::gather_columns(indices, ncols, cols, outs); });
}

}  // extern "C"
