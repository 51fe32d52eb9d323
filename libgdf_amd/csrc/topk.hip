// topk.hip -- gdf_amd_top_k: rows [offset, offset + k) of gdf_amd_order_by_ex's permutation without sorting the table
// (include/gdf/gdf_amd_ext.h has the contract, DESIGN.md section 17 the measurements).  No counterpart in the reference.
//
//   image     L(row): 64 bits built on the fly from the key columns, most significant first, per column [null bit, only with a mask]
//             [value image in the element's own width: integers sign-flipped, floats ob_float_image_of; complemented within the width
//             under DESC; 0 under a null, whose data is not loaded].  The field that straddles bit 64 gives its high bits, later
//             fields are dropped: a before b in the full order implies L(a) <= L(b).  L is COMPLETE when every field fits whole;
//             equal images are then equal rows.  The integer fields are NOT shrunk by key_ranges: that pass over the columns costs
//             as much as one select pass and only helps a key that just misses 64 bits.
//   select    T = the K-th smallest L (K = offset + k) by a radix select in quantile.hip's manner: tk_pass histograms an 11-bit
//             digit of the images that match the decided prefix (LDS histogram, one global atomic per bin and workgroup) and tracks
//             their min / max; the one-workgroup tk_select picks the bucket, counts the images below it and writes the next control
//             state to device memory.  No host round trip between the passes; a pass whose state says "done" returns at once.  All
//             matching images equal (min == max) ends the search, so massive ties cost one pass; and so does a bucket of at most
//             TK_SLACK images: T then stays undecided below that digit, and "L < T" / "L == T" below compare the decided bits only.
//   emit      ordered compaction: tk_count writes per 512-row wave tile the rows with L < T and L == T, scan_u32 turns both into
//             offsets, tk_emit writes the candidates -- first every row with L < T, then the rows with L == T (complete image and exact
//             T: only the first K - c_less of them; otherwise all), row numbers ascending inside both blocks.
//   finish    gather_columns of the candidates' key columns, order_rows_ex on that small table (stable, so equal rows keep their row
//             order), tk_write: out[i] = cand[perm[offset + i]].
//   fallback  order_rows_ex on the whole table and a copy of [offset, offset + m): when K is above TK_MAX_K (K >= rows included) or more
//             than TK_CAND_CAP candidates are left (the ties of a truncated image).
// HOST READ-BACKS of the selection route before the finish: ONE (the final control state: T, c_less, the ties).  gather_columns and
// order_rows_ex read back what they always do, over the candidates only.
#include "internal.h"

#include <gdf/gdf_amd_ext.h>

#include <algorithm>
#include <vector>

namespace gdf_amd {

constexpr int TK_THREADS = 256;
constexpr int TK_DIGIT = 11;
constexpr int TK_BINS = 1 << TK_DIGIT;
constexpr int TK_PER_LANE = 8;
constexpr int TK_TILE = WAVE * TK_PER_LANE;      // 512 rows: one wave's tile, lane l owns rows base + j * 64 + l
constexpr int TK_MAX_FIELDS = 8;                 // 8 x int8 fill 64 bits; a masked column takes 9
// The constants of the route map, from profiles/top_k_bench.jsonl (1e8 rows, tools/bench_topk.py):
//   TK_MAX_K     lines "s: (a) with K = ..., the selection route forced": K = 1e7 still lies under the whole sort's fastest call (2.3
//                against 3.8 ms), K = 5e7 takes 1.5 times the whole sort.  The largest swept K under the yardstick's minimum it is.
//   TK_SLACK     the select stops as soon as at most this many images share T's decided bits; they all become candidates.  Sorting
//                1e4 candidates instead of 1e2 costs 0.08 ms, 1e6 cost 0.4 ms (the same lines, K = 1e2 / 1e4 / 1e6); one more pass
//                over an int64 column costs 0.23 - 0.37 ms (kernels_ms: tk_count, tk_pass / select_passes).
//   TK_CAND_CAP  the finish over nc candidates costs what it costs for K = nc: the same crossover, plus the slack a K at the limit
//                may still bring along.
constexpr long long TK_MAX_K = 10000000;
constexpr long long TK_SLACK = 1 << 15;
constexpr long long TK_CAND_CAP = TK_MAX_K + TK_SLACK;

struct TkField {
  const void *data;
  const uint8_t *valid;      // may be null
  int kind;
  int wbits;                 // the element's width in bits
  int nshift;                // position of the null bit in L, < 0: the column has no mask
  int vbits;                 // value bits kept in L (0: none -- only the null bit fitted)
  int vdrop;                 // low value bits dropped: > 0 only in the straddling field
  int vshift;
  int desc, nulls_first;
};
struct TkImage {
  int nf;
  TkField f[TK_MAX_FIELDS];
};

struct TkCtl {               // written by tk_init / tk_select, read by the other kernels
  uint64_t prefix;           // decided high bits of T (bits >= shift + dbits); T itself once done
  uint64_t rank;             // rank of T among the images matching prefix
  uint64_t count;            // images matching prefix; once done: the images equal to T
  uint64_t c_less;           // images below every image matching prefix; once done: #{L < T}
  int32_t shift, dbits;      // the digit the next pass histograms
  int32_t low;               // bits of L below this are zero in every image
  int32_t done;
  int32_t column_passes;
  int32_t tshift;            // once done: the bits of T below tshift are undecided (0: T is exact)
};
struct TkAcc {
  unsigned long long kmin, kmax;
};
struct TkState {
  TkCtl c;
  TkAcc a;
};

__device__ __forceinline__ uint64_t tk_image(const TkImage &g, int64_t row) {
  uint64_t k = 0;
  for (int c = 0; c < g.nf; ++c) {
    const TkField &f = g.f[c];
    const bool null = f.valid && !bit_is_set(f.valid, row);
    if (f.nshift >= 0) k |= (uint64_t)(null != (f.nulls_first != 0)) << f.nshift;
    if (f.vbits == 0 || null) continue;                     // the data under a null bit is not even loaded
    uint64_t v;
    if (f.kind == K_F32 || f.kind == K_F64) v = ob_float_image(f.data, f.kind, row);
    else v = ob_load_int(f.data, f.kind, row) ^ (1ULL << (f.wbits - 1));
    if (f.desc) v = ~v;
    v &= f.wbits >= 64 ? ~0ULL : ((1ULL << f.wbits) - 1ULL);
    k |= (v >> f.vdrop) << f.vshift;
  }
  return k;
}

__device__ __forceinline__ uint64_t tk_hi_mask(int hi) { return hi >= 64 ? 0ULL : ~0ULL << hi; }

__device__ __forceinline__ uint64_t tk_shfl_xor(uint64_t v, int o) {
  return ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, WAVE) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o, WAVE);
}

__global__ __launch_bounds__(64) void tk_init(TkState *st, TkCtl init, uint32_t *hist) {
  for (int i = threadIdx.x; i < TK_BINS; i += 64) hist[i] = 0;
  if (threadIdx.x == 0) {
    st->c = init;
    st->a.kmin = ~0ULL;
    st->a.kmax = 0;
  }
}

// one pass over the columns: the histogram of the current digit among the images matching the prefix, and their min / max
__global__ __launch_bounds__(TK_THREADS) void tk_pass(TkImage g, uint32_t n, uint32_t ntiles, TkState *st, uint32_t *ghist) {
  __shared__ uint32_t h[TK_BINS];
  __shared__ uint64_t s_red[2][TK_THREADS / WAVE];
  const TkCtl c = st->c;
  if (c.done) return;
  const uint64_t ma = tk_hi_mask(c.shift + c.dbits), pa = c.prefix & ma;
  const uint32_t dmask = (1u << c.dbits) - 1u;
  for (int i = threadIdx.x; i < TK_BINS; i += TK_THREADS) h[i] = 0;
  block_sync();
  const int lane = lane_id();
  const uint32_t wave = (blockIdx.x * TK_THREADS + threadIdx.x) / WAVE, nwaves = gridDim.x * (TK_THREADS / WAVE);
  uint64_t kmin = ~0ULL, kmax = 0;
  for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t base = (int64_t)tile * TK_TILE + lane;
    uint64_t key[TK_PER_LANE];
#pragma unroll
    for (int j = 0; j < TK_PER_LANE; ++j) {
      const int64_t row = base + j * WAVE;
      key[j] = row < (int64_t)n ? tk_image(g, row) : 0ULL;
    }
#pragma unroll
    for (int j = 0; j < TK_PER_LANE; ++j) {
      const bool m = base + j * WAVE < (int64_t)n && (key[j] & ma) == pa;
      const unsigned long long act = __ballot(m);
      if (m) {
        const uint32_t d = (uint32_t)(key[j] >> c.shift) & dmask;
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
        // every matching lane on one bin (ties, a constant digit): one LDS atomic for the wave instead of 64 queued on one address
        if (__ballot(d == d0) == act) {
          if (mask_rank(act) == 0) atomicAdd(&h[d0], (uint32_t)__popcll(act));
        } else {
          atomicAdd(&h[d], 1u);
        }
        kmin = key[j] < kmin ? key[j] : kmin;
        kmax = key[j] > kmax ? key[j] : kmax;
      }
    }
  }
  for (int o = 1; o < WAVE; o <<= 1) {
    const uint64_t a = tk_shfl_xor(kmin, o), b = tk_shfl_xor(kmax, o);
    kmin = a < kmin ? a : kmin;
    kmax = b > kmax ? b : kmax;
  }
  if (lane == 0) {
    s_red[0][threadIdx.x / WAVE] = kmin;
    s_red[1][threadIdx.x / WAVE] = kmax;
  }
  block_sync();
  if (threadIdx.x == 0) {
    for (int w = 1; w < TK_THREADS / WAVE; ++w) {
      kmin = s_red[0][w] < kmin ? s_red[0][w] : kmin;
      kmax = s_red[1][w] > kmax ? s_red[1][w] : kmax;
    }
    if (kmin <= kmax) {
      atomicMin(&st->a.kmin, (unsigned long long)kmin);
      atomicMax(&st->a.kmax, (unsigned long long)kmax);
    }
  }
  for (int i = threadIdx.x; i <= (int)dmask; i += TK_THREADS)
    if (h[i]) atomicAdd(&ghist[i], h[i]);
}

// one workgroup: pick the bucket of the target rank, advance the state, reset the histogram and the accumulators
__global__ __launch_bounds__(TK_THREADS) void tk_select(TkState *st, uint32_t *ghist, uint32_t slack) {
  constexpr int PER = TK_BINS / TK_THREADS;
  __shared__ uint32_t s_sum[TK_THREADS];
  __shared__ uint32_t s_b, s_before, s_cnt;
  TkCtl c = st->c;
  if (c.done) return;
  const TkAcc a = st->a;
  const int t = threadIdx.x;
  const uint32_t bins = 1u << c.dbits;
  uint32_t mine[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const uint32_t b = (uint32_t)(t * PER + i);
    mine[i] = b < bins ? ghist[b] : 0u;
    sum += mine[i];
    ghist[b] = 0;
  }
  s_sum[t] = sum;
  if (t == 0) { s_b = 0; s_before = 0; s_cnt = 0; }
  block_sync();
  uint64_t before = 0;                     // (256 sums: a serial read of the LDS array by every thread, as qt_select)
  for (int u = 0; u < t; ++u) before += s_sum[u];
  if (c.rank >= before && c.rank < before + sum) {
    uint64_t r = c.rank - before;
    for (int i = 0; i < PER; ++i) {
      if (r < mine[i]) { s_b = (uint32_t)(t * PER + i); s_before = (uint32_t)(c.rank - r); s_cnt = mine[i]; break; }
      r -= mine[i];
    }
  }
  block_sync();
  if (t == 0) {
    c.column_passes++;
    if (a.kmin == a.kmax) {                // every matching image is equal: that is T, and c.count of them tie
      c.prefix = a.kmin;
      c.done = 1;
      c.tshift = 0;
    } else {
      c.prefix = (c.prefix & tk_hi_mask(c.shift + c.dbits)) | ((uint64_t)s_b << c.shift);
      c.c_less += s_before;
      c.rank -= s_before;
      c.count = s_cnt;
      if (c.shift <= c.low) {
        c.done = 1;
        c.tshift = 0;                      // (the bits below low are zero in T and in every image)
      } else if (s_cnt <= slack) {         // few enough share T's decided bits: they all become candidates, the finish sorts them out
        c.done = 1;
        c.tshift = c.shift;
      } else {
        const int ns = c.shift - TK_DIGIT > c.low ? c.shift - TK_DIGIT : c.low;
        c.dbits = c.shift - ns;
        c.shift = ns;
      }
    }
    st->c = c;
    st->a.kmin = ~0ULL;
    st->a.kmax = 0;
  }
}

// cnt[tile] = rows of the tile with L < T, cnt[ntiles + tile] = rows with L == T -- both on the decided bits of T only
__global__ __launch_bounds__(TK_THREADS) void tk_count(TkImage g, uint32_t n, uint32_t ntiles, const TkState *st, uint32_t *__restrict__ cnt) {
  const uint64_t tm = tk_hi_mask(st->c.tshift), T = st->c.prefix & tm;
  const int lane = lane_id();
  const uint32_t wave = (blockIdx.x * TK_THREADS + threadIdx.x) / WAVE, nwaves = gridDim.x * (TK_THREADS / WAVE);
  for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {
    const int64_t base = (int64_t)tile * TK_TILE + lane;
    uint64_t key[TK_PER_LANE];
#pragma unroll
    for (int j = 0; j < TK_PER_LANE; ++j) {
      const int64_t row = base + j * WAVE;
      key[j] = row < (int64_t)n ? tk_image(g, row) : ~0ULL;
    }
    uint32_t less = 0, eq = 0;
#pragma unroll
    for (int j = 0; j < TK_PER_LANE; ++j) {
      const bool live = base + j * WAVE < (int64_t)n;
      less += (uint32_t)__popcll(__ballot(live && (key[j] & tm) < T));
      eq += (uint32_t)__popcll(__ballot(live && (key[j] & tm) == T));
    }
    if (lane == 0) {
      cnt[tile] = less;
      cnt[ntiles + tile] = eq;
    }
  }
}

// off: the exclusive scan of cnt.  cand[0, c_less): the rows with L < T; cand[c_less, nc): the first nc - c_less rows with L == T;
// row numbers ascending in both.  No position >= nc is written.
__global__ __launch_bounds__(TK_THREADS) void tk_emit(TkImage g, uint32_t n, uint32_t ntiles, const TkState *st, const uint32_t *__restrict__ off,
                                                      uint32_t *__restrict__ cand, uint32_t c_less, uint32_t nc) {
  const uint64_t tm = tk_hi_mask(st->c.tshift), T = st->c.prefix & tm;
  const int lane = lane_id();
  const uint32_t wave = (blockIdx.x * TK_THREADS + threadIdx.x) / WAVE, nwaves = gridDim.x * (TK_THREADS / WAVE);
  for (uint32_t tile = wave; tile < ntiles; tile += nwaves) {
    uint32_t lb = off[tile], eb = off[ntiles + tile];       // (eb counts from c_less: the "equal" half follows the "less" half in the scan)
    // wave-uniform: a tile without a wanted row (nearly all of them when K is small) is not loaded again
    const bool no_less = off[tile + 1] == lb;
    const bool no_eq = eb >= nc || (tile + 1 < ntiles && off[ntiles + tile + 1] == eb);
    if (no_less && no_eq) continue;
    const int64_t base = (int64_t)tile * TK_TILE + lane;
    uint64_t key[TK_PER_LANE];
#pragma unroll
    for (int j = 0; j < TK_PER_LANE; ++j) {
      const int64_t row = base + j * WAVE;
      key[j] = row < (int64_t)n ? tk_image(g, row) : ~0ULL;
    }
#pragma unroll
    for (int j = 0; j < TK_PER_LANE; ++j) {
      const int64_t row = base + j * WAVE;
      const bool live = row < (int64_t)n;
      const bool is_less = live && (key[j] & tm) < T, is_eq = live && (key[j] & tm) == T;
      const unsigned long long bl = __ballot(is_less), be = __ballot(is_eq);
      if (is_less) {
        const uint32_t pos = lb + (uint32_t)mask_rank(bl);
        if (pos < c_less) cand[pos] = (uint32_t)row;
      }
      if (is_eq) {
        const uint32_t pos = eb + (uint32_t)mask_rank(be);
        if (pos < nc) cand[pos] = (uint32_t)row;
      }
      lb += (uint32_t)__popcll(bl);
      eb += (uint32_t)__popcll(be);
    }
  }
}

// out[i] = cand[perm[offset + i]], 0 <= i < m; perm is a permutation of [0, nc)
__global__ __launch_bounds__(TK_THREADS) void tk_write(const uint32_t *__restrict__ cand, const uint32_t *__restrict__ perm, uint32_t nc, uint32_t offset,
                                                       uint32_t m, int32_t *__restrict__ out) {
  for (uint32_t i = blockIdx.x * TK_THREADS + threadIdx.x; i < m; i += gridDim.x * TK_THREADS) {
    const uint32_t p = perm[offset + i];
    if (p < nc) out[i] = (int32_t)cand[p];
  }
}

// the image plan: which bits of L each column gets.  *low: the bits of L below it are unused; *complete: every field fits whole
static void tk_plan(const KeyTable &t, const uint8_t *flags, TkImage *g, int *low, bool *complete) {
  *g = TkImage{};
  *complete = true;
  int pos = 64;
  for (int c = 0; c < t.ncols; ++c) {
    const int w = t.col[c].width * 8;
    if (pos == 0) { *complete = false; break; }
    TkField f{};
    f.data = t.col[c].data;
    f.valid = t.col[c].valid;
    f.kind = t.col[c].kind;
    f.wbits = w;
    f.nshift = -1;
    const int fl = flags ? flags[c] : 0;
    f.desc = (fl & GDF_AMD_ORDER_DESC) ? 1 : 0;
    f.nulls_first = (fl & GDF_AMD_ORDER_NULLS_FIRST) ? 1 : 0;
    if (f.valid) f.nshift = --pos;
    const int keep = w < pos ? w : pos;
    if (keep < w) *complete = false;
    f.vbits = keep;
    f.vdrop = w - keep;
    pos -= keep;
    f.vshift = pos;
    g->f[g->nf++] = f;                     // (every field takes at least one bit and all but the last at least eight: nf <= 8)
  }
  *low = pos;
}

static gdf_error tk_fallback(gdf_column **cols, int ncols, const uint8_t *flags, uint32_t n, int64_t offset, int64_t m, gdf_column *out) {
  DevBuf perm;
  RMM_TRY(perm.alloc(sizeof(uint32_t) * (size_t)n));
  GDF_TRY(order_rows_ex(cols, ncols, flags, n, perm.as<uint32_t>(), nullptr));
  HIP_TRY(hipMemcpyAsync(out->data, perm.as<uint32_t>() + offset, sizeof(uint32_t) * (size_t)m, hipMemcpyDeviceToDevice, stream0()));
  HIP_TRY(hipStreamSynchronize(stream0()));
  return GDF_SUCCESS;
}

static gdf_error tk_selection(gdf_column **cols, int ncols, const uint8_t *flags, uint32_t n, int64_t K, int64_t offset, int64_t m, long long cap,
                              long long slack, gdf_column *out, bool *too_many) {
  *too_many = false;
  KeyTable t;
  GDF_TRY(make_key_table(cols, ncols, &t));
  TkImage g;
  int low = 0;
  bool complete = true;
  tk_plan(t, flags, &g, &low, &complete);
  lab::note("tk.complete", complete ? 1 : 0);

  const uint32_t ntiles = (uint32_t)(((size_t)n + TK_TILE - 1) / TK_TILE);
  const size_t hist_off = 256, cnt_off = hist_off + sizeof(uint32_t) * TK_BINS;
  static_assert(sizeof(TkState) <= 256, "the state sits in front of the histogram");
  DevBuf scratch;
  RMM_TRY(scratch.alloc(cnt_off + sizeof(uint32_t) * 2 * (size_t)ntiles));
  TkState *st = scratch.as<TkState>();
  uint32_t *hist = reinterpret_cast<uint32_t *>(scratch.as<unsigned char>() + hist_off);
  uint32_t *cnt = reinterpret_cast<uint32_t *>(scratch.as<unsigned char>() + cnt_off);

  TkCtl init{};
  init.rank = (uint64_t)(K - 1);
  init.count = n;
  init.low = low;
  init.shift = 64 - TK_DIGIT > low ? 64 - TK_DIGIT : low;
  init.dbits = 64 - init.shift;
  const int passes = (64 - low + TK_DIGIT - 1) / TK_DIGIT;
  const int tiles_per_block = TK_THREADS / WAVE;
  const int pass_grid = stream_grid(ntiles, tiles_per_block, device_cu_count() * 4);       // (one atomic per bin and workgroup: few workgroups)
  const int grid = stream_grid(ntiles, tiles_per_block);

  hipLaunchKernelGGL(tk_init, dim3(1), dim3(64), 0, stream0(), st, init, hist);
  for (int p = 0; p < passes; ++p) {
    GDF_LAUNCH("tk_pass", tk_pass, dim3(pass_grid), dim3(TK_THREADS), 0, stream0(), g, n, ntiles, st, hist);
    GDF_LAUNCH("tk_select", tk_select, dim3(1), dim3(TK_THREADS), 0, stream0(), st, hist, (uint32_t)slack);
  }
  HIP_CHECK_LAST();
  TkCtl ctl;
  HIP_TRY(read_back(&ctl, &st->c, sizeof(ctl)));
  lab::note("tk.column_passes", ctl.column_passes);
  if (!ctl.done || ctl.c_less >= (uint64_t)K || ctl.c_less + ctl.count < (uint64_t)K || ctl.c_less + ctl.count > n) return GDF_CUDA_ERROR;
  // exactly K candidates when T is exact and equal images are equal rows; otherwise every row that shares T's decided bits
  const bool cut_ties = complete && ctl.tshift == 0;
  const uint64_t nc64 = cut_ties ? (uint64_t)K : ctl.c_less + ctl.count;
  lab::note("tk.exact", ctl.tshift == 0 ? 1 : 0);
  lab::note("tk.candidates", (long long)nc64);
  if (!cut_ties && nc64 > (uint64_t)cap) { *too_many = true; return GDF_SUCCESS; }
  const uint32_t nc = (uint32_t)nc64, c_less = (uint32_t)ctl.c_less;

  DevBuf cand, perm;
  RMM_TRY(cand.alloc(sizeof(uint32_t) * (size_t)nc));
  RMM_TRY(perm.alloc(sizeof(uint32_t) * (size_t)nc));
  GDF_LAUNCH("tk_count", tk_count, dim3(grid), dim3(TK_THREADS), 0, stream0(), g, n, ntiles, (const TkState *)st, cnt);
  HIP_CHECK_LAST();
  GDF_TRY(scan_u32(cnt, cnt, 2 * (size_t)ntiles, false));
  GDF_LAUNCH("tk_emit", tk_emit, dim3(grid), dim3(TK_THREADS), 0, stream0(), g, n, ntiles, (const TkState *)st, (const uint32_t *)cnt,
             cand.as<uint32_t>(), c_less, nc);
  HIP_CHECK_LAST();

  // the finish: the candidates' key columns, sorted; a column without a mask stays without one
  gdf_column idx{};
  idx.data = cand.p;
  idx.size = nc;
  idx.dtype = GDF_INT32;
  std::vector<gdf_column> small((size_t)ncols);
  std::vector<gdf_column *> small_ptr((size_t)ncols);
  for (int c = 0; c < ncols; ++c) small_ptr[c] = &small[c];
  std::vector<DevBuf> own(2 * (size_t)ncols);                            // (made before the gather: its buffers go with these)
  GDF_TRY(gather_columns(&idx, ncols, cols, small_ptr.data()));
  for (int c = 0; c < ncols; ++c) {
    own[2 * c].p = small[c].data;
    own[2 * c + 1].p = small[c].valid;
    if (!cols[c]->valid) small[c].valid = nullptr;
  }
  GDF_TRY(order_rows_ex(small_ptr.data(), ncols, flags, nc, perm.as<uint32_t>(), nullptr));
  GDF_LAUNCH("tk_write", tk_write, dim3(stream_grid((size_t)m, TK_THREADS)), dim3(TK_THREADS), 0, stream0(), (const uint32_t *)cand.as<uint32_t>(),
             (const uint32_t *)perm.as<uint32_t>(), nc, (uint32_t)offset, (uint32_t)m, static_cast<int32_t *>(out->data));
  HIP_CHECK_LAST();
  HIP_TRY(hipStreamSynchronize(stream0()));
  return GDF_SUCCESS;
}

static gdf_error top_k(gdf_column **cols, int ncols, const uint8_t *flags, int64_t k, int64_t offset, gdf_column *out) {
  GDF_REQUIRE(cols != nullptr && ncols > 0, GDF_DATASET_EMPTY);
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(cols[c] != nullptr, GDF_DATASET_EMPTY);
  GDF_REQUIRE(ncols <= MAX_KEY_COLS, GDF_JOIN_TOO_MANY_COLUMNS);
  const gdf_size_type rows = cols[0]->size;
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(cols[c]->size == rows, GDF_COLUMN_SIZE_MISMATCH);
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(elem_kind(cols[c]->dtype) != K_BAD, GDF_UNSUPPORTED_DTYPE);
  const uint8_t known = GDF_AMD_ORDER_DESC | GDF_AMD_ORDER_NULLS_FIRST;
  for (int c = 0; flags && c < ncols; ++c) GDF_REQUIRE((flags[c] & ~known) == 0, GDF_INVALID_API_CALL);
  GDF_REQUIRE(k >= 0 && offset >= 0, GDF_INVALID_API_CALL);
  gdf_size_type m = 0;
  if ((gdf_size_type)offset < rows) m = std::min<gdf_size_type>((gdf_size_type)k, rows - (gdf_size_type)offset);
  GDF_REQUIRE(out != nullptr && out->dtype == GDF_INT32 && out->size == m, GDF_INVALID_API_CALL);
  GDF_REQUIRE(m == 0 || out->data != nullptr, GDF_INVALID_API_CALL);
  GDF_REQUIRE(out->valid == nullptr, GDF_VALIDITY_UNSUPPORTED);
  GDF_REQUIRE(rows < (gdf_size_type)0x7fffffff, GDF_COLUMN_SIZE_TOO_BIG);
  if (m == 0) return GDF_SUCCESS;
  for (int c = 0; c < ncols; ++c) GDF_REQUIRE(cols[c]->data != nullptr, GDF_DATASET_EMPTY);

  const uint32_t n = (uint32_t)rows;
  const int64_t K = offset + (int64_t)m;                                 // (m > 0: offset < rows, K <= rows)
  const long long max_k = lab::path_int("GDF_TK_MAX_K", TK_MAX_K), cap = lab::path_int("GDF_TK_CAND_CAP", TK_CAND_CAP);
  const long long slack = std::min<long long>(std::max<long long>(lab::path_int("GDF_TK_SLACK", TK_SLACK), 0), 0x7fffffff);
  // route: 0 the selection, 1 the whole sort because of K, 2 the whole sort because a truncated image left too many candidates
  if ((int64_t)m < k || K >= (int64_t)n || K > max_k) {
    lab::note("tk.route", 1);
    return tk_fallback(cols, ncols, flags, n, offset, (int64_t)m, out);
  }
  bool too_many = false;
  GDF_TRY(tk_selection(cols, ncols, flags, n, K, offset, (int64_t)m, cap, slack, out, &too_many));
  lab::note("tk.route", too_many ? 2 : 0);
  if (too_many) return tk_fallback(cols, ncols, flags, n, offset, (int64_t)m, out);
  return GDF_SUCCESS;
}

}  // namespace gdf_amd

extern "C" {

gdf_error gdf_amd_top_k(gdf_column **cols, int ncols, const uint8_t *flags, int64_t k, int64_t offset, gdf_column *out_indices) {
  return gdf_amd::guarded([&]() -> gdf_error { return gdf_amd::top_k(cols, ncols, flags, k, offset, out_indices); });
}

}  // extern "C"
