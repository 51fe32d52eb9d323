// quantile.hip -- gdf_quantile_exact / gdf_quantile_aprrox (reference src/quantiles.cu, include/quantiles.hpp; the rule is
// restated in include/gdf/gdf.h, the kernels are described in DESIGN.md §11).
//
// Three modes, chosen by the context:
//   flag_sorted        the column is trusted to be sorted: the one or two elements are read directly (q >= 1: the max reduction
//                      of reduce.hip, as the reference uses max_element);
//   flag_sort_inplace  the column is sorted in place by the radix sort of sort.hip and the answer is read from it;
//   neither            RADIX SELECT: the column is neither modified nor copied.  Keys are the order-preserving unsigned images of
//                      the elements (sign flip for integers; the usual float flip, every NaN mapped to the all-ones key so that it
//                      sorts last).  Pass p histograms the 11-bit digit below the bits already decided, among the elements whose
//                      image matches the decided prefix; a one-workgroup kernel then picks the bucket holding the target rank and
//                      writes the new prefix, the rank left inside the bucket and its count to device memory.  No host round trip
//                      between passes: the only read-back is the final state.  Once the bucket's count fits the candidate buffer,
//                      the next column pass also appends the matching keys to it and the later passes read only those.
//                      Every pass also tracks the min and max of the matching keys, so a bucket of equal values ends the search.
//                      Rank k+1 (exact methods) rides along with rank k while both fall into the same bucket; when they part, k+1
//                      is the smallest key of the next non-empty bucket, which the following pass finds as a min over the elements
//                      of that bucket (or, at the last digit, the bucket itself is the key).
#include "internal.h"

#include <cmath>
#include <limits>

namespace gdf_amd {

gdf_error column_max_element(const gdf_column *col, void *host_result);   // reduce.hip
gdf_error sort_column_inplace(void *data, ElemKind kind, uint32_t n);     // sort.hip

constexpr int QT_THREADS = 256;
constexpr int QT_DIGIT = 11;
constexpr int QT_BINS = 1 << QT_DIGIT;
constexpr uint32_t QT_CAND_CAP = 1u << 22;    // candidate keys (32 MB); a bigger bucket is searched by filtered column passes
// The candidate buffer is QT_NSUB regions of `rs` keys, each with its own append counter (thread g appends to region g % QT_NSUB):
// ONE counter took every matching lane's atomic on one address -- 2M appends cost ~20 ms at 1e9 rows.  A bucket is compacted when
// it fills at most half the buffer; if a region still overflows, the search goes on with filtered column passes.
constexpr int QT_NSUB = 256;

// y1 states (rank k + 1)
enum : int { Y1_FOLLOWS = 0, Y1_KNOWN = 1, Y1_UNWANTED = 2, Y1_MIN_OF_B = 3 };

struct QtCtl {               // written by qt_init / qt_select, read by qt_pass
  uint64_t prefix;           // decided high bits of the target key (bits >= shift + dbits)
  uint64_t prefix_b;         // Y1_MIN_OF_B: rank k + 1 is the smallest key whose bits >= hi_b equal prefix_b's
  uint64_t y1;               // Y1_KNOWN: the key of rank k + 1
  uint32_t rank;             // rank of the target among the elements matching prefix
  uint32_t count;            // number of elements matching prefix
  int32_t shift, dbits;      // the digit the next pass histograms
  int32_t hi_b;
  int32_t done;              // prefix is the whole target key
  int32_t y1_state;
  int32_t src;               // 0: the column, 1: the candidate buffer
  int32_t compact;           // the next column pass appends its matching keys to the candidate buffer
  int32_t allow_compact;
  int32_t column_passes;     // diagnostics: passes that read the column
  int32_t pad;
};
struct QtAcc {               // accumulated by qt_pass (atomics), consumed and reset by qt_select
  unsigned long long kmin, kmax, bmin;
};
struct QtState {
  QtCtl c;
  QtAcc a;
};

template <class T> struct QtBits { using U = typename std::conditional<sizeof(T) == 8, uint64_t, typename std::conditional<sizeof(T) == 4, uint32_t,
                                   typename std::conditional<sizeof(T) == 2, uint16_t, uint8_t>::type>::type>::type; };

template <class T>
__host__ __device__ __forceinline__ uint64_t qt_key(T x) {
  using U = typename QtBits<T>::U;
  constexpr U SIGN = (U)((U)1 << (8 * sizeof(T) - 1));
  U b;
  __builtin_memcpy(&b, &x, sizeof(T));
  if constexpr (std::is_floating_point<T>::value) {
    if (x != x) return (uint64_t)(U)~(U)0;                    // every NaN: the largest key
    return (uint64_t)(U)((b & SIGN) ? (U)~b : (U)(b | SIGN));
  } else {
    return (uint64_t)(U)(b ^ SIGN);
  }
}
template <class T>
static T qt_value(uint64_t key) {
  using U = typename QtBits<T>::U;
  constexpr U SIGN = (U)((U)1 << (8 * sizeof(T) - 1));
  U k = (U)key, b;
  if constexpr (std::is_floating_point<T>::value) {
    if (k == (U)~(U)0) return std::numeric_limits<T>::quiet_NaN();
    b = (k & SIGN) ? (U)(k & (U)~SIGN) : (U)~k;
  } else {
    b = (U)(k ^ SIGN);
  }
  T x;
  __builtin_memcpy(&x, &b, sizeof(T));
  return x;
}

__device__ __forceinline__ uint64_t hi_mask(int hi) { return hi >= 64 ? 0ULL : ~0ULL << hi; }

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
  for (int o = 1; o < WAVE; o <<= 1) {
    const uint64_t w = ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, WAVE) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o, WAVE);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  for (int o = 1; o < WAVE; o <<= 1) {
    const uint64_t w = ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, WAVE) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, o, WAVE);
    v = w > v ? w : v;
  }
  return v;
}

__global__ __launch_bounds__(64) void qt_init(QtState *st, QtCtl init, uint32_t *hist, uint32_t *ncand) {
  for (int i = threadIdx.x; i < QT_BINS; i += 64) hist[i] = 0;
  for (int i = threadIdx.x; i < QT_NSUB; i += 64) ncand[i] = 0;
  if (threadIdx.x == 0) {
    st->c = init;
    st->a.kmin = ~0ULL;
    st->a.kmax = 0;
    st->a.bmin = ~0ULL;
  }
}

// one pass: LDS-privatised histogram of the current digit among the keys matching the prefix, their min / max, the min of
// the keys matching prefix_b (Y1_MIN_OF_B) and, when asked, the matching keys appended to the candidate buffer.
// Column elements [0, head) and [head + nvec * V, n) are the unaligned head and tail; vector j covers head + j*V ...
template <class T>
__global__ __launch_bounds__(QT_THREADS) void qt_pass(const T *__restrict__ data, int64_t n, int64_t head, int64_t nvec,
                                                      QtState *st, uint32_t *ghist, uint64_t *cand, uint32_t *ncand, uint32_t rs) {
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ uint32_t h[QT_BINS];
  __shared__ uint64_t s_red[3][QT_THREADS / WAVE];
  const QtCtl c = st->c;
  const bool want_b = c.y1_state == Y1_MIN_OF_B;
  if (c.done && !want_b) return;
  const bool want_a = !c.done;
  const uint64_t ma = hi_mask(c.shift + c.dbits), pa = c.prefix & ma;
  const uint64_t mb = hi_mask(c.hi_b), pb = c.prefix_b & mb;
  const uint32_t dmask = (1u << c.dbits) - 1u;
  const bool compact = c.compact && c.src == 0;
  for (int i = threadIdx.x; i < QT_BINS; i += QT_THREADS) h[i] = 0;
  block_sync();
  uint64_t kmin = ~0ULL, kmax = 0, bmin = ~0ULL;
  const int64_t gtid = (int64_t)blockIdx.x * QT_THREADS + threadIdx.x, gstride = (int64_t)gridDim.x * QT_THREADS;
  const uint32_t region = (uint32_t)(gtid % QT_NSUB);
  auto visit = [&](uint64_t key) {
    if (want_a && (key & ma) == pa) {
      atomicAdd(&h[(uint32_t)(key >> c.shift) & dmask], 1u);
      kmin = key < kmin ? key : kmin;
      kmax = key > kmax ? key : kmax;
      if (compact) {
        const uint32_t pos = atomicAdd(&ncand[region], 1u);
        if (pos < rs) cand[(size_t)region * rs + pos] = key;
      }
    }
    if (want_b && (key & mb) == pb) bmin = key < bmin ? key : bmin;
  };
  if (c.src == 0) {
    const uint4 *vec = reinterpret_cast<const uint4 *>(data + head);
    for (int64_t j = gtid; j < nvec; j += 2 * gstride) {
      const uint4 w0 = vec[j];
      const uint4 w1 = j + gstride < nvec ? vec[j + gstride] : make_uint4(0, 0, 0, 0);
      T x[V];
      __builtin_memcpy(x, &w0, 16);
#pragma unroll
      for (int k = 0; k < V; ++k) visit(qt_key(x[k]));
      if (j + gstride < nvec) {
        __builtin_memcpy(x, &w1, 16);
#pragma unroll
        for (int k = 0; k < V; ++k) visit(qt_key(x[k]));
      }
    }
    const int64_t tail0 = head + nvec * V, loose = head + (n - tail0);
    for (int64_t t = gtid; t < loose; t += gstride) visit(qt_key(data[t < head ? t : tail0 + (t - head)]));
  } else {
    // (reached only when no region overflowed: qt_select checked)
    for (int64_t i = gtid; i < (int64_t)QT_NSUB * rs; i += gstride)
      if ((uint32_t)(i % rs) < ncand[i / rs]) visit(cand[i]);
  }
  kmin = wave_min_u64(kmin);
  kmax = wave_max_u64(kmax);
  bmin = wave_min_u64(bmin);
  if (lane_id() == 0) {
    s_red[0][threadIdx.x / WAVE] = kmin;
    s_red[1][threadIdx.x / WAVE] = kmax;
    s_red[2][threadIdx.x / WAVE] = bmin;
  }
  block_sync();
  if (threadIdx.x == 0) {
    for (int w = 1; w < QT_THREADS / WAVE; ++w) {
      kmin = s_red[0][w] < kmin ? s_red[0][w] : kmin;
      kmax = s_red[1][w] > kmax ? s_red[1][w] : kmax;
      bmin = s_red[2][w] < bmin ? s_red[2][w] : bmin;
    }
    if (want_a && kmin <= kmax) {
      atomicMin(&st->a.kmin, (unsigned long long)kmin);
      atomicMax(&st->a.kmax, (unsigned long long)kmax);
    }
    if (want_b && bmin != ~0ULL) atomicMin(&st->a.bmin, (unsigned long long)bmin);
  }
  if (want_a)
    for (int i = threadIdx.x; i <= (int)dmask; i += QT_THREADS)
      if (h[i]) atomicAdd(&ghist[i], h[i]);
}

// one workgroup: pick the bucket of the target rank, advance the state, reset the histogram and the accumulators
__global__ __launch_bounds__(QT_THREADS) void qt_select(QtState *st, uint32_t *ghist, const uint32_t *ncand, uint32_t rs) {
  constexpr int PER = QT_BINS / QT_THREADS;
  __shared__ uint32_t s_sum[QT_THREADS];
  __shared__ uint32_t s_b, s_rank, s_cnt, s_next, s_overflow;
  QtCtl c = st->c;
  const QtAcc a = st->a;
  const bool did_a = !c.done;
  if (!did_a && c.y1_state != Y1_MIN_OF_B) return;
  const int t = threadIdx.x;
  const uint32_t bins = 1u << c.dbits;
  uint32_t mine[PER], sum = 0;
#pragma unroll
  for (int i = 0; i < PER; ++i) {
    const uint32_t b = (uint32_t)(t * PER + i);
    mine[i] = (did_a && b < bins) ? ghist[b] : 0u;
    sum += mine[i];
  }
  s_sum[t] = sum;
  if (t == 0) { s_next = 0xffffffffu; s_overflow = 0; }
  block_sync();
  if (c.compact && c.src == 0 && t < QT_NSUB && ncand[t] > rs) atomicOr(&s_overflow, 1u);
  if (did_a) {
    // exclusive prefix of the per-thread sums (256 of them: one serial pass by every thread over the LDS array is cheaper than it
    // looks next to the launch, and needs no scan code)
    uint32_t before = 0;
    for (int u = 0; u < t; ++u) before += s_sum[u];
    if (c.rank >= before && c.rank < before + sum) {
      uint32_t r = c.rank - before;
      for (int i = 0; i < PER; ++i) {
        if (r < mine[i]) { s_b = (uint32_t)(t * PER + i); s_rank = r; s_cnt = mine[i]; break; }
        r -= mine[i];
      }
    }
    block_sync();
    // the first non-empty bucket after s_b (rank k + 1 when it is not in s_b)
    const uint32_t b0 = s_b;
    for (int i = 0; i < PER; ++i) {
      const uint32_t b = (uint32_t)(t * PER + i);
      if (b > b0 && mine[i]) { atomicMin(&s_next, b); break; }
    }
    block_sync();
  }
  if (t == 0) {
    // the pass that just ran looked for rank k + 1 too: its bucket is not empty, so bmin is a key of it (possibly the all-ones one)
    if (c.y1_state == Y1_MIN_OF_B) { c.y1 = a.bmin; c.y1_state = Y1_KNOWN; }
    if (did_a) {
      const uint32_t b = s_b, r = s_rank, cnt = s_cnt;
      const int hi = c.shift + c.dbits;
      c.prefix = (c.prefix & (hi >= 64 ? 0ULL : ~0ULL << hi)) | ((uint64_t)b << c.shift);
      if (c.y1_state == Y1_FOLLOWS && r + 1 >= cnt && s_next != 0xffffffffu) {
        const uint64_t pb = (c.prefix & (hi >= 64 ? 0ULL : ~0ULL << hi)) | ((uint64_t)s_next << c.shift);
        if (c.shift == 0) { c.y1 = pb; c.y1_state = Y1_KNOWN; }
        else { c.prefix_b = pb; c.hi_b = c.shift; c.y1_state = Y1_MIN_OF_B; }
      }
      const bool was_compacting = c.compact && c.src == 0;
      c.rank = r;
      c.count = cnt;
      if (a.kmin == a.kmax) {                                   // every matching key is equal: that is the answer
        c.prefix = a.kmin;
        c.done = 1;
      } else if (c.shift == 0) {
        c.done = 1;
      } else {
        const int ns = c.shift > QT_DIGIT ? c.shift - QT_DIGIT : 0;
        c.dbits = c.shift - ns;
        c.shift = ns;
      }
      if (c.done && c.y1_state == Y1_FOLLOWS) { c.y1 = c.prefix; c.y1_state = Y1_KNOWN; }
      if (c.src == 0) c.column_passes++;
      if (was_compacting) {
        c.compact = 0;
        if (s_overflow) c.allow_compact = 0;         // a region overflowed: keep reading the column
        else c.src = 1;
      } else if (c.src == 0 && c.allow_compact && (uint64_t)cnt * 2 <= (uint64_t)QT_NSUB * rs) {
        c.compact = 1;
      }
    }
    st->c = c;
    st->a.kmin = ~0ULL;
    st->a.kmax = 0;
    st->a.bmin = ~0ULL;
  }
  if (did_a)
    for (int i = 0; i < PER; ++i) ghist[t * PER + i] = 0;
}

// ranks k (and k + 1 unless `one`) of a mask-free column -> host keys
template <class T>
static gdf_error radix_select(const gdf_column *col, uint32_t k, bool one, uint64_t *key0, uint64_t *key1) {
  const int64_t n = (int64_t)col->size;
  constexpr int B = 8 * (int)sizeof(T);
  constexpr int V = 16 / (int)sizeof(T);
  int64_t head = n, nvec = 0;
  const uintptr_t addr = (uintptr_t)col->data;
  if (addr % sizeof(T) == 0) {
    head = (int64_t)(((16 - (addr & 15)) & 15) / sizeof(T));
    if (head > n) head = n;
    nvec = (n - head) / V;
  }
  const uint32_t cap = (uint32_t)(n < (int64_t)QT_CAND_CAP ? n : QT_CAND_CAP);
  const uint32_t rs = (cap + QT_NSUB - 1) / QT_NSUB;
  DevBuf scratch;
  const size_t hist_off = 256, cnt_off = hist_off + sizeof(uint32_t) * QT_BINS, cand_off = cnt_off + sizeof(uint32_t) * QT_NSUB;
  RMM_TRY(scratch.alloc(cand_off + sizeof(uint64_t) * (size_t)QT_NSUB * rs));
  QtState *st = scratch.as<QtState>();
  uint32_t *hist = reinterpret_cast<uint32_t *>(scratch.as<unsigned char>() + hist_off);
  uint64_t *cand = reinterpret_cast<uint64_t *>(scratch.as<unsigned char>() + cand_off);
  uint32_t *ncand = reinterpret_cast<uint32_t *>(scratch.as<unsigned char>() + cnt_off);

  QtCtl init{};
  init.rank = k;
  init.count = (uint32_t)n;
  init.shift = B > QT_DIGIT ? B - QT_DIGIT : 0;
  init.dbits = B - init.shift;
  init.hi_b = 64;
  init.y1_state = one ? Y1_UNWANTED : Y1_FOLLOWS;
  init.allow_compact = lab::path_on("GDF_QT_NO_COMPACT") ? 0 : 1;
  const int passes = (B + QT_DIGIT - 1) / QT_DIGIT;
  const int64_t per_block = (int64_t)QT_THREADS * 2;
  int64_t g = (std::max<int64_t>(nvec, 1) + per_block - 1) / per_block;
  g = std::min<int64_t>(g, (int64_t)device_cu_count() * 4);
  const int grid = (int)std::max<int64_t>(g, 1);

  hipLaunchKernelGGL(qt_init, dim3(1), dim3(64), 0, stream0(), st, init, hist, ncand);
  for (int p = 0; p < passes; ++p) {
    GDF_LAUNCH("qt_pass", (qt_pass<T>), dim3(grid), dim3(QT_THREADS), 0, stream0(), (const T *)col->data, n, head, nvec, st, hist, cand, ncand, rs);
    GDF_LAUNCH("qt_select", qt_select, dim3(1), dim3(QT_THREADS), 0, stream0(), st, hist, (const uint32_t *)ncand, rs);
  }
  HIP_CHECK_LAST();
  QtCtl out;
  HIP_TRY(read_back(&out, &st->c, sizeof(out)));      // (synchronises the stream: the scratch can go)
  lab::note("qt.column_passes", out.column_passes);   // (the route the search took, for the tests; a no-op without the hook library)
  lab::note("qt.src", out.src);
  lab::note("qt.allow_compact", out.allow_compact);
  if (!out.done || (!one && out.y1_state != Y1_KNOWN)) return GDF_CUDA_ERROR;
  *key0 = out.prefix;
  *key1 = one ? out.prefix : out.y1;
  return GDF_SUCCESS;
}

// y0 = s[k], y1 = s[k+1] (y1 only when `one` is false), by the mode the context asks for
template <class T>
static gdf_error read_ranks(gdf_column *col, const gdf_context *ctxt, uint32_t k, bool one, T *y0, T *y1) {
  if (!ctxt->flag_sorted && ctxt->flag_sort_inplace)
    GDF_TRY(sort_column_inplace(col->data, elem_kind(col->dtype), (uint32_t)col->size));
  if (ctxt->flag_sorted || ctxt->flag_sort_inplace) {
    T hv[2];
    HIP_TRY(read_back(hv, (const T *)col->data + k, (one ? 1 : 2) * sizeof(T)));
    *y0 = hv[0];
    *y1 = one ? hv[0] : hv[1];
    return GDF_SUCCESS;
  }
  uint64_t k0 = 0, k1 = 0;
  GDF_TRY(radix_select<T>(col, k, one, &k0, &k1));
  *y0 = qt_value<T>(k0);
  *y1 = qt_value<T>(k1);
  return GDF_SUCCESS;
}

// y1 - y0 and y0 + y1 in the column type under C promotion (int8 / int16 -> int; int32 / int64 wrap; float stays float)
template <class T> static T wrap_sub(T a, T b) {
  if constexpr (std::is_integral<T>::value) { using U = typename std::make_unsigned<T>::type; return (T)(U)((U)a - (U)b); }
  else return a - b;
}
template <class T> static T wrap_add(T a, T b) {
  if constexpr (std::is_integral<T>::value) { using U = typename std::make_unsigned<T>::type; return (T)(U)((U)a + (U)b); }
  else return a + b;
}
template <class T> static double qt_diff(T y0, T y1) {
  if constexpr (sizeof(T) < 4 && std::is_integral<T>::value) return (double)((int)y1 - (int)y0);
  else return (double)wrap_sub(y1, y0);
}
template <class T> static double qt_sum(T y0, T y1) {
  if constexpr (sizeof(T) < 4 && std::is_integral<T>::value) return (double)((int)y0 + (int)y1);
  else return (double)wrap_add(y0, y1);
}

// prec < 0: approx (writes a T); otherwise exact (writes a double).  No fused multiply-add: LINEAR is the two roundings the rule says.
#pragma clang fp contract(off)
template <class T>
static gdf_error quantile_typed(gdf_column *col, int prec, double q, void *res, const gdf_context *ctxt) {
  const size_t n = col->size;
  T y0, y1;
  double x = 0.0;
  if (q >= 1.0 || n == 1) {
    // the max (s[0] when n == 1); the sort route leaves the column sorted and reads its last element
    if (n == 1 && !ctxt->flag_sort_inplace) {
      HIP_TRY(read_back(&y0, col->data, sizeof(T)));
    } else if (!ctxt->flag_sorted && ctxt->flag_sort_inplace) {
      GDF_TRY(read_ranks<T>(col, ctxt, (uint32_t)(n - 1), true, &y0, &y1));
    } else {
      GDF_TRY(column_max_element(col, &y0));
    }
    if (prec < 0) *(T *)res = y0;
    else *(double *)res = (double)y0;
    return GDF_SUCCESS;
  }
  const double pos = q * (double)n;
  size_t k = (size_t)pos;
  x = pos - (double)k;
  if (k > 0) --k;
  GDF_TRY(read_ranks<T>(col, ctxt, (uint32_t)k, prec < 0, &y0, &y1));
  if (prec < 0) { *(T *)res = y0; return GDF_SUCCESS; }
  double r;
  switch (prec) {
    case GDF_QUANT_LINEAR: r = (double)y0 + x * qt_diff(y0, y1); break;
    case GDF_QUANT_LOWER: r = (double)y0; break;
    case GDF_QUANT_HIGHER: r = (double)y1; break;
    case GDF_QUANT_MIDPOINT: r = qt_sum(y0, y1) / 2.0; break;
    default: r = x < 0.5 ? (double)y0 : (double)y1; break;     // GDF_QUANT_NEAREST
  }
  *(double *)res = r;
  return GDF_SUCCESS;
}

static gdf_error quantile_entry(gdf_column *col, int prec, double q, void *res, gdf_context *ctxt) {
  GDF_REQUIRE(col && res && ctxt, GDF_INVALID_API_CALL);
  GDF_REQUIRE(prec < (int)N_GDF_QUANT_METHODS, GDF_UNSUPPORTED_METHOD);      // (prec < 0 is the approx entry point)
  GDF_REQUIRE(!col->valid, GDF_VALIDITY_UNSUPPORTED);
  GDF_REQUIRE(!(q != q) && q >= 0.0, GDF_INVALID_API_CALL);
  GDF_REQUIRE(col->size > 0, GDF_DATASET_EMPTY);
  GDF_REQUIRE(col->data, GDF_INVALID_API_CALL);
  GDF_REQUIRE(col->size < (size_t)0x7fffffff, GDF_COLUMN_SIZE_TOO_BIG);
  return guarded([&]() -> gdf_error {
    switch (col->dtype) {
      case GDF_INT8: return quantile_typed<int8_t>(col, prec, q, res, ctxt);
      case GDF_INT16: return quantile_typed<int16_t>(col, prec, q, res, ctxt);
      case GDF_INT32: return quantile_typed<int32_t>(col, prec, q, res, ctxt);
      case GDF_INT64: return quantile_typed<int64_t>(col, prec, q, res, ctxt);
      case GDF_FLOAT32: return quantile_typed<float>(col, prec, q, res, ctxt);
      case GDF_FLOAT64: return quantile_typed<double>(col, prec, q, res, ctxt);
      default: return GDF_UNSUPPORTED_DTYPE;
    }
  });
}

}  // namespace gdf_amd

using namespace gdf_amd;

extern "C" {

gdf_error gdf_quantile_exact(gdf_column *col_in, gdf_quantile_method prec, double q, void *t_erased_res, gdf_context *ctxt) {
  if ((int)prec < 0) return GDF_UNSUPPORTED_METHOD;
  return quantile_entry(col_in, (int)prec, q, t_erased_res, ctxt);
}
gdf_error gdf_quantile_aprrox(gdf_column *col_in, double q, void *t_erased_res, gdf_context *ctxt) {
  return quantile_entry(col_in, -1, q, t_erased_res, ctxt);
}

}  // extern "C"
