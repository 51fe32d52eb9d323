// reduce.hip -- whole-column reductions: gdf_{sum,product,min,max}_{generic,f64,f32,i64,i32,i8} and
// gdf_sum_squared_{generic,f64,f32} (reference src/reductions.cu; semantics in include/gdf/gdf.h and DESIGN.md §11).
//
// One launch per call, behind one hipMemsetAsync of the ticket word.  A FIXED grid (sized from the column length and the
// device's CU count, never from timing) streams the column with 16-B loads per lane; every workgroup reduces its share
// (wave shuffles, then LDS) into one partial in a library-owned slot array, publishes it with an agent-scope release and
// draws a ticket; the last arriver acquires and combines the partials in a fixed tree over slot order, then writes
// dev_result[0].  The element -> thread mapping and every combine order are functions of (n, data address, CU count)
// only, so a float result is bit-identical from call to call.
#include "internal.h"

#include <limits>

namespace gdf_amd {

enum RedOp : int { R_SUM = 0, R_PRODUCT, R_MIN, R_MAX, R_SUMSQ, R_MAX_ELEM };

// Acc: the accumulator.  Integers accumulate in an unsigned type at least as wide as T (sum and product are ring
// homomorphisms mod 2^w, so truncating at the end is the same as wrapping in T every step, without signed-overflow UB).
// f32 sum / sum_squared accumulate in f64 and round once; product, min and max work in T.
template <class T, int OP> struct Red {
  static constexpr bool FLT = std::is_floating_point<T>::value;
  static constexpr bool ARITH = OP == R_SUM || OP == R_PRODUCT || OP == R_SUMSQ;
  using UInt = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;
  using Acc = typename std::conditional<!ARITH, T,
              typename std::conditional<FLT, typename std::conditional<OP == R_PRODUCT, T, double>::type, UInt>::type>::type;

  __host__ __device__ static Acc identity() {
    if constexpr (OP == R_SUM || OP == R_SUMSQ) return (Acc)0;
    else if constexpr (OP == R_PRODUCT) return (Acc)1;
    else if constexpr (OP == R_MIN) return std::numeric_limits<T>::max();             // FLT_MAX / DBL_MAX for floats, as the reference
    else if constexpr (OP == R_MAX) return std::numeric_limits<T>::lowest();
    else return FLT ? -std::numeric_limits<T>::infinity() : std::numeric_limits<T>::lowest();   // R_MAX_ELEM: an element's value
  }
  __device__ static Acc lift(T x) {
    if constexpr (OP == R_SUMSQ) return (Acc)x * (Acc)x;
    else return (Acc)x;
  }
  __device__ static Acc combine(Acc a, Acc b) {
    if constexpr (OP == R_SUM || OP == R_SUMSQ) return a + b;
    else if constexpr (OP == R_PRODUCT) return a * b;
    else {
      if constexpr (FLT) {                                   // a valid NaN wins (numpy np.min / np.max)
        if (a != a) return a;
        if (b != b) return b;
      }
      if constexpr (OP == R_MIN) return b < a ? b : a;
      else return b > a ? b : a;
    }
  }
};

template <class A>
__device__ __forceinline__ A shfl_xor_any(A v, int o) {
  if constexpr (sizeof(A) == 8) {
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)u, o, WAVE), hi = (uint32_t)__shfl_xor((int)(uint32_t)(u >> 32), o, WAVE);
    u = ((uint64_t)hi << 32) | lo;
    __builtin_memcpy(&v, &u, 8);
    return v;
  } else if constexpr (sizeof(A) == 4) {
    uint32_t u;
    __builtin_memcpy(&u, &v, 4);
    u = (uint32_t)__shfl_xor((int)u, o, WAVE);
    __builtin_memcpy(&v, &u, 4);
    return v;
  } else {
    return (A)__shfl_xor((int)v, o, WAVE);
  }
}

constexpr int RD_THREADS = 256;
constexpr int RD_WAVES = RD_THREADS / WAVE;
constexpr int RD_UNROLL = 4;                 // 16-B vectors per lane in flight per trip
constexpr size_t RD_SLOT_OFFSET = 256;       // scratch: [ticket (16 B, memset per call) | pad | slots]

// one workgroup's share -> *out (thread 0); every thread of the workgroup calls it
template <class R>
__device__ __forceinline__ typename R::Acc block_combine(typename R::Acc v, typename R::Acc *s_wave) {
  using Acc = typename R::Acc;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) v = R::combine(v, shfl_xor_any(v, o));
  if (lane_id() == 0) s_wave[threadIdx.x / WAVE] = v;
  __syncthreads();
  Acc r = s_wave[0];
#pragma unroll
  for (int w = 1; w < RD_WAVES; ++w) r = R::combine(r, s_wave[w]);
  return r;
}

// Elements [0, head) and [head + nvec * V, n) are the unaligned head and tail (or every element when the data pointer is not
// even element-aligned: head = n, nvec = 0); vector j covers elements head + j*V .. head + j*V + V - 1.
template <class T, int OP>
__global__ __launch_bounds__(RD_THREADS) void rd_column(const T *__restrict__ data, const uint8_t *__restrict__ valid, int64_t n,
                                                        int64_t head, int64_t nvec, typename Red<T, OP>::Acc *slots,
                                                        uint32_t *ticket, T *result) {
  using R = Red<T, OP>;
  using Acc = typename R::Acc;
  constexpr int V = 16 / (int)sizeof(T);
  __shared__ Acc s_wave[RD_WAVES];
  __shared__ int s_last;
  const int64_t gtid = (int64_t)blockIdx.x * RD_THREADS + threadIdx.x, gstride = (int64_t)gridDim.x * RD_THREADS;
  const int64_t mbytes = (n + 7) >> 3;
  Acc acc = R::identity();

  // body: 16-B loads; the mask bits of a vector (V <= 16 of them at bit (e & 7) of byte e >> 3) come from at most 3 mask bytes
  const uint4 *vec = reinterpret_cast<const uint4 *>(data + head);
  for (int64_t j0 = gtid; j0 < nvec; j0 += gstride * RD_UNROLL) {
    uint4 w[RD_UNROLL];
#pragma unroll
    for (int u = 0; u < RD_UNROLL; ++u) {
      const int64_t j = j0 + (int64_t)u * gstride;
      w[u] = j < nvec ? vec[j] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < RD_UNROLL; ++u) {
      const int64_t j = j0 + (int64_t)u * gstride;
      if (j >= nvec) break;
      const int64_t e = head + j * V;
      uint32_t bits = 0xffffffffu;
      if (valid) {
        const int64_t b = e >> 3;
        uint32_t win = valid[b];
        if (b + 1 < mbytes) win |= (uint32_t)valid[b + 1] << 8;
        if (V > 8 && b + 2 < mbytes) win |= (uint32_t)valid[b + 2] << 16;
        bits = win >> (e & 7);
      }
      T x[V];
      __builtin_memcpy(x, &w[u], 16);
#pragma unroll
      for (int k = 0; k < V; ++k)
        if ((bits >> k) & 1) acc = R::combine(acc, R::lift(x[k]));
    }
  }
  // head and tail, one element per thread
  const int64_t tail0 = head + nvec * V, loose = head + (n - tail0);
  for (int64_t t = gtid; t < loose; t += gstride) {
    const int64_t i = t < head ? t : tail0 + (t - head);
    if (!valid || bit_is_set(valid, i)) acc = R::combine(acc, R::lift(data[i]));
  }

  const Acc part = block_combine<R>(acc, s_wave);
  // publish (cdna_hip_programming.md §5 'In-launch split-K reduction'): the one storing lane drains its store, releases at agent
  // scope, drains again, then draws a relaxed ticket
  if (threadIdx.x == 0) {
    slots[blockIdx.x] = part;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const uint32_t t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = t == gridDim.x - 1;
  }
  __syncthreads();
  if (!s_last) return;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __syncthreads();
  // the last arriver: thread t folds slots t, t + 256, ... in that order, then the same shuffle / LDS tree as above
  Acc r = R::identity();
  for (uint32_t s = threadIdx.x; s < gridDim.x; s += RD_THREADS) r = R::combine(r, slots[s]);
  const Acc total = block_combine<R>(r, s_wave);
  if (threadIdx.x == 0) *result = (T)total;
}

// grid: enough workgroups for RD_UNROLL vectors per lane, at most 4 per CU; depends on (n, CU count) only
static int rd_grid(int64_t nvec) {
  const int64_t per_block = (int64_t)RD_THREADS * RD_UNROLL;
  int64_t g = (nvec + per_block - 1) / per_block;
  const int64_t cap = (int64_t)device_cu_count() * 4;
  if (g > cap) g = cap;
  if (g < 1) g = 1;
  return (int)g;
}

template <class T, int OP>
static gdf_error reduce_launch(const gdf_column *col, T *dev_result) {
  using Acc = typename Red<T, OP>::Acc;
  const int64_t n = (int64_t)col->size;
  int64_t head = n, nvec = 0;
  const uintptr_t addr = (uintptr_t)col->data;
  if (n > 0 && addr % sizeof(T) == 0) {
    head = (int64_t)(((16 - (addr & 15)) & 15) / sizeof(T));
    if (head > n) head = n;
    nvec = (n - head) / (16 / (int64_t)sizeof(T));
  }
  const int grid = rd_grid(nvec);
  DevBuf scratch;
  RMM_TRY(scratch.alloc(RD_SLOT_OFFSET + sizeof(Acc) * (size_t)grid));
  uint32_t *ticket = scratch.as<uint32_t>();
  Acc *slots = reinterpret_cast<Acc *>(scratch.as<unsigned char>() + RD_SLOT_OFFSET);
  HIP_TRY(hipMemsetAsync(ticket, 0, 16, stream0()));
  static const char *const names[] = {"rd_sum", "rd_product", "rd_min", "rd_max", "rd_sum_squared", "rd_max"};
  GDF_LAUNCH(names[OP], (rd_column<T, OP>), dim3(grid), dim3(RD_THREADS), 0, stream0(), (const T *)col->data,
             (const uint8_t *)col->valid, n, head, nvec, slots, ticket, dev_result);
  HIP_CHECK_LAST();
  HIP_TRY(hipStreamSynchronize(stream0()));      // scratch is released on return
  return GDF_SUCCESS;
}

// op on a column of storage kind `kind` -> dev_result[0]
template <int OP>
static gdf_error reduce_kind(const gdf_column *col, ElemKind kind, void *dev_result) {
  switch (kind) {
    case K_I8: return reduce_launch<int8_t, OP>(col, (int8_t *)dev_result);
    case K_I32: return reduce_launch<int32_t, OP>(col, (int32_t *)dev_result);
    case K_I64: return reduce_launch<int64_t, OP>(col, (int64_t *)dev_result);
    case K_F32: return reduce_launch<float, OP>(col, (float *)dev_result);
    case K_F64: return reduce_launch<double, OP>(col, (double *)dev_result);
    case K_I16:
      if constexpr (OP == R_MAX_ELEM) return reduce_launch<int16_t, OP>(col, (int16_t *)dev_result);
      return GDF_UNSUPPORTED_DTYPE;
    default: return GDF_UNSUPPORTED_DTYPE;
  }
}

static bool reduce_dtype_ok(int op, gdf_dtype t) {
  switch (t) {
    case GDF_FLOAT32: case GDF_FLOAT64: return true;
    case GDF_INT8: case GDF_INT32: case GDF_INT64: return op != R_SUMSQ;      // reference DEF_REDUCE_OP_REAL: floats only
    default: return false;
  }
}

// typed entry point: `want` is the storage kind of T; the column's dtype must have that storage (a DATE32 column is an int32
// column); generic: want == K_BAD, dispatch on the dtype
template <int OP>
static gdf_error reduce_entry(gdf_column *col, void *dev_result, gdf_size_type dev_result_size, ElemKind want) {
  GDF_REQUIRE(col && dev_result && dev_result_size >= 1, GDF_INVALID_API_CALL);
  GDF_REQUIRE(col->size == 0 || col->data, GDF_INVALID_API_CALL);
  ElemKind kind;
  if (want == K_BAD) {
    GDF_REQUIRE(reduce_dtype_ok(OP, col->dtype), GDF_UNSUPPORTED_DTYPE);
    kind = elem_kind(col->dtype);
  } else {
    GDF_REQUIRE(elem_kind(col->dtype) == want, GDF_DTYPE_MISMATCH);
    kind = want;
  }
  return guarded([&]() -> gdf_error { return reduce_kind<OP>(col, kind, dev_result); });
}

// quantile.hip: the largest element of a non-empty, mask-free column (NaN if there is one) -> host
gdf_error column_max_element(const gdf_column *col, void *host_result) {
  const ElemKind kind = elem_kind(col->dtype);
  const int w = kind_width(kind);
  DevBuf out;
  RMM_TRY(out.alloc(16));
  GDF_TRY(reduce_kind<R_MAX_ELEM>(col, kind, out.p));
  HIP_TRY(read_back(host_result, out.p, (size_t)w));
  return GDF_SUCCESS;
}

}  // namespace gdf_amd

using namespace gdf_amd;

extern "C" {

unsigned int gdf_reduce_optimal_output_size(void) { return 128; }   // the reference's value; any size >= 1 works here

#define GDF_REDUCE_DEF(op, OPC, sfx, T, KIND)                                                        \
  gdf_error gdf_##op##_##sfx(gdf_column *col, T *dev_result, gdf_size_type dev_result_size) { \
    return reduce_entry<OPC>(col, (void *)dev_result, dev_result_size, KIND);                        \
  }
#define GDF_X_REDUCE_ALL(op, OPC)                                                                  \
  GDF_REDUCE_DEF(op, OPC, generic, void, K_BAD) GDF_REDUCE_DEF(op, OPC, f64, double, K_F64)        \
  GDF_REDUCE_DEF(op, OPC, f32, float, K_F32)    GDF_REDUCE_DEF(op, OPC, i64, int64_t, K_I64)       \
  GDF_REDUCE_DEF(op, OPC, i32, int32_t, K_I32)  GDF_REDUCE_DEF(op, OPC, i8, int8_t, K_I8)
GDF_X_REDUCE_ALL(sum, R_SUM)
GDF_X_REDUCE_ALL(product, R_PRODUCT)
GDF_X_REDUCE_ALL(min, R_MIN)
GDF_X_REDUCE_ALL(max, R_MAX)
GDF_REDUCE_DEF(sum_squared, R_SUMSQ, generic, void, K_BAD)
GDF_REDUCE_DEF(sum_squared, R_SUMSQ, f64, double, K_F64)
GDF_REDUCE_DEF(sum_squared, R_SUMSQ, f32, float, K_F32)
#undef GDF_X_REDUCE_ALL
#undef GDF_REDUCE_DEF

}  // extern "C"
