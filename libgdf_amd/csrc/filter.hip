// filter.hip -- predicate stencils, stream compaction, row filter and the valid-mask
// helpers that go with them.
//
// Reference code being replaced:
//   gpu_comparison / gpu_comparison_static_*  src/filterops.cu:97-662   (thrust::transform per dtype pair)
//   gpu_apply_stencil                         src/streamcompactionops.cu:208-339 (copy_if + byte-expanded mask re-pack)
//   gdf_filter                                src/sqls_ops.cu:1401-1424 + sqls_rtti_comp.hpp:78-97,343-370
//   gdf_count_nonzero_mask / gdf_mask_concat  src/validops.cu:86-256
//   gdf_validity_and                          src/binaryops.cu (mask AND)
//   gdf_column_concat                         src/column.cpp:53-153
//
// Compaction shape (compact_kernel + its two small helpers): each workgroup owns a
// contiguous chunk, counts its keepers with wave ballots (pass 1), an exclusive scan
// of the per-chunk counts gives every chunk its output base, and pass 2 re-evaluates
// the predicate and writes keepers at base + ballot rank -- output order is the input
// order (stable), no atomics, no temporary index list.
//
// Deliberate deviations from the reference (SURVEY.md 8a "quirks" 1 and 2):
//   * GDF_LESS_THAN / GDF_LESS_THAN_OR_EQUALS compute x < y / x <= y (the reference's
//     functors return x > y / x >= y, filterops.cu:57-75 -- an untested bug);
//   * the stencil's valid mask is read LSB-first like every other mask in libgdf
//     (streamcompactionops.cu:99-105 reads it MSB-first through an uninitialised field).
#include "internal.h"

#include <cstdlib>
#include <type_traits>
#include <vector>

namespace gdf_amd {

constexpr int FL_THREADS = 256;
constexpr int FL_MAX_CHUNKS = 2048;
constexpr int64_t FL_ROUNDS_MIN = (int64_t)1 << 22;      // rows from which gpu_apply_stencil is one pass in lockstep rounds (compact)

// ---------------------------------------------------------------------------
// comparisons
// ---------------------------------------------------------------------------
template <class L, class R>
__device__ __forceinline__ int8_t compare(L x, R y, int op) {
  switch (op) {   // usual arithmetic conversions apply to (L, R), as in the reference's functors
    case GDF_EQUALS: return x == y;
    case GDF_NOT_EQUALS: return x != y;
    case GDF_LESS_THAN: return x < y;
    case GDF_LESS_THAN_OR_EQUALS: return x <= y;
    case GDF_GREATER_THAN: return x > y;
    default: return x >= y;
  }
}

// RIGHT_SCALAR: `rhs` is ignored and `scalar` is compared against every element
template <class L, class R, bool RIGHT_SCALAR>
__global__ __launch_bounds__(FL_THREADS) void compare_kernel(const L *__restrict__ lhs, const R *__restrict__ rhs, R scalar,
                                                             int8_t *__restrict__ out, int64_t n, int op) {
  for (int64_t i = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * FL_THREADS)
    out[i] = compare<L, R>(lhs[i], RIGHT_SCALAR ? scalar : rhs[i], op);
}

// The same on 16-byte vectors (round 5): a lane reads 16 / sizeof(L) consecutive elements of the left column (and of the right one when it
// has the same width), four vectors per lane in flight, and stores their result bytes with one store -- the element-wise kernel above keeps
// 8 bytes per lane in flight and writes one byte per lane (1e9 int64 rows against a scalar: 1.97 ms, 4.6 TB/s).  Columns that are 16-byte
// aligned, n in whole vectors for the body; the tail takes the element-wise kernel.
template <class L, class R, bool RIGHT_SCALAR>
__global__ __launch_bounds__(FL_THREADS) void compare_vec_kernel(const L *__restrict__ lhs, const R *__restrict__ rhs, R scalar,
                                                                 int8_t *__restrict__ out, int64_t nvec, int op) {
  constexpr int EPV = 16 / (int)sizeof(L);
  constexpr int UNROLL = 4;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  union VL { u32x4 q; L e[EPV]; };
  union VR { u32x4 q; R e[EPV]; };
  union Res { int8_t b[EPV]; uint16_t h; uint32_t w; uint64_t d; u32x4 q; };
  // a workgroup takes CONTIGUOUS tiles of FL_THREADS x UNROLL vectors (16 KB of the left column), lane l of round u the vector
  // u * FL_THREADS + l of the tile (round 6; before, a lane's four vectors lay gridDim.x * 4 KB apart -- every workgroup had four
  // distant 4 KB pieces in flight: 1e9 int64 rows against a scalar 1.85 - 1.98 ms, now 1.72 - 1.79; eight vectors per lane: the same)
  constexpr int64_t TILEV = (int64_t)FL_THREADS * UNROLL;
  const int64_t ntile = (nvec + TILEV - 1) / TILEV;
  constexpr int64_t stride = FL_THREADS;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t v0 = tile * TILEV + threadIdx.x;
    VL a[UNROLL];
    VR b[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t v = v0 + u * stride;
      const int64_t vc = v < nvec ? v : nvec - 1;
      a[u].q = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(lhs) + vc);
      if (!RIGHT_SCALAR) b[u].q = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(rhs) + vc);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; ++u) {
      const int64_t v = v0 + u * stride;
      if (v >= nvec) break;
      Res r;
#pragma unroll
      for (int e = 0; e < EPV; ++e) r.b[e] = compare<L, R>(a[u].e[e], RIGHT_SCALAR ? scalar : b[u].e[e], op);
      int8_t *dst = out + v * EPV;
      if (EPV == 2) *reinterpret_cast<uint16_t *>(dst) = r.h;
      else if (EPV == 4) *reinterpret_cast<uint32_t *>(dst) = r.w;
      else if (EPV == 8) *reinterpret_cast<uint64_t *>(dst) = r.d;
      else *reinterpret_cast<u32x4 *>(dst) = r.q;
    }
  }
}

template <class L, class R, bool RIGHT_SCALAR>
static void launch_compare(const void *l, const void *r, R scalar, void *out, int64_t n, int op) {
  if (n == 0) return;
  constexpr int EPV = 16 / (int)sizeof(L);
  int64_t done = 0;
  if constexpr (RIGHT_SCALAR || sizeof(L) == sizeof(R)) {
    const bool aligned = ((uintptr_t)l % 16 == 0) && (RIGHT_SCALAR || (uintptr_t)r % 16 == 0) && ((uintptr_t)out % 16 == 0);
    const int64_t nvec = n / EPV;
    if (aligned && nvec >= 1024) {
      GDF_LAUNCH("compare", (compare_vec_kernel<L, R, RIGHT_SCALAR>), dim3(stream_grid((size_t)nvec, FL_THREADS * 4)), dim3(FL_THREADS), 0,
                 stream0(), (const L *)l, (const R *)r, scalar, (int8_t *)out, nvec, op);
      done = nvec * EPV;
      if (done == n) return;
    }
  }
  GDF_LAUNCH("compare", (compare_kernel<L, R, RIGHT_SCALAR>), dim3(stream_grid((size_t)(n - done), FL_THREADS * 8)), dim3(FL_THREADS), 0,
                     stream0(), (const L *)l + done, RIGHT_SCALAR ? (const R *)r : (const R *)r + done, scalar, (int8_t *)out + done, n - done, op);
}

template <class R, bool RIGHT_SCALAR>
static gdf_error dispatch_left(ElemKind lk, const void *l, const void *r, R scalar, void *out, int64_t n, int op) {
  switch (lk) {
    case K_I8: launch_compare<int8_t, R, RIGHT_SCALAR>(l, r, scalar, out, n, op); break;
    case K_I16: launch_compare<int16_t, R, RIGHT_SCALAR>(l, r, scalar, out, n, op); break;
    case K_I32: launch_compare<int32_t, R, RIGHT_SCALAR>(l, r, scalar, out, n, op); break;
    case K_I64: launch_compare<int64_t, R, RIGHT_SCALAR>(l, r, scalar, out, n, op); break;
    case K_F32: launch_compare<float, R, RIGHT_SCALAR>(l, r, scalar, out, n, op); break;
    case K_F64: launch_compare<double, R, RIGHT_SCALAR>(l, r, scalar, out, n, op); break;
    default: return GDF_UNSUPPORTED_DTYPE;
  }
  return GDF_SUCCESS;
}

// ---------------------------------------------------------------------------
// mask helpers
// ---------------------------------------------------------------------------
// out = a & b (null pointer = all ones) over ceil(n/8) bytes; counts zero bits among the first n
__global__ __launch_bounds__(FL_THREADS) void mask_and_kernel(const uint8_t *a, const uint8_t *b, uint8_t *out, int64_t n,
                                                              unsigned long long *zero_bits) {
  const int64_t nbytes = (n + 7) / 8;
  unsigned long long zeros = 0;
  for (int64_t i = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; i < nbytes; i += (int64_t)gridDim.x * FL_THREADS) {
    const uint8_t v = (a ? a[i] : 0xff) & (b ? b[i] : 0xff);
    if (out) out[i] = v;
    const int live = (i == nbytes - 1 && (n & 7)) ? (int)(n & 7) : 8;
    zeros += live - __popc((unsigned)v & ((1u << live) - 1));
  }
  zeros = wave_reduce_add(zeros);
  if (lane_id() == 0 && zeros) atomicAdd(zero_bits, zeros);
}

__global__ __launch_bounds__(FL_THREADS) void mask_popcount_kernel(const uint8_t *m, int64_t n, unsigned long long *ones) {
  const int64_t nbytes = (n + 7) / 8;
  unsigned long long c = 0;
  for (int64_t i = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; i < nbytes; i += (int64_t)gridDim.x * FL_THREADS) {
    const int live = (i == nbytes - 1 && (n & 7)) ? (int)(n & 7) : 8;
    c += __popc((unsigned)m[i] & ((1u << live) - 1));
  }
  c = wave_reduce_add(c);
  if (lane_id() == 0 && c) atomicAdd(ones, c);
}

static gdf_error mask_and(const uint8_t *a, const uint8_t *b, uint8_t *out, int64_t n, gdf_size_type *null_count) {
  DevBuf z;
  RMM_TRY(z.alloc(sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(z.p, 0, sizeof(unsigned long long), stream0()));
  if (n) hipLaunchKernelGGL(mask_and_kernel, dim3(stream_grid((size_t)(n + 7) / 8, FL_THREADS * 16)), dim3(FL_THREADS), 0, stream0(), a, b, out, n,
                            z.as<unsigned long long>());
  HIP_CHECK_LAST();
  unsigned long long h = 0;
  HIP_TRY(read_back(&h, z.p, sizeof(h)));
  *null_count = (gdf_size_type)h;
  return GDF_SUCCESS;
}

// output mask of a comparison (filterops.cu:139-153)
static gdf_error comparison_mask(gdf_column *out, const gdf_valid_type *vl, const gdf_valid_type *vr, gdf_size_type ncl,
                                 gdf_size_type ncr, int64_t n) {
  if (ncl == 0 && ncr == 0) {
    if (out->valid) HIP_TRY(hipMemsetAsync(out->valid, 0xff, mask_bytes((size_t)n), stream0()));
    out->null_count = 0;
  } else if (vl == vr) {
    if (out->valid && vl) HIP_TRY(hipMemcpyAsync(out->valid, vl, mask_bytes((size_t)n), hipMemcpyDeviceToDevice, stream0()));
    out->null_count = ncl;
  } else {
    GDF_TRY(mask_and(vl, vr, out->valid, n, &out->null_count));
  }
  HIP_TRY(hipStreamSynchronize(stream0()));
  return GDF_SUCCESS;
}

template <class T>
static gdf_error comparison_static(gdf_column *lhs, T value, gdf_column *output, gdf_comparison_operator op) {
  GDF_REQUIRE(lhs && output, GDF_DATASET_EMPTY);
  GDF_REQUIRE(lhs->size == output->size, GDF_COLUMN_SIZE_MISMATCH);
  GDF_REQUIRE(output->dtype == GDF_INT8, GDF_COLUMN_SIZE_MISMATCH);   // sic: filterops.cu:166
  // the reference silently does nothing for other dtypes (filterops.cu:171-228); dates are stored as ints
  const ElemKind lk = (lhs->dtype >= GDF_INT8 && lhs->dtype <= GDF_FLOAT64) ? elem_kind(lhs->dtype) : K_BAD;
  if (lk != K_BAD) {
    GDF_TRY((dispatch_left<T, true>(lk, lhs->data, nullptr, value, output->data, (int64_t)lhs->size, (int)op)));
    HIP_CHECK_LAST();
    GDF_TRY(comparison_mask(output, lhs->valid, lhs->valid, lhs->null_count, lhs->null_count, (int64_t)lhs->size));
  }
  return GDF_SUCCESS;
}

// ---------------------------------------------------------------------------
// stable stream compaction
// ---------------------------------------------------------------------------
struct StencilPred {     // keep row i iff stencil[i] != 0 and its valid bit is set (streamcompactionops.cu:162-172)
  const int8_t *stencil;
  const uint8_t *valid;
  __device__ __forceinline__ bool operator()(int64_t i) const {
    return stencil[i] != 0 && (valid ? bit_is_set(valid, i) : true);
  }
};

struct RowEqualsPred {   // every column equals its scalar (LesserRTTI::equal_v, sqls_rtti_comp.hpp:78-97)
  int ncols;
  void *const *cols;     // device array of column data pointers
  const int *types;      // device array of gdf_dtype
  void *const *vals;     // device array of pointers to one device value each
  __device__ __forceinline__ bool operator()(int64_t i) const {
    for (int c = 0; c < ncols; ++c) {
      const void *d = cols[c];
      const void *v = vals[c];
      bool eq;
      switch (types[c]) {
        case GDF_INT8: eq = ((const int8_t *)d)[i] == *(const int8_t *)v; break;
        case GDF_INT16: eq = ((const int16_t *)d)[i] == *(const int16_t *)v; break;
        case GDF_INT32: case GDF_DATE32: eq = ((const int32_t *)d)[i] == *(const int32_t *)v; break;
        case GDF_INT64: case GDF_DATE64: case GDF_TIMESTAMP: eq = ((const int64_t *)d)[i] == *(const int64_t *)v; break;
        case GDF_FLOAT32: eq = ((const float *)d)[i] == *(const float *)v; break;
        case GDF_FLOAT64: eq = ((const double *)d)[i] == *(const double *)v; break;
        default: eq = false;
      }
      if (!eq) return false;
    }
    return true;
  }
};

template <class Pred>
__global__ __launch_bounds__(FL_THREADS) void compact_count_kernel(Pred pred, int64_t n, int64_t chunk, uint64_t *chunk_count) {
  __shared__ unsigned int wsum[FL_THREADS / WAVE];
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < n ? begin + chunk : n;
  unsigned int c = 0;
  for (int64_t i = begin + threadIdx.x; i < end; i += FL_THREADS) c += pred(i) ? 1u : 0u;
  c = wave_reduce_add(c);
  if (lane_id() == 0) wsum[threadIdx.x / WAVE] = c;
  block_sync();
  if (threadIdx.x == 0) {
    unsigned int t = 0;
    for (int w = 0; w < FL_THREADS / WAVE; ++w) t += wsum[w];
    chunk_count[blockIdx.x] = t;
  }
}

// The count pass of gpu_apply_stencil reads ONE byte per row; with a byte load per thread a wave keeps 64 B in flight
// and the pass ran at 0.6 TB/s.  Here a thread takes 16 consecutive rows with one 16-byte load (the count needs no
// order).  chunk is a multiple of 16 and the stencil buffer is 16-byte aligned (checked by the caller).
__global__ __launch_bounds__(FL_THREADS) void stencil_count_kernel(const int8_t *__restrict__ stencil, const uint8_t *__restrict__ valid,
                                                                   int64_t n, int64_t chunk, uint64_t *chunk_count) {
  __shared__ unsigned int wsum[FL_THREADS / WAVE];
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < n ? begin + chunk : n;
  unsigned int c = 0;
  for (int64_t i = begin + (int64_t)threadIdx.x * 16; i < end; i += (int64_t)FL_THREADS * 16) {
    if (i + 16 <= end) {
      const uint4 w = *reinterpret_cast<const uint4 *>(stencil + i);
      const uint32_t words[4] = {w.x, w.y, w.z, w.w};
      uint32_t keep = 0;                              // bit r: row i + r has a non-zero stencil byte
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int b = 0; b < 4; ++b) keep |= ((words[q] >> (8 * b)) & 0xffu) ? (1u << (4 * q + b)) : 0u;
      if (valid) keep &= (uint32_t)valid[i >> 3] | ((uint32_t)valid[(i >> 3) + 1] << 8);      // i is a multiple of 16
      c += (unsigned)__popc(keep);
    } else {
      for (int64_t r = i; r < end; ++r) c += (stencil[r] != 0 && (valid ? bit_is_set(valid, r) : true)) ? 1u : 0u;
    }
  }
  c = wave_reduce_add(c);
  if (lane_id() == 0) wsum[threadIdx.x / WAVE] = c;
  block_sync();
  if (threadIdx.x == 0) {
    unsigned int t = 0;
    for (int w = 0; w < FL_THREADS / WAVE; ++w) t += wsum[w];
    chunk_count[blockIdx.x] = t;
  }
}

// The matching write pass: a thread owns 16 CONSECUTIVE rows (one 16-byte stencil load, its data elements in
// registers), thread totals are scanned once per 4096-row tile (two barriers per tile instead of two per 256 rows),
// and every thread stores its kept elements one after the other -- adjacent lanes write adjacent ranges.
template <int WIDTH>
__global__ __launch_bounds__(FL_THREADS) void stencil_write_kernel(const int8_t *__restrict__ stencil, const uint8_t *__restrict__ valid,
                                                                   int64_t n, int64_t chunk, const uint64_t *__restrict__ chunk_base,
                                                                   const void *__restrict__ in, void *__restrict__ out) {
  __shared__ unsigned int wsum[FL_THREADS / WAVE];
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < n ? begin + chunk : n;
  uint64_t base = chunk_base[blockIdx.x];
  const int wave = threadIdx.x / WAVE;
  for (int64_t tile = begin; tile < end; tile += (int64_t)FL_THREADS * 16) {
    const int64_t i = tile + (int64_t)threadIdx.x * 16;
    uint32_t keep = 0;
    if (i + 16 <= end) {
      const uint4 w = *reinterpret_cast<const uint4 *>(stencil + i);
      const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int b = 0; b < 4; ++b) keep |= ((words[q] >> (8 * b)) & 0xffu) ? (1u << (4 * q + b)) : 0u;
      if (valid) keep &= (uint32_t)valid[i >> 3] | ((uint32_t)valid[(i >> 3) + 1] << 8);
    } else {
      for (int r = 0; r < 16; ++r)
        if (i + r < end && stencil[i + r] != 0 && (valid ? bit_is_set(valid, i + r) : true)) keep |= 1u << r;
    }
    const unsigned int mine = (unsigned)__popc(keep);
    const unsigned int incl = wave_scan_incl(mine);
    if (lane_id() == WAVE - 1) wsum[wave] = incl;
    block_sync();
    unsigned int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < FL_THREADS / WAVE; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    uint64_t pos = base + before + incl - mine;
    if (mine > 4 && i + 16 <= end) {
      // many keepers: fetch the thread's 16 elements with independent loads first, then store the kept ones
      uint64_t v[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (WIDTH == 1) v[r] = ((const uint8_t *)in)[i + r];
        else if (WIDTH == 2) v[r] = ((const uint16_t *)in)[i + r];
        else if (WIDTH == 4) v[r] = ((const uint32_t *)in)[i + r];
        else v[r] = ((const uint64_t *)in)[i + r];
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (keep & (1u << r)) {
          if (WIDTH == 1) ((uint8_t *)out)[pos] = (uint8_t)v[r];
          else if (WIDTH == 2) ((uint16_t *)out)[pos] = (uint16_t)v[r];
          else if (WIDTH == 4) ((uint32_t *)out)[pos] = (uint32_t)v[r];
          else ((uint64_t *)out)[pos] = v[r];
          ++pos;
        }
      }
    } else {
      while (keep) {
        const int r = __ffs((int)keep) - 1;
        keep &= keep - 1;
        if (WIDTH == 1) ((uint8_t *)out)[pos] = ((const uint8_t *)in)[i + r];
        else if (WIDTH == 2) ((uint16_t *)out)[pos] = ((const uint16_t *)in)[i + r];
        else if (WIDTH == 4) ((uint32_t *)out)[pos] = ((const uint32_t *)in)[i + r];
        else ((uint64_t *)out)[pos] = ((const uint64_t *)in)[i + r];
        ++pos;
      }
    }
    base += total;
    block_sync();
  }
}

// The write pass through an LDS stage (round 5): every global access of a 4096-row tile is a coalesced 16-byte vector.  A thread turns the
// stencil bytes of 16 consecutive rows into keep bits (one 16-byte load) and the tile scans the threads' counts as above; the keep words
// and their prefixes go to LDS.  Then the COLUMN is read as consecutive vectors (lane l of round k takes vector k * 256 + l -- the layout the
// scan kernels use), every element looks its rank up (prefix of its 16-row group + the kept rows before it in the group) and drops into the
// stage at that rank; the stage leaves as one contiguous run.  Three barriers per tile.  stencil_write_kernel read its 16 elements with a
// stride of 16 x WIDTH bytes between lanes and stored element by element; the ballot kernel below takes two barriers per 256 rows -- at
// 1e9 int64 rows they moved 3.4 - 4.9 TB/s depending on the selectivity.
constexpr int FLS_ROWS = FL_THREADS * 16;
template <int WIDTH>
__global__ __launch_bounds__(FL_THREADS) void stencil_stage_write_kernel(const int8_t *__restrict__ stencil, const uint8_t *__restrict__ valid,
                                                                         int64_t n, int64_t chunk, const uint64_t *__restrict__ chunk_base,
                                                                         const void *__restrict__ in, void *__restrict__ out) {
  using T = typename std::conditional<WIDTH == 1, uint8_t, typename std::conditional<WIDTH == 2, uint16_t,
            typename std::conditional<WIDTH == 4, uint32_t, uint64_t>::type>::type>::type;
  constexpr int EPV = 16 / WIDTH;                       // elements per 16-byte vector
  constexpr int ROUNDS = FLS_ROWS / (FL_THREADS * EPV);  // vectors per thread and tile (int64: 8, int8: 1)
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  union Vec { u32x4 q; T e[EPV]; };
  __shared__ unsigned int wsum[FL_THREADS / WAVE];
  __shared__ uint32_t s_keep[FL_THREADS], s_pre[FL_THREADS];
  __shared__ __attribute__((aligned(16))) T stage[FLS_ROWS];
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < n ? begin + chunk : n;
  uint64_t base = chunk_base[blockIdx.x];
  const int wave = threadIdx.x / WAVE;
  const T *src = reinterpret_cast<const T *>(in);
  T *dst = reinterpret_cast<T *>(out);
  for (int64_t tile = begin; tile < end; tile += FLS_ROWS) {
    const bool whole = tile + FLS_ROWS <= end;
    // the column's vectors are requested first: they are in flight under the stencil's load and the scan
    Vec v[ROUNDS];
    if (whole) {
      const u32x4 *vsrc = reinterpret_cast<const u32x4 *>(src + tile);
#pragma unroll
      for (int k = 0; k < ROUNDS; ++k) v[k].q = __builtin_nontemporal_load(vsrc + k * FL_THREADS + threadIdx.x);
    }
    const int64_t i = tile + (int64_t)threadIdx.x * 16;
    uint32_t keep = 0;
    if (i + 16 <= end) {
      const uint4 w = *reinterpret_cast<const uint4 *>(stencil + i);
      const uint32_t words[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int b = 0; b < 4; ++b) keep |= ((words[q] >> (8 * b)) & 0xffu) ? (1u << (4 * q + b)) : 0u;
      if (valid) keep &= (uint32_t)valid[i >> 3] | ((uint32_t)valid[(i >> 3) + 1] << 8);
    } else {
      for (int r = 0; r < 16; ++r)
        if (i + r < end && stencil[i + r] != 0 && (valid ? bit_is_set(valid, i + r) : true)) keep |= 1u << r;
    }
    const unsigned int mine = (unsigned)__popc(keep);
    const unsigned int incl = wave_scan_incl(mine);
    if (lane_id() == WAVE - 1) wsum[wave] = incl;
    block_sync();
    unsigned int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < FL_THREADS / WAVE; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    s_keep[threadIdx.x] = keep;
    s_pre[threadIdx.x] = before + incl - mine;
    block_sync();
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
      const uint32_t row0 = (uint32_t)(k * FL_THREADS + threadIdx.x) * EPV;       // first row of this vector inside the tile
      // (EPV <= 16 and a vector never straddles a 16-row group: one keep word and one prefix per vector)
      const uint32_t kb = s_keep[row0 >> 4], pre = s_pre[row0 >> 4];
#pragma unroll
      for (int e = 0; e < EPV; ++e) {
        const uint32_t bit = (row0 + e) & 15u;
        if ((kb >> bit) & 1u) {
          T x;
          if (whole) x = v[k].e[e];
          else x = src[tile + row0 + e];                 // (kept rows lie below `end`)
          stage[pre + __popc(kb & ((1u << bit) - 1u))] = x;
        }
      }
    }
    block_sync();
    for (uint32_t j = threadIdx.x; j < total; j += FL_THREADS) dst[base + j] = stage[j];
    base += total;
  }
}

// ONE pass in lockstep ROUNDS (round 6; the scheme of csrc/scan.hip's scan_rounds): no count pass.  G resident workgroups; round r is
// the G SUPER-TILES r G ... r G + G - 1 of K consecutive 4096-row tiles each, workgroup b takes super-tile r G + b.  A super-tile's
// number of kept rows is known as soon as its stencil bytes are (K 16-byte loads per thread, requested two rounds AHEAD); it goes into
// slot [r & 3][b] (tagged r + 1) a whole step before the others' are needed, and every workgroup reads ALL G slots of its round in one
// batch and adds them up itself: the counts of the workgroups before it are where its rows start inside the round, their total
// advances its own carry.  The tiles themselves move as in stencil_stage_write_kernel, the column vectors requested one tile ahead.
// K: a round costs one store -> load round trip between all workgroups whatever it moves; with one tile per round (37 KB per
// workgroup) that cadence, not the memory, set the pace (2.6 ms per 1e9 int64 rows at 10 % kept against 2.2 for the two passes).
// state: 4 x G slot words | [4 G]: the number of kept rows (written by the workgroup of the last tile) | [4 G + 1]: the bail-out flag (a
// poll that lasts a quarter of a second -- the workgroups are not all resident -- sets it, everybody leaves, the host takes the two passes).
template <int WIDTH, int K>
__global__ __launch_bounds__(FL_THREADS) void stencil_rounds_kernel(const int8_t *__restrict__ stencil, const uint8_t *__restrict__ valid, int64_t n,
                                                                    uint32_t ntiles, const void *__restrict__ in, void *__restrict__ out,
                                                                    unsigned long long *__restrict__ state) {
  using T = typename std::conditional<WIDTH == 1, uint8_t, typename std::conditional<WIDTH == 2, uint16_t,
            typename std::conditional<WIDTH == 4, uint32_t, uint64_t>::type>::type>::type;
  constexpr int EPV = 16 / WIDTH;
  constexpr int VROUNDS = FLS_ROWS / (FL_THREADS * EPV);
  constexpr int NWAVES = FL_THREADS / WAVE;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  union Vec { u32x4 q; T e[EPV]; };
  __shared__ unsigned int wsum[NWAVES];
  __shared__ unsigned long long s_before[NWAVES], s_total[NWAVES];
  __shared__ int s_ok;
  __shared__ uint32_t s_keep[FL_THREADS], s_pre[FL_THREADS];
  __shared__ __attribute__((aligned(16))) T stage[FLS_ROWS];
  const uint32_t G = gridDim.x;
  const int wave = threadIdx.x / WAVE, lane = lane_id();
  unsigned long long *bail = state + (size_t)4 * G + 1;
  const T *src = reinterpret_cast<const T *>(in);
  T *dst = reinterpret_cast<T *>(out);
  const uint32_t nsuper = (ntiles + K - 1) / K;
  if (threadIdx.x == 0) s_ok = __hip_atomic_load(bail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull ? 2 : 1;      // (GDF_FL_FORCE_BAIL)
  block_sync();
  if (s_ok == 2) return;
  // the stencil bytes of the 16 rows this thread owns in tile t, as they come from memory (whole groups) or as keep bits (the table's
  // end; nothing for a tile beyond it)
  auto stencil_request = [&](uint64_t t, uint4 &raw, uint32_t &tail_keep) {
    const int64_t i = (int64_t)t * FLS_ROWS + (int64_t)threadIdx.x * 16;
    tail_keep = 0;
    raw = make_uint4(0, 0, 0, 0);
    if (i + 16 <= n) raw = *reinterpret_cast<const uint4 *>(stencil + i);
    else
      for (int r = 0; r < 16; ++r)
        if (i + r < n && stencil[i + r] != 0 && (valid ? bit_is_set(valid, i + r) : true)) tail_keep |= 1u << r;
  };
  auto keep_bits = [&](uint64_t t, const uint4 &raw, uint32_t tail_keep) -> uint32_t {
    const int64_t i = (int64_t)t * FLS_ROWS + (int64_t)threadIdx.x * 16;
    if (i + 16 > n) return tail_keep;
    const uint32_t words[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t keep = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int b = 0; b < 4; ++b) keep |= ((words[q] >> (8 * b)) & 0xffu) ? (1u << (4 * q + b)) : 0u;
    if (valid) keep &= (uint32_t)valid[i >> 3] | ((uint32_t)valid[(i >> 3) + 1] << 8);
    return keep;
  };
  // a tile's keep bits -> the prefix of this thread's 16-row group inside the tile, and the tile's total
  auto tile_scan = [&](uint32_t keep, uint32_t &pre, uint32_t &total) {
    const unsigned int mine = (unsigned)__popc(keep);
    const unsigned int incl = wave_scan_incl(mine);
    block_sync();                                  // wsum's previous readers are done
    if (lane == WAVE - 1) wsum[wave] = incl;
    block_sync();
    unsigned int before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NWAVES; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    pre = before + incl - mine;
  };
  auto publish = [&](uint32_t r, uint32_t count) {
    if (threadIdx.x == 0)
      __hip_atomic_store(state + (size_t)(r & 3u) * G + blockIdx.x, ((unsigned long long)(r + 1u) << 32) | (unsigned long long)count, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
  };
  // the column's vectors of a whole tile (a ragged last tile is read element by element when it is staged)
  auto column_request = [&](uint64_t t, Vec (&vv)[VROUNDS]) {
    const int64_t tile0 = (int64_t)t * FLS_ROWS;
    if (tile0 + FLS_ROWS <= n) {
      const u32x4 *vsrc = reinterpret_cast<const u32x4 *>(src + tile0);
#pragma unroll
      for (int k = 0; k < VROUNDS; ++k) vv[k].q = __builtin_nontemporal_load(vsrc + k * FL_THREADS + threadIdx.x);
    }
  };
  unsigned long long carry = 0;
  uint64_t u = blockIdx.x;                          // this workgroup's super-tile
  if (u >= nsuper) return;
  // Pipeline: at step r the stencil bytes of super-tile r + 2 leave, super-tile r + 1's count is PUBLISHED (its stencil bytes left a
  // step ago), and only then round r is polled -- its counts went out a whole step earlier -- and its tiles staged and stored.
  uint4 raw[K], raw1[K];
  uint32_t tail[K], tail1[K], keepC[K], preC[K], totalC[K], keepN[K], preN[K], totalN[K];
  Vec v[VROUNDS], vn[VROUNDS];
#pragma unroll
  for (int j = 0; j < K; ++j) stencil_request(u * K + j, raw[j], tail[j]);
  column_request(u * K, v);
#pragma unroll
  for (int j = 0; j < K; ++j) { raw1[j] = make_uint4(0, 0, 0, 0); tail1[j] = 0; keepN[j] = preN[j] = totalN[j] = 0; }
  if (u + G < nsuper) {
#pragma unroll
    for (int j = 0; j < K; ++j) stencil_request((u + G) * K + j, raw1[j], tail1[j]);
  }
  {
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) { keepC[j] = keep_bits(u * K + j, raw[j], tail[j]); tile_scan(keepC[j], preC[j], totalC[j]); sum += totalC[j]; }
    publish(0u, sum);
  }
  for (uint32_t r = 0;; ++r) {
    const uint64_t un = u + G, unn = un + G;
    const bool more = un < nsuper, more2 = unn < nsuper;
    uint4 raw2[K];
    uint32_t tail2[K];
#pragma unroll
    for (int j = 0; j < K; ++j) { raw2[j] = make_uint4(0, 0, 0, 0); tail2[j] = 0; }
    if (more2) {
#pragma unroll
      for (int j = 0; j < K; ++j) stencil_request(unn * K + j, raw2[j], tail2[j]);
    }
    if (more) {
      uint32_t sum = 0;
#pragma unroll
      for (int j = 0; j < K; ++j) { keepN[j] = keep_bits(un * K + j, raw1[j], tail1[j]); tile_scan(keepN[j], preN[j], totalN[j]); sum += totalN[j]; }
      publish(r + 1u, sum);
    }
    // ---- where this super-tile's rows start: carry + the counts of the workgroups before this one in round r ----
    const uint64_t left = (uint64_t)nsuper - (uint64_t)r * G;
    const uint32_t pubs = left < G ? (uint32_t)left : G;
    const unsigned long long *slots = state + (size_t)(r & 3u) * G;
    unsigned long long before_r = 0, total_r = 0, waiting_since = 0;
    for (uint32_t spins = 0;; ++spins) {
      constexpr int PT = 4;                        // G <= PT * FL_THREADS (the host's grid)
      unsigned long long w[PT];
#pragma unroll
      for (int k = 0; k < PT; ++k) {
        const uint32_t b = threadIdx.x + (uint32_t)k * FL_THREADS;
        w[k] = b < pubs ? __hip_atomic_load(slots + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0ull;
      }
      bool ok = true;
      before_r = 0;
      total_r = 0;
#pragma unroll
      for (int k = 0; k < PT; ++k) {
        const uint32_t b = threadIdx.x + (uint32_t)k * FL_THREADS;
        if (b < pubs) {
          ok = ok && (uint32_t)(w[k] >> 32) == r + 1u;
          total_r += (uint32_t)w[k];
          if (b < blockIdx.x) before_r += (uint32_t)w[k];
        }
      }
      block_sync();
      if (threadIdx.x == 0) s_ok = 1;
      block_sync();
      if (!ok) s_ok = 0;
      block_sync();
      if (s_ok) break;
      if (threadIdx.x == 0) {
        const unsigned long long now = wall_clock64();      // 100 MHz
        if (spins == 0) waiting_since = now;
        if (now - waiting_since > 25000000ull || __hip_atomic_load(bail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull) {
          __hip_atomic_store(bail, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          s_ok = 2;
        }
      }
      block_sync();
      if (s_ok == 2) return;
      __builtin_amdgcn_s_sleep(1);
    }
    before_r = wave_reduce_add(before_r);
    total_r = wave_reduce_add(total_r);
    if (lane == 0) { s_before[wave] = before_r; s_total[wave] = total_r; }
    block_sync();
    unsigned long long bsum = 0, tsum = 0;
#pragma unroll
    for (int w2 = 0; w2 < NWAVES; ++w2) { bsum += s_before[w2]; tsum += s_total[w2]; }
    unsigned long long base = carry + bsum;
    carry += tsum;
    // ---- the tiles: kept elements drop into the stage at their rank, the stage leaves as one contiguous run ----
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const uint64_t t = u * K + j;
      if (t >= ntiles) break;                      // (workgroup-uniform: the table's last super-tile)
      const int64_t tile = (int64_t)t * FLS_ROWS;
      const bool whole = tile + FLS_ROWS <= n;
      // the next tile's column vectors leave now: the next one of this super-tile, or the first one of this workgroup's next
      if (j + 1 < K) { if (t + 1 < ntiles) column_request(t + 1, vn); }
      else if (more) column_request(un * K, vn);
      s_keep[threadIdx.x] = keepC[j];
      s_pre[threadIdx.x] = preC[j];
      block_sync();
#pragma unroll
      for (int k = 0; k < VROUNDS; ++k) {
        const uint32_t row0 = (uint32_t)(k * FL_THREADS + threadIdx.x) * EPV;
        const uint32_t kb = s_keep[row0 >> 4], p0 = s_pre[row0 >> 4];
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          const uint32_t bit = (row0 + e) & 15u;
          if ((kb >> bit) & 1u) {
            T x;
            if (whole) x = v[k].e[e];
            else x = src[tile + row0 + e];                 // (kept rows lie below n)
            stage[p0 + __popc(kb & ((1u << bit) - 1u))] = x;
          }
        }
      }
      block_sync();
      for (uint32_t q = threadIdx.x; q < totalC[j]; q += FL_THREADS) dst[base + q] = stage[q];
      base += totalC[j];
      if (t == (uint64_t)ntiles - 1 && threadIdx.x == 0) state[(size_t)4 * G] = base;       // the number of kept rows
      block_sync();                                // this tile's reads of the stage, s_keep and s_pre are done
#pragma unroll
      for (int k = 0; k < VROUNDS; ++k) v[k] = vn[k];
    }
    if (!more) break;
    u = un;
#pragma unroll
    for (int j = 0; j < K; ++j) { keepC[j] = keepN[j]; preC[j] = preN[j]; totalC[j] = totalN[j]; raw1[j] = raw2[j]; tail1[j] = tail2[j]; }
  }
}

// WIDTH == 0: emit the row index as size_t (gdf_filter); else move WIDTH-byte elements
template <class Pred, int WIDTH>
__global__ __launch_bounds__(FL_THREADS) void compact_write_kernel(Pred pred, int64_t n, int64_t chunk, const uint64_t *chunk_base,
                                                                   const void *in, void *out) {
  __shared__ unsigned int wcount[FL_THREADS / WAVE];
  const int64_t begin = (int64_t)blockIdx.x * chunk;
  const int64_t end = begin + chunk < n ? begin + chunk : n;
  uint64_t base = chunk_base[blockIdx.x];
  const int wave = threadIdx.x / WAVE;
  for (int64_t tile = begin; tile < end; tile += FL_THREADS) {
    const int64_t i = tile + threadIdx.x;
    const bool keep = i < end && pred(i);
    const unsigned long long m = __ballot(keep);
    if (lane_id() == 0) wcount[wave] = (unsigned)__popcll(m);
    block_sync();
    unsigned int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < FL_THREADS / WAVE; ++w) {
      if (w < wave) before += wcount[w];
      total += wcount[w];
    }
    if (keep) {
      const uint64_t pos = base + before + mask_rank(m);
      if (WIDTH == 0) ((size_t *)out)[pos] = (size_t)i;
      else if (WIDTH == 1) ((uint8_t *)out)[pos] = ((const uint8_t *)in)[i];
      else if (WIDTH == 2) ((uint16_t *)out)[pos] = ((const uint16_t *)in)[i];
      else if (WIDTH == 4) ((uint32_t *)out)[pos] = ((const uint32_t *)in)[i];
      else ((uint64_t *)out)[pos] = ((const uint64_t *)in)[i];
    }
    base += total;
    block_sync();
  }
}

__global__ __launch_bounds__(FL_THREADS) void mask_prefix_ones_kernel(uint8_t *mask, int64_t nbytes, int64_t ones) {
  // first `ones` bits set, the rest clear
  for (int64_t i = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; i < nbytes; i += (int64_t)gridDim.x * FL_THREADS) {
    const int64_t lo = i * 8;
    uint8_t v = 0;
    if (lo + 8 <= ones) v = 0xff;
    else if (lo < ones) v = (uint8_t)((1u << (ones - lo)) - 1);
    mask[i] = v;
  }
}

template <class Pred>
static gdf_error compact(Pred pred, int64_t n, int width, const void *in, void *out, uint64_t *kept) {
  *kept = 0;
  if (n == 0) return GDF_SUCCESS;
  if constexpr (std::is_same<Pred, StencilPred>::value) {
    // ONE pass in lockstep rounds (stencil_rounds_kernel): from 2^22 rows on, 16-byte-aligned stencil and column, out != in (a bail-out
    // leaves `out` partly written and starts over below).  GDF_FL_NO_ROUNDS: the two passes; GDF_FL_FORCE_BAIL: the flag set before the launch
    const uint64_t ntiles = ((uint64_t)n + FLS_ROWS - 1) / FLS_ROWS;
    // 8-byte elements only (GDF_FL_ROUNDS_ANY_WIDTH: whatever the width -- the parity tests): the narrower the element, the fewer bytes a
    // round moves for its one store -> load round trip between all workgroups.  1e9 rows, rounds against two passes, 10 % / 50 % kept:
    // int8 1.36 / 1.52 against 0.99 / 1.08 ms, int16 1.06 / 1.18 against 1.02 / 1.13, int32 1.51 / 1.68 against 1.39 / 1.74, int64 2.15 /
    // 2.46 against 2.28 / 2.97 (profiles/r6_r_compact_rounds.txt)
    const bool wide_enough = width == 8 || (width != 0 && lab::path_on("GDF_FL_ROUNDS_ANY_WIDTH"));
    if (n >= FL_ROUNDS_MIN && ((uintptr_t)pred.stencil & 15) == 0 && ((uintptr_t)in & 15) == 0 && wide_enough && in != out && ntiles < 0x7fffffffULL &&
        !lab::path_on("GDF_FL_NO_ROUNDS")) {
      auto rounds = [&](auto kernel) -> gdf_error {
        int fit = 1;
        HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, (const void *)kernel, FL_THREADS, 0));
        size_t grid = (size_t)device_cu_count() * (size_t)std::max(1, std::min(fit, 4));
        if (grid > (size_t)4 * FL_THREADS) grid = (size_t)4 * FL_THREADS;       // (the slots one poll covers)
        if (grid > ntiles) grid = (size_t)ntiles;        // (a grid beyond the super-tiles: the spare workgroups leave at once)
        DevBuf st;
        const size_t words = 4 * grid + 2;
        RMM_TRY(st.alloc(sizeof(unsigned long long) * words));
        HIP_TRY(hipMemsetAsync(st.p, 0, sizeof(unsigned long long) * words, stream0()));
        if (lab::path_on("GDF_FL_FORCE_BAIL")) {
          const unsigned long long one = 1;
          HIP_TRY(hipMemcpyAsync(st.as<unsigned long long>() + 4 * grid + 1, &one, sizeof(one), hipMemcpyHostToDevice, stream0()));
          HIP_TRY(hipStreamSynchronize(stream0()));
        }
        GDF_LAUNCH("compact_rounds", kernel, dim3((unsigned)grid), dim3(FL_THREADS), 0, stream0(), pred.stencil, pred.valid, n, (uint32_t)ntiles, in, out,
                   st.as<unsigned long long>());
        HIP_CHECK_LAST();
        unsigned long long tail[2] = {0, 0};           // kept rows | bail-out flag
        HIP_TRY(read_back(tail, st.as<unsigned long long>() + 4 * grid, sizeof(tail)));
        if (tail[1]) return GDF_UNSUPPORTED_METHOD;
        *kept = tail[0];
        return GDF_SUCCESS;
      };
      gdf_error e;
      switch (width) {                                   // four tiles per workgroup and round (stencil_rounds_kernel)
        case 1: e = rounds(stencil_rounds_kernel<1, 4>); break;
        case 2: e = rounds(stencil_rounds_kernel<2, 4>); break;
        case 4: e = rounds(stencil_rounds_kernel<4, 4>); break;
        default: e = rounds(stencil_rounds_kernel<8, 4>); break;
      }
      if (e != GDF_UNSUPPORTED_METHOD) return e;
      *kept = 0;
    }
  }
  int64_t chunk = (n + FL_MAX_CHUNKS - 1) / FL_MAX_CHUNKS;
  chunk = ((chunk + FLS_ROWS - 1) / FLS_ROWS) * FLS_ROWS;          // whole tiles of the staged write kernel (a multiple of FL_THREADS and of 16)
  const int nchunks = (int)((n + chunk - 1) / chunk);
  DevBuf counts;
  RMM_TRY(counts.alloc(sizeof(uint64_t) * (nchunks + 1)));
  HIP_TRY(hipMemsetAsync(counts.p, 0, sizeof(uint64_t) * (nchunks + 1), stream0()));
  if constexpr (std::is_same<Pred, StencilPred>::value) {
    if (((uintptr_t)pred.stencil & 15) == 0 && chunk % 16 == 0)
      GDF_LAUNCH("compact_count", stencil_count_kernel, dim3(nchunks), dim3(FL_THREADS), 0, stream0(), pred.stencil, pred.valid, n, chunk, counts.as<uint64_t>());
    else
      GDF_LAUNCH("compact_count", compact_count_kernel<Pred>, dim3(nchunks), dim3(FL_THREADS), 0, stream0(), pred, n, chunk, counts.as<uint64_t>());
  } else {
    GDF_LAUNCH("compact_count", compact_count_kernel<Pred>, dim3(nchunks), dim3(FL_THREADS), 0, stream0(), pred, n, chunk, counts.as<uint64_t>());
  }
  HIP_CHECK_LAST();
  GDF_TRY(scan_u64(counts.as<uint64_t>(), counts.as<uint64_t>(), (size_t)nchunks + 1, false));
  const dim3 g(nchunks), b(FL_THREADS);
  if constexpr (std::is_same<Pred, StencilPred>::value) {
    // thread-consecutive rows win while few rows survive (10 % kept: 0.19 vs 0.33 ms per 1e8 rows); at 50 % the
    // ballot kernel below is ahead again (0.39 vs 0.42 ms), so the number of keepers -- known after the scan -- decides
    HIP_TRY(read_back(kept, counts.as<uint64_t>() + nchunks, sizeof(uint64_t)));
    if (((uintptr_t)pred.stencil & 15) == 0 && ((uintptr_t)in & 15) == 0 && chunk % FLS_ROWS == 0 && width != 0) {
      switch (width) {
        case 1: GDF_LAUNCH("compact_write", stencil_stage_write_kernel<1>, g, b, 0, stream0(), pred.stencil, pred.valid, n, chunk, counts.as<uint64_t>(), in, out); break;
        case 2: GDF_LAUNCH("compact_write", stencil_stage_write_kernel<2>, g, b, 0, stream0(), pred.stencil, pred.valid, n, chunk, counts.as<uint64_t>(), in, out); break;
        case 4: GDF_LAUNCH("compact_write", stencil_stage_write_kernel<4>, g, b, 0, stream0(), pred.stencil, pred.valid, n, chunk, counts.as<uint64_t>(), in, out); break;
        default: GDF_LAUNCH("compact_write", stencil_stage_write_kernel<8>, g, b, 0, stream0(), pred.stencil, pred.valid, n, chunk, counts.as<uint64_t>(), in, out); break;
      }
      HIP_CHECK_LAST();
      HIP_TRY(hipStreamSynchronize(stream0()));        // (the keeper count was read above; the counts go out of scope)
      return GDF_SUCCESS;
    }
    if (((uintptr_t)pred.stencil & 15) == 0 && chunk % 16 == 0 && width != 0 && *kept * 3 < (uint64_t)n) {
      switch (width) {
        case 1: GDF_LAUNCH("compact_write", stencil_write_kernel<1>, g, b, 0, stream0(), pred.stencil, pred.valid, n, chunk, counts.as<uint64_t>(), in, out); break;
        case 2: GDF_LAUNCH("compact_write", stencil_write_kernel<2>, g, b, 0, stream0(), pred.stencil, pred.valid, n, chunk, counts.as<uint64_t>(), in, out); break;
        case 4: GDF_LAUNCH("compact_write", stencil_write_kernel<4>, g, b, 0, stream0(), pred.stencil, pred.valid, n, chunk, counts.as<uint64_t>(), in, out); break;
        default: GDF_LAUNCH("compact_write", stencil_write_kernel<8>, g, b, 0, stream0(), pred.stencil, pred.valid, n, chunk, counts.as<uint64_t>(), in, out); break;
      }
      HIP_CHECK_LAST();
      HIP_TRY(read_back(kept, counts.as<uint64_t>() + nchunks, sizeof(uint64_t)));
      return GDF_SUCCESS;
    }
  }
  switch (width) {
    case 0: GDF_LAUNCH("compact_write", (compact_write_kernel<Pred, 0>), g, b, 0, stream0(), pred, n, chunk, counts.as<uint64_t>(), in, out); break;
    case 1: GDF_LAUNCH("compact_write", (compact_write_kernel<Pred, 1>), g, b, 0, stream0(), pred, n, chunk, counts.as<uint64_t>(), in, out); break;
    case 2: GDF_LAUNCH("compact_write", (compact_write_kernel<Pred, 2>), g, b, 0, stream0(), pred, n, chunk, counts.as<uint64_t>(), in, out); break;
    case 4: GDF_LAUNCH("compact_write", (compact_write_kernel<Pred, 4>), g, b, 0, stream0(), pred, n, chunk, counts.as<uint64_t>(), in, out); break;
    default: GDF_LAUNCH("compact_write", (compact_write_kernel<Pred, 8>), g, b, 0, stream0(), pred, n, chunk, counts.as<uint64_t>(), in, out); break;
  }
  HIP_CHECK_LAST();
  HIP_TRY(read_back(kept, counts.as<uint64_t>() + nchunks, sizeof(uint64_t)));
  return GDF_SUCCESS;
}

// ---------------------------------------------------------------------------
// mask concatenation (validops.cu:203-256): one output byte per thread
// ---------------------------------------------------------------------------
struct ConcatSrc { const uint8_t *mask; int64_t start, len; };

__global__ __launch_bounds__(FL_THREADS) void mask_concat_kernel(const ConcatSrc *src, int nsrc, uint8_t *out, int64_t total) {
  const int64_t nbytes = (total + 7) / 8;
  for (int64_t b = (int64_t)blockIdx.x * FL_THREADS + threadIdx.x; b < nbytes; b += (int64_t)gridDim.x * FL_THREADS) {
    uint8_t v = 0;
    // binary search the source that holds bit b*8
    int lo = 0, hi = nsrc - 1;
    const int64_t first = b * 8;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (src[mid].start <= first) lo = mid; else hi = mid - 1; }
    int s = lo;
    for (int bit = 0; bit < 8; ++bit) {
      const int64_t idx = first + bit;
      if (idx >= total) break;
      while (s < nsrc - 1 && idx >= src[s].start + src[s].len) ++s;
      const int64_t local = idx - src[s].start;
      const bool valid = src[s].mask ? bit_is_set(src[s].mask, local) : true;
      if (valid) v |= (uint8_t)(1u << bit);
    }
    out[b] = v;
  }
}

}  // namespace gdf_amd

using namespace gdf_amd;

extern "C" {

gdf_error gpu_comparison_static_i8(gdf_column *lhs, int8_t value, gdf_column *output, gdf_comparison_operator operation) {
  return gdf_amd::guarded([&]() -> gdf_error {
  return comparison_static<int8_t>(lhs, value, output, operation);
  });
}
gdf_error gpu_comparison_static_i16(gdf_column *lhs, int16_t value, gdf_column *output, gdf_comparison_operator operation) {
  return gdf_amd::guarded([&]() -> gdf_error {
  return comparison_static<int16_t>(lhs, value, output, operation);
  });
}
gdf_error gpu_comparison_static_i32(gdf_column *lhs, int32_t value, gdf_column *output, gdf_comparison_operator operation) {
  return gdf_amd::guarded([&]() -> gdf_error {
  return comparison_static<int32_t>(lhs, value, output, operation);
  });
}
gdf_error gpu_comparison_static_i64(gdf_column *lhs, int64_t value, gdf_column *output, gdf_comparison_operator operation) {
  return gdf_amd::guarded([&]() -> gdf_error {
  return comparison_static<int64_t>(lhs, value, output, operation);
  });
}
gdf_error gpu_comparison_static_f32(gdf_column *lhs, float value, gdf_column *output, gdf_comparison_operator operation) {
  return gdf_amd::guarded([&]() -> gdf_error {
  return comparison_static<float>(lhs, value, output, operation);
  });
}
gdf_error gpu_comparison_static_f64(gdf_column *lhs, double value, gdf_column *output, gdf_comparison_operator operation) {
  return gdf_amd::guarded([&]() -> gdf_error {
  return comparison_static<double>(lhs, value, output, operation);
  });
}

gdf_error gpu_comparison(gdf_column *lhs, gdf_column *rhs, gdf_column *output, gdf_comparison_operator operation) {
  return gdf_amd::guarded([&]() -> gdf_error {
  GDF_REQUIRE(lhs && rhs && output, GDF_DATASET_EMPTY);
  GDF_REQUIRE(lhs->size == rhs->size, GDF_COLUMN_SIZE_MISMATCH);
  GDF_REQUIRE(lhs->size == output->size, GDF_COLUMN_SIZE_MISMATCH);
  GDF_REQUIRE(output->dtype == GDF_INT8, GDF_COLUMN_SIZE_MISMATCH);   // sic: filterops.cu:262
  const ElemKind lk = (lhs->dtype >= GDF_INT8 && lhs->dtype <= GDF_FLOAT64) ? elem_kind(lhs->dtype) : K_BAD;
  const ElemKind rk = (rhs->dtype >= GDF_INT8 && rhs->dtype <= GDF_FLOAT64) ? elem_kind(rhs->dtype) : K_BAD;
  if (lk == K_BAD || rk == K_BAD) return GDF_SUCCESS;   // the reference's if-chain falls through silently
  const int64_t n = (int64_t)lhs->size;
  const int op = (int)operation;
  gdf_error e = GDF_SUCCESS;
  switch (rk) {
    case K_I8: e = dispatch_left<int8_t, false>(lk, lhs->data, rhs->data, 0, output->data, n, op); break;
    case K_I16: e = dispatch_left<int16_t, false>(lk, lhs->data, rhs->data, 0, output->data, n, op); break;
    case K_I32: e = dispatch_left<int32_t, false>(lk, lhs->data, rhs->data, 0, output->data, n, op); break;
    case K_I64: e = dispatch_left<int64_t, false>(lk, lhs->data, rhs->data, 0, output->data, n, op); break;
    case K_F32: e = dispatch_left<float, false>(lk, lhs->data, rhs->data, 0, output->data, n, op); break;
    default: e = dispatch_left<double, false>(lk, lhs->data, rhs->data, 0, output->data, n, op); break;
  }
  GDF_TRY(e);
  HIP_CHECK_LAST();
  return comparison_mask(output, lhs->valid, rhs->valid, lhs->null_count, rhs->null_count, n);
  });
}

gdf_error gpu_apply_stencil(gdf_column *lhs, gdf_column *stencil, gdf_column *output) {
  return gdf_amd::guarded([&]() -> gdf_error {
  GDF_REQUIRE(lhs && stencil && output, GDF_DATASET_EMPTY);
  GDF_REQUIRE(output->size == lhs->size, GDF_COLUMN_SIZE_MISMATCH);
  GDF_REQUIRE(lhs->dtype == output->dtype, GDF_DTYPE_MISMATCH);
  GDF_REQUIRE(!lhs->valid, GDF_VALIDITY_UNSUPPORTED);
  GDF_REQUIRE(stencil->size == lhs->size, GDF_COLUMN_SIZE_MISMATCH);
  const int width = dtype_width(lhs->dtype);
  GDF_REQUIRE(width > 0, GDF_UNSUPPORTED_DTYPE);
  const int64_t n = (int64_t)lhs->size;
  StencilPred pred{(const int8_t *)stencil->data, stencil->valid};
  uint64_t kept = 0;
  GDF_TRY(compact(pred, n, width, lhs->data, output->data, &kept));
  // every kept element had a valid stencil bit, so the compacted mask is `kept` ones
  if (output->valid && n) {
    const int64_t nbytes = (int64_t)mask_bytes((size_t)n);
    hipLaunchKernelGGL(mask_prefix_ones_kernel, dim3(stream_grid((size_t)nbytes, FL_THREADS * 16)), dim3(FL_THREADS), 0, stream0(),
                       output->valid, nbytes, (int64_t)kept);
    HIP_CHECK_LAST();
  }
  HIP_TRY(hipStreamSynchronize(stream0()));
  output->size = (gdf_size_type)kept;   // the allocation is NOT shrunk (streamcompactionops.cu:248)
  output->null_count = 0;
  return GDF_SUCCESS;
  });
}

gdf_error gdf_filter(size_t nrows, gdf_column *cols, size_t ncols, void **d_cols, int *d_types, void **d_vals,
                     size_t *d_indx, size_t *new_sz) {
  return gdf_amd::guarded([&]() -> gdf_error {
  GDF_REQUIRE(cols && d_cols && d_types && d_vals && d_indx && new_sz, GDF_DATASET_EMPTY);
  GDF_REQUIRE(!cols->valid, GDF_VALIDITY_UNSUPPORTED);   // sqls_ops.cu:1412 checks the first column only
  // fill the caller's device-side column/type slices (soa_col_info, sqls_ops.cu:27-41)
  std::vector<void *> h_cols(ncols);
  std::vector<int> h_types(ncols);
  for (size_t i = 0; i < ncols; ++i) { h_cols[i] = cols[i].data; h_types[i] = (int)cols[i].dtype; }
  HIP_TRY(hipMemcpy(d_cols, h_cols.data(), ncols * sizeof(void *), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_types, h_types.data(), ncols * sizeof(int), hipMemcpyHostToDevice));
  RowEqualsPred pred{(int)ncols, d_cols, d_types, d_vals};
  uint64_t kept = 0;
  GDF_TRY(compact(pred, (int64_t)nrows, 0, nullptr, d_indx, &kept));
  HIP_TRY(hipStreamSynchronize(stream0()));
  *new_sz = (size_t)kept;
  return GDF_SUCCESS;
  });
}

gdf_error gdf_count_nonzero_mask(gdf_valid_type const *masks, int num_rows, int *count) {
  return gdf_amd::guarded([&]() -> gdf_error {
  if (nullptr == masks || nullptr == count) return GDF_DATASET_EMPTY;   // validops.cu:148
  if (0 == num_rows) return GDF_SUCCESS;
  DevBuf c;
  RMM_TRY(c.alloc(sizeof(unsigned long long)));
  HIP_TRY(hipMemsetAsync(c.p, 0, sizeof(unsigned long long), stream0()));
  hipLaunchKernelGGL(mask_popcount_kernel, dim3(stream_grid((size_t)(num_rows + 7) / 8, FL_THREADS * 16)), dim3(FL_THREADS), 0,
                     stream0(), masks, (int64_t)num_rows, c.as<unsigned long long>());
  HIP_CHECK_LAST();
  unsigned long long h = 0;
  HIP_TRY(read_back(&h, c.p, sizeof(h)));
  *count = (int)h;
  return GDF_SUCCESS;
  });
}

// out.valid = lhs.valid & rhs.valid (a missing mask counts as all ones); sizes must agree
gdf_error gdf_validity_and(gdf_column *lhs, gdf_column *rhs, gdf_column *output) {
  return gdf_amd::guarded([&]() -> gdf_error {
  GDF_REQUIRE(lhs && rhs && output, GDF_DATASET_EMPTY);
  GDF_REQUIRE(lhs->size == rhs->size && lhs->size == output->size, GDF_COLUMN_SIZE_MISMATCH);
  GDF_REQUIRE(output->valid, GDF_VALIDITY_MISSING);
  gdf_size_type nulls = 0;
  GDF_TRY(mask_and(lhs->valid, rhs->valid, output->valid, (int64_t)lhs->size, &nulls));
  output->null_count = nulls;
  return GDF_SUCCESS;
  });
}

gdf_error gdf_column_concat(gdf_column *output, gdf_column *columns_to_concat[], int num_columns) {
  return gdf_amd::guarded([&]() -> gdf_error {
  // checks in the order of column.cpp:56-98
  if (nullptr == columns_to_concat) return GDF_DATASET_EMPTY;
  if (nullptr == columns_to_concat[0] || nullptr == output) return GDF_DATASET_EMPTY;
  const gdf_dtype type = columns_to_concat[0]->dtype;
  if (type != output->dtype) return GDF_DTYPE_MISMATCH;
  gdf_size_type total = 0;
  bool any_mask = false;
  for (int i = 0; i < num_columns; ++i) {
    gdf_column *c = columns_to_concat[i];
    if (nullptr == c) return GDF_DATASET_EMPTY;
    if (c->size > 0 && nullptr == c->data) return GDF_DATASET_EMPTY;
    if (type != c->dtype) return GDF_DTYPE_MISMATCH;
    total += c->size;
    any_mask |= c->valid != nullptr;
  }
  if (output->size != total) return GDF_COLUMN_SIZE_MISMATCH;
  int width = 0;
  GDF_TRY(get_column_byte_width(output, &width));
  output->null_count = 0;
  char *dst = (char *)output->data;
  std::vector<ConcatSrc> src(num_columns);
  int64_t start = 0;
  for (int i = 0; i < num_columns; ++i) {
    gdf_column *c = columns_to_concat[i];
    const size_t bytes = (size_t)width * c->size;
    if (bytes) HIP_TRY(hipMemcpyAsync(dst, c->data, bytes, hipMemcpyDeviceToDevice, stream0()));
    dst += bytes;
    output->null_count += c->null_count;
    src[i] = ConcatSrc{c->valid, start, (int64_t)c->size};
    start += (int64_t)c->size;
  }
  if (any_mask && output->valid && total) {
    DevBuf d_src;
    RMM_TRY(d_src.alloc(sizeof(ConcatSrc) * num_columns));
    HIP_TRY(hipMemcpyAsync(d_src.p, src.data(), sizeof(ConcatSrc) * num_columns, hipMemcpyHostToDevice, stream0()));
    hipLaunchKernelGGL(mask_concat_kernel, dim3(stream_grid(mask_bytes(total), FL_THREADS * 4)), dim3(FL_THREADS), 0, stream0(),
                       d_src.as<ConcatSrc>(), num_columns, output->valid, (int64_t)total);
    HIP_CHECK_LAST();
    HIP_TRY(hipStreamSynchronize(stream0()));
  } else if (output->valid) {
    HIP_TRY(hipMemsetAsync(output->valid, 0xff, mask_bytes(total), stream0()));
  }
  HIP_TRY(hipStreamSynchronize(stream0()));
  return GDF_SUCCESS;
  });
}

// streamcompactionops.cu:389-494: output = lhs ++ rhs, data and validity.  The reference stitches the two masks
// together byte by byte on the host side of thrust with MSB-first helpers; here it is gdf_column_concat's bit-exact
// LSB-first mask concatenation (the layout of every other mask in libgdf).  The reference
// returns GDF_VALIDITY_MISSING for a dtype mismatch (sic, :391) and so does this.
gdf_error gpu_concat(gdf_column *lhs, gdf_column *rhs, gdf_column *output) {
  return gdf_amd::guarded([&]() -> gdf_error {
  GDF_REQUIRE(lhs && rhs && output, GDF_DATASET_EMPTY);
  GDF_REQUIRE(lhs->dtype == output->dtype && rhs->dtype == output->dtype, GDF_VALIDITY_MISSING);
  GDF_REQUIRE(output->size == lhs->size + rhs->size, GDF_COLUMN_SIZE_MISMATCH);
  gdf_column *both[2] = {lhs, rhs};
  return gdf_column_concat(output, both, 2);
  });
}

}  // extern "C"
