// elementwise.hip -- the element-wise operators: binary arithmetic, comparisons and bit operations (reference
// src/binaryops.cu), math functions and casts (src/unaryops.cu) and datetime field extraction (src/datetimeops.cu); 182 entry
// points, prototypes in include/gdf/gdf_elementwise.def, semantics in include/gdf/gdf.h and DESIGN.md §12.
//
// Two kernel shapes, ew_unary<In, Out, F> and ew_binary<T, Out, F>, instantiated from the tables at the end of this file.  A
// lane owns a RUN of R consecutive rows, R = 16 / (width of the narrowest column involved), so that the narrowest column is
// read or written with ONE 16-byte access per run and every wider column with R * width / 16 of them; the output is always
// stored in whole 16-byte vectors.  The host picks `head` (< 16 rows) so that the output is 16-byte aligned at row `head` and
// as many inputs as possible are too; an input that is not co-aligned with the output is read element by element (the stores
// stay wide).  Rows [0, head) and the rows behind the last whole run are handled one per thread in the same launch.
//
// Validity masks are NOT read by the kernels: a null row's output is unspecified (the reference leaves it unwritten) and a
// 16-byte store covers it anyway, so the bits could only select between two permitted results.  The casts and the datetime
// operators copy the input mask to the output mask with one asynchronous device-to-device copy queued behind the launch.
#include "internal.h"

#include <cmath>

namespace gdf_amd {

typedef uint32_t ew_u32x4 __attribute__((ext_vector_type(4)));

constexpr int EW_THREADS = 256;

template <class A, class B> constexpr int ew_min_width() { return (int)(sizeof(A) < sizeof(B) ? sizeof(A) : sizeof(B)); }
template <class A, class B> constexpr int ew_max_width() { return (int)(sizeof(A) > sizeof(B) ? sizeof(A) : sizeof(B)); }
// runs per lane and trip: four 16-byte vectors of the widest column in flight per lane when a run is one vector, fewer when
// a run is several (a run of 16 int64 rows is already eight)
constexpr int ew_unroll(int rows, int max_width) {
  const int vecs = rows * max_width / 16;
  return vecs >= 4 ? 1 : 4 / vecs;
}

template <class T, int R>
union EwRun {
  static constexpr int NV = R * (int)sizeof(T) / 16;
  ew_u32x4 q[NV];
  T e[R];
};

// the run at p: whole vectors when the host found p + k * R 16-byte aligned for every k (vec), element loads otherwise
template <class T, int R>
__device__ __forceinline__ void ew_load(EwRun<T, R> &r, const T *p, bool vec) {
  if (vec) {
#pragma unroll
    for (int v = 0; v < EwRun<T, R>::NV; ++v) r.q[v] = __builtin_nontemporal_load(reinterpret_cast<const ew_u32x4 *>(p) + v);
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k) r.e[k] = p[k];
  }
}
template <class T, int R>
__device__ __forceinline__ void ew_store(const EwRun<T, R> &r, T *p) {
#pragma unroll
  for (int v = 0; v < EwRun<T, R>::NV; ++v) reinterpret_cast<ew_u32x4 *>(p)[v] = r.q[v];
}

// rows [0, head) and [head + nruns * R, n), one per thread; t counts them
__device__ __forceinline__ int64_t ew_loose_row(int64_t t, int64_t head, int64_t tail0) { return t < head ? t : tail0 + (t - head); }

// A workgroup takes contiguous tiles of EW_THREADS * U runs, lane l of round u the run u * EW_THREADS + l of the tile (the
// tiling of filter.hip's compare_vec_kernel).  `in` and `out` may be the same buffer when the widths are equal: a lane reads
// all of its runs of a tile before it stores any, and nobody else touches those rows.  No __restrict__ for that reason.
template <class In, class Out, class F>
__global__ __launch_bounds__(EW_THREADS) void ew_unary(const In *in, Out *out, int64_t n, int64_t head, int64_t nruns, int in_vec, F f) {
  constexpr int R = 16 / ew_min_width<In, Out>();
  constexpr int U = ew_unroll(R, ew_max_width<In, Out>());
  constexpr int64_t TILE = (int64_t)EW_THREADS * U;
  const In *bin = in + head;
  Out *bout = out + head;
  const int64_t ntile = (nruns + TILE - 1) / TILE;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t j0 = tile * TILE + threadIdx.x;
    EwRun<In, R> a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * EW_THREADS;
      ew_load(a[u], bin + (j < nruns ? j : nruns - 1) * R, in_vec != 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * EW_THREADS;
      if (j >= nruns) break;
      EwRun<Out, R> o;
#pragma unroll
      for (int k = 0; k < R; ++k) o.e[k] = f(a[u].e[k]);
      ew_store(o, bout + j * R);
    }
  }
  const int64_t tail0 = head + nruns * R, loose = head + (n - tail0);
  for (int64_t t = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; t < loose; t += (int64_t)gridDim.x * EW_THREADS) {
    const int64_t i = ew_loose_row(t, head, tail0);
    out[i] = f(in[i]);
  }
}

template <class T, class Out, class F>
__global__ __launch_bounds__(EW_THREADS) void ew_binary(const T *lhs, const T *rhs, Out *out, int64_t n, int64_t head, int64_t nruns,
                                                        int lhs_vec, int rhs_vec, F f) {
  constexpr int R = 16 / ew_min_width<T, Out>();
  constexpr int U = ew_unroll(R, ew_max_width<T, Out>());
  constexpr int64_t TILE = (int64_t)EW_THREADS * U;
  const T *bl = lhs + head, *br = rhs + head;
  Out *bout = out + head;
  const int64_t ntile = (nruns + TILE - 1) / TILE;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t j0 = tile * TILE + threadIdx.x;
    EwRun<T, R> a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * EW_THREADS;
      const int64_t jc = j < nruns ? j : nruns - 1;
      ew_load(a[u], bl + jc * R, lhs_vec != 0);
      ew_load(b[u], br + jc * R, rhs_vec != 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t j = j0 + (int64_t)u * EW_THREADS;
      if (j >= nruns) break;
      EwRun<Out, R> o;
#pragma unroll
      for (int k = 0; k < R; ++k) o.e[k] = f(a[u].e[k], b[u].e[k]);
      ew_store(o, bout + j * R);
    }
  }
  const int64_t tail0 = head + nruns * R, loose = head + (n - tail0);
  for (int64_t t = (int64_t)blockIdx.x * EW_THREADS + threadIdx.x; t < loose; t += (int64_t)gridDim.x * EW_THREADS) {
    const int64_t i = ew_loose_row(t, head, tail0);
    out[i] = f(lhs[i], rhs[i]);
  }
}

// ---------------------------------------------------------------------------
// functors
// ---------------------------------------------------------------------------
template <class T> struct EwUnsigned { using type = typename std::make_unsigned<T>::type; };
template <> struct EwUnsigned<float> { using type = float; };
template <> struct EwUnsigned<double> { using type = double; };

// integers wrap (computed in the unsigned type: no signed-overflow UB); floats are the IEEE operation
template <class T> struct OpAdd { __device__ T operator()(T a, T b) const { using W = typename EwUnsigned<T>::type; return (T)((W)a + (W)b); } };
template <class T> struct OpSub { __device__ T operator()(T a, T b) const { using W = typename EwUnsigned<T>::type; return (T)((W)a - (W)b); } };
template <class T> struct OpMul { __device__ T operator()(T a, T b) const { using W = typename EwUnsigned<T>::type; return (T)((W)a * (W)b); } };
template <class T> struct OpDiv { __device__ T operator()(T a, T b) const { return a / b; } };
// floats: floor(a / b) in T.  integers: exact floor division; b == 0 gives 0 and b == -1 gives the wrapped negation (so
// that INT_MIN / -1 is INT_MIN), neither reaches a division the language leaves undefined
template <class T> struct OpFloorDiv {
  __device__ T operator()(T a, T b) const {
    if constexpr (std::is_floating_point<T>::value) {
      if constexpr (sizeof(T) == 4) return ::floorf(a / b);
      else return ::floor(a / b);
    } else {
      using W = typename EwUnsigned<T>::type;
      if (b == 0) return 0;
      if (b == -1) return (T)((W)0 - (W)a);
      const T q = a / b, r = a % b;
      return (r != 0 && ((r < 0) != (b < 0))) ? q - 1 : q;
    }
  }
};
template <class T> struct OpGt { __device__ int8_t operator()(T a, T b) const { return a > b; } };
template <class T> struct OpGe { __device__ int8_t operator()(T a, T b) const { return a >= b; } };
template <class T> struct OpLt { __device__ int8_t operator()(T a, T b) const { return a < b; } };
template <class T> struct OpLe { __device__ int8_t operator()(T a, T b) const { return a <= b; } };
template <class T> struct OpEq { __device__ int8_t operator()(T a, T b) const { return a == b; } };
template <class T> struct OpNe { __device__ int8_t operator()(T a, T b) const { return a != b; } };
template <class T> struct OpAnd { __device__ T operator()(T a, T b) const { return (T)(a & b); } };
template <class T> struct OpOr { __device__ T operator()(T a, T b) const { return (T)(a | b); } };
template <class T> struct OpXor { __device__ T operator()(T a, T b) const { return (T)(a ^ b); } };

// the device math library's routines, f32 and f64 each its own (no fast-math: the Makefile does not ask for it)
#define EW_MATH_FUNCTOR(Name, fn)                                                                  \
  template <class T> struct Name {                                                                 \
    __device__ T operator()(T x) const {                                                           \
      if constexpr (sizeof(T) == 4) return ::fn##f(x);                                             \
      else return ::fn(x);                                                                         \
    }                                                                                              \
  };
EW_MATH_FUNCTOR(OpSin, sin) EW_MATH_FUNCTOR(OpCos, cos) EW_MATH_FUNCTOR(OpTan, tan) EW_MATH_FUNCTOR(OpAsin, asin)
EW_MATH_FUNCTOR(OpAcos, acos) EW_MATH_FUNCTOR(OpAtan, atan) EW_MATH_FUNCTOR(OpExp, exp) EW_MATH_FUNCTOR(OpLog, log)
EW_MATH_FUNCTOR(OpSqrt, sqrt) EW_MATH_FUNCTOR(OpCeil, ceil) EW_MATH_FUNCTOR(OpFloor, floor)
#undef EW_MATH_FUNCTOR

// floor(x / D) and x - D * floor(x / D) for a positive compile-time D (the compiler turns / and % into multiplications)
template <int64_t D> __device__ __forceinline__ int64_t floor_div(int64_t x) { const int64_t q = x / D; return x % D < 0 ? q - 1 : q; }
template <int64_t D> __device__ __forceinline__ int64_t floor_mod(int64_t x) { const int64_t r = x % D; return r < 0 ? r + D : r; }

template <class In, class Out> struct OpCast { __device__ Out operator()(In x) const { return (Out)x; } };
// date / timestamp unit changes: towards the finer unit a wrapping multiplication, towards the coarser one a FLOOR division
template <class In, class Out> struct OpScaleUp {
  uint64_t factor;
  __device__ Out operator()(In x) const { return (Out)(int64_t)((uint64_t)(int64_t)x * factor); }
};
template <class Out, int64_t D> struct OpScaleDown { __device__ Out operator()(int64_t x) const { return (Out)floor_div<D>(x); } };

// Calendar fields of a day number (days since 1970-01-01, proleptic Gregorian).  The 400-year-era decomposition is the
// public-domain algorithm of H. Hinnant, "chrono-Compatible Low-Level Date Algorithms" (civil_from_days), with the day
// number kept in 64 bits up to the era split.
enum DtField : int { DT_YEAR = 0, DT_MONTH, DT_DAY, DT_HOUR, DT_MINUTE, DT_SECOND };
template <int FIELD>
__device__ __forceinline__ int16_t civil_field(int64_t days) {
  const int64_t z = days + 719468;                                  // days since 0000-03-01
  const int64_t era = floor_div<146097>(z);
  const uint32_t doe = (uint32_t)(z - era * 146097);                // [0, 146096]
  const uint32_t yoe = (doe - doe / 1460 + doe / 36524 - doe / 146096) / 365;     // [0, 399]
  const uint32_t doy = doe - (365 * yoe + yoe / 4 - yoe / 100);     // [0, 365], year starting in March
  const uint32_t mp = (5 * doy + 2) / 153;                          // [0, 11], March = 0
  if constexpr (FIELD == DT_DAY) return (int16_t)(doy - (153 * mp + 2) / 5 + 1);
  const uint32_t m = mp < 10 ? mp + 3 : mp - 9;
  if constexpr (FIELD == DT_MONTH) return (int16_t)m;
  return (int16_t)((int64_t)yoe + era * 400 + (m <= 2 ? 1 : 0));    // truncated to int16
}
template <int FIELD> struct OpDateField { __device__ int16_t operator()(int32_t days) const { return civil_field<FIELD>((int64_t)days); } };
// TPS: ticks per second of the input
template <int FIELD, int64_t TPS> struct OpTimeField {
  __device__ int16_t operator()(int64_t t) const {
    if constexpr (FIELD <= DT_DAY) return civil_field<FIELD>(floor_div<86400 * TPS>(t));
    else if constexpr (FIELD == DT_HOUR) return (int16_t)(floor_mod<86400 * TPS>(t) / (3600 * TPS));
    else if constexpr (FIELD == DT_MINUTE) return (int16_t)(floor_mod<3600 * TPS>(t) / (60 * TPS));
    else return (int16_t)(floor_mod<60 * TPS>(t) / TPS);
  }
};

// ---------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------
struct EwPtr { const void *p; int width; };
struct EwPlan { int64_t head, nruns; int vec[2]; int grid; };

// out, then the inputs.  head: the first row at which the output is 16-byte aligned and, among such rows below 16, the one at
// which most inputs are too.  A pointer that is not even element-aligned sends every row to the one-per-thread path.
static EwPlan ew_plan(int64_t n, int rows_per_run, int unroll, EwPtr out, const EwPtr *in, int nin) {
  EwPlan pl{n, 0, {0, 0}, 1};
  bool elem_aligned = (uintptr_t)out.p % (uintptr_t)out.width == 0;
  for (int i = 0; i < nin; ++i) elem_aligned = elem_aligned && (uintptr_t)in[i].p % (uintptr_t)in[i].width == 0;
  if (elem_aligned) {
    int best = -1;
    for (int64_t h = 0; h < 16; ++h) {
      if (((uintptr_t)out.p + (uintptr_t)(h * out.width)) & 15) continue;
      int score = 0;
      for (int i = 0; i < nin; ++i) score += (((uintptr_t)in[i].p + (uintptr_t)(h * in[i].width)) & 15) == 0;
      if (score > best) { best = score; pl.head = h; }
    }
    if (pl.head > n) pl.head = n;
    pl.nruns = (n - pl.head) / rows_per_run;
    if (pl.nruns == 0) pl.head = n;
    for (int i = 0; i < nin; ++i) pl.vec[i] = (((uintptr_t)in[i].p + (uintptr_t)(pl.head * in[i].width)) & 15) == 0;
  }
  const int64_t loose = n - pl.nruns * rows_per_run;
  const int64_t by_runs = (pl.nruns + (int64_t)EW_THREADS * unroll - 1) / ((int64_t)EW_THREADS * unroll);
  const int64_t by_loose = (loose + EW_THREADS - 1) / EW_THREADS;
  int64_t g = by_runs > by_loose ? by_runs : by_loose;
  if (g > NUM_CU * 8) g = NUM_CU * 8;
  pl.grid = (int)(g < 1 ? 1 : g);
  return pl;
}

static gdf_error ew_finish() {
  HIP_CHECK_LAST();
  HIP_TRY(hipStreamSynchronize(stream0()));
  return GDF_SUCCESS;
}

template <class In, class Out, class F>
static gdf_error unary_launch(const char *name, const gdf_column *in, gdf_column *out, F f) {
  constexpr int R = 16 / ew_min_width<In, Out>();
  const int64_t n = (int64_t)in->size;
  const EwPtr ip{in->data, (int)sizeof(In)};
  const EwPlan pl = ew_plan(n, R, ew_unroll(R, ew_max_width<In, Out>()), EwPtr{out->data, (int)sizeof(Out)}, &ip, 1);
  GDF_LAUNCH(name, (ew_unary<In, Out, F>), dim3(pl.grid), dim3(EW_THREADS), 0, stream0(), (const In *)in->data, (Out *)out->data, n,
             pl.head, pl.nruns, pl.vec[0], f);
  return GDF_SUCCESS;
}

template <class T, class Out, class F>
static gdf_error binary_launch(const gdf_column *lhs, const gdf_column *rhs, gdf_column *out) {
  constexpr int R = 16 / ew_min_width<T, Out>();
  const int64_t n = (int64_t)lhs->size;
  const EwPtr ip[2] = {{lhs->data, (int)sizeof(T)}, {rhs->data, (int)sizeof(T)}};
  const EwPlan pl = ew_plan(n, R, ew_unroll(R, ew_max_width<T, Out>()), EwPtr{out->data, (int)sizeof(Out)}, ip, 2);
  GDF_LAUNCH("ew_binary", (ew_binary<T, Out, F>), dim3(pl.grid), dim3(EW_THREADS), 0, stream0(), (const T *)lhs->data,
             (const T *)rhs->data, (Out *)out->data, n, pl.head, pl.nruns, pl.vec[0], pl.vec[1], F{});
  return ew_finish();
}

// the mask of a cast / datetime result: ceil(size / 8) bytes of the input's, when both columns carry one
static gdf_error copy_mask(const gdf_column *in, gdf_column *out) {
  if (in->valid && out->valid && in->valid != out->valid)
    HIP_TRY(hipMemcpyAsync(out->valid, in->valid, mask_bytes((size_t)in->size), hipMemcpyDeviceToDevice, stream0()));
  return GDF_SUCCESS;
}

// ---- binary ----------------------------------------------------------------
enum BinFamily : int { BF_ARITH = 0, BF_REAL, BF_CMP, BF_BIT };

// the host-side checks shared by the typed and the generic entry points; *run says whether there is anything to launch
static gdf_error binary_check(const gdf_column *lhs, const gdf_column *rhs, const gdf_column *out, int family, bool *run) {
  *run = false;
  GDF_REQUIRE(lhs && rhs && out, GDF_UNSUPPORTED_METHOD);
  if (lhs->size == 0 || rhs->size == 0) return GDF_SUCCESS;
  GDF_REQUIRE(lhs->size == rhs->size && lhs->size == out->size, GDF_COLUMN_SIZE_MISMATCH);
  GDF_REQUIRE(lhs->dtype == rhs->dtype, GDF_UNSUPPORTED_DTYPE);
  GDF_REQUIRE(out->dtype == (family == BF_CMP ? GDF_INT8 : lhs->dtype), GDF_UNSUPPORTED_DTYPE);
  GDF_REQUIRE(lhs->data && rhs->data && out->data, GDF_INVALID_API_CALL);
  *run = true;
  return GDF_SUCCESS;
}

template <class T, class Out, class F>
static gdf_error binary_entry(gdf_column *lhs, gdf_column *rhs, gdf_column *out, int family) {
  bool run;
  GDF_TRY(binary_check(lhs, rhs, out, family, &run));
  if (!run) return GDF_SUCCESS;
  return guarded([&]() -> gdf_error { return binary_launch<T, Out, F>(lhs, rhs, out); });
}

// _generic: the reference's switches on lhs->dtype
static ElemKind binary_generic_kind(gdf_dtype t, int family) {
  switch (t) {
    case GDF_INT8: return family == BF_CMP || family == BF_BIT ? K_I8 : K_BAD;
    case GDF_INT32: return family != BF_REAL ? K_I32 : K_BAD;
    case GDF_INT64: return family != BF_REAL ? K_I64 : K_BAD;
    case GDF_FLOAT32: return family != BF_BIT ? K_F32 : K_BAD;
    case GDF_FLOAT64: return family != BF_BIT ? K_F64 : K_BAD;
    case GDF_DATE32: return family == BF_CMP ? K_I32 : K_BAD;
    case GDF_DATE64: case GDF_TIMESTAMP: return family == BF_CMP ? K_I64 : K_BAD;
    default: return K_BAD;
  }
}

template <template <class> class F, int FAMILY>
static gdf_error binary_generic(gdf_column *lhs, gdf_column *rhs, gdf_column *out) {
  GDF_REQUIRE(lhs && rhs && out, GDF_UNSUPPORTED_METHOD);
  if (lhs->size == 0 || rhs->size == 0) return GDF_SUCCESS;
  const ElemKind k = binary_generic_kind(lhs->dtype, FAMILY);
  GDF_REQUIRE(k != K_BAD, GDF_UNSUPPORTED_DTYPE);
  constexpr bool CMP = FAMILY == BF_CMP;
  if constexpr (FAMILY == BF_CMP || FAMILY == BF_BIT)
    if (k == K_I8) return binary_entry<int8_t, int8_t, F<int8_t>>(lhs, rhs, out, FAMILY);
  if constexpr (FAMILY != BF_REAL) {
    if (k == K_I32) return binary_entry<int32_t, typename std::conditional<CMP, int8_t, int32_t>::type, F<int32_t>>(lhs, rhs, out, FAMILY);
    if (k == K_I64) return binary_entry<int64_t, typename std::conditional<CMP, int8_t, int64_t>::type, F<int64_t>>(lhs, rhs, out, FAMILY);
  }
  if constexpr (FAMILY != BF_BIT) {
    if (k == K_F32) return binary_entry<float, typename std::conditional<CMP, int8_t, float>::type, F<float>>(lhs, rhs, out, FAMILY);
    if (k == K_F64) return binary_entry<double, typename std::conditional<CMP, int8_t, double>::type, F<double>>(lhs, rhs, out, FAMILY);
  }
  return GDF_UNSUPPORTED_DTYPE;
}

// ---- math ------------------------------------------------------------------
template <class T, class F>
static gdf_error math_entry(gdf_column *in, gdf_column *out) {
  GDF_REQUIRE(in && out, GDF_UNSUPPORTED_METHOD);
  if (in->size == 0) return GDF_SUCCESS;
  GDF_REQUIRE(in->size == out->size, GDF_COLUMN_SIZE_MISMATCH);
  GDF_REQUIRE(in->data && out->data, GDF_INVALID_API_CALL);
  return guarded([&]() -> gdf_error {
    GDF_TRY((unary_launch<T, T, F>("ew_math", in, out, F{})));
    return ew_finish();
  });
}
template <template <class> class F>
static gdf_error math_generic(gdf_column *in, gdf_column *out) {
  GDF_REQUIRE(in && out, GDF_UNSUPPORTED_METHOD);
  if (in->dtype == GDF_FLOAT32) return math_entry<float, F<float>>(in, out);
  if (in->dtype == GDF_FLOAT64) return math_entry<double, F<double>>(in, out);
  return GDF_UNSUPPORTED_DTYPE;
}

// ---- casts -----------------------------------------------------------------
// ticks per day of a date / timestamp type; 0: not one, or TIME_UNIT_NONE (then the cast is the plain conversion)
static int64_t ticks_per_day(gdf_dtype t, gdf_time_unit u) {
  if (t == GDF_DATE32) return 1;
  if (t == GDF_DATE64) return 86400000LL;
  if (t != GDF_TIMESTAMP) return 0;
  switch (u) {
    case TIME_UNIT_s: return 86400LL;
    case TIME_UNIT_ms: return 86400000LL;
    case TIME_UNIT_us: return 86400000000LL;
    case TIME_UNIT_ns: return 86400000000000LL;
    default: return 0;
  }
}

template <class In, class Out>
static gdf_error cast_plain(const gdf_column *in, gdf_column *out) {
  return unary_launch<In, Out, OpCast<In, Out>>("ew_cast", in, out, OpCast<In, Out>{});
}
template <class In>
static gdf_error cast_plain_to(ElemKind to, const gdf_column *in, gdf_column *out) {
  switch (to) {
    case K_I8: return cast_plain<In, int8_t>(in, out);
    case K_I32: return cast_plain<In, int32_t>(in, out);
    case K_I64: return cast_plain<In, int64_t>(in, out);
    case K_F32: return cast_plain<In, float>(in, out);
    case K_F64: return cast_plain<In, double>(in, out);
    default: return GDF_UNSUPPORTED_DTYPE;
  }
}
template <class Out>
static gdf_error cast_down(int64_t factor, const gdf_column *in, gdf_column *out) {
  // (a division by a day's ticks ends in DATE32, one by a power of 1000 in a 64-bit type)
#define EW_DOWN(D) case D: if constexpr ((D % 86400 == 0) == (sizeof(Out) == 4)) return unary_launch<int64_t, Out, OpScaleDown<Out, D>>("ew_cast", in, out, OpScaleDown<Out, D>{}); else break;
  switch (factor) {
    EW_DOWN(1000LL) EW_DOWN(1000000LL) EW_DOWN(1000000000LL)
    EW_DOWN(86400LL) EW_DOWN(86400000LL) EW_DOWN(86400000000LL) EW_DOWN(86400000000000LL)
    default: break;
  }
#undef EW_DOWN
  return GDF_UNSUPPORTED_DTYPE;
}

static gdf_error cast_run(gdf_dtype from, gdf_time_unit from_unit, gdf_dtype to, gdf_time_unit to_unit, const gdf_column *in,
                          gdf_column *out) {
  const ElemKind fk = elem_kind(from), tk = elem_kind(to);
  const int64_t ft = ticks_per_day(from, from_unit), tt = ticks_per_day(to, to_unit);
  if (ft && tt && ft != tt) {
    if (tt > ft) {                                   // finer unit
      const uint64_t factor = (uint64_t)(tt / ft);
      if (fk == K_I32) return unary_launch<int32_t, int64_t, OpScaleUp<int32_t, int64_t>>("ew_cast", in, out, OpScaleUp<int32_t, int64_t>{factor});
      return unary_launch<int64_t, int64_t, OpScaleUp<int64_t, int64_t>>("ew_cast", in, out, OpScaleUp<int64_t, int64_t>{factor});
    }
    return tk == K_I32 ? cast_down<int32_t>(ft / tt, in, out) : cast_down<int64_t>(ft / tt, in, out);
  }
  switch (fk) {
    case K_I8: return cast_plain_to<int8_t>(tk, in, out);
    case K_I32: return cast_plain_to<int32_t>(tk, in, out);
    case K_I64: return cast_plain_to<int64_t>(tk, in, out);
    case K_F32: return cast_plain_to<float>(tk, in, out);
    case K_F64: return cast_plain_to<double>(tk, in, out);
    default: return GDF_UNSUPPORTED_DTYPE;
  }
}

// from == GDF_invalid: the _generic entry point, which takes the source type from the column
static gdf_error cast_entry(gdf_column *in, gdf_column *out, gdf_dtype from, gdf_dtype to, gdf_time_unit to_unit) {
  GDF_REQUIRE(in && out, GDF_UNSUPPORTED_METHOD);
  if (from == GDF_invalid) {
    switch (in->dtype) {
      case GDF_INT8: case GDF_INT32: case GDF_INT64: case GDF_FLOAT32: case GDF_FLOAT64:
      case GDF_DATE32: case GDF_DATE64: case GDF_TIMESTAMP: from = in->dtype; break;
      default: return GDF_UNSUPPORTED_DTYPE;
    }
  }
  GDF_REQUIRE(in->dtype == from, GDF_UNSUPPORTED_DTYPE);
  if (in->size != 0) {
    GDF_REQUIRE(in->size == out->size, GDF_COLUMN_SIZE_MISMATCH);
      GDF_REQUIRE(in->data && out->data, GDF_INVALID_API_CALL);
  }
  const gdf_time_unit from_unit = in->dtype_info.time_unit;       // (in and out may be the same struct)
  out->dtype = to;
  if (to == GDF_TIMESTAMP) out->dtype_info.time_unit = to_unit;
  if (in->size == 0) return GDF_SUCCESS;
  return guarded([&]() -> gdf_error {
    GDF_TRY(cast_run(from, from_unit, to, to_unit, in, out));
    GDF_TRY(copy_mask(in, out));
    return ew_finish();
  });
}

// ---- datetime --------------------------------------------------------------
template <int FIELD>
static gdf_error datetime_run(const gdf_column *in, gdf_column *out) {
  if (in->dtype == GDF_DATE32) {
    if constexpr (FIELD <= DT_DAY) return unary_launch<int32_t, int16_t, OpDateField<FIELD>>("ew_datetime", in, out, OpDateField<FIELD>{});
    else return GDF_UNSUPPORTED_DTYPE;
  }
#define EW_TIME(TPS) return unary_launch<int64_t, int16_t, OpTimeField<FIELD, TPS>>("ew_datetime", in, out, OpTimeField<FIELD, TPS>{})
  switch (in->dtype == GDF_TIMESTAMP ? in->dtype_info.time_unit : TIME_UNIT_ms) {
    case TIME_UNIT_s: EW_TIME(1LL);
    case TIME_UNIT_us: EW_TIME(1000000LL);
    case TIME_UNIT_ns: EW_TIME(1000000000LL);
    default: EW_TIME(1000LL);                        // ms, and TIME_UNIT_NONE as in the reference
  }
#undef EW_TIME
}

template <int FIELD>
static gdf_error datetime_entry(gdf_column *in, gdf_column *out) {
  GDF_REQUIRE(in && out, GDF_UNSUPPORTED_METHOD);
  GDF_REQUIRE(in->size == out->size, GDF_COLUMN_SIZE_MISMATCH);
  GDF_REQUIRE(out->dtype == GDF_INT16, GDF_UNSUPPORTED_DTYPE);
  GDF_REQUIRE(in->dtype == GDF_DATE64 || in->dtype == GDF_TIMESTAMP || (in->dtype == GDF_DATE32 && FIELD <= DT_DAY), GDF_UNSUPPORTED_DTYPE);
  if (in->size == 0) return GDF_SUCCESS;
  GDF_REQUIRE(in->data && out->data, GDF_INVALID_API_CALL);
  return guarded([&]() -> gdf_error {
    GDF_TRY(datetime_run<FIELD>(in, out));
    GDF_TRY(copy_mask(in, out));
    return ew_finish();
  });
}

}  // namespace gdf_amd

using namespace gdf_amd;

// ---------------------------------------------------------------------------
// the 182 entry points
// ---------------------------------------------------------------------------
extern "C" {

#define EW_BIN(name, T, Out, F, FAMILY) \
  gdf_error name(gdf_column *lhs, gdf_column *rhs, gdf_column *output) { return binary_entry<T, Out, F<T>>(lhs, rhs, output, FAMILY); }
#define EW_BIN_GENERIC(name, F, FAMILY) \
  gdf_error name(gdf_column *lhs, gdf_column *rhs, gdf_column *output) { return binary_generic<F, FAMILY>(lhs, rhs, output); }

#define EW_ARITH(op, F)                                                                                             \
  EW_BIN_GENERIC(gdf_##op##_generic, F, BF_ARITH)                                                                   \
  EW_BIN(gdf_##op##_i32, int32_t, int32_t, F, BF_ARITH) EW_BIN(gdf_##op##_i64, int64_t, int64_t, F, BF_ARITH)       \
  EW_BIN(gdf_##op##_f32, float, float, F, BF_ARITH)     EW_BIN(gdf_##op##_f64, double, double, F, BF_ARITH)
EW_ARITH(add, OpAdd) EW_ARITH(sub, OpSub) EW_ARITH(mul, OpMul) EW_ARITH(floordiv, OpFloorDiv)
#undef EW_ARITH
EW_BIN_GENERIC(gdf_div_generic, OpDiv, BF_REAL)
EW_BIN(gdf_div_f32, float, float, OpDiv, BF_REAL) EW_BIN(gdf_div_f64, double, double, OpDiv, BF_REAL)

#define EW_CMP(op, F)                                                                                               \
  EW_BIN_GENERIC(gdf_##op##_generic, F, BF_CMP)                                                                     \
  EW_BIN(gdf_##op##_i8, int8_t, int8_t, F, BF_CMP)   EW_BIN(gdf_##op##_i32, int32_t, int8_t, F, BF_CMP)             \
  EW_BIN(gdf_##op##_i64, int64_t, int8_t, F, BF_CMP) EW_BIN(gdf_##op##_f32, float, int8_t, F, BF_CMP)               \
  EW_BIN(gdf_##op##_f64, double, int8_t, F, BF_CMP)
EW_CMP(gt, OpGt) EW_CMP(ge, OpGe) EW_CMP(lt, OpLt) EW_CMP(le, OpLe) EW_CMP(eq, OpEq) EW_CMP(ne, OpNe)
#undef EW_CMP

#define EW_BIT(op, F)                                                                                               \
  EW_BIN_GENERIC(gdf_bitwise_##op##_generic, F, BF_BIT)                                                             \
  EW_BIN(gdf_bitwise_##op##_i8, int8_t, int8_t, F, BF_BIT) EW_BIN(gdf_bitwise_##op##_i32, int32_t, int32_t, F, BF_BIT) \
  EW_BIN(gdf_bitwise_##op##_i64, int64_t, int64_t, F, BF_BIT)
EW_BIT(and, OpAnd) EW_BIT(or, OpOr) EW_BIT(xor, OpXor)
#undef EW_BIT
#undef EW_BIN
#undef EW_BIN_GENERIC

#define EW_MATH(op, F)                                                                                              \
  gdf_error gdf_##op##_generic(gdf_column *input, gdf_column *output) { return math_generic<F>(input, output); }    \
  gdf_error gdf_##op##_f32(gdf_column *input, gdf_column *output) { return math_entry<float, F<float>>(input, output); } \
  gdf_error gdf_##op##_f64(gdf_column *input, gdf_column *output) { return math_entry<double, F<double>>(input, output); }
EW_MATH(sin, OpSin) EW_MATH(cos, OpCos) EW_MATH(tan, OpTan) EW_MATH(asin, OpAsin) EW_MATH(acos, OpAcos) EW_MATH(atan, OpAtan)
EW_MATH(exp, OpExp) EW_MATH(log, OpLog) EW_MATH(sqrt, OpSqrt) EW_MATH(ceil, OpCeil) EW_MATH(floor, OpFloor)
#undef EW_MATH

#define EW_CAST_FROM(X, dst, DST)                                                                                   \
  X(generic, GDF_invalid, dst, DST) X(i8, GDF_INT8, dst, DST) X(i32, GDF_INT32, dst, DST) X(i64, GDF_INT64, dst, DST) \
  X(f32, GDF_FLOAT32, dst, DST) X(f64, GDF_FLOAT64, dst, DST) X(date32, GDF_DATE32, dst, DST)                       \
  X(date64, GDF_DATE64, dst, DST) X(timestamp, GDF_TIMESTAMP, dst, DST)
#define EW_CAST(src, SRC, dst, DST) \
  gdf_error gdf_cast_##src##_to_##dst(gdf_column *input, gdf_column *output) { return cast_entry(input, output, SRC, DST, TIME_UNIT_NONE); }
#define EW_CAST_TS(src, SRC, dst, DST)                                                             \
  gdf_error gdf_cast_##src##_to_##dst(gdf_column *input, gdf_column *output, gdf_time_unit time_unit) { \
    return cast_entry(input, output, SRC, DST, time_unit);                                         \
  }
EW_CAST_FROM(EW_CAST, f32, GDF_FLOAT32) EW_CAST_FROM(EW_CAST, f64, GDF_FLOAT64) EW_CAST_FROM(EW_CAST, i8, GDF_INT8)
EW_CAST_FROM(EW_CAST, i32, GDF_INT32) EW_CAST_FROM(EW_CAST, i64, GDF_INT64) EW_CAST_FROM(EW_CAST, date32, GDF_DATE32)
EW_CAST_FROM(EW_CAST, date64, GDF_DATE64) EW_CAST_FROM(EW_CAST_TS, timestamp, GDF_TIMESTAMP)
#undef EW_CAST_FROM
#undef EW_CAST
#undef EW_CAST_TS

#define EW_DATETIME(field, FIELD) \
  gdf_error gdf_extract_datetime_##field(gdf_column *input, gdf_column *output) { return datetime_entry<FIELD>(input, output); }
EW_DATETIME(year, DT_YEAR) EW_DATETIME(month, DT_MONTH) EW_DATETIME(day, DT_DAY)
EW_DATETIME(hour, DT_HOUR) EW_DATETIME(minute, DT_MINUTE) EW_DATETIME(second, DT_SECOND)
#undef EW_DATETIME

}  // extern "C"
