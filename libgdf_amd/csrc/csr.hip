// csr.hip -- gdf_to_csr: nullable columns -> a row-major CSR matrix (reference src/io/convert/gdf-to-csr.cu; the contract is in
// include/gdf/gdf.h, the design and its measurements in DESIGN.md §13).
//
// Entry (r, c) exists when column c's validity bit r is set.  A TILE is R consecutive rows (R a multiple of 64, so a tile's mask
// bytes start on a multiple of 8 bytes of every mask); its entries are one contiguous range of A / JA.
//   count   one wave per tile popcounts the tile's mask words of every masked column -> tile_tot[tile]; every wave adds what it
//           counted to one 64-bit counter (nnz, exact whatever rows * cols is).  Skipped when no column has a mask.
//   scan    scan_u32_async over the tile totals -> the first A / JA index of every tile.
//   emit    one workgroup per tile, one lane per row.  Each wave first fetches the validity of its 64 rows as ONE 64-bit word per
//           column (one lane per column) into LDS; a lane's bit is then a broadcast LDS read, so the column loads that follow wait
//           for no mask byte and go out eight at a time.  Every lane counts its row, the workgroup scans the counts (IA), then every
//           lane walks the columns with a cursor: a column load is row-contiguous across the wave.
//           default route: value and column id go into an LDS image of the tile's output range, placed so that LDS and global
//           addresses agree mod 16; the workgroup then flushes the image with linear 16-B stores.
//           chunked route (cols too many for an image of 64 rows): the columns are walked C at a time, every row collects its run
//           of the chunk in its own LDS slot and the waves write the runs out one row after the other, lanes along the run.
#include "internal.h"
#include "launch.h"

#include <vector>

namespace gdf_amd {

struct CsrCol {            // the column table lives in device memory: num_cols is unbounded
  const void    *data;
  const uint8_t *valid;    // may be null: every row is an entry
  int            kind;     // ElemKind, K_I8 .. K_F64
  int            pad;
};

constexpr int CSR_COUNT_THREADS = 256;
constexpr int CSR_MAX_R = 256;               // rows per tile = threads per workgroup of the default emit route: 64, 128 or 256
constexpr int CSR_CHUNK_R = 128;             // ... of the chunked route
constexpr int CSR_LDS_BUDGET = 64 * 1024;    // image bytes of one workgroup: two of them leave a quarter of a CU's 160 KiB free
constexpr int CSR_CHUNK_BUDGET = 48 * 1024;
constexpr int CSR_HEAD = 64;                 // bytes in front of the images: the per-wave totals of the workgroup scan

template <class T> struct CsrKind;
template <> struct CsrKind<int8_t>  { static constexpr int K = K_I8; };
template <> struct CsrKind<int16_t> { static constexpr int K = K_I16; };
template <> struct CsrKind<int32_t> { static constexpr int K = K_I32; };
template <> struct CsrKind<int64_t> { static constexpr int K = K_I64; };
template <> struct CsrKind<float>   { static constexpr int K = K_F32; };
template <> struct CsrKind<double>  { static constexpr int K = K_F64; };

// ---- count ---------------------------------------------------------------------------------------------------------------------
// Set bits of mask bytes [b0, b1) that fall into GRANULE g: the 8-byte aligned word at (address of byte b0 rounded down to 8) + 8 g.
// A granule wholly inside the range is one 64-bit load, one at an edge is read bytewise (a mask pointer need not be word-aligned and
// nothing outside [b0, b1) is touched).  `last` is the mask's last byte, of which only the bits in `last_keep` are rows.
__device__ __forceinline__ uint32_t csr_granule_bits(const uint8_t *valid, int64_t b0, int64_t b1, int g, int64_t last, uint32_t last_keep) {
  const uintptr_t p0 = (uintptr_t)(valid + b0), p1 = (uintptr_t)(valid + b1);
  const uintptr_t w = (p0 & ~(uintptr_t)7) + 8 * (uintptr_t)g;
  if (w >= p1) return 0;
  const uintptr_t lo = w < p0 ? p0 : w, hi = w + 8 < p1 ? w + 8 : p1;
  uint64_t v = 0;
  if (hi - lo == 8) {
    v = *reinterpret_cast<const uint64_t *>(w);
  } else {
    for (uintptr_t a = lo; a < hi; ++a) v |= (uint64_t)*reinterpret_cast<const uint8_t *>(a) << (8 * (a - w));
  }
  const uintptr_t pl = (uintptr_t)(valid + last);
  if (pl >= w && pl < w + 8) v &= ~((uint64_t)(0xffu & ~last_keep) << (8 * (pl - w)));
  return (uint32_t)__popcll(v);
}

// One WAVE per tile at a time (a tile of 8 columns has some forty granules), tiles strided over the waves of a fixed grid; every
// wave adds what it counted to the 64-bit total once, at its end.
__global__ __launch_bounds__(CSR_COUNT_THREADS) void csr_count(const CsrCol *__restrict__ cols, int ncols, int n_unmasked, int64_t rows,
                                                                int R, int64_t ntiles, uint32_t *__restrict__ tile_tot,
                                                                unsigned long long *total) {
  const int lane = lane_id();
  const int64_t wave = (int64_t)blockIdx.x * (CSR_COUNT_THREADS / WAVE) + threadIdx.x / WAVE;
  const int64_t nwaves = (int64_t)gridDim.x * (CSR_COUNT_THREADS / WAVE);
  const int64_t last = ((rows + 7) >> 3) - 1;
  const uint32_t last_keep = (rows & 7) ? (1u << (rows & 7)) - 1u : 0xffu;
  const int G = R / 64 + 1;                                   // granules a tile's R / 8 mask bytes can touch
  unsigned long long mine = 0;
  for (int64_t tile = wave; tile < ntiles; tile += nwaves) {  // (wave-uniform)
    const int64_t r0 = tile * R;
    const int64_t nrow = rows - r0 < R ? rows - r0 : R;
    const int64_t b0 = r0 >> 3, b1 = (r0 + nrow + 7) >> 3;
    uint32_t sum = 0;
    for (int64_t i = lane; i < (int64_t)ncols * G; i += WAVE) {
      const uint8_t *valid = cols[i / G].valid;
      if (valid) sum += csr_granule_bits(valid, b0, b1, (int)(i % G), last, last_keep);
    }
    sum = wave_reduce_add(sum) + (uint32_t)n_unmasked * (uint32_t)nrow;
    if (lane == 0) tile_tot[tile] = sum;
    mine += sum;
  }
  if (lane == 0 && mine) atomicAdd(total, mine);
}

// ---- emit ----------------------------------------------------------------------------------------------------------------------
// element i of a column of storage `kind`, converted to T.  The result type is the largest dtype enumerator of the call, so only
// kinds up to T's own occur: every conversion is a widening static_cast in enum order.
template <class T>
__device__ __forceinline__ T csr_load(const void *data, int kind, int64_t i) {
  constexpr int TK = CsrKind<T>::K;
  if constexpr (TK >= K_F64) { if (kind == K_F64) return (T)((const double *)data)[i]; }
  if constexpr (TK >= K_F32) { if (kind == K_F32) return (T)((const float *)data)[i]; }
  if constexpr (TK >= K_I64) { if (kind == K_I64) return (T)((const int64_t *)data)[i]; }
  if constexpr (TK >= K_I32) { if (kind == K_I32) return (T)((const int32_t *)data)[i]; }
  if constexpr (TK >= K_I16) { if (kind == K_I16) return (T)((const int16_t *)data)[i]; }
  return (T)((const int8_t *)data)[i];
}

constexpr int CSR_UNROLL = 8;      // column loads a lane has in flight: they do not wait for one another, nor for a mask byte

// Validity of the 64 rows from rw0 (a multiple of 64) on in one column as a word: bit l is row rw0 + l.  mb: bytes of the mask.
// Bits of rows beyond the column's end are whatever the mask holds (the caller's `live` drops them); nothing beyond the mask's
// last byte is read.  One lane fetches the word of one column, so a wave's mask traffic is 8 bytes per column and 64 rows.
__device__ __forceinline__ uint64_t csr_row_word(const uint8_t *valid, int64_t rw0, int64_t mb) {
  if (!valid) return ~0ull;
  const int64_t b = rw0 >> 3;
  if (b >= mb) return 0;
  const uint8_t *p = valid + b;
  if (b + 8 <= mb && ((uintptr_t)p & 7) == 0) return *reinterpret_cast<const uint64_t *>(p);
  const int n = mb - b < 8 ? (int)(mb - b) : 8;
  uint64_t v = 0;
  for (int i = 0; i < n; ++i) v |= (uint64_t)p[i] << (8 * i);
  return v;
}

// this wave's words of columns [c0, c1) -> s_bits[0 .. c1 - c0); every thread of the workgroup calls it (it ends in a barrier)
__device__ __forceinline__ void csr_stage_words(const CsrCol *__restrict__ cols, int c0, int c1, int64_t rw0, int64_t mb, uint64_t *s_bits) {
  for (int c = c0 + lane_id(); c < c1; c += WAVE) s_bits[c - c0] = csr_row_word(cols[c].valid, rw0, mb);
  block_sync();
}

// the workgroup's exclusive scan of cnt -> excl, the sum -> tile_total.  Every thread of the workgroup calls it (wave_scan_incl
// needs full waves: the block size is a multiple of 64).
__device__ __forceinline__ void csr_block_scan(uint32_t cnt, uint32_t *s_wave, uint32_t &excl, uint32_t &tile_total) {
  const uint32_t incl = wave_scan_incl(cnt);
  const int wv = (int)(threadIdx.x / WAVE), nw = (int)(blockDim.x / WAVE);
  if (lane_id() == WAVE - 1) s_wave[wv] = incl;
  block_sync();
  uint32_t before = 0, all = 0;
  for (int w = 0; w < nw; ++w) {
    const uint32_t t = s_wave[w];
    before += w < wv ? t : 0u;
    all += t;
  }
  excl = before + incl - cnt;
  tile_total = all;
}

// The entries of row r in columns [c0, c1), CSR_UNROLL columns at a time: first the loads, then the stores.  put(k, value, column)
// is called for the k-th entry found, k counting from 0; returns their number.  s_bits: the staged words of [c0, c1), null when no
// column has a mask.
template <class T, class Put>
__device__ __forceinline__ uint32_t csr_walk(const CsrCol *__restrict__ cols, int c0, int c1, const uint64_t *s_bits, bool live, int64_t r,
                                             Put &&put) {
  const int lane = lane_id();
  uint32_t k = 0;
  for (int c = c0; c < c1; c += CSR_UNROLL) {
    T v[CSR_UNROLL];
    bool on[CSR_UNROLL];
#pragma unroll
    for (int u = 0; u < CSR_UNROLL; ++u) {
      const int cc = c + u;
      on[u] = live && cc < c1 && (!s_bits || ((s_bits[cc - c0] >> lane) & 1));
      v[u] = T(0);
      if (on[u]) v[u] = csr_load<T>(cols[cc].data, cols[cc].kind, r);
    }
#pragma unroll
    for (int u = 0; u < CSR_UNROLL; ++u)
      if (on[u]) put(k++, v[u], c + u);
  }
  return k;
}

__device__ __forceinline__ uint32_t csr_count_bits(const uint64_t *s_bits, int n, bool live) {
  const int lane = lane_id();
  uint32_t cnt = 0;
  for (int c = 0; c < n; ++c) cnt += (uint32_t)((s_bits[c] >> lane) & 1);
  return live ? cnt : 0u;
}

// default route.  Dynamic LDS: [CSR_HEAD | s_bits: one word per wave and column | imgJ: 2 + R * ncols column ids (uint32) | imgA:
// 16 B + R * ncols elements], each part a multiple of 16 bytes.  Entry k of the tile sits at imgJ[eJ + k] / imgA[eA + k], where
// eJ / eA are the distances of JA + base / A + base from the 16-B boundary below them: a 16-B vector of the image is a 16-B aligned
// vector of the output.
template <class T, bool MASKED>
__global__ __launch_bounds__(CSR_MAX_R) void csr_emit(const CsrCol *__restrict__ cols, int ncols, int64_t rows,
                                                       const uint32_t *__restrict__ tile_off, T *__restrict__ A, int64_t *__restrict__ JA,
                                                       gdf_size_type *__restrict__ IA) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int R = (int)blockDim.x, tid = (int)threadIdx.x, wv = tid / WAVE, nw = R / WAVE;
  const size_t cap = (size_t)R * (size_t)ncols;
  uint32_t *s_wave = reinterpret_cast<uint32_t *>(smem);
  uint64_t *s_bits = reinterpret_cast<uint64_t *>(smem + CSR_HEAD) + (size_t)wv * ncols;
  const size_t bits_bytes = ((size_t)nw * ncols * 8 + 15) & ~(size_t)15;
  uint32_t *imgJ = reinterpret_cast<uint32_t *>(smem + CSR_HEAD + bits_bytes);
  unsigned char *imgA_bytes = smem + CSR_HEAD + bits_bytes + (((cap + 2) * 4 + 15) & ~(size_t)15);
  T *imgA = reinterpret_cast<T *>(imgA_bytes);

  const int64_t r0 = (int64_t)blockIdx.x * R, r = r0 + tid;
  const bool live = r < rows;
  uint32_t cnt = live ? (uint32_t)ncols : 0u, excl, total;
  if (MASKED) {
    csr_stage_words(cols, 0, ncols, r0 + (int64_t)wv * WAVE, (rows + 7) >> 3, s_bits);
    cnt = csr_count_bits(s_bits, ncols, live);
  }
  csr_block_scan(cnt, s_wave, excl, total);
  const int64_t base = MASKED ? (int64_t)tile_off[blockIdx.x] : r0 * ncols;
  if (live) {
    IA[r] = (gdf_size_type)(base + excl);
    if (r == rows - 1) IA[rows] = (gdf_size_type)(base + excl + cnt);
  }
  if (total == 0) return;                                              // (workgroup-uniform)

  const uint32_t offA = (uint32_t)((uintptr_t)(A + base) & 15), eA = offA / (uint32_t)sizeof(T);
  const uint32_t eJ = (uint32_t)(((uintptr_t)(JA + base) & 15) / 8);
  csr_walk<T>(cols, 0, ncols, MASKED ? s_bits : nullptr, live, r, [&](uint32_t k, T v, int c) {
    imgA[eA + excl + k] = v;
    imgJ[eJ + excl + k] = (uint32_t)c;
  });
  block_sync();

  // A: image bytes [sb, eb) -> the same offsets from gA, which is 16-B aligned
  {
    unsigned char *gA = reinterpret_cast<unsigned char *>(A + base) - offA;
    const uint32_t sb = offA, eb = offA + total * (uint32_t)sizeof(T);
    const uint32_t v0 = (sb + 15) & ~15u, v1 = eb & ~15u;
    T *dst = A + base;
    if (v0 > eb) {
      for (uint32_t k = tid; k < total; k += R) dst[k] = imgA[eA + k];
    } else {
      for (uint32_t j = v0 / 16 + tid; j < v1 / 16; j += R)
        *reinterpret_cast<uint4 *>(gA + 16 * (size_t)j) = *reinterpret_cast<const uint4 *>(imgA_bytes + 16 * (size_t)j);
      const uint32_t nhead = (v0 - sb) / (uint32_t)sizeof(T), tail0 = (v1 - sb) / (uint32_t)sizeof(T);
      if ((uint32_t)tid < nhead) dst[tid] = imgA[eA + tid];
      if (tail0 + tid < total) dst[tail0 + tid] = imgA[eA + tail0 + tid];        // fewer than 16 elements
    }
  }
  // JA: two ids per 16-B store
  {
    int64_t *gJ = JA + base - eJ;
    const uint32_t n_img = eJ + total;
    for (uint32_t p = eJ + tid; p < n_img / 2; p += R)                  // (eJ == 1: the pair of image slots 0 and 1 is the head)
      *reinterpret_cast<uint4 *>(gJ + 2 * (size_t)p) = make_uint4(imgJ[2 * p], 0u, imgJ[2 * p + 1], 0u);
    if (tid == 0 && eJ == 1) gJ[1] = (int64_t)imgJ[1];
    if (tid == R - 1 && (n_img & 1)) gJ[n_img - 1] = (int64_t)imgJ[n_img - 1];
  }
}

// chunked route.  Dynamic LDS: [CSR_HEAD | s_cnt: R uint32 | s_dst: R int64 | s_bits: one word per wave and column of a chunk |
// imgJ: R * S uint32 | imgA: R * S elements]; S = C | 1 is odd, so the lanes of a wave -- one row slot each -- start on different
// banks.  The masks are walked twice, a chunk's words at a time: once for the rows' totals (IA, and where each row starts), once
// with the data.
template <class T>
__global__ __launch_bounds__(CSR_CHUNK_R) void csr_emit_chunked(const CsrCol *__restrict__ cols, int ncols, int64_t rows, int masked,
                                                                 const uint32_t *__restrict__ tile_off, int C, T *__restrict__ A,
                                                                 int64_t *__restrict__ JA, gdf_size_type *__restrict__ IA) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int R = (int)blockDim.x, tid = (int)threadIdx.x, S = C | 1;
  const int wv = tid / WAVE, nw = R / WAVE, lane = lane_id();
  uint32_t *s_wave = reinterpret_cast<uint32_t *>(smem);
  uint32_t *s_cnt = reinterpret_cast<uint32_t *>(smem + CSR_HEAD);
  int64_t *s_dst = reinterpret_cast<int64_t *>(smem + CSR_HEAD + (size_t)R * 4);
  uint64_t *s_bits = reinterpret_cast<uint64_t *>(smem + CSR_HEAD + (size_t)R * 12) + (size_t)wv * C;
  const size_t bits_bytes = ((size_t)nw * C * 8 + 15) & ~(size_t)15;
  uint32_t *imgJ = reinterpret_cast<uint32_t *>(smem + CSR_HEAD + (size_t)R * 12 + bits_bytes);
  T *imgA = reinterpret_cast<T *>(smem + CSR_HEAD + (size_t)R * 12 + bits_bytes + ((((size_t)R * S * 4) + 15) & ~(size_t)15));

  const int64_t r0 = (int64_t)blockIdx.x * R, r = r0 + tid, rw0 = r0 + (int64_t)wv * WAVE, mb = (rows + 7) >> 3;
  const bool live = r < rows;
  uint32_t cnt = live ? (uint32_t)ncols : 0u, excl, total;
  if (masked) {
    cnt = 0;
    for (int c0 = 0; c0 < ncols; c0 += C) {
      const int c1 = c0 + C < ncols ? c0 + C : ncols;
      csr_stage_words(cols, c0, c1, rw0, mb, s_bits);
      cnt += csr_count_bits(s_bits, c1 - c0, live);
      block_sync();                                                    // (the next chunk's words overwrite these)
    }
  }
  csr_block_scan(cnt, s_wave, excl, total);
  const int64_t base = masked ? (int64_t)tile_off[blockIdx.x] : r0 * ncols;
  int64_t pos = base + excl;                                           // where this row's next run starts
  if (live) {
    IA[r] = (gdf_size_type)pos;
    if (r == rows - 1) IA[rows] = (gdf_size_type)(pos + cnt);
  }
  if (total == 0) return;                                              // (workgroup-uniform)

  for (int c0 = 0; c0 < ncols; c0 += C) {
    const int c1 = c0 + C < ncols ? c0 + C : ncols;
    if (masked) csr_stage_words(cols, c0, c1, rw0, mb, s_bits);
    const uint32_t k = csr_walk<T>(cols, c0, c1, masked ? s_bits : nullptr, live, r, [&](uint32_t i, T v, int c) {
      imgA[(size_t)tid * S + i] = v;
      imgJ[(size_t)tid * S + i] = (uint32_t)c;
    });
    s_cnt[tid] = k;
    s_dst[tid] = pos;
    pos += k;
    block_sync();
    for (int rr = wv; rr < R; rr += nw) {
      const uint32_t n = s_cnt[rr];
      const int64_t d = s_dst[rr];
      for (uint32_t l = lane; l < n; l += WAVE) {
        A[d + l] = imgA[(size_t)rr * S + l];
        JA[d + l] = (int64_t)imgJ[(size_t)rr * S + l];
      }
    }
    block_sync();
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct CsrPlan {
  bool chunked;
  int R;           // rows per tile
  int C;           // columns per chunk (chunked route)
  size_t lds;
};

static size_t csr_chunk_lds(int R, int C, int w) {
  const size_t S = (size_t)(C | 1);
  const size_t bits = ((size_t)(R / WAVE) * C * 8 + 15) & ~(size_t)15;
  return CSR_HEAD + (size_t)R * 12 + bits + (((size_t)R * S * 4 + 15) & ~(size_t)15) + (size_t)R * S * w;
}
static size_t csr_image_lds(int R, int ncols, int w) {
  const size_t cap = (size_t)R * ncols;
  const size_t bits = ((size_t)(R / WAVE) * ncols * 8 + 15) & ~(size_t)15;
  return CSR_HEAD + bits + (((cap + 2) * 4 + 15) & ~(size_t)15) + 16 + ((cap * w + 15) & ~(size_t)15);
}

// w: bytes of an element of A
static CsrPlan csr_plan(int ncols, int w) {
  CsrPlan p{};
  p.chunked = lab::path_on("GDF_CSR_CHUNKED") || csr_image_lds(WAVE, ncols, w) > (size_t)CSR_LDS_BUDGET;
  if (!p.chunked) {
    p.R = WAVE;
    while (p.R < CSR_MAX_R && csr_image_lds(p.R * 2, ncols, w) <= (size_t)CSR_LDS_BUDGET) p.R *= 2;
    p.lds = csr_image_lds(p.R, ncols, w);
    return p;
  }
  p.R = CSR_CHUNK_R;
  int cmax = WAVE;                                                     // one store instruction per row and chunk
  while (cmax > 1 && csr_chunk_lds(p.R, cmax, w) > (size_t)CSR_CHUNK_BUDGET) --cmax;
  if (cmax > ncols) cmax = ncols;
  long long c = lab::path_int("GDF_CSR_CHUNK", cmax);
  if (c < 1) c = 1;
  if (c > cmax) c = cmax;
  p.C = (int)c;
  p.lds = csr_chunk_lds(p.R, p.C, w);
  return p;
}

template <class T>
static gdf_error csr_run(const CsrPlan &plan, const CsrCol *d_cols, int ncols, int64_t rows, bool masked, const uint32_t *tile_off,
                         void *A, int64_t *JA, gdf_size_type *IA) {
  const dim3 grid((unsigned)((rows + plan.R - 1) / plan.R)), block((unsigned)plan.R);
  if (plan.chunked) {
    GDF_TRY(launch_lds("csr_emit_chunked", csr_emit_chunked<T>, grid, block, plan.lds, d_cols, ncols, rows, masked ? 1 : 0, tile_off,
                       plan.C, (T *)A, JA, IA));
  } else {
    GDF_TRY(with_bools([&](auto M) { return launch_lds("csr_emit", csr_emit<T, M()>, grid, block, plan.lds, d_cols, ncols, rows, tile_off,
                                                       (T *)A, JA, IA); }, masked));
  }
  HIP_CHECK_LAST();
  return GDF_SUCCESS;
}

static gdf_error to_csr(gdf_column **gdfData, int num_cols, csr_gdf *csrReturn) {
  GDF_REQUIRE(csrReturn, GDF_INVALID_API_CALL);
  GDF_REQUIRE(gdfData && num_cols > 0, GDF_DATASET_EMPTY);
  for (int c = 0; c < num_cols; ++c) GDF_REQUIRE(gdfData[c], GDF_DATASET_EMPTY);
  const gdf_size_type rows_u = gdfData[0]->size;
  for (int c = 0; c < num_cols; ++c) GDF_REQUIRE(gdfData[c]->size == rows_u, GDF_COLUMN_SIZE_MISMATCH);
  int out_dtype = GDF_invalid;
  for (int c = 0; c < num_cols; ++c) {
    const int t = (int)gdfData[c]->dtype;
    GDF_REQUIRE(t >= GDF_INT8 && t <= GDF_FLOAT64, GDF_UNSUPPORTED_DTYPE);
    if (t > out_dtype) out_dtype = t;
  }
  for (int c = 0; c < num_cols; ++c) GDF_REQUIRE(rows_u == 0 || gdfData[c]->data, GDF_DATASET_EMPTY);
  GDF_REQUIRE(rows_u <= (gdf_size_type)INT64_MAX / 2, GDF_COLUMN_SIZE_TOO_BIG);
  const int64_t rows = (int64_t)rows_u;
  const int64_t limit = lab::path_int("GDF_CSR_MAX_NNZ", INT32_MAX);
  const int w = dtype_width((gdf_dtype)out_dtype);

  std::vector<CsrCol> table((size_t)num_cols);
  int n_unmasked = 0;
  for (int c = 0; c < num_cols; ++c) {
    table[c] = CsrCol{gdfData[c]->data, (const uint8_t *)gdfData[c]->valid, (int)elem_kind(gdfData[c]->dtype), 0};
    n_unmasked += gdfData[c]->valid ? 0 : 1;
  }
  const bool masked = n_unmasked != num_cols;
  // without a mask nnz is known here
  if (!masked && rows > 0) GDF_REQUIRE(rows <= limit / num_cols, GDF_COLUMN_SIZE_TOO_BIG);

  const CsrPlan plan = csr_plan(num_cols, w);
  lab::note("csr.route", plan.chunked ? 1 : 0);
  lab::note("csr.rows_per_tile", plan.R);
  lab::note("csr.chunk", plan.chunked ? plan.C : 0);
  const int64_t ntiles = (rows + plan.R - 1) / plan.R;
  GDF_REQUIRE(ntiles <= INT32_MAX, GDF_COLUMN_SIZE_TOO_BIG);           // one workgroup per tile

  DevBuf ia, ja, a, d_table, tiles, scan_scratch;
  RMM_TRY(ia.alloc(sizeof(gdf_size_type) * (size_t)(rows + 1)));
  int64_t nnz = 0;
  if (rows > 0) {
    RMM_TRY(d_table.alloc(sizeof(CsrCol) * table.size()));
    HIP_TRY(hipMemcpyAsync(d_table.p, table.data(), sizeof(CsrCol) * table.size(), hipMemcpyHostToDevice, stream0()));
    HIP_TRY(hipStreamSynchronize(stream0()));                          // `table` is pageable host memory
    if (masked) {
      // [total (8 B) | pad to 16 | tile totals, then tile offsets in place]
      RMM_TRY(tiles.alloc(16 + sizeof(uint32_t) * (size_t)ntiles));
      HIP_TRY(hipMemsetAsync(tiles.p, 0, 16, stream0()));
      uint32_t *tile_tot = reinterpret_cast<uint32_t *>(tiles.as<unsigned char>() + 16);
      const int count_grid = stream_grid((size_t)ntiles, CSR_COUNT_THREADS / WAVE);
      GDF_LAUNCH("csr_count", csr_count, dim3(count_grid), dim3(CSR_COUNT_THREADS), 0, stream0(), d_table.as<CsrCol>(), num_cols,
                 n_unmasked, rows, plan.R, ntiles, tile_tot, tiles.as<unsigned long long>());
      HIP_CHECK_LAST();
      GDF_TRY(scan_u32_async(tile_tot, tile_tot, (size_t)ntiles, false, &scan_scratch));
      unsigned long long total = 0;
      HIP_TRY(read_back(&total, tiles.p, sizeof(total)));
      GDF_REQUIRE(total <= (unsigned long long)limit, GDF_COLUMN_SIZE_TOO_BIG);
      nnz = (int64_t)total;
    } else {
      nnz = rows * num_cols;
    }
  }
  if (nnz == 0) {
    HIP_TRY(hipMemsetAsync(ia.p, 0, sizeof(gdf_size_type) * (size_t)(rows + 1), stream0()));
  } else {
    RMM_TRY(a.alloc((size_t)nnz * (size_t)w));
    RMM_TRY(ja.alloc((size_t)nnz * sizeof(int64_t)));
    const uint32_t *tile_off = masked ? reinterpret_cast<const uint32_t *>(tiles.as<unsigned char>() + 16) : nullptr;
    GDF_TRY(with_int<K_I8, K_I16, K_I32, K_I64, K_F32, K_F64>((int)elem_kind((gdf_dtype)out_dtype), [&](auto K) -> gdf_error {
      using T = std::conditional_t<K() == K_I8, int8_t, std::conditional_t<K() == K_I16, int16_t, std::conditional_t<K() == K_I32, int32_t,
                std::conditional_t<K() == K_I64, int64_t, std::conditional_t<K() == K_F32, float, double>>>>>;
      return csr_run<T>(plan, d_table.as<CsrCol>(), num_cols, rows, masked, tile_off, a.p, ja.as<int64_t>(), ia.as<gdf_size_type>());
    }));
  }
  HIP_TRY(hipStreamSynchronize(stream0()));                            // the scratch is released on return; the outputs are written

  csrReturn->A = a.release();
  csrReturn->IA = static_cast<gdf_size_type *>(ia.release());
  csrReturn->JA = static_cast<int64_t *>(ja.release());
  csrReturn->dtype = (gdf_dtype)out_dtype;
  csrReturn->nnz = nnz;
  csrReturn->rows = rows_u;
  csrReturn->cols = (gdf_size_type)num_cols;
  return GDF_SUCCESS;
}

}  // namespace gdf_amd

extern "C" {

gdf_error gdf_to_csr(gdf_column **gdfData, int num_cols, csr_gdf *csrReturn) {
  return gdf_amd::guarded([&]() -> gdf_error { return gdf_amd::to_csr(gdfData, num_cols, csrReturn); });
}

}  // extern "C"
