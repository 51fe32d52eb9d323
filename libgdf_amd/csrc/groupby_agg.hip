// groupby_agg.hip -- gdf_amd_group_by_agg: GROUP BY over masked key columns with several aggregates in ONE pass over the sorted rows
// (include/gdf/gdf_amd_ext.h has the contract).  No counterpart in the reference, whose Python layer loops over (column, op) and whose
// gdf_group_by_* refuse masks (src/sqls_ops.cu:1103-1106).
//
//   order_rows_ex   (order.hip) the stable permutation `perm` of the rows: ascending, a column's nulls behind its values.
//   gba_heads       position i of perm is a HEAD when i == 0 or row perm[i] differs from row perm[i - 1] in some key column: nullness
//                   first, then -- never under a null bit -- integers by value, floats by ob_float_image.  (gba_heads_images: when
//                   order_rows_ex packed the whole key into ONE 64-bit image per row, equal images mean equal rows, nulls included,
//                   and the sorted images it leaves behind are compared instead -- a streaming read, no gather.)  One wave owns 64 positions,
//                   its ballot IS the head word (one 8-byte store by lane 0); one workgroup owns a tile of GBA_TILE positions and leaves
//                   the tile's head count.  scan_u32 over the counts gives every tile's first group number and G, the one number the
//                   outputs are sized from.
//   gba_reduce      one workgroup per tile, one position per lane.  perm and the head word are loaded once; the distinct value columns
//                   the requests name ("tasks": a column is gathered once however many requests name it) go through in batches of
//                   GBA_BATCH, all gathers of a batch issued before the first use.  Per task a lane carries (valid count, sum as int64
//                   or double, min image, max image); the lanes of a group are folded by a head-flag segmented scan over the wave
//                   (__shfl_up, distance 1 .. 32, a lane takes its left neighbour only from inside its segment), the waves of a tile
//                   through LDS in wave order.  The lane on a group's LAST position holds the group's fold: a group whose head lies in
//                   the tile is stored straight to slot (tile's first group + heads up to here - 1); the part of a group that began in
//                   an earlier tile goes to the tile's FRONT carry record, the part of a group that runs on into the next tile to its
//                   BACK record.
//   gba_fixup       one wave per (tile with a BACK record, task): back[t] + front[t + 1] + front[t + 2] ... up to the first tile that
//                   holds a head (or the last one), 64 records per step through an ordered shuffle tree, the steps left to right; one
//                   plain store to the group's slot.
//   gba_finish      one wave per 64 groups and request: AVG's division, COUNT's widening, the copy where two requests share one fold,
//                   the mask word as the ballot of "has a valid value" and the null count.
//   gather_columns  (order.hip) the key outputs: the key columns' rows perm[head of group].
//
// HOST READ-BACKS: G before the outputs can be allocated; the null counts of the aggregates and (inside gather_columns) of the keys at
// the end, because they go into the host structs.  Temporary device memory beyond order_rows_ex's: perm (4 bytes per row), the head
// words (1 bit per row), two carry records per tile and task, and per task one uint32 valid count per GROUP -- nothing per row and request.
//
// DETERMINISM: every fold above has a fixed shape -- lane distances, wave order, tile order -- and every result is a plain store by
// one thread; the only atomics are integer adds of null counts.  A float sum is therefore the same bits on every call.
#include "internal.h"

#include <gdf/gdf_amd_ext.h>

#include <vector>

namespace gdf_amd {

constexpr int GBA_TILE = 1024;                  // T: sorted positions per workgroup of gba_heads / gba_reduce, one per lane
constexpr int GBA_WAVES = GBA_TILE / WAVE;
constexpr int GBA_BATCH = 4;                    // value columns gathered from one load of perm
constexpr int GBA_FIN_BATCH = 8;                // requests finished per launch
constexpr int GBA_MAX_VALUES = 64, GBA_MAX_AGGS = 64;
enum : int { GBA_SUM = 1, GBA_MIN = 2, GBA_MAX = 4 };

// what one lane, one group or one carry record holds of a task
struct GbaAcc {
  uint64_t sum;      // int64, or the bits of a double
  uint64_t mn, mx;   // order images: integers with the sign bit flipped, floats ob_float_image_of
  uint32_t cnt;      // valid values
  uint32_t pad;
};
// one distinct value column (data == nullptr: COUNT(*), every row counts) and where its folds go
struct GbaTask {
  const void *data;
  const uint8_t *valid;    // may be null
  int kind;
  int want;                // GBA_SUM | GBA_MIN | GBA_MAX
  uint32_t *cnt;           // [G]
  uint64_t *sum;           // [G] when want & GBA_SUM
  void *mn, *mx;           // [G] in the column's own width
  GbaAcc *carry;           // [2 * ntiles]: front, back
};
struct GbaBatch {
  int n;
  GbaTask t[GBA_BATCH];
};

__device__ __forceinline__ bool gba_is_float(int kind) { return kind == K_F32 || kind == K_F64; }

__device__ __forceinline__ bool gba_rows_differ(const KeyTable &t, int64_t a, int64_t b) {
  for (int c = 0; c < t.ncols; ++c) {
    const ColView &k = t.col[c];
    const bool na = k.valid && !bit_is_set(k.valid, a), nb = k.valid && !bit_is_set(k.valid, b);
    if (na != nb) return true;
    if (na) continue;                                          // both null: equal, and the data is not loaded
    if (gba_is_float(k.kind)) {
      if (ob_float_image(k.data, k.kind, a) != ob_float_image(k.data, k.kind, b)) return true;
    } else if (load_bits(k, a) != load_bits(k, b)) {
      return true;
    }
  }
  return false;
}

// heads: GBA_WAVES words per tile (the words behind ceil(n / 64) are zero); nheads[tile] = set bits of the tile
__global__ __launch_bounds__(GBA_TILE) void gba_heads(KeyTable t, const uint32_t *__restrict__ perm, uint32_t n, unsigned long long *__restrict__ heads,
                                                      uint32_t *__restrict__ nheads) {
  __shared__ uint32_t wcount[GBA_WAVES];
  const uint32_t tile = blockIdx.x, w = threadIdx.x / WAVE;
  const uint64_t i = (uint64_t)tile * GBA_TILE + threadIdx.x;
  bool head = false;
  if (i < n) head = i == 0 || gba_rows_differ(t, perm[i], perm[i - 1]);
  const unsigned long long word = __ballot(head);
  if (lane_id() == 0) {
    heads[(uint64_t)tile * GBA_WAVES + w] = word;
    wcount[w] = (uint32_t)__popcll(word);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int v = 0; v < GBA_WAVES; ++v) sum += wcount[v];
    nheads[tile] = sum;
  }
}

// the same from the sorted images of order_rows_ex, when one image holds the whole key: no gather
__global__ __launch_bounds__(GBA_TILE) void gba_heads_images(const uint64_t *__restrict__ images, uint32_t n, unsigned long long *__restrict__ heads,
                                                             uint32_t *__restrict__ nheads) {
  __shared__ uint32_t wcount[GBA_WAVES];
  const uint32_t tile = blockIdx.x, w = threadIdx.x / WAVE;
  const uint64_t i = (uint64_t)tile * GBA_TILE + threadIdx.x;
  bool head = false;
  if (i < n) head = i == 0 || images[i] != images[i - 1];
  const unsigned long long word = __ballot(head);
  if (lane_id() == 0) {
    heads[(uint64_t)tile * GBA_WAVES + w] = word;
    wcount[w] = (uint32_t)__popcll(word);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
#pragma unroll
    for (int v = 0; v < GBA_WAVES; ++v) sum += wcount[v];
    nheads[tile] = sum;
  }
}

__device__ __forceinline__ uint64_t gba_add(uint64_t a, uint64_t b, bool isf) {
  return isf ? (uint64_t)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b)) : a + b;
}
// l stands left of r in sorted order
__device__ __forceinline__ GbaAcc gba_fold(const GbaAcc &l, const GbaAcc &r, int want, bool isf) {
  GbaAcc o = r;
  o.cnt = l.cnt + r.cnt;
  if (want & GBA_SUM) o.sum = gba_add(l.sum, r.sum, isf);
  if (want & GBA_MIN) o.mn = l.mn < r.mn ? l.mn : r.mn;
  if (want & GBA_MAX) o.mx = l.mx > r.mx ? l.mx : r.mx;
  return o;
}
// the fold of nothing.  -0.0 is the identity of a float add (+0.0 would turn a sum of -0.0 into +0.0)
__device__ __forceinline__ GbaAcc gba_identity(bool isf) {
  GbaAcc o;
  o.sum = isf ? 0x8000000000000000ULL : 0ULL;
  o.mn = ~0ULL;
  o.mx = 0ULL;
  o.cnt = 0;
  o.pad = 0;
  return o;
}
__device__ __forceinline__ uint64_t gba_unimage(uint64_t img, int kind) {
  if (kind == K_F32) {
    const uint32_t m = (uint32_t)img;
    return m == 0xffffffffu ? 0x7fc00000u : (m >> 31) ? (m ^ 0x80000000u) : (uint32_t)~m;
  }
  if (kind == K_F64) return img == ~0ULL ? 0x7ff8000000000000ULL : (img >> 63) ? (img ^ 0x8000000000000000ULL) : ~img;
  return img ^ 0x8000000000000000ULL;
}
__device__ __forceinline__ void gba_store_kind(void *p, int kind, uint64_t i, uint64_t v) {
  switch (kind) {
    case K_I8: ((uint8_t *)p)[i] = (uint8_t)v; break;
    case K_I16: ((uint16_t *)p)[i] = (uint16_t)v; break;
    case K_I32: case K_F32: ((uint32_t *)p)[i] = (uint32_t)v; break;
    default: ((uint64_t *)p)[i] = v; break;
  }
}
__device__ __forceinline__ uint64_t gba_load_kind(const void *p, int kind, uint64_t i) {
  switch (kind) {
    case K_I8: return ((const uint8_t *)p)[i];
    case K_I16: return ((const uint16_t *)p)[i];
    case K_I32: case K_F32: return ((const uint32_t *)p)[i];
    default: return ((const uint64_t *)p)[i];
  }
}
// a finished group -> its slot; a group without a valid value reports 0 everywhere
__device__ __forceinline__ void gba_store_group(const GbaTask &t, uint64_t g, const GbaAcc &a) {
  t.cnt[g] = a.cnt;
  if (t.want & GBA_SUM) t.sum[g] = a.cnt ? a.sum : 0ULL;
  if (t.want & GBA_MIN) gba_store_kind(t.mn, t.kind, g, a.cnt ? gba_unimage(a.mn, t.kind) : 0ULL);
  if (t.want & GBA_MAX) gba_store_kind(t.mx, t.kind, g, a.cnt ? gba_unimage(a.mx, t.kind) : 0ULL);
}

// heads has one word behind the last tile's (zero), so that the look-ahead below needs no bound.  head_rows (may be null): row of
// every group's first position, the index column of the key outputs.
__global__ __launch_bounds__(GBA_TILE) void gba_reduce(const uint32_t *__restrict__ perm, const unsigned long long *__restrict__ heads,
                                                       const uint32_t *__restrict__ tile_first, uint32_t n, GbaBatch b, int32_t *__restrict__ head_rows) {
  __shared__ uint32_t wheads[GBA_WAVES];
  __shared__ GbaAcc wtail[GBA_BATCH][GBA_WAVES];
  const int lane = lane_id();
  const uint32_t tile = blockIdx.x, w = threadIdx.x / WAVE;
  const uint64_t i = (uint64_t)tile * GBA_TILE + threadIdx.x;
  const bool live = i < n;
  const unsigned long long word = heads[(uint64_t)tile * GBA_WAVES + w];
  const bool head_next = lane < WAVE - 1 ? (word >> (lane + 1)) & 1ULL : heads[(uint64_t)tile * GBA_WAVES + w + 1] & 1ULL;
  const bool tail = live && (i == (uint64_t)n - 1 || head_next);                 // the last position of its group
  const bool tile_end = live && !tail && threadIdx.x == GBA_TILE - 1;            // ... of its tile, the group running on
  const unsigned long long below = word & ((2ULL << lane) - 1ULL);               // heads at or before this lane
  const int start = below ? 63 - __clzll((long long)below) : 0;                  // where this lane's segment begins within the wave
  const bool wave_open = below == 0ULL;                                          // ... or before the wave
  if (lane == 0) wheads[w] = (uint32_t)__popcll(word);
  const uint32_t row = live ? perm[i] : 0u;

  // the gathers of the batch, all issued before the first use
  bool ok[GBA_BATCH];
  uint64_t raw[GBA_BATCH];
#pragma unroll
  for (int k = 0; k < GBA_BATCH; ++k) {
    ok[k] = false;
    raw[k] = 0;
    if (k < b.n) {
      const GbaTask &t = b.t[k];
      ok[k] = live && (!t.valid || bit_is_set(t.valid, row));
      if (ok[k] && t.data) raw[k] = t.kind == K_F32 ? (uint64_t)((const uint32_t *)t.data)[row] : ob_load_int(t.data, t.kind, row);
    }
  }

  GbaAcc acc[GBA_BATCH];
#pragma unroll
  for (int k = 0; k < GBA_BATCH; ++k) {
    if (k < b.n) {
      const GbaTask &t = b.t[k];
      const bool isf = gba_is_float(t.kind);
      GbaAcc a = gba_identity(isf);
      if (ok[k]) {
        a.cnt = 1;
        a.sum = t.kind == K_F32 ? (uint64_t)__double_as_longlong((double)__uint_as_float((uint32_t)raw[k])) : raw[k];
        a.mn = a.mx = isf ? ob_float_image_of(raw[k], t.kind) : raw[k] ^ 0x8000000000000000ULL;
      }
#pragma unroll
      for (int d = 1; d < WAVE; d <<= 1) {
        GbaAcc l = a;
        l.cnt = __shfl_up(a.cnt, d, WAVE);
        if (t.want & GBA_SUM) l.sum = __shfl_up((unsigned long long)a.sum, d, WAVE);
        if (t.want & GBA_MIN) l.mn = __shfl_up((unsigned long long)a.mn, d, WAVE);
        if (t.want & GBA_MAX) l.mx = __shfl_up((unsigned long long)a.mx, d, WAVE);
        if (lane - d >= start) a = gba_fold(l, a, t.want, isf);
      }
      if (lane == WAVE - 1) wtail[k][w] = a;             // the fold of the wave's last segment (of the whole wave when it has no head)
      acc[k] = a;
    }
  }
  __syncthreads();

  uint32_t rank = (uint32_t)__popcll(below);             // heads of the tile at or before this position
  for (uint32_t v = 0; v < w; ++v) rank += wheads[v];
  const uint64_t slot = (uint64_t)tile_first[tile] + rank - 1;
  if (head_rows && live && ((word >> lane) & 1ULL)) head_rows[slot] = (int32_t)row;
#pragma unroll
  for (int k = 0; k < GBA_BATCH; ++k) {
    if (k < b.n) {
      const GbaTask &t = b.t[k];
      const bool isf = gba_is_float(t.kind);
      GbaAcc a = acc[k];
      if (wave_open) {                                   // what the earlier waves hold of this lane's segment, in wave order
        GbaAcc left = gba_identity(isf);
        for (uint32_t v = 0; v < w; ++v) left = wheads[v] ? wtail[k][v] : gba_fold(left, wtail[k][v], t.want, isf);
        a = gba_fold(left, a, t.want, isf);
      }
      if (tail && rank > 0) gba_store_group(t, slot, a);
      else if (tail || tile_end) t.carry[2 * (uint64_t)tile + (rank > 0 ? 1 : 0)] = a;
    }
  }
}

// blockIdx.y = task of the batch, one WAVE per tile.  Tile t has a BACK record when it holds a head and the next tile does not begin
// with one; its group then runs through the FRONT records of the tiles behind it, up to the first tile that holds a head.  The wave
// walks them 64 tiles at a time: every lane loads one record (the fold of nothing behind the end of the walk), an ordered tree
// (__shfl_down, distance 1 .. 32) folds them into lane 0, and the chunks are folded left to right.  The chunks start at t + 1 and
// the tree has one shape, so the association order is the same on every call.
__global__ __launch_bounds__(256) void gba_fixup(const unsigned long long *__restrict__ heads, const uint32_t *__restrict__ nheads,
                                                 const uint32_t *__restrict__ tile_first, uint32_t ntiles, GbaBatch b) {
  const GbaTask &t = b.t[blockIdx.y];
  const int lane = lane_id();
  const uint64_t tile = ((uint64_t)blockIdx.x * 256 + threadIdx.x) / WAVE;
  if (tile + 1 >= ntiles || nheads[tile] == 0 || (heads[(tile + 1) * GBA_WAVES] & 1ULL)) return;      // (wave-uniform)
  const bool isf = gba_is_float(t.kind);
  GbaAcc a = t.carry[2 * tile + 1];
  for (uint64_t base = tile + 1; base < ntiles; base += WAVE) {
    const uint64_t u = base + lane;
    const bool in = u < ntiles;
    const bool starts = in && (heads[u * GBA_WAVES] & 1ULL);       // the group ended with the tile before: u has no FRONT record
    const bool closes = in && nheads[u] > 0;                       // the group ends inside u
    const unsigned long long stop = __ballot(!in || starts || closes);
    const int last = stop ? __ffsll((long long)stop) - 1 : WAVE;   // the lane at which the walk ends
    GbaAcc x = gba_identity(isf);
    if (lane < last || (lane == last && in && !starts)) x = t.carry[2 * u];
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
      GbaAcc r = x;
      r.cnt = __shfl_down(x.cnt, d, WAVE);
      if (t.want & GBA_SUM) r.sum = __shfl_down((unsigned long long)x.sum, d, WAVE);
      if (t.want & GBA_MIN) r.mn = __shfl_down((unsigned long long)x.mn, d, WAVE);
      if (t.want & GBA_MAX) r.mx = __shfl_down((unsigned long long)x.mx, d, WAVE);
      x = gba_fold(x, r, t.want, isf);                             // lane 0: the lanes [0, 2d) in order
    }
    GbaAcc chunk = x;
    chunk.cnt = __shfl(x.cnt, 0, WAVE);
    chunk.sum = __shfl((unsigned long long)x.sum, 0, WAVE);
    chunk.mn = __shfl((unsigned long long)x.mn, 0, WAVE);
    chunk.mx = __shfl((unsigned long long)x.mx, 0, WAVE);
    a = gba_fold(a, chunk, t.want, isf);
    if (stop) break;
  }
  if (lane == 0) gba_store_group(t, (uint64_t)tile_first[tile] + nheads[tile] - 1, a);
}

struct GbaFin {
  int op;                        // gdf_agg_op
  int kind;                      // of the value column
  const uint32_t *cnt;
  const void *src;               // the task's fold (may be dst)
  void *dst;
  unsigned long long *mask, *nulls;
};
struct GbaFinBatch {
  int n;
  GbaFin r[GBA_FIN_BATCH];
};

__global__ __launch_bounds__(256) void gba_finish(GbaFinBatch b, uint32_t G, uint32_t nwords) {
  const int lane = lane_id();
  const uint32_t wave = (blockIdx.x * 256 + threadIdx.x) / WAVE, nwaves = gridDim.x * (256 / WAVE);
  for (uint32_t w = wave; w < nwords; w += nwaves) {
    const uint64_t g = (uint64_t)w * WAVE + lane;
    const bool live = g < G;
    const unsigned long long live_mask = __ballot(live);
#pragma unroll
    for (int k = 0; k < GBA_FIN_BATCH; ++k) {
      if (k < b.n) {
        const GbaFin &r = b.r[k];
        const uint32_t c = live ? r.cnt[g] : 0u;
        if (live) {
          if (r.op == GDF_COUNT) {
            ((long long *)r.dst)[g] = (long long)c;
          } else if (r.op == GDF_AVG) {
            const uint64_t s = ((const uint64_t *)r.src)[g];
            const double sum = gba_is_float(r.kind) ? __longlong_as_double((long long)s) : (double)(long long)s;
            ((double *)r.dst)[g] = c ? sum / (double)c : 0.0;
          } else if (r.dst != r.src) {
            if (r.op == GDF_SUM) ((uint64_t *)r.dst)[g] = ((const uint64_t *)r.src)[g];
            else gba_store_kind(r.dst, r.kind, g, gba_load_kind(r.src, r.kind, g));
          }
        }
        const unsigned long long mword = __ballot(live && (r.op == GDF_COUNT || c > 0));
        if (lane == 0) {
          r.mask[w] = mword;
          const unsigned long long nulls = (unsigned long long)__popcll(live_mask & ~mword);
          if (nulls) atomicAdd(r.nulls, nulls);
        }
      }
    }
  }
}

static bool gba_sum_dtype(gdf_dtype t) { return t >= GDF_INT8 && t <= GDF_FLOAT64; }

static gdf_error group_by_agg(gdf_column **keys, int nkeys, gdf_column **values, int nvalues, const gdf_amd_agg *aggs, int naggs,
                              gdf_column **out_keys, gdf_column **out_aggs) {
  GDF_REQUIRE(keys != nullptr && nkeys > 0, GDF_DATASET_EMPTY);
  for (int c = 0; c < nkeys; ++c) GDF_REQUIRE(keys[c] != nullptr, GDF_DATASET_EMPTY);
  GDF_REQUIRE(nvalues >= 0 && (nvalues == 0 || values != nullptr), GDF_DATASET_EMPTY);
  for (int c = 0; c < nvalues; ++c) GDF_REQUIRE(values[c] != nullptr, GDF_DATASET_EMPTY);
  GDF_REQUIRE(aggs != nullptr && naggs > 0, GDF_DATASET_EMPTY);
  GDF_REQUIRE(out_keys != nullptr && out_aggs != nullptr, GDF_DATASET_EMPTY);
  for (int c = 0; c < nkeys; ++c) GDF_REQUIRE(out_keys[c] != nullptr, GDF_DATASET_EMPTY);
  for (int a = 0; a < naggs; ++a) GDF_REQUIRE(out_aggs[a] != nullptr, GDF_DATASET_EMPTY);
  GDF_REQUIRE(nkeys <= MAX_KEY_COLS, GDF_JOIN_TOO_MANY_COLUMNS);
  GDF_REQUIRE(nvalues <= GBA_MAX_VALUES && naggs <= GBA_MAX_AGGS, GDF_INVALID_API_CALL);
  const gdf_size_type rows = keys[0]->size;
  for (int c = 0; c < nkeys; ++c) GDF_REQUIRE(keys[c]->size == rows, GDF_COLUMN_SIZE_MISMATCH);
  for (int c = 0; c < nvalues; ++c) GDF_REQUIRE(values[c]->size == rows, GDF_COLUMN_SIZE_MISMATCH);
  for (int c = 0; c < nkeys; ++c) GDF_REQUIRE(elem_kind(keys[c]->dtype) != K_BAD, GDF_UNSUPPORTED_DTYPE);
  for (int a = 0; a < naggs; ++a) {
    const int op = aggs[a].op, col = aggs[a].column;
    GDF_REQUIRE(op == GDF_SUM || op == GDF_MIN || op == GDF_MAX || op == GDF_AVG || op == GDF_COUNT, GDF_UNSUPPORTED_METHOD);
    GDF_REQUIRE(col >= -1 && col < nvalues && (col >= 0 || op == GDF_COUNT), GDF_INVALID_API_CALL);
    if (col < 0) continue;
    const gdf_dtype vt = values[col]->dtype;
    GDF_REQUIRE((op == GDF_SUM || op == GDF_AVG) ? gba_sum_dtype(vt) : elem_kind(vt) != K_BAD, GDF_UNSUPPORTED_DTYPE);
  }
  GDF_REQUIRE(rows < (gdf_size_type)0x7fffffff, GDF_COLUMN_SIZE_TOO_BIG);
  if (rows > 0) {
    for (int c = 0; c < nkeys; ++c) GDF_REQUIRE(keys[c]->data != nullptr, GDF_DATASET_EMPTY);
    for (int a = 0; a < naggs; ++a) GDF_REQUIRE(aggs[a].column < 0 || values[aggs[a].column]->data != nullptr, GDF_DATASET_EMPTY);
  }

  // dtype and dtype_info of every aggregate output
  std::vector<gdf_dtype> agg_dtype((size_t)naggs);
  std::vector<gdf_dtype_extra_info> agg_info((size_t)naggs);
  for (int a = 0; a < naggs; ++a) {
    const int op = aggs[a].op, col = aggs[a].column;
    agg_info[a] = gdf_dtype_extra_info{};
    if (op == GDF_COUNT) agg_dtype[a] = GDF_INT64;
    else if (op == GDF_AVG) agg_dtype[a] = GDF_FLOAT64;
    else if (op == GDF_SUM) agg_dtype[a] = (values[col]->dtype == GDF_FLOAT32 || values[col]->dtype == GDF_FLOAT64) ? GDF_FLOAT64 : GDF_INT64;
    else { agg_dtype[a] = values[col]->dtype; agg_info[a] = values[col]->dtype_info; }
  }
  if (rows == 0) {
    for (int c = 0; c < nkeys; ++c) {
      gdf_column *o = out_keys[c];
      o->data = nullptr; o->valid = nullptr; o->size = 0; o->dtype = keys[c]->dtype; o->null_count = 0; o->dtype_info = keys[c]->dtype_info;
    }
    for (int a = 0; a < naggs; ++a) {
      gdf_column *o = out_aggs[a];
      o->data = nullptr; o->valid = nullptr; o->size = 0; o->dtype = agg_dtype[a]; o->null_count = 0; o->dtype_info = agg_info[a];
    }
    return GDF_SUCCESS;
  }
  const uint32_t n = (uint32_t)rows, ntiles = (n + GBA_TILE - 1) / GBA_TILE;

  // a. row order, b. heads and group numbers
  DevBuf perm, images, heads, nheads, tile_first;
  RMM_TRY(perm.alloc(sizeof(uint32_t) * (size_t)n));
  GDF_TRY(order_rows_ex(keys, nkeys, nullptr, n, perm.as<uint32_t>(), &images));
  KeyTable kt;
  GDF_TRY(make_key_table(keys, nkeys, &kt));
  const size_t nhwords = (size_t)ntiles * GBA_WAVES + 1;
  RMM_TRY(heads.alloc(sizeof(unsigned long long) * nhwords));
  RMM_TRY(nheads.alloc(sizeof(uint32_t) * ((size_t)ntiles + 1)));
  RMM_TRY(tile_first.alloc(sizeof(uint32_t) * ((size_t)ntiles + 1)));
  HIP_TRY(hipMemsetAsync(heads.as<unsigned long long>() + nhwords - 1, 0, sizeof(unsigned long long), stream0()));
  HIP_TRY(hipMemsetAsync(nheads.as<uint32_t>() + ntiles, 0, sizeof(uint32_t), stream0()));
  if (images.p)
    GDF_LAUNCH("gba_heads_images", gba_heads_images, dim3(ntiles), dim3(GBA_TILE), 0, stream0(), (const uint64_t *)images.as<uint64_t>(), n,
               heads.as<unsigned long long>(), nheads.as<uint32_t>());
  else
    GDF_LAUNCH("gba_heads", gba_heads, dim3(ntiles), dim3(GBA_TILE), 0, stream0(), kt, perm.as<uint32_t>(), n, heads.as<unsigned long long>(),
               nheads.as<uint32_t>());
  HIP_CHECK_LAST();
  GDF_TRY(scan_u32(nheads.as<uint32_t>(), tile_first.as<uint32_t>(), (size_t)ntiles + 1, false));
  uint32_t G = 0;
  HIP_TRY(read_back(&G, tile_first.as<uint32_t>() + ntiles, sizeof(G)));
  images.reset();                                      // (the kernels that read them are done)
  GDF_REQUIRE(G >= 1 && G <= n, GDF_C_ERROR);
  const uint32_t nwords = (G + 63) / 64;

  // the outputs, and the tasks: one per distinct value column, folding into the buffer of the first request that wants that fold
  std::vector<DevBuf> data((size_t)naggs), mask((size_t)naggs);
  for (int a = 0; a < naggs; ++a) {
    RMM_TRY(data[a].alloc((size_t)G * (size_t)dtype_width(agg_dtype[a])));
    RMM_TRY(mask[a].alloc((size_t)nwords * 8));
  }
  std::vector<GbaTask> tasks;
  std::vector<int> task_of_col((size_t)nvalues + 1, -1), task_of_agg((size_t)naggs);      // [nvalues]: COUNT(*)
  for (int a = 0; a < naggs; ++a) {
    const int op = aggs[a].op, col = aggs[a].column, slot = col < 0 ? nvalues : col;
    if (task_of_col[slot] < 0) {
      task_of_col[slot] = (int)tasks.size();
      GbaTask t{};
      if (col >= 0) {
        t.data = values[col]->data;
        t.valid = (const uint8_t *)values[col]->valid;
        t.kind = elem_kind(values[col]->dtype);
      } else {
        t.kind = K_I64;
      }
      tasks.push_back(t);
    }
    GbaTask &t = tasks[task_of_col[slot]];
    task_of_agg[a] = task_of_col[slot];
    if (op == GDF_SUM || op == GDF_AVG) t.want |= GBA_SUM;
    if (op == GDF_MIN && !t.mn) { t.want |= GBA_MIN; t.mn = data[a].p; }
    if (op == GDF_MAX && !t.mx) { t.want |= GBA_MAX; t.mx = data[a].p; }
  }
  // a task's sum lands in the buffer of a SUM request where there is one: AVG then divides out of it into its own.  With AVG requests
  // only, the first one's buffer takes the sum and is divided in place -- behind every other request (fin_order below).
  for (int pass = 0; pass < 2; ++pass)
    for (int a = 0; a < naggs; ++a) {
      GbaTask &t = tasks[task_of_agg[a]];
      if (aggs[a].op == (pass == 0 ? GDF_SUM : GDF_AVG) && !t.sum) t.sum = data[a].as<uint64_t>();
    }
  std::vector<int> fin_order;
  for (int pass = 0; pass < 2; ++pass)
    for (int a = 0; a < naggs; ++a) {
      const bool in_place_avg = aggs[a].op == GDF_AVG && tasks[task_of_agg[a]].sum == data[a].as<uint64_t>();
      if (in_place_avg == (pass == 1)) fin_order.push_back(a);
    }
  const size_t ntasks = tasks.size();
  std::vector<DevBuf> cnt(ntasks), carry(ntasks);
  for (size_t k = 0; k < ntasks; ++k) {
    RMM_TRY(cnt[k].alloc(sizeof(uint32_t) * (size_t)G));
    RMM_TRY(carry[k].alloc(sizeof(GbaAcc) * 2 * (size_t)ntiles));
    tasks[k].cnt = cnt[k].as<uint32_t>();
    tasks[k].carry = carry[k].as<GbaAcc>();
  }
  DevBuf head_rows, d_nulls;
  RMM_TRY(head_rows.alloc(sizeof(int32_t) * (size_t)G));
  RMM_TRY(d_nulls.alloc(sizeof(unsigned long long) * (size_t)naggs));
  HIP_TRY(hipMemsetAsync(d_nulls.p, 0, sizeof(unsigned long long) * (size_t)naggs, stream0()));

  // c. segmented multi-aggregate, d. carry fix-up
  for (size_t k0 = 0; k0 < ntasks; k0 += GBA_BATCH) {
    GbaBatch b{};
    b.n = (int)(ntasks - k0 < (size_t)GBA_BATCH ? ntasks - k0 : (size_t)GBA_BATCH);
    for (int k = 0; k < b.n; ++k) b.t[k] = tasks[k0 + k];
    GDF_LAUNCH("gba_reduce", gba_reduce, dim3(ntiles), dim3(GBA_TILE), 0, stream0(), (const uint32_t *)perm.as<uint32_t>(),
               (const unsigned long long *)heads.as<unsigned long long>(), (const uint32_t *)tile_first.as<uint32_t>(), n, b,
               k0 == 0 ? head_rows.as<int32_t>() : (int32_t *)nullptr);
    if (ntiles > 1)
      GDF_LAUNCH("gba_fixup", gba_fixup, dim3((ntiles + 256 / WAVE - 1) / (256 / WAVE), b.n), dim3(256), 0, stream0(), (const unsigned long long *)heads.as<unsigned long long>(),
                 (const uint32_t *)nheads.as<uint32_t>(), (const uint32_t *)tile_first.as<uint32_t>(), ntiles, b);
  }
  // e. finish
  const dim3 fgrid(stream_grid((size_t)nwords, 256 / WAVE * 4));
  for (int a0 = 0; a0 < naggs; a0 += GBA_FIN_BATCH) {
    GbaFinBatch f{};
    f.n = naggs - a0 < GBA_FIN_BATCH ? naggs - a0 : GBA_FIN_BATCH;
    for (int k = 0; k < f.n; ++k) {
      const int a = fin_order[a0 + k], op = aggs[a].op;
      const GbaTask &t = tasks[task_of_agg[a]];
      GbaFin &r = f.r[k];
      r.op = op;
      r.kind = t.kind;
      r.cnt = t.cnt;
      r.src = (op == GDF_SUM || op == GDF_AVG) ? (const void *)t.sum : op == GDF_MIN ? (const void *)t.mn : op == GDF_MAX ? (const void *)t.mx : nullptr;
      r.dst = data[a].p;
      r.mask = mask[a].as<unsigned long long>();
      r.nulls = d_nulls.as<unsigned long long>() + a;
    }
    GDF_LAUNCH("gba_finish", gba_finish, fgrid, dim3(256), 0, stream0(), f, G, nwords);
  }
  HIP_CHECK_LAST();
  std::vector<unsigned long long> nulls((size_t)naggs, 0ULL);
  HIP_TRY(read_back(nulls.data(), d_nulls.p, sizeof(unsigned long long) * (size_t)naggs));

  // the key outputs: the key columns' rows at every group's first position.  Nothing can fail behind this call.
  gdf_column idx{};
  idx.data = head_rows.p;
  idx.size = (gdf_size_type)G;
  idx.dtype = GDF_INT32;
  std::vector<gdf_column> key_out((size_t)nkeys);
  std::vector<gdf_column *> key_ptr((size_t)nkeys);
  for (int c = 0; c < nkeys; ++c) { key_out[c] = gdf_column{}; key_ptr[c] = &key_out[c]; }
  GDF_TRY(gather_columns(&idx, nkeys, keys, key_ptr.data()));
  for (int c = 0; c < nkeys; ++c) {
    gdf_column *o = out_keys[c];
    o->data = key_out[c].data; o->valid = key_out[c].valid; o->size = key_out[c].size; o->dtype = key_out[c].dtype;
    o->null_count = key_out[c].null_count; o->dtype_info = key_out[c].dtype_info;
  }
  for (int a = 0; a < naggs; ++a) {
    gdf_column *o = out_aggs[a];
    o->data = data[a].release();
    o->valid = static_cast<gdf_valid_type *>(mask[a].release());
    o->size = (gdf_size_type)G;
    o->dtype = agg_dtype[a];
    o->null_count = (gdf_size_type)nulls[a];
    o->dtype_info = agg_info[a];
  }
  return GDF_SUCCESS;
}

}  // namespace gdf_amd

extern "C" {

gdf_error gdf_amd_group_by_agg(gdf_column **keys, int nkeys, gdf_column **values, int nvalues, const gdf_amd_agg *aggs, int naggs,
                               gdf_column **out_keys, gdf_column **out_aggs) {
  return gdf_amd::guarded([&]() -> gdf_error { return gdf_amd::group_by_agg(keys, nkeys, values, nvalues, aggs, naggs, out_keys, out_aggs); });
}

}  // extern "C"
