// csv.hip -- read_csv: delimited text -> nullable columns (reference src/io/csv/csv-reader.cu; the contract is in include/gdf/gdf.h,
// the design, its byte accounting and its measurements in DESIGN.md §14).
//
// A RECORD is the bytes between two terminators; a TILE of the convert pass is R consecutive records, hence one contiguous byte range.
//   count    every lane takes 16 bytes with one vector load (the bytes in front of the first and behind the last 16-byte boundary
//            bytewise: nothing outside [d, d + n) is read) and marks its terminators -> tile_cnt[tile of 4 KiB]; every workgroup adds
//            what it counted to one 64-bit counter.
//   scan     scan_u32_async over the tile counts -> the number of the first terminator of every tile.
//   sync     the host reads the terminator count and the last byte (is there an unterminated tail record?) and allocates.
//   offsets  the count pass's walk again: terminator number k (tile base + rank from a wave prefix sum of the lanes' counts) at byte p
//            gives starts[k + 1] = p + 1.  In order, no atomics, no sort.  starts[0] = 0; starts[records] = n + 1 when the tail record
//            has no terminator, as if one stood at n: record r is always [starts[r], starts[r + 1] - 1).
//   convert  one workgroup per tile, lane i parses record i.  A tile whose byte range fits CSV_LDS is staged with coalesced 16-byte
//            loads and parsed out of LDS; any other (long records) walks global memory -- a workgroup-uniform choice.  Lane i stores
//            row i of every column; a wave's 64 validity bits of a column are one ballot and one 8-byte store (a tile starts on a
//            multiple of 64 rows, so no two waves share a word); the null count is one popcount and one atomic add per wave and column,
//            spread over CSV_NULL_SLOTS copies of the counters.
#include "internal.h"
#include "launch.h"
#include "hash.cuh"
#include "gdf/gdf_amd_ext.h"

#include <cstdlib>
#include <cstring>
#include <vector>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

namespace gdf_amd {

struct CsvCol {            // the column table lives in device memory: num_cols is unbounded
  void               *data;
  unsigned long long *valid;     // 8-byte words, one per 64 rows
  int                 dtype;     // gdf_dtype
  int                 pad;
};
struct CsvOpts {
  unsigned char delim, term;
  bool skipinitialspace, dayfirst;
};
struct CsvHead {           // the device counters every pass shares; the uint32 null counts follow it, CSV_NULL_SLOTS per column
  unsigned long long nterm;
  uint32_t last_byte;
  uint32_t unstaged;
};

constexpr int CSV_SCAN_THREADS = 256;
constexpr int CSV_SCAN_TILE = CSV_SCAN_THREADS * 16;     // bytes per tile of the count / offsets passes
constexpr int CSV_R = 128;                               // records per tile = threads per workgroup of the convert pass
// Staging bytes of one convert workgroup.  32 KiB: five workgroups (ten waves) share a CU's 160 KiB -- the parse is a byte-serial
// walk per lane, so it lives on waves to switch between, and 64 KiB would leave a CU with four -- and tiles of records up to 255
// bytes on average (the mortgage schema's are ~120) still stage.
constexpr int CSV_LDS = 32 * 1024;
constexpr uint32_t CSV_HASH_SEED = 33;
// Copies of the null counters; a workgroup adds to copy blockIdx % CSV_NULL_SLOTS and the host sums them.  With one copy every wave
// of the grid queued on the same few addresses, one atomic per wave and column: 11.9 of 12.2 ms of a 4 M row mortgage file.
constexpr int CSV_NULL_SLOTS = 64;

// ---- count / offsets -----------------------------------------------------------------------------------------------------------
// bit i: byte pos0 + i is a terminator.  d + pos0 is 16-byte aligned; positions outside [0, n) are not read.
__device__ __forceinline__ uint32_t csv_term_bits(const unsigned char *__restrict__ d, int64_t n, int64_t pos0, unsigned char term) {
  uint32_t m = 0;
  if (pos0 >= 0 && pos0 + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4 *>(d + pos0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) m |= (uint32_t)(((w[i >> 2] >> (8 * (i & 3))) & 0xffu) == term) << i;
  } else {
    for (int i = 0; i < 16; ++i) {
      const int64_t p = pos0 + i;
      if (p >= 0 && p < n && d[p] == term) m |= 1u << i;
    }
  }
  return m;
}

// off: d's distance from the 16-byte boundary below it.  EMIT == false: tile_cnt[tile] = terminators of the tile, *head counts them
// all and learns the last byte.  EMIT == true: tile_cnt holds the exclusive scan of those counts and starts[] is written.
template <bool EMIT>
__global__ __launch_bounds__(CSV_SCAN_THREADS) void csv_scan(const unsigned char *__restrict__ d, int64_t n, int off, unsigned char term,
                                                              int64_t ntiles, uint32_t *__restrict__ tile_cnt, CsvHead *head,
                                                              int64_t *__restrict__ starts, int64_t nterm) {
  __shared__ uint32_t s_wave[CSV_SCAN_THREADS / WAVE];
  const int tid = (int)threadIdx.x, lane = lane_id(), wv = tid / WAVE;
  unsigned long long mine = 0;
  if (blockIdx.x == 0 && tid == 0) {
    if (EMIT) {
      starts[0] = 0;
      starts[nterm + 1] = n + 1;
    } else {
      head->last_byte = d[n - 1];
    }
  }
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {          // (workgroup-uniform)
    const int64_t pos0 = (tile * CSV_SCAN_THREADS + tid) * 16 - off;
    const uint32_t m = csv_term_bits(d, n, pos0, term);
    const uint32_t cnt = (uint32_t)__popc(m);
    const uint32_t incl = wave_scan_incl(cnt);
    if (lane == WAVE - 1) s_wave[wv] = incl;
    block_sync();
    if (!EMIT) {
      if (tid == 0) {
        const uint32_t t = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        tile_cnt[tile] = t;
        mine += t;
      }
    } else {
      int64_t k = (int64_t)tile_cnt[tile] + waves_before_sum<CSV_SCAN_THREADS / WAVE>(s_wave, (uint32_t)tid) + incl - cnt;
      for (uint32_t mm = m; mm; mm &= mm - 1) starts[++k] = pos0 + (__ffs((int)mm) - 1) + 1;
    }
    block_sync();                                                              // (the next tile rewrites s_wave)
  }
  if (!EMIT && tid == 0 && mine) atomicAdd(&head->nterm, mine);
}

// ---- fields --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool csv_digit(unsigned c) { return c - '0' < 10u; }

// optional sign, digits, a ',' only between two digits; a value outside [lo, hi] is no literal
__device__ __forceinline__ bool csv_parse_int(const unsigned char *s, const unsigned char *e, int64_t lo, int64_t hi, int64_t *out) {
  bool neg = false;
  if (s < e && (*s == '+' || *s == '-')) neg = *s++ == '-';
  uint64_t mag = 0;
  bool over = false, prev_digit = false;
  for (; s < e; ++s) {
    const unsigned c = *s;
    if (csv_digit(c)) {
      if (mag > 922337203685477580ull) over = true;                            // (2^63 / 10: mag * 10 + 9 still fits 64 bits)
      else mag = mag * 10 + (c - '0');
      prev_digit = true;
    } else if (c == ',' && prev_digit) {
      prev_digit = false;
    } else {
      return false;
    }
  }
  if (!prev_digit || over || mag > (neg ? 1ull << 63 : (1ull << 63) - 1)) return false;
  const int64_t v = (int64_t)(neg ? 0 - mag : mag);
  if (v < lo || v > hi) return false;
  *out = v;
  return true;
}

__constant__ double CSV_P1[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                  1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};      // exact
__constant__ double CSV_P22[15] = {1e0,   1e22,  1e44,  1e66,  1e88,  1e110, 1e132, 1e154,
                                   1e176, 1e198, 1e220, 1e242, 1e264, 1e286, 1e308};                      // correctly rounded from 1e44 on

// [+-]? (digits [. digits*] | . digits) ([eE] [+-]? digits)?, a ',' only between two digits of the integer part.  The first 19
// significant digits -> m, the rest into the decimal exponent; gdf.h has the rounding argument.
__device__ __forceinline__ bool csv_parse_float(const unsigned char *s, const unsigned char *e, double *out) {
  bool neg = false;
  if (s < e && (*s == '+' || *s == '-')) neg = *s++ == '-';
  uint64_t m = 0;
  int nd = 0;
  int64_t e10 = 0;
  bool any = false, prev_digit = false;
  for (; s < e; ++s) {
    const unsigned c = *s;
    if (csv_digit(c)) {
      any = prev_digit = true;
      if (nd == 19) ++e10;
      else if (m | (c - '0')) { m = m * 10 + (c - '0'); ++nd; }
    } else if (c == ',' && prev_digit) {
      prev_digit = false;
    } else {
      break;
    }
  }
  if (any && !prev_digit) return false;
  if (s < e && *s == '.') {
    for (++s; s < e && csv_digit(*s); ++s) {
      const unsigned c = *s;
      any = true;
      if (nd == 19) continue;
      --e10;
      if (m | (c - '0')) { m = m * 10 + (c - '0'); ++nd; }
    }
  }
  if (!any) return false;
  if (s < e && (*s == 'e' || *s == 'E')) {
    bool eneg = false;
    if (++s < e && (*s == '+' || *s == '-')) eneg = *s++ == '-';
    if (s == e) return false;
    // x saturates near 4e18, e10 counts bytes of a buffer of at most INT64_MAX / 2: the sum fits and the clamp comes after it
    int64_t x = 0;
    for (; s < e; ++s) {
      if (!csv_digit(*s)) return false;
      if (x < 400000000000000000ll) x = x * 10 + (int64_t)(*s - '0');
    }
    e10 += eneg ? -x : x;
  }
  if (s != e) return false;
  double x = 0.0;
  if (m != 0) {
    if (e10 > 308) {
      x = __longlong_as_double(0x7ff0000000000000ll);                          // m >= 1: at least 1e309
    } else if (e10 >= -400) {                                                  // (below: under 1e19 * 1e-401, rounds to 0)
      x = (double)m;
      int a = (int)(e10 < 0 ? -e10 : e10);
      if (e10 < 0) {
        if (a > 308) { x /= CSV_P22[14]; a -= 308; }
        x /= CSV_P1[a % 22];
        x /= CSV_P22[a / 22];
      } else {
        x *= CSV_P22[a / 22];                                                  // (never beyond the value itself: no early overflow)
        x *= CSV_P1[a % 22];
      }
    }
  }
  *out = neg ? -x : x;
  return true;
}

// up to maxd digits -> *v; returns how many
__device__ __forceinline__ int csv_digits(const unsigned char *&s, const unsigned char *e, int maxd, int *v) {
  int n = 0, x = 0;
  for (; s < e && n < maxd && csv_digit(*s); ++s, ++n) x = x * 10 + (int)(*s - '0');
  *v = x;
  return n;
}

// days from 1970-01-01 in the proleptic Gregorian calendar (eras of 400 years, the year starting in March)
__device__ __forceinline__ int64_t csv_days(int y, int mo, int d) {
  y -= mo <= 2;
  const int era = (y >= 0 ? y : y - 399) / 400;
  const int yoe = y - era * 400;
  const int doy = (153 * (mo + (mo > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const int doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return (int64_t)era * 146097 + doe - 719468;
}

// date [(T | one space) time] -> milliseconds; with_time == false: a date alone
__device__ __forceinline__ bool csv_parse_date(const unsigned char *s, const unsigned char *e, bool dayfirst, bool with_time, int64_t *days,
                                               int64_t *ms) {
  int a, b, c = 0;
  const int na = csv_digits(s, e, 4, &a);
  if (na == 0 || na == 3 || s == e) return false;
  const unsigned sep = *s++;
  if (sep != '/' && sep != '-') return false;
  const int nb = csv_digits(s, e, 4, &b);
  if (nb == 0) return false;
  int nc = 0;
  if (s < e && *s == sep) {
    ++s;
    nc = csv_digits(s, e, 4, &c);
    if (nc == 0) return false;
  }
  int y, mo, d = 1;
  if (na == 4) {                                  // Y-M or Y-M-D
    if (nb > 2 || nc > 2) return false;
    y = a; mo = b;
    if (nc) d = c;
  } else if (nc) {                                // M-D-Y, or D-M-Y with dayfirst
    if (nb > 2 || nc != 4) return false;
    y = c; mo = dayfirst ? b : a; d = dayfirst ? a : b;
  } else {                                        // M-Y
    if (nb != 4) return false;
    y = b; mo = a;
  }
  if (y < 1 || mo < 1 || mo > 12 || d < 1) return false;
  const bool leap = (y % 4 == 0 && y % 100 != 0) || y % 400 == 0;
  const int dim = mo == 2 ? (leap ? 29 : 28) : 30 + ((0xAD5 >> (mo - 1)) & 1);               // Jan Mar May Jul Aug Oct Dec
  if (d > dim) return false;
  int h = 0, mi = 0, sec = 0;
  if (s < e) {
    if (!with_time || (*s != 'T' && *s != ' ')) return false;
    ++s;
    const int nh = csv_digits(s, e, 2, &h);
    if (nh == 0 || s == e || *s++ != ':') return false;
    if (csv_digits(s, e, 2, &mi) == 0) return false;
    if (s < e && *s == ':') {
      ++s;
      if (csv_digits(s, e, 2, &sec) == 0) return false;
    }
    if (s < e) {                                  // [space] AM | PM, either case
      if (*s == ' ') ++s;
      if (e - s != 2 || (s[1] | 0x20) != 'm') return false;
      const unsigned ap = s[0] | 0x20;
      if ((ap != 'a' && ap != 'p') || h < 1 || h > 12) return false;
      h = h % 12 + (ap == 'p' ? 12 : 0);          // 12 AM is hour 0, 12 PM hour 12
    }
    if (h > 23 || mi > 59 || sec > 59) return false;
  }
  *days = csv_days(y, mo, d);
  *ms = *days * 86400000ll + (int64_t)(h * 3600 + mi * 60 + sec) * 1000;
  return true;
}

// MurmurHash3 x86_32 over the bytes [s, e)
__device__ __forceinline__ uint32_t csv_murmur(const unsigned char *s, const unsigned char *e, uint32_t seed) {
  uint32_t h = seed;
  const uint32_t len = (uint32_t)(e - s);
  for (; e - s >= 4; s += 4) h = murmur_block(h, (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24);
  uint32_t k = 0;
  const int r = (int)(e - s);
  if (r == 3) k ^= (uint32_t)s[2] << 16;
  if (r >= 2) k ^= (uint32_t)s[1] << 8;
  if (r >= 1) {
    k ^= s[0];
    k *= 0xcc9e2d51u; k = rotl32(k, 15); k *= 0x1b873593u;
    h ^= k;
  }
  return fmix32(h ^ len);
}

// ---- convert -------------------------------------------------------------------------------------------------------------------
// The record [s, e) of this lane -> row `row` of every column.  Every lane of the wave calls it (a lane without a row has live ==
// false): the column loop is wave-uniform and ends in a ballot.  word: the wave's index into the masks, -1 when it has no rows.
__device__ __forceinline__ void csv_record(const unsigned char *s, const unsigned char *e, bool live, int64_t row, int64_t word,
                                           const CsvCol *__restrict__ cols, int ncols, CsvOpts o, uint32_t *__restrict__ nulls) {
  if (o.term == '\n' && e > s && e[-1] == '\r') --e;
  const unsigned long long live_mask = __ballot(live);
  bool more = live;                                                            // a field starts at s
  for (int c = 0; c < ncols; ++c) {
    const CsvCol col = cols[c];
    const unsigned char *fs = s, *fe = s;
    if (more) {
      while (fe < e && *fe != o.delim) ++fe;
      more = fe < e;
      s = fe + 1;
    }
    bool ok = false;
    uint64_t bits = 0;
    if (col.dtype == GDF_CATEGORY) {
      if (o.skipinitialspace) while (fs < fe && *fs == ' ') ++fs;
      if (fs < fe) { ok = true; bits = csv_murmur(fs, fe, CSV_HASH_SEED); }
    } else {
      while (fs < fe && *fs == ' ') ++fs;
      while (fe > fs && fe[-1] == ' ') --fe;
      if (fs < fe) {
        int64_t v = 0, days = 0;
        double x = 0.0;
        switch (col.dtype) {
          case GDF_INT16: ok = csv_parse_int(fs, fe, INT16_MIN, INT16_MAX, &v); bits = (uint64_t)v; break;
          case GDF_INT32: ok = csv_parse_int(fs, fe, INT32_MIN, INT32_MAX, &v); bits = (uint64_t)v; break;
          case GDF_INT64: case GDF_TIMESTAMP: ok = csv_parse_int(fs, fe, INT64_MIN, INT64_MAX, &v); bits = (uint64_t)v; break;
          case GDF_FLOAT32: ok = csv_parse_float(fs, fe, &x); bits = __float_as_uint((float)x); break;
          case GDF_FLOAT64: ok = csv_parse_float(fs, fe, &x); bits = (uint64_t)__double_as_longlong(x); break;
          case GDF_DATE32: ok = csv_parse_date(fs, fe, o.dayfirst, false, &days, &v); bits = (uint64_t)days; break;
          default: ok = csv_parse_date(fs, fe, o.dayfirst, true, &days, &v); bits = (uint64_t)v; break;       // GDF_DATE64
        }
        if (!ok) bits = 0;
      }
    }
    if (live) {
      switch (col.dtype) {
        case GDF_INT16: ((uint16_t *)col.data)[row] = (uint16_t)bits; break;
        case GDF_INT32: case GDF_FLOAT32: case GDF_DATE32: case GDF_CATEGORY: ((uint32_t *)col.data)[row] = (uint32_t)bits; break;
        default: ((uint64_t *)col.data)[row] = bits; break;
      }
    }
    const unsigned long long valid = __ballot(ok);
    if (word >= 0 && lane_id() == 0) {
      col.valid[word] = valid;
      const uint32_t nn = (uint32_t)__popcll(live_mask & ~valid);
      if (nn) atomicAdd(&nulls[c], nn);
    }
  }
}

// rows [blockIdx.x * CSV_R, + CSV_R) of the result = records first_rec + that
__global__ __launch_bounds__(CSV_R) void csv_convert(const unsigned char *__restrict__ d, int64_t n, const int64_t *__restrict__ starts,
                                                      int64_t first_rec, int64_t rows, const CsvCol *__restrict__ cols, int ncols, CsvOpts o,
                                                      int no_stage, CsvHead *head, uint32_t *__restrict__ nulls) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = (int)threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * CSV_R, r1 = r0 + CSV_R < rows ? r0 + CSV_R : rows;
  const int64_t b0 = starts[first_rec + r0], b1 = starts[first_rec + r1] - 1;  // the tile's bytes; b1 <= n
  const int64_t row = r0 + tid, wrow = r0 + (tid / WAVE) * WAVE;
  const bool live = row < rows;
  const int64_t word = wrow < rows ? wrow / WAVE : -1;
  uint32_t *my_nulls = nulls + (size_t)(blockIdx.x % CSV_NULL_SLOTS) * (size_t)ncols;
  int64_t rs = b0, re = b0;
  if (live) {
    rs = starts[first_rec + row];
    re = starts[first_rec + row + 1] - 1;
  }
  if (!no_stage && b1 - b0 + 32 <= CSV_LDS) {                                  // (workgroup-uniform)
    // the image starts at the 16-byte boundary below d + b0: a 16-byte vector of the image is an aligned vector of the buffer
    const int off = (int)((uintptr_t)(d + b0) & 15);
    const int64_t p0 = b0 - off;
    const int total = off + (int)(b1 - b0);
    for (int j = tid * 16; j < total; j += CSV_R * 16) {
      const int64_t p = p0 + j;
      if (p >= 0 && p + 16 <= n) {
        *reinterpret_cast<uint4 *>(smem + j) = *reinterpret_cast<const uint4 *>(d + p);
      } else {
        for (int i = 0; i < 16; ++i) smem[j + i] = (p + i >= 0 && p + i < n) ? d[p + i] : (unsigned char)0;
      }
    }
    block_sync();
    csv_record(smem + (off + (int)(rs - b0)), smem + (off + (int)(re - b0)), live, row, word, cols, ncols, o, my_nulls);
  } else {
    if (tid == 0) atomicAdd(&head->unstaged, 1u);
    csv_record(d + rs, d + re, live, row, word, cols, ncols, o, my_nulls);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
static bool csv_dtype_of(const char *s, gdf_dtype *out) {
  static const struct { const char *name; gdf_dtype dtype; } table[] = {
      {"str", GDF_CATEGORY},    {"category", GDF_CATEGORY}, {"date", GDF_DATE64},    {"date64", GDF_DATE64},
      {"date32", GDF_DATE32},   {"timestamp", GDF_TIMESTAMP}, {"float", GDF_FLOAT32}, {"float32", GDF_FLOAT32},
      {"float64", GDF_FLOAT64}, {"double", GDF_FLOAT64},    {"short", GDF_INT16},    {"int", GDF_INT32},
      {"int32", GDF_INT32},     {"int64", GDF_INT64},       {"long", GDF_INT64}};
  for (const auto &t : table)
    if (std::strcmp(s, t.name) == 0) { *out = t.dtype; return true; }
  return false;
}

// every argument error that does not depend on the bytes, in the order of gdf.h
static gdf_error csv_check(const csv_read_arg *args, std::vector<gdf_dtype> *dtypes) {
  GDF_REQUIRE(args, GDF_INVALID_API_CALL);
  GDF_REQUIRE(args->num_cols > 0 && args->names && args->dtype, GDF_INVALID_API_CALL);
  for (int c = 0; c < args->num_cols; ++c) GDF_REQUIRE(args->names[c] && args->dtype[c], GDF_INVALID_API_CALL);
  GDF_REQUIRE(args->skiprows >= 0 && args->skipfooter >= 0, GDF_INVALID_API_CALL);
  dtypes->resize((size_t)args->num_cols);
  for (int c = 0; c < args->num_cols; ++c) GDF_REQUIRE(csv_dtype_of(args->dtype[c], &(*dtypes)[c]), GDF_UNSUPPORTED_DTYPE);
  return GDF_SUCCESS;
}

static void csv_free_columns(gdf_column **cols, int n) {
  if (!cols) return;
  for (int c = 0; c < n; ++c) {
    if (!cols[c]) continue;
    if (cols[c]->data) (void)rmmFree(cols[c]->data, (cudaStream_t)0);
    if (cols[c]->valid) (void)rmmFree(cols[c]->valid, (cudaStream_t)0);
    std::free(cols[c]->col_name);
    std::free(cols[c]);
  }
  std::free(cols);
}

struct CsvResult {         // a result under construction: everything is released unless it is handed over
  gdf_column **cols = nullptr;
  int n = 0;
  ~CsvResult() { csv_free_columns(cols, n); }
};

static gdf_error csv_read_device(const unsigned char *d, int64_t n, csv_read_arg *args, const std::vector<gdf_dtype> &dtypes) {
  const int ncols = args->num_cols;
  const unsigned char term = (unsigned char)args->lineterminator;
  const CsvOpts opts{(unsigned char)(args->delim_whitespace ? ' ' : args->delimiter), term, args->skipinitialspace, args->dayfirst};
  const size_t counters_bytes = sizeof(CsvHead) + sizeof(uint32_t) * (size_t)ncols * CSV_NULL_SLOTS;

  DevBuf counters, tiles, scan_scratch, starts, d_table;
  const int off = (int)((uintptr_t)d & 15);
  const int64_t ntiles = (off + n + CSV_SCAN_TILE - 1) / CSV_SCAN_TILE;
  const int scan_grid = stream_grid((size_t)ntiles, 1);
  int64_t nterm = 0, nrec = 0;
  if (n > 0) {
    RMM_TRY(counters.alloc(counters_bytes));
    RMM_TRY(tiles.alloc(sizeof(uint32_t) * (size_t)ntiles));
    HIP_TRY(hipMemsetAsync(counters.p, 0, counters_bytes, stream0()));
    GDF_LAUNCH("csv_count", csv_scan<false>, dim3(scan_grid), dim3(CSV_SCAN_THREADS), 0, stream0(), d, n, off, term, ntiles,
               tiles.as<uint32_t>(), counters.as<CsvHead>(), (int64_t *)nullptr, (int64_t)0);
    HIP_CHECK_LAST();
    GDF_TRY(scan_u32_async(tiles.as<uint32_t>(), tiles.as<uint32_t>(), (size_t)ntiles, false, &scan_scratch));
    CsvHead head{};
    HIP_TRY(read_back(&head, counters.p, sizeof(head)));                       // the one sync the allocations wait for
    const unsigned long long records = head.nterm + (head.last_byte != term ? 1u : 0u);
    GDF_REQUIRE(records <= (unsigned long long)INT32_MAX, GDF_COLUMN_SIZE_TOO_BIG);
    nterm = (int64_t)head.nterm;
    nrec = (int64_t)records;
  }
  const int64_t kept = nrec - args->skiprows - args->skipfooter;
  const int64_t rows = kept > 0 ? kept : 0;

  CsvResult res;
  res.cols = static_cast<gdf_column **>(std::calloc((size_t)ncols, sizeof(gdf_column *)));
  if (!res.cols) throw std::bad_alloc();
  res.n = ncols;
  std::vector<CsvCol> table((size_t)ncols);
  for (int c = 0; c < ncols; ++c) {
    gdf_column *col = res.cols[c] = static_cast<gdf_column *>(std::calloc(1, sizeof(gdf_column)));
    if (!col) throw std::bad_alloc();
    col->col_name = strdup(args->names[c]);
    if (!col->col_name) throw std::bad_alloc();
    col->size = (gdf_size_type)rows;
    col->dtype = dtypes[c];
    if (rows > 0) {
      const size_t w = dtypes[c] == GDF_CATEGORY ? 4 : (size_t)dtype_width(dtypes[c]);
      RMM_TRY(rmmAlloc(&col->data, (size_t)rows * w, (cudaStream_t)0));
      RMM_TRY(rmmAlloc((void **)&col->valid, (size_t)((rows + 63) / 64) * 8, (cudaStream_t)0));
    }
    table[c] = CsvCol{col->data, reinterpret_cast<unsigned long long *>(col->valid), (int)dtypes[c], 0};
  }

  long long unstaged = 0;
  if (rows > 0) {
    RMM_TRY(starts.alloc(sizeof(int64_t) * (size_t)(nterm + 2)));
    GDF_LAUNCH("csv_offsets", csv_scan<true>, dim3(scan_grid), dim3(CSV_SCAN_THREADS), 0, stream0(), d, n, off, term, ntiles,
               tiles.as<uint32_t>(), counters.as<CsvHead>(), starts.as<int64_t>(), nterm);
    HIP_CHECK_LAST();
    RMM_TRY(d_table.alloc(sizeof(CsvCol) * table.size()));
    HIP_TRY(hipMemcpyAsync(d_table.p, table.data(), sizeof(CsvCol) * table.size(), hipMemcpyHostToDevice, stream0()));
    HIP_TRY(hipStreamSynchronize(stream0()));                                  // `table` is pageable host memory
    uint32_t *nulls = reinterpret_cast<uint32_t *>(counters.as<unsigned char>() + sizeof(CsvHead));
    GDF_TRY(launch_lds("csv_convert", csv_convert, dim3((unsigned)((rows + CSV_R - 1) / CSV_R)), dim3(CSV_R), (size_t)CSV_LDS, d, n,
                       starts.as<int64_t>(), (int64_t)args->skiprows, rows, d_table.as<CsvCol>(), ncols, opts,
                       lab::path_on("GDF_CSV_NO_STAGE") ? 1 : 0, counters.as<CsvHead>(), nulls));
    HIP_CHECK_LAST();
    std::vector<unsigned char> back(counters_bytes);
    HIP_TRY(read_back(back.data(), counters.p, counters_bytes));               // null counts; the outputs are written
    CsvHead head;
    std::memcpy(&head, back.data(), sizeof(head));
    unstaged = head.unstaged;
    for (int slot = 0; slot < CSV_NULL_SLOTS; ++slot) {
      for (int c = 0; c < ncols; ++c) {
        uint32_t nn;
        std::memcpy(&nn, back.data() + sizeof(CsvHead) + sizeof(uint32_t) * ((size_t)slot * ncols + c), sizeof(nn));
        res.cols[c]->null_count += nn;
      }
    }
  }
  lab::note("csv.rows_per_tile", CSV_R);
  lab::note("csv.unstaged_tiles", unstaged);

  args->data = res.cols;
  args->num_cols_out = ncols;
  args->num_rows_out = (int)rows;
  res.cols = nullptr;
  return GDF_SUCCESS;
}

static gdf_error csv_read_buffer(const char *d_bytes, size_t num_bytes, csv_read_arg *args) {
  std::vector<gdf_dtype> dtypes;
  GDF_TRY(csv_check(args, &dtypes));
  GDF_REQUIRE(d_bytes || num_bytes == 0, GDF_INVALID_API_CALL);
  GDF_REQUIRE(num_bytes <= (size_t)INT64_MAX / 2, GDF_COLUMN_SIZE_TOO_BIG);
  return csv_read_device(reinterpret_cast<const unsigned char *>(d_bytes), (int64_t)num_bytes, args, dtypes);
}

struct CsvFile {           // descriptor and mapping of the input, closed on every way out
  int fd = -1;
  void *map = MAP_FAILED;
  size_t size = 0;
  ~CsvFile() {
    if (map != MAP_FAILED) (void)munmap(map, size);
    if (fd >= 0) (void)close(fd);
  }
};

static gdf_error csv_read_file(csv_read_arg *args) {
  std::vector<gdf_dtype> dtypes;
  GDF_TRY(csv_check(args, &dtypes));
  GDF_REQUIRE(args->file_path, GDF_FILE_ERROR);
  CsvFile f;
  f.fd = open(args->file_path, O_RDONLY | O_CLOEXEC);
  GDF_REQUIRE(f.fd >= 0, GDF_FILE_ERROR);
  struct stat st;
  GDF_REQUIRE(fstat(f.fd, &st) == 0 && S_ISREG(st.st_mode), GDF_FILE_ERROR);
  GDF_REQUIRE((unsigned long long)st.st_size <= (unsigned long long)INT64_MAX / 2, GDF_COLUMN_SIZE_TOO_BIG);
  DevBuf bytes;
  if (st.st_size > 0) {
    f.size = (size_t)st.st_size;
    f.map = mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, f.fd, 0);
    GDF_REQUIRE(f.map != MAP_FAILED, GDF_FILE_ERROR);
    RMM_TRY(bytes.alloc(f.size));
    HIP_TRY(hipMemcpy(bytes.p, f.map, f.size, hipMemcpyHostToDevice));
  }
  return csv_read_device(bytes.as<unsigned char>(), (int64_t)f.size, args, dtypes);
}

}  // namespace gdf_amd

extern "C" {

gdf_error read_csv(csv_read_arg *args) {
  return gdf_amd::guarded([&]() -> gdf_error { return gdf_amd::csv_read_file(args); });
}

gdf_error gdf_amd_read_csv_device(const char *d_bytes, size_t num_bytes, csv_read_arg *args) {
  return gdf_amd::guarded([&]() -> gdf_error { return gdf_amd::csv_read_buffer(d_bytes, num_bytes, args); });
}

gdf_error gdf_amd_read_csv_release(csv_read_arg *args) {
  return gdf_amd::guarded([&]() -> gdf_error {
    GDF_REQUIRE(args, GDF_INVALID_API_CALL);
    gdf_amd::csv_free_columns(args->data, args->num_cols_out);
    args->data = nullptr;
    args->num_cols_out = 0;
    args->num_rows_out = 0;
    return GDF_SUCCESS;
  });
}

}  // extern "C"
