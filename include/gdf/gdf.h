/*
 * gdf.h -- the C ABI of the MI355X-native libgdf.so (drop-in boundary).
 *
 * Every struct, enum value and entry point below is binary compatible with the
 * interface the reference's cffi bindings dlopen (citations are relative to
 * /root/reference/libgdf):
 *   structs / enums ......... include/gdf/cffi/types.h:1-221
 *   entry points ............ include/gdf/cffi/functions.h:1-785
 *   csv / csr argument PODs . include/gdf/cffi/io_types.h, convert_types.h
 * Layout facts pinned by tests/test_abi.py: sizeof(gdf_column)==56 with
 * data@0 valid@8 size@16 dtype@24 null_count@32 dtype_info@40 col_name@48;
 * sizeof(gdf_context)==20; enums are positional ints.
 *
 * The header is plain C (usable from cgo / JNI / ctypes / cffi) and is also
 * what the C++ host code in libgdf_amd/csrc compiles against.  The 182
 * element-wise operators are declared through gdf_elementwise.def.  Every
 * entry point does real work; none answers GDF_UNSUPPORTED_METHOD for
 * being out of scope.
 */
#ifndef GDF_AMD_GDF_H
#define GDF_AMD_GDF_H

#include <stddef.h>
#include <stdint.h>
#ifndef __cplusplus
#include <stdbool.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* the library itself is built with -fvisibility=hidden */
#endif

/* ---- scalar typedefs (types.h:3-8) ------------------------------------- */
typedef size_t         gdf_size_type;
typedef gdf_size_type  gdf_index_type;
typedef unsigned char  gdf_valid_type;   /* 8 rows per mask byte, LSB first   */
typedef long           gdf_date64;
typedef int            gdf_date32;
typedef int            gdf_category;

#define GDF_VALID_BITSIZE 8              /* gdf.h:10 in the reference        */

/* ---- column element types (types.h:15-29) ------------------------------ */
typedef enum {
  GDF_invalid = 0,
  GDF_INT8 = 1, GDF_INT16 = 2, GDF_INT32 = 3, GDF_INT64 = 4,
  GDF_FLOAT32 = 5, GDF_FLOAT64 = 6,
  GDF_DATE32 = 7,      /* int32 days since epoch                             */
  GDF_DATE64 = 8,      /* int64 ms since epoch                               */
  GDF_TIMESTAMP = 9,   /* int64, unit in dtype_info                          */
  GDF_CATEGORY = 10, GDF_STRING = 11,
  N_GDF_TYPES = 12
} gdf_dtype;

/* ---- status codes (types.h:39-64); names via gdf_error_get_name -------- */
typedef enum {
  GDF_SUCCESS = 0,
  GDF_CUDA_ERROR = 1,                /* a HIP runtime call failed            */
  GDF_UNSUPPORTED_DTYPE = 2,
  GDF_COLUMN_SIZE_MISMATCH = 3,
  GDF_COLUMN_SIZE_TOO_BIG = 4,
  GDF_DATASET_EMPTY = 5,
  GDF_VALIDITY_MISSING = 6,
  GDF_VALIDITY_UNSUPPORTED = 7,
  GDF_INVALID_API_CALL = 8,
  GDF_JOIN_DTYPE_MISMATCH = 9,
  GDF_JOIN_TOO_MANY_COLUMNS = 10,
  GDF_DTYPE_MISMATCH = 11,
  GDF_UNSUPPORTED_METHOD = 12,
  GDF_INVALID_AGGREGATOR = 13,
  GDF_INVALID_HASH_FUNCTION = 14,
  GDF_PARTITION_DTYPE_MISMATCH = 15,
  GDF_HASH_TABLE_INSERT_FAILURE = 16,
  GDF_UNSUPPORTED_JOIN_TYPE = 17,
  GDF_C_ERROR = 18,
  GDF_FILE_ERROR = 19,
  GDF_MEMORYMANAGER_ERROR = 20,
  GDF_UNDEFINED_NVTX_COLOR = 21,
  GDF_NULL_NVTX_NAME = 22,
  N_GDF_ERRORS = 23
} gdf_error;

typedef enum { GDF_HASH_MURMUR3 = 0, GDF_HASH_IDENTITY = 1 } gdf_hash_func;   /* types.h:66-69 */

typedef enum {                                                               /* types.h:71-77 */
  TIME_UNIT_NONE = 0, TIME_UNIT_s, TIME_UNIT_ms, TIME_UNIT_us, TIME_UNIT_ns
} gdf_time_unit;

typedef struct { gdf_time_unit time_unit; } gdf_dtype_extra_info;            /* types.h:79-82 */

/* ---- the Arrow-layout column descriptor (types.h:84-92) ----------------
 * A host-side POD; `data` and `valid` are DEVICE pointers.  valid==NULL means
 * "no nulls".  Bit i of the mask is (valid[i/8] >> (i%8)) & 1, 1 = not null
 * (include/gdf/utils.h:9-16). */
typedef struct gdf_column_ {
  void                 *data;
  gdf_valid_type       *valid;
  gdf_size_type         size;
  gdf_dtype             dtype;
  gdf_size_type         null_count;
  gdf_dtype_extra_info  dtype_info;
  char                 *col_name;      /* host string, never touched here    */
} gdf_column;

typedef enum { GDF_SORT = 0, GDF_HASH = 1, N_GDF_METHODS = 2 } gdf_method;   /* types.h:101-105 */

typedef enum {                                                               /* types.h:107-114 */
  GDF_QUANT_LINEAR = 0, GDF_QUANT_LOWER, GDF_QUANT_HIGHER, GDF_QUANT_MIDPOINT,
  GDF_QUANT_NEAREST, N_GDF_QUANT_METHODS
} gdf_quantile_method;

typedef enum {                                                               /* types.h:123-131 */
  GDF_SUM = 0, GDF_MIN, GDF_MAX, GDF_AVG, GDF_COUNT, GDF_COUNT_DISTINCT, N_GDF_AGG_OPS
} gdf_agg_op;

typedef enum {                                                               /* types.h:142-153 */
  GDF_GREEN = 0, GDF_BLUE, GDF_YELLOW, GDF_PURPLE, GDF_CYAN, GDF_RED, GDF_WHITE,
  GDF_DARK_GREEN, GDF_ORANGE, GDF_NUM_COLORS
} gdf_color;

/* ---- per-call options (types.h:161-167) -------------------------------- */
typedef struct gdf_context_ {
  int        flag_sorted;        /* input already sorted? (unused by HASH)   */
  gdf_method flag_method;        /* GDF_HASH selects everything in this lib  */
  int        flag_distinct;
  int        flag_sort_result;   /* HASH group-by: 1 = sort output by key    */
  int        flag_sort_inplace;
} gdf_context;

/* opaque handles of out-of-scope subsystems (types.h:169-182) */
typedef struct _OpaqueIpcParser              gdf_ipc_parser_type;
typedef struct _OpaqueRadixsortPlan          gdf_radixsort_plan_type;
typedef struct _OpaqueSegmentedRadixsortPlan gdf_segmented_radixsort_plan_type;

typedef enum { GDF_ORDER_ASC = 0, GDF_ORDER_DESC } order_by_type;            /* types.h:183-186 */

typedef enum {                                                               /* types.h:188-195 */
  GDF_EQUALS = 0, GDF_NOT_EQUALS, GDF_LESS_THAN, GDF_LESS_THAN_OR_EQUALS,
  GDF_GREATER_THAN, GDF_GREATER_THAN_OR_EQUALS
} gdf_comparison_operator;

typedef enum { GDF_WINDOW_RANGE = 0, GDF_WINDOW_ROW } window_function_type;  /* types.h:197-200 */
typedef enum {                                                               /* types.h:202-210 */
  GDF_WINDOW_AVG = 0, GDF_WINDOW_SUM, GDF_WINDOW_MAX, GDF_WINDOW_MIN, GDF_WINDOW_COUNT,
  GDF_WINDOW_STDDEV, GDF_WINDOW_VAR
} window_reduction_type;

/* argument PODs of the csv reader / csr converter (io_types.h:26-60,
 * convert_types.h:33-41).  csv_read_arg carries the arguments and the three
 * output fields of read_csv; csr_gdf is what gdf_to_csr fills in, see below. */
typedef struct {
  int num_cols_out; int num_rows_out; gdf_column **data;
  char *file_path; char lineterminator; char delimiter; bool delim_whitespace; bool skipinitialspace;
  int num_cols; const char **names; const char **dtype;
  int skiprows; int skipfooter; bool dayfirst;
} csv_read_arg;
typedef struct csr_gdf_ {
  void *A; gdf_size_type *IA; int64_t *JA; gdf_dtype dtype; int64_t nnz;
  gdf_size_type rows; gdf_size_type cols;
} csr_gdf;

/* ======================================================================== *
 *  Hot-path entry points                            *
 * ======================================================================== */

/* --- column / context / error plumbing ---------------------------------- *
 * replaces src/column.cpp:160-275, src/context.cpp:3-11,
 * src/errorhandling.cpp:5-35, src/cudautils.cu:4-14 (functions.h:33-107)   */
gdf_size_type gdf_column_sizeof(void);
gdf_error gdf_column_view(gdf_column *column, void *data, gdf_valid_type *valid,
                          gdf_size_type size, gdf_dtype dtype);
gdf_error gdf_column_view_augmented(gdf_column *column, void *data, gdf_valid_type *valid,
                                    gdf_size_type size, gdf_dtype dtype, gdf_size_type null_count);
gdf_error gdf_column_free(gdf_column *column);           /* rmmFree(data), rmmFree(valid) */
gdf_error gdf_column_concat(gdf_column *output, gdf_column *columns_to_concat[], int num_columns);
gdf_error get_column_byte_width(gdf_column *col, int *width);
gdf_error gdf_context_view(gdf_context *context, int flag_sorted, gdf_method flag_method,
                           int flag_distinct, int flag_sort_result, int flag_sort_inplace);
const char *gdf_error_get_name(gdf_error errcode);
int         gdf_cuda_last_error(void);                   /* hipGetLastError()              */
const char *gdf_cuda_error_string(int cuda_error);       /* hipGetErrorString              */
const char *gdf_cuda_error_name(int cuda_error);         /* hipGetErrorName                */

/* --- profiler ranges: src/nvtx_utils.cpp:19-71 -> roctx (functions.h:18-31) */
gdf_error gdf_nvtx_range_push(char const *const name, gdf_color color);
gdf_error gdf_nvtx_range_push_hex(char const *const name, unsigned int color);
gdf_error gdf_nvtx_range_pop(void);

/* --- valid-mask helpers: src/validops.cu:86-256, src/binaryops.cu (functions.h:32,674) */
gdf_error gdf_count_nonzero_mask(gdf_valid_type const *masks, int num_rows, int *count);
gdf_error gdf_validity_and(gdf_column *lhs, gdf_column *rhs, gdf_column *output);

/* --- hash join: src/join/joining.cu:571-653 (functions.h:226-318) --------
 * left_indices/right_indices receive LIBRARY-allocated GDF_INT32 device
 * arrays of exactly the number of joined pairs (free with gdf_column_free);
 * pair order is unspecified.  result_cols (optional) receives the gathered
 * rows: [left non-key..., key..., right non-key...]. */
gdf_error gdf_inner_join(gdf_column **left_cols, int num_left_cols, int left_join_cols[],
                         gdf_column **right_cols, int num_right_cols, int right_join_cols[],
                         int num_cols_to_join, int result_num_cols, gdf_column **result_cols,
                         gdf_column *left_indices, gdf_column *right_indices,
                         gdf_context *join_context);
gdf_error gdf_left_join(gdf_column **left_cols, int num_left_cols, int left_join_cols[],
                        gdf_column **right_cols, int num_right_cols, int right_join_cols[],
                        int num_cols_to_join, int result_num_cols, gdf_column **result_cols,
                        gdf_column *left_indices, gdf_column *right_indices,
                        gdf_context *join_context);
gdf_error gdf_full_join(gdf_column **left_cols, int num_left_cols, int left_join_cols[],
                        gdf_column **right_cols, int num_right_cols, int right_join_cols[],
                        int num_cols_to_join, int result_num_cols, gdf_column **result_cols,
                        gdf_column *left_indices, gdf_column *right_indices,
                        gdf_context *join_context);

/* --- hash group-by: src/sqls_ops.cu:1426-1487 (functions.h:727-772) ------
 * Outputs are caller-preallocated; ->size of every output is set to the
 * number of groups.  out_col_indices is ignored by the HASH method. */
gdf_error gdf_group_by_sum(int ncols, gdf_column **cols, gdf_column *col_agg,
                           gdf_column *out_col_indices, gdf_column **out_col_values,
                           gdf_column *out_col_agg, gdf_context *ctxt);
gdf_error gdf_group_by_min(int ncols, gdf_column **cols, gdf_column *col_agg,
                           gdf_column *out_col_indices, gdf_column **out_col_values,
                           gdf_column *out_col_agg, gdf_context *ctxt);
gdf_error gdf_group_by_max(int ncols, gdf_column **cols, gdf_column *col_agg,
                           gdf_column *out_col_indices, gdf_column **out_col_values,
                           gdf_column *out_col_agg, gdf_context *ctxt);
gdf_error gdf_group_by_avg(int ncols, gdf_column **cols, gdf_column *col_agg,
                           gdf_column *out_col_indices, gdf_column **out_col_values,
                           gdf_column *out_col_agg, gdf_context *ctxt);
gdf_error gdf_group_by_count(int ncols, gdf_column **cols, gdf_column *col_agg,
                             gdf_column *out_col_indices, gdf_column **out_col_values,
                             gdf_column *out_col_agg, gdf_context *ctxt);

/* --- row hash + hash partition: src/hashing.cu:83-154,559-654 (functions.h:344-378) */
gdf_error gdf_hash(int num_cols, gdf_column **input, gdf_hash_func hash, gdf_column *output);
gdf_error gdf_hash_partition(int num_input_cols, gdf_column *input[], int columns_to_hash[],
                             int num_cols_to_hash, int num_partitions,
                             gdf_column *partitioned_output[], int partition_offsets[],
                             gdf_hash_func hash);

/* --- prefix sum: src/scan.cu:53-76 (functions.h:355-358) ----------------- */
gdf_error gdf_prefixsum_generic(gdf_column *inp, gdf_column *out, int inclusive);
gdf_error gdf_prefixsum_i8(gdf_column *inp, gdf_column *out, int inclusive);
gdf_error gdf_prefixsum_i32(gdf_column *inp, gdf_column *out, int inclusive);
gdf_error gdf_prefixsum_i64(gdf_column *inp, gdf_column *out, int inclusive);

/* --- filter predicates + stream compaction: src/filterops.cu:162-662,
 *     src/streamcompactionops.cu:208-339, src/sqls_ops.cu:1401-1424
 *     (functions.h:677-690,711-725) */
gdf_error gpu_comparison_static_i8 (gdf_column *lhs, int8_t  value, gdf_column *output, gdf_comparison_operator operation);
gdf_error gpu_comparison_static_i16(gdf_column *lhs, int16_t value, gdf_column *output, gdf_comparison_operator operation);
gdf_error gpu_comparison_static_i32(gdf_column *lhs, int32_t value, gdf_column *output, gdf_comparison_operator operation);
gdf_error gpu_comparison_static_i64(gdf_column *lhs, int64_t value, gdf_column *output, gdf_comparison_operator operation);
gdf_error gpu_comparison_static_f32(gdf_column *lhs, float   value, gdf_column *output, gdf_comparison_operator operation);
gdf_error gpu_comparison_static_f64(gdf_column *lhs, double  value, gdf_column *output, gdf_comparison_operator operation);
gdf_error gpu_comparison(gdf_column *lhs, gdf_column *rhs, gdf_column *output, gdf_comparison_operator operation);
gdf_error gpu_apply_stencil(gdf_column *lhs, gdf_column *stencil, gdf_column *output);
gdf_error gdf_filter(size_t nrows, gdf_column *cols, size_t ncols, void **d_cols, int *d_types,
                     void **d_vals, size_t *d_indx, size_t *new_sz);

/* --- whole-column reductions (functions.h:692-705 and the gdf_sum_ family; reference src/reductions.cu): csrc/reduce.hip
 *
 * The result goes to dev_result[0] (DEVICE memory) in the column's own type; nothing else of dev_result is written (the
 * partials live in library scratch).  Any dev_result_size >= 1 works and the result does not depend on it;
 * gdf_reduce_optimal_output_size() returns the reference's 128 because callers size their buffers from it.
 *   errors     NULL col / dev_result or dev_result_size < 1: GDF_INVALID_API_CALL, before any device work.
 *              _generic: sum / product / min / max take INT8, INT32, INT64, FLOAT32, FLOAT64; sum_squared FLOAT32 and
 *              FLOAT64 only; anything else GDF_UNSUPPORTED_DTYPE.  A typed entry point takes a column of its own storage
 *              (_i32: INT32 / DATE32, _i64: INT64 / DATE64 / TIMESTAMP) and answers GDF_DTYPE_MISMATCH otherwise (the
 *              reference would reinterpret the bytes).
 *   nulls      a null row contributes the identity; an empty or all-null column gives the identity: 0 for sum and
 *              sum_squared, 1 for product, numeric_limits<T>::max() for min and ::lowest() for max (for floats
 *              +-FLT_MAX / +-DBL_MAX, not +-inf, as in the reference; the identity takes part in every result).
 *   integers   accumulate and wrap in the input type (an int8 sum is mod 2^8, an int32 product mod 2^32).
 *   floats     f32 sum and sum_squared accumulate in f64 and round once at the end; product, min and max work in the input
 *              type; min and max return NaN when a valid element is NaN (numpy's np.min / np.max).
 *   determinism  the grid and the combine order are fixed: the same input on the same device gives a bit-identical result.
 *   stream     the legacy default stream; the call returns after the result is written.                                    */
unsigned int gdf_reduce_optimal_output_size(void);
gdf_error gdf_sum_generic(gdf_column *col, void *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_sum_f64(gdf_column *col, double *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_sum_f32(gdf_column *col, float *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_sum_i64(gdf_column *col, int64_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_sum_i32(gdf_column *col, int32_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_sum_i8(gdf_column *col, int8_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_product_generic(gdf_column *col, void *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_product_f64(gdf_column *col, double *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_product_f32(gdf_column *col, float *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_product_i64(gdf_column *col, int64_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_product_i32(gdf_column *col, int32_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_product_i8(gdf_column *col, int8_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_min_generic(gdf_column *col, void *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_min_f64(gdf_column *col, double *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_min_f32(gdf_column *col, float *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_min_i64(gdf_column *col, int64_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_min_i32(gdf_column *col, int32_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_min_i8(gdf_column *col, int8_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_max_generic(gdf_column *col, void *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_max_f64(gdf_column *col, double *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_max_f32(gdf_column *col, float *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_max_i64(gdf_column *col, int64_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_max_i32(gdf_column *col, int32_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_max_i8(gdf_column *col, int8_t *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_sum_squared_generic(gdf_column *col, void *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_sum_squared_f64(gdf_column *col, double *dev_result, gdf_size_type dev_result_size);
gdf_error gdf_sum_squared_f32(gdf_column *col, float *dev_result, gdf_size_type dev_result_size);

/* --- quantiles (functions.h:774-785; reference src/quantiles.cu): csrc/quantile.hip
 *
 * Let n be the column size and s the column in ascending order, NaN last.
 *   errors     a validity mask: GDF_VALIDITY_UNSUPPORTED (as the reference).  n == 0: GDF_DATASET_EMPTY.  NULL col, result
 *              pointer or ctxt, q NaN or q < 0: GDF_INVALID_API_CALL.  prec outside gdf_quantile_method:
 *              GDF_UNSUPPORTED_METHOD.  Dtypes INT8, INT16, INT32, INT64, FLOAT32, FLOAT64; anything else
 *              GDF_UNSUPPORTED_DTYPE.
 *   rule       q >= 1 gives s[n-1] (the max) and n == 1 gives s[0], for every method.  Otherwise pos = q * n (double),
 *              k = floor(pos), x = pos - k, and then k is decreased by one if it is positive (x is taken BEFORE that
 *              decrement, as in the reference).  y0 = s[k], y1 = s[k+1].
 *   results    gdf_quantile_aprrox writes y0 as a T to the HOST pointer t_erased_res.  gdf_quantile_exact writes a double
 *              to the host pointer: LINEAR y0 + x * (y1 - y0), LOWER y0, HIGHER y1, MIDPOINT (y0 + y1) / 2.0,
 *              NEAREST x < 0.5 ? y0 : y1.  y1 - y0 and y0 + y1 are computed in the column type under C promotion
 *              before the conversion to double: int8 and int16 promote to int, int32 and int64 wrap in two's
 *              complement, float stays float.
 *   modes      ctxt->flag_sorted: the column is trusted to be sorted and is read, not modified.
 *              ctxt->flag_sort_inplace (and not sorted): the column is left sorted ascending (NaN last).
 *              neither: the column is neither modified nor copied (radix selection).
 *              A zero's sign in a result is that of some zero of the column.                                            */
gdf_error gdf_quantile_exact(gdf_column *col_in, gdf_quantile_method prec, double q, void *t_erased_res, gdf_context *ctxt);
gdf_error gdf_quantile_aprrox(gdf_column *col_in, double q, void *t_erased_res, gdf_context *ctxt);

/* --- element-wise operators (functions.h:380-675; reference src/binaryops.cu, unaryops.cu, datetimeops.cu):
 *     csrc/elementwise.hip, prototypes in gdf_elementwise.def
 *
 * Every call is one kernel launch on the legacy default stream and returns after the output is written.  All argument
 * checks run on the host before any device work; nothing (no data, no field of `output`) is written when an error is
 * returned.  Data pointers need element alignment only (a column may be a slice); any size is accepted.
 *   NULL       a NULL column pointer: GDF_UNSUPPORTED_METHOD, for all 182 entry points (the reference dereferences it).
 *              A NULL data pointer of a non-empty column: GDF_INVALID_API_CALL.
 *   binary     gdf_{add,sub,mul,floordiv}_{generic,i32,i64,f32,f64}, gdf_div_{generic,f32,f64},
 *              gdf_{gt,ge,lt,le,eq,ne}_{generic,i8,i32,i64,f32,f64}, gdf_bitwise_{and,or,xor}_{generic,i8,i32,i64}.
 *              Checks, in this order: either input of size 0: GDF_SUCCESS, nothing done.  lhs->size != rhs->size or
 *              != output->size: GDF_COLUMN_SIZE_MISMATCH.  lhs->dtype != rhs->dtype: GDF_UNSUPPORTED_DTYPE.
 *              output->dtype must be lhs->dtype for arithmetic and bit operations and GDF_INT8 for comparisons, else
 *              GDF_UNSUPPORTED_DTYPE.  A typed entry point trusts its suffix for the element type.  _generic (after the
 *              size-0 rule) dispatches on lhs->dtype: arithmetic INT32 / INT64 / FLOAT32 / FLOAT64; div FLOAT32 /
 *              FLOAT64; comparisons INT8 / INT32 / INT64 / FLOAT32 / FLOAT64, DATE32 as int32, DATE64 and TIMESTAMP as
 *              int64; bit operations INT8 / INT32 / INT64; anything else GDF_UNSUPPORTED_DTYPE.
 *   values     integers wrap.  Float add / sub / mul / div are the correctly rounded IEEE operations.  Float floordiv
 *              is floor(lhs / rhs) in the column type.  Integer floordiv is EXACT floor division (the reference divides
 *              in double: the same for int32, off beyond 2^53 for int64); rhs == 0 gives 0 and INT_MIN / -1 gives
 *              INT_MIN -- the reference leaves both unspecified -- and neither faults.  Comparisons write 0 / 1 as int8;
 *              with a NaN operand only ne is 1.
 *   nulls      (binary and math) a row is null when it is null in any input.  The output DATA at a null row is
 *              unspecified (the reference leaves it unwritten, here it holds the operation applied to whatever the inputs
 *              hold there); output->valid and output->null_count are not touched, as in the reference: the caller ANDs
 *              the input masks.  The kernels do not read the masks.
 *   math       gdf_{sin,cos,tan,asin,acos,atan,exp,log,sqrt,ceil,floor}_{generic,f32,f64}.  size 0: GDF_SUCCESS; sizes
 *              differ: GDF_COLUMN_SIZE_MISMATCH; _generic takes FLOAT32 / FLOAT64, anything else GDF_UNSUPPORTED_DTYPE.
 *              f32 uses the f32 routines of the device math library and f64 the f64 ones, built without fast-math; sqrt,
 *              ceil and floor are exact, the others within a few ulp.
 *   casts      gdf_cast_{generic,i8,i32,i64,f32,f64,date32,date64,timestamp}_to_{f32,f64,i8,i32,i64,date32,date64} and
 *              .._to_timestamp(input, output, time_unit).  input->dtype must be the source the name says (generic: one of
 *              the eight), else GDF_UNSUPPORTED_DTYPE; then the sizes must agree (GDF_COLUMN_SIZE_MISMATCH) unless
 *              input->size is 0.  Then output->dtype is set -- and output->dtype_info.time_unit by _to_timestamp -- also
 *              for size 0; when input->valid and output->valid are both non-NULL, ceil(size / 8) mask bytes are copied.
 *              The conversion is the C conversion, except between date / time types: DATE32 (days) <-> DATE64 (ms),
 *              DATE32 <-> TIMESTAMP(s|ms|us|ns), DATE64 <-> TIMESTAMP(s|us|ns) and TIMESTAMP <-> TIMESTAMP across units
 *              multiply (wrapping) towards the finer unit and FLOOR-divide towards the coarser one.  DATE64 <->
 *              TIMESTAMP(ms), equal units and TIME_UNIT_NONE on either side are plain copies.  Float -> integer of a NaN
 *              or an out-of-range value is unspecified and does not fault.
 *   datetime   gdf_extract_datetime_{year,month,day,hour,minute,second}.  Sizes differ: GDF_COLUMN_SIZE_MISMATCH;
 *              output->dtype != GDF_INT16: GDF_UNSUPPORTED_DTYPE.  Input DATE32 (year / month / day only: hour, minute
 *              and second answer GDF_UNSUPPORTED_DTYPE), DATE64 (ms) or TIMESTAMP in its time_unit (TIME_UNIT_NONE counts
 *              as ms, as in the reference); anything else GDF_UNSUPPORTED_DTYPE.  The mask is copied as for the casts.
 *              The fields are those of the proleptic Gregorian calendar with floor semantics on both sides of the epoch
 *              (numpy.datetime64).  Two deliberate differences from the reference: at a negative exact multiple of a day
 *              / hour / minute it yields hour 24 / minute 60 / second 60, this library 0; it narrows the day number to
 *              32 bits, this library computes it in 64 and truncates the year to int16.
 *   aliasing   output->data may be exactly lhs->data or rhs->data (input->data) when the element widths are equal;
 *              partial overlap is undefined.
 *   determinism  a second call on the same input gives bit-identical output.                                              */
#define GDF_DECL_UNARY(name)        gdf_error name(gdf_column *input, gdf_column *output);
#define GDF_DECL_UNARY_TU(name)     gdf_error name(gdf_column *input, gdf_column *output, gdf_time_unit time_unit);
#define GDF_DECL_BINARY(name)       gdf_error name(gdf_column *lhs, gdf_column *rhs, gdf_column *output);
#include "gdf_elementwise.def"
#undef GDF_DECL_UNARY
#undef GDF_DECL_UNARY_TU
#undef GDF_DECL_BINARY

/* one-off shapes (functions.h:108-224,692-705,774-785; io_functions.h) */
gdf_ipc_parser_type *gdf_ipc_parser_open(const uint8_t *schema, size_t length);
void        gdf_ipc_parser_open_recordbatches(gdf_ipc_parser_type *handle, const uint8_t *recordbatches, size_t length);
void        gdf_ipc_parser_close(gdf_ipc_parser_type *handle);
int         gdf_ipc_parser_failed(gdf_ipc_parser_type *handle);
const char *gdf_ipc_parser_to_json(gdf_ipc_parser_type *handle);
const char *gdf_ipc_parser_get_error(gdf_ipc_parser_type *handle);
const void *gdf_ipc_parser_get_data(gdf_ipc_parser_type *handle);
int64_t     gdf_ipc_parser_get_data_offset(gdf_ipc_parser_type *handle);
const char *gdf_ipc_parser_get_schema_json(gdf_ipc_parser_type *handle);
const char *gdf_ipc_parser_get_layout_json(gdf_ipc_parser_type *handle);
/* radix-sort wrappers (reference functions.h:108-224, src/sorting.cu, src/segmented_sorting.cu): csrc/sort.hip */
gdf_error   gdf_radixsort_i8(gdf_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol);
gdf_error   gdf_radixsort_i32(gdf_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol);
gdf_error   gdf_radixsort_i64(gdf_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol);
gdf_error   gdf_radixsort_f32(gdf_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol);
gdf_error   gdf_radixsort_f64(gdf_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol);
gdf_error   gdf_radixsort_generic(gdf_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol);
gdf_error   gdf_segmented_radixsort_i8(gdf_segmented_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol, unsigned num_segments, unsigned *d_begin_offsets, unsigned *d_end_offsets);
gdf_error   gdf_segmented_radixsort_i32(gdf_segmented_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol, unsigned num_segments, unsigned *d_begin_offsets, unsigned *d_end_offsets);
gdf_error   gdf_segmented_radixsort_i64(gdf_segmented_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol, unsigned num_segments, unsigned *d_begin_offsets, unsigned *d_end_offsets);
gdf_error   gdf_segmented_radixsort_f32(gdf_segmented_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol, unsigned num_segments, unsigned *d_begin_offsets, unsigned *d_end_offsets);
gdf_error   gdf_segmented_radixsort_f64(gdf_segmented_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol, unsigned num_segments, unsigned *d_begin_offsets, unsigned *d_end_offsets);
gdf_error   gdf_segmented_radixsort_generic(gdf_segmented_radixsort_plan_type *hdl, gdf_column *keycol, gdf_column *valcol, unsigned num_segments, unsigned *d_begin_offsets, unsigned *d_end_offsets);
gdf_radixsort_plan_type *gdf_radixsort_plan(size_t num_items, int descending, unsigned begin_bit, unsigned end_bit);
gdf_error   gdf_radixsort_plan_setup(gdf_radixsort_plan_type *hdl, size_t sizeof_key, size_t sizeof_val);
gdf_error   gdf_radixsort_plan_free(gdf_radixsort_plan_type *hdl);
gdf_segmented_radixsort_plan_type *gdf_segmented_radixsort_plan(size_t num_items, int descending, unsigned begin_bit, unsigned end_bit);
gdf_error   gdf_segmented_radixsort_plan_setup(gdf_segmented_radixsort_plan_type *hdl, size_t sizeof_key, size_t sizeof_val);
gdf_error   gdf_segmented_radixsort_plan_free(gdf_segmented_radixsort_plan_type *hdl);
gdf_error   gpu_concat(gdf_column *lhs, gdf_column *rhs, gdf_column *output);
gdf_error   gpu_hash_columns(gdf_column **columns_to_hash, int num_columns, gdf_column *output_column, void *stream);
gdf_error   gdf_order_by(size_t nrows, gdf_column *cols, size_t ncols, void **d_cols, int *d_types, size_t *d_indx);

/* --- delimited text to columns (io_functions.h:18, io_types.h:26-60; reference src/io/csv/csv-reader.cu, type_conversion.cuh,
 *     date-time-parser.cuh): csrc/csv.hip
 *
 * The reference is the model for what the arguments mean, not for its arithmetic; every DEVIATION is marked with the reference
 * line it departs from.  The file is bytes; no quoting (a quote character is an ordinary byte, as in the reference), no header row.
 *   arguments  names, dtype and num_cols are required.  dtype strings (csv-reader.cu:393-413): str, category -> GDF_CATEGORY; date,
 *              date64 -> GDF_DATE64; date32 -> GDF_DATE32; timestamp -> GDF_TIMESTAMP; float, float32 -> GDF_FLOAT32; float64,
 *              double -> GDF_FLOAT64; short -> GDF_INT16; int, int32 -> GDF_INT32; int64, long -> GDF_INT64.
 *              delimiter separates fields; delim_whitespace makes it one space (two spaces enclose an empty field), as the
 *              reference.  lineterminator ends a record; when it is '\n', one '\r' directly in front of it is not part of the
 *              record.  skiprows / skipfooter drop records from the front / the back (dropping all of them: zero rows, success).
 *              skipinitialspace drops the leading spaces of CATEGORY fields; fields of every other dtype are always trimmed of
 *              spaces (0x20) on both sides.  dayfirst: see dates.
 *   records    every terminator ends a record; a non-empty tail behind the last terminator is a record too (DEVIATION:
 *              csv-reader.cu:505-535 counts terminators only and drops it; :528, :595 and :686 look at the byte behind the last
 *              one, this library reads nothing outside the file's bytes).  An empty record is a row of nulls.  Row r, column c is
 *              the c-th delimiter-separated field of record skiprows + r; a record with fewer than num_cols fields has nulls in
 *              the missing ones, fields beyond num_cols are ignored.
 *   nulls      an empty field (after the trimming above) is null, and so is a field that is not a literal of its column's dtype
 *              as defined below.  A null element has validity bit 0 and data element 0 (DEVIATION: csv-reader.cu:460 leaves the
 *              data uninitialised), so whole arrays compare equal.
 *   integers   INT16, INT32, INT64 and TIMESTAMP (int64, time_unit TIME_UNIT_NONE): [+-]? digit (digit | ',')* where every ','
 *              stands between two digits and is skipped -- the reference's thousands separator, type_conversion.cuh:70; it can
 *              only occur when the delimiter is another byte.  DEVIATION: a sign is understood (type_conversion.cuh:47-79 turns
 *              '-' into a digit of value -3), and a value outside the dtype's range is null, not wrapped.
 *   floats     [+-]? (digits [. digits*] | . digits) ([eE] [+-]? digits)?, commas in the integer part as above; inf, nan and
 *              hexadecimal forms are no literals (null).  The first 19 significant digits (leading zeros are not significant)
 *              are kept in a 64-bit integer m, every further digit is dropped, and the decimal exponent e absorbs the dropped
 *              integer digits, the kept fraction digits and the written exponent: the field stands for m * 10^e, truncated after
 *              19 digits.  m == 0 gives a zero; e > 308 gives an infinity; e < -400 a zero.  Otherwise x = (double)m, then
 *                e >= 0:  x * P[e / 22] * 10^(e % 22)           e < 0:  [x / 1e308 first when e < -308, e += 308]
 *                                                                        x / 10^(|e| % 22) / P[|e| / 22]
 *              with P[q] the double nearest to 10^(22 q) and 10^0 .. 10^22 exact doubles.  FAST DOMAIN m < 2^53 and |e| <= 22:
 *              (double)m is exact, P[0] = 1 and P[1] = 1e22 are exact, one of the two factors is 1: ONE rounding, the correctly
 *              rounded value (Clinger's fast path) -- bit-equal to strtod / Python's float().  OUTSIDE it the roundings are:
 *              (double)m; 1e308 and its division; P[q] and its operation; the operation with 10^r -- at most six, each a relative
 *              error of at most 2^-53, which is half an ulp at the top of a binade and one ulp at its bottom.  Their sum puts the
 *              result within 6 ulp of m * 10^e; dropping digits beyond the 19th moves m * 10^e by less than 10^-18 of itself
 *              (under 0.01 ulp); the correctly rounded value is half an ulp from the exact one: the result is within 7 ulp (of
 *              the correctly rounded value) of it.  An intermediate never exceeds the final magnitude for e >= 0 (no early
 *              overflow); for e < 0 an intermediate that is already subnormal is divided further, which shrinks its absolute
 *              error below the final half ulp.  Overflow gives +-inf -- and so may a literal within those 7 ulp of the largest
 *              finite double -- and a written "-0" gives -0.0.  A written exponent saturates at 4 * 10^18 in magnitude, beyond
 *              the digit count of any field (a buffer has at most 2^62 bytes), before it is added to the digits' exponent and
 *              the sum is compared with 308 and -400.  FLOAT32 is (float) of that double.  (DEVIATION:
 *              type_conversion.cuh:82-152 sums digit * pow(10, k) in the column type, knows no sign and no exponent.)
 *   dates      DATE32: days since 1970-01-01 in the proleptic Gregorian calendar, correct on both sides of the epoch (DEVIATION:
 *              date-time-parser.cuh:324-351 is a day ahead -- it adds the day of the month to days that already count from day
 *              1 -- and knows leap years by year % 4 only); DATE64 the same in milliseconds.  Date forms, the separator being
 *              '/' or '-' (the same one twice), Y four digits, M and D one or two:  Y-M-D, Y-M (a four-digit first part is the
 *              year);  M-D-Y, or D-M-Y with dayfirst;  M-Y.  A missing day is 1.  DATE64 only: a time may follow after 'T' or
 *              one space, as H:M or H:M:S (one or two digits each), optionally followed by AM or PM (either case, optionally
 *              after one space); with AM / PM the hour is 1 .. 12, 12 AM is hour 0 and 12 PM hour 12 (DEVIATION:
 *              date-time-parser.cuh:274-291 adds 12 to every PM hour: 12 PM becomes 24).  Checked: year 1 .. 9999, month
 *              1 .. 12, day within the month (leap years by the Gregorian rule), hour 0 .. 23, minute and second 0 .. 59; a
 *              failure, or anything else behind the date or time, is null.
 *   category   MurmurHash3 x86_32 with seed 33 of exactly the field's bytes, as int32 (DEVIATION: csv-reader.cu:763 hashes
 *              through the delimiter or terminator behind the field).
 *   outputs    args->data, num_cols_out (= num_cols) and num_rows_out are set.  data is a malloc'ed array of num_cols malloc'ed
 *              gdf_columns, each with a malloc'ed copy of its name in col_name; data and valid inside each column come from
 *              rmmAlloc and are released by gdf_column_free (the reference's split of ownership; gdf_amd_read_csv_release in
 *              gdf_amd_ext.h releases all of it).  Per column: size = rows, dtype, null_count exact, every other field zero.
 *              valid is never NULL when rows > 0, has ceil(rows / 64) * 8 >= ceil(rows / 8) bytes, LSB first, and the bits
 *              beyond `rows` are 0.  Zero rows: size 0 and data == valid == NULL.  CATEGORY data is int32.
 *   errors     all argument errors are reported before any device work and before the file is opened; on any error the three
 *              output fields are untouched and nothing stays allocated.  GDF_INVALID_API_CALL: args NULL, num_cols <= 0, names
 *              or dtype NULL or with a NULL element, a negative skip count.  Then GDF_UNSUPPORTED_DTYPE: an unknown dtype string.
 *              Then GDF_FILE_ERROR: file_path NULL, the file cannot be opened or mapped, or is not a regular file.  After the
 *              count pass GDF_COLUMN_SIZE_TOO_BIG: more than INT32_MAX records.  An empty file is zero rows, no error.
 *   determinism  a second call on the same bytes gives bit-identical columns and masks (the only atomics add up null counts).
 *   stream     the legacy default stream; the call returns after the outputs are written.                                     */
gdf_error   read_csv(csv_read_arg *args);

/* --- columns to a CSR matrix (io_functions.h:22, convert_types.h:31-39; reference src/io/convert/gdf-to-csr.cu): csrc/csr.hip
 *
 * All num_cols columns have the same size = rows.  The result is the row-major CSR form of the rows x num_cols matrix whose
 * entry (r, c) exists exactly when validity bit r of column c is set; a column with valid == NULL has every entry (the
 * reference dereferences the NULL).  This converts VALIDITY, not non-zeroness: a valid 0 or NaN is an entry.  null_count is
 * not consulted.
 *   outputs    device memory from rmmAlloc, each released by the caller with rmmFree:
 *              IA   gdf_size_type[rows + 1] (8-byte elements, as everywhere in this ABI); IA[0] == 0, IA[rows] == nnz;
 *              JA   int64_t[nnz], the column indices, ascending within a row;
 *              A    nnz elements of `dtype`.
 *              dtype is the largest gdf_dtype enumerator among the columns (as the reference), so every conversion is a
 *              widening static_cast in enum order: int -> wider int, int -> float32 / float64, float32 -> float64; an INT64
 *              column next to a FLOAT32 column gives FLOAT32.  rows, cols and nnz are host fields.
 *              nnz == 0 (rows == 0 included): GDF_SUCCESS, IA is rows + 1 zeros, A == JA == NULL (the reference answers
 *              GDF_CUDA_ERROR and leaks its scratch).
 *   errors     on any error nothing stays allocated and *csrReturn is untouched.  Host checks before any device work:
 *              csrReturn == NULL: GDF_INVALID_API_CALL.  gdfData == NULL, num_cols <= 0, a NULL element, or rows > 0 with a
 *              NULL data pointer: GDF_DATASET_EMPTY.  Sizes differ: GDF_COLUMN_SIZE_MISMATCH (the reference never looks).  A
 *              column dtype outside INT8 .. FLOAT64: GDF_UNSUPPORTED_DTYPE.  After the count pass: nnz > INT32_MAX (the tile
 *              offsets are 32-bit): GDF_COLUMN_SIZE_TOO_BIG.
 *   masks      bits of the last mask byte beyond `rows` are ignored; a mask pointer needs no alignment.
 *   determinism  no atomics touch the outputs: a second call on the same input gives bit-identical A, IA and JA.
 *   stream     the legacy default stream; the call returns after the outputs are written.                                     */
gdf_error   gdf_to_csr(gdf_column **gdfData, int num_cols, csr_gdf *csrReturn);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}  /* extern "C" */
#endif
#endif /* GDF_AMD_GDF_H */
