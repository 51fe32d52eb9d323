/*
 * gdf_amd_ext.h -- exports of libgdf.so that the reference does NOT have.  Nothing here is needed by a
 * caller of the reference API; they exist for measurement (bench.py, tools/), for tests, for the multi-GPU
 * layer (libgdf_amd/multigpu.py), which sits above the unchanged gdf_* ABI, and for what the reference ABI cannot
 * express: a CSV reader over device bytes, ORDER BY over masked columns with a direction per column, a row gather, a GROUP BY with
 * several aggregates whose null keys form groups, ORDER BY ... LIMIT k by selection, EXISTS / NOT EXISTS (semi and anti join).
 */
#ifndef GDF_AMD_EXT_H
#define GDF_AMD_EXT_H
#include <gdf/gdf.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* per-kernel HIP-event timing of everything the library launches (csrc/prof.cpp) */
void gdf_amd_profile_enable(int on);
void gdf_amd_profile_reset(void);
int  gdf_amd_profile_read(char (*names)[64], double *total_ms, int *launches, int capacity);

/* test hook: the join's radix partitioner alone (csrc/join.hip, tests/test_gpu_join_internals.py) */
gdf_error gdf_amd_debug_partition(gdf_column *col, int fb, uint64_t *out_key, int32_t *out_idx, uint32_t *out_fine_off,
                                  uint32_t *out_joinable, uint64_t *out_info);

/* (the path-forcing test hook gdf_amd_debug_force is not exported from libgdf.so any more: include/gdf/gdf_amd_testhook.h,
 * libgdf_testhook.so -- test infrastructure, loaded by the tests only) */

/*
 * out[i] = (int32)(in[i] - lo) when lo <= in[i] <= hi, else -1.   in: GDF_INT64 (or DATE64 / TIMESTAMP), no mask;
 * out: caller-preallocated GDF_INT32 of the same size; requires 0 <= hi - lo < 2^31 - 1.
 * The multi-GPU join ships 4-byte keys instead of 8-byte ones when the global build-key range allows it: probe keys
 * outside the range cannot match and become -1, which no narrowed build key equals.
 */
gdf_error gdf_amd_narrow_keys(gdf_column *in, int64_t lo, int64_t hi, gdf_column *out);

/*
 * A build relation partitioned ONCE and probed many times.  gdf_amd_join_build_probe(b, 0, probe...) returns exactly what
 * gdf_inner_join(probe, build) with GDF_HASH returns (probe_indices = left, build_indices = right; library-allocated
 * int32 columns, gdf_column_free them), left_join != 0 what gdf_left_join returns -- except that the table is always on
 * the prepared relation, never on the smaller one.  The build columns' DATA is not copied: it must stay alive and
 * unchanged until gdf_amd_join_build_free.  The multi-GPU join probes the received build relation once per slice of
 * the probe relation.
 */
typedef struct gdf_amd_join_build gdf_amd_join_build;
gdf_error gdf_amd_join_build_create(gdf_column **build_cols, int num_cols, gdf_amd_join_build **out);
gdf_error gdf_amd_join_build_probe(gdf_amd_join_build *build, int left_join, gdf_column **probe_cols, int num_cols,
                                   gdf_column *probe_indices, gdf_column *build_indices);
void gdf_amd_join_build_free(gdf_amd_join_build *build);

/*
 * A probe relation that arrives in slices (the multi-GPU join receives it that way), partitioned slice by slice and
 * probed ONCE: probe_indices number the rows across the slices in the order they were added; the result is what
 * gdf_amd_join_build_probe(build, 0, all slices concatenated) returns.  INNER joins on one unmasked integer key column
 * whose values fit the 32-bit tuple format only, and expected_rows >= 2^22 (an estimate of the total; a few percent of
 * head-room are built in): anything else -- and a slice sequence so skewed that a partition outgrows its room --
 * returns GDF_UNSUPPORTED_METHOD from _begin / _add / _finish, and the caller probes its slices one by one instead.
 * _finish releases the object whatever it returns.
 */
typedef struct gdf_amd_join_probe gdf_amd_join_probe;
gdf_error gdf_amd_join_probe_begin(gdf_amd_join_build *build, size_t expected_rows, gdf_amd_join_probe **out);
gdf_error gdf_amd_join_probe_add(gdf_amd_join_probe *probe, gdf_column **probe_cols, int num_cols);
gdf_error gdf_amd_join_probe_finish(gdf_amd_join_probe *probe, gdf_column *probe_indices, gdf_column *build_indices);

/*
 * The sender side of the multi-GPU shuffle in ONE pass over the keys (instead of narrow + row-number column +
 * gdf_hash_partition): partitions (key', row) on Murmur3(key') into num_partitions partitions exactly as
 * gdf_hash_partition(GDF_HASH_MURMUR3) places them, where row = row_base + i and key' = keys[i], or, with narrow != 0
 * (keys GDF_INT64-like, out_keys GDF_INT32), the gdf_amd_narrow_keys(lo, hi) image of it.  out_keys / out_rows
 * (GDF_INT32) are caller-preallocated with keys->size rows; partition_offsets is a HOST array of num_partitions ints.
 */
gdf_error gdf_amd_shuffle_partition(gdf_column *keys, int narrow, int64_t lo, int64_t hi, int32_t row_base, int num_partitions,
                                    gdf_column *out_keys, gdf_column *out_rows, int partition_offsets[]);

/*
 * The same split as gdf_amd_shuffle_partition without a row-number column: the partition is STABLE (the keys of a
 * partition keep their input order) and bitmap p -- ceil(rows / 64) 64-bit words at bitmaps + p * ceil(rows / 64), DEVICE
 * memory, bit i of word i / 64 -- has bit i set iff input row i went to partition p.  The j-th key of partition p is
 * therefore input row select(bitmap p, j): a receiver names the original row of a joined key from one bit per row
 * instead of a 4-byte row number (4.125 instead of 8 bytes per row on the links).  num_partitions <= 64.
 * narrow = 2: as narrow = 1, and a row whose key lies outside [lo, hi] -- it cannot match any build key of an inner
 * join -- is DROPPED: it goes to no partition and sets no bitmap bit (with narrow = 1 all such rows become the key -1 and
 * pile up on one rank).  partition_offsets then has num_partitions + 1 entries, the last one = rows that travel.
 */
gdf_error gdf_amd_shuffle_partition_stable(gdf_column *keys, int narrow, int64_t lo, int64_t hi, int num_partitions,
                                           gdf_column *out_keys, uint64_t *bitmaps, int partition_offsets[]);

/*
 * FUSED multi-GPU join: the sender runs the join's level-1 regroup, the receiver continues at level 2 (csrc/join.hip "FUSED
 * multi-GPU join"; libgdf_amd/multigpu.py fused_inner_join).  All ranks share one hash space; rank = mulhi(hash, world).
 *
 * gdf_amd_fj_plan    layout every rank derives from GLOBAL numbers only: fine / coarse partition bits of a rank's share of
 *                    `build_rows_total`, and the room `cap` (keys per (bin, XCD) region) for calls of at most `rows_max` rows
 *                    whose keys repeat `rows_per_key` times on average (all copies of a key share a region).
 *                    GDF_UNSUPPORTED_METHOD: this world size / relation size does not fit the path (use the key shuffle).
 * gdf_amd_fj_send    int64 / int32 keys -> out_keys: (world << coarse_bits) bins x 8 regions x cap 4-byte keys (key - lo; rows
 *                    outside [lo, hi] are dropped), rank r's keys in the r-th contiguous block of (8 << coarse_bits) * cap
 *                    elements (+ one tile = 32768 elements of dump space behind the last block); out_pos[i]: the position in
 *                    out_keys that row i's key went to (0xffffffff: dropped) -- it stays with the sender, who can tell from it
 *                    which row a result position names; out_fill: DEVICE array of (world << coarse_bits) * 8 fill counters
 *                    + 1 word.  *overflowed = 1: some region outgrew cap (skewed keys), the buffers are unusable.
 * gdf_amd_fj_build_create   receive buffer of the build relation (the blocks every sender made for this rank, sender-major,
 *                    with their fill counters in the same order, both in DEVICE memory) -> a build handle
 *                    (gdf_amd_join_probe_begin / gdf_amd_fj_probe_add / gdf_amd_join_probe_finish / gdf_amd_join_build_free).
 * gdf_amd_fj_probe_add      one receive buffer of the probe relation; result indices are POSITIONS: position_base + offset in
 *                    this buffer for the probe side, offset in the build receive buffer for the build side.
 */
gdf_error gdf_amd_fj_plan(int world, int64_t build_rows_total, int64_t rows_max, double rows_per_key, int *fine_bits, int *coarse_bits,
                          uint32_t *cap);
gdf_error gdf_amd_fj_send(gdf_column *keys, int64_t lo, int64_t hi, int world, int coarse_bits, uint32_t cap,
                          uint32_t *out_keys, uint32_t *out_pos, uint32_t *out_fill, int *overflowed);
gdf_error gdf_amd_fj_build_create(const uint32_t *recv_keys, const uint32_t *recv_fill, int world, int64_t lo, int fine_bits,
                                  int coarse_bits, uint32_t cap, int64_t expected_rows, gdf_amd_join_build **out);
gdf_error gdf_amd_fj_probe_add(gdf_amd_join_probe *probe, const uint32_t *recv_keys, const uint32_t *recv_fill, uint32_t cap,
                               int64_t position_base, int64_t buffer_elems);

/*
 * gdf_amd_dist_inner_join -- the multi-GPU inner join behind the C ABI (one process per GPU; BASELINE.json north_star: "host code
 * stays C++ behind the same C ABI ... radix-partitioned on key and shuffled with RCCL all-to-all over xGMI").  No counterpart in
 * the reference, which is single-GPU.  It runs the FUSED join above end to end: global key
 * range and sizes (three small all-reduces), gdf_amd_fj_plan, the sender's level-1 regroup of the build relation and of the probe
 * relation in `chunks` slices, the all-to-all of EQUAL blocks + fill counters per slice (software-pipelined: slice c travels while
 * slice c + 1 is regrouped and slice c - 1 is partitioned at the receiver), level 2 + LDS probe at the receiver, and the
 * collective agreement that decides between result and decline.
 *
 * The wire is a gdf_amd_transport: four function pointers and an optional fifth (all_to_all_v).  gdf_amd_rccl_transport_create gives the RCCL one (ncclSend / ncclRecv
 * groups on a stream of its own, librccl resolved with dlopen at that moment -- libgdf.so itself does not link against it); a host
 * in another language, or a test that moves the blocks through host memory between processes (tests/multirank_common.py), fills
 * the struct itself.
 *
 * Every rank of the transport calls with its shard: one GDF_INT64 (or GDF_INT32) key column each, no validity masks.
 *   probe_pos / build_pos   caller-allocated DEVICE arrays, one uint32 per local probe / build row: the position that row's key
 *                           went to in its send buffer (0xffffffff: dropped, the key lies outside the global build range) -- they
 *                           stay with the sender, who can tell from them which of its rows a result position names
 *   probe_indices / build_indices   library-allocated GDF_INT32 columns (gdf_column_free), exactly as gdf_inner_join's: this
 *                           rank's pairs as POSITIONS in its receive buffers -- probe: slice * world * block_p + offset in slice's
 *                           buffer, build: offset in the build receive buffer; offset / block = the sender's rank
 *   info                    the layout both sides were exchanged in (what turns positions into (rank, row))
 *   *declined = 1           ON EVERY RANK: the shape does not fit the fused path (keys that do not narrow to 31 bits, a relation
 *                           or world size outside gdf_amd_fj_plan's range, skewed keys that overflow the fixed-size regions, the
 *                           31-bit position space) -- nothing is returned and the caller takes the key shuffle
 *                           (libgdf_amd/multigpu.py distributed_inner_join) on all ranks together.
 * A hard LOCAL error (out of memory, a HIP failure) does not make its rank drop out of the collectives: every wire buffer is
 * allocated before the first agreement, the rank keeps posting its (useless) blocks, reports the failure at the next agreement and
 * ALL ranks leave there -- the rank that met the error with its code, its peers with GDF_C_ERROR.  A failing TRANSPORT call
 * (all_to_all / wait / all_reduce_i64 returning non-zero) is returned at once; the peers then see their own transport fail or time out.
 */
typedef struct gdf_amd_transport {
  void *ctx;
  int rank, world;
  /* DEVICE buffers: block r of `send` (bytes_per_rank bytes) goes to rank r, block s of `recv` arrives from rank s.  Ordered behind
     the work the library has issued so far; *ticket names the exchange.  0 = success. */
  int (*all_to_all)(void *ctx, const void *send, void *recv, size_t bytes_per_rank, void **ticket);
  /* orders the library's stream behind the exchange (recv may be read, send reused, afterwards); releases the ticket */
  int (*wait)(void *ctx, void *ticket);
  /* HOST values, reduced in place over all ranks; op 0 = min, 1 = max, 2 = sum */
  int (*all_reduce_i64)(void *ctx, int64_t *values, int count, int op);
  /* releases ctx (may be NULL) */
  void (*destroy)(void *ctx);
  /* OPTIONAL, may be NULL (round 6; the all-to-all-v SURVEY 8(e) names): bytes [send_off[r], send_off[r + 1]) of the DEVICE buffer `send`
     go to rank r, bytes [recv_off[s], recv_off[s + 1]) of `recv` arrive from rank s.  The offset arrays are HOST arrays of world + 1
     entries; what rank a sends to rank b is what b expects from a (the callers exchange their counts first).  Ordering, ticket and
     return value as all_to_all.  With it gdf_amd_dist_group_by* and gdf_amd_dist_shuffle_join ship EXACT sizes straight from their
     partitioned columns into the result columns; without it they pad to equal blocks and stage them.  LAST member: a host that
     fills the struct itself and was written against the four-function version must zero it. */
  int (*all_to_all_v)(void *ctx, const void *send, const size_t *send_off, void *recv, const size_t *recv_off, void **ticket);
} gdf_amd_transport;

typedef struct gdf_amd_dist_info {
  int world, chunks;
  int64_t lo, hi;                      /* global build-side key range: keys travel as (key - lo) */
  int64_t slice_rows;                  /* probe rows per slice (the last one may be shorter) */
  int fine_bits_p, coarse_bits_p;      /* gdf_amd_fj_plan of the probe slices ...                */
  uint32_t cap_p;
  int fine_bits_b, coarse_bits_b;      /* ... and of the build relation                          */
  uint32_t cap_b;
  int64_t block_p, block_b;            /* elements every sender makes for one rank: (8 << coarse_bits) * cap */
} gdf_amd_dist_info;

gdf_error gdf_amd_dist_inner_join(gdf_column *probe_keys, gdf_column *build_keys, gdf_amd_transport *transport, int chunks,
                                  uint32_t *probe_pos, uint32_t *build_pos, gdf_column *probe_indices, gdf_column *build_indices,
                                  gdf_amd_dist_info *info, int *declined);

/* The KEY SHUFFLE join behind the C ABI (csrc/dist_ops.hip) -- what all ranks take TOGETHER when gdf_amd_dist_inner_join says
 * *declined = 1 (keys that do not narrow to 31 bits, skewed keys, a shape outside gdf_amd_fj_plan's range).  COLLECTIVE; any
 * int32 / int64 key column without a mask, any shard sizes (also none).  Every rank splits (key, local row number) of both
 * relations by owner rank = Murmur3(key) % world (gdf_amd_shuffle_partition), the partitions travel as equal blocks over
 * transport->all_to_all (block size and failures agreed by one all-reduce per relation), the owner joins what it received with
 * gdf_inner_join (src/join/joining.cu:571-653 per rank) and resolves the pairs to GLOBAL row ids:
 *   out_probe_ids / out_build_ids   library-allocated GDF_INT64 columns (gdf_column_free): (owner rank << 40) | local row of the
 *                                   probe / build row of every pair this rank produced; every pair of the global join comes out
 *                                   on exactly one rank, in no particular order.
 * One exchange per relation, not pipelined: the fallback trades the fused path's overlap for generality.  Local errors travel
 * into the agreements as in gdf_amd_dist_inner_join. */
gdf_error gdf_amd_dist_shuffle_join(gdf_column *probe_keys, gdf_column *build_keys, gdf_amd_transport *transport,
                                    gdf_column *out_probe_ids, gdf_column *out_build_ids);
/* ... and as a LEFT / FULL join (round 6; reference: gdf_left_join / gdf_full_join, src/join/joining.cu:571-653, per owner rank): every row
 * of either relation reaches exactly one owner, so a probe row without a partner comes out once as (global id, -1) and -- FULL -- a
 * build row without a partner once as (-1, global id).  Semantics of unmatched rows and of the pair order as the single-GPU calls. */
gdf_error gdf_amd_dist_shuffle_left_join(gdf_column *probe_keys, gdf_column *build_keys, gdf_amd_transport *transport,
                                         gdf_column *out_probe_ids, gdf_column *out_build_ids);
gdf_error gdf_amd_dist_shuffle_full_join(gdf_column *probe_keys, gdf_column *build_keys, gdf_amd_transport *transport,
                                         gdf_column *out_probe_ids, gdf_column *out_build_ids);

/* DISTRIBUTED MATERIALISATION (round 6): the multi-GPU face of the joins' result_cols step (src/join/joining.cu:375-479 gathers the
 * relations' columns by the index columns; across ranks the index is a global row id).  COLLECTIVE.  `ids` is a GDF_INT64 column
 * without a mask of global row ids as the gdf_amd_dist_shuffle_*join entries produce them -- (owner rank << 40) | local row, or -1
 * for the missing side of an unmatched row -- in any number and any order (also none); `columns` are 1 ... 16 columns of THIS rank's
 * shard of the relation the ids name (equal sizes, any fixed-width dtype, validity masks honoured).  Every id is asked of its owner
 * (the local rows travel over the transport, split by owner), the owner reads its shard and the values travel back:
 *   outs[c]   library-allocated column (gdf_column_free) of ids->size rows in the dtype of columns[c], ALWAYS with a validity mask:
 *             row i is columns[c]'s row named by ids[i] on its owner -- null where ids[i] is -1 or the source row is null -- and
 *             null_count says how many are.
 * Errors: an id that names no rank or no row of its owner's shard is GDF_INVALID_API_CALL; local errors are carried into the next
 * agreement as in the entries above, every rank returns together. */
gdf_error gdf_amd_dist_gather(gdf_column *ids, int ncols, gdf_column **columns, gdf_amd_transport *transport, gdf_column **outs);

/* MULTI-GPU GROUP-BY behind the C ABI (csrc/dist_ops.hip; no counterpart in the reference, which is single-GPU -- per rank it
 * composes gdf_group_by_<op>, src/sqls_ops.cu:1426-1487, and gdf_hash_partition, src/hashing.cu:559-654).  COLLECTIVE: every rank
 * of the transport calls it with its row shard of (keys, values) -- one int32 / int64 key column, one numeric value column, no
 * validity masks, possibly no rows.  Every rank pre-aggregates its shard, the partial aggregates travel to the rank
 * Murmur3(key) % world owns (equal blocks over transport->all_to_all, their size agreed by one all-reduce) and are combined there:
 * partial sums / minima / maxima by the same operator, partial counts (int64) by a sum, AVG as the quotient of the combined sums
 * (accumulated in int64 / float64) and counts -- a GDF_FLOAT64 column.
 *   out_keys / out_agg   library-allocated columns (gdf_column_free) with THIS RANK'S groups, sorted by key; every group of the
 *                        global relation comes out on exactly one rank.  SUM / MIN / MAX keep the value dtype (a sum wraps as the
 *                        single-GPU gdf_group_by_sum does), COUNT is GDF_INT64, AVG GDF_FLOAT64.
 * Errors: a local error (bad arguments on one rank, out of memory) is carried into the next agreement -- the block size's, or the one
 * behind the wire buffers' allocation (round 6: two all-reduces per exchange) -- and that rank returns its code, the others GDF_C_ERROR:
 * nobody is left waiting in a collective.  A rank whose local work fails BEHIND the last exchange returns its code alone (the others have
 * their results).  op: GDF_SUM, GDF_MIN, GDF_MAX, GDF_COUNT, GDF_AVG. */
gdf_error gdf_amd_dist_group_by(gdf_agg_op op, gdf_column *keys, gdf_column *values, gdf_amd_transport *transport,
                                gdf_column *out_keys, gdf_column *out_agg);
gdf_error gdf_amd_dist_group_by_sum(gdf_column *keys, gdf_column *values, gdf_amd_transport *transport, gdf_column *out_keys, gdf_column *out_agg);
gdf_error gdf_amd_dist_group_by_min(gdf_column *keys, gdf_column *values, gdf_amd_transport *transport, gdf_column *out_keys, gdf_column *out_agg);
gdf_error gdf_amd_dist_group_by_max(gdf_column *keys, gdf_column *values, gdf_amd_transport *transport, gdf_column *out_keys, gdf_column *out_agg);
gdf_error gdf_amd_dist_group_by_count(gdf_column *keys, gdf_column *values, gdf_amd_transport *transport, gdf_column *out_keys, gdf_column *out_agg);
gdf_error gdf_amd_dist_group_by_avg(gdf_column *keys, gdf_column *values, gdf_amd_transport *transport, gdf_column *out_keys, gdf_column *out_agg);

/* The same over SEVERAL key columns and WITH validity masks (round 6; BASELINE configuration C5 -- a two-key, masked AVG -- across ranks).
 * Reference shape: gdf_group_by_* over ncols key columns (src/sqls_ops.cu:1085-1363, src/groupby/groupby.cuh:208-250); a group's owner
 * is its ROW HASH % world -- the Murmur3 fold over the key columns of src/gdf_table.cuh:704-854, i.e. gdf_hash_partition on all key
 * columns.  Key columns: any dtype the local group-by takes; values: numeric.  Mask semantics are the local HASH group-by's extension
 * (the reference rejects masks, sqls_ops.cu:1103-1106): a row with a null in ANY key column is dropped, a null value is skipped, a group
 * without a valid value reports 0 and a cleared validity bit (COUNT: 0, valid).  Per rank: the partial aggregate (AVG: the sum of the
 * widened values) and the number of valid values of every local group travel to the owner, which combines the partials that had a valid
 * value by the same operator and the counts by a sum; AVG = combined sum / combined count (src/groupby/groupby.cuh:308-419 per rank).
 *   out_keys[ncols], out_agg   library-allocated columns (gdf_column_free) with THIS RANK'S groups in ascending lexicographic key order;
 *                              out_agg carries a validity mask (and null_count) unless op is GDF_COUNT.  Dtypes as the single-key entry.
 * Errors travel into the agreements as above; two small all-reduces (block size; "every rank has its wire buffers") precede the exchange. */
gdf_error gdf_amd_dist_group_by_multi(gdf_agg_op op, int ncols, gdf_column **keys, gdf_column *values, gdf_amd_transport *transport,
                                      gdf_column **out_keys, gdf_column *out_agg);

/* RCCL transport.  id: the 128 bytes of an ncclUniqueId -- made by ONE rank with gdf_amd_rccl_unique_id and handed to the others by
   whatever the host has (MPI, a file, torch.distributed's store); every rank then calls gdf_amd_rccl_transport_create (collective:
   ncclCommInitRank) with the device it computes on current.  gdf_amd_transport_free destroys communicator and stream. */
gdf_error gdf_amd_rccl_unique_id(char id[128]);
gdf_error gdf_amd_rccl_transport_create(const char id[128], int world, int rank, gdf_amd_transport **out);
void gdf_amd_transport_free(gdf_amd_transport *transport);
/* the communicator's own answer (ncclCommCount / ncclCommUserRank) for a transport made by gdf_amd_rccl_transport_create */
gdf_error gdf_amd_rccl_transport_ranks(gdf_amd_transport *transport, int *nranks, int *rank);
/* synchronous copy on the library's stream for transports that stage blocks through host memory; direction 0: device -> host,
   1: host -> device, 2: device -> device */
gdf_error gdf_amd_copy(void *dst, const void *src, size_t bytes, int direction);

/*
 * read_csv (include/gdf/gdf.h has the contract) over bytes that already sit in DEVICE memory: the same reader, fields and errors,
 * with args->file_path ignored.  d_bytes needs no alignment and nothing outside [d_bytes, d_bytes + num_bytes) is read; the bytes
 * are not modified and may be released as soon as the call returns.  num_bytes == 0 (d_bytes may then be NULL) is the empty file;
 * d_bytes == NULL with num_bytes > 0 is GDF_INVALID_API_CALL.  read_csv itself is open + fstat + mmap + one upload + this call.
 */
gdf_error gdf_amd_read_csv_device(const char *d_bytes, size_t num_bytes, csv_read_arg *args);
/*
 * Releases everything a successful read_csv / gdf_amd_read_csv_device returned in args: the columns' device memory
 * (gdf_column_free), their names, the column structs and the array; then zeroes args->data, num_cols_out and num_rows_out.
 * Calling it again on the zeroed fields does nothing.  args == NULL: GDF_INVALID_API_CALL.
 */
gdf_error gdf_amd_read_csv_release(csv_read_arg *args);

/*
 * gdf_amd_order_by_ex -- ORDER BY that honours validity masks, with a direction and a null placement per column (csrc/order.hip).
 * gdf_order_by itself stays as the reference has it: ascending only, a mask is GDF_VALIDITY_UNSUPPORTED -- so a table that read_csv
 * returned (every column masked) is sorted through this entry.  out_indices receives the STABLE lexicographic row permutation.
 *
 *   cols         1 ... 16 key columns of equal size; the dtypes gdf_order_by takes (INT8 ... FLOAT64, DATE32, DATE64, TIMESTAMP)
 *   flags        HOST array of ncols bytes, GDF_AMD_ORDER_DESC | GDF_AMD_ORDER_NULLS_FIRST per column; NULL: all zero
 *   out_indices  caller-preallocated GDF_INT32 column without a mask, size == rows
 *
 * Value order  as gdf_order_by: integers signed, -0.0 == +0.0, every NaN equal to every other NaN and greater than +inf.  DESC is
 *              the exact reverse of that order, so NaN comes first among the values of a descending column.
 * Nulls        a row is null in column c when c has a mask and its bit is 0 (LSB first).  All nulls of a column compare equal and
 *              stand AFTER all its values, or before them with NULLS_FIRST -- whatever DESC says (SQL's absolute placement).  The
 *              data under a null bit is never compared and does not widen the integer range the images are built from.  valid ==
 *              NULL means no nulls; null_count is not consulted; mask bits beyond size are ignored; the mask needs no alignment.
 * Stability    rows that compare equal on all columns keep their input order, also under DESC (a reversed ascending sort is not
 *              this).  With no masks and all flags zero the permutation is gdf_order_by's, element for element.
 * Errors       all checked on the host before any device work, out_indices untouched: cols NULL, ncols <= 0 or a NULL element ->
 *              GDF_DATASET_EMPTY; ncols > 16 -> GDF_JOIN_TOO_MANY_COLUMNS; sizes differ -> GDF_COLUMN_SIZE_MISMATCH; a key dtype
 *              outside the list -> GDF_UNSUPPORTED_DTYPE; a flag byte with other bits -> GDF_INVALID_API_CALL; out_indices NULL, not
 *              GDF_INT32, of another size, or data == NULL with rows > 0 -> GDF_INVALID_API_CALL; out_indices with a mask ->
 *              GDF_VALIDITY_UNSUPPORTED; rows >= 2^31 - 1 -> GDF_COLUMN_SIZE_TOO_BIG.  rows == 0: success, nothing written.
 * Determinism  a second call on the same input gives a bit-identical result.  Runs on the legacy default stream and returns after
 *              the output is written.
 */
#define GDF_AMD_ORDER_DESC        1u   /* this column descending                          */
#define GDF_AMD_ORDER_NULLS_FIRST 2u   /* its nulls before every value (default: after)   */
gdf_error gdf_amd_order_by_ex(gdf_column **cols, int ncols, const uint8_t *flags, gdf_column *out_indices);

/*
 * gdf_amd_gather -- outs[c][i] = cols[c][indices[i]]: turns a row permutation (gdf_amd_order_by_ex) or the index columns of
 * gdf_inner_join / gdf_left_join / gdf_full_join, where -1 marks the missing side, into columns (csrc/order.hip).
 *
 *   indices   GDF_INT32 or GDF_INT64 without a mask, m rows; every value in [0, rows) or -1
 *   cols      ncols >= 1 source columns of equal size `rows`, any dtype get_column_byte_width knows; masks honoured
 *   outs      ncols column structs the call fills in: data and valid from rmmAlloc (release with gdf_column_free), size m, dtype
 *             and dtype_info of cols[c].  ALWAYS with a mask of ceil(m / 64) * 8 bytes whose bits beyond m are zero, and an exact
 *             null_count.  Row i is null -- with data element 0, so whole arrays compare equal -- where indices[i] is -1 or the
 *             source row is null.  m == 0: size 0, data == valid == NULL.
 *
 * Errors      nothing stays allocated, outs untouched: NULL arguments (also an element of cols / outs, or data of a column with rows)
 *             or ncols <= 0 -> GDF_DATASET_EMPTY; source sizes differ -> GDF_COLUMN_SIZE_MISMATCH; another index dtype or a source
 *             dtype without a byte width -> GDF_UNSUPPORTED_DTYPE; indices with a mask -> GDF_VALIDITY_UNSUPPORTED; an index < -1 or
 *             >= rows -> GDF_INVALID_API_CALL (found on the device; no address outside a source column is ever formed from it).
 * Determinism and stream as gdf_amd_order_by_ex.
 */
gdf_error gdf_amd_gather(gdf_column *indices, int ncols, gdf_column **cols, gdf_column **outs);

/*
 * gdf_amd_group_by_agg -- GROUP BY over 1 ... 16 key columns with any number of aggregates in ONE call (csrc/groupby_agg.hip):
 * SELECT k1, k2, SUM(a), AVG(a), MIN(b), COUNT(c), COUNT(*) ... GROUP BY k1, k2 over a table whose columns carry masks, as read_csv
 * returns it.  The five gdf_group_by_<op> entries stay as they are (one aggregate per call, caller-preallocated outputs of `rows`
 * elements, a row with a null key dropped by HASH and masks refused by SORT).
 *
 *   keys      1 ... 16 columns of equal size `rows`; the dtypes gdf_amd_order_by_ex takes; masks honoured
 *   values    0 ... 64 columns of that size; masks honoured
 *   aggs      HOST array of 1 ... 64 requests (column, op): column indexes values[], op is GDF_SUM, GDF_MIN, GDF_MAX, GDF_AVG or
 *             GDF_COUNT; column == -1 with GDF_COUNT is COUNT(*).  A value column may stand in any number of requests.
 *   out_keys  nkeys, out_aggs naggs column structs the call fills in, as gdf_amd_gather does: data and valid from rmmAlloc (release
 *             with gdf_column_free), size G = the number of groups.  EVERY output has a mask of ceil(G / 64) * 8 bytes whose bits
 *             beyond G are zero and an exact null_count; a null element has data 0.
 *
 * Groups       two rows belong to one group when in every key column they are both null, or both valid and equal under
 *              gdf_order_by's value equality: -0.0 == +0.0, every NaN equals every NaN.  The data under a null bit is never compared.
 *              Nulls FORM groups: (null, 1), (null, 2) and (1, null) are three groups.  (pandas' dropna: remove the output groups
 *              whose key masks have a zero bit.)  The groups come out in the order gdf_amd_order_by_ex(keys, flags = NULL) gives
 *              their rows: ascending, a column's nulls behind its values.
 * Key outputs  dtype and dtype_info of keys[c]; the element is the bits of the group's FIRST row in input order (which zero, which
 *              NaN payload); null where the group's key is null.
 * Aggregates   GDF_SUM    GDF_INT64 for INT8 ... INT64 values (wraps modulo 2^64), GDF_FLOAT64 for FLOAT32 / FLOAT64 (float32 widened
 *                         before the first add): the sum of the group's valid values; null when the group has none
 *              GDF_AVG    GDF_FLOAT64: (double)sum / count, sum as under GDF_SUM, count = the valid values; null when there is none
 *              GDF_MIN / GDF_MAX   dtype and dtype_info of the value column.  Integers signed; floats in gdf_order_by's order, NaN
 *                         above +inf: MAX is NaN if any valid value is, MIN only if all are (a canonical quiet NaN comes back);
 *                         of -0.0 and +0.0 either may come back.  Null when the group has no valid value
 *              GDF_COUNT  GDF_INT64: the valid values of values[column], or the rows of the group for column == -1; never null
 *              SUM and AVG take INT8 ... FLOAT64 values; MIN and MAX also DATE32, DATE64, TIMESTAMP; COUNT any dtype
 *              get_column_byte_width knows.
 * Determinism  a second call on the same input gives bit-identical outputs, float sums included: every fold has a fixed association
 *              order (which one is the implementation's) and no floating-point atomic takes part.  Runs on the legacy default stream
 *              and returns after the outputs are written.
 * Errors       all checked on the host before any device work, out_keys / out_aggs untouched, nothing stays allocated; in this order:
 *              keys NULL, nkeys <= 0 or a NULL element; nvalues < 0, or nvalues > 0 with values NULL or a NULL element; aggs NULL or
 *              naggs <= 0; out_keys / out_aggs NULL or a NULL element -> GDF_DATASET_EMPTY; nkeys > 16 -> GDF_JOIN_TOO_MANY_COLUMNS;
 *              nvalues > 64 or naggs > 64 -> GDF_INVALID_API_CALL; a key or value size other than keys[0]->size ->
 *              GDF_COLUMN_SIZE_MISMATCH; a key dtype outside the list -> GDF_UNSUPPORTED_DTYPE; then per request in array order: another
 *              op (GDF_COUNT_DISTINCT too) -> GDF_UNSUPPORTED_METHOD, column outside [-1, nvalues) or -1 without GDF_COUNT ->
 *              GDF_INVALID_API_CALL, a value dtype the op does not take -> GDF_UNSUPPORTED_DTYPE; rows >= 2^31 - 1 ->
 *              GDF_COLUMN_SIZE_TOO_BIG; rows > 0 and a key or a referenced value column without data -> GDF_DATASET_EMPTY.
 *              rows == 0: success without device work, every output of size 0 with data == valid == NULL, null_count 0 and the dtype
 *              and dtype_info it would have had.
 */
typedef struct gdf_amd_agg { int32_t column; int32_t op; } gdf_amd_agg;   /* column: index into values[]; -1 with GDF_COUNT = COUNT(*) */
gdf_error gdf_amd_group_by_agg(gdf_column **keys, int nkeys, gdf_column **values, int nvalues, const gdf_amd_agg *aggs, int naggs,
                               gdf_column **out_keys, gdf_column **out_aggs);

/*
 * gdf_amd_top_k -- ORDER BY ... LIMIT k OFFSET offset without sorting the table (csrc/topk.hip): a radix selection over a 64-bit
 * image of the key, then a sort of the few rows that can make the cut.
 *
 *   cols, flags  exactly as for gdf_amd_order_by_ex: 1 ... 16 key columns, the same dtypes, masks honoured at any alignment,
 *                null_count not consulted, the data under a null bit never loaded for comparison; flags a HOST array or NULL
 *   k, offset    the LIMIT and the OFFSET; with rows = cols[0]->size, m = max(0, min(k, rows - offset)) rows come back
 *   out_indices  caller-preallocated GDF_INT32 column without a mask, size == m (the caller knows rows, k and offset)
 *
 * Result       let P be the permutation gdf_amd_order_by_ex(cols, ncols, flags, ...) writes for the same arguments:
 *              out_indices[i] = P[offset + i] for 0 <= i < m, element for element.  Value order, null placement, DESC, NaN, +-0.0
 *              and stability are therefore gdf_amd_order_by_ex's: among rows equal on every key column the lower row number comes
 *              first, and it is also the one that makes the cut.  Nothing outside the first m elements is written.
 * Errors       all checked on the host before any device work, out_indices untouched; in this order: gdf_amd_order_by_ex's checks
 *              on cols, ncols, sizes, dtypes and flags, with its codes; k < 0 or offset < 0 -> GDF_INVALID_API_CALL; out_indices
 *              NULL, not GDF_INT32, size != m, or data == NULL with m > 0 -> GDF_INVALID_API_CALL; out_indices with a mask ->
 *              GDF_VALIDITY_UNSUPPORTED; rows >= 2^31 - 1 -> GDF_COLUMN_SIZE_TOO_BIG; m > 0 and a key column without data ->
 *              GDF_DATASET_EMPTY.  m == 0 (k == 0, rows == 0 or offset >= rows): success without device work.
 * Determinism and stream as gdf_amd_order_by_ex.
 */
gdf_error gdf_amd_top_k(gdf_column **cols, int ncols, const uint8_t *flags, int64_t k, int64_t offset, gdf_column *out_indices);

/*
 * gdf_amd_semi_join -- SELECT ... FROM L WHERE [NOT] EXISTS (SELECT 1 FROM R WHERE L.k1 = R.k1 AND L.k2 = R.k2 ...): the row numbers
 * of the left rows that have (GDF_AMD_SEMI_ANTI: have not) a partner among the right rows (csrc/semijoin.hip).  pandas' isin over
 * several columns, merge(how = "leftsemi" / "leftanti").  At most 4 bytes come back per left row however often the right keys repeat.
 *
 *   left_cols, right_cols   ncols (1 ... 16) key columns each, sizes equal within a side; the dtypes gdf_amd_order_by_ex takes, with
 *                           left_cols[c]->dtype == right_cols[c]->dtype (dtype_info is not consulted, as in the joins).  Masks are
 *                           honoured at any byte alignment, null_count is not consulted, mask bits beyond size are ignored, and the
 *                           data under a null bit is never loaded for comparison.
 *   flags                   GDF_AMD_SEMI_ANTI | GDF_AMD_SEMI_NULLS_EQUAL, or 0
 *   out_indices             filled in by the call, as the joins fill in their index columns: GDF_INT32, data from rmmAlloc (release
 *                           with gdf_column_free), valid == NULL, null_count == 0, size == m.  m == 0: size 0 and data == NULL.
 *
 * Match        a left row has a partner when some right row agrees with it in every key column.  Values agree exactly as in
 *              gdf_inner_join: integers by value, floats by ==, so -0.0 == +0.0 and a NaN equals nothing, itself included, under
 *              either flag.  Without NULLS_EQUAL a row with a null in any key column has no partner and is no partner (the joins'
 *              rule).  With NULLS_EQUAL two elements of a column also agree when both are null (IS NOT DISTINCT FROM); a null never
 *              agrees with a value.  Consequence: ANTI without NULLS_EQUAL RETURNS the left rows with a null key -- that is NOT EXISTS,
 *              not NOT IN.
 * Result       the row numbers of the qualifying left rows in ASCENDING order, each once: gdf_amd_gather(out_indices, L ...) is the
 *              filtered table in input order.  A right side without rows gives nothing for SEMI and every left row for ANTI.
 * Determinism and stream as gdf_amd_order_by_ex: a second call is bit-identical; the call runs on the legacy default stream and
 *              returns after the output is written.
 * Errors       all checked on the host before any device work, out_indices untouched, nothing stays allocated; in this order:
 *              left_cols / right_cols / out_indices NULL, ncols <= 0 or a NULL element -> GDF_DATASET_EMPTY; ncols > 16 ->
 *              GDF_JOIN_TOO_MANY_COLUMNS; sizes differ within a side -> GDF_COLUMN_SIZE_MISMATCH; a dtype outside the list (either
 *              side) -> GDF_UNSUPPORTED_DTYPE; left / right dtype of a column differ -> GDF_JOIN_DTYPE_MISMATCH; flag bits other than
 *              the two -> GDF_INVALID_API_CALL; either side has >= 2^31 - 1 rows -> GDF_COLUMN_SIZE_TOO_BIG; a column of a side that
 *              has rows, with data == NULL -> GDF_DATASET_EMPTY.
 */
#define GDF_AMD_SEMI_ANTI        1u   /* return the left rows WITHOUT a partner (NOT EXISTS)            */
#define GDF_AMD_SEMI_NULLS_EQUAL 2u   /* a null key equals a null key (IS NOT DISTINCT FROM)             */
gdf_error gdf_amd_semi_join(gdf_column **left_cols, gdf_column **right_cols, int ncols, uint32_t flags, gdf_column *out_indices);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GDF_AMD_EXT_H */
