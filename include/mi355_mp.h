/*
 * mi355_mp.h — C-ABI of the MI355X (gfx950) message-passing aggregation engine.
 *
 * This is the drop-in boundary for the hot path of PyG 1.4.3
 * `MessagePassing.propagate()` (gather x_j / x_i -> message -> scatter-reduce)
 * and of the torch_scatter 2.0.4 ops it calls.  Upstream those live in
 * unvendored dependencies pinned at /root/reference/requirement.txt:1-7
 * (torch_sparse 0.6.1, torch-scatter 2.0.4, torch-geometric 1.4.3); the
 * reference tree itself only calls them (examples/gcn.py:18-27,
 * ConvexPruning.py:180-224, examples/ppi.py:22-28, README.md:35-49,
 * gmm_conv.py:131-144).  See SURVEY.md section 8b for the schema list.
 *
 * Conventions
 *   - Plain pointers to DEVICE memory, int64 sizes, a hipStream_t passed as
 *     `void* stream` (NULL = default stream).  No torch types.
 *   - Every entry point only enqueues work on `stream`; none allocates, frees
 *     or synchronises, so every call is hipGraph-capturable.  Work runs on
 *     the stream's device: the calling thread's current device is switched
 *     for the call when it differs, and restored.  The caller owns
 *     all outputs and workspaces (sizes from the *_bytes queries).
 *   - Return value: MP_OK or an MP_ERR_* code; mp_last_error() gives the text
 *     (thread-local).
 *   - Extents (ABI 6): every caller-allocated workspace, partial or per-edge
 *     array whose size is not fixed by the call's own row / edge counts alone
 *     is passed with its size in bytes (`*_bytes`).  A buffer shorter than the
 *     call needs is rejected with MP_ERR_ARG before anything is launched, so a
 *     mis-sized array is an error, never an out-of-bounds device write.
 *   - Graph structure is a destination-sorted CSR (stable: inside a row the
 *     edges keep their original order), described by `mp_csr`.  All kernels
 *     are deterministic: no float atomics on any forward output.
 */
#ifndef MI355_MP_H
#define MI355_MP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MP_ABI_VERSION 7

/* status codes */
#define MP_OK 0
#define MP_ERR_ARG 1   /* bad argument (shape, alignment, null pointer) */
#define MP_ERR_HIP 2   /* a HIP runtime call failed */

/* reductions (torch_scatter names: sum/add, mean, max, min) */
#define MP_REDUCE_SUM 0
#define MP_REDUCE_MEAN 1
#define MP_REDUCE_MAX 2
#define MP_REDUCE_MIN 3

/* aggregate flags */
#define MP_FLAG_INIT_FROM_OUT 1 /* torch_scatter `out=` given: reduce into out's values */
#define MP_FLAG_PYG_MASK 2      /* torch_geometric.utils.scatter_: max -> out<-10000 := 0,
                                   min -> out>10000 := 0 */
#define MP_FLAG_SKIP_EMPTY 4    /* (ABI 7, mp_aggregate_tiles_f32 only) rows with no slot are left
                                   untouched: no store, no bias */

/* aggregate stages (bench times the main kernel on its own) */
#define MP_STAGE_MAIN 1
#define MP_STAGE_FIXUP 2
#define MP_STAGE_STATS 4  /* mp_gat_softmax_aggregate_f32: the softmax row-statistics passes */
#define MP_STAGE_ALL 7

/*
 * Destination-sorted CSR plus its edge-balanced ("merge-path") schedule.
 *   rowptr[n_rows+1]      row r owns CSR slots [rowptr[r], rowptr[r+1])
 *   col[n_edges]          gather row for each slot (source node, or message row);
 *                         NULL = identity (row k of x for slot k: values already
 *                         in CSR slot order)
 *   eid[n_edges]          original edge position of each slot (argmax output)
 * Schedule (merge-path over the N+E work items "row r" and "slot k"; row r
 * sits at merged position rowptr[r]+r, slot k of row r at k+r+1):
 *   wave task w covers merged positions [w*chunk, (w+1)*chunk)
 *   wave_row[n_waves+1]   first row whose marker lies in task w (owned rows)
 *   wave_slot[n_waves+1]  first CSR slot processed by task w
 *   split_waves[n_split]  for each row whose slots span several tasks, the
 *                         last task touching it (fix-up list)
 *   n_cols                number of rows of the gathered tensor (x, or the
 *                         messages when col == eid); required (> 0) with col
 */
typedef struct mp_csr {
  const int32_t* rowptr;
  const int32_t* col;
  const int32_t* eid;
  const int32_t* wave_row;
  const int32_t* wave_slot;
  const int32_t* split_waves;
  int64_t n_rows;
  int64_t n_edges;
  int32_t chunk;
  int32_t n_waves;
  int32_t n_split;
  int32_t n_cols;   /* rows of the gathered x; must be > 0 whenever col != NULL (MP_ERR_ARG
                       otherwise).  It bounds the 32-bit buffer offsets of the gather. */
  int64_t n_ids;    /* size of the edge-id space the eid array indexes: the arg an empty
                       max/min row reports (torch_scatter's src.size(0)).  0 = n_edges.  A CSR
                       whose slots are a subset of the edges (first occurrences of repeated
                       (row, column) pairs) sets it to the full edge count.  (ABI 2) */
} mp_csr;

const char* mp_last_error(void);
int mp_abi_version(void);
/* First 16 hex digits of the sha256 of the native sources this library was
 * compiled from (csrc/Makefile computes it; mi355_mp._lib.source_hash() is the
 * same scheme over the tree).  The Python loader refuses a library whose hash
 * differs from the sources beside it: a stale prebuilt .so never runs.  (ABI 3) */
const char* mp_source_hash(void);

/* Process-wide dispatch table (tests and in-process A/B runs).  Sets `key`
 * to `value` and returns the previous value; value < 0 only queries.
 * Unknown keys return -1.  Every setting gives bitwise-identical results;
 * only the kernel shape changes.  "Flat kernel" = k_agg_flat, the
 * sum/mean/max/min kernel whose tasks stream their slots across row ends.
 *   MP_TUNE_FLAT_VEC1_MIN_BYTES: flat sum/mean over a gathered x of at least
 *     this many bytes use 64-feature tiles (VEC=1); smaller x uses
 *     MP_TUNE_FLAT_VEC.  Default 0 (always 64-feature tiles).
 *   MP_TUNE_FLAT_SMEM: 1 (default) = the flat sum/mean kernel reads slot
 *     columns / weights through scalar-cache batches and gathers with 32-bit
 *     buffer offsets whenever the gathered x spans < 4 GiB; 0 = the per-lane
 *     slot window.
 *   MP_TUNE_FLAT_MIN_F: narrowest sum/mean row (features) that takes the
 *     flat kernel (default 64); narrower rows use lane groups / lane tasks.
 *   MP_TUNE_FLAT_MIN_F_ARG: the same for max/min (default 64).
 *   MP_TUNE_FLAT_NARROW_VEC1: flat rows of at most this many features use
 *     64-feature tiles (VEC=1) whatever the other keys say (default 64: a
 *     64-feature row fills one VEC=1 tile, where VEC=2 would idle half the lanes).
 *   MP_TUNE_FLAT_VEC / MP_TUNE_FLAT_VEC_ARG: features per lane of the flat
 *     kernel for sum/mean (below the VEC1 size threshold) and for max/min:
 *     1, 2 (default) or 4 -- feature tiles of 64, 128 or 256.
 *   MP_TUNE_FLAT_SEQ_TILES: 1 = the flat kernel's feature tiles run one after
 *     another on all eight XCDs; 0 (default) = XCD-affine tiles.
 *   MP_TUNE_FLAT_FAR_MIN_BYTES: the scalar-batch sum/mean kernel keeps 8
 *     instead of 16 row loads in flight per wave over a gathered x larger than
 *     this (default 256 MiB, the Infinity Cache).
 *   MP_TUNE_GAT_BWD_VEC: features per lane of the GAT backward's transposed
 *     pass (mp_gat_backward_*_f32 with C/4 a power of two): 4 (default,
 *     256-feature tiles), 2 or 1 (128- / 64-feature XCD-affine tiles, taken
 *     when a head fits inside one tile).  The exception to the rule above:
 *     the per-slot <g_i, xw_j> sums its features in another order, so the
 *     gradients agree to rounding, not bit for bit.
 *   MP_TUNE_TOPK_WG_LIMIT: the largest graph (nodes) mp_topk_select_f32 ranks
 *     by counting inside one workgroup (default 2048; 64..8192, else -1);
 *     larger graphs are sorted.  mp_topk_path reports the path of a size. */
#define MP_TUNE_FLAT_VEC1_MIN_BYTES 1
#define MP_TUNE_FLAT_SMEM 2
#define MP_TUNE_FLAT_MIN_F 3
#define MP_TUNE_FLAT_MIN_F_ARG 4
#define MP_TUNE_FLAT_NARROW_VEC1 5
#define MP_TUNE_FLAT_VEC 6
#define MP_TUNE_FLAT_VEC_ARG 7
#define MP_TUNE_FLAT_SEQ_TILES 8
#define MP_TUNE_FLAT_FAR_MIN_BYTES 9
#define MP_TUNE_GAT_BWD_VEC 10
#define MP_TUNE_TOPK_WG_LIMIT 11
int64_t mp_tune(int32_t key, int64_t value);

/* ---- CSR build (replaces the sort/bucketing torch_scatter never did: upstream
 *      scatter_add_ walks edges in original order) ---------------- */

/* Workspace bytes for mp_csr_build. */
size_t mp_csr_build_workspace(int64_t n_edges, int64_t n_rows);

/* Stable sort of edges by key (edge_index[i], the aggregation index).
 *   key[n_edges], other[n_edges]: int64 (rows of edge_index; any stride-1 view)
 *   other may be NULL: then col[k] = eid[k] (aggregating materialised messages).
 *   rowptr[n_rows+1], col[n_edges], eid[n_edges]: int32 outputs.
 *   bad[1]: device int32, set to the number of key/other entries outside
 *   [0,n_rows) / [0,n_other).  Replaces the index->CSR step of
 *   torch_scatter segment_csr callers; PyG 1.4.3 scatter_ itself sorts nothing. */
int mp_csr_build(const int64_t* key, const int64_t* other, int64_t n_edges,
                 int64_t n_rows, int64_t n_other, int32_t* rowptr, int32_t* col,
                 int32_t* eid, int32_t* bad, void* ws, size_t ws_bytes,
                 void* stream);

/* Number of wave tasks for `chunk` merged positions per task (chunk a multiple of 8, >= 16). */
int32_t mp_schedule_n_waves(int64_t n_rows, int64_t n_edges, int32_t chunk);
size_t mp_schedule_workspace(int32_t n_waves);

/* Builds wave_row[n_waves+1], wave_slot[n_waves+1] and split_waves[<=n_waves];
 * writes the split count to n_split_dev[0] (device int32).  A task boundary
 * that falls inside a row of <= snap slots is moved back to that row's start
 * (0 <= snap < chunk-1), so only longer rows are ever split. */
int mp_schedule_build(const int32_t* rowptr, int64_t n_rows, int64_t n_edges,
                      int32_t chunk, int32_t snap, int32_t* wave_row, int32_t* wave_slot,
                      int32_t* split_waves, int32_t* n_split_dev, void* ws,
                      size_t ws_bytes, void* stream);

/* ---- fused gather -> (weight) -> segment reduce ---------------------------
 * out[r, :] = REDUCE_{k in row r} ( w[k] * x[col[k], :] )     (w optional)
 * Replaces: index_select(x, edge_index[j]) (PyG MessagePassing.__collect__),
 * message() = norm.view(-1,1)*x_j (GCNConv) or x_j, and
 * torch_scatter scatter_sum/scatter_mean/scatter_max/scatter_min [U8/U9],
 * torch_geometric.utils.scatter_ [U2] (MP_FLAG_PYG_MASK), update() += bias.
 *   w:      CSR-ordered per-slot weights or NULL
 *   x:      [*, ldx] fp32 rows, F features used
 *   bias:   [F] or NULL (added after the reduction, as GCNConv.update)
 *   out:    [n_rows, ldo] fp32
 *   arg_out:[n_rows, F] int64 (max/min only, else NULL): original edge
 *           position of the first maximal element, n_edges for empty rows
 *   slab:   workspace of mp_aggregate_slab_bytes() bytes
 */
size_t mp_aggregate_slab_bytes(const mp_csr* g, int32_t F, int32_t reduce);
int mp_aggregate_f32(const mp_csr* g, const float* w, const float* x,
                     int64_t ldx, int32_t F, int32_t reduce, int32_t flags,
                     const float* bias, float* out, int64_t ldo,
                     int64_t* arg_out, void* slab, size_t slab_bytes,
                     int32_t stages, void* stream);

/* mp_aggregate_f32 for sum / mean over TILE-MAJOR operands (ABI 7): the
 * sharded step's feature tiles (mi355_mp.dist.OverlappedAggregation) in ONE
 * launch per pass instead of one launch per tile.  With x_tile_w > 0, feature f
 * of row r of x lives at x[(f / x_tile_w) * x_tile_stride + r * x_tile_w +
 * f % x_tile_w] (ldx ignored), else at x[r * ldx + f]; likewise out with
 * out_tile_w / out_tile_stride (ldo ignored), else out[r * ldo + f].  Tile
 * widths are multiples of 64 dividing F (F a multiple of 64) and tiles do not
 * overlap (stride >= rows x width: g->n_cols rows of x, g->n_rows rows of
 * out); bias is [F] as ever, and bias_rows (NULL, or int32 [g->n_rows])
 * limits it to the rows r with bias_rows[r] != 0.  flags: MP_FLAG_INIT_FROM_OUT
 * and / or MP_FLAG_SKIP_EMPTY (rows without slots keep out as it is).  The graph
 * needs its column array.  Per row and feature the arithmetic is exactly
 * mp_aggregate_f32's on the same values laid out row-major: the results are
 * bitwise equal.  Replaces, for one rank's step, the per-tile
 * scatter_add(norm * x_j) of the reference's propagate (gcn_conv.py [U5]). */
int mp_aggregate_tiles_f32(const mp_csr* g, const float* w, const float* x,
                           int64_t ldx, int32_t x_tile_w, int64_t x_tile_stride,
                           int32_t F, int32_t reduce, int32_t flags,
                           const float* bias, const int32_t* bias_rows,
                           float* out, int64_t ldo,
                           int32_t out_tile_w, int64_t out_tile_stride,
                           void* slab, size_t slab_bytes, int32_t stages,
                           void* stream);

/* Name (demangled) of the main kernel mp_aggregate_f32 would launch for these
 * arguments (same shape selection, nothing launched), written to buf.  Lets a
 * profile summary be matched to the dispatched kernel (bench.py).  Needs a
 * HIP device for the name lookup; MP_ERR_ARG when none is available. */
int mp_aggregate_kernel_name(const mp_csr* g, const float* w, const float* x,
                             int64_t ldx, int32_t F, int32_t reduce,
                             const float* bias, const float* out, int64_t ldo,
                             char* buf, size_t buf_len, void* stream);

/* ---- GATConv fused attention aggregation (call stack 3.2) ---
 * a_dst[n,h] = <xw[n,h,:], att[h,0:C]>,  a_src[n,h] = <xw[n,h,:], att[h,C:2C]>
 * (the split of (cat[x_i,x_j]*att).sum(-1) of GATConv.message [U6]). */
int mp_gat_node_scores_f32(const float* xw, int64_t n_nodes, int32_t H,
                           int32_t C, const float* att, float* a_src,
                           float* a_dst, void* stream);

/* out[i,h,:] = sum_k softmax_k(leaky_relu(a_src[col_k,h]+a_dst[i,h])) x[col_k,h,:]
 * with torch_geometric.utils.softmax's +1e-16 denominator, single pass
 * (online max/sum), optional bias [H*C], optional row_stats[n_rows,H,2] =
 * (max, denominator) for mp_gat_alpha_f32. */
size_t mp_gat_slab_bytes(const mp_csr* g, int32_t H, int32_t C);
int mp_gat_aggregate_f32(const mp_csr* g, const float* xw, const float* a_src,
                         const float* a_dst, int32_t H, int32_t C, float slope,
                         const float* bias, float* out, int64_t ldo,
                         float* row_stats, void* slab, size_t slab_bytes,
                         int32_t stages, void* stream);
/* The same with att [H, 2C] (GATConv.att): where C % 4 == 0 and C/4 is a
 * power of two <= 64, the kernel recomputes a_src[j,h] from each gathered xw
 * row (bitwise the value mp_gat_node_scores_f32 stores) instead of gathering
 * it; other shapes, or att == NULL, read a_src. */
int mp_gat_aggregate_att_f32(const mp_csr* g, const float* xw, const float* a_src,
                             const float* a_dst, const float* att, int32_t H,
                             int32_t C, float slope, const float* bias, float* out,
                             int64_t ldo, float* row_stats, void* slab,
                             size_t slab_bytes, int32_t stages, void* stream);

/* The same forward with the node scores computed in-kernel (C % 4 == 0 and
 * C/4 a power of two <= 64: mp_gat_train_ok; xw, att, bias, out 16-byte
 * aligned; the graph square -- row i's own xw is row i of xw): a_src / a_dst
 * [n_rows, H] are OUTPUTS, each destination row's scores reduced from its own
 * xw row with mp_gat_node_scores_f32's arithmetic (bitwise its values), so no
 * separate node-score pass over xw runs.  a_src is also recomputed from every
 * gathered row (as mp_gat_aggregate_att_f32).  (ABI 3) */
int mp_gat_forward_f32(const mp_csr* g, const float* xw, const float* att, int32_t H,
                       int32_t C, float slope, const float* bias, float* out, int64_t ldo,
                       float* a_src, float* a_dst, float* row_stats, void* slab,
                       size_t slab_bytes, int32_t stages, void* stream);

/* Training forward of the same layer (C % 4 == 0; with att given and C/4 a power
 * of two <= 64 -- mp_gat_train_ok -- a_src comes from each gathered row, else
 * from the a_src array).  out = aggregate + bias (bias may be NULL); agg
 * (optional, NULL allowed) also receives the pre-bias aggregate [n_rows, H*C]
 * (contiguous).  The backward's rs needs no such copy: the prologues take the
 * output and the bias (ABI 6: rs over out - bias).  Besides these and row_stats it
 * leaves, with the same online rescaling,
 *   out2[i,h,:]  = sum_j alpha_ij leaky'_ij xw[j,h,:]    ([n_rows, H*C], contiguous)
 *   row_s2[i,h]  = sum_j alpha_ij leaky'_ij             ([n_rows, H])
 * with leaky' = 1 where a_src[j,h] + a_dst[i,h] > 0, else slope.  They turn the
 * backward's d a_dst into a node-wise quantity (mp_gat_backward_prep_train_f32),
 * so mp_gat_backward_f32 then runs with de = NULL.
 * Slab: mp_gat_train_slab_bytes(g, H, C). */
int mp_gat_train_ok(int32_t H, int32_t C);
size_t mp_gat_train_slab_bytes(const mp_csr* g, int32_t H, int32_t C);
int mp_gat_aggregate_train_f32(const mp_csr* g, const float* xw, const float* a_src,
                               const float* a_dst, const float* att, int32_t H, int32_t C,
                               float slope, const float* bias, float* out, int64_t ldo,
                               float* agg, float* row_stats, float* out2, float* row_s2,
                               void* slab, size_t slab_bytes, int32_t stages, void* stream);
/* mp_gat_aggregate_train_f32 with the node scores computed in-kernel (the
 * outputs a_src / a_dst, as mp_gat_forward_f32). */
int mp_gat_forward_train_f32(const mp_csr* g, const float* xw, const float* att, int32_t H,
                             int32_t C, float slope, const float* bias, float* out, int64_t ldo,
                             float* agg, float* row_stats, float* out2, float* row_s2,
                             float* a_src, float* a_dst, void* slab, size_t slab_bytes,
                             int32_t stages, void* stream);

/* Two-pass form of the same layer, in the reference's own arithmetic
 * (utils.softmax [U3] then message x_j * alpha and scatter_add in edge order,
 * GATConv.update + bias [U6]):
 *   MP_STAGE_STATS: row_stats[r,h,0] = m = max_k leaky(a_src[col_k,h] + a_dst[r,h]),
 *                   row_stats[r,h,1] = sum_k exp(leaky(.) - m) + 1e-16 (CSR order)
 *   MP_STAGE_MAIN/FIXUP: out[r,h,:] = sum_k (exp(leaky(.) - m) / den) * xw[col_k,h,:] + bias
 * slot_row from mp_csr_slot_rows.  Shapes: mp_gat_two_pass_ok(H, C) != 0
 * (H <= 16; C = 16, 32 or a multiple of 64).  Rows not split across tasks
 * follow the reference's operation order exactly. */
int mp_gat_two_pass_ok(int32_t H, int32_t C);
int mp_gat_softmax_aggregate_f32(const mp_csr* g, const int32_t* slot_row, const float* xw,
                                 const float* a_src, const float* a_dst, int32_t H, int32_t C,
                                 float slope, const float* bias, float* out, int64_t ldo,
                                 float* row_stats, void* slab, size_t slab_bytes,
                                 int32_t stages, void* stream);

/* ---- GATConv backward pieces ------------------------------ */

/* slot_row[k] = the row owning CSR slot k (one-time per graph). */
int mp_csr_slot_rows(const mp_csr* g, int32_t* slot_row, void* stream);

/* alpha_csr[k,h] = exp(leaky(a_src[col_k,h]+a_dst[r,h]) - m[r,h]) / den[r,h]
 * and (if score != NULL) score[k,h] = a_src[col_k,h] + a_dst[r,h] (the
 * pre-activation), both in CSR slot order, r = slot_row[k]. */
int mp_gat_alpha_csr_f32(const mp_csr* g, const int32_t* slot_row, const float* a_src,
                         const float* a_dst, int32_t H, float slope, const float* row_stats,
                         float* alpha_csr, float* score, void* stream);

/* Per-head weighted aggregation: with C = F / H,
 * out[r, h*C + c] = sum_k w[k*H + h] * x[col[k], h*C + c]   (w in CSR slot order)
 * (GATConv's d out / d x_j = alpha, applied over the transposed CSR). */
int mp_aggregate_heads_f32(const mp_csr* g, const float* w, int32_t H, const float* x,
                           int64_t ldx, int32_t F, float* out, int64_t ldo, void* slab,
                           size_t slab_bytes, int32_t stages, void* stream);

/* Sampled dense-dense product over CSR slots (GAT d alpha):
 * out[k*H + h] = sum_c grow[r, h*C + c] * x[col[k], h*C + c], r = slot_row[k]. */
int mp_gat_sddmm_f32(const mp_csr* g, const int32_t* slot_row, const float* grow, int64_t ldg,
                     const float* x, int64_t ldx, int32_t H, int32_t C, float* out,
                     void* stream);

/* Fused GATConv backward over the TRANSPOSED CSR `gt` (rows = source nodes j,
 * col = destination i, slots in original edge order).  Replaces the autograd
 * of GATConv.message + utils.softmax + scatter_add (PyG 1.4.3 [U3,U6];
 * /root/reference/ConvexPruning.py:209-214) with one gather of grad_out rows:
 *   grad_xw[j]      = sum_i alpha_ij g_i + grad_a_src[j,h] * att[h, C:]
 *   de[k, h]        = alpha_ij (<g_i, xw_j>_h - rs[i,h]) leaky'(a_src[j,h]+a_dst[i,h])
 *   grad_a_src[j,h] = sum over the row of de
 * alpha_ij = exp(leaky(score) - m_i) / den_i from the forward's row_stats.
 * pack [n_dst, H, 4] = mp_gat_backward_prep_f32 output.  de [gt.n_edges, H]
 * (de_bytes >= gt.n_edges * H * 4; ABI 6): de[gt.eid[k], h]
 * receives slot k's value: pass the destination-CSR slot of each edge in
 * gt.eid to get de in destination-CSR order (then d a_dst is a contiguous
 * segmented sum: mp_aggregate_f32 with col = NULL).  de = NULL skips it (the
 * training forward's out2 / row_s2 give d a_dst directly).  Needs C/4 or C to
 * be a power of two <= 64.
 * Slab: mp_gat_slab_bytes(gt, H, C). */
int mp_gat_backward_f32(const mp_csr* gt, const float* grad_out, int64_t ldg, const float* xw,
                        const float* a_src, const float* pack, const float* att, int32_t H,
                        int32_t C, float slope, float* grad_xw, float* grad_a_src, float* de,
                        size_t de_bytes, void* slab, size_t slab_bytes, int32_t stages,
                        void* stream);

/* The same pass after the training forward: no per-edge d score; grad_a_dst
 * [n_rows, H] (mp_gat_backward_prep_train_f32) is an input, and each row's
 * grad_xw also receives grad_a_dst[j,h] * att[h, 0:C] (the term
 * mp_gat_backward_finish_f32 adds otherwise; call that with grad_xw = NULL for
 * the att-gradient partials only). */
int mp_gat_backward_train_f32(const mp_csr* gt, const float* grad_out, int64_t ldg, const float* xw,
                              const float* a_src, const float* pack, const float* att, int32_t H,
                              int32_t C, float slope, const float* grad_a_dst, float* grad_xw,
                              float* grad_a_src, void* slab, size_t slab_bytes, int32_t stages,
                              void* stream);

/* pack[n,h,:] = (a_dst[n,h], m[n,h], 1/den[n,h], rs[n,h]) with
 * rs[n,h] = sum_c grad_out[n, h*C+c] * agg[n, h*C+c]  (agg = pre-bias GAT output;
 * rs = sum_j alpha_nj <g_n, xw_j>_h, the softmax-backward row term).
 * bias (ABI 6; NULL = none): agg is then the layer OUTPUT agg + bias [H*C] and
 * rs is taken over out - bias (one rounding per feature), so the forward need
 * not keep a pre-bias copy; 16-byte aligned.
 * gsum_part (optional, [mp_gat_bwd_blocks(n), H*C], needs C%4==0, H*C<=256):
 * per-block column sums of grad_out (the bias gradient is their sum over blocks).
 * Extents (ABI 6): pack_bytes >= n*H*16, gsum_part_bytes >= mp_gat_bwd_blocks(n)*H*C*4
 * (ignored when gsum_part is NULL). */
int mp_gat_backward_prep_f32(const float* grad_out, int64_t ldg, const float* agg, int64_t lda,
                             const float* bias, const float* a_dst, const float* row_stats, int64_t n, int32_t H,
                             int32_t C, float* pack, size_t pack_bytes, float* gsum_part,
                             size_t gsum_part_bytes, void* stream);

/* The same prologue after mp_gat_aggregate_train_f32 (C % 4 == 0, C/4 a power
 * of two <= 64, 16-byte aligned rows), which also writes
 *   grad_a_dst[n,h] = sum_j de_nj = <grad_out[n,h,:], agg2[n,h,:]> - rs[n,h] * row_s2[n,h]
 * (agg2 / row_s2 = the training forward's out2 / row_s2). */
int mp_gat_backward_prep_train_f32(const float* grad_out, int64_t ldg, const float* agg, int64_t lda,
                                   const float* bias, const float* agg2, const float* row_s2, const float* a_dst,
                                   const float* row_stats, int64_t n, int32_t H, int32_t C,
                                   float* pack, size_t pack_bytes, float* gsum_part,
                                   size_t gsum_part_bytes, float* grad_a_dst, void* stream);

/* ---- GATConv with heads of any width (C % 4 == 0) --------------------------
 * The reference's own GAT stacks (ConvexPruning.py:209-214) use heads = 1 and
 * out_channels drawn at random (:106-114), so a head is often wider than one
 * 256-feature tile or C/4 is not a power of two.  For those shapes:
 *   forward: mp_gat_node_scores_wide_f32 (one wave per node, per-head dot
 *     products in 256-feature chunks), then mp_gat_aggregate_f32 (inference)
 *     or mp_gat_aggregate_train_f32 / _drop_f32 (training; these now take any
 *     C % 4 == 0: a_src is read from the node-score array when C/4 is not a
 *     power of two <= 64 or att is NULL);
 *   backward: mp_gat_backward_prep_wide_f32 (pack + node-wise d a_dst, as
 *     mp_gat_backward_prep_train_f32), mp_gat_backward_wide_f32 over the
 *     transposed CSR (no per-slot dot product:
 *       grad_xw[j] = sum_i alpha d g_i,  acc2[j] = sum_i lk alpha d g_i,
 *       sc[j,h] = sum_i lk alpha rs_i,   lk = leaky'(score), d = dropout factor
 *     (p_drop = 0: none; else the eid channel must hold each edge's dst-CSR
 *     slot), slab mp_gat_train_slab_bytes(gt, H, C)), then
 *     mp_gat_backward_epilogue_wide_f32: grad_a_src = <acc2, xw>_h - sc (written
 *     over sc) and grad_xw += grad_a_src att[h, C:] + grad_a_dst att[h, :C].
 * Rows contiguous [n, H*C] unless an ld is given; 16-byte aligned.
 * Extents (ABI 6): pack_bytes >= n*H*16; acc2_bytes >= gt->n_rows*H*C*4,
 * sc_bytes >= gt->n_rows*H*4. */
int mp_gat_wide_ok(int32_t H, int32_t C);
int mp_gat_node_scores_wide_f32(const float* xw, int64_t n_nodes, int32_t H, int32_t C, const float* att,
                                float* a_src, float* a_dst, void* stream);
int mp_gat_backward_prep_wide_f32(const float* grad_out, int64_t ldg, const float* agg, int64_t lda,
                                  const float* bias, const float* agg2, const float* row_s2, const float* a_dst,
                                  const float* row_stats, int64_t n, int32_t H, int32_t C, float* pack,
                                  size_t pack_bytes, float* grad_a_dst, void* stream);
int mp_gat_backward_wide_f32(const mp_csr* gt, const float* grad_out, int64_t ldg, const float* a_src,
                             const float* pack, int32_t H, int32_t C, float slope, uint64_t seed, float p_drop,
                             const int32_t* drop_ids, float* grad_xw, float* acc2, size_t acc2_bytes, float* sc, size_t sc_bytes,
                             void* slab, size_t slab_bytes, int32_t stages, void* stream);
int mp_gat_backward_epilogue_wide_f32(float* grad_xw, const float* acc2, const float* xw, const float* att,
                                      const float* grad_a_dst, float* sc_grad_a_src, int64_t n, int32_t H,
                                      int32_t C, void* stream);

/* ---- Batch.from_data_list on the replica's device ------------------------
 * torch_geometric.data.Batch.from_data_list (PyG 1.4.3 [U8]; the replica path
 * of DataParallel, /root/reference/ConvexPruning.py:530) collates a graph list
 * on the host: per graph `item + cumsum[key]` for index keys and
 * `torch.full((n_g,), g)` for the batch vector.  With the raw items
 * concatenated and copied to the device once, these apply the same per-graph
 * terms on the device.  Segments: starts[0..G] (int64, starts[0] = 0,
 * starts[G] = n, non-decreasing; empty graphs allowed), device arrays.
 *   mp_segment_offset_i64: data[r*ld + i] += inc[g(i)], r < rows, i < n
 *   mp_segment_ids_i64:    ids[i] = g(i)
 * g(i) = the graph whose segment holds element i.  Bit-exact (integers). */
int mp_segment_offset_i64(int64_t* data, int64_t ld, int32_t rows, int64_t n, const int64_t* starts,
                          const int64_t* inc, int64_t n_graphs, void* stream);
int mp_segment_ids_i64(int64_t* ids, int64_t n, const int64_t* starts, int64_t n_graphs, void* stream);

/* ---- GATConv attention dropout (training) --------------------------------
 * GATConv.message applies `F.dropout(alpha, p, training)` to the softmax output
 * (PyG 1.4.3 [U6]; the reference's generic path materialises alpha [E, H] and
 * the [E, H*C] messages for it).  Here the mask is a function of the edge's
 * key k and the head h:
 *   keep(k, h) = hash(seed, k*H + h) >= floor(p * 2^32),  kept alpha * 1/(1-p)
 * (hash: two rounds of the murmur3 32-bit finaliser, oracle/pyg_ref.py
 * restates it), so the forward and the transposed backward evaluate the same
 * mask without storing one.  0 < p < 1, H <= 32.  The key (ABI 7): drop_ids[s]
 * for slot s of the CSR the call walks (int32, one per slot: the forward's
 * destination CSR, the backward's transposed CSR), or -- drop_ids NULL -- the
 * edge's destination-CSR slot.  mi355_mp passes edge ids: the layer's on one
 * GPU, the GLOBAL ones on a shard, so a sharded GATConv draws exactly the mask
 * of the single-GPU layer.
 *
 * mp_gat_aggregate_train_drop_f32: mp_gat_aggregate_train_f32 with the dropped
 *   alpha on the messages: out / agg / out2 use alpha * keep / (1-p); the
 *   softmax statistics (row_stats, row_s2) are those of the undropped alpha.
 * mp_gat_backward_train_drop_f32: mp_gat_backward_train_f32 for that forward
 *   (the transposed CSR's eid channel must hold each edge's dst-CSR slot);
 *   needs C/4 a power of two <= 64 and 16-byte aligned rows.
 * mp_gat_dropout_keep: bits[s] = keep bits of slot s (bit h), s < n_slots (key drop_ids[s],
 *   or s when drop_ids is NULL). */
int mp_gat_aggregate_train_drop_f32(const mp_csr* g, const float* xw, const float* a_src,
                                    const float* a_dst, const float* att, int32_t H, int32_t C,
                                    float slope, const float* bias, float* out, int64_t ldo,
                                    float* agg, float* row_stats, float* out2, float* row_s2,
                                    uint64_t seed, float p_drop, const int32_t* drop_ids, void* slab,
                                    size_t slab_bytes, int32_t stages, void* stream);
int mp_gat_backward_train_drop_f32(const mp_csr* gt, const float* grad_out, int64_t ldg,
                                   const float* xw, const float* a_src, const float* pack,
                                   const float* att, int32_t H, int32_t C, float slope,
                                   const float* grad_a_dst, uint64_t seed, float p_drop,
                                   const int32_t* drop_ids, float* grad_xw, float* grad_a_src, void* slab,
                                   size_t slab_bytes, int32_t stages, void* stream);
int mp_gat_dropout_keep(uint64_t seed, float p_drop, int32_t H, int64_t n_slots, const int32_t* drop_ids,
                        uint32_t* bits, void* stream);

/* ---- Row-exact feature transform (ABI 7) ----------------------------------
 * C[i, n] = the k-ordered fmaf chain over k = 0..K-1 from 0 of A[i, k] * B[k, n],
 * B = W ([K, N] row-major) or, trans_w != 0, W^T (W [N, K] row-major): every
 * output row is a function of its input row alone, so a shard's rows of X W are
 * bitwise the single-GPU rows whatever M is (GATConv's x @ W [U6]; a hipBLASLt
 * GEMM picks its kernel -- and its rounding -- by M).  K = N = 256 with 16-byte
 * aligned rows of A (lda % 4 == 0): the f32 MFMA kernel; any other shape (or
 * force_generic): a tiled fmaf kernel with the same arithmetic.  lda >= K,
 * ldc >= N; M = 0 is a no-op. */
int mp_gemm_rows_f32(const float* A, int64_t lda, int64_t M, int32_t K, const float* W, int32_t trans_w,
                     int32_t N, float* C, int64_t ldc, int32_t force_generic, void* stream);

/* Per-block column sums of x [n, F] (0 < F <= 256, F % 4 == 0, 16-byte aligned
 * rows): part [mp_gat_bwd_blocks(n), F] (part_bytes >= that * 4; ABI 6);
 * sum_i x[i, :] is their sum over the blocks (a layer's bias gradient, sum over
 * rows of grad_out). */
int mp_col_sums_f32(const float* x, int64_t ldx, int64_t n, int32_t F, float* part, size_t part_bytes,
                    void* stream);

/* Rows of the per-block partial arrays of the prep/finish kernels for n nodes. */
int mp_gat_bwd_blocks(int64_t n);

/* Backward epilogue (C%4==0, H*C<=256), one pass over the nodes:
 *   grad_xw[n, h*C+c] += ga_dst[n,h] * att[h, c]        (att = [H, 2C]: dst half first)
 *   att_part[b, 0, :]  = sum over block b's nodes of ga_dst[n,h] * xw[n, h*C+c]
 *   att_part[b, 1, :]  = ... ga_src[n,h] * xw[n, h*C+c]
 * att_part is [mp_gat_bwd_blocks(n), 2, H*C]; d att = its sum over blocks.
 * att_part_bytes >= mp_gat_bwd_blocks(n) * 2*H*C * 4 (ABI 6: a partial array
 * sized for fewer rows than n -- e.g. a sharded rank's own rows when the pass
 * runs over own + halo rows -- is MP_ERR_ARG, not a device write past its end).
 * grad_xw = NULL: the att-gradient partials only. */
int mp_gat_backward_finish_f32(float* grad_xw, const float* xw, const float* ga_dst,
                               const float* ga_src, const float* att, int64_t n, int32_t H,
                               int32_t C, float* att_part, size_t att_part_bytes, void* stream);

/* y[n, h*C+c] += s[n,h] * att[h*att_ld + c]  (per-head outer-product update) */
int mp_heads_outer_add_f32(float* y, int64_t ldy, const float* s, int64_t n, int32_t H,
                           int32_t C, const float* att, int64_t att_ld, void* stream);

/* alpha[e,h] for edges in ORIGINAL order (return_attention_weights, backward) */
int mp_gat_alpha_f32(const int64_t* src_idx, const int64_t* dst_idx,
                     int64_t n_edges, int32_t H, const float* a_src,
                     const float* a_dst, float slope, const float* row_stats,
                     float* alpha, void* stream);

/* ---- sharded GATConv over the hybrid halo cover ---------------
 * Merge of online-softmax partials into a destination row's local piece.
 * Row i (i < n_rows) holds the local piece: out[i] = acc/den (normalised, no
 * bias) and row_stats[i, h] = (m, den) from mp_gat_aggregate_att_f32 /
 * mp_gat_aggregate_train_f32 over the rank's own + pulled sources; partial
 * rows k in [pptr[i], pptr[i+1]) of pidx name rows of part_out [n_parts, ldp] /
 * part_stats [n_parts, H, 2] (peers' pieces of the same row, the same kernels
 * on their send graphs).  Per head, local piece first, then the partials in
 * list order:  M = max m, w_k = den_k e^(m_k - M), tot = sum w_k,
 *   out[i] = sum_k (w_k / tot) out_k + bias,   row_stats[i, h] = (M, tot),
 * and (training, optional) agg2[i] / row_s2[i] (the local piece's out2 / row_s2
 * [n_rows, H*C] / [n_rows, H]) scaled by w_loc / tot, the merged rows'.  A row
 * with no partial keeps its local piece + bias bit for bit.  pptr [n_rows + 1]
 * (int32, non-decreasing, pptr[n_rows] <= n_parts) and every pidx entry in
 * [0, n_parts) are the caller's contract (device arrays, not read on the host).
 * C % 4 == 0; out, part_out, bias, agg2 16-byte aligned, leading dimensions
 * multiples of 4.  Extents (ABI 7): part_out_bytes >= ((n_parts - 1) * ldp +
 * H*C) * 4 and part_stats_bytes >= n_parts * H * 8 when n_parts > 0 (the
 * pidx range itself is checked by the host that builds the merge list:
 * mi355_mp.gat_cover.GatHaloCover).  Head of any width: a head may span two of
 * the kernel's 256-feature chunks (the merged stats are written after every
 * chunk of the row has read them). */
int mp_gat_merge_partials_f32(int64_t n_rows, int32_t H, int32_t C, const int32_t* pptr, const int32_t* pidx,
                              int64_t n_parts, const float* part_out, size_t part_out_bytes, int64_t ldp,
                              const float* part_stats, size_t part_stats_bytes, const float* bias, float* out,
                              int64_t ldo, float* row_stats, float* agg2, float* row_s2, void* stream);

/* ---- self-loop rewrites (PyG 1.4.3 utils.loop [U4]) -----
 * Output edge order is upstream's: the kept edges in original order, then the
 * loop edges (n, n) for n = 0..N-1.
 *   MP_LOOPS_REMOVE         remove_self_loops: the non-loop edges
 *   MP_LOOPS_ADD            add_self_loops: every edge, then the N loops
 *   MP_LOOPS_ADD_REMAINING  add_remaining_self_loops: the non-loop edges, then
 *                           the N loops
 * out_pos[k] = position of the input edge whose weight output edge k carries:
 * kept edges their own position; a loop of ADD_REMAINING the position of the
 * node's LAST pre-existing loop (upstream's sequential index_put_ keeps the
 * last one), else -1; a loop of ADD -1.  Weights: mp_gather_fill_f32(w, out_pos,
 * fill).  n_kept = n_edges - mp_self_loop_count(...) for REMOVE and
 * ADD_REMAINING, n_edges for ADD; the outputs hold n_kept (+ N) entries.
 * out_pos is also the compaction buffer (needed unless nothing is removed). */
#define MP_LOOPS_REMOVE 0
#define MP_LOOPS_ADD 1
#define MP_LOOPS_ADD_REMAINING 2
/* count_dev: device int64[2]; [0] = number of self loops, [1] = self loops (r, r)
 * with r outside [0, n_nodes) -- upstream's `loop_weight[row[inv_mask]]` raises
 * an IndexError for those, and the caller must reject them before
 * mp_self_loops (whose loop bookkeeping ignores them).  (ABI 3: n_nodes and the
 * second counter.) */
int mp_self_loop_count(const int64_t* row, const int64_t* col, int64_t n_edges,
                       int64_t n_nodes, int64_t* count_dev, void* stream);
size_t mp_self_loops_workspace(int64_t n_edges, int64_t n_nodes);
int mp_self_loops(const int64_t* row, const int64_t* col, int64_t n_edges, int64_t n_nodes,
                  int32_t mode, int64_t n_kept, int64_t* out_row, int64_t* out_col,
                  int64_t* out_pos, void* ws, size_t ws_bytes, void* stream);
/* out[k] = pos[k] >= 0 ? src[pos[k]] : fill */
int mp_gather_fill_f32(const float* src, const int64_t* pos, int64_t n, float fill,
                       float* out, void* stream);

/* ---- shard plan (destination-range shards, halo maps) ---------- */

/* The plan of rank `rank` owning the key rows [lo, hi) = [cuts[rank],
 * cuts[rank + 1]) of a range partition (replaces the torch-op construction in
 * mi355_mp/dist.py ShardPlan: nonzero / unique / searchsorted):
 *   edge_pos[k]     positions of the edges with lo <= key < hi, in edge order;
 *   local_key[k]    key[edge_pos[k]] - lo;
 *   local_other[k]  other - lo when lo <= other < hi, else n_own + the rank of
 *                   `other` among halo_nodes;
 *   halo_nodes      the sorted unique remote `other` values of those edges;
 *   counts (device, int64 [2 + world]): [0] = selected edges, [1] = halo nodes
 *                   (-1 when a selected edge's `other` lies outside
 *                   [0, n_nodes): the outputs are then invalid), [2 + q] = halo
 *                   nodes owned by rank q.
 * key = destination, other = source for flow source_to_target (the forward
 * plan); swapped for the transposed (backward) plan.  cuts: device int64
 * [world + 1].  Outputs are sized at their upper bounds (n_edges, n_nodes);
 * the caller reads counts and slices.  Workspace: mp_shard_plan_workspace. */
size_t mp_shard_plan_workspace(int64_t n_edges, int64_t n_nodes);
int mp_shard_plan(const int64_t* key, const int64_t* other, int64_t n_edges, int64_t n_nodes,
                  const int64_t* cuts, int32_t world, int32_t rank, int64_t lo, int64_t hi,
                  int64_t* edge_pos, int64_t* local_key, int64_t* local_other,
                  int64_t* halo_nodes, int64_t* counts, void* ws, size_t ws_bytes, void* stream);

/* ---- SplineConv: fused B-spline aggregation (csrc/mp_spline.hip) -----------
 * Per edge e = (j -> i) with pseudo-coordinates u[e, 0..D) in [0, 1] (pseudo
 * [n_pseudo_edges, D] fp32, ORIGINAL edge order), kernel sizes ks[d], open
 * flags op[d], degree M, S = (M+1)^D and K = prod ks:
 *   v_d = u[e,d] * float(ks[d] - M*op[d])  (one fp32 multiply),  f_d = v_d - floor(v_d)
 *   basis[e,s] = prod_d B_M(f_d, k_d),     k_d = the d-th base-(M+1) digit of s
 *   wi[e,s]    = sum_d ((floor(v_d) + k_d) mod ks[d]) * prod_{d' < d} ks[d']
 * B_1 = {1-f, f}; B_2 = {f^2/2 - f + 1/2, -f^2 + f + 1/2, f^2/2};
 * B_3 = {(1-f)^3/6, (3f^3 - 6f^2 + 4)/6, (-3f^3 + 3f^2 + 3f + 1)/6, f^3/6}.
 * Replaces torch_spline_conv's SplineBasis + SplineWeighting and the
 * scatter_add / scatter_mean after them, reordered so that no per-edge basis,
 * index or message array exists: one segmented pass and one dense GEMM.
 * kernel_size / is_open are HOST int32[D] arrays (copied into the kernel
 * arguments).  Limits (mp_spline_ok != 0): 1 <= D <= 3, 1 <= degree <= 3,
 * ks[d] - degree*op[d] >= 1, K <= 256, F >= 1.  A coordinate outside [0, 1]
 * wraps modulo ks[d]: no bin or column is ever out of range.
 * Both aggregate calls walk g->rowptr / col / eid only (col and eid required;
 * the wave schedule is not read), visit a row's slots in slot order from one
 * owner and add left to right: deterministic, no atomics.  Rows of any length
 * are summed serially; hub rows are not split.  n_pseudo_edges must cover the
 * edge-id space of g (g->n_ids, or g->n_edges when that is 0).
 *   mp_spline_basis_f32: basis [n_edges, S] fp32 and weight_index [n_edges, S]
 *     int64 in edge order (basis_bytes / weight_index_bytes: their extents).
 *   mp_spline_aggregate_bins_f32 (x [n_cols, ldx >= F]):
 *     out[r, k*F + f] = scale[r] * sum_{slots of r} sum_{s: wi = k} basis * x[col[slot], f]
 *     ldo >= K*F; all K*F entries of every row are written exactly once
 *     (zeros for rows without slots).
 *   mp_spline_aggregate_gather_f32 (x [n_cols, K, F], ldx >= K*F):
 *     out[r, f] = scale[r] * sum_{slots of r} sum_s basis * x[col[slot], wi*F + f] (+ bias[f])
 * row_scale [n_rows] or NULL (= 1), bias [F] or NULL. */
int mp_spline_ok(int32_t D, int32_t degree, const int32_t* kernel_size, const int32_t* is_open, int32_t F);
int mp_spline_basis_f32(const float* pseudo, int64_t n_edges, int32_t D, const int32_t* kernel_size,
                        const int32_t* is_open, int32_t degree, float* basis, size_t basis_bytes,
                        int64_t* weight_index, size_t weight_index_bytes, void* stream);
int mp_spline_aggregate_bins_f32(const mp_csr* g, const float* pseudo, int64_t n_pseudo_edges, int32_t D,
                                 const int32_t* kernel_size, const int32_t* is_open, int32_t degree,
                                 const float* x, int64_t ldx, int32_t F, const float* row_scale,
                                 float* out, int64_t ldo, void* stream);
int mp_spline_aggregate_gather_f32(const mp_csr* g, const float* pseudo, int64_t n_pseudo_edges, int32_t D,
                                   const int32_t* kernel_size, const int32_t* is_open, int32_t degree,
                                   const float* x, int64_t ldx, int32_t F, const float* row_scale,
                                   const float* bias, float* out, int64_t ldo, void* stream);

/* ---- NNConv: factored edge-conditioned aggregation (csrc/mp_nnconv.hip) -----
 * For an edge network that ends in a Linear (the head: weight [Cin*Cout, H],
 * bias [Cin*Cout]) the per-edge weight matrices W_e = reshape(head(h_e), [Cin,
 * Cout]) of PyG 1.4.3's nn.conv.NNConv [U] are never built.  With h_e in R^H the
 * head's input, ht_e = [h_e, 1] and L[(h, c), o] = head.weight[c*Cout + o, h]
 * (row block h = H: head.bias):
 *   sum_{e -> i} x_j W_e = (sum_{e -> i} ht_e (x) x_j) L
 * one segmented pass and one dense node-level GEMM (the caller's), in place of
 * an [E, Cin*Cout] array and E mat-vecs.
 * h is [n_h_edges, ldh >= H] fp32 in ORIGINAL edge order, read through g->eid;
 * n_h_edges must cover the edge-id space of g (g->n_ids, or g->n_edges when
 * that is 0).  The trailing 1 of ht is implicit: no concatenated copy is taken.
 * Limits (mp_nnconv_ok != 0): H >= 1, Cin >= 1, Cout >= 1 and (H + 1) * Cin,
 * (H + 1) * Cout <= 2^20 floats (one row of Z or Y, 4 MiB).  A row's
 * accumulators are held in registers and tiled over the grid, so neither LDS
 * nor the register file bounds a shape; the limit keeps every in-row offset and
 * grid dimension in range.  The aggregate calls apply it to their own (H, Cin)
 * or (H, F).
 * Both aggregate calls walk g->rowptr / col / eid only (col and eid required;
 * the wave schedule is not read), one owner per output entry visits its row's
 * slots in slot order and adds left to right (gather: h = 0..H inside a slot):
 * fp32, deterministic, no atomics.  Rows of any length are summed serially;
 * hub rows are not split.  Every output entry of every row is written exactly
 * once (zeros for rows without slots); padding beyond it is left untouched.
 *   mp_nnconv_aggregate_bins_f32 (x [n_cols, ldx >= Cin]):
 *     out[r, h*Cin + c] = scale[r] * sum_{slots of r} ht[eid[slot]][h] * x[col[slot], c]
 *     ldo >= (H + 1) * Cin.  Lanes run over the flattened (h, c) for Cin < 32
 *     (several rows share a wave when (H + 1) * Cin < 64), over c with 16
 *     values of h per lane from Cin = 32 on (ht wave-uniform per slot).
 *   mp_nnconv_aggregate_gather_f32 (y [n_cols, H + 1, F], ldy >= (H + 1) * F):
 *     out[r, f] = scale[r] * sum_{slots of r} sum_h ht[eid[slot]][h] * y[col[slot], h*F + f] (+ bias[f])
 *     ldo >= F.  Lanes run over f.
 *   mp_nnconv_edge_grad_f32 (rows / cols [n_edges] int64: each edge's row of dz
 *     and of x, the caller has range-checked them; dz [.., lddz >= (H+1)*Cin]):
 *     dh[e, h] = sum_c dz[rows[e], h*Cin + c] * x[cols[e], c]  for h < H
 *     edge-parallel, nothing is reduced across edges; written in edge order,
 *     lddh >= H, dh_bytes: the extent of dh, at least ((n_edges - 1) * lddh + H)
 *     floats, checked before any launch.
 * row_scale [n_rows] or NULL (= 1), bias [F] or NULL.
 * Like the graclus and point-set entry points these are additions to ABI 7 that
 * return int64_t, not a status: the launches enqueued, >= 0, or -(MP_ERR_* code)
 * with the reason in mp_last_error() when the call is refused -- for a bad
 * argument (-MP_ERR_ARG), before any launch.  The caller tests the sign.
 * mp_nnconv_edge_grad_width(H, Cin): which kernel mp_nnconv_edge_grad_f32 takes
 * for a shape -- 0 = a lane group per (e, h) pair (Cin <= 32), else the lanes W =
 * 32 or 64 per (edge, W values of h), the width that wastes the fewest lanes
 * and values of h (ties to 64) -- or -MP_ERR_ARG for a shape outside the limits.
 * The call dispatches on this function; it needs no GPU. */
int64_t mp_nnconv_ok(int32_t H, int32_t Cin, int32_t Cout);
int64_t mp_nnconv_edge_grad_width(int32_t H, int32_t Cin);
int64_t mp_nnconv_aggregate_bins_f32(const mp_csr* g, const float* h, int64_t n_h_edges, int64_t ldh, int32_t H,
                                     const float* x, int64_t ldx, int32_t Cin, const float* row_scale, float* out,
                                     int64_t ldo, void* stream);
int64_t mp_nnconv_aggregate_gather_f32(const mp_csr* g, const float* h, int64_t n_h_edges, int64_t ldh, int32_t H,
                                       const float* y, int64_t ldy, int32_t F, const float* row_scale,
                                       const float* bias, float* out, int64_t ldo, void* stream);
int64_t mp_nnconv_edge_grad_f32(const int64_t* rows, const int64_t* cols, int64_t n_edges, const float* dz,
                                int64_t lddz, const float* x, int64_t ldx, int32_t H, int32_t Cin, float* dh,
                                int64_t lddh, size_t dh_bytes, void* stream);

/* ---- GMMConv: Gaussian mixture weights fused into the aggregation (csrc/mp_gmm.hip)
 * PyG 1.4.3's nn.conv.GMMConv [U] with shared Gaussians: per edge e = (j -> i)
 * with pseudo-coordinates p_e in R^D,
 *   w_k(p) = exp(sum_d -0.5 (p_d - mu_kd)^2 * iv_kd),   iv_kd = 1 / (1e-15f + sigma_kd^2)
 *   m_e    = sum_k w_k(p_e) * Y[j, k, :],               Y = (x g).view(N, K, M)
 * The weights are evaluated inside the segmented pass from the D floats of
 * pseudo[e]: neither the [E, K, M] gathered operand nor an [E, K] coefficient
 * array exists.  With G'[(k, c), m] = g[c, k*M + m]:
 *   sum_{e -> i} m_e = (sum_{e -> i} w(p_e) (x) x_j) G'
 * pseudo is [n_p_edges, ldp >= D] fp32 in ORIGINAL edge order, read through
 * g->eid; n_p_edges must cover the edge-id space of g (g->n_ids, or g->n_edges
 * when that is 0).  mu and sigma are [K, D] fp32, contiguous.
 * Limits (mp_gmm_ok != 0; needs no GPU): K, D, Cin, Cout >= 1, K * D <= 1024
 * (the mu / iv table a workgroup stages in LDS: 8 KiB) and K * Cin, K * Cout <=
 * 2^20 floats (one row of Z or Y).  The aggregate calls apply the limits to
 * their own (K, D, Cin) or (K, D, F).
 * Both aggregate calls walk g->rowptr / col / eid only (col and eid required),
 * one owner per output entry visits its row's slots in slot order and adds
 * left to right (gather: k = 0..K-1 inside a slot): fp32, deterministic, no
 * atomics.  Hub rows are not split.  Every output entry of every row is
 * written exactly once (zeros for rows without slots); padding beyond it is
 * left untouched.
 *   mp_gmm_aggregate_bins_f32 (x [n_cols, ldx >= Cin]):
 *     out[r, k*Cin + c] = scale[r] * sum_{slots of r} w_k(pseudo[eid[slot]]) * x[col[slot], c]
 *     ldo >= K * Cin.  Lanes run over the flattened (k, c) for Cin < 32, over c
 *     with 16 values of k per lane from Cin = 32 on; there a wave evaluates the
 *     weights of four slots cooperatively, one exp per (slot, k).
 *   mp_gmm_aggregate_gather_f32 (y [n_cols, K, F], ldy >= K * F):
 *     out[r, f] = scale[r] * sum_{slots of r} sum_k w_k(pseudo[eid[slot]]) * y[col[slot], k*F + f] (+ bias[f])
 *     ldo >= F.  Lanes run over f; a row's lane group evaluates its (slot, k)
 *     weights cooperatively.
 *   mp_gmm_param_grad_f32 (rows / cols [n_edges] int64: each edge's row of dz and
 *     of x, range-checked by the caller; pseudo [n_edges, ldp] indexed by the edge
 *     itself; dz [.., lddz >= K * Cin]): with dw[e, k] = sum_c dz[rows[e], k*Cin + c]
 *     * x[cols[e], c] and t = dw * w_k(pseudo[e]) (w recomputed),
 *       dmu[k, d]     = sum_e t * (p_d - mu_kd) * iv_kd
 *       dsigma[k, d]  = sum_e t * ((p_d - mu_kd)^2 * iv_kd) * (sigma_kd * iv_kd)
 *       dpseudo[e, d] = -sum_k t * (p_d - mu_kd) * iv_kd   (dpseudo may be NULL: not written; lddp >= D)
 *     dmu, dsigma [K, D] contiguous, every entry written (zeros without edges).
 *     The association of dsigma keeps every factor finite wherever w != 0, and
 *     an (edge, k) whose weight underflows to 0 contributes EXACTLY zero to all
 *     three -- upstream's autograd yields NaN there (0 * inf) when sigma is
 *     tiny.  Stage 1: one workgroup per chunk of mp_gmm_grad_chunk(n_edges, K, D)
 *     edges sums its 2 K D partials in a fixed order into ws; stage 2 adds the
 *     partials in chunk order.  The chunk is a pure function of (n_edges, K, D):
 *     at least 1024 edges, at most 4096 chunks and 8 MiB of partials, so the
 *     result does not depend on grid size or occupancy.  ws:
 *     mp_gmm_param_grad_workspace(n_edges, K, D) bytes, checked before any launch.
 * row_scale [n_rows] or NULL (= 1), bias [F] or NULL.
 * Additions to ABI 7 that return int64_t like the NNConv calls: the launches
 * enqueued, >= 0, or -(MP_ERR_* code) with the reason in mp_last_error(); a bad
 * argument is refused before any launch. */
int64_t mp_gmm_ok(int32_t K, int32_t D, int32_t Cin, int32_t Cout);
int64_t mp_gmm_aggregate_bins_f32(const mp_csr* g, const float* pseudo, int64_t n_p_edges, int64_t ldp, int32_t D,
                                  const float* mu, const float* sigma, int32_t K, const float* x, int64_t ldx,
                                  int32_t Cin, const float* row_scale, float* out, int64_t ldo, void* stream);
int64_t mp_gmm_aggregate_gather_f32(const mp_csr* g, const float* pseudo, int64_t n_p_edges, int64_t ldp, int32_t D,
                                    const float* mu, const float* sigma, int32_t K, const float* y, int64_t ldy,
                                    int32_t F, const float* row_scale, const float* bias, float* out, int64_t ldo,
                                    void* stream);
int64_t mp_gmm_grad_chunk(int64_t n_edges, int32_t K, int32_t D);
size_t mp_gmm_param_grad_workspace(int64_t n_edges, int32_t K, int32_t D);
int64_t mp_gmm_param_grad_f32(const int64_t* rows, const int64_t* cols, int64_t n_edges, const float* pseudo,
                              int64_t ldp, int32_t D, const float* mu, const float* sigma, int32_t K, const float* dz,
                              int64_t lddz, const float* x, int64_t ldx, int32_t Cin, float* dmu, float* dsigma,
                              float* dpseudo, int64_t lddp, void* ws, size_t ws_bytes, void* stream);

/* ---- Attention readout: Set2Set / GlobalAttention (csrc/mp_glob.hip) ---------
 * PyG 1.4.3's nn.glob.Set2Set and nn.glob.GlobalAttention [U] share one step: a
 * softmax of one scalar per node over each graph, then the softmax-weighted sum
 * of the graph's node rows.  Here it is one pass over x per graph, forward and
 * backward; nothing of size N is written but e.  All arithmetic is fp32.
 * Graphs are segment starts: starts [n_graphs + 1] int64 on the device, non-
 * decreasing, within [0, n] (ops.cached_batch_layout of a sorted batch vector);
 * g(i) is the graph of node i.  max_n: at least the node count of the largest
 * graph (it sizes grids and the workspace, never a result).
 * Forward, x [n, ldx >= C] and exactly one of
 *   q [n_graphs, ldq >= C]   query mode:  e_i = sum_c x[i, c] * q[g(i), c]
 *   score [n]                score mode:  e_i = score[i]
 * gives per graph g
 *   m_g = max_i e_i,  den_g = sum_i exp(e_i - m_g),  a_i = exp(e_i - m_g) / den_g
 *   out[g, c] = sum_i a_i * x[i, c]            out [n_graphs, ldo >= C]
 * and writes e [n] and stats [n_graphs, 2] = (m, den) for the backward; alpha
 * [n] = a is written when it is not NULL (one more launch).  q_out, when not
 * NULL (query mode only), receives q[g, :] at q_out[g * ldo + c]: with out =
 * base + C and q_out = base, ldo = 2C, Set2Set's q_star = [q | r] is written
 * without a concatenation.
 * Upstream divides by den + 1e-16.  A graph with a node has den >= 1, and in
 * fp32 1 + 1e-16 == 1 (so den + 1e-16 == den bit for bit): the kernels divide
 * by den.  A graph without nodes (anywhere, trailing graphs included) gets
 * out[g, :] = 0 and stats = (0, 0), upstream's result (scatter_max and
 * scatter_add fill 0).  Every entry of out (and q_out), stats, e (and alpha) is
 * written exactly once; padding beyond C is left untouched; nothing needs a
 * memset.  Only finite inputs are specified.
 * Backward, given dr [n_graphs, lddr >= C], the forward's e, stats and r = out
 * (ldr its row stride):
 *   s_g = sum_c dr[g, c] * r[g, c]
 *   de_i = a_i * (sum_c dr[g(i), c] * x[i, c] - s_g)
 *   query mode:  dx[i, :] = a_i * dr[g(i), :] + de_i * q[g(i), :],  dq[g, :] = sum_i de_i * x[i, :]
 *   score mode:  dx[i, :] = a_i * dr[g(i), :],                      dscore[i] = de_i
 * one pass over x; a is recomputed from e and stats.  q NULL selects score
 * mode.  dx, dq and dscore may each be NULL (not computed); dq needs q, dscore
 * needs q == NULL.  Rows of dq of graphs without nodes are zero.
 * Paths, chosen per graph from (n_g, C) alone -- mp_readout_path (needs no GPU):
 *   0  one wave per graph, four graphs per workgroup
 *   1  one workgroup per graph, wave partials merged through LDS in wave order
 *   2  the graph cut into chunks of mp_readout_chunk(C) nodes, a workgroup each;
 *      chunk partials (m, den, r[C]) go to the workspace and a second kernel
 *      merges them in chunk order, rescaled by exp(m_chunk - m_g) (dq: summed)
 * No atomics, every merge order fixed: a graph's out, stats, dx and dq are the
 * same bits run to run and whether the graph is batched alone or among others
 * (given the same C, strides and 16-byte alignment of the row pointers, which
 * select 16-byte or scalar loads and with them the order of the dot's terms).
 * C >= 1 is any width; lanes run over channels, rows wider than a pass are tiled
 * over the grid.  Limits, checked before any launch (a refused call writes
 * nothing): n_graphs < 2^31, max_n <= 65535 * mp_readout_chunk(C), and no launch
 * of 2^24 workgroups or more: n_graphs * ceil(max_n / mp_readout_chunk(C)) *
 * channel tiles < 2^24 when the largest graph is split (one very large graph
 * beside very many others; the grid is sized from max_n alone).
 * ws: mp_readout_workspace(n, n_graphs, max_n, C) bytes, required (not NULL)
 * by both calls, one layout (csrc/mp_glob.hip ReadoutWs); every caller-sized
 * array travels with its extent in bytes, checked before any launch.
 * Additions to ABI 7 that return int64_t like the NNConv calls: the launches
 * enqueued, >= 0, or -(MP_ERR_* code) with the reason in mp_last_error();
 * mp_readout_path / mp_readout_chunk: the answer, or -MP_ERR_ARG for C < 1 (or
 * n_g < 0). */
int64_t mp_readout_path(int64_t n_g, int32_t C);
int64_t mp_readout_chunk(int32_t C);
size_t mp_readout_workspace(int64_t n, int64_t n_graphs, int64_t max_n, int32_t C);
int64_t mp_attention_readout_f32(const float* x, int64_t ldx, int64_t n, int32_t C, const int64_t* starts,
                                 int64_t n_graphs, int64_t max_n, const float* q, int64_t ldq, const float* score,
                                 float* out, int64_t ldo, size_t out_bytes, float* q_out, size_t q_out_bytes,
                                 float* e, size_t e_bytes, float* stats, size_t stats_bytes, float* alpha,
                                 size_t alpha_bytes, void* ws, size_t ws_bytes, void* stream);
int64_t mp_attention_readout_bwd_f32(const float* dr, int64_t lddr, const float* x, int64_t ldx, int64_t n, int32_t C,
                                     const int64_t* starts, int64_t n_graphs, int64_t max_n, const float* q,
                                     int64_t ldq, const float* e, const float* stats, const float* r, int64_t ldr,
                                     float* dx, int64_t lddx, size_t dx_bytes, float* dq, int64_t lddq,
                                     size_t dq_bytes, float* dscore, size_t dscore_bytes, void* ws, size_t ws_bytes,
                                     void* stream);

/* ---- RGCNConv: relational aggregation over a basis decomposition (csrc/mp_rgcn.hip)
 * PyG 1.4.3's nn.conv.RGCNConv [U] builds W_r = sum_b att[r, b] basis[b], gathers
 * one [Cin, Cout] matrix per edge and runs E mat-vecs (x = None: an [R*N, Cout]
 * table every forward).  With edge_type t_e in [0, R), the edge norm n_e, the
 * per-edge coefficients a_e = n_e att[t_e, :] in R^B and V = basis viewed as
 * [B*Cin, Cout]:
 *   sum_{e -> i} n_e x_j W_{t_e} = (sum_{e -> i} a_e (x) x_j) V
 * one segmented pass and one dense node-level GEMM (the caller's).  a_e is never
 * stored: the kernels read edge_type (int64) and edge_norm (fp32, or NULL = 1),
 * both [n_type_edges] in ORIGINAL edge order, through g->eid, and att [R, ld_att
 * >= B] (att_bytes: its extent, at least ((R - 1) * ld_att + B) floats).
 * n_type_edges must cover the edge-id space of g (g->n_ids, or g->n_edges when
 * that is 0).  Types outside [0, R) are the caller's to reject (mi355_mp.ops does,
 * once per edge_type tensor, with an IndexError); the kernels never read att with
 * one: such a slot contributes nothing.
 * Limits (mp_rgcn_ok != 0): 1 <= R <= 65536, B >= 1, Cin >= 1, Cout >= 1 and
 * B * Cin, B * Cout <= 2^20 floats (one row of Z or Y); the calls apply them to
 * their own (R, B, C) or (R, B, F).  Accumulators live in registers, tiled over
 * the grid: neither LDS nor the register file bounds a shape.  att is read
 * through the cache at every size.
 * The aggregate calls walk g->rowptr / col / eid only (col and eid required); one
 * owner per output entry visits its row's slots in slot order and adds left to
 * right (gather: b = 0..B-1 inside a slot): fp32, deterministic, no atomics.  Rows
 * of any length are summed serially; hub rows are not split.  Every output entry
 * of every row is written exactly once (zeros for rows without slots); padding
 * is left untouched.  One operand of each is addressed by TWO strides:
 *   mp_rgcn_aggregate_bins_f32 (x [n_cols, ldx >= C]):
 *     out[r*ld_node + b*ld_block + c] = sum_{slots of r} (n[eid] * att[type[eid], b]) * x[col, c]
 *     Z [N, B*C]: ld_node = its row stride, ld_block = C.  d basis [B, N, Cout] of
 *     the featureless backward, in place: ld_node = Cout, ld_block = N*Cout.  The
 *     entries must not overlap (ld_block >= C and ld_node >= (B-1)*ld_block + C,
 *     or ld_node >= C and ld_block >= (n_rows-1)*ld_node + C); out_bytes: the
 *     extent of out, at least ((n_rows-1)*ld_node + (B-1)*ld_block + C) floats.
 *     Lanes run over the flattened (b, c) for C < 32, over c with 16 values of b
 *     per lane from C = 32 on.
 *   mp_rgcn_aggregate_gather_f32:
 *     out[r, f] = sum_{slots of r} sum_b (n[eid] * att[type[eid], b]) * y[col*ld_node + b*ld_block + f] (+ bias[f])
 *     Y = x @ L' or dZ, [N, B, F]: ld_node = its row stride, ld_block = F.  basis
 *     [B, N, Cout] read in place: ld_node = Cout, ld_block = N*Cout.  ld_node,
 *     ld_block, ldo >= F; y_bytes: the extent of y, at least ((g->n_cols-1)*ld_node
 *     + (B-1)*ld_block + F) floats.  Lanes run over f.
 *   mp_rgcn_att_grad_f32 (a relation plan: perm [n_edges] int64, the edge ids
 *     stably sorted by type, relptr [R + 1] int64, relation r owning the positions
 *     [relptr[r], relptr[r+1]) of perm; rows / cols [n_edges] int64, each edge's
 *     node of P and of Q, range-checked by the caller; edge_norm [n_edges] or NULL):
 *     datt[r, b] = sum_{i in relation r, e = perm[i]} n_e * sum_c P[rows[e]*ldp_node + b*ldp_block + c] * Q[cols[e]*ldq + c]
 *     Stage 1: one workgroup per chunk of mp_rgcn_att_chunk() positions of one
 *     relation sums its B partials in a fixed order into the workspace; stage 2:
 *     one owner per (r, b) adds the relation's chunk partials in chunk order.  A
 *     relation without edges gets zeros; every datt[r, b] is written (ld_datt >= B,
 *     datt_bytes at least ((R-1)*ld_datt + B) floats).  relptr is clamped into
 *     [0, n_edges] and to non-decreasing as it is read and positions of perm
 *     outside [0, n_edges) are skipped: a bad plan gives wrong sums, not a write
 *     outside datt or the workspace.  ws: mp_rgcn_att_grad_workspace(n_edges, R, B)
 *     bytes, required, one layout (csrc/mp_rgcn.hip RgcnAttWs).
 * Additions to ABI 7 that return int64_t like the NNConv calls: the launches
 * enqueued, >= 0, or -(MP_ERR_* code) with the reason in mp_last_error() -- for a
 * bad argument (-MP_ERR_ARG), before any launch.  mp_rgcn_ok and mp_rgcn_att_chunk
 * answer a question (0 / 1, the chunk size) and need no GPU. */
int64_t mp_rgcn_ok(int32_t R, int32_t B, int32_t Cin, int32_t Cout);
int64_t mp_rgcn_att_chunk(void);
int64_t mp_rgcn_aggregate_bins_f32(const mp_csr* g, const int64_t* edge_type, const float* edge_norm,
                                   int64_t n_type_edges, const float* att, int64_t ld_att, size_t att_bytes, int32_t R,
                                   int32_t B, const float* x, int64_t ldx, int32_t C, float* out, int64_t ld_node,
                                   int64_t ld_block, size_t out_bytes, void* stream);
int64_t mp_rgcn_aggregate_gather_f32(const mp_csr* g, const int64_t* edge_type, const float* edge_norm,
                                     int64_t n_type_edges, const float* att, int64_t ld_att, size_t att_bytes,
                                     int32_t R, int32_t B, const float* y, int64_t ld_node, int64_t ld_block,
                                     size_t y_bytes, int32_t F, const float* bias, float* out, int64_t ldo,
                                     void* stream);
size_t mp_rgcn_att_grad_workspace(int64_t n_edges, int32_t R, int32_t B);
int64_t mp_rgcn_att_grad_f32(const int64_t* perm, const int64_t* relptr, const int64_t* rows, const int64_t* cols,
                             int64_t n_edges, const float* edge_norm, const float* P, int64_t ldp_node,
                             int64_t ldp_block, const float* Q, int64_t ldq, int32_t R, int32_t B, int32_t C,
                             float* datt, int64_t ld_datt, size_t datt_bytes, void* ws, size_t ws_bytes, void* stream);

/* ---- DNAConv: per-edge attention over layer histories (csrc/mp_dna.hip)
 * PyG 1.4.3's nn.conv.DNAConv [U] gathers x_j as [E, T, C] and projects keys and
 * values per edge.  The projections depend on the node only, so the caller runs
 * them once per node: Q = lin_q(x[:, T-1]) [n, C], K = lin_k(x), V = lin_v(x)
 * [n, T, C].  Per edge e = (j -> i) and head h (d = C / H channels) what is left is
 *   s_t = <Q_i[h], K_j[t][h]> / sqrt(d)
 *   a_t = exp(s_t - m) / (sum_u exp(s_u - m) + exp(-m)),  m = max(0, max_t s_t)
 *   out_i[h] = sum_{e -> i} norm_e sum_t keep_t scale a_t V_j[t][h]
 * the restricted softmax (margin 0) = the softmax over {0, s_1 .. s_T} without its
 * first entry; lse = m + log(sum_u exp(s_u - m) + exp(-m)) gives a_t = exp(s_t - lse).
 * Rows: q, out, gout, dq [., ld >= C]; k, v, dk, dv [., ld >= T * C] with entry (t, c)
 * of a row at t * C + c (any ld >= T * C: K and V may be two arrays, or the halves
 * of one fused projection [n, 2, T, C] passed as two pointers with ld = 2 * T * C,
 * each with the bytes from its own pointer on).  Every array travels with its extent in bytes, checked before
 * any launch.  norm [n_norm] fp32 in ORIGINAL edge order (read through g->eid), or
 * NULL = 1; n_norm must cover g's edge-id space (g->n_ids, or g->n_edges).  lse
 * [ids, H] in edge-id order.
 * Limits (mp_dna_ok != 0): T, H, C >= 1, C % H == 0, C / H <= 256, T * ceil((C / H)
 * / 64) <= 48 (the source backward keeps 4 * T * ceil(d / 64) floats per lane in
 * LDS: at most 48 KiB per wave) and T * C <= 2^20.  mp_dna_max_layers(H, C): the
 * largest T inside them, 0 when no T is.
 * One lane group (min(64, pow2 >= d) lanes) owns a unit, visits its slots in slot
 * order and adds left to right: fp32, deterministic, no atomics; all three kernels
 * share the mapping, so a recomputed score has the forward's bits.  On a CSR whose
 * schedule has g->chunk >= mp_dna_split_chunk() (64) a unit is (task, head): it
 * walks the task's slots as the engine's main kernel does, a row cut by a task
 * boundary leaves its partial sums in a slab (slot 2 * task: a continuation, 2 *
 * task + 1: a head) and a fix-up launch adds each split row's partials in task
 * order (g->wave_row, wave_slot, split_waves: the engine's sum fix-up protocol), so
 * a hub row is walked by many tasks at once.  On a smaller schedule, or with
 * g->wave_row NULL, a unit is (row, head) and walks the whole row, however long;
 * no slab is used (mi355_mp's DNAConv builds its graphs with chunk >= 64).  ws: mp_dna_workspace(g, slot_floats) bytes, slot_floats = C for the
 * forward and the destination backward, 2 * T * C for the source backward (d K |
 * d V); one layout (csrc/mp_dna.hip DnaWs), required (and its extent checked)
 * exactly when the kernels walk tasks.  Every entry of every output row is written
 * exactly once (zeros for rows without slots), padding is left untouched.
 *   mp_dna_aggregate_f32 (g: destination CSR; q, out by row, k, v by column):
 *     out as above; lse NULL or written for every slot's edge id.
 *   mp_dna_backward_dst_f32 (same CSR): with do = norm_e gout_i[h], dalpha_t = keep_t
 *     scale <do, V_j[t][h]>, ds_t = a_t (dalpha_t - sum_u a_u dalpha_u):
 *     dq_i[h] = sum_{e -> i} sum_t ds_t K_j[t][h] / sqrt(d); two sweeps over t.
 *   mp_dna_backward_src_f32 (g: the source-keyed CSR; k, v, dk, dv by row, q, gout by
 *     column): dv_j[t][h] = sum_e keep_t scale a_t do, dk_j[t][h] = sum_e ds_t Q_i[h] /
 *     sqrt(d).
 * Attention dropout: p_drop = 0 is none, else 0 < p_drop < 1 and keep_t =
 * hash(seed, (eid * H + h) * T + t) >= floor(p * 2^32), scale = 1 / (1 - p): the
 * draw of mp_gat_dropout_keep under another key.  mp_dna_dropout_keep writes keep
 * [n_edges * H * T] bytes (0 / 1) in edge-id order.
 * Additions to ABI 7 that return int64_t like the RGCN calls: the launches
 * enqueued, >= 0, or -(MP_ERR_* code) with the reason in mp_last_error() -- for a
 * bad argument (-MP_ERR_ARG), before any launch.  mp_dna_ok, mp_dna_max_layers,
 * mp_dna_split_chunk and mp_dna_workspace answer a question and need no GPU. */
int64_t mp_dna_ok(int32_t T, int32_t H, int32_t C);
int64_t mp_dna_max_layers(int32_t H, int32_t C);
int64_t mp_dna_split_chunk(void);
size_t mp_dna_workspace(const mp_csr* g, int64_t slot_floats);
int64_t mp_dna_aggregate_f32(const mp_csr* g, const float* q, int64_t ldq, size_t q_bytes, const float* k, int64_t ldk,
                             size_t k_bytes, const float* v, int64_t ldv, size_t v_bytes, const float* norm,
                             int64_t n_norm, int32_t T, int32_t H, int32_t C, uint64_t seed, float p_drop, float* out,
                             int64_t ldo, size_t out_bytes, float* lse, size_t lse_bytes, void* ws, size_t ws_bytes,
                             void* stream);
int64_t mp_dna_backward_dst_f32(const mp_csr* g, const float* q, int64_t ldq, size_t q_bytes, const float* k,
                                int64_t ldk, size_t k_bytes, const float* v, int64_t ldv, size_t v_bytes,
                                const float* norm, int64_t n_norm, const float* gout, int64_t ldg, size_t g_bytes,
                                const float* lse, size_t lse_bytes, int32_t T, int32_t H, int32_t C, uint64_t seed,
                                float p_drop, float* dq, int64_t lddq, size_t dq_bytes, void* ws, size_t ws_bytes,
                                void* stream);
int64_t mp_dna_backward_src_f32(const mp_csr* g, const float* q, int64_t ldq, size_t q_bytes, const float* k,
                                int64_t ldk, size_t k_bytes, const float* v, int64_t ldv, size_t v_bytes,
                                const float* norm, int64_t n_norm, const float* gout, int64_t ldg, size_t g_bytes,
                                const float* lse, size_t lse_bytes, int32_t T, int32_t H, int32_t C, uint64_t seed,
                                float p_drop, float* dk, int64_t lddk, size_t dk_bytes, float* dv, int64_t lddv,
                                size_t dv_bytes, void* ws, size_t ws_bytes, void* stream);
int64_t mp_dna_dropout_keep(uint64_t seed, float p_drop, int32_t H, int32_t T, int64_t n_edges, uint8_t* keep,
                            size_t keep_bytes, void* stream);

/* ---- TopKPooling: score, per-graph select, gate, filter_adj (csrc/mp_pool.hip)
 * PyG 1.4.3 nn.pool.topk_pool [U] as one deterministic native path: no atomics
 * on values (two integer counters and one integer maximum aside), no dense
 * [G, max_nodes] copy, no host loop over the batch.  The caller allocates every
 * output and workspace; every caller-sized array travels with its extent in
 * bytes, checked before any launch.  n < 2^31 nodes and edges.
 *
 * Batch vector (non-decreasing int64 [n]):
 *   mp_batch_stats: stats (device int64[3]) = { batch[n-1] + 1 (the number of
 *     graphs), the longest run of equal ids (the largest graph), the number of
 *     descents batch[i] < batch[i-1] plus 1 when batch[0] < 0 (0 = usable) }.
 *   mp_batch_starts: starts[g] = first i with batch[i] >= g for g < n_graphs,
 *     starts[n_graphs] = n (the convention of mp_segment_ids_i64; an id no node
 *     carries is an empty graph).
 *
 * Score (attn [n, F] fp32, ld >= F; w [F]):
 *   z = <attn[i, :], w>;  u = z / ||w||_2 (MP_POOL_SCORE_RAW: u = z);
 *   score[i] = tanh(u) with MP_POOL_SCORE_TANH, else u.
 *   ||w|| is summed on the device in a fixed order (no host read).  Rows of up
 *   to 32 features share a wave (64 / pow2(F) rows each).
 *   mp_pool_score_bwd_f32, du = g_score * f'(u) (1 - score^2 for tanh):
 *     g_attn[i, :] = (du_i / ||w||) * w                     (NULL: skipped)
 *     g_w = (sum_i du_i attn_i) / ||w|| - (sum_i du_i z_i) * w / ||w||^3
 *   (RAW: g_attn = du * w, g_w = sum_i du_i attn_i), both sums through
 *   mp_pool_score_bwd_parts(n) per-chunk partials added in chunk order.
 *   ws: mp_pool_score_bwd_workspace(n, F) bytes.
 *
 * Select (score [n], starts [n_graphs + 1], ratio in (0, 1]):
 *   graph g of n_g = starts[g+1] - starts[g] nodes keeps
 *     k_g = min(n_g, ceil(fl32(ratio * fl32(n_g))))   (one fp32 multiply; upstream's
 *     (ratio * num_nodes.to(torch.float)).ceil(), e.g. (0.3, 50) -> 16),
 *   its nodes ranked by descending score, equal scores by ascending index
 *   (-0 == +0; NaN above +inf, NaNs among themselves by index):
 *     perm[out_starts[g] + r] = the node of rank r < k_g   (global ids),
 *     out_starts = the exclusive scan of k_g, out_starts[n_graphs] = K,
 *     inv[i] = the output position of node i, or -1 when it is dropped
 *              (every entry written: no memset),
 *     counts[0] = K (device int64; -1 when a graph is larger than max_n).
 *   mp_topk_path(n_g): 0 = one wave ranks the graph by counting (n_g <= 64),
 *   1 = one workgroup, keys in LDS (n_g <= MP_TUNE_TOPK_WG_LIMIT), 2 = sorted
 *   (rocPRIM radix sort of (key, ~local index): device-wide when n_graphs == 1,
 *   else one segment per over-limit graph).  max_n: an upper bound of the
 *   largest n_g (n always is one); it sizes the LDS and decides whether the
 *   sorted path is launched.  perm holds n entries (its upper bound).
 *   mp_topk_counts: out_starts / counts[0] alone (no score is read).
 *
 * Gate (perm [k], k known to the host):
 *   x_out[r, :] = x[perm[r], :] * score[perm[r]], then multiplier * that (a
 *   second rounding) only when multiplier != 1; score_out[r] = score[perm[r]];
 *   batch_out[r] = batch[perm[r]] (batch NULL: 0; batch_out NULL: skipped).
 *   mp_pool_gate_bwd_f32: one pass over all n nodes, every row written once:
 *     g_x[i, :] = (m * s_i) * g_y[inv[i], :],  g_s[i] = m * <g_y[inv[i]], x_i> + g_t[inv[i]]
 *   and exact zeros for a dropped node (inv[i] < 0).  g_t NULL = zeros.
 *
 * filter_adj:
 *   mp_pool_inverse: inv[perm[r]] = r for r < k, -1 elsewhere (for a perm that
 *     did not come from mp_topk_select_f32).  k_dev (device int64, or NULL): the
 *     count when only the device knows it yet; k is then its upper bound.
 *   mp_pool_compact: out_pos = the positions i < n with keep[i] != 0, ascending;
 *     count_dev[0] = their number.  (The min_score path's nonzero().)
 *   mp_pool_filter_adj: edge e is kept iff inv[row[e]] >= 0 and inv[col[e]] >= 0;
 *     kept edges in original order: out_row / out_col = inv[...] (int64),
 *     out_pos[k] = the original position of output edge k (edge_attr and its
 *     gradient); counts[1] = kept edges, counts[2] = edge ends outside
 *     [0, n_nodes) (such edges are dropped; upstream raises IndexError, and so
 *     must the caller).  The three outputs hold n_edges entries each
 *     (out_bytes: the extent of each). */
#define MP_POOL_SCORE_TANH 1
#define MP_POOL_SCORE_RAW 2
int mp_topk_path(int64_t n_g);
int mp_batch_stats(const int64_t* batch, int64_t n, int64_t* stats, size_t stats_bytes, void* stream);
int mp_batch_starts(const int64_t* batch, int64_t n, int64_t n_graphs, int64_t* starts, size_t starts_bytes,
                    void* stream);
int mp_pool_score_f32(const float* attn, int64_t ld, int64_t n, int32_t F, const float* w, int32_t flags,
                      float* score, size_t score_bytes, void* stream);
int32_t mp_pool_score_bwd_parts(int64_t n);
size_t mp_pool_score_bwd_workspace(int64_t n, int32_t F);
int mp_pool_score_bwd_f32(const float* attn, int64_t ld, int64_t n, int32_t F, const float* w, int32_t flags,
                          const float* score, const float* g_score, float* g_attn, int64_t ldg, float* g_w,
                          size_t g_w_bytes, void* ws, size_t ws_bytes, void* stream);
int mp_topk_counts(const int64_t* starts, int64_t n_graphs, float ratio, int64_t max_n, int64_t* out_starts,
                   size_t out_starts_bytes, int64_t* counts, void* stream);
size_t mp_topk_workspace(int64_t n, int64_t n_graphs, int64_t max_n);
int mp_topk_select_f32(const float* score, int64_t n, const int64_t* starts, int64_t n_graphs, int64_t max_n,
                       float ratio, int64_t* perm, size_t perm_bytes, int64_t* out_starts, size_t out_starts_bytes,
                       int64_t* inv, size_t inv_bytes, int64_t* counts, void* ws, size_t ws_bytes, void* stream);
int mp_pool_gate_f32(const float* x, int64_t ldx, const float* score, const int64_t* batch, const int64_t* perm,
                     int64_t k, int64_t n, int32_t F, float multiplier, float* x_out, int64_t ldo,
                     size_t x_out_bytes, int64_t* batch_out, float* score_out, void* stream);
int mp_pool_gate_bwd_f32(const float* g_y, int64_t ldgy, const float* g_t, const float* x, int64_t ldx,
                         const float* score, const int64_t* inv, int64_t k, int64_t n, int32_t F, float multiplier,
                         float* g_x, int64_t ldgx, size_t g_x_bytes, float* g_s, size_t g_s_bytes, void* stream);
int mp_pool_inverse(const int64_t* perm, int64_t k, const int64_t* k_dev, int64_t n, int64_t* inv, size_t inv_bytes,
                    void* stream);
size_t mp_pool_compact_workspace(int64_t n);
int mp_pool_compact(const uint8_t* keep, int64_t n, int64_t* out_pos, size_t out_pos_bytes, int64_t* count_dev,
                    void* ws, size_t ws_bytes, void* stream);
size_t mp_pool_filter_workspace(int64_t n_edges);
int mp_pool_filter_adj(const int64_t* row, const int64_t* col, int64_t n_edges, const int64_t* inv, int64_t n_nodes,
                       int64_t* out_row, int64_t* out_col, int64_t* out_pos, size_t out_bytes, int64_t* counts,
                       void* ws, size_t ws_bytes, void* stream);

/* ---- Cluster pooling (csrc/mp_cluster.hip) ----------------------------------
 * PyG 1.4.3 nn.pool voxel_grid / consecutive_cluster / max_pool / avg_pool /
 * pool_edge [U] (torch_cluster 1.5 grid, torch_sparse 0.6.1 coalesce).  The
 * caller allocates every output at its upper bound (n nodes, n_edges edges);
 * the counts stay on the device (int64 counts[4]: [0] = M clusters, [1] = E'
 * output edges, [2] = edge ends outside [0, n_nodes)) and every kernel that
 * depends on one reads it there.  n, n_edges < 2^31.  No float atomics; every
 * valid output entry is written (no memset by the caller).  The entry points are
 * additions: the ABI version is unchanged.
 *
 * mp_voxel_keys_f32: key[i] = sum_d c_d * prod_{j<d} m_j (wrapping int64) over the
 *   D columns of pos (leading dimension ldp) and, when batch is given, one more
 *   column fl32(batch[i]); size / start / end: device fp32 [D (+ 1)];
 *     c_d = (int64) trunc(fl32(fl32(p_d - start_d) / size_d)),
 *     m_d = (int64) trunc(fl32(fl32(end_d - start_d) / size_d)) + 1
 *   with IEEE fp32 subtraction and division.  D <= 8.  Positions outside
 *   [start, end] follow the same arithmetic (keys may collide or be negative).
 *
 * mp_cluster_build: the consecutive relabelling of any int64 key [n]: one stable
 *   radix sort of (key, node index) over the full signed key, the run heads and
 *   their scan.  inv[i] = the rank of key[i] among the distinct keys (ascending,
 *   signed); rowptr [n + 1] / member [n] (int32): cluster c owns member[rowptr[c]
 *   .. rowptr[c + 1]), node indices ascending (rowptr's first M + 1 entries are
 *   written); perm[c] = the largest node index of cluster c (first M entries);
 *   counts[0] = M.
 *
 * mp_cluster_reduce_f32: one pass over the clusters of rowptr / member, M read
 *   from counts[0]:
 *     x_out[c, :] (leading dimension ldo) = MP_REDUCE_MAX: the maximum over the
 *       members in ascending node order from lowest(), strict compare (the lowest
 *       node index wins a tie); arg[c, f] (int64 [n, F] contiguous, or NULL) =
 *       that node, or n when no member exceeded lowest() (the output is then 0);
 *       MP_FLAG_PYG_MASK: out < -10000 := 0.  MP_REDUCE_MEAN: ((0 + x_0) + x_1)
 *       + ... in ascending node order, divided by the member count.  F = 0: skipped.
 *     pos_out[c, :] ([n, Dp] contiguous) = the mean of pos likewise (Dp = 0: skipped).
 *     batch_out[c] = batch[perm[c]] (batch_out NULL: skipped).
 *   A group of pow2(max(F, Dp)) <= 64 lanes owns a cluster (64 / that many
 *   clusters per wave); the clusters are strided over at most
 *   mp_cluster_max_blocks() workgroups.
 *
 * mp_cluster_edges: pool_edge's index side.  key = inv[row] * M + inv[col]; an
 *   edge with inv[row] == inv[col] is dropped, an edge with an end outside
 *   [0, n_nodes) is dropped and counted in counts[2] (the caller raises).  One
 *   stable radix sort of (key, edge position) over 2 * ceil(log2 n_nodes) + 1
 *   bits, the run heads and their scan:
 *     out_row / out_col (int64 [n_edges], first E' valid) = the distinct pairs in
 *       ascending row * M + col order; edge_slot[e] = the output position of
 *       original edge e, or -1 when it was dropped (every entry written);
 *     seg_ptr [n_edges + 1] / seg_edge [n_edges] (int32): output edge k collects
 *       the original edges seg_edge[seg_ptr[k] .. seg_ptr[k + 1]), ascending;
 *     counts[1] = E'.  counts[0] = M must already be on the device.
 *   out_bytes: the extent of each of out_row, out_col and edge_slot.
 *
 * mp_cluster_edge_attr_f32: out[k, :] = ((0 + attr[e_0, :]) + attr[e_1, :]) + ...
 *   over seg_edge of output edge k in order, for k < counts[1]; out holds
 *   n_edges rows.  mp_cluster_edge_attr_bwd_f32: g_attr[e, :] = g[edge_slot[e], :]
 *   for 0 <= edge_slot[e] < n_out, zeros otherwise (every row written). */
int32_t mp_cluster_max_blocks(void);
int mp_voxel_keys_f32(const float* pos, int64_t ldp, int64_t n, int32_t D, const int64_t* batch, const float* size,
                      const float* start, const float* end, int64_t* key, size_t key_bytes, void* stream);
size_t mp_cluster_build_workspace(int64_t n);
int mp_cluster_build(const int64_t* key, int64_t n, int64_t* inv, size_t inv_bytes, int32_t* rowptr,
                     size_t rowptr_bytes, int32_t* member, size_t member_bytes, int64_t* perm, size_t perm_bytes,
                     int64_t* counts, void* ws, size_t ws_bytes, void* stream);
int mp_cluster_reduce_f32(const float* x, int64_t ldx, int32_t F, int32_t reduce, int32_t flags,
                          const int32_t* rowptr, const int32_t* member, const int64_t* counts, int64_t n,
                          float* x_out, int64_t ldo, size_t x_out_bytes, int64_t* arg, size_t arg_bytes,
                          const float* pos, int64_t ldp, int32_t Dp, float* pos_out, size_t pos_out_bytes,
                          const int64_t* batch, const int64_t* perm, int64_t* batch_out, size_t batch_out_bytes,
                          void* stream);
size_t mp_cluster_edges_workspace(int64_t n_edges, int64_t n_nodes);
int mp_cluster_edges(const int64_t* row, const int64_t* col, int64_t n_edges, const int64_t* inv, int64_t n_nodes,
                     int64_t* counts, int64_t* out_row, int64_t* out_col, int64_t* edge_slot, size_t out_bytes,
                     int32_t* seg_ptr, size_t seg_ptr_bytes, int32_t* seg_edge, size_t seg_edge_bytes, void* ws,
                     size_t ws_bytes, void* stream);
int mp_cluster_edge_attr_f32(const float* attr, int64_t lda, int32_t A, const int32_t* seg_ptr,
                             const int32_t* seg_edge, const int64_t* counts, int64_t n_edges, float* out, int64_t ldo,
                             size_t out_bytes, void* stream);
int mp_cluster_edge_attr_bwd_f32(const float* g, int64_t ldg, const int64_t* edge_slot, int64_t n_edges, int32_t A,
                                 int64_t n_out, float* g_attr, int64_t ldga, size_t g_attr_bytes, void* stream);

/* ---- Graclus (csrc/mp_graclus.hip) --------------------------------------------
 * PyG 1.4.3 nn.pool.graclus [U] (torch_cluster 1.5 graclus_cluster) as a
 * deterministic greedy matching: a pure function of the graph, where upstream's
 * propose / respond rounds depend on a random node order.
 *
 * Pairs.  Edge e = (row[e], col[e]) with row != col is an entry of the unordered
 * pair (a, b), a = min, b = max; loops are ignored, the direction does not
 * matter, an edge present one way only still joins its pair.
 *
 * Priority of an entry: the tuple (wkey, h, a, b), compared lexicographically,
 * the larger wins.
 *   wkey = the order-preserving uint32 image of the fp32 weight: with u its bits,
 *          u >> 31 ? ~u : u | 0x80000000 (so -0.0 < +0.0); 0 when weight is NULL;
 *   h    = the upper 32 bits of mix64(mix64(seed) ^ ((a << 32) | b)), mix64 the
 *          splitmix64 finaliser  z += 0x9E3779B97F4A7C15;
 *          z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *          z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^ (z >> 31)   (mod 2^64).
 * Distinct pairs never compare equal; the entries of one pair differ at most in
 * wkey, so a pair carries the largest weight among its entries of either
 * direction.  NaN weights are outside the contract.
 *
 * Matching.  Walk the entries in descending priority and match (a, b) when both
 * ends are unmatched: cluster[a] = cluster[b] = a; cluster[i] = i for every other
 * node (int64 [n], every entry written).  The kernels compute it in rounds: every
 * live node points at its best entry among unmatched neighbours, mutual pointers
 * match, and a node with no unmatched neighbour left drops out; the order being
 * strict, the result equals the serial walk exactly and depends on neither the
 * launch shape nor the order of the edges.  Hashed priorities take O(log n)
 * rounds in expectation; a path whose weights increase strictly along it takes
 * one round per matched pair.
 *
 * The caller builds the node-sorted incidence list of the 2 * n_edges directed
 * entries with mp_csr_build(key = cat(row, col), other = cat(col, row), 2 *
 * n_edges, n, n): rowptr [n + 1], nbr [2 * n_edges] (= its col) and eid
 * [2 * n_edges] (the entry's position in the concatenation), all int32.
 * n, n_edges < 2^30.  counts (int64[4], device): [0] = rounds run, [1 + (r & 1)] =
 * nodes still live after round r (the nodes with an entry that is no loop count
 * as live before round 0, in [2]), [3] = entries whose position or ends lie
 * outside their range (the caller raises).  ws: mp_graclus_workspace(n, n_edges)
 * bytes, the same block for mp_graclus_init and every mp_graclus_rounds after it.
 *
 * mp_graclus_init: zeroes counts, writes cluster[i] = i, the priority word of every
 *   incidence entry and the live nodes into ws.  weight: fp32 [n_edges] or NULL.
 * mp_graclus_rounds: enqueues rounds first_round .. first_round + n_rounds - 1
 *   (two launches each; n_rounds <= 4096) after mp_graclus_init or an earlier
 *   batch.  A round whose predecessor left nobody live returns at once and is
 *   not counted, so the caller enqueues a batch, reads counts once, and stops
 *   when the slot of the batch's last round is 0.  No grid is capped.
 *
 * Both return int64_t, not a status: the number of launches (init) or rounds
 * (rounds) enqueued, >= 0, or -(MP_ERR_* code) with the reason in mp_last_error()
 * when the call is refused -- for a bad argument, before any launch.  They are
 * therefore not among the `int` status symbols a binding may wrap to raise: the
 * caller tests the sign itself.  The entry points are additions: the ABI version
 * is unchanged. */
size_t mp_graclus_workspace(int64_t n, int64_t n_edges);
int64_t mp_graclus_init(const int64_t* row, const int64_t* col, const float* weight, size_t weight_bytes,
                        int64_t n_edges, int64_t n, uint64_t seed, const int32_t* eid, size_t eid_bytes,
                        int64_t* cluster, size_t cluster_bytes, int64_t* counts, size_t counts_bytes, void* ws,
                        size_t ws_bytes, void* stream);
int64_t mp_graclus_rounds(const int32_t* rowptr, size_t rowptr_bytes, const int32_t* nbr, size_t nbr_bytes,
                          int64_t n_edges, int64_t n, int64_t first_round, int64_t n_rounds, int64_t* cluster,
                          size_t cluster_bytes, int64_t* counts, size_t counts_bytes, void* ws, size_t ws_bytes,
                          void* stream);

/* ---- Point sets: fps, radius, PointConv's edge features (csrc/mp_point.hip) ----
 * The geometry of PyG 1.4.3's PointNet++ set abstraction (nn.fps / nn.radius over
 * torch_cluster 1.5, nn.conv.PointConv [U]) as pure functions of their inputs;
 * tests/_point_ref.py restates them in numpy.  No float is added atomically
 * (the one atomic is an integer count), there is no CPU path, and every index
 * read from device memory is bounded before it is used.  The entry points are
 * additions: the ABI version is unchanged.
 *
 * Squared distance, D = 1..8 columns, fp32, every operation rounded, nothing
 * contracted, left to right:
 *     acc = (a_0 - b_0) * (a_0 - b_0);  acc = acc + (a_d - b_d) * (a_d - b_d), d = 1..D-1
 *
 * mp_fps_f32: farthest point sampling, one workgroup (or wave) per graph.
 *   starts [G + 1]: the graphs' rows of pos (mp_batch_starts); out_starts [G + 1]:
 *   the exclusive scan of k_g (mp_topk_counts: k_g = ceil(fl32(ratio * fl32(n_g))));
 *   start [G] int64: the in-graph offset of each graph's first point, or NULL = 0.
 *   idx[out_starts[g] + t] = the t-th point graph g selects, as a row of pos:
 *   t = 0 is starts[g] + start[g]; then m[i] = d < m[i] ? d : m[i] (from +inf) with
 *   d the squared distance of point i to the last selection, and the next one is
 *   the argmax of m, equal values to the lower index.  A graph with fewer distinct
 *   points than k_g selects points twice.  Non-finite coordinates never fault and
 *   never select outside the graph; what they select is unspecified.
 *   counts (int64[4], device): [0] is left alone (mp_topk_counts wrote K there),
 *   [1] = graphs whose start lies outside [0, n_g) (they start at 0; the caller
 *   raises); a graph of no points ignores its start.
 *   mp_fps_path(n_g): 0 = one wave, m and the points in registers, no barrier
 *   (n_g <= MP_FPS_WAVE_LIMIT, default 256); 1 = one workgroup, registers, one
 *   barrier per step (n_g <= MP_FPS_BLOCK_LIMIT, default 8192); 2 = one workgroup,
 *   m in the workspace; it answers a question and returns int64_t, so it is not among
 *   the `int` status symbols a binding wraps to raise.  max_n: the largest graph (it picks the launches and the
 *   workspace: mp_fps_workspace(n, max_n) bytes; a graph above it is left unsampled).
 *
 * mp_radius_search_f32 / mp_radius_fill: for every row j of y the first `cap`
 *   rows i of x, ascending, of the same graph with d2(x_i, y_j) <= r2,
 *   r2 = fl32(r * r) (squares are compared: one rounding fewer than sqrt(d2) <= r,
 *   and exact on lattice inputs; the boundary is inclusive).  batch_y [n_y] int64
 *   or NULL (graph 0); starts_x [G_x + 1]: graph g of y searches rows
 *   [starts_x[g], starts_x[g + 1]) of x, a g outside [0, G_x) finds nothing.
 *   One wave per query; hits go to a per-query slab of the workspace, their
 *   counts are scanned, counts[0] = E (int64[4], device).  The caller reads E,
 *   allocates out_y / out_x [E] and calls mp_radius_fill with the same workspace
 *   (mp_radius_workspace(n_y, cap) bytes; n_y * cap < 2^31): the pairs sorted by
 *   y, then x.
 *
 * mp_point_edge_features_f32: out[e, :F] = x_src[src[e], :] and
 *   out[e, F + d] = pos_src[src[e], d] - pos_dst[dst[e], d], one pass; F = 0 (x_src
 *   NULL) leaves the differences.  An edge whose src / dst lies outside
 *   [0, n_src) / [0, n_dst) gets a row of zeros (the caller checks the ranges).
 *
 * Like the graclus entry points, the four calls above return int64_t, not a
 * status: the launches enqueued, >= 0, or -(MP_ERR_* code) with the reason in
 * mp_last_error() when the call is refused -- for a bad argument, before any
 * launch.  They are not among the `int` status symbols a binding may wrap to
 * raise: the caller tests the sign itself. */
int64_t mp_fps_path(int64_t n_g);
size_t mp_fps_workspace(int64_t n, int64_t max_n);
int64_t mp_fps_f32(const float* pos, int64_t ldp, int64_t n, int32_t D, const int64_t* starts, int64_t n_graphs,
               int64_t max_n, const int64_t* out_starts, const int64_t* start, int64_t* idx, size_t idx_bytes,
               int64_t* counts, size_t counts_bytes, void* ws, size_t ws_bytes, void* stream);
size_t mp_radius_workspace(int64_t n_y, int64_t cap);
int64_t mp_radius_search_f32(const float* x, int64_t ldx, int64_t n_x, const float* y, int64_t ldy, int64_t n_y, int32_t D,
                         const int64_t* batch_y, const int64_t* starts_x, int64_t n_graphs_x, float r, int64_t cap,
                         int64_t* counts, size_t counts_bytes, void* ws, size_t ws_bytes, void* stream);
int64_t mp_radius_fill(int64_t n_y, int64_t cap, int64_t n_edges, int64_t* out_y, int64_t* out_x, size_t out_bytes,
                   void* ws, size_t ws_bytes, void* stream);
int64_t mp_point_edge_features_f32(const float* x_src, int64_t ldx, int32_t F, const float* pos_src, int64_t ldps,
                               int64_t n_src, const float* pos_dst, int64_t ldpd, int64_t n_dst, int32_t D,
                               const int64_t* src, const int64_t* dst, int64_t n_edges, float* out, int64_t ldo,
                               size_t out_bytes, void* stream);

/* ---- Nearest neighbours: knn, knn_graph, nearest, knn_interpolate (csrc/mp_knn.hip) ----
 * The nearest-neighbour half of torch_cluster 1.5 / PyG 1.4.3 (nn.knn, nn.knn_graph,
 * nn.nearest, nn.unpool.knn_interpolate [U]) as pure functions of their inputs;
 * tests/_knn_ref.py restates them in numpy.  Upstream leaves the order of equal
 * distances to the hardware; here it is defined.  No float is added atomically,
 * there is no CPU path, and every index read from device memory is bounded before
 * it is used.  The entry points are additions: the ABI version is unchanged.
 *
 * Squared distance: the one of "Point sets" with the width lifted.  D = 1 ..
 * MP_KNN_MAX_D columns (a build knob, default 256; mp_knn_max_d()), fp32, every
 * operation rounded, nothing contracted, left to right:
 *     acc = (a_0 - b_0) * (a_0 - b_0);  acc = acc + (a_d - b_d) * (a_d - b_d), d = 1..D-1
 * x and y may have a row stride (ldx, ldy >= D).
 *
 * mp_knn_search_f32: for every row j of y, of the rows i of x in the same graph
 *   (batch_y [n_y] int64 or NULL = graph 0; graph g searches rows [starts_x[g],
 *   starts_x[g + 1]) of x, a g outside [0, n_graphs_x) finds nothing) the
 *   min(k, n_g) smallest under the key (d2(x_i, y_j), i): equal distances go to
 *   the lower index.  d2 >= +0, so (bits(d2) << 32) | in-graph index orders as an
 *   unsigned 64-bit integer; that word is what the kernel compares.  Non-finite
 *   coordinates never fault and never select outside the query's graph; what they
 *   select is unspecified.  1 <= k <= 64 (mp_knn_max_k(): one slot per lane).
 *   One wave per query; lane l holds the l-th smallest key so far, a candidate
 *   below the k-th key is inserted by a wave shift.  mp_knn_path(D): 0 = query and
 *   candidates in registers (D <= 8, a template; a workgroup whose four queries
 *   search the same rows stages its candidates in LDS), 1 = the general width
 *   (the query row in LDS), or -MP_ERR_ARG for a D outside [1, MP_KNN_MAX_D].
 *   The selection goes to a slab of the workspace (mp_knn_workspace(n_y, k) bytes;
 *   n_y * k < 2^31): per query k rows of x as int32, their d2, and a count, in
 *   ascending key.  The counts are scanned; counts[0] = E (int64[4], device).
 *
 * mp_knn_fill: compacts the slab to out_y / out_x [E] int64, sorted by y and
 *   within a y ascending in the key.  out_w (or NULL) [E] float: the pair's
 *   normalised interpolation weight w_t / W_j (below).
 *
 * mp_knn_interpolate_f32: out[j, :] = (sum_t w_t * x[i_t, :]) / (sum_t w_t) over the
 *   slab's entries i_0 .. i_{c-1} of row j, w_t = 1 / max(d2_t, 1e-16f), both sums in
 *   the order t = 0 .. c-1 in fp32, every operation rounded; a row with c = 0 is
 *   zeros.  It needs no E and no host read.  A lane group per row; float4 loads
 *   when x and out are 16-byte aligned with C, ldx and ldo multiples of 4.
 *
 * mp_knn_search_f32, mp_knn_fill and mp_knn_interpolate_f32 return int64_t, not a
 * status: the launches enqueued, >= 0, or -(MP_ERR_* code) with the reason in
 * mp_last_error() when the call is refused -- for a bad argument, before any
 * launch.  They are not among the `int` status symbols a binding may wrap to
 * raise: the caller tests the sign itself.  mp_knn_path, mp_knn_max_k and
 * mp_knn_max_d answer a question. */
int64_t mp_knn_max_k(void);
int64_t mp_knn_max_d(void);
int64_t mp_knn_path(int32_t D);
size_t mp_knn_workspace(int64_t n_y, int64_t k);
int64_t mp_knn_search_f32(const float* x, int64_t ldx, int64_t n_x, const float* y, int64_t ldy, int64_t n_y, int32_t D,
                          const int64_t* batch_y, const int64_t* starts_x, int64_t n_graphs_x, int64_t k,
                          int64_t* counts, size_t counts_bytes, void* ws, size_t ws_bytes, void* stream);
int64_t mp_knn_fill(int64_t n_y, int64_t k, int64_t n_edges, int64_t* out_y, int64_t* out_x, size_t out_bytes,
                    float* out_w, size_t out_w_bytes, void* ws, size_t ws_bytes, void* stream);
int64_t mp_knn_interpolate_f32(const float* x, int64_t ldx, int64_t n_x, int32_t C, int64_t n_y, int64_t k, void* ws,
                               size_t ws_bytes, float* out, int64_t ldo, size_t out_bytes, void* stream);

/* ---- The dense family: DiffPool, DenseSAGEConv, to_dense_* (csrc/mp_dense.hip)
 * PyG 1.4.3's nn.dense.dense_diff_pool [U], per graph b of a dense batch, with
 * x [B, N, F], adj [B, N, N], s [B, N, C] and mask [B, N] (bytes, 0 = padding;
 * NULL = every row live), all contiguous fp32:
 *   P = softmax(s, -1) * mask          T = adj P            V = adj^T P
 *   out [B, C, F] = P^T (x * mask)     out_adj [B, C, C] = P^T T
 *   q_b = sum_ij (adj_ij - p_i . p_j)^2  over all N x N entries, padding included
 *   h_b = sum_ic -p_ic log(p_ic + 1e-15)
 *   loss [4] = (link, ent, Q, H):  Q = sum_b q_b, H = sum_b h_b,
 *              link = sqrt(Q) / (B N N), ent = H / (B N)
 * The residual is formed entry by entry (never as |adj|^2 - 2 tr + |P^T P|^2) and
 * nothing of size [B, N, N] is allocated.  P, T and V ([B, N, C] each) are
 * written for the backward, which never reads adj: with gOut [B, C, F], gOA
 * [B, C, C] and g_loss [2] = (gl, ge) on the device (each may be NULL = zero),
 *   k  = gl / (sqrt(Q) B N N), 0 when Q is 0
 *   dP = x gOut^T + T gOA^T + V gOA - k (T + V - 2 P (P^T P))
 *        - (ge / (B N)) (log(P + 1e-15) + P / (P + 1e-15))
 *   ds = P * (dP - rowsum(dP * P))      (the softmax backward of mask * dP)
 *   dx = P gOut                          (P's masked rows are zero; dx may be NULL)
 * adj receives no gradient from these calls.
 * Forms, from mp_diff_pool_path(N, C, F) (needs no GPU; non-decreasing in N):
 *   0  one workgroup per graph, P, T and V in LDS, adj staged once in row chunks
 *   1  row tiles of a batched fp32 GEMM core; the residual's tile partials and
 *      the rows' entropies go to the workspace and are added in a fixed order
 * No float atomics; every sum has a fixed order, so a call's results are the
 * same bits run to run.  Any B, N, C, F >= 1 within B <= 65535, N <= 2^22 and
 * fewer than 2^24 tiles of 64 x 64 per launch (B * ceil(N / 64)^2 and B * ceil(N /
 * 64) * ceil(max(C, F) / 64)); beyond that, or with a NULL or misaligned (float:
 * 4 bytes, ws: 16) pointer or an array shorter than the call writes, the call is
 * refused before any launch.
 * ws: mp_diff_pool_workspace / mp_diff_pool_bwd_workspace(B, N, C, F) bytes
 * (csrc/mp_dense.hip DiffPoolWs, DiffPoolBwdWs), required.
 *
 * mp_dense_mean_agg_f32, DenseSAGEConv's aggregation: with A^ = adj, its diagonal
 * read as 1 when add_loop (adj itself is never copied or written),
 *   transpose = 0:  deg_out[b, i] = sum_j A^_ij,  out[b, i, :] = (sum_j A^_ij x[b, j, :]) / max(deg, 1)
 *   transpose = 1:  out[b, j, :] = sum_i A^_ij x[b, i, :] / max(deg_in[b, i], 1)
 * one pass over adj each; the second is the first's gradient for x (x = the
 * incoming gradient, deg_in = the saved deg_out).
 *
 * mp_to_dense_batch_f32: over the segment starts of a sorted batch vector
 * (starts [B + 1], as the readout above), out[g, i, :] = x[starts[g] + i, :] for
 * i < n_g, else fill; mask[g, i] = i < n_g (bytes).  Nmax must be at least the
 * largest graph.  mp_to_dense_batch_bwd_f32 is the row gather dx[starts[g] + i,
 * :] = g[g, i, :].  mp_to_dense_adj_f32: out [B, Nmax, Nmax] (D = 0, edge_attr
 * NULL) or [B, Nmax, Nmax, D] is zeroed, then edge e = (row, col) of graph g =
 * batch[row] (batch NULL: one graph) sets cell (g, row - starts[g], col -
 * starts[g]) to 1, or to edge_attr[e, :]; of several edges of one cell the last
 * in edge order wins (an integer maximum over edge indices in the workspace,
 * mp_to_dense_adj_workspace(B, Nmax, D) bytes).  An edge whose ends do not lie
 * in one graph's [0, Nmax) is skipped.
 * Every call returns the launches enqueued, >= 0, or -(MP_ERR_* code). */
int64_t mp_diff_pool_path(int64_t N, int32_t C, int32_t F);
size_t mp_diff_pool_workspace(int64_t B, int64_t N, int32_t C, int32_t F);
size_t mp_diff_pool_bwd_workspace(int64_t B, int64_t N, int32_t C, int32_t F);
int64_t mp_dense_diff_pool_f32(const float* x, const float* adj, const float* s, const uint8_t* mask, int64_t B,
                               int64_t N, int32_t C, int32_t F, float* out, size_t out_bytes, float* out_adj,
                               size_t out_adj_bytes, float* loss, size_t loss_bytes, float* P, size_t P_bytes,
                               float* T, size_t T_bytes, float* V, size_t V_bytes, void* ws, size_t ws_bytes,
                               void* stream);
int64_t mp_dense_diff_pool_bwd_f32(const float* g_out, const float* g_oa, const float* g_loss, const float* x,
                                   const float* P, const float* T, const float* V, const float* loss, int64_t B,
                                   int64_t N, int32_t C, int32_t F, float* dx, size_t dx_bytes, float* ds,
                                   size_t ds_bytes, void* ws, size_t ws_bytes, void* stream);
int64_t mp_dense_mean_agg_f32(const float* adj, const float* x, int64_t B, int64_t N, int32_t F, int32_t add_loop,
                              int32_t transpose, const float* deg_in, float* out, size_t out_bytes, float* deg_out,
                              size_t deg_out_bytes, void* stream);
int64_t mp_to_dense_batch_f32(const float* x, int64_t n, int32_t F, const int64_t* starts, int64_t B, int64_t Nmax,
                              float fill, float* out, size_t out_bytes, uint8_t* mask, size_t mask_bytes,
                              void* stream);
int64_t mp_to_dense_batch_bwd_f32(const float* g, int64_t n, int32_t F, const int64_t* starts, int64_t B,
                                  int64_t Nmax, float* dx, size_t dx_bytes, void* stream);
size_t mp_to_dense_adj_workspace(int64_t B, int64_t Nmax, int32_t D);
int64_t mp_to_dense_adj_f32(const int64_t* row, const int64_t* col, int64_t E, const float* edge_attr, int32_t D,
                            const int64_t* batch, int64_t n, const int64_t* starts, int64_t B, int64_t Nmax,
                            float* out, size_t out_bytes, void* ws, size_t ws_bytes, void* stream);

/* ---- Link prediction: GAE / VGAE decoder, loss and negative sampler (csrc/mp_link.hip)
 * PyG 1.4.x's InnerProductDecoder [U] scores an edge list as (z[row] * z[col]).sum(1)
 * over two [E, C] gathers, GAE.recon_loss takes -log(sigmoid + 1e-15) means of it, and
 * utils.negative_sampling draws on the host and retries.  These calls keep no [E, C]
 * array, use no float atomics and read nothing back.
 *   row, col [E] int64 in any order (repeats and row == col allowed), z [N, ldz] fp32 with
 *   C >= 1 columns used, ldz >= C.  An edge with an end outside [0, N) reads nothing
 *   and scores NaN.  A group of G lanes serves one edge: G = mp_link_lanes(C, vec4), the
 *   power of two covering C / 4 lanes of 16-byte loads, at most 16 (vec4: C % 4 == 0,
 *   ldz % 4 == 0 and z 16-byte aligned), or C scalar lanes, at most 64, looping beyond;
 *   `lanes` overrides it (0 = that rule; else a power of two up to 64).  Each lane adds its
 *   columns' products in column order and the group adds its lanes in a fixed tree, so
 *   v[e] depends on C, the mapping and the two rows only.
 *
 * mp_edge_score_f32: v[e] = sum_c z[row_e, c] * z[col_e, c], or its sigmoid
 *   1 / (1 + expf(-v)).
 * mp_link_loss_f32: one side of the reconstruction loss.  With p = 1 / (1 + expf(-v_e))
 *   and EPS = 1e-15f, in fp32: positive = 1: t_e = -logf(p + EPS), coef[e] = -p (1 - p) /
 *   (p + EPS) / E; positive = 0: t_e = -logf(1 - p + EPS), coef[e] = p (1 - p) / (1 - p +
 *   EPS) / E -- coef[e] is d(mean t) / dv_e, so a backward never forms v again.  1 - p
 *   is evaluated as 1 / (1 + expf(v_e)): the same quantity, without the cancellation
 *   of the fp32 subtraction once p nears 1.  The t_e
 *   are added in fp64 in a fixed order (per-block partials in ws, one block adds them by
 *   index) and loss[0] is the mean, rounded once to fp32; E = 0 gives nan.
 *   ws: mp_link_loss_workspace(E) bytes (csrc/mp_link.hip LinkLossWs), 16-byte aligned.
 * mp_link_grad_rows_f32: dz[r, :] = (init_from_out ? dz[r, :] : 0) + sum over the slots s
 *   of row r, in slot order, of coef[eid[s] mod n_coef] * z[col[s], :] over the rowptr /
 *   col / eid of mp_csr_build -- no schedule and no read of its bad-index count are
 *   needed; a slot whose column is outside [0, N) is skipped.  One lane group walks a
 *   row.  With the CSR built over the 2 E entries key = [row | col], other = [col | row]
 *   and n_coef = E this is the whole gradient of z of a score or a loss over (row,
 *   col): dz[i] = sum_{row_e = i} coef_e z[col_e] + sum_{col_e = i} coef_e z[row_e].
 *   n_slots / 2 <= n_coef <= n_slots.
 * mp_neg_sample: n_samples draws, with replacement, from the keys in [0, T) that are
 *   NOT in the sorted distinct table keys[0..U), U = n_keys[0] read on the device (at
 *   most keys_bytes / 8).  mode 0: key = row * N + col, T = N * N; mode 1: the strict
 *   upper triangle, key = j (j - 1) / 2 + i for i < j, T = N (N - 1) / 2.  Draw s takes
 *   r = mulhi64(h, T - U) with h = mix(mix(seed) ^ s), mix the splitmix64 finaliser,
 *   finds the smallest j with keys[j] - j > r by binary search and returns key r + j:
 *   uniform over the non-edges, exact, and one search whatever the density.  mode 0
 *   writes out_row / out_col [n_samples]; mode 1 writes [2 n_samples], the pair then
 *   its mirror: out_row = [i | j], out_col = [j | i].  With T - U <= 0 every entry is -1.
 * mp_neg_sample_rows: for edge e with i = row[e], the r-th column missing from row i's
 *   keys (mode 0's table; two lower bounds give the row's d_i keys), r = mulhi64(h(seed,
 *   e), N - d_i).  A full row (d_i = N) or an i outside [0, N) gives -1.
 * N <= 3037000499 (N * N below 2^63).  Every call returns the launches enqueued, >= 0,
 * or -(MP_ERR_* code) with the reason in mp_last_error(), for a bad argument before
 * any launch; mp_link_lanes answers a question (or -MP_ERR_ARG for C < 1). */
int64_t mp_link_lanes(int32_t C, int32_t vec4);
int64_t mp_edge_score_f32(const int64_t* row, const int64_t* col, int64_t E, const float* z, int64_t ldz, int64_t N,
                          int32_t C, int32_t sigmoid, int32_t lanes, float* v, size_t v_bytes, void* stream);
size_t mp_link_loss_workspace(int64_t E);
int64_t mp_link_loss_f32(const int64_t* row, const int64_t* col, int64_t E, const float* z, int64_t ldz, int64_t N,
                         int32_t C, int32_t positive, int32_t lanes, float* coef, size_t coef_bytes, float* loss,
                         size_t loss_bytes, void* ws, size_t ws_bytes, void* stream);
int64_t mp_link_grad_rows_f32(const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t n_rows,
                              int64_t n_slots, const float* coef, int64_t n_coef, const float* z, int64_t ldz,
                              int64_t N, int32_t C, int32_t init_from_out, float* dz, int64_t lddz, size_t dz_bytes,
                              void* stream);
int64_t mp_neg_sample(const int64_t* keys, size_t keys_bytes, const int64_t* n_keys, int64_t N, int32_t mode,
                      uint64_t seed, int64_t n_samples, int64_t* out_row, int64_t* out_col, size_t out_bytes,
                      void* stream);
int64_t mp_neg_sample_rows(const int64_t* keys, size_t keys_bytes, const int64_t* n_keys, int64_t N, uint64_t seed,
                           const int64_t* row, int64_t E, int64_t* out, size_t out_bytes, void* stream);

/* ---- other dtypes (csrc/mp_dtype.hip) -------------------------------------
 * torch_scatter 2.0.4 reduces any dtype ([U8/U9]); the fp32 hot path is
 * mp_aggregate_f32, these are the breadth path for the rest. */
#define MP_DTYPE_F32 0
#define MP_DTYPE_F64 1
#define MP_DTYPE_F16 2
#define MP_DTYPE_BF16 3
#define MP_DTYPE_I64 4

/* out[r, :] = REDUCE_{k in row r} src[col[k], :] (col NULL: src row k), rows
 * of `dtype` with leading dimensions lds / ldo in elements.  Every row is
 * reduced by one wave per 64-feature tile in slot (= original edge) order,
 * never split: float64 / int64 follow the reference's arithmetic bit for bit
 * (int64 sums wrap); float16 / bfloat16 accumulate in fp32 and round once.
 * max / min: strict compare (first edge wins), start at the type's lowest() /
 * max(); a row that keeps it reports 0 and arg = n_ids (n_edges when 0); arg_out
 * int64 [n_rows, F] (contiguous).  mean: (sum [+ out]) / max(count, 1), integer
 * division truncating toward zero.  flags: MP_FLAG_INIT_FROM_OUT (torch_scatter
 * `out=`), MP_FLAG_PYG_MASK (utils.scatter_'s +-10000 masks). */
int mp_segment_reduce(const mp_csr* g, int32_t dtype, const void* src, int64_t lds,
                      int32_t F, int32_t reduce, int32_t flags, void* out, int64_t ldo,
                      int64_t* arg_out, void* stream);

/* out[k, :] = x[idx[k], :] for elements of elem_bytes (2, 4 or 8) bytes. */
int mp_gather_rows_any(int32_t elem_bytes, const void* x, int64_t ldx, const int64_t* idx,
                       int64_t n, int32_t F, void* out, int64_t ldo, void* stream);

/* grad[arg[r, f], f] = grad_out[r, f] for arg in [0, n_edges) (ScatterMax
 * backward on materialised messages; grad zero-initialised by the caller). */
int mp_scatter_arg_any(int32_t elem_bytes, const void* grad_out, const int64_t* arg,
                       int64_t n_rows, int32_t F, int64_t n_edges, void* grad, int64_t ldg,
                       void* stream);

/* ---- helpers on the path -------------------------------------------------- */

/* out[k,:] = x[idx[k],:]  (index_select of __collect__, scatter-sum backward,
 * halo packing for the multi-GPU exchange) */
int mp_gather_rows_f32(const float* x, int64_t ldx, const int64_t* idx,
                       int64_t n, int32_t F, float* out, int64_t ldo,
                       void* stream);

/* dst[k] = src[perm[k]] (CSR-ordering of per-edge weights) */
int mp_permute_f32(const float* src, const int32_t* perm, int64_t n,
                   float* dst, void* stream);

/* ---- deterministic source-side reductions (csrc/mp_segment.hip) ----------- */

/* out[r] = ((0 + v[id(k0)]) + v[id(k0+1)]) + ... over the slots k of row r in
 * slot order, id(k) = eid[k] (eid NULL: k).  Bit-identical to the serial CPU
 * loop.  Over the transposed CSR (rows = edge_index[0]) with v = the edge
 * weights in original order it is GCNConv.norm's deg = scatter_add(w, row) [U5]
 * in the reference's edge order (replaces the float atomics of mp_gcn_norm_f32
 * for real-valued weights). */
int mp_segment_sum_serial_f32(const int32_t* rowptr, const int32_t* eid, const float* v,
                              int64_t n_rows, float* out, void* stream);

/* GCNConv.norm steps 2-3 from a given degree: deg is overwritten with
 * deg^-1/2 (inf -> 0), norm[e] = dinv[row[e]] * w[e] * dinv[col[e]]. */
int mp_gcn_norm_from_deg_f32(const int64_t* row, const int64_t* col, const float* w,
                             int64_t n_edges, int64_t n_nodes, float* deg, float* norm,
                             void* stream);

/* inv[eid[k]] = k for every slot k of g (the slot of each edge id). */
int mp_csr_inverse_eid(const mp_csr* g, int32_t* inv, void* stream);

/* Deterministic ScatterMax/ScatterMin backward of a fused message w_e * x[src_e]
 * ([U8] ScatterMax.backward, then the message's and index_select's backward:
 * an index_add_ by source in edge order).  Three steps over the TRANSPOSED CSR
 * gt (rows = source nodes, slots = out-edges in original order, col = the
 * destination row, eid = the edge id):
 *   1. mp_arg_winner_mask: mask [gt.n_edges, mp_arg_mask_words(F)] uint32 in gt
 *      slot order, bit f of slot inv[e] set when arg[r, f] = e (inv =
 *      mp_csr_inverse_eid(gt)); ids outside [0, n_edges) (empty rows) set nothing.
 *   2. mp_scatter_arg_backward_csr_f32: grad[j, f] = sum over the slots of row j
 *      in order of w_e * grad_out[dst, f] where the slot won (j, f) -- the
 *      reference's edge-order sum, bit for bit; every row of grad is written.
 *      w: per-edge weights in ORIGINAL edge order, or NULL (= 1).
 *   3. (optional) mp_scatter_arg_grad_w_f32: grad_w[e] = sum over the features
 *      e won of grad_out[dst_map[e], f] * x[src_map[e], f] (fixed reduction tree),
 *      0 for edges that won nothing; every entry written.
 * The mask must be 8-byte aligned; mask_bytes >= n_edges * mp_arg_mask_words(F) * 4
 * in all three calls (ABI 6). */
int32_t mp_arg_mask_words(int32_t F);
int mp_arg_winner_mask(const int64_t* arg, int64_t n_rows, int32_t F, int64_t n_edges,
                       const int32_t* inv, uint32_t* mask, size_t mask_bytes, void* stream);
int mp_scatter_arg_backward_csr_f32(const mp_csr* gt, const uint32_t* mask, size_t mask_bytes,
                                    const float* grad_out, int64_t ldg, int32_t F,
                                    const float* w, float* grad, int64_t ldgx, void* stream);
int mp_scatter_arg_grad_w_f32(const int64_t* src_map, const int64_t* dst_map, int64_t n_edges,
                              const int32_t* inv, const uint32_t* mask, size_t mask_bytes, int32_t F,
                              const float* grad_out, int64_t ldg, const float* x, int64_t ldx,
                              float* grad_w, void* stream);

/* ScatterMax/ScatterMin backward [U8] on materialised message rows (torch_scatter
 * scatter_max / scatter_min of src [n_edges, F]): for every (r,f) with
 * arg[r,f] = e != n_edges, grad[e, f] = grad_out[r,f] -- a plain store (row e
 * belongs to one output row), deterministic.  grad must be zero-initialised by
 * the caller.  The fused message w_e * x[src_e] takes the CSR form above.
 * (ABI 5: the float-atomic src_map / grad_w form of ABI <= 4 is gone.) */
int mp_scatter_arg_backward_f32(const float* grad_out, const int64_t* arg,
                                int64_t n_rows, int32_t F, int64_t n_edges,
                                float* grad, int64_t ldg, void* stream);

/* GCNConv.norm [U5]: deg = scatter_add(w, row); dinv = deg^-1/2 (inf -> 0);
 * norm[e] = dinv[row[e]] * w[e] * dinv[col[e]] (original edge order).
 * w == NULL means all ones.  deg_ws: n_nodes floats of workspace.  The degree
 * is summed with float atomics: exact (hence deterministic) only for
 * integer-valued weights (self-loop fills 1 / 2, unweighted graphs); for real
 * weights use mp_segment_sum_serial_f32 + mp_gcn_norm_from_deg_f32. */
int mp_gcn_norm_f32(const int64_t* row, const int64_t* col, const float* w,
                    int64_t n_edges, int64_t n_nodes, float* deg_ws,
                    float* norm, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* MI355_MP_H */
