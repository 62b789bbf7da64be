// RGCNConv's aggregation over a basis decomposition (gfx950).
//
// Per edge e = (j -> i) of relation t_e the layer's message is m_e = n_e x_j W_{t_e}
// with W_r = sum_b att[r, b] basis[b] ([Cin, Cout]) and n_e the edge norm.  With the
// per-edge coefficient vector a_e = n_e att[t_e, :] in R^B and V = basis viewed as
// [B * Cin, Cout] the per-edge step (an [E, Cin, Cout] array and E mat-vecs) is
// reordered into ONE segmented pass plus one dense node-level GEMM:
//   bins form    Z[i, b*Cin + c] = sum_{e -> i} a_e[b] * x[j, c],  then out = Z @ V
//   gather form  out[i, f] = sum_{e -> i} sum_b a_e[b] * Y[j, b, f] (+ bias)
//                with Y = x @ L' laid out [n, B, Cout]
// a_e is never stored: the kernels read edge_type (int64) and edge_norm (fp32 or
// NULL = 1) in ORIGINAL edge order through eid, and the [R, B] table att.  A
// type outside [0, R) is the caller's to reject (ops range-checks them once per
// edge_type tensor); the kernels give such a slot the coefficient 0 without
// reading att, so it is never an out-of-bounds read.
//
// Both aggregate kernels address one operand through TWO strides (node, block):
//   bins    out[r * ld_node + b * ld_block + c]     Z [N, B*Cin]: (ldz, Cin);
//           d basis [B, N, Cout] of the featureless backward: (Cout, N*Cout)
//   gather  y[col * ld_node + b * ld_block + f]     Y / dZ [N, B, F]: (B*F, F);
//           basis [B, N, Cout] itself, read in place:  (Cout, N*Cout)
// so the featureless layer (x = None: Cin = N) never takes a permuted copy of basis.
//
// One owner per output entry visits its row's slots in slot order and adds left
// to right (the gather form: b = 0..B-1 inside a slot): deterministic, no
// atomics, bitwise reproducible.  Rows of any length are summed serially; hub
// rows are not split.  The att table is read through the cache at every size (no
// LDS staging).  Lane mappings (NNConv's):
//   bins, C < 32   ("flat"): lanes over the flattened q = b*C + c, a row owned by
//       g = min(64, pow2 >= B*C) lanes and 64/g rows per wave; a wider row gives
//       each lane up to 8 entries (q = lane, lane + 64, ...), so that its slot
//       chain is walked by as few waves as possible, and is tiled by 64 * 8 over
//       blockIdx.y beyond that.
//   bins, C >= 32  ("columns"): one wave per (row, 64 columns c, 16 values of b);
//       lanes map to c, a slot's coefficients are wave-uniform and x[col][c] is
//       one coalesced load reused by the lane's 16 accumulators.
//   gather: lanes map to f (g = min(64, pow2 >= F) lanes per row, 64/g rows per
//       wave, F tiled by 64); b serial, eight load pairs in flight.
//
// d att[r, b] = sum_{e: t_e = r} n_e sum_c P[rows[e], b, c] Q[cols[e], c] runs over
// a relation plan (perm: the edge ids stably sorted by type; relptr [R + 1]):
//   chunks   chunkptr[r] = sum_{r' < r} ceil(count_{r'} / kRgcnAttChunk)
//   stage 1  one workgroup per chunk of kRgcnAttChunk edges of ONE relation:
//            g = pow2 >= min(B, 64) lanes over b, 256/g lane groups; a lane adds
//            its edges i = sub, sub + 256/g, ... in order (four of them loaded
//            at a time, rows in 16-byte pieces where the layout allows: the
//            arithmetic is the same either way), then lane b adds the 256/g
//            lane partials in sub order (LDS): one [B] partial row
//   stage 2  one owner per (r, b) adds the relation's chunk partials in chunk order
// A relation without edges owns no chunk and gets zeros.
#include "mp_workspace.h"

namespace mp {

constexpr int64_t kRgcnMaxRow = 1 << 20;       // floats in one row of Z or Y (4 MiB)
constexpr int kRgcnMaxRelations = 1 << 16;     // chunkptr is one serial pass over the relations
constexpr int kRgcnColumnsMinC = 32;           // bins: lanes over c from here on
constexpr int kRgcnBTile = 16;                 // bins, columns mapping: accumulators per lane
constexpr int kRgcnAttChunk = 256;             // att grad: edges of one relation per stage-1 workgroup

static inline int rg_group_log2(int64_t n) {
  int gl = 0;
  while ((1 << gl) < n && gl < 6) ++gl;
  return gl;
}

// the arguments every kernel reads a slot's coefficients through
struct RgCoef {
  const int64_t* type;  // [n_type_edges], original edge order
  const float* norm;    // the same, or nullptr (= 1)
  const float* att;     // [R, ld_att >= B]
  int64_t ld_att;
  int32_t R, B;
};

// n_e and the row of att of edge id `id`; nullptr for a type outside [0, R)
__device__ __forceinline__ const float* rg_att_row(const RgCoef& k, int64_t id, float* nr) {
  const int64_t t = k.type[id];
  *nr = k.norm ? k.norm[id] : 1.f;
  return (uint64_t)t < (uint64_t)k.R ? k.att + t * k.ld_att : nullptr;
}

// ---------------------------------------------------------------------------
// bins form, lanes over the flattened (b, c)
// ---------------------------------------------------------------------------
// T entries per lane (q = tile * 64 + lane for T consecutive tiles; T > 1 only for
// rows of more than 64 entries, glog = 6): the row's slot chain -- col, eid, type,
// norm -- is walked once for the T entries, whose T load pairs are in flight together
template <int T>
__global__ __launch_bounds__(256) void k_rgcn_bins_flat(const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col,
                                                        const int32_t* __restrict__ eid, int64_t n_rows, RgCoef k,
                                                        const float* __restrict__ x, int64_t ldx, int32_t C,
                                                        int32_t glog, float* __restrict__ out, int64_t ld_node,
                                                        int64_t ld_block) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> glog;
  const int fl = lane & ((1 << glog) - 1);
  const int64_t r = (((int64_t)blockIdx.x * 4 + wave) << (6 - glog)) + sub;
  const int Q = k.B * C;
  int bb[T], c[T];
  bool live[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int q = (blockIdx.y * T + t) * 64 + fl;
    live[t] = q < Q;
    bb[t] = live[t] ? q / C : 0;  // a dead entry reads entry 0 and stores nothing
    c[t] = live[t] ? q - bb[t] * C : 0;
  }
  if (r >= n_rows || !live[0]) return;
  const int b = rowptr[r], e = rowptr[r + 1];
  float acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 0.f;
  int32_t nc = 0, ne = 0;
  if (b < e) {
    nc = col[b];
    ne = eid[b];
  }
  for (int s = b; s < e; ++s) {
    const int32_t cc = nc;
    const int64_t id = ne;
    if (s + 1 < e) {
      nc = col[s + 1];
      ne = eid[s + 1];
    }
    float nr;
    const float* ar = rg_att_row(k, id, &nr);
    const float* xr = x + (int64_t)cc * ldx;
    float av[T], xv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      av[t] = ar ? ar[bb[t]] : 0.f;
      xv[t] = xr[c[t]];
    }
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = __fadd_rn(acc[t], __fmul_rn(__fmul_rn(nr, av[t]), xv[t]));
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (live[t]) out[r * ld_node + (int64_t)bb[t] * ld_block + c[t]] = acc[t];
  }
}

// ---------------------------------------------------------------------------
// bins form, lanes over c; wave = (row, 64 columns, kRgcnBTile values of b)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rgcn_bins_cols(const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col,
                                                        const int32_t* __restrict__ eid, int64_t n_rows, RgCoef k,
                                                        const float* __restrict__ x, int64_t ldx, int32_t C,
                                                        float* __restrict__ out, int64_t ld_node, int64_t ld_block) {
  constexpr int T = kRgcnBTile;
  const int lane = lane_id();
  const int64_t r = (int64_t)blockIdx.x * 4 + uni((int)(threadIdx.x >> 6));
  const int c = blockIdx.y * 64 + lane;
  const int b0 = blockIdx.z * T;
  if (r >= n_rows || c >= C) return;
  const int b = rowptr[r], e = rowptr[r + 1];
  float acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 0.f;
  for (int s = b; s < e; ++s) {
    const int32_t cc = col[s];
    float nr;
    const float* ar = rg_att_row(k, eid[s], &nr);
    const float xv = x[(int64_t)cc * ldx + c];
    float av[T];
#pragma unroll
    for (int t = 0; t < T; ++t) av[t] = (ar && b0 + t < k.B) ? __fmul_rn(nr, ar[b0 + t]) : 0.f;
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = __fadd_rn(acc[t], __fmul_rn(av[t], xv));
  }
  float* o = out + r * ld_node + c;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (b0 + t < k.B) o[(int64_t)(b0 + t) * ld_block] = acc[t];
  }
}

// ---------------------------------------------------------------------------
// gather form: y[col * ld_node + b * ld_block + f]
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rgcn_gather(const int32_t* __restrict__ rowptr,
                                                     const int32_t* __restrict__ col,
                                                     const int32_t* __restrict__ eid, int64_t n_rows, RgCoef k,
                                                     const float* __restrict__ y, int64_t ld_node, int64_t ld_block,
                                                     int32_t F, int32_t glog, const float* __restrict__ bias,
                                                     float* __restrict__ out, int64_t ldo) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> glog;
  const int fl = lane & ((1 << glog) - 1);
  const int64_t r = (((int64_t)blockIdx.x * 4 + wave) << (6 - glog)) + sub;
  const int f = blockIdx.y * 64 + fl;
  if (r >= n_rows || f >= F) return;
  const int b = rowptr[r], e = rowptr[r + 1];
  const int B = k.B;
  float acc = 0.f;
  for (int s = b; s < e; ++s) {
    const float* yr = y + (int64_t)col[s] * ld_node + f;
    float nr;
    const float* ar = rg_att_row(k, eid[s], &nr);
    if (!ar) continue;
    int bb = 0;
    for (; bb + 8 <= B; bb += 8) {  // eight independent load pairs in flight, added in b order
      float av[8], yv[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        av[t] = ar[bb + t];
        yv[t] = yr[(int64_t)(bb + t) * ld_block];
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) acc = __fadd_rn(acc, __fmul_rn(__fmul_rn(nr, av[t]), yv[t]));
    }
    for (; bb < B; ++bb) acc = __fadd_rn(acc, __fmul_rn(__fmul_rn(nr, ar[bb]), yr[(int64_t)bb * ld_block]));
  }
  if (bias) acc = __fadd_rn(acc, bias[f]);
  out[r * ldo + f] = acc;
}

// ---------------------------------------------------------------------------
// att grad: chunk starts, chunk partials, the sum over a relation's chunks
// ---------------------------------------------------------------------------

// chunkptr [R + 1] and part [max_chunks, B] of one mp_rgcn_att_grad_f32 call
static inline int64_t rg_max_chunks(int64_t n_edges, int32_t R) {
  return ceil_div(n_edges > 0 ? n_edges : 0, kRgcnAttChunk) + (R > 0 ? R : 0);
}
struct RgcnAttWs : Carver {
  int64_t* chunkptr;
  float* part;
  RgcnAttWs(void* ws, int64_t n_edges, int32_t R, int32_t B)
      : Carver(ws), chunkptr(take<int64_t>((int64_t)R + 1)), part(take<float>(rg_max_chunks(n_edges, R) * B)) {}
};

// relptr is clamped into [0, n_edges] and made non-decreasing as it is read, so
// no relptr can name more chunks than max_chunks or an edge position outside perm
__device__ __forceinline__ int64_t rg_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ void k_rgcn_chunkptr(const int64_t* __restrict__ relptr, int32_t R, int64_t n_edges,
                                int64_t* __restrict__ chunkptr) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int64_t at = 0, lo = rg_clamp(relptr[0], 0, n_edges);
  chunkptr[0] = 0;
  for (int r = 0; r < R; ++r) {
    const int64_t hi = rg_clamp(relptr[r + 1], lo, n_edges);
    at += (hi - lo + kRgcnAttChunk - 1) / kRgcnAttChunk;
    chunkptr[r + 1] = at;
    lo = hi;
  }
}

// V = 4: 16-byte row loads (C, the strides and the base pointers multiples of four floats); V = 1 otherwise
template <int V>
__global__ __launch_bounds__(256) void k_rgcn_att_part(const int64_t* __restrict__ perm,
                                                       const int64_t* __restrict__ relptr,
                                                       const int64_t* __restrict__ chunkptr,
                                                       const int64_t* __restrict__ rows,
                                                       const int64_t* __restrict__ cols, int64_t n_edges,
                                                       const float* __restrict__ norm, const float* __restrict__ P,
                                                       int64_t ldp_node, int64_t ldp_block,
                                                       const float* __restrict__ Q, int64_t ldq, int32_t R, int32_t B,
                                                       int32_t C, int32_t glog, float* __restrict__ part) {
  __shared__ float lds[256];
  const int64_t j = blockIdx.x;
  if (j >= chunkptr[R]) return;  // the grid is the upper bound; the whole workgroup leaves
  int lo_r = 0, hi_r = R;        // the relation r with chunkptr[r] <= j < chunkptr[r + 1]
  while (hi_r - lo_r > 1) {
    const int mid = (lo_r + hi_r) >> 1;
    if (chunkptr[mid] <= j) lo_r = mid; else hi_r = mid;
  }
  const int r = lo_r;
  const int64_t first = rg_clamp(relptr[r], 0, n_edges);
  const int64_t last = rg_clamp(relptr[r + 1], first, n_edges);
  const int64_t lo = first + (j - chunkptr[r]) * kRgcnAttChunk;
  const int64_t hi = lo + kRgcnAttChunk < last ? lo + kRgcnAttChunk : last;
  const int g = 1 << glog;
  const int nsub = 256 >> glog;
  const int sub = threadIdx.x >> glog;
  const int bl = threadIdx.x & (g - 1);
  const int b = blockIdx.y * 64 + bl;
  float acc = 0.f;
  if (b < B) {
    // a lane's edges four at a time: their index chains (perm -> rows / cols -> P, Q) and row loads are in
    // flight together; each dot adds c = 0..C-1 in order and acc takes the edges in position order, whatever V
    constexpr int U = 4;
    for (int64_t i = lo + sub; i < hi; i += (int64_t)U * nsub) {
      const float *p[U], *q[U];
      float nr[U], s[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int64_t at = i + (int64_t)u * nsub;
        const int64_t e = at < hi ? perm[at] : -1;
        ok[u] = (uint64_t)e < (uint64_t)n_edges;
        const int64_t ee = ok[u] ? e : 0;  // a dead edge reads edge 0's rows and adds nothing
        p[u] = P + rows[ee] * ldp_node + (int64_t)b * ldp_block;
        q[u] = Q + cols[ee] * ldq;
        nr[u] = norm ? norm[ee] : 1.f;
        s[u] = 0.f;
      }
      for (int c = 0; c < C; c += V) {
        float pv[U][V], qv[U][V];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          if constexpr (V == 4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(p[u] + c);
            const f32x4 w = *reinterpret_cast<const f32x4*>(q[u] + c);
            pv[u][0] = a.x; pv[u][1] = a.y; pv[u][2] = a.z; pv[u][3] = a.w;
            qv[u][0] = w.x; qv[u][1] = w.y; qv[u][2] = w.z; qv[u][3] = w.w;
          } else {
            pv[u][0] = p[u][c];
            qv[u][0] = q[u][c];
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
          for (int v = 0; v < V; ++v) s[u] = __fadd_rn(s[u], __fmul_rn(pv[u][v], qv[u][v]));
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (ok[u]) acc = __fadd_rn(acc, norm ? __fmul_rn(nr[u], s[u]) : s[u]);
      }
    }
  }
  lds[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < g && b < B) {
    float t = 0.f;
    for (int s = 0; s < nsub; ++s) t = __fadd_rn(t, lds[s * g + bl]);
    part[j * B + b] = t;
  }
}

__global__ __launch_bounds__(256) void k_rgcn_att_sum(const int64_t* __restrict__ chunkptr,
                                                      const float* __restrict__ part, int64_t max_chunks, int32_t R,
                                                      int32_t B, float* __restrict__ datt, int64_t ld_datt) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (tid >= (int64_t)R * B) return;
  const int r = (int)(tid / B);
  const int b = (int)(tid - (int64_t)r * B);
  const int64_t lo = chunkptr[r];
  const int64_t hi = chunkptr[r + 1] < max_chunks ? chunkptr[r + 1] : max_chunks;
  float t = 0.f;
  int64_t j = lo;
  for (; j + 8 <= hi; j += 8) {  // eight loads in flight, added in chunk order
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(j + u) * B + b];
#pragma unroll
    for (int u = 0; u < 8; ++u) t = __fadd_rn(t, v[u]);
  }
  for (; j < hi; ++j) t = __fadd_rn(t, part[j * B + b]);
  datt[(int64_t)r * ld_datt + b] = t;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// One (B, C) pair of the fused path: a row of B * C floats.
static int rg_shape(const char* fn, int32_t R, int32_t B, int32_t C, const char* cname) {
  MP_CHECK_ARG(R >= 1, "%s: R = %d < 1", fn, R);
  MP_CHECK_ARG(R <= kRgcnMaxRelations, "%s: R = %d above the limit R <= %d", fn, R, kRgcnMaxRelations);
  MP_CHECK_ARG(B >= 1, "%s: B = %d < 1", fn, B);
  MP_CHECK_ARG(C >= 1, "%s: %s = %d < 1", fn, cname, C);
  MP_CHECK_ARG((int64_t)B * C <= kRgcnMaxRow, "%s: B * %s = %lld above the limit B * C <= %lld", fn, cname,
               (long long)((int64_t)B * C), (long long)kRgcnMaxRow);
  return MP_OK;
}

static int rg_csr(const char* fn, const mp_csr* g, const int64_t* edge_type, int64_t n_type_edges, const float* att,
                  int64_t ld_att, size_t att_bytes, int32_t R, int32_t B) {
  MP_CHECK_ARG(g != nullptr, "%s: g is NULL", fn);
  MP_CHECK_ARG(g->n_rows >= 0 && g->n_edges >= 0, "%s: negative n_rows / n_edges", fn);
  MP_CHECK_ARG(g->rowptr != nullptr, "%s: g->rowptr is NULL", fn);
  MP_CHECK_ARG(g->col != nullptr, "%s: g->col is NULL (the RGCN passes gather by column)", fn);
  MP_CHECK_ARG(g->eid != nullptr, "%s: g->eid is NULL (edge_type is read in original edge order)", fn);
  MP_CHECK_ARG(g->n_cols > 0, "%s: g->n_cols must be > 0", fn);
  const int64_t ids = g->n_ids > 0 ? g->n_ids : g->n_edges;
  MP_CHECK_ARG(n_type_edges >= ids, "%s: eid indexes %lld edges, edge_type holds n_type_edges = %lld", fn,
               (long long)ids, (long long)n_type_edges);
  MP_CHECK_ARG(edge_type != nullptr || g->n_edges == 0, "%s: edge_type is NULL", fn);
  MP_CHECK_ARG(ld_att >= B, "%s: ld_att = %lld < B = %d", fn, (long long)ld_att, B);
  MP_CHECK_ARG(att != nullptr, "%s: att is NULL", fn);
  MP_CHECK_EXTENT(fn, "att", att_bytes, ((size_t)(R - 1) * ld_att + B) * sizeof(float));
  return MP_OK;
}

// floats spanned by n nodes x B blocks x C entries under the two strides
static inline size_t rg_span(int64_t n, int32_t B, int32_t C, int64_t ld_node, int64_t ld_block) {
  return n <= 0 ? 0 : (size_t)(n - 1) * ld_node + (size_t)(B - 1) * ld_block + C;
}

}  // namespace mp

using namespace mp;

extern "C" int64_t mp_rgcn_ok(int32_t R, int32_t B, int32_t Cin, int32_t Cout) {
  const char* fn = "mp_rgcn_ok";
  return rg_shape(fn, R, B, Cin, "Cin") == MP_OK && rg_shape(fn, R, B, Cout, "Cout") == MP_OK ? 1 : 0;
}

extern "C" int64_t mp_rgcn_att_chunk(void) { return kRgcnAttChunk; }

static int rgcn_bins(const mp_csr* g, const int64_t* edge_type, const float* edge_norm, int64_t n_type_edges,
                     const float* att, int64_t ld_att, size_t att_bytes, int32_t R, int32_t B, const float* x,
                     int64_t ldx, int32_t C, float* out, int64_t ld_node, int64_t ld_block, size_t out_bytes,
                     void* stream) {
  const char* fn = "mp_rgcn_aggregate_bins_f32";
  if (int rc = rg_shape(fn, R, B, C, "C")) return rc;
  if (int rc = rg_csr(fn, g, edge_type, n_type_edges, att, ld_att, att_bytes, R, B)) return rc;
  const int64_t Q = (int64_t)B * C;
  MP_CHECK_ARG(ldx >= C, "%s: ldx = %lld < C = %d", fn, (long long)ldx, C);
  // the entries of out must not overlap: node-major (a row holds its B blocks) or block-major (a block holds every row)
  const bool node_major = ld_block >= C && ld_node >= (int64_t)(B - 1) * ld_block + C;
  const bool block_major = ld_node >= C && ld_block >= (g->n_rows > 0 ? g->n_rows - 1 : 0) * ld_node + C;
  MP_CHECK_ARG(node_major || block_major,
               "%s: ld_node = %lld, ld_block = %lld overlap (B = %d, C = %d, n_rows = %lld): need ld_block >= C and "
               "ld_node >= (B - 1) * ld_block + C, or ld_node >= C and ld_block >= (n_rows - 1) * ld_node + C",
               fn, (long long)ld_node, (long long)ld_block, B, C, (long long)g->n_rows);
  MP_CHECK_ARG(x != nullptr, "%s: x is NULL", fn);
  MP_CHECK_ARG(out != nullptr, "%s: out is NULL", fn);
  MP_CHECK_EXTENT(fn, "out", out_bytes, rg_span(g->n_rows, B, C, ld_node, ld_block) * sizeof(float));
  if (g->n_rows == 0) return MP_OK;
  const RgCoef k{edge_type, edge_norm, att, ld_att, R, B};
  if (C < kRgcnColumnsMinC) {
    const int glog = rg_group_log2(Q);
    const int64_t bx = ceil_div(g->n_rows, (int64_t)4 << (6 - glog));
    const int T = Q > 256 ? 8 : (Q > 128 ? 4 : (Q > 64 ? 2 : 1));  // entries per lane: the fewest waves per row
    const int64_t by = ceil_div(Q, 64 * T);
    MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535, "%s: grid too large (n_rows %lld, B * C %lld)", fn,
                 (long long)g->n_rows, (long long)Q);
    MP_DEVICE_GUARD(stream);
    auto kern = T == 8 ? k_rgcn_bins_flat<8> : (T == 4 ? k_rgcn_bins_flat<4> : (T == 2 ? k_rgcn_bins_flat<2> : k_rgcn_bins_flat<1>));
    hipLaunchKernelGGL(kern, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, as_stream(stream), g->rowptr, g->col,
                       g->eid, g->n_rows, k, x, ldx, C, glog, out, ld_node, ld_block);
  } else {
    const int64_t bx = ceil_div(g->n_rows, 4);
    const int64_t by = ceil_div(C, 64);
    const int64_t bz = ceil_div(B, kRgcnBTile);
    MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535 && bz <= 65535, "%s: grid too large (n_rows %lld, B %d, C %d)", fn,
                 (long long)g->n_rows, B, C);
    MP_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(k_rgcn_bins_cols, dim3((unsigned)bx, (unsigned)by, (unsigned)bz), dim3(256), 0,
                       as_stream(stream), g->rowptr, g->col, g->eid, g->n_rows, k, x, ldx, C, out, ld_node, ld_block);
  }
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int rgcn_gather(const mp_csr* g, const int64_t* edge_type, const float* edge_norm, int64_t n_type_edges,
                       const float* att, int64_t ld_att, size_t att_bytes, int32_t R, int32_t B, const float* y,
                       int64_t ld_node, int64_t ld_block, size_t y_bytes, int32_t F, const float* bias, float* out,
                       int64_t ldo, void* stream) {
  const char* fn = "mp_rgcn_aggregate_gather_f32";
  if (int rc = rg_shape(fn, R, B, F, "F")) return rc;
  if (int rc = rg_csr(fn, g, edge_type, n_type_edges, att, ld_att, att_bytes, R, B)) return rc;
  MP_CHECK_ARG(ld_node >= F, "%s: ld_node = %lld < F = %d", fn, (long long)ld_node, F);
  MP_CHECK_ARG(ld_block >= F, "%s: ld_block = %lld < F = %d", fn, (long long)ld_block, F);
  MP_CHECK_ARG(ldo >= F, "%s: ldo = %lld < F = %d", fn, (long long)ldo, F);
  MP_CHECK_ARG(y != nullptr, "%s: y is NULL", fn);
  MP_CHECK_ARG(out != nullptr, "%s: out is NULL", fn);
  MP_CHECK_EXTENT(fn, "y", y_bytes, rg_span(g->n_cols, B, F, ld_node, ld_block) * sizeof(float));
  if (g->n_rows == 0) return MP_OK;
  const RgCoef k{edge_type, edge_norm, att, ld_att, R, B};
  const int glog = rg_group_log2(F);
  const int64_t bx = ceil_div(g->n_rows, (int64_t)4 << (6 - glog));
  const int64_t by = ceil_div(F, 64);
  MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535, "%s: grid too large (n_rows %lld, F %d)", fn, (long long)g->n_rows, F);
  MP_DEVICE_GUARD(stream);
  hipLaunchKernelGGL(k_rgcn_gather, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, as_stream(stream), g->rowptr,
                     g->col, g->eid, g->n_rows, k, y, ld_node, ld_block, F, glog, bias, out, ldo);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int rgcn_att_grad(const int64_t* perm, const int64_t* relptr, const int64_t* rows, const int64_t* cols,
                         int64_t n_edges, const float* edge_norm, const float* P, int64_t ldp_node, int64_t ldp_block,
                         const float* Q, int64_t ldq, int32_t R, int32_t B, int32_t C, float* datt, int64_t ld_datt,
                         size_t datt_bytes, void* ws, size_t ws_bytes, void* stream, int64_t* launches) {
  const char* fn = "mp_rgcn_att_grad_f32";
  if (int rc = rg_shape(fn, R, B, C, "C")) return rc;
  MP_CHECK_ARG(n_edges >= 0, "%s: n_edges < 0", fn);
  MP_CHECK_ARG(n_edges <= 0x7fffffff, "%s: n_edges too large", fn);
  MP_CHECK_ARG(ldp_node >= C, "%s: ldp_node = %lld < C = %d", fn, (long long)ldp_node, C);
  MP_CHECK_ARG(ldp_block >= C, "%s: ldp_block = %lld < C = %d", fn, (long long)ldp_block, C);
  MP_CHECK_ARG(ldq >= C, "%s: ldq = %lld < C = %d", fn, (long long)ldq, C);
  MP_CHECK_ARG(ld_datt >= B, "%s: ld_datt = %lld < B = %d", fn, (long long)ld_datt, B);
  MP_CHECK_ARG(datt != nullptr, "%s: datt is NULL", fn);
  MP_CHECK_EXTENT(fn, "datt", datt_bytes, ((size_t)(R - 1) * ld_datt + B) * sizeof(float));
  MP_CHECK_ARG(relptr != nullptr, "%s: relptr is NULL", fn);
  MP_CHECK_ARG(ws != nullptr, "%s: ws is NULL", fn);
  RgcnAttWs w(ws, n_edges, R, B);
  MP_CHECK_EXTENT(fn, "ws", ws_bytes, w.total(0));
  if (n_edges > 0) {
    MP_CHECK_ARG(perm != nullptr, "%s: perm is NULL", fn);
    MP_CHECK_ARG(rows != nullptr, "%s: rows is NULL", fn);
    MP_CHECK_ARG(cols != nullptr, "%s: cols is NULL", fn);
    MP_CHECK_ARG(P != nullptr, "%s: P is NULL", fn);
    MP_CHECK_ARG(Q != nullptr, "%s: Q is NULL", fn);
  }
  const int64_t max_chunks = rg_max_chunks(n_edges, R);
  const int64_t by = ceil_div(B, 64);
  MP_CHECK_ARG(by <= 65535, "%s: grid too large (B %d)", fn, B);
  MP_DEVICE_GUARD(stream);
  hipLaunchKernelGGL(k_rgcn_chunkptr, dim3(1), dim3(64), 0, as_stream(stream), relptr, R, n_edges, w.chunkptr);
  MP_CHECK_LAUNCH();
  ++*launches;
  if (n_edges > 0) {
    const int glog = rg_group_log2(B);
    const bool vec4 = C % 4 == 0 && ldp_node % 4 == 0 && ldp_block % 4 == 0 && ldq % 4 == 0 &&
                      (uintptr_t)P % 16 == 0 && (uintptr_t)Q % 16 == 0;
    hipLaunchKernelGGL(vec4 ? k_rgcn_att_part<4> : k_rgcn_att_part<1>, dim3((unsigned)max_chunks, (unsigned)by),
                       dim3(256), 0, as_stream(stream), perm, relptr, w.chunkptr, rows, cols, n_edges, edge_norm, P,
                       ldp_node, ldp_block, Q, ldq, R, B, C, glog, w.part);
    MP_CHECK_LAUNCH();
    ++*launches;
  }
  hipLaunchKernelGGL(k_rgcn_att_sum, dim3((unsigned)ceil_div((int64_t)R * B, 256)), dim3(256), 0, as_stream(stream),
                     w.chunkptr, w.part, max_chunks, R, B, datt, ld_datt);
  MP_CHECK_LAUNCH();
  ++*launches;
  return MP_OK;
}

// The entry points return int64_t like the NNConv ones: the launches enqueued
// (0 for an empty problem), or -(MP_ERR_* code).
static inline int64_t rg_result(int rc, int64_t launches) { return rc != MP_OK ? -(int64_t)rc : launches; }

extern "C" int64_t mp_rgcn_aggregate_bins_f32(const mp_csr* g, const int64_t* edge_type, const float* edge_norm,
                                              int64_t n_type_edges, const float* att, int64_t ld_att, size_t att_bytes,
                                              int32_t R, int32_t B, const float* x, int64_t ldx, int32_t C, float* out,
                                              int64_t ld_node, int64_t ld_block, size_t out_bytes, void* stream) {
  return rg_result(rgcn_bins(g, edge_type, edge_norm, n_type_edges, att, ld_att, att_bytes, R, B, x, ldx, C, out,
                             ld_node, ld_block, out_bytes, stream),
                   g != nullptr && g->n_rows > 0 ? 1 : 0);
}

extern "C" int64_t mp_rgcn_aggregate_gather_f32(const mp_csr* g, const int64_t* edge_type, const float* edge_norm,
                                                int64_t n_type_edges, const float* att, int64_t ld_att,
                                                size_t att_bytes, int32_t R, int32_t B, const float* y, int64_t ld_node,
                                                int64_t ld_block, size_t y_bytes, int32_t F, const float* bias,
                                                float* out, int64_t ldo, void* stream) {
  return rg_result(rgcn_gather(g, edge_type, edge_norm, n_type_edges, att, ld_att, att_bytes, R, B, y, ld_node,
                               ld_block, y_bytes, F, bias, out, ldo, stream),
                   g != nullptr && g->n_rows > 0 ? 1 : 0);
}

extern "C" size_t mp_rgcn_att_grad_workspace(int64_t n_edges, int32_t R, int32_t B) {
  if (n_edges < 0 || R < 1 || B < 1) return RgcnAttWs{nullptr, 0, 1, 1}.total(0);
  return RgcnAttWs{nullptr, n_edges, R, B}.total(0);
}

extern "C" int64_t mp_rgcn_att_grad_f32(const int64_t* perm, const int64_t* relptr, const int64_t* rows,
                                        const int64_t* cols, int64_t n_edges, const float* edge_norm, const float* P,
                                        int64_t ldp_node, int64_t ldp_block, const float* Q, int64_t ldq, int32_t R,
                                        int32_t B, int32_t C, float* datt, int64_t ld_datt, size_t datt_bytes, void* ws,
                                        size_t ws_bytes, void* stream) {
  int64_t launches = 0;
  const int rc = rgcn_att_grad(perm, relptr, rows, cols, n_edges, edge_norm, P, ldp_node, ldp_block, Q, ldq, R, B, C,
                               datt, ld_datt, datt_bytes, ws, ws_bytes, stream, &launches);
  return rg_result(rc, launches);
}
