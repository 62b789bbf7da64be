// NNConv's aggregation (gfx950) for an edge network that ends in a Linear.
//
// Per edge e = (j -> i) the layer's message is m_e = x_j W_e with
// W_e = reshape(head.weight h_e + head.bias, [Cin, Cout]), h_e in R^H the input
// of the edge network's last Linear.  With ht_e = [h_e, 1] and
// L[(h, c), o] = head.weight[c * Cout + o, h] (row block h = H: head.bias) the
// per-edge step (E x H x Cin x Cout, and an [E, Cin * Cout] array) is reordered
// into ONE segmented pass plus one dense node-level GEMM:
//   bins form    Z[i, h*Cin + c] = scale[i] * sum_{e -> i} ht_e[h] * x[j, c]
//                then out = Z @ L                                   (aggregate first)
//   gather form  out[i, f] = scale[i] * sum_{e -> i} sum_h ht_e[h] * Y[j, h*F + f] (+ bias)
//                with Y = x @ L' laid out [n, H+1, Cout]            (transform first)
// and the backward needs, besides the same two over the transposed CSR,
//   edge grad    dh[e, h] = sum_c dZ[i_e, h*Cin + c] * x[j_e, c]     (h < H)
// h is [n_h_edges, ldh >= H] in ORIGINAL edge order, read through eid; the
// trailing 1 of ht is implicit (no concatenated copy exists).
//
// Both aggregate kernels walk rowptr / col / eid only (no wave schedule).  One
// owner per output entry visits its row's slots in slot order and adds left to
// right (the gather form: h = 0..H inside a slot): deterministic, no atomics,
// bitwise reproducible.  A row's (H+1) * Cin accumulators live in registers,
// tiled over the grid, so no shape is limited by LDS.  Lane mappings:
//   bins, Cin < 32   ("flat"): lanes run over the flattened q = h*Cin + c, a
//       row owned by g = min(64, pow2 >= (H+1)*Cin) lanes and 64/g rows per
//       wave, wider rows tiled by 64 over blockIdx.y -- a Cin = 1 row of 26
//       entries shares its wave with a second row instead of idling 63 lanes.
//       Each lane loads its own ht[eid][h] and x[col][c].
//   bins, Cin >= 32  ("columns"): one wave per (row, 64 columns c, 16 values
//       of h); lanes map to c, so a slot's ht values are wave-uniform (the row
//       is wave-uniform: scalar loads) and x[col][c] is one coalesced load
//       reused by the lane's 16 accumulators.
//   gather: lanes map to f (g = min(64, pow2 >= F) lanes per row, 64/g rows
//       per wave, F tiled by 64); ht is read per row group, h serial.
//   edge grad, Cin <= 32: g = pow2 >= Cin lanes per (e, h) pair, then a fixed
//       DPP tree over the group (64/g pairs per wave; Cin = 1: a lane per pair).
//   edge grad, Cin > 32: W = 32 or 64 lanes per (edge, W values of h), lanes
//       over c (x read once, dz coalesced), each lane summing c = lane, lane +
//       W, ... in order, then a transposing butterfly over the group; W is the
//       width that wastes the fewest lanes and values of h.
// Rows of any length are summed serially by their owner; hub rows are not split.
#include "mp_common.h"

namespace mp {

constexpr int64_t kNNConvMaxRow = 1 << 20;  // floats in one row of Z or Y (4 MiB)
constexpr int kNNConvColumnsMinCin = 32;    // bins: lanes over c from here on
constexpr int kNNConvHTile = 16;            // bins, columns mapping: accumulators per lane
constexpr int kNNConvEdgeGroupMaxCin = 32;  // edge grad: a lane group per (e, h) pair up to here, a wave per edge above

static inline int nn_group_log2(int64_t n) {
  int gl = 0;
  while ((1 << gl) < n && gl < 6) ++gl;
  return gl;
}

// ---------------------------------------------------------------------------
// bins form, lanes over the flattened (h, c)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nnconv_bins_flat(const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col,
                                                          const int32_t* __restrict__ eid, int64_t n_rows,
                                                          const float* __restrict__ h, int64_t ldh, int32_t H,
                                                          const float* __restrict__ x, int64_t ldx, int32_t Cin,
                                                          int32_t glog, const float* __restrict__ row_scale,
                                                          float* __restrict__ out, int64_t ldo) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> glog;
  const int fl = lane & ((1 << glog) - 1);
  const int64_t r = (((int64_t)blockIdx.x * 4 + wave) << (6 - glog)) + sub;
  const int q = blockIdx.y * 64 + fl;
  if (r >= n_rows || q >= (H + 1) * Cin) return;
  const int hh = q / Cin;
  const int c = q - hh * Cin;
  const bool one = hh == H;  // the implicit trailing 1 of ht
  const int b = rowptr[r], e = rowptr[r + 1];
  float acc = 0.f;
  int32_t nc = 0, ne = 0;
  if (b < e) {
    nc = col[b];
    ne = eid[b];
  }
  for (int k = b; k < e; ++k) {
    const int32_t cc = nc;
    const int64_t id = ne;
    if (k + 1 < e) {
      nc = col[k + 1];
      ne = eid[k + 1];
    }
    const float xv = x[(int64_t)cc * ldx + c];
    const float hv = one ? 1.f : h[id * ldh + hh];
    acc = __fadd_rn(acc, __fmul_rn(hv, xv));
  }
  if (row_scale) acc = __fmul_rn(acc, row_scale[r]);
  out[r * ldo + q] = acc;
}

// ---------------------------------------------------------------------------
// bins form, lanes over c; wave = (row, 64 columns, kNNConvHTile values of h)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nnconv_bins_cols(const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col,
                                                          const int32_t* __restrict__ eid, int64_t n_rows,
                                                          const float* __restrict__ h, int64_t ldh, int32_t H,
                                                          const float* __restrict__ x, int64_t ldx, int32_t Cin,
                                                          const float* __restrict__ row_scale,
                                                          float* __restrict__ out, int64_t ldo) {
  constexpr int T = kNNConvHTile;
  const int lane = lane_id();
  const int64_t r = (int64_t)blockIdx.x * 4 + uni((int)(threadIdx.x >> 6));
  const int c = blockIdx.y * 64 + lane;
  const int h0 = blockIdx.z * T;
  if (r >= n_rows || c >= Cin) return;
  const int b = rowptr[r], e = rowptr[r + 1];
  float acc[T];
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = 0.f;
  for (int k = b; k < e; ++k) {
    const int32_t cc = col[k];
    const float* hr = h + (int64_t)eid[k] * ldh;
    const float xv = x[(int64_t)cc * ldx + c];
    float hv[T];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int hh = h0 + t;
      hv[t] = hh < H ? hr[hh] : (hh == H ? 1.f : 0.f);
    }
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = __fadd_rn(acc[t], __fmul_rn(hv[t], xv));
  }
  const float sc = row_scale ? row_scale[r] : 1.f;
  float* o = out + r * ldo + c;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int hh = h0 + t;
    if (hh <= H) o[(int64_t)hh * Cin] = row_scale ? __fmul_rn(acc[t], sc) : acc[t];
  }
}

// ---------------------------------------------------------------------------
// gather form: y is [n_cols, H+1, F]
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nnconv_gather(const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col,
                                                       const int32_t* __restrict__ eid, int64_t n_rows,
                                                       const float* __restrict__ h, int64_t ldh, int32_t H,
                                                       const float* __restrict__ y, int64_t ldy, int32_t F,
                                                       int32_t glog, const float* __restrict__ row_scale,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       int64_t ldo) {
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int sub = lane >> glog;
  const int fl = lane & ((1 << glog) - 1);
  const int64_t r = (((int64_t)blockIdx.x * 4 + wave) << (6 - glog)) + sub;
  const int f = blockIdx.y * 64 + fl;
  if (r >= n_rows || f >= F) return;
  const int b = rowptr[r], e = rowptr[r + 1];
  float acc = 0.f;
  for (int k = b; k < e; ++k) {
    const float* yr = y + (int64_t)col[k] * ldy + f;
    const float* hr = h + (int64_t)eid[k] * ldh;
    int hh = 0;
    for (; hh + 8 <= H; hh += 8) {  // eight independent load pairs in flight, added in h order
      float hv[8], yv[8];
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        hv[t] = hr[hh + t];
        yv[t] = yr[(int64_t)(hh + t) * F];
      }
#pragma unroll
      for (int t = 0; t < 8; ++t) acc = __fadd_rn(acc, __fmul_rn(hv[t], yv[t]));
    }
    for (; hh < H; ++hh) acc = __fadd_rn(acc, __fmul_rn(hr[hh], yr[(int64_t)hh * F]));
    acc = __fadd_rn(acc, yr[(int64_t)H * F]);
  }
  if (row_scale) acc = __fmul_rn(acc, row_scale[r]);
  if (bias) acc = __fadd_rn(acc, bias[f]);
  out[r * ldo + f] = acc;
}

// ---------------------------------------------------------------------------
// edge grad, Cin <= 32: one group of 2^glog lanes per (e, h) pair; every lane
// stays active up to the group sum (its DPP steps read neighbouring lanes)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_nnconv_edge_grad(const int64_t* __restrict__ rows,
                                                          const int64_t* __restrict__ cols, int64_t n_pairs,
                                                          const float* __restrict__ dz, int64_t lddz,
                                                          const float* __restrict__ x, int64_t ldx, int32_t H,
                                                          int32_t Cin, int32_t glog, float* __restrict__ dh,
                                                          int64_t lddh) {
  const int g = 1 << glog;
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t p = tid >> glog;
  const int cl = (int)(tid & (g - 1));
  const bool live = p < n_pairs;
  float s = 0.f;
  int64_t e = 0;
  int hh = 0;
  if (live) {
    if (n_pairs <= 0x7fffffff) {  // the usual case: one 32-bit division
      const uint32_t q = (uint32_t)p / (uint32_t)H;
      e = q;
      hh = (int)((uint32_t)p - q * (uint32_t)H);
    } else {
      e = p / H;
      hh = (int)(p - e * H);
    }
    const float* dr = dz + rows[e] * lddz + (int64_t)hh * Cin;
    const float* xr = x + cols[e] * ldx;
    for (int c = cl; c < Cin; c += g) s = __fadd_rn(s, __fmul_rn(dr[c], xr[c]));
  }
  s = group_sum(s, g);
  if (live && cl == 0) dh[e * lddh + hh] = s;
}

// ---------------------------------------------------------------------------
// edge grad, Cin > 32: W = 32 or 64 lanes per (edge, W values of h), 64 / W
// edges per wave; the lanes of a group run over c (c = lane, lane + W, ... in
// order), so x[cols[e]] is read once and every dz load is one coalesced run.
// The W per-lane partial sums are then summed across the group by a
// transposing butterfly: at the step of lane bit d a lane keeps the half of its
// values whose h has that bit equal to its own and adds its partner's, W - 1
// exchanges for W sums, after which lane l holds h0 + l -- a fixed tree, and
// one coalesced store.  Every lane stays active up to the exchanges.
// ---------------------------------------------------------------------------
template <int W>
__global__ __launch_bounds__(256) void k_nnconv_edge_grad_wave(const int64_t* __restrict__ rows,
                                                               const int64_t* __restrict__ cols, int64_t n_edges,
                                                               const float* __restrict__ dz, int64_t lddz,
                                                               const float* __restrict__ x, int64_t ldx, int32_t H,
                                                               int32_t Cin, float* __restrict__ dh, int64_t lddh) {
  const int lane = lane_id();
  const int cl = lane & (W - 1);
  const int64_t e = ((int64_t)blockIdx.x * 4 + uni((int)(threadIdx.x >> 6))) * (64 / W) + lane / W;
  const bool live = e < n_edges;
  const int h0 = blockIdx.y * W;
  const int nh = H - h0 < W ? H - h0 : W;
  float p[W];
#pragma unroll
  for (int t = 0; t < W; ++t) p[t] = 0.f;
  if (live) {  // no cross-lane step inside
    const float* dr = dz + rows[e] * lddz + (int64_t)h0 * Cin;
    const float* xr = x + cols[e] * ldx;
    for (int c = cl; c < Cin; c += W) {
      const float xv = xr[c];
      const float* q = dr + c;
#pragma unroll
      for (int t = 0; t < W; ++t) {
        p[t] = __fadd_rn(p[t], __fmul_rn(*q, xv));
        q += t + 1 < nh ? Cin : 0;  // past the last h: stay on a valid address, that sum is never stored
      }
    }
  }
#pragma unroll
  for (int d = W / 2; d >= 1; d >>= 1) {
    const bool up = (cl & d) != 0;
#pragma unroll
    for (int i = 0; i < d; ++i) {
      const float send = up ? p[i] : p[i + d];
      const float keep = up ? p[i + d] : p[i];
      p[i] = __fadd_rn(keep, __shfl_xor(send, d));
    }
  }
  if (live && cl < nh) dh[e * lddh + h0 + cl] = p[0];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// The edge gradient's kernel by shape: 0 = a lane group per (e, h) pair (Cin <=
// kNNConvEdgeGroupMaxCin), else the lanes W = 32 or 64 per (edge, W values of h):
// the width that wastes the fewest lanes and values of h; ties to 64
static int nn_edge_grad_width(int32_t H, int32_t Cin) {
  if (Cin <= kNNConvEdgeGroupMaxCin) return 0;
  auto used = [&](int64_t W) { return (double)Cin / (ceil_div(Cin, W) * W) * H / (ceil_div(H, W) * W); };
  return used(32) > used(64) ? 32 : 64;
}

// One (H, C) pair of the fused path: a row of (H+1) * C floats.
static int nn_shape(const char* fn, int32_t H, int32_t C, const char* cname) {
  MP_CHECK_ARG(H >= 1, "%s: H = %d < 1", fn, H);
  MP_CHECK_ARG(C >= 1, "%s: %s = %d < 1", fn, cname, C);
  MP_CHECK_ARG(((int64_t)H + 1) * C <= kNNConvMaxRow, "%s: (H + 1) * %s = %lld above the limit (H + 1) * C <= %lld",
               fn, cname, (long long)(((int64_t)H + 1) * C), (long long)kNNConvMaxRow);
  return MP_OK;
}

static int nn_csr(const char* fn, const mp_csr* g, const float* h, int64_t n_h_edges, int64_t ldh, int32_t H) {
  MP_CHECK_ARG(g != nullptr, "%s: g is NULL", fn);
  MP_CHECK_ARG(g->n_rows >= 0 && g->n_edges >= 0, "%s: negative n_rows / n_edges", fn);
  MP_CHECK_ARG(g->rowptr != nullptr, "%s: g->rowptr is NULL", fn);
  MP_CHECK_ARG(g->col != nullptr, "%s: g->col is NULL (the NNConv passes gather by column)", fn);
  MP_CHECK_ARG(g->eid != nullptr, "%s: g->eid is NULL (h is read in original edge order)", fn);
  MP_CHECK_ARG(g->n_cols > 0, "%s: g->n_cols must be > 0", fn);
  const int64_t ids = g->n_ids > 0 ? g->n_ids : g->n_edges;
  MP_CHECK_ARG(n_h_edges >= ids, "%s: eid indexes %lld edges, h holds n_h_edges = %lld rows", fn, (long long)ids,
               (long long)n_h_edges);
  MP_CHECK_ARG(ldh >= H, "%s: ldh = %lld < H = %d", fn, (long long)ldh, H);
  MP_CHECK_ARG(h != nullptr || g->n_edges == 0, "%s: h is NULL", fn);
  return MP_OK;
}

}  // namespace mp

using namespace mp;

extern "C" int64_t mp_nnconv_ok(int32_t H, int32_t Cin, int32_t Cout) {
  const char* fn = "mp_nnconv_ok";
  return nn_shape(fn, H, Cin, "Cin") == MP_OK && nn_shape(fn, H, Cout, "Cout") == MP_OK ? 1 : 0;
}

extern "C" int64_t mp_nnconv_edge_grad_width(int32_t H, int32_t Cin) {
  if (nn_shape("mp_nnconv_edge_grad_width", H, Cin, "Cin") != MP_OK) return -(int64_t)MP_ERR_ARG;
  return nn_edge_grad_width(H, Cin);
}

static int nnconv_bins(const mp_csr* g, const float* h, int64_t n_h_edges, int64_t ldh, int32_t H, const float* x,
                       int64_t ldx, int32_t Cin, const float* row_scale, float* out, int64_t ldo, void* stream) {
  const char* fn = "mp_nnconv_aggregate_bins_f32";
  if (int rc = nn_shape(fn, H, Cin, "Cin")) return rc;
  if (int rc = nn_csr(fn, g, h, n_h_edges, ldh, H)) return rc;
  const int64_t Q = ((int64_t)H + 1) * Cin;
  MP_CHECK_ARG(ldx >= Cin, "%s: ldx = %lld < Cin = %d", fn, (long long)ldx, Cin);
  MP_CHECK_ARG(ldo >= Q, "%s: ldo = %lld < (H + 1) * Cin = %lld", fn, (long long)ldo, (long long)Q);
  MP_CHECK_ARG(x != nullptr, "%s: x is NULL", fn);
  MP_CHECK_ARG(out != nullptr, "%s: out is NULL", fn);
  if (g->n_rows == 0) return MP_OK;
  if (Cin < kNNConvColumnsMinCin) {
    const int glog = nn_group_log2(Q);
    const int64_t bx = ceil_div(g->n_rows, (int64_t)4 << (6 - glog));
    const int64_t by = ceil_div(Q, 64);
    MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535, "%s: grid too large (n_rows %lld, (H + 1) * Cin %lld)", fn,
                 (long long)g->n_rows, (long long)Q);
    MP_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(k_nnconv_bins_flat, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, as_stream(stream),
                       g->rowptr, g->col, g->eid, g->n_rows, h, ldh, H, x, ldx, Cin, glog, row_scale, out, ldo);
  } else {
    const int64_t bx = ceil_div(g->n_rows, 4);
    const int64_t by = ceil_div(Cin, 64);
    const int64_t bz = ceil_div((int64_t)H + 1, kNNConvHTile);
    MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535 && bz <= 65535, "%s: grid too large (n_rows %lld, H %d, Cin %d)", fn,
                 (long long)g->n_rows, H, Cin);
    MP_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(k_nnconv_bins_cols, dim3((unsigned)bx, (unsigned)by, (unsigned)bz), dim3(256), 0,
                       as_stream(stream), g->rowptr, g->col, g->eid, g->n_rows, h, ldh, H, x, ldx, Cin, row_scale, out,
                       ldo);
  }
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int nnconv_gather(const mp_csr* g, const float* h, int64_t n_h_edges, int64_t ldh, int32_t H, const float* y,
                         int64_t ldy, int32_t F, const float* row_scale, const float* bias, float* out, int64_t ldo,
                         void* stream) {
  const char* fn = "mp_nnconv_aggregate_gather_f32";
  if (int rc = nn_shape(fn, H, F, "F")) return rc;
  if (int rc = nn_csr(fn, g, h, n_h_edges, ldh, H)) return rc;
  const int64_t Q = ((int64_t)H + 1) * F;
  MP_CHECK_ARG(ldy >= Q, "%s: ldy = %lld < (H + 1) * F = %lld", fn, (long long)ldy, (long long)Q);
  MP_CHECK_ARG(ldo >= F, "%s: ldo = %lld < F = %d", fn, (long long)ldo, F);
  MP_CHECK_ARG(y != nullptr, "%s: y is NULL", fn);
  MP_CHECK_ARG(out != nullptr, "%s: out is NULL", fn);
  if (g->n_rows == 0) return MP_OK;
  const int glog = nn_group_log2(F);
  const int64_t bx = ceil_div(g->n_rows, (int64_t)4 << (6 - glog));
  const int64_t by = ceil_div(F, 64);
  MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535, "%s: grid too large (n_rows %lld, F %d)", fn, (long long)g->n_rows,
               F);
  MP_DEVICE_GUARD(stream);
  hipLaunchKernelGGL(k_nnconv_gather, dim3((unsigned)bx, (unsigned)by), dim3(256), 0, as_stream(stream), g->rowptr,
                     g->col, g->eid, g->n_rows, h, ldh, H, y, ldy, F, glog, row_scale, bias, out, ldo);
  MP_CHECK_LAUNCH();
  return MP_OK;
}

static int nnconv_edge_grad(const int64_t* rows, const int64_t* cols, int64_t n_edges, const float* dz, int64_t lddz,
                            const float* x, int64_t ldx, int32_t H, int32_t Cin, float* dh, int64_t lddh,
                            size_t dh_bytes, void* stream) {
  const char* fn = "mp_nnconv_edge_grad_f32";
  if (int rc = nn_shape(fn, H, Cin, "Cin")) return rc;
  MP_CHECK_ARG(n_edges >= 0, "%s: n_edges < 0", fn);
  MP_CHECK_ARG(lddz >= ((int64_t)H + 1) * Cin, "%s: lddz = %lld < (H + 1) * Cin = %lld", fn, (long long)lddz,
               (long long)(((int64_t)H + 1) * Cin));
  MP_CHECK_ARG(ldx >= Cin, "%s: ldx = %lld < Cin = %d", fn, (long long)ldx, Cin);
  MP_CHECK_ARG(lddh >= H, "%s: lddh = %lld < H = %d", fn, (long long)lddh, H);
  MP_CHECK_ARG(n_edges <= 0x7fffffff, "%s: n_edges too large", fn);
  MP_CHECK_EXTENT(fn, "dh", dh_bytes, n_edges == 0 ? 0 : ((size_t)(n_edges - 1) * lddh + H) * sizeof(float));
  if (n_edges == 0) return MP_OK;
  MP_CHECK_ARG(rows != nullptr, "%s: rows is NULL", fn);
  MP_CHECK_ARG(cols != nullptr, "%s: cols is NULL", fn);
  MP_CHECK_ARG(dz != nullptr, "%s: dz is NULL", fn);
  MP_CHECK_ARG(x != nullptr, "%s: x is NULL", fn);
  MP_CHECK_ARG(dh != nullptr, "%s: dh is NULL", fn);
  if (nn_edge_grad_width(H, Cin) == 0) {
    const int glog = nn_group_log2(Cin);
    const int64_t n_pairs = n_edges * H;
    const int64_t blocks = ceil_div(n_pairs << glog, 256);
    MP_CHECK_ARG(blocks <= 0x7fffffff, "%s: grid too large (n_edges %lld, H %d, Cin %d)", fn, (long long)n_edges, H,
                 Cin);
    MP_DEVICE_GUARD(stream);
    hipLaunchKernelGGL(k_nnconv_edge_grad, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), rows, cols,
                       n_pairs, dz, lddz, x, ldx, H, Cin, glog, dh, lddh);
  } else {
    const int W = nn_edge_grad_width(H, Cin);
    const int64_t bx = ceil_div(n_edges, 4 * (64 / W));
    const int64_t by = ceil_div(H, W);
    MP_CHECK_ARG(bx <= 0x7fffffff && by <= 65535, "%s: grid too large (n_edges %lld, H %d)", fn, (long long)n_edges,
                 H);
    MP_DEVICE_GUARD(stream);
    if (W == 32) {
      hipLaunchKernelGGL(k_nnconv_edge_grad_wave<32>, dim3((unsigned)bx, (unsigned)by), dim3(256), 0,
                         as_stream(stream), rows, cols, n_edges, dz, lddz, x, ldx, H, Cin, dh, lddh);
    } else {
      hipLaunchKernelGGL(k_nnconv_edge_grad_wave<64>, dim3((unsigned)bx, (unsigned)by), dim3(256), 0,
                         as_stream(stream), rows, cols, n_edges, dz, lddz, x, ldx, H, Cin, dh, lddh);
    }
  }
  MP_CHECK_LAUNCH();
  return MP_OK;
}

// The entry points return int64_t like the graclus and point-set ones: the
// launches enqueued (0 for an empty problem), or -(MP_ERR_* code).
static inline int64_t nn_result(int rc, bool launched) { return rc != MP_OK ? -(int64_t)rc : (launched ? 1 : 0); }

extern "C" int64_t mp_nnconv_aggregate_bins_f32(const mp_csr* g, const float* h, int64_t n_h_edges, int64_t ldh,
                                                int32_t H, const float* x, int64_t ldx, int32_t Cin,
                                                const float* row_scale, float* out, int64_t ldo, void* stream) {
  return nn_result(nnconv_bins(g, h, n_h_edges, ldh, H, x, ldx, Cin, row_scale, out, ldo, stream),
                   g != nullptr && g->n_rows > 0);
}

extern "C" int64_t mp_nnconv_aggregate_gather_f32(const mp_csr* g, const float* h, int64_t n_h_edges, int64_t ldh,
                                                  int32_t H, const float* y, int64_t ldy, int32_t F,
                                                  const float* row_scale, const float* bias, float* out,
                                                  int64_t ldo, void* stream) {
  return nn_result(nnconv_gather(g, h, n_h_edges, ldh, H, y, ldy, F, row_scale, bias, out, ldo, stream),
                   g != nullptr && g->n_rows > 0);
}

extern "C" int64_t mp_nnconv_edge_grad_f32(const int64_t* rows, const int64_t* cols, int64_t n_edges, const float* dz,
                                           int64_t lddz, const float* x, int64_t ldx, int32_t H, int32_t Cin,
                                           float* dh, int64_t lddh, size_t dh_bytes, void* stream) {
  return nn_result(nnconv_edge_grad(rows, cols, n_edges, dz, lddz, x, ldx, H, Cin, dh, lddh, dh_bytes, stream),
                   n_edges > 0);
}
